"""tfx_put_cars on the device (include/tfx.h, csrc/tfx_put.hpp) against its definition in NumPy (devrng.put_cars) applied to
the image the engine exported before the call: the round trip car_list -> put_cars onto fresh and used handles, lists that
come from no export with partial selections, masks and more items than wavefronts, the continuation on every step path after
pack_envs / unpack_envs between used handles at different clocks (with the CPU oracle loaded through the definition), edits
of a list against the oracle, malformed offsets, a decision whose graph was captured before the call, argument errors as
codes, and the Python surface: set_cars, pack_envs / unpack_envs across E and capacity, tools/scenario_demo.py."""
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from conftest import ROOT
import test_transplant_host as H
from test_gpu_clone import ARCH, Inputs, assert_env_equal, drive, make, snapshot
from test_gpu_ends import capped_engine, load_random
from test_gpu_parity import same_bits
from test_gpu_transplant import MATRIX, DeviceSide, assert_oracle_agrees

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from gym_traffic import _native as nat  # noqa: E402
from gym_traffic import devrng  # noqa: E402
from oracle.oracle import live_mask  # noqa: E402

SEEDS = {(3, 14): 0, (3, 66): 3, (4, 14): 0, (4, 66): 0}                         # tests/test_gpu_car_list.py:SEEDS
SENTINEL = 0xA5
GUARD = 16


def image(eng):
    """the image tfx_export_ring gives right now: (x, v, w | None, arch | None, leading, lastcar) on the host"""
    torch.cuda.synchronize()
    x, v, w = eng.planes_numpy()
    return (x.copy(), v.copy(), w.copy() if eng.P == 3 else None, eng.arch.cpu().numpy().copy() if eng.het else None,
            eng.leading.cpu().numpy().copy(), eng.lastcar.cpu().numpy().copy())


def lead_of(x, ld):
    return np.take_along_axis(x, ld[..., None].astype(np.int64), axis=2)[..., 0]


def live_of(ld, lc, Cc):
    return np.stack([live_mask(ld[k], lc[k], Cc) for k in range(len(ld))])


def assert_image(got, want, Cc, where, lead_roads=None):
    """two images: ring words equal, every live slot of every plane byte for byte, the lead slot's x on lead_roads [E, R]"""
    assert np.array_equal(got[4], want[4]), ("leading", where, np.argwhere(got[4] != want[4])[:5].tolist())
    assert np.array_equal(got[5], want[5]), ("lastcar", where, np.argwhere(got[5] != want[5])[:5].tolist())
    m = live_of(want[4], want[5], Cc)
    for name, g, q in zip(("x", "v", "w", "arch"), got[:4], want[:4]):
        assert (g is None) == (q is None), (name, where)
        if g is not None:
            assert g[m].tobytes() == q[m].tobytes(), (name, where, np.argwhere((g != q) & m)[:5].tolist())
    if lead_roads is not None:
        a, b = lead_of(got[0], got[4])[lead_roads], lead_of(want[0], want[4])[lead_roads]
        assert a.tobytes() == b.tobytes(), ("lead x", where)


def host(t):
    return None if t is None else t.cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def model_put(before, eng, offsets, xv, row, spawn, ids=None, mask=None, leading=None, lead_x=None, shift=0):
    return devrng.put_cars(*before, eng.C, host(offsets), host(xv), host(row), host(spawn) if eng.P == 3 else None,
                           env_ids=host(ids), road_mask=host(mask), new_leading=host(leading), lead_x=host(lead_x),
                           spawn_shift=shift, het=eng.het)


def written_roads(eng, ids, mask, n_sel=None):
    w = np.zeros((eng.E, eng.R), bool)
    on = np.ones(eng.R, bool) if mask is None else np.asarray(host(mask)).reshape(-1) != 0
    for e in (range(eng.E if n_sel is None else n_sel) if ids is None else np.asarray(host(ids)).reshape(-1)):
        if 0 <= e < eng.E:
            w[e] = on
    return w


def use(eng, seed=6):
    """38 ticks of ordinary traffic ending on two-tick passes where the path runs them (tests/test_gpu_car_list.py)"""
    eng.reset(np.zeros((eng.E, eng.I), np.int32))
    inp = Inputs(eng, seed)
    for c in [("step", 8)] * 4 + [("step", 6)]:
        drive(eng, inp, c)


# ---- 1. the round trip ---------------------------------------------------------------------------------------------------
def round_trip(a, b, where):
    ia = image(a)
    lx = torch.as_tensor(lead_of(ia[0], ia[4]))
    cl = a.car_list()
    b.put_cars(cl, leading=a.leading, lead_x=lx, count_lost=True)
    assert b.put_lost() == 0
    assert_image(image(b), ia, a.C, where, np.ones((a.E, a.R), bool))
    back = b.car_list()
    for f, g, q in zip(cl._fields, back, cl):
        assert (g is None) == (q is None) and (g is None or torch.equal(g, q)), (f, where)
    assert torch.equal(b.cars_on_roads_flat(), a.cars_on_roads_flat())


@pytest.mark.parametrize("path,kind", [("pertick", "plain"), ("pertick", "validate"), ("pertick", "het"),
                                       ("ring", "plain"), ("ring", "validate")])
@pytest.mark.parametrize("capacity", [14, 66])
@pytest.mark.parametrize("m,n", [(3, 3), (4, 4)])        # 48 roads: one partial tile; 80: a full tile and 16 lanes of a second
def test_round_trip(path, kind, capacity, m, n):
    a = make(path, 5, kind, m=m, n=n, capacity=capacity)
    count = load_random(a, SEEDS[m, capacity])[0]
    counts = set(count.ravel().tolist())
    assert {0, 1, 7, 8, 9, capacity - 2} <= counts
    if capacity == 66:
        assert {15, 16, 17, 63, 64} <= counts
    b = make(path, 5, kind, m=m, n=n, capacity=capacity)
    b.reset(np.ones((b.E, b.I), np.int32))
    round_trip(a, b, (path, kind, capacity, m))


@pytest.mark.parametrize("kind", ["plain", "validate", "het"])
@pytest.mark.parametrize("m,capacity", [(3, 14), (4, 66)])
def test_round_trip_onto_a_used_handle(kind, m, capacity):
    a = make("pertick", 5, kind, m=m, n=m, capacity=capacity)
    load_random(a, SEEDS[m, capacity])
    b = make("pairs_tail", 5, kind, m=m, n=m, capacity=capacity)
    use(b)
    assert b.pair_ticks() > 0 and b.head_rows().any()      # columns that start a row or two down
    round_trip(a, b, ("used", kind, capacity, m))
    assert not b.head_rows().any()                         # every road was written: every column starts at row 0 again


# ---- 2. against the definition -------------------------------------------------------------------------------------------
def random_list(eng, n_sel, seed, over=False):
    """a list taken from no export: counts 0 .. C-2 (over: some runs longer than a ring holds), random cars"""
    rng = np.random.RandomState(seed)
    R, Cc = eng.R, eng.C
    count = rng.randint(0, Cc - 1, size=n_sel * R)
    count[rng.rand(n_sel * R) < 0.15] = 0
    count[rng.rand(n_sel * R) < 0.1] = Cc - 2
    if over:
        count[rng.rand(n_sel * R) < 0.1] = Cc + 3
    off = np.concatenate([[0], np.cumsum(count)]).astype(np.int32)
    N = int(off[-1])
    xv = np.stack([rng.uniform(-20, float(eng.cfg.length) * 1.4, N), rng.choice([0.0, 3.5, 11.0], N)], axis=1).astype(np.float32)
    row = rng.randint(len(ARCH), size=N).astype(np.uint8)
    spawn = rng.randint(0, 50, size=N).astype(np.float32)
    ld = rng.randint(0, Cc + 1, size=n_sel * R).astype(np.int32)              # 0 and C are no ring indices
    lx = rng.uniform(100, 400, n_sel * R).astype(np.float32)
    return off, xv, row, spawn, ld, lx


def put_and_check(eng, lst, where, ids=None, mask=None, shift=0):
    off, xv, row, spawn, ld, lx = lst
    before = image(eng)
    want = model_put(before, eng, off, xv, row, spawn, ids, mask, ld, lx, shift)
    eng.put_cars(off, xv, row=row, spawn=spawn, env_ids=ids, roads=mask, leading=ld.reshape(-1, eng.R), lead_x=lx,
                 spawn_shift=shift, count_lost=True)
    got = image(eng)
    wr = written_roads(eng, ids, mask, (len(off) - 1) // eng.R)
    assert_image(got, want[:6], eng.C, where, wr)
    assert eng.put_lost() == want[6], where
    # roads that were not written: the ring words and every live slot as before (the model leaves them as they were)
    assert np.array_equal(got[4][~wr], before[4][~wr]) and np.array_equal(got[5][~wr], before[5][~wr]), where
    # ... and the whole batch reads back as the definition says, columns that start a row down included
    cl = eng.car_list()
    ref = devrng.car_list(want[0], want[1], want[2], want[3], want[4], want[5], eng.C)
    assert int(cl.n) == ref[0] and cl.xv.cpu().numpy().tobytes() == ref[2].tobytes(), where
    assert cl.row.cpu().numpy().tobytes() == ref[4].tobytes(), where
    if eng.P == 3:
        assert cl.spawn.cpu().numpy().tobytes() == ref[5].tobytes(), where
    return want


@pytest.mark.parametrize("path,kind", [("pertick", "plain"), ("pertick", "validate"), ("pertick", "het"),
                                       ("ring", "plain"), ("ring", "validate")])
@pytest.mark.parametrize("capacity", [14, 66])
def test_against_the_definition(path, kind, capacity):
    eng = make(path, 5, kind, m=4, n=4, capacity=capacity)
    load_random(eng, 11)
    E, R = eng.E, eng.R
    mask = (np.arange(R) % 3 != 1).astype(np.uint8)
    put_and_check(eng, random_list(eng, 3, 1), (path, kind, "a permutation of three"), ids=[3, 0, 4])
    put_and_check(eng, random_list(eng, 4, 2), (path, kind, "ids outside the batch"), ids=[-1, 2, E + 3, 1], shift=-5)
    put_and_check(eng, random_list(eng, 2, 3), (path, kind, "a device tensor"),
                  ids=torch.tensor([4, 1], dtype=torch.int32, device=eng.device), mask=mask)
    put_and_check(eng, random_list(eng, 1, 4), (path, kind, "one env"), ids=[2], mask=mask, shift=9)
    put_and_check(eng, random_list(eng, E, 5), (path, kind, "every env, no ids"))
    put_and_check(eng, random_list(eng, 2, 6), (path, kind, "the first two, no ids"), mask=mask)


@pytest.mark.parametrize("kind", ["plain", "het"])
def test_untouched_envs_keep_their_row_offsets(kind):
    """a handle whose last call was a two-tick pass: the roads that are not written keep columns that start a row or two
    down, and the whole batch still reads back as the definition says"""
    eng = make("pairs_tail", 5, kind, m=4, n=4)
    use(eng)
    hb = eng.head_rows()
    assert hb.any()
    ids, mask = [3, 1], (np.arange(eng.R) % 2 == 0).astype(np.uint8)
    put_and_check(eng, random_list(eng, 2, 7), ("used", kind), ids=ids, mask=mask)
    wr = written_roads(eng, ids, mask)
    after = eng.head_rows()
    assert not after[wr].any() and np.array_equal(after[~wr], hb[~wr]) and hb[~wr].any()


@pytest.mark.parametrize("layout", ["transposed", "ring"])
def test_stride_rounds(layout):
    """7 envs of the 4x4 grid are 14 (env, tile) items; TFX_GRID_CAP=1 leaves one workgroup - four wavefronts, four rounds,
    the last one with two at work.  Every item fills its LDS planes anew: the image is that of the uncapped launch."""
    E = 7
    cfg = dict(m=4, n=4, length=120.0, capacity=14, rate=0.5, layout=layout, planes=3, validate=True)
    free, one = capped_engine(None, E, **cfg), capped_engine(1, E, **cfg)
    assert free.put_launch(E) == (4, 16) and one.put_launch(E) == (1, 4)
    imgs = []
    for eng in (free, one):
        load_random(eng, 5, empty_envs=(2, 5))
        put_and_check(eng, random_list(eng, E, 8), (layout, "stride"), ids=[6, 5, 4, 3, 2, 1, 0])
        imgs.append(image(eng))
    assert_image(imgs[1], imgs[0], free.C, (layout, "capped == free"), np.ones((E, free.R), bool))


# ---- 3. the continuation on every step path ------------------------------------------------------------------------------
SRC = {"g33": [0, 3, 7, 10], "g44": [4, 0]}            # envs of A ...
DST = {"g33": [5, 1, 2, 11], "g44": [1, 3]}            # ... that these envs of B receive
CONTS = H.CONTS                                          # step1, step2, step5, agent3r, agent4, halves


def remap(ops, src, dst, E):
    """the ops for A: env src[i] receives what env dst[i] of B receives"""
    out = []
    for op in ops:
        op = dict(op)
        for k, a in op.items():
            if isinstance(a, np.ndarray) and a.ndim >= 2:
                axis = 0 if k == "act" else 1          # act [E, I]; acts, cnt, rows [n, E, ...]
                b = a.copy()
                idx = [slice(None)] * a.ndim
                jdx = [slice(None)] * a.ndim
                idx[axis], jdx[axis] = src, dst
                b[tuple(idx)] = a[tuple(jdx)]
                op[k] = b
        out.append(op)
    return out


def host_packed(p):
    return {k: host(v) if torch.is_tensor(v) else v for k, v in p.items()}


def model_unpack(s, p, dst, w, dt):
    """the export `s` of B with the packed envs `p` (host arrays) written into envs `dst` through the definition"""
    s = dict(s)
    x, v, wt, arch, ld, lc, lost = devrng.put_cars(s["x"], s["v"], s["w"] if w.validate else None, s["arch"], s["leading"],
                                                   s["lastcar"], w.C, p["offsets"], p["xv"], p["row"], p["spawn"], env_ids=dst,
                                                   new_leading=p["leading"], spawn_shift=dt, het=w.het)
    assert lost == 0
    s.update(x=x, v=v, leading=ld, lastcar=lc, arch=arch)
    if w.validate:
        s["w"] = wt
    for f in ("obs", "rewards", "waiting", "passed_dst", "done") + (("n_trips", "trip_times") if w.validate else ()):
        a = s[f].copy()
        a[dst] = p[f]
        s[f] = a
    return s


@pytest.mark.parametrize("path,kind,geom", MATRIX)
def test_continuation(path, kind, geom):
    w = H.World(geom, kind)
    src, dst = SRC[geom], DST[geom]
    rest = [e for e in range(w.E) if e not in dst]
    failures, t0 = [], time.time()
    for cont in CONTS:
        where = (path, kind, geom, cont)
        try:
            a = DeviceSide(w, path, "P1").run(H.prefix_ops(geom, "P1"))
            b = DeviceSide(w, path, "P2").run(H.prefix_ops(geom, "P2"))
            twin = DeviceSide(w, path, "P2").run(H.prefix_ops(geom, "P2"))
            dt = b.eng.tick - a.eng.tick
            assert dt == 3
            if path.startswith("pairs"):
                assert a.eng.head_rows().any()
            sb = b.export()
            p = a.eng.pack_envs(src)
            b.eng.unpack_envs(dst, p)
            assert b.eng.put_lost() == 0
            orc = H.OracleSide(w).load(model_unpack(sb, host_packed(p), dst, w, dt))
            for side in (a, b, twin):
                side.outs = None
                side.eng.reset_counters()
            ops = H.cont_ops(geom, cont)
            a.run(remap(ops, src, dst, w.E))
            b.run(ops)
            twin.run(ops)
            sa, sB, st = snapshot(a.eng), snapshot(b.eng), snapshot(twin.eng)
            for i, j in zip(src, dst):
                assert_env_equal(sB, j, sa, i, where, w_shift=dt)
            for e in rest:
                assert_env_equal(sB, e, st, e, where)
            if b.outs is not None:
                for name, u, q, t in zip(("aobs", "areward", "adone"), b.outs, a.outs, twin.outs):
                    u, q, t = u.cpu().numpy(), q.cpu().numpy(), t.cpu().numpy()
                    assert same_bits(u[dst].astype(np.float32), q[src].astype(np.float32)), (name, where)
                    assert same_bits(u[rest].astype(np.float32), t[rest].astype(np.float32)), (name, where)
            updates0 = orc.orc.vehicle_updates
            orc.run(ops)
            assert_oracle_agrees(b, orc, cont, updates0, where)
        except AssertionError as exc:
            failures.append("%s: %s" % (cont, str(exc).splitlines()[0][:300] if str(exc) else repr(exc)))
    print("%s/%s/%s: %d continuations in %.1f s, %d failed" % (path, kind, geom, len(CONTS), time.time() - t0, len(failures)))
    assert not failures, "\n  ".join(failures)


# ---- 4. edits against the oracle -----------------------------------------------------------------------------------------
class VecSide(DeviceSide):
    """a DeviceSide whose handle is a TrafficVecEnv's"""

    def __init__(self, w):
        from gym_traffic.envs.vec_env import TrafficVecEnv
        self.w, self.path, self.device_inputs = w, "default", False
        self.venv = TrafficVecEnv(w.E, w.m, w.n, w.length, capacity=w.C, rate=w.rate, spawn="none", validate=w.validate,
                                  archetypes=ARCH if w.het else None)
        self.eng = self.venv.engine
        self.eng.reset(np.zeros((w.E, self.eng.I), np.int32))
        self.outs = None


def edit(cl, Cc, R, tick, seed):
    """a list on the host with the k-th car of some roads deleted and a stalled car inserted into others"""
    rng = np.random.RandomState(seed)
    off, xv, row, spawn = cl
    runs, n_del, n_ins = [], 0, 0
    for k in range(len(off) - 1):
        cars = [(xv[i].copy(), int(row[i]), float(spawn[i])) for i in range(off[k], off[k + 1])]
        what = rng.randint(4)
        if what == 0 and len(cars) >= 2:
            del cars[rng.randint(len(cars))]
            n_del += 1
        elif what == 1 and len(cars) <= Cc - 4:
            j = rng.randint(len(cars) + 1)
            ahead = cars[j - 1][0][0] if j > 0 else (cars[0][0][0] + 10.0 if cars else 60.0)
            behind = cars[j][0][0] if j < len(cars) else ahead - 10.0
            cars.insert(j, (np.array([(ahead + behind) / 2, 0.0], np.float32), int(rng.randint(len(ARCH))), float(tick - 2)))
            n_ins += 1
        runs.append(cars)
    assert n_del > 10 and n_ins > 10
    new_off = np.concatenate([[0], np.cumsum([len(c) for c in runs])]).astype(np.int32)
    flat = [c for cars in runs for c in cars]
    return (new_off, np.stack([c[0] for c in flat]).astype(np.float32), np.array([c[1] for c in flat], np.uint8),
            np.array([c[2] for c in flat], np.float32))


@pytest.mark.parametrize("kind", ["plain", "validate", "het"])
def test_edits_against_the_oracle(kind):
    from gym_traffic.core import CarList
    w = H.World("g44", kind)
    side = VecSide(w).run(H.prefix_ops("g44", "P1"))
    eng, venv = side.eng, side.venv
    s = side.export()
    ids = [3, 1, 4]
    cars = venv.cars(envs=ids)
    lst = edit([host(t) if t is not None else np.zeros(int(cars.n), np.float32) for t in (cars.offsets, cars.xv, cars.row, cars.spawn)],
               w.C, w.R, eng.tick, 3)
    off, xv, row, spawn = [torch.as_tensor(a).to(eng.device) for a in lst]
    venv.set_cars(CarList(off[-1], off, xv, None, row if w.het else torch.zeros_like(row), spawn if w.validate else None),
                  envs=ids)
    assert eng.put_lost() == 0
    x, v, wt, arch, ld, lc, lost = devrng.put_cars(s["x"], s["v"], s["w"] if w.validate else None, s["arch"], s["leading"],
                                                   s["lastcar"], w.C, lst[0], lst[1], lst[2], lst[3], env_ids=ids, het=w.het)
    assert lost == 0
    s.update(x=x, v=v, leading=ld, lastcar=lc, arch=arch)
    if w.validate:
        s["w"] = wt
    orc = H.OracleSide(w).load(s)
    eng.reset_counters()
    updates0 = orc.orc.vehicle_updates
    ops = [H._step(np.random.RandomState(9), w, 6)]
    side.run(ops)
    orc.run(ops)
    assert_oracle_agrees(side, orc, "step6", updates0, ("edits", kind))


# ---- 5. malformed offsets --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path,kind", [("pertick", "validate"), ("pairs_tail", "het"), ("ring", "validate"), ("ring", "plain")])
def test_malformed_offsets(path, kind):
    """offsets that decrease, go negative or point past cap, runs longer than a ring holds: data the bounds of the call
    deal with.  The planes lie between guard zones of sentinel bytes; the device equals the definition, which reads no
    entry outside [0, cap); then the oracle, started from the model image, goes on as the device does."""
    w = H.World("g44", kind)
    side = DeviceSide(w, path, "P1").run(H.prefix_ops("g44", "P1"))
    eng = side.eng
    rng = np.random.RandomState(12)
    ids = [2, 0, 9, 4]
    n_keys = len(ids) * eng.R
    off, xv, row, spawn, ld, lx = random_list(eng, len(ids), 13, over=True)
    lx.reshape(len(ids), eng.R)[:, eng.r:] = np.inf       # (exit roads: no light ever rewrites their leader, the model keeps +inf)
    cap = len(xv) - 40                                                        # the last runs reach past the planes
    off = off.copy()
    off[rng.randint(1, n_keys, 12)] -= rng.randint(1, 30, 12).astype(np.int32)    # decreasing here and there
    off[:3] = [-9, -2, 5]                                                         # negative
    off[-4:] = [cap + 50, cap + 70, cap - 3, 2 ** 31 - 1]                         # past cap
    planes = {}
    for name, a in (("xv", xv[:cap]), ("row", row[:cap]), ("spawn", spawn[:cap])):
        t = torch.empty((cap + 2 * GUARD,) + a.shape[1:], dtype=torch.as_tensor(a).dtype, device=eng.device)
        t.view(torch.uint8).fill_(SENTINEL)
        t[GUARD:GUARD + cap] = torch.as_tensor(a).to(eng.device)
        planes[name] = t
    before = image(eng)
    s = side.export()
    want = model_put(before, eng, off, xv[:cap], row[:cap], spawn[:cap], ids, None, ld, lx)
    eng.put_cars(off, planes["xv"][GUARD:GUARD + cap], row=planes["row"][GUARD:GUARD + cap],
                 spawn=planes["spawn"][GUARD:GUARD + cap], env_ids=ids, leading=ld, lead_x=lx, count_lost=True)
    got = image(eng)
    wr = written_roads(eng, ids, None)
    assert_image(got, want[:6], eng.C, (path, kind), wr)
    assert want[6] > 50 and eng.put_lost() == want[6]
    for t in planes.values():                                                  # the guards (and the planes) are as they were
        g = t.cpu().numpy()
        assert (g[:GUARD].view(np.uint8) == SENTINEL).all() and (g[GUARD + cap:].view(np.uint8) == SENTINEL).all()
    count = eng.cars_on_roads_flat().cpu().numpy()
    assert count.min() >= 0 and count.max() <= eng.C - 1 and (count[wr] == eng.C - 2).any()
    for e in (1, 3):                                                           # not selected
        assert np.array_equal(got[4][e], before[4][e]) and np.array_equal(got[5][e], before[5][e])
    # four ticks without arrivals: the device goes on as the oracle does from the model image, and no car appears
    s.update(x=want[0], v=want[1], leading=want[4], lastcar=want[5], arch=want[3])
    s["w"] = want[2] if want[2] is not None else s["w"]
    orc = H.OracleSide(w).load(s)
    op = H._step(np.random.RandomState(14), w, 4)
    op["cnt"][:] = 0
    eng.reset_counters()
    updates0 = orc.orc.vehicle_updates
    n0 = int(count.sum())
    side.run([op])
    orc.run([op])
    assert_oracle_agrees(side, orc, "step4", updates0, (path, kind, "after"))
    assert int(eng.cars_on_roads_flat().sum()) <= n0


# ---- 6. a decision whose graph was captured before the call --------------------------------------------------------------
@pytest.mark.parametrize("kind", ["plain", "validate"])
def test_captured_graph_replays_after_put_cars(kind):
    """pairs_tail keeps a captured graph per decision shape, pairs_nograph enqueues every launch: the same decision shape
    before and after the put, so the first handle replays what it captured before its cars were rewritten"""
    w = H.World("g33", kind)
    rng = np.random.RandomState(21)
    first = [H.prefix_ops("g33", "P1")[0], H._agent(rng, w, 4, True), H._agent(rng, w, 4, True)]
    after = [H._agent(rng, w, 4, True), H._agent(rng, w, 4, True)]
    sides = [DeviceSide(w, p, "P1").run(first) for p in ("pairs_tail", "pairs_nograph")]
    lst = random_list(sides[0].eng, 5, 22)
    ids = [7, 2, 11, 0, 5]
    for side in sides:
        off, xv, row, spawn, ld, lx = lst
        side.eng.put_cars(off, xv, row=row, spawn=spawn, env_ids=ids, leading=ld, lead_x=lx)
        side.run(after)
    sa, sb = snapshot(sides[0].eng), snapshot(sides[1].eng)
    for e in range(w.E):
        assert_env_equal(sa, e, sb, e, ("graph", kind))
    for u, q in zip(sides[0].outs, sides[1].outs):
        assert same_bits(u.cpu().numpy().astype(np.float32), q.cpu().numpy().astype(np.float32))
    assert sides[0].eng.pair_ticks() > 0 and int(sides[0].eng.cars_on_roads_flat().sum()) > 50


# ---- 7. argument errors and the Python surface -----------------------------------------------------------------------------
def test_argument_errors_are_codes():
    eng = make("pertick", 3, "validate")
    eng.reset(np.zeros((eng.E, eng.I), np.int32))
    lib, R = eng.lib, eng.R
    off = torch.zeros((3 * R + 1,), dtype=torch.int32, device=eng.device)
    xv = torch.zeros((4, 2), dtype=torch.float32, device=eng.device)
    b = nat.TfxPutBuffers(C.c_void_p(xv.data_ptr()), None, None, None, None)
    p = C.c_void_p(off.data_ptr())

    def call(h=eng.h, ids=None, n_sel=3, offsets=p, cap=4, buf=b, flags=0):
        return lib.tfx_put_cars(h, ids, n_sel, None, offsets, cap, C.byref(buf) if buf is not None else None, 0, None, flags,
                                eng._stream())
    before = image(eng)
    assert call(h=None) == -1
    assert call(buf=None) == -1
    assert call(buf=nat.TfxPutBuffers()) == -1
    assert call(offsets=None) == -1
    assert call(n_sel=0) == -1 and call(n_sel=-2) == -1
    assert call(n_sel=4) == -1                                          # more than E without ids
    assert call(n_sel=(2 ** 31) // R + 1, ids=p) == -1
    assert call(cap=-1) == -1
    assert call(flags=1) == -1
    after = image(eng)
    assert np.array_equal(after[4], before[4]) and np.array_equal(after[5], before[5])
    # cap == 0 is a call: the selected roads are emptied
    load_random(eng, 1)
    assert int(eng.cars_on_roads_flat().sum()) > 0
    ids = torch.tensor([2, 0], dtype=torch.int32, device=eng.device)
    ld0 = eng.leading.cpu().numpy().copy()
    kept = eng.cars_on_roads_flat()[1].clone()
    assert lib.tfx_put_cars(eng.h, C.c_void_p(ids.data_ptr()), 2, None, p, 0, C.byref(b), 0, None, 0, eng._stream()) == 0
    cnt = eng.cars_on_roads_flat().cpu().numpy()
    assert not cnt[[0, 2]].any() and np.array_equal(cnt[1], kept.cpu().numpy()) and cnt[1].any()
    assert np.array_equal(eng.leading.cpu().numpy(), ld0) and np.array_equal(eng.lastcar.cpu().numpy()[[0, 2]], ld0[[0, 2]])
    with pytest.raises(ValueError):
        eng.put_cars(off, xv, env_ids=[1, 0, 1])
    with pytest.raises(ValueError):
        eng.put_cars(off[:-1], xv)


def test_before_bind_is_a_state_error():
    src = make("pertick", 1)
    lib = src.lib
    h = C.c_void_p()
    nat.check(lib.tfx_create(C.byref(src.cfg), C.byref(h)))
    try:
        word = torch.zeros((src.R + 1,), dtype=torch.int32, device=src.device)
        xv = torch.zeros((1, 2), dtype=torch.float32, device=src.device)
        b = nat.TfxPutBuffers(C.c_void_p(xv.data_ptr()), None, None, None, None)
        assert lib.tfx_put_cars(h, None, 1, None, C.c_void_p(word.data_ptr()), 1, C.byref(b), 0, None, 0, None) == -2
        assert b"tfx_bind_buffers" in lib.tfx_last_error()
    finally:
        lib.tfx_destroy(h)


def vec(E, capacity, **kw):
    from gym_traffic.envs.vec_env import TrafficVecEnv
    return TrafficVecEnv(E, 3, 3, 80.0, capacity=capacity, spawn="device", validate=True, seed=5, **kw)


def test_unpack_into_another_batch():
    """envs of a 6-env batch of capacity 14 go into a 4-env batch of capacity 66 that stands at another clock: the cars,
    their ages and the trip figures arrive, and both go on alike under the same lights and without arrivals"""
    a, b = vec(6, 14), vec(4, 66, env_id_offset=100)
    a.reset(np.zeros((6, a.engine.I), np.int32))
    b.reset(np.ones((4, b.engine.I), np.int32))
    for _ in range(16):
        a.agent_step(n_ticks=10, cycle_period=8)
    for _ in range(2):
        b.agent_step(n_ticks=7, cycle_period=5)
    ea, eb = a.engine, b.engine
    dt = eb.tick - ea.tick
    assert ea.tick == 160 and eb.tick == 14 and int(ea.n_trips.sum()) > 0
    ta = a.travel_times()
    b.travel_times()
    src, dst = [5, 0, 2], [1, 3, 0]
    p = a.pack_envs(src)
    b.unpack_envs(dst, p)
    assert eb.put_lost() == 0
    assert torch.equal(eb.cars_on_roads_flat()[dst], ea.cars_on_roads_flat()[src]) and int(eb.cars_on_roads_flat()[dst].sum()) > 10
    ga, gb = ea.car_ages(), eb.car_ages()
    for f in ("n_cars", "age_sum", "age_max"):
        assert torch.equal(getattr(gb, f)[dst], getattr(ga, f)[src]), f
    la, lb = a.cars(envs=src), b.cars(envs=dst)
    assert torch.equal(la.xv, lb.xv) and torch.equal(la.age_ticks, lb.age_ticks) and torch.equal(la.spawn + dt, lb.spawn)
    assert torch.equal(eb.n_trips[dst], ea.n_trips[src])
    n = int(ea.n_trips[src].max())
    assert torch.equal(eb.trip_times[dst, :n], ea.trip_times[src, :n])
    # both go on: no arrivals, the same held lights
    for env in (a, b):
        env.engine.set_spawns()
    act = torch.zeros((6, ea.I), dtype=torch.int32, device=ea.device)
    a.step(act, n_ticks=12)
    b.step(act[:4], n_ticks=12)
    assert torch.equal(eb.cars_on_roads_flat()[dst], ea.cars_on_roads_flat()[src])
    la, lb = a.cars(envs=src), b.cars(envs=dst)
    assert torch.equal(la.xv, lb.xv) and torch.equal(la.age_ticks, lb.age_ticks)
    assert torch.equal(eb.n_trips[dst], ea.n_trips[src])
    tb = b.travel_times()
    ta2 = a.travel_times()
    # b's running figures hold only the trips the written envs finished after they arrived
    assert torch.equal(tb.finished[dst], (ta2.finished - ta.finished)[src])
    assert torch.equal(tb.unfinished_s[dst], ta2.unfinished_s[src])
    # a capacity that does not hold a road's cars: the excess is counted
    small = vec(2, 6)
    small.reset(np.zeros((2, small.engine.I), np.int32))
    small.unpack_envs([1], a.pack_envs([5]))
    want = int((ea.cars_on_roads_flat()[5] - 4).clamp(min=0).sum())
    assert want > 0 and small.engine.put_lost() == want


def test_set_cars_and_repeats():
    v = vec(4, 14)
    v.reset(np.zeros((4, v.engine.I), np.int32))
    for _ in range(8):
        v.agent_step(n_ticks=10, cycle_period=8)
    art = v.arterial(1, 0)
    cars = v.cars(envs=[2, 0], roads=art)
    assert int(cars.n) > 3
    before = v.cars()
    with pytest.raises(ValueError):
        v.set_cars(cars, envs=[2, 2], roads=art)
    # the head car of every listed road stalls
    xv = cars.xv.clone()
    xv[cars.rank == 0, 1] = 0.0
    v.set_cars(cars._replace(xv=xv), envs=[2, 0], roads=art)
    after = v.cars()
    assert torch.equal(after.offsets, before.offsets) and torch.equal(after.xv[:, 0], before.xv[:, 0])
    changed = (after.xv[:, 1] != before.xv[:, 1])
    on = torch.as_tensor(art, device=changed.device).bool()[after.road_id] & ((after.sel == 2) | (after.sel == 0)) & (after.rank == 0)
    assert torch.equal(changed, on & (before.xv[:, 1] != 0)) and int(changed.sum()) > 0
    assert v.engine.put_lost() == 0


def test_scenario_demo_runs():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "scenario_demo.py"), "--envs", "6", "--restart-envs", "4",
                          "--decisions", "6", "--every", "2"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "library" in out.stdout and "stalled" in out.stdout
