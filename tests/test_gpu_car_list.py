"""tfx_car_list on the device (include/tfx.h, csrc/tfx_cars.hpp) against its definition in NumPy (devrng.car_list) applied to
the engine's own ring planes - every plane byte for byte: nothing is computed - on synthetic states through the ring import,
on driven states on every forced step path (and against the CPU oracle's run of the same scenario), between tfx_move_cars and
the advance, plus: entries past min(N, cap) and planes that are not asked for keep their bytes, the selection (lists, arrays,
device tensors, repeats, ids outside the batch, road masks), more items than wavefronts, the call writes nothing, clones and
warm restarts, argument errors as codes, and TrafficVecEnv.cars / arterial and tools/timespace_demo.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_gpu_clone import ARCH, Inputs, assert_env_equal, drive, make, snapshot
from test_gpu_measures import DRIVEN, SEQUENCE, run_scenario, same_snapshot
from test_measures_host import E_DRIVEN, GRID, scenario, oracle_driven
from test_gpu_ends import capped_engine, load_random
from test_car_list_host import PLANES, SENTINEL

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from gym_traffic import _native as nat  # noqa: E402
from gym_traffic.core import CarList  # noqa: E402
from gym_traffic.devrng import car_list  # noqa: E402

assert CarList._fields == ("n", "offsets") + PLANES
DTYPES = dict(xv=torch.float32, road=torch.int32, row=torch.uint8, spawn=torch.float32)
GUARD = 16      # entries behind the caller's planes that no call may touch


def model_of(eng, ids=None, mask=None, cap=None, out=None):
    """the definition applied to the image tfx_export_ring produces right now"""
    x, v, w = eng.planes_numpy()
    arch = eng.arch.cpu().numpy() if eng.het else None
    ids, mask = [t.cpu().numpy() if torch.is_tensor(t) else t for t in (ids, mask)]
    return car_list(x, v, w if eng.P == 3 else None, arch, eng.leading.cpu().numpy(), eng.lastcar.cpu().numpy(), eng.C,
                    ids, mask, cap, out)


def host(cl):
    torch.cuda.synchronize()
    return [int(cl.n)] + [None if t is None else t.cpu().numpy().copy() for t in cl[1:]]


def assert_list(got, want, where):
    assert got[0] == want[0], (where, got[0], want[0])
    for name, g, w in zip(("offsets",) + PLANES, got[1:], want[1:]):
        assert (g is None) == (w is None), (name, where)
        if g is None:
            continue
        assert g.shape == w.shape and g.dtype == w.dtype, (name, where, g.shape, g.dtype, w.shape, w.dtype)
        if g.tobytes() != w.tobytes():
            bad = np.argwhere(g.reshape(len(g), -1).view(np.uint8) != w.reshape(len(w), -1).view(np.uint8))[:5, 0].tolist()
            raise AssertionError((name, where, bad))


def check(eng, where, ids=None, mask=None, max_cars=None):
    got = host(eng.car_list(ids, mask, max_cars))
    assert_list(got, model_of(eng, ids, mask, max_cars), where)
    return dict(zip(CarList._fields, got))


# ---- 1. synthetic states through the ring import -----------------------------------------------------------------------
# picked on the CPU (random_rings alone): the road counts hold 0, 1, 7, 8, 9 (the edge of the 8-visit block) and C - 2; at
# capacity 66 also 15, 16, 17 and 63, 64
SEEDS = {(3, 14): 0, (3, 66): 3, (4, 14): 0, (4, 66): 0}


@pytest.mark.parametrize("path,kind", [("pertick", "plain"), ("pertick", "validate"), ("pertick", "het"),
                                       ("ring", "plain"), ("ring", "validate")])
@pytest.mark.parametrize("capacity", [14, 66])
@pytest.mark.parametrize("m,n", [(3, 3), (4, 4)])        # 48 roads: one partial tile; 80: a full tile and 16 lanes of a second
def test_synthetic_states(path, kind, capacity, m, n):
    eng = make(path, 5, kind, m=m, n=n, capacity=capacity)
    assert eng.R == {3: 48, 4: 80}[m]
    count, ld, lc, arch = load_random(eng, SEEDS[m, capacity])
    counts = set(count.ravel().tolist())
    assert {0, 1, 7, 8, 9, capacity - 2} <= counts and (ld > lc).any()
    if capacity == 66:
        assert {15, 16, 17, 63, 64} <= counts
    d = check(eng, (path, kind, capacity, m))
    assert d["n"] == int(count.sum()) == len(d["xv"]) and np.array_equal(np.diff(d["offsets"]), count.ravel())
    assert np.array_equal(np.diff(d["offsets"]), eng.cars_on_roads_flat().cpu().numpy().ravel())
    assert np.array_equal(d["road"], np.repeat(np.arange(eng.E * eng.R), count.ravel()))
    assert (d["spawn"] is None) == (kind == "plain")
    if kind == "het":
        assert set(d["row"].tolist()) == set(range(len(ARCH)))                # every row of the table shows
    else:
        assert not d["row"].any()
    # the same list with room to spare, without the host synchronisation
    check(eng, "room to spare", max_cars=d["n"] + 7)


# ---- 2. driven states on every forced path -----------------------------------------------------------------------------
@pytest.mark.parametrize("path", DRIVEN)
def test_driven_states(path):
    eng = make(path, E_DRIVEN)
    assert dict(GRID) == dict(m=eng.m, n=eng.n, length=float(eng.cfg.length), capacity=eng.C, rate=float(eng.cfg.rate))
    run_scenario(eng)
    if path.startswith("pairs"):
        # the run ended on a two-tick pass: columns that start a row or two down are really read
        assert eng.pair_ticks() > 0 and eng.head_rows().any()
    s = oracle_driven()
    d = check(eng, path)
    # HIP equals the oracle bit for bit, so its list is the oracle's
    want = car_list(s["x"], s["v"], None, None, s["leading"], s["lastcar"], eng.C)
    assert_list([d[f] for f in CarList._fields], want, (path, "oracle"))
    assert np.array_equal(np.diff(d["offsets"]).reshape(eng.E, eng.R), s["cars"]) and d["n"] > 20
    ids = [4, 1, 4]
    d = check(eng, (path, "chosen"), ids=ids)
    assert_list([d[f] for f in CarList._fields], car_list(s["x"], s["v"], None, None, s["leading"], s["lastcar"], eng.C, ids),
                (path, "oracle, chosen"))


@pytest.mark.parametrize("path,kind", [("pertick", "validate"), ("ring", "validate"), ("pairs_tail", "het")])
def test_between_move_and_advance(path, kind):
    """tick by tick: the image tfx_export_ring gives between tfx_move_cars and tfx_advance_finished_cars is listed too"""
    eng = make(path, E_DRIVEN, kind)
    if kind == "het":
        eng.reset(np.zeros((eng.E, eng.I), np.int32))
        inp = Inputs(eng, 6)
        for c in [("step", 8)] * 4 + [("step", 6)]:
            drive(eng, inp, c)
        assert eng.head_rows().any()
        assert len(set(check(eng, (path, kind))["row"].tolist())) > 1          # mixed cars on the roads
        return
    run_scenario(eng)
    act, cnt = scenario(eng.I, eng.n_entry, seed=77)[0]
    for t in range(3):
        eng.set_actions(act)
        eng.set_spawns(counts=cnt[0])
        eng.move_cars()
        assert check(eng, ("after move_cars", t))["n"] > 20
        check(eng, ("after move_cars, chosen", t), ids=[5, 0, 2], mask=np.arange(eng.R) % 3 != 0)
        eng.advance_finished_cars()
        check(eng, ("after the advance", t))


# ---- 3. cap and sentinels ----------------------------------------------------------------------------------------------
def fresh(eng, cap, only=PLANES):
    """the caller's planes of `cap` entries, every byte 0xA5, as views of tensors with GUARD entries more -> (out, whole)"""
    whole, out = [], []
    for f in PLANES:
        if f not in only:
            whole.append(None)
            out.append(None)
            continue
        t = torch.empty((cap + GUARD,) + ((2,) if f == "xv" else ()), dtype=DTYPES[f], device=eng.device)
        t.view(torch.uint8).fill_(SENTINEL)
        whole.append(t)
        out.append(t[:cap])
    return out, whole


def sentinel_planes(cap, names):
    out = []
    for f in PLANES:
        a = None
        if f in names:
            a = np.empty((cap, 2) if f == "xv" else (cap,), dict(xv=np.float32, road=np.int32, row=np.uint8, spawn=np.float32)[f])
            a.view(np.uint8)[...] = SENTINEL
        out.append(a)
    return out


def check_out(eng, cap, names, where, ids=None, mask=None):
    out, whole = fresh(eng, cap, names)
    cl = eng.car_list(ids, mask, out=out)
    torch.cuda.synchronize()
    want = model_of(eng, ids, mask, cap, sentinel_planes(cap, PLANES if eng.P == 3 else PLANES[:3]))
    assert int(cl.n) == want[0] and cl.offsets.cpu().numpy().tobytes() == want[1].tobytes(), where
    for f, t, big, w in zip(PLANES, cl[2:], whole, want[2:]):
        assert (t is None) == (f not in names), (f, where)
        if t is None:
            continue
        g = big.cpu().numpy()
        assert g[:cap].tobytes() == w.tobytes(), (f, where, cap)               # the definition below min(N, cap), 0xA5 beyond
        assert (g[cap:].view(np.uint8) == SENTINEL).all(), (f, where, "guard")
    return want[0]


@pytest.mark.parametrize("path,kind", [("pairs_tail", "validate"), ("pertick", "het"), ("ring", "validate"), ("ring", "plain")])
def test_cap_and_sentinels(path, kind):
    eng = make(path, 5, kind, m=4, n=4)
    count = load_random(eng, 11)[0]
    names = PLANES if eng.P == 3 else PLANES[:3]
    N = int(count.sum())
    off = np.concatenate([[0], np.cumsum(count.ravel())])
    long_road = int(np.flatnonzero(count.ravel() >= 9)[3])
    cut = int(off[long_road]) + 3                                             # in the middle of a road's first 8-car block
    assert 0 < cut < N - 1
    for cap in (0, 1, cut, N - 1, N, N + 5):
        assert check_out(eng, cap, names, (path, kind, cap)) == N
    for cap in (cut, N + 5):
        for f in names:                                                       # each plane alone, the others NULL
            check_out(eng, cap, (f,), (path, kind, cap, f))
        check_out(eng, cap, ("road", "row"), (path, kind, cap, "two"))
    # a tensor that is not asked for keeps its sentinel
    out, whole = fresh(eng, N, names)
    eng.car_list(out=[out[0], None, None, None])
    torch.cuda.synchronize()
    assert all((t.cpu().numpy().view(np.uint8) == SENTINEL).all() for t in whole[1:] if t is not None)
    assert not (whole[0][:N].cpu().numpy().view(np.uint8) == SENTINEL).all()
    if eng.P != 3:
        with pytest.raises(ValueError):
            eng.car_list(out=[None, None, None, torch.zeros(4, device=eng.device)])
    with pytest.raises(ValueError):
        eng.car_list(out=[torch.zeros((4, 2), device=eng.device), torch.zeros(5, dtype=torch.int32, device=eng.device), None, None])
    with pytest.raises(ValueError):
        eng.car_list(max_cars=-1)


# ---- 4. selection ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path,kind", [("pertick", "het"), ("ring", "validate")])
def test_selection(path, kind):
    from gym_traffic.envs.roadgraph import GridRoad
    E = 6
    eng = make(path, E, kind, m=4, n=4)
    count = load_random(eng, 7, empty_envs=(1, 4))[0]
    assert not count[1].any() and not count[4].any() and count[0].any() and count[5].any()
    R = eng.R
    ids = [3, 0, 3, -1, 5, E, 1, 3]
    as_list = check(eng, "a list", ids=ids)
    as_array = check(eng, "an array", ids=np.array(ids, np.int64))
    as_tensor = check(eng, "a device tensor", ids=torch.as_tensor(ids, dtype=torch.int32).to(eng.device))
    for other in (as_array, as_tensor):
        assert all(as_list[f].tobytes() == other[f].tobytes() for f in CarList._fields[1:])
    cnt = np.diff(as_list["offsets"]).reshape(len(ids), R)
    assert np.array_equal(cnt[0], count[3]) and np.array_equal(cnt[2], cnt[0]) and np.array_equal(cnt[7], cnt[0])
    assert not cnt[3].any() and not cnt[5].any() and not cnt[6].any() and cnt[4].any()   # -1, E: empty runs; env 1: no cars
    off = as_list["offsets"]
    runs = [slice(off[s * R], off[(s + 1) * R]) for s in range(len(ids))]
    for f in ("xv", "row", "spawn"):                                          # repeats give identical runs
        assert as_list[f][runs[0]].tobytes() == as_list[f][runs[2]].tobytes() == as_list[f][runs[7]].tobytes(), f
    assert np.array_equal(as_list["road"][runs[2]], as_list["road"][runs[0]] + 2 * R)
    # road masks: one arterial (eastbound along row 1, by the GridRoad tables), nothing, a bool tensor
    g = GridRoad(eng.m, eng.n, float(eng.cfg.length))
    mask = np.zeros(R, np.uint8)
    road = 1 * eng.n
    while road >= 0:
        mask[road] = 1
        road = int(g.nexts[road])
    assert mask.sum() == eng.n + 1
    d = check(eng, "an arterial", mask=mask)
    assert 0 < d["n"] == int((count * mask).sum()) and mask[d["road"] % R].all()
    d = check(eng, "an arterial of chosen envs", ids=ids, mask=mask)
    assert 0 < d["n"] < as_list["n"]
    assert check(eng, "the all-zero mask", ids=ids, mask=np.zeros(R, np.uint8))["n"] == 0
    d2 = host(eng.car_list(ids, torch.as_tensor(mask != 0).to(eng.device)))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(d2[1:], [d[f] for f in CarList._fields[1:]]))
    assert check(eng, "ids outside the batch only", ids=[-1, E, 99])["n"] == 0
    with pytest.raises(ValueError):
        eng.car_list([])
    with pytest.raises(ValueError):
        eng.car_list(roads=np.ones(R + 1, np.uint8))


# ---- 5. more items than wavefronts -------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["transposed", "ring"])
def test_stride_rounds(layout):
    """7 envs of the 4x4 grid are 14 (env, tile) items (80 roads: a full tile and 16 lanes of a second).  The uncapped
    launch has a wavefront for every item (4 workgroups); TFX_GRID_CAP=1 leaves one workgroup - four wavefronts, four
    rounds, the last one with two at work.  Envs 2 and 5 hold no car.  Every block fills its LDS planes anew, so the bytes
    are those of the uncapped launch."""
    E = 7
    cfg = dict(m=4, n=4, length=120.0, capacity=14, rate=0.5, layout=layout)
    free = capped_engine(None, E, **cfg)
    one = capped_engine(1, E, **cfg)
    out = []
    for eng in (free, one):
        count = load_random(eng, 5, empty_envs=(2, 5))[0]
        assert not count[2].any() and not count[5].any() and count[0].any() and count[6].any()
        assert eng.car_list_launch(E) == ((4, 16) if eng is free else (1, 4))
        assert eng.car_list_launch(2) == (1, 4)
        out.append([check(eng, (layout, "all")), check(eng, (layout, "chosen"), ids=[6, 0, 3, 3, 1, 6, 4, 0, 2])])
    assert free.R == 80 and E * ((free.R + 63) // 64) == 14 > one.car_list_launch(E)[1]
    for a, b in zip(*out):
        assert a["n"] == b["n"] > 0 and all(a[f].tobytes() == b[f].tobytes() for f in CarList._fields[1:] if a[f] is not None)


# ---- 6. read-only ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path,kind", [("pairs_tail", "plain"), ("pertick", "validate"), ("pairs_tail", "het"), ("ring", "plain")])
def test_the_call_writes_nothing(path, kind):
    eng = make(path, E_DRIVEN, kind)
    if kind == "het":
        eng.reset(np.zeros((eng.E, eng.I), np.int32))
        inp = Inputs(eng, 6)
        for c in [("step", 8)] * 4 + [("step", 6)]:
            drive(eng, inp, c)
    else:
        run_scenario(eng)
    before = snapshot(eng)
    hb = eng.head_rows().copy()
    eng.car_list()
    eng.car_list([2, 2, 5], max_cars=40)
    same_snapshot(before, snapshot(eng))
    assert np.array_equal(hb, eng.head_rows())
    check(eng, (path, kind))


def test_the_launch_is_not_counted_by_fail_after():
    eng = make("pertick", 3)
    load_random(eng, 2)
    lib = nat.lib()
    nat.check(lib.tfx_debug_fail_after(eng.h, 1))                            # the NEXT counted launch fails
    for _ in range(3):
        check(eng, "under fail_after")                                     # (tfx_export_ring is not counted either)
    with pytest.raises(nat.TfxError, match="injected"):
        eng.clone_envs(np.array([-1, 0, -1], np.int32))
    nat.check(lib.tfx_debug_fail_after(eng.h, 0))
    check(eng, "after the injected failure")


@pytest.mark.parametrize("path", ["resident", "pairs_tail", "pairs_split", "pertick", "ring"])
def test_twin_that_never_asks(path):
    """An engine asked between every call of a mixed step / agent_step sequence stays bit-identical to one that never is."""
    E = E_DRIVEN
    eng, ref = make(path, E), make(path, E)
    rng = np.random.RandomState(31)
    for e_ in (eng, ref):
        e_.reset(np.zeros((E, eng.I), np.int32))
    cars = 0
    for kind, n in SEQUENCE:
        act = rng.randint(2, size=(E, eng.I)).astype(np.int32)
        cnt = ((rng.rand(n, E, eng.n_entry) < 0.15) * rng.randint(1, 3, size=(n, E, eng.n_entry))).astype(np.int32)
        eng.car_list(max_cars=64)
        eng.car_list([1, 4], max_cars=500)
        for e_ in (eng, ref):
            e_.set_actions(act)
            e_.set_spawns(counts=cnt, per_tick=True)
            (e_.agent_step if kind == "agent" else e_.step)(n)
        cars = check(eng, (path, kind, n))["n"]
        sa, sb = snapshot(eng), snapshot(ref)
        for k in range(E):
            assert_env_equal(sa, k, sb, k, (path, kind, n))
        assert np.array_equal(eng.head_rows(), ref.head_rows())
    assert cars > 0


# ---- 7. clones and warm restarts ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["pairs_tail", "ring"])
def test_after_clone_envs(path):
    eng = make(path, E_DRIVEN)
    run_scenario(eng)
    before = check(eng, "before the clone")
    src = np.array([-1, -1, -1, 1, 2, -1], np.int32)
    eng.clone_envs(src)
    assert eng.clone_skipped() == 0
    d = check(eng, "after the clone", ids=[1, 3, 2, 4])
    R, off = eng.R, d["offsets"]
    for a, b in ((0, 1), (2, 3)):                                             # the clone's run equals its source's
        ra, rb = slice(off[a * R], off[(a + 1) * R]), slice(off[b * R], off[(b + 1) * R])
        assert ra.stop > ra.start and d["xv"][ra].tobytes() == d["xv"][rb].tobytes()
        assert np.array_equal(d["road"][ra] + R, d["road"][rb])
    ob = before["offsets"]
    assert d["xv"][:off[R]].tobytes() == before["xv"][ob[R]:ob[2 * R]].tobytes()
    eng.set_actions(np.zeros((eng.E, eng.I), np.int32))
    eng.set_spawns(counts=np.zeros((4, eng.E, eng.n_entry), np.int32), per_tick=True)
    eng.step(4)
    d = check(eng, "clone, stepped", ids=[1, 3])
    half = d["n"] // 2
    assert half > 0 and d["xv"][:half].tobytes() == d["xv"][half:].tobytes()   # the clone goes on as its source does


def test_under_autoreset_with_a_warm_pool(monkeypatch):
    """episodes on, a warm pool attached (tests/test_gpu_warm_pool.py's "limit" scenario): ahead of every decision - after
    decisions that restarted envs from the pool among them - the device equals the definition"""
    import test_gpu_warm_pool as wp
    wp.force_path(monkeypatch, "pairs")
    seen = dict(calls=0, after_restart=0, index=None, pending=False)

    def hook(s, a, pool):
        idx = a.ep_index.cpu().numpy().copy()
        seen["after_restart"] += int(seen["pending"])                       # the last decision began with a restart
        seen["pending"] = seen["index"] is not None and bool((idx > seen["index"]).any())
        seen["index"] = idx
        seen["calls"] += int(check(a, ("decision", s))["n"] > 0)
        if s == 0:
            check(pool, "the pool")
    o = wp.run_warm(wp.SCENARIOS["limit"], hook=hook)
    assert (o["restart"] >= 2).any() and seen["after_restart"] >= 2 and seen["calls"] >= 10
    check(o["a"], "final", ids=[0, 0, 1])


# ---- 8. errors ---------------------------------------------------------------------------------------------------------
def test_errors_are_codes_and_the_handle_stays_usable():
    lib = nat.lib()
    eng = make("pertick", 3)                                                 # planes == 2: no spawn ticks
    run_scenario(eng, 6)
    cl = eng.car_list()
    N = int(cl.n)
    assert N > 0
    out, whole = fresh(eng, N, PLANES)
    b = nat.TfxCarListBuffers(*[C.c_void_p(t.data_ptr()) for t in out[:3]], None)
    with_spawn = nat.TfxCarListBuffers(*[C.c_void_p(t.data_ptr()) for t in out])
    off = C.c_void_p(cl.offsets.data_ptr())
    st = eng._stream()

    def untouched():
        torch.cuda.synchronize()
        return all((t.cpu().numpy().view(np.uint8) == SENTINEL).all() for t in whole)
    # before tfx_bind_buffers
    h = C.c_void_p()
    nat.check(lib.tfx_create(C.byref(eng.cfg), C.byref(h)))
    assert lib.tfx_car_list(h, None, eng.E, None, off, N, C.byref(b), 0, st) == -2
    assert b"tfx_bind_buffers" in lib.tfx_last_error()
    nat.check(lib.tfx_destroy(h))
    assert untouched()
    E = eng.E
    for args, msg in (((None, E, None, off, N, None, 0), b"out is null"), ((None, E, None, None, N, C.byref(b), 0), b"offsets is null"),
                      ((None, 0, None, off, N, C.byref(b), 0), b"n_sel 0"), ((None, -2, None, off, N, C.byref(b), 0), b"n_sel -2"),
                      ((None, E + 1, None, off, N, C.byref(b), 0), b"env_ids is null"),
                      ((None, E, None, off, -1, C.byref(b), 0), b"cap -1"), ((None, E, None, off, N, C.byref(b), 1), b"flags"),
                      ((None, E, None, off, N, C.byref(b), -1), b"flags"), ((None, E, None, off, N, C.byref(with_spawn), 0), b"spawn")):
        assert lib.tfx_car_list(eng.h, *args, st) == -1, msg
        assert msg in lib.tfx_last_error(), (msg, lib.tfx_last_error())
        assert untouched(), msg
    assert lib.tfx_car_list(None, None, E, None, off, N, C.byref(b), 0, st) == -1
    for bad in (0, -1):
        assert lib.tfx_car_list_launch(eng.h, bad, None, None) == -1
    assert lib.tfx_car_list(eng.h, None, E, None, off, 0, C.byref(b), 0, st) == 0                  # cap == 0: a valid no-op
    assert untouched()
    assert lib.tfx_car_list(eng.h, None, E, None, off, N, C.byref(b), 0, st) == 0
    torch.cuda.synchronize()
    want = model_of(eng)
    for t, w in zip(out[:3], want[2:5]):
        assert t.cpu().numpy().tobytes() == w.tobytes()
    assert (whole[3].cpu().numpy().view(np.uint8) == SENTINEL).all()
    # offsets that do not match the counts lose or overlap cars, and never send a store outside the planes
    wrong = cl.offsets.clone()
    wrong[1::2] += 3
    wrong[5] = -4
    wrong[-1] = 2 ** 31 - 1
    out2, whole2 = fresh(eng, N // 2, PLANES[:3])
    b2 = nat.TfxCarListBuffers(*[C.c_void_p(t.data_ptr()) for t in out2[:3]], None)
    assert lib.tfx_car_list(eng.h, None, E, None, C.c_void_p(wrong.data_ptr()), N // 2, C.byref(b2), 0, st) == 0
    torch.cuda.synchronize()
    assert all((t[N // 2:].cpu().numpy().view(np.uint8) == SENTINEL).all() for t in whole2[:3])
    eng.step(3)
    check(eng, "stepped after the errors")


# ---- 9. TrafficVecEnv.cars ---------------------------------------------------------------------------------------------
HET_ROWS = np.array([[11.11, 4.0, 3.0, 4.0, 13.89, 6.0, 2.0, 1.0], [9.0, 7.5, 2.0, 3.0, 11.0, 5.0, 1.5, 2.0]], np.float32)


@pytest.mark.parametrize("kind", ["het", "validate", "plain"])
def test_vec_env_cars(kind):
    from gym_traffic.envs.roadgraph import GridRoad
    from gym_traffic.envs.vec_env import TrafficVecEnv
    from gym_traffic.wrappers.vec import VecRemiRepeater
    E = 5
    kw = dict(archetypes=HET_ROWS, spawn='device', local_cars_per_sec=0.3) if kind == "het" else \
        dict(spawn='periodic', spawn_period=3, validate=(kind == "validate"))
    venv = TrafficVecEnv(E, 3, 3, 120.0, capacity=14, seed=3, **kw)
    wrapped = VecRemiRepeater(venv, 5)
    wrapped.reset()
    eng, g = venv.engine, venv.graph
    R, m, n, v = eng.R, eng.m, eng.n, eng.m * eng.n
    rng = np.random.RandomState(4)
    for d in range(9):
        wrapped.step(torch.as_tensor(rng.randint(2, size=(E, eng.I)).astype(np.int32)).to(eng.device))
    # arterial: the chain the GridRoad tables give
    for d, i, first in ((0, 1, 1 * n), (1, 2, v + 2 * n + n - 1), (2, 0, 2 * v), (3, 2, 3 * v + (m - 1) * n + 2)):
        mask = wrapped.arterial(i, d)                                         # through VecWrapper.__getattr__
        assert mask.dtype == np.uint8 and mask.shape == (R,) and mask.sum() == (n if d < 2 else m) + 1 and mask[first]
        chain = np.flatnonzero(mask)
        assert first in GridRoad(m, n, 120.0).generate_entrypoints(0)
        assert all(g.nexts[e] < 0 or mask[g.nexts[e]] for e in chain) and (g.nexts[chain] < 0).sum() == 1
        assert all((e // v == d) for e in chain if e < 4 * v)
        cell = chain[chain < 4 * v] % v
        assert ((cell // n == i) if d < 2 else (cell % n == i)).all()
    for bad in ((m, 0), (-1, 2), (0, 4)):
        with pytest.raises(ValueError):
            venv.arterial(*bad)
    mask = venv.arterial(1, 0)
    for envs, roads, max_cars in ((None, None, None), ([3, 0, 3], mask, None), ([4, 1], None, 300), (None, mask, 5)):
        c = venv.cars(envs, roads, max_cars)
        want = model_of(eng, envs, roads, max_cars)
        assert_list(host(CarList(*c[:6])), want, (kind, envs, max_cars))
        N, off, xv, road = want[0], want[1].astype(np.int64), want[2], want[3].astype(np.int64)
        L = len(xv)
        assert L == (N if max_cars is None else max_cars)                    # max_cars = None trims to N
        top = min(N, L)
        valid = np.arange(L) < N
        assert np.array_equal(c.valid.cpu().numpy(), valid) and (N > 0)
        assert np.array_equal(c.sel.cpu().numpy(), road // R) and np.array_equal(c.road_id.cpu().numpy(), road % R)
        rank = np.where(valid, np.arange(L) - off[:-1][road], 0)
        assert np.array_equal(c.rank.cpu().numpy(), rank) and (rank[:top] >= 0).all() and (rank[:top] < eng.C - 1).all()
        assert (rank[:top][np.diff(road[:top], prepend=-1) != 0] == 0).all()  # a road's first car is its head
        dist = (np.float32(eng.cfg.length) - xv[:, 0]).astype(np.float32)
        assert c.dist.cpu().numpy().tobytes() == dist.tobytes()
        if kind == "plain":
            assert c.spawn is None and c.age_ticks is None
            continue
        spawn = want[5]
        if kind == "het":
            age = ((int(eng.tick) - spawn.astype(np.int64)) & 0xFFFFFF).astype(np.int32)
        else:
            age = (np.float32(int(eng.tick)) - spawn).astype(np.float32).astype(np.int32)
        age = np.where(valid, age, 0).astype(np.int32)
        got = c.age_ticks.cpu().numpy()
        assert got.dtype == np.int32 and np.array_equal(got, age) and (age >= 0).all() and (age[:top] > 0).any()
    if kind != "plain":
        # the ages of the list add up to what tfx_car_ages reports per road
        c = venv.cars()
        ages = eng.car_ages()
        assert int(c.age_ticks.sum()) == int(ages.age_sum.sum()) and int(c.age_ticks.max()) == int(ages.age_max.max())
    if kind == "het":
        assert set(venv.cars().row.cpu().numpy().tolist()) == {0, 1}


# ---- 10. the demo ------------------------------------------------------------------------------------------------------
def test_timespace_demo_runs(tmp_path):
    png = tmp_path / "timespace.png"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "timespace_demo.py"), "--envs", "2", "--ticks", "20",
                          "--out", str(png)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    print(out.stdout)
    assert "ms per cars call" in out.stdout
    data = png.read_bytes()
    assert data[:8] == b"\x89PNG\r\n\x1a\n" and len(data) > 100
