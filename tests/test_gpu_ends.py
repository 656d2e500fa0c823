"""tfx_road_ends on the device (include/tfx.h, csrc/tfx_ends.hpp) against its definition in NumPy (devrng.road_ends) applied
to the engine's own ring planes - bit for bit: the integer and byte fields with np.array_equal, heads and tail with same_bits
(pads, NaN included, by their bits too) - on synthetic states through the ring import, on driven states on every forced step
path (and against the CPU oracle's run of the same scenario, tests/test_ends_host.py), between tfx_move_cars and the advance,
plus: the call writes nothing, skips NULL members, strides over more items than it has wavefronts, survives clones and warm
restarts, reports argument errors as codes, and feeds TrafficVecEnv.stop_lines and tools/actuated_demo.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_gpu_parity import same_bits
from test_gpu_clone import ARCH, Inputs, assert_env_equal, drive, make, snapshot
from test_gpu_measures import DRIVEN, SEQUENCE, run_scenario, same_snapshot
from test_measures_host import E_DRIVEN, GRID, scenario, oracle_driven, random_rings
from test_ends_host import FLOATS, NAMES, NO_CAR, PADS

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from gym_traffic import _native as nat  # noqa: E402
from gym_traffic.core import RoadEnds  # noqa: E402
from gym_traffic.devrng import road_ends  # noqa: E402

assert RoadEnds._fields == NAMES
INF = float("inf")
DEFAULT = (INF, 0.0, INF)
KS = (1, 3, 4, 8, 16)


def model_of(eng, k, pads=DEFAULT, arch=None):
    """the definition applied to the image tfx_export_ring produces right now"""
    x, v, _ = eng.planes_numpy()
    if arch is None and eng.het:
        arch = eng.arch.cpu().numpy()
    return road_ends(x, v, eng.leading.cpu().numpy(), eng.lastcar.cpu().numpy(), eng.C, float(eng.cfg.length), k, *pads,
                     arch=arch)


def call(eng, k, pads=DEFAULT, **kw):
    return eng.road_ends(k, *pads, **kw)


def host(re_):
    torch.cuda.synchronize()
    return [None if t is None else t.cpu().numpy().copy() for t in re_]


def assert_ends(got, want, where):
    for name, g, w in zip(NAMES, got, want):
        if g is None:
            continue
        assert g.shape == w.shape and g.dtype == w.dtype, (name, where, g.shape, g.dtype)
        if name in FLOATS:
            assert same_bits(g, w), (name, where, np.argwhere(g.view(np.uint32) != w.view(np.uint32))[:5].tolist())
        else:
            assert np.array_equal(g, w), (name, where, np.argwhere(g != w)[:5].tolist())


def check(eng, k, where, pads=DEFAULT, arch=None):
    got = host(call(eng, k, pads))
    assert_ends(got, model_of(eng, k, pads, arch), (where, k, pads))
    return dict(zip(NAMES, got))


def load_random(eng, seed, empty_envs=()):
    """tests/test_gpu_measures.py:load_random, which also returns the rows it loaded; empty_envs: envs without a car"""
    rng = np.random.RandomState(seed)
    E, R, Cc = eng.E, eng.R, eng.C
    x, v, ld, lc, n = random_rings(rng, E * R, Cc)
    w = rng.randint(0, 50, size=(E, R, Cc)).astype(np.float32)
    arch = rng.randint(len(ARCH), size=(E, R, Cc)).astype(np.uint8) if eng.het else None
    ld, lc, n = ld.reshape(E, R), lc.reshape(E, R).copy(), n.reshape(E, R).copy()
    for e in empty_envs:
        lc[e], n[e] = ld[e], 0
    eng.reset(np.zeros((E, eng.I), np.int32))
    eng.load_state(x.reshape(E, R, Cc), v.reshape(E, R, Cc), ld, lc, w=w, arch=arch)
    return n, ld, lc, arch


# ---- 1. synthetic states through the ring import -----------------------------------------------------------------------
# picked on the CPU (random_rings alone): the road counts hold 0, C - 2 and, for every k of KS, those of k - 1, k, k + 1
# that a ring of this capacity can hold (at most C - 2 cars: with capacity 14 a road never has 15 .. 17)
SEEDS = {(3, 14): 1, (3, 66): 3, (4, 14): 1, (4, 66): 1}


@pytest.mark.parametrize("path,kind", [("pertick", "plain"), ("pertick", "validate"), ("pertick", "het"),
                                       ("ring", "plain"), ("ring", "validate")])
@pytest.mark.parametrize("capacity", [14, 66])
@pytest.mark.parametrize("m,n", [(3, 3), (4, 4)])        # 48 roads: one partial tile; 80: a full tile and 16 lanes of a second
def test_synthetic_states(path, kind, capacity, m, n):
    eng = make(path, 5, kind, m=m, n=n, capacity=capacity)
    assert eng.R == {3: 48, 4: 80}[m]
    count, ld, lc, arch = load_random(eng, SEEDS[m, capacity])
    counts = set(count.ravel().tolist())
    nan = float(np.array([0x7FC12345], np.uint32).view(np.float32)[0])
    for k in KS:
        assert {0, capacity - 2} <= counts and {q for q in (k - 1, k, k + 1) if q <= capacity - 2} <= counts, k
        assert (ld > lc).any()
        for pads in (DEFAULT, PADS, (nan, -0.0, -INF)):
            d = check(eng, k, (path, kind, capacity, m), pads, arch)
            assert np.array_equal(d["n_cars"], count) and np.array_equal(d["n_heads"], np.minimum(count, k))
            assert np.array_equal(d["n_cars"], eng.cars_on_roads_flat().cpu().numpy())
            assert np.array_equal(d["head_rows"] == NO_CAR, np.arange(k) >= count[..., None])
            assert np.array_equal(d["tail_row"] == NO_CAR, count == 0)
        if kind == "het":
            assert len(set(d["head_rows"][d["head_rows"] != NO_CAR].tolist())) == len(ARCH)      # every row of the table shows
            assert len(set(d["tail_row"][count > 0].tolist())) == len(ARCH)
        else:
            assert not d["head_rows"][d["head_rows"] != NO_CAR].any() and not d["tail_row"][count > 0].any()
    d = check(eng, 4, "again")
    # random x is unsorted, and a wrapped ring's head cars sit on both sides of the wrap
    assert (d["heads"][..., 1:, 0] < d["heads"][..., :-1, 0]).any() and ((ld > lc) & (ld >= capacity - 3) & (count >= 4)).any()
    one = count == 1
    assert one.any() and same_bits(d["heads"][one][:, 0, 1], d["tail"][one][:, 1])      # one car: the head is the tail


# ---- 2. driven states on every forced path -----------------------------------------------------------------------------
@pytest.mark.parametrize("path", DRIVEN)
def test_driven_states(path):
    eng = make(path, E_DRIVEN)
    assert dict(GRID) == dict(m=eng.m, n=eng.n, length=float(eng.cfg.length), capacity=eng.C, rate=float(eng.cfg.rate))
    run_scenario(eng)
    if path.startswith("pairs"):
        # the run ended on a two-tick pass: columns that start a row or two down are really read
        assert eng.pair_ticks() > 0 and eng.head_rows().any()
    if path.endswith("resident"):
        assert eng.fused_ticks()[0] > 0
    s = oracle_driven()
    for k in KS:
        d = check(eng, k, path, PADS)
        # HIP equals the oracle bit for bit, so its values are the oracle's
        assert_ends([d[f] for f in NAMES], road_ends(s["x"], s["v"], s["leading"], s["lastcar"], eng.C, GRID["length"], k, *PADS),
                    (path, "oracle", k))
    d = check(eng, 4, path)
    assert np.array_equal(d["n_cars"], host(eng.road_measures(x_from=None))[0]) and np.array_equal(d["n_cars"], s["cars"])
    assert (d["n_cars"] > 4).any() and (d["n_cars"] == 0).any() and (d["n_heads"] == 4).any() and (d["n_heads"] < 4).any()
    assert not d["head_rows"][d["head_rows"] != NO_CAR].any()


@pytest.mark.parametrize("path", ["pertick", "ring"])
def test_between_move_and_advance(path):
    """tick by tick: the image tfx_export_ring gives between tfx_move_cars and tfx_advance_finished_cars is listed too.  On
    the ring layout a head car then stands past its road's end, at a negative distance, until the advance; the transposed
    layout's mover hands such a car to the outbox at once, so its image never holds one."""
    eng = make(path, E_DRIVEN)
    run_scenario(eng)
    act, cnt = scenario(eng.I, eng.n_entry, seed=77)[0]
    negative = 0
    for t in range(3):
        eng.set_actions(act)
        eng.set_spawns(counts=cnt[0])
        eng.move_cars()
        d = check(eng, 4, ("after move_cars", t))
        check(eng, 16, ("after move_cars, sixteen", t), PADS)
        assert d["n_heads"].any()
        negative += int((d["heads"][..., 0, 0] < 0).sum())
        eng.advance_finished_cars()
        d = check(eng, 4, ("after the advance", t))
        assert not (d["heads"][..., 0] < 0).any()
    assert (negative > 0) == (path == "ring")


# ---- 3. read-only ------------------------------------------------------------------------------------------------------------
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
    call(eng, 3)
    call(eng, 16, PADS)
    same_snapshot(before, snapshot(eng))
    assert np.array_equal(hb, eng.head_rows())
    d = check(eng, 8, (path, kind))
    if kind == "het":
        assert len(set(d["tail_row"][d["n_cars"] > 0].tolist())) > 1          # mixed cars on the roads


def test_the_launch_is_not_counted_by_fail_after():
    eng = make("pertick", 3)
    load_random(eng, 2)
    lib = nat.lib()
    nat.check(lib.tfx_debug_fail_after(eng.h, 1))                            # the NEXT counted launch fails
    for _ in range(3):
        check(eng, 4, "under fail_after")                                  # (tfx_export_ring is not counted either)
    with pytest.raises(nat.TfxError, match="injected"):
        eng.clone_envs(np.array([-1, 0, -1], np.int32))
    nat.check(lib.tfx_debug_fail_after(eng.h, 0))
    check(eng, 4, "after the injected failure")


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
        call(eng, 4)
        call(eng, 16, PADS)
        for e_ in (eng, ref):
            e_.set_actions(act)
            e_.set_spawns(counts=cnt, per_tick=True)
            (e_.agent_step if kind == "agent" else e_.step)(n)
        cars = int(check(eng, 4, (path, kind, n))["n_heads"].sum())
        sa, sb = snapshot(eng), snapshot(ref)
        for k in range(E):
            assert_env_equal(sa, k, sb, k, (path, kind, n))
        assert np.array_equal(eng.head_rows(), ref.head_rows())
    assert cars > 0


# ---- 4. NULL members, the caller's tensors -----------------------------------------------------------------------------------
def fresh(eng, k, fill, only=None):
    """a caller's RoadEnds with every byte of every member `fill` (0xA5: a sentinel no result shares in every byte)"""
    E, R = eng.E, eng.R
    shapes = dict(n_cars=(E, R), n_heads=(E, R), heads=(E, R, k, 2), head_rows=(E, R, k), tail=(E, R, 2), tail_row=(E, R))
    dtypes = dict(n_cars=torch.int32, n_heads=torch.int32, heads=torch.float32, head_rows=torch.uint8, tail=torch.float32,
                  tail_row=torch.uint8)
    out = []
    for f in NAMES:
        if only is not None and f not in only:
            out.append(None)
            continue
        t = torch.empty(shapes[f], dtype=dtypes[f], device=eng.device)
        t.view(torch.uint8).fill_(fill)
        out.append(t)
    return RoadEnds(*out)


@pytest.mark.parametrize("path,kind", [("pairs_tail", "plain"), ("pertick", "het"), ("ring", "validate")])
def test_null_members_and_out(path, kind):
    eng = make(path, 5, kind, m=4, n=4)
    load_random(eng, 11)
    for k in (3, 16):
        own = call(eng, k, PADS)
        assert call(eng, k, PADS) is own                                    # allocated once per k, reused
        want = model_of(eng, k, PADS)
        assert_ends(host(own), want, "own")
        mine = fresh(eng, k, 0xA5)
        assert call(eng, k, PADS, out=mine) is not own
        assert_ends(host(mine), want, "the caller's tensors")
        for f in NAMES:                                                     # each plane alone
            alone = fresh(eng, k, 0xA5, only=(f,))
            got = host(call(eng, k, PADS, out=alone))
            assert [g is None for g in got] == [x != f for x in NAMES]
            assert_ends(got, want, ("alone", f))
        # a tensor that is not asked for keeps its sentinel
        kept = fresh(eng, k, 0xA5)
        part = RoadEnds(*[t if f in ("n_heads", "tail") else None for f, t in zip(NAMES, kept)])
        call(eng, k, PADS, out=part)
        got = host(kept)
        assert_ends([g if f in ("n_heads", "tail") else None for f, g in zip(NAMES, got)], want, "two members")
        for f, g in zip(NAMES, got):
            if f not in ("n_heads", "tail"):
                assert (g.view(np.uint8) == 0xA5).all(), f
    assert call(eng, 3) is not call(eng, 16)
    bad = fresh(eng, 4, 0)
    with pytest.raises(ValueError):
        call(eng, 3, out=bad)                                               # heads of another k
    with pytest.raises(ValueError):
        call(eng, 0)
    with pytest.raises(ValueError):
        call(eng, 17)


# ---- 5. more items than wavefronts -------------------------------------------------------------------------------------------
def capped_engine(cap, E, **cfg):
    """tests/test_gpu_stride_rounds.py:make_engine on a grid of this test's choice: a handle created under TFX_RESIDENT=0
    and TFX_GRID_CAP=cap alone - every other TFX_* switch is taken out of the environment while the handle reads it"""
    from gym_traffic.core import TfxEngine
    env = {"TFX_RESIDENT": "0"}
    if cap is not None:
        env["TFX_GRID_CAP"] = str(cap)
    keep = {k: v for k, v in os.environ.items() if k.startswith("TFX_") and k != "TFX_LIB"}
    for k in keep:
        del os.environ[k]
    os.environ.update(env)
    try:
        eng = TfxEngine(n_envs=E, **cfg)
    finally:
        for k in env:
            os.environ.pop(k, None)
        os.environ.update(keep)
    return eng


@pytest.mark.parametrize("layout", ["transposed", "ring"])
def test_stride_rounds(layout):
    """7 envs of the 4x4 grid are 14 (env, tile) items (80 roads: a full tile and 16 lanes of a second).  The uncapped
    launch has a wavefront for every item (4 workgroups); TFX_GRID_CAP=1 leaves one workgroup - four wavefronts, four
    rounds, the last one with two at work.  Envs 2 and 5 hold no car.  Every item fills its LDS planes anew, so the bits
    are those of the uncapped launch."""
    E = 7
    cfg = dict(m=4, n=4, length=120.0, capacity=14, rate=0.5, layout=layout)
    free = capped_engine(None, E, **cfg)
    one = capped_engine(1, E, **cfg)
    items = E * ((free.R + 63) // 64)
    out = []
    for eng in (free, one):
        count = load_random(eng, 5, empty_envs=(2, 5))[0]
        assert not count[2].any() and not count[5].any() and count[0].any() and count[6].any()
        res = []
        for k in (1, 4, 16):
            assert eng.ends_launch(k) == ((4, 16) if eng is free else (1, 4))
            res.append(check(eng, k, (layout, eng.ends_launch(k)), PADS))
        out.append(res)
    assert free.R == 80 and items == 14 > one.ends_launch(4)[1]
    for a, b in zip(*out):
        assert all(a[f].tobytes() == b[f].tobytes() for f in NAMES)
    assert (out[0][1]["n_heads"] == 4).any(axis=1)[[0, 1, 3, 4, 6]].all()


# ---- 6. clones and warm restarts ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["pairs_tail", "ring"])
def test_after_clone_envs(path):
    eng = make(path, E_DRIVEN)
    run_scenario(eng)
    before = check(eng, 4, "before the clone", PADS)
    src = np.array([-1, -1, -1, 1, 2, -1], np.int32)
    eng.clone_envs(src)
    assert eng.clone_skipped() == 0
    d = check(eng, 4, "after the clone", PADS)
    for f in NAMES:
        assert d[f][3].tobytes() == before[f][1].tobytes() and d[f][4].tobytes() == before[f][2].tobytes(), f
        assert d[f][5].tobytes() == before[f][5].tobytes() and d[f][:3].tobytes() == before[f][:3].tobytes(), f
    assert d["n_cars"][3].any() and not np.array_equal(before["n_cars"][3], before["n_cars"][1])
    eng.set_actions(np.zeros((eng.E, eng.I), np.int32))
    eng.set_spawns(counts=np.zeros((4, eng.E, eng.n_entry), np.int32), per_tick=True)
    eng.step(4)
    d = check(eng, 16, "clone, stepped")
    assert all(d[f][3].tobytes() == d[f][1].tobytes() for f in NAMES)          # the clone goes on as its source does


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
        d = check(a, 4, ("decision", s), PADS)
        seen["calls"] += int(d["n_heads"].any())
        if s == 0:
            check(pool, 4, "the pool")
    o = wp.run_warm(wp.SCENARIOS["limit"], hook=hook)
    assert (o["restart"] >= 2).any() and seen["after_restart"] >= 2 and seen["calls"] >= 10
    check(o["a"], 16, "final")


# ---- 7. errors -------------------------------------------------------------------------------------------------------------------
def test_errors_are_codes_and_the_handle_stays_usable():
    lib = nat.lib()
    eng = make("pertick", 3)
    run_scenario(eng, 6)
    k = 4
    mine = fresh(eng, k, 0xA5)
    b = nat.TfxEndsBuffers(*[C.c_void_p(t.data_ptr()) for t in mine])
    st = eng._stream()
    P = nat.TfxEndsParams
    ok = P(k, 1.0, 2.0, 3.0)

    def untouched():
        torch.cuda.synchronize()
        return all((t.cpu().numpy().view(np.uint8) == 0xA5).all() for t in mine)
    # before tfx_bind_buffers
    h = C.c_void_p()
    nat.check(lib.tfx_create(C.byref(eng.cfg), C.byref(h)))
    assert lib.tfx_road_ends(h, C.byref(ok), C.byref(b), 0, st) == -2
    assert b"tfx_bind_buffers" in lib.tfx_last_error()
    nat.check(lib.tfx_destroy(h))
    assert untouched()
    for args, msg in (((C.byref(P(0, 1.0, 2.0, 3.0)), C.byref(b), 0), b"k 0"), ((C.byref(P(17, 1.0, 2.0, 3.0)), C.byref(b), 0), b"k 17"),
                      ((C.byref(P(-1, 1.0, 2.0, 3.0)), C.byref(b), 0), b"k -1"),
                      ((C.byref(ok), C.byref(b), 1), b"flags"), ((C.byref(ok), C.byref(b), -1), b"flags"),
                      ((C.byref(ok), None, 0), b"out is null"), ((None, C.byref(b), 0), b"p is null")):
        assert lib.tfx_road_ends(eng.h, *args, st) == -1, msg
        assert msg in lib.tfx_last_error(), (msg, lib.tfx_last_error())
        assert untouched(), msg
    assert lib.tfx_road_ends(None, C.byref(ok), C.byref(b), 0, st) == -1
    for bad in (0, 17):
        assert lib.tfx_ends_launch(eng.h, bad, None, None) == -1
    assert untouched()
    nan = float("nan")
    assert lib.tfx_road_ends(eng.h, C.byref(P(k, nan, -INF, nan)), C.byref(b), 0, st) == 0        # any float32 is a pad
    assert_ends(host(mine), model_of(eng, k, (nan, -INF, nan)), "after the errors")
    eng.step(3)
    check(eng, k, "stepped after the errors")


# ---- 8. TrafficVecEnv.stop_lines ---------------------------------------------------------------------------------------------
HET_ROWS = np.array([[11.11, 4.0, 3.0, 4.0, 13.89, 6.0, 2.0, 1.0], [9.0, 7.5, 2.0, 3.0, 11.0, 5.0, 1.5, 2.0]], np.float32)


@pytest.mark.parametrize("het", [True, False])
def test_vec_env_stop_lines(het):
    from gym_traffic.envs.vec_env import TrafficVecEnv
    from gym_traffic.wrappers.vec import VecRemiRepeater
    E, K, v_min = 5, 3, 0.5
    # (periodic arrivals are all of row 0: mixed cars come from the on-device Poisson stream)
    kw = dict(archetypes=HET_ROWS, spawn='device', local_cars_per_sec=0.3) if het else dict(spawn='periodic', spawn_period=3)
    venv = TrafficVecEnv(E, 3, 3, 120.0, capacity=14, seed=3, **kw)
    wrapped = VecRemiRepeater(venv, 5)
    wrapped.reset()
    eng, g = venv.engine, venv.graph
    assert eng.het == het
    r, I, R, m, n = eng.r, eng.I, eng.R, eng.m, eng.n
    rng = np.random.RandomState(4)
    for d in range(9):
        wrapped.step(torch.as_tensor(rng.randint(2, size=(E, I)).astype(np.int32)).to(eng.device))
    s = wrapped.stop_lines(k=K, v_min=v_min)                                # through VecWrapper.__getattr__
    want = dict(zip(NAMES, model_of(eng, K)))
    assert_ends(host(s[:6]), [want[f] for f in NAMES], "per road")
    heads, tail, cars = want["heads"], want["tail"], want["n_cars"]
    # approach: the train road of direction d into intersection (row, col) is road d * m * n + row * n + col (GridRoad)
    approach = s.approach.cpu().numpy()
    assert approach.shape == (E, m, n, 4, K, 2) and approach.dtype == np.float32
    for d in range(4):
        for row in range(m):
            for col in range(n):
                e = d * m * n + row * n + col
                assert g.dest[e] == row * n + col
                assert approach[:, row, col, d].tobytes() == heads[:, e].tobytes(), (d, row, col)
    assert tuple(approach.shape[:4]) == tuple(venv.cars_on_roads().shape)
    assert np.array_equal(venv.cars_on_roads().cpu().numpy(), cars[:, :r].reshape(E, 4, m, n).transpose(0, 2, 3, 1))
    # eta_s: the same expression in NumPy, rtol 1e-6 (the device's float32 division need not be correctly rounded)
    listed = np.arange(K) < want["n_heads"][:, :r, None]
    eta = s.eta_s.cpu().numpy()
    assert eta.shape == (E, r, K) and eta.dtype == np.float32
    ref = heads[:, :r, :, 0] / np.maximum(heads[:, :r, :, 1], np.float32(v_min))
    assert np.isposinf(eta[~listed]).all() and np.isfinite(eta[listed]).all() and listed.any() and (~listed).any()
    assert np.allclose(eta[listed], ref[listed], rtol=1e-6, atol=0.0)
    assert (heads[:, :r, :, 1][listed] < v_min).any() and (heads[:, :r, :, 1][listed] > v_min).any()
    # entry_room, downstream_room, cross_gap: one subtraction, gathers, one addition - exact
    some = cars > 0
    if het:
        assert len(set(want["tail_row"][some].tolist())) == 2                 # two car lengths at the tails
        lengths = HET_ROWS[:, 1][np.where(some, want["tail_row"], 0)]
    else:
        lengths = np.full((E, R), np.float32(eng.cfg.car_l), np.float32)
    room = np.where(some, (tail[..., 0] - lengths).astype(np.float32), np.float32(INF)).astype(np.float32)
    assert same_bits(s.entry_room.cpu().numpy(), room)
    nxt = g.nexts[:r].astype(np.int64)
    assert (nxt >= 0).all() and (nxt >= r).any()
    down = room[:, nxt]
    assert same_bits(s.downstream_room.cpu().numpy(), down)
    both = some[:, :r] & some[:, nxt]
    gap = np.where(both, (heads[:, :r, 0, 0] + down).astype(np.float32), np.float32(INF)).astype(np.float32)
    assert same_bits(s.cross_gap.cpu().numpy(), gap)
    assert both.any() and (~both).any() and np.isposinf(gap[~both]).all() and np.isfinite(gap[both]).all()
    assert (~some).any() and np.isposinf(room[~some]).all() and np.isposinf(down[~some[:, nxt]]).all()
    with pytest.raises(ValueError):
        venv.stop_lines(k=K, v_min=0.0)


# ---- 9. the demo -----------------------------------------------------------------------------------------------------------------
def test_actuated_demo_runs():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "actuated_demo.py"), "--envs", "8", "--decisions", "6"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    print(out.stdout)
    rows = {ln.split("  ")[0].strip(): ln.split() for ln in out.stdout.splitlines()}
    for key in ("actuated (gap-out)", "fixed cycle", "greedy (on device)"):
        assert key in rows, out.stdout
        ret, overflowed = float(rows[key][-2]), float(rows[key][-1])
        assert np.isfinite(ret) and overflowed >= 0
    assert "ms per stop_lines call" in out.stdout
