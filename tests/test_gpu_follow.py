"""tfx_road_following on the device (include/tfx.h, csrc/tfx_follow.hpp) against its definition in NumPy
(devrng.road_following) applied to the engine's own ring planes - bit for bit: the six counters with np.array_equal, the five
float fields with same_bits (+inf and 0 by their bits too) - on synthetic states through the ring import, on driven states on
every forced step path (and against the CPU oracle's run of the same scenario, tests/test_follow_host.py), on heterogeneous
handles where a leader's length is not its follower's, plus: the call writes nothing, accumulates, strides over more items
than it has wavefronts, reports argument errors as codes, and feeds TrafficVecEnv.following and tools/following_demo.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_gpu_parity import same_bits
from test_gpu_fused import engine_with
from test_gpu_clone import ARCH, HET_PATHS, Inputs, assert_env_equal, drive, make, snapshot
from test_gpu_measures import DRIVEN, SEQUENCE, load_random, run_scenario, same_snapshot
from test_measures_host import E_DRIVEN, GRID, scenario, oracle_driven
from test_follow_host import FLOATS, FOLLOW, NAMES

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from gym_traffic import _native as nat  # noqa: E402
from gym_traffic.core import RoadFollowing  # noqa: E402
from gym_traffic.devrng import road_following, road_measures  # noqa: E402
from oracle.oracle import ring_order  # noqa: E402

assert RoadFollowing._fields == NAMES
INF = float("inf")
# (x_from, platoon_gap, v_min, ttc_crit): every car; nothing in range; the stop zone; a mid-road cut with wide thresholds; no
# critical TTC is too large; tight thresholds
PARAMS = [(None, 10.0, 0.5, 3.0), (INF, 10.0, 0.5, 3.0), (70.0, 10.0, 0.5, 3.0), (60.0, 40.0, 0.1, 30.0), (-INF, 10.0, 1.5, INF),
          (30.0, 0.0, 1e-3, 0.25)]


def model_of(eng, params):
    """the definition applied to the image tfx_export_ring produces right now"""
    x, v, _ = eng.planes_numpy()
    het = dict(arch_rows=eng.arch.cpu().numpy(), arch_l=eng.archetypes[:, 1]) if eng.het else {}
    return road_following(x, v, eng.leading.cpu().numpy(), eng.lastcar.cpu().numpy(), eng.C, params,
                          car_l=float(eng.cfg.car_l), **het)


def call(eng, params, **kw):
    x_from, platoon_gap, v_min, ttc_crit = params
    return eng.road_following(platoon_gap, v_min, ttc_crit, x_from=x_from, **kw)


def host(rf):
    torch.cuda.synchronize()
    return [None if t is None else t.cpu().numpy().copy() for t in rf]


def assert_following(got, want, where):
    for name, g, w in zip(NAMES, got, want):
        if g is None:
            continue
        if name in FLOATS:
            assert g.dtype == np.float32 and same_bits(g, w), (name, where, np.argwhere(g.view(np.uint32) != w.view(np.uint32))[:5].tolist())
        else:
            assert g.dtype == np.int32 and np.array_equal(g, w), (name, where, np.argwhere(g != w)[:5].tolist())


def check(eng, params, where):
    got = host(call(eng, params))
    assert_following(got, model_of(eng, params), (where, params))
    return dict(zip(NAMES, got))


# ---- 1. synthetic states through the ring import -----------------------------------------------------------------------
@pytest.mark.parametrize("path,kind", [("pertick", "plain"), ("pertick", "validate"), ("pertick", "het"),
                                       ("ring", "plain"), ("ring", "validate")])
@pytest.mark.parametrize("capacity", [14, 66])          # 66: road counts 0 .. 64 straddle every multiple of WALK_P = 8
@pytest.mark.parametrize("m,n", [(3, 3), (4, 4)])        # 48 roads: one partial tile; 80: a full tile and 16 lanes of a second
def test_synthetic_states(path, kind, capacity, m, n):
    eng = make(path, 5, kind, m=m, n=n, capacity=capacity)
    assert eng.R == {3: 48, 4: 80}[m]
    count = load_random(eng, 1000 * m + capacity)
    if capacity == 66:
        assert set(range(0, 65, 8)) <= set(count.ravel().tolist()) | set((count.ravel() + 1).tolist())
    for params in PARAMS:
        d = check(eng, params, (path, kind, capacity, m))
        if params[0] in (None, -INF):
            assert np.array_equal(d["n_cars"], count) and np.array_equal(d["n_pairs"], np.maximum(count - 1, 0))
        if params[0] == INF:
            assert not any(d[k].any() for k in NAMES if k not in ("gap_min", "ttc_min"))
            assert np.isposinf(d["gap_min"]).all() and np.isposinf(d["ttc_min"]).all()
        if params[3] == INF:
            assert np.array_equal(d["n_conflict"] > 0, np.isfinite(d["ttc_min"]))
    d = check(eng, PARAMS[3], "again")
    # random x is unsorted: overlaps, joins and gaps, closing pairs under and over the critical TTC, slow followers
    assert d["n_overlap"].any() and d["n_joined"].any() and (d["n_pairs"] > d["n_joined"]).any() and d["n_conflict"].any()
    assert (np.isfinite(d["ttc_min"]) & (d["n_conflict"] == 0)).any() and (d["n_hw"] < d["n_pairs"]).any() and d["n_hw"].any()
    assert (d["n_cars"] < count).any() and (d["drac_max"] > 0).any()
    if kind == "het":
        # pairs whose two cars carry different rows - and different lengths: with every car as long as car_l the gaps differ
        rows, ld, lc = eng.arch.cpu().numpy(), eng.leading.cpu().numpy(), eng.lastcar.cpu().numpy()
        mixed = 0
        for e in range(eng.R):
            s = ring_order(int(ld[0, e]), int(lc[0, e]), eng.C)
            mixed += sum(1 for a, b in zip(s[:-1], s[1:]) if ARCH[rows[0, e, a], 1] != ARCH[rows[0, e, b], 1])
        assert mixed > 10
        x, v, _ = eng.planes_numpy()
        plain = road_following(x, v, ld, lc, eng.C, PARAMS[3], car_l=float(eng.cfg.car_l))
        assert not same_bits(plain[4], d["gap_sum"]) and not np.array_equal(plain[2], d["n_joined"])


# ---- 2. driven states on every forced path -----------------------------------------------------------------------------
@pytest.mark.parametrize("path", DRIVEN)
def test_driven_states(path):
    eng = make(path, E_DRIVEN)
    assert dict(GRID) == dict(m=eng.m, n=eng.n, length=float(eng.cfg.length), capacity=eng.C, rate=float(eng.cfg.rate))
    run_scenario(eng)
    if path.startswith("pairs"):
        # the run ended on a two-tick pass: columns that start a row or two down are really walked
        assert eng.pair_ticks() > 0 and eng.head_rows().any()
    if path.endswith("resident"):
        assert eng.fused_ticks()[0] > 0
    s = oracle_driven()
    for params in (FOLLOW, (None,) + FOLLOW[1:], (30.0, 6.0, 1.0, 5.0)):
        d = check(eng, params, path)
        # HIP equals the oracle bit for bit, so its values are the oracle's
        assert_following([d[k] for k in NAMES], road_following(s["x"], s["v"], s["leading"], s["lastcar"], eng.C, params,
                                                               car_l=float(eng.cfg.car_l)), (path, "oracle", params))
    d = check(eng, FOLLOW, path)
    assert d["n_joined"].any() and (d["n_pairs"] > d["n_joined"]).any() and d["n_conflict"].any()
    assert np.isfinite(d["ttc_min"]).any() and np.isposinf(d["ttc_min"]).any() and (d["n_hw"] < d["n_pairs"]).any()
    assert np.array_equal(d["n_cars"], road_measures(s["x"], s["v"], s["leading"], s["lastcar"], eng.C, 0.1, FOLLOW[0])[0])


@pytest.mark.parametrize("path", HET_PATHS)
def test_het_driven(path):
    """mixed cars driven on the paths heterogeneous handles take: the leader's row, read from the side plane, sets the gap"""
    E = 4
    eng = make(path, E, "het")
    eng.reset(np.zeros((E, eng.I), np.int32))
    inp = Inputs(eng, 5)
    for c in [("step", 8)] * 5 + [("step", 1), ("step", 2), ("agent", 6), ("agent", 6), ("step", 7), ("step", 4)]:
        drive(eng, inp, c)
    if path.startswith("pairs"):
        assert eng.pair_ticks() > 0
    for params in (FOLLOW, (None, 10.0, 0.5, 3.0)):
        d = check(eng, params, (path, "het"))
    assert d["n_pairs"].any() and d["n_joined"].any() and np.isfinite(d["ttc_min"]).any()
    x, v, _ = eng.planes_numpy()
    plain = road_following(x, v, eng.leading.cpu().numpy(), eng.lastcar.cpu().numpy(), eng.C, (None, 10.0, 0.5, 3.0),
                           car_l=float(eng.cfg.car_l))
    assert not same_bits(plain[4], d["gap_sum"])                          # the lengths of the table are really used


def test_between_move_and_advance():
    """tick by tick: the image tfx_export_ring gives between tfx_move_cars and tfx_advance_finished_cars is measured too"""
    eng = make("pertick", E_DRIVEN)
    run_scenario(eng)
    act, cnt = scenario(eng.I, eng.n_entry, seed=77)[0]
    for t in range(3):
        eng.set_actions(act)
        eng.set_spawns(counts=cnt[0])
        eng.move_cars()
        d = check(eng, FOLLOW, ("after move_cars", t))
        check(eng, (None, 10.0, 0.5, 3.0), ("after move_cars, every car", t))
        assert d["n_pairs"].any()
        eng.advance_finished_cars()
        check(eng, FOLLOW, ("after the advance", t))


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
    call(eng, FOLLOW)
    call(eng, (None,) + FOLLOW[1:], accumulate=True)
    same_snapshot(before, snapshot(eng))
    assert np.array_equal(hb, eng.head_rows())


def test_the_launch_is_not_counted_by_fail_after():
    eng = make("pertick", 3)
    load_random(eng, 2)
    lib = nat.lib()
    nat.check(lib.tfx_debug_fail_after(eng.h, 1))                            # the NEXT counted launch fails
    for _ in range(3):
        check(eng, FOLLOW, "under fail_after")                             # (tfx_export_ring is not counted either)
    with pytest.raises(nat.TfxError, match="injected"):
        eng.clone_envs(np.array([-1, 0, -1], np.int32))
    nat.check(lib.tfx_debug_fail_after(eng.h, 0))
    check(eng, FOLLOW, "after the injected failure")


@pytest.mark.parametrize("path", ["resident", "pairs_tail", "pairs_split", "pertick", "ring"])
def test_twin_that_never_asks(path):
    """An engine asked between every call of a mixed step / agent_step sequence stays bit-identical to one that never is."""
    E = E_DRIVEN
    eng, ref = make(path, E), make(path, E)
    rng = np.random.RandomState(31)
    for e_ in (eng, ref):
        e_.reset(np.zeros((E, eng.I), np.int32))
    pairs = 0
    for kind, n in SEQUENCE:
        act = rng.randint(2, size=(E, eng.I)).astype(np.int32)
        cnt = ((rng.rand(n, E, eng.n_entry) < 0.15) * rng.randint(1, 3, size=(n, E, eng.n_entry))).astype(np.int32)
        call(eng, FOLLOW)
        call(eng, (None,) + FOLLOW[1:], accumulate=True)
        for e_ in (eng, ref):
            e_.set_actions(act)
            e_.set_spawns(counts=cnt, per_tick=True)
            (e_.agent_step if kind == "agent" else e_.step)(n)
        pairs = int(check(eng, FOLLOW, (path, kind, n))["n_pairs"].sum())
        sa, sb = snapshot(eng), snapshot(ref)
        for k in range(E):
            assert_env_equal(sa, k, sb, k, (path, kind, n))
        assert np.array_equal(eng.head_rows(), ref.head_rows())
    assert pairs > 0


# ---- 4. accumulate, NULL members, the caller's tensors ---------------------------------------------------------------------------
def fresh(eng, fill=None):
    """a caller's RoadFollowing: the counters, sums and the maximum 0, the minima +inf - or every member `fill`"""
    return RoadFollowing(*[torch.full((eng.E, eng.R), (INF if f in ("gap_min", "ttc_min") else 0) if fill is None else fill,
                                      dtype=torch.float32 if f in FLOATS else torch.int32, device=eng.device) for f in NAMES])


def combine(acc, want):
    """what TFX_FOLLOW_ACCUMULATE does to a buffer: int adds, ONE float32 add of a road's sum, min of minima, max of maxima"""
    out = []
    for name, a, w in zip(NAMES, acc, want):
        if a is None:                                                      # a member the caller left out stays out
            out.append(None)
        elif name in ("gap_min", "ttc_min"):
            out.append(np.where(w < a, w, a))
        elif name == "drac_max":
            out.append(np.where(w > a, w, a))
        else:
            out.append((a + w).astype(a.dtype))
    return out


@pytest.mark.parametrize("path", ["pairs_tail", "ring"])
def test_accumulate_and_out(path):
    eng = make(path, E_DRIVEN)
    E, R = eng.E, eng.R
    own = call(eng, FOLLOW)
    assert call(eng, FOLLOW) is own                                        # allocated once, reused
    mine = fresh(eng)
    members = ("n_joined", "gap_min", "hw_sum", "drac_max")
    start = dict(n_joined=5, gap_min=2.5, hw_sum=0.25, drac_max=0.125)     # a buffer that is not fresh: its values take part
    part = RoadFollowing(*[torch.full((E, R), start[f], dtype=torch.float32 if f in FLOATS else torch.int32, device=eng.device)
                           if f in members else None for f in NAMES])
    acc = host(fresh(eng))
    acc_part = host(part)
    states = 0
    for calls in (8, 10, 11):                                           # three states of the scenario: 24, 36 and 42 ticks
        run_scenario(eng, calls)
        want = model_of(eng, FOLLOW)
        assert call(eng, FOLLOW, accumulate=True, out=mine) is not own
        call(eng, FOLLOW, accumulate=True, out=part)
        acc = combine(acc, want)
        acc_part = combine(acc_part, want)
        states += int(want[1].sum() > 0)
        assert_following(host(call(eng, FOLLOW)), want, ("overwrite", calls))
    assert states == 3 and acc[4].any() and np.isfinite(acc[9]).any() and (acc[10] > 0).any()
    assert_following(host(mine), acc, "three accumulated calls")
    got = host(part)
    assert [g is None for g in got] == [f not in members for f in NAMES]
    assert_following(got, acc_part, "three accumulated calls, four members")
    assert (got[5] == np.float32(2.5)).any() and (got[5] < np.float32(2.5)).any()     # the buffer's own minimum took part
    # the engine's own tensors accumulate from 0 / +inf too
    run_scenario(eng, 11)
    assert_following(host(call(eng, FOLLOW)), model_of(eng, FOLLOW), "own, overwritten")
    assert_following(host(call(eng, FOLLOW, accumulate=True)), combine(model_of(eng, FOLLOW), model_of(eng, FOLLOW)), "own, twice")
    # without the flag a caller's tensors are overwritten, members left out stay out
    only = RoadFollowing(*[torch.full((E, R), -7.0, dtype=torch.float32, device=eng.device) if f == "ttc_min" else None for f in NAMES])
    assert_following(host(call(eng, FOLLOW, out=only)), model_of(eng, FOLLOW), "ttc_min alone")
    bad = [None] * len(NAMES)
    bad[0] = torch.zeros((E, R), dtype=torch.float32, device=eng.device)
    with pytest.raises(ValueError):
        call(eng, FOLLOW, out=RoadFollowing(*bad))


# ---- 5. more items than wavefronts -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["transposed", "ring"])
def test_stride_loop(layout):
    """9 envs of the 4x4 grid are 18 (env, tile) items (80 roads: a full tile and 16 lanes of a second).  The uncapped
    launch has a wavefront for every item (5 workgroups).  TFX_MEASURE_GRID=1 leaves one workgroup - four wavefronts, five
    rounds, the last one with two at work - and a cap of three workgroups twelve wavefronts and two rounds; a fresh
    accumulator per item gives the bits of the uncapped launch."""
    E = 9
    cfg = dict(m=4, n=4, length=120.0, capacity=14, rate=0.5)
    free = engine_with({"TFX_RESIDENT": "0"}, E, layout=layout, **cfg)
    one = engine_with({"TFX_RESIDENT": "0", "TFX_MEASURE_GRID": "1"}, E, layout=layout, **cfg)
    three = engine_with({"TFX_RESIDENT": "0", "TFX_GRID_CAP": "3"}, E, layout=layout, **cfg)
    items = E * ((free.R + 63) // 64)
    assert free.follow_launch() == (5, 20) and one.follow_launch() == (1, 4) and three.follow_launch() == (3, 12)
    assert free.R == 80 and items == 18 > three.follow_launch()[1]
    out = []
    for eng in (free, one, three):
        count = load_random(eng, 5)
        out.append([check(eng, p, (layout, eng.follow_launch())) for p in (PARAMS[3], PARAMS[0])])
    for other in out[1:]:
        for a, b in zip(out[0], other):
            assert all(a[k].tobytes() == b[k].tobytes() for k in NAMES)
    assert out[0][0]["n_pairs"].any(axis=1).all() and (out[0][1]["n_cars"] == count).all()     # every env has pairs in range


# ---- 6. errors -------------------------------------------------------------------------------------------------------------------------
def test_errors_are_codes_and_the_handle_stays_usable():
    lib = nat.lib()
    eng = make("pertick", 3)
    run_scenario(eng, 6)
    word = torch.zeros((eng.E, eng.R), dtype=torch.int32, device=eng.device)
    b = nat.TfxFollowBuffers()
    b.n_cars = C.c_void_p(word.data_ptr())
    st = eng._stream()
    P = nat.TfxFollowParams
    ok = P(0.0, 10.0, 0.5, 3.0)
    # before tfx_bind_buffers
    h = C.c_void_p()
    nat.check(lib.tfx_create(C.byref(eng.cfg), C.byref(h)))
    assert lib.tfx_road_following(h, C.byref(ok), C.byref(b), 0, st) == -2
    assert b"tfx_bind_buffers" in lib.tfx_last_error()
    nat.check(lib.tfx_destroy(h))
    nan = float("nan")
    for args, msg in (((C.byref(P(nan, 10.0, 0.5, 3.0)), C.byref(b), 0), b"NaN"), ((C.byref(P(0.0, nan, 0.5, 3.0)), C.byref(b), 0), b"NaN"),
                      ((C.byref(P(0.0, 10.0, nan, 3.0)), C.byref(b), 0), b"NaN"), ((C.byref(P(0.0, 10.0, 0.5, nan)), C.byref(b), 0), b"NaN"),
                      ((C.byref(P(0.0, 10.0, 0.0, 3.0)), C.byref(b), 0), b"v_min"), ((C.byref(P(0.0, 10.0, -1.0, 3.0)), C.byref(b), 0), b"v_min"),
                      ((C.byref(P(0.0, 10.0, -INF, 3.0)), C.byref(b), 0), b"v_min"),
                      ((C.byref(ok), C.byref(b), 2), b"flags"), ((C.byref(ok), C.byref(b), -1), b"flags"),
                      ((C.byref(ok), C.byref(nat.TfxFollowBuffers()), 0), b"null"), ((C.byref(ok), None, 0), b"out is null"),
                      ((None, C.byref(b), 0), b"p is null")):
        assert lib.tfx_road_following(eng.h, *args, st) == -1, msg
        assert msg in lib.tfx_last_error(), (msg, lib.tfx_last_error())
    assert lib.tfx_road_following(None, C.byref(ok), C.byref(b), 0, st) == -1
    torch.cuda.synchronize()
    assert not word.any()
    assert lib.tfx_road_following(eng.h, C.byref(P(-INF, INF, INF, INF)), C.byref(b), 0, st) == 0     # infinities are fine
    assert np.array_equal(word.cpu().numpy(), eng.cars_on_roads_flat().cpu().numpy()) and word.any()
    eng.step(3)
    check(eng, FOLLOW, "after the errors")


# ---- 7. TrafficVecEnv.following ------------------------------------------------------------------------------------------------------
def test_vec_env_following():
    from gym_traffic.envs.vec_env import TrafficVecEnv
    from gym_traffic.wrappers.vec import VecRemiRepeater
    E = 5
    venv = TrafficVecEnv(E, 3, 3, 120.0, capacity=14, spawn='periodic', spawn_period=3, seed=3)
    wrapped = VecRemiRepeater(venv, 5)
    wrapped.reset()
    eng = venv.engine
    r, I = eng.r, eng.I
    rng = np.random.RandomState(4)
    for d in range(9):
        wrapped.step(torch.as_tensor(rng.randint(2, size=(E, I)).astype(np.int32)).to(eng.device))
    for x_from in (None, FOLLOW[0], INF):
        f = wrapped.following(platoon_gap=FOLLOW[1], v_min=FOLLOW[2], ttc_crit=FOLLOW[3], x_from=x_from)    # through VecWrapper.__getattr__
        want = model_of(eng, (x_from,) + FOLLOW[1:])
        assert_following(host(f[:11]), want, "per road")
        w = dict(zip(NAMES, want))
        tot = {k: w[k][:, :r].sum(axis=1, dtype=np.int64) for k in NAMES if k not in FLOATS}
        assert f.pairs.dtype == torch.int64 and f.conflicts.dtype == torch.int64 and f.overlaps.dtype == torch.int64
        assert np.array_equal(f.pairs.cpu().numpy(), tot["n_pairs"]) and np.array_equal(f.conflicts.cpu().numpy(), tot["n_conflict"])
        assert np.array_equal(f.overlaps.cpu().numpy(), tot["n_overlap"])
        assert np.array_equal(f.platoons.cpu().numpy(), w["n_cars"].astype(np.int64) - w["n_joined"])
        assert same_bits(f.min_gap.cpu().numpy(), w["gap_min"][:, :r].min(axis=1))
        assert same_bits(f.min_ttc_s.cpu().numpy(), w["ttc_min"][:, :r].min(axis=1))
        assert same_bits(f.max_drac.cpu().numpy(), w["drac_max"][:, :r].max(axis=1))
        platoons = (w["n_cars"].astype(np.int64) - w["n_joined"])[:, :r].sum(axis=1)
        with np.errstate(all="ignore"):
            for got, num, den in ((f.mean_gap, w["gap_sum"][:, :r].astype(np.float64).sum(axis=1), tot["n_pairs"]),
                                  (f.mean_headway_s, w["hw_sum"][:, :r].astype(np.float64).sum(axis=1), tot["n_hw"]),
                                  (f.mean_platoon_size, tot["n_cars"].astype(np.float64), platoons)):
                got, mean = got.cpu().numpy(), np.where(den > 0, num / np.maximum(den, 1), np.nan)
                assert got.dtype == np.float64 and np.array_equal(np.isnan(got), den == 0)
                # a float64 sum of at most r float32 terms is good to about r * 2^-53 of the sum of their magnitudes
                assert np.all(np.abs(got - mean)[den > 0] <= 1e-9 * np.abs(mean)[den > 0]), (got, mean)
        if x_from is None:
            assert tot["n_pairs"].all() and tot["n_joined"].any() and np.isfinite(w["ttc_min"]).any() and tot["n_hw"].any()
        if x_from == INF:                                                  # empty denominators: nan, no exception
            assert np.isnan(f.mean_gap.cpu().numpy()).all() and np.isnan(f.mean_platoon_size.cpu().numpy()).all()
            assert np.isposinf(f.min_gap.cpu().numpy()).all() and not f.pairs.any()
    before = host(venv.following(x_from=None)[:11])
    acc = venv.following(x_from=None, accumulate=True)
    assert np.array_equal(acc.n_pairs.cpu().numpy(), 2 * before[1]) and np.array_equal(acc.pairs.cpu().numpy(), 2 * before[1][:, :r].sum(axis=1))
    assert same_bits(acc.gap_min.cpu().numpy(), before[5])


# ---- 8. the demo ---------------------------------------------------------------------------------------------------------------------
def test_following_demo_runs():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "following_demo.py"), "--envs", "8", "--m", "3", "--n", "3",
                          "--length", "120", "--capacity", "14", "--decisions", "10", "--ticks", "6", "--cycle", "12"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    print(out.stdout)
    rows = {ln.split("  ")[0].strip(): ln.split() for ln in out.stdout.splitlines()}
    assert "fixed cycle" in rows and "greedy (on device)" in rows
    for key in ("fixed cycle", "greedy (on device)"):
        conflicts, platoon, headway, overlaps = [float(t) for t in rows[key][-4:]]
        assert conflicts >= 0.0 and platoon >= 1.0 and headway > 0.0 and overlaps >= 0
    assert "median ms per decision" in out.stdout
