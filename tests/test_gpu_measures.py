"""tfx_road_measures on the device (include/tfx.h, csrc/tfx_measure.hpp) against its definition in NumPy
(devrng.road_measures) applied to the engine's own ring planes - bit for bit: the three integer fields with
np.array_equal, speed_sum with same_bits - on synthetic states through the ring import, on driven states on every forced
step path (and against the CPU oracle's run of the same scenario, tests/test_measures_host.py), plus: the call writes
nothing, accumulates, strides over more items than it has wavefronts, reports argument errors as codes, and feeds
TrafficVecEnv.measures and tools/pressure_demo.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_gpu_parity import same_bits
from test_gpu_fused import engine_with
from test_gpu_clone import ARCH, PATHS, assert_env_equal, make, snapshot
from test_measures_host import CALLS, E_DRIVEN, GRID, HALT, X_FROM, oracle_driven, random_rings, scenario

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from gym_traffic import _native as nat  # noqa: E402
from gym_traffic.core import RoadMeasures  # noqa: E402
from gym_traffic.devrng import road_measures  # noqa: E402

NAMES = RoadMeasures._fields


def model_of(eng, halt, x_from):
    """the definition applied to the image tfx_export_ring produces right now"""
    x, v, _ = eng.planes_numpy()
    return road_measures(x, v, eng.leading.cpu().numpy(), eng.lastcar.cpu().numpy(), eng.C, halt, x_from)


def host(rm):
    torch.cuda.synchronize()
    return [None if t is None else t.cpu().numpy().copy() for t in rm]


def assert_measures(got, want, where):
    for name, g, w in zip(NAMES, got, want):
        if g is None:
            continue
        if name == "speed_sum":
            assert g.dtype == np.float32 and same_bits(g, w), (name, where)
        else:
            assert g.dtype == np.int32 and np.array_equal(g, w), (name, where, np.argwhere(g != w)[:5].tolist())


def check(eng, halt, x_from, where):
    got = host(eng.road_measures(halt, x_from))
    want = model_of(eng, halt, x_from)
    assert_measures(got, want, where)
    return got


def load_random(eng, seed):
    rng = np.random.RandomState(seed)
    E, R, Cc = eng.E, eng.R, eng.C
    x, v, ld, lc, n = random_rings(rng, E * R, Cc)
    assert (n == 0).any() and (n == Cc - 2).any() and (ld > lc).any()
    w = rng.randint(0, 50, size=(E, R, Cc)).astype(np.float32)
    arch = rng.randint(len(ARCH), size=(E, R, Cc)).astype(np.uint8) if eng.het else None
    eng.reset(np.zeros((E, eng.I), np.int32))
    eng.load_state(x.reshape(E, R, Cc), v.reshape(E, R, Cc), ld.reshape(E, R), lc.reshape(E, R), w=w, arch=arch)
    return n.reshape(E, R)


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
    for halt, x_from in ((0.1, None), (0.1, float("inf")), (0.1, 60.0), (0.0, 30.0), (float("inf"), 90.0), (1.0, float("-inf"))):
        got = check(eng, halt, x_from, (path, kind, capacity, m, halt, x_from))
        if x_from in (None, float("-inf")):
            assert np.array_equal(got[0], count) and np.array_equal(got[0], eng.cars_on_roads_flat().cpu().numpy())
        if x_from == float("inf"):
            assert not any(g.any() for g in got)
    got = check(eng, 0.1, 60.0, "again")
    assert (got[2] >= 2).any() and (got[1] > got[2]).any() and (got[0] < count).any() and (got[3] > 0).any()


# ---- 2. driven states on every forced path -----------------------------------------------------------------------------
DRIVEN = ["resident", "pertick", "pairs_tail", "pairs_launches", "pairs_split", "pairs_seg", "ring", "ring_resident"]


def run_scenario(eng, calls=None):
    eng.reset(np.zeros((eng.E, eng.I), np.int32))
    for act, cnt in scenario(eng.I, eng.n_entry, E=eng.E)[:calls]:
        eng.set_actions(act)
        eng.set_spawns(counts=cnt, per_tick=True)
        eng.step(cnt.shape[0])


@pytest.mark.parametrize("path", DRIVEN)
def test_driven_states(path):
    eng = make(path, E_DRIVEN)
    assert dict(GRID) == dict(m=eng.m, n=eng.n, length=float(eng.cfg.length), capacity=eng.C, rate=float(eng.cfg.rate))
    run_scenario(eng)
    if path.startswith("pairs"):
        # the run ended on a two-tick pass: columns that start a row or two down are really measured
        assert eng.pair_ticks() > 0 and eng.head_rows().any()
    if path.endswith("resident"):
        assert eng.fused_ticks()[0] > 0
    s = oracle_driven()
    for halt, x_from in ((HALT, X_FROM), (HALT, None), (2.0, 30.0)):
        got = check(eng, halt, x_from, (path, halt, x_from))
        # HIP equals the oracle bit for bit, so its measures are the oracle's
        assert_measures(got, road_measures(s["x"], s["v"], s["leading"], s["lastcar"], eng.C, halt, x_from), (path, "oracle", halt, x_from))
    got = check(eng, HALT, X_FROM, path)
    assert (got[2] >= 2).any() and (got[1] > got[2]).any() and (got[0] == 0).any()


def test_between_move_and_advance():
    """tick by tick: the image tfx_export_ring gives between tfx_move_cars and tfx_advance_finished_cars is measured too"""
    eng = make("pertick", E_DRIVEN)
    run_scenario(eng)
    act, cnt = scenario(eng.I, eng.n_entry, seed=77)[0]
    for t in range(3):
        eng.set_actions(act)
        eng.set_spawns(counts=cnt[0])
        eng.move_cars()
        got = check(eng, HALT, X_FROM, ("after move_cars", t))
        check(eng, 3.0, None, ("after move_cars, every car", t))
        assert got[0].any()
        eng.advance_finished_cars()
        check(eng, HALT, X_FROM, ("after the advance", t))


# ---- 3. read-only ------------------------------------------------------------------------------------------------------------
def same_snapshot(a, b):
    (A, _), (B, _) = a, b
    for k in A:
        if isinstance(A[k], np.ndarray):
            assert A[k].tobytes() == B[k].tobytes(), k
        else:
            assert A[k] is B[k] or A[k] == B[k], k


@pytest.mark.parametrize("path,kind", [("pairs_tail", "plain"), ("pertick", "validate"), ("ring", "plain")])
def test_measuring_writes_nothing(path, kind):
    eng = make(path, E_DRIVEN, kind)
    run_scenario(eng)
    before = snapshot(eng)
    hb = eng.head_rows().copy()
    eng.road_measures(HALT, X_FROM)
    eng.road_measures(HALT, None, accumulate=True)
    same_snapshot(before, snapshot(eng))
    assert np.array_equal(hb, eng.head_rows())


SEQUENCE = [("step", 1), ("step", 4), ("agent", 6), ("agent", 6), ("step", 4), ("step", 3), ("agent", 6), ("step", 2), ("step", 4),
            ("agent", 5), ("agent", 6), ("step", 7), ("step", 4), ("step", 1), ("agent", 6)]      # (repeats replay captured graphs)


@pytest.mark.parametrize("path", ["resident", "pairs_tail", "pairs_split", "pertick", "ring"])
def test_twin_that_never_measures(path):
    """An engine measured between every call of a mixed step / agent_step sequence stays bit-identical to one that never is."""
    E = E_DRIVEN
    eng, ref = make(path, E), make(path, E)
    rng = np.random.RandomState(31)
    for e_ in (eng, ref):
        e_.reset(np.zeros((E, eng.I), np.int32))
    cars = 0
    for kind, n in SEQUENCE:
        act = rng.randint(2, size=(E, eng.I)).astype(np.int32)
        cnt = ((rng.rand(n, E, eng.n_entry) < 0.15) * rng.randint(1, 3, size=(n, E, eng.n_entry))).astype(np.int32)
        eng.road_measures(HALT, X_FROM)
        eng.road_measures(HALT, None, accumulate=True)
        for e_ in (eng, ref):
            e_.set_actions(act)
            e_.set_spawns(counts=cnt, per_tick=True)
            (e_.agent_step if kind == "agent" else e_.step)(n)
        got = check(eng, HALT, X_FROM, (path, kind, n))
        cars = int(got[0].sum())
        sa, sb = snapshot(eng), snapshot(ref)
        for k in range(E):
            assert_env_equal(sa, k, sb, k, (path, kind, n))
        assert np.array_equal(eng.head_rows(), ref.head_rows())
    assert cars > 0


# ---- 4. accumulate, NULL members, the caller's tensors ---------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["pairs_tail", "ring"])
def test_accumulate_and_out(path):
    eng = make(path, E_DRIVEN)
    E, R, dev = eng.E, eng.R, eng.device
    own = eng.road_measures(HALT, X_FROM)
    assert eng.road_measures(HALT, X_FROM) is own                       # allocated once, reused
    mine = RoadMeasures(torch.zeros((E, R), dtype=torch.int32, device=dev), torch.zeros((E, R), dtype=torch.int32, device=dev),
                        torch.zeros((E, R), dtype=torch.int32, device=dev), torch.zeros((E, R), dtype=torch.float32, device=dev))
    part = RoadMeasures(None, torch.full((E, R), 5, dtype=torch.int32, device=dev), None,
                        torch.full((E, R), 0.25, dtype=torch.float32, device=dev))
    ints = [np.zeros((E, R), np.int64) for _ in range(3)]
    total = np.zeros((E, R), np.float32)
    states = 0
    for calls in (5, 8, 11):                                            # three different states of the scenario
        run_scenario(eng, calls)
        want = model_of(eng, HALT, X_FROM)
        assert eng.road_measures(HALT, X_FROM, accumulate=True, out=mine) is not own
        eng.road_measures(HALT, X_FROM, accumulate=True, out=part)
        for acc, wv in zip(ints, want[:3]):
            acc += wv
        total = (total + want[3]).astype(np.float32)                    # one float32 add of the road's sum per call
        states += int(want[0].sum() > 0)
        assert_measures(host(eng.road_measures(HALT, X_FROM)), want, ("overwrite", calls))
    assert states == 3 and total.any()
    got = host(mine)
    assert_measures(got, [a.astype(np.int32) for a in ints] + [total], "three accumulated calls")
    got = host(part)
    assert np.array_equal(got[1], ints[1] + 5)
    t = np.full((E, R), 0.25, np.float32)
    for calls in (5, 8, 11):
        run_scenario(eng, calls)
        t = (t + model_of(eng, HALT, X_FROM)[3]).astype(np.float32)
    assert same_bits(got[3], t)
    # without the flag a caller's tensors are overwritten, members left out stay out
    only = RoadMeasures(None, None, torch.full((E, R), -7, dtype=torch.int32, device=dev), None)
    assert_measures(host(eng.road_measures(HALT, X_FROM, out=only)), model_of(eng, HALT, X_FROM), "queue alone")
    with pytest.raises(ValueError):
        eng.road_measures(out=RoadMeasures(torch.zeros((E, R), dtype=torch.float32, device=dev), None, None, None))


# ---- 5. more items than wavefronts -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["transposed", "ring"])
def test_stride_loop(layout):
    """300 envs of the 2x2 grid are 300 (env, tile) items (24 roads: one tile per env).  The launch is one wavefront per
    item, four to a workgroup, capped at 16 workgroups per compute unit (tfx_measure_launch reports what the code uses):
    the default launch therefore has 75 workgroups and no wavefront takes a second item.  TFX_MEASURE_GRID=8 caps this
    handle's launch at 8 workgroups = 32 wavefronts, so every wavefront strides over nine or ten items."""
    E = 300
    cfg = dict(m=2, n=2, length=120.0, capacity=10, rate=0.5)
    plain = engine_with({"TFX_RESIDENT": "0"}, 8, layout=layout, **cfg)
    assert plain.measure_launch() == (2, 8)
    eng = engine_with({"TFX_RESIDENT": "0", "TFX_MEASURE_GRID": "8"}, E, layout=layout, **cfg)
    grid, waves = eng.measure_launch()
    assert (grid, waves) == (8, 32) and eng.R == 24 and E * ((eng.R + 63) // 64) > waves
    count = load_random(eng, 5)
    got = check(eng, 0.1, 60.0, layout)
    assert got[0].any(axis=1).all() and (got[0] <= count).all()          # every env has cars in range
    check(eng, 0.1, None, layout)


# ---- 6. errors -------------------------------------------------------------------------------------------------------------------------
def test_errors_are_codes_and_the_handle_stays_usable():
    lib = nat.lib()
    eng = make("pertick", 3)
    run_scenario(eng, 6)
    word = torch.zeros((eng.E, eng.R), dtype=torch.int32, device=eng.device)
    b = nat.TfxMeasureBuffers()
    b.n_cars = C.c_void_p(word.data_ptr())
    st = eng._stream()
    # before tfx_bind_buffers
    h = C.c_void_p()
    nat.check(lib.tfx_create(C.byref(eng.cfg), C.byref(h)))
    assert lib.tfx_road_measures(h, 0.1, 0.0, C.byref(b), 0, st) == -2
    assert b"tfx_bind_buffers" in lib.tfx_last_error()
    nat.check(lib.tfx_destroy(h))
    for args, msg in (((float("nan"), 0.0, C.byref(b), 0), b"NaN"), ((0.1, float("nan"), C.byref(b), 0), b"NaN"),
                      ((0.1, 0.0, C.byref(b), 2), b"flags"), ((0.1, 0.0, C.byref(b), -1), b"flags"),
                      ((0.1, 0.0, C.byref(nat.TfxMeasureBuffers()), 0), b"null"), ((0.1, 0.0, None, 0), b"out is null")):
        assert lib.tfx_road_measures(eng.h, *args, st) == -1, args
        assert msg in lib.tfx_last_error(), (args, lib.tfx_last_error())
    assert lib.tfx_road_measures(None, 0.1, 0.0, C.byref(b), 0, st) == -1
    torch.cuda.synchronize()
    assert not word.any()
    assert lib.tfx_road_measures(eng.h, float("inf"), float("-inf"), C.byref(b), 0, st) == 0      # infinities are fine
    assert np.array_equal(word.cpu().numpy(), eng.cars_on_roads_flat().cpu().numpy()) and word.any()
    eng.step(3)
    check(eng, HALT, X_FROM, "after the errors")


# ---- 7. TrafficVecEnv.measures -------------------------------------------------------------------------------------------------------
def test_vec_env_measures():
    from gym_traffic.envs.vec_env import TrafficVecEnv
    from gym_traffic.wrappers.vec import VecRemiRepeater
    E = 5
    venv = TrafficVecEnv(E, 3, 3, 120.0, capacity=14, spawn='periodic', spawn_period=3, seed=3)
    wrapped = VecRemiRepeater(venv, 5)
    wrapped.reset()
    eng, g = venv.engine, venv.graph
    r, I = eng.r, eng.I
    rng = np.random.RandomState(4)
    for d in range(9):
        wrapped.step(torch.as_tensor(rng.randint(2, size=(E, I)).astype(np.int32)).to(eng.device))
    for x_from in (None, X_FROM):
        m = wrapped.measures(halt_speed=HALT, x_from=x_from)             # through VecWrapper.__getattr__
        want = model_of(eng, HALT, x_from)
        assert_measures(host(m[:4]), want, "per road")
        n, h, q, s = want
        assert m.halted.dtype == torch.int64 and m.cars.dtype == torch.int64 and m.pressure.dtype == torch.int64
        assert np.array_equal(m.cars.cpu().numpy(), n[:, :r].sum(axis=1, dtype=np.int64))
        assert np.array_equal(m.halted.cpu().numpy(), h[:, :r].sum(axis=1, dtype=np.int64))
        pressure = np.zeros((E, I, 2), np.int64)
        for e in range(r):
            pressure[:, g.dest[e], g.phases[e]] += n[:, e].astype(np.int64) - n[:, g.nexts[e]]
        assert m.pressure.shape == (E, I, 2) and np.array_equal(m.pressure.cpu().numpy(), pressure)
        cars = n[:, :r].sum(axis=1)
        mean = np.where(cars > 0, s[:, :r].astype(np.float64).sum(axis=1) / np.maximum(cars, 1), 0.0)
        got = m.mean_speed.cpu().numpy()
        assert got.dtype == np.float64
        # a float64 sum of at most r float32 terms is good to about r * 2^-53
        assert np.all(np.abs(got - mean) <= 1e-9 * np.abs(mean)), (got, mean)
        assert cars.all() and h.any() and pressure.any() and (pressure[..., 0] != pressure[..., 1]).any()
    before = host(venv.measures(HALT, None)[:4])
    acc = venv.measures(HALT, None, accumulate=True)
    assert np.array_equal(acc.n_halted.cpu().numpy(), 2 * before[1]) and np.array_equal(acc.cars.cpu().numpy(), 2 * before[0][:, :r].sum(axis=1))


# ---- 8. the demo ---------------------------------------------------------------------------------------------------------------------
def test_pressure_demo_runs():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "pressure_demo.py"), "--envs", "8", "--m", "3", "--n", "3",
                          "--length", "120", "--capacity", "14", "--decisions", "6", "--ticks", "6"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    print(out.stdout)
    rows = {ln.split("  ")[0].strip(): ln.split() for ln in out.stdout.splitlines()}
    assert "max pressure" in rows and "greedy (on device)" in rows
    for key in ("max pressure", "greedy (on device)"):
        ret, halted = float(rows[key][-2]), float(rows[key][-1])
        assert np.isfinite(ret) and halted >= 0.0
    assert "median ms per decision" in out.stdout
