"""tfx_road_cells on the device (include/tfx.h, csrc/tfx_cells.hpp) against its definition in NumPy (devrng.road_cells)
applied to the engine's own ring planes - bit for bit: the counts with np.array_equal, speed_sum with same_bits - on
synthetic states through the ring import (unsorted positions, exact ties on the edges, cars out of range), on driven
states on every forced step path (and against the CPU oracle's run of the same scenario), and cross-checked with
tfx_road_measures (one cell [x_from, inf) must equal its n_cars / speed_sum bit for bit); plus: the call writes nothing,
accumulates, strides over more items than it has wavefronts, reports argument errors as codes, and feeds
TrafficVecEnv.cell_obs and tools/cells_demo.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_gpu_parity import same_bits
from test_gpu_fused import engine_with
from test_gpu_clone import assert_env_equal, make, snapshot
from test_measures_host import E_DRIVEN, GRID, HALT, oracle_driven, scenario
from test_cells_host import BAD_ARGS

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from gym_traffic import _native as nat  # noqa: E402
from gym_traffic.core import RoadCells  # noqa: E402
from gym_traffic.devrng import cell_edges, road_cells  # noqa: E402
from oracle.oracle import live_mask  # noqa: E402
from test_gpu_measures import DRIVEN, SEQUENCE, load_random, run_scenario, same_snapshot  # noqa: E402

INF = float("inf")
CELLS = (1, 5, 8, 32)           # the ends of the range, a non-power of two, two instantiation bounds (16: the synthetic test)
LENGTH = GRID["length"]


def planes(eng):
    x, v, _ = eng.planes_numpy()
    return x, v, eng.leading.cpu().numpy(), eng.lastcar.cpu().numpy()


def model_of(eng, edges):
    """the definition applied to the image tfx_export_ring produces right now"""
    x, v, ld, lc = planes(eng)
    return road_cells(x, v, ld, lc, eng.C, edges)


def host(rc):
    torch.cuda.synchronize()
    return [None if t is None else t.cpu().numpy().copy() for t in rc]


def assert_cells(got, want, where):
    n, s = got
    if n is not None:
        assert n.dtype == np.int32 and n.shape == want[0].shape, where
        assert np.array_equal(n, want[0]), ("n_cars", where, np.argwhere(n != want[0])[:5].tolist())
    if s is not None:
        assert s.dtype == np.float32 and s.shape == want[1].shape and same_bits(s, want[1]), ("speed_sum", where)


def check(eng, edges, where):
    got = host(eng.road_cells(edges))
    assert_cells(got, model_of(eng, edges), where)
    return got


def tie_edges(eng, B, lo=10.0, hi=110.0):
    """B cells with finite outer edges (cars below lo and from hi on are in no cell) whose inner edges are x values of
    live cars of the state: cars sit exactly on them."""
    x, _, ld, lc = planes(eng)
    live = np.stack([live_mask(ld[k], lc[k], eng.C) for k in range(eng.E)])
    u = np.unique(x[live])
    u = u[(u > lo) & (u < hi)]
    assert len(u) > B
    inner = u[np.linspace(0, len(u) - 1, B + 1).astype(int)[1:-1]]
    edges = np.concatenate([[lo], inner, [hi]]).astype(np.float32)
    assert (edges[:-1] < edges[1:]).all()
    return edges, int(np.isin(x[live], inner).sum()), int(((x[live] < lo) | (x[live] >= hi)).sum())


# ---- 1. synthetic states through the ring import -----------------------------------------------------------------------
@pytest.mark.parametrize("path,kind", [("pertick", "plain"), ("pertick", "validate"), ("pertick", "het"),
                                       ("ring", "plain"), ("ring", "validate")])
@pytest.mark.parametrize("capacity", [14, 66])          # 66: road counts 0 .. 64 straddle every multiple of the 8 rows in flight
@pytest.mark.parametrize("m,n", [(3, 3), (4, 4)])        # 48 roads: one partial tile; 80: a full tile and 16 lanes of a second
def test_synthetic_states(path, kind, capacity, m, n):
    eng = make(path, 5, kind, m=m, n=n, capacity=capacity)
    assert eng.R == {3: 48, 4: 80}[m]
    count = load_random(eng, 1000 * m + capacity)          # x is random per slot: unsorted down every road
    cars = eng.cars_on_roads_flat().cpu().numpy()
    assert np.array_equal(cars, count)
    for B in CELLS + (16,):
        got = check(eng, cell_edges(LENGTH, B), (path, kind, capacity, m, B, "uniform"))
        assert got[0].shape == (5, eng.R, B) and np.array_equal(got[0].sum(axis=-1), cars)       # no car left out
        if B > 1:
            assert ((got[0] > 0).sum(axis=-1) >= min(B, 3)).any() and (got[0] >= 2).any()
        edges, ties, outside = tie_edges(eng, B)
        assert outside > 0 and (B == 1 or ties >= B - 1)
        got = check(eng, edges, (path, kind, capacity, m, B, "ties"))
        assert got[0].sum() == cars.sum() - outside
    # one cell [x_from, inf) is tfx_road_measures' n_cars and speed_sum, bit for bit: the two kernels against each other
    for x_from in (-INF, 60.0, float(edges[1])):
        got = host(eng.road_cells([x_from, INF]))
        rm = host(eng.road_measures(0.1, x_from))
        assert np.array_equal(got[0][..., 0], rm[0]) and same_bits(got[1][..., 0], rm[3]), x_from
    assert rm[0].any() and rm[3].any()


# ---- 2. driven states on every forced path -----------------------------------------------------------------------------
@pytest.mark.parametrize("path", DRIVEN)
def test_driven_states(path):
    eng = make(path, E_DRIVEN)
    run_scenario(eng)
    if path.startswith("pairs"):
        # the run ended on a two-tick pass: columns that start a row or two down are really binned
        assert eng.pair_ticks() > 0 and eng.head_rows().any()
    if path.endswith("resident"):
        assert eng.fused_ticks()[0] > 0
    s = oracle_driven()
    for B in CELLS:
        for edges in (cell_edges(LENGTH, B), tie_edges(eng, B, 20.0, 100.0)[0]):
            got = check(eng, edges, (path, B))
            # HIP equals the oracle bit for bit, so its cells are the oracle's
            assert_cells(got, road_cells(s["x"], s["v"], s["leading"], s["lastcar"], eng.C, edges), (path, "oracle", B))
    got = check(eng, cell_edges(LENGTH, 8), path)
    assert ((got[0] > 0).sum(axis=-1) >= 3).any() and (got[0] >= 2).any() and not got[0][0].any()
    rm = host(eng.road_measures(HALT, None))
    assert np.array_equal(got[0].sum(axis=-1), rm[0])


def test_between_move_and_advance():
    """tick by tick: the image tfx_export_ring gives between tfx_move_cars and tfx_advance_finished_cars is binned too"""
    eng = make("pertick", E_DRIVEN)
    run_scenario(eng)
    act, cnt = scenario(eng.I, eng.n_entry, seed=77)[0]
    for t in range(3):
        eng.set_actions(act)
        eng.set_spawns(counts=cnt[0])
        eng.move_cars()
        got = check(eng, cell_edges(LENGTH, 8), ("after move_cars", t))
        check(eng, [0.0, 30.0, 60.0, 90.0, LENGTH], ("after move_cars, cars past the road end left out", t))
        assert got[0].any()
        eng.advance_finished_cars()
        check(eng, cell_edges(LENGTH, 8), ("after the advance", t))


# ---- 3. read-only ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path,kind", [("pairs_tail", "plain"), ("pertick", "validate"), ("ring", "plain")])
def test_binning_writes_nothing(path, kind):
    eng = make(path, E_DRIVEN, kind)
    run_scenario(eng)
    before = snapshot(eng)
    hb = eng.head_rows().copy()
    eng.road_cells(cell_edges(LENGTH, 8))
    eng.road_cells(cell_edges(LENGTH, 32), accumulate=True)
    same_snapshot(before, snapshot(eng))
    assert np.array_equal(hb, eng.head_rows())


@pytest.mark.parametrize("path", ["resident", "pairs_tail", "pairs_split", "pertick", "ring"])
def test_twin_that_is_never_binned(path):
    """An engine binned between every call of a mixed step / agent_step sequence stays bit-identical to one that never is."""
    E = E_DRIVEN
    eng, ref = make(path, E), make(path, E)
    rng = np.random.RandomState(31)
    for e_ in (eng, ref):
        e_.reset(np.zeros((E, eng.I), np.int32))
    cars = 0
    for kind, n in SEQUENCE:
        act = rng.randint(2, size=(E, eng.I)).astype(np.int32)
        cnt = ((rng.rand(n, E, eng.n_entry) < 0.15) * rng.randint(1, 3, size=(n, E, eng.n_entry))).astype(np.int32)
        eng.road_cells(cell_edges(LENGTH, 5))
        eng.road_cells(cell_edges(LENGTH, 32), accumulate=True)
        for e_ in (eng, ref):
            e_.set_actions(act)
            e_.set_spawns(counts=cnt, per_tick=True)
            (e_.agent_step if kind == "agent" else e_.step)(n)
        got = check(eng, cell_edges(LENGTH, 8), (path, kind, n))
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
    B = 8
    edges = cell_edges(LENGTH, B)
    own = eng.road_cells(edges)
    assert eng.road_cells(edges) is own                                   # allocated once per B, reused
    other = eng.road_cells(cell_edges(LENGTH, 5))                         # another B: tensors of its own shape
    assert other is not own and tuple(other.n_cars.shape) == (E, R, 5) and tuple(own.speed_sum.shape) == (E, R, B)
    assert eng.road_cells(edges) is own
    mine = RoadCells(torch.zeros((E, R, B), dtype=torch.int32, device=dev), torch.zeros((E, R, B), dtype=torch.float32, device=dev))
    part = RoadCells(None, torch.full((E, R, B), 0.25, dtype=torch.float32, device=dev))
    ints = np.zeros((E, R, B), np.int64)
    total = np.zeros((E, R, B), np.float32)
    t = np.full((E, R, B), 0.25, np.float32)
    states = 0
    for calls in (5, 8, 11):                                              # three different states of the scenario
        run_scenario(eng, calls)
        want = model_of(eng, edges)
        assert eng.road_cells(edges, accumulate=True, out=mine) is not own
        eng.road_cells(edges, accumulate=True, out=part)
        ints += want[0]
        total = (total + want[1]).astype(np.float32)                      # one float32 add per cell per call
        t = (t + want[1]).astype(np.float32)
        states += int(want[0].sum() > 0)
        assert_cells(host(eng.road_cells(edges)), want, ("overwrite", calls))
    assert states == 3 and total.any()
    assert_cells(host(mine), [ints.astype(np.int32), total], "three accumulated calls")
    assert same_bits(host(part)[1], t)
    # without the flag a caller's tensors are overwritten, a member left out stays out
    only = RoadCells(torch.full((E, R, B), -7, dtype=torch.int32, device=dev), None)
    got = host(eng.road_cells(edges, out=only))
    assert got[1] is None
    assert_cells(got, model_of(eng, edges), "counts alone")
    for bad in (RoadCells(torch.zeros((E, R, B), dtype=torch.float32, device=dev), None),
                RoadCells(None, torch.zeros((E, R, B), dtype=torch.int32, device=dev)),
                RoadCells(torch.zeros((E, R, B + 1), dtype=torch.int32, device=dev), None),
                RoadCells(torch.zeros((E, R), dtype=torch.int32, device=dev), None)):
        with pytest.raises(ValueError):
            eng.road_cells(edges, out=bad)


# ---- 5. more items than wavefronts -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["transposed", "ring"])
def test_stride_loop(layout):
    """300 envs of the 2x2 grid are 300 (env, tile) items (24 roads: one tile per env).  TFX_MEASURE_GRID=8 caps this
    handle's launch at 8 workgroups = 32 wavefronts, so every wavefront strides over nine or ten items - and clears and
    refills its LDS planes as often."""
    E = 300
    cfg = dict(m=2, n=2, length=120.0, capacity=10, rate=0.5)
    plain = engine_with({"TFX_RESIDENT": "0"}, 8, layout=layout, **cfg)
    assert plain.cells_launch(8) == (2, 8)
    eng = engine_with({"TFX_RESIDENT": "0", "TFX_MEASURE_GRID": "8"}, E, layout=layout, **cfg)
    for B in (8, 16, 32):
        assert eng.cells_launch(B) == (8, 32)
    assert eng.R == 24 and E * ((eng.R + 63) // 64) > 32
    count = load_random(eng, 5)
    for B in (5, 32):
        got = check(eng, cell_edges(120.0, B), (layout, B))
        assert np.array_equal(got[0].sum(axis=-1), count) and got[0].any(axis=(1, 2)).all()      # every env has cars
    check(eng, tie_edges(eng, 8)[0], (layout, "ties"))


# ---- 6. errors -------------------------------------------------------------------------------------------------------------------------
def test_errors_are_codes_and_the_handle_stays_usable():
    lib = nat.lib()
    eng = make("pertick", 3)
    run_scenario(eng, 6)
    B = 3
    word = torch.zeros((eng.E, eng.R, B), dtype=torch.int32, device=eng.device)
    b = nat.TfxCellBuffers()
    b.n_cars = C.c_void_p(word.data_ptr())
    st = eng._stream()

    def edges(*vals):
        return (C.c_float * len(vals))(*vals)

    good = edges(-INF, 40.0, 80.0, INF)
    # before tfx_bind_buffers
    h = C.c_void_p()
    nat.check(lib.tfx_create(C.byref(eng.cfg), C.byref(h)))
    assert lib.tfx_road_cells(h, good, B, C.byref(b), 0, st) == -2
    assert b"tfx_bind_buffers" in lib.tfx_last_error()
    nat.check(lib.tfx_destroy(h))
    for args, msg in BAD_ARGS(good, edges, b, nat.TfxCellBuffers(), float("nan")):
        assert lib.tfx_road_cells(eng.h, *args, st) == -1, msg
        assert msg in lib.tfx_last_error(), (msg, lib.tfx_last_error())
    assert lib.tfx_road_cells(None, good, B, C.byref(b), 0, st) == -1 and b"null handle" in lib.tfx_last_error()
    with pytest.raises(ValueError):
        eng.road_cells(np.arange(34, dtype=np.float32))                  # 33 cells
    with pytest.raises(ValueError):
        eng.road_cells([1.0])                                            # no cell
    with pytest.raises(nat.TfxError, match="ascending"):
        eng.road_cells([0.0, 50.0, 50.0])
    torch.cuda.synchronize()
    assert not word.any()
    assert lib.tfx_road_cells(eng.h, good, B, C.byref(b), 0, st) == 0
    assert np.array_equal(word.sum(dim=-1).cpu().numpy(), eng.cars_on_roads_flat().cpu().numpy()) and word.any()
    eng.step(3)
    check(eng, cell_edges(LENGTH, 8), "after the errors")


# ---- 7. TrafficVecEnv.cell_obs -----------------------------------------------------------------------------------------------------
def test_vec_env_cell_obs():
    from gym_traffic.core import ARCHETYPE
    from gym_traffic.envs.vec_env import TrafficVecEnv
    from gym_traffic.wrappers.vec import VecRemiRepeater
    E, m, n = 5, 3, 3
    venv = TrafficVecEnv(E, m, n, 120.0, capacity=14, spawn='periodic', spawn_period=3, seed=3)
    wrapped = VecRemiRepeater(venv, 5)
    wrapped.reset()
    eng = venv.engine
    rng = np.random.RandomState(4)
    for d in range(9):
        wrapped.step(torch.as_tensor(rng.randint(2, size=(E, eng.I)).astype(np.int32)).to(eng.device))
    for B, v_scale in ((8, None), (5, 2.5)):
        obs = wrapped.cell_obs(n_cells=B, v_scale=v_scale)               # through VecWrapper.__getattr__
        edges = cell_edges(120.0, B)
        cars, total = model_of(eng, edges)
        assert_cells(host(obs[:2]), (cars, total), "per road and cell")
        img = obs.image
        assert img.dtype == torch.float32 and tuple(img.shape) == (E, 2, 4, B, m, n) and img.is_contiguous()
        flat = img.view(E, 8 * B, m, n)
        assert flat.data_ptr() == img.data_ptr()                         # the channels-first form is no copy
        got = img.cpu().numpy()
        scale = np.float32(ARCHETYPE["car_v0"] if v_scale is None else v_scale)
        seen = 0
        for d in range(4):
            for row in range(m):
                for col in range(n):
                    road = d * m * n + row * n + col
                    assert int(venv.graph.dest[road]) == row * n + col
                    assert np.array_equal(got[:, 0, d, :, row, col], cars[:, road].astype(np.float32))
                    cnt, tot = cars[:, road], total[:, road]
                    with np.errstate(invalid="ignore", divide="ignore"):
                        want = np.where(cnt > 0, tot / cnt.astype(np.float32) / scale, np.float32(0)).astype(np.float32)
                    mean = got[:, 1, d, :, row, col]
                    assert (mean[cnt == 0] == 0).all()
                    # torch's divisions are outside this library's bit contract: 1 ulp, not 0
                    assert (np.abs(mean - want) <= np.spacing(np.abs(want))).all(), (d, row, col)
                    seen += int((cnt > 0).sum())
        assert seen > 20 and total.any()
        assert np.array_equal(flat.cpu().numpy()[:, B:2 * B], got[:, 0, 1])
    # explicit edges; accumulate adds to the engine's tensors
    edges = [0.0, 50.0, 100.0, 120.0]
    once = host(venv.cell_obs(edges=edges)[:2])
    twice = venv.cell_obs(edges=edges, accumulate=True)
    assert tuple(twice.image.shape) == (E, 2, 4, 3, m, n) and np.array_equal(twice.n_cars.cpu().numpy(), 2 * once[0])


# ---- 8. the demo ---------------------------------------------------------------------------------------------------------------------
def test_cells_demo_runs():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "cells_demo.py"), "--envs", "8", "--m", "3", "--n", "3",
                          "--length", "120", "--capacity", "14", "--decisions", "6", "--ticks", "6"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    print(out.stdout)
    ret = float(out.stdout.split("mean return per env")[1].split()[0])
    assert np.isfinite(ret)
    ms = out.stdout.split("median ms per decision:")[1].split()
    vals = dict(zip(ms[0::2], map(float, ms[1::2])))
    assert set(vals) == {"env", "cells", "policy"} and all(np.isfinite(x) and x >= 0.0 for x in vals.values())
