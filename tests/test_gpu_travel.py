"""Travel times on the device (tfx_car_ages / k_ages, tfx_trip_stats / k_trips: include/tfx.h, csrc/tfx_travel.hpp) against
their rules in NumPy (devrng.car_ages, devrng.trip_stats) - integers, so np.array_equal throughout: on synthetic side planes
through the ring import and synthetic logs written into the bound buffers, on the driven scenario of
tests/test_travel_host.py on every step path a validate handle has (and against the CPU oracle's run of it), plus: the
calls write nothing, follow the handle's own clock across clones, stride over more items than they have wavefronts,
report argument errors as codes, and feed TrafficVecEnv.travel_times and tools/travel_demo.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_gpu_fused import engine_with
from test_gpu_clone import ARCH, PATHS, assert_env_equal, make, snapshot
from test_measures_host import random_rings
from test_travel_host import E_DRIVEN, EDGES, GRID, HOLD, SMALL_CAP, TICKS, oracle_driven, scenario

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from gym_traffic import _native as nat  # noqa: E402
from gym_traffic import devrng  # noqa: E402
from gym_traffic.core import CarAges, TripStats  # noqa: E402


def host(ts):
    torch.cuda.synchronize()
    return [None if t is None else t.cpu().numpy().copy() for t in ts]


def ages_model(eng):
    """the definition applied to the image tfx_export_ring produces right now, at the engine's clock"""
    _, _, w = eng.planes_numpy()
    return devrng.car_ages(w, eng.leading.cpu().numpy(), eng.lastcar.cpu().numpy(), eng.C, eng.tick, het=eng.het)


def assert_fields(got, want, names, where):
    for name, g, w in zip(names, got, want):
        if g is None:
            assert w is None or name == "hist", (name, where)
            continue
        assert g.dtype == w.dtype and np.array_equal(g, w), (name, where, np.argwhere(g != w)[:5].tolist())


def check_ages(eng, where):
    got = host(eng.car_ages())
    assert_fields(got, ages_model(eng), CarAges._fields, where)
    return got


def zeros_like_stats(eng, n_bins):
    dev = eng.device
    return TripStats(torch.zeros((eng.E,), dtype=torch.int32, device=dev), torch.zeros((eng.E,), dtype=torch.int64, device=dev),
                     torch.zeros((eng.E,), dtype=torch.int32, device=dev), torch.zeros((eng.E,), dtype=torch.int32, device=dev),
                     torch.zeros((eng.E, n_bins), dtype=torch.int32, device=dev) if n_bins else None)


# ---- 1. synthetic ages through the ring import ----------------------------------------------------------------------------
@pytest.mark.parametrize("path,kind", [("pertick", "validate"), ("pertick", "het"), ("ring", "validate")])
@pytest.mark.parametrize("capacity", [14, 66])          # 66: road counts 0 .. 64 straddle every multiple of WALK_P = 8
@pytest.mark.parametrize("m,n", [(3, 3), (4, 4)])        # 48 roads: one partial tile; 80: a full tile and 16 lanes of a second
def test_synthetic_ages(path, kind, capacity, m, n):
    eng = make(path, 5, kind, m=m, n=n, capacity=capacity)
    E, R, Cc = eng.E, eng.R, eng.C
    assert R == {3: 48, 4: 80}[m]
    rng = np.random.RandomState(1000 * m + capacity)
    x, v, ld, lc, count = random_rings(rng, E * R, Cc)
    assert (count == 0).any() and (count == Cc - 2).any() and (ld > lc).any()
    if capacity == 66:
        assert set(range(0, 65, 8)) <= set(count.tolist()) | set((count + 1).tolist())
    M = 1 << 24
    now = M + 37 if kind == "het" else 5000               # het: spawn ticks are kept modulo 2^24, the clock is past it
    born = now - rng.randint(0, 5001, size=(E, R, Cc))
    born[rng.rand(E, R, Cc) < 0.1] = now                   # spawned in this very tick: age 0
    if kind == "het":
        assert (born < M).any() and (born >= M).any()
        born = born % M
    arch = rng.randint(len(ARCH), size=(E, R, Cc)).astype(np.uint8) if eng.het else None
    eng.reset(np.zeros((E, eng.I), np.int32))
    eng.set_tick(now)
    eng.load_state(x.reshape(E, R, Cc), v.reshape(E, R, Cc), ld.reshape(E, R), lc.reshape(E, R), w=born.astype(np.float32), arch=arch)
    got = check_ages(eng, (path, kind, capacity, m))
    assert np.array_equal(got[0], count.reshape(E, R)) and np.array_equal(got[0], eng.cars_on_roads_flat().cpu().numpy())
    assert got[2].max() > 4000 and (got[2][got[0] > 0] <= 5000).all() and not got[2][got[0] == 0].any()
    assert (got[1] >= got[2]).all() and (got[1] > got[2]).any()
    # accumulate twice into the caller's tensors: doubled sums, the same maximum
    dev = eng.device
    mine = CarAges(torch.zeros((E, R), dtype=torch.int32, device=dev), torch.zeros((E, R), dtype=torch.int64, device=dev),
                   torch.zeros((E, R), dtype=torch.int32, device=dev))
    eng.car_ages(accumulate=True, out=mine)
    assert eng.car_ages(accumulate=True, out=mine) is not eng.car_ages()
    twice = host(mine)
    assert np.array_equal(twice[0], 2 * got[0]) and np.array_equal(twice[1], 2 * got[1]) and np.array_equal(twice[2], got[2])
    # members left out stay out; without the flag the caller's tensors are overwritten
    only = CarAges(None, None, torch.full((E, R), -7, dtype=torch.int32, device=dev))
    assert np.array_equal(host(eng.car_ages(out=only))[2], got[2])
    with pytest.raises(ValueError):
        eng.car_ages(out=CarAges(None, torch.zeros((E, R), dtype=torch.int32, device=dev), None))


# ---- 2. synthetic logs, written straight into the bound buffers ----------------------------------------------------------
# (n_trips, cursor): spans of 0, 1, 63, 64, 65 and 200 entries from the start and from a cursor; a log past its cap; cursors
# at n, above n, above the cap, negative
BIG = [(0, 0), (1, 0), (63, 0), (64, 0), (65, 0), (200, 0), (70, 7), (100, 36), (255, 190), (256, 56), (300, 100), (300, 280),
       (50, 50), (20, 33), (5, -1), (256, 256), (1000, 0)]
SMALL = [(3, 0), (3, 1), (3, 3), (3, 5), (8, 0), (8, 8), (9, 0), (9, 2), (9, 8), (9, 9), (40, 0), (40, 8), (40, 20), (40, 40), (40, 41)]
BINS = {0: None, 1: [30, 200], 7: EDGES, 32: [10 * k for k in range(16)] + [150] + [160 + 15 * k for k in range(16)]}


@pytest.mark.parametrize("n_bins", [0, 1, 7, 32])
@pytest.mark.parametrize("cap,cases", [(256, BIG), (8, SMALL)])
def test_synthetic_logs(cap, cases, n_bins):
    edges = BINS[n_bins]
    assert n_bins == 0 or (len(edges) == n_bins + 1 and (np.diff(edges) >= 0).all())
    assert n_bins != 32 or (np.diff(edges) == 0).any()
    E = len(cases)
    eng = make("pertick", E, "validate", m=2, n=2, trip_cap=cap)
    rng = np.random.RandomState(cap + n_bins)
    log = (rng.randint(1, 400, size=(E, cap)) / 2.0).astype(np.float32)
    n = np.array([c[0] for c in cases], np.int32)
    cur0 = np.array([c[1] for c in cases], np.int32)
    eng.trip_times.copy_(torch.as_tensor(log).to(eng.device))
    eng.n_trips.copy_(torch.as_tensor(n).to(eng.device))
    cursor = torch.as_tensor(cur0.copy()).to(eng.device)
    want = devrng.trip_stats(log, n, cap, cur0, edges)
    spans = set(want[0].tolist())
    assert ({0, 1, 63, 64, 65, 200} <= spans) if cap == 256 else ({0, 2, 3, 8} <= spans and (want[3] > 0).any())
    got = host(eng.trip_stats(edges=edges, cursor=cursor))
    assert (got[4] is None) == (n_bins == 0)
    assert_fields(got, want[:5], TripStats._fields, (cap, n_bins))
    assert np.array_equal(cursor.cpu().numpy(), want[5]) and np.array_equal(want[5], n)
    # the log itself is not written
    assert np.array_equal(eng.trip_times.cpu().numpy(), log) and np.array_equal(eng.n_trips.cpu().numpy(), n)
    # a second call with the advanced cursor finds nothing new
    again = host(eng.trip_stats(edges=edges, cursor=cursor))
    assert not any(a.any() for a in again if a is not None) and np.array_equal(cursor.cpu().numpy(), n)
    # no cursor: the whole log; accumulate: added to and maxed, and the caller's tensors
    whole = devrng.trip_stats(log, n, cap, None, edges)
    mine = zeros_like_stats(eng, n_bins)
    mine.tick_max.fill_(150)
    eng.trip_stats(edges=edges, accumulate=True, out=mine)
    twice = host(eng.trip_stats(edges=edges, accumulate=True, out=mine))
    for k in (0, 1, 3) + ((4,) if n_bins else ()):
        assert np.array_equal(twice[k], 2 * whole[k]), k
    assert np.array_equal(twice[2], np.maximum(whole[2], 150))
    # members left out stay out
    part = TripStats(None, torch.full((E,), -5, dtype=torch.int64, device=eng.device), None, None, None)
    assert np.array_equal(host(eng.trip_stats(out=part))[1], whole[1])


# ---- 3. driven runs on every path of a validate handle --------------------------------------------------------------------
VALIDATE_PATHS = [p for p in PATHS if "resident" not in p]       # (a handle that logs trips never runs LDS-resident)
assert len(VALIDATE_PATHS) >= 7 and "ring" in VALIDATE_PATHS and "pairs_seg" in VALIDATE_PATHS
# tfx_step calls per held action (HOLD = 10 ticks each): mixed lengths, the run ends on three pairs
SPLITS = [[1, 4, 5], [3, 2, 5], [7, 3], [6, 4], [10], [2, 8], [5, 5], [1, 1, 8], [4, 6], [9, 1], [2, 2, 6], [4, 6]]
assert len(SPLITS) == TICKS // HOLD and all(sum(s) == HOLD for s in SPLITS)


def drive(eng, agent, after_call=None):
    eng.reset(np.zeros((eng.E, eng.I), np.int32))
    for (act, cnt), split in zip(scenario(eng.I, eng.n_entry, E=eng.E), SPLITS):
        eng.set_actions(act)
        off = 0
        for n in ([HOLD] if agent else split):
            eng.set_spawns(counts=cnt[off:off + n], per_tick=True)
            (eng.agent_step if agent else eng.step)(n)
            off += n
            if after_call:
                after_call()


@pytest.mark.parametrize("path,agent,cap", [(p, False, 4096) for p in VALIDATE_PATHS] +
                         [("pairs_tail", True, 4096), ("pertick", True, 4096), ("pairs_tail", False, SMALL_CAP), ("ring", False, SMALL_CAP)])
def test_driven_runs(path, agent, cap):
    eng = make(path, E_DRIVEN, "validate", trip_cap=cap, **GRID)
    assert dict(GRID) == dict(m=eng.m, n=eng.n, length=float(eng.cfg.length), capacity=eng.C, rate=float(eng.cfg.rate))
    acc = zeros_like_stats(eng, len(EDGES) - 1)
    cursor = torch.zeros((eng.E,), dtype=torch.int32, device=eng.device)
    calls = []

    def after_call():
        eng.trip_stats(edges=EDGES, cursor=cursor, accumulate=True, out=acc)
        calls.append(1)
    drive(eng, agent, after_call)
    assert eng.tick == TICKS and len(calls) == (TICKS // HOLD if agent else sum(len(s) for s in SPLITS))
    if path.startswith("pairs"):
        # the run ended on a two-tick pass: columns that start a row or two down are really walked
        assert eng.pair_ticks() > 0 and eng.head_rows().any()
    got = host(acc)
    n = eng.n_trips.cpu().numpy()
    want = devrng.trip_stats(eng.trip_times.cpu().numpy(), n, cap, None, EDGES)
    assert_fields(got, want[:5], TripStats._fields, (path, agent, cap, "the whole log"))
    assert np.array_equal(cursor.cpu().numpy(), n)
    s = oracle_driven(cap, agent)
    orc = devrng.trip_stats(s["trip_times"], s["n_trips"], cap, None, EDGES)
    assert_fields(got, orc[:5], TripStats._fields, (path, agent, cap, "the oracle's log"))
    assert (got[0][1:] > 0).all() and got[0][0] == 0 and ((got[3][1:] > 0).all() if cap == SMALL_CAP else not got[3].any())
    ages = check_ages(eng, (path, agent, cap))
    assert_fields(ages, devrng.car_ages(s["w"], s["leading"], s["lastcar"], eng.C, s["now"]), CarAges._fields, (path, agent, "oracle"))
    assert (ages[0][1:].sum(axis=1) > 20).all() and not ages[0][0].any() and ages[2].max() > 20


# ---- 4. read-only -------------------------------------------------------------------------------------------------------------
def same_snapshot(a, b):
    (A, _), (B, _) = a, b
    for k in A:
        if isinstance(A[k], np.ndarray):
            assert A[k].tobytes() == B[k].tobytes(), k
        else:
            assert A[k] is B[k] or A[k] == B[k], k


@pytest.mark.parametrize("path", ["pairs_tail", "pertick", "ring"])
def test_the_calls_write_nothing(path):
    eng = make(path, E_DRIVEN, "validate", **GRID)
    drive(eng, False)
    before = snapshot(eng)
    hb = eng.head_rows().copy()
    tick = C.c_int32()
    eng.car_ages()
    eng.car_ages(accumulate=True)
    eng.trip_stats(edges=EDGES)
    eng.trip_stats(cursor=torch.zeros((eng.E,), dtype=torch.int32, device=eng.device), accumulate=True)
    same_snapshot(before, snapshot(eng))
    assert np.array_equal(hb, eng.head_rows())
    nat.check(nat.lib().tfx_get_tick(eng.h, C.byref(tick)))
    assert tick.value == TICKS


SEQUENCE = [("step", 1), ("step", 4), ("agent", 6), ("agent", 6), ("step", 4), ("step", 3), ("agent", 6), ("step", 2), ("step", 4),
            ("agent", 5), ("agent", 6), ("step", 7), ("step", 4), ("step", 1), ("agent", 6)]      # (repeats replay captured graphs)


@pytest.mark.parametrize("path", ["pairs_tail", "pairs_split", "pertick", "ring"])
def test_twin_that_never_asks(path):
    """An engine asked for ages and trip statistics between every call of a mixed step / agent_step sequence (the agent
    steps replay their captured graph) stays bit-identical to one that never is."""
    E = E_DRIVEN
    eng, ref = make(path, E, "validate", **GRID), make(path, E, "validate", **GRID)
    rng = np.random.RandomState(31)
    for e_ in (eng, ref):
        e_.reset(np.zeros((E, eng.I), np.int32))
    cursor = torch.zeros((E,), dtype=torch.int32, device=eng.device)
    for kind, n in SEQUENCE:
        act = rng.randint(2, size=(E, eng.I)).astype(np.int32)
        cnt = ((rng.rand(n, E, eng.n_entry) < 0.15) * rng.randint(1, 3, size=(n, E, eng.n_entry))).astype(np.int32)
        eng.car_ages()
        eng.trip_stats(edges=EDGES, cursor=cursor, accumulate=True)
        for e_ in (eng, ref):
            e_.set_actions(act)
            e_.set_spawns(counts=cnt, per_tick=True)
            (e_.agent_step if kind == "agent" else e_.step)(n)
        sa, sb = snapshot(eng), snapshot(ref)
        for k in range(E):
            assert_env_equal(sa, k, sb, k, (path, kind, n))
        assert np.array_equal(eng.head_rows(), ref.head_rows())
    got = check_ages(eng, path)
    assert got[0].any() and eng.n_trips.cpu().numpy().any()


# ---- 5. clocks ------------------------------------------------------------------------------------------------------------------
def test_ages_follow_the_handles_own_clock():
    """snapshot() and restore() go between two handles whose ticks differ: spawn ticks are rebased by the clone, `now` is
    each handle's own clock, so the clone's ages are its source's."""
    from gym_traffic.envs.vec_env import TrafficVecEnv
    E = 4
    venv = TrafficVecEnv(E, 2, 2, 60.0, capacity=14, spawn='periodic', spawn_period=3, validate=True, seed=2)
    venv.reset()
    for d in range(3):
        venv.agent_step(n_ticks=10, cycle_period=7)
    src = host(venv.engine.car_ages())
    assert src[0].any() and src[2].max() >= 20
    snap = venv.snapshot()
    assert snap.engine.tick == 0 and venv.engine.tick == 30
    assert_fields(host(snap.engine.car_ages()), src, CarAges._fields, "snapshot")
    check_ages(snap.engine, "snapshot, its own planes and clock")
    venv.agent_step(n_ticks=10, cycle_period=7)
    later = host(venv.engine.car_ages())
    assert not np.array_equal(later[1], src[1])
    venv.restore(snap)
    assert venv.engine.tick == 40
    assert_fields(host(venv.engine.car_ages()), src, CarAges._fields, "restore")
    check_ages(venv.engine, "restored, its own planes and clock")


# ---- 6. more items than wavefronts -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["transposed", "ring"])
@pytest.mark.parametrize("knob", ["TFX_GRID_CAP", "TFX_MEASURE_GRID"])
def test_stride_rounds(layout, knob):
    """9 envs of the 3x3 grid are 9 (env, tile) items and 9 logs.  One workgroup - four wavefronts - takes them in three
    rounds, the last one with a single wavefront at work; the results are those of the uncapped launch."""
    E, cap = 9, 64
    cfg = dict(m=3, n=3, length=120.0, capacity=14, rate=0.5, validate=True, trip_cap=cap)
    free = engine_with({"TFX_RESIDENT": "0"}, E, layout=layout, planes=3, **cfg)
    eng = engine_with({"TFX_RESIDENT": "0", knob: "1"}, E, layout=layout, planes=3, **cfg)
    assert eng.ages_launch() == (1, 4) and free.ages_launch() == (3, 12)
    rng = np.random.RandomState(9)
    x, v, ld, lc, count = random_rings(rng, E * eng.R, eng.C)
    w = rng.randint(0, 301, size=(E, eng.R, eng.C)).astype(np.float32)
    log = (rng.randint(1, 400, size=(E, cap)) / 2.0).astype(np.float32)
    n = rng.randint(1, 2 * cap, size=E).astype(np.int32)
    cur = rng.randint(0, cap, size=E).astype(np.int32)
    out = []
    for e_ in (eng, free):
        e_.reset(np.zeros((E, e_.I), np.int32))
        e_.set_tick(300)
        e_.load_state(x.reshape(E, -1, e_.C), v.reshape(E, -1, e_.C), ld.reshape(E, -1), lc.reshape(E, -1), w=w)
        e_.trip_times.copy_(torch.as_tensor(log).to(e_.device))
        e_.n_trips.copy_(torch.as_tensor(n).to(e_.device))
        cursor = torch.as_tensor(cur.copy()).to(e_.device)
        out.append(host(e_.car_ages()) + host(e_.trip_stats(edges=EDGES, cursor=cursor)) + host([cursor]))
    assert all(np.array_equal(a, b) for a, b in zip(*out))
    assert_fields(out[0][:3], ages_model(eng), CarAges._fields, (layout, knob))
    want = devrng.trip_stats(log, n, cap, cur, EDGES)
    assert_fields(out[0][3:8], want[:5], TripStats._fields, (layout, knob))
    assert np.array_equal(out[0][8], n) and out[0][0].any(axis=1).all() and out[0][3].any()


# ---- 7. errors -----------------------------------------------------------------------------------------------------------------------
def test_errors_are_codes_and_the_handle_stays_usable():
    lib = nat.lib()
    eng = make("pertick", 3, "validate", **GRID)
    drive(eng, False)
    st = eng._stream()
    word = torch.zeros((eng.E, eng.R), dtype=torch.int32, device=eng.device)
    a = nat.TfxAgeBuffers()
    a.n_cars = C.c_void_p(word.data_ptr())
    t = nat.TfxTripStatBuffers()
    t.count = C.c_void_p(word.data_ptr())
    th = nat.TfxTripStatBuffers()
    th.hist = C.c_void_p(word.data_ptr())
    good = (C.c_int32 * 3)(0, 10, 20)
    bad = (C.c_int32 * 3)(0, 20, 10)
    # before tfx_bind_buffers
    h = C.c_void_p()
    nat.check(lib.tfx_create(C.byref(eng.cfg), C.byref(h)))
    assert lib.tfx_car_ages(h, C.byref(a), 0, st) == -2 and b"tfx_bind_buffers" in lib.tfx_last_error()
    assert lib.tfx_trip_stats(h, None, 0, None, C.byref(t), 0, st) == -2 and b"tfx_bind_buffers" in lib.tfx_last_error()
    nat.check(lib.tfx_destroy(h))
    # a handle without the side plane; handles that keep no trip log
    plain = make("pertick", 3, "plain", **GRID)
    assert lib.tfx_car_ages(plain.h, C.byref(a), 0, st) == -2 and b"planes == 2" in lib.tfx_last_error()
    assert lib.tfx_trip_stats(plain.h, None, 0, None, C.byref(t), 0, st) == -2 and b"validate" in lib.tfx_last_error()
    with pytest.raises(nat.TfxError):
        plain.car_ages()
    side = engine_with(PATHS["pertick"], 3, planes=3, **GRID)          # the side plane, but no validate mode
    assert lib.tfx_trip_stats(side.h, None, 0, None, C.byref(t), 0, st) == -2 and b"validate" in lib.tfx_last_error()
    assert lib.tfx_car_ages(side.h, C.byref(a), 0, st) == 0
    torch.cuda.synchronize()
    assert not word.any()                                                # (no cars on that handle: zeros were written)
    for args, msg in (((C.byref(a), 2), b"flags"), ((C.byref(a), -1), b"flags"), ((C.byref(nat.TfxAgeBuffers()), 0), b"null"),
                      ((None, 0), b"out is null")):
        assert lib.tfx_car_ages(eng.h, *args, st) == -1, args
        assert msg in lib.tfx_last_error(), (args, lib.tfx_last_error())
    assert lib.tfx_car_ages(None, C.byref(a), 0, st) == -1 and b"null handle" in lib.tfx_last_error()
    for args, msg in (((None, 0, None, C.byref(t), 2), b"flags"), ((None, 0, None, C.byref(nat.TfxTripStatBuffers()), 0), b"null"),
                      ((None, 0, None, None, 0), b"out is null"), ((good, 33, None, C.byref(t), 0), b"n_bins"),
                      ((good, -1, None, C.byref(t), 0), b"n_bins"), ((good, 0, None, C.byref(th), 0), b"n_bins"),
                      ((None, 2, None, C.byref(th), 0), b"edges is null"), ((bad, 2, None, C.byref(th), 0), b"decrease")):
        assert lib.tfx_trip_stats(eng.h, *args, st) == -1, args
        assert msg in lib.tfx_last_error(), (args, lib.tfx_last_error())
    assert lib.tfx_trip_stats(None, None, 0, None, C.byref(t), 0, st) == -1 and b"null handle" in lib.tfx_last_error()
    torch.cuda.synchronize()
    assert not word.any()                                                # a refused call launches nothing
    assert lib.tfx_car_ages(eng.h, C.byref(a), 0, st) == 0
    assert np.array_equal(word.cpu().numpy(), eng.cars_on_roads_flat().cpu().numpy()) and word.any()
    assert lib.tfx_trip_stats(eng.h, good, 2, None, C.byref(th), 0, st) == 0     # equal and increasing edges are fine
    eng.step(3)
    check_ages(eng, "after the errors")


# ---- 8. TrafficVecEnv.travel_times -------------------------------------------------------------------------------------------------
DEMAND = dict(means=[[0.9, 0.3]], seg_ticks=15)
EDGES_S = [0.0, 15.0, 20.0, 30.0, 1e5]


def check_travel(venv, tv, finished, ticks, hist, lost):
    eng = venv.engine
    got = host(tv)
    f, fs, mean, mx, h, lo, u, us, old, incl = got
    assert f.dtype == np.int64 and u.dtype == np.int64 and fs.dtype == np.float64 and incl.dtype == np.float64
    assert np.array_equal(f, finished) and np.array_equal(fs, ticks / 2.0) and np.array_equal(h, hist) and np.array_equal(lo, lost)
    ages = ages_model(eng)
    assert np.array_equal(u, ages[0].sum(axis=1, dtype=np.int64)) and np.array_equal(u, eng.cars_on_roads_flat().cpu().numpy().sum(axis=1))
    assert np.array_equal(us, ages[1].sum(axis=1) / 2.0) and np.array_equal(old, ages[2].max(axis=1) / 2.0)
    # exact: every term is a multiple of 1/2 far below 2^53, one float64 division
    both = f + u
    assert np.array_equal(incl, np.where(both > 0, (fs + us) / np.maximum(both, 1), 0.0))
    assert np.array_equal(mean, np.where(f > 0, fs / np.maximum(f, 1), 0.0))
    return got


def test_vec_env_travel_times_autoreset():
    """Episodes of 4 decisions restarting on the device, a log of 3 entries: travel_times() once per decision against the
    logs read on the host just before each restart."""
    from gym_traffic.envs.vec_env import TrafficVecEnv
    E, cap, T = 5, 3, 15
    venv = TrafficVecEnv(E, 2, 2, 60.0, capacity=14, spawn='demand', demand=DEMAND, validate=True, autoreset=True, episode_len=4,
                         seed=11, trip_cap=cap)
    eng = venv.engine
    venv.reset()
    ed = [int(round(2 * t)) for t in EDGES_S]
    finished, ticks, lost = np.zeros(E, np.int64), np.zeros(E, np.int64), np.zeros(E, np.int64)
    hist = np.zeros((E, len(ed) - 1), np.int64)
    rng = np.random.RandomState(4)
    restarts = 0
    for d in range(14):
        act = torch.as_tensor(rng.randint(2, size=(E, eng.I)).astype(np.int32)).to(eng.device)
        _, _, adone = venv.agent_step(act, n_ticks=T)
        tv = venv.travel_times(edges_s=EDGES_S)
        ended = (adone.cpu().numpy() != 0) | (venv.truncated.cpu().numpy() != 0)
        last = d == 13
        n = eng.n_trips.cpu().numpy()
        for k in np.where(ended | last)[0]:                    # the log as the host route reads it, just before the restart
            t = np.round(2 * venv.trip_times(k)).astype(np.int64)
            finished[k] += len(t)
            ticks[k] += t.sum()
            lost[k] += max(int(n[k]), cap) - cap
            hist[k] += np.histogram(t, bins=ed)[0] if len(t) else 0
        restarts += int(ended.sum())
    assert restarts >= E and finished.all() and lost.any()
    got = check_travel(venv, tv, finished, ticks, hist, lost)
    assert got[6].all() and (got[9] > 0).all() and (got[9] != got[2]).any()


def test_vec_env_travel_times_reset_done():
    from gym_traffic.envs.vec_env import TrafficVecEnv
    E = 4
    venv = TrafficVecEnv(E, 2, 2, 60.0, capacity=14, spawn='demand', demand=DEMAND, validate=True, seed=5, trip_cap=64)
    eng = venv.engine
    venv.reset()
    finished, ticks = np.zeros(E, np.int64), np.zeros(E, np.int64)

    def bank(envs):
        for k in envs:
            t = np.round(2 * venv.trip_times(k)).astype(np.int64)
            finished[k] += len(t)
            ticks[k] += t.sum()
    rng = np.random.RandomState(6)
    for d in range(18):
        venv.agent_step(torch.as_tensor(rng.randint(2, size=(E, eng.I)).astype(np.int32)).to(eng.device), n_ticks=10)
        venv.travel_times()
        if d == 6:
            before = eng.n_trips.cpu().numpy().copy()
            bank([1, 3])
            venv.reset_done(torch.as_tensor(np.array([0, 1, 0, 1], np.uint8)).to(eng.device))
    n = eng.n_trips.cpu().numpy()
    assert (before[[1, 3]] > 0).all() and (n[[1, 3]] > before[[1, 3]]).all()   # the logs grew back past the old cursors
    bank(range(E))
    got = check_travel(venv, venv.travel_times(), finished, ticks, None, np.zeros(E, np.int64))
    assert (got[0] > 0).all()
    # clear=True: the figures of the call, then the running tensors start again
    again = venv.travel_times(clear=True)
    assert np.array_equal(again.finished.cpu().numpy(), finished) and np.array_equal(again.unfinished.cpu().numpy(), got[6])
    zero = host(venv.travel_times())
    assert not zero[0].any() and not zero[1].any() and not zero[3].any() and np.array_equal(zero[6], got[6])
    finished[:], ticks[:] = 0, 0
    venv.reset()                                                     # every log starts again; the running figures stay
    venv.agent_step(torch.zeros((E, eng.I), dtype=torch.int32, device=eng.device), n_ticks=10)
    bank(range(E))
    check_travel(venv, venv.travel_times(), finished, ticks, None, np.zeros(E, np.int64))
    plain = TrafficVecEnv(2, 2, 2, 60.0, capacity=14, spawn='periodic')
    with pytest.raises(RuntimeError):
        plain.travel_times()


def bank_logs(venv, envs, finished, ticks, base=None):
    """the host route: the log of each of `envs` as trip_times() copies it (from entry base[k] on; base[k] is then spent)"""
    for k in envs:
        t = np.round(2 * venv.trip_times(k)).astype(np.int64)
        if base is not None:
            t, base[k] = t[base[k]:], 0
        finished[k] += len(t)
        ticks[k] += t.sum()


def decide(venv, rng, T):
    eng = venv.engine
    act = torch.as_tensor(rng.randint(2, size=(eng.E, eng.I)).astype(np.int32)).to(eng.device)
    _, _, adone = venv.agent_step(act, n_ticks=T)
    return (adone.cpu().numpy() != 0) | (venv.truncated.cpu().numpy() != 0)


@pytest.mark.parametrize("snap_after", [3, 4])
def test_vec_env_travel_times_across_snapshot_and_restore(snap_after):
    """autoreset with episodes of 3 decisions.  A snapshot taken after decision 3 holds envs that are about to restart
    (their logs will be cleared), one taken after decision 4 holds envs one decision into their second episode.  The run
    goes on past a restart, is restored, and goes on again: from the restore on, the running figures are the logs the host
    reads just before each restart."""
    from gym_traffic.envs.vec_env import TrafficVecEnv
    E, T = 5, 20
    venv = TrafficVecEnv(E, 2, 2, 60.0, capacity=14, spawn='demand', demand=DEMAND, validate=True, autoreset=True, episode_len=3,
                         seed=21, trip_cap=64)
    venv.reset()
    rng = np.random.RandomState(8)
    for d in range(snap_after):
        ended = decide(venv, rng, T)
        venv.travel_times()
    assert snap_after != 3 or ended.any()                          # (the time limit: restarts are pending in the snapshot)
    pending = ended.copy()                                         # these envs restart when the next decision begins
    snap = venv.snapshot()
    index_then = venv.episode_index.cpu().numpy().copy()
    for d in range(4):                                             # past the next restart of every env
        decide(venv, rng, T)
        venv.travel_times()
    assert (venv.episode_index.cpu().numpy() > index_then).all()
    venv.travel_times(clear=True)                                  # what follows counts from the restore on
    venv.restore(snap)
    assert np.array_equal(venv.episode_index.cpu().numpy(), index_then)
    finished, ticks = np.zeros(E, np.int64), np.zeros(E, np.int64)
    # asked between the restore and the next decision: the restored logs are read here, and those of the envs that are
    # about to restart are then cleared although no decision of THIS env ended their episodes
    tv = venv.travel_times()
    bank_logs(venv, range(E), finished, ticks)
    base = np.where(pending, 0, venv.engine.n_trips.cpu().numpy()).astype(np.int64)
    assert np.array_equal(tv.finished.cpu().numpy(), finished) and (snap_after != 3 or finished.any())
    n_dec = 5
    for d in range(n_dec):
        # (decisions three times as long as before: a log that starts again outgrows the restored one's cursor within one
        # decision, which the rule of tfx_trip_stats cannot see by itself)
        ended = decide(venv, rng, 3 * T)
        tv = venv.travel_times()
        again = venv.travel_times()                                # a second call between two decisions adds nothing
        assert np.array_equal(again.finished.cpu().numpy(), tv.finished.cpu().numpy())
        bank_logs(venv, np.where(ended | (d == n_dec - 1))[0], finished, ticks, base)
        if d >= 1:                                                 # two decisions and more after the restore
            running = ended | (d == n_dec - 1)
            got = host(tv)
            assert np.array_equal(got[0][running], finished[running]) and np.array_equal(got[1][running], ticks[running] / 2.0), d
    assert finished.all() and (venv.episode_index.cpu().numpy() > index_then).all()
    check_travel(venv, tv, finished, ticks, None, np.zeros(E, np.int64))


def test_vec_env_travel_times_first_asked_late():
    """The first travel_times() call comes after a decision that ended every episode: nothing of the next logs is skipped."""
    from gym_traffic.envs.vec_env import TrafficVecEnv
    E, T = 4, 30
    venv = TrafficVecEnv(E, 2, 2, 60.0, capacity=14, spawn='demand', demand=DEMAND, validate=True, autoreset=True, episode_len=2,
                         seed=3, trip_cap=64)
    venv.reset()
    rng = np.random.RandomState(2)
    finished, ticks = np.zeros(E, np.int64), np.zeros(E, np.int64)
    decide(venv, rng, T)
    for d in range(1, 8):
        ended = decide(venv, rng, T)
        tv = venv.travel_times()
        bank_logs(venv, np.where(ended | (d == 7))[0], finished, ticks)
    assert finished.all()
    check_travel(venv, tv, finished, ticks, None, np.zeros(E, np.int64))


def test_vec_env_travel_times_after_a_branch_in_place():
    """clone_envs() in place: the clone's running figures go on from the end of the log it received."""
    from gym_traffic.envs.vec_env import TrafficVecEnv
    E, T = 4, 10
    venv = TrafficVecEnv(E, 2, 2, 60.0, capacity=14, spawn='demand', demand=DEMAND, validate=True, seed=5, trip_cap=64)
    eng = venv.engine
    venv.reset()
    rng = np.random.RandomState(6)
    finished, ticks = np.zeros(E, np.int64), np.zeros(E, np.int64)
    for d in range(16):
        venv.agent_step(torch.as_tensor(rng.randint(2, size=(E, eng.I)).astype(np.int32)).to(eng.device), n_ticks=T)
        venv.travel_times()
        if d == 7:
            bank_logs(venv, [1, 3], finished, ticks)               # what envs 1 and 3 finished themselves
            venv.clone_envs(np.array([-1, 0, -1, 2], np.int32))
            at = eng.n_trips.cpu().numpy().copy()
            assert at[1] == at[0] > 0 and at[3] == at[2] > 0
    n = eng.n_trips.cpu().numpy()
    assert (n[[1, 3]] > at[[1, 3]]).all()
    bank_logs(venv, [0, 2], finished, ticks)
    for k in (1, 3):                                               # ... and what they finished after the branch
        t = np.round(2 * venv.trip_times(k)[at[k]:]).astype(np.int64)
        finished[k] += len(t)
        ticks[k] += t.sum()
    check_travel(venv, venv.travel_times(), finished, ticks, None, np.zeros(E, np.int64))


def test_travel_demo_runs():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "travel_demo.py"), "--envs", "6", "--m", "2", "--n", "2",
                          "--length", "60", "--capacity", "14", "--decisions", "8", "--ticks", "10"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    print(out.stdout)
    rows = {ln.split("  ")[0].strip(): ln.split() for ln in out.stdout.splitlines()}
    assert "fixed cycle" in rows and "greedy (on device)" in rows
    for key in ("fixed cycle", "greedy (on device)"):
        mean, incl = float(rows[key][-2]), float(rows[key][-1])
        assert np.isfinite(mean) and np.isfinite(incl) and mean > 0 and incl > 0
