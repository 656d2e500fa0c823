"""Road measures on the device (tfx_road_measures, include/tfx.h), the parts that need no GPU: the entry point and its
argument checks, the binding, the definition as a NumPy function (devrng.road_measures - what tests/test_gpu_measures.py
holds the device to) on hand-written and random rings, and the driven scenario of the GPU test run on the CPU oracle,
with the conditions that keep the GPU comparison from passing on an all-zero field."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "tfx.h")
LIB = os.path.join(ROOT, "traffic-env_amd", "lib", "libtfx_hip.so")

# ---- the driven scenario, shared with tests/test_gpu_measures.py ---------------------------------------------------------
GRID = dict(m=3, n=3, length=120.0, capacity=14, rate=0.5)
E_DRIVEN = 6
HALT, X_FROM = 0.1, GRID["length"] - 50.0
# ticks per tfx_step call, every call under one held action: 42 ticks (a car needs some 22 to reach the end of its first
# road), the last calls two-tick passes where those run
CALLS = [1, 1, 1, 4, 5, 3, 2, 7, 6, 6, 6]


def scenario(I, n_entry, E=E_DRIVEN, seed=2024, density=0.12):
    """[(held action int32 [E, I], arrival counts int32 [n, E, n_entry])] for CALLS - a pure function of its arguments.
    Env 0 receives no cars at all (empty roads), the others one or two per entry road in `density` of the ticks."""
    rng = np.random.RandomState(seed)
    out = []
    for n in CALLS:
        act = rng.randint(2, size=(E, I)).astype(np.int32)
        cnt = (rng.rand(n, E, n_entry) < density).astype(np.int32) * rng.randint(1, 3, size=(n, E, n_entry))
        cnt[:, 0] = 0
        out.append((act, cnt.astype(np.int32)))
    return out


def roads_of(cnt_row, entrypoints):
    """one tick's counts [E, n_entry] -> per env the list of entry roads, a road once per car"""
    return [[int(entrypoints[j]) for j in range(len(entrypoints)) for _ in range(int(row[j]))] for row in cnt_row]


_driven = {}


def oracle_driven():
    """The scenario on the CPU oracle: dict(x, v [E, R, C], leading, lastcar, cars, handed_over [E, R]) after the last call."""
    if not _driven:
        from gym_traffic.envs.roadgraph import GridRoad
        from oracle.oracle import OracleEnv
        g = GridRoad(GRID["m"], GRID["n"], GRID["length"])
        entry = g.generate_entrypoints(0)
        orc = OracleEnv(GRID["m"], GRID["n"], GRID["length"], GRID["capacity"], g.dest, g.phases, g.nexts,
                        n_envs=E_DRIVEN, rate=GRID["rate"])
        orc.reset(np.zeros((E_DRIVEN, orc.I), np.int32))
        for act, cnt in scenario(orc.I, len(entry)):
            for t in range(cnt.shape[0]):
                before = orc.leading.copy()
                orc.step(act, roads_of(cnt[t], entry))
        _driven.update(handed_over=orc.leading != before,      # roads whose head left them in the last tick
                       x=orc.x.copy(), v=orc.v.copy(), leading=orc.leading.copy(), lastcar=orc.lastcar.copy(),
                       cars=orc.cars_on_roads_flat())
    return _driven


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import subprocess
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "traffic-env_amd", "csrc")])
    return C.CDLL(LIB)


# ---- ABI -----------------------------------------------------------------------------------------------------------------
def test_header_declares_the_call_the_struct_and_the_flag():
    from gym_traffic import _native
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"int\s+tfx_road_measures\s*\(\s*tfx_handle\s+h\s*,\s*float\s+halt_speed\s*,\s*float\s+x_from\s*,\s*"
                     r"const\s+tfx_measure_buffers\s*\*\s*out\s*,\s*int32_t\s+flags\s*,\s*void\s*\*\s*stream\s*\)\s*;", src)
    body = re.search(r"typedef struct tfx_measure_buffers \{(.*?)\} tfx_measure_buffers;", src, re.S).group(1)
    decls = [re.sub(r"\s+", " ", d.strip()) for d in body.split(";") if d.strip()]
    assert decls == ["int32_t *n_cars", "int32_t *n_halted", "int32_t *queue", "float *speed_sum"]
    assert re.search(r"enum\s*\{\s*TFX_MEASURE_ACCUMULATE\s*=\s*1\s*\}", src)
    assert re.search(r"#define\s+TFX_ABI_VERSION\s+13\b", src)
    assert _native.ABI_VERSION == 13 and _native.MEASURE_ACCUMULATE == 1
    assert len(_native._PROTOS["tfx_road_measures"][1]) == 6


def test_ctypes_struct_has_the_c_layout():
    from gym_traffic import _native
    S = _native.TfxMeasureBuffers
    assert [f[0] for f in S._fields_] == ["n_cars", "n_halted", "queue", "speed_sum"]
    p = C.sizeof(C.c_void_p)
    assert C.sizeof(S) == 4 * p
    assert [getattr(S, f[0]).offset for f in S._fields_] == [0, p, 2 * p, 3 * p]


def test_call_is_exported_and_argument_errors_are_codes(lib):
    from gym_traffic import _native
    assert lib.tfx_abi_version() == 13
    fn = lib.tfx_road_measures
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_float, C.c_float, C.POINTER(_native.TfxMeasureBuffers), C.c_int32, C.c_void_p]
    lib.tfx_last_error.restype = C.c_char_p
    word = (C.c_int32 * 4)()
    b = _native.TfxMeasureBuffers()
    b.n_cars = C.cast(word, C.c_void_p)
    assert fn(None, 0.1, 0.0, C.byref(b), 0, None) == -1
    assert b"null handle" in lib.tfx_last_error()
    assert fn(None, 0.1, 0.0, None, 0, None) == -1
    assert b"out is null" in lib.tfx_last_error()
    assert list(word) == [0, 0, 0, 0]


# ---- the NumPy model on hand-written rings ---------------------------------------------------------------------------------
def ring(C, leading, cars):
    """one road: cars = [(x, v)] from the head on -> x, v [1, C], leading, lastcar [1]"""
    x, v = np.full((1, C), 777.0, np.float32), np.full((1, C), 9.0, np.float32)       # junk in the dead slots
    s = leading
    for cx, cv in cars:
        s = s + 1 if s + 1 < C else 1
        x[0, s], v[0, s] = cx, cv
    return x, v, np.array([leading]), np.array([s])


def measures_of(C, leading, cars, halt=0.5, x_from=None):
    from gym_traffic.devrng import road_measures
    x, v, ld, lc = ring(C, leading, cars)
    n, h, q, s = road_measures(x, v, ld, lc, C, halt, x_from)
    assert n.dtype == np.int32 and h.dtype == np.int32 and q.dtype == np.int32 and s.dtype == np.float32
    return int(n[0]), int(h[0]), int(q[0]), s[0]


def f32sum(vals):
    s = np.float32(0)
    for val in vals:
        s = np.float32(s + np.float32(val))
    return s


def test_model_known_answers():
    # an empty road (leading == lastcar), wherever its fake leader sits
    assert measures_of(8, 1, []) == (0, 0, 0, 0.0)
    assert measures_of(8, 7, []) == (0, 0, 0, 0.0)
    # a wrapped ring: leading = 6 of C = 8, cars in slots 7, 1, 2
    cars = [(90.0, 0.0), (80.0, 0.25), (70.0, 3.0)]
    assert measures_of(8, 6, cars) == (3, 2, 2, f32sum([0.0, 0.25, 3.0]))
    # a full ring: C - 2 = 6 cars, the most a road holds (one more and lastcar would meet leading, which means "empty")
    cars = [(100.0 - 5 * k, 0.0) for k in range(6)]
    assert measures_of(8, 3, cars) == (6, 6, 6, 0.0)
    # v exactly equal to halt_speed is not halted
    assert measures_of(8, 1, [(50.0, 0.5), (40.0, np.nextafter(np.float32(0.5), np.float32(0)))]) == \
        (2, 1, 0, f32sum([0.5, np.nextafter(np.float32(0.5), np.float32(0))]))
    # a moving car in front of halted ones: no queue, but halted cars
    assert measures_of(8, 2, [(110.0, 4.0), (60.0, 0.0), (55.0, 0.0)])[:3] == (3, 2, 0)
    # x_from cuts the tail off: the queue ends at the first car out of range, although that car stands too
    cars = [(100.0, 0.0), (95.0, 0.0), (69.9, 0.0), (60.0, 0.0)]
    assert measures_of(8, 5, cars, x_from=70.0) == (2, 2, 2, 0.0)
    assert measures_of(8, 5, cars, x_from=None)[:3] == (4, 4, 4)
    # ... and a car back in range behind one out of range counts as a car, not as part of the queue
    cars = [(100.0, 0.0), (10.0, 0.0), (90.0, 0.0)]
    assert measures_of(8, 1, cars, x_from=70.0)[:3] == (2, 2, 1)
    # x == x_from is in range; +inf leaves nothing in range
    assert measures_of(8, 1, [(70.0, 1.0)], x_from=70.0)[:3] == (1, 0, 0)
    assert measures_of(8, 1, [(70.0, 0.0), (60.0, 0.0)], x_from=np.inf) == (0, 0, 0, 0.0)
    # the sum is the sequential float32 one, not the exact one: 1e8 + 1 - 1e8 in car order
    assert measures_of(8, 1, [(9.0, 1e8), (8.0, 1.0), (7.0, -1e8)], halt=-1.0)[3] == np.float32(0.0)
    assert measures_of(8, 1, [(9.0, 1e8), (8.0, -1e8), (7.0, 1.0)], halt=-1.0)[3] == np.float32(1.0)


def random_rings(rng, n_roads, C):
    """leading / lastcar with empty, wrapped and full (C - 2 cars) roads among them; x, v with exact ties"""
    ld = rng.randint(1, C, size=n_roads)
    n = rng.randint(0, C - 1, size=n_roads)
    n[rng.rand(n_roads) < 0.15] = 0
    n[rng.rand(n_roads) < 0.15] = C - 2
    lc = ld + n
    lc = np.where(lc > C - 1, lc - (C - 1), lc)
    x = (rng.rand(n_roads, C) * 120).astype(np.float32)
    v = (rng.rand(n_roads, C) * 2).astype(np.float32)
    v[rng.rand(n_roads, C) < 0.2] = np.float32(0.1)        # exactly halt_speed
    v[rng.rand(n_roads, C) < 0.3] = 0.0
    return x, v, ld.astype(np.int32), lc.astype(np.int32), n


def test_model_invariants_on_random_rings():
    from gym_traffic.devrng import road_measures
    from oracle.oracle import ring_order
    rng = np.random.RandomState(8)
    for C in (6, 14, 66):
        x, v, ld, lc, n = random_rings(rng, 400, C)
        assert (n == 0).any() and (n == C - 2).any() and (ld > lc).any()
        for x_from in (None, 60.0):
            cars, halted, queue, total = road_measures(x, v, ld, lc, C, 0.1, x_from)
            assert (0 <= queue).all() and (queue <= halted).all() and (halted <= cars).all() and (cars <= n).all()
            if x_from is None:
                assert np.array_equal(cars, n)
            # the definition, road by road in plain Python
            for e in range(0, 400, 7):
                slots = ring_order(int(ld[e]), int(lc[e]), C)
                inr = [s for s in slots if x_from is None or x[e, s] >= np.float32(x_from)]
                assert cars[e] == len(inr) and halted[e] == sum(1 for s in inr if v[e, s] < np.float32(0.1))
                q = 0
                for s in slots:
                    if s in inr and v[e, s] < np.float32(0.1):
                        q += 1
                    else:
                        break
                assert queue[e] == q
                assert total[e].tobytes() == f32sum([v[e, s] for s in inr]).tobytes()
        # leading dimensions pass through
        a = road_measures(x.reshape(4, 100, C), v.reshape(4, 100, C), ld.reshape(4, 100), lc.reshape(4, 100), C, 0.1, 60.0)
        b = road_measures(x, v, ld, lc, C, 0.1, 60.0)
        assert all(p.shape == (4, 100) and np.array_equal(p.ravel(), q_) for p, q_ in zip(a, b))


# ---- the GPU test's driven scenario on the CPU oracle ----------------------------------------------------------------------
def test_driven_scenario_is_not_vacuous():
    """Conditions on the INPUTS of tests/test_gpu_measures.py (the oracle alone, no device): the field the GPU is
    compared on has standing queues, halted cars behind moving ones, cars out of range, and empty roads."""
    from gym_traffic.devrng import road_measures
    s = oracle_driven()
    C = GRID["capacity"]
    cars, halted, queue, total = road_measures(s["x"], s["v"], s["leading"], s["lastcar"], C, HALT, X_FROM)
    every = road_measures(s["x"], s["v"], s["leading"], s["lastcar"], C, HALT, None)[0]
    assert np.array_equal(every, s["cars"])
    assert sum(CALLS) % 2 == 0 and CALLS[-1] % 2 == 0
    assert (queue >= 2).any()
    assert (halted > queue).any()
    assert (cars < s["cars"]).any()
    assert (s["cars"] == 0).any() and (s["cars"][1:] > 0).any()
    assert (total > 0).any()
    # where two-tick passes run, a road whose head left it in the run's last tick starts a row down its column
    assert s["handed_over"].any()
    print("driven scenario: %d cars, %d in range, %d halted, longest queue %d, %d roads with halted cars outside the queue"
          % (s["cars"].sum(), cars.sum(), halted.sum(), queue.max(), (halted > queue).sum()))
