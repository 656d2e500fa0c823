"""Road cells on the device (tfx_road_cells, include/tfx.h), the parts that need no GPU: the entry point and its argument
checks, the binding, the definition as a NumPy function (devrng.road_cells - what tests/test_gpu_cells.py holds the
device to) on hand-written and random rings and against devrng.road_measures, and the driven scenario of
tests/test_measures_host.py binned on the CPU oracle, with the conditions that keep the GPU comparison from passing on a
trivial field."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from test_measures_host import GRID, f32sum, oracle_driven, random_rings, ring

HEADER = os.path.join(ROOT, "include", "tfx.h")
LIB = os.path.join(ROOT, "traffic-env_amd", "lib", "libtfx_hip.so")
INF = float("inf")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import subprocess
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "traffic-env_amd", "csrc")])
    return C.CDLL(LIB)


# ---- ABI -----------------------------------------------------------------------------------------------------------------
def test_header_declares_the_call_the_struct_the_flag_and_the_bound():
    from gym_traffic import _native
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"int\s+tfx_road_cells\s*\(\s*tfx_handle\s+h\s*,\s*const\s+float\s*\*\s*edges\s*,\s*int32_t\s+n_cells\s*,\s*"
                     r"const\s+tfx_cell_buffers\s*\*\s*out\s*,\s*int32_t\s+flags\s*,\s*void\s*\*\s*stream\s*\)\s*;", src)
    assert re.search(r"int\s+tfx_cells_launch\s*\(\s*tfx_handle\s+h\s*,\s*int32_t\s+n_cells\s*,\s*int32_t\s*\*\s*grid\s*,\s*"
                     r"int32_t\s*\*\s*waves\s*\)\s*;", src)
    body = re.search(r"typedef struct tfx_cell_buffers \{(.*?)\} tfx_cell_buffers;", src, re.S).group(1)
    decls = [re.sub(r"\s+", " ", d.strip()) for d in body.split(";") if d.strip()]
    assert decls == ["int32_t *n_cars", "float *speed_sum"]
    assert re.search(r"enum\s*\{\s*TFX_CELLS_ACCUMULATE\s*=\s*1\s*\}", src)
    assert re.search(r"#define\s+TFX_MAX_CELLS\s+32\b", src)
    assert re.search(r"#define\s+TFX_ABI_VERSION\s+13\b", src)
    assert _native.ABI_VERSION == 13 and _native.CELLS_ACCUMULATE == 1 and _native.MAX_CELLS == 32
    assert len(_native._PROTOS["tfx_road_cells"][1]) == 6 and len(_native._PROTOS["tfx_cells_launch"][1]) == 4


def test_ctypes_struct_has_the_c_layout():
    from gym_traffic import _native
    S = _native.TfxCellBuffers
    assert [f[0] for f in S._fields_] == ["n_cars", "speed_sum"]
    p = C.sizeof(C.c_void_p)
    assert C.sizeof(S) == 2 * p
    assert [getattr(S, f[0]).offset for f in S._fields_] == [0, p]


def test_calls_are_exported_and_argument_errors_are_codes(lib):
    """Every TFX_EINVAL of include/tfx.h with its message.  The arguments are checked before the handle, so each cause is
    reachable here, where no device - hence no handle - exists; with good arguments the NULL handle is the cause.
    TFX_ESTATE needs a handle, and tfx_create needs a device to make one: tests/test_gpu_cells.py asserts that code (and
    these again) on a live handle."""
    from gym_traffic import _native
    assert lib.tfx_abi_version() == 13
    fn = lib.tfx_road_cells
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.c_int32, C.POINTER(_native.TfxCellBuffers), C.c_int32, C.c_void_p]
    geo = lib.tfx_cells_launch
    geo.restype = C.c_int
    geo.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    lib.tfx_last_error.restype = C.c_char_p
    word = (C.c_int32 * 4)()
    b = _native.TfxCellBuffers()
    b.n_cars = C.cast(word, C.c_void_p)

    def edges(*vals):
        return (C.c_float * len(vals))(*vals)

    good = edges(-INF, 40.0, 80.0, INF)
    none = _native.TfxCellBuffers()
    nan = float("nan")
    for args, msg in BAD_ARGS(good, edges, b, none, nan):
        assert fn(None, *args, None) == -1, msg
        assert msg in lib.tfx_last_error(), (msg, lib.tfx_last_error())
    for flags in (0, 1):
        assert fn(None, good, 3, C.byref(b), flags, None) == -1
        assert b"null handle" in lib.tfx_last_error()
    assert fn(None, edges(-INF, INF), 1, C.byref(b), 0, None) == -1 and b"null handle" in lib.tfx_last_error()
    assert fn(None, np.arange(33, dtype=np.float32).ctypes.data_as(C.POINTER(C.c_float)), 32, C.byref(b), 0, None) == -1
    assert b"null handle" in lib.tfx_last_error()
    assert geo(None, 3, None, None) == -1
    assert b"null handle" in lib.tfx_last_error()

    assert list(word) == [0, 0, 0, 0]


def BAD_ARGS(good, edges, b, none, nan):
    """(edges, n_cells, out, flags) and the words its refusal must contain - shared with tests/test_gpu_cells.py"""
    return (((None, 3, C.byref(b), 0), b"edges is null"),
            ((good, 3, None, 0), b"out is null"),
            ((good, 3, C.byref(none), 0), b"every output pointer is null"),
            ((good, 0, C.byref(b), 0), b"n_cells 0"),
            ((good, -1, C.byref(b), 0), b"n_cells -1"),
            ((good, 33, C.byref(b), 0), b"n_cells 33"),
            ((edges(-INF, nan, 80.0, INF), 3, C.byref(b), 0), b"edge 1 is NaN"),
            ((edges(nan, 40.0, 80.0, INF), 3, C.byref(b), 0), b"edge 0 is NaN"),
            ((edges(0.0, 40.0, 80.0, nan), 3, C.byref(b), 0), b"edge 3 is NaN"),
            ((edges(0.0, 40.0, 40.0, INF), 3, C.byref(b), 0), b"not strictly ascending at 1"),
            ((edges(0.0, 40.0, 30.0, INF), 3, C.byref(b), 0), b"not strictly ascending at 1"),
            ((edges(INF, INF), 1, C.byref(b), 0), b"not strictly ascending at 0"),
            ((edges(-INF, -INF, 0.0), 2, C.byref(b), 0), b"not strictly ascending at 0"),
            ((good, 3, C.byref(b), 2), b"flags"),
            ((good, 3, C.byref(b), -1), b"flags"))


# ---- the NumPy model on hand-written rings ---------------------------------------------------------------------------------
def cells_of(C_, leading, cars, edges):
    from gym_traffic.devrng import road_cells
    x, v, ld, lc = ring(C_, leading, cars)
    n, s = road_cells(x, v, ld, lc, C_, edges)
    B = len(edges) - 1
    assert n.dtype == np.int32 and s.dtype == np.float32 and n.shape == (1, B) and s.shape == (1, B)
    return n[0].tolist(), s[0]


def sums(*cells):
    return np.array([f32sum(c) for c in cells], np.float32)


def test_model_known_answers():
    from gym_traffic.devrng import cell_edges, road_cells
    e3 = [0.0, 40.0, 80.0, 120.0]
    # empty roads, wherever the fake leader sits: every cell 0
    for ld in (1, 7):
        n, s = cells_of(8, ld, [], e3)
        assert n == [0, 0, 0] and s.tobytes() == sums([], [], []).tobytes()
    # a car exactly on an edge goes to the upper cell; one just below it to the lower
    below = np.nextafter(np.float32(80.0), np.float32(0))
    n, s = cells_of(8, 1, [(80.0, 1.0), (below, 2.0), (40.0, 4.0), (0.0, 8.0)], e3)
    assert n == [1, 2, 1] and s.tobytes() == sums([8.0], [2.0, 4.0], [1.0]).tobytes()
    # out of range: below edges[0], at or past edges[B]; a NaN x is in no cell
    n, s = cells_of(8, 1, [(120.0, 1.0), (119.0, 2.0), (float("nan"), 4.0), (-1.0, 8.0), (np.nextafter(np.float32(120), np.float32(0)), 16.0)], e3)
    assert n == [0, 0, 2] and s.tobytes() == sums([], [], [2.0, 16.0]).tobytes()
    # infinite outer edges take every car but the NaN one - cell_edges makes such edges
    ce = cell_edges(120.0, 3)
    assert ce.dtype == np.float32 and ce[0] == -INF and ce[3] == INF and ce[1] == np.float32(40.0) and ce[2] == np.float32(80.0)
    n, s = cells_of(8, 1, [(500.0, 1.0), (119.0, 2.0), (float("nan"), 4.0), (-1.0, 8.0)], ce)
    assert n == [1, 0, 2] and s.tobytes() == sums([8.0], [], [1.0, 2.0]).tobytes()
    assert cell_edges(100.0, 1).tolist() == [-INF, INF]
    e7 = cell_edges(100.0, 7)
    assert all(e7[b] == np.float32(100.0 * b / 7) for b in range(1, 7)) and (e7[:-1] < e7[1:]).all()
    # a wrapped ring: leading = 6 of C = 8, cars in slots 7, 1, 2
    n, s = cells_of(8, 6, [(90.0, 0.5), (85.0, 0.25), (30.0, 3.0)], e3)
    assert n == [1, 0, 2] and s.tobytes() == sums([3.0], [], [0.5, 0.25]).tobytes()
    # a full ring: C - 2 = 6 cars at x = 100, 85, 70, 55, 40 (on an edge), 25
    n, s = cells_of(8, 3, [(100.0 - 15 * k, 1.0 + k) for k in range(6)], e3)
    assert n == [1, 3, 2] and s.tobytes() == sums([6.0], [3.0, 4.0, 5.0], [1.0, 2.0]).tobytes()
    # unsorted x: a cell's sum is taken in car order, across the visits of other cells in between
    cars = [(10.0, 1e8), (90.0, 3.0), (20.0, 1.0), (95.0, 5.0), (30.0, -1e8), (50.0, 7.0)]
    n, s = cells_of(8, 1, cars, e3)
    assert n == [3, 1, 2] and s.tobytes() == sums([1e8, 1.0, -1e8], [7.0], [3.0, 5.0]).tobytes() and s[0] == 0.0
    cars = [(10.0, 1e8), (90.0, 3.0), (30.0, -1e8), (95.0, 5.0), (20.0, 1.0)]
    assert cells_of(8, 1, cars, e3)[1][0] == np.float32(1.0)
    # one cell, 32 cells, non-uniform edges
    assert cells_of(8, 1, [(5.0, 1.0), (3.0, 2.0)], [4.0, INF])[0] == [1]
    n, s = cells_of(8, 1, [(31.0, 1.0), (30.5, 2.0), (0.0, 4.0)], np.arange(33, dtype=np.float32))
    assert n == [1] + [0] * 29 + [1, 1] and s[31] == 1.0 and s[30] == 2.0 and s[0] == 4.0
    n, s = cells_of(8, 1, [(7.0, 1.0), (1.5, 2.0), (1.0, 4.0)], [1.0, 1.5, 100.0])
    assert n == [1, 2]
    # edges are checked
    x, v, ld, lc = ring(8, 1, [(1.0, 1.0)])
    for bad in ([1.0], [1.0, 1.0], [2.0, 1.0], [0.0, float("nan"), 2.0]):
        with pytest.raises(ValueError):
            road_cells(x, v, ld, lc, 8, bad)


def test_model_on_random_rings():
    from gym_traffic.devrng import cell_edges, road_cells, road_measures
    from oracle.oracle import ring_order
    rng = np.random.RandomState(18)
    for C_ in (6, 14, 66):
        x, v, ld, lc, n = random_rings(rng, 400, C_)
        assert (n == 0).any() and (n == C_ - 2).any() and (ld > lc).any()
        for B in (1, 5, 8, 32):
            edges = cell_edges(120.0, B)
            cars, total = road_cells(x, v, ld, lc, C_, edges)
            assert cars.shape == (400, B) and np.array_equal(cars.sum(axis=1), n)      # the cells sum to the ring count
            # the definition, road by road in plain Python
            for e in range(0, 400, 7):
                slots = ring_order(int(ld[e]), int(lc[e]), C_)
                cell = [sum(1 for k in range(1, B) if x[e, s] >= edges[k]) for s in slots]
                for b in range(B):
                    mine = [s for s, c in zip(slots, cell) if c == b]
                    assert cars[e, b] == len(mine)
                    assert total[e, b].tobytes() == f32sum([v[e, s] for s in mine]).tobytes()
        # one cell [x_from, inf) is road_measures' n_cars / speed_sum, bit for bit
        for x_from in (-INF, 60.0, float(x[3, 2])):
            cars, total = road_cells(x, v, ld, lc, C_, [x_from, INF])
            want = road_measures(x, v, ld, lc, C_, 0.1, x_from)
            assert np.array_equal(cars[:, 0], want[0]) and total[:, 0].tobytes() == want[3].tobytes()
        # leading dimensions pass through
        edges = cell_edges(120.0, 5)
        a = road_cells(x.reshape(4, 100, C_), v.reshape(4, 100, C_), ld.reshape(4, 100), lc.reshape(4, 100), C_, edges)
        b_ = road_cells(x, v, ld, lc, C_, edges)
        assert all(p.shape == (4, 100, 5) and np.array_equal(p.reshape(400, 5), q) for p, q in zip(a, b_))


# ---- the GPU test's driven scenario on the CPU oracle ----------------------------------------------------------------------
def test_driven_scenario_is_not_vacuous():
    """Conditions on the INPUTS of tests/test_gpu_cells.py (the oracle alone, no device): binned into eight cells, some
    road has cars in three or more different cells and some cell holds two or more cars."""
    from gym_traffic.devrng import cell_edges, road_cells
    s = oracle_driven()
    C_ = GRID["capacity"]
    cars, total = road_cells(s["x"], s["v"], s["leading"], s["lastcar"], C_, cell_edges(GRID["length"], 8))
    assert np.array_equal(cars.sum(axis=-1), s["cars"])
    assert ((cars > 0).sum(axis=-1) >= 3).any()
    assert (cars >= 2).any()
    assert (total > 0).any() and not cars[0].any()
    print("driven scenario in 8 cells: %d cars, %d occupied cells, fullest cell %d, most cells occupied on one road %d"
          % (cars.sum(), (cars > 0).sum(), cars.max(), (cars > 0).sum(axis=-1).max()))
