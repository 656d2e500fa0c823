"""Top-view frames on the device (tfx_frames, include/tfx.h), the parts that need no GPU: the entry points and their
argument checks, the binding, the roads' geometry (devrng.frame_geometry), the definition as a NumPy function
(devrng.frames - what tests/test_gpu_frames.py holds the device to) on hand-computed pictures and, on random rings,
against cars_on_roads, and the driven scenario of tests/test_measures_host.py drawn on the CPU oracle, with the conditions
that keep the GPU comparison from passing on a trivial picture."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from test_measures_host import E_DRIVEN, GRID, oracle_driven, random_rings, roads_of, scenario

HEADER = os.path.join(ROOT, "include", "tfx.h")
LIB = os.path.join(ROOT, "traffic-env_amd", "lib", "libtfx_hip.so")
WHITE, GREEN, YELLOW, RED, BLUE = (255,) * 4, (0, 255, 0, 255), (255, 255, 0, 255), (255, 0, 0, 255), (0, 0, 255, 255)
PX_DRIVEN = 32


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import subprocess
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "traffic-env_amd", "csrc")])
    return C.CDLL(LIB)


# ---- ABI -----------------------------------------------------------------------------------------------------------------
def test_header_declares_the_calls_and_the_flag():
    from gym_traffic import _native
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"int\s+tfx_frame_size\s*\(\s*tfx_handle\s+h\s*,\s*int32_t\s+px\s*,\s*int32_t\s*\*\s*height\s*,\s*"
                     r"int32_t\s*\*\s*width\s*\)\s*;", src)
    assert re.search(r"int\s+tfx_frames\s*\(\s*tfx_handle\s+h\s*,\s*const\s+int32_t\s*\*\s*env_ids\s*,\s*int32_t\s+n_frames\s*,\s*"
                     r"int32_t\s+px\s*,\s*uint8_t\s*\*\s*out\s*,\s*int32_t\s+flags\s*,\s*void\s*\*\s*stream\s*\)\s*;", src)
    assert re.search(r"int\s+tfx_frames_launch\s*\(\s*tfx_handle\s+h\s*,\s*int32_t\s+n_frames\s*,\s*int32_t\s+px\s*,\s*"
                     r"int32_t\s*\*\s*grid\s*,\s*int32_t\s*\*\s*waves\s*\)\s*;", src)
    assert re.search(r"enum\s*\{\s*TFX_FRAMES_ROADS_ONLY\s*=\s*1\s*\}", src)
    assert re.search(r"#define\s+TFX_ABI_VERSION\s+13\b", src)
    assert _native.ABI_VERSION == 13 and _native.FRAMES_ROADS_ONLY == 1
    assert (_native.FRAME_PX_MIN, _native.FRAME_PX_MAX) == (8, 256)
    assert len(_native._PROTOS["tfx_frames"][1]) == 7 and len(_native._PROTOS["tfx_frame_size"][1]) == 4
    assert len(_native._PROTOS["tfx_frames_launch"][1]) == 5


def BAD_ARGS(ids, out):
    """(env_ids, n_frames, px, out, flags) and the words its refusal must contain - shared with tests/test_gpu_frames.py"""
    return (((ids, 2, 32, None, 0), b"out is null"),
            ((ids, 0, 32, out, 0), b"n_frames 0"),
            ((ids, -3, 32, out, 0), b"n_frames -3"),
            ((ids, 2, 7, out, 0), b"px 7 is outside 8..256"),
            ((ids, 2, 257, out, 0), b"px 257 is outside 8..256"),
            ((ids, 2, -1, out, 0), b"px -1 is outside 8..256"),
            ((ids, 2, 32, out, 2), b"flags"),
            ((ids, 2, 32, out, 3), b"flags"),
            ((ids, 2, 32, out, -1), b"flags"))


def frames_fn(lib):
    fn = lib.tfx_frames
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]
    lib.tfx_last_error.restype = C.c_char_p
    return fn


def test_calls_are_exported_and_argument_errors_are_codes(lib):
    """Every TFX_EINVAL of include/tfx.h that needs no handle, with its message: the arguments are checked before the
    handle, so each cause is reachable here, where no device - hence no handle - exists; with good arguments the NULL
    handle is the cause.  `n_frames > E` with NULL env_ids and TFX_ESTATE need a handle: tests/test_gpu_frames.py."""
    assert lib.tfx_abi_version() == 13
    fn = frames_fn(lib)
    word = (C.c_uint8 * 16)()
    ids = (C.c_int32 * 2)(0, 1)
    out = C.cast(word, C.c_void_p)
    for args, msg in BAD_ARGS(C.cast(ids, C.c_void_p), out):
        assert fn(None, *args, None) == -1, msg
        assert msg in lib.tfx_last_error(), (msg, lib.tfx_last_error())
    for px in (8, 256):
        for flags in (0, 1):
            for e in (C.cast(ids, C.c_void_p), None):
                assert fn(None, e, 2, px, out, flags, None) == -1
                assert b"null handle" in lib.tfx_last_error()
    size = lib.tfx_frame_size
    size.restype = C.c_int
    size.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    assert size(None, 7, None, None) == -1 and b"px 7" in lib.tfx_last_error()
    assert size(None, 32, None, None) == -1 and b"null handle" in lib.tfx_last_error()
    geo = lib.tfx_frames_launch
    geo.restype = C.c_int
    geo.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    assert geo(None, 0, 32, None, None) == -1 and b"n_frames 0" in lib.tfx_last_error()
    assert geo(None, 1, 300, None, None) == -1 and b"px 300" in lib.tfx_last_error()
    assert geo(None, 1, 32, None, None) == -1 and b"null handle" in lib.tfx_last_error()
    assert bytes(word) == bytes(16)


# ---- geometry ------------------------------------------------------------------------------------------------------------
def owned_pixels(m, n, S):
    """per road the list of (column, row) it owns"""
    from gym_traffic.devrng import frame_geometry
    start, step, (H, W) = frame_geometry(m, n, S)
    assert (H, W) == ((m + 1) * S + 1, (n + 1) * S + 1)
    t = np.arange(2, S - 1)
    return [list(zip((start[e, 0] + t * step[e, 0]).tolist(), (start[e, 1] + t * step[e, 1]).tolist()))
            for e in range(len(start))], H, W


@pytest.mark.parametrize("m,n", [(1, 1), (2, 2), (3, 2), (2, 3), (4, 4)])
@pytest.mark.parametrize("S", [8, 9, 13, 32])
def test_geometry_roads_are_disjoint_inside_and_off_the_boxes(m, n, S):
    from gym_traffic.envs.roadgraph import GridRoad
    px, H, W = owned_pixels(m, n, S)
    g = GridRoad(m, n, 1.0)
    assert len(px) == g.roads and all(len(p) == S - 3 for p in px)
    every = [q for p in px for q in p]
    assert len(set(every)) == len(every)                                     # no pixel has two roads
    assert all(0 <= c < W and 0 <= r < H for c, r in every)
    centres = [((col + 1) * S, (row + 1) * S) for row in range(m) for col in range(n)]
    assert not any(abs(c - cx) <= 1 and abs(r - cy) <= 1 for c, r in every for cx, cy in centres)
    # the side and the direction are GridRoad's: the pixel at t and GridRoad.locs agree in sign about where the road
    # lies beside its centre line and which way it runs
    seg = g._unit_segments(0.02)
    for e in range(g.roads):
        (c0, r0), (c1, r1) = px[e][0], px[e][-1]
        way = seg[e, 1] - seg[e, 0]
        assert (np.sign(c1 - c0), np.sign(r1 - r0)) == (np.sign(way[0]), np.sign(way[1])), e
        mid = (seg[e, 0] + seg[e, 1]) / 2 + 1                                # the road's middle, in units of S from pixel 0
        if way[0]:
            assert r0 == r1 and r0 - round(float(mid[1])) * S == np.sign(mid[1] - round(float(mid[1]))), e
        else:
            assert c0 == c1 and c0 - round(float(mid[0])) * S == np.sign(mid[0] - round(float(mid[0]))), e
    # a train road ends two pixels before its intersection's centre, its exit road starts two pixels past it
    assert px[0][-1] == (S - 2, S - 1) and px[0][0] == (2, S - 1)


# ---- the NumPy definition: known answers -----------------------------------------------------------------------------------
M2, N2, S2, C2, LEN2 = 2, 2, 13, 8, 100.0         # k = float32(10) / float32(100): ten pixels of 10 units of x each
R2 = 4 * M2 * N2 + 2 * M2 + 2 * N2


def draw(cars_by_road, leading=1, phase=0, elapsed=100, rows_by_road=None, lengths=None, **kw):
    """one 2 x 2 env at 13 pixels per road; cars_by_road: {road: [x from the head on]} -> [H, W, 4]"""
    from gym_traffic.devrng import frames
    x = np.full((1, R2, C2), 777.0, np.float32)                               # junk in the dead slots
    rows = np.full((1, R2, C2), 63, np.uint8) if rows_by_road is not None else None
    ld = np.full((1, R2), leading, np.int64)
    lc = ld.copy()
    for e, xs in cars_by_road.items():
        s = leading
        for j, cx in enumerate(xs):
            s = s + 1 if s + 1 < C2 else 1
            x[0, e, s] = cx
            if rows is not None:
                rows[0, e, s] = rows_by_road[e][j]
        lc[0, e] = s
    img = frames(x, ld, lc, np.full((1, 4), phase), np.full((1, 4), elapsed), M2, N2, S2, LEN2, yellow_ticks=6,
                 rows=rows, lengths=lengths, **kw)
    assert img.dtype == np.uint8 and img.shape == (1, 40, 40, 4) and (img[..., 3] == 255).all()
    return img[0]


def blue(img):
    """the set of (column, row) of the blue pixels"""
    r, c = np.nonzero((img == BLUE).all(axis=-1))
    return set(zip(c.tolist(), r.tolist()))


def blue_t(img):
    """pixels t of road 1 (eastbound into (0, 1): pixel t at (13 + t, 12)) that are blue; nothing else in the frame is"""
    got = blue(img)
    assert all(r == 12 for _, r in got)
    return sorted(c - 13 for c, _ in got)


def test_an_empty_env_is_background_and_light_colours():
    from gym_traffic.devrng import frames
    from gym_traffic.envs.roadgraph import GridRoad
    from gym_traffic.render import light_colours
    rng = np.random.RandomState(5)
    for m, n, S in ((2, 2, 13), (3, 2, 8), (2, 3, 9)):
        g = GridRoad(m, n, 100.0)
        E, C_ = 4, 6
        phase = rng.randint(2, size=(E, g.intersections))
        elapsed = rng.randint(0, 12, size=(E, g.intersections))
        x = np.zeros((E, g.roads, C_), np.float32)
        ld = rng.randint(1, C_, size=(E, g.roads))
        img = frames(x, ld, ld, phase, elapsed, m, n, S, 100.0, yellow_ticks=6)
        px, H, W = owned_pixels(m, n, S)
        assert img.shape == (E, H, W, 4)
        seen = set()
        for k in range(E):
            cols = light_colours(g, phase[k], elapsed[k], 6)
            rest = np.ones((H, W), bool)
            for e in range(g.roads):
                want = tuple(int(255 * c) for c in cols[e]) + (255,) if e < g.train_roads else GREEN
                seen.add(want)
                for c, r in px[e]:
                    assert tuple(img[k, r, c]) == want, (k, e)
                    rest[r, c] = False
            assert (img[k][rest] == 255).all()
        assert seen == {GREEN, YELLOW, RED}


def test_one_car_in_each_direction_and_on_each_exit_side():
    # x = 52, l = 4: a = floor(5.2) = 5, b = floor(4.8) = 4 -> pixels t = 6, 7 of the road, worked out by hand from the
    # table of include/tfx.h at S = 13 (centres at 13 and 26)
    cases = {1: {(19, 12), (20, 12)},         # d = 0 into (0, 1): (cx - S + t, cy - 1) = (13 + t, 12)
             6: {(20, 27), (19, 27)},         # d = 1 into (1, 0): (cx + S - t, cy + 1) = (26 - t, 27)
             11: {(27, 19), (27, 20)},        # d = 2 into (1, 1): (cx + 1, cy - S + t) = (27, 13 + t)
             12: {(12, 20), (12, 19)},        # d = 3 into (0, 0): (cx - 1, cy + S - t) = (12, 26 - t)
             17: {(25, 7), (25, 6)},          # exit out of row 0 at column 1: (cx - 1, cy - t) = (25, 13 - t)
             19: {(32, 25), (33, 25)},        # exit out of the last column at row 1: (cx + t, cy - 1) = (26 + t, 25)
             20: {(14, 32), (14, 33)},        # exit out of the last row at column 0: (cx + 1, cy + t) = (14, 26 + t)
             22: {(7, 14), (6, 14)}}          # exit out of column 0 at row 0: (cx - t, cy + 1) = (13 - t, 14)
    for road, want in cases.items():
        for leading in (1, 7):
            assert blue(draw({road: [52.0]}, leading=leading)) == want, road
    # a single pixel: x = 55 -> a = b = 5
    assert blue(draw({1: [55.0]})) == {(20, 12)}
    # all eight at once: no road's car shows on another
    assert blue(draw({road: [52.0] for road in cases})) == set().union(*cases.values())
    # the road's other pixels keep its light's colour (phase 0 held long: E-W green, N-S red, exits green)
    img = draw({1: [52.0], 11: [52.0]})
    assert tuple(img[12, 15]) == GREEN and tuple(img[12, 24]) == GREEN and tuple(img[12, 14]) == WHITE
    assert tuple(img[15, 27]) == RED and tuple(img[24, 27]) == RED and tuple(img[25, 27]) == WHITE


def test_clamps_nan_lengths_and_rings():
    assert blue_t(draw({1: [150.0]})) == [11]                  # x > length: a and b clamp to S - 4
    assert blue_t(draw({1: [2.0]})) == [2]                     # x - l < 0: b clamps to 0
    assert blue_t(draw({1: [-7.0]})) == [2]
    assert blue_t(draw({1: [float("inf")]})) == [11] and blue_t(draw({1: [float("-inf")]})) == [2]
    assert blue_t(draw({1: [float("nan")]})) == []             # a NaN x is not drawn ...
    assert blue_t(draw({1: [float("nan"), 52.0]})) == [6, 7]   # ... and the cars behind it are
    assert blue_t(draw({1: [99.0, 3.0]})) == [2, 11]           # the road's two ends
    # two lengths from a table: rows 0 and 1 of lengths (4, 12) at x = 51: b = floor(4.7) = 4 / floor(3.9) = 3
    assert blue_t(draw({1: [51.0]}, rows_by_road={1: [0]}, lengths=[4.0, 12.0])) == [6, 7]
    assert blue_t(draw({1: [51.0]}, rows_by_road={1: [1]}, lengths=[4.0, 12.0])) == [5, 6, 7]
    assert blue_t(draw({1: [91.0, 51.0]}, rows_by_road={1: [1, 0]}, lengths=[4.0, 12.0])) == [6, 7, 9, 10, 11]
    # a wrapped ring: leading = 6 of C = 8, cars in slots 7, 1, 2; (91, 87) -> 9, 8; (86, 82) -> 8; (31, 27) -> 3, 2
    assert blue_t(draw({1: [91.0, 86.0, 31.0]}, leading=6)) == [4, 5, 10, 11]
    # a full ring: C - 2 = 6 cars, whose bars leave only the road's first pixel
    full = [95.0, 81.0, 65.0, 51.0, 35.0, 21.0]               # bits 9 | 8, 7 | 6 | 5, 4 | 3 | 2, 1
    for leading in (1, 3, 7):
        img = draw({1: full}, leading=leading)
        assert blue_t(img) == list(range(3, 12)) and tuple(img[12, 15]) == GREEN
    # env_ids: a subset in any order, a repeat, ids out of range
    from gym_traffic.devrng import frames
    x = np.full((3, R2, C2), 52.0, np.float32)
    ld = np.ones((3, R2), np.int64)
    lc = ld.copy()
    lc[1, 1], lc[2, 6] = 2, 2
    ph, el = np.zeros((3, 4), np.int64), np.full((3, 4), 100)
    img = frames(x, ld, lc, ph, el, M2, N2, S2, LEN2, env_ids=[2, -1, 1, 3, 1, 0])
    assert [sorted(blue(f)) for f in img] == [[(19, 27), (20, 27)], [], [(19, 12), (20, 12)], [], [(19, 12), (20, 12)], []]
    assert (img[1] == 255).all() and (img[3] == 255).all() and not (img[5] == 255).all()
    with pytest.raises(ValueError):
        frames(x, ld, lc, ph, el, M2, N2, 7, LEN2)
    with pytest.raises(ValueError):
        frames(x, ld, lc, ph, el, 3, 2, S2, LEN2)


# ---- a property that does not rest on the mirror's own arithmetic ------------------------------------------------------------
def test_blue_pixels_follow_cars_on_roads():
    """Every car covers at least one pixel (a >= b), so a road has a blue pixel iff it has a car - whatever the bars'
    positions are - and every blue pixel lies on a road that has cars."""
    from gym_traffic.devrng import frames
    rng = np.random.RandomState(40)
    for (m, n), C_, S in (((2, 2), 6, 32), ((3, 2), 14, 32), ((2, 3), 66, 64)):      # (at 32 px a car is 0.97 pixels long)
        R = 4 * m * n + 2 * m + 2 * n
        E = 3
        x, _, ld, lc, count = random_rings(rng, E * R, C_)
        assert (count == 0).any() and (count == C_ - 2).any() and (ld > lc).any()
        img = frames(x.reshape(E, R, C_), ld.reshape(E, R), lc.reshape(E, R), rng.randint(2, size=(E, m * n)),
                     rng.randint(0, 12, size=(E, m * n)), m, n, S, 120.0)
        px, H, W = owned_pixels(m, n, S)
        is_blue = (img == BLUE).all(axis=-1)
        count = count.reshape(E, R)
        for k in range(E):
            on_roads = 0
            for e in range(R):
                mine = sum(bool(is_blue[k, r, c]) for c, r in px[e])
                assert (mine > 0) == (count[k, e] > 0), (k, e)
                assert mine <= S - 3
                on_roads += mine
            assert on_roads == is_blue[k].sum()


# ---- the GPU test's driven scenario on the CPU oracle ----------------------------------------------------------------------
_lights = {}
# The scenario of tests/test_measures_host.py ends after 42 ticks, before any car has crossed the 3 x 3 grid: no exit road
# holds a car then.  The frames are therefore taken after the scenario AND a second round of it under another seed
# (84 ticks): the same calls, the first 42 ticks checked against oracle_driven().
DRIVEN_SEEDS = (2024, 2025)


def driven_calls(I, n_entry, E=E_DRIVEN):
    """[(held action, arrival counts per tick)] of the frames' driven scenario: test_measures_host.scenario, twice"""
    return [call for seed in DRIVEN_SEEDS for call in scenario(I, n_entry, E=E, seed=seed)]


def driven_with_lights():
    """The driven scenario on the CPU oracle: dict(x, v [E, R, C], leading, lastcar, cars [E, R], current_phase, elapsed
    [E, I]) after the last call.  Its first half is oracle_driven()'s run, and is checked against it."""
    if not _lights:
        from gym_traffic.envs.roadgraph import GridRoad
        from oracle.oracle import OracleEnv
        g = GridRoad(GRID["m"], GRID["n"], GRID["length"])
        entry = g.generate_entrypoints(0)
        orc = OracleEnv(GRID["m"], GRID["n"], GRID["length"], GRID["capacity"], g.dest, g.phases, g.nexts,
                        n_envs=E_DRIVEN, rate=GRID["rate"])
        orc.reset(np.zeros((E_DRIVEN, orc.I), np.int32))
        calls = driven_calls(orc.I, len(entry))
        for i, (act, cnt) in enumerate(calls):
            for t in range(cnt.shape[0]):
                orc.step(act, roads_of(cnt[t], entry))
            if i + 1 == len(calls) // 2:
                s = oracle_driven()
                assert orc.x.tobytes() == s["x"].tobytes() and np.array_equal(orc.leading, s["leading"])
                assert np.array_equal(orc.lastcar, s["lastcar"])
        _lights.update(x=orc.x.copy(), v=orc.v.copy(), leading=orc.leading.copy(), lastcar=orc.lastcar.copy(),
                       cars=orc.cars_on_roads_flat(), current_phase=orc.current_phase.copy(), elapsed=orc.elapsed.copy())
    return _lights


def driven_frames(s, px=PX_DRIVEN, **kw):
    from gym_traffic.core import ARCHETYPE, CONSTANTS
    from gym_traffic.devrng import frames
    return frames(s["x"], s["leading"], s["lastcar"], s["current_phase"], s["elapsed"], GRID["m"], GRID["n"], px,
                  GRID["length"], yellow_ticks=CONSTANTS["yellow_ticks"], car_l=ARCHETYPE["car_l"], **kw)


def test_driven_scenario_is_not_vacuous():
    """Conditions on the INPUTS of tests/test_gpu_frames.py (the oracle alone, no device): cars on roads of all four
    directions and on an exit road, a bar of two or more pixels, roads of all three colours, a wrapped ring."""
    s = driven_with_lights()
    m, n = GRID["m"], GRID["n"]
    v = m * n
    cars = s["cars"]
    for d in range(4):
        assert cars[:, d * v:(d + 1) * v].any(), d
    assert cars[:, 4 * v:].any()
    assert (s["leading"] > s["lastcar"]).any()                               # a wrapped ring
    img = driven_frames(s)
    px, H, W = owned_pixels(m, n, PX_DRIVEN)
    is_blue = (img == BLUE).all(axis=-1)
    seen, longest = set(), 0
    for k in range(E_DRIVEN):
        for e in range(len(px)):
            line = [bool(is_blue[k, r, c]) for c, r in px[e]]
            assert any(line) == (cars[k, e] > 0)
            run = 0
            for bit in line:
                run = run + 1 if bit else 0
                longest = max(longest, run)
            seen |= {tuple(img[k, r, c]) for c, r in px[e]}
    assert longest >= 2
    assert seen == {GREEN, YELLOW, RED, BLUE}
    assert not is_blue[0].any() and is_blue[1:].any(axis=(1, 2)).all()        # env 0 receives no cars
    print("driven scenario at %d px: %d cars, %d blue pixels, longest bar %d" % (PX_DRIVEN, cars.sum(), is_blue.sum(), longest))
