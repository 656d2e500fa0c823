"""State digests on the device (tfx_state_digest, include/tfx.h), the parts that need no GPU: the header's rule, the entry
points and the binding, the definition as a NumPy function (devrng.state_digest - what tests/test_gpu_digest.py holds the
device to) against a brute-force loop in Python integers, and what the rule must tell apart."""
import ctypes as C
import itertools
import os
import re
import subprocess
import warnings

import numpy as np
import pytest

from conftest import ROOT
from test_car_list_host import rings
from test_measures_host import HEADER, LIB

CARS, ROWS, SPAWN, RING, LIGHTS, OBS = 1, 2, 4, 8, 16, 32
M64 = (1 << 64) - 1
G = 0x9e3779b97f4a7c15


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "traffic-env_amd", "csrc")])
    return C.CDLL(LIB)


# ---- ABI -----------------------------------------------------------------------------------------------------------------
def test_header_declares_the_calls_the_parts_and_the_rule():
    from gym_traffic import _native, devrng
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"int\s+tfx_state_digest\s*\(\s*tfx_handle\s+h\s*,\s*const\s+int32_t\s*\*\s*env_ids\s*,\s*int32_t\s+n_sel\s*,\s*"
                     r"const\s+uint8_t\s*\*\s*road_mask\s*,\s*int32_t\s+parts\s*,\s*uint64_t\s*\*\s*env_digest\s*,\s*"
                     r"uint64_t\s*\*\s*road_digest\s*,\s*int32_t\s+flags\s*,\s*void\s*\*\s*stream\s*\)\s*;", src)
    assert re.search(r"int\s+tfx_digest_launch\s*\(\s*tfx_handle\s+h\s*,\s*int32_t\s+n_sel\s*,\s*int32_t\s*\*\s*grid\s*,\s*"
                     r"int32_t\s*\*\s*waves\s*\)\s*;", src)
    for name, bit in (("CARS", 1), ("ROWS", 2), ("SPAWN", 4), ("RING", 8), ("LIGHTS", 16), ("OBS", 32)):
        assert re.search(r"#define\s+TFX_DIGEST_%s\s+%d\b" % (name, bit), src)
        assert getattr(_native, "DIGEST_" + name) == bit == getattr(devrng, "DIGEST_" + name)
    assert _native.DIGEST_ALL == 63
    assert "tfx_digest_buffers" not in text                                      # two plain pointers, no struct
    # the rule is in the header as text: the constants, and that this is no cryptographic hash
    for word in ("0xbf58476d1ce4e5b9", "0x94d049bb133111eb", "0x9e3779b97f4a7c15", "z >> 30", "z >> 27", "z >> 31",
                 "(2j + 1) * G", "(2j + 2) * G", "(e + 1) * G", "mix(1 + n)", "(2 << 56) | leading"):
        assert word in text, word
    assert re.search(r"not a cryptographic hash", text, re.I)
    assert re.search(r"#define\s+TFX_ABI_VERSION\s+13\b", src)                  # new exports only
    assert _native.ABI_VERSION == 13
    assert len(_native._PROTOS["tfx_state_digest"][1]) == 9 and len(_native._PROTOS["tfx_digest_launch"][1]) == 4
    from gym_traffic import core
    assert not any("digest" in q for q in core.QUERIES)                         # not a row of the query table


def test_calls_are_exported_and_argument_errors_are_codes(lib):
    from gym_traffic import _native
    assert lib.tfx_abi_version() == 13
    fn = lib.tfx_state_digest
    fn.restype, fn.argtypes = _native._PROTOS["tfx_state_digest"]
    lib.tfx_digest_launch.restype, lib.tfx_digest_launch.argtypes = _native._PROTOS["tfx_digest_launch"]
    lib.tfx_last_error.restype = C.c_char_p
    word = (C.c_uint64 * 4)(7, 7, 7, 7)
    out = C.cast(word, C.c_void_p)
    assert fn(None, None, 1, None, CARS, out, None, 0, None) == -1
    assert b"null handle" in lib.tfx_last_error()
    assert fn(None, None, 1, None, CARS, None, None, 0, None) == -1
    assert b"env_digest is null" in lib.tfx_last_error()
    assert fn(None, None, 1, None, CARS, out, None, 1, None) == -1
    assert b"flags" in lib.tfx_last_error()
    for parts in (0, 64, 1 | 128, -1):
        assert fn(None, None, 1, None, parts, out, None, 0, None) == -1
        assert b"parts" in lib.tfx_last_error()
    assert lib.tfx_digest_launch(None, 4, None, None) == -1
    assert list(word) == [7, 7, 7, 7]                                            # a refused call writes nothing


# ---- the NumPy definition against a brute-force loop in Python integers ------------------------------------------------
def mix(z):
    z &= M64
    z ^= z >> 30
    z = z * 0xbf58476d1ce4e5b9 & M64
    z ^= z >> 27
    z = z * 0x94d049bb133111eb & M64
    z ^= z >> 31
    return z


def bits(a):
    """the 32-bit patterns of a float32 / int32 array as Python-int-friendly uint32 (a uint8 array: zero-extended)"""
    a = np.ascontiguousarray(a)
    return a.astype(np.uint32) if a.dtype == np.uint8 else a.view(np.uint32)


def brute(x, v, w, arch, ld, lc, Cc, flags, env_ids=None, road_mask=None, obs=None, rewards=None, waiting=None,
          passed_dst=None, done_tick=None, I=None, r=None):
    """the rule of include/tfx.h once more, car by car and word by word in Python integers"""
    E, R = ld.shape
    ids = list(range(E)) if env_ids is None else [int(e) for e in env_ids]
    env_d, road_d = [], []
    road_parts = flags & (CARS | ROWS | SPAWN | RING)
    for e in ids:
        total, roads = 0, [0] * R
        if 0 <= e < E:
            for rd in range(R if road_parts else 0):
                if road_mask is not None and not road_mask[rd]:
                    continue
                n = int(lc[e, rd]) - int(ld[e, rd]) + (Cc - 1 if ld[e, rd] > lc[e, rd] else 0)
                n = min(max(n, 0), Cc - 1)
                d = mix(1 + n)
                if flags & RING:
                    d += mix((2 << 56) | int(ld[e, rd]))
                slot = int(ld[e, rd])
                for j in range(n):
                    slot = slot + 1 if slot + 1 < Cc else 1
                    if flags & CARS:
                        a = int(bits(x)[e, rd, slot]) | int(bits(v)[e, rd, slot]) << 32
                        d += mix(a + (2 * j + 1) * G)
                    if flags & (ROWS | SPAWN):
                        b = int(bits(w)[e, rd, slot]) if flags & SPAWN else 0
                        if flags & ROWS and arch is not None:
                            b |= int(arch[e, rd, slot]) << 32
                        d += mix(b + (2 * j + 2) * G)
                roads[rd] = d & M64
                total += mix(roads[rd] + (rd + 1) * G)
            sections = []
            if flags & LIGHTS:
                sections += [(1, bits(obs)[e, 2 * r:2 * r + I]), (2, bits(obs)[e, 2 * r + I:])]
            if flags & OBS:
                sections += [(3, bits(obs)[e, :r]), (4, bits(obs)[e, r:2 * r]), (5, bits(waiting)[e]), (6, bits(passed_dst)[e]),
                             (7, bits(rewards)[e]), (8, bits(done_tick)[e:e + 1])]
            for s, vals in sections:
                for i, val in enumerate(vals):
                    total += mix(s << 56 | i << 32 | int(val))
        env_d.append(total & M64)
        road_d.append(roads)
    return np.array(env_d, np.uint64), np.array(road_d, np.uint64).reshape(len(ids), R)


def words_of(rng, E, I, r):
    """random bound buffers: obs, rewards (with -0.0 and a NaN), waiting, passed_dst, done_tick"""
    obs = rng.randint(0, 40, size=(E, 2 * r + 2 * I)).astype(np.int32)
    obs[0, 1] = -3                                                                # a negative int32 is its bit pattern
    rewards = rng.uniform(-5, 5, size=(E, I)).astype(np.float32)
    rewards[0, 0] = -0.0
    rewards[1 % E, 1] = np.array([0x7FC00777], np.uint32).view(np.float32)[0]
    return dict(obs=obs, rewards=rewards, waiting=rng.randint(0, 9, size=(E, r)).astype(np.int32),
                passed_dst=rng.randint(0, 256, size=(E, I)).astype(np.uint8),
                done_tick=rng.randint(0, 2 ** 31 - 1, size=E).astype(np.int32), I=I, r=r)


PART_SETS = (CARS, ROWS, SPAWN, RING, LIGHTS, OBS, CARS | ROWS, CARS | SPAWN, ROWS | SPAWN, CARS | RING, RING | LIGHTS,
             CARS | ROWS | RING | LIGHTS | OBS, 63)


def same(got, want, where):
    for g, q in zip(got, want):
        assert g.dtype == np.uint64 and g.shape == q.shape and g.tobytes() == q.tobytes(), where


@pytest.mark.parametrize("Cc", [5, 14, 66])
def test_definition_against_a_brute_force_loop(Cc):
    from gym_traffic.devrng import state_digest
    E, R, I, r = 4, 23, 4, 16
    x, v, w, arch, ld, lc, n = rings(Cc, E, R, Cc)
    assert (ld > lc).any() and (n == 0).any() and (n == Cc - 2).any()           # wrapped, empty and full roads
    x[0, 0, :] = np.array([0x7FC12345], np.uint32).view(np.float32)[0]        # a NaN's payload is hashed
    wd = words_of(np.random.RandomState(Cc), E, I, r)
    arterial = np.zeros(R, np.uint8)
    arterial[[2, 3, 11]] = 1
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                          # the rule wraps without a warning
        for ids in (None, [2], [3, 0, 3, 3], [-1, 1, E, 1, 7]):
            for mask in (None, arterial, np.zeros(R, np.uint8)):
                for flags in PART_SETS:
                    for het in (True, False):
                        a_ = arch if het else None
                        got = state_digest(x, v, w, a_, ld, lc, Cc, flags, ids, mask, **wd)
                        same(got, brute(x, v, w, a_, ld, lc, Cc, flags, ids, mask, **wd), (ids, flags, het))
    # ids outside the batch and masked roads give 0; repeats give equal words
    env, road = state_digest(x, v, w, arch, ld, lc, Cc, 63, [1, -1, 1, E], arterial, **wd)
    assert env[1] == 0 and env[3] == 0 and not road[1].any() and not road[3].any()
    assert env[0] == env[2] != 0 and np.array_equal(road[0], road[2])
    assert not road[0][arterial == 0].any() and road[0][arterial != 0].all()
    # no road part: no road term, road_digest 0
    env, road = state_digest(None, None, None, None, ld, lc, Cc, LIGHTS | OBS, **wd)
    assert not road.any() and env.all() and len(set(env.tolist())) == E
    for bad in (0, 64, -1):
        with pytest.raises(ValueError):
            state_digest(x, v, w, arch, ld, lc, Cc, bad)


def test_pathological_ring_states():
    """wrapped, full, empty and unsorted rings of oracle/ring_states.py: the definition follows ring order, not x"""
    from gym_traffic.devrng import state_digest
    from oracle.ring_states import random_state
    Cc, E, R = 10, 3, 12
    for seed, sorted_x in ((1, True), (2, False)):
        rng = np.random.RandomState(seed)
        x, v, w, ld, lc = random_state(rng, E, R, Cc, 100.0, crowd=0.6, sorted_x=sorted_x)
        n = lc - ld + np.where(ld > lc, Cc - 1, 0)
        assert (ld > lc).any() and (n == 0).any() and (n == Cc - 2).any()
        for flags in (CARS, CARS | SPAWN | RING, SPAWN):
            same(state_digest(x, v, w, None, ld, lc, Cc, flags), brute(x, v, w, None, ld, lc, Cc, flags), (seed, flags))
    # a ring whose words say C - 1 cars (lastcar just behind leading) is clamped as tfx_cars_on_roads clamps it
    ld1, lc1 = np.array([[3]], np.int32), np.array([[2]], np.int32)
    x1 = np.arange(Cc, dtype=np.float32).reshape(1, 1, Cc)
    same(state_digest(x1, x1, x1, None, ld1, lc1, Cc, CARS), brute(x1, x1, x1, None, ld1, lc1, Cc, CARS), "full")


# ---- what the rule tells apart -------------------------------------------------------------------------------------------
def test_every_small_road_state_has_its_own_digest():
    """every road state with 0..5 cars, x in {0, 1, 2} and v in {0, 1}: sum of 6^k for k = 0..5 = 9331 states, all digests
    distinct - order, count and every value enter"""
    from gym_traffic.devrng import state_digest
    Cc = 8
    states = [cars for k in range(6) for cars in itertools.product(itertools.product((0.0, 1.0, 2.0), (0.0, 1.0)), repeat=k)]
    assert len(states) == 9331
    x = np.zeros((1, len(states), Cc), np.float32)
    v = np.zeros((1, len(states), Cc), np.float32)
    ld = np.full((1, len(states)), 1, np.int32)
    lc = np.array([[1 + len(cars) for cars in states]], np.int32)
    for i, cars in enumerate(states):
        for j, (cx, cv) in enumerate(cars):
            x[0, i, 2 + j], v[0, i, 2 + j] = cx, cv
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                          # evaluates without overflow warnings
        env, road = state_digest(x, v, None, None, ld, lc, Cc, CARS)
    assert len(set(road[0].tolist())) == 9331


def one_road(cars, leading=1, Cc=8):
    x, v = np.full((1, 1, Cc), 5.5, np.float32), np.full((1, 1, Cc), 6.5, np.float32)    # junk in the dead slots
    s = leading
    for cx, cv in cars:
        s = s + 1 if s + 1 < Cc else 1
        x[0, 0, s], v[0, 0, s] = cx, cv
    return x, v, np.array([[leading]], np.int32), np.array([[s]], np.int32), Cc


def test_sensitivity():
    from gym_traffic.devrng import state_digest

    def d(cars, flags=CARS, leading=1, **kw):
        x, v, ld, lc, Cc = one_road(cars, leading)
        env, road = state_digest(x, v, None, None, ld, lc, Cc, flags, **kw)
        return int(env[0]), int(road[0, 0])

    base = [(30.0, 2.0), (20.0, 1.0), (10.0, 0.0)]
    assert d(base) == d(list(base))
    assert d(base) != d([base[1], base[0], base[2]])                             # two cars swapped
    assert d(base) != d(base[:2])                                                # the last car dropped
    assert d(base) != d(base[:2] + [(10.0, -0.0)])                               # -0.0 is not 0.0
    assert d(base[:2] + [(10.0, -0.0)]) == d(base[:2] + [(10.0, -0.0)])
    # the same cars one ring step further: only RING sees it (dead slots do not enter)
    assert d(base, CARS, leading=1) == d(base, CARS, leading=2) == d(base, CARS, leading=6)
    assert d(base, CARS | RING, leading=1) != d(base, CARS | RING, leading=2)
    # one elapsed tick: only LIGHTS sees it
    I, r = 2, 8
    wd = words_of(np.random.RandomState(3), 1, I, r)
    later = dict(wd, obs=wd["obs"].copy())
    later["obs"][0, 2 * r + I + 1] += 1
    for flags, differs in ((CARS | LIGHTS, True), (LIGHTS, True), (CARS | OBS, False), (OBS, False)):
        assert (d(base, flags, **wd) != d(base, flags, **later)) == differs, flags
    # a counter: only OBS sees it
    more = dict(wd, waiting=wd["waiting"] + (np.arange(r) == 5))
    assert d(base, OBS, **wd) != d(base, OBS, **more) and d(base, LIGHTS, **wd) == d(base, LIGHTS, **more)


def test_parts_that_are_off_do_not_read_their_arrays():
    from gym_traffic.devrng import state_digest
    E, R, Cc, I, r = 2, 7, 9, 2, 8
    x, v, w, arch, ld, lc, n = rings(5, E, R, Cc)
    wd = words_of(np.random.RandomState(5), E, I, r)
    full = state_digest(x, v, w, arch, ld, lc, Cc, CARS)
    same(state_digest(x, v, None, None, ld, lc, Cc, CARS), full, "cars")
    same(state_digest(None, None, None, None, ld, lc, Cc, RING), state_digest(x, v, w, arch, ld, lc, Cc, RING, **wd), "ring")
    same(state_digest(None, None, w, None, ld, lc, Cc, SPAWN), state_digest(x, v, w, arch, ld, lc, Cc, SPAWN), "spawn")
    same(state_digest(None, None, None, arch, ld, lc, Cc, ROWS), state_digest(x, v, w, arch, ld, lc, Cc, ROWS), "rows")
    lights = dict(obs=wd["obs"], I=I, r=r)
    same(state_digest(None, None, None, None, ld, lc, Cc, LIGHTS, **lights),
         state_digest(x, v, w, arch, ld, lc, Cc, LIGHTS, **wd), "lights")
    with pytest.raises(ValueError):
        state_digest(x, v, None, arch, ld, lc, Cc, SPAWN)                       # no spawn plane to hash
    with pytest.raises(ValueError):
        state_digest(x, v, w, arch, ld, lc, Cc, LIGHTS)                         # no obs to hash
