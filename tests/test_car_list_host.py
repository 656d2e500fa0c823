"""Car lists on the device (tfx_car_list, include/tfx.h), the parts that need no GPU: the entry points, the struct and the
binding, the definition as a NumPy function (devrng.car_list - what tests/test_gpu_car_list.py holds the device to) against
a brute-force loop over random rings, and the definition applied to the CPU oracle's driven state."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_measures_host import GRID, HEADER, LIB, oracle_driven, random_rings

PLANES = ("xv", "road", "row", "spawn")
SENTINEL = 0xA5


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "traffic-env_amd", "csrc")])
    return C.CDLL(LIB)


# ---- ABI -----------------------------------------------------------------------------------------------------------------
def test_header_declares_the_calls_and_the_struct():
    from gym_traffic import _native
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"int\s+tfx_car_list\s*\(\s*tfx_handle\s+h\s*,\s*const\s+int32_t\s*\*\s*env_ids\s*,\s*int32_t\s+n_sel\s*,\s*"
                     r"const\s+uint8_t\s*\*\s*road_mask\s*,\s*const\s+int32_t\s*\*\s*offsets\s*,\s*int32_t\s+cap\s*,\s*"
                     r"const\s+tfx_car_list_buffers\s*\*\s*out\s*,\s*int32_t\s+flags\s*,\s*void\s*\*\s*stream\s*\)\s*;", src)
    assert re.search(r"int\s+tfx_car_list_launch\s*\(\s*tfx_handle\s+h\s*,\s*int32_t\s+n_sel\s*,\s*int32_t\s*\*\s*grid\s*,\s*"
                     r"int32_t\s*\*\s*waves\s*\)\s*;", src)
    body = re.search(r"typedef struct \{([^{}]*)\} tfx_car_list_buffers;", src, re.S).group(1)
    assert [re.sub(r"\s+", " ", d.strip()) for d in body.split(";") if d.strip()] == \
        ["float *xv", "int32_t *road", "uint8_t *row", "float *spawn"]
    assert re.search(r"#define\s+TFX_ABI_VERSION\s+13\b", src)                  # new exports only
    assert _native.ABI_VERSION == 13
    assert len(_native._PROTOS["tfx_car_list"][1]) == 9 and len(_native._PROTOS["tfx_car_list_launch"][1]) == 4


def test_ctypes_struct_has_the_c_layout(tmp_path):
    """size and offsets as the C compiler lays the struct of include/tfx.h out, through a tiny compiled probe"""
    from gym_traffic import _native
    B = _native.TfxCarListBuffers
    assert [f[0] for f in B._fields_] == list(PLANES)
    probe = tmp_path / "probe.c"
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "tfx.h"', "int main(void) {",
             '  printf("%zu\\n", sizeof(tfx_car_list_buffers));']
    for f in PLANES:
        lines.append('  printf("%%zu\\n", offsetof(tfx_car_list_buffers, %s));' % f)
    probe.write_text("\n".join(lines + ["  return 0;", "}"]) + "\n")
    exe = tmp_path / "probe"
    cc = os.environ.get("CC") or shutil.which("cc") or shutil.which("gcc")       # the compiler that builds the oracle
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(probe)])
    words = [int(w) for w in subprocess.check_output([str(exe)], text=True).split()]
    assert words[0] == C.sizeof(B) == 4 * C.sizeof(C.c_void_p)
    assert words[1:] == [getattr(B, f).offset for f in PLANES]


def test_calls_are_exported_and_argument_errors_are_codes(lib):
    from gym_traffic import _native
    assert lib.tfx_abi_version() == 13
    fn = lib.tfx_car_list
    fn.restype, fn.argtypes = _native._PROTOS["tfx_car_list"]
    lib.tfx_car_list_launch.restype, lib.tfx_car_list_launch.argtypes = _native._PROTOS["tfx_car_list_launch"]
    lib.tfx_last_error.restype = C.c_char_p
    word = (C.c_int32 * 4)()
    b = _native.TfxCarListBuffers()
    b.road = C.cast(word, C.c_void_p)
    off = C.cast(word, C.c_void_p)
    assert fn(None, None, 1, None, off, 4, C.byref(b), 0, None) == -1
    assert b"null handle" in lib.tfx_last_error()
    assert fn(None, None, 1, None, off, 4, None, 0, None) == -1
    assert b"out is null" in lib.tfx_last_error()
    assert fn(None, None, 1, None, None, 4, C.byref(b), 0, None) == -1
    assert b"offsets is null" in lib.tfx_last_error()
    assert fn(None, None, 1, None, off, -1, C.byref(b), 0, None) == -1
    assert b"cap -1" in lib.tfx_last_error()
    assert fn(None, None, 1, None, off, 4, C.byref(b), 2, None) == -1
    assert b"flags" in lib.tfx_last_error()
    assert lib.tfx_car_list_launch(None, 4, None, None) == -1
    assert list(word) == [0, 0, 0, 0]


# ---- the NumPy definition against a brute-force loop -------------------------------------------------------------------
def brute(x, v, w, arch, ld, lc, Cc, env_ids, road_mask, cap, fill):
    """the rule of include/tfx.h once more, car by car in plain Python; planes prefilled with `fill` bytes"""
    E, R = ld.shape
    ids = list(range(E)) if env_ids is None else [int(e) for e in env_ids]
    cars, offsets = [], [0]
    for s, e in enumerate(ids):
        for rd in range(R):
            n = 0
            if 0 <= e < E and (road_mask is None or road_mask[rd]):
                n = int(lc[e, rd]) - int(ld[e, rd]) + (Cc - 1 if ld[e, rd] > lc[e, rd] else 0)
                n = min(max(n, 0), Cc - 1)
            slot = int(ld[e, rd]) if n else 0
            for j in range(n):
                slot = slot + 1 if slot + 1 < Cc else 1
                cars.append((s * R + rd, e, rd, slot))
            offsets.append(len(cars))
    N = len(cars)
    cap = N if cap is None else cap
    xv = np.full((cap, 2), 0, np.float32)
    road, row, spawn = np.zeros(cap, np.int32), np.zeros(cap, np.uint8), np.zeros(cap, np.float32)
    for a in (xv, road, row, spawn):
        a.view(np.uint8)[...] = fill
    for i, (key, e, rd, slot) in enumerate(cars[:cap]):
        xv.view(np.uint32)[i] = (x.view(np.uint32)[e, rd, slot], v.view(np.uint32)[e, rd, slot])    # bits, not values
        road[i] = key
        row[i] = 0 if arch is None else arch[e, rd, slot]
        spawn[i] = 0.0 if w is None else w[e, rd, slot]
    return N, np.array(offsets, np.int32), xv, road, row, (None if w is None else spawn)


def same(got, want, where):
    assert got[0] == want[0], where
    for name, g, q in zip(("offsets",) + PLANES, got[1:], want[1:]):
        assert (g is None) == (q is None), (name, where)
        if g is not None:
            assert g.dtype == q.dtype and g.shape == q.shape and g.tobytes() == q.tobytes(), (name, where)


def sentinels(cap, spawn=True):
    out = [np.empty((cap, 2), np.float32), np.empty(cap, np.int32), np.empty(cap, np.uint8),
           np.empty(cap, np.float32) if spawn else None]
    for a in out:
        if a is not None:
            a.view(np.uint8)[...] = SENTINEL
    return out


def rings(seed, E, R, Cc, het=True):
    rng = np.random.RandomState(seed)
    x, v, ld, lc, n = random_rings(rng, E * R, Cc)
    w = rng.randint(0, 50, size=(E, R, Cc)).astype(np.float32)
    arch = rng.randint(3, size=(E, R, Cc)).astype(np.uint8) if het else None
    return x.reshape(E, R, Cc), v.reshape(E, R, Cc), w, arch, ld.reshape(E, R), lc.reshape(E, R), n.reshape(E, R)


@pytest.mark.parametrize("Cc", [5, 14, 66])
def test_definition_against_a_brute_force_loop(Cc):
    from gym_traffic.devrng import car_list
    E, R = 4, 23
    x, v, w, arch, ld, lc, n = rings(Cc, E, R, Cc)
    assert (ld > lc).any() and (n == 0).any() and (n == Cc - 2).any()           # wrapped, empty and full roads
    x[0, 0, :] = np.array([0x7FC12345], np.uint32).view(np.float32)[0]        # a NaN's payload travels
    arterial = np.zeros(R, np.uint8)
    arterial[[2, 3, 11]] = 1
    total = int(n.sum())
    for ids in (None, [2], [3, 0, 3, 3], [-1, 1, E, 1, 7], np.array([0, 1, 2, 3, 2, 1, 0])):
        for mask in (None, arterial, np.zeros(R, np.uint8), np.ones(R, np.uint8)):
            N = car_list(x, v, w, arch, ld, lc, Cc, ids, mask)[0]
            for cap in sorted({None, 0, 1, max(N - 1, 0), N, N + 5}, key=lambda c: -1 if c is None else c):
                for het, val in ((True, True), (False, True), (False, False)):
                    a_, w_ = (arch if het else None), (w if val else None)
                    where = (ids, None if mask is None else mask.tolist(), cap, het, val)
                    got = car_list(x, v, w_, a_, ld, lc, Cc, ids, mask, cap,
                                   out=None if cap is None else sentinels(cap, val))
                    want = brute(x, v, w_, a_, ld, lc, Cc, ids, mask, cap, SENTINEL if cap is not None else 0)
                    same(got, want, where)
    got = car_list(x, v, w, arch, ld, lc, Cc)
    assert got[0] == total == len(got[2]) and got[1][-1] == total and got[1].dtype == np.int32
    assert np.array_equal(np.diff(got[1]), n.reshape(-1))
    # repeats give identical runs; an invalid id and a masked road give empty ones
    got = car_list(x, v, w, arch, ld, lc, Cc, [1, -1, 1, E], arterial)
    cnt = np.diff(got[1]).reshape(4, R)
    assert not cnt[1].any() and not cnt[3].any() and np.array_equal(cnt[0], n[1] * arterial) and np.array_equal(cnt[0], cnt[2])
    half = got[0] // 2
    assert half > 0 and got[2][:half].tobytes() == got[2][half:].tobytes() and got[4][:half].tobytes() == got[4][half:].tobytes()
    assert np.array_equal(got[3][:half] + 2 * R, got[3][half:])
    with pytest.raises(ValueError):
        car_list(x, v, w, arch, ld, lc, Cc, cap=-1)


# ---- the definition on the CPU oracle's driven state ---------------------------------------------------------------------
def test_against_the_oracle():
    from gym_traffic.devrng import car_list
    from oracle.oracle import ring_order
    s = oracle_driven()
    Cc = GRID["capacity"]
    E, R = s["cars"].shape
    N, offsets, xv, road, row, spawn = car_list(s["x"], s["v"], None, None, s["leading"], s["lastcar"], Cc)
    assert spawn is None and not row.any()
    assert np.array_equal(np.diff(offsets).reshape(E, R), s["cars"]) and N == int(s["cars"].sum()) > 20
    # scattering the list back rebuilds the ring image: every live slot, and nothing else
    x = np.full(s["x"].shape, np.nan, np.float32)
    v = np.full(s["v"].shape, np.nan, np.float32)
    for e in range(E):
        for rd in range(R):
            slots = ring_order(int(s["leading"][e, rd]), int(s["lastcar"][e, rd]), Cc)
            k = e * R + rd
            assert len(slots) == offsets[k + 1] - offsets[k]
            assert (road[offsets[k]:offsets[k + 1]] == k).all()
            for j, slot in enumerate(slots):
                x[e, rd, slot], v[e, rd, slot] = xv[offsets[k] + j]
    live = ~np.isnan(x)
    assert live.sum() == N
    assert x[live].tobytes() == s["x"][live].tobytes() and v[live].tobytes() == s["v"][live].tobytes()
