"""Car lists back in (tfx_put_cars, include/tfx.h), the parts that need no GPU: the entry points, the struct and the
binding, and the definition as a NumPy function (devrng.put_cars - what tests/test_gpu_put_cars.py holds the device to):
the inverse of devrng.car_list on random rings and on the pathological family of oracle/ring_states.py, clipping and the
lost count, masks, ids outside the batch, the `leading` rule and spawn_shift on plain and heterogeneous side words."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_measures_host import HEADER, LIB
from test_car_list_host import rings

FIELDS = ("xv", "row", "spawn", "leading", "lead_x")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "traffic-env_amd", "csrc")])
    return C.CDLL(LIB)


# ---- ABI -----------------------------------------------------------------------------------------------------------------
def test_header_declares_the_calls_and_the_struct():
    from gym_traffic import _native
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"int\s+tfx_put_cars\s*\(\s*tfx_handle\s+h\s*,\s*const\s+int32_t\s*\*\s*env_ids\s*,\s*int32_t\s+n_sel\s*,\s*"
                     r"const\s+uint8_t\s*\*\s*road_mask\s*,\s*const\s+int32_t\s*\*\s*offsets\s*,\s*int32_t\s+cap\s*,\s*"
                     r"const\s+tfx_put_buffers\s*\*\s*in\s*,\s*int32_t\s+spawn_shift\s*,\s*uint64_t\s*\*\s*lost\s*,\s*"
                     r"int32_t\s+flags\s*,\s*void\s*\*\s*stream\s*\)\s*;", src)
    assert re.search(r"int\s+tfx_put_launch\s*\(\s*tfx_handle\s+h\s*,\s*int32_t\s+n_sel\s*,\s*int32_t\s*\*\s*grid\s*,\s*"
                     r"int32_t\s*\*\s*waves\s*\)\s*;", src)
    body = re.search(r"typedef struct \{([^{}]*)\} tfx_put_buffers;", src, re.S).group(1)
    assert [re.sub(r"\s+", " ", d.strip()) for d in body.split(";") if d.strip()] == \
        ["const float *xv", "const uint8_t *row", "const float *spawn", "const int32_t *leading", "const float *lead_x"]
    assert re.search(r"#define\s+TFX_ABI_VERSION\s+13\b", src)                  # new exports only
    assert _native.ABI_VERSION == 13
    assert len(_native._PROTOS["tfx_put_cars"][1]) == 11 and len(_native._PROTOS["tfx_put_launch"][1]) == 4


def test_ctypes_struct_has_the_c_layout(tmp_path):
    """size and offsets as the C compiler lays the struct of include/tfx.h out, through a tiny compiled probe"""
    from gym_traffic import _native
    B = _native.TfxPutBuffers
    assert [f[0] for f in B._fields_] == list(FIELDS)
    probe = tmp_path / "probe.c"
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "tfx.h"', "int main(void) {",
             '  printf("%zu\\n", sizeof(tfx_put_buffers));']
    for f in FIELDS:
        lines.append('  printf("%%zu\\n", offsetof(tfx_put_buffers, %s));' % f)
    probe.write_text("\n".join(lines + ["  return 0;", "}"]) + "\n")
    exe = tmp_path / "probe"
    cc = os.environ.get("CC") or shutil.which("cc") or shutil.which("gcc")
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(probe)])
    words = [int(w) for w in subprocess.check_output([str(exe)], text=True).split()]
    assert words[0] == C.sizeof(B) == 5 * C.sizeof(C.c_void_p)
    assert words[1:] == [getattr(B, f).offset for f in FIELDS]


def test_calls_are_exported_and_argument_errors_are_codes(lib):
    from gym_traffic import _native
    assert lib.tfx_abi_version() == 13
    fn = lib.tfx_put_cars
    fn.restype, fn.argtypes = _native._PROTOS["tfx_put_cars"]
    lib.tfx_put_launch.restype, lib.tfx_put_launch.argtypes = _native._PROTOS["tfx_put_launch"]
    lib.tfx_last_error.restype = C.c_char_p
    word = (C.c_int32 * 4)()
    b = _native.TfxPutBuffers()
    b.xv = C.cast(word, C.c_void_p)
    off = C.cast(word, C.c_void_p)
    assert fn(None, None, 1, None, off, 4, C.byref(b), 0, None, 0, None) == -1
    assert b"null handle" in lib.tfx_last_error()
    assert fn(None, None, 1, None, off, 4, None, 0, None, 0, None) == -1
    assert b"in is null" in lib.tfx_last_error()
    assert fn(None, None, 1, None, off, 4, C.byref(_native.TfxPutBuffers()), 0, None, 0, None) == -1
    assert b"xv is null" in lib.tfx_last_error()
    assert fn(None, None, 1, None, None, 4, C.byref(b), 0, None, 0, None) == -1
    assert b"offsets is null" in lib.tfx_last_error()
    assert fn(None, None, 1, None, off, -1, C.byref(b), 0, None, 0, None) == -1
    assert b"cap -1" in lib.tfx_last_error()
    assert fn(None, None, 1, None, off, 4, C.byref(b), 0, None, 2, None) == -1
    assert b"flags" in lib.tfx_last_error()
    assert lib.tfx_put_launch(None, 4, None, None) == -1
    assert list(word) == [0, 0, 0, 0]


# ---- the definition: the inverse of car_list -----------------------------------------------------------------------------
def live(ld, lc, Cc):
    from oracle.ring_states import live_slots
    E, R = ld.shape
    return live_slots(ld.reshape(-1), lc.reshape(-1), Cc).reshape(E, R, Cc)


def lead_of(x, ld):
    return np.take_along_axis(x, ld[..., None].astype(np.int64), axis=2)[..., 0]


def blank(x, v, w, arch, ld, lc, seed):
    """another image of the same shapes: every slot a sentinel, the ring words elsewhere"""
    rng = np.random.RandomState(seed)
    Cc = x.shape[2]
    f = lambda a: None if a is None else np.full(a.shape, 77, a.dtype)  # noqa: E731
    ld2 = rng.randint(1, Cc, size=ld.shape).astype(np.int32)
    return f(x), f(v), f(w), f(arch), ld2, ld2.copy()


def assert_image(got, want_planes, ld, lc, Cc, where, lead_x=None):
    x, v, w, arch, gl, gc, _ = got
    assert np.array_equal(gl, ld) and np.array_equal(gc, lc), where
    m = live(ld, lc, Cc)
    for g, q in zip((x, v, w, arch), want_planes):
        assert (g is None) == (q is None), where
        if g is not None:
            assert g[m].tobytes() == q[m].tobytes(), where
    if lead_x is not None:
        assert lead_of(x, ld).tobytes() == lead_x.tobytes(), where


@pytest.mark.parametrize("Cc", [5, 14, 66])
def test_put_is_the_inverse_of_car_list_on_random_rings(Cc):
    from gym_traffic.devrng import car_list, put_cars
    E, R = 4, 23
    x, v, w, arch, ld, lc, n = rings(Cc, E, R, Cc)
    ld, lc = ld.astype(np.int32), lc.astype(np.int32)
    assert (ld > lc).any() and (n == 0).any() and (n == Cc - 2).any()           # wrapped, empty and full roads
    x[0, 0, :] = np.array([0x7FC12345], np.uint32).view(np.float32)[0]          # a NaN's payload travels
    lx = lead_of(x, ld)
    for het, val in ((True, True), (False, True), (False, False)):
        w_, a_ = (w if val else None), (arch if het else None)
        N, off, xv, road, row, spawn = car_list(x, v, w_, a_, ld, lc, Cc)
        b = blank(x, v, w_, a_, ld, lc, 1)
        got = put_cars(*b, Cc, off, xv, row, spawn, new_leading=ld.reshape(-1), lead_x=lx.reshape(-1), het=het)
        assert got[6] == 0
        assert_image(got, (x, v, w_, a_), ld, lc, Cc, (het, val), lx)
        # slots that hold no car afterwards, and the lead slot aside, keep what they held
        free = ~live(ld, lc, Cc)
        free[np.arange(E)[:, None], np.arange(R)[None, :], ld] = False
        assert (got[0][free] == 77).all() and (got[1][free] == 77).all()
        # without `leading` a road keeps its own: the same cars, head first, behind another slot
        got = put_cars(*b, Cc, off, xv, row, spawn, het=het)
        assert np.array_equal(got[4], b[4]) and np.isinf(lead_of(got[0], got[4])).all()
        again = car_list(got[0], got[1], got[2], got[3], got[4], got[5], Cc)
        assert again[0] == N and again[1].tobytes() == off.tobytes() and again[2].tobytes() == xv.tobytes()
        assert again[4].tobytes() == row.tobytes() and (spawn is None or again[5].tobytes() == spawn.tobytes())


@pytest.mark.parametrize("crowd,beyond", [(0.3, 0.0), (0.8, 1.6)])
def test_put_is_the_inverse_on_the_pathological_states(crowd, beyond):
    from gym_traffic.devrng import car_list, put_cars
    from oracle.ring_states import random_state
    E, R, Cc = 3, 48, 14
    x, v, w, ld, lc = random_state(np.random.RandomState(5), E, R, Cc, 120.0, crowd, beyond)
    n = lc - ld + np.where(ld > lc, Cc - 1, 0)
    assert (ld > lc).any() and (n == 0).any() and (n == Cc - 2).any()
    lx = lead_of(x, ld)
    N, off, xv, road, row, spawn = car_list(x, v, w, None, ld, lc, Cc)
    got = put_cars(*blank(x, v, w, None, ld, lc, 2), Cc, off, xv, None, spawn, new_leading=ld, lead_x=lx)
    assert got[6] == 0 and N == int(n.sum())
    assert_image(got, (x, v, w, None), ld, lc, Cc, (crowd, beyond), lx)


# ---- clipping and the lost count ---------------------------------------------------------------------------------------
def test_clipping_and_lost():
    from gym_traffic.devrng import put_cars
    E, R, Cc = 2, 3, 6
    z = np.zeros((E, R, Cc), np.float32)
    ones = np.ones((E, R), np.int32)
    # runs per key: 0, 9 (over C - 2 = 4), 2, decreasing (-> 0), 3 cut by cap to 1, 2 wholly past cap
    off = np.array([0, 0, 9, 11, 10, 13, 15], np.int32)
    cap = 11
    xv = np.stack([np.arange(cap, dtype=np.float32) + 100, np.arange(cap, dtype=np.float32)], axis=1)
    x, v, w, arch, ld, lc, lost = put_cars(z, z, None, None, ones, ones, Cc, off, xv, None, None)
    cnt = lc - ld + np.where(ld > lc, Cc - 1, 0)
    assert cnt.reshape(-1).tolist() == [0, 4, 2, 0, 1, 0]
    assert lost == (9 - 4) + (3 - 1) + 2
    assert x[0, 1, 2:6].tolist() == [100, 101, 102, 103] and x[0, 2, 2:4].tolist() == [109, 110]
    assert x[1, 1, 2] == 110 and v[1, 1, 2] == 10                              # entry 10 = first entry of the run
    # offsets that go negative: the run is cut to the entries that exist
    off = np.array([-3, 2, 2, 2, 2, 2, 2], np.int32)
    x, v, w, arch, ld, lc, lost = put_cars(z, z, None, None, ones, ones, Cc, off, xv, None, None)
    assert (lc - ld).reshape(-1).tolist() == [2, 0, 0, 0, 0, 0] and lost == 3 and x[0, 0, 2:4].tolist() == [100, 101]
    # cap == 0 empties the selected roads
    x, v, w, arch, ld, lc, lost = put_cars(z, z, None, None, ones * 3, ones * 5, Cc, off * 0 + np.arange(7, dtype=np.int32),
                                           np.zeros((0, 2), np.float32), None, None)
    assert np.array_equal(ld, lc) and (ld == 3).all() and lost == 6


# ---- masks, ids outside the batch, the leading rule, the spawn shift -----------------------------------------------------
def test_masks_ids_leading_and_shift():
    from gym_traffic.devrng import car_list, put_cars
    E, R, Cc = 4, 23, 14
    x, v, w, arch, ld, lc, n = rings(3, E, R, Cc)
    ld, lc = ld.astype(np.int32), lc.astype(np.int32)
    b = blank(x, v, w, arch, ld, lc, 4)
    ids = [2, -1, 0, E]
    mask = (np.arange(R) % 3 != 1).astype(np.uint8)
    N, off, xv, road, row, spawn = car_list(x, v, w, arch, ld, lc, Cc, ids, mask)
    new_ld = np.stack([ld[2], ld[0], ld[0], ld[0]]).reshape(-1).copy()
    new_ld[0], new_ld[1] = 0, Cc                                              # no ring indices: those roads keep their own
    got = put_cars(*b, Cc, off, xv, row, spawn, env_ids=ids, road_mask=mask, new_leading=new_ld, het=True)
    assert got[6] == 0
    on = mask != 0
    for e in (1, 3):                                                          # not selected: untouched
        for g, q in zip(got[:6], b):
            assert np.array_equal(g[e], q[e])
    for e in (2, 0):
        for g, q in zip(got[:6], b):                                          # masked roads: untouched
            assert np.array_equal(g[e][~on], q[e][~on])
        want_ld = ld[e].copy()
        if e == 2:
            want_ld[:2] = b[4][2][:2]
        assert np.array_equal(got[4][e][on], want_ld[on])
        cnt = got[5][e] - got[4][e] + np.where(got[4][e] > got[5][e], Cc - 1, 0)
        assert np.array_equal(cnt[on], n[e][on])
    again = car_list(got[0], got[1], got[2], got[3], got[4], got[5], Cc, ids, mask)
    assert again[0] == N and all(a.tobytes() == q.tobytes() for a, q in zip(again[1:], (off, xv, road, row, spawn)))
    # the spawn shift: plain words move as floats, heterogeneous ones as integers modulo 2^24 with the row kept
    plain = put_cars(*b, Cc, off, xv, row, spawn, env_ids=ids, road_mask=mask, new_leading=new_ld, spawn_shift=-7)
    het = put_cars(*b, Cc, off, xv, row, spawn, env_ids=ids, road_mask=mask, new_leading=new_ld, spawn_shift=-7, het=True)
    m = live(got[4], got[5], Cc)
    m[[1, 3]] = False
    m[:, ~on] = False
    assert m.sum() == N
    assert np.array_equal(plain[2][m], got[2][m] - np.float32(7))
    assert np.array_equal(het[2][m], ((got[2][m].astype(np.int64) - 7) & 0xFFFFFF).astype(np.float32))
    assert (het[2][m] > 2 ** 23).any() and np.array_equal(het[3][m], got[3][m])       # a tick below 7 wraps
    far = put_cars(*b, Cc, off, xv, row, spawn, env_ids=ids, road_mask=mask, new_leading=new_ld, spawn_shift=2 ** 24 + 5,
                   het=True)
    assert np.array_equal(far[2][m], got[2][m] + np.float32(5))                # a whole turn of the 24-bit clock and 5
