"""Clone env states on the device (tfx_clone_envs, include/tfx.h), the parts that need no GPU: the two entry points and
their argument checks, the binding, the in-place rule as a NumPy function (devrng.clone_plan - what
tests/test_gpu_clone.py holds the device to), and the copy of host-replayed arrival streams."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "tfx.h")
LIB = os.path.join(ROOT, "traffic-env_amd", "lib", "libtfx_hip.so")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import subprocess
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "traffic-env_amd", "csrc")])
    return C.CDLL(LIB)


def test_header_declares_the_clone_calls_and_flags():
    from gym_traffic import _native
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"int\s+tfx_clone_envs\s*\(\s*tfx_handle\s+dst\s*,\s*tfx_handle\s+src\s*,\s*const\s+int32_t\s*\*\s*"
                     r"src_of_env\s*,\s*int32_t\s+flags\s*,\s*void\s*\*\s*stream\s*\)\s*;", src)
    assert re.search(r"int\s+tfx_clone_skipped\s*\(\s*tfx_handle\s+h\s*,\s*uint64_t\s*\*\s*skipped\s*,\s*void\s*\*\s*stream\s*\)\s*;", src)
    assert re.search(r"enum\s*\{\s*TFX_CLONE_STREAM\s*=\s*1\s*,\s*TFX_CLONE_EPISODE\s*=\s*2\s*\}", src)
    assert re.search(r"#define\s+TFX_ABI_VERSION\s+13\b", src)
    assert "tfx_clone_envs" in _native._PROTOS and "tfx_clone_skipped" in _native._PROTOS
    assert len(_native._PROTOS["tfx_clone_envs"][1]) == 5 and len(_native._PROTOS["tfx_clone_skipped"][1]) == 3
    assert (_native.CLONE_STREAM, _native.CLONE_EPISODE) == (1, 2)
    assert _native.ABI_VERSION == 13


def test_clone_calls_are_exported_and_errors_are_codes(lib):
    assert lib.tfx_abi_version() == 13
    fn = lib.tfx_clone_envs
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    sk = lib.tfx_clone_skipped
    sk.restype = C.c_int
    sk.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.c_void_p]
    lib.tfx_last_error.restype = C.c_char_p
    idx = (C.c_int32 * 4)(-1, -1, -1, -1)
    assert fn(None, None, idx, 0, None) == -1
    assert b"null handle" in lib.tfx_last_error()
    assert fn(None, None, idx, 3, None) == -1
    assert fn(None, None, None, 0, None) == -1
    assert b"src_of_env" in lib.tfx_last_error()
    assert fn(None, None, idx, 4, None) == -1
    assert b"flags" in lib.tfx_last_error()
    n = C.c_uint64(7)
    assert sk(None, C.byref(n), None) == -1
    assert b"null handle" in lib.tfx_last_error() and n.value == 7


def test_clone_plan_known_answers():
    from gym_traffic.devrng import clone_plan
    # nothing asked
    a, s = clone_plan([-1, -1, -1])
    assert a.tolist() == [False] * 3 and s == 0
    # a fan-out from untouched sources
    a, s = clone_plan([-1, 0, 0, -1, 3])
    assert a.tolist() == [False, True, True, False, True] and s == 0
    # a chain 0 <- 1 <- 2: env 1 takes env 0 (untouched); env 2's source, env 1, is itself overwritten
    a, s = clone_plan([-1, 0, 1])
    assert a.tolist() == [False, True, False] and s == 1
    # cycles: a swap, and a ring of three - nobody moves
    a, s = clone_plan([1, 0])
    assert a.tolist() == [False, False] and s == 2
    a, s = clone_plan([1, 2, 0, -1])
    assert a.tolist() == [False, False, False, False] and s == 3
    # a self-reference is applied (a copy of itself), and a self-referencing env may serve as a source
    a, s = clone_plan([0, 0, -1])
    assert a.tolist() == [True, True, False] and s == 0
    # out of range on either side: left alone and counted; an env whose source has an out-of-range wish is skipped too
    a, s = clone_plan([-1, 5, -2, 1])
    assert a.tolist() == [False, False, False, False] and s == 3
    a, s = clone_plan([3, -1, 1, -7])
    assert a.tolist() == [False, False, True, False] and s == 2
    # another source handle: only the range counts
    a, s = clone_plan([1, 0, 2, 3, -1], n_src=3)
    assert a.tolist() == [True, True, True, False, False] and s == 1
    # a randomised cross-check against the rule spelt out env by env
    rng = np.random.RandomState(5)
    for _ in range(50):
        E = int(rng.randint(1, 40))
        src = rng.randint(-3, E + 2, size=E)
        want = [0 <= s_ < E and (src[s_] == -1 or src[s_] == s_) for s_ in src]
        a, s = clone_plan(src)
        assert a.tolist() == want and s == sum(1 for k in range(E) if src[k] != -1 and not want[k])


def _streams(E, poisson=True, **kw):
    from gym_traffic.spawner import ArrivalStreams
    entry = [0, 3, 5, 6]
    return ArrivalStreams([100 + k for k in range(E)], poisson, entry, {0: 0, 3: 1, 5: 2, 6: 3}, 4, 0.7, **kw)


@pytest.mark.parametrize("poisson", [True, False])
def test_arrival_streams_copy(lib, poisson):
    """After copying stream 3 onto stream 5 both yield the same next_ticks forever, stream 4 is unaffected."""
    a, ref = _streams(8, poisson), _streams(8, poisson)
    for s in (a, ref):
        s.next_ticks(13)
    a.copy_streams([-1, -1, -1, -1, -1, 3, -1, -1])
    diverged = False
    for n in (1, 7, 40, 200):
        ca, ma = [x.copy() for x in a.next_ticks(n)]
        cr, mr = [x.copy() for x in ref.next_ticks(n)]
        assert np.array_equal(ca[:, 5], ca[:, 3]) and np.array_equal(ma[:, 5], ma[:, 3])
        keep = [0, 1, 2, 3, 4, 6, 7]
        assert np.array_equal(ca[:, keep], cr[:, keep]) and np.array_equal(ma[:, keep], mr[:, keep])
        diverged |= not np.array_equal(ca[:, 5], cr[:, 5])
    assert diverged or not poisson          # (stream 5 no longer replays what it would have)
    assert np.array_equal(a.random_state(5).get_state()[1], a.random_state(3).get_state()[1])
    assert np.array_equal(a.random_state(4).get_state()[1], ref.random_state(4).get_state()[1])


def test_arrival_streams_copy_between_objects_and_rows(lib):
    """From another ArrivalStreams object, several destinations per source, with archetype rows; sources are read
    before anything is written (a chain copies the OLD state)."""
    a, b = _streams(6, n_archetypes=3, per_road=4), _streams(6, n_archetypes=3, per_road=4)
    b.next_ticks(9)
    a.next_ticks(2)
    a.copy_streams([2, 2, -1, 0, -1, 5], source=b)
    ca, ma, ra = [x.copy() for x in a.next_ticks(60)]
    cb, mb, rb = [x.copy() for x in b.next_ticks(60)]
    for k, s in ((0, 2), (1, 2), (3, 0), (5, 5)):
        assert np.array_equal(ca[:, k], cb[:, s]) and np.array_equal(ra[:, k], rb[:, s]), (k, s)
    c = _streams(3)
    c.next_ticks(5)
    before1 = c.random_state(1).get_state()[1].copy()
    c.copy_streams([-1, 0, 1])
    assert np.array_equal(c.random_state(2).get_state()[1], before1)
    with pytest.raises(IndexError):
        c.copy_streams([7, -1, -1])
