"""Warm restarts (tfx_set_episode_pool, include/tfx.h), the parts that need no GPU: rule 3 as a NumPy function
(devrng.episode_pool_slots - what tests/test_gpu_warm_pool.py holds the device to) against devrng's own Philox on the
stated counter, the entry point in the header, the binding and the built library."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "tfx.h")
LIB = os.path.join(ROOT, "traffic-env_amd", "lib", "libtfx_hip.so")
TAG_POOL = 0x504F4F4C


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import subprocess
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "traffic-env_amd", "csrc")])
    return C.CDLL(LIB)


def direct(seed, g, n, n_pool):
    """rule 3 spelt out for one env: (u0 * n_pool) >> 32, u = philox4x32({n, g, TAG_POOL, 0}, seed)"""
    from gym_traffic import devrng
    u0 = devrng.philox4x32(n & 0xFFFFFFFF, g, TAG_POOL, 0, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)[0]
    return (u0 * n_pool) >> 32


def test_the_tag_is_new():
    from gym_traffic import devrng
    assert devrng.TAG_POOL == TAG_POOL
    assert len({devrng.TAG_GAP, devrng.TAG_ROAD, devrng.TAG_ARCH, devrng.TAG_EPISODE, devrng.TAG_POOL}) == 5


@pytest.mark.parametrize("n_pool", [1, 3, 64, 4096])
def test_slots_equal_the_stated_counter_and_stay_in_range(n_pool):
    from gym_traffic import devrng
    rng = np.random.RandomState(11)
    for seed in (0, 3, 0x123456789ABCDEF0, 2 ** 64 - 1):
        ids = np.concatenate([np.arange(8), rng.randint(0, 2 ** 31 - 1, size=24), [2 ** 30, 2 ** 31 - 1]])
        eps = np.concatenate([np.arange(8), rng.randint(0, 2 ** 31 - 1, size=26)])
        got = devrng.episode_pool_slots(seed, ids, eps, n_pool)
        assert got.dtype == np.int32 and got.shape == (len(ids),)
        assert got.min() >= 0 and got.max() < n_pool
        assert got.tolist() == [direct(seed, int(g), int(n), n_pool) for g, n in zip(ids, eps)]
        # a scalar episode number is broadcast over the envs
        assert devrng.episode_pool_slots(seed, ids, 5, n_pool).tolist() == [direct(seed, int(g), 5, n_pool) for g in ids]


def test_slots_do_not_depend_on_sharding():
    from gym_traffic import devrng
    ids, eps = np.arange(8) + 40, np.array([0, 3, 1, 1, 7, 2, 0, 9])
    whole = devrng.episode_pool_slots(3, ids, eps, 3)
    parts = np.concatenate([devrng.episode_pool_slots(3, ids[:3], eps[:3], 3), devrng.episode_pool_slots(3, ids[3:], eps[3:], 3)])
    assert np.array_equal(whole, parts)


def test_every_slot_occurs_and_both_counters_matter():
    from gym_traffic import devrng
    by_env = devrng.episode_pool_slots(3, np.arange(4096), 1, 3)
    by_episode = devrng.episode_pool_slots(3, np.full(4096, 5), np.arange(4096), 3)
    for draws in (by_env, by_episode):
        assert sorted(set(draws.tolist())) == [0, 1, 2]
        assert np.bincount(draws, minlength=3).min() > 4096 // 6          # (roughly a third each)
    assert not np.array_equal(by_env, by_episode)
    assert not np.array_equal(by_env, devrng.episode_pool_slots(4, np.arange(4096), 1, 3))     # ... and the seed


def test_header_declares_the_call_and_the_abi_stays():
    from gym_traffic import _native
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"int\s+tfx_set_episode_pool\s*\(\s*tfx_handle\s+h\s*,\s*tfx_handle\s+pool\s*\)\s*;", src)
    assert re.search(r"#define\s+TFX_ABI_VERSION\s+13\b", src)
    assert "0x504F4F4C" in text and "Rule 3" in text
    assert _native.ABI_VERSION == 13
    assert "tfx_set_episode_pool" in _native._PROTOS and len(_native._PROTOS["tfx_set_episode_pool"][1]) == 2


def test_the_call_is_exported_and_errors_are_codes(lib):
    assert lib.tfx_abi_version() == 13
    fn = lib.tfx_set_episode_pool
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p]
    lib.tfx_last_error.restype = C.c_char_p
    assert fn(None, None) == -1
    assert b"null handle" in lib.tfx_last_error()
