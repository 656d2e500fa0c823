"""Episodes on the device (tfx_set_episodes, include/tfx.h), the parts that need no GPU: the entry point and its
argument checks, the ctypes mirror of its struct, the host mirror of the on-device phase draw (rule 2 of tfx.h), and
the NumPy model of the per-decision accounting that tests/test_gpu_episodes.py holds the device to."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "tfx.h")
LIB = os.path.join(ROOT, "traffic-env_amd", "lib", "libtfx_hip.so")


class EpisodeModel(object):
    """Step 3 of tfx_set_episodes in NumPy: feed it every decision's (areward, adone) in order."""

    def __init__(self, E, I, max_decisions=0):
        self.max = int(max_decisions or 0)
        self.ep_return = np.zeros((E, I), np.float32)
        self.final_return = np.zeros((E, I), np.float32)
        self.ep_len = np.zeros(E, np.int32)
        self.final_len = np.zeros(E, np.int32)
        self.ep_index = np.zeros(E, np.int32)
        self.truncated = np.zeros(E, np.uint8)

    def decision(self, areward, adone):
        """Accounts for one decision; returns the bool mask of the envs whose episode it ended."""
        self.ep_return += np.asarray(areward, np.float32)          # one float32 add per element, in decision order
        self.ep_len += 1
        term = np.asarray(adone) != 0
        trunc = ~term & (self.max > 0) & (self.ep_len == self.max)
        end = term | trunc
        self.final_return[end] = self.ep_return[end]
        self.final_len[end] = self.ep_len[end]
        self.ep_return[end] = 0
        self.ep_len[end] = 0
        self.ep_index[end] += 1
        self.truncated = trunc.astype(np.uint8)
        return end

    def abandon(self, mask):
        """tfx_reset / tfx_reset_envs from outside: the accumulators of those envs cleared, ep_index unmoved."""
        mask = np.asarray(mask).astype(bool)
        self.ep_return[mask] = 0
        self.ep_len[mask] = 0


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import subprocess
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "traffic-env_amd", "csrc")])
    return C.CDLL(LIB)


def test_set_episodes_is_exported_and_errors_are_codes(lib):
    from gym_traffic import _native
    assert hasattr(lib, "tfx_set_episodes")
    fn = lib.tfx_set_episodes
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_uint64, C.POINTER(_native.TfxEpisodeBuffers)]
    lib.tfx_last_error.restype = C.c_char_p
    good = _native.TfxEpisodeBuffers()
    keep = (C.c_char * 64)()
    for name, _ in _native.TfxEpisodeBuffers._fields_:
        setattr(good, name, C.addressof(keep))
    # a null handle
    assert fn(None, 1, 5, 0, C.byref(good)) == -1
    assert b"null handle" in lib.tfx_last_error()
    assert fn(None, 0, 0, 0, None) == -1
    # a negative limit
    assert fn(None, 1, -1, 0, C.byref(good)) == -1
    assert b"max_decisions" in lib.tfx_last_error()
    # null buffers: the struct itself, and any one member
    assert fn(None, 1, 5, 0, None) == -1
    assert b"null episode buffers" in lib.tfx_last_error()
    for name, _ in _native.TfxEpisodeBuffers._fields_:
        b = _native.TfxEpisodeBuffers()
        for other, _ in _native.TfxEpisodeBuffers._fields_:
            setattr(b, other, None if other == name else C.addressof(keep))
        assert fn(None, 1, 5, 0, C.byref(b)) == -1, name
        assert b"required" in lib.tfx_last_error()


def test_episode_struct_layout_matches_header():
    from gym_traffic import _native
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct tfx_episode_buffers \{(.*?)\} tfx_episode_buffers;", src, re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            fields += [n.strip().lstrip("*") for n in re.sub(r"^[a-z0-9_]+\s+", "", decl).split(",")]
    assert fields == [f[0] for f in _native.TfxEpisodeBuffers._fields_]
    assert fields == ["ep_return", "ep_len", "final_return", "final_len", "truncated", "ep_index"]
    assert "tfx_set_episodes" in _native._PROTOS
    assert _native.ABI_VERSION == 13


def test_episode_phases_known_answer():
    """Rule 2 of include/tfx.h, spelt out here with devrng.philox4x32 alone: the phase of intersection i in episode
    number n of global env g is bit 0 of the first word of philox4x32({n, g, 0x45504953, i}, key = seed)."""
    from gym_traffic import devrng
    text = open(HEADER).read()
    assert "TAG_EPISODE = 0x45504953" in text and "ctr = {n, g, TAG_EPISODE, i}" in text and "u0 & 1" in text
    assert 0x45504953 not in (0x47415021, 0x524F4144, 0x41524348)
    seed, g, n, I = 0x1234567890ABCDEF, 4099, 3, 9
    want = [devrng.philox4x32(n, g, 0x45504953, i, seed & 0xFFFFFFFF, seed >> 32)[0] & 1 for i in range(I)]
    got = devrng.episode_phases(seed, [g], n, I)
    assert got.dtype == np.int32 and got.shape == (1, I)
    assert got[0].tolist() == want
    assert 0 < sum(want) < I                      # (this vector has both values)


def test_episode_phases_is_a_pure_function_of_its_key():
    from gym_traffic import devrng
    E, I, seed = 64, 16, 11
    rng = np.random.RandomState(0)
    n = rng.randint(1, 9, size=E)
    whole = devrng.episode_phases(seed, np.arange(E), n, I)
    assert whole.shape == (E, I) and set(np.unique(whole).tolist()) == {0, 1}
    # a sharded call equals the slice of the whole
    for lo, hi in ((0, 32), (32, 64), (17, 23)):
        assert np.array_equal(devrng.episode_phases(seed, np.arange(lo, hi), n[lo:hi], I), whole[lo:hi])
    # a scalar episode number broadcasts; every part of the key matters
    same_n = devrng.episode_phases(seed, np.arange(E), 2, I)
    assert np.array_equal(same_n[5], devrng.episode_phases(seed, [5], [2], I)[0])
    assert not np.array_equal(same_n, devrng.episode_phases(seed, np.arange(E), 3, I))
    assert not np.array_equal(same_n, devrng.episode_phases(seed + 1, np.arange(E), 2, I))
    assert not np.array_equal(same_n, devrng.episode_phases(seed, np.arange(E) + E, 2, I))
    # a wider grid only appends intersections
    assert np.array_equal(devrng.episode_phases(seed, np.arange(E), 2, 2 * I)[:, :I], same_n)
    assert abs(float(whole.mean()) - 0.5) < 0.1


def test_accounting_model():
    m = EpisodeModel(3, 2, max_decisions=3)
    r = np.array([[1, 2], [0.5, 0.25], [-1, 0]], np.float32)
    assert not m.decision(r, [0, 0, 0]).any()
    assert m.decision(r, [0, 1, 0]).tolist() == [False, True, False]
    assert m.truncated.tolist() == [0, 0, 0] and m.ep_index.tolist() == [0, 1, 0]
    assert m.final_return[1].tolist() == [1.0, 0.5] and m.final_len[1] == 2 and m.ep_len.tolist() == [2, 0, 2]
    end = m.decision(r, [0, 0, 1])
    assert end.tolist() == [True, False, True] and m.truncated.tolist() == [1, 0, 0]      # overflow wins over the limit
    assert m.final_return[0].tolist() == [3.0, 6.0] and m.final_len.tolist() == [3, 2, 3]
    assert m.ep_return[1].tolist() == [0.5, 0.25] and m.ep_len.tolist() == [0, 1, 0] and m.ep_index.tolist() == [1, 1, 1]
    m.abandon([False, True, False])
    assert m.ep_len.tolist() == [0, 0, 0] and not m.ep_return.any() and m.ep_index.tolist() == [1, 1, 1]
    free = EpisodeModel(1, 1)                                      # no limit: overflow only
    for _ in range(50):
        assert not free.decision([[1.0]], [0]).any()
    assert free.ep_len[0] == 50 and free.truncated[0] == 0


def test_vec_env_rejects_episode_len_without_autoreset():
    from gym_traffic.envs.vec_env import TrafficVecEnv
    with pytest.raises(ValueError):
        TrafficVecEnv(2, 2, 2, 100.0, episode_len=5)
