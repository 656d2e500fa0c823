"""Demand profiles on the device (tfx_set_demand, rule 4 of include/tfx.h), the parts that need no GPU: the threshold
tables, the rule as a NumPy function (devrng.demand_counts - what tests/test_gpu_demand.py holds the device to) against a
plain-Python statement of it, its purity, its statistics with DERIVED bounds, the argument checks of the entry point that
are decided before any device work, and the binding."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "tfx.h")
LIB = os.path.join(ROOT, "traffic-env_amd", "lib", "libtfx_hip.so")
MASK = 0xFFFFFFFF


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        import subprocess
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "traffic-env_amd", "csrc")])
    return C.CDLL(LIB)


# ---- ABI -----------------------------------------------------------------------------------------------------------------
def test_header_declares_the_calls_and_the_struct_and_the_abi_stays_13():
    from gym_traffic import _native
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"int\s+tfx_set_demand\s*\(\s*tfx_handle\s+h\s*,\s*const\s+tfx_demand\s*\*\s*dm\s*\)\s*;", src)
    assert re.search(r"int\s+tfx_demand_counts\s*\(\s*tfx_handle\s+h\s*,\s*int32_t\s+tick0\s*,\s*int32_t\s+n_ticks\s*,\s*"
                     r"int32_t\s*\*\s*out\s*,\s*void\s*\*\s*stream\s*\)\s*;", src)
    body = re.search(r"typedef struct tfx_demand \{(.*?)\} tfx_demand;", src, re.S).group(1)
    names = []
    for decl in [d.strip() for d in body.split(";") if d.strip()]:
        decl = re.sub(r"^const\s+", "", decl)
        names += [n.strip().lstrip("*") for n in re.sub(r"^[a-z0-9_]+\s+", "", decl).split(",")]
    assert names == [f[0] for f in _native.TfxDemand._fields_]
    assert re.search(r"#define\s+TFX_ABI_VERSION\s+13\b", src)
    assert _native.ABI_VERSION == 13
    assert len(_native._PROTOS["tfx_set_demand"][1]) == 2 and len(_native._PROTOS["tfx_demand_counts"][1]) == 5
    # rule 4 is written down where rules 1-3 are, with its tags, and says what it is not
    text = open(HEADER).read()
    assert "Rule 4" in text and "0x44434E54" in text and "0x44524F44" in text and "TRUE per-tick Poisson" in text


def test_ctypes_struct_has_the_c_layout():
    from gym_traffic import _native
    S = _native.TfxDemand
    p = C.sizeof(C.c_void_p)
    assert p == 8
    assert [getattr(S, f[0]).offset for f in S._fields_] == [0, 4, 8, 12, 16, 24, 32, 40, 48]
    assert C.sizeof(S) == 56


def BAD_ARGS(nat, n_entry=None):
    """(tfx_demand, words its refusal must contain): every TFX_EINVAL that is decided before the handle is looked at -
    shared with tests/test_gpu_demand.py, which adds the ones that need a handle's n_entry"""
    good_cc = np.array([[1 << 30, 1 << 31, MASK], [5, 5, MASK]], np.uint32)            # K = 1, S = 2, n_cdf = 3
    good_rc = np.full((1, 2, n_entry or 4), MASK, np.uint32)
    keep = [good_cc, good_rc]

    def dm(**over):
        cc = np.ascontiguousarray(over.pop("cc", good_cc), np.uint32)
        rc = np.ascontiguousarray(over.pop("rc", good_rc), np.uint32)
        keep.extend([cc, rc])
        d = nat.TfxDemand()
        d.n_profiles, d.n_segments, d.seg_ticks, d.tick_offset, d.n_cdf = 1, 2, 5, 0, 3
        d.count_cdf, d.road_cdf = cc.ctypes.data_as(C.c_void_p), rc.ctypes.data_as(C.c_void_p)
        d.profile_of_env, d.seed = None, 1
        for k, v in over.items():
            setattr(d, k, v)
        return d

    cases = [(None, b"dm is null"),
             (dm(count_cdf=None), b"count_cdf is null"),
             (dm(road_cdf=None), b"road_cdf is null"),
             (dm(n_profiles=0), b"n_profiles 0"),
             (dm(n_profiles=17), b"n_profiles 17"),
             (dm(n_segments=0), b"n_segments 0"),
             (dm(n_segments=65), b"n_segments 65"),
             (dm(seg_ticks=0), b"seg_ticks 0"),
             (dm(seg_ticks=-3), b"seg_ticks -3"),
             (dm(n_cdf=0), b"n_cdf 0"),
             (dm(n_cdf=257), b"n_cdf 257"),
             (dm(seg_ticks=1 << 30), b"does not fit an int32"),                        # P = 2 * 2^30 = 2^31
             (dm(cc=[[9, 8, MASK], [5, 5, MASK]]), b"count_cdf row (0, 0) decreases at 1"),
             (dm(cc=[[1, 2, MASK], [5, 5, MASK - 1]]), b"count_cdf row (0, 1) does not end in 0xFFFFFFFF"),
             (dm(cc=[[1, 2, MASK], [5, MASK, 7]]), b"count_cdf row (0, 1) decreases at 2")]
    return dm, cases, keep


def test_calls_are_exported_and_argument_errors_are_codes(lib):
    """The arguments are checked before the handle, so each of these causes is reachable here, where no device - hence no
    handle - exists; with good arguments the NULL handle is the cause.  The road_cdf checks need the handle's n_entry,
    TFX_ESTATE needs a handle: tests/test_gpu_demand.py asserts those (and these again) on a live one."""
    from gym_traffic import _native as nat
    assert lib.tfx_abi_version() == 13
    fn = lib.tfx_set_demand
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.POINTER(nat.TfxDemand)]
    cnt = lib.tfx_demand_counts
    cnt.restype = C.c_int
    cnt.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    lib.tfx_last_error.restype = C.c_char_p
    dm, cases, keep = BAD_ARGS(nat)
    for d, msg in cases:
        assert fn(None, None if d is None else C.byref(d)) == -1, msg
        assert msg in lib.tfx_last_error(), (msg, lib.tfx_last_error())
    assert fn(None, C.byref(dm())) == -1 and b"null handle" in lib.tfx_last_error()
    assert fn(None, C.byref(dm(seg_ticks=(1 << 30) - 1))) == -1 and b"null handle" in lib.tfx_last_error()   # P = 2^31 - 2
    word = (C.c_int32 * 4)()
    assert cnt(None, 0, 1, None, None) == -1 and b"out is null" in lib.tfx_last_error()
    assert cnt(None, 0, -1, word, None) == -1 and b"n_ticks -1" in lib.tfx_last_error()
    assert cnt(None, 0, 1, word, None) == -1 and b"null handle" in lib.tfx_last_error()
    assert list(word) == [0, 0, 0, 0]
    assert keep


# ---- the tables ----------------------------------------------------------------------------------------------------------
def test_tables():
    from gym_traffic.devrng import demand_tables
    rng = np.random.RandomState(1)
    means = [[0.0, 0.48, 3.0], [70.0, 1e-3, 12.5]]
    weights = rng.rand(2, 3, 6)
    weights[0, 1, 2] = 0.0
    weights[1, 0, 0] = 0.0
    weights[1, 2, 5] = 0.0
    cc, rc = demand_tables(means, weights)
    K, S, n_cdf = cc.shape
    assert cc.dtype == np.uint32 and rc.dtype == np.uint32 and (K, S) == (2, 3) and rc.shape == (2, 3, 6)
    for tab in (cc, rc):
        t = tab.astype(np.int64)
        assert (np.diff(t, axis=-1) >= 0).all() and (t[..., -1] == MASK).all()
    # the entries are the definition's, computed here another way (math.fsum over the probability masses)
    import math
    for k in range(K):
        for s in range(S):
            lam, acc = means[k][s], []
            for c in range(n_cdf - 1):
                acc.append(math.exp(-lam + (c * math.log(lam) if lam > 0 else 0.0) - math.lgamma(c + 1)) if (lam > 0 or c == 0) else 0.0)
                want = min(int(math.fsum(acc) * 4294967296.0), MASK)
                assert abs(int(cc[k, s, c]) - want) <= 64, (k, s, c)          # binary64 sums in another order: 2^-26 relative
    # mean 0: every threshold is the last one's - N = 0 for every u0 but 0xFFFFFFFF itself
    assert (cc[0, 0] == MASK).all()
    # default n_cdf: the smallest whose tail mass is below 1e-12 for the largest mean (70), capped at 256
    tail = 1.0 - sum(math.exp(-70.0 + c * math.log(70.0) - math.lgamma(c + 1)) for c in range(n_cdf))
    tail_short = 1.0 - sum(math.exp(-70.0 + c * math.log(70.0) - math.lgamma(c + 1)) for c in range(n_cdf - 1))
    assert 64 + 1 < n_cdf <= 256 and tail < 1e-12 + 1e-14 and tail_short > 1e-12 - 1e-14, n_cdf
    assert demand_tables([[250.0]], n_entry=2).count_cdf.shape[2] == 256
    assert demand_tables([[0.0]], n_entry=2).count_cdf.shape[2] == 1
    assert demand_tables([[3.0]], n_entry=2, n_cdf=9).count_cdf.shape[2] == 9
    # equal weights; a weight vector for every profile and segment
    eq = demand_tables([[1.0]], n_entry=6).road_cdf[0, 0].astype(np.int64)
    assert eq.tolist() == [(j + 1) * 4294967296 // 6 for j in range(5)] + [MASK]
    one = demand_tables(means, [1, 0, 2, 3, 0, 4]).road_cdf
    assert (one == one[0, 0]).all() and one[0, 0, 1] == one[0, 0, 0] and one[0, 0, 4] == one[0, 0, 3]
    for bad in (dict(means=[1.0]), dict(means=[[-1.0]], n_entry=2), dict(means=[[1.0]]), dict(means=[[1.0]], weights=[0, 0]),
                dict(means=[[1.0]], weights=[1, -1]), dict(means=[[1.0]], n_entry=2, n_cdf=257),
                dict(means=[[1.0]], weights=[1, 1, 1], n_entry=2), dict(means=[[float("nan")]], n_entry=2)):
        with pytest.raises(ValueError):
            demand_tables(**bad)


def test_segments():
    from gym_traffic.devrng import demand_segment
    # S = 3 segments of 2 ticks: period 6; floor modulo for negative ticks
    got = demand_segment(np.arange(-7, 8), 3, 2, 0).tolist()
    assert got == [2, 0, 0, 1, 1, 2, 2, 0, 0, 1, 1, 2, 2, 0, 0]
    assert demand_segment(-1, 3, 2, 0) == 2 and demand_segment(5, 3, 2, 1) == 0 and demand_segment(0, 3, 2, -1) == 2
    # 64-bit: the largest clock tick plus the largest offset does not wrap
    big = demand_segment(2 ** 31 - 1, 4, 10, 2 ** 31 - 1)
    assert big == ((2 ** 32 - 2) % 40) // 10
    # the clock is an int32 that wraps: tick 2^31 is tick -2^31, as `clock + row` is on the device
    assert demand_segment(2 ** 31, 3, 2, 0) == demand_segment(-2 ** 31, 3, 2, 0) == ((-2 ** 31) % 6) // 2
    assert demand_segment(2 ** 31, 3, 2, 0) != ((2 ** 31) % 6) // 2


# ---- the rule ------------------------------------------------------------------------------------------------------------
def rule4(seed, g, t, cc, rc, k, seg_ticks, off):
    """Rule 4 of include/tfx.h for one (tick, env), line by line in plain Python"""
    from gym_traffic import devrng as d
    K, S, n_cdf = cc.shape
    ne = rc.shape[2]
    out = [0] * ne
    if not 0 <= k < K:
        return out
    P = S * seg_ticks
    s = ((t + off) % P) // seg_ticks                      # (Python's % is the floor modulo)
    k0, k1 = seed & MASK, seed >> 32
    u = d.philox4x32(t & MASK, g, d.TAG_DCNT, 0, k0, k1)
    N = sum(1 for c in range(n_cdf - 1) if u[0] >= int(cc[k, s, c]))
    for c in range(N):
        w = d.philox4x32(t & MASK, g, d.TAG_DROAD, c >> 2, k0, k1)[c & 3]
        out[sum(1 for j in range(ne - 1) if w >= int(rc[k, s, j]))] += 1
    return out


def test_model_is_rule_4_and_pure():
    from gym_traffic import devrng as d
    assert (d.TAG_DCNT, d.TAG_DROAD) == (0x44434E54, 0x44524F44)
    assert len({d.TAG_DCNT, d.TAG_DROAD, d.TAG_GAP, d.TAG_ROAD, d.TAG_ARCH, d.TAG_EPISODE, d.TAG_POOL}) == 7
    tb = d.demand_tables([[0.5, 70.0, 0.0], [2.0, 1.0, 9.0]], np.random.RandomState(0).rand(2, 3, 6))
    seed = (0xABCD << 32) | 77
    ticks, ids, prof = np.arange(-9, 5), np.arange(5) + 100, [0, 1, -1, 2, 1]
    kw = dict(seg_ticks=2, tick_offset=3)
    got = d.demand_counts(seed, ids, ticks, tb, prof, **kw)
    assert got.dtype == np.int32 and got.shape == (14, 5, 6)
    for i, t in enumerate(ticks):
        for e in range(5):
            assert got[i, e].tolist() == rule4(seed, int(ids[e]), int(t), tb.count_cdf, tb.road_cdf, prof[e], 2, 3), (t, e)
    assert not got[:, 2].any() and not got[:, 3].any()                  # profiles -1 and K: no cars
    assert (got[:, 0].sum(axis=1) > 64).any()                            # the mean-70 segment: more cars than lanes
    # any subset of envs or ticks, in any order, gives the same rows
    rng = np.random.RandomState(2)
    for _ in range(4):
        ti, ei = rng.permutation(14)[:rng.randint(1, 14)], rng.permutation(5)[:rng.randint(1, 5)]
        sub = d.demand_counts(seed, ids[ei], ticks[ti], tb, np.asarray(prof)[ei], **kw)
        assert np.array_equal(sub, got[ti][:, ei])
    assert np.array_equal(d.demand_counts(seed, ids[:1], ticks[3:4], tb, prof[:1], **kw), got[3:4, :1])
    assert d.demand_counts(seed, ids, [], tb, prof, **kw).shape == (0, 5, 6)
    wrapped = d.demand_counts(seed, ids, [2 ** 31 - 1, 2 ** 31, 2 ** 31 + 1], tb, prof, **kw)
    assert np.array_equal(wrapped, d.demand_counts(seed, ids, [2 ** 31 - 1, -2 ** 31, -2 ** 31 + 1], tb, prof, **kw))
    assert wrapped[1].tolist() == [rule4(seed, int(ids[e]), -2 ** 31, tb.count_cdf, tb.road_cdf, prof[e], 2, 3) for e in range(5)]
    # profile None is profile 0; another seed, stream id, or tick gives other cars
    assert np.array_equal(d.demand_counts(seed, ids, ticks, tb, None, **kw), d.demand_counts(seed, ids, ticks, tb, [0] * 5, **kw))
    base = d.demand_counts(seed, ids, ticks, tb, None, **kw)
    assert not np.array_equal(base, d.demand_counts(seed + 1, ids, ticks, tb, None, **kw))
    assert not np.array_equal(base, d.demand_counts(seed, ids + 1, ticks, tb, None, **kw))
    assert not np.array_equal(base[:, 0], base[:, 1])
    # the period: tick t and tick t + P see the same tables, not the same cars
    assert np.array_equal(d.demand_segment(ticks, 3, 2, 3), d.demand_segment(ticks + 6, 3, 2, 3))
    assert not np.array_equal(base, d.demand_counts(seed, ids, ticks + 6, tb, None, **kw))


@pytest.mark.parametrize("lam", [0.48, 3.0, 70.0])
def test_mean_is_the_poissons(lam):
    """T x E = 2000 x 50 independent Poisson(lam) samples: the sample mean has standard error sqrt(lam / (T E)); six of
    them is a 2e-9 event for a correct generator.  The variance of a Poisson is its mean: the sample variance of n
    samples has standard error sqrt((lam + 2 lam^2) / n) (fourth central moment lam + 3 lam^2), six again."""
    from gym_traffic.devrng import demand_counts, demand_tables
    T, E = 2000, 50
    tb = demand_tables([[lam]], n_entry=1)
    n = demand_counts(11, np.arange(E), np.arange(T), tb)[..., 0].astype(np.float64)
    se = np.sqrt(lam / (T * E))
    print("lambda %g: n_cdf %d, sample mean %.5f, %.2f standard errors off" % (lam, tb.count_cdf.shape[2], n.mean(), (n.mean() - lam) / se))
    assert abs(n.mean() - lam) <= 6 * se
    assert abs(n.var() - lam) <= 6 * np.sqrt((lam + 2 * lam * lam) / (T * E))
    # ticks are independent: the lag-1 correlation of an env's counts is 0 +- 1/sqrt(n)
    z = n - n.mean()
    assert abs((z[1:] * z[:-1]).mean() / n.var()) <= 6 / np.sqrt((T - 1) * E)


def test_road_shares_are_the_weights():
    """Given the total M, the cars on road j are Binomial(M, p_j): within 6 sqrt(M p_j (1 - p_j)) of M p_j; a road of
    weight zero gets none."""
    from gym_traffic.devrng import demand_counts, demand_tables
    w = np.array([1.0, 0.0, 2.0, 3.0, 0.0, 4.0])
    c = demand_counts(5, np.arange(50), np.arange(2000), demand_tables([[3.0]], w)).astype(np.int64)
    per_road, M = c.sum(axis=(0, 1)), int(c.sum())
    p = w / w.sum()
    print("cars", M, "per road", per_road.tolist())
    assert abs(M - 3.0 * 100000) <= 6 * np.sqrt(3.0 * 100000)
    assert (np.abs(per_road - M * p) <= 6 * np.sqrt(M * p * (1 - p))).all()
    assert per_road[1] == 0 and per_road[4] == 0


# ---- the GPU test's agent scenario on the CPU oracle ------------------------------------------------------------------------
# 2x2 grid with the first side closed (6 entry roads), 5 envs with global ids 40..44, capacity 6 (four cars per road), three
# 10-tick decisions; profile 0 is light, profile 1 heavy, env g holds phase (decision // (g + 1)) & 1.  The seed was picked
# with agent_scenario_on_the_oracle below: in the second AND in the third decision - the ones tests/test_gpu_demand.py runs
# on graph replay - some envs overflow part-way through the decision and some do not.
AGENT = dict(m=2, n=2, length=120.0, capacity=6, rate=0.5, entry_spec=1, E=5, off=40, T=10, decisions=3, seed=6,
             means=[[0.3, 0.6], [2.5, 1.5]], seg_ticks=7, tick_offset=-3, profiles=[1, 0, 1, 0, 1])


def agent_weights(n_entry):
    return np.stack([np.stack([1.0 + ((np.arange(n_entry) + k + s) % 3) for s in range(2)]) for k in range(2)])


def agent_actions(E, I, s, off=0):
    a = np.array([((s // (g + off + 1)) & 1) for g in range(E)], np.int32)
    return np.ascontiguousarray(np.repeat(a[:, None], I, axis=1))


def agent_scenario_on_the_oracle(sc=AGENT):
    """-> (stopped_at int [decisions, E]: the tick of the decision in which the env overflowed, -1 if it did not;
    counts int32 [decisions * T, E, n_entry], the mirrored rows).  `if done: break` on single-env oracles."""
    from gym_traffic import devrng
    from gym_traffic.envs.roadgraph import GridRoad
    from oracle.oracle import OracleEnv
    from test_measures_host import roads_of
    g = GridRoad(sc["m"], sc["n"], sc["length"])
    entry = g.generate_entrypoints(sc["entry_spec"])
    E, T, D = sc["E"], sc["T"], sc["decisions"]
    tables = devrng.demand_tables(sc["means"], agent_weights(len(entry)))
    counts = devrng.demand_counts(sc["seed"], np.arange(E) + sc["off"], np.arange(D * T), tables, sc["profiles"],
                                  seg_ticks=sc["seg_ticks"], tick_offset=sc["tick_offset"])
    orcs = [OracleEnv(sc["m"], sc["n"], sc["length"], sc["capacity"], g.dest, g.phases, g.nexts, rate=sc["rate"]) for _ in range(E)]
    stopped = np.full((D, E), -1)
    for k, orc in enumerate(orcs):
        orc.reset(np.zeros((1, orc.I), np.int32))
        for s in range(D):
            act = agent_actions(E, orc.I, s)[k:k + 1]
            for j in range(T):
                _, _, done = orc.step(act, roads_of(counts[s * T + j, k:k + 1], entry))
                if done[0]:
                    stopped[s, k] = j
                    break
    return stopped, counts


def test_agent_scenario_is_not_vacuous():
    stopped, counts = agent_scenario_on_the_oracle()
    print("overflow tick per decision and env:\n%s\ncars per env: %s" % (stopped, counts.sum(axis=(0, 2)).tolist()))
    for s in (1, 2):                                  # the decisions that run on graph replay
        mid = (stopped[s] >= 0) & (stopped[s] < AGENT["T"] - 1)
        assert mid.any() and (stopped[s] < 0).any(), (s, stopped[s])
