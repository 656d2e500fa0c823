"""The arrival kernels at every launch form and table limit: k_poisson (csrc/tfx_misc.hpp), k_demand (csrc/tfx_demand.hpp)
and the Poisson block of k_res (csrc/tfx_resident.hpp), each against the host statement of its rule in gym_traffic/devrng.py
and the oracle fed the mirrored counts and rows.  Every comparison is exact.

  A  k_poisson at its three workgroup sizes (1024 lanes up to 64 envs, 256 up to 1024, 64 beyond): bursts that take two and
     three rounds of the burst loop at 64 and 256 lanes, the pair walk of the archetype rows with more rows per road than
     lanes, 66 entry roads (a second stride of every n_entry loop at 64 lanes), the regular stream with burst > lanes.
     Rates and seeds: tests/test_arrival_forms_host.py:CASES, where the condition each case is there for is asserted on
     the mirror alone.
  B  k_demand through the previews against devrng.demand_counts / demand_rows: 66 and 2048 entry roads, n_cdf = 256, 16
     profiles, 64 segments, 64 archetype rows, rows kept per road below and above the cars a road takes.
  C  a world of 66 entry roads on every step path (k_res in two packings, the two-tick passes with k_tail in two halves,
     the per-tick kernels) under every stream kind.
  D  0.02 cars per tick: a gap table of more than a thousand thresholds and countdowns of hundreds of ticks.

Between the plain calls and the decisions of a group-A case every third env is reset (tfx_reset_envs; the streams run on):
at these rates every ring is full after ten ticks, so without it every env would overflow - and stand still - in the first
tick of a decision, and no launch of k_poisson would see an env that stands still next to one that draws."""
import numpy as np
import pytest

from oracle.oracle import LI, S0I
from test_arrival_forms_host import (CASES, DECISIONS, DEMAND_E, DEMAND_OFF, DEMAND_SEED, LOW, MANY, MANY_MEANS, MAX, MAX_CDF,
                                     MAX_K, MAX_PROFILES, MAX_RANGE, MAX_ROWS, MAX_S, PLAIN_CALLS, SMALL, SMALL_MEANS,
                                     SMALL_PROFILE, SMALL_RANGES, WORLDS, FastPoisson, FastRegular, case_mirror, lanes_of,
                                     max_means, max_mirror, max_row_weights, max_tables, road_weights)
from test_gpu_fused import engine_with
from test_gpu_parity import assert_same_state, oracle_like
from test_gpu_stride_rounds import (ORC_FIELDS, assert_cars_wide, assert_decision, csr, emulate_decision, greedy_actions, live_all,
                                    rows_of, tab10_of)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from gym_traffic import _native as nat  # noqa: E402
from gym_traffic import devrng  # noqa: E402

PERTICK = {"TFX_RESIDENT": "0", "TFX_PAIRS": "0", "TFX_TAIL": "2", "TFX_SPLIT": "2"}
PAIRS = {"TFX_RESIDENT": "0", "TFX_PAIRS": "2", "TFX_TAIL": "2", "TFX_SPLIT": "2"}
# v, l, a, delta, v0, b, T, s0: the reference's car, a long slow truck, a short quick car
TAB3 = np.array([[11.11, 4, 3, 4, 13.89, 6, 2, 1], [8.0, 8, 1.5, 4, 10.0, 4, 2.5, 2], [12.0, 3.5, 4, 2, 16.0, 7, 1.5, 1]], np.float32)


def table64():
    """TFX_MAX_ARCH = 64 rows, no two alike in (l, a, delta, v0, b, T, s0)"""
    i = np.arange(64)
    t = np.zeros((64, 8), np.float32)
    t[:, 0] = 11.11
    t[:, 1] = 3.5 + (i % 8) * 0.5
    t[:, 2] = 1.5 + ((i // 8) % 4) * 0.75
    t[:, 3] = np.array([4.0, 2.0, 1.0, 4.0])[i % 4]
    t[:, 4] = 10.0 + (i // 32) * 3.0 + (i % 4)
    t[:, 5] = 4.0 + (i % 3)
    t[:, 6] = 1.5 + (i % 5) * 0.25
    t[:, 7] = 1.0 + (i % 2)
    assert len({tuple(r[1:]) for r in t.tolist()}) == 64
    return t


def table(n_rows):
    return TAB3 if n_rows == 3 else table64()


def padded(cnt, rows):
    """cars past the S rows held per road overflow: row 0 (devrng.cars_of)"""
    if rows is not None and rows.shape[-1] < int(cnt.max()):
        rows = np.concatenate([rows, np.zeros(rows.shape[:2] + (int(cnt.max()) - rows.shape[-1],), np.uint8)], axis=2)
    return cnt, rows


def mirror_tick(mirror, het, frozen=None):
    got = mirror.next_tick(frozen=frozen)
    return padded(*(got if het else (got, None)))


def oracle_tick(orc, act, cnt, rows, tab10, entrypoints):
    off, roads = csr(cnt, entrypoints)
    return orc.step(act, (off, roads), nthreads=8, spawn_arch=rows_of(cnt, rows, off) if rows is not None else None,
                    archetypes=tab10)[2].astype(bool)


def assert_words(eng, orc, where, obs=True):
    """ring indices and, after plain calls, the observation words and the rewards of every env.  The rewards of a call's
    last tick hold the overflow penalty of every car a full ring refused: where the rings are saturated and the state no
    longer tells 60 cars on a road from 61, they still do."""
    for name in ("leading", "lastcar") + (("obs", "rewards") if obs else ()):
        got, want = getattr(eng, name).cpu().numpy(), getattr(orc, name)
        if name == "rewards":
            got, want = got.view(np.int32), want.view(np.int32)
        bad = np.nonzero((got != want).reshape(eng.E, -1).any(axis=1))[0]
        assert bad.size == 0, "%s: %d envs differ, first %s %s" % (name, bad.size, bad[:8], where)


def assert_rows_wide(eng, orc, tab10, where):
    """every live car's archetype row: the oracle's car equals the table row the device names, in every parameter"""
    ld, lc = eng.leading.cpu().numpy(), eng.lastcar.cpu().numpy()
    live = live_all(ld, lc, eng.C)
    a = eng.arch.cpu().numpy().astype(np.int64)
    cols = list(range(LI, S0I + 1))
    got = np.transpose(orc.state[:, :, cols, :], (0, 1, 3, 2))              # [E, R, C, 7]
    want = np.asarray(tab10, np.float32)[a][..., cols]
    bad = np.nonzero(((got != want).any(axis=3) & live).reshape(eng.E, -1).any(axis=1))[0]
    assert bad.size == 0, "rows: %d envs differ, first %s %s" % (bad.size, bad[:8], where)
    return np.bincount(a[live], minlength=len(tab10))


def reset_some(eng, orc, mask, ph):
    eng.reset_envs(mask, ph)
    keep = [getattr(orc, f)[~mask].copy() for f in ORC_FIELDS]
    orc.reset(ph)
    for f, a in zip(ORC_FIELDS, keep):
        getattr(orc, f)[~mask] = a


# ---- A. k_poisson at its three widths -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["pertick", "pairs"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_poisson_kernel_at_every_width(name, path):
    """step(1) x 3, step(7) - a call's rows drawn up front, n_ticks > 1 -, then two agent_step(5, remi=True), the
    n_ticks == 1 form, in which envs that overflowed stand still and consume nothing.  After every call every env's ring
    indices, observation, rewards and done flags against the oracle under the mirrored stream; at the end waiting and
    every live car's x, v and archetype row, bit for bit."""
    c = CASES[name]
    E, het = c["E"], c["rows"] > 1
    tab8 = table(c["rows"]) if het else None
    tab10 = tab10_of(tab8) if het else None
    eng = engine_with(PERTICK if path == "pertick" else PAIRS, E, planes=3 if het else 2, env_id_offset=c["off"],
                      archetypes=tab8, **WORLDS[c["world"]])
    assert eng.fused_ticks() == (0, False) and eng.het == het
    orc = oracle_like(eng)
    orc.entrypoints = eng.entrypoints
    ph = np.zeros((E, eng.I), np.int32)
    eng.reset(ph)
    orc.reset(ph)
    if c["stream"] == "poisson":
        eng.set_poisson(c["cpt"], seed=c["seed"])
    else:
        eng.set_regular(c["cpt"], seed=c["seed"])
    mirror = case_mirror(name)
    assert mirror.n_entry == eng.n_entry and lanes_of(E) in (64, 256, 1024)
    rng = np.random.RandomState(len(name) + E)
    t, arrived = 0, np.zeros(eng.n_entry, np.int64)
    for k in PLAIN_CALLS:
        act = rng.randint(2, size=(E, eng.I)).astype(np.int32)
        eng.set_actions(act)
        eng.step(k)
        done = np.zeros(E, bool)
        for _ in range(k):
            cnt, rows = mirror_tick(mirror, het)
            done |= oracle_tick(orc, act, cnt, rows, tab10, eng.entrypoints)
            t += 1
        where = "%s %s tick %d" % (name, path, t)
        assert_words(eng, orc, where)
        assert np.array_equal(eng.done.cpu().numpy().astype(bool), done), "done " + where
        arrived += (eng.cars_on_roads_flat().cpu().numpy()[:, eng.entrypoints] > 0).sum(axis=0)
    # cars were refused at full rings (an env is done when a ring refuses a car), and cars arrived on every entry road
    assert int((eng.done_tick.cpu().numpy() > 0).sum()) > E // 2 and (arrived > 0).all()
    reset_some(eng, orc, np.arange(E) % 3 == 1, ph)
    mixed = False
    for T in DECISIONS:
        act = rng.randint(2, size=(E, eng.I)).astype(np.int32)
        eng.set_actions(act)
        tick0 = eng.tick
        out = eng.agent_step(T, remi=True)
        want = emulate_decision(orc, tick0, act, lambda j, frozen: mirror_tick(mirror, het, frozen.copy()), T, True, tab10,
                                nthreads=8)
        t += T
        where = "%s %s decision to tick %d" % (name, path, t)
        aobs, arew, adone = [o.cpu().numpy() for o in out]
        assert np.array_equal(adone, want[2]), "adone " + where
        assert np.array_equal(aobs.view(np.int32), want[0].view(np.int32)), "aobs " + where
        assert_words(eng, orc, where, obs=False)
        ends = want[3]
        # an env that stands still next to one that draws, in one launch of k_poisson: some envs ended in the decision's
        # first tick, others later or not at all
        mixed = mixed or bool((ends == 0).any() and (ends != 0).any())
        assert adone.any()
    assert mixed
    # the end: what the last decision returned and left behind
    assert np.array_equal(arew.view(np.int32), want[1].view(np.int32)), "areward " + where
    assert np.array_equal(eng.rewards.cpu().numpy().view(np.int32), orc.rewards.view(np.int32)), "rewards " + where
    assert np.array_equal(eng.waiting.cpu().numpy(), orc.waiting), "waiting " + where
    assert np.array_equal(eng.passed_dst.cpu().numpy(), orc.passed_dst), "passed_dst " + where
    assert_cars_wide(eng, orc, eng.leading.cpu().numpy(), eng.lastcar.cpu().numpy(), where)
    if het:
        seen = assert_rows_wide(eng, orc, tab10, where)
        assert (seen > 0).all() if c["stream"] == "poisson" else not seen[1:].any()
    assert eng.tick == t == sum(PLAIN_CALLS) + sum(DECISIONS)
    assert eng.fused_ticks()[0] == 0 and (eng.pair_ticks() > 0) == (path == "pairs")


# ---- B. k_demand against the rule, through the previews -----------------------------------------------------------------------
def demand_engine(world, E=DEMAND_E, off=DEMAND_OFF, rows=0, **grid):
    tab8 = table(rows) if rows else None
    return engine_with({}, E, planes=3 if rows else 2, env_id_offset=off, archetypes=tab8, **dict(WORLDS[world], **grid))


def on_device(a, eng):
    return torch.as_tensor(np.asarray(a, np.int32)).to(eng.device)


@pytest.mark.parametrize("mixed", [False, True])
def test_demand_small_table_on_66_entry_roads(mixed):
    """n_cdf = 137, K = 2, S = 3 on the 1 x 32 world: a second lane stride over the road thresholds, the histogram and the
    row that leaves; plain, and mixed with three archetype rows (C = 14: 12 rows kept per road)."""
    eng = demand_engine("line", rows=3 if mixed else 0, capacity=14)
    w = road_weights(66, 2, 3, seed=1)
    eng.set_demand(SMALL_MEANS, w, seed=DEMAND_SEED, profile_of_env=on_device(SMALL_PROFILE, eng),
                   row_weights=[1.0, 0.5, 2.0] if mixed else None, **SMALL)
    assert eng.n_entry == 66 and eng.demand_tables.count_cdf.shape == (2, 3, 137)
    ids = np.arange(DEMAND_E) + DEMAND_OFF
    past = 0
    for tick0, n in SMALL_RANGES:
        ticks = np.arange(tick0, tick0 + n)
        got = eng.demand_counts(tick0, n).cpu().numpy()
        want = devrng.demand_counts(DEMAND_SEED, ids, ticks, eng.demand_tables, SMALL_PROFILE, **SMALL)
        assert got.dtype == np.int32 and np.array_equal(got, want), (tick0, n, np.argwhere(got != want)[:5])
        past += int(want[..., 64:].sum())
        if mixed:
            assert eng.demand_rows_per_road == 12
            gc, gr = [a.cpu().numpy() for a in eng.demand_rows(tick0, n)]
            wc, wr = devrng.demand_rows(DEMAND_SEED, ids, ticks, eng.demand_tables, eng.demand_row_cdf, 12, SMALL_PROFILE, **SMALL)
            live = np.arange(12) < np.minimum(wc, 12)[..., None]
            assert np.array_equal(gc, wc) and np.array_equal(wc, want)
            assert np.array_equal(gr[live], wr[live]) and not gr[~live].any(), (tick0, n)
    want = devrng.demand_counts(DEMAND_SEED, ids, np.arange(3, 10), eng.demand_tables, SMALL_PROFILE, **SMALL)
    assert (want[:, 0].sum(axis=1) > 64).any() and (want[:, 0].sum(axis=1) == 0).any() and past > 0
    assert not want[:, 2].any() and not want[:, 3].any()                    # profiles -1 and K


@pytest.mark.parametrize("capacity", [258, 14])
def test_demand_everything_at_its_maximum(capacity):
    """n_cdf = 256 (the fourth ballot round of the count; four rounds of 64 cars in k_demand<true>), 16 profiles and 64
    segments in the ((k * S + s) * n) table indexing, TFX_MAX_ARCH = 64 rows, over 67 ticks that visit every segment and
    wrap the period; the profiles of the five envs rewritten between previews so that every one of the 16 is drawn.
    C = 258 keeps 255 rows per road - every car's; C = 14 keeps 12, and roads take more.  The rows buffer starts as 0xEE:
    the bytes past min(count, S) stay that, the bytes before are the rule's."""
    S = min(capacity - 2, MAX_CDF - 1)
    eng = demand_engine("line", rows=MAX_ROWS, capacity=capacity)
    prof = on_device(MAX_PROFILES[0], eng)
    eng.set_demand(max_means(), road_weights(66, MAX_K, MAX_S), seed=DEMAND_SEED, profile_of_env=prof, n_cdf=MAX_CDF,
                   row_weights=max_row_weights(), **MAX)
    tables, row_cdf = max_tables()
    assert eng.demand_rows_per_road == S and eng.demand_tables.count_cdf.shape == (MAX_K, MAX_S, MAX_CDF)
    assert np.array_equal(eng.demand_tables.road_cdf, tables.road_cdf) and np.array_equal(eng.demand_row_cdf, row_cdf)
    tick0, n = MAX_RANGE
    counts = torch.empty((n, DEMAND_E, 66), dtype=torch.int32, device=eng.device)
    rows = torch.empty((n, DEMAND_E, 66, S), dtype=torch.uint8, device=eng.device)
    over = deep = 0
    for which, profile in enumerate(MAX_PROFILES):
        eng.demand_profile.copy_(on_device(profile, eng))
        counts.fill_(-1)
        rows.fill_(0xEE)
        eng.demand_rows(tick0, n, out=(counts, rows))
        gc, gr = counts.cpu().numpy(), rows.cpu().numpy()
        wc, wr = max_mirror(S, which)
        assert np.array_equal(gc, wc), (which, np.argwhere(gc != wc)[:5])
        live = np.arange(S) < np.minimum(wc, S)[..., None]
        assert np.array_equal(gr[live], wr[live]), (which, np.argwhere((gr != wr) & live)[:5])
        assert (gr[~live] == 0xEE).all(), (which, np.argwhere((gr != 0xEE) & ~live)[:5])
        assert np.array_equal(eng.demand_counts(tick0, n).cpu().numpy(), wc), which        # (k_demand<false> on the same tables)
        over += int((wc > S).sum())
        deep += int((wc.sum(axis=2) >= 193).sum())
    assert deep > 0 and (over > 0) == (capacity == 14)


def test_demand_2048_entry_roads():
    """The entry-road limit of tfx_set_demand: a 1 x 1023 world has 2 * 1024 = 2048 entry roads.  launch_demand then asks
    for 4 wavefronts * 2 arrays * 2048 roads * 4 B = 65536 B of dynamic LDS.  That is within what the launch may ask for:
    k_demand declares no static LDS (its only __shared__ object is the extern array), and a kernel may take up to 64 KiB =
    65536 B of dynamic LDS without hipFuncSetAttribute - the bound is inclusive.  Inside, wavefront wv (0..3) uses words
    [wv * 4096, wv * 4096 + 4096): its thresholds at [0, 2048), its histogram at [2048, 4096); the highest word touched is
    3 * 4096 + 4095 = 16383, byte 65532.  The binary search keeps lo and hi inside [0, 2047], and the row that leaves is
    written at dst[j], j < 2048.  Eleven levels of the search, 32 lane strides over the slice."""
    eng = engine_with({}, 1, env_id_offset=DEMAND_OFF, m=1, n=1023, length=60.0, capacity=6)
    assert eng.n_entry == 2048 and eng.R == 4 * 1023 + 2048
    w = road_weights(2048, 1, 3, seed=2)
    eng.set_demand(MANY_MEANS, w, seed=DEMAND_SEED, **MANY)
    got = eng.demand_counts(0, 8).cpu().numpy()
    want = devrng.demand_counts(DEMAND_SEED, [DEMAND_OFF], np.arange(0, 8), eng.demand_tables, None, **MANY)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    N = want.sum(axis=2)[:, 0]
    assert (N == 0).any() and (N >= 193).any() and want[..., :64].sum() > 0 and want[..., 1984:].sum() > 0
    # ... and the handle steps under it
    eng.reset(np.zeros((1, eng.I), np.int32))
    eng.set_actions(cycle_period=3)
    eng.step(2)
    assert 0 < int(eng.cars_on_roads_flat().sum()) <= int(want[:2].sum())   # (a heavy road is offered more cars than its ring takes)


def test_demand_refuses_2050_entry_roads():
    """one more entry road than the LDS slice holds: TFX_EINVAL naming the entry roads, and the handle still steps"""
    eng = engine_with({}, 1, m=1, n=1024, length=60.0, capacity=6)
    assert eng.n_entry == 2050
    with pytest.raises(nat.TfxError, match="tfx error -1: demand: more than 2048 entry roads"):
        eng.set_demand([[1.0]])
    assert eng.demand is None
    eng.reset(np.zeros((1, eng.I), np.int32))
    eng.set_spawns(period=2)
    eng.set_actions(cycle_period=3)
    eng.step(4)
    assert int(eng.cars_on_roads_flat().sum()) > 2050


# ---- C. 66 entry roads on every step path -------------------------------------------------------------------------------------
WIDE_E, WIDE_OFF, WIDE_SEED, SPACING = 5, 31, 0xC0DE0066, 3
WIDE_CALLS = (("step", 1), ("step", 6), ("agent", 4), ("step", 3))
WIDE_PATHS = {"resident": {"TFX_RESIDENT": "1"},                           # two lanes per road, an env per workgroup
              "resident_two_envs": {"TFX_RESIDENT": "1", "TFX_RES_LPR": "1", "TFX_RES_EPB": "2"},      # s_spawn[2][66]
              "pairs": PAIRS, "pertick": PERTICK}
WIDE_DEMAND = dict(means=[[3.0, 0.5], [1.0, 6.0]], seg_ticks=4, tick_offset=2)
WIDE_PROFILE = [0, 1, 0, 1, 1]
# heterogeneous cars never run LDS-resident (res_usable, csrc/tfx_launch.hpp): their streams take the other two paths
WIDE_CASES = [(s, p) for s in ("poisson_greedy", "regular", "demand") for p in WIDE_PATHS] + \
             [(s, p) for s in ("poisson_rows", "demand_rows") for p in ("pairs", "pertick")]


class DemandFeed(object):
    """rules 4 and 5 by clock tick, as a mirror with next_tick"""

    def __init__(self, eng):
        self.eng, self.t = eng, 0
        self.ids = np.arange(eng.E) + eng.cfg.env_id_offset

    def next_tick(self, frozen=None):
        e, dm = self.eng, self.eng.demand
        args = dict(seg_ticks=dm["seg_ticks"], tick_offset=dm["tick_offset"])
        if e.het:
            c, r = devrng.demand_rows(dm["seed"], self.ids, [self.t], e.demand_tables, e.demand_row_cdf, e.demand_rows_per_road,
                                      WIDE_PROFILE, **args)
            out = (c[0], r[0])
        else:
            out = devrng.demand_counts(dm["seed"], self.ids, [self.t], e.demand_tables, WIDE_PROFILE, **args)[0]
        self.t += 1
        return out


@pytest.mark.parametrize("stream,path", WIDE_CASES)
def test_wide_world_on_every_step_path(stream, path):
    """The 1 x 32 world (194 roads, 66 entry roads), C = 10, five envs: step(1), step(6), agent_step(4), step(3), the whole
    state against the oracle under the mirrored inputs after every call."""
    het = stream.endswith("rows")
    tab10 = tab10_of(TAB3) if het else None
    eng = engine_with(WIDE_PATHS[path], WIDE_E, planes=3 if het else 2, env_id_offset=WIDE_OFF, archetypes=TAB3 if het else None,
                      m=1, n=32, length=60.0, capacity=10)
    assert eng.n_entry == 66 and eng.R == 194
    resident = path.startswith("resident")
    assert eng.fused_ticks() == (0, resident)
    orc = oracle_like(eng)
    orc.entrypoints = eng.entrypoints
    rng = np.random.RandomState(66 + len(stream))
    ph = rng.randint(2, size=(WIDE_E, eng.I)).astype(np.int32)
    eng.reset(ph)
    orc.reset(ph)
    ids = range(WIDE_OFF, WIDE_OFF + WIDE_E)
    rows_kw = dict(n_archetypes=3, per_road=eng.C - 2) if het else {}
    if stream.startswith("poisson"):
        eng.set_poisson(3.0, seed=WIDE_SEED)
        mirror = FastPoisson(3.0, WIDE_SEED, 66, ids, **rows_kw)
    elif stream == "regular":
        eng.set_regular(2.6, seed=WIDE_SEED)                                # three cars in every tick
        mirror = FastRegular(2.6, WIDE_SEED, 66, ids)
    else:
        eng.set_demand(weights=road_weights(66, 2, 2, seed=3), seed=WIDE_SEED, profile_of_env=on_device(WIDE_PROFILE, eng),
                       row_weights=[2.0, 1.0, 1.0] if het else None, **WIDE_DEMAND)
        mirror = DemandFeed(eng)
    greedy = stream == "poisson_greedy"
    if greedy:
        eng.set_greedy(SPACING)
    act = np.zeros((WIDE_E, eng.I), np.int32)
    t, past64, on_past64 = 0, 0, 0

    def arrivals(j, frozen):
        return mirror_tick(mirror, het, frozen.copy())

    for kind, T in WIDE_CALLS:
        if not greedy:
            act = rng.randint(2, size=(WIDE_E, eng.I)).astype(np.int32)
            eng.set_actions(act)
        where = "%s %s %s(%d) from tick %d" % (stream, path, kind, T, t)
        if kind == "step":
            eng.step(T)
            done = np.zeros(WIDE_E, bool)
            for _ in range(T):
                if greedy and t % SPACING == 0:
                    act = greedy_actions(orc)
                cnt, rows = mirror_tick(mirror, het)
                past64 += int(cnt[:, 64:].sum())
                done |= oracle_tick(orc, act, cnt, rows, tab10, eng.entrypoints)
                t += 1
            assert np.array_equal(eng.done.cpu().numpy().astype(bool), done), "done " + where
            assert_same_state(eng, orc, where)
            if het:
                assert_rows_wide(eng, orc, tab10, where)
        else:
            tick0 = eng.tick
            out = eng.agent_step(T, remi=True)
            frozen = np.zeros(WIDE_E, bool)
            want_obs = np.zeros((WIDE_E, 2 * eng.r + eng.I), np.float32)
            # the decision in spans that end where the greedy controller decides again (one span without it)
            cuts = [tick0] + [u for u in range(tick0 + 1, tick0 + T) if greedy and u % SPACING == 0] + [tick0 + T]
            for a, b in zip(cuts[:-1], cuts[1:]):
                if greedy and a % SPACING == 0:
                    act = np.where(frozen[:, None], act, greedy_actions(orc))
                keep = [getattr(orc, f)[frozen].copy() for f in ORC_FIELDS]
                aobs, _, adone, _ = emulate_decision(orc, a, act, lambda j, fr: arrivals(j, fr | frozen), b - a, False, tab10)
                for f, kept in zip(ORC_FIELDS, keep):
                    getattr(orc, f)[frozen] = kept
                run = ~frozen
                want_obs[run, :eng.r] += aobs[run, :eng.r]
                want_obs[run, eng.r:] = aobs[run, eng.r:]
                frozen |= adone.astype(bool)
            t += T
            # (under the greedy controller no env stands still here: what it holds for one that does is not this test's)
            assert not (greedy and frozen.any())
            assert_decision(eng, orc, out, (want_obs, orc.remi_reward().copy(), frozen.astype(np.uint8)), tab10, where)
        assert eng.tick == t, where
        on_past64 += int(eng.cars_on_roads_flat().cpu().numpy()[:, eng.entrypoints[64:]].sum())
        if resident:
            assert eng.step_kernel() == "k_res" and eng.fused_ticks() == (t, True), where
    assert past64 > 0 and on_past64 > 0                                     # entry indices 64 and 65 received cars
    assert int(eng.cars_on_roads_flat().sum()) > 60
    if not resident:
        assert eng.fused_ticks()[0] == 0 and (eng.pair_ticks() > 0) == (path == "pairs")


# ---- D. a low rate ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["resident", "pertick"])
def test_low_rate_long_table_and_long_countdowns(path):
    """set_poisson(0.02) on a 2 x 2 world, step(64) seven times: the threshold search of k_poisson / k_res hundreds of
    entries into a table of more than a thousand, countdowns that outlast several calls."""
    E, off = LOW["E"], LOW["off"]
    eng = engine_with(WIDE_PATHS[path], E, env_id_offset=off, m=2, n=2, length=120.0, capacity=14)
    assert eng.fused_ticks() == (0, path == "resident") and eng.n_entry == 8
    assert len(devrng.gap_table(LOW["cpt"])) > 1000
    orc = oracle_like(eng)
    rng = np.random.RandomState(2)
    ph = rng.randint(2, size=(E, eng.I)).astype(np.int32)
    eng.reset(ph)
    orc.reset(ph)
    eng.set_poisson(LOW["cpt"], seed=LOW["seed"])
    mirror = FastPoisson(LOW["cpt"], LOW["seed"], eng.n_entry, range(off, off + E))
    t, cars = 0, 0
    for T in LOW["calls"]:
        act = rng.randint(2, size=(E, eng.I)).astype(np.int32)
        eng.set_actions(act)
        eng.step(T)
        for _ in range(T):
            cnt = mirror.next_tick()
            cars += int(cnt.sum())
            oracle_tick(orc, act, cnt, None, None, eng.entrypoints)
            t += 1
        assert_same_state(eng, orc, "%s tick %d" % (path, t))
    assert mirror.max_gap > 200 and cars >= 10 and t == 448
    if path == "resident":
        assert eng.step_kernel() == "k_res" and eng.fused_ticks() == (t, True)
