"""The arrival kernels at every launch form and table limit - the host half (tests/test_gpu_arrival_forms.py runs the device).

Two things live here, both on the CPU:

1. A vectorised evaluation of the arrival rules over the env axis (FastPoisson, FastRegular): devrng.PoissonMirror and
   devrng.RegularMirror loop over envs and cars in Python, which 1025 loaded envs cannot afford.  The definition stays in
   gym_traffic/devrng.py; the fast forms use its philox4x32_words, gap_table and tags, the fixed draw indexing (draw 0 is the
   first gap; car c takes draw 1 + 2c for its entry road and 2 + 2c for the gap behind it; rule 1 of include/tfx.h for the
   archetype rows) and are held to the slow mirrors exactly - counts and rows, frozen envs included.

2. The rates, seeds and tables of every GPU case (CASES, DEMAND_*), with the condition each one is there for asserted on
   the mirror alone: a GPU case cannot pass while skipping the branch it was written for.  The conditions are evaluated
   over the ten ticks of the plain calls of a case (step(1) x 3, step(7)), where no env stands still and the mirror alone
   says what the device draws - a subset of the case's ticks, so no weaker than counting the decisions' ticks as well."""
import numpy as np
import pytest

from gym_traffic import devrng
from gym_traffic.devrng import MASK, TAG_ARCH, TAG_GAP, TAG_ROAD, philox4x32_words

U64 = np.uint64


def first_word(c0, c1, c2, c3, k0, k1):
    return philox4x32_words(c0, c1, c2, c3, k0, k1)[0]


class _FastRows(object):
    """devrng._Rows over the env axis: seq [E, n_entry] cars put on each entry road so far"""

    def __init__(self, n_archetypes, per_road, env_ids, n_entry, k0, k1):
        self.n, self.S = int(n_archetypes), int(per_road)
        self.ids = np.asarray(env_ids, U64)
        self.seq = np.zeros((len(self.ids), n_entry), U64)
        self.k0, self.k1 = k0, k1

    def tick(self, counts, draw=True):
        E, ne = counts.shape
        rows = np.zeros((E, ne, self.S), np.uint8)
        if draw and self.n > 1:
            m = np.minimum(counts, self.S).astype(np.int64).reshape(-1)
            road = np.repeat(np.arange(E * ne), m)                       # flat (env, entry) of every kept car
            if road.size:
                j = np.arange(road.size) - np.repeat(np.cumsum(m) - m, m)
                env, ej = road // ne, road % ne
                u = first_word((self.seq[env, ej] + j.astype(U64)) & U64(MASK), self.ids[env], TAG_ARCH, ej.astype(U64),
                               self.k0, self.k1)
                rows[env, ej, j] = ((u * U64(self.n)) >> U64(32)).astype(np.uint8)
        self.seq += counts.astype(U64)
        return rows


class _FastStream(object):
    def __init__(self, seed, n_entry, env_ids, n_archetypes, per_road):
        self.k0, self.k1 = int(seed) & MASK, (int(seed) >> 32) & MASK
        self.n_entry = int(n_entry)
        self.ids = np.asarray(list(env_ids), U64)
        self.E = len(self.ids)
        self.car = np.zeros(self.E, U64)
        if per_road is None and int(n_archetypes) > 1:
            raise ValueError("rows of an archetype table need per_road")
        self.rows = None if per_road is None else _FastRows(n_archetypes, per_road, self.ids, self.n_entry, self.k0, self.k1)

    def _roads(self, out, env, car):
        """one more car per (env, car index) pair on the entry road its draw 1 + 2c names"""
        ur = first_word(U64(1) + U64(2) * car, self.ids[env], TAG_ROAD, 0, self.k0, self.k1)
        np.add.at(out, (env, ((ur * U64(self.n_entry)) >> U64(32)).astype(np.int64)), 1)

    def _active(self, frozen):
        if frozen is None:
            return np.ones(self.E, bool)
        if isinstance(frozen, np.ndarray) and frozen.dtype == bool:
            return ~frozen
        return ~np.isin(self.ids, np.asarray(sorted(frozen), U64))      # global env ids, as the slow mirrors take them


class FastPoisson(_FastStream):
    """devrng.PoissonMirror for all envs at once.  next_tick(frozen) -> counts int32 [E, n_entry], or (counts, rows uint8
    [E, n_entry, S]) with per_road given; frozen: bool [E] or a collection of global env ids.  max_gap: the longest gap
    drawn so far, in ticks."""

    def __init__(self, cars_per_tick, seed, n_entry, env_ids, n_archetypes=1, per_road=None):
        _FastStream.__init__(self, seed, n_entry, env_ids, n_archetypes, per_road)
        self.cdf = devrng.gap_table(cars_per_tick)
        self.cdf_np = self.cdf[:-1].astype(U64)
        self.gap = np.full(self.E, -1, np.int64)
        self.max_gap = 0

    def _gaps(self, draw, env):
        g = np.searchsorted(self.cdf_np, first_word(draw, self.ids[env], TAG_GAP, 0, self.k0, self.k1), side="right")
        if g.size:
            self.max_gap = max(self.max_gap, int(g.max()))
        return g.astype(np.int64)

    def next_tick(self, frozen=None):
        out = np.zeros((self.E, self.n_entry), np.int32)
        active = self._active(frozen)
        new = np.nonzero(active & (self.gap < 0))[0]
        self.gap[new] = self._gaps(np.zeros(new.size, U64), new)
        burst = np.nonzero(active & (self.gap == 0))[0]
        self.gap[active & (self.gap > 0)] -= 1
        lanes = np.arange(64, dtype=U64)
        while burst.size:                                                 # 64 consecutive cars of every bursting env at a time
            c = self.car[burst][:, None] + lanes[None, :]
            env = np.broadcast_to(burst[:, None], c.shape)
            gaps = self._gaps(U64(2) + U64(2) * c, env)
            stop = gaps > 0
            ends = stop.any(axis=1)
            f = np.where(ends, stop.argmax(axis=1), 63)                   # the last car of the tick within the batch
            take = np.arange(64)[None, :] <= f[:, None]
            self._roads(out, env[take], c[take])
            self.car[burst] += (f + 1).astype(U64)
            self.gap[burst[ends]] = gaps[ends, f[ends]] - 1
            burst = burst[~ends]
        return out if self.rows is None else (out, self.rows.tick(out))


class FastRegular(_FastStream):
    """devrng.RegularMirror for all envs at once (rows: all 0, the reference's archetypes[0])."""

    def __init__(self, cars_per_tick, seed, n_entry, env_ids, n_archetypes=1, per_road=None):
        import math
        _FastStream.__init__(self, seed, n_entry, env_ids, n_archetypes, per_road)
        self.every, self.burst = round(1 / cars_per_tick), math.ceil(cars_per_tick)
        self.i = np.zeros(self.E, np.int64)

    def next_tick(self, frozen=None):
        out = np.zeros((self.E, self.n_entry), np.int32)
        active = self._active(frozen)
        due = active & (np.ones(self.E, bool) if self.every == 0 else self.i % max(self.every, 1) == 0)
        self.i[active] += 1
        env = np.nonzero(due)[0]
        if env.size:
            c = self.car[env][:, None] + np.arange(self.burst, dtype=U64)[None, :]
            self._roads(out, np.broadcast_to(env[:, None], c.shape).reshape(-1), c.reshape(-1))
            self.car[env] += U64(self.burst)
        return out if self.rows is None else (out, self.rows.tick(out, draw=False))


# ---- 1. the fast mirrors are the slow ones -----------------------------------------------------------------------------
def frozen_schedule(t, ids):
    """which global env ids stand still in tick t: two envs for a few ticks each, one from tick 30 to the end"""
    out = set()
    if 5 <= t < 9:
        out.add(ids[1])
    if 12 <= t < 14 or t == 20:
        out.add(ids[4])
    if t >= 30:
        out.add(ids[6])
    return out


@pytest.mark.parametrize("cpt", [0.02, 1.4, 9.0])
@pytest.mark.parametrize("kind", ["poisson", "regular"])
def test_fast_mirror_equals_devrng(kind, cpt):
    """8 envs, 40 ticks, 3 archetype rows with S = 8 rows kept per road, frozen envs included; counts and rows exact.
    4 entry roads: at 9 cars per tick roads receive more cars than rows are kept."""
    ids = list(range(37, 45))
    seed, ne, S = 0x5EED0000ABCD1, 4, 8
    slow_cls, fast_cls = (devrng.PoissonMirror, FastPoisson) if kind == "poisson" else (devrng.RegularMirror, FastRegular)
    slow = slow_cls(cpt, seed, ne, ids, n_archetypes=3, per_road=S)
    fast = fast_cls(cpt, seed, ne, ids, n_archetypes=3, per_road=S)
    plain = fast_cls(cpt, seed, ne, ids)
    total, most = 0, 0
    for t in range(40):
        fr = frozen_schedule(t, ids)
        mask = np.array([e in fr for e in ids])
        want_c, want_r = slow.next_tick(frozen=fr)
        got_c, got_r = fast.next_tick(frozen=mask if t % 2 else fr)      # both ways of naming the envs that stand still
        assert got_c.dtype == np.int32 and got_r.dtype == np.uint8 and got_r.shape == (8, ne, S)
        assert np.array_equal(got_c, want_c), t
        assert np.array_equal(got_r, want_r), t
        assert np.array_equal(plain.next_tick(frozen=mask), want_c), t
        assert not got_c[mask].any()
        total += int(want_c.sum())
        most = max(most, int(want_c.max()))
    assert np.array_equal(fast.rows.seq, slow.rows.seq)
    if kind == "poisson":
        assert fast.gap.tolist() == [slow.gap[e] for e in ids] and fast.car.tolist() == [slow.car[e] for e in ids]
        if cpt == 0.02:
            assert fast.max_gap > 10
        if cpt == 9.0:
            assert most > S and len(set(np.unique(want_r).tolist())) == 3
    else:
        assert fast.car.tolist() == [slow.car[e] for e in ids]
    assert total > (0 if cpt == 0.02 else 40)


def test_fast_mirror_is_sharding_independent():
    """a subset of the envs draws what it draws inside the batch (the streams are keyed by global env id)"""
    whole = FastPoisson(8.0, 99, 66, range(100, 140), n_archetypes=64, per_road=4)
    part = FastPoisson(8.0, 99, 66, [103, 139], n_archetypes=64, per_road=4)
    for t in range(6):
        (c, r), (pc, pr) = whole.next_tick(), part.next_tick()
        assert np.array_equal(c[[3, 39]], pc) and np.array_equal(r[[3, 39]], pr), t


# ---- 2. the GPU cases of group A and the branch each one is there for ----------------------------------------------------
# worlds (m, n, length, capacity) and the entry roads 2 (m + n) each has
WORLDS = {"small": dict(m=1, n=1, length=60.0, capacity=10),              # 4 entry roads, 8 roads
          "deep": dict(m=1, n=1, length=60.0, capacity=130),              # S = 128 rows per road: more pairs than lanes
          "line": dict(m=1, n=32, length=60.0, capacity=6)}               # 66 entry roads: more than one wavefront of them
N_ENTRY = {"small": 4, "deep": 4, "line": 66}
PLAIN_CALLS = (1, 1, 1, 7)          # then two agent_step(5, remi=True)
DECISIONS = (5, 5)


def lanes_of(E):
    """launch_poisson's workgroup size (csrc/tfx_launch.hpp)"""
    return 1024 if E <= 64 else (256 if E <= 1024 else 64)


def case(world, E, off, cpt, seed, rows=1, stream="poisson"):
    return dict(world=world, E=E, off=off, cpt=cpt, seed=seed, rows=rows, stream=stream)


# P(gap = 0) = 1 - exp(-cpt / 2): 8 cars per tick give P(burst > 64) ~ 0.3 and P(burst > 128) ~ 0.09 per burst, 10 cars per
# tick P(burst > 256) ~ 0.18 and P(burst > 512) ~ 0.03.  The 64-lane cases take 8 (or 10), the 256-lane ones 10.  At these rates
# an env skips a tick almost only through its first gap (P ~ exp(-cpt / 2)): the seeds of the 65-env cases are the first of a
# short scan with such an env.
CASES = {
    "small_64": case("small", 64, 7, 10.0, 0xA11CE0001),
    "small_65": case("small", 65, 1000, 10.0, 0xA11CE0901),
    "small_1024": case("small", 1024, 3, 10.0, 0xA11CE0003),
    "small_1025": case("small", 1025, 2048, 8.0, 0xA11CE0004),
    "deep_rows_1025": case("deep", 1025, 5, 10.0, 0xA11CE0005, rows=3),
    "line_65": case("line", 65, 11, 10.0, 0xA11CE0301),
    "line_1025": case("line", 1025, 90, 8.0, 0xA11CE0007),
    "line_rows_65": case("line", 65, 13, 10.0, 0xA11CE0301, rows=64),
    "line_rows_1025": case("line", 1025, 400, 8.0, 0xA11CE0009, rows=64),
    "line_regular_1025": case("line", 1025, 17, 70.0, 0xA11CE000A, stream="regular"),
}


def case_mirror(name):
    c = CASES[name]
    cls = FastPoisson if c["stream"] == "poisson" else FastRegular
    ne = N_ENTRY[c["world"]]
    kw = dict(n_archetypes=c["rows"], per_road=WORLDS[c["world"]]["capacity"] - 2) if c["rows"] > 1 else {}
    return cls(c["cpt"], c["seed"], ne, range(c["off"], c["off"] + c["E"]), **kw)


_PLAIN_TICKS = {}


def plain_ticks(name):
    """the counts [10, E, n_entry] the case's plain calls draw (made once)"""
    if name not in _PLAIN_TICKS:
        m = case_mirror(name)
        ticks = [m.next_tick() for _ in range(sum(PLAIN_CALLS))]
        _PLAIN_TICKS[name] = np.stack([t[0] if isinstance(t, tuple) else t for t in ticks])
    return _PLAIN_TICKS[name]


@pytest.mark.parametrize("name", sorted(CASES))
def test_case_reaches_its_branch(name):
    c = CASES[name]
    nthr = lanes_of(c["E"])
    cnt = plain_ticks(name)
    per_item = cnt.sum(axis=2)                                              # cars of every (tick, env)
    ne = N_ENTRY[c["world"]]
    assert cnt.shape == (10, c["E"], ne) and c["off"] > 0
    print("%s: %d lanes, items with more than %d cars: %d, more than %d: %d, largest %d, items without a car %d" % (
        name, nthr, nthr, (per_item > nthr).sum(), 2 * nthr, (per_item > 2 * nthr).sum(), per_item.max(), (per_item == 0).sum()))
    assert (cnt.sum(axis=(0, 1)) > 0).all()                                 # every entry road is drawn
    if c["stream"] == "regular":
        assert c["E"] > 1024 and nthr == 64 and round(1 / c["cpt"]) == 0    # every = 0: a burst in every tick
        assert (per_item == 70).all() and 70 > nthr                         # the j += nthr stride of the regular branch
        return
    if nthr in (64, 256):
        assert (per_item > nthr).sum() >= 20                                # a second round of the burst loop
        assert (per_item > 2 * nthr).sum() >= 1                             # ... and a third
    assert ((per_item == 0).any(axis=1)).any()                              # a tick in which some env's gap is positive
    if c["rows"] > 1:
        S = WORLDS[c["world"]]["capacity"] - 2
        assert (cnt > S).any()                                              # roads offered more cars than rows are kept
        if c["world"] == "deep":
            assert S > nthr and ne * S > 2 * nthr                           # dq = nthr / S == 0 in the pair walk
    if c["world"] == "line":
        assert ne > 64 and (cnt[:, :, 64:].sum(axis=(0, 1)) > 0).all()      # entry indices a 64-lane stride reaches second


def test_every_launch_form_has_a_case():
    forms = {}
    for name, c in CASES.items():
        forms.setdefault((lanes_of(c["E"]), c["world"], c["rows"] > 1, c["stream"]), []).append(name)
    assert {k[0] for k in forms} == {64, 256, 1024}
    for world, rows in (("small", False), ("line", False), ("line", True)):
        assert {k[0] for k in forms if k[1] == world and k[2] == rows and k[3] == "poisson"} >= {64, 256}
    assert (64, "deep", True, "poisson") in forms and (64, "line", False, "regular") in forms
    assert sorted(CASES[n]["E"] for n in CASES if CASES[n]["world"] == "small") == [64, 65, 1024, 1025]


# ---- 3. the demand tables of group B -------------------------------------------------------------------------------------
DEMAND_SEED = (0xD3 << 32) | 4242
DEMAND_E, DEMAND_OFF = 5, 21
# the small table of tests/test_gpu_demand.py on 66 entry roads: K = 2, S = 3 segments of 2 ticks, n_cdf = 137
SMALL_MEANS = [[0.5, 70.0, 0.0], [2.0, 1.0, 9.0]]
SMALL = dict(seg_ticks=2, tick_offset=3)
SMALL_PROFILE = [0, 1, -1, 2, 1]
SMALL_RANGES = ((3, 7), (-9, 7), (2 ** 31 - 2, 4))          # two segment boundaries and the period wrap; negative; clock wrap
# everything at its declared maximum: 16 profiles x 64 segments of one tick, n_cdf = 256, 64 rows
MAX_K, MAX_S, MAX_CDF, MAX_ROWS = 16, 64, 256, 64
MAX = dict(seg_ticks=1, tick_offset=5)
MAX_RANGE = (40, 67)                                        # 67 ticks from clock tick 40: every segment, across the wrap
# the profiles of the five envs, rewritten between previews: every profile 0..15, and -1 / 16 (no cars)
MAX_PROFILES = ([0, 1, 2, 3, 4], [5, 6, 7, 8, 9], [10, 11, 12, 13, 14], [15, -1, 16, 0, 7])
MANY_MEANS, MANY = [[40.0, 0.0, 200.0]], dict(seg_ticks=2, tick_offset=0)     # the 2048 entry roads: one profile, three segments


def road_weights(n_entry, K, S, seed=0):
    """skewed: a few heavy roads per (profile, segment) - also beyond entry index 63 - so that single roads take tens of
    cars of an item of 180"""
    rng = np.random.RandomState(seed)
    w = rng.rand(K, S, n_entry) ** 4 + 0.01
    heavy = rng.randint(0, n_entry, size=(K, S))
    np.put_along_axis(w, heavy[..., None], 3.0 + n_entry / 16.0, axis=2)
    return w


def max_means():
    """near 180 cars per env per tick (193 and more: about one item in six); two (profile, segment) pairs of mean 0"""
    rng = np.random.RandomState(16)
    means = rng.uniform(170.0, 190.0, size=(MAX_K, MAX_S))
    means[3, 10] = means[12, 63] = 0.0
    return means


def max_row_weights():
    rng = np.random.RandomState(64)
    w = rng.rand(MAX_K, MAX_S, MAX_ROWS) + 0.05
    w[:, ::2, 17] = 0.0                                                    # (a row of weight zero is not drawn)
    return w


_MAX = {}


def max_tables(n_entry=66):
    if n_entry not in _MAX:
        t = devrng.demand_tables(max_means(), road_weights(n_entry, MAX_K, MAX_S), n_cdf=MAX_CDF, n_entry=n_entry)
        _MAX[n_entry] = (t, devrng.demand_row_table(max_row_weights(), MAX_K, MAX_S, MAX_ROWS))
    return _MAX[n_entry]


_MAX_ROWS = {}


def max_mirror(per_road, which):
    """devrng.demand_rows of the maximal table for profile assignment `which` over MAX_RANGE (made once per per_road)"""
    key = (per_road, which)
    if key not in _MAX_ROWS:
        tables, row_cdf = max_tables()
        ids = np.arange(DEMAND_E) + DEMAND_OFF
        ticks = np.arange(MAX_RANGE[0], MAX_RANGE[0] + MAX_RANGE[1])
        _MAX_ROWS[key] = devrng.demand_rows(DEMAND_SEED, ids, ticks, tables, row_cdf, per_road, MAX_PROFILES[which], **MAX)
    return _MAX_ROWS[key]


def test_demand_tables_reach_their_limits():
    tables, row_cdf = max_tables()
    assert tables.count_cdf.shape == (MAX_K, MAX_S, MAX_CDF) and tables.road_cdf.shape == (MAX_K, MAX_S, 66)
    assert row_cdf.shape == (MAX_K, MAX_S, MAX_ROWS)
    small = devrng.demand_tables(SMALL_MEANS, road_weights(66, 2, 3, seed=1), n_entry=66)
    assert small.count_cdf.shape == (2, 3, 137)
    ticks = np.arange(MAX_RANGE[0], MAX_RANGE[0] + MAX_RANGE[1])
    segs = devrng.demand_segment(ticks, MAX_S, **MAX)
    assert set(segs.tolist()) == set(range(MAX_S)) and (np.diff(segs) < 0).any()            # every segment, and the wrap
    used = set()
    for prof in MAX_PROFILES:
        used |= {p for p in prof if 0 <= p < MAX_K}
    assert used == set(range(MAX_K))
    big = zero = trunc = rows_seen = 0
    seen = np.zeros(MAX_ROWS, bool)
    for which in range(len(MAX_PROFILES)):
        cnt, rows = max_mirror(12, which)
        N = cnt.sum(axis=2)
        valid = np.array([0 <= p < MAX_K for p in MAX_PROFILES[which]])
        big += int((N >= 193).sum())                                        # the fourth ballot round; four rounds of 64 cars
        zero += int((N[:, valid] == 0).sum())                               # an item of a drawn profile without a car
        trunc += int((cnt > 12).sum())                                      # roads that take more cars than rows are kept
        assert not N[:, ~valid].any() and N.max() <= MAX_CDF - 1
        live = np.arange(12) < np.minimum(cnt, 12)[..., None]
        seen |= np.bincount(rows[live], minlength=MAX_ROWS) > 0
        rows_seen += int(live.sum())
        assert (cnt[:, :, 64:].sum() > 0)                                   # entry indices past the first wavefront
    print("items with N >= 193: %d, N == 0: %d, roads over 12 cars: %d, rows kept %d" % (big, zero, trunc, rows_seen))
    assert big >= 1 and zero >= 1 and trunc >= 1
    assert seen[np.arange(MAX_ROWS) != 17].all()
    # the deep form keeps every car's row: no road takes more than 255
    cnt, rows = max_mirror(255, 0)
    assert cnt.max() <= 255 and np.array_equal(cnt, max_mirror(12, 0)[0])
    assert np.array_equal(rows[..., :12], max_mirror(12, 0)[1])


def test_many_entry_roads_table():
    """2048 entry roads: the binary search of k_demand goes eleven levels deep, and roads at both ends receive cars"""
    t = devrng.demand_tables(MANY_MEANS, road_weights(2048, 1, 3, seed=2), n_entry=2048)
    assert t.road_cdf.shape == (1, 3, 2048) and t.count_cdf.shape[2] == 256
    cnt = devrng.demand_counts(DEMAND_SEED, [DEMAND_OFF], np.arange(0, 8), t, None, **MANY)
    N = cnt.sum(axis=2)[:, 0]
    assert (N == 0).any() and (N >= 193).any() and (cnt[..., :64].sum() > 0) and (cnt[..., 1984:].sum() > 0)
    assert (cnt.sum(axis=(0, 1)) > 0).sum() > 300


# ---- 4. the low rate of group D --------------------------------------------------------------------------------------------
LOW = dict(cpt=0.02, seed=0x10E0001, E=3, off=9, calls=(64,) * 7)


def test_low_rate_has_a_long_table_and_long_gaps():
    """0.02 cars per tick: a gap table of more than a thousand thresholds, walked hundreds of entries deep"""
    assert len(devrng.gap_table(LOW["cpt"])) > 1000
    m = FastPoisson(LOW["cpt"], LOW["seed"], 8, range(LOW["off"], LOW["off"] + LOW["E"]))
    cars = sum(int(m.next_tick().sum()) for _ in range(sum(LOW["calls"])))
    print("low rate: %d cars in %d ticks, longest gap %d" % (cars, sum(LOW["calls"]), m.max_gap))
    assert m.max_gap > 200 and cars >= 10
