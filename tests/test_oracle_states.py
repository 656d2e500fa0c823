"""The CPU oracle against reference runs that START from loaded ring states (tests/golden/states/, captured by
oracle/gen_golden.py --set states).  Every other fixture is a free run from the empty map; these start the reference's
TrafficEnv from the family of oracle/ring_states.py - wrapped, full and empty rings, unsorted cars, cars up to 1.6 road
lengths past the road end - so the reference itself goes through several pops per road and tick, cars that are handed
on and popped again downstream in the same tick, full destination rings and the wrapped branch of move_cars
(traffic_env.py:117-157, 187-212).  A fixture holds N independent states (8; the rows fixture a ninth at a clock
beyond 2^21) of K = 6 ticks each, with random actions and 0-3 arrivals per tick that went through the reference's own
add_new_cars, and the tallies of the branches the reference took.  On top of the family the generator lets the head of
about one road in seven stand exactly at the road end (x = L, v = 0: the edge of `x > length`, :123).

Bars, per fixture:
  * teacher-forced from every recorded tick of every state: integers, the fake leaders' x, spawn ticks, table rows
    and trip times exact; x and v within conftest.assert_floats_match_reference (a_max from the table, the scenario's
    rate).  A car beyond that bound is held to a bound derived from the ulp of its own power term (power_bound below),
    car by car, and the number of such cars per fixture is pinned (BEYOND_BOUND);
  * free-running from tick 0 of every state: every integer exact over all K ticks, and the trip log;
  * the tallies: over the set every branch was taken (test_every_branch_was_taken).
"""
import glob
import os

import numpy as np
import pytest

from conftest import GOLDEN_DIR, Golden, assert_floats_match_reference, ulp_diff
from oracle.oracle import AI, ARCHETYPE, DELTAI, V0I, OracleEnv, live_mask
from test_oracle_params import Tally

SCENARIOS = ["st_2x2_c10", "st_3x2_c20_validate", "st_2x3_c6_rate1_ls_validate", "st_2x2_c34_rate07", "st_2x3_c66",
             "st_2x2_c130", "st_1x1_c258", "st_3x2_c20_rows_validate", "st_2x2_c16_constants"]
TALLIES = ("wrapped_road_ticks", "wrapped_waiting_quirk", "multi_pop_road_ticks", "max_pops", "cascades",
           "handoffs_refused", "spawns_refused", "full_pop_and_receive", "leaders_at_next_tail", "heads_at_road_end", "trips")
# cars beyond conftest's float bound, teacher-forced, oracle vs reference (all other fixtures: none)
# (two cars that brake by 7 to 10 m/s within the tick - cars the state family dropped right behind their leader:
#   st_2x2_c130   v 10.17096 -> 0.001189232  8192 ulp  |dv| 9.54e-07  bound 2.76e-06
#   st_1x1_c258   v 7.26575  -> 0.4561276      16 ulp  |dv| 4.77e-07  bound 1.8e-06
#  at both old speeds NumPy's float32 q**4 and the contract's multiply chain differ by exactly one ulp; B = 1 - q**4 - u^2
#  lies beyond -2 there, so one flipped rounding of B is one or two steps of dv's grid, as at rate = 1 in
#  tests/test_oracle_params.py; x stays within 1 ulp on both)
BEYOND_BOUND = {"st_2x2_c130": 1, "st_1x1_c258": 1}


def state_names():
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN_DIR, "states", "*.npz")))


class States(Golden):
    """One fixture of tests/golden/states/: arrays [N, K + 1, ...] (actions: [N, K, I])"""

    @property
    def N(self):
        return int(self.sc["N"])

    @property
    def K(self):
        return int(self.sc["K"])

    @property
    def validate(self):
        return self.sc["mode"] == "validate"

    def _cars(self, i, t, key):
        off = self["spawn_off"]
        j = i * self.K + t
        return self[key][off[j]:off[j + 1]]

    def roads(self, i, t):
        return self._cars(i, t, "spawn_road")

    def rows(self, i, t):
        """table row of every car of roads(i, t), in creation order (zeros without a table)"""
        return self._cars(i, t, "spawn_arch")

    def trips(self, i, k0, k1):
        """the trip times state i logged in the ticks k0 + 1 .. k1"""
        base, cnt = int(self["trip_off"][i]), self["trip_count"][i]
        return self["trip_times"][base + int(cnt[k0]):base + int(cnt[k1])]

    def tally(self, k):
        return int(self["tally_" + k])

    @property
    def a_max(self):
        return 3.0 if self.archetypes is None else float(self.archetypes[:, AI].max())


_CACHE = {}


def fixture(name):
    if name not in _CACHE:
        _CACHE[name] = States("states/" + name)
    return _CACHE[name]


def make_env(g, n_envs=1):
    sc = g.sc
    return OracleEnv(sc["m"], sc["n"], sc["L"], sc["C"], g["dest"], g["phases"], g["nexts"], n_envs=n_envs, rate=sc["rate"],
                     learn_switch=sc["learn_switch"], validate=g.validate, constants=sc.get("constants"))


def load(env, k, g, i, t):
    """env k of the oracle <- state i of the fixture as the reference held it after t ticks"""
    tab = g.archetypes
    env.load_planes(k, g["state_x"][i, t], g["state_v"][i, t], g["state_w"][i, t], g["leading"][i, t], g["lastcar"][i, t],
                    arch=g["state_a"][i, t] if tab is not None else None, archetypes=tab)
    env.obs[k] = g["obs"][i, t]
    env.rewards[k] = g["rewards"][i, t]
    env.waiting[k] = g["waiting"][i, t]
    env.passed_dst[k] = g["passed_dst"][i, t]
    env.steps[k] = g["ticks"][i] + t
    env.n_trips[k] = 0


def step(env, g, states, t):
    """tick t of the given states, one per env of the oracle"""
    tab = g.archetypes
    return env.step(np.stack([g["actions"][i, t] for i in states]), [g.roads(i, t) for i in states],
                    spawn_arch=None if tab is None else [g.rows(i, t) for i in states], archetypes=tab)


def ints_differ(env, k, done, g, i, t):
    """names of the integers of env k that differ from state i's after t ticks"""
    return [n for n, a, b in (("leading", env.leading[k], g["leading"][i, t]), ("lastcar", env.lastcar[k], g["lastcar"][i, t]),
                              ("obs", env.obs[k], g["obs"][i, t]), ("rewards", env.rewards[k], g["rewards"][i, t]),
                              ("done", int(done), int(g["done"][i, t])), ("waiting", env.waiting[k], g["waiting"][i, t]),
                              ("passed_dst", env.passed_dst[k], g["passed_dst"][i, t]))
            if not np.array_equal(a, b)]


def power_bound(v_old, v_new, a, rate, v0, delta):
    """test_oracle_params.rate1_bound for a car of any exponent: with P = ulp(q**delta) at the car's q = v / v0,
    A = 1 - q**delta, dvr = v_new - v, dv = dvr / rate, B = dv / a, every operation between the power and the new speed
    passes on what it received and can flip its own rounding:
        |v_new - reference| <= rate (a (P + ulp(A) + ulp(B)) + ulp(dv)) + ulp(dvr) + ulp(v_new)"""
    f = np.float32
    q = f(v_old) / f(v0)
    qd = f(float(q) ** float(delta))
    A = f(1) - qd
    dvr = f(v_new) - f(v_old)
    dv = dvr / f(rate)
    B = dv / f(a)
    u = lambda y: float(np.spacing(np.abs(f(y))))
    return rate * (a * (u(qd) + u(A) + u(B)) + u(dv)) + u(dvr) + u(v_new)


def check_floats(g, i, k, live, x, v, arch, tally):
    """The float bars of one teacher-forced tick: x, v [R, C] after tick k of state i against the fixture."""
    sc = g.sc
    gx, gv = g["state_x"][i, k], g["state_v"][i, k]
    tally.add(x[live], v[live], gx[live], gv[live])
    kw = dict(a_max=g.a_max, rate=sc["rate"], where=("states/" + g.name, i, k))
    try:
        assert_floats_match_reference(x[live], v[live], gx[live], gv[live], **kw)
        return
    except AssertionError:
        pass
    # car by car; those beyond conftest's bound get power_bound, which needs the car's old speed: it must have kept its slot
    tab = g.archetypes
    prev_live = live_mask(g["leading"][i, k - 1], g["lastcar"][i, k - 1], sc["C"])
    prev_v = g["state_v"][i, k - 1]
    for e, s in zip(*np.nonzero(live)):
        one = lambda a: a[e, s:s + 1]
        try:
            assert_floats_match_reference(one(x), one(v), one(gx), one(gv), **kw)
            continue
        except AssertionError:
            pass
        assert prev_live[e, s], "a car beyond the bound that changed its slot: %s state %d tick %d road %d slot %d" % (g.name, i, k, e, s)
        car = tab[int(arch[e, s])] if tab is not None else ARCHETYPE
        bound = power_bound(prev_v[e, s], gv[e, s], float(car[AI]), sc["rate"], float(car[V0I]), float(car[DELTAI]))
        dv = abs(float(v[e, s]) - float(gv[e, s]))
        tally.beyond.append((k, float(prev_v[e, s]), float(gv[e, s]), float(v[e, s]), int(ulp_diff(one(v), one(gv))[0]), dv, bound))
        assert dv <= bound, (g.name, i, tally.beyond[-1])
        assert ulp_diff(one(x), one(gx))[0] <= 1, (g.name, i, k, e, s)


def teacher_forced(g):
    """Reference state at t -> one oracle tick -> reference state at t + 1, from every tick of every state.  -> Tally"""
    sc, tab = g.sc, g.archetypes
    env = make_env(g)
    roads = np.arange(env.R)
    tally = Tally(os.path.basename(g.name), sc["rate"])
    for i in range(g.N):
        for t in range(g.K):
            load(env, 0, g, i, t)
            _, _, done = step(env, g, [i], t)
            k = t + 1
            assert ints_differ(env, 0, done[0], g, i, k) == [], (g.name, i, k)
            assert np.array_equal(env.x[0][roads, env.leading[0]], g["leader_x"][i, k]), (g.name, i, k)
            if g.validate:
                n = int(env.n_trips[0])
                assert np.array_equal(env.trip_times[0, :n].astype(np.float64), g.trips(i, t, k)), (g.name, i, k)
            x, v, w = env.planes(0)
            live = live_mask(env.leading[0], env.lastcar[0], sc["C"])
            if not live.any():
                continue
            assert np.array_equal(w[live], g["state_w"][i, k][live]), (g.name, i, k)
            arch = None
            if tab is not None:
                arch = env.arch_plane(0, tab)
                assert np.array_equal(arch[live], g["state_a"][i, k][live]), (g.name, i, k)
            check_floats(g, i, k, live, x, v, arch, tally)
    return tally


def print_tally(tally):
    print(tally.row())
    for car in tally.beyond:
        print("   tick %d: v %.7g -> reference %.7g, oracle %.7g: %d ulp, |dv| %.3g, bound %.3g" % car)


@pytest.mark.parametrize("name", SCENARIOS)
def test_teacher_forced_every_tick(name):
    g = fixture(name)
    tally = teacher_forced(g)
    print_tally(tally)
    assert tally.cars > 1000, tally.row()
    assert len(tally.beyond) == BEYOND_BOUND.get(name, 0), (tally.row(), tally.beyond)


@pytest.mark.parametrize("name", SCENARIOS)
def test_free_running_integers(name):
    """all N states side by side from their tick 0: every integer over all K ticks, and the trip log"""
    g = fixture(name)
    env = make_env(g, g.N)
    states = list(range(g.N))
    for i in states:
        load(env, i, g, i, 0)
    for t in range(g.K):
        _, _, done = step(env, g, states, t)
        for i in states:
            assert ints_differ(env, i, done[i], g, i, t + 1) == [], (name, i, t + 1)
            if g.validate:
                assert int(env.n_trips[i]) == int(g["trip_count"][i, t + 1]), (name, i, t + 1)
    if g.validate:
        for i in states:
            n = int(env.n_trips[i])
            assert np.array_equal(env.trip_times[i, :n].astype(np.float64), g.trips(i, 0, g.K)), (name, i)


@pytest.mark.parametrize("name", [n for n in SCENARIOS if "validate" not in n])
def test_numpy_env_from_the_loaded_states(name):
    """oracle/numpy_env.py, the second CPU restatement (default row, no trip log), free-running from tick 0 of every
    state: the reference's integers over all K ticks, and the C oracle's x and v bit for bit"""
    from oracle.numpy_env import NumpyBatchedEnv
    g = fixture(name)
    sc = g.sc
    states = list(range(g.N))
    orc = make_env(g, g.N)
    npe = NumpyBatchedEnv(sc["m"], sc["n"], sc["L"], sc["C"], g["dest"], g["phases"], g["nexts"], n_envs=g.N, rate=sc["rate"],
                          constants=sc.get("constants"))
    for i in states:
        load(orc, i, g, i, 0)
    npe.x[:], npe.v[:] = g["state_x"][:, 0], g["state_v"][:, 0]
    npe.leading[:], npe.lastcar[:] = g["leading"][:, 0], g["lastcar"][:, 0]
    npe.obs[:], npe.rewards[:], npe.waiting[:], npe.passed_dst[:] = g["obs"][:, 0], g["rewards"][:, 0], g["waiting"][:, 0], g["passed_dst"][:, 0]
    entry = np.asarray(g["entrypoints"])
    for t in range(g.K):
        cnt = np.array([[int((g.roads(i, t) == rd).sum()) for rd in entry] for i in states], np.int32)
        step(orc, g, states, t)
        _, _, done = npe.step(np.stack([g["actions"][i, t] for i in states]), cnt, entrypoints=entry)
        for i in states:
            assert ints_differ(npe, i, done[i], g, i, t + 1) == [], (name, i, t + 1)
            live = live_mask(orc.leading[i], orc.lastcar[i], sc["C"])
            assert np.array_equal(npe.x[i][live].view(np.int32), orc.x[i][live].view(np.int32)), (name, i, t + 1)
            assert np.array_equal(npe.v[i][live].view(np.int32), orc.v[i][live].view(np.int32)), (name, i, t + 1)


def test_the_fixtures_are_the_ones_the_bars_speak_of():
    """the list of scenarios, that each is what its name says, and the draws of the family"""
    assert state_names() == sorted(SCENARIOS)
    sc = {n: fixture(n).sc for n in SCENARIOS}
    shape = lambda n: (sc[n]["m"], sc[n]["n"], sc[n]["C"], sc[n]["L"])
    assert [shape(n) for n in SCENARIOS] == [(2, 2, 10, 60.0), (3, 2, 20, 120.0), (2, 3, 6, 30.0), (2, 2, 34, 200.0), (2, 3, 66, 400.0),
                                             (2, 2, 130, 800.0), (1, 1, 258, 900.0), (3, 2, 20, 120.0), (2, 2, 16, 120.0)]
    assert [n for n in SCENARIOS if sc[n]["mode"] == "validate"] == [n for n in SCENARIOS if n.endswith("validate")]
    assert {n: sc[n]["rate"] for n in SCENARIOS if sc[n]["rate"] != 0.5} == {"st_2x3_c6_rate1_ls_validate": 1.0, "st_2x2_c34_rate07": 0.7}
    assert [n for n in SCENARIOS if sc[n]["learn_switch"]] == ["st_2x3_c6_rate1_ls_validate"]
    assert sc["st_2x2_c16_constants"]["constants"] == dict(yellow_ticks=4, thresh=0.35, overflow_penalty=7, eps=3e-7)
    rows = fixture("st_3x2_c20_rows_validate")
    assert rows.archetypes.shape == (6, 10) and sorted(rows.archetypes[:, DELTAI].tolist()) == [0.75, 1, 2, 2.5, 4, 8]
    assert all(fixture(n).archetypes is None for n in SCENARIOS if "rows" not in n)
    for n in SCENARIOS:
        g = fixture(n)
        assert g.K == 6 and g["actions"].shape[:2] == (g.N, 6) and g["state_x"].shape[:2] == (g.N, 7)
        assert g.N == (9 if "rows" in n else 8)
        assert g["ticks"].tolist() == [60] * 8 + ([3000000] if "rows" in n else [])
        per_tick = np.diff(g["spawn_off"])
        assert per_tick.min() == 0 and per_tick.max() == 3 and len(per_tick) == g.N * g.K
        assert os.path.getsize(os.path.join(GOLDEN_DIR, "states", n + ".npz")) <= 1000 * 1000
        live = np.stack([[live_mask(g["leading"][i, k], g["lastcar"][i, k], g.sc["C"]) for k in range(7)] for i in range(g.N)])
        assert np.isfinite(g["state_x"][live]).all() and np.isfinite(g["state_v"][live]).all()      # the generator asserts it too


def test_every_branch_was_taken():
    """the tallies counted from the reference's own runs: over the whole set none is zero, and the long rings wrap"""
    total = {k: sum(fixture(n).tally(k) for n in SCENARIOS) for k in TALLIES}
    for n in SCENARIOS:
        print("%-30s %s" % (n, "  ".join("%s %d" % (k, fixture(n).tally(k)) for k in TALLIES)))
    assert all(v > 0 for v in total.values()), total
    assert max(fixture(n).tally("max_pops") for n in SCENARIOS) > 2          # more pops than the outbox of the parallel path holds
    for n in ("st_2x2_c130", "st_2x3_c66"):
        assert fixture(n).tally("wrapped_road_ticks") > 0, n
    for n in SCENARIOS:
        if fixture(n).validate:
            assert fixture(n).tally("trips") == len(fixture(n)["trip_times"]) > 0, n
    g = fixture("st_1x1_c258")
    cars = np.where(g["leading"] > g["lastcar"], g["lastcar"] + 257 - g["leading"], g["lastcar"] - g["leading"])
    assert cars.max() == 256                                                  # a full ring of the largest size
    g = fixture("st_3x2_c20_rows_validate")
    for i in range(g.N):
        live = live_mask(g["leading"][i, 0], g["lastcar"][i, 0], 20)
        assert sorted(set(g["state_a"][i, 0][live].tolist())) == list(range(6)), i    # live cars of every row
    assert sorted(set(g["spawn_arch"].tolist())) == list(range(6))               # and arrivals of every row
