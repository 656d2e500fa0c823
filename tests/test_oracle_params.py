"""The CPU oracle against reference runs OFF the reference's defaults (tests/golden/params/, captured by
oracle/gen_golden.py --set params): `rate` 0.3 and 0.7 (no powers of two: every product with `rate` rounds), 0.25 and
1.0, one ordinary archetype row other than the reference's, three rows at rate 0.7, the module constants replaced
(YELLOW_TICKS 4, THRESH 0.35, OVERFLOW_PENALTY 7, EPS 3e-7), line grids (1x3, 3x1, 1x1) and roads of 2 to 4 cars.

Bars, per fixture:
  * free-running from reset: every integer exact for 120 ticks;
  * teacher-forced from every tick: integers, spawn ticks and archetype rows exact; x and v within
    conftest.assert_floats_match_reference where rate != 1;
  * the expression order around `rate` (dx = r v + (0.5 dvr) r, traffic_env.py:58-59), which a 1-ulp bound cannot pin:
    at least V_SHARE of the compared v values and X_SHARE of the x values are BIT-EQUAL to the reference.  The
    reference's own power routine leaves 0.9879 / 0.9991 at the worst fixture; dx = r (v + 0.5 dvr) leaves 0.974 of x
    at rate 0.3.

The bound at rate = 1 (stated here once; DESIGN section 2 repeats it).  conftest's bound supposes that every rounding
behind the power term q**delta happens at the scale of the result.  With a step of a whole second a car that brakes hard
(rate1, tick 156: v = 6.57 -> 0.0554 m/s; the three others 8.1 - 8.9 -> 2.9 - 3.2 m/s) has B = 1 - q**4 - u^2 near -2 and
dv = a B of magnitude 4 to 8: one flipped rounding of B (2.4e-7) times a = 3 is one or two steps of dv's grid of 4.8e-7,
and v + dv rate then cancels to a speed whose own ulp is far smaller - 2 ulp at 3.2 m/s, 256 ulp at 0.055 m/s, |dv| =
4.8e-7 or 9.5e-7 against conftest's a rate 2^-22 = 7.2e-7 (and 1 ulp on the default row).  Every float operation between
the power and the new speed passes on what it received and can flip its own rounding, |fl(y + d) - fl(y)| <= |d| +
ulp(fl(y)), so with P = ulp(q**delta) at that car's q = v / v0, A = 1 - q**delta, dvr = v_new - v, dv = dvr / rate,
B = dv / a:

    |v_new - reference| <= rate (a (P + ulp(A) + ulp(B)) + ulp(dv)) + ulp(dvr) + ulp(v_new)          (RATE1_BOUND)

(1.75e-6 to 1.86e-6 for the four cars.)  It is applied ONLY to the cars beyond conftest's bound, which must be cars that stayed in their ring slot over the tick
(so the fixture holds their old speed), and their number per fixture is pinned: BEYOND_OLD_BOUND.  x stays within
conftest's bound on every car of every fixture.
"""
import glob
import os

import numpy as np
import pytest

from conftest import GOLDEN_DIR, Golden, assert_floats_match_reference, ulp_diff
from oracle.oracle import AI, ARCHETYPE, CONSTANTS, V0I, OracleEnv, live_mask

FREE_TICKS = 120
V_SHARE, X_SHARE = 0.98, 0.998
# cars beyond conftest's float bound, teacher-forced, oracle vs reference (all other fixtures: none)
BEYOND_OLD_BOUND = {"rate1": 3, "rate1_light": 1}


def param_names():
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN_DIR, "params", "*.npz")))


_CACHE = {}


def fixture(name):
    if name not in _CACHE:
        _CACHE[name] = Golden("params/" + name)
    return _CACHE[name]


def table_of(g):
    """-> (the config's single row [10] or None, the table [n, 10] of a run with several rows or None)"""
    tab = g.archetypes
    if tab is None:
        return None, None
    return (tab[0], None) if len(tab) == 1 else (None, tab)


def a_max_of(g):
    return 3.0 if g.archetypes is None else float(g.archetypes[:, 3].max())


def constants_of(g):
    return dict(CONSTANTS, **(g.sc.get("constants") or {}))


def make_env(g):
    sc = g.sc
    row, _ = table_of(g)
    return OracleEnv(sc["m"], sc["n"], sc["L"], sc["C"], g["dest"], g["phases"], g["nexts"], rate=sc["rate"],
                     learn_switch=sc["learn_switch"], validate=sc["mode"] == "validate", archetype=row,
                     constants=g.sc.get("constants"))


def step(env, g, t):
    _, tab = table_of(g)
    return env.step(g["actions"][t], [g.spawns(t)], spawn_arch=None if tab is None else [g.spawn_archs(t)], archetypes=tab)


def ints_differ(leading, lastcar, obs, rew, done, waiting, passed_dst, g, k):
    return [n for n, a, b in (("leading", leading, g["leading"][k]), ("lastcar", lastcar, g["lastcar"][k]),
                              ("obs", obs, g["obs"][k]), ("rewards", rew, g["rewards"][k]), ("done", int(done), int(g["done"][k])),
                              ("waiting", waiting, g["waiting"][k]), ("passed_dst", passed_dst, g["passed_dst"][k]))
            if not np.array_equal(a, b)]


def rate1_bound(v_old, v_new, a, rate, v0):
    """RATE1_BOUND of the module docstring for one car (a, v0: its own row's; delta = 4)"""
    f = np.float32
    q = f(v_old) / f(v0)
    qd = f(float(q) ** 4)
    A = f(1) - qd
    dvr = f(v_new) - f(v_old)
    dv = dvr / f(rate)
    B = dv / f(a)
    u = lambda y: float(np.spacing(np.abs(f(y))))
    return rate * (a * (u(qd) + u(A) + u(B)) + u(dv)) + u(dvr) + u(v_new)


class Tally(object):
    """what the table of DESIGN section 2 lists for one fixture"""

    def __init__(self, name, rate):
        self.name, self.rate = name, rate
        self.cars = self.v_equal = self.x_equal = self.max_v = self.max_x = 0
        self.beyond = []            # (tick, old v, reference v, v, ulp, |dv|, RATE1_BOUND) of the cars beyond conftest's bound

    def add(self, x, v, gx, gv):
        ux, uv = ulp_diff(x, gx), ulp_diff(v, gv)
        self.cars += int(ux.size)
        self.v_equal += int((uv == 0).sum())
        self.x_equal += int((ux == 0).sum())
        self.max_v, self.max_x = max(self.max_v, int(uv.max())), max(self.max_x, int(ux.max()))

    def row(self):
        return "%-28s rate %-4g cars %6d  v bit-equal %.4f  x bit-equal %.4f  max ulp v / x %d / %d  beyond conftest's bound %d" % (
            self.name, self.rate, self.cars, self.v_equal / max(1, self.cars), self.x_equal / max(1, self.cars),
            self.max_v, self.max_x, len(self.beyond))

    def assert_shares(self):
        assert self.cars > 3000, self.row()
        assert self.v_equal >= V_SHARE * self.cars and self.x_equal >= X_SHARE * self.cars, self.row()
        assert len(self.beyond) <= BEYOND_OLD_BOUND.get(self.name, 0), (self.row(), self.beyond)


def check_floats(g, k, live, x, v, prev_live, prev_v, arch, tally):
    """The float bars of one teacher-forced tick: x, v [R, C] of tick k against the fixture; prev_*: the reference's
    tick k - 1 (for the cars that kept their slot); arch [R, C]: every slot's table row (None: one row)."""
    sc = g.sc
    gx, gv = g["state_x"][k], g["state_v"][k]
    tally.add(x[live], v[live], gx[live], gv[live])
    kw = dict(a_max=a_max_of(g), rate=sc["rate"], single_default_archetype=g.archetypes is None)
    try:
        assert_floats_match_reference(x[live], v[live], gx[live], gv[live], where=("params/" + g.name, k), **kw)
        return
    except AssertionError:
        if sc["rate"] != 1:
            raise
    # rate = 1: car by car; those beyond conftest's bound get RATE1_BOUND
    row, tab = table_of(g)
    for e, s in zip(*np.nonzero(live)):
        one = lambda a: a[e, s:s + 1]
        try:
            assert_floats_match_reference(one(x), one(v), one(gx), one(gv), where=("params/" + g.name, k), **kw)
            continue
        except AssertionError:
            pass
        assert prev_live[e, s], "a car beyond the bound that changed its slot: %s tick %d road %d slot %d" % (g.name, k, e, s)
        car = tab[int(arch[e, s])] if tab is not None else (row if row is not None else ARCHETYPE)
        bound = rate1_bound(prev_v[e, s], gv[e, s], float(car[AI]), sc["rate"], float(car[V0I]))
        dv = abs(float(v[e, s]) - float(gv[e, s]))
        tally.beyond.append((k, float(prev_v[e, s]), float(gv[e, s]), float(v[e, s]), int(ulp_diff(one(v), one(gv))[0]), dv, bound))
        assert dv <= bound, (g.name, tally.beyond[-1])
        assert ulp_diff(one(x), one(gx))[0] <= 1, (g.name, k, e, s)


def teacher_forced(g):
    """Reference state at t -> one oracle tick -> reference state at t + 1, from every tick.  -> Tally"""
    sc = g.sc
    env = make_env(g)
    _, tab = table_of(g)
    rows = np.arange(env.R)
    tally = Tally(os.path.basename(g.name), sc["rate"])
    for t in range(sc["T"]):
        env.load_planes(0, g["state_x"][t], g["state_v"][t], g["state_w"][t], g["leading"][t], g["lastcar"][t],
                        arch=g["state_a"][t] if tab is not None else None, archetypes=tab)
        env.obs[0] = g["obs"][t]
        env.rewards[0] = g["rewards"][t]
        env.waiting[0] = g["waiting"][t]
        env.passed_dst[0] = g["passed_dst"][t]
        if sc["remi_every"] and t > 0 and t % sc["remi_every"] == 0:
            env.remi_reward()          # the capture called remi_reward() after recording tick t
        env.steps[0] = t
        obs, rew, done = step(env, g, t)
        k = t + 1
        assert ints_differ(env.leading[0], env.lastcar[0], obs[0], rew[0], done[0], env.waiting[0], env.passed_dst[0], g, k) == [], (g.name, k)
        assert np.array_equal(env.x[0][rows, env.leading[0]], g["leader_x"][k])
        x, v, w = env.planes(0)
        live = live_mask(env.leading[0], env.lastcar[0], sc["C"])
        if not live.any():
            continue
        assert np.array_equal(w[live], g["state_w"][k][live])
        arch = None
        if tab is not None:
            arch = env.arch_plane(0, tab)
            assert np.array_equal(arch[live], g["state_a"][k][live])
        check_floats(g, k, live, x, v, live_mask(g["leading"][t], g["lastcar"][t], sc["C"]), g["state_v"][t], arch, tally)
    return tally


@pytest.mark.parametrize("name", param_names())
def test_free_running_integers(name):
    g = fixture(name)
    env = make_env(g)
    env.reset(g["init_phase"])
    ri = 0
    for t in range(FREE_TICKS):
        obs, rew, done = step(env, g, t)
        k = t + 1
        assert ints_differ(env.leading[0], env.lastcar[0], obs[0], rew[0], done[0], env.waiting[0], env.passed_dst[0], g, k) == [], (name, k)
        if sc_remi(g, k):
            assert np.array_equal(env.cars_on_roads()[0], g["cars_on_roads"][ri])
            assert np.array_equal(env.remi_reward()[0], g["remi_rewards"][ri])
            ri += 1
        if g.sc["mode"] == "validate":
            assert int(env.n_trips[0]) == int(g["trip_count"][k])
    assert ri == FREE_TICKS // g.sc["remi_every"]
    if g.sc["mode"] == "validate":
        n = int(env.n_trips[0])
        assert n > 10 and np.array_equal(env.trip_times[0, :n].astype(np.float64), g["trip_times"][:n])


def sc_remi(g, k):
    return bool(g.sc["remi_every"]) and k % g.sc["remi_every"] == 0


@pytest.mark.parametrize("name", param_names())
def test_teacher_forced_every_tick(name):
    tally = teacher_forced(fixture(name))
    print(tally.row())
    for car in tally.beyond:
        print("   tick %d: v %.7g -> reference %.7g, oracle %.7g: %d ulp, |dv| %.3g, bound %.3g" % car)
    tally.assert_shares()


def test_the_fixtures_are_the_ones_the_bars_speak_of():
    """the list of scenarios, and that each is off the defaults in the way its name says"""
    sc = {n: fixture(n).sc for n in param_names()}
    assert sorted(sc) == sorted(["rate03", "rate07", "rate025", "rate1", "rate1_light", "one_row", "truck_rate07", "line_1x3",
                                 "line_3x1", "line_1x1", "short_2x3_c6", "short_2x2_c5_rate1", "short_2x2_c4_rate1_validate",
                                 "three_rows_rate07", "constants"])
    assert [sc[n]["rate"] for n in ("rate03", "rate07", "rate025", "rate1", "truck_rate07", "three_rows_rate07")] == [0.3, 0.7, 0.25, 1.0, 0.7, 0.7]
    assert fixture("one_row").archetypes.shape == (1, 10) and fixture("three_rows_rate07").archetypes.shape == (3, 10)
    assert constants_of(fixture("constants")) == dict(yellow_ticks=4, thresh=0.35, detect_dist=10.0, overflow_penalty=7, eps=3e-7)
    assert [(sc[n]["m"], sc[n]["n"]) for n in ("line_1x3", "line_3x1", "line_1x1")] == [(1, 3), (3, 1), (1, 1)]
    assert all(s["T"] <= 300 and s["m"] * s["n"] <= 6 for s in sc.values())
    for n in param_names():
        assert os.path.getsize(os.path.join(GOLDEN_DIR, "params", n + ".npz")) < 300 * 1024


@pytest.mark.parametrize("name", ["rate03", "rate07", "rate1", "one_row", "truck_rate07", "line_1x3", "short_2x2_c5_rate1", "constants"])
def test_numpy_env_equals_the_oracle_off_the_defaults(name):
    """oracle/numpy_env.py (the second CPU baseline) stays bit-equal to the C oracle on these runs, free-running"""
    from oracle.numpy_env import NumpyBatchedEnv
    g = fixture(name)
    sc = g.sc
    row, _ = table_of(g)
    car = {} if row is None else dict(zip(("v", "l", "a", "v0", "b", "T", "s0"), [float(row[j]) for j in (1, 2, 3, 5, 6, 7, 8)]))
    orc = make_env(g)
    npe = NumpyBatchedEnv(sc["m"], sc["n"], sc["L"], sc["C"], g["dest"], g["phases"], g["nexts"], rate=sc["rate"],
                          constants=sc.get("constants"), **car)
    orc.reset(g["init_phase"])
    npe.reset(g["init_phase"])
    entry = np.asarray(g["entrypoints"])
    for t in range(sc["T"]):
        roads = g.spawns(t)
        cnt = np.array([[int((roads == rd).sum()) for rd in entry]], np.int32)
        # (both get the tick's cars entry road by entry road: cars spawned on different roads do not interact)
        _, _, od = orc.step(g["actions"][t], [np.repeat(entry, cnt[0])])
        _, _, nd = npe.step(g["actions"][t][None], cnt, entrypoints=entry)
        assert bool(nd[0]) == bool(od[0]), t
        assert np.array_equal(npe.leading, orc.leading) and np.array_equal(npe.lastcar, orc.lastcar), t
        assert np.array_equal(npe.obs, orc.obs) and np.array_equal(npe.rewards, orc.rewards), t
        assert np.array_equal(npe.waiting, orc.waiting), t
        live = live_mask(orc.leading[0], orc.lastcar[0], sc["C"])
        assert np.array_equal(npe.x[0][live].view(np.int32), orc.x[0][live].view(np.int32)), t
        assert np.array_equal(npe.v[0][live].view(np.int32), orc.v[0][live].view(np.int32)), t
    assert npe.vehicle_updates == orc.vehicle_updates > 3000
