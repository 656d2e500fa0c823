"""Every step path at late clocks: 2^24 (where float32 stops holding every tick and the mixed cars' 24-bit spawn ticks
wrap), 3 * 2^24 (a second wrap, float32 ticks on a grid of 4) and the top of the clock's domain, TFX_TICK_MAX
(include/tfx.h).  The oracle cannot be run there - its clock is a float32 - so every case is a SHIFTED TWIN: handle A
and the oracle run a scenario of tests/test_transplant_host.py at the low clock, handle L runs shift_ops of the same, D
ticks later, and L must equal the exact integer map of A (tests/test_late_clock_host.py:ClockMap: spawn ticks, done_tick
and the trip log move, everything else is the same bits) while A agrees with the oracle - so A and L cannot be wrong
alike.  Nothing here has a tolerance.

  A  test_shifted_twin          every (path, kind, geometry) of the transplant matrix x every clock class
  B  test_state_across_a_gap    state taken at the low clock continues on a late handle: clone_envs across handles,
                                pack_envs / unpack_envs, car_list -> put_cars(spawn_shift=D);
     test_restart_from_a_pool_at_the_low_clock   restarts from an episode pool whose handle stayed at the low clock
  C  test_inputs_that_read_the_clock   the fixed cycle, periodic spawns (held to their NumPy statement at the late ticks
                                through the oracle), the greedy controller's spacing, a demand profile
  D  queries on a late state that was stepped to: inside A (car_ages, trip_stats, car_list) and
     test_vec_env_surface_late (travel_times(), cars().age_ticks)
  E  test_the_clocks_domain     tfx_set_tick and the stepping calls refuse what leaves 0 .. TFX_TICK_MAX, and change nothing;
     test_the_handles_own_mirror_counts_every_tick   the same on the C ABI alone, the device clock never read in between;
     test_cycle_period_bound, test_longest_cycle_at_the_top   the bound TFX_TICK_MAX rests on, and the sum it allows

Every parametrised case prints its triples and seconds (tests/test_gpu_transplant.py:run_case does the same)."""
import ctypes as C
import time

import numpy as np
import pytest

import test_late_clock_host as L
import test_transplant_host as H
from test_gpu_parity import assert_same_state, same_bits
from test_gpu_stride_rounds import device_tick, live_all

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from gym_traffic import _native as nat  # noqa: E402
from gym_traffic import devrng  # noqa: E402
from gym_traffic import workload as wl  # noqa: E402
from test_gpu_clone import ARCH, HET_PATHS, PATHS, assert_env_equal, snapshot  # noqa: E402
from test_gpu_fused import engine_with  # noqa: E402
from test_gpu_episodes import GRID as WARM_GRID, force_path  # noqa: E402
from test_gpu_transplant import CLONE_PATHS, MATRIX, DeviceSide, Residue, assert_oracle_agrees  # noqa: E402
from test_gpu_warm_pool import HET_ROWS, SCENARIOS as WARM_SCENARIOS, run_warm  # noqa: E402

W24, TICK_MAX = L.W24, L.TICK_MAX


# ---- comparisons ---------------------------------------------------------------------------------------------------------------------
def assert_late_equals(l, a, cmap, where, undated=False):
    """handle L == the map of handle A: every env (assert_env_equal under the map), the clock - the engine's mirror and
    the device's word -, a decision's outputs, the vehicle updates, and under device inputs the episode accounting.
    undated: no oracle dates the trip log - its entries are left out, n_trips is compared"""
    sl, sa = snapshot(l.eng), snapshot(a.eng)
    cl, ca = (sl, sa)
    if undated:
        assert np.array_equal(sl[0]["n_trips"], sa[0]["n_trips"]), ("n_trips", where)
        cl, ca = without_trip_entries(sl), without_trip_entries(sa)
    for k in range(a.w.E):
        assert_env_equal(cl, k, ca, k, where, clock_map=cmap)
    assert a.eng.tick == device_tick(a.eng) and l.eng.tick == device_tick(l.eng), ("the engine's clock mirror", where)
    assert l.eng.tick == a.eng.tick + cmap.D, ("tick", l.eng.tick, a.eng.tick, where)
    assert (a.outs is None) == (l.outs is None), where
    for name, u, v in zip(("aobs", "areward", "adone"), l.outs or (), a.outs or ()):
        u, v = u.cpu().numpy(), v.cpu().numpy()
        assert same_bits(u, v) if u.dtype == np.float32 else np.array_equal(u, v), (name, where)
    assert l.eng.vehicle_updates() == a.eng.vehicle_updates(), ("vehicle_updates", where)
    if a.device_inputs:
        for f in ("ep_return", "ep_len", "ep_index"):
            assert torch.equal(getattr(l.eng, f), getattr(a.eng, f)), (f, where)
    return sl, sa


def mapped_planes(sa, cmap):
    """A's snapshot as L must hold it: (w plane with the live slots mapped, the trip log mapped)"""
    s, Cc = sa
    live = live_all(s["leading"], s["lastcar"], Cc)
    w = np.zeros_like(s["w"])
    w[live] = cmap.w(s["w"][live])
    trips = s["trip_times"].copy()
    for k in range(len(trips)):
        n = int(s["n_trips"][k])
        trips[k, :n] = cmap.trips(k, s["trip_times"][k, :n])
    return w, trips


def assert_queries(l, a, sa, cmap, where):
    """D: the read-only queries of the late handle against their NumPy statements (gym_traffic/devrng.py) evaluated on the
    MAP of A's state at A's clock + D"""
    eng, (s, Cc) = l.eng, sa
    w, trips = mapped_planes(sa, cmap)
    now = a.eng.tick + cmap.D
    got = eng.car_ages()
    want = devrng.car_ages(w, s["leading"], s["lastcar"], Cc, now, het=eng.het)
    for name, g, x in zip(("n_cars", "age_sum", "age_max"), got, want):
        assert np.array_equal(g.cpu().numpy(), x), ("car_ages." + name, where)
    got = eng.trip_stats()
    want = devrng.trip_stats(trips, s["n_trips"], eng.trip_cap)
    for name, g, x in zip(("count", "tick_sum", "tick_max", "lost"), got, want):
        assert np.array_equal(g.cpu().numpy(), x), ("trip_stats." + name, where)
    cl = eng.car_list()
    want = devrng.car_list(s["x"], s["v"], w, s["arch"], s["leading"], s["lastcar"], Cc)
    assert int(cl.n) == want[0] and np.array_equal(cl.offsets.cpu().numpy(), want[1]), ("car_list offsets", where)
    assert same_bits(cl.spawn.cpu().numpy(), want[5]), ("car_list.spawn", where)


def without_trip_entries(snap):
    """a snapshot whose trip log assert_env_equal leaves alone (where no oracle dates the entries; n_trips is compared
    by the caller)"""
    s, Cc = snap
    return {k: v for k, v in s.items() if k not in ("n_trips", "trip_times")}, Cc


def describe(exc):
    return str(exc).splitlines()[0][:300] if str(exc) else repr(exc)


# ---- A. the shifted twin --------------------------------------------------------------------------------------------------------
def twin_triple(w, path, cls, triple, queries):
    p, m, c = triple
    D = L.shift_of(cls, p)
    where = (path, w.kind, w.geom, cls, p, m, c)
    pre, mut, cont = L.case_ops(w.geom, triple)
    a, l, orc = DeviceSide(w, path, p), DeviceSide(w, path, p), L.DatedOracle(w)
    a.run(pre, after=Residue(a, p))
    l.run(L.shift_ops(pre, D, w.het), after=Residue(l, p))            # (the late handle took the paths the prefix is about)
    orc.run(pre)
    assert_late_equals(l, a, L.ClockMap(D, w.het, orc.dated()), ("after the prefix",) + where)
    if p == "P4":
        stamps = l.eng.done_tick.cpu().numpy()
        assert (stamps != 0).any() and (stamps == 0).any() and (stamps[stamps != 0] > D).all(), ("P4's stamps", stamps, where)
    for side in (a, orc):
        side.run(mut)
    l.run(L.shift_ops(mut, D, w.het))
    live = int((l.eng.done == 0).sum())
    assert 2 * live >= w.E, "only %d of %d envs are live at the hand-over" % (live, w.E)
    a.outs = l.outs = None
    a.eng.reset_counters()
    l.eng.reset_counters()
    updates0 = orc.orc.vehicle_updates
    for side in (a, orc):
        side.run(cont)
    l.run(L.shift_ops(cont, D, w.het))
    cmap = L.ClockMap(D, w.het, orc.dated())
    _, sa = assert_late_equals(l, a, cmap, where)
    assert_oracle_agrees(a, orc, c, updates0, where)
    if queries:
        assert_queries(l, a, sa, cmap, where)


def run_late_case(label, triples, body):
    failures, t_start = [], time.time()
    for triple in triples:
        try:
            body(triple)
        except AssertionError as exc:
            failures.append("%s: %s" % (" x ".join(triple), describe(exc)))
    print("%s: %d triples in %.1f s, %d failed" % (label, len(triples), time.time() - t_start, len(failures)))
    assert not failures, "%d of %d triples differ:\n  %s" % (len(failures), len(triples), "\n  ".join(failures))


@pytest.mark.parametrize("cls", L.CLASSES)
@pytest.mark.parametrize("path,kind,geom", MATRIX)
def test_shifted_twin(path, kind, geom, cls):
    w = H.World(geom, kind)
    queries = geom == "g33" and kind != "plain"                         # (D: the queries need the spawn plane)
    run_late_case("%s/%s/%s %s" % (path, kind, geom, cls), L.LATE_CASES[cls],
                  lambda triple: twin_triple(w, path, cls, triple, queries))


# ---- B. state that crosses a clock gap of 2^24 or more --------------------------------------------------------------------------
GAP_CLOCK = {"CROSS24": W24 - 3, "TOP": TICK_MAX - 40}          # the late handle's clock at the hand-over, or up to 2 more
GAP_TRIPLES = [(p, route, c) for p in ("P1", "P3", "P6") for route in ("clone", "pack", "put") for c in ("step5", "agent4")]
# single-archetype validate handles: the clone with TFX_CLONE_STREAM | TFX_CLONE_EPISODE as well (see gap_triple)
FLAG_TRIPLES = [(p, "clone_flags", c) for p in ("P1", "P3", "P6") for c in ("step5", "agent4")]
GREEDY_SPACING = 3                                               # DeviceSide's greedy controller under device inputs


def hand_over(route, s, l, D, flags):
    se, le, w = s.eng, l.eng, s.w
    every = np.arange(w.E)
    if route == "clone":
        le.clone_envs(torch.arange(w.E, dtype=torch.int32), source=se, streams=flags, episodes=flags)
        assert le.clone_skipped() == 0
    elif route == "pack":
        le.unpack_envs(every, se.pack_envs(every))
    else:
        # the caller's own route: the bound tensors copied, the stamps rebased by hand, the cars as a list taken at another clock
        for f in ["obs", "waiting", "rewards", "passed_dst", "done"] + (["n_trips", "trip_times"] if w.validate else []):
            getattr(le, f).copy_(getattr(se, f))
        le.done_tick.copy_(torch.where(se.done_tick != 0, se.done_tick + D, se.done_tick))
        cl = se.car_list()
        le.put_cars(cl.offsets, cl.xv, row=cl.row, spawn=cl.spawn, leading=se.leading.clone(), spawn_shift=D)


def gap_triple(w, path, cls, triple):
    p, route, c = triple
    where = (path, w.kind, cls, p, route, c)
    # tfx_clone_envs hands streams and episodes on only between handles that draw their arrivals on the device, which the
    # oracle cannot follow; single-archetype validate handles need the oracle's dates for the trip map, so route "clone"
    # runs them under bound inputs without the two flags, and route "clone_flags" under device inputs with both - there
    # the entries the continuation logs are left out (n_trips, the spawn plane and the stamps are compared)
    device_inputs = route == "clone_flags" or (route == "clone" and w.kind != "validate")
    undated = device_inputs and w.validate and not w.het
    if route == "clone_flags":
        route = "clone"
    pre, cont = H.prefix_ops(w.geom, p), H.cont_ops(w.geom, c)
    s = DeviceSide(w, path, p, device_inputs=device_inputs)
    s.run(pre, after=Residue(s, p, bound_inputs=not device_inputs))
    orc = None if device_inputs else L.DatedOracle(w).run(pre)
    D = GAP_CLOCK[cls] - s.eng.tick
    D += -D % GREEDY_SPACING                                        # (the controller decides when (tick + 1) % spacing == 0)
    assert D >= W24 - 128 and D % GREEDY_SPACING == 0
    l = DeviceSide(w, path, p, device_inputs=device_inputs)
    l.eng.set_tick(s.eng.tick + D)
    hand_over(route, s, l, D, device_inputs)
    first = s.eng.n_trips.cpu().numpy().copy() if w.validate else None
    s.outs = l.outs = None
    s.eng.reset_counters()
    l.eng.reset_counters()
    assert_late_equals(l, s, L.ClockMap(D, w.het, None if orc is None else orc.dated(), first), ("at the hand-over",) + where)
    s.run(cont)
    l.run(cont)
    if orc is not None:
        updates0 = orc.orc.vehicle_updates
        orc.run(cont)
    assert_late_equals(l, s, L.ClockMap(D, w.het, None if orc is None else orc.dated(), first), where, undated=undated)
    if orc is not None:
        assert_oracle_agrees(s, orc, c, updates0, where)
    if cls == "CROSS24":
        assert l.eng.tick - 8 < W24 < l.eng.tick, "the continuation did not cross 2^24"


def _gap_matrix():
    out = []
    for path in CLONE_PATHS:
        out.append((path, "plain"))
        if not path.endswith("resident"):
            out.append((path, "validate"))
        if path in HET_PATHS:
            out.append((path, "het"))
    return out


@pytest.mark.parametrize("cls", sorted(GAP_CLOCK))
@pytest.mark.parametrize("path,kind", _gap_matrix())
def test_state_across_a_gap(path, kind, cls):
    w = H.World("g33", kind)
    triples = GAP_TRIPLES + (FLAG_TRIPLES if kind == "validate" else [])
    run_late_case("%s/%s across a gap to %s" % (path, kind, cls), triples, lambda triple: gap_triple(w, path, cls, triple))


def test_rebase_rounds_once_pin():
    """tests/golden/regress/rebase_rounds_once.json: tfx_put_cars' spawn_shift (clone_side, which tfx_clone_envs and the
    warm restart share) on a single-archetype handle gives float32(spawn + shift), rounded once"""
    from gym_traffic.core import TfxEngine
    cases = L.rebase_cases()
    eng = TfxEngine(2, 2, 100.0, 8, n_envs=1, validate=True, planes=3)
    eng.reset(np.zeros((1, eng.I), np.int32))
    for shift in sorted({c["shift"] for c in cases}):
        mine = [c for c in cases if c["shift"] == shift][:6]          # (a ring of 8 slots holds 6 cars)
        offsets = np.zeros(eng.R + 1, np.int32)
        offsets[1:] = len(mine)
        xv = np.float32([[50.0 - 6.0 * i, 0.0] for i in range(len(mine))])
        eng.put_cars(offsets, xv, spawn=np.float32([c["spawn"] for c in mine]), spawn_shift=shift)
        got = eng.car_list().spawn.cpu().numpy()
        assert any(c["want"] != c["rounded_twice"] for c in mine), shift    # (two roundings would show)
        assert [int(t) for t in got] == [c["want"] for c in mine], (shift, got)


# the fourth route: a restart from an episode pool whose handle sits at the low clock while the live handle is late
WARM_KINDS = {"plain": {}, "het": dict(archetypes=HET_ROWS, planes=3, layout="transposed"), "validate": dict(validate=True)}


@pytest.mark.parametrize("cls", sorted(GAP_CLOCK))
@pytest.mark.parametrize("path,kind", [("resident", "plain"), ("pairs", "plain"), ("pertick", "het"), ("pairs", "het"),
                                       ("pairs", "validate")])
def test_restart_from_a_pool_at_the_low_clock(monkeypatch, path, kind, cls):
    """tests/test_gpu_warm_pool.py:run_warm with the live handles' clock started late: the pool is warmed up from tick 0,
    so every restart rebases a pool env by 2^24 or more.  run_warm itself holds the restart to tfx_clone_envs from the
    pool on a second late handle after every decision (trip logs included; test_state_across_a_gap holds that clone to
    the low clock); here the whole late run must equal the same run from tick 0 under the map - periodic arrivals with D
    a multiple of the period, episode phases and pool slots do not read the clock.  (Single-archetype validate handles:
    the trip map needs the oracle's dates, which run_warm has none of - the entries of the trip log are left out of the
    comparison with the low run, n_trips, the spawn plane and the stamps are in it.)"""
    force_path(monkeypatch, path)
    t_start = time.time()
    sc, warm = (dict(C=12, period=8, M=12, K=30), 6) if kind == "validate" else (WARM_SCENARIOS["limit"], 3)
    ticks = sc["K"] * WARM_GRID["T"]
    D = ((W24 - ticks // 2) if cls == "CROSS24" else (TICK_MAX - ticks)) // sc["period"] * sc["period"]
    late = run_warm(sc, WARM_KINDS[kind], tick0=D, warm=warm)
    a = late["a"]
    assert a.tick == D + ticks == device_tick(a) and a.tick <= TICK_MAX
    assert (D < W24 < a.tick) if cls == "CROSS24" else (a.tick >= TICK_MAX - 64)
    assert (late["restart"] >= 2).any() and (late["term"] > 0).any() and late["pool"].tick < 100
    low = run_warm(sc, WARM_KINDS[kind], tick0=0, warm=warm)
    assert np.array_equal(low["restart"], late["restart"]) and np.array_equal(low["term"], late["term"])
    sl, sa = snapshot(a), snapshot(low["a"])
    if kind == "validate":
        assert late["trips"] > 0 and np.array_equal(sl[0]["n_trips"], sa[0]["n_trips"])
        sl, sa = without_trip_entries(sl), without_trip_entries(sa)
    for k in range(a.E):
        assert_env_equal(sl, k, sa, k, (path, kind, cls, "restarts from a low pool"), clock_map=L.ClockMap(D, a.het))
    print("%s/%s restarts from a low pool, live clock at %s: %d ticks in %.1f s" % (path, kind, cls, ticks, time.time() - t_start))


# ---- C. inputs that read the clock ----------------------------------------------------------------------------------------------
CYCLE_P, SPAWN_Q = 7, 4
KEYED_LCM = 84                                                   # lcm(2 * CYCLE_P, SPAWN_Q, GREEDY_SPACING)
CALLS = (1, 4, 5, 2, 3, 6)
KEYED_PATHS = ("pertick", "pairs_tail", "resident")


def keyed_clocks(cls):
    """(the low twin's clock, D): D a multiple of every period, the late clock 3 ticks below 2^24 / 40 below the top"""
    late = GAP_CLOCK[cls]
    D = (late - 60) // KEYED_LCM * KEYED_LCM
    assert D % (2 * CYCLE_P) == 0 and D % SPAWN_Q == 0 and D % GREEDY_SPACING == 0 and 60 <= late - D < 60 + KEYED_LCM
    return late - D, D


def rule_inputs(w, tick, n):
    """The two on-device rules, stated once in NumPy with Python integers (include/tfx.h): in tick t env e's lights take
    a = ((t + (e + env_id_offset) % P) // P) & 1, and entry road rd receives one car iff t % Q == rd % Q"""
    acts = np.zeros((n, w.E, w.I), np.int32)
    cnt = np.zeros((n, w.E, w.n_entry), np.int32)
    for i in range(n):
        t = int(tick) + i
        for e in range(w.E):
            acts[i, e, :] = ((t + e % CYCLE_P) // CYCLE_P) & 1
        for j, rd in enumerate(w.entry.tolist()):
            cnt[i, :, j] = 1 if t % SPAWN_Q == rd % SPAWN_Q else 0
        assert np.array_equal(acts[i], wl.cycle_actions(np.arange(w.E), w.I, t, CYCLE_P))
        assert sorted(w.entry[cnt[i, 0] > 0].tolist()) == sorted(wl.spawn_roads_for_tick(w.entry, t, SPAWN_Q))
    return acts, cnt


@pytest.mark.parametrize("cls", sorted(GAP_CLOCK))
@pytest.mark.parametrize("path", KEYED_PATHS)
def test_inputs_that_read_the_clock(path, cls):
    w = H.World("g33", "plain")
    low, D = keyed_clocks(cls)
    t_start = time.time()
    for mode in ("cycle", "greedy", "demand"):
        rng = H._rng("g33", "keyed/" + mode)
        load = [H._load(rng, w, H._calm(rng, w), low)]
        a, l = DeviceSide(w, path, "P1"), DeviceSide(w, path, "P1")
        a.run(load)
        l.run(L.shift_ops(load, D, False))
        orc = H.OracleSide(w).run(load)
        cmap = L.ClockMap(D, False)
        if mode == "demand":
            # rule 4 is keyed by the clock tick itself: no shift leaves it alone.  The late handle draws its arrivals on
            # the device; the low one is fed the rule's NumPy statement for the LATE ticks through a bound buffer
            means = np.array([[0.8, 2.5, 0.2]])
            l.eng.set_demand(means, seg_ticks=5, tick_offset=3, seed=77)
        for e in (a.eng, l.eng):
            if mode == "greedy":
                e.set_greedy(GREEDY_SPACING)
            else:
                e.set_actions(cycle_period=CYCLE_P)
            if mode != "demand":
                e.set_spawns(period=SPAWN_Q)
        for n in CALLS:
            where = (path, cls, mode, "step(%d) from %d" % (n, l.eng.tick))
            acts, cnt = rule_inputs(w, l.eng.tick, n)
            if mode == "demand":
                cnt = devrng.demand_counts(77, np.arange(w.E), np.arange(l.eng.tick, l.eng.tick + n), l.eng.demand_tables,
                                           None, 5, 3)
                assert cnt.sum() > 0
                a.eng.set_spawns(counts=cnt, per_tick=True)
            a.eng.step(n)
            l.eng.step(n)
            assert_late_equals(l, a, cmap, where)
            if mode != "greedy":
                # ... and to the rules' own statement: the oracle under the actions and arrivals of the LATE ticks
                orc.run([dict(op="step", n=n, acts=acts, cnt=cnt, rows=np.zeros((n, w.E, w.n_entry, H.ROWS_PER_ROAD), np.uint8))])
                assert_same_state(l.eng, orc.orc, str(where))
                assert np.array_equal(l.eng.done.cpu().numpy(), orc.done), ("done", where)
        if mode == "demand":
            cnt = devrng.demand_counts(77, np.arange(w.E), np.arange(l.eng.tick, l.eng.tick + 5), l.eng.demand_tables, None, 5, 3)
            a.eng.set_spawns(counts=cnt, per_tick=True)
        a.outs = [t.clone() for t in a.eng.agent_step(5)]
        l.outs = [t.clone() for t in l.eng.agent_step(5)]
        assert_late_equals(l, a, cmap, (path, cls, mode, "agent_step(5)"))
        if cls == "CROSS24":
            assert l.eng.tick > W24
        if path == "resident":
            assert l.eng.fused_ticks()[0] > 0
        if path.startswith("pairs"):
            assert l.eng.pair_ticks() > 0
    print("%s inputs at %s: 3 rules in %.1f s" % (path, cls, time.time() - t_start))


# ---- D. the batched surface on a late state that was stepped to -----------------------------------------------------------------------
class VecSide(DeviceSide):
    """the ops on the engine of a TrafficVecEnv (its default step path)"""

    def __init__(self, w):
        from gym_traffic.envs.vec_env import TrafficVecEnv
        self.w, self.path, self.device_inputs = w, "default", False
        self.venv = TrafficVecEnv(w.E, w.m, w.n, w.length, capacity=w.C, rate=w.rate, spawn=None, validate=True,
                                  archetypes=ARCH if w.het else None)
        self.eng = self.venv.engine
        self.eng.reset(np.zeros((w.E, self.eng.I), np.int32))
        self.outs = None


@pytest.mark.parametrize("cls", ["CROSS24", "CROSS3x24", "TOP"])
@pytest.mark.parametrize("kind", ["validate", "het"])
def test_vec_env_surface_late(kind, cls):
    w = H.World("g33", kind)
    t_start = time.time()
    triples = [t for t in L.LATE_CASES[cls] if t[1] in ("M0", "M2", "M5")][:3]
    for triple in triples:
        p = triple[0]
        D = L.shift_of(cls, p)
        where = (kind, cls) + triple
        ops = sum(L.case_ops("g33", triple), [])
        a, l, orc = VecSide(w), VecSide(w), L.DatedOracle(w)
        a.run(ops)
        l.run(L.shift_ops(ops, D, w.het))
        orc.run(ops)
        cmap = L.ClockMap(D, w.het, orc.dated())
        _, sa = assert_late_equals(l, a, cmap, where)
        wmap, trips = mapped_planes(sa, cmap)
        s, Cc = sa
        # travel_times(): the whole log and the live cars' ages, from the map of A
        tv = l.venv.travel_times()
        ts = devrng.trip_stats(trips, s["n_trips"], l.eng.trip_cap)
        ages = devrng.car_ages(wmap, s["leading"], s["lastcar"], Cc, a.eng.tick + D, het=w.het)
        assert np.array_equal(tv.finished.cpu().numpy(), ts[0]) and ts[0].sum() > 0, ("finished", where)
        assert np.array_equal(tv.finished_s.cpu().numpy(), ts[1] / 2.0), ("finished_s", where)
        assert np.array_equal(tv.max_trip_s.cpu().numpy(), ts[2] / 2.0), ("max_trip_s", where)
        assert np.array_equal(tv.unfinished.cpu().numpy(), ages[0].sum(axis=1)), ("unfinished", where)
        assert np.array_equal(tv.unfinished_s.cpu().numpy(), ages[1].sum(axis=1) / 2.0), ("unfinished_s", where)
        assert np.array_equal(tv.oldest_s.cpu().numpy(), ages[2].max(axis=1) / 2.0), ("oldest_s", where)
        # cars().age_ticks: the rule of car_ages per car, in car_list's order
        cars = l.venv.cars()
        spawn = devrng.car_list(s["x"], s["v"], wmap, s["arch"], s["leading"], s["lastcar"], Cc)[5]
        now = a.eng.tick + D
        if w.het:
            want = ((now - spawn.astype(np.int64)) & 0xFFFFFF).astype(np.int32)
        else:
            want = (np.float32(now) - spawn).astype(np.float32).astype(np.int32)
        assert same_bits(cars.spawn.cpu().numpy(), spawn), ("cars().spawn", where)
        assert np.array_equal(cars.age_ticks.cpu().numpy(), want), ("cars().age_ticks", where)
    print("vec env surface %s %s: %d triples in %.1f s" % (kind, cls, len(triples), time.time() - t_start))


# ---- E. the clock's domain --------------------------------------------------------------------------------------------------------
def same_snapshot(x, y):
    (a, _), (b, _) = x, y
    return all((a[k] is None and b[k] is None) or (np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes()) for k in a)


def refused(eng, rc, what, code, word):
    assert rc == code, (what, rc)
    assert word in eng.lib.tfx_last_error(), (what, eng.lib.tfx_last_error())


@pytest.mark.parametrize("path,kind", [("pertick", "plain"), ("pairs_tail", "validate"), ("resident", "plain"), ("pairs_split", "het"),
                                       ("ring", "validate")])
def test_the_clocks_domain(path, kind):
    """Argument checks on the host: nothing is enqueued by a refused call, so nothing can go wrong on the device."""
    w = H.World("g33", kind)
    rng = H._rng("g33", "domain")
    t_start = time.time()
    ops = [H._load(rng, w, H._calm(rng, w), 60), H._agent(rng, w, 3, True)]
    three, five = H._step(rng, w, 3), H._step(rng, w, 5)
    D = TICK_MAX - 6 - 60
    a, l, orc = DeviceSide(w, path, "P1"), DeviceSide(w, path, "P1"), L.DatedOracle(w)
    a.run(ops)
    l.run(L.shift_ops(ops, D, w.het))
    orc.run(ops)
    eng, lib = l.eng, l.eng.lib
    assert eng.tick == TICK_MAX - 3 == device_tick(eng)
    assert_late_equals(l, a, L.ClockMap(D, w.het, orc.dated()), (path, kind, "the decision that ends at TFX_TICK_MAX - 3"))

    def unchanged(before, what):
        assert same_snapshot(snapshot(eng), before[0]), (what, "changed the state")
        assert (eng.tick, device_tick(eng), eng.vehicle_updates(), eng.pair_ticks(), eng.fused_ticks()) == before[1], what

    def state():
        return snapshot(eng), (eng.tick, device_tick(eng), eng.vehicle_updates(), eng.pair_ticks(), eng.fused_ticks())

    # tfx_set_tick: the domain is 0 .. TFX_TICK_MAX
    before = state()
    for bad in (-1, TICK_MAX + 1, -2 ** 31, 2 ** 31 - 1):
        refused(eng, lib.tfx_set_tick(eng.h, bad), "tfx_set_tick(%d)" % bad, nat.EINVAL, b"TFX_TICK_MAX")
        unchanged(before, "tfx_set_tick(%d)" % bad)
    for bad in (-1, TICK_MAX + 1, 2 ** 31, 2 ** 32 + 5):                 # (ctypes would wrap the last two into the domain)
        with pytest.raises(nat.TfxError, match="tfx error -1"):
            eng.set_tick(bad)
        unchanged(before, "set_tick(%d)" % bad)
    # three ticks are left: four are refused, by the handle and by the engine's mirror
    eng.set_actions(three["acts"][0])
    eng.set_spawns()
    st = eng._stream()
    refused(eng, lib.tfx_step(eng.h, 4, st), "tfx_step(4)", nat.ESTATE, b"clock")
    refused(eng, lib.tfx_agent_step(eng.h, 4, 1, C.c_void_p(l.outs[0].data_ptr()), C.c_void_p(l.outs[1].data_ptr()),
                                    C.c_void_p(eng.done.data_ptr()), st), "tfx_agent_step(4)", nat.ESTATE, b"clock")
    for call in (lambda: eng.step(4), lambda: eng.agent_step(4), lambda: eng.step(2 ** 31 - 1)):
        with pytest.raises(nat.TfxError, match="tfx error -2"):
            call()
    unchanged(before, "a call of four ticks at TFX_TICK_MAX - 3")
    # ... and three run, to the last tick of the domain
    for side in (a, orc):
        side.run([three])
    l.run([three])
    assert eng.tick == TICK_MAX == device_tick(eng)
    assert_late_equals(l, a, L.ClockMap(D, w.het, orc.dated()), (path, kind, "step(3) to TFX_TICK_MAX"))
    assert_oracle_agrees(a, orc, "step3", orc.orc.vehicle_updates - a.eng.vehicle_updates(), (path, kind, "step(3)"))
    before = state()
    refused(eng, lib.tfx_move_cars(eng.h, st), "tfx_move_cars", nat.ESTATE, b"clock")
    refused(eng, lib.tfx_advance_finished_cars(eng.h, st), "tfx_advance_finished_cars", nat.ESTATE, b"clock")
    refused(eng, lib.tfx_step(eng.h, 1, st), "tfx_step(1)", nat.ESTATE, b"clock")
    for call in (eng.move_cars, eng.advance_finished_cars, lambda: eng.step(1), lambda: eng.agent_step(1)):
        with pytest.raises(nat.TfxError, match="tfx error -2"):
            call()
    assert lib.tfx_step(eng.h, 0, st) == 0                                # (no tick: nothing to refuse)
    unchanged(before, "a tick at TFX_TICK_MAX")
    # the handle is as good as before: set back, with a low-clock state loaded into all three, L equals A under the
    # identity and A the oracle
    eng.set_tick(60)
    assert eng.tick == 60 == device_tick(eng)
    back = [H._load(rng, w, H._calm(rng, w), 60), five]
    for side in (a, l, orc):
        side.run(back)
    assert eng.tick == 65 == device_tick(eng)
    assert_late_equals(l, a, L.ClockMap(0, w.het, orc.dated()), (path, kind, "back at a low clock"))
    assert_oracle_agrees(a, orc, "step5", orc.orc.vehicle_updates - a.eng.vehicle_updates(), (path, kind, "back at a low clock"))
    print("%s/%s the clock's domain: %.1f s" % (path, kind, time.time() - t_start))



def _ptr(t):
    return C.c_void_p(t.data_ptr())


@pytest.mark.parametrize("path,kind", [("pertick", "plain"), ("pairs_tail", "plain"), ("pairs_tail", "validate"), ("pairs_split", "plain"),
                                       ("pairs_split", "het"), ("pairs_nograph", "plain"), ("resident", "plain"), ("ring", "plain")])
def test_the_handles_own_mirror_counts_every_tick(path, kind):
    """The check of the stepping calls reads the handle's HOST mirror of the clock, which only tfx_reset and tfx_set_tick
    set and the calls themselves advance.  So here the C ABI is driven directly and nothing reads the device clock
    (tfx_get_tick) between a stage's calls: the ticks that fit run, the next one is refused by every call that would run
    it, and a call that still fits after a refusal is taken - the mirror counts neither too little nor too much, behind
    tfx_step, tfx_agent_step and tfx_move_cars + tfx_advance_finished_cars, eager and replayed from a graph."""
    w = H.World("g33", kind)
    rng = H._rng("g33", "mirror")
    t_start = time.time()
    side = DeviceSide(w, path, "P7")                                    # (P7's knob: calls of 3 ticks and more run resident)
    side.run([H._load(rng, w, H._calm(rng, w), 60)])
    eng, lib = side.eng, side.eng.lib
    st = eng._stream()
    eng.set_actions(rng.randint(2, size=(w.E, w.I)).astype(np.int32))
    eng.set_spawns()
    aobs = torch.zeros((w.E, 2 * w.r + w.I), dtype=torch.float32, device=eng.device)
    arew = torch.zeros((w.E, w.I), dtype=torch.float32, device=eng.device)
    adone = torch.zeros((w.E,), dtype=torch.uint8, device=eng.device)

    def step(n):
        return lib.tfx_step(eng.h, n, st)

    def agent(n):
        return lib.tfx_agent_step(eng.h, n, 1, _ptr(aobs), _ptr(arew), _ptr(adone), st)

    def at_the_end(stage):
        for what, rc in (("tfx_step(1)", step(1)), ("tfx_move_cars", lib.tfx_move_cars(eng.h, st)),
                         ("tfx_advance_finished_cars", lib.tfx_advance_finished_cars(eng.h, st)),
                         ("tfx_agent_step(1)", agent(1)), ("tfx_step(7)", step(7))):
            refused(eng, rc, "%s: %s at TFX_TICK_MAX" % (stage, what), nat.ESTATE, b"clock")
        assert device_tick(eng) == TICK_MAX, stage                         # (read only now: the refused calls ran nothing)

    eng.set_tick(TICK_MAX - 3)
    assert step(3) == 0
    at_the_end("behind tfx_step(3)")
    eng.set_tick(TICK_MAX - 5)
    assert step(3) == 0
    refused(eng, step(3), "tfx_step(3) with two ticks left", nat.ESTATE, b"clock")
    refused(eng, agent(3), "tfx_agent_step(3) with two ticks left", nat.ESTATE, b"clock")
    assert step(2) == 0, "the mirror counted more than the ticks that ran"
    at_the_end("behind tfx_step(3), a refusal, tfx_step(2)")
    eng.set_tick(TICK_MAX - 4)
    assert agent(4) == 0
    at_the_end("behind tfx_agent_step(4)")
    eng.set_tick(TICK_MAX - 2)
    for _ in range(2):
        assert lib.tfx_move_cars(eng.h, st) == 0 and lib.tfx_advance_finished_cars(eng.h, st) == 0
    at_the_end("behind two ticks in halves")
    for replay in (False, True):                                           # (the second time the launches come from a graph)
        eng.set_tick(TICK_MAX - 10)
        assert step(6) == 0 and agent(4) == 0
        at_the_end("behind tfx_step(6) and tfx_agent_step(4)%s" % (", again" if replay else ""))
    if path.startswith("pairs"):
        assert eng.pair_ticks() > 0
    if path == "pairs_split":
        assert eng.split_ticks() > 0
    if path == "resident":
        assert eng.fused_ticks()[0] > 0
    # tfx_reset sets the mirror as well
    eng.reset(np.zeros((w.E, w.I), np.int32))
    assert step(5) == 0 and device_tick(eng) == 5
    eng.set_tick(60)                                                       # (and the engine's own mirror is right again)
    eng.step(2)
    assert eng.tick == 62 == device_tick(eng)
    print("%s/%s the handle's own mirror: %.1f s" % (path, kind, time.time() - t_start))


def test_cycle_period_bound():
    """TFX_TICK_MAX is derived from the longest cycle tfx_set_actions takes: one more is refused, as is none"""
    w = H.World("g33", "plain")
    eng = DeviceSide(w, "pertick", "P1").eng
    lib = eng.lib
    for bad in (nat.PERIOD_MAX + 1, 2 ** 31 - 1, 0, -3):
        refused(eng, lib.tfx_set_actions(eng.h, nat.ACTION_CYCLE, None, bad, 0), "cycle period %d" % bad, nat.EINVAL, b"TFX_PERIOD_MAX")
    with pytest.raises(nat.TfxError, match="tfx error -1"):
        eng.set_actions(cycle_period=nat.PERIOD_MAX + 1)
    assert lib.tfx_set_actions(eng.h, nat.ACTION_CYCLE, None, nat.PERIOD_MAX, 0) == 0
    assert lib.tfx_set_actions(eng.h, nat.ACTION_CYCLE, None, 1, 0) == 0
    eng.set_actions(cycle_period=nat.PERIOD_MAX)


@pytest.mark.parametrize("path", KEYED_PATHS)
def test_longest_cycle_at_the_top(path):
    """The largest sum the header derives TFX_TICK_MAX from, run: the longest cycle, an env_id_offset that puts half of
    the envs at (env + offset) % period = period - 6 .. period - 1 and the others at 0 .. 5, the last 21 ticks of the
    clock's domain.  tick + (env + offset) % period reaches INT32_MAX - 2, and the envs at 1 .. 5 cross a multiple of the
    period - their lights change - in the last five ticks.  The oracle runs under the rule stated in Python integers."""
    w = H.World("g33", "plain")
    P, off = nat.PERIOD_MAX, nat.PERIOD_MAX - 6
    rng = H._rng("g33", "longest cycle")
    t_start = time.time()
    side = DeviceSide.__new__(DeviceSide)
    side.w, side.path, side.device_inputs, side.outs = w, path, False, None
    side.eng = eng = engine_with(dict(PATHS[path]), w.E, layout="transposed", planes=2, m=w.m, n=w.n, length=w.length,
                                 capacity=w.C, rate=w.rate, env_id_offset=off)
    eng.reset(np.zeros((w.E, w.I), np.int32))
    load = [H._load(rng, w, H._calm(rng, w), TICK_MAX - sum(CALLS))]
    side.run(load)
    orc = H.OracleSide(w).run(load)
    eng.set_actions(cycle_period=P)
    eng.set_spawns()
    largest, seen = 0, set()
    for n in CALLS:
        where = (path, "step(%d) from %d" % (n, eng.tick))
        acts = np.zeros((n, w.E, w.I), np.int32)
        for i in range(n):
            for e in range(w.E):
                total = eng.tick + i + (e + off) % P
                largest = max(largest, total)
                acts[i, e, :] = (total // P) & 1
            seen.add(acts[i, :, 0].tobytes())
        eng.step(n)
        orc.run([dict(op="step", n=n, acts=acts, cnt=np.zeros((n, w.E, w.n_entry), np.int32),
                      rows=np.zeros((n, w.E, w.n_entry, H.ROWS_PER_ROAD), np.uint8))])
        assert_same_state(eng, orc.orc, str(where))
        assert np.array_equal(eng.done.cpu().numpy(), orc.done), ("done", where)
    assert eng.tick == TICK_MAX == device_tick(eng)
    assert largest == 2 ** 31 - 3 and len(seen) >= 5, (largest, len(seen))
    if path == "resident":
        assert eng.fused_ticks()[0] > 0
    print("%s the longest cycle at the top: %.1f s" % (path, time.time() - t_start))
