#!/usr/bin/env python3
"""Capture golden vectors from the reference TrafficEnv (build container only).

TEST INFRASTRUCTURE.  Runs the reference's own `gym_traffic.envs.TrafficEnv`
(/root/reference/gym_traffic/envs/traffic_env.py:221-394, imported in place through
oracle/ref_loader.py) on a fixed list of scenarios and writes small `.npz` fixtures to
tests/golden/.  A fixture is DATA only: the inputs that drive a run (tables, initial
phase, per-tick actions, per-tick spawn roads) and the outputs the reference produced
(per-tick ring indices, obs, rewards, done, waiting, passed_dst, car x/v/w by slot,
remi rewards, cars_on_roads, trip times).  No reference source text is stored.

Instrumentation (wrappers around reference callables; no reference logic is changed):
  * `add_car` is wrapped to log the entry road of every car spawned by
    `TrafficEnv.add_new_cars` (traffic_env.py:274-283) -> the spawn schedule.
  * `advance_finished_cars` / `advance_hack` are wrapped to snapshot the state
    between `move_cars` and the advance (the "mid" state) for kernel-level parity.

The third set (--set states, tests/golden/states/) does not start from the empty map: every state of a scenario is a
reference env whose `state`, `leading`, `lastcar`, `current_phase`, `elapsed` and `steps` are overwritten with a drawn
ring state of oracle/ring_states.py, stepped for a few ticks with scripted arrivals that go through the reference's own
add_new_cars.  Wrappers around move_cars, add_car and the advance count the branches the run took (run_states).

Usage:  python oracle/gen_golden.py [--only NAME] [--set main|params|states]
"""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from ref_loader import load_reference  # noqa: E402
from ring_states import BEYOND, CROWD, live_slots, random_state, state_rows  # noqa: E402

OUT = os.path.join(os.path.dirname(HERE), "tests", "golden")

# name -> scenario.  C = CAPACITY (slots per road); cars/road = C-2.
SCENARIOS = {}


def scen(name, _table=None, **kw):
    d = dict(m=2, n=2, L=250.0, C=20, seed=0, T=300, poisson=True, rate=0.5, lcps=0.12,
             entry='all', learn_switch=False, mode='train', actions='random10',
             remi_every=10, state_every=1, state_next=False, mid=False, archetypes=None)
    d.update(kw)
    (SCENARIOS if _table is None else _table)[name] = d


for _s in (0, 1, 2, 3):
    for _p in (True, False):
        for _c in (10, 20):
            scen("g2x2_s%d_%s_c%d" % (_s, "poi" if _p else "reg", _c), seed=_s, poisson=_p, C=_c,
                 mid=(_s == 0))
scen("g2x2_fixedcycle", seed=2, actions='cycle3')
scen("g2x2_learnswitch", seed=3, learn_switch=True)
scen("g2x2_validate", seed=2, mode='validate', T=400)
scen("g2x2_entry_one", seed=1, entry='one', lcps=0.3)
scen("g2x2_const0_jam", seed=4, actions='const0', lcps=0.3, C=12, T=200)
scen("g3x3_default", m=3, n=3, seed=0, T=400)
scen("g3x2_rect", m=3, n=2, seed=5, T=240, C=16, lcps=0.2)
# the two benchmark shapes: car states of ticks 10 j and 10 j + 1 (4x4) / 30 j and 30 j + 1 (16x16), so the reference's
# floats are compared there too (teacher-forced), not only its integers
scen("g4x4_cfg1", m=4, n=4, L=200.0, C=34, seed=0, T=300, lcps=0.3, state_every=10, state_next=True)
scen("g16x16_cfg2_ints", m=16, n=16, L=400.0, C=66, seed=0, T=150, lcps=0.25, state_every=0)
scen("g16x16_cfg2", m=16, n=16, L=400.0, C=66, seed=1, T=181, lcps=0.12, state_every=30, state_next=True)
# CAPACITY = 130 (BASELINE config 5's 128-car roads, traffic_env.py:46-47,202-212 with rings longer than one
# wavefront): one car per entry road every two ticks - more than a signalised road discharges - so all 32 entry roads
# grow past 64 cars (from tick ~130), reach 128, overflow (from tick 206) and wrap their rings (14 000 wrapped
# road-ticks) while they keep handing cars over; car states of ticks 20 j and 20 j + 1 (teacher-forced floats)
scen("g8x8_c130", m=8, n=8, L=800.0, C=130, seed=6, T=700, poisson=False, lcps=1.0, state_every=20, state_next=True)
# More than the one archetype the reference ships (traffic_env.py:35-43 is a TABLE, :164 draws a row per car): the
# default car, a long slow truck and a short quick car with delta = 2.  Rows: v, l, a, delta, v0, b, T, s0.
scen("g2x2_three_archetypes", seed=7, T=300, lcps=0.25,
     archetypes=[[11.11, 4, 3, 4, 13.89, 6, 2, 1], [8.0, 8, 1.5, 4, 10.0, 4, 2.5, 2], [12.0, 3.5, 4, 2, 16.0, 7, 1.5, 1]])
scen("g3x3_two_archetypes_c10", m=3, n=3, C=10, seed=8, T=300, lcps=0.2,
     archetypes=[[11.11, 4, 3, 4, 13.89, 6, 2, 1], [8.0, 8, 1.5, 4, 10.0, 4, 2.5, 2]])
# exponents that are no integers (the reference's `**` takes any float, traffic_env.py:56): delta = 2.5, 4 and 0.75
scen("g2x2_archetypes_fractional_delta", seed=9, T=300, lcps=0.25,
     archetypes=[[11.11, 4, 3, 2.5, 13.89, 6, 2, 1], [8.0, 8, 1.5, 4, 10.0, 4, 2.5, 2], [12.0, 3.5, 4, 0.75, 16.0, 7, 1.5, 1]])
# config 5 itself for the first 130 ticks (integers only): 64x64, Poisson arrivals at the default rate
scen("g64x64_c130_ints", m=64, n=64, L=800.0, C=130, seed=0, T=130, state_every=0)


# ---- the second list: runs OFF the reference's defaults, written to tests/golden/params/ -----------------------------
# `rate` other than a power of two (every product with it rounds), `rate` = 1 (coarse steps: cars overshoot v0), one
# ordinary archetype row other than the reference's, several rows at such a rate, the reference's module constants
# replaced, line grids (m = 1 or n = 1) and roads of a few cars.  The subfolder keeps them out of the parametrised
# tests over tests/golden/*.npz; tests/test_oracle_params.py and tests/test_gpu_params.py read them.
OUT_PARAMS = os.path.join(OUT, "params")
PARAM_SCENARIOS = {}
ONE_ROW = [[9.0, 5, 2, 4, 12.0, 5, 2, 1.5]]
TRUCK = [[8.0, 8, 1.5, 4, 10.0, 4, 2.5, 2]]


def pscen(name, **kw):
    kw.setdefault("T", 240)
    scen(name, _table=PARAM_SCENARIOS, **kw)


pscen("rate03", L=120.0, C=16, seed=11, rate=0.3, lcps=0.2)
pscen("rate07", L=120.0, C=16, seed=12, rate=0.7, lcps=0.2)
pscen("rate025", L=120.0, C=16, seed=13, rate=0.25, lcps=0.2)
pscen("rate1_light", L=250.0, C=20, seed=14, rate=1.0, lcps=0.12)
pscen("rate1", L=75.0, C=10, seed=15, rate=1.0, lcps=0.2)
pscen("one_row", L=120.0, C=16, seed=16, lcps=0.25, archetypes=ONE_ROW)
pscen("truck_rate07", L=120.0, C=16, seed=17, rate=0.7, lcps=0.2, archetypes=TRUCK)
pscen("line_1x3", m=1, n=3, L=120.0, C=12, seed=18, lcps=0.25)
pscen("line_3x1", m=3, n=1, L=120.0, C=12, seed=19, lcps=0.25)
pscen("line_1x1", m=1, n=1, L=120.0, C=12, seed=20, lcps=0.5)
pscen("short_2x3_c6", m=2, n=3, L=30.0, C=6, seed=21, lcps=0.2)
pscen("short_2x2_c5_rate1", L=20.0, C=5, seed=22, rate=1.0, lcps=0.15)
pscen("short_2x2_c4_rate1_validate", L=12.0, C=4, seed=23, rate=1.0, lcps=0.15, mode='validate')
pscen("three_rows_rate07", L=120.0, C=16, seed=24, rate=0.7, lcps=0.2,
      archetypes=[[11.11, 4, 3, 4, 13.89, 6, 2, 1], [8.0, 8, 1.5, 4, 10.0, 4, 2.5, 2], [12.0, 3.5, 4, 2, 16.0, 7, 1.5, 1]])
# the reference's module constants (traffic_env.py:17-25) replaced the way CAPACITY is; the detection distance is a
# literal there (:201) and stays 10
pscen("constants", L=120.0, C=16, seed=25, lcps=0.3,
      constants=dict(yellow_ticks=4, thresh=0.35, overflow_penalty=7, eps=3e-7))
REF_CONSTANT_NAMES = dict(yellow_ticks="YELLOW_TICKS", thresh="THRESH", overflow_penalty="OVERFLOW_PENALTY", eps="EPS")


# ---- the third list: runs that START from loaded ring states, written to tests/golden/states/ ---------------------------
# N independent states per scenario, K ticks each, 0-3 scripted arrivals per tick.  State i draws beyond = BEYOND[i % 4],
# crowd from CROWD, and has sorted x where (i // 4 + i) is even: with N = 8 every `beyond` occurs sorted and unsorted,
# with N = 4 every `beyond` occurs once.  On top of the family, the head of about one road in seven stands exactly at the
# road end (x = L, v = 0): the edge of `x > length`.  `ticks`: the clock of every state (60, as in the tests that use the family).
# Seeds: a seed would be replaced, with a note here, if a 1-ulp float at a threshold flipped an integer of the oracle's
# free run (tests/test_oracle_states.py); none had to be.
OUT_STATES = os.path.join(OUT, "states")
STATE_SCENARIOS = {}
# tests/test_gpu_archetypes.py:MIXED_ROWS (exponents 4, 1, 2, 8, 2.5, 0.75)
MIXED_ROWS = [[11.11, 4, 3, 4, 13.89, 6, 2, 1], [8.0, 8, 1.5, 1, 10.0, 4, 2.5, 2], [12.0, 3.5, 4, 2, 16.0, 7, 1.5, 1],
              [9.0, 12, 1.0, 8, 11.0, 3, 3.0, 3], [10.0, 5, 2.5, 2.5, 14.0, 5, 1.8, 1.5], [7.0, 6, 2.0, 0.75, 9.0, 4, 2.2, 2]]


def sscen(name, **kw):
    d = dict(m=2, n=2, L=60.0, C=10, seed=0, N=8, K=6, rate=0.5, learn_switch=False, mode='train', entry='all',
             archetypes=None, constants=None, ticks=None)
    d.update(kw)
    d["ticks"] = list(d["ticks"] or [60] * d["N"])
    assert len(d["ticks"]) == d["N"]
    STATE_SCENARIOS[name] = d


sscen("st_2x2_c10", seed=101)
sscen("st_3x2_c20_validate", m=3, n=2, C=20, L=120.0, seed=102, mode='validate')
sscen("st_2x3_c6_rate1_ls_validate", m=2, n=3, C=6, L=30.0, seed=103, rate=1.0, learn_switch=True, mode='validate')
sscen("st_2x2_c34_rate07", C=34, L=200.0, seed=104, rate=0.7)
sscen("st_2x3_c66", m=2, n=3, C=66, L=400.0, seed=105)
sscen("st_2x2_c130", C=130, L=800.0, seed=106)
sscen("st_1x1_c258", m=1, n=1, C=258, L=900.0, seed=107)
# every car a random row; a ninth state at a clock beyond 2^21 (its cars spawned in the last few hundred ticks)
sscen("st_3x2_c20_rows_validate", m=3, n=2, C=20, L=120.0, seed=108, mode='validate', archetypes=MIXED_ROWS, N=9,
      ticks=[60] * 8 + [3000000])
sscen("st_2x2_c16_constants", C=16, L=120.0, seed=109,
      constants=dict(yellow_ticks=4, thresh=0.35, overflow_penalty=7, eps=3e-7))

TALLIES = ("wrapped_road_ticks", "wrapped_waiting_quirk", "multi_pop_road_ticks", "max_pops", "cascades",
           "handoffs_refused", "spawns_refused", "full_pop_and_receive", "leaders_at_next_tail", "heads_at_road_end", "trips")


def run_states(name, sc, mods):
    """-> the fixture of one scenario of STATE_SCENARIOS (arrays stacked over its N states)"""
    te = mods["gym_traffic.envs.traffic_env"]
    rg = mods["gym_traffic.envs.roadgraph"]
    gym = mods["gym"]
    args = mods["args"]

    te.CAPACITY = C = int(sc["C"])
    args.update_flags(poisson=True, rate=float(sc["rate"]), local_cars_per_sec=0.12, entry=sc["entry"],
                      learn_switch=bool(sc["learn_switch"]), mode=sc["mode"])
    xi, vi, wi = te.xi, te.vi, te.wi
    keep_archetypes = te.archetypes
    keep_constants = {ref: getattr(te, ref) for ref in REF_CONSTANT_NAMES.values()}
    for k, val in (sc.get("constants") or {}).items():
        setattr(te, REF_CONSTANT_NAMES[k], val)
    arch_cols = [te.vi, te.li, te.ai, te.deltai, te.v0i, te.bi, te.ti, te.s0i]
    if sc.get("archetypes"):
        tab = np.zeros((len(sc["archetypes"]), te.params), np.float32)
        tab[:, arch_cols] = np.asarray(sc["archetypes"], np.float32)
        te.archetypes = tab
    n_rows = te.archetypes.shape[0]
    key_cols = arch_cols[1:]

    def row_plane(state):
        """row of te.archetypes each slot's car equals in everything but x, v, w (0 where none does)"""
        out = np.zeros((state.shape[0], state.shape[2]), np.int8)
        for a in range(n_rows):
            out[(state[:, key_cols, :] == te.archetypes[a, key_cols][None, :, None]).all(axis=1)] = a
        return out

    road_length = float(sc["L"])
    tally = dict.fromkeys(TALLIES, 0)
    phase_of = ["idle"]          # "spawn" inside add_new_cars, "advance" inside the advance
    received = set()             # roads that took a handed-off car in the current advance
    orig_add_car, orig_adv, orig_hack, orig_move = te.add_car, te.advance_finished_cars, te.advance_hack, te.move_cars

    def counted_add_car(road, car, state, leading, lastcar, rewards, dests):
        if phase_of[0] == "advance" and car[xi] > road_length:
            tally["cascades"] += 1          # still beyond the road end after the subtraction of :130
        refused = orig_add_car(road, car, state, leading, lastcar, rewards, dests)
        if phase_of[0] == "advance":
            tally["handoffs_refused"] += int(bool(refused))
            if not refused:
                received.add(int(road))
        elif phase_of[0] == "spawn":
            tally["spawns_refused"] += int(bool(refused))
        return refused

    def counted_move(dests, phases, length, nexts, state, leading, lastcar, rate, current_phase, elapsed, *a):
        wrapped = np.nonzero(leading > lastcar)[0]
        tally["wrapped_road_ticks"] += len(wrapped)
        for e, dst in enumerate(dests):        # (the condition of update_lights, :86-90, read - only to count)
            if dst >= 0 and not (phases[e] == current_phase[dst] or elapsed[dst] < te.YELLOW_TICKS) \
                    and nexts[e] >= 0 and lastcar[nexts[e]] != leading[nexts[e]]:
                tally["leaders_at_next_tail"] += 1
        out = orig_move(dests, phases, length, nexts, state, leading, lastcar, rate, current_phase, elapsed, *a)
        for e in wrapped:
            if dests[e] >= 0:                  # :210 counts x < THRESH on the slots 1 .. lastcar, :200 counts v
                by_x = int((state[e, xi, 1:lastcar[e] + 1] < te.THRESH).sum())
                by_v = int((state[e, vi, 1:lastcar[e] + 1] < te.THRESH).sum())
                tally["wrapped_waiting_quirk"] += int(by_x != by_v)
        return out

    def counted_advance(orig):
        def f(dests, length, nexts, state, leading, lastcar, *a):
            before = leading.copy()
            heads = np.where(leading + 1 < C, leading + 1, 1)
            tally["heads_at_road_end"] += int(((leading != lastcar) & (state[np.arange(len(leading)), xi, heads] == length)).sum())
            cars = np.where(leading > lastcar, lastcar + (C - 1) - leading, lastcar - leading)
            phase_of[0] = "advance"
            received.clear()
            try:
                out = orig(dests, length, nexts, state, leading, lastcar, *a)
            finally:
                phase_of[0] = "idle"
            pops = np.where(leading >= before, leading - before, leading + (C - 1) - before)
            tally["multi_pop_road_ticks"] += int((pops >= 2).sum())
            tally["max_pops"] = max(tally["max_pops"], int(pops.max()))
            tally["full_pop_and_receive"] += sum(1 for e in received if cars[e] == C - 2 and pops[e] > 0)
            return out
        return f

    te.add_car = counted_add_car
    te.move_cars = counted_move
    te.advance_finished_cars = counted_advance(orig_adv)
    te.advance_hack = counted_advance(orig_hack)
    try:
        N, K = sc["N"], sc["K"]
        rng = np.random.RandomState(sc["seed"])
        graph = env = None
        per_state = []
        spawn_road, spawn_row, spawn_off, trip_times, trip_off = [], [], [0], [], [0]
        for i in range(N):
            env = gym.make('traffic-v0')
            graph = rg.GridRoad(sc["m"], sc["n"], sc["L"])
            env.set_graph(graph)
            env.seed_generator(sc["seed"])
            env.reset_entrypoints()
            np.random.seed(sc["seed"])
            env.state[:] = 0
            env.rewards[:] = 0
            env.reset()
            Iq, r, R = graph.intersections, graph.train_roads, graph.roads
            tick0 = int(sc["ticks"][i])
            x, v, w, leading, lastcar = [a[0] for a in random_state(
                rng, 1, R, C, sc["L"], crowd=rng.choice(CROWD), beyond=BEYOND[i % 4], sorted_x=(i // 4 + i) % 2 == 0)]
            # what the family does not reach by itself: a standing head exactly AT the road end, which `x > length` (:123)
            # leaves on its road for as long as its light is red
            for e in range(R):
                if lastcar[e] != leading[e] and rng.rand() < 0.15:
                    h = leading[e] + 1 if leading[e] + 1 < C else 1
                    x[e, h], v[e, h] = sc["L"], 0.0
            if tick0 > 400:
                w = (tick0 - 400 + 8 * w).astype(np.float32)
            row = rng.randint(0, n_rows, size=x.shape).astype(np.int8) if sc.get("archetypes") else np.zeros(x.shape, np.int8)
            table = te.archetypes.copy()
            table[:, wi] = 0
            env.state[:] = state_rows(x, v, w, leading, lastcar, table, row)
            env.leading[:] = leading
            env.lastcar[:] = lastcar
            env.current_phase[:] = rng.randint(2, size=Iq)
            env.elapsed[:] = rng.randint(0, 12, size=Iq)
            env.steps = np.float32(tick0)
            for a in (env.waiting, env.passed_dst, env.rewards, env.passed, env.detected):
                a[:] = 0
            env.trip_times = []
            acts = rng.randint(2, size=(K, Iq)).astype(np.int32)
            script_roads = [rng.choice(graph.entrypoints, size=rng.randint(0, 4)).astype(np.int32) for _ in range(K)]
            script_rows = [rng.randint(0, n_rows, size=len(rd)).astype(np.int32) for rd in script_roads]

            # arrivals go through the reference's own add_new_cars (:274-283): it draws the tick's cars from rand_car
            # until None and every car's road from rand.choice
            def cars():
                for rows_t in script_rows:
                    for a in rows_t:
                        yield te.archetypes[a]
                    yield None
            roads_flat = iter([int(rd) for rds in script_roads for rd in rds])

            class Roads(object):
                def choice(self, entrypoints):
                    rd = next(roads_flat)
                    assert rd in entrypoints
                    return rd
            env.rand_car = cars()
            env.rand = Roads()
            orig_add_new = env.add_new_cars

            def add_new(tick, orig_add_new=orig_add_new):
                phase_of[0] = "spawn"
                try:
                    return orig_add_new(tick)
                finally:
                    phase_of[0] = "idle"
            env.add_new_cars = add_new

            rec = dict(leading=[], lastcar=[], obs=[], rewards=[], waiting=[], passed_dst=[], leader_x=[], state_x=[],
                       state_v=[], state_w=[], state_a=[], done=[0], trip_count=[0])

            def record():
                rec["leading"].append(env.leading.copy())
                rec["lastcar"].append(env.lastcar.copy())
                rec["obs"].append(env.obs.copy())
                rec["rewards"].append(env.rewards.copy())
                rec["waiting"].append(env.waiting.copy())
                rec["passed_dst"].append(env.passed_dst.astype(np.uint8))
                rec["leader_x"].append(env.state[np.arange(R), xi, env.leading].copy())
                px, pv, pw = live_planes(env.state, env.leading, env.lastcar, C, (xi, vi, wi))
                live = live_slots(env.leading, env.lastcar, C)
                assert np.isfinite(px[live]).all() and np.isfinite(pv[live]).all(), (name, i, "a live value is not finite")
                rec["state_x"].append(px)
                rec["state_v"].append(pv)
                rec["state_w"].append(pw)
                rec["state_a"].append(np.where(live, row_plane(env.state), 0).astype(np.int8))
            record()
            assert np.array_equal(rec["state_a"][0], np.where(live_slots(leading, lastcar, C), row, 0))
            for t in range(K):
                _, _, d, _ = env.step(acts[t].copy())
                rec["done"].append(int(bool(d)))
                rec["trip_count"].append(len(env.trip_times))
                record()
                spawn_road.extend(script_roads[t].tolist())
                spawn_row.extend(script_rows[t].tolist())
                spawn_off.append(len(spawn_road))
            assert next(env.rand_car, "end") == "end" and next(roads_flat, "end") == "end"
            tally["trips"] += len(env.trip_times)
            trip_times.extend(env.trip_times)
            trip_off.append(len(trip_times))
            rec["actions"] = acts
            per_state.append(rec)
        out = dict(phases=graph.phases.copy(), dest=graph.dest.copy(), nexts=graph.nexts.copy(),
                   entrypoints=graph.entrypoints.copy(), ticks=np.asarray(sc["ticks"], np.int64))
        for k in per_state[0]:
            out[k] = np.stack([np.asarray(rec[k]) for rec in per_state])          # [N, K + 1 (actions: K), ...]
        for k in ("leading", "lastcar", "obs", "waiting"):
            out[k] = out[k].astype(np.int32)
        out.update(done=out["done"].astype(np.uint8), trip_count=out["trip_count"].astype(np.int64),
                   spawn_off=np.asarray(spawn_off, np.int64).reshape(-1),       # cars of state i, tick t: [i * K + t]
                   spawn_road=np.asarray(spawn_road, np.int32), spawn_arch=np.asarray(spawn_row, np.int32),
                   trip_times=np.asarray(trip_times, np.float64), trip_off=np.asarray(trip_off, np.int64))
        if sc.get("archetypes"):
            out["archetypes"] = te.archetypes.copy()
        for k in TALLIES:
            out["tally_" + k] = np.int64(tally[k])
        out["scenario"] = np.array(json.dumps(sc))
        out["numpy_version"] = np.array(np.__version__)
        return out
    finally:
        te.add_car, te.move_cars, te.advance_finished_cars, te.advance_hack = orig_add_car, orig_move, orig_adv, orig_hack
        te.archetypes = keep_archetypes
        for ref, val in keep_constants.items():
            setattr(te, ref, val)


def run(name, sc, mods):
    te = mods["gym_traffic.envs.traffic_env"]
    rg = mods["gym_traffic.envs.roadgraph"]
    gym = mods["gym"]
    args = mods["args"]
    FLAGS = args.FLAGS

    te.CAPACITY = int(sc["C"])
    args.update_flags(poisson=bool(sc["poisson"]), rate=float(sc["rate"]),
                      local_cars_per_sec=float(sc["lcps"]), entry=sc["entry"],
                      learn_switch=bool(sc["learn_switch"]), mode=sc["mode"])
    C = te.CAPACITY
    xi, vi, wi = te.xi, te.vi, te.wi
    keep_archetypes = te.archetypes
    keep_constants = {ref: getattr(te, ref) for ref in REF_CONSTANT_NAMES.values()}
    for k, val in (sc.get("constants") or {}).items():
        setattr(te, REF_CONSTANT_NAMES[k], val)
    arch_cols = [te.vi, te.li, te.ai, te.deltai, te.v0i, te.bi, te.ti, te.s0i]
    if sc.get("archetypes"):
        tab = np.zeros((len(sc["archetypes"]), te.params), np.float32)
        tab[:, arch_cols] = np.asarray(sc["archetypes"], np.float32)
        te.archetypes = tab
    spawn_arch_log = []     # archetype row of every car spawned in the current tick

    def arch_of(state):
        """Row of te.archetypes each slot's car was copied from (by its length, accel, ... - everything but x, v, w);
        -1 where no row matches (dead slots, fake leaders)."""
        key = state[:, [te.li, te.ai, te.deltai, te.v0i, te.bi, te.ti, te.s0i], :]          # [R, 7, C]
        rows = te.archetypes[:, [te.li, te.ai, te.deltai, te.v0i, te.bi, te.ti, te.s0i]]   # [n, 7]
        out = np.full((state.shape[0], state.shape[2]), -1, np.int8)
        for a in range(rows.shape[0]):
            out[(key == rows[a][None, :, None]).all(axis=1)] = a
        return out

    spawn_log = []          # roads of cars spawned in the current tick
    in_spawn = [False]
    mid_snap = {}

    orig_add_car = te.add_car
    orig_adv = te.advance_finished_cars
    orig_hack = te.advance_hack

    def logged_add_car(road, car, *a):
        if in_spawn[0]:
            spawn_log.append(int(road))
            rows = te.archetypes[:, arch_cols[1:]]
            spawn_arch_log.append(int(np.argmax((rows == np.asarray(car)[arch_cols[1:]][None, :]).all(axis=1))))
        return orig_add_car(road, car, *a)

    def snap_mid(state, leading, lastcar):
        mid_snap["x"], mid_snap["v"] = live_planes(state, leading, lastcar, C, (xi, vi))

    def logged_adv(dests, length, nexts, state, leading, lastcar, *a):
        snap_mid(state, leading, lastcar)
        return orig_adv(dests, length, nexts, state, leading, lastcar, *a)

    def logged_hack(dests, length, nexts, state, leading, lastcar, *a):
        snap_mid(state, leading, lastcar)
        return orig_hack(dests, length, nexts, state, leading, lastcar, *a)

    te.add_car = logged_add_car
    te.advance_finished_cars = logged_adv
    te.advance_hack = logged_hack
    try:
        env = gym.make('traffic-v0')
        graph = rg.GridRoad(sc["m"], sc["n"], sc["L"])
        env.set_graph(graph)
        env.seed_generator(sc["seed"])
        env.reset_entrypoints()
        orig_add_new = env.add_new_cars

        def add_new(tick):
            in_spawn[0] = True
            try:
                return orig_add_new(tick)
            finally:
                in_spawn[0] = False
        env.add_new_cars = add_new

        np.random.seed(sc["seed"])
        # np.empty garbage in never-written arrays is not a golden value: pin it to 0 so the
        # fixture is reproducible (detected/rewards/waiting are stale-on-purpose in the
        # reference, traffic_env.py:259-272; their *initial* content is undefined there).
        env.state[:] = 0
        env.rewards[:] = 0
        env.reset()
        Iq, r, R = graph.intersections, graph.train_roads, graph.roads
        T = sc["T"]
        arng = np.random.RandomState(sc["seed"] + 1)

        out = dict(
            phases=graph.phases.copy(), dest=graph.dest.copy(), nexts=graph.nexts.copy(),
            entrypoints=graph.entrypoints.copy(), cars_per_sec=np.float64(FLAGS.cars_per_sec),
            init_phase=env.current_phase.copy(),
        )
        actions = np.zeros((T, Iq), np.int32)
        leading = np.zeros((T + 1, R), np.int32)
        lastcar = np.zeros((T + 1, R), np.int32)
        obs = np.zeros((T + 1, 2 * r + 2 * Iq), np.int32)
        rewards = np.zeros((T + 1, Iq), np.float32)
        waiting = np.zeros((T + 1, r), np.int32)
        passed_dst = np.zeros((T + 1, Iq), np.uint8)
        done = np.zeros(T + 1, np.uint8)
        leader_x = np.zeros((T + 1, R), np.float32)
        spawn_off = np.zeros(T + 1, np.int64)
        spawn_road = []
        spawn_arch = []
        se = sc["state_every"]
        st_ticks, st_x, st_v, st_w, st_a, mid_x, mid_v = [], [], [], [], [], [], []
        remi_ticks, remi_rew, cor = [], [], []
        trip_count = np.zeros(T + 1, np.int64)

        def record(k):
            leading[k] = env.leading
            lastcar[k] = env.lastcar
            obs[k] = env.obs
            rewards[k] = env.rewards
            waiting[k] = env.waiting
            passed_dst[k] = env.passed_dst
            leader_x[k] = env.state[np.arange(R), xi, env.leading]
            if se and (k % se == 0 or (sc.get("state_next") and k % se == 1)):
                x, v, w = live_planes(env.state, env.leading, env.lastcar, C, (xi, vi, wi))
                st_ticks.append(k)
                st_x.append(x)
                st_v.append(v)
                st_w.append(w)
                if sc.get("archetypes"):
                    live = (x != 0) | (v != 0) | (w != 0)
                    a = arch_of(env.state)
                    st_a.append(np.where(a >= 0, a, 0).astype(np.int8))

        env.waiting[:] = 0
        record(0)
        cur = None
        for t in range(T):
            if sc["actions"] == 'random10':
                if t % 10 == 0:
                    cur = arng.randint(2, size=Iq).astype(np.int32)
            elif sc["actions"] == 'cycle3':
                cur = np.full(Iq, int((t % 6) >= 3), np.int32)
            elif sc["actions"] == 'const0':
                cur = np.zeros(Iq, np.int32)
            actions[t] = cur
            del spawn_log[:]
            del spawn_arch_log[:]
            # the reference accepts any dtype here (bool from a3c, float64 from const0)
            _, _, d, _ = env.step(cur.copy())
            spawn_road.extend(spawn_log)
            spawn_arch.extend(spawn_arch_log)
            spawn_off[t + 1] = len(spawn_road)
            done[t + 1] = bool(d)
            trip_count[t + 1] = len(env.trip_times)
            if sc["mid"]:
                mid_x.append(mid_snap["x"])
                mid_v.append(mid_snap["v"])
            record(t + 1)
            if sc["remi_every"] and (t + 1) % sc["remi_every"] == 0:
                cor.append(env.cars_on_roads().copy())
                remi_rew.append(env.remi_reward().copy())
                remi_ticks.append(t + 1)
        out.update(actions=actions, leading=leading, lastcar=lastcar, obs=obs, rewards=rewards,
                   waiting=waiting, passed_dst=passed_dst, done=done, leader_x=leader_x,
                   spawn_off=spawn_off, spawn_road=np.asarray(spawn_road, np.int32),
                   generated_cars=np.int64(env.generated_cars),
                   remi_ticks=np.asarray(remi_ticks, np.int64),
                   remi_rewards=np.asarray(remi_rew, np.float32).reshape(len(remi_ticks), Iq),
                   cars_on_roads=np.asarray(cor, np.int32).reshape(len(remi_ticks), sc["m"], sc["n"], 4),
                   trip_times=np.asarray(env.trip_times, np.float64), trip_count=trip_count)
        if se:
            out.update(state_ticks=np.asarray(st_ticks, np.int64), state_x=np.stack(st_x),
                       state_v=np.stack(st_v), state_w=np.stack(st_w))
        if sc.get("archetypes"):
            out.update(archetypes=te.archetypes.copy(), spawn_arch=np.asarray(spawn_arch, np.int32),
                       state_a=np.stack(st_a))
        if sc["mid"]:
            out.update(mid_x=np.stack(mid_x), mid_v=np.stack(mid_v))
        out["scenario"] = np.array(json.dumps(sc))
        out["numpy_version"] = np.array(np.__version__)
        return out
    finally:
        te.add_car = orig_add_car
        te.advance_finished_cars = orig_adv
        te.advance_hack = orig_hack
        te.archetypes = keep_archetypes
        for ref, val in keep_constants.items():
            setattr(te, ref, val)


def live_planes(state, leading, lastcar, C, planes):
    """Copies of the requested parameter planes [R, C] with every slot that is neither a live
    car nor the fake leader set to 0 (dead slots / slot 0 hold garbage in the reference)."""
    R = state.shape[0]
    slots = np.arange(C)[None, :]
    ld = leading[:, None]
    lc = lastcar[:, None]
    unwrapped = (slots > ld) & (slots <= lc)
    wrapped = (slots > ld) | ((slots >= 1) & (slots <= lc))
    live = np.where(ld <= lc, unwrapped, wrapped) & (ld != lc)
    keep = live | (slots == ld)
    outs = []
    for p in planes:
        a = state[:, p, :].copy()
        a[~keep] = 0
        outs.append(a)
    return outs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None)
    ap.add_argument("--set", default="all", choices=["all", "main", "params", "states"],
                    help="main: tests/golden/, params: tests/golden/params/ (the runs off the defaults), "
                         "states: tests/golden/states/ (the runs from loaded ring states)")
    a = ap.parse_args()
    mods = load_reference()
    todo = [(OUT, n, sc) for n, sc in SCENARIOS.items() if a.set in ("all", "main")]
    todo += [(OUT_PARAMS, n, sc) for n, sc in PARAM_SCENARIOS.items() if a.set in ("all", "params")]
    todo += [(OUT_STATES, n, sc) for n, sc in STATE_SCENARIOS.items() if a.set in ("all", "states")]
    for folder, name, sc in todo:
        if a.only and a.only != name:
            continue
        os.makedirs(folder, exist_ok=True)
        if folder == OUT_STATES:
            out = run_states(name, sc, mods)
            path = os.path.join(folder, name + ".npz")
            np.savez_compressed(path, **out)
            print("%-30s N=%d K=%d %s  %.1f KB" % (name, sc["N"], sc["K"], " ".join(
                "%s=%d" % (k, int(out["tally_" + k])) for k in TALLIES), os.path.getsize(path) / 1024.0))
            continue
        out = run(name, sc, mods)
        path = os.path.join(folder, name + ".npz")
        np.savez_compressed(path, **out)
        print("%-24s T=%d spawned=%d overflow_ticks=%d trips=%d  %.1f KB" % (
            name, sc["T"], int(out["generated_cars"]), int(out["done"].sum()),
            len(out["trip_times"]), os.path.getsize(path) / 1024.0))


if __name__ == "__main__":
    main()
