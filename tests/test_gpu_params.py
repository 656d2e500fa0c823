"""Every step path OFF the default car, rate and constants.

The C ABI takes the car (car_v .. car_s0, or one row through `arch`), `rate`, yellow_ticks, thresh, detect_dist,
overflow_penalty and eps as runtime values; everywhere else in this suite the single-archetype kernels run the
reference's default row at rate 0.25, 0.5 or 1.0 - powers of two, with which every product is exact - and the default
constants.  A kernel with one of those numbers written into it, or with the expression order around `rate` changed
(dx = r v + (0.5 dvr) r, traffic_env.py:58-59), would pass all of it.  Here every kernel family of DESIGN section 4 runs
at three parameter points (POINTS):

  P1  rate 0.3, the row [9, 5, 2, 4, 12, 5, 2, 1.5] (v, l, a, delta, v0, b, T, s0) given as a one-row table
  P2  rate 0.7, the row [8, 8, 1.5, 4, 10, 4, 2.5, 2]
  P3  rate 0.5, the default row, yellow_ticks 4, thresh 0.35, detect_dist 17.5, overflow_penalty 7, eps 3e-7

Part A, device against the oracle, bit for bit, on ragged states (tests/test_gpu_stride_rounds.py: ragged_state, load_both
and its call pattern - a fresh state per call, per-env per-tick random actions and arrival counts, calls of 3, 4, 7, 2, 5
and 1 ticks, every env compared after every call): 5 envs of the 3x3 grid of 120 m roads, C = 14 (C = 34 / 66 where 2, 4 or
8 segments need rings that long).  Which case covers which kernel family:

  kernel family                 case
  k_res, 1 / 2 / 4 / mixed lanes per road, three   test_plain_calls[res_lpr1 | res_lpr2 | res_lpr4 | res_lpr3], ring:
    envs per workgroup; ring layout resident         [res_ring] (k_res does not serve validate mode: res_usable)
  k_move_t, k_move_ts (+ k_advance)                test_plain_calls[move_t | move_ts] and their validate forms
  k_move_tt + k_tail | three launches | split      test_plain_calls[pairs_tail | pairs_launches | pairs_split] (W forms:
    (k_edge, k_advance; odd tick on k_move_ts)       [pairs_tail-validate], [pairs_split-validate])
  k_move_tts, S = 2, 4, 8                          test_plain_calls[tts2 | tts4 | tts8], [tts4-validate]
  k_move_dma, k_move<1> (ring layout)              test_plain_calls[ring_dma | ring_move] and their validate forms
  HET forms: k_move_tt, k_edge, k_tail, k_move_t   test_mixed_rows_at_rates_that_round (MIXED_ROWS at rate 0.3 and 0.7)
  idm_step_fast against the IEEE divisions         test_fast_division_on_and_off (k_div_selftest at these divisors)
  k_risk, the AGENT forms, k_agent_tail, k_remi    test_agent_steps (P1, P2: the bound's a and rate; k_res, tick by tick,
                                                     pairs through the captured graph and eagerly; remi on and off)
  k_poisson (Poisson and regular streams)          test_device_arrivals (P1, pairs)
  k_frames (reads car_l), k_measure                test_frames_draw_the_rows_own_car_length, test_road_measures (P2)

Part B, device against the reference runs of tests/golden/params/ (tests/test_oracle_params.py states the bars): integers
free-running, floats teacher-forced with the same bounds and the same two bit-equal shares, on the handle's own choice of
path and on TFX_RESIDENT=0; the one-row and the three-row run through the gym surface as well.  The line grids (1x3, 3x1,
1x1) and the C = 4 / 5 / 6 runs are the smallest tiles and rings these kernels see anywhere.

The CPU tests of this module run the oracle alone through the same inputs and assert what the cases rely on: rings
overflow in the plain calls, envs end at different ticks of a decision next to envs that run on.

No case provokes a fault; every switch used here is one the suite already uses."""
import os

import numpy as np
import pytest

from oracle.oracle import OracleEnv, live_mask
from test_gpu_parity import assert_same_state, same_bits
from test_gpu_stride_rounds import (BEYOND, ROWS_PER_ROAD, arrival_counts, assert_decision, assert_pair_counters,
                                    assert_rows_and_trips, csr, device_tick, emulate_decision, load_both, load_oracle,
                                    ragged_state, rows_of, tab10_of)
from test_oracle_params import (Tally, check_floats, constants_of, fixture, ints_differ, param_names, sc_remi, table_of)

gpu = pytest.mark.gpu

M, N, LENGTH = 3, 3, 120.0
E, C_SHORT = 5, 14
CALLS = [3, 4, 7, 2, 5, 1]
ROW_P1 = [9.0, 5, 2, 4, 12.0, 5, 2, 1.5]
ROW_P2 = [8.0, 8, 1.5, 4, 10.0, 4, 2.5, 2]
POINTS = {
    "P1": dict(rate=0.3, row=ROW_P1, constants=None),
    "P2": dict(rate=0.7, row=ROW_P2, constants=None),
    "P3": dict(rate=0.5, row=None, constants=dict(yellow_ticks=4, thresh=0.35, detect_dist=17.5, overflow_penalty=7, eps=3e-7)),
}
# exponents 4, 1, 2, 8, 2.5 and 0.75: tests/test_gpu_archetypes.py:MIXED_ROWS
MIXED_ROWS = np.array([[11.11, 4, 3, 4, 13.89, 6, 2, 1], [8.0, 8, 1.5, 1, 10.0, 4, 2.5, 2],
                       [12.0, 3.5, 4, 2, 16.0, 7, 1.5, 1], [9.0, 12, 1.0, 8, 11.0, 3, 3.0, 3],
                       [10.0, 5, 2.5, 2.5, 14.0, 5, 1.8, 1.5], [7.0, 6, 2.0, 0.75, 9.0, 4, 2.2, 2]], np.float32)

PAIRS = {"TFX_RESIDENT": "0", "TFX_PAIRS": "2", "TFX_TAIL": "2", "TFX_SPLIT": "0", "TFX_TT_SEG": "0"}
PERTICK = {"TFX_RESIDENT": "0", "TFX_PAIRS": "0"}


def res(lpr):
    return {"TFX_RESIDENT": "1", "TFX_RES_EPB": "3", "TFX_RES_LPR": str(lpr)}


def tts(S):
    return dict(PAIRS, TFX_TT_SEG="2", TFX_TT_SEGS=str(S))


def even_odd(even, odd):
    return lambda T: even if T % 2 == 0 else odd


# name -> (switches, C, layout, the mover of a T-tick call's last tick, k_tail follows the pass, the call splits)
PATHS = {
    "res_lpr1": (res(1), C_SHORT, "transposed", lambda T: "k_res", None, None),
    "res_lpr2": (res(2), C_SHORT, "transposed", lambda T: "k_res", None, None),
    "res_lpr4": (res(4), C_SHORT, "transposed", lambda T: "k_res", None, None),
    "res_lpr3": (res(3), C_SHORT, "transposed", lambda T: "k_res", None, None),
    "res_ring": (res(2), C_SHORT, "ring", lambda T: "k_res", None, None),
    "move_t": (dict(PERTICK, TFX_MOVE_VARIANT="91"), C_SHORT, "transposed", lambda T: "k_move_t", None, None),
    "move_ts": (dict(PERTICK, TFX_MOVE_VARIANT="90"), C_SHORT, "transposed", lambda T: "k_move_ts", None, None),
    "pairs_tail": (dict(PAIRS), C_SHORT, "transposed", even_odd("k_move_tt", "k_move_ts"), True, False),
    "pairs_launches": (dict(PAIRS, TFX_TAIL="0"), C_SHORT, "transposed", even_odd("k_move_tt", "k_move_ts"), False, False),
    "pairs_split": (dict(PAIRS, TFX_SPLIT="2"), C_SHORT, "transposed", even_odd("k_move_tt", "k_move_ts"), True, True),
    "tts2": (tts(2), 34, "transposed", even_odd("k_move_tts", "k_move_ts"), True, False),
    "tts4": (tts(4), 34, "transposed", even_odd("k_move_tts", "k_move_ts"), True, False),
    "tts8": (tts(8), 66, "transposed", even_odd("k_move_tts", "k_move_ts"), True, False),
    "ring_dma": ({"TFX_RESIDENT": "0", "TFX_MOVE_VARIANT": "2"}, C_SHORT, "ring", lambda T: "k_move_dma", None, None),
    "ring_move": ({"TFX_RESIDENT": "0", "TFX_MOVE_VARIANT": "0"}, C_SHORT, "ring", lambda T: "k_move", None, None),
}
VALIDATE_TOO = ["move_t", "move_ts", "pairs_tail", "pairs_split", "tts4", "ring_dma", "ring_move"]
PLAIN_CASES = [(p, False) for p in PATHS] + [(p, True) for p in VALIDATE_TOO]


# ---- handles and oracles at a parameter point ---------------------------------------------------------------------------
def with_switches(knobs, make):
    """make() under exactly the TFX_* switches of `knobs`: every other one is taken out of the environment while
    tfx_create and tfx_bind_buffers read it (TFX_LIB names the library itself)"""
    keep = {k: v for k, v in os.environ.items() if k.startswith("TFX_") and k != "TFX_LIB"}
    for k in keep:
        del os.environ[k]
    os.environ.update(knobs)
    try:
        return make()
    finally:
        for k in knobs:
            os.environ.pop(k, None)
        os.environ.update(keep)


def make_engine(point, knobs, C=C_SHORT, n_envs=E, rate=None, **cfg):
    from gym_traffic.core import TfxEngine
    p = POINTS[point] if isinstance(point, str) else point
    cfg.setdefault("layout", "transposed")
    if p["row"] is not None:
        cfg.setdefault("archetypes", [p["row"]])
    return with_switches(knobs, lambda: TfxEngine(M, N, LENGTH, C, n_envs=n_envs, rate=p["rate"] if rate is None else rate,
                                                  constants=p["constants"], **cfg))


def row10(row8):
    if row8 is None:
        return None
    out = np.zeros(10, np.float32)
    out[1:9] = row8
    return out


def oracle_at(point, tables, C=C_SHORT, n_envs=E, validate=False, rate=None):
    p = POINTS[point] if isinstance(point, str) else point
    dest, phases, nexts, entry = tables
    orc = OracleEnv(M, N, LENGTH, C, dest, phases, nexts, n_envs=n_envs, rate=p["rate"] if rate is None else rate,
                    validate=validate, archetype=row10(p["row"]), constants=p["constants"])
    orc.entrypoints = np.asarray(entry, np.int32)
    return orc


def tables_of(eng):
    return eng.dest, eng.phases, eng.nexts, eng.entrypoints


def host_tables():
    """the 3x3 grid's tables without a handle (the CPU tests)"""
    from gym_traffic.envs.roadgraph import GridRoad
    g = GridRoad(M, N, LENGTH)
    g.generate_entrypoints(0)
    return np.asarray(g.dest, np.int32), np.asarray(g.phases, np.int32), np.asarray(g.nexts, np.int32), np.asarray(g.entrypoints, np.int32)


# ---- plain calls ---------------------------------------------------------------------------------------------------------
def plain_inputs(seed, n_envs, R, C, I, n_entry, calls=CALLS, n_rows=0, sorted_x=True, spawn_mean=0.08):
    """What the calls of a plain-call case run on, call by call: a fresh ragged state, light words, per-env per-tick
    actions and arrival counts (and, n_rows > 0, every car's and every arrival's table row)"""
    rng = np.random.RandomState(seed)
    out = []
    for T in calls:
        d = dict(T=T)
        d["state"] = ragged_state(rng, n_envs, R, C, LENGTH, crowd=rng.choice([0.3, 0.8]), beyond=rng.choice(BEYOND), sorted_x=sorted_x)
        d["arch"] = rng.randint(0, n_rows, size=d["state"][0].shape).astype(np.uint8) if n_rows else None
        d["phase"] = rng.randint(2, size=(n_envs, I)).astype(np.int32)
        d["elapsed"] = rng.randint(0, 12, size=(n_envs, I)).astype(np.int32)
        d["acts"] = rng.randint(2, size=(T, n_envs, I)).astype(np.int32)
        d["cnt"] = arrival_counts(rng, T, n_envs, n_entry, spawn_mean)
        d["rows"] = rng.randint(0, n_rows, size=(T, n_envs, n_entry, ROWS_PER_ROAD)).astype(np.uint8) if n_rows else None
        out.append(d)
    return out


def load_oracle_call(orc, d, tab10):
    """the oracle's half of load_both"""
    x, v, w, leading, lastcar = d["state"]
    if d["arch"] is None:
        load_oracle(orc, x, v, w, leading, lastcar)
    else:
        for k in range(orc.E):
            orc.load_planes(k, x[k], v[k], w[k], leading[k], lastcar[k], arch=d["arch"][k], archetypes=tab10)
    orc.obs[:] = 0
    orc.obs[:, 2 * orc.r:2 * orc.r + orc.I] = d["phase"]
    orc.obs[:, 2 * orc.r + orc.I:] = d["elapsed"]
    for a in (orc.waiting, orc.passed_dst, orc.rewards, orc.n_trips):
        a[:] = 0


def oracle_call(orc, d, tab10):
    """the call's ticks on the oracle -> the envs in which a ring overflowed"""
    orc.steps[:] = 60
    done = np.zeros(orc.E, bool)
    for t in range(d["T"]):
        off, roads = csr(d["cnt"][t], orc.entrypoints)
        spawn_arch = rows_of(d["cnt"][t], d["rows"][t], off) if d["rows"] is not None else None
        done |= orc.step(d["acts"][t], (off, roads), spawn_arch=spawn_arch, archetypes=tab10)[2].astype(bool)
    return done


def run_plain_calls(eng, orc, seed, kernel_after, sorted_x=True, others=()):
    """The call pattern of tests/test_gpu_stride_rounds.py:run_plain_calls at a parameter point.  others: further
    handles that get the same calls and must hold the same state."""
    tab10 = tab10_of(eng.archetypes) if eng.het else None
    inputs = plain_inputs(seed, eng.E, eng.R, eng.C, eng.I, eng.n_entry, n_rows=len(tab10) if eng.het else 0, sorted_x=sorted_x)
    eng.reset_counters()
    overflowed = 0
    for trial, d in enumerate(inputs):
        T = d["T"]
        for e_ in (eng,) + tuple(others):
            load_both(e_, orc, d["state"], d["phase"], d["elapsed"], d["arch"], tab10)
            e_.set_tick(60)
            e_.set_actions(d["acts"], per_tick=True)
            e_.set_spawns(counts=d["cnt"], per_tick=True, rows=d["rows"])
            e_.step(T)
        done = oracle_call(orc, d, tab10)
        where = "call %d (%d ticks)" % (trial, T)
        overflowed += int(done.sum())
        for e_ in (eng,) + tuple(others):
            assert np.array_equal(e_.done.cpu().numpy().astype(bool), done), "done " + where
            assert_same_state(e_, orc, where)
            assert_rows_and_trips(e_, orc, tab10, where)
            assert e_.tick == device_tick(e_) == 60 + T, where
        assert eng.vehicle_updates() == orc.vehicle_updates, "vehicle updates " + where
        assert eng.step_kernel() == kernel_after(T), (eng.step_kernel(), where)
    assert overflowed > 0


def plain_seed(point, path, validate):
    return 7000 + 100 * int(point[1]) + 3 * sorted(PATHS).index(path) + int(validate)


@gpu
@pytest.mark.parametrize("path,validate", PLAIN_CASES, ids=[p + ("-validate" if v else "") for p, v in PLAIN_CASES])
@pytest.mark.parametrize("point", sorted(POINTS))
def test_plain_calls(point, path, validate):
    knobs, C, layout, kernel_after, tail, split = PATHS[path]
    planes = 3 if (validate or layout == "ring") else 2
    eng = make_engine(point, knobs, C, layout=layout, planes=planes, validate=validate)
    assert (eng.E, eng.R, eng.I, eng.n_entry, eng.het) == (5, 48, 9, 12, False)
    if path.startswith("tts"):
        assert (C - 2) // int(knobs["TFX_TT_SEGS"]) >= 8                      # every segment of a full ring holds cars
    orc = oracle_at(point, tables_of(eng), C, validate=validate)
    run_plain_calls(eng, orc, plain_seed(point, path, validate), kernel_after, sorted_x=path != "pairs_launches")
    if path.startswith("res"):
        assert eng.fused_ticks() == (sum(CALLS), True) and eng.pair_ticks() == 0
    else:
        assert eng.fused_ticks()[0] == 0
        if tail is None:
            assert eng.pair_ticks() == 0 and eng.split_ticks() == 0
        else:
            assert_pair_counters(eng, tail, split, CALLS)


def test_plain_call_inputs_overflow_on_the_oracle():
    """CPU: the inputs of the plain-call cases on the oracle alone, at every point - rings overflow (the penalty and
    `done` are exercised), cars wait and are detected under the point's own thresholds, rewards carry the point's penalty."""
    tables = host_tables()
    assert (len(tables[0]), len(tables[3])) == (48, 12)
    for point in sorted(POINTS):
        orc = oracle_at(point, tables)
        pen = float(orc.constants["overflow_penalty"])
        overflowed = penalised = 0
        for d in plain_inputs(plain_seed(point, "pairs_tail", False), E, 48, C_SHORT, 9, 12):
            load_oracle_call(orc, d, None)
            overflowed += int(oracle_call(orc, d, None).sum())
            penalised += int((orc.rewards == -pen).sum())
            assert orc.waiting.sum() > 0 and orc.detected.sum() > 0
        assert overflowed > 0 and penalised > 0, point


# ---- heterogeneous cars at rates that round -------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("path", ["pairs_tail", "pairs_launches", "pairs_split", "move_t"])
@pytest.mark.parametrize("rate", [0.3, 0.7])
def test_mixed_rows_at_rates_that_round(rate, path):
    """MIXED_ROWS (six rows, exponents 4, 1, 2, 8, 2.5, 0.75) through the HET forms of the pass, of k_tail, of k_edge and
    of k_move_t - idm_step_het's products with `rate`"""
    knobs, C, layout, _, tail, split = PATHS[path]
    point = dict(rate=rate, row=None, constants=None)
    eng = make_engine(point, knobs, C, planes=3, archetypes=MIXED_ROWS)
    assert eng.het
    orc = oracle_at(point, tables_of(eng), C)
    run_plain_calls(eng, orc, 8000 + int(10 * rate) + len(path), lambda T: "k_move_t" if path == "move_t" else "k_move_tt")
    if tail is None:
        assert eng.pair_ticks() == 0
    else:
        assert_pair_counters(eng, tail, split, CALLS)


# ---- the fast division on and off -----------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("path", ["res_lpr2", "pairs_tail", "move_t"])
@pytest.mark.parametrize("point", sorted(POINTS))
def test_fast_division_on_and_off(point, path):
    """TFX_FASTDIV=0 (IEEE divisions) and the default (the reciprocal form, if the handle's self-test over these
    divisors - 2 sqrt(a b) and v0 of the point's row - kept it): the same calls, the same state, both the oracle's."""
    knobs, C, layout, kernel_after, _, _ = PATHS[path]
    fast = make_engine(point, knobs, C, planes=2)
    ieee = make_engine(point, dict(knobs, TFX_FASTDIV="0"), C, planes=2)
    print("tfx_fastdiv_status at %s: default %s, TFX_FASTDIV=0 %s" % (point, fast.fastdiv_status(), ieee.fastdiv_status()))
    assert not ieee.fastdiv_status()["enabled"]
    orc = oracle_at(point, tables_of(fast), C)
    run_plain_calls(fast, orc, 8500 + int(point[1]) + len(path), kernel_after, others=(ieee,))
    from test_gpu_parity import assert_engines_equal
    assert_engines_equal(fast, ieee)


# ---- agent steps ------------------------------------------------------------------------------------------------------------
AGENT_PATHS = {
    "res": (res(2), lambda T: "k_res"),
    "pertick": (dict(PERTICK), None),
    "pairs_graph": (dict(PAIRS, TFX_GRAPH="1"), None),
    "pairs_eager": (dict(PAIRS, TFX_GRAPH="0"), None),
}
DECISIONS = [4, 5, 4, 5]


def decision_inputs(seed, n_envs, R, C, I, n_entry, entry, lengths=DECISIONS, per_state=3, spawn_mean=0.12):
    """States crowded enough that the bound sorts envs out, without full rings (envs end one after another), a held random
    action and per-tick arrival counts per decision (tests/test_gpu_stride_rounds.py:run_decisions)"""
    rng = np.random.RandomState(seed)
    out = []
    for trial, T in enumerate(lengths):
        d = dict(T=T, arch=None, rows=None)
        d["state"] = ragged_state(rng, n_envs, R, C, LENGTH, crowd=rng.choice([0.5, 0.8]), beyond=rng.choice(BEYOND[:3]),
                                  sorted_x=bool(trial % 2), full="none", entry_roads=entry)
        d["phase"] = rng.randint(2, size=(n_envs, I)).astype(np.int32)
        d["elapsed"] = rng.randint(0, 12, size=(n_envs, I)).astype(np.int32)
        d["steps"] = [(rng.randint(2, size=(n_envs, I)).astype(np.int32), arrival_counts(rng, T, n_envs, n_entry, spawn_mean))
                      for _ in range(per_state)]
        out.append(d)
    return out


def run_decisions(eng, orc, seed, remi):
    """eng None: the oracle alone.  -> the tick at which each env ended, per decision"""
    ends = []
    for trial, d in enumerate(decision_inputs(seed, orc.E, orc.R, orc.C, orc.I, len(orc.entrypoints), orc.entrypoints)):
        if eng is None:
            load_oracle_call(orc, d, None)
        else:
            load_both(eng, orc, d["state"], d["phase"], d["elapsed"])
            eng.set_tick(40)
        tick0 = 40
        for step, (act, cnt) in enumerate(d["steps"]):
            want = emulate_decision(orc, tick0, act, lambda t, frozen: (cnt[t], None), d["T"], remi)
            if eng is not None:
                eng.set_actions(act)
                eng.set_spawns(counts=cnt, per_tick=True)
                out = eng.agent_step(d["T"], remi=remi)
                where = "state %d decision %d (%d ticks)" % (trial, step, d["T"])
                assert_decision(eng, orc, out, want, None, where)
                assert eng.tick == device_tick(eng) == tick0 + d["T"], where
            tick0 += d["T"]
            ends.append(want[3])
    return np.stack(ends)


def assert_ends_are_mixed(ends):
    # envs ended, at different ticks of a decision, next to envs that ran on
    assert (ends >= 0).any() and len(set(ends[ends >= 0].tolist())) >= 2 and ((ends >= 0).any(axis=1) & (ends < 0).any(axis=1)).any()


def agent_seed(point, remi):
    return 9000 + 10 * int(point[1]) + int(remi)


@gpu
@pytest.mark.parametrize("remi", [True, False])
@pytest.mark.parametrize("path", sorted(AGENT_PATHS))
@pytest.mark.parametrize("point", ["P1", "P2"])
def test_agent_steps(point, path, remi):
    """tfx_agent_step (`if done: break`) against emulate_decision.  On the pairs k_risk's bound rate v + a rate^2 / 2 takes
    the row's own a (2 and 1.5, not 3) and these rates: a bound too small lets an env that overflows in a pair's first tick
    run the second, one too large only costs time - so the states are crowded enough that envs ARE sorted out."""
    knobs, _ = AGENT_PATHS[path]
    eng = make_engine(point, knobs, planes=2)
    orc = oracle_at(point, tables_of(eng))
    ends = run_decisions(eng, orc, agent_seed(point, remi), remi)
    assert_ends_are_mixed(ends)
    if path.startswith("pairs"):
        assert eng.pair_ticks() == 3 * (4 + 4 + 4 + 4) and eng.fused_ticks()[0] == 0
        assert eng.slow_pairs() > 0
    elif path == "res":
        assert eng.step_kernel() == "k_res" and eng.fused_ticks()[0] > 0 and eng.pair_ticks() == 0
    else:
        assert eng.pair_ticks() == 0 and eng.fused_ticks()[0] == 0


@pytest.mark.parametrize("remi", [True, False])
@pytest.mark.parametrize("point", ["P1", "P2"])
def test_decision_inputs_end_envs_one_after_another_on_the_oracle(point, remi):
    """CPU: what test_agent_steps asserts about its own inputs, on the oracle alone"""
    assert_ends_are_mixed(run_decisions(None, oracle_at(point, host_tables()), agent_seed(point, remi), remi))


# ---- arrivals made on the device ---------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("stream", ["poisson", "regular"])
def test_device_arrivals(stream):
    """tfx_set_poisson / tfx_set_regular at P1 on the pairs against their host mirrors (gym_traffic.devrng): spawned_x
    queues a new car behind the tail's own length and gap, l = 5 and s0 = 1.5 here"""
    from gym_traffic.devrng import PoissonMirror, RegularMirror
    cpt, seed = 2.2, 0xC0FFEE1234
    eng = make_engine("P1", PAIRS, planes=2)
    orc = oracle_at("P1", tables_of(eng))
    eng.set_poisson(cpt, seed=seed) if stream == "poisson" else eng.set_regular(cpt, seed=seed)
    mirror = (PoissonMirror if stream == "poisson" else RegularMirror)(cpt, seed, eng.n_entry, range(E))
    rng = np.random.RandomState(97)
    state = ragged_state(rng, E, eng.R, eng.C, LENGTH, crowd=0.4, beyond=0.05, sorted_x=True, full="none")
    load_both(eng, orc, state, rng.randint(2, size=(E, eng.I)).astype(np.int32), rng.randint(0, 12, size=(E, eng.I)).astype(np.int32))
    eng.set_tick(0)
    orc.steps[:] = 0
    t = cars = 0
    for T in CALLS:
        acts = rng.randint(2, size=(T, E, eng.I)).astype(np.int32)
        eng.set_actions(acts, per_tick=True)
        eng.step(T)
        for j in range(T):
            cnt = mirror.next_tick()
            cars += int(cnt.sum())
            orc.step(acts[j], csr(cnt, eng.entrypoints))
        t += T
        where = "%s at tick %d" % (stream, t)
        assert_same_state(eng, orc, where)
        assert eng.tick == device_tick(eng) == t, where
    assert cars > E * t
    assert_pair_counters(eng, True, False, CALLS)


# ---- part B: the reference runs off the defaults ---------------------------------------------------------------------------
FIXTURE_PATHS = {"own": {}, "pertick": {"TFX_RESIDENT": "0"}}


def fixture_engine(g, knobs):
    from gym_traffic.core import TfxEngine
    sc, tab = g.sc, g.archetypes
    validate = sc["mode"] == "validate"
    return with_switches(knobs, lambda: TfxEngine(
        sc["m"], sc["n"], sc["L"], sc["C"], rate=sc["rate"], learn_switch=sc["learn_switch"], validate=validate,
        planes=3 if (validate or tab is not None) else 2, archetypes=None if tab is None else tab[:, 1:9],
        constants=sc.get("constants")))


def fixture_oracle(g, eng):
    sc = g.sc
    row, _ = table_of(g)
    return OracleEnv(sc["m"], sc["n"], sc["L"], sc["C"], eng.dest, eng.phases, eng.nexts, rate=sc["rate"],
                     learn_switch=sc["learn_switch"], validate=sc["mode"] == "validate", archetype=row, constants=sc.get("constants"))


def bind_tick(eng, g, t):
    from test_gpu_archetypes import spawn_rows
    from test_gpu_parity import counts
    roads = g.spawns(t)
    eng.set_spawns(counts=counts(eng, [roads]), rows=spawn_rows(eng, roads, g.spawn_archs(t)) if eng.het else None)
    eng.set_actions(g["actions"][t][None, :])


def device_ints_differ(eng, g, k):
    return ints_differ(eng.leading[0].cpu().numpy(), eng.lastcar[0].cpu().numpy(), eng.obs[0].cpu().numpy(),
                       eng.rewards[0].cpu().numpy(), int(eng.done[0]), eng.waiting[0].cpu().numpy(),
                       eng.passed_dst[0].cpu().numpy(), g, k)


@gpu
@pytest.mark.parametrize("path", sorted(FIXTURE_PATHS))
@pytest.mark.parametrize("name", param_names())
def test_fixture_free_running(name, path):
    """A captured run replayed through tfx_step: bit-equal to the oracle for the whole run, integer-equal to the reference
    for the first 120 ticks (tests/test_gpu_parity.py:test_free_running_vs_oracle_and_golden)"""
    g = fixture(name)
    sc = g.sc
    _, tab = table_of(g)
    eng = fixture_engine(g, FIXTURE_PATHS[path])
    orc = fixture_oracle(g, eng)
    assert eng.het == (tab is not None) and eng.constants == constants_of(g)
    assert np.array_equal(eng.nexts, g["nexts"]) and np.array_equal(eng.dest, g["dest"])
    assert np.array_equal(eng.phases, g["phases"]) and np.array_equal(eng.entrypoints, g["entrypoints"])
    eng.reset(g["init_phase"])
    orc.reset(g["init_phase"])
    ri = 0
    for t in range(sc["T"]):
        bind_tick(eng, g, t)
        eng.step(1)
        _, _, odone = orc.step(g["actions"][t], [g.spawns(t)], spawn_arch=None if tab is None else [g.spawn_archs(t)], archetypes=tab)
        k = t + 1
        assert np.array_equal(eng.done.cpu().numpy(), odone), (name, k)
        if k % 7 == 0 or k < 20 or k == sc["T"]:
            assert_same_state(eng, orc, "%s tick %d" % (name, k))
            assert_rows_and_trips(eng, orc, tab, "%s tick %d" % (name, k))
        if k <= 120:
            assert device_ints_differ(eng, g, k) == [], (name, k)
        if sc_remi(g, k):
            cor, rr = eng.cars_on_roads()[0].cpu().numpy(), eng.remi_reward()[0].cpu().numpy()
            assert np.array_equal(cor, orc.cars_on_roads()[0]) and np.array_equal(rr, orc.remi_reward()[0])
            if k <= 120:
                assert np.array_equal(cor, g["cars_on_roads"][ri]) and np.array_equal(rr, g["remi_rewards"][ri])
            ri += 1
    if sc["mode"] == "validate":
        assert int(eng.n_trips[0]) == int(orc.n_trips[0]) > 10
    print("%s on %s: %s" % (name, path, eng.step_kernel()))


@gpu
@pytest.mark.parametrize("path", sorted(FIXTURE_PATHS))
@pytest.mark.parametrize("name", param_names())
def test_fixture_teacher_forced(name, path):
    """Reference state at t -> one tfx_step -> reference state at t + 1, from every tick: integers, spawn ticks and rows
    exact, floats within the bounds of tests/test_oracle_params.py, and its two bit-equal shares"""
    import torch
    g = fixture(name)
    sc = g.sc
    _, tab = table_of(g)
    eng = fixture_engine(g, FIXTURE_PATHS[path])
    tally = Tally(name, sc["rate"])
    for t in range(sc["T"]):
        eng.load_state(g["state_x"][t][None], g["state_v"][t][None], g["leading"][t][None], g["lastcar"][t][None],
                       w=g["state_w"][t][None], arch=g["state_a"][t][None] if tab is not None else None)
        for name_, t_ in (("obs", eng.obs), ("rewards", eng.rewards), ("waiting", eng.waiting), ("passed_dst", eng.passed_dst)):
            t_.copy_(torch.as_tensor(g[name_][t][None]))
        if sc_remi(g, t) and t > 0:
            eng.remi_reward()
        eng.set_tick(t)
        bind_tick(eng, g, t)
        eng.step(1)
        k = t + 1
        assert device_ints_differ(eng, g, k) == [], (name, k)
        ld, lc = eng.leading[0].cpu().numpy(), eng.lastcar[0].cpu().numpy()
        live = live_mask(ld, lc, sc["C"])
        if not live.any():
            continue
        x, v, w = [a[0] for a in eng.planes_numpy()]
        arch = None
        if eng.w is not None:
            assert np.array_equal(w[live], g["state_w"][k][live]), (name, k)
        if tab is not None:
            arch = eng.arch[0].cpu().numpy()
            assert np.array_equal(arch[live], g["state_a"][k][live]), (name, k)
        check_floats(g, k, live, x, v, live_mask(g["leading"][t], g["lastcar"][t], sc["C"]), g["state_v"][t], arch, tally)
    print(tally.row())
    tally.assert_shares()


@gpu
@pytest.mark.parametrize("name", ["one_row", "three_rows_rate07"])
def test_fixture_through_the_gym_surface(name):
    """tests/test_gpu_archetypes.py:test_gym_surface_with_a_user_archetype_table on the one-row run (the single-archetype
    kernels at a user's row) and on three rows at rate 0.7: `traffic_env.archetypes` replaced, env.step for 120 ticks of
    the reference's integers, env.state shows the rows, env.repeat equals ten steps"""
    import gym_traffic  # noqa: F401
    import gym
    from gym_traffic.envs import traffic_env as te
    from gym_traffic.envs.roadgraph import GridRoad
    from gym_traffic.flags import update_flags
    g = fixture(name)
    sc, tab = g.sc, g.archetypes
    keep = te.archetypes
    try:
        te.archetypes = tab.copy()
        update_flags(poisson=bool(sc["poisson"]), rate=float(sc["rate"]), local_cars_per_sec=float(sc["lcps"]),
                     entry=sc["entry"], learn_switch=bool(sc["learn_switch"]), mode=sc["mode"])

        def make():
            env = gym.make('traffic-v0')
            env.set_graph(GridRoad(sc["m"], sc["n"], sc["L"]), capacity=sc["C"])
            env.seed_generator(sc["seed"])
            env.reset_entrypoints()
            np.random.seed(sc["seed"])
            env.reset()
            return env
        env = make()
        assert env.engine.het == (len(tab) > 1) and np.array_equal(env.current_phase, g["init_phase"])
        if len(tab) == 1:
            assert [env.engine.car[k] for k in ("car_v", "car_l", "car_a", "car_v0", "car_s0")] == [9.0, 5.0, 2.0, 12.0, 1.5]
        for t in range(120):
            obs, rew, done, _ = env.step(g["actions"][t])
            k = t + 1
            assert np.array_equal(obs, g["obs"][k]) and np.array_equal(rew, g["rewards"][k]), (name, k)
            assert bool(done) == bool(g["done"][k]), (name, k)
            assert np.array_equal(np.asarray(env.leading), g["leading"][k]), (name, k)
            assert np.array_equal(np.asarray(env.lastcar), g["lastcar"][k]), (name, k)
        assert env.generated_cars == int(g["spawn_off"][120])
        st = env.state.numpy()
        live = live_mask(g["leading"][120], g["lastcar"][120], sc["C"])
        rows = g["state_a"][120]
        for col in (te.li, te.ai, te.deltai, te.v0i, te.bi, te.ti, te.s0i):
            assert np.array_equal(st[:, col, :][live], tab[rows[live], col]), col
        assert np.array_equal(st[:, te.wi, :][live], g["state_w"][120][live])
        a, b = make(), make()
        r = sc["m"] * sc["n"] * 4
        for dec in range(6):
            act = g["actions"][10 * dec]
            tot, rsum, done_a = a.repeat(act, 10)
            want = np.zeros_like(tot)
            for _ in range(10):
                obs, rew, done_b, _ = b.step(act)
                want[:r] += obs[:r]
                want[r:2 * r] = obs[r:2 * r]
                want[2 * r:] = obs[-(len(obs) - 2 * r) // 2:] / 100 * (2 * obs[2 * r:2 * r + (len(obs) - 2 * r) // 2] - 1)
                if done_b:
                    break
            assert np.array_equal(tot, want) and bool(done_a) == bool(done_b), dec
            assert np.array_equal(np.asarray(a.leading), np.asarray(b.leading)), dec
            lv = live_mask(np.asarray(a.leading), np.asarray(a.lastcar), sc["C"])
            assert np.array_equal(a.state.numpy().transpose(0, 2, 1)[lv], b.state.numpy().transpose(0, 2, 1)[lv]), dec
    finally:
        te.archetypes = keep
        update_flags(poisson=True, rate=0.5, local_cars_per_sec=0.12, entry='all', learn_switch=False, mode='train')


# ---- observers, and what the Python layer reports ----------------------------------------------------------------------------
def driven_p2(knobs=PAIRS):
    """the P2 handle (cars 8 m long) and its oracle after a driven run: 40 ticks from reset, arrivals on every entry road"""
    eng = make_engine("P2", knobs, planes=2)
    orc = oracle_at("P2", tables_of(eng))
    rng = np.random.RandomState(321)
    ph = rng.randint(2, size=(E, eng.I)).astype(np.int32)
    eng.reset(ph)
    orc.reset(ph)
    for T in (7, 8, 8, 8, 9):
        acts = np.repeat(rng.randint(2, size=(1, E, eng.I)), T, axis=0).astype(np.int32)
        cnt = (rng.rand(T, E, eng.n_entry) < 0.3).astype(np.int32)
        eng.set_actions(acts, per_tick=True)
        eng.set_spawns(counts=cnt, per_tick=True)
        eng.step(T)
        for j in range(T):
            orc.step(acts[j], csr(cnt[j], eng.entrypoints))
    assert_same_state(eng, orc, "driven run")
    return eng, orc


@gpu
def test_frames_draw_the_rows_own_car_length():
    """tfx_frames (px 13) on the P2 handle against devrng.frames applied to the ORACLE's state with car_l = 8 spelled out:
    k_frames reads d.car_l; the picture with the default 4 m cars is another one"""
    from gym_traffic.devrng import frames
    eng, orc = driven_p2()
    got = eng.frames(None, px=13).cpu().numpy()

    def picture(car_l):
        return frames(orc.x, orc.leading, orc.lastcar, orc.current_phase, orc.elapsed, M, N, 13, LENGTH, yellow_ticks=6, car_l=car_l)
    assert float(eng.cfg.car_l) == 8.0 and eng.car["car_l"] == 8.0
    assert got.shape == (E,) + eng.frame_size(13) + (4,) == (E, 53, 53, 4)
    assert np.array_equal(got, picture(8.0))
    assert not np.array_equal(got, picture(4.0))


@gpu
def test_road_measures():
    """tfx_road_measures on the P2 handle against devrng.road_measures applied to the oracle's state"""
    from gym_traffic.devrng import road_measures
    eng, orc = driven_p2()
    import torch
    for halt, x_from in ((0.1, None), (0.35, 60.0)):
        got = eng.road_measures(halt, x_from)
        torch.cuda.synchronize()
        want = road_measures(orc.x, orc.v, orc.leading, orc.lastcar, eng.C, halt, x_from)
        for name, g_, w_ in zip(("n_cars", "n_halted", "queue"), got, want):
            assert np.array_equal(g_.cpu().numpy(), w_), (name, halt, x_from)
        assert same_bits(got[3].cpu().numpy(), want[3]), (halt, x_from)
    assert int(got[0].sum()) > 50 and int(got[1].sum()) > 0


@gpu
def test_the_python_layer_reports_the_row_and_the_constants_in_use():
    """A one-row table IS the engine's archetype (csrc/tfx_hip.hip:tfx_create): TfxEngine and TrafficVecEnv report that
    row and the constants they were given, not ARCHETYPE and CONSTANTS"""
    from gym_traffic.core import ARCHETYPE, CONSTANTS
    from gym_traffic.envs.vec_env import TrafficVecEnv
    eng = make_engine("P1", {}, planes=2)
    names = ("car_v", "car_l", "car_a", "car_delta", "car_v0", "car_b", "car_T", "car_s0")
    assert not eng.het and [eng.car[k] for k in names] == ROW_P1 and [float(getattr(eng.cfg, k)) for k in names] == ROW_P1
    assert np.array_equal(eng.archetypes, np.asarray([ROW_P1], np.float32)) and eng.constants == CONSTANTS
    dflt = make_engine(dict(rate=0.5, row=None, constants=None), {}, planes=2)
    assert dflt.car == ARCHETYPE and dflt.archetypes is None
    p3 = POINTS["P3"]["constants"]
    eng3 = make_engine("P3", {}, planes=2)
    assert eng3.constants == p3 and int(eng3.cfg.yellow_ticks) == 4 and float(eng3.cfg.detect_dist) == 17.5
    with pytest.raises(ValueError):
        make_engine(dict(rate=0.5, row=None, constants=dict(yellow=4)), {}, planes=2)
    vec = TrafficVecEnv(2, 2, 2, 100.0, capacity=10, rate=0.7, spawn='device', archetypes=[ROW_P2], constants=dict(thresh=0.35))
    assert not vec.engine.het and vec.engine.car["car_l"] == 8.0 and vec.engine.car["car_v0"] == 10.0
    assert vec.constants == dict(CONSTANTS, thresh=0.35) and abs(float(vec.engine.cfg.thresh) - 0.35) < 1e-7
    vec.reset(np.zeros((2, vec.engine.I), np.int32))
    assert vec.snapshot().engine.constants == vec.constants
