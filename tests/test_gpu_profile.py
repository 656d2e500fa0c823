"""What tfx_profile records (csrc/tfx_sequence.hpp `TickTimer`): one entry of three events per timed pair, single tick
or k_res launch of a plain tfx_step call, weighted by the ticks it covers; the budget counts ENTRIES; a read empties the
record; agent steps record nothing; a timed call never splits; and timing changes no bit of the state.

Shapes: those of test_gpu_launch_plan.py - a 2x2 grid of 60 m roads, four envs, rings of 10 slots, the on-device
periodic spawns and cycle actions.  Every case builds one small handle and runs at most 13 ticks; the oracle runs those
13 ticks once, for all cases, and stays clear of ring overflows (asserted)."""
import math

import numpy as np
import pytest

from test_gpu_fused import engine_with
from test_gpu_launch_plan import CYCLE_PERIOD, E, LENGTH, SPAWN_PERIOD, Snapshot
from test_gpu_parity import assert_same_state, oracle_like, same_bits
from oracle.oracle import live_mask

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from gym_traffic import workload as wl  # noqa: E402

T_MAX = 13
PAIRS_TAIL = {"TFX_RESIDENT": "0", "TFX_PAIRS": "2", "TFX_TAIL": "2", "TFX_SPLIT": "2"}
PAIRS_NO_TAIL = dict(PAIRS_TAIL, TFX_TAIL="0")
TICK_BY_TICK = {"TFX_RESIDENT": "0", "TFX_PAIRS": "0"}
RESIDENT = {"TFX_RESIDENT": "1"}

_AFTER = {}


def after(eng, t):
    """The oracle after t plain ticks from the reset (t <= T_MAX): computed once, shared, left unchanged."""
    if not _AFTER:
        orc = oracle_like(eng)
        orc.reset(np.zeros((E, eng.I), np.int32))
        ids = np.arange(E)
        _AFTER[0] = Snapshot(orc, None, None)
        for k in range(T_MAX):
            roads = wl.spawn_roads_for_tick(eng.entrypoints, k, period=SPAWN_PERIOD)
            done = orc.step(wl.cycle_actions(ids, eng.I, k, period=CYCLE_PERIOD), [roads] * E)[2]
            assert not done.any(), "the scenario must stay clear of ring overflows (tick %d)" % k
            _AFTER[k + 1] = Snapshot(orc, None, None)
    return _AFTER[t]


def engine(knobs, layout="transposed"):
    eng = engine_with(knobs, E, layout=layout, m=2, n=2, length=LENGTH, capacity=10, rate=0.5)
    eng.reset(np.zeros((E, eng.I), np.int32))
    eng.set_spawns(period=SPAWN_PERIOD)
    eng.set_actions(cycle_period=CYCLE_PERIOD)
    eng.reset_counters()
    return eng


def read(eng, ticks):
    """profile_read(): `ticks` ticks recorded; the two durations are finite and not negative, and - where anything was
    recorded - not both zero."""
    got = eng.profile_read()
    assert got["ticks"] == ticks, got
    for name in ("move_ms", "advance_ms"):
        assert math.isfinite(got[name]) and got[name] >= 0.0, got
    if ticks:
        assert got["move_ms"] + got["advance_ms"] > 0.0, got
    else:
        assert got["move_ms"] == 0.0 and got["advance_ms"] == 0.0, got
    return got


def same_as_oracle(eng, t):
    assert_same_state(eng, after(eng, t), "after %d ticks" % t)
    assert eng.tick == t and eng.vehicle_updates() == after(eng, t).updates and not eng.done.any()


def test_pairs_with_k_tail_two_pair_entries_and_a_single():
    eng = engine(PAIRS_TAIL)
    split0 = eng.split_ticks()
    eng.profile(8)
    eng.step(5)
    read(eng, 5)                                  # two entries of weight 2, one of weight 1
    assert eng.split_ticks() == split0            # (a timed call never splits)
    assert (eng.pair_ticks(), eng.tail_ticks()) == (4, 4)
    assert eng.step_kernel() == "k_move_ts"
    same_as_oracle(eng, 5)


def test_the_budget_counts_entries_and_a_read_empties_the_record():
    eng = engine(PAIRS_TAIL)
    eng.profile(2)
    eng.step(5)
    read(eng, 4)                                  # two pairs used the two entries: the single tick is not timed
    read(eng, 0)
    eng.step(2)
    read(eng, 2)                                  # the record was emptied: it takes entries again
    assert (eng.pair_ticks(), eng.tail_ticks(), eng.split_ticks()) == (6, 6, 0)
    same_as_oracle(eng, 7)


def test_pairs_without_k_tail():
    eng = engine(PAIRS_NO_TAIL)
    eng.profile(8)
    eng.step(4)
    read(eng, 4)
    assert (eng.pair_ticks(), eng.tail_ticks(), eng.split_ticks()) == (4, 0, 0)
    same_as_oracle(eng, 4)


@pytest.mark.parametrize("layout", ["transposed", "ring"])
def test_tick_by_tick(layout):
    eng = engine(TICK_BY_TICK, layout)
    eng.profile(8)
    eng.step(5)
    read(eng, 5)
    assert (eng.pair_ticks(), eng.tail_ticks(), eng.split_ticks()) == (0, 0, 0)
    same_as_oracle(eng, 5)


def test_resident_one_entry_per_call():
    eng = engine(RESIDENT)
    assert eng.fused_ticks() == (0, True)
    eng.profile(8)
    eng.step(5)
    read(eng, 5)
    assert eng.fused_ticks()[0] == 5 and eng.step_kernel() == "k_res"
    same_as_oracle(eng, 5)
    eng.profile(1)                                # one entry: the first call takes it, whatever its length
    eng.step(3)
    eng.step(3)
    read(eng, 3)
    assert eng.fused_ticks()[0] == 11
    same_as_oracle(eng, 11)


@pytest.mark.parametrize("knobs", [PAIRS_TAIL, RESIDENT], ids=["pairs", "resident"])
def test_agent_steps_record_nothing(knobs):
    eng = engine(knobs)
    eng.profile(8)
    eng.agent_step(4, remi=True)
    read(eng, 0)
    # (the engine's obs and rewards hold the decision's accumulations, Remi cleared `waiting`: the cars are compared)
    now = after(eng, 4)
    ld, lc = eng.leading.cpu().numpy(), eng.lastcar.cpu().numpy()
    assert np.array_equal(ld, now.leading) and np.array_equal(lc, now.lastcar)
    x, v, _ = eng.planes_numpy()
    for k in range(E):
        live = live_mask(ld[k], lc[k], eng.C)
        assert same_bits(x[k][live], now.x[k][live]) and same_bits(v[k][live], now.v[k][live]), k
    assert eng.tick == 4 and eng.vehicle_updates() == now.updates
    eng.step(2)                                   # plain calls are still recorded
    read(eng, 2)


def test_profile_0_turns_it_off_and_calls_split_again():
    eng = engine(PAIRS_TAIL)
    eng.profile(8)
    eng.step(4)
    assert eng.split_ticks() == 0
    read(eng, 4)
    eng.profile(0)
    eng.step(4)
    read(eng, 0)
    assert eng.split_ticks() == 4
    assert (eng.pair_ticks(), eng.tail_ticks()) == (8, 8)
    same_as_oracle(eng, 8)
