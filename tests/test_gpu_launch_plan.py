"""The launch plan of a handle (csrc/tfx_launch.hpp): every grid is sized at the entry of the first API call that can
launch with it, whichever entry point that is and whether the call then captures a graph, forks onto a second stream or
runs eagerly.  Property: for every first call and every order of the calls after it, each call finds its grids sized
and gives the oracle's bits - state, the agent step's outputs and the handle's counters - and tfx_step_kernel names a
mover that call can launch.

Shapes: a 2x2 grid of 60 m roads, four envs (a forced split has two per half), rings of 10 and of 130 slots (the
long-ring picks), the on-device cycle and periodic rules (no host input between calls), TFX_RESIDENT=0 (the per-tick
kernels).  At this size step(5) and step(6) replay a captured graph unless the call splits, and agent steps capture
unless they split.  No case provokes a failure; the run stays clear of ring overflows (checked on the oracle), so an
agent step's `if done: break` never cuts a decision short."""
import numpy as np
import pytest

from test_gpu_fused import engine_with
from test_gpu_parity import assert_same_state, oracle_like, same_bits
from oracle.oracle import live_mask

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from gym_traffic import workload as wl  # noqa: E402

E, LENGTH, SPAWN_PERIOD, CYCLE_PERIOD = 4, 60.0, 3, 5

ENVS = {
    "pairs_tail": {"TFX_PAIRS": "2", "TFX_TAIL": "2"},
    "pairs_tail_split": {"TFX_PAIRS": "2", "TFX_TAIL": "2", "TFX_SPLIT": "2"},
    "pairs_seg_launches": {"TFX_PAIRS": "2", "TFX_TAIL": "0", "TFX_TT_SEG": "2"},
    "tick_by_tick": {"TFX_PAIRS": "0"},
}

# (kind, ticks): a tfx_step call, a tfx_agent_step call (remi), tfx_move_cars + tfx_advance_finished_cars
CALLS = [("step", 5), ("agent", 5, True), ("step", 1), ("halves", 1), ("agent", 4, True), ("step", 6)]
T_ALL = sum(c[1] for c in CALLS)


def ordering(first):
    return CALLS[first:] + CALLS[:first]


class Snapshot(object):
    """The oracle after a call, with the attributes assert_same_state reads, and what an agent step returns."""

    def __init__(self, orc, aobs, areward):
        for name in ("leading", "lastcar", "obs", "rewards", "waiting", "passed_dst", "x", "v", "w"):
            setattr(self, name, getattr(orc, name).copy())
        self.aobs, self.areward = aobs, areward
        self.updates = orc.vehicle_updates


_REFERENCE = {}


def reference(eng, first):
    """The oracle after every call of ordering(first): computed once per ring size and ordering, shared by the cases
    that run it and left unchanged.  (The ticks are the same in every ordering, but Remi clears `waiting` and
    `passed_dst` where a decision ends.)  Agent steps: Repeater (+ Remi) of the reference, traffic_test.py:27-64."""
    key = (eng.C, first)
    if key not in _REFERENCE:
        orc = oracle_like(eng)
        orc.reset(np.zeros((E, eng.I), np.int32))
        r, I, ids, t, after = eng.r, eng.I, np.arange(E), 0, []
        for call in ordering(first):
            aobs = np.zeros((E, 2 * r + I), np.float32)
            areward = 0
            for t in range(t, t + call[1]):
                roads = wl.spawn_roads_for_tick(eng.entrypoints, t, period=SPAWN_PERIOD)
                obs, rew, done = orc.step(wl.cycle_actions(ids, I, t, period=CYCLE_PERIOD), [roads] * E)
                assert not done.any(), "the scenario must stay clear of ring overflows (tick %d)" % t
                aobs[:, :r] += obs[:, :r]
                aobs[:, r:2 * r] = obs[:, r:2 * r]
                aobs[:, -I:] = obs[:, -I:] / 100 * (2 * obs[:, -2 * I:-I] - 1)
                areward = areward + rew
            t += 1
            if call[0] == "agent" and call[2]:
                areward = orc.remi_reward().copy()
            after.append(Snapshot(orc, aobs, areward))
        assert t == T_ALL
        end = after[-1]
        cars = sum(int(live_mask(end.leading[k], end.lastcar[k], eng.C).sum()) for k in range(E))
        assert cars > 2 * E * r, cars   # a loaded network: more than two cars per train road
        _REFERENCE[key] = after
    return _REFERENCE[key]


def movers(env, call):
    """The kernels that can have moved the cars in the last tick of `call` at this size."""
    if ENVS[env]["TFX_PAIRS"] == "0":
        return {"k_move_ts"}
    if call[1] % 2:                  # a single tick: four wavefronts per tile (single_tick_ts)
        return {"k_move_ts"}
    return {"k_move_tt", "k_move_tts"}   # the last tick is the second of a pair


@pytest.mark.parametrize("first", range(len(CALLS)))
@pytest.mark.parametrize("capacity", [10, 130])
@pytest.mark.parametrize("env", sorted(ENVS))
def test_any_first_call_sizes_the_grids_every_later_call_needs(env, capacity, first):
    knobs = dict(ENVS[env], TFX_RESIDENT="0")
    eng = engine_with(knobs, E, m=2, n=2, length=LENGTH, capacity=capacity, rate=0.5)
    after = reference(eng, first)
    eng.reset(np.zeros((E, eng.I), np.int32))
    eng.set_spawns(period=SPAWN_PERIOD)
    eng.set_actions(cycle_period=CYCLE_PERIOD)
    eng.reset_counters()
    pairs = knobs["TFX_PAIRS"] == "2"
    tail = pairs and knobs["TFX_TAIL"] == "2"
    split = tail and knobs.get("TFX_SPLIT") == "2"
    t = pair_ticks = tail_ticks = split_ticks = 0
    for call, now in zip(ordering(first), after):
        kind, n = call[0], call[1]
        where = "%s%s at tick %d" % (kind, call[1:], t)
        if kind == "step":
            eng.step(n)
        elif kind == "halves":
            eng.move_cars()
            eng.advance_finished_cars()
        else:
            out = [o.cpu().numpy() for o in eng.agent_step(n, remi=call[2])]
        t += n
        if kind == "agent":
            # (the engine's obs and rewards hold the decision's accumulations: its outputs are compared instead)
            assert same_bits(out[0], now.aobs), "aobs " + where
            assert same_bits(out[1], now.areward), "areward " + where
            assert not out[2].any(), "adone " + where
            ld, lc = eng.leading.cpu().numpy(), eng.lastcar.cpu().numpy()
            assert np.array_equal(ld, now.leading) and np.array_equal(lc, now.lastcar), where
            assert np.array_equal(eng.waiting.cpu().numpy(), now.waiting), "waiting " + where
            x, v, _ = eng.planes_numpy()
            for k in range(E):
                live = live_mask(ld[k], lc[k], eng.C)
                assert same_bits(x[k][live], now.x[k][live]) and same_bits(v[k][live], now.v[k][live]), (where, k)
        else:
            assert_same_state(eng, now, where)
            assert not eng.done.any(), where
        # the counters: ticks, the cars moved, and the ticks that took each path
        if kind != "halves" and pairs:
            pair_ticks += n - n % 2
            tail_ticks += (n - n % 2) if (tail and kind == "step") else 0     # (tfx_tail_ticks counts tfx_step's)
            split_ticks += n if (split and n >= 2) else 0
        assert eng.tick == t and eng.vehicle_updates() == now.updates, where
        assert (eng.pair_ticks(), eng.tail_ticks(), eng.split_ticks()) == (pair_ticks, tail_ticks, split_ticks), where
        assert eng.fused_ticks()[0] == 0, where
        assert eng.step_kernel() in movers(env, call), (where, eng.step_kernel())
    assert t == T_ALL


@pytest.mark.parametrize("layout", ["ring", "transposed"])
def test_single_launches_size_their_grids_on_a_handle_k_res_serves(layout):
    """tfx_move_cars and tfx_advance_finished_cars run the per-tick kernels on every handle: on one whose tfx_step calls
    k_res serves - calls that size no grid - they size their own, as a handle's first call and between k_res calls."""
    eng = engine_with({"TFX_RESIDENT": "1"}, E, layout=layout, m=2, n=2, length=LENGTH, capacity=10, rate=0.5)
    assert eng.fused_ticks() == (0, True)
    orc = oracle_like(eng)
    orc.reset(np.zeros((E, eng.I), np.int32))
    eng.reset(np.zeros((E, eng.I), np.int32))
    eng.set_spawns(period=SPAWN_PERIOD)
    eng.set_actions(cycle_period=CYCLE_PERIOD)
    eng.reset_counters()
    ids, t, fused = np.arange(E), 0, 0
    for kind, n in (("halves", 1), ("step", 5), ("halves", 1), ("step", 2)):
        where = "%s(%d) at tick %d" % (kind, n, t)
        if kind == "step":
            eng.step(n)
            fused += n
        else:
            eng.move_cars()
            eng.advance_finished_cars()
        for t in range(t, t + n):
            roads = wl.spawn_roads_for_tick(eng.entrypoints, t, period=SPAWN_PERIOD)
            orc.step(wl.cycle_actions(ids, eng.I, t, period=CYCLE_PERIOD), [roads] * E)
        t += 1
        assert_same_state(eng, orc, where)
        assert eng.tick == t and eng.vehicle_updates() == orc.vehicle_updates, where
        assert eng.fused_ticks()[0] == fused and eng.pair_ticks() == 0, where
        assert eng.step_kernel() in ({"k_res"} if kind == "step" else {"k_move", "k_move_ts"}), (where, eng.step_kernel())
