"""Every step path against the REFERENCE on loaded ring states (tests/golden/states/, tests/test_oracle_states.py states
what the fixtures hold and the bars).  The other GPU tests on pathological ring states compare the device with the
oracle only; here a fixture's N states form one batch of N envs (the rows fixture: eight envs at tick 60 and one at a
clock of three million, a handle has one clock) that is loaded as load_both and run_pairs_case load theirs, and the
oracle runs beside the device through the same calls.

  * one tick, from every recorded tick (step(1)): integers, spawn ticks, rows and trip times equal the reference's, x
    and v stay within the bounds of tests/test_oracle_states.py (the same pinned cars beyond conftest's), everything is
    bit-equal to the oracle - on k_res with 1, 2, 4 and mixed lanes per road and three envs per workgroup (where the
    handle takes k_res: not in validate mode, not with mixed rows), tick by tick, k_move_t forced, both ring-layout paths;
  * calls of [6], [3, 3] and [2, 1, 3] ticks from tick 0 with per-tick action, count and row buffers: after every call
    the integers equal the reference's at that tick, `done` the OR over the call's ticks, spawn ticks, rows and the trip
    log are equal, the floats are bit-equal to the oracle's - on k_res, the two-tick passes with k_tail / separate
    launches / two streams / segments (2; 4 and 8 on the two longest rings) / without the graph, and the ring layout;
    the counters say that the path meant is the path taken.
"""
import numpy as np
import pytest

from oracle.oracle import live_mask
from test_gpu_parity import assert_same_state, counts
from test_gpu_params import with_switches
from test_gpu_stride_rounds import assert_pair_counters, assert_rows_and_trips
from test_oracle_params import Tally
from test_oracle_states import BEYOND_BOUND, SCENARIOS, check_floats, fixture, load, make_env, print_tally, step

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROWS_PER_ROAD = 4       # a tick brings at most 3 cars
PAIRS = {"TFX_RESIDENT": "0", "TFX_PAIRS": "2", "TFX_TAIL": "2", "TFX_SPLIT": "0", "TFX_TT_SEG": "0"}
PERTICK = {"TFX_RESIDENT": "0", "TFX_PAIRS": "0"}


def res(lpr):
    return {"TFX_RESIDENT": "1", "TFX_RES_EPB": "3", "TFX_RES_LPR": str(lpr)}


# name -> (switches, layout, kind); kind: what the counters must say afterwards
PATHS = {
    "res_lpr1": (res(1), "transposed", "res"), "res_lpr2": (res(2), "transposed", "res"),
    "res_lpr4": (res(4), "transposed", "res"), "res_lpr3": (res(3), "transposed", "res"),
    "resident": ({"TFX_RESIDENT": "1"}, "transposed", "res"),
    "pertick": (PERTICK, "transposed", "pertick"),
    "move_t": (dict(PERTICK, TFX_MOVE_VARIANT="91"), "transposed", "move_t"),
    "ring": ({"TFX_RESIDENT": "0"}, "ring", "pertick"),
    "ring_resident": ({"TFX_RESIDENT": "1"}, "ring", "res"),
    "pairs_tail": (PAIRS, "transposed", "pairs"),
    "pairs_launches": (dict(PAIRS, TFX_TAIL="0"), "transposed", "pairs"),
    "pairs_split": (dict(PAIRS, TFX_SPLIT="2"), "transposed", "pairs"),
    "pairs_seg": (dict(PAIRS, TFX_TT_SEG="2", TFX_TT_SEGS="2"), "transposed", "pairs"),
    "pairs_seg4": (dict(PAIRS, TFX_TT_SEG="2", TFX_TT_SEGS="4"), "transposed", "pairs"),
    "pairs_seg8": (dict(PAIRS, TFX_TT_SEG="2", TFX_TT_SEGS="8"), "transposed", "pairs"),
    "pairs_nograph": (dict(PAIRS, TFX_GRAPH="0"), "transposed", "pairs"),
}
HET_PATHS = ["pertick", "pairs_tail", "pairs_launches", "pairs_split"]      # tests/test_gpu_clone.py:HET_PATHS
ROWS = "st_3x2_c20_rows_validate"
PLAIN = [n for n in SCENARIOS if n != ROWS]
K_RES = [n for n in PLAIN if "validate" not in n]          # k_res does not serve validate mode (res_usable)
LONG = ["st_2x2_c130", "st_1x1_c258"]

ONE_TICK = ([(n, p) for p in ("res_lpr1", "res_lpr2", "res_lpr4", "res_lpr3", "ring_resident") for n in K_RES] +
            [(n, p) for p in ("pertick", "move_t", "ring") for n in PLAIN] + [(ROWS, "pertick")])
MULTI = ([(n, p) for p in ("resident",) for n in K_RES] +
         [(n, p) for p in ("pairs_tail", "pairs_launches", "pairs_split", "pairs_seg", "pairs_nograph", "ring") for n in PLAIN] +
         [(n, p) for p in ("pairs_seg4", "pairs_seg8") for n in LONG] + [(ROWS, p) for p in HET_PATHS])
CALLS = [[6], [3, 3], [2, 1, 3]]


def groups(g):
    """the states of a fixture that share a clock: [(tick, [state, ...]), ...]"""
    ticks = g["ticks"].tolist()
    return [(t, [i for i, u in enumerate(ticks) if u == t]) for t in sorted(set(ticks))]


def make_engine(g, path, n_envs):
    from gym_traffic.core import TfxEngine
    knobs, layout, _ = PATHS[path]
    sc, tab = g.sc, g.archetypes
    planes = 3 if (g.validate or tab is not None or layout == "ring") else 2
    eng = with_switches(knobs, lambda: TfxEngine(
        sc["m"], sc["n"], sc["L"], sc["C"], n_envs=n_envs, rate=sc["rate"], learn_switch=sc["learn_switch"], validate=g.validate,
        planes=planes, layout=layout, archetypes=None if tab is None else tab[:, 1:9], constants=sc.get("constants")))
    assert eng.het == (tab is not None)
    for name in ("dest", "phases", "nexts", "entrypoints"):
        assert np.array_equal(getattr(eng, name), g[name]), name
    eng.reset(np.zeros((n_envs, eng.I), np.int32))
    return eng


def load_device(eng, g, states, t):
    """the handle's envs <- the given states as the reference held them after t ticks"""
    pick = lambda key: g[key][states, t]
    eng.load_state(pick("state_x"), pick("state_v"), pick("leading"), pick("lastcar"), w=pick("state_w"),
                   arch=pick("state_a").astype(np.uint8) if eng.het else None)
    for name in ("obs", "rewards", "waiting", "passed_dst"):
        getattr(eng, name).copy_(torch.as_tensor(np.ascontiguousarray(pick(name))))
    eng.set_tick(int(g["ticks"][states[0]]) + t)
    if g.validate:
        eng.n_trips.zero_()


def tick_inputs(eng, g, states, t):
    """-> (actions [E, I], counts [E, n_entry], rows uint8 [E, n_entry, ROWS_PER_ROAD]) of tick t"""
    act = np.stack([g["actions"][i, t] for i in states]).astype(np.int32)
    cnt = counts(eng, [g.roads(i, t) for i in states])
    rows = np.zeros((len(states), eng.n_entry, ROWS_PER_ROAD), np.uint8)
    for k, i in enumerate(states):
        seen = {}
        for rd, a in zip(g.roads(i, t), g.rows(i, t)):
            j = eng.entry_index[int(rd)]
            rows[k, j, seen.get(j, 0)] = a
            seen[j] = seen.get(j, 0) + 1
    return act, cnt, rows


def snapshot(eng):
    s = {n: getattr(eng, n).cpu().numpy() for n in ("leading", "lastcar", "obs", "rewards", "waiting", "passed_dst", "done")}
    s["x"], s["v"], s["w"] = eng.planes_numpy()
    s["arch"] = eng.arch.cpu().numpy() if eng.het else None
    if eng.n_trips is not None:
        s["n_trips"], s["trip_times"] = eng.n_trips.cpu().numpy(), eng.trip_times.cpu().numpy()
    return s


def assert_reference(eng, s, g, states, k0, k1, where, trips_from=0, tally=None):
    """The device after the ticks k0 + 1 .. k1 of the given states against the fixture: integers, spawn ticks, rows and
    trip times exact (`done`: the OR over those ticks; the trip log: what the reference logged after tick `trips_from`,
    where load_device emptied it); tally: x and v against the reference's within the bounds of
    tests/test_oracle_states.py (one tick)."""
    C = g.sc["C"]
    for k, i in enumerate(states):
        at = (where, "state %d" % i, "tick %d" % k1)
        for name in ("leading", "lastcar", "obs", "rewards", "waiting", "passed_dst"):
            assert np.array_equal(s[name][k], g[name][i, k1]), (name,) + at
        assert bool(s["done"][k]) == bool(g["done"][i, k0 + 1:k1 + 1].any()), ("done",) + at
        live = live_mask(s["leading"][k], s["lastcar"][k], C)
        if eng.P == 3:
            assert np.array_equal(s["w"][k][live], g["state_w"][i, k1][live]), ("w",) + at
        if eng.het:
            assert np.array_equal(s["arch"][k][live], g["state_a"][i, k1][live]), ("rows",) + at
        if g.validate:
            n = int(s["n_trips"][k])
            assert np.array_equal(s["trip_times"][k, :n].astype(np.float64), g.trips(i, trips_from, k1)), ("trips",) + at
        if tally is not None and live.any():
            check_floats(g, i, k1, live, s["x"][k], s["v"][k], None if s["arch"] is None else s["arch"][k], tally)


def assert_path(eng, kind, path, calls):
    """the counters after `calls` (ticks per call) on a fresh handle: the path meant is the path taken"""
    ticks = sum(calls)
    if kind == "res":
        assert eng.fused_ticks() == (ticks, True) and eng.pair_ticks() == 0 and eng.step_kernel() == "k_res", path
        return
    assert eng.fused_ticks()[0] == 0, path
    if kind == "pairs":
        knobs = PATHS[path][0]
        assert_pair_counters(eng, knobs["TFX_TAIL"] == "2", knobs["TFX_SPLIT"] == "2" and eng.E >= 2, calls)
    else:
        assert eng.pair_ticks() == 0 and eng.split_ticks() == 0, path
        if kind == "move_t":
            assert eng.step_kernel() == "k_move_t", path


@pytest.mark.parametrize("name,path", ONE_TICK, ids=["%s-%s" % c for c in ONE_TICK])
def test_one_tick_from_every_recorded_tick(name, path):
    g = fixture(name)
    tab = g.archetypes
    tally = Tally(name, g.sc["rate"])
    for tick0, states in groups(g):
        eng = make_engine(g, path, len(states))
        orc = make_env(g, len(states))
        for t in range(g.K):
            where = "%s on %s, from tick %d" % (name, path, t)
            load_device(eng, g, states, t)
            for k, i in enumerate(states):
                load(orc, k, g, i, t)
            act, cnt, rows = tick_inputs(eng, g, states, t)
            eng.set_actions(act)
            eng.set_spawns(counts=cnt, rows=rows if eng.het else None)
            eng.step(1)
            _, _, odone = step(orc, g, states, t)
            s = snapshot(eng)
            assert np.array_equal(s["done"], odone), where
            assert_same_state(eng, orc, where)
            assert_rows_and_trips(eng, orc, tab, where)
            assert_reference(eng, s, g, states, t, t + 1, where, trips_from=t, tally=tally)
        assert_path(eng, PATHS[path][2], path, [1] * g.K)
    print_tally(tally)
    assert tally.cars > 1000 and len(tally.beyond) <= BEYOND_BOUND.get(name, 0), (tally.row(), tally.beyond)


@pytest.mark.parametrize("calls", CALLS, ids=["-".join(str(T) for T in c) for c in CALLS])
@pytest.mark.parametrize("name,path", MULTI, ids=["%s-%s" % c for c in MULTI])
def test_calls_from_tick_0(name, path, calls):
    g = fixture(name)
    tab = g.archetypes
    assert sum(calls) == g.K
    for tick0, states in groups(g):
        eng = make_engine(g, path, len(states))
        orc = make_env(g, len(states))
        load_device(eng, g, states, 0)
        for k, i in enumerate(states):
            load(orc, k, g, i, 0)
        k0 = 0
        for T in calls:
            where = "%s on %s, calls %s, ticks %d..%d" % (name, path, calls, k0 + 1, k0 + T)
            per_tick = [tick_inputs(eng, g, states, k0 + j) for j in range(T)]
            eng.set_actions(np.stack([p[0] for p in per_tick]), per_tick=True)
            eng.set_spawns(counts=np.stack([p[1] for p in per_tick]), per_tick=True,
                           rows=np.stack([p[2] for p in per_tick]) if eng.het else None)
            eng.step(T)
            done = np.zeros(len(states), bool)
            for j in range(T):
                done |= step(orc, g, states, k0 + j)[2].astype(bool)
            s = snapshot(eng)
            assert np.array_equal(s["done"].astype(bool), done), where
            assert_same_state(eng, orc, where)
            assert_rows_and_trips(eng, orc, tab, where)
            assert_reference(eng, s, g, states, k0, k0 + T, where)
            if PATHS[path][2] == "pairs" and T % 2 == 0:
                assert eng.step_kernel() == ("k_move_tts" if "seg" in path else "k_move_tt"), where
            k0 += T
        assert eng.tick == tick0 + g.K
        assert_path(eng, PATHS[path][2], path, calls)
