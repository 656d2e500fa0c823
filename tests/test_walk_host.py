"""The state tests/test_gpu_walk.py puts the read-only road kernels on (csrc/tfx_walk.hpp), built and checked on the CPU
oracle alone: long columns (C = 66, counts on both sides of a multiple of eight) that start a row down after a
two-tick pass, a partial second tile, empty roads - the hazards of the shared walk, all in one state."""
import numpy as np

GRID = dict(m=4, n=4, length=400.0, capacity=66, rate=0.5)     # 80 roads: a full tile and 16 lanes of a second
E_WALK = 3
DEPTHS = (7, 9, 48)            # cars per road and env at the start: below eight, above it, six rounds of eight
EMPTY = (5, 70)                # roads without a car at the start, one of each tile: (road 5 is entered from others, 70 is not)
# ticks per tfx_step call, every call under one held action: with it the lights let the heads of sixteen roads of the first
# tile and those of the exit roads go in tick 7 - the second tick of the last two-tick pass where those run
CALLS = [1, 1, 2, 4]
NOW = 500                      # the clock at the start; the prefilled cars were born in the ticks before it


def initial_state():
    """(x, v, w float32 [E, R, C], leading, lastcar int32 [E, R]): workload.prefill_one_env at DEPTHS, one per env, the
    roads EMPTY cleared, spawn ticks NOW - 3 * slot - env"""
    from gym_traffic import workload as wl
    per = [wl.prefill_one_env(GRID["m"], GRID["n"], GRID["length"], GRID["capacity"], d, 8.0) for d in DEPTHS]
    x, v, ld, lc = [np.stack([p[i] for p in per]) for i in range(4)]
    lc[:, EMPTY] = ld[:, EMPTY]
    slot = np.arange(GRID["capacity"], dtype=np.float32)
    w = np.broadcast_to(NOW - 3.0 * slot, x.shape) - np.arange(E_WALK, dtype=np.float32)[:, None, None]
    return x, v, np.ascontiguousarray(w, np.float32), ld, lc


def scenario(I, n_entry, seed=66):
    """[(held action int32 [E, I]: phase i % 2 at intersection i, arrival counts int32 [n, E, n_entry])] for CALLS - a pure
    function of its arguments"""
    rng = np.random.RandomState(seed)
    act = np.ascontiguousarray(np.broadcast_to(np.arange(I, dtype=np.int32) % 2, (E_WALK, I)))
    out = []
    for n in CALLS:
        cnt = (rng.rand(n, E_WALK, n_entry) < 0.2).astype(np.int32) * rng.randint(1, 3, size=(n, E_WALK, n_entry))
        out.append((act, cnt.astype(np.int32)))
    return out


def tiles_of(nexts, r):
    """the roads of each 64-slot tile, in the handle's slot order (build_slots, csrc/tfx_handle.hpp): the train roads
    other roads lead into in id order, the entry roads, the exit roads"""
    nexts = np.asarray(nexts)
    R = len(nexts)
    fed = np.zeros(R, bool)
    fed[nexts[nexts >= 0]] = True
    order = [e for e in range(r) if fed[e]] + [e for e in range(r) if not fed[e]] + list(range(r, R))
    return [order[s:s + 64] for s in range(0, R, 64)]


_walk = {}


def oracle_walk():
    """The scenario on the CPU oracle: dict(x, v [E, R, C], leading, lastcar, cars [E, R], popped bool [E, R]: roads whose
    head left them in the last tick - where two-tick passes run, their columns start a row down - tiles)"""
    if not _walk:
        from gym_traffic.envs.roadgraph import GridRoad
        from oracle.oracle import OracleEnv
        from test_measures_host import roads_of
        g = GridRoad(GRID["m"], GRID["n"], GRID["length"])
        entry = g.generate_entrypoints(0)
        orc = OracleEnv(GRID["m"], GRID["n"], GRID["length"], GRID["capacity"], g.dest, g.phases, g.nexts, n_envs=E_WALK,
                        rate=GRID["rate"], validate=True)
        orc.reset(np.zeros((E_WALK, orc.I), np.int32))
        x, v, w, ld, lc = initial_state()
        for k in range(E_WALK):
            orc.load_planes(k, x[k], v[k], w[k], ld[k], lc[k])
        ticks = []
        for act, cnt in scenario(orc.I, len(entry)):
            for t in range(cnt.shape[0]):
                ticks.append(orc.leading.copy())
                orc.step(act, roads_of(cnt[t], entry))
        _walk.update(popped=orc.leading != ticks[-1], x=orc.x.copy(), v=orc.v.copy(), leading=orc.leading.copy(),
                     lastcar=orc.lastcar.copy(), cars=orc.cars_on_roads_flat(), tiles=tiles_of(g.nexts, 4 * GRID["m"] * GRID["n"]))
    return _walk


def test_walk_scenario_is_not_vacuous():
    """Conditions on the INPUTS of tests/test_gpu_walk.py (the oracle alone, no device)"""
    s = oracle_walk()
    cars, popped, tiles = s["cars"], s["popped"], s["tiles"]
    assert cars.shape == (E_WALK, 80) and [len(t) for t in tiles] == [64, 16]
    assert CALLS[-1] % 2 == 0 and CALLS[-1] >= 2
    for t in tiles:
        assert popped[:, t].any()                                   # head_rows().any() where two-tick passes run ...
        assert (cars[:, t][popped[:, t]] >= 9).any()                # ... above a column of nine cars or more, in both tiles
        assert (cars[:, t] > 0).any(axis=1).all()                   # both tiles hold live roads in every env
    assert (cars == 0).any()
    counts = set(cars.ravel().tolist())
    assert any(c % 8 == 7 for c in counts) and any(c % 8 in (0, 1) and c >= 8 for c in counts)     # either side of a multiple of eight
    print("walk scenario: %d cars, counts %s, %d roads handed a head over in the last tick, %d of them with nine cars or more, "
          "%d empty roads" % (cars.sum(), sorted(counts), popped.sum(), (cars[popped] >= 9).sum(), (cars == 0).sum()))
