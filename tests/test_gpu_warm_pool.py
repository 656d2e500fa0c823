"""Warm restarts (tfx_set_episode_pool, include/tfx.h): with a pool of warmed-up envs attached, the masked restart at the
begin of a decision is a clone of the pool env rule 3 names - against today's loop on a second handle with episodes off
(bit for bit): `agent_step()`, then `clone_envs(where(end, slots, -1), source=pool, streams=False, episodes=False)` with
`end` from the NumPy model of the accounting (tests/test_episodes_host.py) and `slots` from devrng.episode_pool_slots.
B's clone is enqueued where A's restart runs: ahead of the next decision (and behind a step of the pool in between).

The scenarios were picked with the CPU oracle (oracle/oracle.py), the loop above emulated on single-env oracles as the
docstring of tests/test_gpu_episodes.py describes (the wrappers tick by tick, a restart = the pool oracle's arrays copied
over the env's): 3x3 grid of 150 m roads, 8 live envs from an empty reset, 10-tick decisions with remi, periodic arrivals,
env k holding phase (decision // (k + 1)) & 1, first phases from RandomState(3), seed 3, a pool of 3 envs warmed up for
3 decisions under the same rule (60 / 46 cars on each pool env's train roads, none overflowed):
  "limit"  capacity 12, a car per entry road every 6 ticks, max_decisions 8, 20 decisions.  The oracle run showed
           overflows [4, 3, 3, 4, 2, 3, 4, 4], truncations [0, 0, 0, 0, 1, 0, 0, 0] and restarts [3, 3, 3, 3, 3, 3, 4, 3] per
           env; ends (decision: envs -> slots) 6: 2 5 6 7 -> 2 0 0 2, 7: 0 1 3 4 -> 0 0 0 0, 10: 5 6 -> 1 1,
           11: 0 2 3 7 -> 0 2 2 1, 12: 1 4 -> 0 2, 14: 6 -> 1, 15: 0 2 3 5 7 -> 2 0 0 1 2, 17: 1 4 -> 0 0, 18: 6 -> 1.
           From an empty map the first overflow takes 6-7 decisions, from a pool env 3-4.  The same run with the live
           clock started at tick 7 gave the same counts.
  "free"   capacity 12, a car every 8 ticks, no limit, 14 decisions: overflows and restarts [1, 0, 0, 0, 1, 1, 1, 1]
           (ends 8: 7 -> 2, 10: 4 -> 0, 11: 0 5 -> 0 0, 12: 6 -> 0), envs 1, 2, 3 never end.
As in tests/test_gpu_episodes.py "an env never ends" cannot share a run with a time limit, so the conditions are asserted
over the two scenarios: overflow, truncation, two restarts, two envs on one slot and two envs on different slots in one
decision in "limit"; overflow next to an env that never ends, and two envs on one slot, in "free"."""
import ctypes

import numpy as np
import pytest

from oracle.oracle import live_mask
from test_gpu_episodes import (EpisodeModel, GRID, PATHS, SEED, actions_for, assert_accounting, assert_same_state,
                               count_launches, first_phases, force_path, host, make_engine)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from gym_traffic import _native as nat  # noqa: E402
from gym_traffic import devrng  # noqa: E402
from gym_traffic.core import TfxEngine  # noqa: E402

SCENARIOS = {"limit": dict(C=12, period=6, M=8, K=20), "free": dict(C=12, period=8, M=0, K=14)}
N_POOL, WARM, POOL_OFF = 3, 3, 100
HET_ROWS = np.array([[11.11, 4.0, 3.0, 4.0, 13.89, 6.0, 2.0, 1.0], [9.0, 5.0, 2.0, 3.0, 11.0, 5.0, 1.5, 2.0]], np.float32)


@pytest.fixture(params=PATHS)
def step_path(request, monkeypatch):
    force_path(monkeypatch, request.param)
    yield request.param


def periodic(sc):
    return lambda eng: eng.set_spawns(period=sc["period"])


def pool_decision(pool, s):
    pool.set_actions(actions_for(np.arange(pool.E), pool.I, s))
    return host(pool.agent_step(GRID["T"]))


def make_pool(sc, engine_kw=None, arrivals=None, n=N_POOL, warm=WARM):
    """n envs warmed up for `warm` decisions; none may overflow (a condition on the scenario)"""
    pool = make_engine(sc["C"], n, POOL_OFF, **(engine_kw or {}))
    pool.reset(first_phases(GRID["E"], pool.I)[:n])
    (arrivals or periodic(sc))(pool)
    for s in range(warm):
        assert not pool_decision(pool, s)[2].any(), s
    return pool


def train_cars(eng):
    ld, lc = eng.leading.cpu().numpy(), eng.lastcar.cpu().numpy()
    return np.array([int(live_mask(ld[k], lc[k], eng.C)[:eng.r].sum()) for k in range(eng.E)])


def stash(pool):
    """a snapshot of every pool env on a third handle under the pool's clock, and the per-env words assert_same_state skips"""
    snap = TfxEngine(GRID["m"], GRID["n"], GRID["L"], pool.C, n_envs=pool.E, env_id_offset=POOL_OFF, validate=pool.validate,
                     **(dict(archetypes=pool.archetypes, planes=3, layout="transposed") if pool.het else {}))
    snap.reset(np.zeros((pool.E, pool.I), np.int32))
    snap.set_tick(pool.tick)
    snap.clone_envs(np.arange(pool.E, dtype=np.int32), source=pool)
    return snap, host((pool.rewards, pool.passed_dst, pool.done_tick))


def assert_pool_untouched(pool, snap, words):
    assert_same_state(pool, snap, "pool")
    for u, v in zip(host((pool.rewards, pool.passed_dst, pool.done_tick)), words):
        assert np.array_equal(u.view(np.uint8), v.view(np.uint8))
    if pool.n_trips is not None:
        assert np.array_equal(pool.n_trips.cpu().numpy(), snap.n_trips.cpu().numpy())


def run_warm(sc, engine_kw=None, arrivals=None, tick0=0, pool_step_at=None, detach_at=None, hook=None, remi=True, warm=WARM):
    """Handle A (episodes on, the pool attached) against handle B (episodes off, today's loop), the accounting against the
    model after every decision.  pool_step_at: the pool runs one more decision ahead of that live decision; detach_at: A
    loses its pool ahead of that decision and B turns to reset_envs(end, episode_phases(...)); hook(s, a, pool): called
    ahead of every decision.  Returns a dict of what happened."""
    engine_kw = engine_kw or {}
    arrivals = arrivals or periodic(sc)
    E, T, K, M = GRID["E"], GRID["T"], sc["K"], sc["M"]
    pool = make_pool(sc, engine_kw, arrivals, warm=warm)
    assert (train_cars(pool) > 0).all()                       # every pool env holds cars on its train roads
    assert not (pool.done_tick.cpu().numpy() > 0).any()       # ... and none is overflowed when attached
    a, b = make_engine(sc["C"], **engine_kw), make_engine(sc["C"], **engine_kw)
    I, ids = a.I, np.arange(E)
    ph = first_phases(E, I)
    for eng in (a, b):
        eng.reset(ph)
        if tick0:
            eng.set_tick(tick0)
        arrivals(eng)
    a.set_episodes(max_decisions=M, seed=SEED)
    a.set_episode_pool(pool)
    assert a.episode_pool is pool
    snap, words = stash(pool)
    model = EpisodeModel(E, I, M)
    out = dict(term=np.zeros(E, int), trunc=np.zeros(E, int), restart=np.zeros(E, int), same=False, diff=False, trips=0,
               a=a, b=b, pool=pool, model=model)
    end = np.zeros(E, bool)
    for s in range(K):
        if hook:
            hook(s, a, pool)
        if s == pool_step_at:
            before = host((pool.leading, pool.lastcar))
            assert not pool_decision(pool, warm)[2].any()
            assert any(not np.array_equal(u, v) for u, v in zip(before, host((pool.leading, pool.lastcar))))
            assert end.any()                                  # (the restart that follows reads the stepped pool)
        if s == detach_at:
            assert end.any()                                  # (the restart that follows is an empty one)
            a.set_episode_pool(None)
        # B's restart, where A's runs: ahead of the decision, behind whatever happened to the pool
        if end.any():
            out["restart"] += end
            if detach_at is not None and s >= detach_at:
                b.reset_envs(end, devrng.episode_phases(SEED, ids, model.ep_index, I))
            else:
                slots = devrng.episode_pool_slots(SEED, ids, model.ep_index, pool.E)
                taken = slots[end]
                out["same"] |= len(set(taken.tolist())) < len(taken)
                out["diff"] |= len(set(taken.tolist())) > 1
                b.clone_envs(np.where(end, slots, -1).astype(np.int32), source=pool, streams=False, episodes=False)
        act = actions_for(ids, I, s)
        a.set_actions(act)
        b.set_actions(act)
        oa = host(a.agent_step(T, remi=remi))
        ob = host(b.agent_step(T, remi=remi))
        for u, v, name in zip(oa, ob, ("aobs", "areward", "adone")):
            assert np.array_equal(u.view(np.uint8), v.view(np.uint8)), (s, name)
        end = model.decision(ob[1], ob[2]).astype(bool)
        assert_accounting(a, model, s)
        if a.n_trips is not None:
            assert np.array_equal(a.n_trips.cpu().numpy(), b.n_trips.cpu().numpy()), s
            assert np.array_equal(a.trip_times.cpu().numpy().view(np.int32), b.trip_times.cpu().numpy().view(np.int32)), s
            # (the trips logged in episodes that began as a clone of a pool env)
            out["trips"] = max(out["trips"], int((a.n_trips.cpu().numpy() * (out["restart"] > 0)).max()))
        out["term"] += ob[2] != 0
        out["trunc"] += model.truncated
    out["cars"] = assert_same_state(a, b, "final")
    assert a.clone_skipped() == 0                             # (the restart never touches the counter)
    if pool_step_at is None:
        assert_pool_untouched(pool, snap, words)
    return out


# ---- 1, 2: equivalence on every step path, and the runs are not vacuous ------------------------------------------------
@pytest.mark.parametrize("scenario", ["limit", "free"])
def test_state_equivalence_and_accounting(step_path, scenario):
    o = run_warm(SCENARIOS[scenario])
    assert o["cars"] > 20
    assert (o["term"] > 0).any()                              # an env ends by overflow
    assert o["same"]                                          # two envs restart from the same slot in one decision
    if scenario == "limit":
        assert (o["trunc"] > 0).any()                         # ... one by the time limit
        assert (o["restart"] >= 2).any()                      # ... one restarts twice
        assert o["diff"]                                      # ... two envs from different slots in one decision
    else:
        assert ((o["term"] + o["trunc"]) == 0).any()          # ... and one never ends
        assert o["trunc"].sum() == 0
    kernel = o["a"].lib.tfx_step_kernel(o["a"].h).decode()
    assert (kernel == "k_res") == (step_path == "resident"), kernel


def test_equivalence_summed_rewards(step_path):
    o = run_warm(SCENARIOS["limit"], remi=False)
    assert (o["term"] > 0).any() and (o["restart"] >= 2).any()


# ---- 3: the pool is read at restart time (run_warm checks that it is never written) -----------------------------------
@pytest.mark.parametrize("path", ["resident", "pairs"])
def test_pool_is_read_when_the_restart_runs(monkeypatch, path):
    """The pool runs one more decision between live decisions 6 and 7 (the oracle: envs 2, 5, 6, 7 end in decision 6):
    the restart inside decision 7 takes the stepped envs, as B's clone - enqueued behind the pool's step - does."""
    force_path(monkeypatch, path)
    o = run_warm(SCENARIOS["limit"], pool_step_at=7)
    assert (o["restart"] >= 2).any() and o["cars"] > 20


# ---- 4: the clocks differ by an odd number of ticks that is no multiple of the decision length -------------------------
@pytest.mark.parametrize("path", ["pertick", "pairs"])
def test_clock_rebasing_validate_mode(monkeypatch, path):
    """A trip through the 3x3 grid takes some 90 ticks, more than a warm episode of "limit" lasts, so this test has a
    scenario of its own (the oracle again, validate mode, the trip log copied with the pool oracle's arrays): capacity
    12, a car every 8 ticks, max_decisions 12, 30 decisions, the pool warmed up for 6 decisions - restarts [4, 3, 3, 4, 5,
    4, 3, 5], overflows [4, 3, 2, 3, 5, 4, 2, 5], up to 6 trips logged in an episode that began as a clone, every one of
    them by a car that arrived from the pool or behind one.  The pool's clock stands at 60 after its warm-up, the live
    handles' starts at 7 (set after the reset, which zeroes the clock): ahead of decision s spawn ticks are rebased by
    10 s - 53, odd and no multiple of the decision length, read by the kernel on the device - and the trips of cars that
    arrived from the pool take what they would have taken (run_warm compares n_trips and trip_times after every
    decision)."""
    force_path(monkeypatch, path)
    o = run_warm(dict(C=12, period=8, M=12, K=30), dict(validate=True), tick0=7, warm=6)
    a, pool = o["a"], o["pool"]
    assert (a.tick - pool.tick) % 2 == 1 and (a.tick - pool.tick) % GRID["T"] != 0
    assert a.n_trips is not None and o["trips"] > 0
    assert (o["term"] > 0).any() and (o["trunc"] > 0).any() and (o["restart"] >= 2).any()


# ---- 5: heterogeneous cars ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["pertick", "pairs"])
def test_equivalence_heterogeneous_cars(monkeypatch, path):
    force_path(monkeypatch, path)
    o = run_warm(SCENARIOS["limit"], dict(archetypes=HET_ROWS, planes=3, layout="transposed"))
    assert o["a"].het and o["cars"] > 20 and (o["term"] > 0).any() and (o["restart"] >= 2).any()


# ---- 6: on-device arrival streams run on across a warm restart -------------------------------------------------------------
@pytest.mark.parametrize("kind", ["poisson", "regular"])
@pytest.mark.parametrize("path", ["resident", "pairs"])
def test_restarted_envs_continue_their_own_stream(monkeypatch, path, kind):
    """One car per tick and env from the on-device stream (seed 5), a time limit of 4 decisions so that every env
    restarts; B's clone is made without TFX_CLONE_STREAM, so B's envs keep stream and position - and A equals B."""
    force_path(monkeypatch, path)
    sc = dict(C=12, M=4, K=10)
    arrivals = (lambda eng: eng.set_poisson(1.0, seed=5)) if kind == "poisson" else (lambda eng: eng.set_regular(1.0, seed=5))
    o = run_warm(sc, arrivals=arrivals)
    assert o["restart"].min() >= 2 and o["cars"] > 20 and o["same"] and o["diff"]


# ---- 7: sharding -------------------------------------------------------------------------------------------------------------
def test_sharding(step_path):
    """8 envs as one handle equal 3 + 5 envs as two handles with env_id_offset 0 and 3, all attached to the same pool."""
    sc, E = SCENARIOS["limit"], GRID["E"]
    pool = make_pool(sc)
    outs = []
    for n_envs, off in ((E, 0), (3, 0), (E - 3, 3)):
        eng = make_engine(sc["C"], n_envs, off)
        ids = np.arange(n_envs) + off
        eng.reset(first_phases(E, eng.I)[ids])
        eng.set_spawns(period=sc["period"])
        eng.set_episodes(max_decisions=sc["M"], seed=SEED)
        eng.set_episode_pool(pool)
        per = []
        for s in range(sc["K"]):
            eng.set_actions(actions_for(ids, eng.I, s))
            per.append(host(eng.agent_step(GRID["T"])) + host((eng.ep_index, eng.ep_len, eng.final_return, eng.obs, eng.leading)))
        outs.append(per)
    whole, lo, hi = outs
    for s in range(sc["K"]):
        for j in range(len(whole[s])):
            assert np.array_equal(whole[s][j][:3], lo[s][j]), (s, j)
            assert np.array_equal(whole[s][j][3:], hi[s][j]), (s, j)
    assert whole[-1][3].max() >= 2                               # (ep_index: somebody restarted twice)


# ---- 8: attach / detach ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["resident", "pairs"])
def test_detaching_returns_to_empty_restarts(monkeypatch, path):
    """Detached ahead of decision 11 (the oracle: envs 5 and 6 end in decision 10): from then on rule-2 restarts."""
    force_path(monkeypatch, path)
    o = run_warm(SCENARIOS["limit"], detach_at=11)
    assert o["a"].episode_pool is None and (o["restart"] >= 2).any() and o["cars"] > 20


@pytest.mark.parametrize("path", ["resident", "pertick", "pairs"])
def test_attaching_and_detaching_recaptures_the_graph(monkeypatch, path):
    """attach / detach / attach between decisions: the captured graph is never a stale one - results equal the eager run"""
    sc, E = SCENARIOS["limit"], GRID["E"]
    outs = []
    for graph in ("1", "0"):
        force_path(monkeypatch, path)
        monkeypatch.setenv("TFX_GRAPH", graph)
        pool = make_pool(sc)
        eng = make_engine(sc["C"])
        eng.reset(first_phases(E, eng.I))
        eng.set_spawns(period=sc["period"])
        eng.set_episodes(max_decisions=3, seed=SEED)
        res = []
        for s in range(16):
            if s in (2, 11):
                eng.set_episode_pool(pool)
            if s == 8:
                eng.set_episode_pool(None)
            eng.set_actions(actions_for(np.arange(E), eng.I, s))
            res.append(host(eng.agent_step(GRID["T"])) + host((eng.ep_index, eng.ep_len, eng.final_return, eng.obs, eng.leading)))
        outs.append(res)
    for s, (u, v) in enumerate(zip(*outs)):
        for p, q in zip(u, v):
            assert np.array_equal(p, q), s
    assert outs[0][-1][3].min() >= 4                             # (every env restarted in every span)


def test_pool_is_inert_while_episodes_are_off(step_path):
    sc, E = SCENARIOS["limit"], GRID["E"]
    pool = make_pool(sc)
    a, b = make_engine(sc["C"]), make_engine(sc["C"])
    for eng in (a, b):
        eng.reset(first_phases(E, eng.I))
        eng.set_spawns(period=sc["period"])
    a.set_episode_pool(pool)
    for s in range(8):
        act = actions_for(np.arange(E), a.I, s)
        a.set_actions(act)
        b.set_actions(act)
        for u, v in zip(host(a.agent_step(GRID["T"])), host(b.agent_step(GRID["T"]))):
            assert np.array_equal(u.view(np.uint8), v.view(np.uint8)), s
    assert assert_same_state(a, b) > 20


# ---- 9: the launch budget ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["resident", "pertick", "pairs"])
def test_launch_budget(monkeypatch, path):
    force_path(monkeypatch, path)
    monkeypatch.setenv("TFX_GRAPH", "0")          # (replays of a captured graph bypass the injection)
    sc = SCENARIOS["limit"]
    pool = make_pool(sc)
    eng = make_engine(sc["C"])
    eng.set_spawns(period=sc["period"])
    eng.set_actions(actions_for(np.arange(eng.E), eng.I, 0))
    eng.set_episodes(max_decisions=4, seed=SEED)
    on = count_launches(eng, GRID["T"])
    eng.set_episode_pool(pool)
    warm = count_launches(eng, GRID["T"])
    print("launches per decision, %s: %d with episodes on, %d with a pool attached" % (path, on, warm))
    assert on <= warm <= on + 1
    eng.set_episode_pool(None)
    assert count_launches(eng, GRID["T"]) == on


# ---- 10: errors ----------------------------------------------------------------------------------------------------------------
def refused(eng, pool_handle, code, word):
    with pytest.raises(nat.TfxError) as exc:
        nat.check(eng.lib.tfx_set_episode_pool(eng.h, pool_handle))
    assert ("tfx error %d:" % code) in str(exc.value) and word in str(exc.value), str(exc.value)


def test_refusals_leave_the_handle_and_its_pool_alone(monkeypatch):
    force_path(monkeypatch, "pairs")
    sc = SCENARIOS["limit"]
    C = sc["C"]
    others = [(make_engine(C + 1, N_POOL), "capacity"),
              (TfxEngine(GRID["m"], GRID["n"], GRID["L"] + 10.0, C, n_envs=N_POOL), "length"),
              (make_engine(C, N_POOL, archetypes=np.array([[11.11, 4.0, 3.0, 4.0, 12.5, 6.0, 2.0, 1.0]], np.float32)), "archetype table")]
    for eng, _ in others:
        eng.reset(np.zeros((eng.E, eng.I), np.int32))
    unbound = ctypes.c_void_p()

    def hook(s, a, pool):
        if s not in (0, 7, 12):
            return
        for eng, word in others:
            refused(a, eng.h, -1, word)
        refused(a, a.h, -1, "own pool")
        if not unbound.value:
            nat.check(a.lib.tfx_create(ctypes.byref(a.cfg), ctypes.byref(unbound)))
        refused(a, unbound, -2, "tfx_bind_buffers")
        assert a.episode_pool is pool

    try:
        o = run_warm(sc, hook=hook)          # (equal to B's loop on the pool attached before the refusals)
    finally:
        if unbound.value:
            nat.lib().tfx_destroy(unbound)
    assert (o["restart"] >= 2).any() and o["same"] and o["diff"]
    # ... and a handle with no pool attached stays without one
    eng = make_engine(C)
    eng.reset(first_phases(eng.E, eng.I))
    eng.set_spawns(period=sc["period"])
    refused(eng, others[0][0].h, -1, "capacity")
    eng.set_episodes(max_decisions=2, seed=SEED)
    for s in range(3):
        eng.agent_step(GRID["T"])
    assert train_cars(eng).max() < 30 and eng.ep_index.cpu().numpy().min() == 1      # (restarted empty after decision 2)


# ---- 11: TrafficVecEnv ---------------------------------------------------------------------------------------------------------
def make_venv(E=6, **kw):
    from gym_traffic.envs.vec_env import TrafficVecEnv
    args = dict(capacity=12, spawn='periodic', spawn_period=6, seed=SEED)
    args.update(kw)
    return TrafficVecEnv(E, 3, 3, 150.0, **args)


def test_vec_env_make_warm_pool(monkeypatch):
    force_path(monkeypatch, "pairs")
    venv = make_venv(validate=True, autoreset=True, episode_len=4)
    pool = venv.make_warm_pool(N_POOL, WARM)
    assert pool.num_envs == N_POOL and not pool.autoreset and pool.env_id_offset == venv.POOL_ENV_ID_OFFSET
    assert pool.engine.tick == WARM * 10 and not pool.done.cpu().numpy().any()
    assert (train_cars(pool.engine) > 0).all()
    assert not pool.engine.n_trips.cpu().numpy().any()
    assert venv.warm_pool is None                                # (made, not attached)
    # the same seed makes the same pool; the fixed cycle is the other action rule
    again = venv.make_warm_pool(N_POOL, WARM)
    assert assert_same_state(pool.engine, again.engine) > 0
    assert (train_cars(venv.make_warm_pool(2, 2, cycle_period=5, env_id_offset=50).engine) > 0).all()
    # capacity 3 holds one car per road and a car arrives on every entry road in every tick: the second tick overflows
    # whatever the lights do (the oracle agrees: done after one decision under either phase)
    tiny = make_venv(capacity=3, spawn_period=1, autoreset=True)
    with pytest.raises(RuntimeError, match="Episode completed during warmup"):
        tiny.make_warm_pool(2, 1)
    plain = make_venv()
    with pytest.raises(RuntimeError, match="autoreset"):
        plain.set_warm_pool(pool)
    with pytest.raises(RuntimeError, match="set_warm_pool"):
        venv.reset(warm=True)


def test_vec_env_autoreset_with_a_pool_equals_the_manual_loop(step_path):
    E, M = 6, 4
    a = make_venv(E, autoreset=True, episode_len=M)
    b = make_venv(E)
    pool = a.make_warm_pool(N_POOL, WARM)
    a.set_warm_pool(pool)
    ph = first_phases(E, a.engine.I)
    a.reset(ph)
    b.reset(ph)
    model = EpisodeModel(E, a.engine.I, M)
    ids = np.arange(E)
    for s in range(10):
        act = torch.as_tensor(actions_for(ids, a.engine.I, s)).to(a.engine.device)
        oa = host(a.agent_step(act, n_ticks=10))
        ob = host(b.agent_step(act, n_ticks=10))
        for u, v in zip(oa, ob):
            assert np.array_equal(u.view(np.uint8), v.view(np.uint8)), s
        end = model.decision(ob[1], ob[2]).astype(bool)
        assert np.array_equal(a.episode_length.cpu().numpy(), model.ep_len)
        assert np.array_equal(a.final_return.cpu().numpy(), model.final_return)
        if s + 1 < 10:
            slots = devrng.episode_pool_slots(SEED, ids, model.ep_index, N_POOL)
            b.clone_envs(np.where(end, slots, -1).astype(np.int32), source=pool, streams=False, episodes=False)
    assert model.ep_index.min() >= 2 and assert_same_state(a.engine, b.engine) > 20
    a.set_warm_pool(None)
    assert a.warm_pool is None and a.engine.episode_pool is None


def test_vec_env_warm_reset(monkeypatch):
    """reset(warm=True): env e is the pool env episode_pool_slots names - cars, lights, spawn ticks under the env's clock"""
    force_path(monkeypatch, "pairs")
    E = 8
    venv = make_venv(E, validate=True, autoreset=True, episode_len=4, env_id_offset=5)
    pool = venv.make_warm_pool(N_POOL, WARM)
    venv.set_warm_pool(pool)
    venv.reset(warm=True)
    slots = devrng.episode_pool_slots(SEED, np.arange(E) + 5, 0, N_POOL)
    assert len(set(slots.tolist())) > 1
    eng, src = venv.engine, pool.engine
    for name in ("leading", "lastcar", "obs", "waiting"):
        assert np.array_equal(getattr(eng, name).cpu().numpy(), getattr(src, name).cpu().numpy()[slots]), name
    (x, v, w), (px, pv, pw) = eng.planes_numpy(), src.planes_numpy()
    ld, lc = eng.leading.cpu().numpy(), eng.lastcar.cpu().numpy()
    n_cars = 0
    for e in range(E):
        live = live_mask(ld[e], lc[e], eng.C)
        n_cars += int(live.sum())
        assert np.array_equal(x[e][live].view(np.int32), px[slots[e]][live].view(np.int32)), e
        assert np.array_equal(v[e][live].view(np.int32), pv[slots[e]][live].view(np.int32)), e
        assert np.array_equal(w[e][live], pw[slots[e]][live] - np.float32(src.tick)), e      # (tick 0 here, 30 there)
    assert n_cars > 20 and not venv.episode_length.cpu().numpy().any()
    out = venv.agent_step(cycle_period=5)
    assert len(out) == 3
