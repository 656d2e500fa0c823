"""Episodes on the device (tfx_set_episodes, include/tfx.h): masked restart with phases drawn on the device at the
begin of a decision, the time limit, return / length per episode at its end - against today's host loop
`agent_step(); reset_envs(mask, phase_init)` on a second handle (bit for bit), against the oracle, and against the NumPy
model of the accounting in tests/test_episodes_host.py.

The scenarios were picked with the CPU oracle (oracle/oracle.py, the wrappers emulated tick by tick as
emulate_agent_step below does, restarts by devrng.episode_phases with seed 3), 3x3 grid of 150 m roads, 8 envs,
10-tick decisions with remi, periodic arrivals, env k holding phase (decision // (k + 1)) & 1, first phases from
RandomState(3):
  "limit"  capacity 12, a car per entry road every 6 ticks, max_decisions 8, 20 decisions.  The oracle run showed
           overflows [2, 2, 1, 2, 1, 1, 2, 2] and truncations [0, 0, 1, 0, 1, 1, 0, 0] per env (first overflows at
           decisions 7, 7, 6, 7, 8, 6, 6, 6), every env ending twice before the last decision, i.e. restarting twice.
  "free"   capacity 12, a car every 8 ticks, no limit, 14 decisions: envs 0, 4, 5, 6, 7 overflow once (decisions 11, 10,
           11, 12, 8), envs 1, 2, 3 never end.
With a time limit every env's episode ends by then, so "an env that never ends" cannot share a run with "an env ends by
the time limit": the four conditions are asserted over the two scenarios - overflow, time limit and two restarts in
"limit", overflow next to an env that never ends in "free"."""
import ctypes

import numpy as np
import pytest

from oracle.oracle import OracleEnv, live_mask
from test_episodes_host import EpisodeModel

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from gym_traffic import _native as nat  # noqa: E402
from gym_traffic import devrng  # noqa: E402
from gym_traffic import workload as wl  # noqa: E402
from gym_traffic.core import TfxEngine  # noqa: E402

SEED = 3
GRID = dict(m=3, n=3, L=150.0, T=10, E=8)
SCENARIOS = {"limit": dict(C=12, period=6, M=8, K=20), "free": dict(C=12, period=8, M=0, K=14)}
PATHS = ["resident", "pertick", "pairs", "pairs_seg", "pairs_seg_launches", "ring", "pairs_eager"]
EP_NAMES = ("ep_return", "ep_len", "final_return", "final_len", "truncated", "ep_index")


def force_path(monkeypatch, path):
    """The switches of tests/test_gpu_agent_step.py's fixture, plus the ring layout and the eager (no graph) sequence."""
    monkeypatch.setenv("TFX_RESIDENT", "1" if path == "resident" else "0")
    monkeypatch.setenv("TFX_RES_EPB", "3")
    monkeypatch.setenv("TFX_PAIRS", "2" if path.startswith("pairs") else "0")
    monkeypatch.setenv("TFX_TAIL", "0" if path == "pairs_seg_launches" else "2")
    monkeypatch.setenv("TFX_SPLIT", "2")
    monkeypatch.setenv("TFX_TT_SEG", "2" if path.startswith("pairs_seg") else "0")
    monkeypatch.setenv("TFX_TT_SEGS", "4" if path == "pairs_seg_launches" else "2")
    monkeypatch.setenv("TFX_GRAPH", "0" if path == "pairs_eager" else "1")
    if path == "ring":
        monkeypatch.setenv("TFX_LAYOUT", "ring")
    else:
        monkeypatch.delenv("TFX_LAYOUT", raising=False)


@pytest.fixture(params=PATHS)
def step_path(request, monkeypatch):
    force_path(monkeypatch, request.param)
    yield request.param


def actions_for(env_ids, I, s):
    """env g holds phase (s // (g + 1)) & 1 in decision s"""
    a = np.array([((s // (int(g) + 1)) & 1) for g in env_ids], np.int32)
    return np.ascontiguousarray(np.repeat(a[:, None], I, axis=1))


def first_phases(E, I):
    return np.random.RandomState(SEED).randint(2, size=(E, I)).astype(np.int32)


def make_engine(C, E=GRID["E"], off=0, **kw):
    return TfxEngine(GRID["m"], GRID["n"], GRID["L"], C, n_envs=E, env_id_offset=off, **kw)


def host(tensors):
    return [t.cpu().numpy().copy() for t in tensors]


def assert_same_state(a, b, where=""):
    """leading, lastcar, obs, waiting and every live car's (x, v[, w, row]) by ring slot; returns the live cars"""
    la, ca = a.leading.cpu().numpy(), a.lastcar.cpu().numpy()
    assert np.array_equal(la, b.leading.cpu().numpy()), where
    assert np.array_equal(ca, b.lastcar.cpu().numpy()), where
    assert np.array_equal(a.obs.cpu().numpy(), b.obs.cpu().numpy()), where
    assert np.array_equal(a.waiting.cpu().numpy(), b.waiting.cpu().numpy()), where
    pa, pb = a.planes_numpy(), b.planes_numpy()
    ra = a.arch.cpu().numpy() if a.het else None
    rb = b.arch.cpu().numpy() if b.het else None
    n_cars = 0
    for k in range(a.E):
        live = live_mask(la[k], ca[k], a.C)
        n_cars += int(live.sum())
        for u, v in zip(pa, pb):
            assert np.array_equal(u[k][live].view(np.int32), v[k][live].view(np.int32)), (where, k)
        if ra is not None:
            assert np.array_equal(ra[k][live], rb[k][live]), (where, k)
    return n_cars


def assert_accounting(eng, model, where=""):
    for name in EP_NAMES:
        got, want = getattr(eng, name).cpu().numpy(), getattr(model, name)
        assert got.dtype == want.dtype and np.array_equal(got.view(np.uint8), want.view(np.uint8)), (where, name, got, want)


def run_equivalence(sc, engine_kw=None, remi=True):
    """Handle A with episodes on against handle B driven by today's loop, the accounting against the model after every
    decision; returns per-env (overflows, truncations, restarts), the live cars at the end, A and the model."""
    engine_kw = engine_kw or {}
    E, T, K, M = GRID["E"], GRID["T"], sc["K"], sc["M"]
    a = make_engine(sc["C"], **engine_kw)
    b = make_engine(sc["C"], **engine_kw)
    I, ids = a.I, np.arange(E)
    ph = first_phases(E, I)
    for eng in (a, b):
        eng.reset(ph)
        eng.set_spawns(period=sc["period"])
    a.set_episodes(max_decisions=M, seed=SEED)
    model = EpisodeModel(E, I, M)
    n_term, n_trunc, n_restart = np.zeros(E, int), np.zeros(E, int), np.zeros(E, int)
    for s in range(K):
        act = actions_for(ids, I, s)
        a.set_actions(act)
        b.set_actions(act)
        oa = host(a.agent_step(T, remi=remi))
        ob = host(b.agent_step(T, remi=remi))
        for u, v, name in zip(oa, ob, ("aobs", "areward", "adone")):
            assert np.array_equal(u.view(np.uint8), v.view(np.uint8)), (s, name)
        end = model.decision(ob[1], ob[2])
        assert_accounting(a, model, s)
        if a.n_trips is not None:
            # validate mode: the trip log of an episode that has just ended is still there (B's reset has not run yet)
            assert np.array_equal(a.n_trips.cpu().numpy(), b.n_trips.cpu().numpy()), s
            assert np.array_equal(a.trip_times.cpu().numpy(), b.trip_times.cpu().numpy()), s
        n_term += ob[2] != 0
        n_trunc += model.truncated
        if s + 1 < K:      # (A restarts these envs when its next decision begins: after the last one neither does)
            n_restart += end
            b.reset_envs(end, devrng.episode_phases(SEED, ids, model.ep_index, I))
    n_cars = assert_same_state(a, b, "final")
    return n_term, n_trunc, n_restart, n_cars, a, model


@pytest.mark.parametrize("scenario", ["limit", "free"])
def test_state_equivalence_and_accounting(step_path, scenario):
    """Bit for bit the state sequence of `agent_step(); reset_envs(adone | truncated, episode_phases(...))`, the
    accounting exactly the NumPy model's - and the run is not vacuous (module docstring)."""
    n_term, n_trunc, n_restart, n_cars, a, _ = run_equivalence(SCENARIOS[scenario])
    assert n_cars > 20
    assert (n_term > 0).any()                                   # an env ends by overflow
    if scenario == "limit":
        assert (n_trunc > 0).any()                              # ... one by the time limit
        assert (n_restart >= 2).any()                           # ... one restarts twice
    else:
        assert ((n_term + n_trunc) == 0).any()                  # ... and one never ends
        assert n_trunc.sum() == 0
    kernel = a.lib.tfx_step_kernel(a.h).decode()
    assert (kernel == "k_res") == (step_path == "resident"), kernel


def test_equivalence_summed_rewards(step_path):
    """remi off: the decision's reward is the sum over its ticks (overflow penalties included)"""
    n_term, n_trunc, _, _, _, model = run_equivalence(SCENARIOS["limit"], remi=False)
    assert (n_term > 0).any() and (n_trunc > 0).any()
    assert (model.final_return < 0).any()


@pytest.mark.parametrize("path", ["pertick", "pairs"])
def test_equivalence_heterogeneous_cars(monkeypatch, path):
    force_path(monkeypatch, path)
    rows = np.array([[11.11, 4.0, 3.0, 4.0, 13.89, 6.0, 2.0, 1.0], [9.0, 5.0, 2.0, 3.0, 11.0, 5.0, 1.5, 2.0]], np.float32)
    n_term, _, n_restart, n_cars, a, _ = run_equivalence(SCENARIOS["limit"], dict(archetypes=rows, planes=3, layout="transposed"))
    assert a.het and n_cars > 20 and (n_term > 0).any() and (n_restart > 0).any()


@pytest.mark.parametrize("path", ["pertick", "pairs"])
def test_equivalence_validate_mode(monkeypatch, path):
    """... and the trip log of an ended episode stays readable until the next decision begins (run_equivalence compares
    it after every decision, before the other handle's reset clears it)"""
    force_path(monkeypatch, path)
    n_term, _, n_restart, _, a, _ = run_equivalence(SCENARIOS["limit"], dict(validate=True))
    assert a.n_trips is not None and (n_term > 0).any() and (n_restart > 0).any()


def emulate_agent_step(orcs, tick0, action, entry, n_ticks, remi, period, archetypes=None):
    """Repeater._step + Remi._step per env on single-env oracles; returns (aobs, areward, adone).
    (a copy of tests/test_gpu_agent_step.py's helper)"""
    E = len(orcs)
    r, I = orcs[0].r, orcs[0].I
    aobs = np.zeros((E, 2 * r + I), np.float32)
    arew = np.zeros((E, I), np.float32)
    adone = np.zeros(E, np.uint8)
    for k, orc in enumerate(orcs):
        total_obs = np.zeros(2 * r + I, np.float32)
        total_reward = 0
        done = False
        for t in range(n_ticks):
            tick = tick0 + t
            orc.steps[:] = tick                        # batched envs share one clock on the device
            obs, rew, d = orc.step(action[k], [wl.spawn_roads_for_tick(entry, tick, period=period)], archetypes=archetypes)
            obs, rew, done = obs[0], rew[0], bool(d[0])
            total_obs[:r] += obs[:r]
            total_obs[r:2 * r] = obs[r:2 * r]
            multiplier = 2 * obs[-2 * I:-I] - 1
            total_obs[-I:] = obs[-I:] / 100 * multiplier
            total_reward = total_reward + rew
            if done:
                break
        if remi:
            total_reward = orc.remi_reward()[0].copy()
        aobs[k], arew[k], adone[k] = total_obs, total_reward, done
    return aobs, arew, adone


@pytest.mark.parametrize("path", ["resident", "pairs"])
def test_against_the_oracle(monkeypatch, path):
    """The wrappers emulated tick by tick on single-env oracles, orc.reset(episode_phases) wherever the model says an
    episode ended: aobs / areward / adone per decision, the cars after every decision, bit for bit."""
    force_path(monkeypatch, path)
    sc = SCENARIOS["limit"]
    E, T, cap = GRID["E"], GRID["T"], sc["C"]
    eng = make_engine(cap)
    orcs = [OracleEnv(GRID["m"], GRID["n"], GRID["L"], cap, eng.dest, eng.phases, eng.nexts) for _ in range(E)]
    ph = first_phases(E, eng.I)
    eng.reset(ph)
    for k, o in enumerate(orcs):
        o.reset(ph[k])
    eng.set_spawns(period=sc["period"])
    eng.set_episodes(max_decisions=sc["M"], seed=SEED)
    model = EpisodeModel(E, eng.I, sc["M"])
    ends = np.zeros(E, int)
    truncs = 0
    for s in range(sc["K"]):
        act = actions_for(np.arange(E), eng.I, s)
        eng.set_actions(act)
        tick0 = eng.tick
        aobs, arew, adone = eng.agent_step(T, remi=True)
        eo, er, ed = emulate_agent_step(orcs, tick0, act, eng.entrypoints, T, True, sc["period"])
        assert np.array_equal(adone.cpu().numpy(), ed), s
        assert np.array_equal(aobs.cpu().numpy(), eo), s
        assert np.array_equal(arew.cpu().numpy(), er), s
        ld, lc = eng.leading.cpu().numpy(), eng.lastcar.cpu().numpy()
        x, v, _ = eng.planes_numpy()
        for k, o in enumerate(orcs):            # (the terminal state of an env that ended: it restarts with the next decision)
            assert np.array_equal(ld[k], o.leading[0]) and np.array_equal(lc[k], o.lastcar[0]), (s, k)
            live = live_mask(ld[k], lc[k], cap)
            assert np.array_equal(x[k][live].view(np.int32), o.x[0][live].view(np.int32)), (s, k)
            assert np.array_equal(v[k][live].view(np.int32), o.v[0][live].view(np.int32)), (s, k)
        end = model.decision(er, ed)
        assert_accounting(eng, model, s)
        ends += end
        truncs += int(model.truncated.sum())
        for k in np.nonzero(end)[0]:
            orcs[k].reset(devrng.episode_phases(SEED, [k], model.ep_index[k], eng.I)[0])
    assert (ends >= 2).any() and truncs > 0 and int(ends.sum()) > truncs


def test_sharding(step_path):
    """Two handles with env_id_offset 0 and E/2 equal the halves of one handle of E envs."""
    sc, E = SCENARIOS["limit"], GRID["E"]
    h = E // 2
    outs = []
    for n_envs, off in ((E, 0), (h, 0), (h, h)):
        eng = make_engine(sc["C"], n_envs, off)
        ids = np.arange(n_envs) + off
        eng.reset(first_phases(E, eng.I)[ids])
        eng.set_spawns(period=sc["period"])
        eng.set_episodes(max_decisions=sc["M"], seed=SEED)
        per = []
        for s in range(sc["K"]):
            eng.set_actions(actions_for(ids, eng.I, s))
            per.append(host(eng.agent_step(GRID["T"])) + host(getattr(eng, nm) for nm in EP_NAMES))
        outs.append((per, eng.leading.cpu().numpy(), eng.obs.cpu().numpy()))
    whole, lo, hi = outs
    for s in range(sc["K"]):
        for j in range(len(whole[0][s])):
            assert np.array_equal(whole[0][s][j][:h], lo[0][s][j]), (s, j)
            assert np.array_equal(whole[0][s][j][h:], hi[0][s][j]), (s, j)
    for j in (1, 2):
        assert np.array_equal(whole[j][:h], lo[j]) and np.array_equal(whole[j][h:], hi[j])
    assert whole[0][-1][8].max() >= 2                            # (ep_index: somebody restarted twice)


def test_explicit_resets_abandon_the_episode(step_path):
    """reset_envs from outside clears the accumulators and the restart mark of those envs only; ep_index unmoved."""
    sc, E = SCENARIOS["limit"], GRID["E"]
    a, b = make_engine(sc["C"]), make_engine(sc["C"])
    ph = first_phases(E, a.I)
    for eng in (a, b):
        eng.reset(ph)
        eng.set_spawns(period=sc["period"])
    a.set_episodes(max_decisions=3, seed=SEED)
    model = EpisodeModel(E, a.I, 3)
    ids = np.arange(E)
    own = np.ascontiguousarray(1 - ph)
    for s in range(9):
        act = actions_for(ids, a.I, s)
        a.set_actions(act)
        b.set_actions(act)
        oa = host(a.agent_step(GRID["T"]))
        ob = host(b.agent_step(GRID["T"]))
        for u, v in zip(oa, ob):
            assert np.array_equal(u.view(np.uint8), v.view(np.uint8)), s
        end = model.decision(ob[1], ob[2])
        assert_accounting(a, model, s)
        if s in (2, 4, 5):
            # s = 2: every env has just hit the limit and is marked - envs 0..3 are reset from outside with phases of
            # the caller's own, which must stay (no second restart on the device); the others restart on the device.
            # s = 4: envs 0..3 are abandoned in the middle of an episode; s = 5: the others have just ended again
            mask = ids < 4
            idx_before = a.ep_index.cpu().numpy().copy()
            a.reset_envs(mask, own)
            model.abandon(mask)
            assert_accounting(a, model, s)
            assert np.array_equal(a.ep_index.cpu().numpy(), idx_before)
            phb = devrng.episode_phases(SEED, ids, model.ep_index, a.I)
            phb[mask] = own[mask]
            b.reset_envs(end | mask, phb)
        else:
            b.reset_envs(end, devrng.episode_phases(SEED, ids, model.ep_index, a.I))
        if s == 2:
            assert end.all() and model.truncated.all()
    # a full reset abandons everybody's episode
    a.agent_step(GRID["T"])
    idx = a.ep_index.cpu().numpy().copy()
    a.reset(ph)
    assert not a.ep_return.cpu().numpy().any() and not a.ep_len.cpu().numpy().any()
    assert np.array_equal(a.ep_index.cpu().numpy(), idx)


# Launches tfx_debug_fail_after counts in ONE 10-tick decision of 8 envs of the 3x3 grid (capacity 12, periodic
# arrivals, a held action buffer, remi) with episodes off and TFX_GRAPH=0, on the forced paths of force_path():
# counted on the parent commit 56367d8 with count_launches below
PARENT_LAUNCHES = {"resident": 1, "pertick": 20, "pairs": 22, "pairs_seg_launches": 30, "ring": 20}


def count_launches(eng, n_ticks):
    """How many launches of one decision the injection counts: the largest n for which the n-th launch still exists."""
    n = 0
    ph = first_phases(eng.E, eng.I)
    while n < 400:
        eng.reset(ph)
        nat.check(eng.lib.tfx_debug_fail_after(eng.h, n + 1))
        try:
            eng.agent_step(n_ticks)
        except nat.TfxError as exc:
            assert "injected" in str(exc)
            torch.cuda.synchronize()
            n += 1
            continue
        break
    nat.check(eng.lib.tfx_debug_fail_after(eng.h, 0))
    torch.cuda.synchronize()
    return n


@pytest.mark.parametrize("path", sorted(PARENT_LAUNCHES))
def test_off_means_off_launch_for_launch(monkeypatch, path):
    force_path(monkeypatch, path)
    monkeypatch.setenv("TFX_GRAPH", "0")          # (replays of a captured graph bypass the injection)
    sc = SCENARIOS["limit"]
    eng = make_engine(sc["C"])
    eng.set_spawns(period=sc["period"])
    eng.set_actions(actions_for(np.arange(eng.E), eng.I, 0))
    off = count_launches(eng, GRID["T"])
    print("launches per decision, %s: %d with episodes off" % (path, off))
    assert off == PARENT_LAUNCHES[path]
    eng.set_episodes(max_decisions=4, seed=SEED)
    on = count_launches(eng, GRID["T"])
    print("launches per decision, %s: %d with episodes on" % (path, on))
    assert on == off + 1                           # the masked restart, counted like any other launch
    eng.set_episodes(enabled=False)
    assert count_launches(eng, GRID["T"]) == off


@pytest.mark.parametrize("path", ["resident", "pertick", "pairs"])
def test_switching_episodes_recaptures_the_graph(monkeypatch, path):
    """set_episodes on / off / on with another limit and seed on an existing handle between decisions: the captured
    graph is never a stale one - results equal the eager run (TFX_GRAPH=0)."""
    sc, E = SCENARIOS["limit"], GRID["E"]
    outs = []
    for graph in ("1", "0"):
        force_path(monkeypatch, path)
        monkeypatch.setenv("TFX_GRAPH", graph)
        eng = make_engine(sc["C"])
        eng.reset(first_phases(E, eng.I))
        eng.set_spawns(period=sc["period"])
        res = []
        for s in range(16):
            if s == 3:
                eng.set_episodes(max_decisions=2, seed=SEED)
            if s == 8:
                eng.set_episodes(enabled=False)
            if s == 11:
                eng.set_episodes(max_decisions=3, seed=SEED + 1)
            eng.set_actions(actions_for(np.arange(E), eng.I, s))
            res.append(host(eng.agent_step(GRID["T"])))
            if eng.ep_len is not None:
                res[-1] += host((eng.ep_index, eng.ep_len, eng.final_return, eng.obs))
        outs.append((res, eng.leading.cpu().numpy(), eng.obs.cpu().numpy()))
    for s, (u, v) in enumerate(zip(outs[0][0], outs[1][0])):
        assert len(u) == len(v)
        for p, q in zip(u, v):
            assert np.array_equal(p, q), s
    assert np.array_equal(outs[0][1], outs[1][1]) and np.array_equal(outs[0][2], outs[1][2])
    assert outs[0][0][7][3].max() >= 2 and outs[0][0][-1][3].max() >= 1       # (ep_index moved in both enabled spans)


def test_vec_env_autoreset(step_path):
    """TrafficVecEnv(autoreset=True): the attributes, the same three tensors, reset_done() refused."""
    from gym_traffic.envs.vec_env import TrafficVecEnv
    E = 6
    venv = TrafficVecEnv(E, 3, 3, 150.0, capacity=12, spawn='periodic', spawn_period=6, seed=SEED, autoreset=True, episode_len=4)
    venv.reset()
    model = EpisodeModel(E, venv.engine.I, 4)
    for s in range(9):
        out = venv.agent_step(torch.as_tensor(actions_for(np.arange(E), venv.engine.I, s)).to(venv.engine.device), n_ticks=10)
        assert len(out) == 3
        model.decision(out[1].cpu().numpy(), out[2].cpu().numpy())
        assert np.array_equal(venv.truncated.cpu().numpy(), model.truncated)
        assert np.array_equal(venv.episode_return.cpu().numpy(), model.ep_return)
        assert np.array_equal(venv.episode_length.cpu().numpy(), model.ep_len)
        assert np.array_equal(venv.final_return.cpu().numpy(), model.final_return)
        assert np.array_equal(venv.final_length.cpu().numpy(), model.final_len)
    assert model.ep_index.min() >= 2
    with pytest.raises(RuntimeError, match="autoreset"):
        venv.reset_done()
    plain = TrafficVecEnv(2, 3, 3, 150.0, capacity=12, spawn='periodic')
    plain.reset()
    plain.agent_step(cycle_period=5)
    plain.reset_done()
    assert plain.engine.ep_len is None


def split_ticks(eng):
    t = ctypes.c_int64()
    fn = eng.lib.tfx_split_ticks
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64)]
    nat.check(fn(eng.h, ctypes.byref(t)))
    return int(t.value)


def test_fullsize_split_path(monkeypatch):
    """cfg2's shape x 4096 envs (the split path: two halves of the env range on two streams), episode_len 3, six
    decisions: equivalence with the host loop - outputs and road words of every env, the cars of a sample of envs that
    includes env 0, the two envs at the split point and the last env; accounting against the model for every env."""
    for k in ("TFX_RESIDENT", "TFX_PAIRS", "TFX_TAIL", "TFX_SPLIT", "TFX_TT_SEG", "TFX_TT_SEGS", "TFX_GRAPH", "TFX_LAYOUT",
              "TFX_RES_EPB"):
        monkeypatch.delenv(k, raising=False)
    E, M, K = 4096, 3, 6
    sample = np.array([0, 1, 777, 2047, 2048, 3000, 4095])
    a = wl.setup_engine("cfg2", envs=E)
    b = wl.setup_engine("cfg2", envs=E)
    I = a.I
    a.set_episodes(max_decisions=M, seed=SEED)
    model = EpisodeModel(E, I, M)
    ids = np.arange(E)
    split0 = split_ticks(a)
    for s in range(K):
        oa = host(a.agent_step(10))
        ob = host(b.agent_step(10))
        for u, v, name in zip(oa, ob, ("aobs", "areward", "adone")):
            assert np.array_equal(u.view(np.uint8), v.view(np.uint8)), (s, name)
        end = model.decision(ob[1], ob[2])
        assert_accounting(a, model, s)
        if s + 1 < K:
            b.reset_envs(end, devrng.episode_phases(SEED, ids, model.ep_index, I))
    assert model.ep_index.min() >= 1 and model.truncated.any()
    assert split_ticks(a) - split0 == 10 * K                      # every decision ran split
    la, ca = a.leading.cpu().numpy(), a.lastcar.cpu().numpy()
    assert np.array_equal(la, b.leading.cpu().numpy()) and np.array_equal(ca, b.lastcar.cpu().numpy())
    assert np.array_equal(a.obs.cpu().numpy(), b.obs.cpu().numpy())
    assert np.array_equal(a.waiting.cpu().numpy(), b.waiting.cpu().numpy())
    xa, xb = a.xv[sample].cpu().numpy(), b.xv[sample].cpu().numpy()
    n_cars = 0
    for j, k in enumerate(sample):
        live = live_mask(la[k], ca[k], a.C)
        n_cars += int(live.sum())
        assert np.array_equal(xa[j][live].view(np.int32), xb[j][live].view(np.int32)), k
    assert n_cars > 1000
