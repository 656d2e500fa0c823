"""Demand profiles on the device (tfx_set_demand / tfx_demand_counts, rule 4 of include/tfx.h; k_demand,
csrc/tfx_demand.hpp).  Two references, both exact (np.array_equal, bit for bit):
  * tfx_demand_counts against devrng.demand_counts, the NumPy statement of the rule (tests/test_demand_host.py holds that
    to a line-by-line Python one);
  * an engine with the demand set against an engine with spawn 'none' that is fed the mirrored counts as a per-tick count
    buffer for the same ticks - on every step path, for plain calls, decisions, episodes, clones and warm restarts."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_gpu_fused import engine_with
from test_gpu_clone import assert_env_equal, snapshot
from test_gpu_episodes import EpisodeModel, first_phases, force_path, host
from test_demand_host import AGENT, BAD_ARGS, MASK, agent_actions, agent_scenario_on_the_oracle, agent_weights

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from gym_traffic import _native as nat  # noqa: E402
from gym_traffic import devrng  # noqa: E402
from gym_traffic.core import TfxEngine  # noqa: E402

# 2x2 grid with the west side closed: 6 entry roads (no power of two); 5 envs: ragged against four wavefronts per workgroup
GRID = dict(m=2, n=2, length=120.0, capacity=14, rate=0.5, entry_spec=1)
E, OFF, SEED = 5, 40, (0xABCD << 32) | 77
# K = 2 profiles, S = 3 segments of 2 ticks (period 6).  Profile 0 has a segment of mean 70 (n_cdf 137: lanes take a second
# round of cars, a Philox block is shared by four cars) and one of mean 0.
MEANS = [[0.5, 70.0, 0.0], [2.0, 1.0, 9.0]]
DEMAND = dict(means=MEANS, seg_ticks=2, tick_offset=3)
PROFILE = [0, 1, -1, 2, 1]            # -1 and K: no cars
SPLIT = {"TFX_RESIDENT": "0", "TFX_PAIRS": "2", "TFX_TAIL": "2", "TFX_SPLIT": "2"}      # two halves of the envs on two streams
PATHS = {"resident": {"TFX_RESIDENT": "1"}, "pairs": {"TFX_RESIDENT": "0"}, "pertick": {"TFX_RESIDENT": "0", "TFX_PAIRS": "0"},
         "pairs_split": SPLIT}


def weights(n_entry, K=2, S=3):
    return np.random.RandomState(0).rand(K, S, n_entry) + 0.05


def demand_engine(env=None, n_envs=E, off=OFF, profile=PROFILE, seed=SEED, demand=None, **grid):
    cfg = dict(GRID, **grid)
    eng = engine_with(env or {}, n_envs, env_id_offset=off, **cfg)
    dm = dict(DEMAND if demand is None else demand)
    dm.setdefault("weights", weights(eng.n_entry, *np.shape(dm["means"])))
    prof = None if profile is None else torch.as_tensor(np.asarray(profile, np.int32)).to(eng.device)
    eng.set_demand(seed=seed, profile_of_env=prof, **dm)
    return eng


def plain_engine(env=None, n_envs=E, off=OFF, **grid):
    return engine_with(env or {}, n_envs, env_id_offset=off, **dict(GRID, **grid))


def mirror(eng, tick0, n, ids=None, profile=None):
    """devrng.demand_counts for the engine's demand as it stands: rows of clock ticks tick0 .. tick0 + n - 1"""
    ids = np.arange(eng.E) + eng.cfg.env_id_offset if ids is None else ids
    prof = eng.demand_profile.cpu().numpy() if profile is None else profile
    return devrng.demand_counts(eng.demand["seed"], ids, np.arange(tick0, tick0 + n), eng.demand_tables, prof,
                                seg_ticks=eng.demand["seg_ticks"], tick_offset=eng.demand["tick_offset"])


def assert_same(a, b, where, envs=None):
    sa, sb = snapshot(a), snapshot(b)
    for e in (range(a.E) if envs is None else envs):
        assert_env_equal(sa, e, sb, e, where)


def cars(eng):
    return int(eng.cars_on_roads_flat().sum().item())


# ---- 1. the kernel against the rule ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [None, "1"])
def test_counts_equal_the_rule(cap):
    """tick0 = 3: 7 ticks cross two segment boundaries and the period wrap (period 6).  tick0 = -9 with tick_offset 3: a
    negative t + tick_offset (floor modulo).  TFX_GRID_CAP=1: one workgroup - every wavefront strides over nine items."""
    eng = demand_engine({} if cap is None else {"TFX_GRID_CAP": cap})
    assert eng.n_entry == 6 and eng.demand_tables.count_cdf.shape[2] > 65
    # (2^31 - 2, 4): the int32 clock wraps inside the call, and the mirror wraps with it
    for tick0, n in ((3, 7), (-9, 7), (2 ** 31 - 4, 3), (2 ** 31 - 2, 4), (0, 1), (5, 0)):
        got = eng.demand_counts(tick0, n).cpu().numpy()
        want = mirror(eng, tick0, n)
        assert got.dtype == np.int32 and got.shape == (n, E, 6)
        assert np.array_equal(got, want), (tick0, n, np.argwhere(got != want)[:5])
    want = mirror(eng, 3, 7)
    assert (want[:, 0].sum(axis=1) > 64).any()                 # the mean-70 segment: a second round of lanes
    assert (want[:, 0].sum(axis=1) == 0).any()                 # the mean-0 segment
    assert not want[:, 2].any() and not want[:, 3].any()       # profiles -1 and K
    assert want[:, 1].any() and want[:, 4].any() and not np.array_equal(want[:, 1], want[:, 4])
    segs = devrng.demand_segment(np.arange(3, 10), 3, 2, 3)
    assert set(segs.tolist()) == {0, 1, 2} and (np.diff(segs) < 0).any()      # the wrap
    assert (np.arange(-9, -2) + 3 < 0).sum() == 6            # (t + tick_offset = -6 .. 0)
    # NULL profile_of_env is profile 0 everywhere; the stream id is env + env_id_offset
    eng0 = demand_engine({} if cap is None else {"TFX_GRID_CAP": cap}, profile=None, off=7)
    dm = nat.TfxDemand()
    t = eng0.demand_tables
    dm.n_profiles, dm.n_segments, dm.seg_ticks, dm.tick_offset, dm.n_cdf = 2, 3, 2, 3, t.count_cdf.shape[2]
    dm.count_cdf, dm.road_cdf = t.count_cdf.ctypes.data_as(C.c_void_p), t.road_cdf.ctypes.data_as(C.c_void_p)
    dm.profile_of_env, dm.seed = None, SEED
    nat.check(eng0.lib.tfx_set_demand(eng0.h, C.byref(dm)))
    got = eng0.demand_counts(3, 7).cpu().numpy()
    assert np.array_equal(got, mirror(eng0, 3, 7, profile=np.zeros(E, np.int64)))
    assert not np.array_equal(got[:, 0], mirror(eng, 3, 7, profile=np.zeros(E, np.int64))[:, 0])      # (ids 7.. against 40..)


def test_counts_many_entry_roads_and_several_workgroups():
    """5x5 grid: 20 entry roads; 40 ticks x 3 envs = 120 items over 30 workgroups; one profile, one segment"""
    eng = demand_engine(n_envs=3, profile=[0, 0, 0], m=5, n=5, entry_spec=0, demand=dict(means=[[6.0]], seg_ticks=1, tick_offset=0))
    assert eng.n_entry == 20
    got = eng.demand_counts(100, 40).cpu().numpy()
    assert np.array_equal(got, mirror(eng, 100, 40)) and (got.sum(axis=(0, 1)) > 0).all()


# ---- 2. errors ---------------------------------------------------------------------------------------------------------------------
def test_errors_are_codes_and_a_refused_call_changes_nothing():
    lib = nat.lib()
    eng = demand_engine()
    before = eng.demand_counts(3, 7).cpu().numpy()
    dm, cases, keep = BAD_ARGS(nat, eng.n_entry)
    bad_rc = np.full((1, 2, eng.n_entry), MASK, np.uint32)
    bad_rc[0, 1, :3] = [1, 9, 5]
    short = np.full((1, 2, eng.n_entry), 7, np.uint32)
    cases = cases + [(dm(rc=bad_rc), b"road_cdf row (0, 1) decreases at 2"), (dm(rc=short), b"road_cdf row (0, 0) does not end in 0xFFFFFFFF")]
    for d, msg in cases:
        assert lib.tfx_set_demand(eng.h, None if d is None else C.byref(d)) == -1, msg
        assert msg in lib.tfx_last_error(), (msg, lib.tfx_last_error())
    assert lib.tfx_set_demand(None, C.byref(dm())) == -1 and b"null handle" in lib.tfx_last_error()
    # before tfx_bind_buffers
    h = C.c_void_p()
    nat.check(lib.tfx_create(C.byref(eng.cfg), C.byref(h)))
    assert lib.tfx_set_demand(h, C.byref(dm())) == -2 and b"tfx_bind_buffers" in lib.tfx_last_error()
    word = torch.zeros((7, E, eng.n_entry), dtype=torch.int32, device=eng.device)
    assert lib.tfx_demand_counts(h, 0, 7, C.c_void_p(word.data_ptr()), None) == -2
    nat.check(lib.tfx_destroy(h))
    # a heterogeneous handle
    rows = np.array([[11.11, 4.0, 3.0, 4.0, 13.89, 6.0, 2.0, 1.0], [9.0, 5.0, 2.0, 3.0, 11.0, 5.0, 1.5, 2.0]], np.float32)
    het = TfxEngine(2, 2, 120.0, 14, n_envs=2, entry_spec=1, archetypes=rows, planes=3, layout="transposed")
    assert lib.tfx_set_demand(het.h, C.byref(dm())) == -1 and b"heterogeneous" in lib.tfx_last_error()
    # nothing changed: the demand set before the refusals still makes the same rows, and steps
    assert np.array_equal(eng.demand_counts(3, 7).cpu().numpy(), before)
    eng.reset(np.zeros((E, eng.I), np.int32))
    eng.set_actions(cycle_period=5)
    eng.step(4)
    assert cars(eng) > 0
    # no demand: TFX_ESTATE; another spawn rule replaces it
    plain = plain_engine()
    with pytest.raises(nat.TfxError, match="tfx error -2"):
        plain.demand_counts(0, 1)
    eng.set_spawns(period=4)
    with pytest.raises(nat.TfxError, match="tfx error -2"):
        eng.demand_counts(0, 1)
    assert eng.demand is None and eng.demand_profile is None and eng.demand_tables is None
    n = cars(eng)
    eng.step(8)
    assert cars(eng) != n
    with pytest.raises(nat.TfxError, match="n_ticks = 65"):          # a decision's rows are drawn up front: 64 at most
        e2 = demand_engine()
        e2.reset(np.zeros((E, e2.I), np.int32))
        e2.agent_step(65)
    assert keep


# ---- 3. plain calls against mirrored counts --------------------------------------------------------------------------------------
def run_steps(path, calls, **grid):
    n_envs = grid.pop("n_envs", E)
    profile = grid.pop("profile", PROFILE)
    a = demand_engine(PATHS[path], n_envs=n_envs, profile=profile, demand=grid.pop("demand", None), **grid)
    b = plain_engine(PATHS[path], n_envs=n_envs, **grid)
    ph = first_phases(n_envs, a.I)
    rng = np.random.RandomState(9)
    for eng in (a, b):
        eng.reset(ph)
    tick = 0
    for n in calls:
        act = rng.randint(2, size=(n_envs, a.I)).astype(np.int32)
        a.set_actions(act)
        b.set_actions(act)
        b.set_spawns(counts=mirror(a, tick, n), per_tick=True)
        a.step(n)
        b.step(n)
        tick += n
        assert_same(a, b, (path, tick))
    assert a.tick == tick and cars(a) > 10
    return a, b


@pytest.mark.parametrize("path", list(PATHS))
def test_step_equals_mirrored_counts(path):
    """step(7): k_res / three pairs and an odd tick / tick by tick; then calls that start on other clock values"""
    a, b = run_steps(path, [7, 7, 1, 4])
    fused, capable = a.fused_ticks()
    assert (fused == 19) == (path == "resident") and capable == (path == "resident")
    pairs = path.startswith("pairs")
    assert (a.pair_ticks() == 6 + 6 + 4) == pairs and (a.pair_ticks() == 0) == (not pairs)
    assert (a.split_ticks() == 7 + 7 + 4) == (path == "pairs_split") and (a.split_ticks() == 0) == (path != "pairs_split")
    dt = a.done_tick.cpu().numpy()
    assert dt[0] > 0 and not dt[2] and not dt[3]                     # the env with the mean-70 segment overflows; no cars, no overflow


@pytest.mark.parametrize("path", ["pairs", "pertick"])
def test_step_two_tiles(path):
    """5x5 grid x 1 env: 120 roads, two tiles of 64"""
    a, _ = run_steps(path, [7, 6], n_envs=1, profile=[1], m=5, n=5, entry_spec=0)
    assert a.R == 120 and a.n_entry == 20


@pytest.mark.parametrize("path", ["pairs", "pertick"])
def test_move_cars_draws_the_row_of_the_clocks_tick(path):
    """tfx_move_cars / tfx_advance_finished_cars, tick by tick: the demand handle draws one row for the tick the clock
    stands at; the other engine holds that tick's mirrored counts"""
    a, b = demand_engine(PATHS[path]), plain_engine(PATHS[path])
    ph = first_phases(E, a.I)
    rng = np.random.RandomState(3)
    for eng in (a, b):
        eng.reset(ph)
    for t in range(9):
        act = rng.randint(2, size=(E, a.I)).astype(np.int32)
        a.set_actions(act)
        b.set_actions(act)
        b.set_spawns(counts=mirror(a, t, 1)[0])
        for eng in (a, b):
            eng.move_cars()
            eng.advance_finished_cars()
        assert_same(a, b, (path, t))
    assert a.tick == 9 and cars(a) > 10 and a.demand is not None


@pytest.mark.parametrize("path", ["resident", "pairs", "pairs_split"])
def test_step_longer_than_the_count_buffer(path):
    """70 ticks: the handle's count buffer holds 64 rows, so the call is drawn in two chunks (split: the second chunk's
    rows are drawn behind the join of the first chunk's halves)"""
    a, _ = run_steps(path, [70, 3], demand=dict(means=[[0.3, 0.8, 0.0], [0.6, 0.2, 1.0]], seg_ticks=2, tick_offset=3))
    assert a.tick == 73


# ---- 4. decisions -----------------------------------------------------------------------------------------------------------------
AGENT_PATHS = {"resident": {"TFX_RESIDENT": "1"}, "pairs": {"TFX_RESIDENT": "0"},
               "pairs_tail": {"TFX_RESIDENT": "0", "TFX_PAIRS": "2", "TFX_TAIL": "2", "TFX_SPLIT": "0"},
               "pairs_split": SPLIT, "pertick": {"TFX_RESIDENT": "0", "TFX_PAIRS": "0"}}


def agent_engines(env):
    sc = AGENT
    grid = dict(m=sc["m"], n=sc["n"], length=sc["length"], capacity=sc["capacity"], rate=sc["rate"], entry_spec=sc["entry_spec"])
    a = engine_with(env, sc["E"], env_id_offset=sc["off"], **grid)
    b = engine_with(env, sc["E"], env_id_offset=sc["off"], **grid)
    prof = torch.as_tensor(np.asarray(sc["profiles"], np.int32)).to(a.device)
    a.set_demand(sc["means"], agent_weights(a.n_entry), seg_ticks=sc["seg_ticks"], tick_offset=sc["tick_offset"], seed=sc["seed"],
                 profile_of_env=prof)
    return a, b


_oracle = {}


def oracle_scenario():
    if not _oracle:
        _oracle["stopped"], _oracle["counts"] = agent_scenario_on_the_oracle()
    return _oracle["stopped"], _oracle["counts"]


@pytest.mark.parametrize("graph", ["1", "0"])
@pytest.mark.parametrize("path", list(AGENT_PATHS))
def test_agent_step_equals_mirrored_counts(path, graph):
    """10-tick decisions at capacity 6 under a demand that overflows some envs, not all, part-way through the second and
    the third decision - the replays of the captured graph (tests/test_demand_host.py picked the seed on the oracle and
    asserts as much there).  The rows of a decision are drawn up front; an env that stops does not consume the rest."""
    sc = AGENT
    T = sc["T"]
    stopped, counts = oracle_scenario()
    a, b = agent_engines(dict(AGENT_PATHS[path], TFX_GRAPH=graph))
    assert np.array_equal(mirror(a, 0, sc["decisions"] * T), counts)
    for eng in (a, b):
        eng.reset(np.zeros((sc["E"], eng.I), np.int32))
    for s in range(sc["decisions"]):
        act = agent_actions(sc["E"], a.I, s)
        a.set_actions(act)
        b.set_actions(act)
        b.set_spawns(counts=counts[s * T:(s + 1) * T], per_tick=True)
        oa, ob = host(a.agent_step(T)), host(b.agent_step(T))
        for u, v, name in zip(oa, ob, ("aobs", "areward", "adone")):
            assert np.array_equal(u.view(np.uint8), v.view(np.uint8)), (s, name)
        assert_same(a, b, (path, graph, s))
        # the oracle's overflow ticks: done_tick holds (clock tick of the overflow) + 1
        dt = a.done_tick.cpu().numpy()
        want = np.where(stopped[s] >= 0, s * T + stopped[s] + 1, 0)
        assert np.array_equal(np.where(dt > s * T, dt, 0), want), (s, dt, want)
        assert np.array_equal(oa[2] != 0, stopped[s] >= 0)
        if s >= 1:
            mid = (stopped[s] >= 0) & (stopped[s] < T - 1)
            assert mid.any() and (stopped[s] < 0).any()
    assert (a.fused_ticks()[0] > 0) == (path == "resident")
    assert (a.split_ticks() == sc["decisions"] * T) == (path == "pairs_split")      # (the rows are drawn ahead of the fork)


@pytest.mark.parametrize("path", ["resident", "pairs"])
def test_autoreset_equals_mirrored_counts(monkeypatch, path):
    """episode_len = 3 over 8 decisions: the restarts do not touch the rule - it reads the clock, which runs on"""
    from gym_traffic.envs.vec_env import TrafficVecEnv
    force_path(monkeypatch, path)
    kw = dict(capacity=6, entry_spec=1, seed=5, env_id_offset=OFF, autoreset=True, episode_len=3)
    dm = dict(means=AGENT["means"], weights=None, seg_ticks=7, tick_offset=-3)      # (profile 1 overflows four-car roads)
    a = TrafficVecEnv(E, 2, 2, 120.0, spawn='demand', demand=dm, **kw)
    b = TrafficVecEnv(E, 2, 2, 120.0, spawn='none', **kw)
    a.demand_profile.copy_(torch.as_tensor(np.array([1, 0, 1, 0, 1], np.int32)))
    ph = first_phases(E, a.engine.I)
    a.reset(ph)
    b.reset(ph)
    model = EpisodeModel(E, a.engine.I, 3)
    ended = 0
    for s in range(8):
        act = torch.as_tensor(agent_actions(E, a.engine.I, s)).to(a.engine.device)
        b.engine.set_spawns(counts=mirror(a.engine, 10 * s, 10), per_tick=True)
        oa, ob = host(a.agent_step(act, n_ticks=10)), host(b.agent_step(act, n_ticks=10))
        for u, v in zip(oa, ob):
            assert np.array_equal(u.view(np.uint8), v.view(np.uint8)), s
        model.decision(ob[1], ob[2])
        assert np.array_equal(a.episode_length.cpu().numpy(), model.ep_len)
        assert np.array_equal(a.episode_index.cpu().numpy(), b.episode_index.cpu().numpy())
        assert_same(a.engine, b.engine, (path, s))
        ended += int(oa[2].sum())
    assert model.ep_index.min() >= 2 and ended > 0 and cars(a.engine) > 0


@pytest.mark.parametrize("path", ["resident", "pairs"])
def test_rewriting_the_profile_between_replayed_decisions(path):
    """demand_profile is read when the arrivals are drawn: rewritten between the second and the third decision - both
    replays of the captured graph - it changes the arrivals of exactly the rewritten envs, with no re-capture."""
    T = 10
    dm = dict(means=[[0.4, 1.0, 0.2], [1.6, 0.1, 0.9]], seg_ticks=2, tick_offset=3)
    a = demand_engine(dict(PATHS[path], TFX_GRAPH="1"), profile=[0, 0, 0, 0, 0], demand=dm)
    b = plain_engine(PATHS[path])
    for eng in (a, b):
        eng.reset(np.zeros((E, eng.I), np.int32))
    rewritten = [1, 3]
    for s in range(4):
        if s == 2:
            old = a.demand_counts(s * T, T).cpu().numpy()
            a.demand_profile[rewritten] = 1
            new = a.demand_counts(s * T, T).cpu().numpy()
            for e in range(E):
                assert np.array_equal(old[:, e], new[:, e]) == (e not in rewritten), e
        act = agent_actions(E, a.I, s)
        a.set_actions(act)
        b.set_actions(act)
        b.set_spawns(counts=mirror(a, s * T, T), per_tick=True)
        oa, ob = host(a.agent_step(T)), host(b.agent_step(T))
        for u, v in zip(oa, ob):
            assert np.array_equal(u.view(np.uint8), v.view(np.uint8)), s
        assert_same(a, b, (path, s))
    assert cars(a) > 10


# ---- 5. clones ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["resident", "pairs"])
def test_clone_with_its_stream_receives_its_sources_cars(path):
    dm = dict(means=[[0.4, 1.0, 0.2], [1.6, 0.1, 0.9]], seg_ticks=2, tick_offset=3)
    src = demand_engine(PATHS[path], profile=[0, 1, 0, 1, 1], demand=dm, capacity=10)
    dst = demand_engine(PATHS[path], off=100, profile=[0, 0, 0, 0, 0], demand=dm, capacity=10)
    idx = np.array([3, -1, 0, 1, -1], np.int32)
    rng = np.random.RandomState(4)

    def bind_actions():
        act = rng.randint(2, size=(E, src.I)).astype(np.int32)
        src.set_actions(act)
        dst.set_actions(act[np.where(idx >= 0, idx, np.arange(E))])      # a clone is held as its source is

    for eng in (src, dst):
        eng.reset(first_phases(E, eng.I))
    bind_actions()
    for eng in (src, dst):
        eng.step(9)                                   # (the rule reads the destination's clock: both stand at tick 9)
    dst.clone_envs(idx, source=src, streams=True)
    dst.demand_profile.copy_(torch.as_tensor(np.array([1, 0, 0, 1, 0], np.int32)))       # (the sources' profiles: the caller's)
    for n, kind in ((7, "step"), (10, "agent"), (4, "step")):
        bind_actions()
        for eng in (src, dst):
            eng.agent_step(n) if kind == "agent" else eng.step(n)
        ss, sd = snapshot(src), snapshot(dst)
        for e, s in enumerate(idx):
            if s >= 0:
                assert_env_equal(sd, e, ss, int(s), (path, kind, e))
    # the preview shows it: stream ids 43, 101, 40, 41, 104
    got = dst.demand_counts(30, 6).cpu().numpy()
    assert np.array_equal(got, mirror(dst, 30, 6, ids=np.array([43, 101, 40, 41, 104])))
    assert cars(dst) > 10 and not np.array_equal(got[:, 1], mirror(src, 30, 6)[:, 1])
    # without the flag a clone keeps its own stream
    dst.clone_envs(np.array([-1, 2, -1, -1, -1], np.int32), source=src, streams=False)
    assert np.array_equal(dst.demand_counts(30, 6).cpu().numpy(), got)


def test_clone_refusals():
    dm = dict(means=[[0.4, 1.0, 0.2], [1.6, 0.1, 0.9]], seg_ticks=2, tick_offset=3)
    src = demand_engine(demand=dm)
    idx = np.arange(E, dtype=np.int32)

    def refused(dst, word):
        dst.reset(np.zeros((E, dst.I), np.int32))
        with pytest.raises(nat.TfxError) as exc:
            dst.clone_envs(idx, source=src, streams=True)
        assert "tfx error -1:" in str(exc.value) and word in str(exc.value), str(exc.value)
        dst.clone_envs(idx, source=src, streams=False)          # (the same world: fine without the stream)

    src.reset(np.zeros((E, src.I), np.int32))
    refused(demand_engine(demand=dict(dm, means=[[0.4, 1.0, 0.2], [1.6, 0.1, 0.8]])), "demand tables")
    refused(demand_engine(demand=dict(dm, weights=weights(6) + 0.01)), "demand tables")
    refused(demand_engine(demand=dm, seed=SEED + 1), "demand seed")
    refused(demand_engine(demand=dict(dm, tick_offset=4)), "tick_offset")
    refused(demand_engine(demand=dict(dm, seg_ticks=3)), "demand sizes")
    poisson = plain_engine()
    poisson.set_poisson(0.5, seed=SEED)
    refused(poisson, "stream kind")
    regular = plain_engine()
    regular.set_regular(0.5, seed=SEED)
    refused(regular, "stream kind")
    refused(plain_engine(), "stream kind")
    src2 = poisson
    with pytest.raises(nat.TfxError, match="stream kind"):
        src.clone_envs(idx, source=src2, streams=True)


def make_venv(n_envs=E, **kw):
    from gym_traffic.envs.vec_env import TrafficVecEnv
    args = dict(capacity=10, entry_spec=1, seed=5, spawn='demand',
                demand=dict(means=[[0.3, 0.6], [0.9, 0.3]], weights=None, seg_ticks=7, tick_offset=-3))
    args.update(kw)
    return TrafficVecEnv(n_envs, 2, 2, 120.0, **args)


def test_vec_env_clone_carries_the_profile_and_snapshot_restores():
    venv = make_venv()
    assert venv.demand_profile.dtype == torch.int32 and tuple(venv.demand_profile.shape) == (E,) and not venv.demand_profile.any()
    venv.demand_profile.copy_(torch.as_tensor(np.array([1, 0, 1, 0, 1], np.int32)))
    venv.reset(np.zeros((E, venv.engine.I), np.int32))

    def held(s):                                      # (every env under the same action: a clone is held as its source is)
        return torch.full((E, venv.engine.I), s & 1, dtype=torch.int32, device=venv.engine.device)

    venv.step(held(1), n_ticks=12)
    # in place: env 1 <- env 0, env 4 <- env 3; env 2 asks for env 1, which is itself overwritten: left alone (clone_plan)
    venv.clone_envs(torch.as_tensor(np.array([-1, 0, 1, -1, 3], np.int32)))
    assert venv.demand_profile.cpu().numpy().tolist() == [1, 1, 1, 0, 0]
    assert venv.engine.clone_skipped() == 1
    snap = venv.snapshot()
    assert np.array_equal(snap.demand_profile.cpu().numpy(), venv.demand_profile.cpu().numpy())
    assert snap.demand_profile.data_ptr() != venv.demand_profile.data_ptr()
    for s in range(3):
        venv.agent_step(held(s), n_ticks=10)
        st = snapshot(venv.engine)
        assert_env_equal(st, 1, st, 0, ("in place", s))
        assert_env_equal(st, 4, st, 3, ("in place", s))
    assert cars(venv.engine) > 10
    # the snapshot stands at the clock it was made at... its own: 0.  Restored, the env continues from the snapshot's state
    after = snapshot(venv.engine)
    venv.restore(snap)
    back = snapshot(venv.engine)
    assert not np.array_equal(after[0]["lastcar"], back[0]["lastcar"])
    assert np.array_equal(back[0]["lastcar"], snapshot(snap.engine)[0]["lastcar"])
    # other source, other size: the profile is gathered through the index tensor; out-of-range indices are left alone
    small = make_venv(3)
    small.demand_profile.copy_(torch.as_tensor(np.array([0, 1, 0], np.int32)))
    small.reset()
    venv.clone_envs(torch.as_tensor(np.array([1, -1, 7, 2, 1], np.int32)), source=small)
    assert venv.demand_profile.cpu().numpy().tolist() == [1, 1, 1, 0, 1]
    with pytest.raises(ValueError):
        venv.clone_envs(torch.arange(E, dtype=torch.int32), source=make_venv(spawn='none', demand=None))


def test_vec_env_warm_pool_equals_the_manual_loop(monkeypatch):
    """tests/test_gpu_warm_pool.py's manual loop with demand envs: restarted envs keep their own stream ids, and the rule
    has no position to carry - A (restarts on the device from the pool) equals B (clone_envs by hand), both 'demand'"""
    force_path(monkeypatch, "pairs")
    M, n_pool, seed = 4, 3, 5
    a = make_venv(autoreset=True, episode_len=M)
    b = make_venv()
    pool = a.make_warm_pool(n_pool, 3)
    assert pool.spawn == 'demand' and pool.env_id_offset == a.POOL_ENV_ID_OFFSET and cars(pool.engine) > 0
    a.set_warm_pool(pool)
    for v in (a, b):
        v.demand_profile.copy_(torch.as_tensor(np.array([1, 0, 1, 0, 1], np.int32)))
    ph = first_phases(E, a.engine.I)
    a.reset(ph)
    b.reset(ph)
    model = EpisodeModel(E, a.engine.I, M)
    ids = np.arange(E)
    for s in range(10):
        act = torch.as_tensor(agent_actions(E, a.engine.I, s)).to(a.engine.device)
        oa, ob = host(a.agent_step(act, n_ticks=10)), host(b.agent_step(act, n_ticks=10))
        for u, v in zip(oa, ob):
            assert np.array_equal(u.view(np.uint8), v.view(np.uint8)), s
        end = model.decision(ob[1], ob[2]).astype(bool)
        assert np.array_equal(a.episode_length.cpu().numpy(), model.ep_len)
        if s + 1 < 10:
            slots = devrng.episode_pool_slots(seed, ids, model.ep_index, n_pool)
            b.clone_envs(np.where(end, slots, -1).astype(np.int32), source=pool, streams=False, episodes=False)
    assert model.ep_index.min() >= 2
    assert_same(a.engine, b.engine, "final")
    assert cars(a.engine) > 10 and a.demand_profile.cpu().numpy().tolist() == [1, 0, 1, 0, 1]


# ---- 6. the demo --------------------------------------------------------------------------------------------------------------------
def test_demand_demo_runs():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "demand_demo.py"), "--envs", "8", "--m", "3", "--n", "3",
                          "--length", "120", "--capacity", "14", "--decisions", "8", "--ticks", "6", "--seg-decisions", "2"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    print(out.stdout)
    rets = {}
    for line in out.stdout.splitlines():
        if line.startswith("return "):
            rets[line.split()[1]] = float(line.split()[-1])
    assert set(rets) == {"cycle", "greedy"} and all(np.isfinite(v) for v in rets.values())
    seg = [l for l in out.stdout.splitlines() if l.startswith("segment ")]
    assert len(seg) == 2 and all(int(l.split("cars")[1].split()[0]) > 0 for l in seg)
