"""Mixed cars under demand profiles (tfx_set_demand_mixed / tfx_demand_rows, rule 5 of include/tfx.h; k_demand<true>,
csrc/tfx_demand.hpp).  Two references, both exact (np.array_equal, bit for bit), as in tests/test_gpu_demand.py:
  * tfx_demand_rows against devrng.demand_rows, the NumPy statement of rules 4 and 5 (tests/test_demand_rows_host.py holds
    that to a line-by-line Python one);
  * a heterogeneous engine with the mixed demand against the same engine with spawn 'none' that is fed the mirrored counts
    AND rows as per-tick buffers - on every step path heterogeneous cars take, for plain calls, decisions, episodes, warm
    restarts and clones.  assert_env_equal compares every live car's row."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_gpu_fused import engine_with
from test_gpu_clone import assert_env_equal, live_mask, snapshot
from test_gpu_episodes import EpisodeModel, first_phases, force_path, host
from test_demand_host import AGENT, BAD_ARGS, MASK, agent_actions, agent_weights
from test_gpu_demand import DEMAND, E, GRID, OFF, PROFILE, SEED, cars, weights
from test_demand_rows_host import RANGES, row_weights

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from gym_traffic import _native as nat  # noqa: E402
from gym_traffic import devrng  # noqa: E402

# rows (v, l, a, delta, v0, b, T, s0): the reference's car, a long slow truck, a short quick car - three: no power of two
TAB = np.array([[11.11, 4.0, 3.0, 4.0, 13.89, 6.0, 2.0, 1.0], [8.0, 8.0, 1.5, 4.0, 10.0, 4.0, 2.5, 2.0],
                [12.0, 3.5, 4.0, 2.0, 16.0, 7.0, 1.5, 1.0]], np.float32)
# heterogeneous cars never run LDS-resident: the per-tick kernels, two-tick passes alone, with k_tail, and split in halves.
# (TFX_RESIDENT=0 everywhere: envs this small would fit k_res, and a handle whose envs fit it takes no two-tick pass)
PATHS = {"pertick": {"TFX_RESIDENT": "0", "TFX_PAIRS": "0"},
         "pairs": {"TFX_RESIDENT": "0", "TFX_PAIRS": "2", "TFX_TAIL": "0", "TFX_SPLIT": "0"},
         "pairs_tail": {"TFX_RESIDENT": "0", "TFX_PAIRS": "2", "TFX_TAIL": "2", "TFX_SPLIT": "0"},
         "pairs_split": {"TFX_RESIDENT": "0", "TFX_PAIRS": "2", "TFX_TAIL": "2", "TFX_SPLIT": "2"}}
LIGHT = dict(means=[[0.3, 0.8, 0.0], [0.6, 0.2, 1.0]], seg_ticks=2, tick_offset=3)


def het_engine(env=None, n_envs=E, off=OFF, **grid):
    return engine_with(env or {}, n_envs, planes=3, env_id_offset=off, archetypes=TAB, **dict(GRID, **grid))


def mixed_engine(env=None, n_envs=E, off=OFF, profile=PROFILE, seed=SEED, demand=None, rw="default", **grid):
    eng = het_engine(env, n_envs, off, **grid)
    dm = dict(DEMAND if demand is None else demand)
    K, S = np.shape(dm["means"])
    dm.setdefault("weights", weights(eng.n_entry, K, S))
    prof = None if profile is None else torch.as_tensor(np.asarray(profile, np.int32)).to(eng.device)
    eng.set_demand(seed=seed, profile_of_env=prof, row_weights=row_weights(K, S) if isinstance(rw, str) else rw, **dm)
    return eng


def mirror(eng, tick0, n, ids=None, profile=None):
    """devrng.demand_rows for the engine's demand as it stands -> (counts, rows) of clock ticks tick0 .. tick0 + n - 1"""
    ids = np.arange(eng.E) + eng.cfg.env_id_offset if ids is None else ids
    prof = eng.demand_profile.cpu().numpy() if profile is None else profile
    return devrng.demand_rows(eng.demand["seed"], ids, np.arange(tick0, tick0 + n), eng.demand_tables, eng.demand_row_cdf,
                              eng.demand_rows_per_road, prof, seg_ticks=eng.demand["seg_ticks"], tick_offset=eng.demand["tick_offset"])


def feed(b, counts, rows, per_tick=True):
    b.set_spawns(counts=counts, rows=rows, per_tick=per_tick)


def assert_rows_equal(got, want, where):
    """counts in full; rows where the rule defines them: j < min(count, S)"""
    (gc, gr), (wc, wr) = got, want
    assert gc.dtype == np.int32 and gr.dtype == np.uint8 and gc.shape == wc.shape and gr.shape == wr.shape, where
    assert np.array_equal(gc, wc), (where, np.argwhere(gc != wc)[:5])
    S = wr.shape[-1]
    live = np.arange(S) < np.minimum(wc, S)[..., None]
    assert np.array_equal(gr[live], wr[live]), (where, np.argwhere((gr != wr) & live)[:5])
    return live


def assert_same(a, b, where, envs=None):
    sa, sb = snapshot(a), snapshot(b)
    for e in (range(a.E) if envs is None else envs):
        assert_env_equal(sa, e, sb, e, where)


def live_rows(eng):
    """the set of archetype rows the live cars of the engine carry"""
    s, Cc = snapshot(eng)
    out = set()
    for e in range(eng.E):
        out |= set(s["arch"][e][live_mask(s["leading"][e], s["lastcar"][e], Cc)].tolist())
    return out


# ---- 1. the kernel against the rule ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [None, "1"])
def test_rows_equal_the_rule(cap):
    """the ranges of tests/test_demand_rows_host.py: an item of 65 cars (a second round of lanes whose ranks start from the
    first round's histogram), roads with more cars than rows are kept, the clock wrap.  TFX_GRID_CAP=1: one workgroup -
    every wavefront strides over several items, its LDS slice handed from one to the next."""
    eng = mixed_engine({} if cap is None else {"TFX_GRID_CAP": cap})
    assert eng.n_entry == 6 and eng.demand_rows_per_road == 12 and eng.demand_row_cdf.shape == (2, 3, 3)
    seen = np.zeros(3, bool)
    for tick0, n in RANGES + ((0, 1), (5, 0)):
        got = [t.cpu().numpy() for t in eng.demand_rows(tick0, n)]
        want = mirror(eng, tick0, n)
        assert got[1].shape == (n, E, 6, 12)
        live = assert_rows_equal(got, want, (tick0, n))
        assert not got[1][~live].any()                      # (nothing written past the cars: the tensor's zeros)
        assert np.array_equal(eng.demand_counts(tick0, n).cpu().numpy(), want[0])
        if n == 7 and tick0 == 3:
            c, r = want
            assert (c[:, 0].sum(axis=1) > 64).any() and (c > 12).any()
            seen |= np.bincount(r[live], minlength=3) > 0
            two = [len(set(r[i, e, j, :min(c[i, e, j], 12)].tolist())) > 1 for i in range(7) for e in range(E) for j in range(6)]
            assert any(two)
    assert seen.all()


def test_rows_many_entry_roads_and_several_workgroups():
    """5x5 grid: 20 entry roads; 40 ticks x 3 envs = 120 items over 30 workgroups.  n_cdf - 1 is below C - 2 here"""
    eng = mixed_engine(n_envs=3, profile=[0, 0, 0], m=5, n=5, entry_spec=0, demand=dict(means=[[6.0]], seg_ticks=1, tick_offset=0),
                       rw=[1.0, 0.5, 2.0], capacity=40)
    S = eng.demand_tables.count_cdf.shape[2] - 1
    assert eng.n_entry == 20 and S < 38 and eng.demand_rows_per_road == S
    got = [t.cpu().numpy() for t in eng.demand_rows(100, 40)]
    live = assert_rows_equal(got, mirror(eng, 100, 40), "5x5")
    assert (got[0].sum(axis=(0, 1)) > 0).all() and set(got[1][live].tolist()) == {0, 1, 2}
    assert np.array_equal(eng.demand_counts(100, 40).cpu().numpy(), got[0])


# ---- 2. errors ---------------------------------------------------------------------------------------------------------------------
def test_errors_are_codes_and_a_refused_call_changes_nothing():
    lib = nat.lib()
    eng = mixed_engine()
    before = [t.cpu().numpy() for t in eng.demand_rows(3, 7)]
    dm, cases, keep = BAD_ARGS(nat, eng.n_entry)
    good = np.full((1, 2, 3), MASK, np.uint32)
    good[..., 0] = 1 << 30

    def call(h, d, rw, n_rows=3):
        rw = None if rw is None else np.ascontiguousarray(rw, np.uint32)
        keep.append(rw)
        return lib.tfx_set_demand_mixed(h, None if d is None else C.byref(d), None if rw is None else rw.ctypes.data_as(C.c_void_p), n_rows)

    # every check tfx_set_demand makes ...
    bad_rc = np.full((1, 2, eng.n_entry), MASK, np.uint32)
    bad_rc[0, 1, :3] = [1, 9, 5]
    for d, msg in cases + [(dm(rc=bad_rc), b"road_cdf row (0, 1) decreases at 2")]:
        assert call(eng.h, d, good) == -1, msg
        assert msg in lib.tfx_last_error(), (msg, lib.tfx_last_error())
    # ... and its own
    decreasing, short = good.copy(), np.full((1, 2, 3), 7, np.uint32)
    decreasing[0, 1] = [9, 5, MASK]
    for rw, n_rows, msg in ((None, 3, b"row_cdf is null"), (good, 2, b"n_rows 2 is not the handle's n_archetypes 3"), (good, 4, b"n_rows 4"),
                            (decreasing, 3, b"row_cdf row (0, 1) decreases at 1"), (short, 3, b"row_cdf row (0, 0) does not end in 0xFFFFFFFF")):
        assert call(eng.h, dm(), rw, n_rows) == -1, msg
        assert msg in lib.tfx_last_error(), (msg, lib.tfx_last_error())
    assert call(None, dm(), good) == -1 and b"null handle" in lib.tfx_last_error()
    # the plain call keeps refusing a heterogeneous handle; the mixed call refuses a handle that is not
    assert lib.tfx_set_demand(eng.h, C.byref(dm())) == -1 and b"heterogeneous" in lib.tfx_last_error()
    plain = engine_with({}, E, env_id_offset=OFF, **GRID)
    assert call(plain.h, dm(), good) == -1 and b"heterogeneous" in lib.tfx_last_error()
    with pytest.raises(ValueError, match="row_weights"):
        plain.set_demand([[1.0]], row_weights=[1, 1, 1])
    # before tfx_bind_buffers
    h = C.c_void_p()
    nat.check(lib.tfx_create(C.byref(eng.cfg), C.byref(h)))
    assert call(h, dm(), good) == -2 and b"tfx_bind_buffers" in lib.tfx_last_error()
    nat.check(lib.tfx_destroy(h))
    # tfx_demand_rows without a mixed demand: a plain demand, no demand, a demand replaced
    cnt = torch.zeros((2, E, eng.n_entry), dtype=torch.int32, device=eng.device)
    rws = torch.zeros((2, E, eng.n_entry, 12), dtype=torch.uint8, device=eng.device)
    args = (0, 2, C.c_void_p(cnt.data_ptr()), C.c_void_p(rws.data_ptr()), None)
    assert lib.tfx_demand_rows(plain.h, *args) == -2 and b"tfx_set_demand_mixed" in lib.tfx_last_error()
    plain.set_demand([[1.0]])
    assert lib.tfx_demand_rows(plain.h, *args) == -2
    per_road = C.c_int32(-7)
    assert lib.tfx_demand_rows_per_road(plain.h, C.byref(per_road)) == -2 and per_road.value == -7
    with pytest.raises(nat.TfxError, match="tfx error -2"):
        plain.demand_rows(0, 2)
    assert lib.tfx_demand_rows(eng.h, 0, 2, None, args[3], None) == -1 and b"counts is null" in lib.tfx_last_error()
    assert lib.tfx_demand_rows(eng.h, 0, 2, args[2], None, None) == -1 and b"rows is null" in lib.tfx_last_error()
    assert lib.tfx_demand_rows(eng.h, 0, -1, args[2], args[3], None) == -1 and b"n_ticks -1" in lib.tfx_last_error()
    assert not cnt.any() and not rws.any()
    # nothing changed: the demand set before the refusals still makes the same rows, and steps
    assert lib.tfx_demand_rows_per_road(eng.h, C.byref(per_road)) == 0 and per_road.value == 12
    after = [t.cpu().numpy() for t in eng.demand_rows(3, 7)]
    assert np.array_equal(after[0], before[0]) and np.array_equal(after[1], before[1])
    eng.reset(np.zeros((E, eng.I), np.int32))
    eng.set_actions(cycle_period=5)
    eng.step(4)
    assert cars(eng) > 0
    # another spawn rule replaces it, and what the engine exposes goes
    eng.set_spawns(period=4)
    assert lib.tfx_demand_rows(eng.h, *args) == -2
    assert eng.demand is None and eng.demand_row_cdf is None and eng.demand_rows_per_road is None
    n = cars(eng)
    eng.step(8)
    assert cars(eng) != n
    with pytest.raises(nat.TfxError, match="n_ticks = 65"):          # a decision's rows are drawn up front: 64 at most
        e2 = mixed_engine()
        e2.reset(np.zeros((E, e2.I), np.int32))
        e2.agent_step(65)
    assert keep


# ---- 3. plain calls against mirrored counts and rows -------------------------------------------------------------------------
def run_steps(path, calls, **grid):
    n_envs = grid.pop("n_envs", E)
    profile = grid.pop("profile", PROFILE)
    a = mixed_engine(PATHS[path], n_envs=n_envs, profile=profile, demand=grid.pop("demand", None), **grid)
    b = het_engine(PATHS[path], n_envs=n_envs, **grid)
    ph = first_phases(n_envs, a.I)
    rng = np.random.RandomState(9)
    for eng in (a, b):
        eng.reset(ph)
    tick = 0
    for n in calls:
        act = rng.randint(2, size=(n_envs, a.I)).astype(np.int32)
        a.set_actions(act)
        b.set_actions(act)
        feed(b, *mirror(a, tick, n))
        a.step(n)
        b.step(n)
        tick += n
        assert_same(a, b, (path, tick))
    assert a.tick == tick and cars(a) > 10 and len(live_rows(a)) >= 2
    return a, b


@pytest.mark.parametrize("path", list(PATHS))
def test_step_equals_mirrored_rows(path):
    a, b = run_steps(path, [7, 7, 1, 4])
    assert a.fused_ticks()[0] == 0
    pairs = path.startswith("pairs")
    assert a.pair_ticks() == (6 + 6 + 4 if pairs else 0)
    assert (a.tail_ticks() > 0) == (path in ("pairs_tail", "pairs_split"))
    assert a.split_ticks() == (7 + 7 + 4 if path == "pairs_split" else 0)
    dt = a.done_tick.cpu().numpy()
    assert dt[0] > 0 and not dt[2] and not dt[3]                     # the env with the mean-70 segment overflows; no cars, no overflow


@pytest.mark.parametrize("path", ["pairs", "pertick"])
def test_step_two_tiles(path):
    """5x5 grid x 1 env: 120 roads, two tiles of 64"""
    a, _ = run_steps(path, [7, 6], n_envs=1, profile=[1], m=5, n=5, entry_spec=0)
    assert a.R == 120 and a.n_entry == 20


@pytest.mark.parametrize("path", ["pairs", "pertick"])
def test_move_cars_draws_the_rows_of_the_clocks_tick(path):
    """tfx_move_cars / tfx_advance_finished_cars, tick by tick: the mixed handle draws one row of counts and of archetype
    rows for the tick the clock stands at, and its move kernel reads them under the per-tick stride install_stream left"""
    a, b = mixed_engine(PATHS[path]), het_engine(PATHS[path])
    ph = first_phases(E, a.I)
    rng = np.random.RandomState(3)
    for eng in (a, b):
        eng.reset(ph)
    for t in range(9):
        act = rng.randint(2, size=(E, a.I)).astype(np.int32)
        a.set_actions(act)
        b.set_actions(act)
        c, r = mirror(a, t, 1)
        feed(b, c[0], r[0], per_tick=False)
        for eng in (a, b):
            eng.move_cars()
            eng.advance_finished_cars()
        assert_same(a, b, (path, t))
    assert a.tick == 9 and cars(a) > 10 and len(live_rows(a)) >= 2 and a.demand_rows_per_road == 12


@pytest.mark.parametrize("path", ["pairs_tail", "pairs_split"])
def test_step_longer_than_the_buffer(path):
    """70 ticks: the handle's buffers hold 64 rows of counts and of archetype rows, so the call is drawn in two chunks"""
    a, _ = run_steps(path, [70, 3], demand=LIGHT)
    assert a.tick == 73


# ---- 4. decisions -----------------------------------------------------------------------------------------------------------------
AGENT_PATHS = {k: PATHS[k] for k in ("pertick", "pairs_tail", "pairs_split")}


def agent_engines(env):
    sc = AGENT
    grid = dict(m=sc["m"], n=sc["n"], length=sc["length"], capacity=sc["capacity"], rate=sc["rate"], entry_spec=sc["entry_spec"])
    a = het_engine(env, sc["E"], sc["off"], **grid)
    b = het_engine(env, sc["E"], sc["off"], **grid)
    prof = torch.as_tensor(np.asarray(sc["profiles"], np.int32)).to(a.device)
    a.set_demand(sc["means"], agent_weights(a.n_entry), seg_ticks=sc["seg_ticks"], tick_offset=sc["tick_offset"], seed=sc["seed"],
                 profile_of_env=prof, row_weights=[[[3.0, 1.0, 2.0], [1.0, 0.0, 1.0]], [[1.0, 1.0, 1.0], [0.2, 1.0, 0.5]]])
    return a, b


@pytest.mark.parametrize("graph", ["1", "0"])
@pytest.mark.parametrize("path", list(AGENT_PATHS))
def test_agent_step_equals_mirrored_rows(path, graph):
    """10-tick decisions at capacity 6 (S = 4 rows per road) under the demand of tests/test_demand_host.py's AGENT scenario,
    whose heavy profile overflows four-car roads part-way through a decision: counts and rows of a decision are drawn up
    front, an env that stops does not consume the rest.  The second and third decision replay the captured graph."""
    sc = AGENT
    T = sc["T"]
    a, b = agent_engines(dict(AGENT_PATHS[path], TFX_GRAPH=graph))
    assert a.demand_rows_per_road == 4
    counts, rows = mirror(a, 0, sc["decisions"] * T)
    for eng in (a, b):
        eng.reset(np.zeros((sc["E"], eng.I), np.int32))
    mid = 0
    for s in range(sc["decisions"]):
        act = agent_actions(sc["E"], a.I, s)
        a.set_actions(act)
        b.set_actions(act)
        feed(b, counts[s * T:(s + 1) * T], rows[s * T:(s + 1) * T])
        oa, ob = host(a.agent_step(T)), host(b.agent_step(T))
        for u, v, name in zip(oa, ob, ("aobs", "areward", "adone")):
            assert np.array_equal(u.view(np.uint8), v.view(np.uint8)), (s, name)
        assert_same(a, b, (path, graph, s))
        dt = a.done_tick.cpu().numpy()
        mid += int(((dt > s * T) & (dt < (s + 1) * T)).sum())            # (done_tick: the overflow's clock tick + 1)
    assert mid > 0 and len(live_rows(a)) >= 2
    assert a.fused_ticks()[0] == 0 and (a.pair_ticks() > 0) == path.startswith("pairs")
    assert (a.split_ticks() == sc["decisions"] * T) == (path == "pairs_split")


@pytest.mark.parametrize("path", ["pairs_tail", "pertick"])
def test_rewriting_the_profile_between_replayed_decisions(path):
    """demand_profile is read when the arrivals are drawn: rewritten between the second and the third decision - both
    replays of the captured graph - it changes counts and rows of exactly the rewritten envs, with no re-capture."""
    T = 10
    dm = dict(means=[[0.4, 1.0, 0.2], [1.6, 0.1, 0.9]], seg_ticks=2, tick_offset=3)
    a = mixed_engine(dict(PATHS[path], TFX_GRAPH="1"), profile=[0, 0, 0, 0, 0], demand=dm)
    b = het_engine(PATHS[path])
    for eng in (a, b):
        eng.reset(np.zeros((E, eng.I), np.int32))
    rewritten = [1, 3]
    for s in range(4):
        if s == 2:
            old = [t.cpu().numpy() for t in a.demand_rows(s * T, T)]
            a.demand_profile[rewritten] = 1
            new = [t.cpu().numpy() for t in a.demand_rows(s * T, T)]
            for e in range(E):
                same = np.array_equal(old[0][:, e], new[0][:, e]) and np.array_equal(old[1][:, e], new[1][:, e])
                assert same == (e not in rewritten), e
                assert (e not in rewritten) or not np.array_equal(old[1][:, e], new[1][:, e])
        act = agent_actions(E, a.I, s)
        a.set_actions(act)
        b.set_actions(act)
        feed(b, *mirror(a, s * T, T))
        oa, ob = host(a.agent_step(T)), host(b.agent_step(T))
        for u, v in zip(oa, ob):
            assert np.array_equal(u.view(np.uint8), v.view(np.uint8)), s
        assert_same(a, b, (path, s))
    assert cars(a) > 10 and len(live_rows(a)) >= 2


# ---- 5. the batched env -------------------------------------------------------------------------------------------------------------
VENV_ROWS = [[[2.0, 1.0, 1.0], [1.0, 3.0, 0.0]], [[1.0, 1.0, 2.0], [0.0, 1.0, 1.0]]]


def make_venv(n_envs=E, **kw):
    from gym_traffic.envs.vec_env import TrafficVecEnv
    args = dict(capacity=10, entry_spec=1, seed=5, spawn='demand', archetypes=TAB,
                demand=dict(means=[[0.3, 0.6], [0.9, 0.3]], weights=None, seg_ticks=7, tick_offset=-3, row_weights=VENV_ROWS))
    args.update(kw)
    return TrafficVecEnv(n_envs, 2, 2, 120.0, **args)


def test_autoreset_equals_mirrored_rows(monkeypatch):
    """episode_len = 3 over 8 decisions: the restarts do not touch the rules - they read the clock, which runs on"""
    force_path(monkeypatch, "pairs")
    kw = dict(capacity=6, env_id_offset=OFF, autoreset=True, episode_len=3)
    dm = dict(means=AGENT["means"], weights=None, seg_ticks=7, tick_offset=-3, row_weights=VENV_ROWS)
    a = make_venv(demand=dm, **kw)
    b = make_venv(spawn='none', demand=None, **kw)
    assert a.engine.het and a.engine.demand_rows_per_road == 4 and a.engine.demand_row_cdf.shape == (2, 2, 3)
    a.demand_profile.copy_(torch.as_tensor(np.array([1, 0, 1, 0, 1], np.int32)))
    ph = first_phases(E, a.engine.I)
    a.reset(ph)
    b.reset(ph)
    model = EpisodeModel(E, a.engine.I, 3)
    ended, kinds = 0, set()
    for s in range(8):
        act = torch.as_tensor(agent_actions(E, a.engine.I, s)).to(a.engine.device)
        feed(b.engine, *mirror(a.engine, 10 * s, 10))
        oa, ob = host(a.agent_step(act, n_ticks=10)), host(b.agent_step(act, n_ticks=10))
        for u, v in zip(oa, ob):
            assert np.array_equal(u.view(np.uint8), v.view(np.uint8)), s
        model.decision(ob[1], ob[2])
        assert np.array_equal(a.episode_length.cpu().numpy(), model.ep_len)
        assert np.array_equal(a.episode_index.cpu().numpy(), b.episode_index.cpu().numpy())
        assert_same(a.engine, b.engine, s)
        ended += int(oa[2].sum())
        kinds |= live_rows(a.engine)
    assert model.ep_index.min() >= 2 and ended > 0 and cars(a.engine) > 0 and len(kinds) >= 2


def test_vec_env_warm_pool_snapshot_and_clone_carry_the_rows(monkeypatch):
    """tests/test_gpu_demand.py's warm-pool loop with mixed cars: A restarts on the device from the pool, B is cloned by
    hand; the pool, a snapshot and a clone are made with the env's row_weights"""
    force_path(monkeypatch, "pairs")
    M, n_pool, seed = 4, 3, 5
    a = make_venv(autoreset=True, episode_len=M)
    b = make_venv()
    pool = a.make_warm_pool(n_pool, 3)
    assert pool.spawn == 'demand' and pool.engine.het and cars(pool.engine) > 0
    assert np.array_equal(pool.engine.demand_row_cdf, a.engine.demand_row_cdf)
    assert pool.engine.demand_rows_per_road == a.engine.demand_rows_per_road == 10 - 2
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
        if s + 1 < 10:
            slots = devrng.episode_pool_slots(seed, ids, model.ep_index, n_pool)
            b.clone_envs(np.where(end, slots, -1).astype(np.int32), source=pool, streams=False, episodes=False)
    assert model.ep_index.min() >= 2
    assert_same(a.engine, b.engine, "final")
    assert cars(a.engine) > 10 and len(live_rows(a.engine)) >= 2
    # a snapshot is made like the env - the same row table - and follows it; restore brings the env back
    snap = b.snapshot()
    assert np.array_equal(snap.engine.demand_row_cdf, b.engine.demand_row_cdf)
    held = torch.ones((E, b.engine.I), dtype=torch.int32, device=b.engine.device)
    b.step(held, n_ticks=9)
    moved = snapshot(b.engine)
    b.restore(snap)
    (back, Cc), (kept, _) = snapshot(b.engine), snapshot(snap.engine)
    assert not np.array_equal(moved[0]["lastcar"], back["lastcar"])
    # (the two stand at different clocks, so the cars' spawn ticks are rebased: positions and rows are what must agree)
    assert np.array_equal(back["lastcar"], kept["lastcar"]) and np.array_equal(back["leading"], kept["leading"])
    for e in range(E):
        live = live_mask(back["leading"][e], back["lastcar"][e], Cc)
        assert np.array_equal(back["arch"][e][live], kept["arch"][e][live]) and np.array_equal(back["x"][e][live], kept["x"][e][live]), e


# ---- 6. clones ----------------------------------------------------------------------------------------------------------------------
def test_clone_with_its_stream_receives_its_sources_cars_and_rows():
    dm = dict(means=[[0.4, 1.0, 0.2], [1.6, 0.1, 0.9]], seg_ticks=2, tick_offset=3)
    env = PATHS["pairs_tail"]
    src = mixed_engine(env, profile=[0, 1, 0, 1, 1], demand=dm, capacity=10)
    dst = mixed_engine(env, off=100, profile=[0, 0, 0, 0, 0], demand=dm, capacity=10)
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
        eng.step(9)
    dst.clone_envs(idx, source=src, streams=True)
    dst.demand_profile.copy_(torch.as_tensor(np.array([1, 0, 0, 1, 0], np.int32)))       # (the sources' profiles: the caller's)
    for n, kind in ((7, "step"), (10, "agent"), (4, "step")):
        bind_actions()
        for eng in (src, dst):
            eng.agent_step(n) if kind == "agent" else eng.step(n)
        ss, sd = snapshot(src), snapshot(dst)
        for e, s in enumerate(idx):
            if s >= 0:
                assert_env_equal(sd, e, ss, int(s), (kind, e))
    # the preview shows it: stream ids 43, 101, 40, 41, 104
    got = [t.cpu().numpy() for t in dst.demand_rows(30, 6)]
    assert_rows_equal(got, mirror(dst, 30, 6, ids=np.array([43, 101, 40, 41, 104])), "clone")
    assert cars(dst) > 10 and len(live_rows(dst)) >= 2


def test_clone_refusals():
    dm = dict(means=[[0.4, 1.0, 0.2], [1.6, 0.1, 0.9]], seg_ticks=2, tick_offset=3)
    src = mixed_engine(demand=dm)
    idx = np.arange(E, dtype=np.int32)
    src.reset(np.zeros((E, src.I), np.int32))

    def refused(dst, word, same_world=True):
        dst.reset(np.zeros((E, dst.I), np.int32))
        with pytest.raises(nat.TfxError) as exc:
            dst.clone_envs(idx, source=src, streams=True)
        assert "tfx error -1:" in str(exc.value) and word in str(exc.value), str(exc.value)
        if same_world:
            dst.clone_envs(idx, source=src, streams=False)          # (the same world: fine without the stream)

    other = row_weights()
    other[1, 1] += [0.0, 0.5, 0.0]
    refused(mixed_engine(demand=dm, rw=other), "demand tables")
    refused(mixed_engine(demand=dict(dm, weights=weights(6) + 0.01)), "demand tables")
    refused(mixed_engine(demand=dm, seed=SEED + 1), "demand seed")
    poisson = het_engine()
    poisson.set_poisson(0.5, seed=SEED)
    refused(poisson, "stream kind")
    # a plain demand handle has a single archetype: another world
    plain = engine_with({}, E, planes=3, env_id_offset=OFF, **GRID)
    plain.set_demand(seed=SEED, weights=weights(6), **dm)
    refused(plain, "n_archetypes", same_world=False)
    same = mixed_engine(demand=dm)
    same.reset(np.zeros((E, same.I), np.int32))
    same.clone_envs(idx, source=src, streams=True)                         # (equal tables: accepted)


# ---- 7. the demo --------------------------------------------------------------------------------------------------------------------
def test_demand_demo_with_trucks():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "demand_demo.py"), "--envs", "8", "--m", "3", "--n", "3",
                          "--length", "120", "--capacity", "14", "--decisions", "8", "--ticks", "6", "--seg-decisions", "2",
                          "--trucks", "0.4,0.1"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    print(out.stdout)
    lines = out.stdout.splitlines()
    rets = {l.split()[1]: float(l.split()[-1]) for l in lines if l.startswith("return ")}
    assert set(rets) == {"cycle", "greedy"} and all(np.isfinite(v) for v in rets.values())
    seg = [l for l in lines if l.startswith("segment ")]
    assert len(seg) == 2 and all(int(l.split("cars")[1].split()[0]) > 0 for l in seg)
    rows = [l for l in lines if l.startswith("rows")]
    assert len(rows) == 1
    peak, off = [float(part.split(":")[1].split()[0]) for part in rows[0].split("segment ")[1:]]
    # some 170 cars per segment at shares 0.4 and 0.1: 68 +- 6 trucks against 17 +- 4
    assert 0.0 < peak < 1.0 and 0.0 <= off < peak
