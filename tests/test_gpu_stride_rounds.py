"""Later rounds of every grid-stride loop, on ragged batches.

Nearly every kernel on the step path walks its work in a stride loop, and everywhere else in this suite the first
round covers all the work (1-9 envs of one-tile grids) or the traffic is the benchmark's (every env alike, no wrapped
ring, no overflow, no frozen env).  A second trip through such a loop is where a missing barrier, LDS staged for one env
while another is still being read, a register carried over from the previous tile or a `continue` that skips a barrier
shows.  Here the loops go round at the smallest batch that can show it.

Part A: 11 envs of the 6x5 grid of 60 m roads (R = 142 roads = 3 tiles per env, the last one with 14 live lanes; I = 30,
22 entry roads; 33 tiles, so a workgroup's four wavefronts straddle two envs; the halves of a split call are 5 and 6 envs)
with TFX_GRID_CAP=2 (one case per mover at 3, and 1 where only that makes three rounds): every strided launch takes at
most that many workgroups.  Rounds a kernel then makes = ceil(items / (items per workgroup * cap)):

  kernel                            items                    per workgroup   rounds at cap 2 (3) [1]
  k_move_tt, k_move_t, k_risk,      33 tiles                 4 (a wavefront  5 (3)
    k_edge                                                     each)
  ... as the halves of a split call 15 / 18 tiles            4               2 / 3
  k_move_dma (ring layout)          25 tiles of 64 roads     4               4 (3)
  k_move<1> (ring layout, odd C)    391 groups of 4 roads    a chunk of 196  196 passes per workgroup (131)
  k_move_tts, two wavefronts a tile 17 tile pairs            1               9
  k_move_tts, four / eight          33 tiles                 1               17
  k_move_ts                         33 tiles                 1               17 (11)
  k_tail                            11 envs                  1               6 (4)
  ... as the halves of a split call 5 / 6 envs               1               3 / 3
  k_poisson                         11 envs                  1               6 [11; 18 with 18 envs]
  k_advance*                        11 * (30 + 22) = 572     256             2 [3]
  k_clone (in place, across, pool)  33 tiles                 4               5
  k_reset, k_refresh, k_import/     11 * 142 = 1562 roads    256             4
    export_ring, k_cars_on_roads,
    k_episode_begin
  k_agent_tail                      11 * 270 = 2970          256             6
  k_remi, k_greedy                  11 * 30 = 330            256             1 [2; 18 envs: 540, 3 rounds]
  k_measure, k_cells                TFX_MEASURE_GRID keeps priority (tests/test_gpu_measures.py, test_gpu_cells.py)
k_remi and k_greedy have one lane per intersection and no state between elements: at 11 envs they cannot make three
rounds, so one case runs 18 envs at cap 1.  k_done has a lane per env (one round).  Each test asserts its own rows of
this table as arithmetic from eng.E, eng.R, eng.I and the cap.

Inputs of part A: ring states from `ragged_state` (below; the distribution of tests/test_gpu_parity.py:random_state,
vectorised) - crowd 0.3 and 0.8, cars up to 0 / 5 / 40 / 160 % of a road length past the road end, sorted and
unsorted - a fresh one per call, per-env and per-tick random actions and arrival counts, calls of 3, 4, 7, 2, 5, 1, 6 ticks.
After every call EVERY env is compared with the oracle (tests/test_gpu_parity.py:assert_same_state: ring words, obs,
rewards, waiting, passed_dst, every live car bit for bit), and so are the done flags, the vehicle updates, the clock and
in validate mode the trip log; the path counters must say the intended kernels ran.

Part B: 2309 envs (a prime: halves of 1154 and 1155 envs, a part-filled last workgroup) of the same grid on the shipped
defaults, TFX_GRID_CAP unset, ragged states, per-env Poisson(0.1) arrivals per entry road and tick, per-env random
actions, every env compared with the oracle.

Nothing here depends on where a heuristic flips.  No case provokes a fault: the cap only makes grids smaller."""
import ctypes
import os

import numpy as np
import pytest

from oracle.oracle import OracleEnv, XI, VI, WI, live_mask
from test_gpu_parity import assert_same_state, same_bits

gpu = pytest.mark.gpu

M, N, LENGTH, RATE = 6, 5, 60.0, 0.5
E_A, E_B = 11, 2309
CALLS = [3, 4, 7, 2, 5, 1, 6]
BEYOND = [0.0, 0.05, 0.4, 1.6]
# v, l, a, delta, v0, b, T, s0: the first three rows of tests/test_gpu_archetypes.py:MIXED_ROWS
TAB8 = np.array([[11.11, 4, 3, 4, 13.89, 6, 2, 1], [8.0, 8, 1.5, 1, 10.0, 4, 2.5, 2], [12.0, 3.5, 4, 2, 16.0, 7, 1.5, 1]],
                np.float32)
ROWS_PER_ROAD = 4       # S of the spawn-row buffers (no road receives more cars in a tick here)

PAIRS = {"TFX_RESIDENT": "0", "TFX_PAIRS": "2", "TFX_TAIL": "2", "TFX_SPLIT": "0", "TFX_TT_SEG": "0"}
FOLLOW = {"tail": {}, "launches": {"TFX_TAIL": "0"}, "split": {"TFX_SPLIT": "2"}}


# ---- the ragged ring states ----------------------------------------------------------------------------------------------
def ragged_state(rng, E, R, C, length, crowd=0.5, beyond=0.15, sorted_x=True, full="any", entry_roads=None,
                 return_counts=False):
    """tests/test_gpu_parity.py:random_state without its Python loop over envs x roads x cars (NumPy only): `leading`
    uniform in 1..C-1, so wrapped rings are common; binomial(C - 2, crowd) cars per road with a tenth of the roads empty
    and a tenth full; x from -20 to length * (1 + beyond), non-increasing from head to tail when sorted_x; half the cars
    standing, the others at 0-15 m/s; spawn ticks 0..49; +inf in the leader slot; zeros in the dead slots.
    full: "any" - full rings as above; "not_entry" - none on `entry_roads` (at most C - 3 cars there); "none" - nowhere.
    -> x, v, w [E, R, C] float32, leading, lastcar [E, R] int32 (and the car counts with return_counts)."""
    leading = rng.randint(1, C, size=(E, R)).astype(np.int32)
    n = np.minimum(rng.binomial(C - 2, crowd, size=(E, R)), C - 2)
    n[rng.rand(E, R) < 0.1] = 0
    fill = rng.rand(E, R) < 0.1
    if full == "any":
        n[fill] = C - 2
    elif full == "not_entry":
        fill[:, np.asarray(entry_roads, np.int64)] = False
        n[fill] = C - 2
        n[:, np.asarray(entry_roads, np.int64)] = np.minimum(n[:, np.asarray(entry_roads, np.int64)], C - 3)
    elif full == "none":
        n = np.minimum(n, C - 3)
    else:
        raise ValueError(full)
    n = np.maximum(n, 0).astype(np.int32)
    j = np.arange(C - 2)
    car = j[None, None, :] < n[:, :, None]                      # car j of the road, counted from the head
    pos = rng.uniform(-20, length * (1 + beyond), size=(E, R, C - 2))
    if sorted_x:
        pos = -np.sort(-np.where(car, pos, -np.inf), axis=2)    # the road's own cars first, head to tail
    speed = np.where(rng.rand(E, R, C - 2) < 0.5, 0.0, rng.uniform(0, 15, size=(E, R, C - 2)))
    tick = rng.randint(0, 50, size=(E, R, C - 2))
    # car j sits j + 1 slots behind the leader on the ring of the slots 1..C-1
    slot = (leading[:, :, None].astype(np.int64) - 1 + j[None, None, :] + 1) % (C - 1) + 1
    x = np.zeros((E, R, C), np.float32)
    v = np.zeros((E, R, C), np.float32)
    w = np.zeros((E, R, C), np.float32)
    np.put_along_axis(x, slot, np.where(car, pos, 0.0).astype(np.float32), axis=2)
    np.put_along_axis(v, slot, np.where(car, speed, 0.0).astype(np.float32), axis=2)
    np.put_along_axis(w, slot, np.where(car, tick, 0).astype(np.float32), axis=2)
    lastcar = ((leading.astype(np.int64) - 1 + n) % (C - 1) + 1).astype(np.int32)
    # exit roads keep the +inf leader they got at reset (traffic_env.py:263); train roads get theirs rewritten every tick
    np.put_along_axis(x, leading[:, :, None].astype(np.int64), np.float32(np.inf), axis=2)
    out = (x, v, w, leading, lastcar)
    return out + (n,) if return_counts else out


def live_all(leading, lastcar, C):
    """oracle.live_mask for every env at once: bool [E, R, C]"""
    E, R = leading.shape
    return live_mask(leading.reshape(-1), lastcar.reshape(-1), C).reshape(E, R, C)


def load_oracle(orc, x, v, w, leading, lastcar):
    """OracleEnv.load_planes for every env at once (the config's single archetype)"""
    orc.leading[:] = leading
    orc.lastcar[:] = lastcar
    live = live_all(orc.leading, orc.lastcar, orc.C)
    row = np.asarray(orc.cfg.archetype[:], np.float32)
    orc.state[:] = row[None, None, :, None] * live[:, :, None, :].astype(np.float32)
    orc.state[:, :, XI, :] = np.where(live, x, 0)
    orc.state[:, :, VI, :] = np.where(live, v, 0)
    orc.state[:, :, WI, :] = np.where(live, w, 0)
    ld = orc.leading[:, :, None].astype(np.int64)
    np.put_along_axis(orc.state[:, :, XI, :], ld, np.take_along_axis(np.asarray(x, np.float32), ld, axis=2), axis=2)


def grid_tables(m=M, n=N):
    """dest, phases, nexts and the entry roads of the m x n grid (default: the 6x5 one), built as
    csrc/tfx_handle.hpp:build_tables does (roadgraph.py:26-64) - the CPU tests have no handle to ask"""
    I = m * n
    r = 4 * I
    R = r + 2 * m + 2 * n
    dest, phases, nexts = np.full(R, -1, np.int32), np.zeros(R, np.int32), np.full(R, -1, np.int32)
    for d in range(4):
        for row in range(m):
            for col in range(n):
                li = row * n + col
                e = d * I + li
                dest[e] = li
                phases[e] = 1 if d < 2 else 0
                if d == 0:
                    nexts[e] = e + 1 if col < n - 1 else r + n + row
                elif d == 1:
                    nexts[e] = e - 1 if col > 0 else r + 2 * n + m + row
                elif d == 2:
                    nexts[e] = e + n if row < m - 1 else r + n + m + col
                else:
                    nexts[e] = e - n if row > 0 else r + col
    fed = set(int(t) for t in nexts if t >= 0)
    entry = np.array([e for e in range(r) if e not in fed], np.int32)
    return dest, phases, nexts, entry


def test_ragged_state_ring_invariants():
    """CPU: the generator against the ring invariants - live_mask counts n cars, lastcar follows from leading and n, x is
    non-increasing from head to tail when sorted, the switches keep full rings away - and through OracleEnv.load_planes."""
    dest, phases, nexts, entry = grid_tables()
    R = len(dest)
    assert (R, len(entry)) == (142, 22)
    for C, sorted_x, full in [(10, True, "any"), (34, False, "any"), (10, True, "not_entry"), (66, True, "none"), (11, False, "any")]:
        rng = np.random.RandomState(100 + C)
        E = 23
        x, v, w, ld, lc, n = ragged_state(rng, E, R, C, LENGTH, crowd=0.55, beyond=0.4, sorted_x=sorted_x, full=full,
                                          entry_roads=entry, return_counts=True)
        assert x.dtype == v.dtype == w.dtype == np.float32 and ld.dtype == lc.dtype == np.int32
        assert ld.min() >= 1 and ld.max() == C - 1 and lc.min() >= 1 and lc.max() <= C - 1
        live = live_all(ld, lc, C)
        assert np.array_equal(live.sum(axis=2), n)
        assert np.array_equal((lc - ld) % (C - 1), n % (C - 1)) and n.max() <= C - 2
        assert (ld > lc).any() and (n == 0).any()                              # wrapped rings and empty roads are there
        assert np.isinf(np.take_along_axis(x, ld[:, :, None].astype(np.int64), axis=2)).all()
        dead = ~live & (np.arange(C)[None, None, :] != ld[:, :, None])
        assert not x[dead].any() and not v[dead].any() and not w[dead].any()
        assert x[live].min() >= -20 and x[live].max() <= LENGTH * 1.4 and (x[live] > LENGTH).any()
        assert 0.4 < (v[live] == 0).mean() < 0.6 and v[live].max() <= 15
        if full == "any":
            assert (n == C - 2).mean() > 0.05
        elif full == "none":
            assert n.max() <= C - 3
        else:
            assert n[:, entry].max() == C - 3 and (n == C - 2).any()
        # head to tail
        order = (ld[:, :, None].astype(np.int64) - 1 + np.arange(1, C - 1)[None, None, :]) % (C - 1) + 1
        xs = np.take_along_axis(x, order, axis=2)
        inside = np.arange(C - 2)[None, None, :] < n[:, :, None]
        assert np.array_equal(np.take_along_axis(live, order, axis=2), inside)
        steps = np.diff(xs, axis=2)[inside[:, :, 1:]]
        assert (steps <= 0).all() if sorted_x else (steps > 0).any()
        # through the oracle's own loader, env by env, and the batched loader used at 2309 envs
        a = OracleEnv(M, N, LENGTH, C, dest, phases, nexts, n_envs=E)
        b = OracleEnv(M, N, LENGTH, C, dest, phases, nexts, n_envs=E)
        for k in range(E):
            a.load_planes(k, x[k], v[k], w[k], ld[k], lc[k])
        load_oracle(b, x, v, w, ld, lc)
        assert np.array_equal(a.state.view(np.int32), b.state.view(np.int32))
        assert np.array_equal(a.leading, ld) and np.array_equal(a.lastcar, lc)
        for k in (0, E - 1):
            for got, want in zip(a.planes(k), (x[k], v[k], w[k])):
                assert np.array_equal(got.view(np.int32), want.view(np.int32))
        assert np.array_equal(a.cars_on_roads_flat(), n)
        done = a.step(np.zeros((E, M * N), np.int32), None)[2]                 # ... and it steps
        assert done.shape == (E,)


# ---- engines ---------------------------------------------------------------------------------------------------------------
def make_engine(knobs, E, C, cap=None, **cfg):
    """A handle created under exactly the TFX_* switches of `knobs` (and TFX_GRID_CAP=cap): every other one is taken out
    of the environment while tfx_create and tfx_bind_buffers read it (TFX_LIB names the library itself)."""
    from gym_traffic.core import TfxEngine
    env = dict(knobs)
    if cap is not None:
        env["TFX_GRID_CAP"] = str(cap)
    keep = {k: v for k, v in os.environ.items() if k.startswith("TFX_") and k != "TFX_LIB"}
    for k in keep:
        del os.environ[k]
    os.environ.update(env)
    try:
        cfg.setdefault("layout", "transposed")
        eng = TfxEngine(M, N, LENGTH, C, n_envs=E, rate=RATE, **cfg)
    finally:
        for k in env:
            os.environ.pop(k, None)
        os.environ.update(keep)
    return eng


def rounds(items, per_workgroup, cap):
    return -(-items // (per_workgroup * cap))


def tiles_of(eng):
    return eng.E * ((eng.R + 63) // 64)


def device_tick(eng):
    t = ctypes.c_int32()
    from gym_traffic import _native as nat
    nat.check(eng.lib.tfx_get_tick(eng.h, ctypes.byref(t)))
    return int(t.value)


def tab10_of(tab8):
    t = np.zeros((len(tab8), 10), np.float32)
    t[:, 1:9] = tab8
    return t


def csr(cnt, entrypoints):
    """arrival counts [E, n_entry] -> the oracle's (offsets, roads): per env by entry index, a road once per car"""
    E = cnt.shape[0]
    off = np.zeros(E + 1, np.int64)
    off[1:] = np.cumsum(cnt.sum(axis=1))
    return off, np.repeat(np.tile(np.asarray(entrypoints, np.int32), E), cnt.reshape(-1)).astype(np.int32)


def rows_of(cnt, rows, off):
    """... and the archetype row of every one of those cars (rows [E, n_entry, S]), env by env"""
    assert cnt.max() <= rows.shape[-1]
    flat = rows[np.arange(rows.shape[-1])[None, None, :] < cnt[:, :, None]].astype(np.int32)
    return np.split(flat, off[1:-1])


def arrival_counts(rng, T, E, n_entry, mean=0.08):
    return rng.poisson(mean, size=(T, E, n_entry)).clip(0, ROWS_PER_ROAD).astype(np.int32)


def load_both(eng, orc, state, phase, elapsed, arch=None, tab10=None):
    """tests/test_gpu_parity.py:load_both for any number of envs (and with archetype rows)"""
    import torch
    x, v, w, leading, lastcar = state
    eng.load_state(x, v, leading, lastcar, w=w, arch=arch)
    r, I = eng.r, eng.I
    obs = np.zeros((eng.E, eng.obs_len), np.int32)
    obs[:, 2 * r:2 * r + I] = phase
    obs[:, 2 * r + I:] = elapsed
    eng.obs.copy_(torch.as_tensor(obs))
    eng.waiting.zero_()
    eng.passed_dst.zero_()
    eng.rewards.zero_()
    if arch is None:
        load_oracle(orc, x, v, w, leading, lastcar)
    else:
        for k in range(eng.E):
            orc.load_planes(k, x[k], v[k], w[k], leading[k], lastcar[k], arch=arch[k], archetypes=tab10)
    orc.obs[:] = obs
    orc.waiting[:] = 0
    orc.passed_dst[:] = 0
    orc.rewards[:] = 0
    orc.n_trips[:] = 0
    if eng.n_trips is not None:
        eng.n_trips.zero_()


def assert_rows_and_trips(eng, orc, tab10, where):
    """what assert_same_state leaves out: every live car's archetype row, the trip log of validate mode"""
    if eng.het:
        ld, lc = eng.leading.cpu().numpy(), eng.lastcar.cpu().numpy()
        a = eng.arch.cpu().numpy()
        for k in range(eng.E):
            live = live_mask(ld[k], lc[k], eng.C)
            assert np.array_equal(a[k][live], orc.arch_plane(k, tab10)[live]), "rows env %d %s" % (k, where)
    if eng.n_trips is not None:
        nt = eng.n_trips.cpu().numpy()
        assert np.array_equal(nt, orc.n_trips), "n_trips " + where
        tt = eng.trip_times.cpu().numpy()
        for k in range(eng.E):
            kk = min(int(nt[k]), eng.trip_cap)
            assert np.array_equal(tt[k, :kk], orc.trip_times[k, :kk]), "trip_times env %d %s" % (k, where)


def assert_same_state_wide(eng, orc, where):
    """assert_same_state without its loop over the envs (2309 of them): the same words and the same live cars"""
    ld, lc = eng.leading.cpu().numpy(), eng.lastcar.cpu().numpy()
    for name, got in (("leading", ld), ("lastcar", lc), ("obs", eng.obs.cpu().numpy()), ("rewards", eng.rewards.cpu().numpy()),
                      ("waiting", eng.waiting.cpu().numpy()), ("passed_dst", eng.passed_dst.cpu().numpy())):
        want = getattr(orc, name)
        bad = np.nonzero((got != want).reshape(eng.E, -1).any(axis=1))[0]
        assert bad.size == 0, "%s: %d envs differ, first %s %s" % (name, bad.size, bad[:8], where)
    assert_cars_wide(eng, orc, ld, lc, where)


def assert_cars_wide(eng, orc, ld, lc, where):
    live = live_all(ld, lc, eng.C)
    planes = eng.planes_numpy()
    for name, got, want in (("x", planes[0], orc.x), ("v", planes[1], orc.v), ("w", planes[2], orc.w)):
        if name == "w" and eng.w is None:
            continue
        got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
        same = (got.view(np.int32) == want.view(np.int32)) | (np.isnan(got) & np.isnan(want))
        bad = np.nonzero((~same & live).reshape(eng.E, -1).any(axis=1))[0]
        assert bad.size == 0, "%s: %d envs differ, first %s %s" % (name, bad.size, bad[:8], where)
    idx = ld[:, :, None].astype(np.int64)
    assert same_bits(np.take_along_axis(planes[0], idx, axis=2), np.take_along_axis(orc.x, idx, axis=2)), "leader x " + where


# ---- plain calls -------------------------------------------------------------------------------------------------------------
def run_plain_calls(eng, seed, sorted_x, kernel_after, calls=CALLS, spawn_mean=0.08):
    """A fresh ragged state per call, per-env per-tick actions and arrivals, every env against the oracle after every
    call.  kernel_after(T) -> the mover of a T-tick call's last tick.  -> the oracle (for what the caller asserts)."""
    rng = np.random.RandomState(seed)
    E, C = eng.E, eng.C
    tab10 = tab10_of(eng.archetypes) if eng.het else None
    orc = OracleEnv(M, N, LENGTH, C, eng.dest, eng.phases, eng.nexts, n_envs=E, rate=RATE, validate=eng.validate)
    eng.reset_counters()
    overflowed = 0
    for trial, T in enumerate(calls):
        state = ragged_state(rng, E, eng.R, C, LENGTH, crowd=rng.choice([0.3, 0.8]), beyond=rng.choice(BEYOND), sorted_x=sorted_x)
        arch = rng.randint(0, len(tab10), size=state[0].shape).astype(np.uint8) if eng.het else None
        phase = rng.randint(2, size=(E, eng.I)).astype(np.int32)
        elapsed = rng.randint(0, 12, size=(E, eng.I)).astype(np.int32)
        load_both(eng, orc, state, phase, elapsed, arch, tab10)
        eng.set_tick(60)
        orc.steps[:] = 60
        acts = rng.randint(2, size=(T, E, eng.I)).astype(np.int32)
        cnt = arrival_counts(rng, T, E, eng.n_entry, spawn_mean)
        rows = rng.randint(0, len(tab10), size=(T, E, eng.n_entry, ROWS_PER_ROAD)).astype(np.uint8) if eng.het else None
        eng.set_actions(acts, per_tick=True)
        eng.set_spawns(counts=cnt, per_tick=True, rows=rows)
        eng.step(T)
        done = np.zeros(E, bool)
        for t in range(T):
            off, roads = csr(cnt[t], eng.entrypoints)
            spawn_arch = rows_of(cnt[t], rows[t], off) if eng.het else None
            done |= orc.step(acts[t], (off, roads), spawn_arch=spawn_arch, archetypes=tab10)[2].astype(bool)
        where = "call %d (%d ticks)" % (trial, T)
        overflowed += int(done.sum())
        assert np.array_equal(eng.done.cpu().numpy().astype(bool), done), "done " + where
        assert_same_state(eng, orc, where)
        assert_rows_and_trips(eng, orc, tab10, where)
        assert eng.tick == device_tick(eng) == 60 + T, where
        got, want = eng.vehicle_updates(), orc.vehicle_updates
        assert got == want, "vehicle updates %d / %d %s" % (got, want, where)
        assert eng.step_kernel() == kernel_after(T), (eng.step_kernel(), where)
    assert overflowed > 0 and eng.fused_ticks()[0] == 0
    return orc


def paired(calls=CALLS):
    return sum(2 * (T // 2) for T in calls)


def assert_pair_counters(eng, tail, split, calls=CALLS):
    assert eng.pair_ticks() == paired(calls)
    assert eng.tail_ticks() == (paired(calls) if tail else 0)
    assert eng.split_ticks() == (sum(T for T in calls if T >= 2) if split else 0)


def mover_engine(kind, follow, cap, C=None):
    """kind: plain (C = 10) | validate (the W forms, C = 34) | het (the HET forms, three rows, C = 10)"""
    knobs = dict(PAIRS, **FOLLOW[follow])
    if kind == "validate":
        return make_engine(knobs, E_A, C or 34, cap, planes=3, validate=True)
    if kind == "het":
        return make_engine(knobs, E_A, C or 10, cap, planes=3, archetypes=TAB8)
    return make_engine(knobs, E_A, C or 10, cap, planes=2)


@gpu
@pytest.mark.parametrize("sorted_x", [True, False])
@pytest.mark.parametrize("kind,follow,cap", [(k, f, 2) for k in ("plain", "validate", "het") for f in ("tail", "launches", "split")] +
                         [("plain", "tail", 3), ("plain", "launches", 1)])
def test_two_tick_pass_goes_round(kind, follow, cap, sorted_x):
    """k_move_tt (pairs forced) in its plain, W and HET forms, with k_tail, with k_advance / k_edge / k_advance, and with
    k_tail in two halves behind it; a call's odd last tick on k_move_ts (HET: the one-tick form of k_move_tt)."""
    eng = mover_engine(kind, follow, cap)
    tiles = tiles_of(eng)
    assert (eng.E, eng.R, eng.I, eng.n_entry, tiles) == (11, 142, 30, 22, 33)
    if follow == "split":
        # each half on its own: the pass at least twice round, k_tail (5 and 6 envs) three times
        assert rounds((eng.E // 2) * 3, 4, cap) >= 2 and rounds(eng.E // 2, 1, cap) >= 3
    else:
        assert rounds(tiles, 4, cap) >= 3                                     # k_move_tt, k_edge
        if follow == "tail":
            assert rounds(eng.E, 1, cap) >= 3                                 # k_tail
        elif cap == 1:
            assert rounds(eng.E * (eng.I + eng.n_entry), 256, cap) >= 3       # k_advance
        assert kind == "het" or rounds(tiles, 1, cap) >= 3                    # k_move_ts (a call's odd tick)
    run_plain_calls(eng, 2000 + 7 * cap + len(kind) + int(sorted_x), sorted_x,
                    lambda T: "k_move_tt" if (T % 2 == 0 or kind == "het") else "k_move_ts")
    assert_pair_counters(eng, follow != "launches", follow == "split")


@gpu
@pytest.mark.parametrize("follow", ["tail", "launches"])
@pytest.mark.parametrize("validate", [False, True])
@pytest.mark.parametrize("S,C", [(2, 34), (4, 34), (8, 66)])
def test_segmented_pass_goes_round(S, C, validate, follow):
    """k_move_tts (TFX_TT_SEG=2): a tile's walk over S wavefronts with TtsShare in LDS reused from tile to tile.  A
    segment is 8 cars or more, so at crowd 0.8 and in every full ring all S segments of a column hold cars."""
    knobs = dict(PAIRS, TFX_TT_SEG="2", TFX_TT_SEGS=str(S), **FOLLOW[follow])
    eng = make_engine(knobs, E_A, C, 2, planes=3 if validate else 2, validate=validate)
    groups = (tiles_of(eng) + 1) // 2 if S == 2 else tiles_of(eng)
    assert rounds(groups, 1, 2) >= 3 and (C - 2) // S >= 8
    if follow == "tail":
        assert rounds(eng.E, 1, 2) >= 3
    run_plain_calls(eng, 3000 + S + C + int(validate), bool(S & 4), lambda T: "k_move_tts" if T % 2 == 0 else "k_move_ts")
    assert_pair_counters(eng, follow == "tail", False)


@gpu
@pytest.mark.parametrize("variant,kind,C,cap", [("90", "plain", 10, 2), ("90", "plain", 130, 2), ("90", "plain", 10, 3),
                                                ("90", "validate", 34, 2), ("91", "plain", 10, 2), ("91", "plain", 10, 3),
                                                ("91", "validate", 34, 2), ("91", "het", 10, 2)])
def test_tick_by_tick_movers_go_round(variant, kind, C, cap):
    """TFX_PAIRS=0: k_move_ts (TFX_MOVE_VARIANT=90; C = 130: its sixteen-segment form) and k_move_t (91; plain, W and
    HET), each followed by k_advance."""
    knobs = {"TFX_RESIDENT": "0", "TFX_PAIRS": "0", "TFX_MOVE_VARIANT": variant}
    extra = dict(planes=3, validate=True) if kind == "validate" else (dict(planes=3, archetypes=TAB8) if kind == "het" else dict(planes=2))
    eng = make_engine(knobs, E_A, C, cap, **extra)
    name = "k_move_ts" if variant == "90" else "k_move_t"
    assert rounds(tiles_of(eng), 1 if variant == "90" else 4, cap) >= 3
    run_plain_calls(eng, 4000 + int(variant) + C + cap, cap == 2, lambda T: name, calls=[3, 4, 2, 5, 1])
    assert eng.pair_ticks() == 0 and eng.split_ticks() == 0


@gpu
@pytest.mark.parametrize("variant,C,cap,name", [("2", 34, 2, "k_move_dma"), ("2", 66, 2, "k_move_dma"), ("26", 20, 3, "k_move_dma"),
                                                ("0", 11, 2, "k_move"), ("0", 11, 3, "k_move")])
def test_ring_layout_movers_go_round(variant, C, cap, name):
    """The ring layout: k_move_dma in its forms for C = 34 and C = 66 and with the capacity read at run time (C = 20), and
    the generic k_move at an odd capacity (a chunk of road groups per workgroup)."""
    eng = make_engine({"TFX_RESIDENT": "0", "TFX_MOVE_VARIANT": variant}, E_A, C, cap, layout="ring", planes=3)
    roads = eng.E * eng.R
    if name == "k_move_dma":
        assert rounds((roads + 63) // 64, 4, cap) >= 3
    else:
        assert rounds((roads + 3) // 4, 1, cap) >= 3
    assert rounds(roads, 256, cap) >= 3                                       # k_refresh / k_reset, a lane per road
    run_plain_calls(eng, 5000 + int(variant) + C + cap, C != 66, lambda T: name, calls=[3, 4, 2, 5, 1])
    assert eng.pair_ticks() == 0


# ---- agent steps -----------------------------------------------------------------------------------------------------------
ORC_FIELDS = ("state", "leading", "lastcar", "obs", "rewards", "waiting", "passed_dst", "n_trips", "trip_times")


def emulate_decision(orc, tick0, action, arrivals, n_ticks, remi, tab10=None, nthreads=1):
    """Repeater._step + Remi._step (traffic_test.py:27-64) for every env of a batched oracle, as
    tests/test_gpu_agent_step.py:emulate_agent_step does on single-env ones: an env whose tick overflows stands still for
    the rest of the decision (`if done: break`).  arrivals(t, frozen) -> (counts [E, n_entry], rows or None) of tick t.
    orc.entrypoints: the entry roads in entry-index order (the caller sets it).
    -> aobs, areward, adone, the tick of the decision at which each env ended (-1: it did not)."""
    E, r, I = orc.E, orc.r, orc.I
    aobs = np.zeros((E, 2 * r + I), np.float32)
    arew = np.zeros((E, I), np.float32)
    frozen = np.zeros(E, bool)
    ended_at = np.full(E, -1)
    for t in range(n_ticks):
        cnt, rows = arrivals(t, frozen)
        cnt = np.where(frozen[:, None], 0, cnt).astype(np.int32)
        keep = [getattr(orc, f)[frozen].copy() for f in ORC_FIELDS] if frozen.any() else None
        orc.steps[:] = tick0 + t                       # batched envs share one clock on the device
        off, roads = csr(cnt, orc.entrypoints)
        obs, rew, done = orc.step(action, (off, roads), nthreads=nthreads,
                                  spawn_arch=rows_of(cnt, rows, off) if rows is not None else None, archetypes=tab10)
        if keep is not None:
            for f, a in zip(ORC_FIELDS, keep):
                getattr(orc, f)[frozen] = a
        run = ~frozen
        aobs[run, :r] += obs[run, :r]
        aobs[run, r:2 * r] = obs[run, r:2 * r]
        aobs[run, -I:] = (obs[run, -I:] / 100 * (2 * obs[run, -2 * I:-I] - 1))
        arew[run] = arew[run] + rew[run]
        ended = run & done.astype(bool)
        ended_at[ended] = t
        frozen |= ended
    if remi:
        arew = orc.remi_reward().copy()
    return aobs, arew, frozen.astype(np.uint8), ended_at


def assert_decision(eng, orc, out, want, tab10, where):
    """what a decision returns and leaves behind, for every env (the engine's obs and rewards hold the decision's
    accumulations: its outputs are compared instead)"""
    aobs, arew, adone = [o.cpu().numpy() for o in out]
    assert np.array_equal(adone, want[2]), "adone %s: %s / %s" % (where, np.nonzero(adone)[0][:8], np.nonzero(want[2])[0][:8])
    bad = np.nonzero((aobs.view(np.int32) != want[0].view(np.int32)).any(axis=1))[0]
    assert bad.size == 0, "aobs: %d envs differ, first %s %s" % (bad.size, bad[:8], where)
    bad = np.nonzero((arew.view(np.int32) != want[1].view(np.int32)).any(axis=1))[0]
    assert bad.size == 0, "areward: %d envs differ, first %s %s" % (bad.size, bad[:8], where)
    ld, lc = eng.leading.cpu().numpy(), eng.lastcar.cpu().numpy()
    for name, got in (("leading", ld), ("lastcar", lc), ("waiting", eng.waiting.cpu().numpy()),
                      ("passed_dst", eng.passed_dst.cpu().numpy())):
        bad = np.nonzero((got != getattr(orc, name)).reshape(eng.E, -1).any(axis=1))[0]
        assert bad.size == 0, "%s: %d envs differ, first %s %s" % (name, bad.size, bad[:8], where)
    assert_cars_wide(eng, orc, ld, lc, where)
    assert_rows_and_trips(eng, orc, tab10, where)


def run_decisions(eng, seed, lengths, remi, per_state=3, full="none", crowd=(0.5, 0.8), spawn_mean=0.12):
    """Decisions from ragged states without full rings - envs overflow, and freeze, one after another rather than all at
    once - under a held random action and per-tick arrival counts; every env against the emulation after every decision
    (an env that ended simply goes on in the next one, as a caller that does not reset it would)."""
    rng = np.random.RandomState(seed)
    E, C = eng.E, eng.C
    tab10 = tab10_of(eng.archetypes) if eng.het else None
    orc = OracleEnv(M, N, LENGTH, C, eng.dest, eng.phases, eng.nexts, n_envs=E, rate=RATE, validate=eng.validate)
    orc.entrypoints = eng.entrypoints
    ends = []
    for trial, T in enumerate(lengths):
        state = ragged_state(rng, E, eng.R, C, LENGTH, crowd=rng.choice(crowd), beyond=rng.choice(BEYOND[:3]),
                             sorted_x=bool(trial % 2), full=full, entry_roads=eng.entrypoints)
        arch = rng.randint(0, len(tab10), size=state[0].shape).astype(np.uint8) if eng.het else None
        phase = rng.randint(2, size=(E, eng.I)).astype(np.int32)
        load_both(eng, orc, state, phase, rng.randint(0, 12, size=(E, eng.I)).astype(np.int32), arch, tab10)
        eng.set_tick(40)
        for step in range(per_state):
            act = rng.randint(2, size=(E, eng.I)).astype(np.int32)
            cnt = arrival_counts(rng, T, E, eng.n_entry, spawn_mean)
            rows = rng.randint(0, len(tab10), size=(T, E, eng.n_entry, ROWS_PER_ROAD)).astype(np.uint8) if eng.het else None
            eng.set_actions(act)
            eng.set_spawns(counts=cnt, per_tick=True, rows=rows)
            tick0 = eng.tick
            out = eng.agent_step(T, remi=remi)
            want = emulate_decision(orc, tick0, act, lambda t, frozen: (cnt[t], rows[t] if rows is not None else None), T, remi, tab10)
            where = "state %d decision %d (%d ticks)" % (trial, step, T)
            assert_decision(eng, orc, out, want, tab10, where)
            assert eng.tick == device_tick(eng) == tick0 + T, where
            ends.append(want[3])
    ends = np.stack(ends)
    # envs ended, at different ticks of a decision, next to envs that ran on
    assert (ends >= 0).any() and len(set(ends[ends >= 0].tolist())) >= 2 and ((ends >= 0).any(axis=1) & (ends < 0).any(axis=1)).any()
    return ends


@gpu
@pytest.mark.parametrize("remi", [True, False])
@pytest.mark.parametrize("kind,follow,graph", [("plain", "tail", "1"), ("plain", "launches", "1"), ("plain", "tail", "0"),
                                               ("het", "tail", "1"), ("het", "launches", "0"), ("validate", "tail", "1")])
def test_agent_steps_go_round(kind, follow, graph, remi):
    """tfx_agent_step over the pairs under the cap: k_risk, the AGENT forms of the pass, of k_tail and of k_edge, the
    restricted one-tick pass, k_agent_tail - decisions of 4 and 5 ticks, through the captured graph and eagerly."""
    knobs = dict(PAIRS, TFX_GRAPH=graph, **FOLLOW[follow])
    extra = dict(planes=3, validate=True) if kind == "validate" else (dict(planes=3, archetypes=TAB8) if kind == "het" else dict(planes=2))
    eng = make_engine(knobs, E_A, 10, 2, **extra)
    assert rounds(tiles_of(eng), 4, 2) >= 3                                   # k_risk, k_move_tt, k_edge
    assert rounds(eng.E * (2 * eng.r + eng.I), 256, 2) >= 3                   # k_agent_tail
    if follow == "tail":
        assert rounds(eng.E, 1, 2) >= 3                                       # k_tail
    run_decisions(eng, 6000 + len(kind) + len(follow) + int(graph) + 2 * int(remi), [4, 5, 4, 5], remi)
    assert eng.pair_ticks() == 3 * (4 + 4 + 4 + 4) and eng.tail_ticks() == 0 and eng.fused_ticks()[0] == 0


# ---- inputs made on the device -------------------------------------------------------------------------------------------
def greedy_actions(orc):
    c = orc.cars_on_roads()                                                   # [E, m, n, 4]
    return (c.reshape(orc.E, orc.I, 4).dot([1, 1, -1, -1]) < 0).astype(np.int32)


def device_inputs_engine(E, cap, het, pairs, stream, cpt, seed, spacing):
    from gym_traffic.devrng import PoissonMirror, RegularMirror
    knobs = dict(PAIRS) if pairs else {"TFX_RESIDENT": "0", "TFX_PAIRS": "0"}
    eng = make_engine(knobs, E, 10, cap, **(dict(planes=3, archetypes=TAB8) if het else dict(planes=2)))
    eng.set_poisson(cpt, seed=seed) if stream == "poisson" else eng.set_regular(cpt, seed=seed)
    eng.set_greedy(spacing)
    mirror = (PoissonMirror if stream == "poisson" else RegularMirror)(
        cpt, seed, eng.n_entry, range(E), **(dict(n_archetypes=len(TAB8), per_road=eng.C - 2) if het else {}))
    return eng, mirror


def start_device_inputs(eng, rng):
    """a ragged state without full rings at tick 0 (the greedy controller decides at ticks that are multiples of its spacing)"""
    tab10 = tab10_of(eng.archetypes) if eng.het else None
    orc = OracleEnv(M, N, LENGTH, eng.C, eng.dest, eng.phases, eng.nexts, n_envs=eng.E, rate=RATE)
    state = ragged_state(rng, eng.E, eng.R, eng.C, LENGTH, crowd=0.4, beyond=0.05, sorted_x=True, full="none")
    arch = rng.randint(0, len(TAB8), size=state[0].shape).astype(np.uint8) if eng.het else None
    load_both(eng, orc, state, rng.randint(2, size=(eng.E, eng.I)).astype(np.int32),
              rng.randint(0, 12, size=(eng.E, eng.I)).astype(np.int32), arch, tab10)
    eng.set_tick(0)
    orc.steps[:] = 0
    return orc, tab10


def mirror_tick(mirror, het, frozen_ids=()):
    got = mirror.next_tick(frozen=frozen_ids) if frozen_ids else mirror.next_tick()
    cnt, rows = got if het else (got, None)
    if rows is not None and rows.shape[-1] < int(cnt.max()):                  # cars past the S rows held per road: row 0
        rows = np.concatenate([rows, np.zeros(rows.shape[:2] + (int(cnt.max()) - rows.shape[-1],), np.uint8)], axis=2)
    return cnt, rows


@gpu
@pytest.mark.parametrize("stream,het,pairs", [("poisson", False, True), ("poisson", True, True), ("poisson", False, False),
                                              ("regular", False, True)])
def test_device_inputs_in_plain_calls_go_round(stream, het, pairs):
    """set_poisson / set_regular + set_greedy in tfx_step: k_poisson generates a call's arrivals up front (11 envs: six
    rounds of envs, s_hist / s_seq / s_first reused), k_greedy and the greedy decision of the advance under the cap -
    against the host mirrors of gym_traffic.devrng and the controller's rule."""
    run_device_inputs_in_plain_calls(stream, het, pairs, 2, 71 + int(het) + 2 * int(pairs))


# Found by the cases above (not by the cap): a ragged state sends envs through the serial advance, whose one lane wrote
# the greedy controller's decisions for the NEXT tick into the buffer the env's lanes read THIS tick's action from - the
# stored phase then switched a tick before the cars saw it (csrc/tfx_advance.hpp:advance_item).  The seeds that showed
# it, on the shipped grids: 74 (k_tail<GREEDY, HET>, obs differed after 16 ticks) and 71 (k_advance<GREEDY>, after 28).
GREEDY_ON_THE_SERIAL_ADVANCE = [(74, True, True), (71, False, False)]


@gpu
@pytest.mark.parametrize("seed,het,pairs", GREEDY_ON_THE_SERIAL_ADVANCE)
def test_regression_greedy_decides_on_the_serial_advance(seed, het, pairs):
    run_device_inputs_in_plain_calls("poisson", het, pairs, None, seed)


def run_device_inputs_in_plain_calls(stream, het, pairs, cap, seed):
    spacing = 3
    eng, mirror = device_inputs_engine(E_A, cap, het, pairs, stream, 2.2, 0xC0FFEE1234, spacing)
    assert cap is None or rounds(eng.E, 1, cap) >= 3                          # k_poisson, k_tail
    orc, tab10 = start_device_inputs(eng, np.random.RandomState(seed))
    act, t, cars = np.zeros((eng.E, eng.I), np.int32), 0, 0
    for T in CALLS + [8]:
        eng.step(T)
        for _ in range(T):
            if t % spacing == 0:
                act = greedy_actions(orc)
            cnt, rows = mirror_tick(mirror, het)
            cars += int(cnt.sum())
            off, roads = csr(cnt, eng.entrypoints)
            orc.step(act, (off, roads), spawn_arch=rows_of(cnt, rows, off) if het else None, archetypes=tab10)
            t += 1
        where = "%s at tick %d" % (stream, t)
        assert_same_state(eng, orc, where)
        assert_rows_and_trips(eng, orc, tab10, where)
        assert eng.tick == device_tick(eng) == t, where
    assert cars > eng.E * t
    assert eng.pair_ticks() == (paired(CALLS + [8]) if pairs else 0)
    assert eng.tail_ticks() == (paired(CALLS + [8]) if pairs else 0)          # (generated up front: k_tail stays)


@gpu
@pytest.mark.parametrize("E,cap,het,pairs", [(E_A, 2, False, True), (E_A, 2, True, True), (E_A, 2, False, False), (18, 1, False, True)])
def test_device_inputs_in_agent_steps_go_round(E, cap, het, pairs):
    """... and inside agent steps, where k_poisson runs tick by tick and a frozen env's stream stands still.  Decisions
    of 6 ticks with the controller deciding every 3: each decision begins with a decision of k_greedy.  18 envs at cap 1:
    the three rounds of k_remi's rule in k_agent_tail's first 540 elements and of k_greedy (a lane per intersection)."""
    spacing, T = 3, 6
    eng, mirror = device_inputs_engine(E, cap, het, pairs, "poisson", 3.3, 0xABCDE12345, spacing)
    assert rounds(eng.E, 1, cap) >= 3                                         # k_poisson
    if E > E_A:
        assert rounds(eng.E * eng.I, 256, cap) >= 3                           # k_greedy
    orc, tab10 = start_device_inputs(eng, np.random.RandomState(83 + E + int(het) + 2 * int(pairs)))
    orc.entrypoints = eng.entrypoints
    held = [np.zeros((E, eng.I), np.int32)]
    ended = 0
    for dec in range(6):
        tick0 = eng.tick
        out = eng.agent_step(T, remi=True)

        # (the action differs from tick to tick here: the emulation runs the decision in spans of one greedy period)
        want_obs = np.zeros((E, 2 * eng.r + eng.I), np.float32)
        frozen = np.zeros(E, bool)
        for t0 in range(0, T, spacing):
            held[0] = np.where(frozen[:, None], held[0], greedy_actions(orc))

            def arrivals(t, fr):
                return mirror_tick(mirror, het, frozenset(int(k) for k in np.nonzero(fr | frozen)[0]))
            keep = [getattr(orc, f)[frozen].copy() for f in ORC_FIELDS]
            aobs, arew, adone, _ = emulate_decision(orc, tick0 + t0, held[0], arrivals, spacing, False, tab10)
            for f, a in zip(ORC_FIELDS, keep):
                getattr(orc, f)[frozen] = a
            run = ~frozen
            want_obs[run, :eng.r] += aobs[run, :eng.r]
            want_obs[run, eng.r:] = aobs[run, eng.r:]
            frozen |= adone.astype(bool)
        want = (want_obs, orc.remi_reward().copy(), frozen.astype(np.uint8))
        ended += int(frozen.sum())
        assert_decision(eng, orc, out, want, tab10, "decision %d" % dec)
        assert eng.tick == device_tick(eng) == tick0 + T
    assert eng.pair_ticks() == (6 * T if pairs else 0) and eng.tail_ticks() == 0
    print("envs that ended a decision early:", ended)


# ---- clones, episodes, warm restarts -------------------------------------------------------------------------------------
@gpu
def test_clones_go_round():
    """k_clone under the cap (33 tiles: five rounds): a fan-out in place, a snapshot onto a second handle and the way
    back, each held to the source's bits; the restored envs then run on as the oracle says."""
    from test_gpu_clone import assert_env_equal, snapshot
    rng = np.random.RandomState(909)
    eng = make_engine(PAIRS, E_A, 10, 2, planes=3, validate=True)
    spare = make_engine(PAIRS, E_A, 10, 2, planes=3, validate=True)
    assert rounds(tiles_of(eng), 4, 2) >= 3
    orc = OracleEnv(M, N, LENGTH, 10, eng.dest, eng.phases, eng.nexts, n_envs=E_A, rate=RATE, validate=True)
    state = ragged_state(rng, E_A, eng.R, 10, LENGTH, crowd=0.6, beyond=0.4, sorted_x=False)
    phase = rng.randint(2, size=(E_A, eng.I)).astype(np.int32)
    elapsed = rng.randint(0, 12, size=(E_A, eng.I)).astype(np.int32)
    load_both(eng, orc, state, phase, elapsed)
    eng.set_tick(60)
    spare.reset(np.zeros((E_A, eng.I), np.int32))
    spare.set_tick(60)
    before = snapshot(eng)
    src = np.array([-1, 0, 0, 5, -1, -1, 5, 10, 0, 10, -1], np.int32)         # fan-outs across tiles, envs and halves
    mapped = np.where(src >= 0, src, np.arange(E_A))
    eng.clone_envs(src)
    assert eng.clone_skipped() == 0
    now = snapshot(eng)
    for k in range(E_A):
        assert_env_equal(now, k, before, mapped[k], "in place")
    back = np.arange(E_A, dtype=np.int32)[::-1].copy()
    spare.clone_envs(back, source=eng)
    kept = snapshot(spare)
    for k in range(E_A):
        assert_env_equal(kept, k, now, back[k], "on the second handle")
    eng.set_spawns(period=2)
    eng.set_actions(cycle_period=3)
    eng.step(5)                                                               # the first handle runs on and loses the state
    eng.set_tick(60)
    eng.clone_envs(back, source=spare)
    again = snapshot(eng)
    for k in range(E_A):
        assert_env_equal(again, k, now, k, "restored", stamps=False)
    # ... and continues from there as the oracle does from the same state
    load_oracle(orc, *[a[mapped] for a in state])
    obs = np.zeros((E_A, eng.obs_len), np.int32)
    obs[:, 2 * eng.r:2 * eng.r + eng.I] = phase[mapped]
    obs[:, 2 * eng.r + eng.I:] = elapsed[mapped]
    assert np.array_equal(again[0]["obs"], obs)
    orc.obs[:] = obs
    orc.steps[:] = 60
    eng.n_trips.zero_()
    T = 6
    acts = rng.randint(2, size=(T, E_A, eng.I)).astype(np.int32)
    cnt = arrival_counts(rng, T, E_A, eng.n_entry)
    eng.set_actions(acts, per_tick=True)
    eng.set_spawns(counts=cnt, per_tick=True)
    eng.step(T)
    for t in range(T):
        orc.step(acts[t], csr(cnt[t], eng.entrypoints))
    assert_same_state(eng, orc, "after the restore")
    assert_rows_and_trips(eng, orc, None, "after the restore")


def episode_shape(monkeypatch):
    """the helpers of tests/test_gpu_episodes.py / test_gpu_warm_pool.py on this module's shape, pairs + k_tail, cap 2"""
    import test_gpu_episodes as ep
    ep.force_path(monkeypatch, "pairs")
    monkeypatch.setenv("TFX_SPLIT", "0")
    monkeypatch.setenv("TFX_GRID_CAP", "2")
    for k, val in dict(m=M, n=N, L=LENGTH, T=5, E=E_A).items():
        monkeypatch.setitem(ep.GRID, k, val)
    monkeypatch.setattr(ep.make_engine, "__defaults__", (E_A, 0))             # (its default E was taken from GRID at import)
    # every episode ends by the time limit at the latest: every env restarts, twice; arrivals every 3 ticks on every entry road
    return dict(C=10, period=3, M=3, K=8)


@gpu
def test_episodes_go_round(monkeypatch):
    """tfx_set_episodes under the cap: k_episode_begin (1562 roads: four rounds) and the accounting in k_agent_tail,
    against the manual loop agent_step(); reset_envs(...) on a second handle (tests/test_gpu_episodes.py:run_equivalence)."""
    import test_gpu_episodes as ep
    sc = episode_shape(monkeypatch)
    n_term, n_trunc, n_restart, n_cars, a, _ = ep.run_equivalence(sc)
    assert (a.E, a.R) == (E_A, 142) and rounds(a.E * a.R, 256, 2) >= 3
    assert n_cars > 20 and (n_restart >= 2).all() and (n_term + n_trunc >= 2).all()
    assert a.pair_ticks() == sc["K"] * 4
    print("episodes: ends by overflow %s, by the time limit %s" % (n_term.tolist(), n_trunc.tolist()))


@gpu
def test_warm_restarts_go_round(monkeypatch):
    """tfx_set_episode_pool under the cap: the masked restart as k_clone<true> (33 tiles: five rounds), against the manual
    loop agent_step(); clone_envs(where(end, slots, -1), source=pool) (tests/test_gpu_warm_pool.py:run_warm)."""
    import test_gpu_warm_pool as wp
    sc = episode_shape(monkeypatch)
    o = wp.run_warm(sc)
    assert (o["a"].E, o["a"].R) == (E_A, 142) and rounds(tiles_of(o["a"]), 4, 2) >= 3
    assert o["cars"] > 20 and (o["restart"] >= 2).all() and o["same"] and o["diff"]
    print("warm restarts: ends by overflow %s, by the time limit %s" % (o["term"].tolist(), o["trunc"].tolist()))


# ---- the hook itself -------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("E", [E_A, 600])
def test_grid_cap_unset_is_grid_cap_zero(E):
    """With TFX_GRID_CAP unset or 0 every grid is the one the handle sizes on its own: tfx_launch_info,
    tfx_measure_launch and tfx_cells_launch report the same numbers either way, at a small and at a mid size - and the
    numbers of the plan as it stood before the hook; a cap applies to each, TFX_MEASURE_GRID keeps priority for its two."""
    import torch
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    seen = {}
    for name, knobs in (("unset", {}), ("zero", {"TFX_GRID_CAP": "0"}), ("cap", {"TFX_GRID_CAP": "2"}),
                        ("both", {"TFX_GRID_CAP": "2", "TFX_MEASURE_GRID": "5"})):
        eng = make_engine(dict(knobs, TFX_RESIDENT="0"), E, 10, planes=2)
        eng.reset(np.zeros((E, eng.I), np.int32))
        eng.step(1)
        seen[name] = (eng.launch_info(), eng.measure_launch(), eng.cells_launch(8))
    assert seen["unset"] == seen["zero"]
    tiles = E * 3
    info, measure, cells = seen["unset"]
    want = min((tiles + 3) // 4, n_cu * 16)
    assert measure == cells == (want, 4 * want)
    assert info["grid"] > 2 and (tiles > 2 * n_cu or info["grid"] == min(tiles, n_cu * 8))    # (k_move_ts: a workgroup per tile)
    assert seen["cap"][0]["grid"] == 2 and seen["cap"][1] == seen["cap"][2] == (2, 8)
    assert seen["both"][0]["grid"] == 2 and seen["both"][1] == seen["both"][2] == (5, 20)


# ---- part B: one wide ragged batch on the shipped defaults --------------------------------------------------------------
WIDE_CALLS = [2, 5, 1, 8]
_WIDE = {}


def wide_inputs(kind):
    """The states, actions and arrivals of a part-B case, made once: "calls" (a and b; full rings allowed) or
    "decisions" (c: crowd 0.3, beyond 0.4, no full rings)."""
    if kind not in _WIDE:
        dest, phases, nexts, entry = grid_tables()
        rng = np.random.RandomState(2309 if kind == "calls" else 9032)
        R, I = len(dest), M * N
        if kind == "calls":
            state = ragged_state(rng, E_B, R, 10, LENGTH, crowd=0.5, beyond=0.4, sorted_x=False)
        else:
            state = ragged_state(rng, E_B, R, 10, LENGTH, crowd=0.3, beyond=0.4, sorted_x=True, full="none")
        T = sum(WIDE_CALLS) + 8
        _WIDE[kind] = dict(state=state, phase=rng.randint(2, size=(E_B, I)).astype(np.int32),
                           elapsed=rng.randint(0, 12, size=(E_B, I)).astype(np.int32),
                           acts=rng.randint(2, size=(T, E_B, I)).astype(np.int32),
                           cnt=rng.poisson(0.1, size=(T, E_B, len(entry))).astype(np.int32))
    return _WIDE[kind]


def wide_start(knobs, kind):
    inp = wide_inputs(kind)
    eng = make_engine(knobs, E_B, 10, planes=2)
    assert (eng.E, eng.R, eng.n_entry) == (E_B, 142, 22)
    orc = OracleEnv(M, N, LENGTH, 10, eng.dest, eng.phases, eng.nexts, n_envs=E_B, rate=RATE)
    orc.entrypoints = eng.entrypoints
    load_both(eng, orc, inp["state"], inp["phase"], inp["elapsed"])
    eng.set_tick(60)
    orc.steps[:] = 60
    eng.reset_counters()
    return eng, orc, inp


def wide_calls(eng, orc, inp):
    t = 0
    for T in WIDE_CALLS:
        eng.set_actions(inp["acts"][t:t + T], per_tick=True)
        eng.set_spawns(counts=inp["cnt"][t:t + T], per_tick=True)
        eng.step(T)
        done = np.zeros(E_B, bool)
        for j in range(t, t + T):
            done |= orc.step(inp["acts"][j], csr(inp["cnt"][j], eng.entrypoints), nthreads=8)[2].astype(bool)
        t += T
        where = "after %d ticks" % t
        assert np.array_equal(eng.done.cpu().numpy().astype(bool), done), "done " + where
        assert_same_state_wide(eng, orc, where)
        assert eng.tick == device_tick(eng) == 60 + t and eng.vehicle_updates() == orc.vehicle_updates, where
    return t


def wide_decisions(eng, orc, inp, t, n_decisions):
    ended = np.zeros(E_B, bool)
    for dec in range(n_decisions):
        act, cnt = inp["acts"][t], inp["cnt"][t:t + 4]
        eng.set_actions(act)
        eng.set_spawns(counts=cnt, per_tick=True)
        tick0 = eng.tick
        out = eng.agent_step(4, remi=True)
        want = emulate_decision(orc, tick0, act, lambda j, frozen: (cnt[j], None), 4, True, nthreads=8)
        assert_decision(eng, orc, out, want, None, "decision %d" % dec)
        ended |= want[2].astype(bool)
        t += 4
    return ended


@gpu
def test_wide_batch_no_switch_set():
    """(a) No TFX_* variable set: these envs fit k_res and take it with its default packing - plain calls, then two
    4-tick decisions with remi."""
    eng, orc, inp = wide_start({}, "calls")
    assert eng.fused_ticks() == (0, True)
    t = wide_calls(eng, orc, inp)
    assert eng.step_kernel() == "k_res" and eng.fused_ticks() == (t, True)
    ended = wide_decisions(eng, orc, inp, t, 2)
    assert eng.step_kernel() == "k_res" and eng.fused_ticks() == (t + 8, True)
    assert eng.pair_ticks() == 0 and eng.split_ticks() == 0
    print("envs that ended a decision: %d of %d" % (int(ended.sum()), E_B))


@gpu
def test_wide_batch_plain_calls_per_tick_kernels():
    """(b) TFX_RESIDENT=0 only: on the 256 compute units of an MI355X the handle's own choice is pairs + k_tail + two
    halves (1154 and 1155 envs) on two streams; states hold full rings, and plain calls run on through overflow."""
    eng, orc, inp = wide_start({"TFX_RESIDENT": "0"}, "calls")
    assert eng.fused_ticks() == (0, False)
    wide_calls(eng, orc, inp)
    assert eng.pair_ticks() == 2 + 4 + 8 and eng.tail_ticks() == 2 + 4 + 8 and eng.split_ticks() == 2 + 5 + 8
    assert eng.step_kernel() == "k_move_tt" and eng.fused_ticks()[0] == 0


def reference_ends_of_wide_decisions():
    """The oracle alone through case (c): which envs end at some decision"""
    dest, phases, nexts, entry = grid_tables()
    inp = wide_inputs("decisions")
    orc = OracleEnv(M, N, LENGTH, 10, dest, phases, nexts, n_envs=E_B, rate=RATE)
    orc.entrypoints = entry
    load_oracle(orc, *inp["state"])
    orc.obs[:, 2 * orc.r:2 * orc.r + orc.I] = inp["phase"]
    orc.obs[:, 2 * orc.r + orc.I:] = inp["elapsed"]
    ended, first = np.zeros(E_B, bool), None
    for dec in range(4):
        t = 4 * dec
        cnt = inp["cnt"][t:t + 4]
        want = emulate_decision(orc, 60 + t, inp["acts"][t], lambda j, frozen: (cnt[j], None), 4, True, nthreads=8)
        ended |= want[2].astype(bool)
        first = first if first is not None else float(want[2].mean())
    return ended, first


def test_wide_decisions_reference_is_inside_the_band():
    """CPU: the condition of case (c) on the oracle - at the end of the 16 ticks between 5 % and 50 % of the envs have
    ended at some decision, so frozen envs and running envs share workgroups (with a tenth of the rings full nearly
    every env ends within two ticks: hence states without full rings)."""
    ended, first = reference_ends_of_wide_decisions()
    print("ended in the first decision %.3f, at some decision %.3f" % (first, ended.mean()))
    assert 0.05 <= ended.mean() <= 0.50 and first < ended.mean()


@gpu
def test_wide_batch_decisions_per_tick_kernels():
    """(c) TFX_RESIDENT=0 only: four 4-tick decisions with remi from states without full rings; the halves of the split
    hold frozen envs next to running ones."""
    eng, orc, inp = wide_start({"TFX_RESIDENT": "0"}, "decisions")
    ended = wide_decisions(eng, orc, inp, 0, 4)
    assert 0.05 <= ended.mean() <= 0.50, ended.mean()
    assert eng.pair_ticks() == 16 and eng.split_ticks() == 16 and eng.tail_ticks() == 0 and eng.fused_ticks()[0] == 0
    assert eng.step_kernel() == "k_move_tt"
