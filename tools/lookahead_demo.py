"""Lookahead control on cloned envs (tfx_clone_envs): N live envs in one TrafficVecEnv, N x K branches in a second.

Every decision: the branches take the live envs' states, arrival streams included (branch n*K + k is a copy of live
env n: common random numbers - every candidate sees the cars the live env will see); candidate k of env n - hold the
phases, flip them all, the greedy rule of the reference (algorithms/greedy.py:14-16: phase 1 iff the N-S approaches hold
more cars than the E-W ones), random settings - is applied and held for H decisions; score = summed remi reward; the
live env takes the winner.  Prints the mean return per env against the greedy controller on the same seeds, and the
time per decision split into clone / branches / live step.

    python tools/lookahead_demo.py --envs 64 --candidates 8 --horizon 3 --decisions 60
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "traffic-env_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from gym_traffic.envs.vec_env import TrafficVecEnv  # noqa: E402


def greedy_actions(venv):
    """int32 [E, I]: algorithms/greedy.py:14-16 for every intersection of every env."""
    cars = venv.cars_on_roads().to(torch.int32)                       # [E, m, n, 4]: east-, west-, south-, northbound
    score = cars[..., 0] + cars[..., 1] - cars[..., 2] - cars[..., 3]
    return (score < 0).to(torch.int32).reshape(venv.num_envs, -1)


def candidates(venv, K, gen):
    """int32 [E, K, I]: hold, flip all, greedy, then random settings."""
    eng = venv.engine
    hold = (eng.current_phase != 0).to(torch.int32)
    c = [hold, 1 - hold, greedy_actions(venv)]
    while len(c) < K:
        c.append(torch.randint(0, 2, hold.shape, generator=gen, device=eng.device, dtype=torch.int32))
    return torch.stack(c[:K], dim=1).contiguous()


def make(envs, a, offset=0):
    return TrafficVecEnv(envs, a.m, a.n, a.length, capacity=a.capacity, spawn='device', seed=a.seed,
                         local_cars_per_sec=a.cars_per_sec, env_id_offset=offset)


def run(a):
    N, K, H, T = a.envs, a.candidates, a.horizon, a.ticks
    live, branches, base = make(N, a), make(N * K, a, offset=N), make(N, a)
    I = live.engine.I
    dev = live.engine.device
    ph = np.random.RandomState(a.seed).randint(2, size=(N, I)).astype(np.int32)
    for v in (live, base):
        v.reset(ph)
    branches.reset(np.zeros((N * K, I), np.int32))
    gen = torch.Generator(device=dev)
    gen.manual_seed(a.seed)
    src = (torch.arange(N * K, device=dev) // K).to(torch.int32)
    ret_live = torch.zeros(N, device=dev)
    ret_base = torch.zeros(N, device=dev)
    wins = torch.zeros(K, device=dev)
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range(a.decisions)]
    for d in range(a.decisions):
        cand = candidates(live, K, gen)                                # [N, K, I]
        ev[d][0].record()
        branches.clone_envs(src, source=live, streams=True, episodes=False)
        ev[d][1].record()
        score = torch.zeros(N * K, device=dev)
        flat = cand.reshape(N * K, I)
        for _ in range(H):
            _, rew, _ = branches.agent_step(flat, n_ticks=T)
            score += rew.sum(dim=1)
        best = score.reshape(N, K).argmax(dim=1)                       # (ties: the first - hold - wins)
        ev[d][2].record()
        _, rew, _ = live.agent_step(cand[torch.arange(N, device=dev), best], n_ticks=T)
        ev[d][3].record()
        ret_live += rew.sum(dim=1)
        wins += torch.bincount(best, minlength=K).to(wins.dtype)
        _, rew, _ = base.agent_step(greedy_actions(base), n_ticks=T)
        ret_base += rew.sum(dim=1)
    torch.cuda.synchronize()
    assert branches.engine.clone_skipped() == 0
    skip = min(3, a.decisions - 1)
    ms = np.array([[e[i].elapsed_time(e[i + 1]) for i in range(3)] for e in ev[skip:]])
    return dict(envs=N, candidates=K, horizon=H, decisions=a.decisions, ticks=T,
                lookahead_return=float(ret_live.mean()), greedy_return=float(ret_base.mean()),
                wins=[int(w) for w in wins.tolist()], clone_ms=float(np.median(ms[:, 0])),
                branches_ms=float(np.median(ms[:, 1])), live_ms=float(np.median(ms[:, 2])))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=64)
    ap.add_argument("--candidates", type=int, default=8)
    ap.add_argument("--horizon", type=int, default=3)
    ap.add_argument("--decisions", type=int, default=60)
    ap.add_argument("--ticks", type=int, default=10)
    ap.add_argument("--m", type=int, default=4)
    ap.add_argument("--n", type=int, default=4)
    ap.add_argument("--length", type=float, default=200.0)
    ap.add_argument("--capacity", type=int, default=34)
    ap.add_argument("--cars-per-sec", type=float, default=0.12)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    r = run(a)
    lines = ["lookahead demo: %d live envs (%dx%d grid, L=%g, C=%d), %d candidates x %d decisions ahead (%d branches), "
             "%d decisions of %d ticks" % (r["envs"], a.m, a.n, a.length, a.capacity, r["candidates"], r["horizon"],
                                           r["envs"] * r["candidates"], r["decisions"], r["ticks"]),
             "mean return per env (summed remi reward): lookahead %.2f   greedy controller %.2f"
             % (r["lookahead_return"], r["greedy_return"]),
             "winning candidate counts (hold, flip all, greedy, random...): %s" % r["wins"],
             "median ms per decision: clone %.3f   branches (%d decisions of %d envs) %.3f   live step %.3f"
             % (r["clone_ms"], r["horizon"], r["envs"] * r["candidates"], r["branches_ms"], r["live_ms"])]
    for ln in lines:
        print(ln)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n\n")
    return r


if __name__ == "__main__":
    main()
