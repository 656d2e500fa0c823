"""Mean travel time of two controllers, kept on the device (TrafficVecEnv.travel_times): N batched envs in validate mode
under a demand profile (spawn='demand': a rush that builds up and ebbs away), once under the fixed cycle
(algorithms/fixed.py) and once under the on-device greedy controller (TFX_ACTION_GREEDY, algorithms/greedy.py:14-16) in a
second batch that receives the same cars.  travel_times() runs at every decision - two read-only launches, no host
round trip - and at the end the mean travel time of the finished trips is printed next to the one that also counts the
time the cars still on the map have spent there: a controller that leaves its cars in a jam looks good on the first
figure only.

    python tools/travel_demo.py --envs 256 --decisions 120
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


def make(a):
    seg = max(1, a.decisions * a.ticks // 6)
    level = a.cars_per_tick
    demand = dict(means=[[0.5 * level, level, 1.5 * level, level, 0.5 * level, 0.25 * level]], seg_ticks=seg)
    return TrafficVecEnv(a.envs, a.m, a.n, a.length, capacity=a.capacity, spawn='demand', demand=demand, validate=True,
                         seed=a.seed, trip_cap=a.trip_cap)


def run(a):
    N, T = a.envs, a.ticks
    fixed, greedy = make(a), make(a)                    # same seed, same env ids: the same cars arrive in both
    ph = np.random.RandomState(a.seed).randint(2, size=(N, fixed.engine.I)).astype(np.int32)
    fixed.reset(ph)
    greedy.reset(ph)
    greedy.engine.set_greedy(T)                         # one greedy decision per agent step
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(a.decisions)]
    out = {}
    for d in range(a.decisions):
        ev[d][0].record()
        fixed.agent_step(None, n_ticks=T, cycle_period=a.cycle)
        greedy.agent_step(None, n_ticks=T)
        ev[d][1].record()
        out["fixed cycle"] = fixed.travel_times()
        out["greedy (on device)"] = greedy.travel_times()
        ev[d][2].record()
    torch.cuda.synchronize()
    skip = min(3, a.decisions - 1)
    ms = np.array([[e[i].elapsed_time(e[i + 1]) for i in range(2)] for e in ev[skip:]])
    rows = {}
    for name, tv in out.items():
        f, u = float(tv.finished.sum()), float(tv.unfinished.sum())
        fs, us = float(tv.finished_s.sum()), float(tv.unfinished_s.sum())
        rows[name] = dict(finished=f / N, unfinished=u / N, lost=float(tv.lost.sum()) / N, oldest=float(tv.oldest_s.max()),
                          mean=fs / max(f, 1.0), incl=(fs + us) / max(f + u, 1.0))
    return rows, float(np.median(ms[:, 0])) / 2, float(np.median(ms[:, 1])) / 2


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--decisions", type=int, default=120)
    ap.add_argument("--ticks", type=int, default=10)
    ap.add_argument("--m", type=int, default=4)
    ap.add_argument("--n", type=int, default=4)
    ap.add_argument("--length", type=float, default=200.0)
    ap.add_argument("--capacity", type=int, default=34)
    ap.add_argument("--cars-per-tick", type=float, default=0.5, help="mean arrivals per env per tick at the middle level")
    ap.add_argument("--cycle", type=int, default=20, help="ticks per phase of the fixed cycle")
    ap.add_argument("--trip-cap", type=int, default=4096)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    rows, step_ms, travel_ms = run(a)
    lines = ["travel demo: %d envs (%dx%d grid, L=%g, C=%d), %d decisions of %d ticks, the same cars for both controllers"
             % (a.envs, a.m, a.n, a.length, a.capacity, a.decisions, a.ticks),
             "%-20s %14s %16s %10s %12s %16s %24s" % ("controller", "trips per env", "on the map / env", "lost / env", "oldest (s)",
                                                       "mean trip (s)", "mean incl. unfinished (s)")]
    for name in ("fixed cycle", "greedy (on device)"):
        r = rows[name]
        lines.append("%-20s %14.1f %16.1f %10.1f %12.1f %16.2f %24.2f" % (name, r["finished"], r["unfinished"], r["lost"],
                                                                           r["oldest"], r["mean"], r["incl"]))
    lines.append("median ms per decision and batch: step %.3f   travel_times (two launches + the derived views) %.3f"
                 % (step_ms, travel_ms))
    for ln in lines:
        print(ln)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n\n")
    return rows


if __name__ == "__main__":
    main()
