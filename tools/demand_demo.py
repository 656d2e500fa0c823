"""Tidal demand on the device (tfx_set_demand, rule 4 of include/tfx.h): N batched envs whose arrivals change over time
and are not symmetric - segments in which the N-S entry roads carry most of the cars alternate with segments in which
the E-W ones do - at two demand levels spread over the envs of the batch (profile 0: the base level, profile 1: `--boost`
times as much).  The fixed cycle and the on-device greedy controller (TFX_ACTION_GREEDY, algorithms/greedy.py:14-16) run
on the same seed, so on the same cars; an asymmetric demand is where the two differ at all.  Prints both mean returns per
env and, from the read-only preview tfx_demand_counts, the cars every segment brought and the share of them that
entered on N-S roads.  --trucks SHARE_PEAK,SHARE_OFF makes the cars of two kinds (tfx_set_demand_mixed, rule 5): a table of
two archetype rows, car and truck, the trucks' share of the arrivals by segment (segment 0 is the peak); a `rows` line
then gives the share of trucks among the cars every segment spawned, from the preview tfx_demand_rows.

    python tools/demand_demo.py --envs 256 --decisions 120
    python tools/demand_demo.py --envs 256 --decisions 120 --trucks 0.4,0.1
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


def tidal(a):
    """means [2][2] and weights [2][2][n_entry]: segment 0 N-S heavy, segment 1 E-W heavy; entry roads come in the order
    west side, east side, first row, last row (roadgraph.py generate_entrypoints): the first 2m are E-W, the last 2n N-S"""
    ns = np.r_[np.zeros(2 * a.m), np.ones(2 * a.n)]
    w = np.stack([np.where(ns > 0, a.tide, 1.0), np.where(ns > 0, 1.0, a.tide)])
    per_tick = a.cars_per_sec * 0.5 * (2 * a.m + 2 * a.n)          # cars per env per tick at the base level (rate 0.5 s)
    means = np.array([[per_tick, per_tick], [a.boost * per_tick, a.boost * per_tick]])
    return means, np.stack([w, w]), ns


# rows (v, l, a, delta, v0, b, T, s0) of the archetype table under --trucks: the reference's car, and a long slow truck
CAR_AND_TRUCK = [[11.11, 4.0, 3.0, 4.0, 13.89, 6.0, 2.0, 1.0], [8.0, 8.0, 1.5, 4.0, 10.0, 4.0, 2.5, 2.0]]


def make(a, means, weights):
    mixed = {}
    demand = dict(means=means, weights=weights, seg_ticks=a.seg_decisions * a.ticks, tick_offset=0)
    if a.trucks is not None:
        mixed = dict(archetypes=CAR_AND_TRUCK)
        demand["row_weights"] = [[[1.0 - share, share] for share in a.trucks]] * 2      # [profile][segment][car, truck]
    venv = TrafficVecEnv(a.envs, a.m, a.n, a.length, capacity=a.capacity, spawn='demand', seed=a.seed, demand=demand, **mixed)
    venv.demand_profile.copy_(torch.arange(a.envs, device=venv.engine.device, dtype=torch.int32) % 2)    # two levels
    return venv


def run(a):
    means, weights, ns = tidal(a)
    T = a.ticks
    ph = np.random.RandomState(a.seed).randint(2, size=(a.envs, a.m * a.n)).astype(np.int32)
    rets = {}
    for name in ("cycle", "greedy"):
        venv = make(a, means, weights)
        venv.reset(ph)
        if name == "greedy":
            venv.engine.set_greedy(T)                               # one greedy decision per agent step, held for it
        ret = torch.zeros(a.envs, device=venv.engine.device)
        for _ in range(a.decisions):
            _, rew, _ = venv.agent_step(None, n_ticks=T, cycle_period=a.cycle if name == "cycle" else None)
            ret += rew.sum(dim=1)
        rets[name] = float(ret.mean())
    # what arrived, by segment: the preview is a pure function of the clock tick - no env had to run for it
    eng = venv.engine
    seg_ticks = a.seg_decisions * T
    north_south = torch.as_tensor(ns > 0, device=eng.device)
    per_seg = np.zeros((2, 2), np.int64)                            # [segment][all cars, N-S cars]
    trucks = np.zeros((2, 2), np.int64)                             # [segment][cars with a row, trucks among them]
    for t0 in range(0, a.decisions * T, seg_ticks):
        n = min(seg_ticks, a.decisions * T - t0)
        s = (t0 // seg_ticks) % 2
        if a.trucks is None:
            c = eng.demand_counts(t0, n).sum(dim=(0, 1))
        else:
            c, rows = eng.demand_rows(t0, n)            # (row 1 is the truck; the entries past a road's cars are 0)
            trucks[s] += [int(c.clamp(max=rows.shape[-1]).sum()), int(rows.sum())]
            c = c.sum(dim=(0, 1))
        per_seg[s] += [int(c.sum()), int(c[north_south].sum())]
    return rets, per_seg, trucks


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--decisions", type=int, default=120)
    ap.add_argument("--ticks", type=int, default=10)
    ap.add_argument("--seg-decisions", type=int, default=20, help="decisions per demand segment")
    ap.add_argument("--m", type=int, default=4)
    ap.add_argument("--n", type=int, default=4)
    ap.add_argument("--length", type=float, default=200.0)
    ap.add_argument("--capacity", type=int, default=34)
    ap.add_argument("--cars-per-sec", type=float, default=0.12, help="per entry road at the base level, averaged over the sides")
    ap.add_argument("--tide", type=float, default=4.0, help="weight of an entry road on the heavy axis (the light axis: 1)")
    ap.add_argument("--boost", type=float, default=1.5, help="demand level of profile 1 relative to profile 0")
    ap.add_argument("--cycle", type=int, default=20, help="ticks per phase of the fixed cycle")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--trucks", default=None, metavar="SHARE_PEAK,SHARE_OFF",
                    help="two kinds of cars: the trucks' share of the arrivals in segment 0 and in segment 1")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if a.trucks is not None:
        a.trucks = [float(x) for x in a.trucks.split(",")]
        if len(a.trucks) != 2 or not all(0.0 <= x <= 1.0 for x in a.trucks):
            ap.error("--trucks takes two shares in [0, 1]: SHARE_PEAK,SHARE_OFF")
    rets, per_seg, trucks = run(a)
    lines = ["demand demo: %d envs (%dx%d grid, L=%g, C=%d), %d decisions of %d ticks, segments of %d decisions, tide x%g, "
             "every second env at x%g" % (a.envs, a.m, a.n, a.length, a.capacity, a.decisions, a.ticks, a.seg_decisions,
                                          a.tide, a.boost),
             "return cycle   (fixed, %d ticks per phase), mean per env: %.2f" % (a.cycle, rets["cycle"]),
             "return greedy  (on device), mean per env: %.2f" % rets["greedy"]]
    for s, label in enumerate(("N-S heavy", "E-W heavy")):
        cars, ns = per_seg[s]
        lines.append("segment %d (%s): cars %d over the batch, N-S share %.3f" % (s, label, cars, ns / max(1, cars)))
    if a.trucks is not None:
        lines.append("rows: trucks among the cars spawned, " + ", ".join(
            "segment %d: %.3f (asked %.3f)" % (s, trucks[s][1] / max(1, trucks[s][0]), a.trucks[s]) for s in range(2)))
    for ln in lines:
        print(ln)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n\n")
    return rets, per_seg


if __name__ == "__main__":
    main()
