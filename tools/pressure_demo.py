"""Max-pressure control from the road measures (tfx_road_measures): N batched envs with on-device arrivals; at every
decision each intersection takes the phase whose approaches have the larger pressure - cars on the approach roads minus
cars on the roads they feed (TrafficVecEnv.measures().pressure, computed on the device from one read-only launch over
the live cars) - and holds it for the decision's ticks.  The baseline is the on-device greedy controller
(TFX_ACTION_GREEDY, algorithms/greedy.py:14-16) in a second batch of envs on the same arrival streams.  Prints the mean
return per env of both, the halted vehicle-decisions (cars standing within the stop zone at a decision, added up over
the decisions on the device with accumulate=True) and the time per decision split into measure and step.

    python tools/pressure_demo.py --envs 256 --decisions 120
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

from gym_traffic.core import RoadMeasures  # noqa: E402
from gym_traffic.envs.vec_env import TrafficVecEnv  # noqa: E402


def make(a):
    return TrafficVecEnv(a.envs, a.m, a.n, a.length, capacity=a.capacity, spawn='device', seed=a.seed,
                         local_cars_per_sec=a.cars_per_sec)


def halted_total(venv, a):
    """A zeroed [E, R] tensor and the call that adds this decision's halted cars within the stop zone to it."""
    eng = venv.engine
    acc = RoadMeasures(None, torch.zeros((eng.E, eng.R), dtype=torch.int32, device=eng.device), None, None)
    return acc, lambda: eng.road_measures(halt_speed=a.halt_speed, x_from=a.length - a.stop_zone, accumulate=True, out=acc)


def run(a):
    N, T = a.envs, a.ticks
    live, base = make(a), make(a)                       # same seed, same env ids: the same cars arrive in both
    eng = live.engine
    dev = eng.device
    ph = np.random.RandomState(a.seed).randint(2, size=(N, eng.I)).astype(np.int32)
    live.reset(ph)
    base.reset(ph)
    base.engine.set_greedy(T)                           # one greedy decision per agent step, held like ours
    acc_live, add_live = halted_total(live, a)
    acc_base, add_base = halted_total(base, a)
    ret_live = torch.zeros(N, device=dev)
    ret_base = torch.zeros(N, device=dev)
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(a.decisions)]
    for d in range(a.decisions):
        ev[d][0].record()
        pressure = live.measures(halt_speed=a.halt_speed).pressure      # [N, I, 2], every car counts
        add_live()
        ev[d][1].record()
        # phase 1 serves the N-S approaches (graph.phases == 0), as the greedy rule has it
        actions = (pressure[..., 0] > pressure[..., 1]).to(torch.int32)
        _, rew, _ = live.agent_step(actions, n_ticks=T)
        ev[d][2].record()
        ret_live += rew.sum(dim=1)
        add_base()
        _, rew, _ = base.agent_step(None, n_ticks=T)
        ret_base += rew.sum(dim=1)
    torch.cuda.synchronize()
    skip = min(3, a.decisions - 1)
    ms = np.array([[e[i].elapsed_time(e[i + 1]) for i in range(2)] for e in ev[skip:]])
    r = eng.r
    return dict(pressure_return=float(ret_live.mean()), greedy_return=float(ret_base.mean()),
                pressure_halted=float(acc_live.n_halted[:, :r].sum()) / N,
                greedy_halted=float(acc_base.n_halted[:, :r].sum()) / N,
                measure_ms=float(np.median(ms[:, 0])), step_ms=float(np.median(ms[:, 1])))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--decisions", type=int, default=120)
    ap.add_argument("--ticks", type=int, default=10)
    ap.add_argument("--m", type=int, default=4)
    ap.add_argument("--n", type=int, default=4)
    ap.add_argument("--length", type=float, default=200.0)
    ap.add_argument("--capacity", type=int, default=34)
    ap.add_argument("--cars-per-sec", type=float, default=0.12)
    ap.add_argument("--halt-speed", type=float, default=0.1)
    ap.add_argument("--stop-zone", type=float, default=50.0, help="metres before the end of a road in which halted cars count")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    r = run(a)
    lines = ["pressure demo: %d envs (%dx%d grid, L=%g, C=%d), %d decisions of %d ticks, the same arrival streams for both "
             "controllers" % (a.envs, a.m, a.n, a.length, a.capacity, a.decisions, a.ticks),
             "%-22s %22s %34s" % ("controller", "mean return per env", "halted vehicle-decisions per env"),
             "%-22s %22.2f %34.1f" % ("max pressure", r["pressure_return"], r["pressure_halted"]),
             "%-22s %22.2f %34.1f" % ("greedy (on device)", r["greedy_return"], r["greedy_halted"]),
             "median ms per decision: measure (two launches + the derived views) %.3f   step %.3f"
             % (r["measure_ms"], r["step_ms"])]
    for ln in lines:
        print(ln)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n\n")
    return r


if __name__ == "__main__":
    main()
