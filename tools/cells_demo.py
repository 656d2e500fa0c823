"""A convolutional policy over the road-cell observation (tfx_road_cells): N batched envs with on-device arrivals; at
every decision TrafficVecEnv.cell_obs() gives the image [E, 2, 4, B, m, n] - per approach and cell the car count and the
mean speed, computed on the device from one read-only launch over the live cars - and a small torch.nn.Conv2d network
over image.view(E, 8 * B, m, n) picks the phase of every intersection, held for the decision's ticks.  The network is
untrained (seeded random weights): the demo shows the data path and what it costs, not a learned controller.  Prints the
mean return per env and the median time per decision split into env / cells / policy.

    python tools/cells_demo.py --envs 256 --decisions 60
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


def policy(cells, hidden, device, seed):
    """[E, 8 B, m, n] -> [E, 2, m, n]: a score per phase and intersection"""
    torch.manual_seed(seed)
    net = torch.nn.Sequential(torch.nn.Conv2d(8 * cells, hidden, 3, padding=1), torch.nn.ReLU(),
                              torch.nn.Conv2d(hidden, 2, 1))
    return net.to(device).eval()


def run(a):
    N, T, B = a.envs, a.ticks, a.cells
    venv = TrafficVecEnv(N, a.m, a.n, a.length, capacity=a.capacity, spawn='device', seed=a.seed,
                         local_cars_per_sec=a.cars_per_sec)
    eng = venv.engine
    dev = eng.device
    net = policy(B, a.hidden, dev, a.seed)
    venv.reset(np.random.RandomState(a.seed).randint(2, size=(N, eng.I)).astype(np.int32))
    ret = torch.zeros(N, device=dev)
    cars = torch.zeros((), dtype=torch.int64, device=dev)
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range(a.decisions)]
    with torch.no_grad():
        for d in range(a.decisions):
            ev[d][0].record()
            obs = venv.cell_obs(n_cells=B)
            ev[d][1].record()
            score = net(obs.image.view(N, 8 * B, a.m, a.n))
            actions = (score[:, 1] > score[:, 0]).reshape(N, eng.I).to(torch.int32)
            ev[d][2].record()
            _, rew, _ = venv.agent_step(actions, n_ticks=T)
            ev[d][3].record()
            ret += rew.sum(dim=1)
            cars += obs.n_cars[:, :eng.r].sum(dtype=torch.int64)
    torch.cuda.synchronize()
    skip = min(3, a.decisions - 1)
    ms = np.array([[e[i].elapsed_time(e[i + 1]) for i in range(3)] for e in ev[skip:]])
    return dict(ret=float(ret.mean()), cars=float(cars) / (N * a.decisions), cells_ms=float(np.median(ms[:, 0])),
                policy_ms=float(np.median(ms[:, 1])), env_ms=float(np.median(ms[:, 2])))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--decisions", type=int, default=60)
    ap.add_argument("--ticks", type=int, default=10)
    ap.add_argument("--cells", type=int, default=8)
    ap.add_argument("--hidden", type=int, default=32)
    ap.add_argument("--m", type=int, default=4)
    ap.add_argument("--n", type=int, default=4)
    ap.add_argument("--length", type=float, default=200.0)
    ap.add_argument("--capacity", type=int, default=34)
    ap.add_argument("--cars-per-sec", type=float, default=0.12)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    r = run(a)
    lines = ["cells demo: %d envs (%dx%d grid, L=%g, C=%d), %d decisions of %d ticks, %d cells per approach, Conv2d(%d, %d, 3) "
             "+ Conv2d(%d, 2, 1), untrained" % (a.envs, a.m, a.n, a.length, a.capacity, a.decisions, a.ticks, a.cells,
                                                  8 * a.cells, a.hidden, a.hidden),
             "mean return per env %.2f   cars seen on the approaches per env and decision %.1f" % (r["ret"], r["cars"]),
             "median ms per decision: env %.3f   cells %.3f   policy %.3f" % (r["env_ms"], r["cells_ms"], r["policy_ms"])]
    for ln in lines:
        print(ln)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n\n")
    return r


if __name__ == "__main__":
    main()
