"""Surrogate safety and platoons of two signal controllers from the car-following measures (tfx_road_following): N batched
envs under the on-device fixed cycle and N under the on-device greedy controller (TFX_ACTION_GREEDY,
algorithms/greedy.py:14-16), both on the same arrival streams.  Once per decision TrafficVecEnv.following(accumulate=True)
adds the state's eleven words per road to the engine's tensors - one read-only launch over the live cars, no host
synchronisation - and at the end the demo prints, per controller: conflicts (closing pairs with a time to collision under
--ttc-crit) per 1000 car-decisions, the mean platoon size, the mean time headway and the followers found past their
leader's rear bumper.

    python tools/following_demo.py --envs 256 --decisions 120
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
    return TrafficVecEnv(a.envs, a.m, a.n, a.length, capacity=a.capacity, spawn='device', seed=a.seed,
                         local_cars_per_sec=a.cars_per_sec)


def run(a):
    N, T = a.envs, a.ticks
    fixed, greedy = make(a), make(a)                    # same seed, same env ids: the same cars arrive in both
    ph = np.random.RandomState(a.seed).randint(2, size=(N, fixed.engine.I)).astype(np.int32)
    fixed.reset(ph)
    greedy.reset(ph)
    greedy.engine.set_greedy(T)                         # one greedy decision per agent step
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(a.decisions)]
    last = {}
    for d in range(a.decisions):
        for name, venv, kw in (("fixed cycle", fixed, dict(cycle_period=a.cycle)), ("greedy (on device)", greedy, {})):
            if venv is fixed:
                ev[d][0].record()
            last[name] = venv.following(a.platoon_gap, a.v_min, a.ttc_crit, accumulate=True)
            if venv is fixed:
                ev[d][1].record()
            venv.agent_step(None, n_ticks=T, **kw)
            if venv is fixed:
                ev[d][2].record()
    torch.cuda.synchronize()
    skip = min(3, a.decisions - 1)
    ms = np.array([[e[i].elapsed_time(e[i + 1]) for i in range(2)] for e in ev[skip:]])
    out = {}
    for name, venv in (("fixed cycle", fixed), ("greedy (on device)", greedy)):
        f, r = last[name], venv.engine.r
        cars = int(f.n_cars[:, :r].sum())
        platoons = int(f.platoons[:, :r].sum())
        n_hw = int(f.n_hw[:, :r].sum())
        out[name] = dict(car_decisions=cars, conflicts_per_1000=1000.0 * int(f.conflicts.sum()) / cars if cars else float("nan"),
                         platoon_size=cars / platoons if platoons else float("nan"),
                         headway_s=float(f.hw_sum[:, :r].sum(dtype=torch.float64)) / n_hw if n_hw else float("nan"),
                         overlaps=int(f.overlaps.sum()), min_ttc_s=float(f.min_ttc_s.min()), max_drac=float(f.max_drac.max()))
    out["follow_ms"], out["step_ms"] = float(np.median(ms[:, 0])), float(np.median(ms[:, 1]))
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--decisions", type=int, default=120)
    ap.add_argument("--ticks", type=int, default=10)
    ap.add_argument("--cycle", type=int, default=20, help="ticks between the fixed cycle's phase changes")
    ap.add_argument("--m", type=int, default=4)
    ap.add_argument("--n", type=int, default=4)
    ap.add_argument("--length", type=float, default=200.0)
    ap.add_argument("--capacity", type=int, default=34)
    ap.add_argument("--cars-per-sec", type=float, default=0.12)
    ap.add_argument("--platoon-gap", type=float, default=10.0, help="metres: a follower no further behind belongs to the platoon")
    ap.add_argument("--v-min", type=float, default=0.5, help="m/s: slower followers have no time headway")
    ap.add_argument("--ttc-crit", type=float, default=3.0, help="seconds: a closing pair under it is a conflict")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    r = run(a)
    lines = ["following demo: %d envs (%dx%d grid, L=%g, C=%d), %d decisions of %d ticks, the same arrival streams for both "
             "controllers; platoon gap %g m, v_min %g m/s, critical TTC %g s"
             % (a.envs, a.m, a.n, a.length, a.capacity, a.decisions, a.ticks, a.platoon_gap, a.v_min, a.ttc_crit),
             "%-20s %30s %18s %16s %10s" % ("controller", "conflicts / 1000 car-decisions", "mean platoon size",
                                            "mean headway s", "overlaps")]
    for name in ("fixed cycle", "greedy (on device)"):
        c = r[name]
        lines.append("%-20s %30.3f %18.3f %16.3f %10d" % (name, c["conflicts_per_1000"], c["platoon_size"], c["headway_s"],
                                                          c["overlaps"]))
    lines.append("median ms per decision (fixed cycle): following (one launch + the derived views) %.3f   step %.3f"
                 % (r["follow_ms"], r["step_ms"]))
    for ln in lines:
        print(ln)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n\n")
    return r


if __name__ == "__main__":
    main()
