"""Time a 10-tick decision whose restarts come from a pool of warmed-up envs (TrafficVecEnv.set_warm_pool,
tfx_set_episode_pool) against the same decision with episodes on and no pool - launch for launch and kernel for kernel
the decision of the commit before the pool existed - and against an explicit clone_envs of the same number of envs.

Envs as tools/rollout_demo.py makes them (spawn='device', 200 m roads, cycle lights), at two sizes: 1024 envs of the 4x4
grid with capacity 34 (cfg1's shape) and 4096 envs of the 16x16 grid.  The share of envs that restarts per decision is set
through the time limit: episode_len M with the envs' running lengths staggered so that E / M envs reach it in every
decision - 0 % (no limit), about 1 % (M = 100) and 100 % (M = 1: every env in every decision).  Overflows end episodes
as well; the share that really restarted is counted on the device and printed next to each figure.

Each figure: median (min .. max) microseconds over `--calls` decisions, device events around every call, after a
warm-up; the two variants of a case alternate in blocks, twice, so that the spread between blocks of the same variant
is on the page next to the difference between the variants.  `--out FILE` appends the lines to FILE.

    python tools/time_warm_restart.py                       # both sizes
    python tools/time_warm_restart.py --size small --calls 100
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

SIZES = {"small": dict(envs=1024, m=4, n=4, capacity=34), "large": dict(envs=4096, m=16, n=16, capacity=34)}
SHARES = (("0 %", 0), ("1 %", 100), ("100 %", 1))


def timed(fn, calls, warmup):
    """median / min / max microseconds per call, each call between its own pair of events; fn returns a 0-d tensor that
    is summed on the device (the envs that ended)"""
    total = None
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    for a, b in ev:
        a.record()
        n = fn()
        b.record()
        if n is not None:
            total = n.clone() if total is None else total + n
    torch.cuda.synchronize()
    us = np.array([a.elapsed_time(b) * 1e3 for a, b in ev])
    return (float(np.median(us)), float(us.min()), float(us.max())), (0 if total is None else int(total))


def make_env(size, limit):
    s = SIZES[size]
    venv = TrafficVecEnv(s["envs"], s["m"], s["n"], 200.0, capacity=s["capacity"], spawn='device', seed=0,
                         autoreset=True, episode_len=limit or None)
    venv.reset()
    if limit > 1:       # E / limit envs reach the limit in every decision
        venv.episode_length.copy_(torch.arange(s["envs"], dtype=torch.int32, device=venv.engine.device) % limit)
    return venv


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="both", choices=sorted(SIZES) + ["both"])
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--pool", type=int, default=64, help="envs in the pool")
    ap.add_argument("--pool-decisions", type=int, default=6, help="decisions the pool is warmed up for")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_warm_restart.py measures on the GPU; none is visible")
    lines = []
    for size in (sorted(SIZES) if a.size == "both" else [a.size]):
        s = SIZES[size]
        lines.append("%d envs of the %dx%d grid, capacity %d, spawn='device', 10-tick decisions under the 5-tick cycle; a pool of "
                     "%d envs warmed up for %d decisions" % (s["envs"], s["m"], s["n"], s["capacity"], a.pool, a.pool_decisions))
        lines.append("median (min .. max) us per decision over %d decisions, events around each; [envs that ended per decision]" % a.calls)
        for label, limit in SHARES:
            plain, warm = make_env(size, limit), make_env(size, limit)
            pool = warm.make_warm_pool(a.pool, a.pool_decisions, cycle_period=5)
            warm.set_warm_pool(pool)

            def decide(venv):
                def fn():
                    out = venv.agent_step(n_ticks=10, cycle_period=5)
                    return (out[2] | venv.truncated).sum()
                return fn
            for rep in range(2):
                for name, venv in (("episodes on, no pool", plain), ("pool attached", warm)):
                    t, ended = timed(decide(venv), a.calls, a.warmup if rep == 0 else 2)
                    lines.append("  %-6s %-22s %9.1f (%.1f .. %.1f)   [%.1f]   %s, cars on the roads %d"
                                 % ((label, name) + t + (ended / a.calls, venv.engine.step_kernel(),
                                                         int(venv.engine.cars_on_roads_flat().sum()))))
            if limit == 1:
                # the yardstick of the 100 % case: every env cloned from the pool by an explicit call, the launch alone
                import ctypes as C
                from gym_traffic import _native as nat
                eng = plain.engine
                idx = (torch.arange(eng.E, dtype=torch.int32, device=eng.device) % a.pool).contiguous()
                raw, st = C.c_void_p(idx.data_ptr()), eng._stream()
                t, _ = timed(lambda: nat.check(eng.lib.tfx_clone_envs(eng.h, pool.engine.h, raw, 0, st)), a.calls, 5)
                lines.append("  %-6s %-22s %9.1f (%.1f .. %.1f)   tfx_clone_envs alone, %d envs from the pool"
                             % ((label, "explicit clone") + t + (eng.E,)))
            del plain, warm, pool
        lines.append("")
    for ln in lines:
        print(ln)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
