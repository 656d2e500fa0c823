"""Time the demand profiles (tfx_set_demand, rule 4 of include/tfx.h) against the reference-shaped on-device stream
(tfx_set_poisson, spawn='device') on the benchmark's configurations, in one run: ms per tick of 50-tick step() calls and of
10-tick decisions, with spawn 'demand' (K = S = 1, equal weights, the same mean cars per tick) and with spawn 'device',
and the k_demand launch alone (tfx_demand_counts of a call's worth of rows).  The 'device' path is not touched by the
demand code, so its figure is also what the commit before the demand gives.

--mixed adds the same shape with an archetype table of three rows, from an empty start (the prefill has no rows): spawn
'demand' there draws every car's row as well (tfx_set_demand_mixed, rule 5: k_demand<true>, timed alone through
tfx_demand_rows), spawn 'device' draws them in k_poisson<true>.

    python tools/time_demand.py --out profiles/demand.txt          # cfg2 x 4096 and cfg4 x 1
    python tools/time_demand.py --cases cfg2:4096 --mixed --out profiles/demand_mixed.txt
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

from gym_traffic import workload as wl  # noqa: E402


def timed(fn, calls, warmup=3):
    """median / min / max milliseconds per call, each call between its own pair of events"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    ms = np.array([a.elapsed_time(b) for a, b in ev])
    return float(np.median(ms)), float(ms.min()), float(ms.max())


def case(config, envs, spawn, calls):
    eng = wl.setup_engine(config, envs=envs)
    mean = eng.n_entry / float(wl.SPAWN_PERIOD)              # the benchmark's rate: a car per entry road every 8 ticks
    if spawn == "demand":
        eng.set_demand([[mean]], seed=1)
    else:
        eng.set_poisson(mean, seed=1)
    eng.step(wl.SETTLE_TICKS.get(config, 100))
    out = {"step": timed(lambda: eng.step(50, update_done=False), calls), "agent": timed(lambda: eng.agent_step(10), calls)}
    if spawn == "demand":
        for n in (50, 10):
            buf = torch.empty((n, eng.E, eng.n_entry), dtype=torch.int32, device=eng.device)
            out["k_demand %d rows" % n] = timed(lambda: eng.demand_counts(eng.tick, n, out=buf), calls)
    return out, mean


TAB = [[11.11, 4, 3, 4, 13.89, 6, 2, 1], [8.0, 8, 1.5, 4, 10.0, 4, 2.5, 2], [12.0, 3.5, 4, 2, 16.0, 7, 1.5, 1]]


def mixed_case(config, envs, spawn, calls, fill=400):
    """`case` for cars of three archetypes: the roads fill from the stream itself"""
    from gym_traffic.core import TfxEngine
    c = wl.CONFIGS[config]
    eng = TfxEngine(c["m"], c["n"], c["length"], c["capacity"], n_envs=envs, rate=0.5, planes=3, archetypes=np.asarray(TAB, np.float32))
    eng.reset(np.zeros((1, eng.I), np.int32))
    eng.set_actions(cycle_period=wl.LIGHT_PERIOD)
    mean = eng.n_entry / float(wl.SPAWN_PERIOD)
    if spawn == "demand":
        eng.set_demand([[mean]], seed=1, row_weights=[3.0, 1.0, 2.0])
    else:
        eng.set_poisson(mean, seed=1)
    eng.step(fill)
    out = {"step": timed(lambda: eng.step(50, update_done=False), calls), "agent": timed(lambda: eng.agent_step(10), calls)}
    if spawn == "demand":
        n = 10
        buf = (torch.empty((n, eng.E, eng.n_entry), dtype=torch.int32, device=eng.device),
               torch.zeros((n, eng.E, eng.n_entry, eng.demand_rows_per_road), dtype=torch.uint8, device=eng.device))
        out["k_demand<true> %d rows, S = %d" % (n, eng.demand_rows_per_road)] = timed(lambda: eng.demand_rows(eng.tick, n, out=buf), calls)
        out["k_demand<false> %d rows" % n] = timed(lambda: eng.demand_counts(eng.tick, n, out=buf[0]), calls)
    return out, mean


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="cfg2:4096,cfg4:1", help="config:envs, comma separated")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--mixed", action="store_true", help="also time the cases with an archetype table of three rows")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    lines = ["median (min .. max) over %d calls, events around each call" % a.calls]
    for item in a.cases.split(","):
        config, envs = item.split(":")
        envs = int(envs)
        for spawn, mixed in [("demand", False), ("device", False)] + ([("demand", True), ("device", True)] if a.mixed else []):
            r, mean = (mixed_case if mixed else case)(config, envs, spawn, a.calls)
            head = "%s x %d%s, spawn %-6s (%.1f cars per env per tick)" % (config, envs, ", 3 archetypes" if mixed else "", spawn, mean)
            lines.append("%s  step(50): %.4f (%.4f .. %.4f) ms per tick" % ((head,) + tuple(x / 50 for x in r["step"])))
            lines.append("%s  agent_step(10): %.4f (%.4f .. %.4f) ms per tick" % ((head,) + tuple(x / 10 for x in r["agent"])))
            for k, v in r.items():
                if k.startswith("k_demand"):
                    lines.append("%s  %s alone: %.4f (%.4f .. %.4f) ms per launch" % ((head, k) + v))
    for ln in lines:
        print(ln)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n\n")


if __name__ == "__main__":
    main()
