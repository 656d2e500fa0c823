"""Time tfx_road_measures (one launch, all four outputs) against the route there was before the call existed, in the same
run on the same state: tfx_export_ring of every ring slot into a preallocated staging copy, then the torch expressions
that compute the same four fields from the image.

Shapes: cfg2 x 4096 envs and cfg1 x 1024 envs at the benchmark's density (its prefill and settle), and the same shapes
nearly empty (a reset and a few arrivals).  Events around each of `--calls` calls after a warm-up; median (min .. max)
per call, the bytes of live cars read per second (8 B per car) against the 8 TB/s HBM figure of the README, and the
kernel's answer checked against the torch route's on the spot (the integer fields exactly).

    python tools/time_measures.py [--out FILE] [--calls 50] [--small]
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
from gym_traffic.core import TfxEngine  # noqa: E402

HBM_BYTES_PER_S = 8e12
HALT = 0.1


def timed(fn, calls, warmup=3):
    """median / min / max microseconds per call, each call between its own pair of events"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    us = np.array([a.elapsed_time(b) * 1e3 for a, b in ev])
    return float(np.median(us)), float(us.min()), float(us.max())


def export_route(eng, halt, x_from):
    """The four fields from the ring image: tfx_export_ring, then masked torch operations in car order."""
    xv = eng.xv                                        # tfx_export_ring of the whole batch into the staging copy
    C = eng.C
    ld, lc = eng.leading.long(), eng.lastcar.long()
    n = lc - ld + (ld > lc) * (C - 1)
    j = torch.arange(C - 1, device=eng.device)
    slot = ld[..., None] + 1 + j
    slot = torch.where(slot > C - 1, slot - (C - 1), slot)
    live = j < n[..., None]
    slot = torch.where(live, slot, torch.zeros_like(slot))
    x = torch.gather(xv[..., 0], 2, slot)
    v = torch.gather(xv[..., 1], 2, slot)
    inr = live & (x >= x_from)
    still = inr & (v < halt)
    broken = torch.cumsum((live & ~still).to(torch.int32), dim=-1)
    queue = (live & (broken == 0)).sum(dim=-1, dtype=torch.int32)
    return (inr.sum(dim=-1, dtype=torch.int32), still.sum(dim=-1, dtype=torch.int32), queue,
            torch.where(inr, v, torch.zeros_like(v)).sum(dim=-1))


def nearly_empty(name, envs):
    c = wl.CONFIGS[name]
    eng = TfxEngine(c["m"], c["n"], c["length"], c["capacity"], n_envs=envs, rate=0.5, planes=2)
    eng.reset(np.zeros((1, eng.I), np.int32))
    eng.set_spawns(period=wl.SPAWN_PERIOD)
    eng.set_actions(cycle_period=wl.LIGHT_PERIOD)
    eng.step(16)
    return eng


def case(title, eng, length, calls, lines):
    x_from = length - 50.0
    cars = int(eng.cars_on_roads_flat().sum())
    t_new = timed(lambda: eng.road_measures(HALT, x_from), calls)
    t_all = timed(lambda: eng.road_measures(HALT, None), calls)
    t_old = timed(lambda: export_route(eng, HALT, x_from), max(5, calls // 5), warmup=2)
    got = eng.road_measures(HALT, x_from)
    want = export_route(eng, HALT, x_from)
    same = all(bool(torch.equal(g, w)) for g, w in zip(got[:3], want[:3]))
    close = bool(torch.allclose(got[3], want[3], rtol=1e-5, atol=1e-4))
    eng.drop_staging()
    rate = cars * 8 / (t_new[0] * 1e-6)
    lines.append("%s: %d envs, %d roads, %d cars on the roads (%.1f per road)" % (title, eng.E, eng.E * eng.R, cars, cars / (eng.E * eng.R)))
    lines.append("  tfx_road_measures, x_from = L - 50     %9.1f (%.1f .. %.1f) us" % t_new)
    lines.append("  tfx_road_measures, every car in range  %9.1f (%.1f .. %.1f) us" % t_all)
    lines.append("  tfx_export_ring + torch expressions    %9.1f (%.1f .. %.1f) us   x%.1f" % (t_old + (t_old[0] / t_new[0],)))
    lines.append("  live-car bytes read: %.3e B/s = %.1f %% of %.0e B/s; integer fields equal the export route's: %s, speed sums "
                 "close: %s" % (rate, 100 * rate / HBM_BYTES_PER_S, HBM_BYTES_PER_S, same, close))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="64 envs per shape: a rehearsal, not a measurement")
    a = ap.parse_args()
    lines = ["tfx_road_measures, all four outputs: median (min .. max) per call over %d calls, events around each call" % a.calls]
    for name, envs in (("cfg2", 4096), ("cfg1", 1024)):
        E = 64 if a.small else envs
        length = wl.CONFIGS[name]["length"]
        eng = wl.setup_engine(name, envs=E)
        eng.step(wl.SETTLE_TICKS.get(name, 100))
        case("%s at the benchmark's density" % name, eng, length, a.calls, lines)
        del eng
        torch.cuda.empty_cache()
        eng = nearly_empty(name, E)
        case("%s nearly empty" % name, eng, length, a.calls, lines)
        del eng
        torch.cuda.empty_cache()
    for ln in lines:
        print(ln)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n\n")


if __name__ == "__main__":
    main()
