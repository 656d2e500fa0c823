"""Time tfx_road_cells (one launch, both planes) at B = 8 and B = 32 cells against the route there was before the call
existed, in the same run on the same state - tfx_export_ring of every ring slot into a preallocated staging copy, then
torch.bucketize and scatter_add_ over the image for the same two planes - and against tfx_road_measures on that state,
the floor: the same read of the live cars with four words stored per road.

Shapes: cfg2 x 4096 envs and cfg1 x 1024 envs at the benchmark's density (its prefill and settle), and the same shapes
nearly empty (a reset and a few arrivals).  Events around each of `--calls` calls after a warm-up; median (min .. max)
per call; the bytes the kernel has to move per second (8 B read per live car, 8 B written per cell) against the 8 TB/s
HBM figure of the README; the kernel's counts checked against the export route's on the spot.

    python tools/time_cells.py [--out FILE] [--calls 50] [--small]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "traffic-env_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from gym_traffic import workload as wl  # noqa: E402
from gym_traffic.devrng import cell_edges  # noqa: E402
from time_measures import HALT, HBM_BYTES_PER_S, nearly_empty, timed  # noqa: E402


def export_route(eng, edges_dev):
    """The two planes from the ring image: tfx_export_ring, then bucketize and scatter_add_ over every car slot.
    edges_dev: the INNER edges on the device (uniform edges with infinite ends: every live car is in a cell)."""
    xv = eng.xv                                        # tfx_export_ring of the whole batch into the staging copy
    C = eng.C
    B = edges_dev.numel() + 1
    ld, lc = eng.leading.long(), eng.lastcar.long()
    n = lc - ld + (ld > lc) * (C - 1)
    j = torch.arange(C - 1, device=eng.device)
    slot = ld[..., None] + 1 + j
    slot = torch.where(slot > C - 1, slot - (C - 1), slot)
    live = j < n[..., None]
    slot = torch.where(live, slot, torch.zeros_like(slot))
    x = torch.gather(xv[..., 0], 2, slot)
    v = torch.gather(xv[..., 1], 2, slot)
    cell = torch.bucketize(x, edges_dev, right=True)    # #{k : x >= inner[k]}
    cars = torch.zeros((eng.E, eng.R, B), dtype=torch.int32, device=eng.device)
    total = torch.zeros((eng.E, eng.R, B), dtype=torch.float32, device=eng.device)
    cars.scatter_add_(2, cell, live.to(torch.int32))
    total.scatter_add_(2, cell, torch.where(live, v, torch.zeros_like(v)))
    return cars, total


def case(title, eng, length, calls, lines):
    cars = int(eng.cars_on_roads_flat().sum())
    lines.append("%s: %d envs, %d roads, %d cars on the roads (%.1f per road)" % (title, eng.E, eng.E * eng.R, cars, cars / (eng.E * eng.R)))
    t_floor = timed(lambda: eng.road_measures(HALT, None), calls)
    lines.append("  tfx_road_measures (4 words per road)    %9.1f (%.1f .. %.1f) us" % t_floor)
    for B in (8, 32):
        edges = cell_edges(length, B)
        inner = torch.as_tensor(edges[1:-1]).to(eng.device)
        t_new = timed(lambda: eng.road_cells(edges), calls)
        t_old = timed(lambda: export_route(eng, inner), max(5, calls // 5), warmup=2)
        got = eng.road_cells(edges)
        want = export_route(eng, inner)
        same = bool(torch.equal(got.n_cars, want[0]))
        close = bool(torch.allclose(got.speed_sum, want[1], rtol=1e-5, atol=1e-4))
        eng.drop_staging()
        moved = cars * 8 + eng.E * eng.R * B * 8
        rate = moved / (t_new[0] * 1e-6)
        lines.append("  B = %2d: tfx_road_cells, both planes     %9.1f (%.1f .. %.1f) us   x%.2f of road_measures"
                     % ((B,) + t_new + (t_new[0] / t_floor[0],)))
        lines.append("          export + bucketize + scatter_add %9.1f (%.1f .. %.1f) us   x%.1f of tfx_road_cells"
                     % (t_old + (t_old[0] / t_new[0],)))
        lines.append("          %.3e B read and written per call: %.3e B/s = %.1f %% of %.0e B/s; counts equal the export "
                     "route's: %s, speed sums close: %s" % (moved, rate, 100 * rate / HBM_BYTES_PER_S, HBM_BYTES_PER_S, same, close))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="64 envs per shape: a rehearsal, not a measurement")
    a = ap.parse_args()
    lines = ["tfx_road_cells, both planes: median (min .. max) per call over %d calls, events around each call" % a.calls]
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
