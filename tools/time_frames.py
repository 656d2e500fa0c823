"""Time tfx_frames (one memset and one launch; roads only: the launch alone) for 1, 64 and all envs of a batch, in the same
run on the same state against the route there was before the call existed - tfx_export_ring of every ring slot of every
env into a preallocated staging copy, the image and the ring indices to the host, then devrng.frames over the chosen envs
(timed for ONE env: the host loop is linear in the envs drawn) - and against tfx_road_cells at 32 cells on the whole
batch, the nearest read-only pass over the live cars.

Shapes: cfg2 x 4096 envs and cfg1 x 1024 envs at the benchmark's density (its prefill and settle).  Events around each of
`--calls` calls after a warm-up; median (min .. max) per call; the bytes the call has to move - 8 B read per live car of
the envs drawn, 4 B written per frame pixel by the memset, 4 B per road pixel by the kernel - per second against the
8 TB/s HBM figure of the README; the kernel's picture of env 0 checked against the export route's on the spot.

    python tools/time_frames.py [--out FILE] [--calls 50] [--small] [--px 32]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "traffic-env_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from gym_traffic import workload as wl  # noqa: E402
from gym_traffic.devrng import cell_edges, frames  # noqa: E402
from time_measures import HBM_BYTES_PER_S, timed  # noqa: E402


def export_route(eng, px, envs):
    """The frames of `envs` from the ring image: tfx_export_ring of the whole batch, the host copies, devrng.frames."""
    x = eng.xv[..., 0].cpu().numpy()                   # tfx_export_ring into the staging copy, then device to host
    return frames(x, eng.leading.cpu().numpy(), eng.lastcar.cpu().numpy(), eng.current_phase.cpu().numpy(),
                  eng.elapsed.cpu().numpy(), eng.m, eng.n, px, float(eng.cfg.length), yellow_ticks=int(eng.cfg.yellow_ticks),
                  car_l=float(eng.cfg.car_l), env_ids=envs)


def wall(fn, calls):
    """median / min / max microseconds per call on the host clock (the export route ends on the host)"""
    us = []
    for _ in range(calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        us.append((time.perf_counter() - t0) * 1e6)
    return float(np.median(us)), float(min(us)), float(max(us))


def case(title, eng, px, calls, lines):
    cars_all = eng.cars_on_roads_flat()
    cars = int(cars_all.sum())
    H, W = eng.frame_size(px)
    lines.append("%s: %d envs, %d roads, %d cars on the roads (%.1f per road); frames of %d x %d at %d px"
                 % (title, eng.E, eng.E * eng.R, cars, cars / (eng.E * eng.R), H, W, px))
    edges = cell_edges(float(eng.cfg.length), 32)
    t_cells = timed(lambda: eng.road_cells(edges), calls)
    lines.append("  tfx_road_cells, 32 cells, every env        %9.1f (%.1f .. %.1f) us" % t_cells)
    t_old = wall(lambda: export_route(eng, px, [0]), max(3, calls // 10))
    lines.append("  export + host copies + devrng.frames, 1 env %8.1f (%.1f .. %.1f) us (host clock)" % t_old)
    same = bool(np.array_equal(eng.frames([0], px=px).cpu().numpy(), export_route(eng, px, [0])))
    eng.drop_staging()
    for n in sorted({1, min(64, eng.E), eng.E}):
        ids = torch.arange(n, dtype=torch.int32, device=eng.device)
        out = torch.empty((n, H, W, 4), dtype=torch.uint8, device=eng.device)
        t_full = timed(lambda: eng.frames(ids, px=px, out=out), calls)
        t_roads = timed(lambda: eng.frames(ids, px=px, out=out, roads_only=True), calls)
        n_cars = int(cars_all[:n].sum())
        road_px = n * eng.R * (px - 3)
        for name, t, moved in (("memset + launch", t_full, n_cars * 8 + n * H * W * 4 + road_px * 4),
                               ("roads only     ", t_roads, n_cars * 8 + road_px * 4)):
            rate = moved / (t[0] * 1e-6)
            lines.append("  tfx_frames, %4d envs, %s      %9.1f (%.1f .. %.1f) us   x%.3f of road_cells; %.3e B moved: "
                         "%.3e B/s = %.2f %% of %.0e B/s" % ((n, name) + t + (t[0] / t_cells[0], moved, rate,
                                                                            100 * rate / HBM_BYTES_PER_S, HBM_BYTES_PER_S)))
        del out
    lines.append("  the kernel's picture of env 0 equals the export route's: %s" % same)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--px", type=int, default=32)
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="64 envs per shape: a rehearsal, not a measurement")
    a = ap.parse_args()
    lines = ["tfx_frames: median (min .. max) per call over %d calls, events around each call" % a.calls]
    for name, envs in (("cfg2", 4096), ("cfg1", 1024)):
        E = 64 if a.small else envs
        eng = wl.setup_engine(name, envs=E)
        eng.step(wl.SETTLE_TICKS.get(name, 100))
        case("%s at the benchmark's density" % name, eng, a.px, a.calls, lines)
        del eng
        torch.cuda.empty_cache()
    for ln in lines:
        print(ln)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n\n")


if __name__ == "__main__":
    main()
