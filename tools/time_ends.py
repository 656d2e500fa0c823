"""Time tfx_road_ends (one launch, all six outputs) at k = 1, 4 and 16 against its two baselines, in the same run on the
same state: tfx_road_measures, the sibling that reads every live car where this launch reads at most k + 3 rows of a tile,
and the route there was before the call existed - tfx_export_ring of every ring slot into a preallocated staging copy,
then the torch expressions that gather the same six fields from the image.

Shape: cfg2 x 4096 envs at the benchmark's density (its prefill and settle), and the same shape nearly empty (a reset and
a few arrivals).  Events around each of `--calls` calls after a warm-up; median (min .. max) per call, and the kernel's
answer checked against the torch route's on the spot - every field bit for bit: nothing but one subtraction is computed.

    python tools/time_ends.py [--out FILE] [--calls 50] [--small]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "traffic-env_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from gym_traffic import workload as wl  # noqa: E402
from gym_traffic.core import RoadEnds  # noqa: E402
from time_measures import HALT, nearly_empty, timed  # noqa: E402

KS = (1, 4, 16)
INF = float("inf")


def export_route(eng, k):
    """The six fields from the ring image: tfx_export_ring, then gathers over the first k slots and the last one
    (single-archetype handles: every row is 0)."""
    xv = eng.xv                                        # tfx_export_ring of the whole batch into the staging copy
    C = eng.C
    ld, lc = eng.leading.long(), eng.lastcar.long()
    n = (lc - ld + (ld > lc) * (C - 1)).clamp(0, C - 1)
    j = torch.arange(k, device=eng.device)
    slot = ld[..., None] + 1 + j
    slot = torch.where(slot > C - 1, slot - (C - 1), slot)
    live = j < n[..., None]
    slot = torch.where(live, slot, torch.zeros_like(slot))
    x = torch.gather(xv[..., 0], 2, slot)
    v = torch.gather(xv[..., 1], 2, slot)
    inf, zero = torch.full_like(x, INF), torch.zeros_like(x)
    heads = torch.stack([torch.where(live, float(eng.cfg.length) - x, inf), torch.where(live, v, zero)], dim=-1)
    rows = torch.where(live, torch.zeros_like(slot), torch.full_like(slot, 255)).to(torch.uint8)
    some = n > 0
    last = torch.where(some, lc, torch.zeros_like(lc))[..., None]
    tx, tv = torch.gather(xv[..., 0], 2, last)[..., 0], torch.gather(xv[..., 1], 2, last)[..., 0]
    tail = torch.stack([torch.where(some, tx, torch.full_like(tx, INF)), torch.where(some, tv, torch.zeros_like(tv))], dim=-1)
    tail_row = torch.where(some, torch.zeros_like(n), torch.full_like(n, 255)).to(torch.uint8)
    return RoadEnds(n.to(torch.int32), n.clamp(max=k).to(torch.int32), heads, rows, tail, tail_row)


def case(title, eng, calls, lines):
    cars = int(eng.cars_on_roads_flat().sum())
    lines.append("%s: %d envs, %d roads, %d cars on the roads (%.1f per road)"
                 % (title, eng.E, eng.E * eng.R, cars, cars / (eng.E * eng.R)))
    t_sib = timed(lambda: eng.road_measures(HALT, None), calls)
    lines.append("  tfx_road_measures, every car in range   %9.1f (%.1f .. %.1f) us" % t_sib)
    for k in KS:
        t_new = timed(lambda: eng.road_ends(k), calls)
        t_old = timed(lambda: export_route(eng, k), max(5, calls // 5), warmup=2)
        got, want = eng.road_ends(k), export_route(eng, k)
        same = all(bool(torch.equal(g.view(torch.uint8), w.contiguous().view(torch.uint8))) for g, w in zip(got, want))
        eng.drop_staging()
        lines.append("  tfx_road_ends, k = %-2d                    %9.1f (%.1f .. %.1f) us   ends / measures x%.2f"
                     % ((k,) + t_new + (t_new[0] / t_sib[0],)))
        lines.append("  tfx_export_ring + torch gathers, k = %-2d  %9.1f (%.1f .. %.1f) us   x%.1f; every field equals the "
                     "export route's bit for bit: %s" % ((k,) + t_old + (t_old[0] / t_new[0], same)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="64 envs: a rehearsal, not a measurement")
    a = ap.parse_args()
    lines = ["tfx_road_ends, all six outputs: median (min .. max) per call over %d calls, events around each call" % a.calls]
    name = "cfg2"
    E = 64 if a.small else 4096
    eng = wl.setup_engine(name, envs=E)
    eng.step(wl.SETTLE_TICKS.get(name, 100))
    case("%s at the benchmark's density" % name, eng, a.calls, lines)
    del eng
    torch.cuda.empty_cache()
    eng = nearly_empty(name, E)
    case("%s nearly empty" % name, eng, a.calls, lines)
    for ln in lines:
        print(ln)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n\n")


if __name__ == "__main__":
    main()
