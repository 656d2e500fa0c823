"""Time tfx_road_following (one launch, all eleven outputs) against the route there was before the call existed, in the
same run on the same state: tfx_export_ring of every ring slot into a preallocated staging copy, then the torch
expressions that compute the same eleven fields from the image - and against tfx_road_measures on that state, the
sibling that reads the same cars and carries nothing from one to the next.

Shapes: cfg2 x 4096 envs and cfg1 x 1024 envs at the benchmark's density (its prefill and settle), and the same shapes
nearly empty (a reset and a few arrivals).  Events around each of `--calls` calls after a warm-up; median (min .. max)
per call, the bytes of live cars read per second (8 B per car) against the 8 TB/s HBM figure of the README, and the
kernel's answer checked against the torch route's on the spot (what subtractions and comparisons decide exactly; the
sums and what a division decides closely: torch adds in another order and rounds its divisions its own way).

    python tools/time_following.py [--out FILE] [--calls 50] [--small]
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
from gym_traffic.core import RoadFollowing, TfxEngine  # noqa: E402
from time_measures import HALT, HBM_BYTES_PER_S, nearly_empty, timed  # noqa: E402

PLATOON_GAP, V_MIN, TTC_CRIT = 10.0, 0.5, 3.0


def export_route(eng, x_from):
    """The eleven fields from the ring image: tfx_export_ring, then masked torch operations over (leader, follower) pairs."""
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
    xf, vf, xl, vl = x[..., 1:], v[..., 1:], x[..., :-1], v[..., :-1]
    pair = inr[..., 1:]
    g = (xl - xf) - float(eng.cfg.car_l)
    dv = vf - vl
    inf, zero = torch.full_like(g, float("inf")), torch.zeros_like(g)
    timed_ = pair & (vf >= V_MIN)
    closing = pair & (dv > 0) & (g > 0)
    ttc = g / dv
    drac = (dv * dv) / (g + g)

    def count(m):
        return m.sum(dim=-1, dtype=torch.int32)
    return RoadFollowing(count(inr), count(pair), count(pair & (g <= PLATOON_GAP)), count(pair & (g < 0)),
                         torch.where(pair, g, zero).sum(dim=-1), torch.where(pair, g, inf).min(dim=-1).values,
                         count(timed_), torch.where(timed_, g / vf, zero).sum(dim=-1), count(closing & (ttc < TTC_CRIT)),
                         torch.where(closing, ttc, inf).min(dim=-1).values, torch.where(closing, drac, zero).max(dim=-1).values)


def case(title, eng, length, calls, lines):
    x_from = length - 50.0
    cars = int(eng.cars_on_roads_flat().sum())
    t_new = timed(lambda: eng.road_following(PLATOON_GAP, V_MIN, TTC_CRIT, x_from), calls)
    t_all = timed(lambda: eng.road_following(PLATOON_GAP, V_MIN, TTC_CRIT, None), calls)
    t_sib = timed(lambda: eng.road_measures(HALT, None), calls)
    t_old = timed(lambda: export_route(eng, x_from), max(5, calls // 5), warmup=2)
    got = eng.road_following(PLATOON_GAP, V_MIN, TTC_CRIT, x_from)
    want = export_route(eng, x_from)
    # what comparisons and subtractions alone decide is equal whatever torch's division rounds like; the rest is close
    exact = ("n_cars", "n_pairs", "n_joined", "n_overlap", "n_hw", "gap_min")
    same = all(bool(torch.equal(getattr(got, f), getattr(want, f))) for f in exact)
    close = all(bool(torch.allclose(getattr(got, f), getattr(want, f), rtol=1e-5, atol=1e-3))
                for f in ("gap_sum", "hw_sum", "ttc_min", "drac_max"))
    off = int((got.n_conflict != want.n_conflict).sum())
    pairs = int(got.n_pairs.sum())
    eng.drop_staging()
    rate = cars * 8 / (t_all[0] * 1e-6)
    lines.append("%s: %d envs, %d roads, %d cars on the roads (%.1f per road), %d pairs with x_F >= L - 50"
                 % (title, eng.E, eng.E * eng.R, cars, cars / (eng.E * eng.R), pairs))
    lines.append("  tfx_road_following, x_from = L - 50     %9.1f (%.1f .. %.1f) us" % t_new)
    lines.append("  tfx_road_following, every car in range  %9.1f (%.1f .. %.1f) us" % t_all)
    lines.append("  tfx_road_measures, every car in range   %9.1f (%.1f .. %.1f) us   following / measures x%.2f"
                 % (t_sib + (t_all[0] / t_sib[0],)))
    lines.append("  tfx_export_ring + torch expressions     %9.1f (%.1f .. %.1f) us   x%.1f" % (t_old + (t_old[0] / t_new[0],)))
    lines.append("  live-car bytes read: %.3e B/s = %.1f %% of %.0e B/s; counters and gap_min equal the export route's: %s, sums, "
                 "ttc_min, drac_max close: %s, roads whose n_conflict differs: %d"
                 % (rate, 100 * rate / HBM_BYTES_PER_S, HBM_BYTES_PER_S, same, close, off))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="64 envs per shape: a rehearsal, not a measurement")
    a = ap.parse_args()
    lines = ["tfx_road_following, all eleven outputs: median (min .. max) per call over %d calls, events around each call" % a.calls]
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
