"""Time tfx_car_list (TfxEngine.car_list: the torch expressions for the offsets, then one launch) for 1, 16 and 256 chosen
envs and for all envs, xv only and all planes, against its two baselines, in the same run on the same state:
tfx_road_following, the sibling that walks the same cars with the same loads and stores a few words per road - the floor
of any kernel that reads every car - and the route there was before the call existed: tfx_export_ring of every ring slot
of the whole batch into a preallocated staging copy plus the torch gather that compacts the chosen envs' cars.

Shape: cfg2 x 4096 envs at the benchmark's density (its prefill and settle), validate mode so that the spawn plane
exists.  Events around each of `--calls` calls after a warm-up; median (min .. max) per call; the launch alone (offsets
and planes prepared once) beside the whole call; achieved store bytes per second of the launch (8 B of xv, 4 B of road,
1 B of row, 4 B of spawn per car); the kernel's list checked against the export route's on the spot, bit for bit.

    python tools/time_car_list.py [--out FILE] [--calls 50] [--small]
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "traffic-env_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from gym_traffic import _native as nat  # noqa: E402
from gym_traffic import workload as wl  # noqa: E402
from time_measures import timed  # noqa: E402

SELECTIONS = (1, 16, 256, None)


def export_route(eng, ids):
    """(x, v) of the chosen envs' cars, compacted in (s, road, rank) order: tfx_export_ring of the whole batch, then a
    masked gather of the chosen envs' rings in ring order"""
    xv = eng.xv                                        # tfx_export_ring of the whole batch into the staging copy
    Cc = eng.C
    ld, lc = eng.leading.long(), eng.lastcar.long()
    if ids is not None:
        xv, ld, lc = xv[ids.long()], ld[ids.long()], lc[ids.long()]
    n = (lc - ld + (ld > lc) * (Cc - 1)).clamp(0, Cc - 1)
    j = torch.arange(Cc - 1, device=eng.device)
    slot = ld[..., None] + 1 + j
    slot = torch.where(slot > Cc - 1, slot - (Cc - 1), slot)
    live = j < n[..., None]
    slot = torch.where(live, slot, torch.zeros_like(slot))
    cars = torch.gather(xv, 2, slot[..., None].expand(-1, -1, -1, 2))
    return cars[live]                                  # (a host synchronisation: the size of the result)


def launch_only(eng, ids, n_sel, offsets, cap, planes):
    b = nat.TfxCarListBuffers(*[None if t is None else C.c_void_p(t.data_ptr()) for t in planes])
    ip = None if ids is None else C.c_void_p(ids.data_ptr())
    op = C.c_void_p(offsets.data_ptr())
    st = eng._stream()

    def call():
        nat.check(eng.lib.tfx_car_list(eng.h, ip, n_sel, None, op, cap, C.byref(b), 0, st))
    return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="64 envs: a rehearsal, not a measurement")
    a = ap.parse_args()
    name = "cfg2"
    E = 64 if a.small else 4096
    eng = wl.setup_engine(name, envs=E, validate=True)
    eng.step(wl.SETTLE_TICKS.get(name, 100))
    cars = int(eng.cars_on_roads_flat().sum())
    lines = ["tfx_car_list: median (min .. max) per call over %d calls, events around each call" % a.calls,
             "%s at the benchmark's density, validate mode: %d envs, %d roads, %d cars on the roads (%.1f per road)"
             % (name, eng.E, eng.E * eng.R, cars, cars / (eng.E * eng.R))]
    t_floor = timed(lambda: eng.road_following(2.0, 0.5, 3.0), a.calls)
    lines.append("  tfx_road_following, every car of the batch (the same loads, a few words stored per road) %9.1f (%.1f .. %.1f) us"
                 % t_floor)
    rng = np.random.RandomState(0)
    for k in SELECTIONS:
        if k is not None and k > E:
            continue
        ids = None if k is None else torch.as_tensor(np.sort(rng.choice(E, size=k, replace=False)).astype(np.int32)).to(eng.device)
        n_sel = E if k is None else k
        full = eng.car_list(ids)                       # sized exactly
        N = int(full.n)
        title = "all %d envs" % E if k is None else "%d chosen env%s" % (k, "" if k == 1 else "s")
        lines.append("  %s: %d cars" % (title, N))
        for what, planes, per_car in (("xv only", [full.xv, None, None, None], 8), ("all planes", list(full[2:]), 17)):
            t_call = timed(lambda: eng.car_list(ids, max_cars=N, out=planes), a.calls)
            t_launch = timed(launch_only(eng, ids, n_sel, full.offsets, N, planes), a.calls)
            rate = N * per_car / (t_launch[0] * 1e-6)
            lines.append("    car_list, %-10s  whole call %9.1f (%.1f .. %.1f) us" % ((what,) + t_call))
            lines.append("    %-20s  launch alone %7.1f (%.1f .. %.1f) us   %.3e B/s stored" % (("",) + t_launch + (rate,)))
        t_old = timed(lambda: export_route(eng, ids), max(5, a.calls // 5), warmup=2)
        same = bool(torch.equal(export_route(eng, ids).view(torch.int32), eng.car_list(ids).xv.view(torch.int32)))
        eng.drop_staging()
        lines.append("    tfx_export_ring of the batch + torch gather  %9.1f (%.1f .. %.1f) us; xv equals the export route's bit for bit: %s"
                     % (t_old + (same,)))
    for ln in lines:
        print(ln)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n\n")


if __name__ == "__main__":
    main()
