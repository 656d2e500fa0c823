"""Time tfx_put_cars (TfxEngine.put_cars: one launch) for 1, 16, 256 and all chosen envs, xv only and all planes, with plain
and with non-temporal row stores (TFX_PUT_NT, read per call), and TrafficVecEnv / TfxEngine.unpack_envs end to end, against
the two routes there were before the call existed, in the same run on the same state: tfx_export_ring of the whole batch
followed by tfx_import_ring + tfx_refresh (what an edit of one env cost), and tfx_clone_envs of as many envs from a second
batch of the same world.  tfx_car_list of the same selection runs alongside: it moves the same bytes the other way.

Shape: cfg2 x 4096 envs at the benchmark's density (its prefill and settle), validate mode so that the spawn plane exists;
the lists are those of a second batch that settled 40 ticks longer.  Events around each of `--calls` calls after a warm-up;
median (min .. max) per call; achieved load bytes per second of the launch (8 B of xv, 1 B of row, 4 B of spawn per car);
what was put is read back with tfx_car_list and compared on the spot, bit for bit.

    python tools/time_put_cars.py [--out FILE] [--calls 50] [--small]
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


def launch_only(eng, ids, n_sel, offsets, cap, xv, row, spawn, leading):
    b = nat.TfxPutBuffers(*[None if t is None else C.c_void_p(t.data_ptr()) for t in (xv, row, spawn, leading, None)])
    ip = None if ids is None else C.c_void_p(ids.data_ptr())
    op = C.c_void_p(offsets.data_ptr())
    st = eng._stream()

    def call():
        nat.check(eng.lib.tfx_put_cars(eng.h, ip, n_sel, None, op, cap, C.byref(b), 0, None, 0, st))
    return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="64 envs: a rehearsal, not a measurement")
    a = ap.parse_args()
    name = "cfg2"
    E = 64 if a.small else 4096
    settle = wl.SETTLE_TICKS.get(name, 100)
    eng = wl.setup_engine(name, envs=E, validate=True)
    eng.step(settle)
    src = wl.setup_engine(name, envs=E, validate=True)
    src.step(settle + 40)
    cars = int(src.cars_on_roads_flat().sum())
    lines = ["tfx_put_cars: median (min .. max) per call over %d calls, events around each call" % a.calls,
             "%s at the benchmark's density, validate mode: %d envs, %d roads, %d cars on the source's roads (%.1f per road)"
             % (name, eng.E, eng.E * eng.R, cars, cars / (eng.E * eng.R))]
    t_old = timed(lambda: (eng.xv, eng.refresh()), max(5, a.calls // 5), warmup=2)
    eng.drop_staging()
    lines.append("  tfx_export_ring of the batch, then tfx_import_ring + tfx_refresh (any number of envs) %9.1f (%.1f .. %.1f) us"
                 % t_old)
    rng = np.random.RandomState(0)
    for k in SELECTIONS:
        if k is not None and k > E:
            continue
        ids = None if k is None else torch.as_tensor(np.sort(rng.choice(E, size=k, replace=False)).astype(np.int32)).to(eng.device)
        n_sel = E if k is None else k
        lst = src.car_list(ids)                        # sized exactly
        N = int(lst.n)
        leading = (src.leading if ids is None else src.leading[ids.long()]).contiguous()
        title = "all %d envs" % E if k is None else "%d chosen env%s" % (k, "" if k == 1 else "s")
        lines.append("  %s: %d cars" % (title, N))
        t_list = timed(launch_only_list(src, ids, n_sel, lst), a.calls)
        lines.append("    tfx_car_list of the same selection, all planes, launch alone   %7.1f (%.1f .. %.1f) us" % t_list)
        for what, row, spawn, per_car in (("xv only", None, None, 8), ("all planes", lst.row, lst.spawn, 13)):
            for nt in ("0", "1"):
                os.environ["TFX_PUT_NT"] = nt
                t = timed(launch_only(eng, ids, n_sel, lst.offsets, N, lst.xv, row, spawn, leading), a.calls)
                lines.append("    put_cars, %-10s %s stores  launch alone %7.1f (%.1f .. %.1f) us   %.3e B/s loaded"
                             % ((what, "non-temporal" if nt == "1" else "plain       ") + t + (N * per_car / (t[0] * 1e-6),)))
            os.environ.pop("TFX_PUT_NT")
        back = eng.car_list(ids)
        same = all(torch.equal(getattr(back, f).view(torch.uint8), getattr(lst, f).view(torch.uint8)) for f in ("offsets", "xv", "row", "spawn"))
        packed = src.pack_envs(torch.arange(E, device=eng.device) if ids is None else ids)
        dst = torch.arange(E, device=eng.device) if ids is None else ids.long()
        t_unpack = timed(lambda: eng.unpack_envs(dst, packed), a.calls)
        lines.append("    unpack_envs end to end (the launch and nine torch index writes)     %9.1f (%.1f .. %.1f) us; "
                     "the list reads back bit for bit: %s" % (t_unpack + (same,)))
        idx = torch.full((E,), -1, dtype=torch.int32, device=eng.device)
        idx[dst] = dst.to(torch.int32)
        t_clone = timed(lambda: eng.clone_envs(idx, source=src), a.calls)
        lines.append("    tfx_clone_envs of the same envs from the second batch               %9.1f (%.1f .. %.1f) us" % t_clone)
    for ln in lines:
        print(ln)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n\n")


def launch_only_list(eng, ids, n_sel, lst):
    b = nat.TfxCarListBuffers(*[C.c_void_p(t.data_ptr()) for t in (lst.xv, lst.road, lst.row, lst.spawn)])
    ip = None if ids is None else C.c_void_p(ids.data_ptr())
    op = C.c_void_p(lst.offsets.data_ptr())
    st, N = eng._stream(), int(lst.n)

    def call():
        nat.check(eng.lib.tfx_car_list(eng.h, ip, n_sel, None, op, N, C.byref(b), 0, st))
    return call


if __name__ == "__main__":
    main()
