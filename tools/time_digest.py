"""Time tfx_state_digest (one memset and one launch) for 1, 16 and 256 chosen envs and for all envs, with parts CARS,
'state' and 'all', with and without the per-road words, next to three calls that were there before it, in the same run on
the same state: tfx_road_following, which loads the same (x, v) rows and stores next to nothing - the bound a
bandwidth-limited digest should sit near; tfx_car_list of the same selection; and the route the digest replaces,
tfx_export_ring of the whole batch plus the copy of the chosen envs' rings to the host.

Shape: cfg2 x 4096 envs at the benchmark's density (its prefill and settle), validate mode so that the spawn plane
exists.  Events around each of `--calls` calls after a warm-up; median (min .. max) per call; bytes the digest's walk
loads per second (8 B of (x, v) per car, 4 B of side word where the parts need it); the device's digests checked against
the NumPy definition for a few envs on the spot.

    python tools/time_digest.py [--out FILE] [--calls 50] [--small]
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
from gym_traffic import devrng  # noqa: E402
from gym_traffic import workload as wl  # noqa: E402
from time_measures import timed  # noqa: E402

SELECTIONS = (1, 16, 256, None)
STATE = nat.DIGEST_CARS | nat.DIGEST_ROWS | nat.DIGEST_RING | nat.DIGEST_LIGHTS | nat.DIGEST_OBS
PARTS = (("CARS", nat.DIGEST_CARS, 8), ("'state'", STATE, 8), ("'all'", STATE | nat.DIGEST_SPAWN, 12))


def launch_only(eng, ids, n_sel, parts, env, road):
    ip = None if ids is None else C.c_void_p(ids.data_ptr())
    ep, rp = C.c_void_p(env.data_ptr()), None if road is None else C.c_void_p(road.data_ptr())
    st = eng._stream()

    def call():
        nat.check(eng.lib.tfx_state_digest(eng.h, ip, n_sel, None, parts, ep, rp, 0, st))
    return call


def export_route(eng, ids):
    """what a host-side comparison needs of the chosen envs: tfx_export_ring of the whole batch, then their rings and ring
    words copied to the host"""
    xv = eng.xv
    if ids is not None:
        xv = xv[ids.long()]
    return xv.cpu(), eng.leading.cpu(), eng.lastcar.cpu()


def equals_the_definition(eng, envs, parts):
    idx = torch.as_tensor(envs, dtype=torch.int64).to(eng.device)

    def rows(t):        # the chosen envs' rows alone travel to the host
        return t[idx].cpu().numpy()
    ring = rows(eng.xv)
    want = devrng.state_digest(ring[..., 0], ring[..., 1], rows(eng.w) if eng.P == 3 else None, None, rows(eng.leading),
                               rows(eng.lastcar), eng.C, parts, obs=rows(eng.obs), rewards=rows(eng.rewards),
                               waiting=rows(eng.waiting), passed_dst=rows(eng.passed_dst), done_tick=rows(eng.done_tick),
                               I=eng.I, r=eng.r)
    got = eng.state_digest(envs, parts=parts, per_road=True)
    return all(g.cpu().numpy().tobytes() == m.view(np.int64).tobytes() for g, m in zip(got, want))


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
    lines = ["tfx_state_digest: median (min .. max) per call over %d calls, events around each call" % a.calls,
             "%s at the benchmark's density, validate mode: %d envs, %d roads, %d cars on the roads (%.1f per road)"
             % (name, eng.E, eng.E * eng.R, cars, cars / (eng.E * eng.R))]
    ok = equals_the_definition(eng, [0, E // 2, E - 1, 0], STATE | nat.DIGEST_SPAWN)
    eng.drop_staging()
    lines.append("  the device's digests of envs 0, %d, %d equal devrng.state_digest bit for bit: %s" % (E // 2, E - 1, ok))
    t_floor = timed(lambda: eng.road_following(2.0, 0.5, 3.0), a.calls)
    lines.append("  tfx_road_following, every car of the batch (the same (x, v) loads, a few words stored per road) %9.1f (%.1f .. %.1f) us"
                 % t_floor)
    rng = np.random.RandomState(0)
    per_env = cars / float(E)
    for k in SELECTIONS:
        if k is not None and k > E:
            continue
        ids = None if k is None else torch.as_tensor(np.sort(rng.choice(E, size=k, replace=False)).astype(np.int32)).to(eng.device)
        n_sel = E if k is None else k
        title = "all %d envs" % E if k is None else "%d chosen env%s" % (k, "" if k == 1 else "s")
        n_cars = int(eng.car_list(ids).n)
        lines.append("  %s: %d cars" % (title, n_cars))
        env = torch.zeros((n_sel,), dtype=torch.int64, device=eng.device)
        road = torch.zeros((n_sel, eng.R), dtype=torch.int64, device=eng.device)
        for what, parts, per_car in PARTS:
            for rd, label in ((None, "env words only"), (road, "with road words")):
                t = timed(launch_only(eng, ids, n_sel, parts, env, rd), a.calls)
                lines.append("    digest %-8s %-16s %9.1f (%.1f .. %.1f) us   %.3e B/s loaded"
                             % ((what, label) + t + (n_cars * per_car / (t[0] * 1e-6),)))
        t_call = timed(lambda: eng.state_digest(ids, parts=STATE), a.calls)
        lines.append("    TfxEngine.state_digest 'state', whole Python call %9.1f (%.1f .. %.1f) us" % t_call)
        full = eng.car_list(ids)
        N = int(full.n)
        planes = list(full[2:])
        t_list = timed(lambda: eng.car_list(ids, max_cars=N, out=planes), a.calls)
        lines.append("    tfx_car_list of the selection, all planes (whole call) %9.1f (%.1f .. %.1f) us" % t_list)
        t_old = timed(lambda: export_route(eng, ids), max(5, a.calls // 5), warmup=2)
        eng.drop_staging()
        lines.append("    tfx_export_ring of the batch + copy of the selection to the host %9.1f (%.1f .. %.1f) us" % t_old)
    for ln in lines:
        print(ln)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n\n")


if __name__ == "__main__":
    main()
