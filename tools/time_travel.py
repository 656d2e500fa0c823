"""Time TrafficVecEnv.travel_times() per decision (tfx_trip_stats + tfx_car_ages: two read-only launches and a few torch
expressions, no host synchronisation) against the route there was before the calls existed, in the same run on the same
state: trip_times() - the whole [E][trip_cap] log and n_trips copied to the host - plus engine.w - tfx_export_ring of
every ring slot, copied to the host - and NumPy over both.

Shape: 4096 envs of the 16x16 grid (cfg2) in validate mode, warmed up for 1500 ticks of plain steps under the fixed cycle
with a car per entry road every 16 ticks (a car needs some 1000 ticks to cross the grid), so that trips finish in every
env and the logs are partly full.  Events around each of `--calls` calls of travel_times(), each after a step of 10
ticks, so a call reads the trips of those ticks; then around tfx_trip_stats over the whole log and tfx_car_ages alone;
wall-clock time around the host route (it synchronises).  The two routes' figures are compared on the spot.  No
threshold is set: the numbers are a record.

    python tools/time_travel.py [--out FILE] [--calls 30] [--small]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "traffic-env_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from gym_traffic import workload as wl  # noqa: E402
from gym_traffic.envs.vec_env import TrafficVecEnv  # noqa: E402


def host_route(venv):
    """(finished, finished ticks, unfinished, unfinished ticks, oldest) per env from host copies"""
    eng = venv.engine
    logs = venv.trip_times()
    finished = np.array([len(t) for t in logs], np.int64)
    ticks = np.array([np.round(2 * t.astype(np.float64)).sum() for t in logs]).astype(np.int64)
    w = eng.w.cpu().numpy()
    ld, lc = eng.leading.cpu().numpy(), eng.lastcar.cpu().numpy()
    C = eng.C
    n = lc - ld + np.where(ld > lc, C - 1, 0)
    slot = np.arange(C)
    live = (slot >= 1) & (((slot - ld[..., None] - 1) % (C - 1)) < n[..., None])
    age = np.where(live, (np.float32(eng.tick) - w).astype(np.int64), 0)
    return finished, ticks, n.sum(axis=1), age.sum(axis=(1, 2)), age.max(axis=(1, 2))


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warm", type=int, default=150, help="decisions of 10 ticks before anything is timed")
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="64 envs: a rehearsal, not a measurement")
    a = ap.parse_args()
    c = wl.CONFIGS["cfg2"]
    E = 64 if a.small else 4096
    venv = TrafficVecEnv(E, c["m"], c["n"], c["length"], capacity=c["capacity"], spawn='periodic', spawn_period=2 * wl.SPAWN_PERIOD,
                         validate=True)
    eng = venv.engine
    venv.reset()
    for _ in range(a.warm):
        venv.step(None, n_ticks=10, cycle_period=wl.LIGHT_PERIOD)
    venv.travel_times()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.calls)]
    step_ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.calls)]
    for (s0, s1), (t0, t1) in zip(step_ev, ev):
        s0.record()
        venv.step(None, n_ticks=10, cycle_period=wl.LIGHT_PERIOD)
        s1.record()
        t0.record()
        tv = venv.travel_times()
        t1.record()
    torch.cuda.synchronize()
    us = np.array([x.elapsed_time(y) * 1e3 for x, y in ev])
    step_us = np.array([x.elapsed_time(y) * 1e3 for x, y in step_ev])
    whole = timed(lambda: eng.trip_stats(), a.calls)
    ages = timed(lambda: eng.car_ages(), a.calls)
    host_s = []
    for _ in range(2 if a.small else 3):
        t0 = time.perf_counter()
        got = host_route(venv)
        host_s.append(time.perf_counter() - t0)
    same = (np.array_equal(tv.finished.cpu().numpy(), got[0]) and np.array_equal(tv.finished_s.cpu().numpy() * 2, got[1])
            and np.array_equal(tv.unfinished.cpu().numpy(), got[2]) and np.array_equal(tv.unfinished_s.cpu().numpy() * 2, got[3])
            and np.array_equal(tv.oldest_s.cpu().numpy() * 2, got[4]))
    log_mb = eng.trip_times.numel() * 4 / 1e6
    lines = ["travel_times() per decision, %d envs of the 16x16 grid (C = %d) in validate mode after %d ticks: %d trips logged, "
             "%d more fell off the logs (trip_cap %d), %d cars on the map"
             % (E, eng.C, eng.tick, int(got[0].sum()), int(tv.lost.sum()), eng.trip_cap, int(got[2].sum())),
             "  travel_times(): tfx_trip_stats + tfx_car_ages + the derived views  %9.1f (%.1f .. %.1f) us, median (min .. max) of %d"
             % (float(np.median(us)), float(us.min()), float(us.max()), a.calls),
             "  tfx_trip_stats alone, the whole log, no cursor                      %9.1f (%.1f .. %.1f) us" % whole,
             "  tfx_car_ages alone                                                  %9.1f (%.1f .. %.1f) us" % ages,
             "  the decision it follows (a step of 10 ticks)                        %9.1f us, median" % float(np.median(step_us)),
             "  host route: trip_times() (%.0f MB log) + engine.w + NumPy           %9.1f ms, best of %d   x%.0f"
             % (log_mb, 1e3 * min(host_s), len(host_s), 1e6 * min(host_s) / float(np.median(us))),
             "  both routes give the same figures: %s" % same]
    for ln in lines:
        print(ln)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n\n")


if __name__ == "__main__":
    main()
