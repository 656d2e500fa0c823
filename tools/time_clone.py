"""Time tfx_clone_envs on the benchmark's workload against two yardsticks taken in the same run:
the export / index / import / refresh route (what there was before the call existed: a ring-layout copy of the
whole batch, torch indexing, and back) and one two-tick tfx_step of the same batch.

Events around `--calls` calls after a warm-up, per call; cases: (a) every env cloned from 20 sources, (b) 1 % of the
envs.  Prints one line per figure; `--out FILE` also appends them to FILE.

    python tools/time_clone.py --config cfg2            # 4096 x 16x16, C = 66, after the benchmark's settle
    python tools/time_clone.py --config cfg1            # 1024 x 4x4
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


def timed(fn, calls, warmup=5):
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


def old_route(eng, src_long, mask):
    """The same clone through the ring-layout staging copy: export, index, import, refresh."""
    xv = eng.xv                                        # tfx_export_ring of the whole batch
    m4 = mask[:, None, None, None]
    xv.copy_(torch.where(m4, xv[src_long], xv))
    for name in ("leading", "lastcar", "obs", "rewards", "waiting", "passed_dst", "done_tick"):
        t = getattr(eng, name)
        t.copy_(torch.where(mask.view(-1, *([1] * (t.dim() - 1))), t[src_long], t))
    eng.refresh()                                      # tfx_import_ring + tfx_refresh


def never_cloned(a):
    lines = ["%s, a handle that never clones: median (min .. max) us per call over %d calls" % (a.config, a.calls)]
    for stream in ("periodic", "poisson"):
        eng = wl.setup_engine(a.config, envs=a.envs)
        if stream == "poisson":
            eng.set_poisson(0.5 * eng.n_entry / wl.SPAWN_PERIOD, seed=1)
        eng.step(wl.SETTLE_TICKS.get(a.config, 100))
        for rep in range(2):
            lines.append("  %-8s tfx_step(2)        %9.1f (%.1f .. %.1f)" % ((stream,) + timed(lambda: eng.step(2, update_done=False), a.calls)))
            lines.append("  %-8s agent_step(10)     %9.1f (%.1f .. %.1f)" % ((stream,) + timed(lambda: eng.agent_step(10), a.calls)))
        del eng
    for ln in lines:
        print(ln)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg2", choices=sorted(wl.CONFIGS))
    ap.add_argument("--envs", type=int, default=None)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--out", default=None)
    ap.add_argument("--never-cloned", action="store_true",
                    help="time tfx_step(2) and 10-tick decisions of a handle that never clones (periodic arrivals, and the "
                         "on-device Poisson stream) and nothing else: run it on two commits to compare them")
    a = ap.parse_args()
    if a.never_cloned:
        return never_cloned(a)
    eng = wl.setup_engine(a.config, envs=a.envs)
    E = eng.E
    eng.step(wl.SETTLE_TICKS.get(a.config, 100))
    torch.cuda.synchronize()
    k = torch.arange(E, dtype=torch.int32, device=eng.device)
    cases = {"all envs from 20 sources": torch.where(k < 20, torch.full_like(k, -1), k % 20),
             "1 %% of the envs (%d)" % max(1, E // 100): torch.where((k >= 20) & (k % 100 == 20 % 100), k % 20, torch.full_like(k, -1))}
    lines = ["%s" % wl.describe(a.config).replace("%d envs/GPU" % wl.CONFIGS[a.config]["envs"], "%d envs" % E),
             "cars on the roads: %d" % int(eng.cars_on_roads_flat().sum()),
             "median (min .. max) us per call over %d calls, events around each call" % a.calls]
    for _ in range(2):                                 # (twice: the run-to-run spread of the yardstick)
        lines.append("tfx_step(2), never cloned yet       %9.1f (%.1f .. %.1f)" % timed(lambda: eng.step(2, update_done=False), a.calls))
    for name, src in cases.items():
        mask, src_long = src >= 0, src.clamp(min=0).long()
        n = int(mask.sum())
        t_new = timed(lambda: eng.clone_envs(src), a.calls)
        # the launch alone: the C call, without the torch launches that fix up the Python-side `done` flags
        import ctypes as C
        from gym_traffic import _native as nat
        raw, st = C.c_void_p(src.data_ptr()), eng._stream()
        t_k = timed(lambda: nat.check(eng.lib.tfx_clone_envs(eng.h, eng.h, raw, 0, st)), a.calls)
        assert eng.clone_skipped() == 0
        t_old = timed(lambda: old_route(eng, src_long, mask), max(5, a.calls // 5), warmup=2)
        lines.append("%-36s clone_envs() %9.1f (%.1f .. %.1f)   tfx_clone_envs alone %9.1f (%.1f .. %.1f)   "
                     "export/index/import/refresh %9.1f (%.1f .. %.1f)   x%.1f"
                     % ((name + ", %d cloned:" % n,) + t_new + t_k + t_old + (t_old[0] / t_new[0],)))
    eng.drop_staging()
    lines.append("tfx_step(2), after the clones       %9.1f (%.1f .. %.1f)" % timed(lambda: eng.step(2, update_done=False), a.calls))
    for ln in lines:
        print(ln)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n\n")


if __name__ == "__main__":
    main()
