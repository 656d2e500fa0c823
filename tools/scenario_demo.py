"""A scenario library on the device, and an incident written into a running env (tfx_put_cars): a small batch runs under
the on-device greedy controller (TFX_ACTION_GREEDY) with a tidal demand (spawn='demand'); every few decisions
TrafficVecEnv.pack_envs takes a few of its envs - live cars only, with the counters, lights and clock that go with them -
into a library, a list of dicts of device tensors, which is also written with torch.save and read back.  A second batch
with a DIFFERENT number of envs then starts every env from a random library entry through unpack_envs and runs on.
Last, one env of it becomes the twin of another (clone_envs: the same arrivals from then on) and the head car of one
arterial road of the first stalls: every tick cars() lists the arterial, the car is pinned in torch and set_cars() writes
the list back; the queue that builds behind it (measures()) is printed against the unedited twin's.  The orchestration is
on the CPU, everything that touches a car runs on the device.

    python tools/scenario_demo.py --envs 16 --restart-envs 24 --decisions 24 --every 4
"""
import argparse
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "traffic-env_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from gym_traffic.envs.vec_env import TrafficVecEnv  # noqa: E402


def make(a, envs):
    """a batch under the tidal demand of tools/demand_demo.py: N-S heavy and E-W heavy segments in turn"""
    ns = np.r_[np.zeros(2 * a.m), np.ones(2 * a.n)]
    w = np.stack([np.where(ns > 0, a.tide, 1.0), np.where(ns > 0, 1.0, a.tide)])
    per_tick = a.cars_per_sec * 0.5 * (2 * a.m + 2 * a.n)
    demand = dict(means=np.array([[per_tick, per_tick]]), weights=w[None], seg_ticks=4 * a.ticks, tick_offset=0)
    venv = TrafficVecEnv(envs, a.m, a.n, a.length, capacity=a.capacity, spawn='demand', seed=a.seed, demand=demand)
    venv.reset(np.random.RandomState(a.seed).randint(2, size=(envs, a.m * a.n)).astype(np.int32))
    return venv


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=16, help="envs of the batch the library is taken from")
    ap.add_argument("--restart-envs", type=int, default=24, help="envs of the batch that starts from the library (>= 2)")
    ap.add_argument("--decisions", type=int, default=24)
    ap.add_argument("--every", type=int, default=4, help="decisions between two visits of the library")
    ap.add_argument("--take", type=int, default=2, help="envs packed per visit")
    ap.add_argument("--ticks", type=int, default=10)
    ap.add_argument("--stall-ticks", type=int, default=60)
    ap.add_argument("--m", type=int, default=3)
    ap.add_argument("--n", type=int, default=3)
    ap.add_argument("--length", type=float, default=150.0)
    ap.add_argument("--capacity", type=int, default=24)
    ap.add_argument("--cars-per-sec", type=float, default=0.1)
    ap.add_argument("--tide", type=float, default=4.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--library", default=None, help="where torch.save writes the library (default: a temporary file)")
    a = ap.parse_args(argv)
    rng = np.random.RandomState(a.seed)
    T = a.ticks

    # ---- 1. the library ---------------------------------------------------------------------------------------------------
    venv = make(a, a.envs)
    venv.engine.set_greedy(T)                                               # one greedy decision per agent step, held for it
    library = []
    for d in range(a.decisions):
        venv.agent_step(n_ticks=T)
        if (d + 1) % a.every == 0:
            for e in rng.choice(a.envs, size=min(a.take, a.envs), replace=False):
                library.append(venv.pack_envs([int(e)]))                    # one env per entry: entries restart envs one by one
    ring_bytes = venv.engine.R * venv.engine.C * 8
    list_bytes = float(np.mean([p["xv"].numel() * 4 + p["offsets"].numel() * 4 + p["row"].numel() for p in library]))
    path = a.library or os.path.join(tempfile.mkdtemp(prefix="scenario_demo_"), "library.pt")
    torch.save(library, path)
    library = torch.load(path, map_location=venv.engine.device, weights_only=True)
    print("scenario demo: %d envs (%dx%d grid, L=%g, C=%d) under the on-device greedy controller and a tidal demand, %d decisions"
          % (a.envs, a.m, a.n, a.length, a.capacity, a.decisions))
    print("library: %d entries taken at ticks %s, %.0f bytes of cars per entry against %d for an env's rings; saved to and "
          "reloaded from %s (%d bytes)" % (len(library), sorted({p["tick"] for p in library}), list_bytes, ring_bytes, path,
                                           os.path.getsize(path)))

    # ---- 2. another batch starts from it --------------------------------------------------------------------------------------
    other = make(a, a.restart_envs)
    other.engine.set_greedy(T)
    picks = rng.randint(len(library), size=a.restart_envs)
    for e, k in enumerate(picks):
        other.unpack_envs([e], library[int(k)])
    start = other.engine.cars_on_roads_flat().sum(dim=1)
    ret = torch.zeros(a.restart_envs, device=other.engine.device)
    for _ in range(max(2, a.decisions // 4)):
        ret += other.agent_step(n_ticks=T)[1].sum(dim=1)
    print("a batch of %d envs started from library entries %s: %.1f cars per env at the start (a cold start has 0), %d cars lost "
          "to a smaller capacity; mean return over %d decisions %.2f"
          % (a.restart_envs, picks.tolist(), float(start.float().mean()), other.engine.put_lost(), max(2, a.decisions // 4),
             float(ret.mean())))

    # ---- 3. an incident: the head car of one arterial road stalls -----------------------------------------------------------
    eng = other.engine
    src = np.full(a.restart_envs, -1, np.int32)
    src[1] = 0
    other.clone_envs(src)                                                   # env 1: the twin of env 0, the same arrivals from now on
    mask = other.arterial(a.m // 2, 0)
    chain = np.flatnonzero(mask)
    road = int(chain[np.argmax(eng.cars_on_roads_flat()[0, torch.as_tensor(chain, device=eng.device)].cpu().numpy())])
    on = torch.as_tensor(mask, device=eng.device).bool()
    pin = None
    print("env 0: the head car of road %d (arterial row %d, eastbound) stalled for %d ticks; queue on the arterial, env 0 / twin:"
          % (road, a.m // 2, a.stall_ticks))
    for t in range(a.stall_ticks):
        other.step(n_ticks=1)
        cars = other.cars(envs=[0], roads=mask)
        head = cars.valid & (cars.road_id == road) & (cars.rank == 0)
        if pin is None and bool(head.any()):
            pin = cars.xv[head][0, 0].clone()                               # where it stands from now on
        if pin is not None and bool(head.any()):
            xv = cars.xv.clone()
            xv[head, 0] = pin
            xv[head, 1] = 0.0
            other.set_cars(cars._replace(xv=xv), envs=[0], roads=mask)
        if (t + 1) % max(1, a.stall_ticks // 6) == 0:
            m = other.measures()
            q = m.queue[:2][:, on].sum(dim=1).cpu().numpy()
            h = m.n_halted[:2][:, on].sum(dim=1).cpu().numpy()
            print("  tick %3d: stalled %s   queued cars %3d / %3d   halted %3d / %3d"
                  % (t + 1, "at x = %.1f" % float(pin) if pin is not None else "(no car yet)", int(q[0]), int(q[1]), int(h[0]), int(h[1])))
    return 0


if __name__ == "__main__":
    sys.exit(main())
