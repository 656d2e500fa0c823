"""A time-space diagram of one arterial, from car lists taken on the device (tfx_car_list): a few envs of a batch with
on-device arrivals under the on-device greedy controller (TFX_ACTION_GREEDY); after every tick TrafficVecEnv.cars() lists
the cars of the chosen envs on the roads of one arterial - one read-only launch that stores them compacted - and the list
is copied, still on the device, into one log tensor [ticks, max_cars].  Nothing in the loop waits for the device; at the
end the log comes to the host once and every chosen env becomes one PNG: a column per tick, the arterial from its entrance
(top) to its exit (bottom), every car a pixel coloured by its speed (red: standing, green: at the desired speed) - queues
show as red wedges that grow against the direction of travel and dissolve in green waves.  Prints the median time per
tick split into step / cars.

    python tools/timespace_demo.py --envs 4 --ticks 400 --line 1 --direction 0 --out timespace.png
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

from gym_traffic.envs.vec_env import TrafficVecEnv  # noqa: E402


def run(a):
    N, T = a.batch, a.ticks
    venv = TrafficVecEnv(N, a.m, a.n, a.length, capacity=a.capacity, spawn='device', seed=a.seed,
                         local_cars_per_sec=a.cars_per_sec)
    eng, g = venv.engine, venv.graph
    venv.reset(np.random.RandomState(a.seed).randint(2, size=(N, eng.I)).astype(np.int32))
    eng.set_greedy(a.spacing)
    mask = venv.arterial(a.line, a.direction)
    # where every road of the chain starts along the arterial, in road lengths
    place = np.full(eng.R, -1, np.int64)
    road = int(np.flatnonzero(mask & ~np.isin(np.arange(eng.R), g.nexts[np.flatnonzero(mask)]))[0])   # no road leads into it
    chain = []
    while road >= 0:
        place[road] = len(chain)
        chain.append(road)
        road = int(g.nexts[road])
    envs = torch.arange(a.envs, dtype=torch.int32, device=eng.device)       # the envs listed: on the device, once
    L = a.envs * len(chain) * (eng.C - 1)                                  # room for every ring slot of the chain
    log_xv = torch.zeros((T, L, 2), dtype=torch.float32, device=eng.device)
    log_road = torch.zeros((T, L), dtype=torch.int32, device=eng.device)
    log_n = torch.zeros((T,), dtype=torch.int32, device=eng.device)
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(T)]
    for t in range(T):
        ev[t][0].record()
        eng.step(1)
        ev[t][1].record()
        c = venv.cars(envs, mask, max_cars=L)                               # no host synchronisation
        log_xv[t].copy_(c.xv)
        log_road[t].copy_(c.road)
        log_n[t].copy_(c.n)
        ev[t][2].record()
    torch.cuda.synchronize()
    skip = min(3, T - 1)
    ms = np.array([[e[i].elapsed_time(e[i + 1]) for i in range(2)] for e in ev[skip:]])
    return dict(step_ms=float(np.median(ms[:, 0])), cars_ms=float(np.median(ms[:, 1])), xv=log_xv.cpu().numpy(),
                road=log_road.cpu().numpy(), n=log_n.cpu().numpy(), place=place, chain=chain, R=eng.R, v0=float(eng.car["car_v0"]))


def diagram(r, a):
    """uint8 [envs * (H + 1) - 1, ticks * px, 3]: one band per env, white background, a white line between bands"""
    T, roads = a.ticks, len(r["chain"])
    H = roads * a.rows
    img = np.full((a.envs, H, T, 3), 255, np.uint8)
    for t in range(T):
        n = int(r["n"][t])
        key = r["road"][t, :n].astype(np.int64)
        x, v = r["xv"][t, :n, 0], r["xv"][t, :n, 1]
        sel, rid = key // r["R"], key % r["R"]
        pos = (r["place"][rid] + np.clip(x / a.length, 0.0, 1.0)) / roads            # 0 at the entrance, 1 at the exit
        y = np.minimum((pos * H).astype(np.int64), H - 1)
        f = np.clip(v / r["v0"], 0.0, 1.0)
        img[sel, y, t] = np.stack([255 * (1 - f), 200 * f, np.zeros_like(f)], axis=-1).astype(np.uint8)
    img[:, ::a.rows, :, :] = np.minimum(img[:, ::a.rows, :, :], 225)                 # a faint line at every stop line
    bands = [np.repeat(b, a.px, axis=1) for b in img]
    gap = np.full((1, T * a.px, 3), 255, np.uint8)
    out = []
    for b in bands:
        out += [b, gap]
    return np.concatenate(out[:-1], axis=0)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4, help="envs 0 .. envs-1 are listed and drawn")
    ap.add_argument("--batch", type=int, default=0, help="envs in the batch (default: as many as are drawn)")
    ap.add_argument("--ticks", type=int, default=400)
    ap.add_argument("--line", type=int, default=1, help="the row (directions 0, 1) or column (2, 3) of the arterial")
    ap.add_argument("--direction", type=int, default=0, help="0 eastbound, 1 westbound, 2 towards higher rows, 3 towards lower rows")
    ap.add_argument("--spacing", type=int, default=10, help="ticks between greedy decisions")
    ap.add_argument("--rows", type=int, default=48, help="pixel rows per road")
    ap.add_argument("--px", type=int, default=2, help="pixel columns per tick")
    ap.add_argument("--m", type=int, default=4)
    ap.add_argument("--n", type=int, default=4)
    ap.add_argument("--length", type=float, default=200.0)
    ap.add_argument("--capacity", type=int, default=34)
    ap.add_argument("--cars-per-sec", type=float, default=0.12)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default="timespace.png", help="the PNG")
    a = ap.parse_args(argv)
    a.batch = max(a.batch, a.envs)
    r = run(a)
    from PIL import Image
    img = diagram(r, a)
    d = os.path.dirname(os.path.abspath(a.out))
    os.makedirs(d, exist_ok=True)
    Image.fromarray(img).save(a.out)
    print("time-space demo: %d envs (%dx%d grid, L=%g, C=%d) under the on-device greedy controller, %d ticks; the %d roads of "
          "line %d, direction %d of envs 0..%d listed after every tick" % (a.batch, a.m, a.n, a.length, a.capacity, a.ticks,
                                                                          len(r["chain"]), a.line, a.direction, a.envs - 1))
    print("%d cars listed in all (%.1f per tick)   PNG of %d x %d in %s" % (int(r["n"].sum()), float(r["n"].mean()),
                                                                           img.shape[0], img.shape[1], a.out))
    print("median ms per tick: step %.3f   ms per cars call %.3f" % (r["step_ms"], r["cars_ms"]))
    return r


if __name__ == "__main__":
    main()
