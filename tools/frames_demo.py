"""A video of what a controller does, from frames drawn on the device (tfx_frames): N batched envs with on-device arrivals
under the on-device greedy controller (TFX_ACTION_GREEDY, algorithms/greedy.py:14-16); after every decision
TrafficVecEnv.frames() draws the chosen envs - one read-only launch over their live cars - and the pictures are copied,
still on the device, into one log tensor [decisions, envs, H, W, 4].  Nothing in the loop waits for the device; at the end
the log comes to the host once and every picture is written as a PNG (white background, roads in their lights' colours,
cars as blue bars).  Prints the median time per decision split into env / frames.

    python tools/frames_demo.py --envs 256 --decisions 40 --show 0 17 255 --out /tmp/frames
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
    N, T = a.envs, a.ticks
    venv = TrafficVecEnv(N, a.m, a.n, a.length, capacity=a.capacity, spawn='device', seed=a.seed,
                         local_cars_per_sec=a.cars_per_sec)
    eng = venv.engine
    venv.reset(np.random.RandomState(a.seed).randint(2, size=(N, eng.I)).astype(np.int32))
    eng.set_greedy(T)                                                   # one greedy decision per agent step, held for it
    show = torch.as_tensor(np.asarray(a.show, np.int32)).to(eng.device)   # the envs drawn: on the device, once
    H, W = eng.frame_size(a.px)
    log = torch.empty((a.decisions, len(a.show), H, W, 4), dtype=torch.uint8, device=eng.device)
    ret = torch.zeros(N, device=eng.device)
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(a.decisions)]
    for d in range(a.decisions):
        ev[d][0].record()
        _, rew, _ = venv.agent_step(n_ticks=T)
        ev[d][1].record()
        log[d].copy_(venv.frames(show, px=a.px))                        # the engine's tensor: only its road pixels are rewritten
        ev[d][2].record()
        ret += rew.sum(dim=1)
    torch.cuda.synchronize()
    skip = min(3, a.decisions - 1)
    ms = np.array([[e[i].elapsed_time(e[i + 1]) for i in range(2)] for e in ev[skip:]])
    return dict(ret=float(ret.mean()), env_ms=float(np.median(ms[:, 0])), frames_ms=float(np.median(ms[:, 1])),
                log=log[..., :3].cpu().numpy())


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--decisions", type=int, default=40)
    ap.add_argument("--ticks", type=int, default=10)
    ap.add_argument("--show", type=int, nargs="+", default=[0, 1, 2, 3], help="the envs to draw")
    ap.add_argument("--px", type=int, default=32, help="pixels per road length")
    ap.add_argument("--m", type=int, default=4)
    ap.add_argument("--n", type=int, default=4)
    ap.add_argument("--length", type=float, default=200.0)
    ap.add_argument("--capacity", type=int, default=34)
    ap.add_argument("--cars-per-sec", type=float, default=0.12)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default="frames_out", help="directory for the PNGs")
    a = ap.parse_args(argv)
    r = run(a)
    from PIL import Image
    os.makedirs(a.out, exist_ok=True)
    for d in range(a.decisions):
        for j, k in enumerate(a.show):
            Image.fromarray(r["log"][d, j]).save(os.path.join(a.out, "env%d_%03d.png" % (k, d)))
    print("frames demo: %d envs (%dx%d grid, L=%g, C=%d) under the on-device greedy controller, %d decisions of %d ticks; "
          "envs %s drawn at %d px after every decision" % (a.envs, a.m, a.n, a.length, a.capacity, a.decisions, a.ticks,
                                                          a.show, a.px))
    print("mean return per env %.2f   %d PNGs of %d x %d in %s" % (r["ret"], a.decisions * len(a.show), r["log"].shape[2],
                                                                 r["log"].shape[3], a.out))
    print("median ms per decision: env %.3f   frames %.3f" % (r["env_ms"], r["frames_ms"]))
    return r


if __name__ == "__main__":
    main()
