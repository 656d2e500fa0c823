"""A gap-out actuated signal controller from the road ends (tfx_road_ends): N batched envs under three controllers on the
same spawn='demand' arrival streams - the actuated controller, written in torch over TrafficVecEnv.stop_lines(); the
on-device fixed cycle; the on-device greedy controller (TFX_ACTION_GREEDY, algorithms/greedy.py:14-16).

The actuated controller decides once per agent step, per intersection, from what one read-only launch hands out - the
nearest cars of every approach as (distance to the stop line, speed), and the room at the entrance of every road:
  * a phase is held for at least --min-green decisions and at most --max-green;
  * in between it is held while a car on one of its green approaches is less than --gap seconds from the stop line at
    its current speed (eta_s) - the phase "gaps out" when nobody is about to arrive;
  * it never switches TO a phase whose approaches drive into a road with less room at its entrance than a car length
    plus s0 (entry_room): releasing cars into a full road is what overflows it, and the first overflow ends the episode.
Prints, per controller, the mean return per env and the envs whose episode ended by overflow, and the time one
stop_lines call takes (the launch plus the derived views).

    python tools/actuated_demo.py --envs 256 --decisions 120
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

from gym_traffic.core import ARCHETYPE  # noqa: E402
from gym_traffic.envs.vec_env import TrafficVecEnv  # noqa: E402


def make(a):
    n_entry = 2 * a.m + 2 * a.n
    per_tick = a.cars_per_sec * 0.5 * n_entry                     # cars per env per tick (rate 0.5 s)
    # two segments: the base level, then a peak - the same for every env
    demand = dict(means=[[per_tick, a.peak * per_tick]], weights=None, seg_ticks=a.seg_decisions * a.ticks, tick_offset=0)
    return TrafficVecEnv(a.envs, a.m, a.n, a.length, capacity=a.capacity, spawn='demand', seed=a.seed, demand=demand)


class Actuated(object):
    """the controller's state per intersection: the phase it shows and for how many decisions it has shown it"""

    def __init__(self, venv, a, first_phase):
        eng, g = venv.engine, venv.graph
        dev, r = eng.device, eng.r
        self.venv, self.a, self.I = venv, a, eng.I
        self.phase = torch.as_tensor(first_phase).to(device=dev, dtype=torch.int64)            # [E, I]
        self.held = torch.zeros_like(self.phase)
        # approach road e of intersection dest[e] is green in phase phases[e]: slot dest * 2 + phase
        slot = torch.as_tensor(g.dest[:r].astype(np.int64) * 2 + g.phases[:r]).to(dev)
        self.slot = slot.expand(eng.E, -1).contiguous()                                     # [E, r]
        self.need = float(ARCHETYPE["car_l"] + ARCHETYPE["car_s0"])

    def act(self, s):
        a, E, I = self.a, self.phase.shape[0], self.I
        inf = torch.full((E, 2 * I), float("inf"), device=s.eta_s.device)
        # the soonest arrival and the tightest downstream entrance per (intersection, phase)
        eta = inf.clone().scatter_reduce_(1, self.slot, s.eta_s.clamp(min=0.0).min(dim=2).values, "amin")
        room = inf.clone().scatter_reduce_(1, self.slot, s.downstream_room, "amin")
        eta, room = eta.view(E, I, 2), room.view(E, I, 2)
        mine = eta.gather(2, self.phase[..., None])[..., 0]
        other_room = room.gather(2, (1 - self.phase)[..., None])[..., 0]
        arriving = mine < a.gap
        want = (self.held >= a.max_green) | ((self.held >= a.min_green) & ~arriving)
        switch = want & (other_room >= self.need)
        self.phase = torch.where(switch, 1 - self.phase, self.phase)
        self.held = torch.where(switch, torch.zeros_like(self.held), self.held + 1)
        return self.phase.to(torch.int32)


def run(a):
    T = a.ticks
    ph = np.random.RandomState(a.seed).randint(2, size=(a.envs, a.m * a.n)).astype(np.int32)
    out, ms = {}, None
    for name in ("actuated (gap-out)", "fixed cycle", "greedy (on device)"):
        venv = make(a)                                              # same seed, same env ids: the same cars arrive
        venv.reset(ph)
        eng = venv.engine
        if name.startswith("greedy"):
            eng.set_greedy(T)                                       # one greedy decision per agent step, held for it
        ctl = Actuated(venv, a, ph) if name.startswith("actuated") else None
        ret = torch.zeros(a.envs, device=eng.device)
        over = torch.zeros(a.envs, dtype=torch.bool, device=eng.device)
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.decisions)]
        for d in range(a.decisions):
            act = None
            if ctl is not None:
                ev[d][0].record()
                s = venv.stop_lines(k=a.k, v_min=a.v_min)
                ev[d][1].record()
                act = ctl.act(s)
            _, rew, done = venv.agent_step(act, n_ticks=T, cycle_period=a.cycle if name == "fixed cycle" else None)
            ret += torch.where(over, torch.zeros_like(ret), rew.sum(dim=1))     # an episode ends at its first overflow
            over |= done.bool()
        torch.cuda.synchronize()
        if ctl is not None:
            ms = float(np.median([e0.elapsed_time(e1) for e0, e1 in ev[min(3, a.decisions - 1):]]))
        out[name] = (float(ret.mean()), int(over.sum()))
    return out, ms


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--decisions", type=int, default=120)
    ap.add_argument("--ticks", type=int, default=10)
    ap.add_argument("--cycle", type=int, default=20, help="ticks between the fixed cycle's phase changes")
    ap.add_argument("--m", type=int, default=3)
    ap.add_argument("--n", type=int, default=3)
    ap.add_argument("--length", type=float, default=120.0)
    ap.add_argument("--capacity", type=int, default=14)
    ap.add_argument("--cars-per-sec", type=float, default=0.08, help="per entry road, at the base level")
    ap.add_argument("--peak", type=float, default=1.5, help="demand of the second segment relative to the first")
    ap.add_argument("--seg-decisions", type=int, default=30, help="decisions per demand segment")
    ap.add_argument("--k", type=int, default=4, help="cars listed per approach")
    ap.add_argument("--v-min", type=float, default=0.5, help="m/s: a slower car's arrival time is taken at this speed")
    ap.add_argument("--gap", type=float, default=2.0, help="seconds: green is held while a car is nearer than this")
    ap.add_argument("--min-green", type=int, default=1, help="decisions")
    ap.add_argument("--max-green", type=int, default=3, help="decisions")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    r, ms = run(a)
    lines = ["actuated demo: %d envs (%dx%d grid, L=%g, C=%d), %d decisions of %d ticks, the same demand streams for every "
             "controller; k %d, gap %g s, green %d .. %d decisions" % (a.envs, a.m, a.n, a.length, a.capacity, a.decisions,
                                                                     a.ticks, a.k, a.gap, a.min_green, a.max_green),
             "%-20s %24s %24s" % ("controller", "mean return per env", "envs ended by overflow")]
    for name in ("actuated (gap-out)", "fixed cycle", "greedy (on device)"):
        lines.append("%-20s %24.3f %24d" % ((name,) + r[name]))
    lines.append("median %.3f ms per stop_lines call (one launch + the derived views)" % ms)
    for ln in lines:
        print(ln)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n\n")
    return r


if __name__ == "__main__":
    main()
