"""us per batched decision of the rollout loop's env part, with and without episodes on the device.  Runs on a tree
with tfx_set_episodes and on one without (there only the modes that exist), so that a change and its parent commit can
be timed alternately in one sitting:

    python tools/time_autoreset.py MODE [small|big]       MODE: host_reset | autoreset | step_only

  host_reset  agent_step + reset_done(adone): the restart through the host (phases drawn with NumPy, copied over)
  autoreset   TrafficVecEnv(autoreset=True), no time limit: the same envs restart, on the device
  step_only   agent_step alone (episodes off)
  small: 1024 envs of the 4x4 grid, C = 34 (k_res); big: 4096 envs of the 16x16 grid, C = 66 (pairs, two halves).
spawn='device', no policy (the actions stay as they are).  20 warm-up decisions, then 5 regions of at least one second
each, a device synchronise at the end of every region; prints one line: median, min, max, spread of the regions."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "traffic-env_amd")]
import torch
from gym_traffic.envs.vec_env import TrafficVecEnv

mode = sys.argv[1]
size = sys.argv[2] if len(sys.argv) > 2 else "small"
E, m, n, L, cap = (1024, 4, 4, 200.0, 34) if size == "small" else (4096, 16, 16, 400.0, 66)
kw = dict(autoreset=True) if mode == "autoreset" else {}
venv = TrafficVecEnv(E, m, n, L, capacity=cap, spawn='device', local_cars_per_sec=0.12, seed=0, **kw)
venv.reset()
actions = torch.zeros((E, venv.engine.I), dtype=torch.int32, device=venv.engine.device)
ended = torch.zeros((), dtype=torch.int64, device=venv.engine.device)


def decide():
    aobs, arew, adone = venv.agent_step(actions, n_ticks=10)
    ended.add_(adone.sum())
    if mode == "host_reset":
        venv.reset_done(adone)


for _ in range(20):
    decide()
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(20):
    decide()
torch.cuda.synchronize()
k = max(20, int(1.25 / ((time.perf_counter() - t0) / 20)))   # decisions per region: a good second
regions = []
while len(regions) < 5:
    t0 = time.perf_counter()
    for _ in range(k):
        decide()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if dt < 1.0:            # (the probe was slow: longer regions, this one does not count)
        k *= 2
        continue
    regions.append(dt / k * 1e6)
regions.sort()
print("%-10s %-5s %d envs %dx%d C=%d %s: median %.1f us per batched decision (min %.1f max %.1f spread %.1f; %d episodes ended)"
      % (mode, size, E, m, n, cap, venv.engine.step_kernel(), regions[2], regions[0], regions[-1], regions[-1] - regions[0],
         int(ended)), flush=True)
