"""A complete RL rollout loop on the device: E batched traffic envs (on-device Poisson arrivals), a small torch
policy reading the fused decision's observation and writing the light actions, one `agent_step` (10 ticks + remi
reward) per decision.  Prints decisions/s and env-ticks/s.

    python tools/rollout_demo.py [envs] [m] [n] [capacity] [decisions] [--autoreset [EPISODE_LEN]] [--warm-pool N[,DECISIONS]]

Without --autoreset episodes restart on overflow through `reset_done`: no synchronisation, but the new phases are drawn
on the host and copied over on every decision.  With it the envs keep their episodes on the device (restart, time limit
of EPISODE_LEN decisions if given, return and length per episode): nothing but the loop's Python runs on the host, and
the mean return / length of the finished episodes are printed.  --warm-pool N[,DECISIONS] (with --autoreset): episodes
start from a pool of N envs warmed up for DECISIONS decisions (default 10) under sampled actions, as the reference's
WarmupWrapper starts them, instead of from an empty map - the first one too (reset(warm=True)).
"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "traffic-env_amd")]
import torch
from gym_traffic.envs.vec_env import TrafficVecEnv

AUTORESET, EPISODE_LEN = False, None
if "--autoreset" in sys.argv:
    at = sys.argv.index("--autoreset")
    AUTORESET = True
    if at + 1 < len(sys.argv) and sys.argv[at + 1].isdigit():
        EPISODE_LEN = int(sys.argv.pop(at + 1))
    sys.argv.pop(at)
WARM_POOL = None
if "--warm-pool" in sys.argv:
    at = sys.argv.index("--warm-pool")
    if not AUTORESET or at + 1 >= len(sys.argv):
        sys.exit("--warm-pool N[,DECISIONS] needs --autoreset: the restarts it warms are those on the device")
    WARM_POOL = [int(v) for v in sys.argv.pop(at + 1).split(",")]
    WARM_POOL = (WARM_POOL[0], WARM_POOL[1] if len(WARM_POOL) > 1 else 10)
    sys.argv.pop(at)
E = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
m = int(sys.argv[2]) if len(sys.argv) > 2 else 4
n = int(sys.argv[3]) if len(sys.argv) > 3 else 4
cap = int(sys.argv[4]) if len(sys.argv) > 4 else 34
N = int(sys.argv[5]) if len(sys.argv) > 5 else 300
venv = TrafficVecEnv(E, m, n, 200.0, capacity=cap, spawn='device', local_cars_per_sec=0.12, seed=0,
                     autoreset=AUTORESET, episode_len=EPISODE_LEN)
eng = venv.engine
if WARM_POOL:
    venv.set_warm_pool(venv.make_warm_pool(*WARM_POOL))
venv.reset(warm=bool(WARM_POOL))
dev = eng.device
torch.manual_seed(0)
policy = torch.nn.Sequential(torch.nn.Linear(2 * eng.r + eng.I, 128), torch.nn.Tanh(), torch.nn.Linear(128, eng.I)).to(dev)
actions = torch.zeros((E, eng.I), dtype=torch.int32, device=dev)
ret = torch.zeros((E,), device=dev)
episodes = torch.zeros((), dtype=torch.int64, device=dev)
fin_ret = torch.zeros((), device=dev)          # --autoreset: sums over the finished episodes
fin_len = torch.zeros((), dtype=torch.int64, device=dev)
fin_n = torch.zeros((), dtype=torch.int64, device=dev)


def decide(k):
    global ret
    aobs, arew, adone = venv.agent_step(actions, n_ticks=10)
    with torch.no_grad():
        actions.copy_((policy(aobs) > 0).to(torch.int32))
    episodes.add_(adone.sum())
    if AUTORESET:                           # the next decision restarts the envs that ended, on the device
        ended = (adone | venv.truncated).bool()
        fin_ret.add_((venv.final_return.mean(dim=1) * ended).sum())
        fin_len.add_((venv.final_length * ended).sum())
        fin_n.add_(ended.sum())
        return
    ret += arew.mean(dim=1)
    venv.reset_done(adone)                  # masked restart; no synchronisation, phases drawn on the host


for k in range(20):
    decide(k)
torch.cuda.synchronize()
t0 = time.perf_counter()
for k in range(N):
    decide(k)
torch.cuda.synchronize()
dt = time.perf_counter() - t0
print("%d envs %dx%d C=%d, step kernel %s: %d decisions in %.3f s = %.0f env-decisions/s, %.3e env-ticks/s "
      "(%.0f us per batched decision incl. the policy); %d episodes ended by an overflow, mean return %.2f"
      % (E, m, n, cap, eng.step_kernel(), N, dt, E * N / dt, E * N * 10 / dt, dt / N * 1e6, int(episodes),
         float(venv.episode_return.mean()) if AUTORESET else float(ret.mean())))
if AUTORESET:
    k = max(1, int(fin_n))
    if WARM_POOL:
        print("warm pool: %d envs warmed up for %d decisions, %d cars on their roads"
              % (WARM_POOL + (int(venv.warm_pool.engine.cars_on_roads_flat().sum()),)))
    print("autoreset%s: %d episodes finished, mean final_return %.3f, mean final_length %.2f decisions"
          % ("" if EPISODE_LEN is None else " (episode_len %d)" % EPISODE_LEN, int(fin_n), float(fin_ret) / k, float(fin_len) / k))
