"""Self-check of a whole batch by state digests (tfx_state_digest): the benchmark's workload at a given size, every env
checked on the device, a handful of envs checked against the CPU oracle.

In the workload recipe (gym_traffic/workload.py) an env's inputs depend on its id only through id % LIGHT_PERIOD, so env
k must hold the bits of env k % period at every tick.  After --ticks ticks one digest launch gives a 64-bit word per env
and per road - every part the handle has - and a few torch expressions compare every env with its representative: the
whole batch is checked without exporting a car.  The `period` representatives themselves are then compared with the CPU
oracle's run of the same recipe: their cars through car_list of just those envs, byte for byte, and their digests with
the NumPy definition (devrng.state_digest) applied to the oracle's state.

    python tools/batch_selfcheck.py --config cfg2 --envs 4096 --ticks 60
"""
import argparse
import json
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

# ticks per tfx_step call, in turn: odd and even lengths, so one-tick movers and two-tick passes both run
CHUNKS = (10, 5, 8, 1, 6)


def first_difference(env, road, period):
    """(envs that differ from their representative, the first such (env, road) or None) - one read-back at the end"""
    E = env.shape[0]
    rep = torch.arange(E, device=env.device) % period
    bad_env = env != env[rep]
    bad_road = road != road[rep]
    n_bad = int((bad_env | bad_road.any(dim=1)).sum())
    if n_bad == 0:
        return 0, None
    k = int(torch.nonzero(bad_env | bad_road.any(dim=1))[0])
    roads = torch.nonzero(bad_road[k])
    return n_bad, (k, int(roads[0]) if len(roads) else -1)


def selfcheck(config="cfg2", envs=None, ticks=60, period=wl.LIGHT_PERIOD, layout=None, validate=False, oracle=True,
              threads=8):
    """-> dict(selfcheck 'ok' | 'FAILED', ...).  period: envs k and k % period must agree (the recipe's light period)."""
    from oracle.oracle import OracleEnv
    c = wl.CONFIGS[config]
    eng = wl.setup_engine(config, envs=envs, layout=layout, validate=validate)
    E = eng.E
    period = min(int(period), E)
    reps = list(range(period))
    orc = None
    if oracle:
        orc = OracleEnv(c["m"], c["n"], c["length"], c["capacity"], eng.dest, eng.phases, eng.nexts, n_envs=period,
                        validate=validate)
        orc.reset(np.zeros(orc.I, np.int32))
        x, v, leading, lastcar = wl.prefill_one_env(c["m"], c["n"], c["length"], c["capacity"], c["prefill"], c["gap"])
        for k in reps:
            orc.load_planes(k, x, v, np.zeros_like(x), leading, lastcar)
    t, call = 0, 0
    while t < ticks:
        n = min(CHUNKS[call % len(CHUNKS)], ticks - t)
        eng.step(n)
        for tt in range(t, t + n) if orc is not None else ():
            orc.step(wl.cycle_actions(np.arange(period), orc.I, tt), [wl.spawn_roads_for_tick(eng.entrypoints, tt)] * period,
                     nthreads=threads)
        t, call = t + n, call + 1
    parts = eng.digest_parts()
    env, road = eng.state_digest(parts=parts, per_road=True)
    n_bad, where = first_difference(env, road, period)
    out = dict(config=config, envs=E, ticks=int(ticks), period=period, layout=eng.layout, parts=parts,
               cars=int(eng.cars_on_roads_flat().sum()), envs_differing=n_bad, first_difference=where,
               distinct_digests=int(torch.unique(env).numel()))
    ok = n_bad == 0
    if orc is not None:
        # the representatives against the oracle: their cars, byte for byte, and their digests by the NumPy definition
        cl = eng.car_list(env_ids=reps)
        w = orc.w if validate else None
        want = devrng.car_list(orc.x, orc.v, w, None, orc.leading, orc.lastcar, eng.C)
        same_cars = int(cl.n) == want[0] and cl.offsets.cpu().numpy().tobytes() == want[1].tobytes() and \
            cl.xv.cpu().numpy().tobytes() == want[2].tobytes()
        vis = nat.DIGEST_CARS | nat.DIGEST_RING | nat.DIGEST_LIGHTS | (nat.DIGEST_SPAWN if validate else 0)
        got = eng.state_digest(reps, parts=vis, per_road=True)
        model = devrng.state_digest(orc.x, orc.v, w, None, orc.leading, orc.lastcar, eng.C, vis, obs=orc.obs, I=orc.I, r=orc.r)
        same_digest = all(g.cpu().numpy().tobytes() == m.view(np.int64).tobytes() for g, m in zip(got, model))
        out.update(oracle_cars=want[0], oracle_cars_equal=bool(same_cars), oracle_digests_equal=bool(same_digest))
        ok = ok and same_cars and same_digest
    out["selfcheck"] = "ok" if ok else "FAILED"
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg2", choices=sorted(wl.CONFIGS))
    ap.add_argument("--envs", type=int, default=None, help="default: the config's benchmark size")
    ap.add_argument("--ticks", type=int, default=60)
    ap.add_argument("--period", type=int, default=wl.LIGHT_PERIOD)
    ap.add_argument("--layout", default=None, choices=["ring", "transposed"])
    ap.add_argument("--validate", action="store_true", help="validate mode: spawn ticks are kept and checked too")
    ap.add_argument("--no-oracle", action="store_true", help="skip the CPU oracle's run of the representatives")
    ap.add_argument("--threads", type=int, default=8)
    a = ap.parse_args(argv)
    r = selfcheck(a.config, a.envs, a.ticks, a.period, a.layout, a.validate, not a.no_oracle, a.threads)
    if r["first_difference"] is not None:
        print("first differing (env, road): %r" % (r["first_difference"],))
    print(json.dumps(r))
    return 0 if r["selfcheck"] == "ok" else 1


if __name__ == "__main__":
    sys.exit(main())
