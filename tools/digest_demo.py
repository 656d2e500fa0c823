"""Transpositions in a lookahead search, found by state digests (tfx_state_digest): the branch batch of
tools/lookahead_demo.py - N live envs, N x K branches that each try a candidate action for H decisions - with one digest
launch per decision over the branches.  Candidates often coincide (holding the phases IS the greedy choice, two random
settings agree), and different actions can lead to the same state; such branches reach the same bits, and a search that
keys its table by the digest expands them once.  Every decision the demo counts the branches whose 'state' digest equals
that of another branch, and verifies a sample of those pairs the long way: their car lists (cars() of just the two envs),
ring positions and observation rows, byte for byte.

    python tools/digest_demo.py --envs 64 --candidates 8 --horizon 3 --decisions 20
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "traffic-env_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from gym_traffic import _native as nat  # noqa: E402
from lookahead_demo import candidates, make  # noqa: E402


def duplicate_pairs(digest, limit):
    """(branches whose digest another branch has too - all but one of each group, up to `limit` pairs (a, b) of equal digests)"""
    d, order = torch.sort(digest)
    same = d[1:] == d[:-1]
    at = torch.nonzero(same).reshape(-1)[:limit]
    return int(same.sum()), [(int(order[i]), int(order[i + 1])) for i in at.tolist()]


def same_the_long_way(venv, a, b):
    """envs a and b of the batch hold the same caller-visible state: car lists, ring positions, obs, counters"""
    eng = venv.engine
    c = venv.cars([a, b])
    R = eng.R
    off = c.offsets.cpu().numpy().astype(np.int64)
    half = int(off[R])
    if int(c.n) != 2 * half or not np.array_equal(off[:R + 1], off[R:] - half):
        return False
    xv = c.xv.cpu().numpy()
    if xv[:half].tobytes() != xv[half:].tobytes():
        return False
    return all(bool(torch.equal(t[a], t[b])) for t in (eng.leading, eng.obs, eng.waiting, eng.passed_dst, eng.done_tick)) and \
        eng.rewards[a].cpu().numpy().tobytes() == eng.rewards[b].cpu().numpy().tobytes()


def run(a):
    N, K, H, T = a.envs, a.candidates, a.horizon, a.ticks
    live, branches = make(N, a), make(N * K, a, offset=N)
    I = live.engine.I
    dev = live.engine.device
    live.reset(np.random.RandomState(a.seed).randint(2, size=(N, I)).astype(np.int32))
    branches.reset(np.zeros((N * K, I), np.int32))
    gen = torch.Generator(device=dev)
    gen.manual_seed(a.seed)
    src = (torch.arange(N * K, device=dev) // K).to(torch.int32)
    dups, checked, wrong, cloned_ok = [], 0, 0, 0
    start_parts = branches.digest_parts('state') & ~nat.DIGEST_OBS
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(2)] for _ in range(a.decisions)]
    for d in range(a.decisions):
        cand = candidates(live, K, gen)                                # [N, K, I]
        branches.clone_envs(src, source=live, streams=True, episodes=False)
        # every branch starts as its live env: cars, ring positions, lights.  (Not the counters' part: the branches run
        # at a clock of their own, and the stamp of an env that has overflowed is rebased by the difference.)
        cloned_ok += int(branches.same_state(src, source=live, parts=start_parts).all())
        score = torch.zeros(N * K, device=dev)
        flat = cand.reshape(N * K, I)
        for _ in range(H):
            _, rew, _ = branches.agent_step(flat, n_ticks=T)
            score += rew.sum(dim=1)
        ev[d][0].record()
        digest = branches.digest(parts='state')
        ev[d][1].record()
        n_dup, pairs = duplicate_pairs(digest, a.sample)
        dups.append(n_dup)
        for x, y in pairs:
            checked += 1
            wrong += int(not same_the_long_way(branches, x, y))
        best = score.reshape(N, K).argmax(dim=1)
        live.agent_step(cand[torch.arange(N, device=dev), best], n_ticks=T)
    torch.cuda.synchronize()
    skip = min(3, a.decisions - 1)
    ms = [e[0].elapsed_time(e[1]) for e in ev[skip:]]
    return dict(envs=N, candidates=K, horizon=H, decisions=a.decisions, ticks=T, branches=N * K, duplicates=dups,
                pairs_checked=checked, pairs_wrong=wrong, clones_verified=cloned_ok, digest_ms=float(np.median(ms)))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=64)
    ap.add_argument("--candidates", type=int, default=8)
    ap.add_argument("--horizon", type=int, default=3)
    ap.add_argument("--decisions", type=int, default=20)
    ap.add_argument("--ticks", type=int, default=10)
    ap.add_argument("--sample", type=int, default=4, help="duplicate pairs verified by their car lists per decision")
    ap.add_argument("--m", type=int, default=4)
    ap.add_argument("--n", type=int, default=4)
    ap.add_argument("--length", type=float, default=200.0)
    ap.add_argument("--capacity", type=int, default=34)
    ap.add_argument("--cars-per-sec", type=float, default=0.12)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args(argv)
    r = run(a)
    print("digest demo: %d live envs (%dx%d grid, C=%d), %d candidates x %d decisions ahead: %d branches, %d decisions of %d ticks"
          % (r["envs"], a.m, a.n, a.capacity, r["candidates"], r["horizon"], r["branches"], r["decisions"], r["ticks"]))
    print("clones verified by same_state: %d of %d decisions" % (r["clones_verified"], r["decisions"]))
    print("duplicate branches per decision (by digest): %s" % r["duplicates"])
    print("mean share of the branch batch a transposition table would skip: %.1f %%"
          % (100.0 * float(np.mean(r["duplicates"])) / r["branches"]))
    print("duplicate pairs verified by their car lists: %d, of which differ: %d" % (r["pairs_checked"], r["pairs_wrong"]))
    print("median ms per digest of the %d branches: %.3f" % (r["branches"], r["digest_ms"]))
    return r


if __name__ == "__main__":
    main()
