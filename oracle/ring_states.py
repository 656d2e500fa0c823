"""The family of pathological ring states the parity tests run on.  TEST INFRASTRUCTURE.

One home for it: tests/test_gpu_parity.py re-exports `random_state` (HIP against the oracle), oracle/gen_golden.py
--set states starts the REFERENCE from the same family (tests/golden/states/, oracle and HIP against the reference).
NumPy only: the generator imports it as `ring_states`, the tests as `oracle.ring_states`.
"""
import numpy as np

# what the callers draw `beyond` and `crowd` from
BEYOND = (0.0, 0.05, 0.4, 1.6)
CROWD = (0.3, 0.8)


def random_state(rng, E, R, C, length, crowd=0.5, beyond=0.15, sorted_x=True):
    """Random ring states incl. wrapped rings, empty and full roads, cars past the road end."""
    x = np.zeros((E, R, C), np.float32)
    v = np.zeros((E, R, C), np.float32)
    w = np.zeros((E, R, C), np.float32)
    leading = rng.randint(1, C, size=(E, R)).astype(np.int32)
    n = np.minimum(rng.binomial(C - 2, crowd, size=(E, R)), C - 2)
    n[rng.rand(E, R) < 0.1] = 0
    n[rng.rand(E, R) < 0.1] = C - 2
    lastcar = leading.copy()
    for k in range(E):
        for e in range(R):
            cnt = int(n[k, e])
            pos = np.sort(rng.uniform(-20, length * (1 + beyond), size=cnt))[::-1] if sorted_x \
                else rng.uniform(-20, length * (1 + beyond), size=cnt)
            s = int(leading[k, e])
            for j in range(cnt):
                s = s + 1 if s + 1 < C else 1
                x[k, e, s] = pos[j]
                v[k, e, s] = rng.choice([0.0, rng.uniform(0, 15)])
                w[k, e, s] = rng.randint(0, 50)
            lastcar[k, e] = s
            # exit roads keep the +inf leader they got at reset (traffic_env.py:263; update_lights
            # never touches them); train roads get theirs rewritten every tick
            x[k, e, leading[k, e]] = np.inf
    return x, v, w, leading, lastcar


def live_slots(leading, lastcar, C):
    """bool [R, C]: the slots wrap(leading + 1) .. lastcar of every road"""
    slots = np.arange(C)[None, :]
    ld, lc = np.asarray(leading)[:, None], np.asarray(lastcar)[:, None]
    return np.where(ld <= lc, (slots > ld) & (slots <= lc), (slots > ld) | ((slots >= 1) & (slots <= lc))) & (ld != lc)


def state_rows(x, v, w, leading, lastcar, table, row=None):
    """One env's planes [R, C] as the reference's `state` [R, 10, C]: a live slot holds the whole row of `table`
    (float32 [n, 10]) that `row` [R, C] names (None: row 0) with its x, v and w; the fake-leader slot is zero but for
    its x - what _reset sets up and every pop preserves (traffic_env.py:262-263,133); every other slot is zero."""
    R, C = x.shape
    live = live_slots(leading, lastcar, C)
    pick = np.zeros((R, C), np.int64) if row is None else np.asarray(row, np.int64)
    st = np.transpose(np.asarray(table, np.float32)[pick], (0, 2, 1)) * live[:, None, :].astype(np.float32)   # [R, 10, C]
    st[:, 0, :] = np.where(live, x, 0)
    st[:, 1, :] = np.where(live, v, 0)
    st[:, 9, :] = np.where(live, w, 0)
    roads = np.arange(R)
    st[roads, 0, leading] = np.asarray(x)[roads, leading]
    return np.ascontiguousarray(st, np.float32)
