"""Host mirror of the on-device arrival generator (csrc/tfx_misc.hpp k_poisson).

The device draws car arrivals with Philox4x32-10 streams keyed by (seed, global env id) and turns
uniforms into whole-tick gaps through a table of 32-bit thresholds built here from the exact
distribution of `round(Exp(mean))` - the reference's gap rule (traffic_env.py:161-163; Python's
round is half-to-even: gap k >= 1 covers [k - 1/2, k + 1/2], with the ties at even k).  Because both
sides compare the same integers, `PoissonMirror` reproduces the device's (tick, road) sequence bit
for bit; tests feed it to the oracle.

With an archetype table of n > 1 rows the device also draws every car's row (rule 1 of include/tfx.h): car j (0-based)
of a tick on entry index ej of global env g takes row (u0 * n) >> 32 of philox4x32({s + j, g, TAG_ARCH, ej}, seed),
s = the cars the stream has put on that entry road of the env before the tick.  The mirrors keep s per (env, entry)
and return the rows of each tick next to its counts.

`episode_phases` mirrors the other draw the device makes: the light phases of an env that restarts on the device
(tfx_set_episodes, rule 2 of include/tfx.h).  `clone_plan` and `road_measures` state two more device rules in NumPy: which
envs an in-place tfx_clone_envs applies, and what tfx_road_measures computes per road.  `road_cells` does the same for
tfx_road_cells (cars and speeds per cell of road); `cell_edges` makes the uniform edges that leave no car out.  `frames`
states what tfx_frames draws (top-view RGBA pictures of chosen envs), `frame_geometry` where every road lies in them.
`car_ages` and `trip_stats` state the travel-time rules (tfx_car_ages, tfx_trip_stats): the ages of the live cars per
road, and the finished trips of every env's log reduced from a cursor on.  `road_following` states the car-following
measures (tfx_road_following): gaps, headways, time to collision and platoon joins of every car and its leader.

`demand_tables`, `demand_segment` and `demand_counts` belong to the demand profiles (tfx_set_demand, rule 4 of
include/tfx.h): the threshold tables the device reads, the segment of a clock tick, and the rule itself in NumPy - a pure
function of (seed, stream id, clock tick), with no state to carry: a true per-tick Poisson process, not the reference's
rounded-gap generator that PoissonMirror mirrors.  `demand_row_table` and `demand_rows` add rule 5 (tfx_set_demand_mixed): the
third threshold table, and the archetype row of every one of those cars in creation order per road.
"""
import collections
import math

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
TAG_GAP, TAG_ROAD, TAG_ARCH = 0x47415021, 0x524F4144, 0x41524348
TAG_EPISODE = 0x45504953
TAG_POOL = 0x504F4F4C
TAG_DCNT, TAG_DROAD = 0x44434E54, 0x44524F44
TAG_DROW = 0x44524F57
MASK = 0xFFFFFFFF


def philox4x32(c0, c1, c2, c3, k0, k1):
    for _ in range(10):
        p0 = M0 * c0
        p1 = M1 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & MASK, p1 & MASK, ((p0 >> 32) ^ c3 ^ k1) & MASK, p0 & MASK
        k0 = (k0 + W0) & MASK
        k1 = (k1 + W1) & MASK
    return c0, c1, c2, c3


def philox4x32_first(c0, c1, c2, c3, k0, k1):
    """First output word of philox4x32 for an array of counters c0 (uint32 values in uint64 arrays); c1..c3 are
    scalars or arrays of c0's shape."""
    c0 = np.asarray(c0, np.uint64) & np.uint64(MASK)
    c1 = np.zeros_like(c0) + np.asarray(c1, np.uint64)
    c2 = np.zeros_like(c0) + np.asarray(c2, np.uint64)
    c3 = np.zeros_like(c0) + np.asarray(c3, np.uint64)
    m = np.uint64(MASK)
    s32 = np.uint64(32)
    for _ in range(10):
        p0 = np.uint64(M0) * c0
        p1 = np.uint64(M1) * c2
        c0, c1, c2, c3 = ((p1 >> s32) ^ c1 ^ np.uint64(k0)) & m, p1 & m, ((p0 >> s32) ^ c3 ^ np.uint64(k1)) & m, p0 & m
        k0 = (k0 + W0) & MASK
        k1 = (k1 + W1) & MASK
    return c0


def philox4x32_words(c0, c1, c2, c3, k0, k1):
    """All four output words of philox4x32 for arrays of counters (uint32 values in uint64 arrays, broadcast against
    each other)."""
    c0, c1, c2, c3 = np.broadcast_arrays(*[np.asarray(c, np.uint64) & np.uint64(MASK) for c in (c0, c1, c2, c3)])
    m = np.uint64(MASK)
    s32 = np.uint64(32)
    for _ in range(10):
        p0 = np.uint64(M0) * c0
        p1 = np.uint64(M1) * c2
        c0, c1, c2, c3 = ((p1 >> s32) ^ c1 ^ np.uint64(k0)) & m, p1 & m, ((p0 >> s32) ^ c3 ^ np.uint64(k1)) & m, p0 & m
        k0 = (k0 + W0) & MASK
        k1 = (k1 + W1) & MASK
    return c0, c1, c2, c3


def episode_phases(seed, env_ids, ep_index, I):
    """int32 [len(env_ids), I]: the phases a restart on the device gives the intersections of global envs `env_ids`
    at the start of their episode number `ep_index` (a scalar or one per env) - rule 2 of include/tfx.h: bit 0 of the
    first word of philox4x32({episode number, global env id, TAG_EPISODE, intersection}, key = seed).  A pure function
    of (seed, global env id, episode number, intersection)."""
    env_ids = np.asarray(env_ids, np.uint64).reshape(-1)
    n = np.zeros_like(env_ids) + (np.asarray(ep_index, np.int64).astype(np.uint64) & np.uint64(MASK))
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    shape = (len(env_ids), int(I))
    u0 = philox4x32_first(np.broadcast_to(n[:, None], shape), np.broadcast_to(env_ids[:, None], shape), TAG_EPISODE,
                          np.broadcast_to(np.arange(int(I), dtype=np.uint64)[None, :], shape), seed & MASK, seed >> 32)
    return (u0 & np.uint64(1)).astype(np.int32)


def episode_pool_slots(seed, env_ids, ep_index, n_pool):
    """int32 [len(env_ids)]: the env of a pool of `n_pool` warmed-up envs that global envs `env_ids` restart from at the
    start of their episode number `ep_index` (a scalar or one per env) - rule 3 of include/tfx.h (tfx_set_episode_pool):
    (u0 * n_pool) >> 32 with u0 the first word of philox4x32({episode number, global env id, TAG_POOL, 0}, key = seed).
    A pure function of (seed, global env id, episode number, n_pool)."""
    env_ids = np.asarray(env_ids, np.uint64).reshape(-1)
    n = np.zeros_like(env_ids) + (np.asarray(ep_index, np.int64).astype(np.uint64) & np.uint64(MASK))
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    u0 = philox4x32_first(n, env_ids, TAG_POOL, 0, seed & MASK, seed >> 32)
    return ((u0 * np.uint64(int(n_pool))) >> np.uint64(32)).astype(np.int32)


def clone_plan(src_of_env, n_src=None):
    """The in-place rule of tfx_clone_envs (include/tfx.h) in NumPy: -> (applied bool [E], skipped int).  Env e takes
    the state of env s = src_of_env[e] only if s is inside [0, E) and s is not itself overwritten by the call
    (src_of_env[s] is -1 or s); -1 asks for nothing; every other env is left untouched and counted.  A self-reference
    is applied (and changes nothing).  n_src: the env count of ANOTHER source handle - then only the range is checked,
    a source cannot be overwritten."""
    src = np.asarray(src_of_env, np.int64).reshape(-1)
    E = len(src)
    n = E if n_src is None else int(n_src)
    inside = (src >= 0) & (src < n)
    applied = inside.copy()
    if n_src is None:
        of_src = src[np.where(inside, src, 0)]
        applied &= (of_src == -1) | (of_src == src)
    skipped = int(np.count_nonzero((src != -1) & ~applied))
    return applied, skipped


def road_measures(x, v, leading, lastcar, C, halt_speed=0.1, x_from=None):
    """The definition of tfx_road_measures (include/tfx.h) in NumPy, over ring planes: x, v float32 [..., R, C] by ring
    slot (what tfx_export_ring produces), leading / lastcar int [..., R].  -> (n_cars, n_halted, queue int32 [..., R],
    speed_sum float32 [..., R]).  Car j of a road (j = 0: the head) sits in slot wrap(leading + 1 + j); it is in range
    iff x >= x_from (None: -inf), halted iff in range and v < halt_speed (float32, strict); queue counts the cars from
    the head on while every one is in range and halted; speed_sum adds v of the cars in range one at a time in
    ascending j, in float32, starting from 0 - the order the device keeps, so the bits agree."""
    C = int(C)
    x = np.asarray(x, np.float32)
    v = np.asarray(v, np.float32)
    shape = x.shape[:-1]
    x, v = x.reshape(-1, C), v.reshape(-1, C)
    ld = np.asarray(leading, np.int64).reshape(-1)
    lc = np.asarray(lastcar, np.int64).reshape(-1)
    n = lc - ld + np.where(ld > lc, C - 1, 0)
    halt = np.float32(halt_speed)
    lo = np.float32(-np.inf if x_from is None else x_from)
    rows = np.arange(len(ld))
    cars = np.zeros(len(ld), np.int32)
    halted = np.zeros(len(ld), np.int32)
    queue = np.zeros(len(ld), np.int32)
    unbroken = np.ones(len(ld), bool)
    total = np.zeros(len(ld), np.float32)
    for j in range(C - 1):
        live = j < n
        slot = ld + 1 + j
        slot = np.where(slot > C - 1, slot - (C - 1), slot)
        slot = np.where(live, slot, 0)
        xj, vj = x[rows, slot], v[rows, slot]
        with np.errstate(invalid="ignore"):
            inr = live & (xj >= lo)
            still = inr & (vj < halt)
            added = (total + vj).astype(np.float32)        # one float32 add per car
        cars += inr
        halted += still
        unbroken &= still | ~live
        queue += unbroken & live
        total = np.where(inr, added, total)
    return cars.reshape(shape), halted.reshape(shape), queue.reshape(shape), total.reshape(shape)


FOLLOW_FIELDS = ("n_cars", "n_pairs", "n_joined", "n_overlap", "gap_sum", "gap_min", "n_hw", "hw_sum", "n_conflict",
                 "ttc_min", "drac_max")


def road_following(x, v, leading, lastcar, C, params, car_l=4.0, arch_rows=None, arch_l=None):
    """The definition of tfx_road_following (include/tfx.h) in NumPy, over ring planes: x, v float32 [..., R, C] by ring
    slot (what tfx_export_ring produces), leading / lastcar int [..., R]; params = (x_from or None, platoon_gap, v_min,
    ttc_crit).  A car's length: car_l, or - with arch_rows uint8 [..., R, C] (the archetype row of every ring slot) and
    arch_l float32 [rows of the table] - arch_l[arch_rows].  -> a tuple in the order of FOLLOW_FIELDS, [..., R]: int32
    counters, float32 gap_sum, gap_min, hw_sum, ttc_min, drac_max.  Car j of a road (j = 0: the head) sits in slot
    wrap(leading + 1 + j); car j >= 1 is the follower F of a pair whose leader L is car j-1; the pair is in range iff
    x_F >= x_from.  g = (x_L - x_F) - l_L, dv = v_F - v_L; every operation one float32 rounding, sums in ascending j
    from 0, minima from +inf and the maximum from 0 by compare and select - the order and the NaN behaviour the device
    keeps, so the bits agree."""
    C = int(C)
    x_from, platoon_gap, v_min, ttc_crit = params
    lo = np.float32(-np.inf if x_from is None else x_from)
    join, slow, crit = np.float32(platoon_gap), np.float32(v_min), np.float32(ttc_crit)
    if np.isnan([lo, join, slow, crit]).any() or not slow > 0:
        raise ValueError("road_following: a NaN parameter, or v_min is not above 0")
    x = np.asarray(x, np.float32)
    v = np.asarray(v, np.float32)
    shape = x.shape[:-1]
    x, v = x.reshape(-1, C), v.reshape(-1, C)
    ld = np.asarray(leading, np.int64).reshape(-1)
    lc = np.asarray(lastcar, np.int64).reshape(-1)
    n = lc - ld + np.where(ld > lc, C - 1, 0)
    N = len(ld)
    rows = np.arange(N)
    if arch_rows is not None:
        lengths = np.asarray(arch_l, np.float32)[np.asarray(arch_rows).reshape(-1, C)]
    zero = np.float32(0)
    cars, pairs, joined, overlap, hw, conflict = [np.zeros(N, np.int32) for _ in range(6)]
    gap_sum, hw_sum, drac_max = [np.zeros(N, np.float32) for _ in range(3)]
    gap_min, ttc_min = [np.full(N, np.inf, np.float32) for _ in range(2)]
    xl, vl, ll = [np.zeros(N, np.float32) for _ in range(3)]      # the leader: the car taken just before
    have = np.zeros(N, bool)
    for j in range(C - 1):
        live = j < n
        slot = ld + 1 + j
        slot = np.where(slot > C - 1, slot - (C - 1), slot)
        slot = np.where(live, slot, 0)
        xj, vj = x[rows, slot], v[rows, slot]
        lj = np.full(N, car_l, np.float32) if arch_rows is None else lengths[rows, slot]
        with np.errstate(all="ignore"):
            inr = live & (xj >= lo)
            pair = inr & have
            g = ((xl - xj).astype(np.float32) - ll).astype(np.float32)
            dv = (vj - vl).astype(np.float32)
            timed = pair & (vj >= slow)
            closing = pair & (dv > zero) & (g > zero)
            ttc = (g / dv).astype(np.float32)
            drac = ((dv * dv).astype(np.float32) / (g + g).astype(np.float32)).astype(np.float32)
            cars += inr
            pairs += pair
            joined += pair & (g <= join)
            overlap += pair & (g < zero)
            gap_sum = np.where(pair, (gap_sum + g).astype(np.float32), gap_sum)
            gap_min = np.where(pair & (g < gap_min), g, gap_min)
            hw += timed
            hw_sum = np.where(timed, (hw_sum + (g / vj).astype(np.float32)).astype(np.float32), hw_sum)
            conflict += closing & (ttc < crit)
            ttc_min = np.where(closing & (ttc < ttc_min), ttc, ttc_min)
            drac_max = np.where(closing & (drac > drac_max), drac, drac_max)
        xl, vl, ll = np.where(live, xj, xl), np.where(live, vj, vl), np.where(live, lj, ll)
        have = have | live
    out = (cars, pairs, joined, overlap, gap_sum, gap_min, hw, hw_sum, conflict, ttc_min, drac_max)
    return tuple(a.reshape(shape) for a in out)


ENDS_FIELDS = ("n_cars", "n_heads", "heads", "head_rows", "tail", "tail_row")
ENDS_NO_CAR = 255     # TFX_ENDS_NO_CAR


def road_ends(x, v, leading, lastcar, C, length, k, pad_dist, pad_v, pad_tail_x, arch=None):
    """The definition of tfx_road_ends (include/tfx.h) in NumPy, over ring planes: x, v float32 [..., R, C] by ring slot
    (what tfx_export_ring produces), leading / lastcar int [..., R]; arch uint8 [..., R, C]: the archetype row of every
    ring slot on heterogeneous handles (None: every row is 0).  -> a tuple in the order of ENDS_FIELDS: n_cars, n_heads
    int32 [..., R]; heads float32 [..., R, k, 2]; head_rows uint8 [..., R, k]; tail float32 [..., R, 2]; tail_row uint8
    [..., R].  n is the ring count clamped to 0 .. C-1; car j of a road (j = 0: the head) sits in slot
    wrap(leading + 1 + j) - ring order, never sorted by x.  heads[j] = (float32(length) - x_j, v_j) for j < min(n, k) and
    (pad_dist, pad_v) beyond, rows ENDS_NO_CAR there; tail = (x, v) of car n - 1, or (pad_tail_x, pad_v) and row
    ENDS_NO_CAR on an empty road.  The pads are stored as given, bit for bit (NaN payloads included)."""
    C, k = int(C), int(k)
    if not 1 <= k <= 16:
        raise ValueError("road_ends: k %d is outside 1..16" % k)
    x = np.asarray(x, np.float32)
    v = np.asarray(v, np.float32)
    shape = x.shape[:-1]
    x, v = x.reshape(-1, C), v.reshape(-1, C)
    ld = np.asarray(leading, np.int64).reshape(-1)
    lc = np.asarray(lastcar, np.int64).reshape(-1)
    n = np.clip(lc - ld + np.where(ld > lc, C - 1, 0), 0, C - 1)
    N = len(ld)
    roads = np.arange(N)
    rows = np.zeros((N, C), np.uint8) if arch is None else np.asarray(arch, np.uint8).reshape(-1, C)
    L = np.float32(length)
    pads = np.array([pad_dist, pad_v, pad_tail_x], np.float32)      # (an array keeps a NaN's bits; a scalar may not)
    heads = np.empty((N, k, 2), np.float32)
    heads[..., 0], heads[..., 1] = pads[0], pads[1]
    head_rows = np.full((N, k), ENDS_NO_CAR, np.uint8)

    def slot_of(j):
        s = ld + 1 + j
        return np.where(s > C - 1, s - (C - 1), s)

    for j in range(k):
        live = j < n
        slot = np.where(live, slot_of(j), 0)
        with np.errstate(invalid="ignore"):
            dist = (L - x[roads, slot]).astype(np.float32)           # one float32 subtraction
        heads[live, j, 0] = dist[live]
        heads[live, j, 1] = v[roads, slot][live]
        head_rows[live, j] = rows[roads, slot][live]
    some = n > 0
    slot = np.where(some, slot_of(n - 1), 0)
    tail = np.empty((N, 2), np.float32)
    tail[:, 0], tail[:, 1] = pads[2], pads[1]
    tail[some, 0], tail[some, 1] = x[roads, slot][some], v[roads, slot][some]
    tail_row = np.where(some, rows[roads, slot], ENDS_NO_CAR).astype(np.uint8)
    return (n.astype(np.int32).reshape(shape), np.minimum(n, k).astype(np.int32).reshape(shape),
            heads.reshape(shape + (k, 2)), head_rows.reshape(shape + (k,)), tail.reshape(shape + (2,)),
            tail_row.reshape(shape))


CAR_LIST_FIELDS = ("n", "offsets", "xv", "road", "row", "spawn")


def car_list(x, v, w, arch, leading, lastcar, C, env_ids=None, road_mask=None, cap=None, out=None):
    """The definition of tfx_car_list (include/tfx.h) in NumPy, over ring planes: x, v float32 [E, R, C] by ring slot (what
    tfx_export_ring produces), w float32 [E, R, C] the spawn ticks (None on handles with planes == 2: no spawn plane),
    arch uint8 [E, R, C] the archetype row of every ring slot on heterogeneous handles (None: every row is 0), leading /
    lastcar int [E, R].  env_ids: n_sel env numbers (None: every env in order; repeats allowed; an id outside [0, E)
    contributes no cars); road_mask uint8 [R] or None (a road with mask 0 contributes no cars); cap: entries the planes
    hold (None: exactly N).  -> a tuple in the order of CAR_LIST_FIELDS: n (the total N, an int), offsets int32
    [n_sel * R + 1], xv float32 [cap, 2], road int32 [cap], row uint8 [cap], spawn float32 [cap] or None.
    count[s][road] is the ring count clamped to 0 .. C-1, 0 for masked-out roads and envs that are not shown; offsets is
    its exclusive prefix sum in (s, road id) order.  Car j from the head, in ring order (slot wrap(leading + 1 + j), never
    sorted by x), of (s, road) has index i = offsets[s * R + road] + j; for i < min(N, cap): xv[i] = (x, v), road[i] =
    s * R + road, row[i] its archetype row, spawn[i] its spawn tick - all moved bit for bit.  Entries at i >= min(N, cap)
    are never written: they keep what `out` (xv, road, row, spawn - any None) held, zeros where it gave nothing."""
    C = int(C)
    x = np.asarray(x, np.float32)
    v = np.asarray(v, np.float32)
    E, R = x.shape[0], x.shape[1]
    ld = np.asarray(leading, np.int64).reshape(E, R)
    lc = np.asarray(lastcar, np.int64).reshape(E, R)
    n = np.clip(lc - ld + np.where(ld > lc, C - 1, 0), 0, C - 1)
    ids = np.arange(E, dtype=np.int64) if env_ids is None else np.asarray(env_ids, np.int64).reshape(-1)
    shown = (ids >= 0) & (ids < E)
    env = np.where(shown, ids, 0)
    count = n[env] * shown[:, None]
    if road_mask is not None:
        count = count * (np.asarray(road_mask).reshape(R) != 0)[None, :]
    n_sel = len(ids)
    offsets = np.zeros(n_sel * R + 1, np.int64)
    np.cumsum(count.reshape(-1), out=offsets[1:])
    N = int(offsets[-1])
    cap = N if cap is None else int(cap)
    if cap < 0:
        raise ValueError("car_list: cap %d is negative" % cap)
    planes = dict(xv=(np.float32, (cap, 2)), road=(np.int32, (cap,)), row=(np.uint8, (cap,)), spawn=(np.float32, (cap,)))
    given = dict(zip(("xv", "road", "row", "spawn"), out if out is not None else (None,) * 4))
    res = {}
    for name, (dtype, shape) in planes.items():
        a = given[name]
        res[name] = np.zeros(shape, dtype) if a is None else np.array(a, dtype).reshape(shape)
    if w is None:
        res["spawn"] = None
    top = min(N, cap)
    # every listed car: its key, its rank from the head, its ring slot
    key = np.repeat(np.arange(n_sel * R), count.reshape(-1))[:top]
    rank = np.arange(top) - offsets[key]
    sel, rd = key // R, key % R
    e = env[sel]
    slot = ld[e, rd] + 1 + rank
    slot = np.where(slot > C - 1, slot - (C - 1), slot)
    res["xv"][:top, 0] = x[e, rd, slot]
    res["xv"][:top, 1] = v[e, rd, slot]
    res["road"][:top] = key
    res["row"][:top] = 0 if arch is None else np.asarray(arch, np.uint8)[e, rd, slot]
    if w is not None:
        res["spawn"][:top] = np.asarray(w, np.float32)[e, rd, slot]
    return (N, offsets.astype(np.int32), res["xv"], res["road"], res["row"], res["spawn"])


def put_cars(x, v, w, arch, leading, lastcar, C, offsets, xv, row, spawn, env_ids=None, road_mask=None, new_leading=None,
             lead_x=None, spawn_shift=0, het=False):
    """The definition of tfx_put_cars (include/tfx.h) in NumPy, over ring planes - the inverse of car_list where nothing is
    clipped: x, v float32 [E, R, C] by ring slot, w float32 [E, R, C] the spawn ticks (None on handles with planes == 2),
    arch uint8 [E, R, C] (None: no rows kept), leading / lastcar int [E, R] are the image before the call; offsets int
    [n_sel * R + 1], xv float32 [cap, 2], row uint8 [cap] or None (row 0), spawn float32 [cap] or None (tick 0) the list;
    env_ids n_sel env numbers (None: selection s is env s; an id outside [0, E) writes nothing); road_mask uint8 [R] or None;
    new_leading int [n_sel * R] or None, lead_x float32 [n_sel * R] or None (+inf).  -> (x', v', w', arch', leading',
    lastcar', lost): copies; slots the call leaves unspecified keep what they held.
    For key = s * R + road: base = offsets[key], run = max(0, offsets[key + 1] - base), first = max(base, 0), fit =
    max(0, min(base + run, cap) - first); the road then holds n = min(fit, C - 2) cars, car j in slot wrap(leading' + 1 + j)
    from entry first + j; leading' = new_leading[key] where that lies in 1 .. C-1, otherwise the road's own; lastcar' the
    slot of car n - 1, leading' when n == 0; slot leading' shows lead_x[key]; lost sums run - n.  The spawn tick becomes
    float32(spawn + spawn_shift), the exact sum rounded once (heterogeneous handles, het: int(spawn) + spawn_shift modulo
    2^24, the row modulo 64)."""
    C = int(C)
    x, v = np.array(x, np.float32), np.array(v, np.float32)
    E, R = x.shape[0], x.shape[1]
    w = None if w is None else np.array(w, np.float32)
    arch = None if arch is None else np.array(arch, np.uint8)
    ld = np.array(leading, np.int64).reshape(E, R)
    lc = np.array(lastcar, np.int64).reshape(E, R)
    xv = np.asarray(xv, np.float32).reshape(-1, 2)
    cap = len(xv)
    off = np.asarray(offsets, np.int64).reshape(-1)
    ids = np.arange((len(off) - 1) // R, dtype=np.int64) if env_ids is None else np.asarray(env_ids, np.int64).reshape(-1)
    mask = np.ones(R, bool) if road_mask is None else np.asarray(road_mask).reshape(R) != 0
    shift = int(spawn_shift)
    lost = 0
    for s, env in enumerate(ids):
        if not 0 <= env < E:
            continue
        for rd in np.flatnonzero(mask):
            key = s * R + rd
            base = int(off[key])
            run = max(0, int(off[key + 1]) - base)
            first = max(base, 0)
            n = min(max(0, min(base + run, cap) - first), C - 2)
            lost += run - n
            l = ld[env, rd]
            if new_leading is not None and 1 <= int(np.asarray(new_leading).reshape(-1)[key]) <= C - 1:
                l = int(np.asarray(new_leading).reshape(-1)[key])
            slot = (l + np.arange(n)) % (C - 1) + 1
            take = first + np.arange(n)
            x[env, rd, slot] = xv[take, 0]
            v[env, rd, slot] = xv[take, 1]
            if w is not None:
                tk = np.zeros(n, np.float32) if spawn is None else np.asarray(spawn, np.float32).reshape(-1)[take]
                if het:
                    w[env, rd, slot] = ((tk.astype(np.int64) + shift) & 0xFFFFFF).astype(np.float32)
                else:
                    # (one rounding of the sum: a shift float32 does not hold is added in binary64, csrc/tfx_clone.hpp)
                    exact = float(np.float32(shift)) == float(shift)
                    w[env, rd, slot] = tk if shift == 0 else tk + np.float32(shift) if exact else \
                        (tk.astype(np.float64) + float(shift)).astype(np.float32)
            if arch is not None:
                arch[env, rd, slot] = 0 if row is None else np.asarray(row, np.uint8).reshape(-1)[take] & 63
            x[env, rd, l] = np.inf if lead_x is None else np.asarray(lead_x, np.float32).reshape(-1)[key]
            ld[env, rd] = l
            lc[env, rd] = (l + n - 1) % (C - 1) + 1 if n else l
    return x, v, w, arch, ld.astype(np.int32), lc.astype(np.int32), lost


DIGEST_CARS, DIGEST_ROWS, DIGEST_SPAWN, DIGEST_RING, DIGEST_LIGHTS, DIGEST_OBS = 1, 2, 4, 8, 16, 32
DIGEST_G = np.uint64(0x9e3779b97f4a7c15)


def digest_mix(z):
    """the splitmix64 finaliser over a uint64 array (modulo 2^64; integer arrays wrap without a warning)"""
    z = np.array(z, np.uint64)
    z ^= z >> np.uint64(30)
    z *= np.uint64(0xbf58476d1ce4e5b9)
    z ^= z >> np.uint64(27)
    z *= np.uint64(0x94d049bb133111eb)
    z ^= z >> np.uint64(31)
    return z


def _bits32(a, dtype):
    """the 32-bit patterns of an array of `dtype` (float32 / int32: as they are; uint8: zero-extended) as uint64"""
    a = np.ascontiguousarray(np.asarray(a, dtype))
    return (a if dtype == np.uint8 else a.view(np.uint32)).astype(np.uint64)


def state_digest(x, v, w, arch, leading, lastcar, C, flags, env_ids=None, road_mask=None, obs=None, rewards=None,
                 waiting=None, passed_dst=None, done_tick=None, I=None, r=None):
    """The definition of tfx_state_digest (include/tfx.h) in NumPy, over ring planes and car_list's ordering: x, v float32
    [E, R, C] by ring slot (what tfx_export_ring produces), w float32 [E, R, C] the spawn ticks, arch uint8 [E, R, C] the
    archetype rows (None: every row is 0), leading / lastcar int [E, R]; flags: a non-zero sum of DIGEST_CARS | ROWS |
    SPAWN | RING | LIGHTS | OBS.  env_ids: n_sel env numbers (None: every env in order; repeats allowed; an id outside
    [0, E) gives 0 everywhere); road_mask uint8 [R] or None (a road with mask 0 enters no digest, its road word is 0).
    LIGHTS and OBS read obs int32 [E, 2r + 2I] (passed | detected | current_phase | elapsed) with I and r given; OBS also
    rewards float32 [E, I], waiting int32 [E, r], passed_dst uint8 [E, I], done_tick int32 [E].  An array whose part is off
    is not read: pass None.  -> uint64 (env [n_sel], road [n_sel, R]).
    All arithmetic is uint64 modulo 2^64; mix = digest_mix, G = DIGEST_G.  With n the clamped ring count of a road and car
    j the j-th from its head in ring order, A_j = xbits | vbits << 32, B_j = spawnbits | row << 32 (a half is 0 where its
    part is off):  road = mix(1 + n) + [RING] mix(2 << 56 | leading) + [CARS] sum_j mix(A_j + (2j + 1) G) + [ROWS or
    SPAWN] sum_j mix(B_j + (2j + 2) G);  env = sum over unmasked roads e of mix(road_e + (e + 1) G) + the word terms
    mix(s << 56 | i << 32 | val) of sections s = 1 current_phase, 2 elapsed (LIGHTS), 3 passed, 4 detected, 5 waiting,
    6 passed_dst, 7 rewards, 8 done_tick (OBS).  With none of CARS, ROWS, SPAWN, RING no road term enters and road is 0."""
    flags = int(flags)
    if flags <= 0 or flags & ~63:
        raise ValueError("state_digest: flags 0x%x is empty or has unknown bits" % flags)
    u64 = np.uint64
    ld = np.asarray(leading, np.int64)
    E, R = ld.shape
    ids = np.arange(E, dtype=np.int64) if env_ids is None else np.asarray(env_ids, np.int64).reshape(-1)
    n_sel = len(ids)
    shown = (ids >= 0) & (ids < E)
    env = np.where(shown, ids, 0)
    mask = np.ones(R, bool) if road_mask is None else np.asarray(road_mask).reshape(R) != 0
    live = shown[:, None] & mask[None, :]                     # [n_sel, R]: roads that enter
    road = np.zeros((n_sel, R), u64)
    env_d = np.zeros(n_sel, u64)
    cars, rows, spawn = flags & DIGEST_CARS, flags & DIGEST_ROWS, flags & DIGEST_SPAWN
    if flags & (DIGEST_CARS | DIGEST_ROWS | DIGEST_SPAWN | DIGEST_RING):
        if spawn and w is None:
            raise ValueError("state_digest: DIGEST_SPAWN needs the spawn plane w")
        if cars:
            xs, vs = x, v
        else:       # car_list wants the shapes only
            xs = vs = np.zeros(ld.shape + (int(C),), np.float32)
        N, offsets, xv, key, row, sp = car_list(xs, vs, w if spawn else None, arch if rows else None, leading, lastcar, C,
                                                env_ids=ids, road_mask=road_mask)
        off = offsets.astype(np.int64)
        n = (off[1:] - off[:-1]).reshape(n_sel, R)            # clamped counts, 0 where masked or not shown
        road = digest_mix(u64(1) + n.astype(u64))
        if flags & DIGEST_RING:
            road += digest_mix((u64(2) << u64(56)) | (ld[env] & 0xFFFFFFFF).astype(u64))
        j = (np.arange(N) - off[key]).astype(u64)             # every listed car's place from the head
        if cars:
            a = _bits32(xv[:, 0], np.float32) | (_bits32(xv[:, 1], np.float32) << u64(32))
            np.add.at(road.reshape(-1), key, digest_mix(a + (u64(2) * j + u64(1)) * DIGEST_G))
        if rows or spawn:
            b = np.zeros(N, u64)
            if spawn:
                b |= _bits32(sp, np.float32)
            if rows:
                b |= row.astype(u64) << u64(32)
            np.add.at(road.reshape(-1), key, digest_mix(b + (u64(2) * j + u64(2)) * DIGEST_G))
        road = np.where(live, road, u64(0))
        e1 = (np.arange(R, dtype=u64) + u64(1)) * DIGEST_G
        env_d += np.where(live, digest_mix(road + e1[None, :]), u64(0)).sum(axis=1, dtype=u64)

    def words(s, vals):     # the terms of section s over vals [n_sel, count] of 32-bit patterns
        i = np.arange(vals.shape[1], dtype=u64)[None, :]
        t = digest_mix((u64(s) << u64(56)) | (i << u64(32)) | vals)
        return np.where(shown, t.sum(axis=1, dtype=u64), u64(0))

    if flags & (DIGEST_LIGHTS | DIGEST_OBS):
        if obs is None or I is None or r is None:
            raise ValueError("state_digest: DIGEST_LIGHTS / DIGEST_OBS need obs, I and r")
        I, r = int(I), int(r)
        ob = _bits32(np.asarray(obs).reshape(E, 2 * r + 2 * I)[env], np.int32)
        if flags & DIGEST_LIGHTS:
            env_d += words(1, ob[:, 2 * r:2 * r + I]) + words(2, ob[:, 2 * r + I:])
        if flags & DIGEST_OBS:
            env_d += words(3, ob[:, :r]) + words(4, ob[:, r:2 * r])
            env_d += words(5, _bits32(np.asarray(waiting).reshape(E, r)[env], np.int32))
            env_d += words(6, _bits32(np.asarray(passed_dst).reshape(E, I)[env], np.uint8))
            env_d += words(7, _bits32(np.asarray(rewards).reshape(E, I)[env], np.float32))
            env_d += words(8, _bits32(np.asarray(done_tick).reshape(E, 1)[env], np.int32))
    return env_d, road


def car_ages(w, leading, lastcar, C, now, het=False):
    """The definition of tfx_car_ages (include/tfx.h) in NumPy, over the ring plane w float32 [..., R, C] of spawn ticks
    by ring slot (what tfx_export_ring produces; heterogeneous handles: the spawn tick modulo 2^24), leading / lastcar
    int [..., R], `now` the handle's clock.  -> (n_cars int32, age_sum int64, age_max int32), [..., R].  Car j of a road
    sits in slot wrap(leading + 1 + j); its age is int32(float32(now) - w), or with het (now - spawn tick) & 0xFFFFFF -
    twice the trip time in seconds advance_hack would log for it in this tick.  age_max is 0 on an empty road."""
    C = int(C)
    w = np.asarray(w, np.float32)
    shape = w.shape[:-1]
    w = w.reshape(-1, C)
    ld = np.asarray(leading, np.int64).reshape(-1)
    lc = np.asarray(lastcar, np.int64).reshape(-1)
    n = lc - ld + np.where(ld > lc, C - 1, 0)
    rows = np.arange(len(ld))
    total = np.zeros(len(ld), np.int64)
    oldest = np.zeros(len(ld), np.int32)
    for j in range(C - 1):
        live = j < n
        slot = ld + 1 + j
        slot = np.where(slot > C - 1, slot - (C - 1), slot)
        slot = np.where(live, slot, 0)
        wj = w[rows, slot]
        if het:
            age = ((int(now) - wj.astype(np.int64)) & 0xFFFFFF).astype(np.int32)
        else:
            with np.errstate(invalid="ignore"):
                age = (np.float32(int(now)) - wj).astype(np.float32).astype(np.int32)
        age = np.where(live, age, 0).astype(np.int32)
        total += age
        oldest = np.maximum(oldest, age)
    return n.astype(np.int32).reshape(shape), total.reshape(shape), oldest.reshape(shape)


def trip_stats(trip_times, n_trips, trip_cap, cursor=None, edges=None):
    """The rule of tfx_trip_stats (include/tfx.h) in NumPy: trip_times float32 [E, trip_cap] (seconds, as advance_hack
    logs them), n_trips int [E], cursor int [E] or None, edges n_bins + 1 non-decreasing ints in ticks or None.
    -> (count int32 [E], tick_sum int64 [E], tick_max int32 [E], lost int32 [E], hist int32 [E, n_bins] or None,
    new_cursor int32 [E]).  Env e: n = n_trips[e]; c = cursor[e] if 0 <= cursor[e] <= n else 0; the entries i in
    [min(c, cap), min(n, cap)) count t_i = int32(trip_times[e, i] * 2) ticks; lost = max(n, cap) - max(c, cap);
    hist[b] = #{i: edges[b] <= t_i < edges[b + 1]}; new_cursor = n."""
    cap = int(trip_cap)
    tt = np.asarray(trip_times, np.float32).reshape(-1, cap)
    n_trips = np.asarray(n_trips, np.int64).reshape(-1)
    E = len(n_trips)
    cur = np.zeros(E, np.int64) if cursor is None else np.asarray(cursor, np.int64).reshape(-1)
    ed = None if edges is None else np.asarray(edges, np.int64).reshape(-1)
    count = np.zeros(E, np.int32)
    tick_sum = np.zeros(E, np.int64)
    tick_max = np.zeros(E, np.int32)
    lost = np.zeros(E, np.int32)
    hist = None if ed is None else np.zeros((E, len(ed) - 1), np.int32)
    for e in range(E):
        n = int(n_trips[e])
        c = int(cur[e])
        if c < 0 or c > n:
            c = 0
        lo, hi = min(c, cap), min(n, cap)
        t = (tt[e, lo:max(lo, hi)] * np.float32(2.0)).astype(np.int32)
        count[e] = len(t)
        tick_sum[e] = t.astype(np.int64).sum()
        tick_max[e] = t.max() if len(t) else 0
        lost[e] = max(n, cap) - max(c, cap)
        if ed is not None:
            for b in range(len(ed) - 1):
                hist[e, b] = np.count_nonzero((t >= ed[b]) & (t < ed[b + 1]))
    return count, tick_sum, tick_max, lost, hist, n_trips.astype(np.int32)


def cell_edges(length, n_cells):
    """float32 edges [-inf, e_1 .. e_{n-1}, +inf] of n_cells equal cells of a road of `length`: e_b = float32(length * b /
    n_cells), computed in binary64.  The outer edges are infinite, so every car is in some cell (a car that overshot the
    road end is in the last one) and the cells of a road sum to its cars_on_roads."""
    n_cells = int(n_cells)
    if n_cells < 1:
        raise ValueError("cell_edges: n_cells must be at least 1")
    e = np.empty(n_cells + 1, np.float32)
    e[0], e[n_cells] = -np.inf, np.inf
    for b in range(1, n_cells):
        e[b] = np.float32(float(length) * b / n_cells)
    return e


def road_cells(x, v, leading, lastcar, C, edges):
    """The definition of tfx_road_cells (include/tfx.h) in NumPy, over ring planes: x, v float32 [..., R, C] by ring slot
    (what tfx_export_ring produces), leading / lastcar int [..., R], edges float32 [B + 1] strictly ascending.
    -> (n_cars int32 [..., R, B], speed_sum float32 [..., R, B]).  Car j of a road (j = 0: the head) sits in slot
    wrap(leading + 1 + j); it is in range iff edges[0] <= x < edges[B] (a NaN x is in no cell); its cell is the number
    of inner edges k = 1 .. B-1 with x >= edges[k] - comparisons only, a car on an edge goes to the upper cell;
    speed_sum adds v of a cell's cars one at a time in ascending j, in float32, starting from 0 - the order the device
    keeps, so the bits agree."""
    C = int(C)
    edges = np.asarray(edges, np.float32).reshape(-1)
    B = len(edges) - 1
    if B < 1 or np.isnan(edges).any() or not (edges[:-1] < edges[1:]).all():
        raise ValueError("road_cells: edges must be at least two strictly ascending float32 values")
    x = np.asarray(x, np.float32)
    v = np.asarray(v, np.float32)
    shape = x.shape[:-1]
    x, v = x.reshape(-1, C), v.reshape(-1, C)
    ld = np.asarray(leading, np.int64).reshape(-1)
    lc = np.asarray(lastcar, np.int64).reshape(-1)
    n = lc - ld + np.where(ld > lc, C - 1, 0)
    rows = np.arange(len(ld))
    cars = np.zeros((len(ld), B), np.int32)
    total = np.zeros((len(ld), B), np.float32)
    for j in range(C - 1):
        live = j < n
        slot = ld + 1 + j
        slot = np.where(slot > C - 1, slot - (C - 1), slot)
        slot = np.where(live, slot, 0)
        xj, vj = x[rows, slot], v[rows, slot]
        with np.errstate(invalid="ignore"):
            inr = live & (xj >= edges[0]) & (xj < edges[B])
            b = (xj[:, None] >= edges[None, 1:B]).sum(axis=1)
            added = (total[rows, b] + vj).astype(np.float32)      # one float32 add per car
        at = rows[inr], b[inr]
        cars[at] += 1
        total[at] = added[inr]
    return cars.reshape(shape + (B,)), total.reshape(shape + (B,))


FRAME_GREEN, FRAME_YELLOW, FRAME_RED, FRAME_CAR = (0, 255, 0, 255), (255, 255, 0, 255), (255, 0, 0, 255), (0, 0, 255, 255)


def frame_geometry(m, n, px):
    """The roads of tfx_frames (include/tfx.h) on an m x n grid at px = S pixels per road length -> (start int64 [R, 2],
    step int64 [R, 2], (H, W)): road e has the pixel t along it at (column, row) = start[e] + t * step[e] and owns t =
    2 .. S - 2.  Train road d * m * n + row * n + col runs into the intersection centred at (cx, cy) = ((col + 1) * S,
    (row + 1) * S), one pixel beside the centre line on the side of GridRoad._unit_segments' eps; the four exit blocks,
    in that function's order, continue d = 3, 0, 2, 1 from the centre of their road's intersection away from the grid."""
    m, n, S = int(m), int(n), int(px)
    v = m * n
    R = 4 * v + 2 * n + 2 * m
    cell = np.arange(v)
    cy, cx = (cell // n + 1) * S, (cell % n + 1) * S
    start, step = np.zeros((R, 2), np.int64), np.zeros((R, 2), np.int64)
    # per direction: offset of the start from the centre in units of S, offset beside the centre line, step
    along = {0: ((-1, 0), (0, -1), (1, 0)), 1: ((1, 0), (0, 1), (-1, 0)), 2: ((0, -1), (1, 0), (0, 1)), 3: ((0, 1), (-1, 0), (0, -1))}

    def put(roads, d, cx, cy, back):
        (bx, by), (ox, oy), st = along[d]
        start[roads, 0], start[roads, 1] = cx + back * bx * S + ox, cy + back * by * S + oy
        step[roads] = st
    for d in range(4):
        put(slice(d * v, (d + 1) * v), d, cx, cy, 1)
    b = 4 * v
    j, i = np.arange(n), np.arange(m)
    put(slice(b, b + n), 3, (j + 1) * S, S, 0)                            # out of row 0
    put(slice(b + n, b + n + m), 0, n * S, (i + 1) * S, 0)                # out of the last column
    put(slice(b + n + m, b + 2 * n + m), 2, (j + 1) * S, m * S, 0)        # out of the last row
    put(slice(b + 2 * n + m, R), 1, S, (i + 1) * S, 0)                    # out of column 0
    return start, step, ((m + 1) * S + 1, (n + 1) * S + 1)


def _frame_pixel(t, top):
    """clamp(floor(t), 0, top) in float32 before the conversion (a NaN gives 0)"""
    with np.errstate(invalid="ignore"):
        fl = np.floor(np.asarray(t, np.float32))
        return np.where(fl >= 0, np.where(fl > top, top, fl), np.float32(0)).astype(np.int64)


def frames(x, leading, lastcar, current_phase, elapsed, m, n, px, length, yellow_ticks=6, car_l=4.0, rows=None,
           lengths=None, env_ids=None):
    """The definition of tfx_frames (include/tfx.h) in NumPy -> uint8 [n_frames, H, W, 4] (R, G, B, A).  x float32 [E, R,
    C] by ring slot (what tfx_export_ring produces), leading / lastcar int [E, R], current_phase / elapsed int [E, I] (the
    light words of obs), m, n the grid, px = S pixels per road length, length the road length, yellow_ticks the
    yellow time.  A car's length: car_l, or - with rows uint8 [E, R, C] (the archetype row of every ring slot) and
    lengths float32 [rows of the table] - lengths[rows].  env_ids: the env of every frame (None: every env in order; an
    id outside [0, E) gives an all-0xFF frame).  A pure function of its arguments: phases and destinations of the roads
    are arithmetic on their ids, as in GridRoad.  Car j of a road sits in ring slot wrap(leading + 1 + j); with k =
    float32(S - 3) / float32(length) it turns pixels t = 2 + b .. 2 + a blue, a = clamp(floor(x * k), 0, S - 4), b =
    clamp(floor((x - l) * k), 0, S - 4), one float32 rounding per operation; a car whose x is NaN is not drawn."""
    m, n, S = int(m), int(n), int(px)
    if not 8 <= S <= 256:
        raise ValueError("frames: px must be in 8 .. 256")
    x = np.asarray(x, np.float32)
    E, R, C = x.shape
    v = m * n
    if R != 4 * v + 2 * n + 2 * m:
        raise ValueError("frames: x holds %d roads, an %d x %d grid has %d" % (R, m, n, 4 * v + 2 * n + 2 * m))
    ld_all = np.asarray(leading, np.int64).reshape(E, R)
    lc_all = np.asarray(lastcar, np.int64).reshape(E, R)
    phase_now = np.asarray(current_phase, np.int64).reshape(E, v)
    age = np.asarray(elapsed, np.int64).reshape(E, v)
    ids = np.arange(E) if env_ids is None else np.asarray(env_ids, np.int64).reshape(-1)
    start, step, (H, W) = frame_geometry(m, n, S)
    k = np.float32(S - 3) / np.float32(length)
    top = np.float32(S - 4)
    road = np.arange(4 * v)
    road_phase, dst = (road < 2 * v).astype(np.int64), road % v
    out = np.full((len(ids), H, W, 4), 255, np.uint8)
    t_own = np.arange(2, S - 1)
    for f, env in enumerate(ids):
        if not 0 <= env < E:
            continue
        mine = road_phase == phase_now[env, dst]
        fresh = age[env, dst] < int(yellow_ticks)
        colour = np.empty((R, 4), np.uint8)
        colour[:] = FRAME_GREEN
        colour[:4 * v][mine & fresh] = FRAME_YELLOW
        colour[:4 * v][mine != fresh] = FRAME_RED
        for e in range(R):
            cols = start[e, 0] + t_own * step[e, 0]
            rws = start[e, 1] + t_own * step[e, 1]
            line = np.empty((S - 3, 4), np.uint8)
            line[:] = colour[e]
            ld, lc = int(ld_all[env, e]), int(lc_all[env, e])
            slot = ld
            for _ in range(lc - ld + (C - 1 if ld > lc else 0)):
                slot = slot + 1 if slot + 1 < C else 1
                xj = x[env, e, slot]
                if np.isnan(xj):
                    continue
                lj = np.float32(car_l if rows is None else np.asarray(lengths, np.float32)[int(rows[env, e, slot])])
                with np.errstate(invalid="ignore", over="ignore"):
                    a = int(_frame_pixel(np.float32(xj * k), top))
                    b = int(_frame_pixel(np.float32(np.float32(xj - lj) * k), top))
                line[b:a + 1] = FRAME_CAR
            out[f, rws, cols] = line
    return out


def gap_table(cars_per_tick, tail=1e-12):
    """uint32 thresholds cdf[k] = floor(P(gap <= k) * 2^32), last entry 0xFFFFFFFF."""
    mean = 1.0 / float(cars_per_tick)
    cdf = []
    k = 0
    while True:
        p = 1.0 - math.exp(-(k + 0.5) / mean)            # P(Exp(mean) < k + 1/2)
        cdf.append(min(MASK, int(p * 4294967296.0)))
        if 1.0 - p < tail or k > 60000:
            break
        k += 1
    cdf[-1] = MASK
    return np.asarray(cdf, np.uint32)


class _Rows(object):
    """Rule 1 for the envs of a mirror: `seq` [len(env_ids), n_entry] cars put on each entry road so far."""

    def __init__(self, n_archetypes, per_road, n_envs, n_entry, k0, k1):
        self.n_archetypes, self.S = int(n_archetypes), int(per_road)
        if not 1 <= self.n_archetypes <= 64 or self.S < 1:
            raise ValueError("n_archetypes must be in 1..64 and per_road >= 1")
        self.seq = np.zeros((n_envs, n_entry), np.uint64)
        self.k0, self.k1 = k0, k1

    def tick(self, counts, env_ids, draw=True):
        """uint8 [len(env_ids), n_entry, S]: row of car j of each entry road this tick for j < min(count, S), 0 past the
        cars; advances seq by the full counts.  draw=False (the regular stream): every car is row 0."""
        n_env, n_entry = counts.shape
        rows = np.zeros((n_env, n_entry, self.S), np.uint8)
        if draw and self.n_archetypes > 1:
            for r, g in enumerate(env_ids):
                m = np.minimum(counts[r], self.S).astype(np.int64)
                if not m.any():
                    continue
                ej = np.repeat(np.arange(n_entry), m)
                j = np.arange(ej.size) - np.repeat(np.cumsum(m) - m, m)
                u = philox4x32_first((self.seq[r, ej] + j.astype(np.uint64)) & np.uint64(MASK), g, TAG_ARCH,
                                     ej.astype(np.uint64), self.k0, self.k1)
                rows[r, ej, j] = ((u * np.uint64(self.n_archetypes)) >> np.uint64(32)).astype(np.uint8)
        self.seq += counts.astype(np.uint64)
        return rows


def _rows_or_none(n_archetypes, per_road, n_envs, n_entry, k0, k1):
    if per_road is None:
        if int(n_archetypes) > 1:
            raise ValueError("rows of an archetype table need per_road (the engine's capacity - 2)")
        return None
    return _Rows(n_archetypes, per_road, n_envs, n_entry, k0, k1)


def cars_of(counts, rows, entrypoints):
    """One env's tick as the oracle takes it: (roads, rows) lists of its cars, grouped by entry road in entry-index order
    and in creation order within a road (cars past the S rows held per road get row 0: they overflow)."""
    roads, arch = [], []
    S = rows.shape[-1]
    for ej, c in enumerate(counts):
        c = int(c)
        roads += [int(entrypoints[ej])] * c
        arch += [int(a) for a in rows[ej, :min(c, S)]] + [0] * max(0, c - S)
    return roads, arch


class PoissonMirror(object):
    """Draw 0 = the first gap; car c uses draw 1 + 2c for its entry road and draw 2 + 2c for the gap
    that follows it (the device evaluates 64 cars at a time from these fixed indices)."""

    def __init__(self, cars_per_tick, seed, n_entry, env_ids, n_archetypes=1, per_road=None):
        """n_archetypes > 1 (with per_road = the engine's capacity - 2, the S of rule 1): next_tick also returns
        the rows of the tick's cars (also with per_road given for a single row: all 0)."""
        self.cdf = [int(c) for c in gap_table(cars_per_tick)]
        self.cdf_np = np.asarray(self.cdf[:-1], np.uint64)
        self.k0, self.k1 = int(seed) & MASK, (int(seed) >> 32) & MASK
        self.n_entry = int(n_entry)
        self.env_ids = [int(e) for e in env_ids]
        self.gap = {e: -1 for e in self.env_ids}
        self.car = {e: 0 for e in self.env_ids}
        self.rows = _rows_or_none(n_archetypes, per_road, len(self.env_ids), self.n_entry, self.k0, self.k1)

    def _gap(self, e, draw):
        u = philox4x32(draw & MASK, e, TAG_GAP, 0, self.k0, self.k1)[0]
        k = 0
        while k < len(self.cdf) - 1 and u >= self.cdf[k]:
            k += 1
        return k

    def next_tick(self, frozen=()):
        """int32 [len(env_ids), n_entry] cars per entry road this tick (entry index order); with rows: (counts, uint8
        [len(env_ids), n_entry, S] row of car j of each road).  Envs in `frozen` (global ids) draw nothing."""
        out = np.zeros((len(self.env_ids), self.n_entry), np.int32)
        for row, e in enumerate(self.env_ids):
            if e in frozen:
                continue
            if self.gap[e] < 0:
                self.gap[e] = self._gap(e, 0)
            if self.gap[e] > 0:
                self.gap[e] -= 1
                continue
            while True:
                # 64 consecutive cars at a time, like the device's wavefront (bursts of thousands of
                # cars per tick at cfg4's rate): every car up to the first non-zero gap arrives now
                c = self.car[e] + np.arange(64, dtype=np.uint64)
                ug = philox4x32_first(np.uint64(2) + np.uint64(2) * c, e, TAG_GAP, 0, self.k0, self.k1)
                gaps = np.searchsorted(self.cdf_np, ug, side='right')     # k with cdf[k-1] <= u < cdf[k]
                stop = np.nonzero(gaps > 0)[0]
                f = int(stop[0]) if stop.size else 63
                ur = philox4x32_first(np.uint64(1) + np.uint64(2) * c[:f + 1], e, TAG_ROAD, 0, self.k0, self.k1)
                np.add.at(out[row], ((ur * np.uint64(self.n_entry)) >> np.uint64(32)).astype(np.int64), 1)
                self.car[e] += f + 1
                if stop.size:
                    self.gap[e] = int(gaps[f]) - 1
                    break
        return out if self.rows is None else (out, self.rows.tick(out, self.env_ids))


class RegularMirror(object):
    """Host mirror of the on-device `regular` generator (tfx_set_regular; the reference's traffic_env.py:167-176):
    `burst` = ceil(cars_per_tick) cars in every tick i of an env's generator with i % every == 0, every =
    round(1 / cars_per_tick); car c of env e (counted over the env's whole stream) enters on entry index
    floor(u * n_entry / 2^32) with u the first word of draw 1 + 2c of the env's Philox stream."""

    def __init__(self, cars_per_tick, seed, n_entry, env_ids, n_archetypes=1, per_road=None):
        """n_archetypes / per_road as in PoissonMirror: the rows returned are all 0 (the reference's `regular`
        generator yields archetypes[0], traffic_env.py:174)."""
        self.every, self.burst = round(1 / cars_per_tick), math.ceil(cars_per_tick)
        self.k0, self.k1 = int(seed) & MASK, (int(seed) >> 32) & MASK
        self.n_entry = int(n_entry)
        self.env_ids = [int(e) for e in env_ids]
        self.i = {e: 0 for e in self.env_ids}
        self.car = {e: 0 for e in self.env_ids}
        self.rows = _rows_or_none(n_archetypes, per_road, len(self.env_ids), self.n_entry, self.k0, self.k1)

    def next_tick(self, frozen=()):
        """int32 [len(env_ids), n_entry] cars per entry road this tick (entry index order); with rows: (counts, rows)."""
        out = np.zeros((len(self.env_ids), self.n_entry), np.int32)
        for row, e in enumerate(self.env_ids):
            if e in frozen:
                continue
            due = self.every == 0 or self.i[e] % self.every == 0
            self.i[e] += 1
            if due:
                c = self.car[e] + np.arange(self.burst, dtype=np.uint64)
                ur = philox4x32_first(np.uint64(1) + np.uint64(2) * c, e, TAG_ROAD, 0, self.k0, self.k1)
                np.add.at(out[row], ((ur * np.uint64(self.n_entry)) >> np.uint64(32)).astype(np.int64), 1)
                self.car[e] += self.burst
        return out if self.rows is None else (out, self.rows.tick(out, self.env_ids, draw=False))


# ---- demand profiles (tfx_set_demand, rule 4 of include/tfx.h) ----------------------------------------------------------
DemandTables = collections.namedtuple("DemandTables", "count_cdf road_cdf")
DEMAND_MAX_CDF = 256


def _poisson_cdf(mean, n):
    """P(N <= c) for c = 0 .. n-1, N ~ Poisson(mean), in binary64 (the terms through logarithms: no overflow)."""
    if mean == 0.0:
        return np.ones(n)
    c = np.arange(n, dtype=np.float64)
    lg = np.array([math.lgamma(i + 1.0) for i in range(n)])
    return np.minimum(np.cumsum(np.exp(c * math.log(mean) - mean - lg)), 1.0)


def _thresholds(p):
    """min(floor(p * 2^32), 0xFFFFFFFF) along the last axis, the last entry forced to 0xFFFFFFFF."""
    t = np.minimum(np.floor(np.asarray(p, np.float64) * 4294967296.0), float(MASK)).astype(np.uint64)
    t = np.maximum.accumulate(t, axis=-1)
    t[..., -1] = MASK
    return t.astype(np.uint32)


def demand_tables(means, weights=None, n_cdf=None, n_entry=None, tail=1e-12):
    """The two host tables of tfx_set_demand -> DemandTables(count_cdf uint32 [K, S, n_cdf], road_cdf uint32 [K, S, n_entry]).
    means: [K][S] mean cars per env per tick of profile k in segment s (>= 0).  weights: [K][S][n_entry] (or [n_entry],
    for every profile and segment) non-negative weights of the entry roads, in entry-index order; None: equal weights
    (then n_entry is needed).  A road of weight zero receives no car.  n_cdf: entries per count row (at most n_cdf - 1
    cars per env per tick); default: the smallest one that leaves less than `tail` of any row's mass beyond it, capped
    at 256.  count_cdf[k][s][c] = min(floor(P(N <= c) * 2^32), 0xFFFFFFFF) for N ~ Poisson(means[k][s]); road_cdf holds the
    cumulative weights scaled the same way; the last entry of every row is 0xFFFFFFFF."""
    means = np.asarray(means, np.float64)
    if means.ndim != 2 or means.size == 0 or not np.all(np.isfinite(means)) or (means < 0).any():
        raise ValueError("means must be a [K][S] array of finite values >= 0")
    K, S = means.shape
    if weights is None:
        if n_entry is None:
            raise ValueError("equal weights need n_entry")
        weights = np.ones(int(n_entry))
    weights = np.asarray(weights, np.float64)
    if weights.ndim == 1:
        weights = np.broadcast_to(weights, (K, S, weights.shape[0]))
    if weights.shape[:2] != (K, S) or weights.ndim != 3 or weights.shape[2] < 1:
        raise ValueError("weights must be [K][S][n_entry] (or [n_entry])")
    if n_entry is not None and weights.shape[2] != int(n_entry):
        raise ValueError("weights hold %d entry roads, n_entry is %d" % (weights.shape[2], int(n_entry)))
    if not np.all(np.isfinite(weights)) or (weights < 0).any() or (weights.sum(axis=-1) <= 0).any():
        raise ValueError("weights must be finite, >= 0, and not all zero in any row")
    if n_cdf is None:
        n_cdf = 1
        for mean in means.ravel():
            cdf = _poisson_cdf(float(mean), DEMAND_MAX_CDF)
            enough = np.nonzero(1.0 - cdf < tail)[0]
            n_cdf = max(n_cdf, int(enough[0]) + 1 if enough.size else DEMAND_MAX_CDF)
    n_cdf = int(n_cdf)
    if not 1 <= n_cdf <= DEMAND_MAX_CDF:
        raise ValueError("n_cdf must be in 1..%d" % DEMAND_MAX_CDF)
    count = np.stack([np.stack([_poisson_cdf(float(means[k, s]), n_cdf) for s in range(S)]) for k in range(K)])
    road = np.cumsum(weights, axis=-1) / weights.sum(axis=-1, keepdims=True)
    return DemandTables(_thresholds(count), _thresholds(road))


def _clock32(ticks):
    """int64 array of the int32 clock values the ticks wrap to"""
    t = np.asarray(ticks, np.int64)
    return ((t + (1 << 31)) & MASK) - (1 << 31)


def demand_segment(ticks, n_segments, seg_ticks=1, tick_offset=0):
    """Segment of clock tick(s) t (rule 4): floormod(t + tick_offset, n_segments * seg_ticks) // seg_ticks, in 64 bits.
    The device clock is an int32 that wraps: ticks outside the int32 range are wrapped into it first, as the device
    does with `clock + row`."""
    t = _clock32(ticks) + np.int64(tick_offset)
    return (np.mod(t, np.int64(int(n_segments) * int(seg_ticks))) // np.int64(seg_ticks)).astype(np.int64)


def demand_row_table(row_weights, K, S, n_rows):
    """The third host table of tfx_set_demand_mixed -> row_cdf uint32 [K, S, n_rows]: the cumulative weights of the
    archetype-table rows of profile k in segment s, scaled by 2^32, the last entry of every row 0xFFFFFFFF (the format of
    DemandTables.road_cdf).  row_weights: [K][S][n_rows] (or [n_rows], for every profile and segment) non-negative
    weights; None: equal weights.  A row of weight zero is not drawn (a LAST row of weight zero: for one v in 2^32)."""
    K, S, n_rows = int(K), int(S), int(n_rows)
    if not 1 <= n_rows <= 64:
        raise ValueError("n_rows must be in 1..64")
    w = np.ones(n_rows) if row_weights is None else np.asarray(row_weights, np.float64)
    if w.ndim == 1:
        w = np.broadcast_to(w, (K, S, w.shape[0]))
    if w.shape != (K, S, n_rows):
        raise ValueError("row_weights must be [%d][%d][%d] (or [%d])" % (K, S, n_rows, n_rows))
    if not np.all(np.isfinite(w)) or (w < 0).any() or (w.sum(axis=-1) <= 0).any():
        raise ValueError("row_weights must be finite, >= 0, and not all zero in any row")
    return _thresholds(np.cumsum(w, axis=-1) / w.sum(axis=-1, keepdims=True))


def demand_counts(seed, stream_ids, ticks, tables, profile_of_env=None, seg_ticks=1, tick_offset=0):
    """Rule 4 of include/tfx.h in NumPy -> int32 [T, E, n_entry]: the cars env e (stream id stream_ids[e]: its global env
    id, or its source's after a clone with its stream) receives on each entry road in clock tick ticks[t] (an int32 clock
    value; anything else wraps to one, as the device clock does).  tables: a
    DemandTables; profile_of_env: int [E] (None: profile 0; outside [0, K): no cars).  A pure function of its arguments:
    any subset of envs or ticks, in any order, gives the same rows."""
    return _demand(seed, stream_ids, ticks, tables, profile_of_env, seg_ticks, tick_offset)


def demand_rows(seed, stream_ids, ticks, tables, row_cdf, per_road, profile_of_env=None, seg_ticks=1, tick_offset=0):
    """Rules 4 and 5 of include/tfx.h in NumPy -> (counts int32 [T, E, n_entry] - demand_counts' -, rows uint8 [T, E,
    n_entry, per_road]): rows[t, e, ej, j] is the archetype-table row of the j-th car, in car-index order, that env e
    receives on entry road ej in clock tick ticks[t], for j < min(count, per_road); 0 past it.  row_cdf: uint32 [K, S,
    n_rows] (demand_row_table); per_road: the S of rule 5, min(capacity - 2, n_cdf - 1) on the device.  Pure, like
    demand_counts: any subset of envs or ticks, in any order, gives the same rows."""
    return _demand(seed, stream_ids, ticks, tables, profile_of_env, seg_ticks, tick_offset, row_cdf, int(per_road))


def _demand(seed, stream_ids, ticks, tables, profile_of_env, seg_ticks, tick_offset, row_cdf=None, per_road=0):
    """demand_counts (row_cdf None) or demand_rows"""
    count_cdf, road_cdf = [np.asarray(a, np.uint32).astype(np.uint64) for a in tables]
    K, S, n_cdf = count_cdf.shape
    ne = road_cdf.shape[2]
    g = np.asarray(stream_ids, np.int64).reshape(-1) & MASK
    t = _clock32(ticks).reshape(-1)
    T, E = len(t), len(g)
    prof = np.zeros(E, np.int64) if profile_of_env is None else np.asarray(profile_of_env, np.int64).reshape(-1)
    if len(prof) != E:
        raise ValueError("profile_of_env must hold one profile per env")
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    k0, k1 = seed & MASK, seed >> 32
    out = np.zeros((T, E, ne), np.int32)
    arch = None
    if row_cdf is not None:
        row_cdf = np.asarray(row_cdf, np.uint32).astype(np.uint64)
        if row_cdf.ndim != 3 or row_cdf.shape[:2] != (K, S) or per_road < 0:
            raise ValueError("row_cdf must be [K][S][n_rows] for the tables' K and S, per_road >= 0")
        n_rows = row_cdf.shape[2]
        row_rows = row_cdf.reshape(K * S, n_rows)
        arch = np.zeros((T, E, ne, per_road), np.uint8)
    ret = (lambda: out) if arch is None else (lambda: (out, arch))
    if T == 0 or E == 0:
        return ret()
    valid = (prof >= 0) & (prof < K)
    k = np.where(valid, prof, 0)
    seg = demand_segment(t, S, seg_ticks, tick_offset)
    tw = np.broadcast_to((t & MASK)[:, None], (T, E))
    gw = np.broadcast_to(g[None, :], (T, E))
    u0 = philox4x32_first(tw, gw, TAG_DCNT, 0, k0, k1)
    rows = count_cdf[k[None, :], seg[:, None]]                       # [T, E, n_cdf]
    N = (u0[..., None] >= rows[..., :n_cdf - 1]).sum(axis=-1)
    N = np.where(valid[None, :], N, 0).reshape(-1)
    if ne == 1 and arch is None:
        out.reshape(-1)[:] = N
        return out
    item = np.repeat(np.arange(T * E), N)
    if item.size == 0:
        return ret()
    c = np.arange(item.size) - np.repeat(np.cumsum(N) - N, N)      # car index within its item
    flat = out.reshape(-1)
    ks = (k[None, :] * S + seg[:, None]).reshape(-1)
    road_rows = road_cdf.reshape(K * S, ne)
    for lo in range(0, item.size, 1 << 18):
        it, cc = item[lo:lo + (1 << 18)], c[lo:lo + (1 << 18)]
        words = philox4x32_words(tw.reshape(-1)[it], gw.reshape(-1)[it], TAG_DROAD, cc >> 2, k0, k1)
        w = np.choose(cc & 3, words)
        ej = (w[:, None] >= road_rows[ks[it]][:, :ne - 1]).sum(axis=1)
        road = it * ne + ej
        if arch is not None and per_road > 0:
            # rule 5.  The cars of the chunk stand in (item, car index) order: a stable sort by road keeps the car-index
            # order within a road; the cars of the chunks before are in `flat` already
            order = np.argsort(road, kind="stable")
            sr = road[order]
            first = np.nonzero(np.r_[True, sr[1:] != sr[:-1]])[0]
            run = np.diff(np.r_[first, sr.size])
            j = np.empty(sr.size, np.int64)
            j[order] = np.arange(sr.size) - np.repeat(first, run)
            j += flat[road]
            words = philox4x32_words(tw.reshape(-1)[it], gw.reshape(-1)[it], TAG_DROW, cc >> 2, k0, k1)
            v = np.choose(cc & 3, words)
            row = (v[:, None] >= row_rows[ks[it]][:, :n_rows - 1]).sum(axis=1)
            keep = j < per_road
            arch.reshape(-1)[road[keep] * per_road + j[keep]] = row[keep].astype(np.uint8)
        flat += np.bincount(road, minlength=flat.size).astype(np.int32)
    return ret()
