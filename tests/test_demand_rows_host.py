"""Archetype rows of demand cars (tfx_set_demand_mixed, rule 5 of include/tfx.h), the parts that need no GPU: the third
threshold table, the rule as a NumPy function (devrng.demand_rows - what tests/test_gpu_demand_rows.py holds the device to)
against a plain-Python statement of it, its purity, both branches of S = min(C - 2, n_cdf - 1), and the declarations."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from test_demand_host import MASK

HEADER = os.path.join(ROOT, "include", "tfx.h")

# the configuration of tests/test_gpu_demand.py: a 2x2 grid with one side closed has 6 entry roads; capacity 14
SEED, IDS, PROFILE = (0xABCD << 32) | 77, np.arange(40, 45), [0, 1, -1, 2, 1]
MEANS = [[0.5, 70.0, 0.0], [2.0, 1.0, 9.0]]
KW = dict(seg_ticks=2, tick_offset=3)
N_ENTRY, PER_ROAD, N_ROWS = 6, 12, 3
RANGES = ((3, 7), (-9, 7), (2 ** 31 - 2, 4))
ZERO_ROW_1, ONLY_ROW_2 = (0, 1), (1, 2)       # the (k, s) whose row 1 has weight zero / whose weights are [0, 0, 1]


def road_weights(n_entry=N_ENTRY, K=2, S=3):
    return np.random.RandomState(0).rand(K, S, n_entry) + 0.05        # (tests/test_gpu_demand.py's weights())


def row_weights(K=2, S=3, n_rows=N_ROWS):
    w = np.random.RandomState(1).rand(K, S, n_rows) + 0.05
    w[ZERO_ROW_1][1] = 0.0
    w[ONLY_ROW_2] = [0.0, 0.0, 1.0]
    return w


def tables():
    from gym_traffic import devrng as d
    return d.demand_tables(MEANS, road_weights()), d.demand_row_table(row_weights(), 2, 3, N_ROWS)


def rule5(seed, g, t, cc, rc, rw, k, seg_ticks, off, per_road):
    """Rules 4 and 5 of include/tfx.h for one (tick, env), line by line in plain Python -> (counts [n_entry], rows
    [n_entry][per_road], 0 where the rule stores nothing)"""
    from gym_traffic import devrng as d
    K, S, n_cdf = cc.shape
    ne, n_rows = rc.shape[2], rw.shape[2]
    counts, rows = [0] * ne, [[0] * per_road for _ in range(ne)]
    if not 0 <= k < K:
        return counts, rows
    s = ((t + off) % (S * seg_ticks)) // seg_ticks
    k0, k1 = seed & MASK, seed >> 32
    u = d.philox4x32(t & MASK, g, d.TAG_DCNT, 0, k0, k1)
    N = sum(1 for c in range(n_cdf - 1) if u[0] >= int(cc[k, s, c]))
    for c in range(N):
        w = d.philox4x32(t & MASK, g, d.TAG_DROAD, c >> 2, k0, k1)[c & 3]
        ej = sum(1 for j in range(ne - 1) if w >= int(rc[k, s, j]))
        v = d.philox4x32(t & MASK, g, d.TAG_DROW, c >> 2, k0, k1)[c & 3]
        row = sum(1 for i in range(n_rows - 1) if v >= int(rw[k, s, i]))
        j = counts[ej]                                   # the cars c' < c with the same entry road
        if j < per_road:
            rows[ej][j] = row
        counts[ej] += 1
    return counts, rows


def clock32(t):
    return ((int(t) + 2 ** 31) & MASK) - 2 ** 31


def test_model_is_rule_5():
    from gym_traffic import devrng as d
    assert d.TAG_DROW == 0x44524F57
    assert len({d.TAG_DROW, d.TAG_DCNT, d.TAG_DROAD, d.TAG_GAP, d.TAG_ROAD, d.TAG_ARCH, d.TAG_EPISODE, d.TAG_POOL}) == 8
    tb, rw = tables()
    assert rw.shape == (2, 3, 3) and rw.dtype == np.uint32
    seen = {"item": 0, "over": 0, "mixed": 0}
    drawn = {ZERO_ROW_1: set(), ONLY_ROW_2: set()}
    for tick0, n in RANGES:
        ticks = np.arange(tick0, tick0 + n)
        counts, rows = d.demand_rows(SEED, IDS, ticks, tb, rw, PER_ROAD, PROFILE, **KW)
        assert counts.dtype == np.int32 and counts.shape == (n, 5, N_ENTRY)
        assert rows.dtype == np.uint8 and rows.shape == (n, 5, N_ENTRY, PER_ROAD)
        assert np.array_equal(counts, d.demand_counts(SEED, IDS, ticks, tb, PROFILE, **KW))
        seg = d.demand_segment(ticks, 3, **KW)
        for i, t in enumerate(ticks):
            for e in range(5):
                wc, wr = rule5(SEED, int(IDS[e]), clock32(t), tb.count_cdf, tb.road_cdf, rw, PROFILE[e], 2, 3, PER_ROAD)
                assert counts[i, e].tolist() == wc and rows[i, e].tolist() == wr, (t, e)
                seen["item"] = max(seen["item"], sum(wc))
                for ej, c in enumerate(wc):
                    live = wr[ej][:min(c, PER_ROAD)]
                    seen["over"] += c > PER_ROAD
                    seen["mixed"] += len(set(live)) > 1
                    key = (PROFILE[e], int(seg[i]))
                    if key in drawn:
                        drawn[key].update(live)
    # the preconditions: a second round of 64 cars, a road past its rows, mixed rows on one road, the zero weights
    assert seen["item"] > 64 and seen["over"] >= 1 and seen["mixed"] >= 1, seen
    assert drawn[ZERO_ROW_1] == {0, 2} and drawn[ONLY_ROW_2] == {2}, drawn


def test_rows_are_pure():
    """any subset or permutation of envs and ticks gives the same rows; two shards equal the whole"""
    from gym_traffic import devrng as d
    tb, rw = tables()
    ticks, prof = np.arange(-9, 10), np.asarray(PROFILE)
    counts, rows = d.demand_rows(SEED, IDS, ticks, tb, rw, PER_ROAD, prof, **KW)
    rng = np.random.RandomState(2)
    for _ in range(4):
        ti, ei = rng.permutation(len(ticks))[:rng.randint(1, len(ticks))], rng.permutation(5)[:rng.randint(1, 5)]
        c, r = d.demand_rows(SEED, IDS[ei], ticks[ti], tb, rw, PER_ROAD, prof[ei], **KW)
        assert np.array_equal(c, counts[ti][:, ei]) and np.array_equal(r, rows[ti][:, ei])
    lo = d.demand_rows(SEED, IDS[:2], ticks, tb, rw, PER_ROAD, prof[:2], **KW)
    hi = d.demand_rows(SEED, IDS[2:], ticks, tb, rw, PER_ROAD, prof[2:], **KW)
    assert np.array_equal(np.concatenate([lo[1], hi[1]], axis=1), rows) and np.array_equal(np.concatenate([lo[0], hi[0]], axis=1), counts)
    c, r = d.demand_rows(SEED, IDS, [], tb, rw, PER_ROAD, prof, **KW)
    assert c.shape == (0, 5, N_ENTRY) and r.shape == (0, 5, N_ENTRY, PER_ROAD)
    # fewer rows kept per road: a prefix; another table: other rows, the same cars
    c, r = d.demand_rows(SEED, IDS, ticks, tb, rw, 5, prof, **KW)
    assert np.array_equal(c, counts) and np.array_equal(r, rows[..., :5])
    c, r = d.demand_rows(SEED, IDS, ticks, tb, d.demand_row_table(None, 2, 3, 3), PER_ROAD, prof, **KW)
    assert np.array_equal(c, counts) and not np.array_equal(r, rows)


def test_rows_per_road_bounded_by_the_count_table():
    """the other branch of S = min(C - 2, n_cdf - 1): n_cdf = 4 lets an env have at most 3 cars in a tick, so at capacity
    14 the device keeps S = 3 rows per road - and loses nothing"""
    from gym_traffic import devrng as d
    tb = d.demand_tables([[0.9, 1.4]], n_entry=N_ENTRY, n_cdf=4)
    rw = d.demand_row_table([1.0, 2.0, 1.5], 1, 2, 3)
    S = min(14 - 2, tb.count_cdf.shape[2] - 1)
    assert S == 3
    ticks, ids = np.arange(0, 40), np.arange(7)
    counts, rows = d.demand_rows(5, ids, ticks, tb, rw, S, None, seg_ticks=3)
    assert counts.sum(axis=2).max() == 3 and counts.max() == 2
    seen = set()
    for i, t in enumerate(ticks):
        for e in ids:
            wc, wr = rule5(5, int(e), int(t), tb.count_cdf, tb.road_cdf, rw, 0, 3, 0, S)
            assert counts[i, e].tolist() == wc and rows[i, e].tolist() == wr, (t, e)
            seen.update(r for ej, c in enumerate(wc) for r in wr[ej][:c])
    assert seen == {0, 1, 2}


def test_row_table():
    from gym_traffic.devrng import demand_row_table
    t = demand_row_table([1, 0, 3], 2, 3, 3).astype(np.int64)
    assert t.shape == (2, 3, 3) and (t == [1 << 30, 1 << 30, MASK]).all()
    eq = demand_row_table(None, 1, 2, 3).astype(np.int64)
    assert eq.tolist() == [[[4294967296 // 3, 2 * 4294967296 // 3, MASK]] * 2]
    w = np.ones((2, 3, 4))
    w[1, 2] = [0, 0, 1, 1]
    t = demand_row_table(w, 2, 3, 4).astype(np.int64)
    assert t[0, 0].tolist() == [1 << 30, 1 << 31, 3 << 30, MASK] and t[1, 2].tolist() == [0, 0, 1 << 31, MASK]
    assert (np.diff(t, axis=-1) >= 0).all() and (t[..., -1] == MASK).all()
    assert demand_row_table([5.0], 1, 1, 1).tolist() == [[[MASK]]]
    assert demand_row_table(None, 1, 1, 64).shape == (1, 1, 64)
    for bad in (dict(row_weights=[1, -1], K=1, S=1, n_rows=2), dict(row_weights=[1, float("nan")], K=1, S=1, n_rows=2),
                dict(row_weights=[1, float("inf")], K=1, S=1, n_rows=2), dict(row_weights=[0, 0], K=1, S=1, n_rows=2),
                dict(row_weights=[[[1, 1], [0, 0]]], K=1, S=2, n_rows=2), dict(row_weights=[1, 1, 1], K=1, S=1, n_rows=2),
                dict(row_weights=np.ones((2, 1, 2)), K=1, S=2, n_rows=2), dict(row_weights=None, K=1, S=1, n_rows=65),
                dict(row_weights=np.ones(65), K=1, S=1, n_rows=65), dict(row_weights=None, K=1, S=1, n_rows=0)):
        with pytest.raises(ValueError):
            demand_row_table(**bad)


def test_header_declares_the_calls_and_the_abi_stays_13():
    from gym_traffic import _native
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"int\s+tfx_set_demand_mixed\s*\(\s*tfx_handle\s+h\s*,\s*const\s+tfx_demand\s*\*\s*dm\s*,\s*const\s+uint32_t\s*\*\s*"
                     r"row_cdf\s*,\s*int32_t\s+n_rows\s*\)\s*;", src)
    assert re.search(r"int\s+tfx_demand_rows\s*\(\s*tfx_handle\s+h\s*,\s*int32_t\s+tick0\s*,\s*int32_t\s+n_ticks\s*,\s*int32_t\s*\*\s*"
                     r"counts\s*,\s*uint8_t\s*\*\s*rows\s*,\s*void\s*\*\s*stream\s*\)\s*;", src)
    assert re.search(r"int\s+tfx_demand_rows_per_road\s*\(\s*tfx_handle\s+h\s*,\s*int32_t\s*\*\s*per_road\s*\)\s*;", src)
    assert re.search(r"#define\s+TFX_ABI_VERSION\s+13\b", src) and _native.ABI_VERSION == 13
    assert len(_native._PROTOS["tfx_set_demand_mixed"][1]) == 4 and len(_native._PROTOS["tfx_demand_rows"][1]) == 6
    assert len(_native._PROTOS["tfx_demand_rows_per_road"][1]) == 2
    assert "Rule 5" in text and "TAG_DROW = 0x44524F57" in text
    assert text.count("0x44524F57") >= 3          # rule 5 itself, and the tag lists of the rules before it
