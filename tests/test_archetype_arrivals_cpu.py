"""Mixed car archetypes from the arrival streams, host side (no GPU): the batched replay of the reference's seeded
generators with the `randint(n_archetypes)` draw of every car (tfx_arrivals_replay_rows) against SpawnSchedule on a
legacy RandomState, and the host mirror of the on-device row rule (rule 1 of include/tfx.h, gym_traffic/devrng.py)."""
import numpy as np
import pytest

from gym_traffic.devrng import MASK, TAG_ARCH, PoissonMirror, RegularMirror, cars_of, philox4x32
from gym_traffic.spawner import ArrivalStreams, SpawnSchedule

ENTRY = np.array([0, 2, 5, 7, 8, 9, 14, 15, 20, 21])      # ten entry roads, columns in this order


def per_road(roads, rows, columns, S):
    """{column: rows of its cars in creation order (the first S)}"""
    out = {}
    for rd, a in zip(roads, rows):
        out.setdefault(columns[rd], []).append(a)
    return {c: v[:S] for c, v in out.items()}


@pytest.mark.parametrize("n_arch", [2, 3, 5])
@pytest.mark.parametrize("poisson,cpt", [(True, 0.4), (True, 3.7), (False, 0.3), (False, 2.6)])
def test_replay_rows_equals_spawn_schedule(n_arch, poisson, cpt):
    E, T, S = 5, 320, 4
    seeds = [100 + 7 * k for k in range(E)]
    columns = {int(rd): j for j, rd in enumerate(ENTRY)}
    ar = ArrivalStreams(seeds, poisson, ENTRY, columns, len(ENTRY), cpt, n_archetypes=n_arch, per_road=S)
    scheds = [SpawnSchedule(np.random.RandomState(s), poisson, ENTRY, lambda: (cpt, 1.0), n_archetypes=n_arch)
              for s in seeds]
    got_c, got_m, got_r = [], [], []
    for n in (1, 17, 100, 202):                       # calls of several lengths continue one stream
        c, m, r = ar.next_ticks(n)
        got_c.append(c.copy()), got_m.append(m.copy()), got_r.append(r.copy())
    counts, made, rows = np.concatenate(got_c), np.concatenate(got_m), np.concatenate(got_r)
    assert counts.shape[0] == T
    seen_rows = set()
    for k, s in enumerate(scheds):
        for t in range(T):
            roads = s.next_tick()
            assert made[t, k] == len(roads)
            want = np.zeros(len(ENTRY), np.int32)
            for rd in roads:
                want[columns[rd]] += 1
            assert np.array_equal(counts[t, k], want), (k, t)
            for col, v in per_road(roads, s.rows, columns, S).items():
                assert rows[t, k, col, :len(v)].tolist() == v, (k, t, col)
                seen_rows.update(v)
        # the stream has consumed exactly what the reference's RandomState consumed
        assert ar.random_state(k).randint(1 << 30, size=8).tolist() == s.rand.randint(1 << 30, size=8).tolist()
    if poisson:
        assert seen_rows == set(range(n_arch))
    else:
        assert seen_rows == {0}                       # the regular generator yields archetypes[0]


@pytest.mark.parametrize("poisson,cpt", [(True, 0.6), (True, 4.2), (False, 1.5)])
def test_replay_rows_single_archetype_is_the_plain_replay(poisson, cpt):
    E, T, S = 4, 300, 6
    seeds = [3, 4, 5, 6]
    columns = {int(rd): j for j, rd in enumerate(ENTRY)}
    a = ArrivalStreams(seeds, poisson, ENTRY, columns, len(ENTRY), cpt)
    b = ArrivalStreams(seeds, poisson, ENTRY, columns, len(ENTRY), cpt, n_archetypes=1, per_road=S)
    ca, ma = a.next_ticks(T)
    cb, mb, rb = b.next_ticks(T, counts=np.empty((T, E, len(ENTRY)), np.int32), made=np.empty((T, E), np.int32),
                              rows=np.full((T, E, len(ENTRY), S), 0xAB, np.uint8))
    assert np.array_equal(ca, cb) and np.array_equal(ma, mb)
    j = np.arange(S)[None, None, None, :]
    written = j < np.minimum(cb, S)[..., None]
    assert written.any() and (rb[written] == 0).all() and (rb[~written] == 0xAB).all()
    for k in range(E):
        assert np.array_equal(a.random_state(k).get_state()[1], b.random_state(k).get_state()[1])


def test_rows_need_per_road():
    with pytest.raises(ValueError):
        ArrivalStreams([1], True, ENTRY, {int(rd): j for j, rd in enumerate(ENTRY)}, len(ENTRY), 1.0, n_archetypes=3)
    with pytest.raises(ValueError):
        PoissonMirror(1.0, 1, 8, [0], n_archetypes=3)


def rule1(seed, g, ej, s, j, n):
    u = philox4x32((s + j) & MASK, g, TAG_ARCH, ej, seed & MASK, (seed >> 32) & MASK)[0]
    return (u * n) >> 32


def test_mirror_rows_follow_rule_1_and_carry_seq_across_ticks_and_frozen_envs():
    seed, n, S, n_entry = 0x5EED0000ABCD, 5, 3, 6
    envs = [4, 9, 10]
    m = PoissonMirror(2.5, seed, n_entry, envs, n_archetypes=n, per_road=S)
    plain = PoissonMirror(2.5, seed, n_entry, envs)
    seq = np.zeros((len(envs), n_entry), np.int64)
    for t in range(60):
        frozen = {9} if t % 4 == 1 else ()
        cnt, rows = m.next_tick(frozen=frozen)
        assert np.array_equal(cnt, plain.next_tick(frozen=frozen))      # the counts are the single-archetype stream's
        assert rows.shape == (len(envs), n_entry, S) and rows.dtype == np.uint8
        for r, g in enumerate(envs):
            if g in frozen:
                assert not cnt[r].any() and not rows[r].any()
            for ej in range(n_entry):
                c = int(cnt[r, ej])
                want = [rule1(seed, g, ej, int(seq[r, ej]), j, n) for j in range(min(c, S))]
                assert rows[r, ej, :len(want)].tolist() == want, (t, g, ej)
                assert not rows[r, ej, len(want):].any()
        seq += cnt
        assert np.array_equal(m.rows.seq, seq)                       # overflowing cars (past S) counted too
    assert seq.max() > S


def test_mirror_is_deterministic_and_rows_are_uniform():
    seed, n, S = 77, 3, 64
    envs = list(range(40))
    a = PoissonMirror(3.0, seed, 8, envs, n_archetypes=n, per_road=S)
    b = PoissonMirror(3.0, seed, 8, envs, n_archetypes=n, per_road=S)
    hist = np.zeros(n, np.int64)
    for _ in range(300):
        ca, ra = a.next_tick()
        cb, rb = b.next_tick()
        assert np.array_equal(ca, cb) and np.array_equal(ra, rb)
        j = np.arange(S)[None, None, :]
        live = j < ca[..., None]
        assert (ra[live] < n).all()
        hist += np.bincount(ra[live], minlength=n)
    total = int(hist.sum())
    assert total > 30000
    p = 1.0 / n
    sd = np.sqrt(total * p * (1 - p))
    assert (np.abs(hist - total * p) < 5 * sd).all(), hist


def test_regular_mirror_rows_are_row_0():
    m = RegularMirror(2.6, 5, 6, [0, 1], n_archetypes=4, per_road=5)
    for _ in range(20):
        cnt, rows = m.next_tick()
        assert cnt.sum() > 0 and not rows.any()
    assert np.array_equal(m.rows.seq.sum(axis=1), [60, 60])


def test_cars_of_groups_by_road_in_creation_order():
    cnt = np.array([2, 0, 3], np.int32)
    rows = np.array([[1, 2], [0, 0], [2, 1]], np.uint8)
    roads, arch = cars_of(cnt, rows, [10, 11, 12])
    assert roads == [10, 10, 12, 12, 12] and arch == [1, 2, 2, 1, 0]
