"""Mixed car archetypes from the arrival streams on the device: the on-device Poisson stream of a heterogeneous engine
draws every car's archetype row (rule 1 of include/tfx.h, k_poisson<true>), mirrored on the host
(gym_traffic/devrng.py) and fed to the oracle car by car - bit-exact over every step path, agent steps with envs that
freeze, shards; the `regular` streams give row 0; TrafficVecEnv(archetypes=...) replays the reference's
`archetypes[random.randint(n)]` per env (host streams) or uses rule 1 (spawn='device')."""
import numpy as np
import pytest

from oracle.oracle import OracleEnv, live_mask
from test_gpu_archetypes import assert_cars_equal
from test_gpu_parity import same_bits

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from gym_traffic.core import TfxEngine  # noqa: E402
from gym_traffic.devrng import PoissonMirror, RegularMirror, cars_of  # noqa: E402

TAB8 = np.array([[11.11, 4, 3, 4, 13.89, 6, 2, 1], [8.0, 8, 1.5, 4, 10.0, 4, 2.5, 2],
                 [12.0, 3.5, 4, 2, 16.0, 7, 1.5, 1]], np.float32)          # v, l, a, delta, v0, b, T, s0
SEED = 0x00C0FFEE12345


def tab10(tab8):
    t = np.zeros((len(tab8), 10), np.float32)
    t[:, 1:9] = tab8
    return t


def oracle_cars(eng, cnt, rows):
    """per env (roads, rows) of a tick, as OracleEnv.step takes them"""
    per = [cars_of(cnt[k], rows[k], eng.entrypoints) for k in range(cnt.shape[0])]
    return [p[0] for p in per], [p[1] for p in per]


@pytest.fixture(params=["pertick", "pairs"])
def step_path(request, monkeypatch):
    monkeypatch.setenv("TFX_RESIDENT", "0")
    monkeypatch.setenv("TFX_PAIRS", "2" if request.param == "pairs" else "0")
    monkeypatch.setenv("TFX_TAIL", "2")
    monkeypatch.setenv("TFX_SPLIT", "2")
    yield request.param


@pytest.mark.parametrize("validate", [False, True])
@pytest.mark.parametrize("m,n,cap,cpt,calls", [
    (3, 2, 20, 1.4, (1, 3, 70, 2, 5)),            # 70 ticks > poisson_rows at this size (64): chunks are crossed
    (2, 1, 10, 6.0, (1, 2, 4, 9, 3, 1, 6))])     # S = 8: bursts of more than S cars on one road
def test_device_poisson_rows_vs_oracle(step_path, validate, m, n, cap, cpt, calls):
    E, L, off = 5, 150.0, 11
    eng = TfxEngine(m, n, L, cap, n_envs=E, planes=3, validate=validate, env_id_offset=off, archetypes=TAB8)
    assert eng.het
    orc = OracleEnv(m, n, L, cap, eng.dest, eng.phases, eng.nexts, n_envs=E, validate=validate)
    rng = np.random.RandomState(5)
    ph = rng.randint(2, size=(E, eng.I)).astype(np.int32)
    eng.reset(ph)
    orc.reset(ph)
    eng.set_poisson(cpt, seed=SEED)
    mirror = PoissonMirror(cpt, SEED, eng.n_entry, range(off, off + E), n_archetypes=len(TAB8), per_road=cap - 2)
    t, burst, hist = 0, 0, np.zeros(len(TAB8), np.int64)
    for k in calls:
        act = rng.randint(2, size=(E, eng.I)).astype(np.int32)
        eng.set_actions(act)
        eng.step(k)
        for _ in range(k):
            cnt, rows = mirror.next_tick()
            burst = max(burst, int(cnt.max()))
            roads, arch = oracle_cars(eng, cnt, rows)
            for a in arch:
                hist[a] += 1
            orc.step(act, roads, spawn_arch=arch, archetypes=tab10(TAB8))
            t += 1
        assert np.array_equal(eng.leading.cpu().numpy(), orc.leading), (k, t)
        assert np.array_equal(eng.lastcar.cpu().numpy(), orc.lastcar), (k, t)
        assert np.array_equal(eng.obs.cpu().numpy(), orc.obs), (k, t)
        assert_cars_equal(eng, orc, tab10(TAB8), "tick %d" % t)
    assert (hist > 0).all() and int(eng.cars_on_roads_flat().sum()) > 20
    if cap == 10:
        assert burst > cap - 2                       # a road was offered more cars than it can take in a tick
    if step_path == "pairs":
        assert eng.pair_ticks() > 0


def emulate_decisions(eng, orcs, mirror, act, n_ticks, tick0, off):
    """tfx_agent_step with the device stream, tick by tick on single-env oracles: an env that overflows stands still
    for the rest of the decision and its stream draws nothing (its seq does not move).  -> adone"""
    E = len(orcs)
    done = np.zeros(E, bool)
    for t in range(n_ticks):
        cnt, rows = mirror.next_tick(frozen={off + k for k in range(E) if done[k]})
        roads, arch = oracle_cars(eng, cnt, rows)
        for k, orc in enumerate(orcs):
            if done[k]:
                continue
            orc.steps[:] = tick0 + t
            _, _, d = orc.step(act[k], [roads[k]], spawn_arch=[arch[k]], archetypes=tab10(TAB8))
            done[k] = bool(d[0])
    return done


def test_agent_step_device_rows_with_frozen_envs(monkeypatch):
    monkeypatch.setenv("TFX_RESIDENT", "0")
    E, m, n, L, cap, cpt, off, N = 6, 2, 2, 120.0, 10, 2.2, 3, 8
    eng = TfxEngine(m, n, L, cap, n_envs=E, planes=3, env_id_offset=off, archetypes=TAB8)
    orcs = [OracleEnv(m, n, L, cap, eng.dest, eng.phases, eng.nexts) for _ in range(E)]
    ph = np.zeros((E, eng.I), np.int32)
    eng.reset(ph)
    for o in orcs:
        o.reset(ph[:1])
    eng.set_poisson(cpt, seed=SEED)
    mirror = PoissonMirror(cpt, SEED, eng.n_entry, range(off, off + E), n_archetypes=len(TAB8), per_road=cap - 2)
    rng = np.random.RandomState(2)
    froze = 0
    for dec in range(8):
        act = rng.randint(2, size=(E, eng.I)).astype(np.int32)
        eng.set_actions(act)
        tick0 = eng.tick
        _, _, adone = eng.agent_step(N, remi=False)
        want = emulate_decisions(eng, orcs, mirror, act, N, tick0, off)
        got = adone.cpu().numpy().astype(bool)
        assert np.array_equal(got, want), dec
        froze += int(want.sum())
        ld, lc = eng.leading.cpu().numpy(), eng.lastcar.cpu().numpy()
        x, v, _ = eng.planes_numpy()
        a = eng.arch.cpu().numpy()
        for k, o in enumerate(orcs):
            assert np.array_equal(ld[k], o.leading[0]) and np.array_equal(lc[k], o.lastcar[0]), (dec, k)
            live = live_mask(ld[k], lc[k], cap)
            assert same_bits(x[k][live], o.x[0][live]) and same_bits(v[k][live], o.v[0][live]), (dec, k)
            assert np.array_equal(a[k][live], o.arch_plane(0, tab10(TAB8))[live]), (dec, k)
    assert froze > 0                                  # envs overflowed mid-decision and froze


def test_sharded_env_equals_env_of_batch(step_path):
    E, m, n, L, cap, cpt, g = 6, 3, 3, 150.0, 20, 2.0, 4
    eng = TfxEngine(m, n, L, cap, n_envs=E, planes=3, archetypes=TAB8)
    solo = TfxEngine(m, n, L, cap, n_envs=1, planes=3, env_id_offset=g, archetypes=TAB8)
    ph = np.ones((E, eng.I), np.int32)
    for e in (eng, solo):
        e.reset(ph[:e.E])
        e.set_poisson(cpt, seed=SEED)
        e.set_actions(cycle_period=7)
    for k in (1, 6, 30, 3):
        eng.step(k)
        solo.step(k)
    assert torch.equal(solo.leading[0], eng.leading[g]) and torch.equal(solo.lastcar[0], eng.lastcar[g])
    assert torch.equal(solo.obs[0], eng.obs[g])
    live = live_mask(eng.leading[g].cpu().numpy(), eng.lastcar[g].cpu().numpy(), cap)
    assert np.array_equal(solo.arch[0].cpu().numpy()[live], eng.arch[g].cpu().numpy()[live])
    assert same_bits(solo.xv[0].cpu().numpy()[live], eng.xv[g].cpu().numpy()[live])
    assert len(set(eng.arch[g].cpu().numpy().ravel().tolist())) == len(TAB8)


def test_set_regular_on_heterogeneous_engine_gives_row_0():
    E, m, n, L, cap, cpt = 4, 3, 2, 150.0, 20, 1.6
    eng = TfxEngine(m, n, L, cap, n_envs=E, planes=3, archetypes=TAB8)
    orc = OracleEnv(m, n, L, cap, eng.dest, eng.phases, eng.nexts, n_envs=E)
    ph = np.zeros((E, eng.I), np.int32)
    eng.reset(ph)
    orc.reset(ph)
    eng.set_poisson(cpt, seed=1)                       # (its rows are unbound again by set_regular)
    eng.set_regular(cpt, seed=SEED)
    mirror = RegularMirror(cpt, SEED, eng.n_entry, range(E), n_archetypes=len(TAB8), per_road=cap - 2)
    rng = np.random.RandomState(8)
    for t in range(40):
        act = rng.randint(2, size=(E, eng.I)).astype(np.int32)
        eng.set_actions(act)
        eng.step(1)
        cnt, rows = mirror.next_tick()
        assert not rows.any()
        roads, arch = oracle_cars(eng, cnt, rows)
        orc.step(act, roads, spawn_arch=arch, archetypes=tab10(TAB8))
    assert_cars_equal(eng, orc, tab10(TAB8), "regular")
    ld, lc = eng.leading.cpu().numpy(), eng.lastcar.cpu().numpy()
    a = eng.arch.cpu().numpy()
    n_live = sum(int(live_mask(ld[k], lc[k], cap).sum()) for k in range(E))
    assert n_live > 30 and all(not a[k][live_mask(ld[k], lc[k], cap)].any() for k in range(E))


def test_vec_env_seeded_poisson_archetypes_vs_oracle_and_golden(golden_cache):
    """Env k of TrafficVecEnv(archetypes=tab, spawn='poisson', seed=s) draws what a reference env seeded s + k draws
    (SpawnSchedule on its RandomState, a table row per car); on the captured three-archetype run its integers are the
    reference's."""
    from gym_traffic.envs.vec_env import TrafficVecEnv
    from gym_traffic.spawner import SpawnSchedule
    g = golden_cache("g2x2_three_archetypes")
    sc = g.sc
    tab = g.archetypes
    E = 4
    vec = TrafficVecEnv(E, sc["m"], sc["n"], sc["L"], capacity=sc["C"], rate=sc["rate"], local_cars_per_sec=sc["lcps"],
                        spawn='poisson', seed=sc["seed"], archetypes=tab[:, 1:9])
    eng = vec.engine
    assert eng.het and eng.layout == "transposed"
    cps = sc["lcps"] * sc["m"] * 4
    sched = [SpawnSchedule(np.random.RandomState(sc["seed"] + k), True, eng.entrypoints, lambda: (cps, sc["rate"]),
                           n_archetypes=len(tab)) for k in range(E)]
    orc = OracleEnv(sc["m"], sc["n"], sc["L"], sc["C"], eng.dest, eng.phases, eng.nexts, n_envs=E, rate=sc["rate"])
    ph = np.tile(g["init_phase"][None], (E, 1)).astype(np.int32)
    vec.reset(ph)
    orc.reset(ph)
    t = 0
    for n_ticks in (1,) * 120 + (20, 3):
        act = np.tile(g["actions"][t][None], (E, 1)).astype(np.int32)
        vec.step(torch.as_tensor(act, device=eng.device), n_ticks=n_ticks)
        for _ in range(n_ticks):
            roads = [s.next_tick() for s in sched]
            orc.step(act, roads, spawn_arch=[s.rows for s in sched], archetypes=tab)
            t += 1
        assert np.array_equal(eng.leading.cpu().numpy(), orc.leading), t
        assert np.array_equal(eng.lastcar.cpu().numpy(), orc.lastcar), t
        assert np.array_equal(eng.obs.cpu().numpy(), orc.obs), t
        if t <= 120:
            assert np.array_equal(eng.leading[0].cpu().numpy(), g["leading"][t]), t
            assert np.array_equal(eng.lastcar[0].cpu().numpy(), g["lastcar"][t]), t
            assert np.array_equal(eng.obs[0].cpu().numpy(), g["obs"][t]), t
    assert_cars_equal(eng, orc, tab, "vec poisson")


@pytest.mark.parametrize("validate", [False, True])
def test_vec_env_archetypes_agent_step_and_reset_done(validate):
    """agent_step (host streams with rows bound per decision) and reset_done keep working with a table."""
    from gym_traffic.envs.vec_env import TrafficVecEnv
    from gym_traffic.spawner import SpawnSchedule
    E, m, n, L, cap, lcps, seed = 3, 2, 2, 200.0, 30, 0.15, 40
    vec = TrafficVecEnv(E, m, n, L, capacity=cap, local_cars_per_sec=lcps, spawn='poisson', seed=seed,
                        validate=validate, archetypes=TAB8)
    eng = vec.engine
    sched = [SpawnSchedule(np.random.RandomState(seed + k), True, eng.entrypoints, lambda: (lcps * m * 4, 0.5),
                           n_archetypes=len(TAB8)) for k in range(E)]
    orc = OracleEnv(m, n, L, cap, eng.dest, eng.phases, eng.nexts, n_envs=E, validate=validate)
    ph = np.zeros((E, eng.I), np.int32)
    vec.reset(ph)
    orc.reset(ph)
    for dec in range(4):
        act = np.full((E, eng.I), dec & 1, np.int32)
        _, _, adone = vec.agent_step(torch.as_tensor(act, device=eng.device), n_ticks=6, remi=True)
        assert not adone.any()
        for _ in range(6):
            roads = [s.next_tick() for s in sched]
            orc.step(act, roads, spawn_arch=[s.rows for s in sched], archetypes=tab10(TAB8))
        orc.remi_reward()                              # (what the fused decision ends with, remi=True)
        assert_cars_equal(eng, orc, tab10(TAB8), "decision %d" % dec)
    mask = torch.tensor([0, 1, 0], dtype=torch.uint8, device=eng.device)
    vec.reset_done(mask, phase_init=ph)
    assert int(eng.cars_on_roads_flat()[1].sum()) == 0 and int(eng.cars_on_roads_flat()[0].sum()) > 0
    vec.step(torch.as_tensor(ph, device=eng.device), n_ticks=10)
    assert int(eng.cars_on_roads_flat()[1].sum()) > 0


def test_vec_env_device_archetypes_at_batch():
    """spawn='device' at 1024 envs: the rows of the cars made are uniform over the table, and sampled envs are the
    oracle fed the host mirror of rule 1."""
    from gym_traffic.envs.vec_env import TrafficVecEnv
    E, m, n, L, cap, lcps, seed, T = 1024, 2, 2, 400.0, 24, 0.5, 99, 3
    vec = TrafficVecEnv(E, m, n, L, capacity=cap, local_cars_per_sec=lcps, spawn='device', seed=seed, archetypes=TAB8)
    eng = vec.engine
    ph = np.zeros((E, eng.I), np.int32)
    vec.reset(ph)
    act = torch.zeros((E, eng.I), dtype=torch.int32, device=eng.device)
    vec.step(act, n_ticks=T)                          # (no car reaches the end of a 400 m road in 3 ticks)
    ld, lc = eng.leading.cpu().numpy(), eng.lastcar.cpu().numpy()
    a = eng.arch.cpu().numpy()
    hist = np.zeros(len(TAB8), np.int64)
    for k in range(E):
        hist += np.bincount(a[k][live_mask(ld[k], lc[k], cap)].astype(np.int64), minlength=len(TAB8))
    total = int(hist.sum())
    cpt = lcps * m * 4 * 0.5
    mirror = PoissonMirror(cpt, seed, eng.n_entry, range(E))
    made = sum(int(mirror.next_tick().sum()) for _ in range(T))
    assert total == made and total > 2000            # every car made is on the map
    p = 1.0 / len(TAB8)
    assert (np.abs(hist - total * p) < 5 * np.sqrt(total * p * (1 - p))).all(), hist
    sample = [0, 517, 1023]
    mir = PoissonMirror(cpt, seed, eng.n_entry, sample, n_archetypes=len(TAB8), per_road=cap - 2)
    orc = OracleEnv(m, n, L, cap, eng.dest, eng.phases, eng.nexts, n_envs=len(sample))
    orc.reset(ph[:len(sample)])
    for _ in range(T):
        cnt, rows = mir.next_tick()
        roads, arch = oracle_cars(eng, cnt, rows)
        orc.step(np.zeros((len(sample), eng.I), np.int32), roads, spawn_arch=arch, archetypes=tab10(TAB8))
    x, v, _ = eng.planes_numpy()
    for i, k in enumerate(sample):
        assert np.array_equal(ld[k], orc.leading[i]) and np.array_equal(lc[k], orc.lastcar[i])
        live = live_mask(ld[k], lc[k], cap)
        assert same_bits(x[k][live], orc.x[i][live]) and same_bits(v[k][live], orc.v[i][live])
        assert np.array_equal(a[k][live], orc.arch_plane(i, tab10(TAB8))[live])
