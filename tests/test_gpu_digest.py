"""tfx_state_digest on the device (include/tfx.h, csrc/tfx_digest.hpp) against its definition in NumPy (devrng.state_digest)
applied to the engine's own ring planes and bound buffers - env and road words bit for bit, for every set of parts - on
synthetic states through the ring import, on driven states on every forced step path (and against the CPU oracle's run of
the same scenario), between tfx_move_cars and the advance, on both layouts fed the same inputs, plus: the selection (lists,
arrays, device tensors, repeats, ids outside the batch, road masks), more items than wavefronts, the call writes nothing,
what clone_envs / snapshot / restore / pack_envs / unpack_envs claim checked by TrafficVecEnv.same_state, argument errors
as codes, and tools/batch_selfcheck.py and tools/digest_demo.py at small sizes."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_gpu_clone import ARCH, Inputs, assert_env_equal, drive, make, snapshot
from test_gpu_measures import DRIVEN, SEQUENCE, run_scenario, same_snapshot
from test_measures_host import E_DRIVEN, GRID, scenario, oracle_driven
from test_gpu_ends import load_random

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from gym_traffic import _native as nat  # noqa: E402
from gym_traffic.devrng import state_digest  # noqa: E402

CARS, ROWS, SPAWN, RING, LIGHTS, OBS = (nat.DIGEST_CARS, nat.DIGEST_ROWS, nat.DIGEST_SPAWN, nat.DIGEST_RING,
                                        nat.DIGEST_LIGHTS, nat.DIGEST_OBS)
STATE = CARS | ROWS | RING | LIGHTS | OBS
SENTINEL = 0x5A5A5A5A5A5A5A5A


def part_sets(eng):
    """every walk of the kernel: (x, v) alone, with the B word, the B word alone (with and without a side plane to read),
    the ring words alone, no road part at all, and the named sets"""
    sets = [CARS, CARS | ROWS, ROWS, RING, CARS | RING, LIGHTS, OBS, LIGHTS | OBS, STATE, eng.digest_parts()]
    if eng.P == 3:
        sets += [SPAWN, CARS | SPAWN, ROWS | SPAWN, STATE | SPAWN]
    return sets


def model_of(eng, parts, ids=None, mask=None):
    """the definition applied to the image tfx_export_ring produces right now, and to the bound buffers"""
    x, v, w = eng.planes_numpy()
    arch = eng.arch.cpu().numpy() if eng.het else None
    ids, mask = [t.cpu().numpy() if torch.is_tensor(t) else t for t in (ids, mask)]
    return state_digest(x, v, w if eng.P == 3 else None, arch, eng.leading.cpu().numpy(), eng.lastcar.cpu().numpy(), eng.C,
                        parts, ids, mask, obs=eng.obs.cpu().numpy(), rewards=eng.rewards.cpu().numpy(),
                        waiting=eng.waiting.cpu().numpy(), passed_dst=eng.passed_dst.cpu().numpy(),
                        done_tick=eng.done_tick.cpu().numpy(), I=eng.I, r=eng.r)


def bits(t):
    torch.cuda.synchronize()
    return t.cpu().numpy().copy()


def check(eng, where, ids=None, mask=None, sets=None):
    """device == definition for every set of parts, as int64 views; -> {parts: (env, road)} of the device"""
    out = {}
    for parts in (part_sets(eng) if sets is None else sets):
        env, road = eng.state_digest(ids, parts=parts, roads=mask, per_road=True)
        env, road = bits(env), bits(road)
        alone = bits(eng.state_digest(ids, parts=parts, roads=mask))             # without the road words: the same env words
        want_env, want_road = [a.view(np.int64) for a in model_of(eng, parts, ids, mask)]
        assert env.dtype == np.int64 and env.shape == want_env.shape and road.shape == want_road.shape, (where, parts)
        if road.tobytes() != want_road.tobytes():
            raise AssertionError((where, parts, "road", np.argwhere(road != want_road)[:5].tolist()))
        if env.tobytes() != want_env.tobytes():
            raise AssertionError((where, parts, "env", np.flatnonzero(env != want_env)[:5].tolist()))
        assert alone.tobytes() == env.tobytes(), (where, parts, "env words without road words")
        if not parts & (CARS | ROWS | SPAWN | RING):
            assert not road.any(), (where, parts)
        out[parts] = (env, road)
    return out


# ---- 1. synthetic states through the ring import: the geometry -------------------------------------------------------------
@pytest.mark.parametrize("path,kind", [("pertick", "plain"), ("pertick", "validate"), ("pertick", "het"),
                                       ("ring", "plain"), ("ring", "validate")])
@pytest.mark.parametrize("capacity", [14, 66])
@pytest.mark.parametrize("m,n", [(3, 3), (4, 4)])        # 48 roads: one partial tile; 80: a full tile and 16 lanes of a second
def test_synthetic_states(path, kind, capacity, m, n):
    eng = make(path, 5, kind, m=m, n=n, capacity=capacity)
    assert eng.R == {3: 48, 4: 80}[m]
    count, ld, lc, arch = load_random(eng, 3)
    counts = set(count.ravel().tolist())
    assert {0, capacity - 2} <= counts and (ld > lc).any()                     # empty, full and wrapped rings
    assert any(c > 8 for c in counts)                                          # more than one block of the walk
    # counters and lights that are not a reset's zeros
    rng = np.random.RandomState(9)
    eng.obs.copy_(torch.as_tensor(rng.randint(0, 50, size=tuple(eng.obs.shape)).astype(np.int32)))
    eng.waiting.copy_(torch.as_tensor(rng.randint(0, 9, size=tuple(eng.waiting.shape)).astype(np.int32)))
    eng.passed_dst.copy_(torch.as_tensor(rng.randint(0, 256, size=tuple(eng.passed_dst.shape)).astype(np.uint8)))
    eng.rewards.copy_(torch.as_tensor(rng.uniform(-3, 3, size=tuple(eng.rewards.shape)).astype(np.float32)))
    eng.rewards[0, 0] = -0.0
    eng.done_tick.copy_(torch.as_tensor(np.array([0, 7, 0, 2 ** 31 - 5, 1], np.int32)))
    d = check(eng, (path, kind, capacity, m))
    env, road = d[eng.digest_parts()]
    assert len(set(env.tolist())) == eng.E and len(set(road.ravel().tolist())) > eng.E * eng.R // 2
    # ROWS adds the B term of every car - of zeros where a single-archetype car's row is 0 - so the words differ from CARS'
    assert (d[CARS | ROWS][0] != d[CARS][0]).all()
    if kind == "het":
        assert len(set(arch.ravel().tolist())) == len(ARCH)                    # every row of the table is on the roads
    if eng.P == 3:
        assert (d[SPAWN][0] != 0).all() and (d[CARS | SPAWN][0] != d[CARS][0]).all()


# ---- 2. driven states on every forced path --------------------------------------------------------------------------------
@pytest.mark.parametrize("path", DRIVEN)
def test_driven_states(path):
    eng = make(path, E_DRIVEN)
    run_scenario(eng)
    if path.startswith("pairs"):
        # the run ended on a two-tick pass: columns that start a row or two down are really read
        assert eng.pair_ticks() > 0 and eng.head_rows().any()
    if path.endswith("resident"):
        assert eng.fused_ticks()[0] > 0
    s = oracle_driven()
    d = check(eng, path)
    # HIP equals the oracle bit for bit, so its digests are those of the oracle's state
    want = state_digest(s["x"], s["v"], None, None, s["leading"], s["lastcar"], eng.C, CARS | RING)
    got = d[CARS | RING]
    assert got[0].tobytes() == want[0].view(np.int64).tobytes() and got[1].tobytes() == want[1].view(np.int64).tobytes()
    check(eng, (path, "chosen"), ids=[4, 1, 4], sets=[STATE, CARS])


@pytest.mark.parametrize("path,kind", [("pertick", "validate"), ("ring", "validate"), ("pairs_tail", "het")])
def test_between_move_and_advance(path, kind):
    """tick by tick: the image tfx_export_ring gives between tfx_move_cars and tfx_advance_finished_cars is hashed too;
    heterogeneous cars after two-tick passes that left head rows"""
    eng = make(path, E_DRIVEN, kind)
    if kind == "het":
        eng.reset(np.zeros((eng.E, eng.I), np.int32))
        inp = Inputs(eng, 6)
        for c in [("step", 8)] * 4 + [("step", 6)]:
            drive(eng, inp, c)
        assert eng.head_rows().any()
        d = check(eng, (path, kind))
        assert d[CARS | ROWS][0].tobytes() != d[CARS][0].tobytes()
        return
    run_scenario(eng)
    act, cnt = scenario(eng.I, eng.n_entry, seed=77)[0]
    for t in range(3):
        eng.set_actions(act)
        eng.set_spawns(counts=cnt[0])
        eng.move_cars()
        check(eng, ("after move_cars", t), sets=[STATE | SPAWN, CARS, SPAWN])
        check(eng, ("after move_cars, chosen", t), ids=[5, 0, 2], mask=np.arange(eng.R) % 3 != 0, sets=[STATE | SPAWN])
        eng.advance_finished_cars()
        check(eng, ("after the advance", t), sets=[STATE | SPAWN])


@pytest.mark.parametrize("path", ["resident", "pairs_tail", "pairs_split", "pairs_nograph", "pertick", "ring"])
def test_twin_that_never_asks(path):
    """An engine asked between every call of a mixed step / agent_step sequence (the agent steps replay their captured
    graph where graphs are on, run eagerly on pairs_nograph) stays bit-identical to one that never is - a decision graph
    captured before a digest call replays to the same bits - and after every call the device equals the definition."""
    E = E_DRIVEN
    eng, ref = make(path, E), make(path, E)
    rng = np.random.RandomState(31)
    for e_ in (eng, ref):
        e_.reset(np.zeros((E, eng.I), np.int32))
    for kind, n in SEQUENCE:
        act = rng.randint(2, size=(E, eng.I)).astype(np.int32)
        cnt = ((rng.rand(n, E, eng.n_entry) < 0.15) * rng.randint(1, 3, size=(n, E, eng.n_entry))).astype(np.int32)
        eng.state_digest()
        eng.state_digest([1, 4], parts=CARS, per_road=True)
        for e_ in (eng, ref):
            e_.set_actions(act)
            e_.set_spawns(counts=cnt, per_tick=True)
            (e_.agent_step if kind == "agent" else e_.step)(n)
        check(eng, (path, kind, n), sets=[STATE, CARS])
    sa, sb = snapshot(eng), snapshot(ref)
    for k in range(E):
        assert_env_equal(sa, k, sb, k, path)
    assert np.array_equal(eng.head_rows(), ref.head_rows())
    assert torch.equal(eng.state_digest(), ref.state_digest())                # two handles, the same bits, the same digests
    assert len(set(bits(eng.state_digest()).tolist())) == E


# ---- 3. layout independence ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["plain", "validate"])
def test_both_layouts_agree(kind):
    """a ring handle and transposed handles on their step paths, fed the same inputs, have equal digests"""
    engines = [make(p, E_DRIVEN, kind) for p in ("ring", "pertick", "pairs_tail") + (("resident",) if kind == "plain" else ())]
    for eng in engines:
        run_scenario(eng)
    assert engines[2].head_rows().any()
    parts = engines[0].digest_parts()
    assert bool(parts & SPAWN) == (kind == "validate")
    got = [[bits(t) for t in eng.state_digest(parts=parts, per_road=True)] for eng in engines]
    for other in got[1:]:
        assert other[0].tobytes() == got[0][0].tobytes() and other[1].tobytes() == got[0][1].tobytes()
    assert len(set(got[0][0].tolist())) == E_DRIVEN


# ---- 4. selection -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path,kind", [("pertick", "het"), ("ring", "validate")])
def test_selection(path, kind):
    E = 6
    eng = make(path, E, kind, m=4, n=4)
    count = load_random(eng, 7, empty_envs=(1, 4))[0]
    assert not count[1].any() and not count[4].any() and count[0].any()
    parts = [eng.digest_parts(), CARS]
    ids = [3, 0, 3, -1, 5, E, 1, 3]
    as_list = check(eng, "a list", ids=ids, sets=parts)
    as_array = check(eng, "an array", ids=np.array(ids, np.int64), sets=parts)
    as_tensor = check(eng, "a device tensor", ids=torch.as_tensor(ids, dtype=torch.int32).to(eng.device), sets=parts)
    everyone = check(eng, "every env", sets=parts)
    for p in parts:
        env, road = as_list[p]
        for other in (as_array, as_tensor):
            assert other[p][0].tobytes() == env.tobytes() and other[p][1].tobytes() == road.tobytes()
        assert env[0] == env[2] == env[7] == everyone[p][0][3] != 0 and np.array_equal(road[0], road[2])   # repeats
        assert env[3] == 0 and env[5] == 0 and not road[3].any() and not road[5].any()                    # -1 and E: 0
        assert env[1] == everyone[p][0][0] and env[4] == everyone[p][0][5] and env[6] == everyone[p][0][1]
    one = check(eng, "one env", ids=[5], sets=parts)
    assert one[CARS][0][0] == everyone[CARS][0][5]
    assert not check(eng, "ids outside the batch only", ids=[-1, E, 99], sets=parts)[CARS][0].any()
    # road masks
    mask = (np.arange(eng.R) % 5 == 1).astype(np.uint8)
    d = check(eng, "a mask", ids=ids, mask=mask, sets=parts)[CARS]
    assert not d[1][:, mask == 0].any() and d[1][0][mask != 0].all() and d[0][0] != as_list[CARS][0][0]
    d0 = check(eng, "the all-zero mask", mask=np.zeros(eng.R, np.uint8), sets=[CARS, STATE])
    assert not d0[CARS][0].any() and not d0[CARS][1].any() and d0[STATE][0].all()       # no road enters; the words still do
    d2 = eng.state_digest(ids, parts=CARS, roads=torch.as_tensor(mask != 0).to(eng.device), per_road=True)
    assert bits(d2[0]).tobytes() == d[0].tobytes() and bits(d2[1]).tobytes() == d[1].tobytes()
    # the caller's tensors
    env = torch.full((3,), 7, dtype=torch.int64, device=eng.device)
    road = torch.full((3, eng.R), 7, dtype=torch.int64, device=eng.device)
    got = eng.state_digest([5, -1, 0], parts=CARS, per_road=True, out=(env, road))
    assert got[0] is env and got[1] is road
    assert bits(env).tolist() == [everyone[CARS][0][5], 0, everyone[CARS][0][0]] and not bits(road)[1].any()
    assert eng.state_digest([5, -1, 0], parts=CARS, out=env) is env
    for bad in (dict(envs=[]), dict(roads=np.ones(eng.R + 1, np.uint8)), dict(parts=0), dict(parts=64),
                dict(out=torch.zeros(2, dtype=torch.int64, device=eng.device)), dict(out=env.to(torch.int32))):
        with pytest.raises(ValueError):
            eng.state_digest(**bad)


# ---- 5. more items than wavefronts -------------------------------------------------------------------------------------
def engine_under(env, E, **cfg):
    """a handle created under TFX_RESIDENT=0 and the switches of `env` alone - every other TFX_* switch is taken out of the
    environment while the handle reads it (tests/test_gpu_stride_rounds.py:make_engine's way)"""
    from gym_traffic.core import TfxEngine
    env = dict(env, TFX_RESIDENT="0")
    keep = {k: v for k, v in os.environ.items() if k.startswith("TFX_") and k != "TFX_LIB"}
    for k in keep:
        del os.environ[k]
    os.environ.update(env)
    try:
        eng = TfxEngine(n_envs=E, **cfg)
    finally:
        for k in env:
            os.environ.pop(k, None)
        os.environ.update(keep)
    return eng


@pytest.mark.parametrize("layout", ["transposed", "ring"])
def test_stride_rounds(layout):
    """7 envs of the 4x4 grid are 14 (env, tile) items (80 roads: a full tile and 16 lanes of a second).  The uncapped
    launch has a wavefront for every item (4 workgroups); TFX_GRID_CAP=1 and TFX_MEASURE_GRID=1 leave one workgroup - four
    wavefronts, four rounds, the last one with two at work, every env's tiles arriving in different rounds.  Envs 2 and 5
    hold no car.  The sums do not depend on the order: the bits are those of the uncapped launch."""
    E = 7
    cfg = dict(m=4, n=4, length=120.0, capacity=14, rate=0.5, layout=layout, planes=3, validate=True)
    free = engine_under({}, E, **cfg)
    capped = [engine_under({"TFX_GRID_CAP": "1"}, E, **cfg), engine_under({"TFX_MEASURE_GRID": "1"}, E, **cfg)]
    out = []
    for eng in [free] + capped:
        count = load_random(eng, 5, empty_envs=(2, 5))[0]
        assert not count[2].any() and not count[5].any() and count[0].any() and count[6].any()
        assert eng.digest_launch(E) == ((4, 16) if eng is free else (1, 4))
        assert eng.digest_launch(2) == (1, 4)
        sets = [eng.digest_parts(), CARS, SPAWN, RING]
        out.append([check(eng, (layout, "all"), sets=sets), check(eng, (layout, "chosen"), ids=[6, 0, 3, 3, 1, 6, 4, 0, 2], sets=sets)])
    assert free.R == 80 and E * ((free.R + 63) // 64) == 14 > capped[0].digest_launch(E)[1]
    for other in out[1:]:
        for a, b in zip(out[0], other):
            assert all(a[p][0].tobytes() == b[p][0].tobytes() and a[p][1].tobytes() == b[p][1].tobytes() for p in a)


# ---- 6. read-only ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path,kind", [("pairs_tail", "plain"), ("pertick", "validate"), ("pairs_tail", "het"), ("ring", "plain")])
def test_the_call_writes_nothing(path, kind):
    eng = make(path, E_DRIVEN, kind)
    if kind == "het":
        eng.reset(np.zeros((eng.E, eng.I), np.int32))
        inp = Inputs(eng, 6)
        for c in [("step", 8)] * 4 + [("step", 6)]:
            drive(eng, inp, c)
    else:
        run_scenario(eng)
    before = snapshot(eng)
    hb = eng.head_rows().copy()
    tick = C.c_int32()
    nat.check(eng.lib.tfx_get_tick(eng.h, C.byref(tick)))
    eng.state_digest()
    eng.state_digest([2, 2, 5], parts=CARS | RING, per_road=True)
    same_snapshot(before, snapshot(eng))
    assert np.array_equal(hb, eng.head_rows())
    now = C.c_int32()
    nat.check(eng.lib.tfx_get_tick(eng.h, C.byref(now)))
    assert now.value == tick.value
    check(eng, (path, kind), sets=[eng.digest_parts()])


def test_the_launch_is_not_counted_by_fail_after():
    eng = make("pertick", 3)
    load_random(eng, 2)
    lib = nat.lib()
    nat.check(lib.tfx_debug_fail_after(eng.h, 1))                            # the NEXT counted launch fails
    for _ in range(3):
        check(eng, "under fail_after", sets=[STATE])                       # (tfx_export_ring is not counted either)
    with pytest.raises(nat.TfxError, match="injected"):
        eng.clone_envs(np.array([-1, 0, -1], np.int32))
    nat.check(lib.tfx_debug_fail_after(eng.h, 0))
    check(eng, "after the injected failure", sets=[STATE])


# ---- 7. what the state calls claim ------------------------------------------------------------------------------------
HET_ROWS = np.array([[11.11, 4.0, 3.0, 4.0, 13.89, 6.0, 2.0, 1.0], [9.0, 7.5, 2.0, 3.0, 11.0, 5.0, 1.5, 2.0]], np.float32)


def vec_env(kind, E=6, capacity=14, seed=3, cars_per_sec=0.3):
    from gym_traffic.envs.vec_env import TrafficVecEnv
    kw = dict(archetypes=HET_ROWS, spawn='device', local_cars_per_sec=cars_per_sec) if kind == "het" else \
        dict(spawn='periodic', spawn_period=5, validate=(kind == "validate"))
    return TrafficVecEnv(E, 3, 3, 120.0, capacity=capacity, seed=seed, **kw)


def run_decisions(venv, n, seed=4, ticks=5):
    eng = venv.engine
    rng = np.random.RandomState(seed)
    for _ in range(n):
        venv.agent_step(torch.as_tensor(rng.randint(2, size=(eng.E, eng.I)).astype(np.int32)).to(eng.device), n_ticks=ticks)


@pytest.mark.parametrize("kind", ["het", "validate", "plain"])
def test_vec_env_digest_and_clone(kind):
    venv = vec_env(kind)
    venv.reset()
    eng = venv.engine
    E = eng.E
    run_decisions(venv, 7)
    # the named sets
    rows = ROWS if kind == "het" else 0
    assert venv.digest_parts('cars') == CARS | rows and venv.digest_parts('state') == CARS | rows | RING | LIGHTS | OBS
    assert venv.digest_parts('all') == venv.digest_parts('state') | (SPAWN if kind != "plain" else 0)
    assert venv.digest_parts(CARS | RING) == CARS | RING
    with pytest.raises(ValueError):
        venv.digest_parts('everything')
    for name in ('cars', 'state', 'all'):
        want = model_of(eng, venv.digest_parts(name))
        env, road = venv.digest(parts=name, per_road=True)
        assert bits(env).tobytes() == want[0].view(np.int64).tobytes() and bits(road).tobytes() == want[1].view(np.int64).tobytes()
        assert env.shape == (E,) and road.shape == (E, eng.R) and env.dtype == torch.int64
    d = bits(venv.digest())
    assert len(set(d.tolist())) == E                                         # different actions: different states
    assert venv.same_state(np.arange(E)).all()
    assert bits(venv.same_state([1, 0, -1, 3, E, 4])).tolist() == [False, False, False, True, False, False]
    # an arterial as the mask
    mask = venv.arterial(1, 0)
    env, road = eng.state_digest([0, 3], parts=CARS, roads=mask, per_road=True)
    want = model_of(eng, CARS, [0, 3], mask)
    assert bits(env).tobytes() == want[0].view(np.int64).tobytes() and bits(road).tobytes() == want[1].view(np.int64).tobytes()
    assert bits(road)[:, mask != 0].all() and not bits(road)[:, mask == 0].any()
    # a clone in place: afterwards env e IS env src[e], in every part
    src = np.array([-1, -1, -1, 0, 1, -1], np.int32)
    assert bits(venv.same_state(src, parts='all')).tolist() == [False] * E
    idx = venv.clone_envs(src)
    assert eng.clone_skipped() == 0
    same = venv.same_state(idx, parts='all')                                 # the device tensor clone_envs returned
    assert same.dtype == torch.bool and bits(same).tolist() == [False, False, False, True, True, False]
    # one different action, then enough ticks to move a car: that env alone parts from its source
    act = torch.as_tensor(np.random.RandomState(8).randint(2, size=(E, eng.I)).astype(np.int32)).to(eng.device)
    act[3], act[4] = act[0], act[1]
    venv.agent_step(act, n_ticks=4)                                          # (a device arrival stream travelled with the clone)
    assert bits(venv.same_state(src, parts='all')).tolist() == [False, False, False, True, True, False]
    act[4] = 1 - act[1]
    venv.agent_step(act, n_ticks=8)
    assert bits(venv.same_state(src, parts='cars')).tolist() == [False, False, False, True, False, False]
    assert bits(venv.same_state(src, parts='state')).tolist() == [False, False, False, True, False, False]


@pytest.mark.parametrize("kind", ["validate", "het"])
def test_snapshot_restore_at_another_clock(kind):
    venv = vec_env(kind, cars_per_sec=0.15)
    venv.reset()
    eng = venv.engine
    E = eng.E
    run_decisions(venv, 6)
    every = torch.arange(E, dtype=torch.int32)
    snap = venv.snapshot()                                                   # a fresh handle: its clock stands at 0
    assert snap.engine.tick == 0 != eng.tick
    # Everything stored as a tick was rebased by the difference of the clocks.  'state' holds one such word: done_tick,
    # the stamp of an env that has overflowed (0 otherwise) - so 'state' is equal exactly where an env never overflowed
    calm = bits(eng.done_tick == 0)
    # (periodic arrivals: at most 6 cars a road in 30 ticks, a road holds 12 - no env can have overflowed)
    assert calm.all() if kind == "validate" else calm.any()
    assert np.array_equal(bits(venv.same_state(every, source=snap, parts='state')), calm)
    assert np.array_equal(bits(snap.same_state(every, source=venv, parts='state')), calm)
    assert venv.same_state(every, source=snap, parts=venv.digest_parts('state') & ~OBS).all()
    # ... and 'all' holds every car's spawn tick: different exactly where an env has a car
    has_cars = bits(eng.cars_on_roads_flat().sum(dim=1) > 0)
    assert (has_cars & calm).any()
    assert np.array_equal(bits(venv.same_state(every, source=snap, parts='all')), calm & ~has_cars)
    run_decisions(venv, 3, seed=11)
    assert not venv.same_state(every, source=snap, parts='state').any()
    venv.restore(snap)
    assert np.array_equal(bits(venv.same_state(every, source=snap, parts='state')), calm)
    assert venv.same_state(every, source=snap, parts=venv.digest_parts('state') & ~OBS).all()
    assert venv.same_state(every, source=snap, parts='cars').all()


def test_pack_unpack_into_another_batch():
    from gym_traffic.envs.vec_env import TrafficVecEnv
    venv = vec_env("validate")
    venv.reset()
    run_decisions(venv, 7)
    other = TrafficVecEnv(3, 3, 3, 120.0, capacity=20, spawn='periodic', spawn_period=3, validate=True, seed=9)
    other.reset()
    src = [4, -1, 1]
    assert not other.same_state(src, source=venv, parts='cars').any()
    other.unpack_envs([2, 0], venv.pack_envs([1, 4]))
    assert other.engine.put_lost() == 0
    assert bits(other.same_state(src, source=venv, parts='cars')).tolist() == [True, False, True]
    # the ring position travelled too (a ring index of both capacities); the lights and counters are torch index writes
    assert bits(other.same_state(src, source=venv, parts=CARS | RING | LIGHTS)).tolist() == [True, False, True]


# ---- 8. errors ---------------------------------------------------------------------------------------------------------
def test_errors_are_codes_and_the_handle_stays_usable():
    lib = nat.lib()
    eng = make("pertick", 3)                                                 # planes == 2: no spawn ticks
    run_scenario(eng, 6)
    E, R = eng.E, eng.R
    env = torch.full((E + 2,), SENTINEL, dtype=torch.int64, device=eng.device)
    road = torch.full((E + 2, R), SENTINEL, dtype=torch.int64, device=eng.device)
    ids = torch.zeros((E,), dtype=torch.int32, device=eng.device)
    ep, rp, ip = C.c_void_p(env.data_ptr()), C.c_void_p(road.data_ptr()), C.c_void_p(ids.data_ptr())
    st = eng._stream()

    def untouched():
        torch.cuda.synchronize()
        return bool((env == SENTINEL).all()) and bool((road == SENTINEL).all())
    # before tfx_bind_buffers
    h = C.c_void_p()
    nat.check(lib.tfx_create(C.byref(eng.cfg), C.byref(h)))
    assert lib.tfx_state_digest(h, None, E, None, CARS, ep, rp, 0, st) == nat.ESTATE
    assert b"tfx_bind_buffers" in lib.tfx_last_error()
    nat.check(lib.tfx_destroy(h))
    assert untouched()
    too_many = (2 ** 31) // R + 1
    for args, msg in (((None, E, None, CARS, None, rp, 0), b"env_digest is null"), ((None, 0, None, CARS, ep, rp, 0), b"n_sel 0"),
                      ((None, -2, None, CARS, ep, rp, 0), b"n_sel -2"), ((None, E + 1, None, CARS, ep, rp, 0), b"env_ids is null"),
                      ((ip, too_many, None, CARS, ep, None, 0), b"do not fit int32"),
                      ((None, E, None, 0, ep, rp, 0), b"parts"), ((None, E, None, 64, ep, rp, 0), b"parts"),
                      ((None, E, None, CARS | 256, ep, rp, 0), b"parts"), ((None, E, None, -1, ep, rp, 0), b"parts"),
                      ((None, E, None, CARS | SPAWN, ep, rp, 0), b"planes == 2"),
                      ((None, E, None, CARS, ep, rp, 1), b"flags"), ((None, E, None, CARS, ep, rp, -1), b"flags")):
        assert lib.tfx_state_digest(eng.h, *args, st) == nat.EINVAL, msg
        assert msg in lib.tfx_last_error(), (msg, lib.tfx_last_error())
        assert untouched(), msg
    assert lib.tfx_state_digest(None, None, E, None, CARS, ep, rp, 0, st) == nat.EINVAL
    for bad in (0, -1, too_many):
        assert lib.tfx_digest_launch(eng.h, bad, None, None) == nat.EINVAL
    with pytest.raises(ValueError):
        eng.state_digest(parts=CARS | SPAWN)
    # a good call writes its n_sel words and road rows and nothing behind them
    assert lib.tfx_state_digest(eng.h, None, E, None, STATE, ep, rp, 0, st) == 0
    want = model_of(eng, STATE)
    assert bits(env)[:E].tobytes() == want[0].view(np.int64).tobytes() and bits(road)[:E].tobytes() == want[1].view(np.int64).tobytes()
    assert bool((env[E:] == SENTINEL).all()) and bool((road[E:] == SENTINEL).all())
    eng.step(3)
    check(eng, "stepped after the errors", sets=[STATE])


# ---- 9. the tools ------------------------------------------------------------------------------------------------------
def tool(name):
    tools = os.path.join(ROOT, "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    return __import__(name)


@pytest.mark.parametrize("layout", ["transposed", "ring"])
def test_batch_selfcheck_small(layout, capsys):
    """the workload self-check on the 4x4 config with 45 envs: 20 representatives, 25 envs that must repeat them"""
    bs = tool("batch_selfcheck")
    r = bs.selfcheck("cfg1", envs=45, ticks=37, layout=layout, threads=4)
    assert r["selfcheck"] == "ok" and r["envs"] == 45 and r["period"] == 20 and r["envs_differing"] == 0
    assert r["first_difference"] is None and r["oracle_cars_equal"] and r["oracle_digests_equal"]
    assert r["distinct_digests"] == 20 and r["cars"] > 45 * 80 * 10
    # an env that does not repeat its representative is found, with its first road
    env = torch.arange(45, dtype=torch.int64) % 20
    road = (torch.arange(45, dtype=torch.int64) % 20)[:, None].repeat(1, 80)
    assert bs.first_difference(env, road, 20) == (0, None)
    road[33, 17] += 1
    env[33] += 1
    env[41] += 1
    assert bs.first_difference(env, road, 20) == (2, (33, 17))
    assert bs.main(["--config", "cfg1", "--envs", "21", "--ticks", "12", "--layout", layout, "--no-oracle"]) == 0
    assert '"selfcheck": "ok"' in capsys.readouterr().out


def test_digest_demo_small(capsys):
    """two lights: four possible settings among six candidates, so every live env has duplicate branches"""
    dd = tool("digest_demo")
    r = dd.main(["--envs", "3", "--candidates", "6", "--horizon", "2", "--decisions", "4", "--ticks", "6", "--m", "1", "--n", "2",
                 "--length", "120", "--capacity", "14", "--cars-per-sec", "0.3", "--sample", "3"])
    assert r["branches"] == 18 and len(r["duplicates"]) == 4 and all(d >= 3 * 2 for d in r["duplicates"])
    assert r["pairs_checked"] == 12 and r["pairs_wrong"] == 0 and r["clones_verified"] == 4
    assert "duplicate branches per decision" in capsys.readouterr().out
