"""tfx_clone_envs on the device (include/tfx.h, csrc/tfx_clone.hpp): after a clone ANY sequence of calls gives the
clone the bits it would give its source under the same inputs.  Every case runs under both layouts and, where it
applies, on every forced step path (LDS-resident, tick by tick, two-tick passes with k_tail / with separate launches /
split over two streams / segmented, graph off), because what must be copied differs per path."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_parity import assert_same_state, oracle_like, same_bits
from test_gpu_fused import engine_with
from test_episodes_host import EpisodeModel

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from gym_traffic import _native as nat  # noqa: E402
from gym_traffic import devrng  # noqa: E402
from gym_traffic import workload as wl  # noqa: E402
from oracle.oracle import live_mask  # noqa: E402

PAIRS = {"TFX_RESIDENT": "0", "TFX_PAIRS": "2", "TFX_TAIL": "2", "TFX_SPLIT": "0", "TFX_TT_SEG": "0"}
PATHS = {
    "resident": {"TFX_RESIDENT": "1"},
    "pertick": {"TFX_RESIDENT": "0", "TFX_PAIRS": "0"},
    "pairs_tail": PAIRS,
    "pairs_launches": dict(PAIRS, TFX_TAIL="0"),
    "pairs_split": dict(PAIRS, TFX_SPLIT="2"),
    "pairs_seg": dict(PAIRS, TFX_TT_SEG="2", TFX_TT_SEGS="2"),
    "pairs_nograph": dict(PAIRS, TFX_GRAPH="0"),
    "ring": {"TFX_RESIDENT": "0"},
    "ring_resident": {"TFX_RESIDENT": "1"},
}
TRANSPOSED = ["resident", "pertick", "pairs_tail", "pairs_launches", "pairs_split", "pairs_seg", "pairs_nograph"]
HET_PATHS = ["pertick", "pairs_tail", "pairs_launches", "pairs_split"]     # (heterogeneous cars: never resident, no segments)
ARCH = np.array([[11.11, 4.0, 3.0, 4.0, 13.89, 6.0, 2.0, 1.0], [8.0, 7.5, 1.5, 3.0, 11.0, 4.0, 2.5, 2.0],
                 [13.0, 3.0, 4.0, 2.5, 16.0, 7.0, 1.5, 0.8]], np.float32)
GRID = dict(m=3, n=3, length=120.0, capacity=14, rate=0.5)


def make(path, E, kind="plain", **over):
    cfg = dict(GRID, **over)
    layout = "ring" if path.startswith("ring") else "transposed"
    if kind == "validate":
        return engine_with(PATHS[path], E, layout=layout, planes=3, validate=True, **cfg)
    if kind == "het":
        return engine_with(PATHS[path], E, layout=layout, planes=3, validate=True, archetypes=ARCH, **cfg)
    return engine_with(PATHS[path], E, layout=layout, planes=2, **cfg)


def snapshot(eng):
    """Everything a test may compare, as host arrays."""
    torch.cuda.synchronize()
    s = {k: getattr(eng, k).cpu().numpy().copy() for k in ("leading", "lastcar", "obs", "rewards", "waiting", "passed_dst", "done")}
    x, v, w = eng.planes_numpy()
    s["x"], s["v"], s["w"] = x.copy(), v.copy(), w.copy()
    s["arch"] = eng.arch.cpu().numpy().copy() if eng.het else None
    s["has_w"] = eng.P == 3
    s["done_tick"] = eng.done_tick.cpu().numpy().copy()
    if eng.n_trips is not None:
        s["n_trips"] = eng.n_trips.cpu().numpy().copy()
        s["trip_times"] = eng.trip_times.cpu().numpy().copy()
    return s, eng.C


def assert_env_equal(sa, a, sb, b, where, w_shift=0, stamps=True, clock_map=None):
    """env a of snapshot sa == env b of snapshot sb, bit for bit: counters, ring indices, every live (x, v, w, row).
    clock_map: sa was taken at a clock far from sb's - sb's spawn ticks, overflow stamp and trip log go through the exact
    integer maps of tests/test_late_clock_host.py:ClockMap (w, stamp, trips) first; everything is still compared bit for
    bit."""
    (A, Cc), (B, _) = sa, sb
    for k in ("leading", "lastcar", "obs", "waiting", "passed_dst", "done"):
        assert np.array_equal(A[k][a], B[k][b]), (k, a, b, where)
    assert same_bits(A["rewards"][a], B["rewards"][b]), ("rewards", a, b, where)
    live = live_mask(A["leading"][a], A["lastcar"][a], Cc)
    assert same_bits(A["x"][a][live], B["x"][b][live]) and same_bits(A["v"][a][live], B["v"][b][live]), ("cars", a, b, where)
    if A["has_w"]:
        want = B["w"][b][live] + np.float32(w_shift) if clock_map is None else clock_map.w(B["w"][b][live])
        assert same_bits(A["w"][a][live], want), ("w", a, b, where)
    if A["arch"] is not None:
        assert np.array_equal(A["arch"][a][live], B["arch"][b][live]), ("rows", a, b, where)
    if stamps:
        want = B["done_tick"][b] + (w_shift if B["done_tick"][b] else 0) if clock_map is None else clock_map.stamp(B["done_tick"][b])
        assert A["done_tick"][a] == want, ("done_tick", a, b, where)
    if "n_trips" in A:
        n = int(A["n_trips"][a])
        assert n == int(B["n_trips"][b]), ("n_trips", a, b, where)
        want = B["trip_times"][b][:n] if clock_map is None else clock_map.trips(b, B["trip_times"][b][:n])
        assert same_bits(A["trip_times"][a][:n], want), ("trip_times", a, b, where)


class Inputs(object):
    """Held actions and per-tick arrival counts (and rows) for E envs; env e receives what env of[e] receives."""

    def __init__(self, eng, seed, density=0.2):
        self.eng, self.rng, self.density = eng, np.random.RandomState(seed), density
        self.of = np.arange(eng.E)

    def bind(self, n):
        eng, rng = self.eng, self.rng
        act = rng.randint(2, size=(eng.E, eng.I)).astype(np.int32)[self.of]
        cnt = (rng.rand(n, eng.E, eng.n_entry) < self.density).astype(np.int32) * rng.randint(1, 3, size=(n, eng.E, eng.n_entry))
        cnt = cnt.astype(np.int32)[:, self.of]
        eng.set_actions(act)
        if eng.het:
            rows = rng.randint(len(ARCH), size=(n, eng.E, eng.n_entry, eng.C - 2)).astype(np.uint8)[:, self.of]
            eng.set_spawns(counts=cnt, per_tick=True, rows=rows)
        else:
            eng.set_spawns(counts=cnt, per_tick=True)


def drive(eng, inp, call):
    kind, n = call
    inp.bind(n)
    if kind == "agent":
        eng.agent_step(n)
    else:
        eng.step(n)


# 41 ticks (a car needs some 22 to reach the end of its first road), ending on three pairs: where the pairs run, roads that
# handed a car over in the call's last tick then start one row down their column (hb = 1; two cars in ONE tick, hb = 2, is
# rare in ordinary traffic - the twin test states what it finds)
WARMUP = [("step", 1), ("step", 1), ("step", 1), ("step", 4), ("agent", 5), ("step", 3), ("step", 2), ("step", 7), ("agent", 6),
          ("step", 5), ("step", 6)]
WARM_TICKS = sum(n for _, n in WARMUP)
WARMUP_ODD = WARMUP + [("step", 1), ("step", 6), ("step", 1)]                                             # ends tick by tick
AFTER = [("step", 1), ("step", 4), ("agent", 6), ("step", 3), ("step", 2), ("agent", 5), ("step", 1), ("step", 8),
         ("agent", 10), ("step", 7), ("step", 2), ("step", 1), ("agent", 4), ("step", 6), ("step", 5)]      # 65 ticks
SRC = np.array([-1, -1, -1, 0, 1, 2, 0, 1, 2, 0, -1, 1, 2, -1], np.int32)


# ---- 1. the twin test --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("warm", ["pair", "odd"])
@pytest.mark.parametrize("path,kind", [(p, "plain") for p in TRANSPOSED + ["ring", "ring_resident"]] +
                         [(p, "validate") for p in ("pertick", "pairs_tail", "pairs_split", "pairs_seg", "ring")] +
                         [(p, "het") for p in HET_PATHS])
def test_twin(path, kind, warm):
    E = len(SRC)
    src = SRC
    eng, ref = make(path, E, kind), make(path, E, kind)       # ref: the same run, never cloned
    ph = np.random.RandomState(3).randint(2, size=(E, eng.I)).astype(np.int32)
    ia, ib = Inputs(eng, 77), Inputs(ref, 77)
    for e_, i_ in ((eng, ia), (ref, ib)):
        e_.reset(ph)
        for call in (WARMUP if warm == "pair" else WARMUP_ODD):
            drive(e_, i_, call)
    before = snapshot(eng)
    assert len({before[0]["x"][k].tobytes() for k in range(E)}) == E      # (the envs differ)
    if path.startswith("pairs"):
        # the sources stand between two two-tick passes: the three envs with the most columns that start a row or two
        # down (roads that handed cars over in the call's last tick) serve as the sources
        hb = eng.head_rows()
        srcs = np.argsort(-(hb > 0).sum(axis=1), kind="stable")[:3]
        rest = [k for k in range(E) if k not in srcs]
        src = np.full(E, -1, np.int32)
        for i, k in enumerate(rest[:-2]):
            src[k] = srcs[i % 3]
        print("rows without a car at the top of the sources' columns, roads by count:", np.bincount(hb[srcs].ravel()).tolist())
        assert warm != "pair" or (hb[srcs] > 0).any()
    else:
        assert not eng.head_rows().any()
    eng.clone_envs(src)
    assert np.array_equal(eng.head_rows()[np.where(src >= 0)[0]], eng.head_rows()[src[src >= 0]])
    assert eng.clone_skipped() == 0
    mapped = np.where(src >= 0, src, np.arange(E))
    now = snapshot(eng)
    for k in range(E):                                            # the clone itself, before anything runs
        assert_env_equal(now, k, before, mapped[k], "right after the clone")
    ia.of = ib.of = mapped
    ticks = 0
    for call in AFTER:
        drive(eng, ia, call)
        drive(ref, ib, call)
        ticks += call[1]
        sa, sb = snapshot(eng), snapshot(ref)
        for k in range(E):
            if src[k] >= 0:
                assert_env_equal(sa, k, sa, src[k], (path, kind, call, ticks))
            else:
                assert_env_equal(sa, k, sb, k, (path, kind, "undisturbed", call, ticks))
    assert ticks >= 60
    if path.startswith("pairs"):
        assert eng.pair_ticks() > 0
    if path.endswith("resident") and kind == "plain":
        assert eng.fused_ticks()[0] > 0
    assert sa[0]["lastcar"].max() > 1 and sa[0]["leading"].max() > 1       # (cars arrived, and cars left roads)


# ---- 2. a cloned env against the checker -------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["pairs_tail", "pertick", "ring"])
def test_clone_vs_oracle(path):
    E = len(SRC)
    eng = make(path, E, "validate")
    orc = oracle_like(eng)
    inp = Inputs(eng, 5)
    eng.reset(np.zeros((E, eng.I), np.int32))
    for call in WARMUP:
        drive(eng, inp, call)
    eng.clone_envs(SRC)
    # the oracle starts from the exported state of the batch (as tests/test_gpu_parity.py loads one)
    s, _ = snapshot(eng)
    for k in range(E):
        orc.load_planes(k, s["x"][k], s["v"][k], s["w"][k], s["leading"][k], s["lastcar"][k])
    orc.obs[:] = s["obs"]
    orc.waiting[:] = s["waiting"]
    orc.passed_dst[:] = s["passed_dst"]
    orc.rewards[:] = s["rewards"]
    orc.steps[:] = eng.tick
    rng = np.random.RandomState(11)
    for n in (1, 4, 3, 2, 6, 5):
        acts = rng.randint(2, size=(n, E, eng.I)).astype(np.int32)
        roads = [[rng.choice(eng.entrypoints, size=rng.randint(0, 3)).tolist() for _ in range(E)] for _ in range(n)]
        cnt = np.zeros((n, E, eng.n_entry), np.int32)
        for t in range(n):
            for k in range(E):
                for rd in roads[t][k]:
                    cnt[t, k, eng.entry_index[int(rd)]] += 1
        eng.set_actions(acts, per_tick=True)
        eng.set_spawns(counts=cnt, per_tick=True)
        eng.step(n)
        for t in range(n):
            orc.step(acts[t], roads[t])
        assert_same_state(eng, orc, "%s after %d more ticks" % (path, n))


# ---- 3. across handles: snapshot, run on, restore ------------------------------------------------------------------------
@pytest.mark.parametrize("path,kind", [("pairs_tail", "validate"), ("pertick", "validate"), ("pairs_split", "het"),
                                       ("pertick", "het"), ("ring", "validate"), ("resident", "plain"), ("pairs_seg", "plain")])
def test_snapshot_restore_across_clocks(path, kind):
    E = 6
    eng, ref, stash = make(path, E, kind), make(path, E, kind), make(path, E + 3, kind, env_id_offset=40)
    ph = np.random.RandomState(9).randint(2, size=(E, eng.I)).astype(np.int32)
    ia, ib = Inputs(eng, 21), Inputs(ref, 21)
    for e_, i_ in ((eng, ia), (ref, ib)):
        e_.reset(ph)
        for call in WARMUP:
            drive(e_, i_, call)
    # the stash's clock differs by an odd number of ticks
    stash.reset(np.zeros((E + 3, eng.I), np.int32))
    stash.set_spawns()
    stash.set_actions(np.zeros((E + 3, eng.I), np.int32))
    stash.step(WARM_TICKS + 13)
    shift = stash.tick - eng.tick
    assert shift % 2 != 0
    to_stash = torch.tensor([5, 4, 3, 2, 1, 0, -1, 0, -1], dtype=torch.int32)
    stash.clone_envs(to_stash, source=eng)
    assert stash.clone_skipped() == 0
    a, b = snapshot(stash), snapshot(eng)
    for k in range(E):
        assert_env_equal(a, k, b, 5 - k, "in the stash", w_shift=shift)
    # the first handle runs on (and loses the state); then everything comes back
    detour = Inputs(eng, 99)
    for call in [("step", 3), ("agent", 4), ("step", 2)]:
        drive(eng, detour, call)
    gone = eng.tick - WARM_TICKS
    back = torch.tensor([5, 4, 3, 2, 1, 0], dtype=torch.int32)
    eng.clone_envs(back, source=stash)
    a = snapshot(eng)
    for k in range(E):
        assert_env_equal(a, k, b, k, "restored", w_shift=gone)
    # ... and continues as the uninterrupted run does: spawn ticks differ by the detour, trip times do not
    for call in AFTER + AFTER:             # (130 ticks: long enough for cars that entered after the restore to leave the map)
        drive(eng, ia, call)
        drive(ref, ib, call)
        sa, sb = snapshot(eng), snapshot(ref)
        for k in range(E):
            assert_env_equal(sa, k, sb, k, (path, kind, call), w_shift=gone, stamps=False)
    if kind != "plain":
        assert sa[0]["n_trips"].sum() > b[0]["n_trips"].sum()       # (trips were logged after the restore)


# ---- 4. arrival streams on the device ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["resident", "pertick", "pairs_tail", "ring"])
@pytest.mark.parametrize("regular", [False, True])
def test_streams_follow_the_flag(path, regular):
    """Entry roads long enough that no car leaves one inside the test: a road's car count grows by its arrivals."""
    E, off, rate, seed = 8, 100, 0.9, 0xABCDEF0123
    src = np.array([-1, -1, 0, 0, 1, -1, 1, 0], np.int32)
    Mirror = devrng.RegularMirror if regular else devrng.PoissonMirror
    for with_stream in (True, False):
        eng = make(path, E, m=2, n=2, length=400.0, capacity=66, env_id_offset=off)
        (eng.set_regular if regular else eng.set_poisson)(rate, seed=seed)
        eng.set_actions(np.zeros((E, eng.I), np.int32))
        eng.reset(np.zeros((E, eng.I), np.int32))
        mir = Mirror(rate, seed, eng.n_entry, [off + k for k in range(E)])
        entry = torch.as_tensor(eng.entrypoints.astype(np.int64)).to(eng.device)
        cars = eng.cars_on_roads_flat()[:, entry].cpu().numpy().copy()
        hist = []
        for t in range(10):
            eng.step(1 if t % 3 else 2)
            for _ in range(1 if t % 3 else 2):
                hist.append(mir.next_tick())
        eng.clone_envs(src, streams=with_stream)
        now = eng.cars_on_roads_flat()[:, entry].cpu().numpy().copy()
        want = np.sum(hist, axis=0)
        assert np.array_equal(now, np.where(src[:, None] >= 0, want[np.maximum(src, 0)], want))
        for t in range(8):
            n = 1 + t % 3
            eng.step(n)
            got = eng.cars_on_roads_flat()[:, entry].cpu().numpy().copy()
            arrivals = np.sum([mir.next_tick() for _ in range(n)], axis=0)
            follow = np.where(src >= 0, src, np.arange(E)) if with_stream else np.arange(E)
            assert np.array_equal(got - now, arrivals[follow]), (path, regular, with_stream, t)
            now = got
        assert int(now.sum()) > 20


# ---- 5. episodes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["resident", "pairs_tail", "ring"])
@pytest.mark.parametrize("flag", [True, False])
def test_episode_accounting_travels_with_the_flag(path, flag):
    E, off, seed, limit, T = 6, 30, 4242, 4, 4
    eng = make(path, E, learn_switch=True, env_id_offset=off)
    eng.set_episodes(max_decisions=limit, seed=seed)
    eng.set_spawns(period=3)
    eng.set_actions(np.zeros((E, eng.I), np.int32))          # learn_switch: action 0 keeps the phases as drawn
    ph = np.random.RandomState(1).randint(2, size=(E, eng.I)).astype(np.int32)
    eng.reset(ph)
    model = EpisodeModel(E, eng.I, limit)
    for _ in range(2):
        _, rew, done = eng.agent_step(T)
        model.decision(rew.cpu().numpy(), done.cpu().numpy())
    # stagger the episodes: envs 0 and 1 start anew, the others are two decisions in
    mask = np.array([1, 1, 0, 0, 0, 0], np.uint8)
    eng.reset_envs(mask, ph)
    model.abandon(mask)
    _, rew, done = eng.agent_step(T)
    model.decision(rew.cpu().numpy(), done.cpu().numpy())
    src = np.array([-1, -1, 0, -1, 1, 3], np.int32)           # clones of a young episode (2, 4) and of an old one (5)
    eng.clone_envs(src, episodes=flag)
    if flag:
        for k in np.nonzero(src >= 0)[0]:
            model.ep_return[k], model.ep_len[k], model.ep_index[k] = model.ep_return[src[k]], model.ep_len[src[k]], model.ep_index[src[k]]
    assert np.array_equal(eng.ep_len.cpu().numpy(), model.ep_len) and np.array_equal(eng.ep_index.cpu().numpy(), model.ep_index)
    assert same_bits(eng.ep_return.cpu().numpy(), model.ep_return)
    ids = off + np.arange(E)
    for d in range(2 * limit + 1):
        index_before = model.ep_index.copy()
        restarting = eng.ep_len.cpu().numpy() == 0
        _, rew, done = eng.agent_step(T)
        end = model.decision(rew.cpu().numpy(), done.cpu().numpy())
        for name in ("ep_len", "ep_index", "final_len", "truncated"):
            assert np.array_equal(getattr(eng, name).cpu().numpy(), getattr(model, name)), (name, d)
        assert same_bits(eng.ep_return.cpu().numpy(), model.ep_return) and same_bits(eng.final_return.cpu().numpy(), model.final_return)
        # a restart draws its phases by rule 2 under the env's OWN global id
        want = devrng.episode_phases(seed, ids, index_before, eng.I)
        got = eng.current_phase.cpu().numpy()
        fresh = restarting & (index_before > 0)
        assert np.array_equal(got[fresh], want[fresh]), d
    assert model.ep_index.min() >= 2
    # flag set, episodes on in one handle only: refused
    other = make(path, E, learn_switch=True)
    other.reset(ph)
    with pytest.raises(nat.TfxError, match="episodes on in one handle only"):
        other.clone_envs(src, source=eng, episodes=True)
    other.clone_envs(src, source=eng)                                       # (fine without the flag)


# ---- 6. the in-place rule on the device ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["pairs_tail", "ring"])
def test_in_place_rule_matches_clone_plan(path):
    E = 24
    eng = make(path, E, "validate")
    inp = Inputs(eng, 13)
    eng.reset(np.random.RandomState(2).randint(2, size=(E, eng.I)).astype(np.int32))
    rng = np.random.RandomState(17)
    fixed = [np.r_[-1, 0, 1, np.full(E - 3, -1)], np.r_[1, 2, 0, np.full(E - 3, -1)], np.arange(E), np.full(E, E), np.full(E, -2),
             np.r_[0, np.zeros(E - 1)]]
    for trial in range(14):
        for call in [("step", 3), ("step", 4)]:
            drive(eng, inp, call)
        src = (fixed[trial] if trial < len(fixed) else rng.randint(-3, E + 3, size=E)).astype(np.int32)
        if trial >= 10:
            src[rng.rand(E) < 0.6] = -1                       # (sparser wishes: more of them can be granted)
        applied, skipped = devrng.clone_plan(src)
        before = snapshot(eng)
        eng.clone_envs(torch.as_tensor(src).to(eng.device))
        after = snapshot(eng)
        assert eng.clone_skipped() == skipped and eng.clone_skipped() == 0, trial
        for k in range(E):
            assert_env_equal(after, k, before, src[k] if applied[k] else k, (trial, k))
    assert applied.any()


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_field_and_leave_the_handles_usable():
    E = 4
    a = make("pertick", E)
    idx = torch.full((E,), -1, dtype=torch.int32, device=a.device)
    idx[1] = 0
    for field, other in (("capacity", make("pertick", E, capacity=16)), ("length", make("pertick", E, length=130.0)),
                         ("in m ", make("pertick", E, m=2)), ("layout", make("ring", E)), ("planes", make("pertick", E, "validate")),
                         ("entry_spec", make("pertick", E, entry_spec=1)), ("learn_switch", make("pertick", E, learn_switch=True)),
                         ("in rate", make("pertick", E, rate=0.25))):
        with pytest.raises(nat.TfxError, match=field):
            other.clone_envs(idx, source=a)
        with pytest.raises(nat.TfxError, match=field):
            a.clone_envs(idx, source=other)
    two = make("pertick", E, "het")
    with pytest.raises(nat.TfxError, match="n_archetypes"):
        two.clone_envs(idx, source=make("pertick", E, "validate"))
    tab = ARCH.copy()
    tab[1, 2] = 2.0
    three = engine_with(PATHS["pertick"], E, planes=3, validate=True, archetypes=tab, **GRID)
    with pytest.raises(nat.TfxError, match="archetype table"):
        two.clone_envs(idx, source=three)
    # streams: none / different seed / different kind / different rate
    b = make("pertick", E)
    with pytest.raises(nat.TfxError, match="arrival stream"):
        b.clone_envs(idx, source=a, streams=True)
    a.set_poisson(0.5, seed=1)
    for setup, word in ((lambda: b.set_poisson(0.5, seed=2), "seed"), (lambda: b.set_regular(0.5, seed=1), "kind"),
                        (lambda: b.set_poisson(0.6, seed=1), "rate")):
        setup()
        with pytest.raises(nat.TfxError, match=word):
            b.clone_envs(idx, source=a, streams=True)
    b.set_poisson(0.5, seed=1)
    lib = a.lib
    # an unbound handle, bad flags, a null index array
    raw = C.c_void_p()
    nat.check(lib.tfx_create(C.byref(a.cfg), C.byref(raw)))
    assert lib.tfx_clone_envs(raw, raw, C.c_void_p(idx.data_ptr()), 0, None) == -2
    assert lib.tfx_clone_envs(a.h, raw, C.c_void_p(idx.data_ptr()), 0, None) == -2
    assert b"tfx_bind_buffers" in lib.tfx_last_error()
    nat.check(lib.tfx_destroy(raw))
    assert lib.tfx_clone_envs(a.h, a.h, C.c_void_p(idx.data_ptr()), 8, None) == -1
    assert lib.tfx_clone_envs(a.h, a.h, None, 0, None) == -1
    with pytest.raises(ValueError):
        a.clone_envs(np.zeros(E + 1, np.int32))
    # an injected launch failure of the clone
    ph = np.zeros((E, a.I), np.int32)
    a.reset(ph)
    b.reset(ph)
    a.set_actions(ph)
    b.set_actions(ph)
    a.step(5)
    nat.check(lib.tfx_debug_fail_after(b.h, 1))
    with pytest.raises(nat.TfxError, match="injected"):
        b.clone_envs(idx, source=a, streams=True)
    # both handles still work: the clone goes through, and clone and source then move in step
    b.clone_envs(idx, source=a, streams=True)
    a.clone_envs(idx, streams=True)
    for n in (3, 4):
        a.step(n)
        b.step(n)
    sa, sb = snapshot(a), snapshot(b)
    assert_env_equal(sb, 1, sa, 0, "after the refusals", w_shift=b.tick - a.tick)
    assert_env_equal(sa, 1, sa, 0, "after the refusals")
    assert sa[0]["lastcar"][0].max() > 1


# ---- 8. sizes ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,envs", [("cfg0", 1), ("cfg0", 7), ("cfg1", 32), ("cfg2", 1), ("cfg2", 32)])
def test_sizes_fan_out(name, envs):
    """The benchmark's workload at small batch sizes (cfg0 / cfg1: k_res handles; cfg2 = 16x16, C = 66): a snapshot in a
    second handle, the envs wiped, a restore - then equal to an uninterrupted run; with more than 20 envs a fan-out in
    place as well."""
    eng, ref, stash = [wl.setup_engine(name, envs=envs) for _ in range(3)]
    for e_ in (eng, ref):
        e_.step(11)
    ident = torch.arange(envs, dtype=torch.int32)
    stash.step(2)
    stash.clone_envs(ident, source=eng)
    # (the workload's lights and arrivals are rules of the clock: the state goes back at the tick it was taken)
    eng.reset_envs(np.ones(envs, np.uint8), np.zeros((envs, eng.I), np.int32))
    assert int(eng.lastcar.max()) == 1
    eng.clone_envs(ident, source=stash)
    if envs > 20:                        # (env k and env k mod 20 receive the same inputs)
        fan = np.where(np.arange(envs) < 20, -1, np.arange(envs) % 20).astype(np.int32)
        eng.clone_envs(fan)
        assert eng.clone_skipped() == 0
    for n in (1, 10, 9):
        eng.step(n)
        ref.step(n)
    sa, sb = snapshot(eng), snapshot(ref)
    for k in range(envs):
        assert_env_equal(sa, k, sb, k, (name, k), stamps=False)


def test_headline_shape_all_envs_pinned():
    """4096 envs of the 16x16 grid (C = 66) after the benchmark's settle: every env cloned from envs 0..19, 20 more ticks,
    and env k equals env k mod 20 bit for bit - the workload's inputs depend on the env id modulo the light period only,
    so this also pins ALL 4096 envs of the benchmark's batch to twenty of them."""
    eng = wl.setup_engine("cfg2")
    E = eng.E
    eng.step(wl.SETTLE_TICKS["cfg2"])
    k = torch.arange(E, dtype=torch.int32, device=eng.device)
    src = torch.where(k < 20, torch.full_like(k, -1), k % 20)
    pre = {n: getattr(eng, n).clone() for n in ("leading", "lastcar", "obs")}
    eng.clone_envs(src)
    assert eng.clone_skipped() == 0
    for n in pre:                                  # (the workload guarantees it: the clone changed nothing visible)
        assert torch.equal(getattr(eng, n), pre[n]), n
    eng.step(20)
    pin = (k % 20).long()
    for n in ("leading", "lastcar", "obs", "rewards", "waiting", "passed_dst", "done_tick"):
        t = getattr(eng, n)
        assert torch.equal(t, t[pin]), n
    xv = eng.xv                                    # ring-layout staging copy [E,R,C,2]
    ld, lc = eng.leading.long(), eng.lastcar.long()
    slot = torch.arange(eng.C, device=eng.device)[None, None, :]
    live = torch.where((ld <= lc)[..., None], (slot > ld[..., None]) & (slot <= lc[..., None]),
                       ((slot > ld[..., None]) | (slot <= lc[..., None])) & (slot >= 1))
    bits = xv.view(torch.int32)
    assert bool(((bits == bits[pin]).all(dim=-1) | ~live).all())
    assert int(live.sum()) > 10 * E * eng.R


# ---- the batched env's surface ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spawn", ["poisson", "regular", "device", "regular_device"])
def test_vec_env_snapshot_restore_and_branch(spawn):
    """TrafficVecEnv: snapshot(), a detour, restore() - then the env replays what an undisturbed twin does, arrivals
    included (host-replayed generator states are copied, on-device streams cloned); and an in-place branch makes env 3
    follow env 0."""
    from gym_traffic.envs.vec_env import TrafficVecEnv
    E = 5
    kw = dict(capacity=14, spawn=spawn, seed=31, local_cars_per_sec=0.12, autoreset=True, episode_len=50)
    venv, twin = TrafficVecEnv(E, 3, 3, 120.0, **kw), TrafficVecEnv(E, 3, 3, 120.0, **kw)
    ph = np.random.RandomState(4).randint(2, size=(E, venv.engine.I)).astype(np.int32)
    rng = np.random.RandomState(6)
    acts = [torch.as_tensor(rng.randint(2, size=(E, venv.engine.I)).astype(np.int32)).to(venv.engine.device) for _ in range(12)]
    for v in (venv, twin):
        v.reset(ph)
        for a in acts[:3]:
            v.agent_step(a, n_ticks=5)
    snap = venv.snapshot()
    for a in acts[3:6]:
        venv.agent_step(a, n_ticks=4)                      # the detour
    venv.restore(snap)
    shift = venv.engine.tick - twin.engine.tick
    for a in acts[6:9]:
        oa, ob = venv.agent_step(a, n_ticks=5), twin.agent_step(a, n_ticks=5)
        for u, w in zip(oa, ob):
            assert torch.equal(u, w)
        assert torch.equal(venv.episode_return, twin.episode_return) and torch.equal(venv.episode_length, twin.episode_length)
    sa, sb = snapshot(venv.engine), snapshot(twin.engine)
    for k in range(E):
        assert_env_equal(sa, k, sb, k, spawn, w_shift=shift, stamps=False)
    assert sa[0]["lastcar"].max() > 1
    # a branch in place: env 3 becomes env 0 and, fed env 0's actions, stays env 0
    venv.clone_envs(np.array([-1, -1, -1, 0, -1], np.int32))
    assert venv.engine.clone_skipped() == 0
    for a in acts[9:]:
        a = a.clone()
        a[3] = a[0]
        venv.agent_step(a, n_ticks=5)
    s = snapshot(venv.engine)
    assert_env_equal(s, 3, s, 0, "branch " + spawn)
    assert not np.array_equal(s[0]["obs"][1], s[0]["obs"][0])


# ---- heterogeneous cars on the on-device streams: counts AND rows, in place and across handles ----------------------------------------------
@pytest.mark.parametrize("path", HET_PATHS)
@pytest.mark.parametrize("regular", [False, True])
@pytest.mark.parametrize("with_stream", [True, False])
def test_het_streams_rows_follow_the_flag(path, regular, with_stream):
    """Mixed cars from tfx_set_poisson / tfx_set_regular.  Roads long enough that no car leaves an entry road inside the
    test, so the cars of an entry road, in ring order, are its arrivals in order: their table rows must be the rows rule 1
    of include/tfx.h draws under the stream the env follows - its source's with TFX_CLONE_STREAM (id, position and the
    per-entry counters `seq` travel), its own without - and with the flag clone and source stay equal bit for bit.
    (The regular stream makes every car row 0, traffic_env.py:174: that half checks counts, roads and positions; the
    identity of the rows is what the Poisson half checks.)"""
    Ea, Eb, offa, offb, rate, seed = 8, 12, 10, 50, 0.9, 0x5EED5
    cfg = dict(m=2, n=2, length=400.0, capacity=66)
    a, b = make(path, Ea, "het", env_id_offset=offa, **cfg), make(path, Eb, "het", env_id_offset=offb, **cfg)
    ids = [offa + k for k in range(Ea)] + [offb + k for k in range(Eb)]
    Mirror = devrng.RegularMirror if regular else devrng.PoissonMirror
    mir = Mirror(rate, seed, a.n_entry, ids, n_archetypes=len(ARCH), per_road=a.C - 2)
    for e_ in (a, b):
        (e_.set_regular if regular else e_.set_poisson)(rate, seed=seed)
        e_.set_actions(np.zeros((e_.E, e_.I), np.int32))
        e_.reset(np.zeros((e_.E, e_.I), np.int32))
    b.step(3)                                          # (the clocks differ by an odd number of ticks)
    for _ in range(3):
        mir_b_only = mir.next_tick()                   # ... and b's streams have moved on; a's have not yet:
    # a's ids must not advance with b's three ticks - a mirror of its own for each handle
    mira = Mirror(rate, seed, a.n_entry, ids[:Ea], n_archetypes=len(ARCH), per_road=a.C - 2)
    mirb = Mirror(rate, seed, a.n_entry, ids[Ea:], n_archetypes=len(ARCH), per_road=a.C - 2)
    for _ in range(3):
        mirb.next_tick()
    del mir, mir_b_only
    follow = {("a", k): ("a", k) for k in range(Ea)}
    follow.update({("b", k): ("b", k) for k in range(Eb)})
    seqs = {key: [[] for _ in range(a.n_entry)] for key in follow}
    seqs_b_before = None

    def ticks(n, kind="step"):
        for e_ in (a, b):
            e_.agent_step(n) if kind == "agent" else e_.step(n)
        for _ in range(n):
            ca, ra = mira.next_tick()
            cb, rb = mirb.next_tick()
            data = {("a", k): (ca[k], ra[k]) for k in range(Ea)}
            data.update({("b", k): (cb[k], rb[k]) for k in range(Eb)})
            for key in seqs:
                cnt, rows = data[follow[key]]
                for ej in range(a.n_entry):
                    seqs[key][ej] += [int(x) for x in rows[ej, :cnt[ej]]]

    # b's first three ticks happened before the bookkeeping began: its envs are overwritten or not compared below
    for n, kind in ((1, "step"), (2, "step"), (3, "agent"), (1, "step"), (4, "step")):
        ticks(n, kind)
    src_a = np.array([-1, -1, -1, 0, 1, 2, 0, -1], np.int32)
    src_b = np.array([0, 1, 2, 3, 0, 1, 2, 3, 7, 7, 4, 5], np.int32)          # every env of b: a fan-out across handles
    b.clone_envs(src_b, source=a, streams=with_stream)
    a.clone_envs(src_a, streams=with_stream)
    assert a.clone_skipped() == 0 and b.clone_skipped() == 0
    new = {}
    for k, s in enumerate(src_b):
        new[("b", k)] = ("a", int(s))
    for k, s in enumerate(src_a):
        if s >= 0:
            new[("a", k)] = ("a", int(s))
    old = {key: [list(x) for x in seqs[key]] for key in seqs}
    for key, s in new.items():
        seqs[key] = [list(x) for x in old[s]]
        if with_stream:
            follow[key] = follow[s]
    for n, kind in ((1, "step"), (2, "step"), (2, "agent"), (3, "step"), (1, "step"), (4, "step")):
        ticks(n, kind)
    total = 0
    for name, eng in (("a", a), ("b", b)):
        arch, lc = eng.arch.cpu().numpy(), eng.lastcar.cpu().numpy()
        assert (eng.leading.cpu().numpy()[:, eng.entrypoints] == 1).all()      # (no car has left an entry road)
        for k in range(eng.E):
            for ej, road in enumerate(eng.entrypoints):
                want = seqs[(name, k)][ej]
                assert lc[k, road] == 1 + len(want), (name, k, ej)
                assert arch[k, road, 2:2 + len(want)].tolist() == want, (name, k, ej, with_stream)
                total += len(want)
    assert total > 100 and (regular or len({tuple(seqs[("a", 0)][ej]) for ej in range(a.n_entry)}) > 1)
    sa, sb = snapshot(a), snapshot(b)
    if with_stream:
        for k, s in enumerate(src_b):
            if src_a[s] == -1:              # (a's envs 3..6 were overwritten in place after b took its copies of them)
                assert_env_equal(sb, k, sa, int(s), ("across handles", path, regular), w_shift=b.tick - a.tick)
        for k, s in enumerate(src_a):
            if s >= 0:
                assert_env_equal(sa, k, sa, int(s), ("in place", path, regular))
    elif not regular:
        assert any(seqs[("a", 3)][ej] != seqs[("a", 0)][ej] for ej in range(a.n_entry))   # (independent arrivals)


# ---- more refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_constants_kinds_burst(monkeypatch):
    from gym_traffic import core
    E = 3
    a = make("pertick", E)
    idx = torch.full((E,), -1, dtype=torch.int32, device=a.device)
    for name, value in (("yellow_ticks", 4), ("thresh", 0.3), ("detect_dist", 12.0), ("overflow_penalty", 5.0), ("eps", 1e-6)):
        monkeypatch.setitem(core.CONSTANTS, name, value)
        other = make("pertick", E)
        monkeypatch.undo()
        with pytest.raises(nat.TfxError, match=name):
            other.clone_envs(idx, source=a)
    plain_order = engine_with(dict(PATHS["pertick"], TFX_KINDS="0"), E, **GRID)
    with pytest.raises(nat.TfxError, match="kinds ordering"):
        plain_order.clone_envs(idx, source=a)
    b = make("pertick", E)
    a.set_regular(0.9, seed=1)          # every tick, one car
    b.set_regular(1.2, seed=1)          # every tick, two cars
    with pytest.raises(nat.TfxError, match="burst"):
        b.clone_envs(idx, source=a, streams=True)
    b.set_regular(0.9, seed=1)
    b.clone_envs(idx, source=a, streams=True)


# ---- 9. no change elsewhere: a handle that never clones makes the parent's launches ------------------------------------------------------------
# Launches tfx_debug_fail_after counts in ONE 10-tick call of 8 envs of the 3x3 grid (capacity 12, a held action buffer,
# TFX_GRAPH=0): counted on the parent commit 3211ebf with count_call_launches below
# To recount after an intended change of the launch structure: check out the commit whose numbers are wanted, build it,
# and for every key "path/stream/call" make the engine exactly as test_never_cloning_handle_makes_the_parents_launches
# does (COUNT_PATHS[path] + TFX_GRAPH=0, 8 envs, 3x3, L = 120, C = 12, a held zero action buffer; periodic: period 3,
# poisson / regular: 0.8 cars per tick, seed 5) and print count_call_launches(eng, call) - it uses nothing newer than
# tfx_debug_fail_after.  The injection fails launches on the host; no device fault is involved.
PARENT_CALL_LAUNCHES = {
    "pairs/periodic/agent": 11, "pairs/periodic/step": 10, "pairs/poisson/agent": 30, "pairs/poisson/step": 10,
    "pairs/regular/agent": 30, "pairs/regular/step": 10, "pertick/periodic/agent": 20, "pertick/periodic/step": 20,
    "pertick/poisson/agent": 20, "pertick/poisson/step": 20, "pertick/regular/agent": 20, "pertick/regular/step": 20,
    "resident/periodic/agent": 1, "resident/periodic/step": 1, "resident/poisson/agent": 1, "resident/poisson/step": 1,
    "resident/regular/agent": 1, "resident/regular/step": 1, "ring/periodic/agent": 20, "ring/periodic/step": 20,
    "ring/poisson/agent": 20, "ring/poisson/step": 20, "ring/regular/agent": 20, "ring/regular/step": 20}
COUNT_PATHS = {"resident": PATHS["resident"], "pertick": PATHS["pertick"], "pairs": PAIRS, "ring": PATHS["ring"]}


def count_call_launches(eng, call):
    """The largest n for which the n-th launch of the call still exists (as tests/test_gpu_episodes.py counts)."""
    n = 0
    ph = np.zeros((eng.E, eng.I), np.int32)
    while n < 400:
        eng.reset(ph)
        nat.check(eng.lib.tfx_debug_fail_after(eng.h, n + 1))
        try:
            eng.step(10) if call == "step" else eng.agent_step(10)
        except nat.TfxError as exc:
            assert "injected" in str(exc)
            torch.cuda.synchronize()
            n += 1
            continue
        break
    nat.check(eng.lib.tfx_debug_fail_after(eng.h, 0))
    torch.cuda.synchronize()
    return n


@pytest.mark.parametrize("case", sorted(PARENT_CALL_LAUNCHES))
def test_never_cloning_handle_makes_the_parents_launches(case):
    path, stream, call = case.split("/")
    eng = engine_with(dict(COUNT_PATHS[path], TFX_GRAPH="0"), 8, layout="ring" if path == "ring" else "transposed",
                      m=3, n=3, length=120.0, capacity=12)
    eng.set_actions(np.zeros((8, eng.I), np.int32))
    if stream == "periodic":
        eng.set_spawns(period=3)
    elif stream == "poisson":
        eng.set_poisson(0.8, seed=5)
    else:
        eng.set_regular(0.8, seed=5)
    assert count_call_launches(eng, call) == PARENT_CALL_LAUNCHES[case]
    # ... and a clone is one launch more, exactly
    nat.check(eng.lib.tfx_debug_fail_after(eng.h, 2))
    eng.clone_envs(np.array([-1, 0, 0, -1, -1, -1, -1, -1], np.int32))
    with pytest.raises(nat.TfxError, match="injected"):
        eng.clone_envs(np.array([-1, 0, 0, -1, -1, -1, -1, -1], np.int32))
    nat.check(eng.lib.tfx_debug_fail_after(eng.h, 0))


# ---- the lookahead demo, end to end ---------------------------------------------------------------------------------------------------------------
def test_lookahead_demo_runs():
    import importlib.util
    import os
    from conftest import ROOT
    spec = importlib.util.spec_from_file_location("lookahead_demo", os.path.join(ROOT, "tools", "lookahead_demo.py"))
    demo = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(demo)
    r = demo.main(["--envs", "6", "--candidates", "4", "--horizon", "2", "--decisions", "8", "--m", "3", "--n", "3",
                   "--length", "120", "--capacity", "14", "--ticks", "5"])
    assert sum(r["wins"]) == 6 * 8 and np.isfinite(r["lookahead_return"]) and np.isfinite(r["greedy_return"])
    assert r["clone_ms"] > 0 and r["branches_ms"] > 0 and r["live_ms"] > 0
