"""Used handles must equal fresh ones: what a handle computes next depends only on what the caller can see - the ring
image, the bound buffers, the clock - and on its inputs (include/tfx.h, "What the next call depends on").

Handle A runs a PREFIX that leaves residue in the handle's own state (row offsets of a two-tick pass, stamps of the
risk bound in both planes, overflow and serial-advance stamps, the second stream's clock, a captured graph ...),
optionally a MUTATOR is applied, then A's caller-visible state goes to a handle B that has done nothing else, and both
run the same CONTINUATION on the same inputs.  Afterwards A and B are equal bit for bit (tests/test_gpu_clone.py:
assert_env_equal: ring words, obs, rewards, waiting, passed_dst, done, done_tick, every live car's x, v, w and row,
the trip log; plus the decision's three outputs and the vehicle updates), and the oracle, loaded from the same export
and fed the same inputs, agrees with A - so A and B cannot be wrong alike.  The scenarios and the list of triples are
tests/test_transplant_host.py's; a case here is one (path, kind, geometry, route) and runs the whole list.

Routes: "export" - B.reset, the bound tensors copied, B.load_state(A's export), B.set_tick(A.tick) (set_tick clears the
done stamps, so those are copied behind it), with the oracle leg; "self" - A loads its own export while a twin that ran
everything A ran does not: a no-op for all that follows; "clone" - B.set_tick(A.tick), B.clone_envs(every env, source=A,
streams, episodes) under on-device arrivals, the greedy controller and episodes: the state a caller cannot export.
Every prefix asserts that its residue is there, from counters the handle already has; no case provokes a failure."""
import time

import numpy as np
import pytest

import test_transplant_host as H
from test_gpu_fused import engine_with
from test_gpu_parity import assert_same_state, same_bits
from test_gpu_stride_rounds import assert_decision, assert_rows_and_trips

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from test_gpu_clone import ARCH, HET_PATHS, PATHS, assert_env_equal, snapshot  # noqa: E402

TAIL_PATHS = ("pairs_tail", "pairs_split", "pairs_seg", "pairs_nograph")          # k_tail behind every pass
CLONE_PATHS = ("resident", "pertick", "pairs_tail", "ring")
TWO_TILES = ("pairs_split", "pairs_seg", "ring")                                  # the paths that also run the 4x4 grid


def _matrix():
    out = []
    for geom, paths in (("g33", list(PATHS)), ("g44", list(TWO_TILES))):
        for path in paths:
            out.append((path, "plain", geom))
            if not path.endswith("resident"):                                     # (validate handles never run resident)
                out.append((path, "validate", geom))
            if path in HET_PATHS:
                out.append((path, "het", geom))
    return out


MATRIX = _matrix()
RULED_OUT = (len(PATHS) + len(TWO_TILES)) * len(H.KINDS) - len(MATRIX)


def make(w, path, prefix):
    knobs = dict(PATHS[path])
    if prefix == "P7":
        knobs["TFX_RES_MIN_TICKS"] = "3"                 # calls of one or two ticks leave k_res to the per-tick kernels
    cfg = dict(m=w.m, n=w.n, length=w.length, capacity=w.C, rate=w.rate)
    layout = "ring" if path.startswith("ring") else "transposed"
    if w.kind == "plain":
        return engine_with(knobs, w.E, layout=layout, planes=2, **cfg)
    return engine_with(knobs, w.E, layout=layout, planes=3, validate=True, **(dict(cfg, archetypes=ARCH) if w.het else cfg))


class DeviceSide(object):
    """A handle that executes the ops of tests/test_transplant_host.py.  device_inputs: arrivals from tfx_set_poisson,
    actions from the greedy controller, episodes on - the ops' own action and count arrays are then not used."""

    def __init__(self, w, path, prefix, device_inputs=False):
        self.w, self.path, self.device_inputs = w, path, device_inputs
        self.eng = eng = make(w, path, prefix)
        assert np.array_equal(eng.entrypoints, w.entry) and np.array_equal(eng.nexts, w.nexts)
        assert np.array_equal(eng.dest, w.dest) and np.array_equal(eng.phases, w.phases)
        if device_inputs:
            eng.set_poisson(2.0, seed=0xD1CE5)
            eng.set_greedy(3)
            eng.set_episodes(max_decisions=3, seed=5)
        eng.reset(np.zeros((w.E, eng.I), np.int32))
        self.outs = None

    def run(self, ops, after=None):
        for i, op in enumerate(ops):
            getattr(self, "_" + op["op"])(op)
            if after is not None:
                after(i, op)
        return self

    def _rows(self, rows):
        return rows if self.w.het else None

    def _load(self, op):
        eng, w = self.eng, self.w
        if op["reset"]:
            eng.reset(op["phase"])
        eng.load_state(op["x"], op["v"], op["leading"], op["lastcar"], w=op["w"], arch=op["arch"] if w.het else None)
        obs = np.zeros((w.E, eng.obs_len), np.int32)
        obs[:, 2 * w.r:2 * w.r + w.I] = op["phase"]
        obs[:, 2 * w.r + w.I:] = op["elapsed"]
        eng.obs.copy_(torch.as_tensor(obs))
        eng.waiting.zero_()
        eng.passed_dst.zero_()
        eng.rewards.zero_()
        if eng.n_trips is not None:
            eng.n_trips.zero_()
        eng.set_tick(op["tick"])

    def _step(self, op):
        if not self.device_inputs:
            self.eng.set_actions(op["acts"], per_tick=True)
            self.eng.set_spawns(counts=op["cnt"], per_tick=True, rows=self._rows(op["rows"]))
        self.eng.step(op["n"])

    def _agent(self, op):
        if not self.device_inputs:
            self.eng.set_actions(op["act"])
            self.eng.set_spawns(counts=op["cnt"], per_tick=True, rows=self._rows(op["rows"]))
        self.outs = [t.clone() for t in self.eng.agent_step(op["n"], remi=op["remi"])]

    def _halves(self, op):
        if not self.device_inputs:
            self.eng.set_spawns()
            self.eng.set_actions(self.eng.current_phase.clone())     # (no light changes: the oracle's side does the same)
        self.eng.move_cars()
        self.eng.advance_finished_cars()

    def _set_tick(self, op):
        self.eng.set_tick(op["to"] if "to" in op else self.eng.tick + op["rel"])

    def _reset_envs(self, op):
        self.eng.reset_envs(op["mask"], op["phase"])

    def _drop_tail(self, op):
        # the caller rewrites lastcar alone: every road's k-th car stays its k-th car, the tails are rebuilt
        eng = self.eng
        new = H.dropped_tails(eng.leading.cpu().numpy(), eng.lastcar.cpu().numpy(), op["pick"], eng.C)
        eng.lastcar.copy_(torch.as_tensor(new).to(eng.device))
        eng.refresh(cars=False)

    def _clone(self, op):
        self.eng.clone_envs(op["src"])
        assert self.eng.clone_skipped() == 0

    def export(self):
        """what the caller can see, as host arrays (the state tests/test_transplant_host.py:OracleSide.load takes)"""
        eng, w = self.eng, self.w
        x, v, wt = eng.planes_numpy()
        s = dict(x=x.copy(), v=v.copy(), w=wt.copy(), arch=eng.arch.cpu().numpy().copy() if w.het else None, tick=eng.tick)
        for f in ("leading", "lastcar", "obs", "rewards", "waiting", "passed_dst", "done", "done_tick"):
            s[f] = getattr(eng, f).cpu().numpy().copy()
        s["n_trips"] = eng.n_trips.cpu().numpy().copy() if w.validate else np.zeros(w.E, np.int64)
        s["trip_times"] = eng.trip_times.cpu().numpy().copy() if w.validate else np.zeros((w.E, eng.trip_cap), np.float32)
        return s


# ---- the three ways to hand the state over ------------------------------------------------------------------------------------
def hand_over_export(a, b, s):
    ea, eb, w = a.eng, b.eng, a.w
    eb.reset(s["obs"][:, 2 * w.r:2 * w.r + w.I])
    names = ["obs", "waiting", "rewards", "passed_dst"] + (["n_trips", "trip_times"] if w.validate else [])
    for f in names:
        getattr(eb, f).copy_(getattr(ea, f))
    eb.load_state(s["x"], s["v"], s["leading"], s["lastcar"], w=s["w"], arch=s["arch"])
    eb.set_tick(ea.tick)
    eb.done_tick.copy_(ea.done_tick)                      # (behind set_tick, which clears the stamps of the old clock)
    eb.done.copy_(ea.done)


def hand_over_self(a, s):
    a.eng.load_state(s["x"], s["v"], s["leading"], s["lastcar"], w=s["w"], arch=s["arch"])


def hand_over_clone(a, b):
    ea, eb = a.eng, b.eng
    eb.set_tick(ea.tick)
    eb.clone_envs(torch.arange(ea.E, dtype=torch.int32), source=ea, streams=True, episodes=True)
    assert eb.clone_skipped() == 0


# ---- comparisons ---------------------------------------------------------------------------------------------------------------------
def assert_handles_equal(a, b, where):
    sa, sb = snapshot(a.eng), snapshot(b.eng)
    for k in range(a.w.E):
        assert_env_equal(sa, k, sb, k, where)
    assert a.eng.tick == b.eng.tick, where
    assert (a.outs is None) == (b.outs is None), where
    for name, u, v in zip(("aobs", "areward", "adone"), a.outs or (), b.outs or ()):
        u, v = u.cpu().numpy(), v.cpu().numpy()
        assert same_bits(u, v) if u.dtype == np.float32 else np.array_equal(u, v), (name, where)
    assert a.eng.vehicle_updates() == b.eng.vehicle_updates(), ("vehicle_updates", where)
    if a.device_inputs:
        for f in ("ep_return", "ep_len", "ep_index"):
            assert torch.equal(getattr(a.eng, f), getattr(b.eng, f)), (f, where)
        if a.outs is not None:
            assert torch.equal(a.eng.truncated, b.eng.truncated), ("truncated", where)
            ended = (a.outs[2].bool() | a.eng.truncated.bool())
            assert torch.equal(a.eng.final_len[ended], b.eng.final_len[ended]), ("final_len", where)
            assert same_bits(a.eng.final_return[ended].cpu().numpy(), b.eng.final_return[ended].cpu().numpy()), ("final_return", where)


def assert_oracle_agrees(a, o, cont, updates0, where):
    eng, orc, w = a.eng, o.orc, a.w
    assert eng.tick == o.tick, where
    assert np.array_equal(eng.done.cpu().numpy(), o.done), ("done", where)
    if cont.startswith("agent"):
        assert_decision(eng, orc, a.outs, o.outs, w.tab10, str(where))
        assert np.array_equal(eng.obs.cpu().numpy()[:, w.r:], orc.obs[:, w.r:]), ("detected | phase | elapsed", where)
    else:
        assert_same_state(eng, orc, str(where))
        assert_rows_and_trips(eng, orc, w.tab10, str(where))
        assert eng.vehicle_updates() == orc.vehicle_updates - updates0, ("vehicle_updates", where)


# ---- the residue a prefix must leave --------------------------------------------------------------------------------------------
class Residue(object):
    """after=: called behind every op of the prefix; asserts what the table of prefixes promises, where the path has it"""

    def __init__(self, side, prefix, bound_inputs=True):
        self.side, self.prefix, self.bound, self.seen = side, prefix, bound_inputs, {}

    def __call__(self, i, op):
        eng, path, p = self.side.eng, self.side.path, self.prefix
        pairs = path.startswith("pairs")
        if p == "P1" and i == 1 and pairs:
            assert eng.head_rows().any(), "P1: no column starts a row down"
        if p == "P2" and i == 2 and pairs:
            # 4 + 2 of the 7 ticks in pairs: a call runs its pairs first, so the last mover was a one-tick kernel
            assert eng.pair_ticks() == 6, "P2: %d of 7 ticks ran in pairs" % eng.pair_ticks()
        if p == "P3" and op["op"] == "agent" and self.bound and path in TAIL_PATHS:
            now = eng.slow_pairs()
            assert now > self.seen.get("slow", 0), "P3: no env pair ran one tick at a time in decision %d" % (i // 2)
            self.seen["slow"] = now
        if p == "P4" and i == 1:
            adone = self.side.outs[2].cpu().numpy().astype(bool)
            assert adone.any() and not adone.all(), "P4: %s" % adone
        if p == "P5" and i == 1:
            assert int(eng.passed.max()) > 2, "P5: at most %d cars left one road in the last tick" % int(eng.passed.max())
        if p == "P6" and path == "pairs_split":
            if i == 1:
                self.seen["split"] = eng.split_ticks()
                assert self.seen["split"] > 0, "P6: the long call did not split"
            if i == 2:
                assert eng.split_ticks() == self.seen["split"], "P6: the short call split"
        if p == "P7" and path.endswith("resident") and self.side.w.kind == "plain":
            if i == 1:
                self.seen["fused"] = eng.fused_ticks()[0]
                assert self.seen["fused"] > 0, "P7: the long call did not run resident"
            if i == 2:
                assert eng.fused_ticks()[0] == self.seen["fused"], "P7: the short call ran resident"


def run_case(path, kind, geom, route, cases):
    w = H.World(geom, kind)
    clone = route == "clone"
    failures, t_start = [], time.time()
    for p, m, c in cases:
        where = (path, kind, geom, route, p, m, c)
        try:
            a = DeviceSide(w, path, p, device_inputs=clone)
            a.run(H.prefix_ops(geom, p), after=Residue(a, p, bound_inputs=not clone))
            a.run(H.mutator_ops(geom, m, p))
            live = int((a.eng.done == 0).sum())
            assert 2 * live >= w.E, "only %d of %d envs are live at the hand-over" % (live, w.E)
            orc = None
            if route == "export":
                b = DeviceSide(w, path, p)
                s = a.export()
                hand_over_export(a, b, s)
                orc = H.OracleSide(w).load(s)
            elif route == "self":
                b = DeviceSide(w, path, p)
                b.run(H.prefix_ops(geom, p)).run(H.mutator_ops(geom, m, p))        # the twin
                hand_over_self(a, a.export())
            else:
                b = DeviceSide(w, path, p, device_inputs=True)
                hand_over_clone(a, b)
            a.outs = b.outs = None
            a.eng.reset_counters()
            b.eng.reset_counters()
            assert_handles_equal(a, b, ("at the hand-over",) + where)
            a.run(H.cont_ops(geom, c))
            b.run(H.cont_ops(geom, c))
            assert_handles_equal(a, b, where)
            if orc is not None:
                updates0 = orc.orc.vehicle_updates
                orc.run(H.cont_ops(geom, c))
                assert_oracle_agrees(a, orc, c, updates0, where)
        except AssertionError as exc:
            failures.append("%s x %s x %s by %s: %s" % (p, m, c, route, str(exc).splitlines()[0][:300] if str(exc) else repr(exc)))
    print("%s/%s/%s by %s: %d triples in %.1f s, %d failed" % (path, kind, geom, route, len(cases), time.time() - t_start, len(failures)))
    assert not failures, "%d of %d triples differ:\n  %s\nthe list: %s" % (len(failures), len(cases), "\n  ".join(failures), cases)


def test_the_case_matrix():
    """(path, kind) pairs the rules leave out - validate never runs resident, mixed cars run on HET_PATHS only - are the
    only cases not run; their number is printed"""
    print("%d (path, kind, geometry) cases x 2 routes + %d by clone; %d (path, kind) pairs ruled out; %d + %d triples each"
          % (len(MATRIX), len(CLONE_PATHS), RULED_OUT, len(H.CASES), len(H.CLONE_CASES)))
    assert len(MATRIX) == 27 and RULED_OUT == 9


@pytest.mark.parametrize("route", ["export", "self"])
@pytest.mark.parametrize("path,kind,geom", MATRIX)
def test_transplant(path, kind, geom, route):
    run_case(path, kind, geom, route, H.CASES)


@pytest.mark.parametrize("path", CLONE_PATHS)
def test_transplant_by_clone(path):
    run_case(path, "plain", "g33", "clone", H.CLONE_CASES)
