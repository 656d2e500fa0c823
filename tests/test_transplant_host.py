"""Used handles must equal fresh ones - the scenario builder of the transplant tests, and what can be known of it
without a device.

The contract (include/tfx.h): what a handle computes next depends only on what the caller can see - the ring
image, the bound buffers, the clock - and on its inputs.  tests/test_gpu_transplant.py runs a PREFIX that leaves residue
in a handle, optionally a MUTATOR, hands the caller-visible state to a fresh handle and runs the same CONTINUATION on
both.  Everything that describes those runs lives here, as plain data (lists of ops) that any side can execute:
OracleSide below (the checker, oracle/idm_oracle.c) and the device side of the GPU module.

  prefixes       P1 a call that ends on a two-tick pass            P5 a last tick that pops more than TFX_KP cars of a road
                 P2 pairs, then an odd last tick                   P6 a call long enough to split, then a one-tick call
                 P3 two remi decisions, risky envs in disjoint     P7 a call long enough for k_res, then one too short
                    halves of the batch, 5 pairs apart                (TFX_RES_MIN_TICKS=3 while P7 runs)
                 P4 a decision in which some envs overflow
  mutators       M0 none   M1 set_tick back to the prefix's first tick   M2 set_tick(tick + 1)   M3 reset_envs of every
                 other env   M4 the tail car of some roads dropped through lastcar + refresh(cars=False)   M5 an in-place
                 clone of a third of the envs
  continuations  step(1), step(2), step(5), agent_step(3, remi), agent_step(4, no remi), move_cars + advance_finished_cars

CASES is the written-out list of triples every (path, kind, route) case runs: every prefix with every continuation, every
mutator with every continuation, every prefix with every mutator (test_case_list_covers_every_pair), plus the pairings
two seeded value-only defects need (k_refresh taking the tail from row n - 1 of a column that starts lower; tfx_set_tick
keeping the overflow stamps).  The tests of this module run on the oracle alone: the prefixes leave what
they are meant to leave, at least half of the envs are live at every hand-over, and the oracle itself has the property -
an OracleEnv loaded from another's exported state continues bit for bit, validate mode and mixed rows included."""
import functools
import zlib

import numpy as np
import pytest

from oracle.oracle import OracleEnv, live_mask
from oracle.ring_states import random_state
from test_gpu_parity import same_bits
from test_gpu_clone import ARCH                       # (v, l, a, delta, v0, b, T, s0: the table of the `het` handles)
from test_gpu_stride_rounds import ORC_FIELDS, csr, emulate_decision, grid_tables, ragged_state, rows_of, tab10_of

# the smallest shapes that have the structure: the stale-stamp test's grid (a forced split is 6 + 6 envs), and one with
# two tiles per env (R = 80) whose halves are 2 and 3 envs - a tile boundary and an uneven split inside the batch
GEOMS = {"g33": dict(m=3, n=3, length=200.0, capacity=20, rate=0.5, E=12),
         "g44": dict(m=4, n=4, length=120.0, capacity=14, rate=0.5, E=5)}
KINDS = ("plain", "validate", "het")
ROWS_PER_ROAD = 2       # S of the spawn-row buffers: no road receives more cars in a tick here

PREFIXES = ("P1", "P2", "P3", "P4", "P5", "P6", "P7")
MUTATORS = ("M0", "M1", "M2", "M3", "M4", "M5")
CONTS = ("step1", "step2", "step5", "agent3r", "agent4", "halves")
# the clock a prefix starts at: behind every spawn tick of the loaded cars (0..49) - a car from the future is no state of
# the model (mixed cars keep the spawn tick modulo 2^24: a negative trip time would not even have one meaning)
T0 = {"P1": 60, "P2": 60, "P3": 60, "P4": 70, "P5": 50, "P6": 60, "P7": 60}
CLEAR = ("P1", "P2", "P6", "P7")                                                 # prefixes without an overflow

# prefix -> the mutator (its digit) that goes with each continuation, in CONTS' order
_GRID = {"P1": "012345", "P2": "123450", "P3": "234501", "P4": "345012", "P5": "450123", "P6": "501234", "P7": "012345"}
# what the grid leaves thin: columns that start a row or two down when the tails are rebuilt (P1 x M4), stamps of the
# risk bound, of overflows and of the serial advance under a clock that was set back (P3, P4, P5 x M1)
_EXTRA = [("P1", "M4", c) for c in CONTS] + [("P3", "M1", c) for c in ("step2", "step5", "agent3r", "agent4")] + \
         [("P4", "M1", c) for c in ("step1", "agent3r", "agent4")] + [("P5", "M1", "step2"), ("P5", "M1", "agent4")]
CASES = []
for _p in PREFIXES:
    for _c, _m in zip(CONTS, _GRID[_p]):
        CASES.append((_p, "M" + _m, _c))
for _t in _EXTRA:
    if _t not in CASES:
        CASES.append(_t)
# the route through tfx_clone_envs hands on what the caller cannot export; it needs fewer cases
CLONE_CASES = [(p, m, c) for p in ("P1", "P3", "P6") for m in ("M0", "M2") for c in CONTS]


class World(object):
    """One geometry and one kind of handle (tests/test_gpu_clone.py:make): plain; validate - the spawn ticks and the
    trip log; het - validate with the three-row table ARCH"""

    def __init__(self, geom, kind):
        self.geom, self.kind = geom, kind
        g = GEOMS[geom]
        self.m, self.n, self.length, self.C, self.rate, self.E = g["m"], g["n"], g["length"], g["capacity"], g["rate"], g["E"]
        self.dest, self.phases, self.nexts, self.entry = grid_tables(self.m, self.n)
        self.I = self.m * self.n
        self.r = 4 * self.I
        self.R = len(self.dest)
        self.n_entry = len(self.entry)
        self.validate, self.het = kind != "plain", kind == "het"
        self.tab10 = tab10_of(ARCH) if self.het else None

    def oracle(self):
        orc = OracleEnv(self.m, self.n, self.length, self.C, self.dest, self.phases, self.nexts, n_envs=self.E,
                        rate=self.rate, validate=self.validate)
        orc.entrypoints = self.entry
        return orc


# ---- the scenarios, as data ------------------------------------------------------------------------------------------------
def _rng(geom, item):
    return np.random.RandomState(zlib.crc32(("%s/%s" % (geom, item)).encode()) & 0x7FFFFFFF)


def _calm(rng, w):
    """ordinary traffic: a third of every ring, cars up to the road end, no full ring"""
    return ragged_state(rng, w.E, w.R, w.C, w.length, crowd=0.3, beyond=0.05, sorted_x=True, full="none")


def _wild(rng, w, envs):
    """the pathological family (oracle/ring_states.py) in `envs` - risky for sure -, ordinary traffic everywhere else"""
    wild = random_state(rng, w.E, w.R, w.C, w.length, crowd=0.9, beyond=1.6, sorted_x=False)
    calm = _calm(rng, w)
    pick = np.zeros(w.E, bool)
    pick[envs] = True
    return tuple(np.where(pick.reshape((-1,) + (1,) * (a.ndim - 1)), a, b) for a, b in zip(wild, calm))


def _popping(rng, w):
    """tests/test_gpu_pairs.py:test_second_tick_pops_more_than_the_outbox_holds: unsorted columns - a head just short of
    the road end with cars BEYOND the end queued behind it; in the second tick the head leaves and takes the run with it.
    The first half of the envs keeps every ring short enough to take such a run (they stay live), the others have the full
    rings of that test."""
    E, R, C, length = w.E, w.R, w.C, w.length
    x, v, wt = np.zeros((E, R, C), np.float32), np.zeros((E, R, C), np.float32), np.zeros((E, R, C), np.float32)
    leading = rng.randint(1, C, size=(E, R)).astype(np.int32)
    lastcar = leading.copy()
    for k in range(E):
        roomy = k < (E + 1) // 2
        for e in range(R):
            kind = rng.randint(3)
            if roomy:
                cnt = int(rng.randint(3, C - 7))
            else:
                cnt = C - 2 if kind == 0 else int(rng.randint(3, C - 2))
            s = int(leading[k, e])
            for j in range(cnt):
                s = s + 1 if s + 1 < C else 1
                if kind == 1 and j == 0:
                    x[k, e, s], v[k, e, s] = length - 3.0, 4.0
                elif kind == 1 and j <= 4:
                    x[k, e, s], v[k, e, s] = length + 10.0 * j, 0.0
                else:
                    x[k, e, s] = length - 12.0 - 5.5 * j
                    v[k, e, s] = rng.uniform(0.0, 6.0)
                wt[k, e, s] = rng.randint(0, 9)
            lastcar[k, e] = s
            x[k, e, leading[k, e]] = np.inf
    return x, v, wt, leading, lastcar


def _load(rng, w, state, tick, reset=True, elapsed=(0, 12)):
    x, v, wt, leading, lastcar = state
    return dict(op="load", reset=reset, x=x, v=v, w=wt, leading=leading, lastcar=lastcar, tick=tick,
                arch=rng.randint(0, len(ARCH), size=x.shape).astype(np.uint8),
                phase=rng.randint(2, size=(w.E, w.I)).astype(np.int32),
                elapsed=rng.randint(elapsed[0], elapsed[1], size=(w.E, w.I)).astype(np.int32))


def _arrivals(rng, w, n):
    cnt = (rng.rand(n, w.E, w.n_entry) < 0.2).astype(np.int32) * rng.randint(1, ROWS_PER_ROAD + 1, size=(n, w.E, w.n_entry))
    return cnt.astype(np.int32), rng.randint(0, len(ARCH), size=(n, w.E, w.n_entry, ROWS_PER_ROAD)).astype(np.uint8)


def _step(rng, w, n):
    cnt, rows = _arrivals(rng, w, n)
    return dict(op="step", n=n, acts=rng.randint(2, size=(n, w.E, w.I)).astype(np.int32), cnt=cnt, rows=rows)


def _agent(rng, w, n, remi):
    cnt, rows = _arrivals(rng, w, n)
    return dict(op="agent", n=n, remi=remi, act=rng.randint(2, size=(w.E, w.I)).astype(np.int32), cnt=cnt, rows=rows)


@functools.lru_cache(maxsize=None)
def prefix_ops(geom, name):
    """(the geometry's part of a World is all that shapes the data: every kind of handle runs the same scenario)"""
    w, rng, t0 = World(geom, "plain"), _rng(geom, name), T0[name]
    E = w.E
    if name == "P1":
        return [_load(rng, w, _calm(rng, w), t0), _step(rng, w, 4)]
    if name == "P2":
        return [_load(rng, w, _calm(rng, w), t0), _step(rng, w, 4), _step(rng, w, 3)]
    if name == "P3":
        # two decisions of two pairs each, five pairs apart: pair p of a call stamps plane p & 1 of env_risk and word
        # p & 1 of risk_any, so both planes and both words carry stamps of both decisions' envs afterwards
        first, second = np.arange(0, E // 2), np.arange(E - E // 2, E)
        return [_load(rng, w, _wild(rng, w, first), t0), _agent(rng, w, 4, True),
                _load(rng, w, _wild(rng, w, second), t0 + 10, reset=False), _agent(rng, w, 4, True)]
    if name == "P4":
        return [_load(rng, w, _wild(rng, w, np.arange(0, E, 3)), t0), _agent(rng, w, 4, False)]
    if name == "P5":
        load = _load(rng, w, _popping(rng, w), t0, elapsed=(6, 12))      # (past yellow: half the lights are green)
        held = dict(op="step", n=2, acts=np.repeat(load["phase"][None], 2, 0), cnt=np.zeros((2, E, w.n_entry), np.int32),
                    rows=np.zeros((2, E, w.n_entry, ROWS_PER_ROAD), np.uint8))
        return [load, held]
    if name == "P6":
        return [_load(rng, w, _calm(rng, w), t0), _step(rng, w, 4), _step(rng, w, 1)]
    if name == "P7":
        return [_load(rng, w, _calm(rng, w), t0), _step(rng, w, 5), _step(rng, w, 2)]
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def mutator_ops(geom, name, prefix):
    w, rng = World(geom, "plain"), _rng(geom, name)
    E = w.E
    if name == "M0":
        return []
    if name == "M1":
        return [dict(op="set_tick", to=T0[prefix])]
    if name == "M2":
        return [dict(op="set_tick", rel=1)]
    if name == "M3":
        return [dict(op="reset_envs", mask=(np.arange(E) % 2 == 1).astype(np.uint8),
                     phase=rng.randint(2, size=(E, w.I)).astype(np.int32))]
    if name == "M4":
        return [dict(op="drop_tail", pick=rng.rand(E, w.R) < 0.12)]
    if name == "M5":
        # env 3j + 2 becomes env 3j + 1: no source is itself overwritten
        return [dict(op="clone", src=np.where(np.arange(E) % 3 == 2, np.arange(E) - 1, -1).astype(np.int32))]
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def cont_ops(geom, name):
    w, rng = World(geom, "plain"), _rng(geom, name)
    if name.startswith("step"):
        return [_step(rng, w, int(name[4:]))]
    if name == "agent3r":
        return [_agent(rng, w, 3, True)]
    if name == "agent4":
        return [_agent(rng, w, 4, False)]
    if name == "halves":
        return [dict(op="halves")]
    raise KeyError(name)


def dropped_tails(leading, lastcar, pick, C):
    """M4: lastcar with the tail car of the picked roads that hold a car taken off (the ring runs over the slots 1..C-1)"""
    has = pick & (leading != lastcar)
    return np.where(has, np.where(lastcar > 1, lastcar - 1, C - 1), lastcar).astype(np.int32)


# ---- the checker's side ------------------------------------------------------------------------------------------------------
class OracleSide(object):
    """A batched OracleEnv that executes the ops; `done`: the envs that overflowed in the last call (what the engine's
    `done` holds), `ever`: in any call so far, `pops`: the most cars one road handed on, per tick run so far.  on_tick:
    called behind every tick the oracle runs, with the clock that tick ran at (tests/test_late_clock_host.py dates the
    trip log with it)."""

    def __init__(self, world):
        self.w, self.orc = world, world.oracle()
        self.tick = 0
        self.done = np.zeros(world.E, np.uint8)
        self.ever = np.zeros(world.E, bool)
        self.pops = []
        self.outs = None
        self.on_tick = None

    def run(self, ops):
        for op in ops:
            getattr(self, "_" + op["op"])(op)
        return self

    def _load(self, op):
        o, w = self.orc, self.w
        if op["reset"]:
            o.reset(op["phase"])
            self.done[:] = 0
        for k in range(w.E):
            o.load_planes(k, op["x"][k], op["v"][k], op["w"][k], op["leading"][k], op["lastcar"][k],
                          arch=op["arch"][k] if w.het else None, archetypes=w.tab10)
        o.obs[:] = 0
        o.current_phase[:] = op["phase"]
        o.elapsed[:] = op["elapsed"]
        o.waiting[:] = 0
        o.passed_dst[:] = 0
        o.rewards[:] = 0
        o.n_trips[:] = 0
        self.tick = op["tick"]

    def _tick(self, act, cnt, rows):
        o, w = self.orc, self.w
        o.steps[:] = self.tick                            # (batched envs share one clock on the device)
        off, roads = csr(cnt, w.entry)
        done = o.step(act, (off, roads), spawn_arch=rows_of(cnt, rows, off) if w.het else None, archetypes=w.tab10)[2]
        self.pops.append(int(o.passed.max()))
        if self.on_tick is not None:
            self.on_tick(self.tick)
        self.tick += 1
        return done.astype(bool)

    def _step(self, op):
        done = np.zeros(self.w.E, bool)
        for t in range(op["n"]):
            done |= self._tick(op["acts"][t], op["cnt"][t], op["rows"][t])
        self._called(done)

    def _halves(self, op):
        # tfx_move_cars + tfx_advance_finished_cars under the phases as they stand and without arrivals: one tick whose
        # action changes no light (idm_oracle.c:orc_step_arch is the same composition)
        w = self.w
        self._called(self._tick(self.orc.current_phase.copy(), np.zeros((w.E, w.n_entry), np.int32),
                                np.zeros((w.E, w.n_entry, ROWS_PER_ROAD), np.uint8)))

    def _agent(self, op):
        w = self.w

        def arrivals(t, frozen):                          # (asked for when tick t begins: tick t - 1 is through)
            if t > 0 and self.on_tick is not None:
                self.on_tick(self.tick + t - 1)
            return op["cnt"][t], op["rows"][t] if w.het else None

        aobs, arew, adone, _ = emulate_decision(self.orc, self.tick, op["act"], arrivals, op["n"], op["remi"], w.tab10)
        self.tick += op["n"]
        if self.on_tick is not None:
            self.on_tick(self.tick - 1)
        self.outs = (aobs, arew, adone)
        self._called(adone.astype(bool))

    def _called(self, done):
        self.done = done.astype(np.uint8)
        self.ever |= done

    def _set_tick(self, op):
        self.tick = op["to"] if "to" in op else self.tick + op["rel"]

    def _reset_envs(self, op):
        o = self.orc
        m = op["mask"].astype(bool)
        keep = [getattr(o, f)[~m].copy() for f in ORC_FIELDS]
        o.reset(op["phase"])
        for f, a in zip(ORC_FIELDS, keep):
            getattr(o, f)[~m] = a
        self.done[m] = 0

    def _drop_tail(self, op):
        o = self.orc
        new = dropped_tails(o.leading, o.lastcar, op["pick"], self.w.C)
        k, e = np.nonzero(new != o.lastcar)
        o.state[k, e, :, o.lastcar[k, e]] = 0             # (the slot is dead now)
        o.lastcar[:] = new

    def _clone(self, op):
        o = self.orc
        dst = np.nonzero(op["src"] >= 0)[0]
        for f in ORC_FIELDS:
            getattr(o, f)[dst] = getattr(o, f)[op["src"][dst]]
        self.done[dst] = self.done[op["src"][dst]]

    # what the caller of a device handle could export, and its import into a side that has done nothing else
    def export(self):
        o, w = self.orc, self.w
        planes = [o.planes(k) for k in range(w.E)]
        s = dict(x=np.stack([p[0] for p in planes]), v=np.stack([p[1] for p in planes]), w=np.stack([p[2] for p in planes]),
                 arch=np.stack([o.arch_plane(k, w.tab10) for k in range(w.E)]).astype(np.uint8) if w.het else None,
                 tick=self.tick, done=self.done.copy())
        for f in ORC_FIELDS[1:]:
            s[f] = getattr(o, f).copy()
        return s

    def load(self, s):
        o, w = self.orc, self.w
        for k in range(w.E):
            o.load_planes(k, s["x"][k], s["v"][k], s["w"][k], s["leading"][k], s["lastcar"][k],
                          arch=s["arch"][k] if w.het else None, archetypes=w.tab10)
        for f in ORC_FIELDS[3:]:
            getattr(o, f)[:] = s[f]
        self.tick, self.done = s["tick"], s["done"].copy()
        return self


def assert_sides_equal(a, b, where):
    """two OracleSides: integers exact, floats bit for bit, every live car with all ten of its parameters"""
    oa, ob = a.orc, b.orc
    assert a.tick == b.tick and np.array_equal(a.done, b.done), where
    for f in ("leading", "lastcar", "obs", "waiting", "passed_dst", "n_trips"):
        assert np.array_equal(getattr(oa, f), getattr(ob, f)), (f, where)
    assert same_bits(oa.rewards, ob.rewards), ("rewards", where)
    for k in range(oa.E):
        live = live_mask(oa.leading[k], oa.lastcar[k], oa.C)
        for p in range(oa.state.shape[2]):
            assert same_bits(oa.state[k, :, p, :][live], ob.state[k, :, p, :][live]), ("car parameter %d" % p, k, where)
        n = min(int(oa.n_trips[k]), oa.trip_cap)
        assert same_bits(oa.trip_times[k, :n], ob.trip_times[k, :n]), ("trip_times", k, where)
    if a.outs is not None or b.outs is not None:
        for u, v in zip(a.outs, b.outs):
            assert same_bits(u, v) if u.dtype == np.float32 else np.array_equal(u, v), ("decision", where)


def live_envs(side_done):
    return int((np.asarray(side_done) == 0).sum())


def _used(geom, kind, prefix):
    """a side that has run the prefix: the USED oracle of a triple (run anew for every one of them)"""
    return OracleSide(World(geom, kind)).run(prefix_ops(geom, prefix))


# ---- what can be known without a device ------------------------------------------------------------------------------------------
def test_case_list_covers_every_pair():
    assert len(CASES) == len(set(CASES)) and 42 <= len(CASES) <= 60
    assert {(p, c) for p, _, c in CASES} == {(p, c) for p in PREFIXES for c in CONTS}
    assert {(m, c) for _, m, c in CASES} == {(m, c) for m in MUTATORS for c in CONTS}
    assert {(p, m) for p, m, _ in CASES} == {(p, m) for p in PREFIXES for m in MUTATORS}
    assert set(CLONE_CASES) == {(p, m, c) for p in ("P1", "P3", "P6") for m in ("M0", "M2") for c in CONTS}


@pytest.mark.parametrize("geom", sorted(GEOMS))
def test_grid_tables_are_a_grid(geom):
    w = World(geom, "plain")
    assert w.R == 4 * w.I + 2 * w.m + 2 * w.n and w.n_entry == 2 * w.m + 2 * w.n
    assert sorted(w.nexts[w.nexts >= 0].tolist()) == sorted(set(range(w.R)) - set(w.entry.tolist()))
    assert (w.nexts[w.r:] == -1).all() and (w.dest[:w.r] >= 0).all()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("geom", sorted(GEOMS))
def test_prefixes_leave_what_they_are_meant_to(geom, kind):
    w = World(geom, kind)
    for p in PREFIXES:
        side = _used(geom, kind, p)
        ever, pops, outs = side.ever, side.pops, side.outs
        if p in CLEAR:
            assert not ever.any(), (p, "overflowed", np.nonzero(ever)[0])
        if p == "P4":
            adone = outs[2].astype(bool)
            assert adone.any() and not adone.all(), (p, adone)
        if p == "P5":
            assert pops[-1] > 2, (p, pops)             # more than TFX_KP cars of one road in the prefix's last tick
        if p == "P3":
            assert ever[:w.E // 2].any() and ever[w.E - w.E // 2:].any(), (p, ever)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("geom", sorted(GEOMS))
def test_half_of_the_envs_live_and_the_oracle_transplants(geom, kind):
    """Every triple: a side runs the prefix and the mutator - at least half of its envs are not done then - and goes on
    itself; a second side, which has done nothing else, is loaded from its export.  Both run the continuation: equal bit
    for bit, so nothing the oracle keeps outside the export (slots a popped car left, dead slots, its clock) bears on what
    it computes next."""
    w = World(geom, kind)
    for p, m, c in CASES:
        where = (geom, kind, p, m, c)
        a = _used(geom, kind, p).run(mutator_ops(geom, m, p))
        assert 2 * live_envs(a.done) >= w.E, ("live at the hand-over", where, a.done)
        b = OracleSide(w).load(a.export())
        a.outs = None                                      # (a decision of the prefix is no output of the continuation)
        assert_sides_equal(a, b, ("at the hand-over",) + where)
        a.run(cont_ops(geom, c))
        b.run(cont_ops(geom, c))
        assert_sides_equal(a, b, where)
