"""Late clocks - the shift of the late-clock tests as data, and what can be known of it without a device.

The suite holds every step path to the oracle with the clock within a few hundred ticks of zero.  The oracle cannot be
run late (its clock is a float32 that sticks at 2^24), so tests/test_gpu_late_clock.py runs a SHIFTED TWIN instead: the
scenarios of tests/test_transplant_host.py on a handle whose every clock value is moved up by D, compared with the same
scenario at the low clock - device and oracle - under an exact integer map.  Everything that describes the shift is here:

  shift_ops(ops, D, het)   the same ops with load's tick, set_tick's `to` and the loaded spawn ticks moved by D
  ClockMap                 low-clock result -> expected late-clock result: the spawn plane, done_tick, the trip log;
                           everything else (ring words, x, v, rows, obs, rewards, waiting, passed_dst, done, a decision's
                           outputs, the vehicle updates) is unchanged
  DatedOracle              an OracleSide that knows the clock tick at which every entry of the trip log was written
  CLASSES / LATE_CASES     where the clock is (a D per prefix: start_clock - T0[prefix]) and the written-out triples

  BELOW24    the whole case ends at or below 2^24 - 1: float32 spawn ticks are still exact, the trip map is the identity
  CROSS24    the prefix's first call starts 2 to 4 ticks below 2^24 and runs up to or across it
  CROSS3x24  the same at 3 * 2^24: a second wrap of the mixed cars' 24-bit spawn ticks, and float32 ticks on a grid of 4
  TOP        the case's last tick is within 64 ticks of TFX_TICK_MAX, the end of the clock's domain (include/tfx.h)

The tests of this module run on the oracle alone and keep the device tests from passing vacuously: the lists cover what
they must, trips and live cars do straddle the boundaries, the quantised trip formula is exercised where it differs."""
import os
import re

import numpy as np
import pytest

import test_transplant_host as H
from oracle.oracle import live_mask

W24 = 1 << 24
PERIOD_MAX = 1 << 20
TICK_MAX = 0x7fffffff - PERIOD_MAX                       # TFX_TICK_MAX (test_the_constants_are_the_headers)
CLASSES = ("BELOW24", "CROSS24", "CROSS3x24", "TOP")
BOUNDARY = {"CROSS24": W24, "CROSS3x24": 3 * W24}
# how far below the boundary a prefix's first call starts: its ticks then straddle the boundary (P1-P4, P6, P7: the pair or
# the tick in the middle of the call) or end on it (P5, a two-tick call: the continuation begins exactly at the boundary)
BELOW = {"P1": 3, "P2": 3, "P3": 3, "P4": 3, "P5": 2, "P6": 3, "P7": 4}
MOST_TICKS = 32                                          # no case runs more (test_the_classes_are_where_they_say)

# every prefix, every continuation and M1, M2, M5 in every class; M0, M3 and M4 somewhere; every (prefix, mutator) pair is
# one of H.CASES, whose hand-overs the transplant module has checked
LATE_CASES = {
    "BELOW24": [("P1", "M1", "step1"), ("P2", "M2", "step2"), ("P3", "M5", "step5"), ("P4", "M0", "agent3r"),
                ("P5", "M1", "agent4"), ("P6", "M2", "halves"), ("P7", "M5", "step2")],
    "CROSS24": [("P1", "M2", "agent3r"), ("P2", "M5", "agent4"), ("P3", "M1", "halves"), ("P4", "M1", "step1"),
                ("P5", "M2", "step2"), ("P6", "M5", "step5"), ("P7", "M0", "agent3r"), ("P1", "M4", "step5")],
    "CROSS3x24": [("P1", "M5", "step5"), ("P2", "M1", "halves"), ("P3", "M2", "step1"), ("P4", "M5", "step2"),
                  ("P5", "M0", "agent3r"), ("P6", "M1", "agent4"), ("P7", "M2", "step5"), ("P2", "M3", "agent3r")],
    "TOP": [("P1", "M1", "agent4"), ("P2", "M2", "step5"), ("P3", "M5", "agent3r"), ("P4", "M2", "halves"),
            ("P5", "M5", "step1"), ("P6", "M1", "step2"), ("P7", "M1", "step5"), ("P3", "M0", "step2")],
}


def start_clock(cls, prefix):
    """the clock the prefix's first call of a case of this class starts at"""
    if cls == "BELOW24":
        return W24 - 1 - 2 * MOST_TICKS
    if cls in BOUNDARY:
        return BOUNDARY[cls] - BELOW[prefix]
    return TICK_MAX - MOST_TICKS - 8


def shift_of(cls, prefix):
    return start_clock(cls, prefix) - H.T0[prefix]


# ---- the shift -------------------------------------------------------------------------------------------------------------
def _ticks_of(w):
    """a low-clock spawn plane as integers (they are: spawn ticks below 2^24 are exact in float32)"""
    wi = np.asarray(w).astype(np.int64)
    assert np.array_equal(wi.astype(np.float32), np.asarray(w, np.float32)), "a spawn tick that is no integer"
    return wi


def shift_w(w, D, het):
    """Spawn ticks moved by D as integers, then as the handle keeps them: float32(w + D), ONE rounding to nearest even
    as v_cvt_f32_i32 does (int64 -> float32 rounds the same way), on single-archetype handles; (w + D) mod 2^24 - always
    exact in float32 - on heterogeneous ones."""
    wi = _ticks_of(w) + int(D)
    return (wi % W24).astype(np.float32) if het else wi.astype(np.float32)


def shift_ops(ops, D, het):
    """the same ops with every clock value moved by D"""
    out = []
    for op in ops:
        op = dict(op)
        if op["op"] == "load":
            op["tick"] = op["tick"] + D
            op["w"] = shift_w(op["w"], D, het)
        elif op["op"] == "set_tick" and "to" in op:
            op["to"] = op["to"] + D
        out.append(op)
    return out


class ClockMap(object):
    """low-clock result -> expected late-clock result, in exact integer arithmetic.  pops: per env the clock tick (low) at
    which each entry of the trip log was written (DatedOracle.pop); first: per env the entry from which the log was written
    at the late clock (state that came over from a low clock brings its log as it is), None: all of it."""

    def __init__(self, D, het, pops=None, first=None):
        self.D, self.het, self.pops, self.first = int(D), het, pops, first

    def w(self, w_low):
        return shift_w(w_low, self.D, self.het)

    def stamp(self, s):
        s = np.asarray(s, np.int64)
        return np.where(s != 0, s + self.D, 0)

    def trips(self, k, low):
        """(float32(pop + D) - float32(spawn + D)) / 2 in float32 with spawn = pop - 2 * trip_low; unchanged on
        heterogeneous handles (tick differences modulo 2^24)"""
        low = np.asarray(low, np.float32)
        if self.het or len(low) == 0 or (self.first is not None and int(self.first[k]) >= len(low)):
            return low
        pop = np.asarray(self.pops[k][:len(low)], np.int64)
        assert len(pop) == len(low), ("the oracle dated %d of env %d's %d trips" % (len(pop), k, len(low)))
        spawn = pop - _ticks_of(low * np.float32(2))
        late = ((pop + self.D).astype(np.float32) - (spawn + self.D).astype(np.float32)) / np.float32(2)
        if self.first is not None:
            late[:int(self.first[k])] = low[:int(self.first[k])]
        return late

    def spawn_of(self, k, low):
        pop = np.asarray(self.pops[k][:len(low)], np.int64)
        return pop - _ticks_of(np.asarray(low, np.float32) * np.float32(2)), pop


class DatedOracle(H.OracleSide):
    """an OracleSide that records, for every entry of every env's trip log, the clock of the tick that wrote it"""

    def __init__(self, world):
        super(DatedOracle, self).__init__(world)
        self.pop = [[] for _ in range(world.E)]
        self.on_tick = self._date

    def _date(self, clock):
        for k, n in enumerate(self.orc.n_trips.tolist()):
            p = self.pop[k]
            del p[n:]
            p.extend([clock] * (n - len(p)))

    def _load(self, op):
        super(DatedOracle, self)._load(op)
        self.pop = [[] for _ in range(self.w.E)]            # (the log starts anew: n_trips is cleared)

    def _reset_envs(self, op):
        super(DatedOracle, self)._reset_envs(op)
        for k, n in enumerate(self.orc.n_trips.tolist()):
            del self.pop[k][n:]

    def _clone(self, op):
        super(DatedOracle, self)._clone(op)
        for k in np.nonzero(op["src"] >= 0)[0]:
            self.pop[k] = list(self.pop[op["src"][k]])

    def dated(self):
        """a copy of the dates, for a map that outlives further ticks"""
        return [list(p) for p in self.pop]


def case_ops(geom, triple):
    p, m, c = triple
    return H.prefix_ops(geom, p), H.mutator_ops(geom, m, p), H.cont_ops(geom, c)


# ---- what can be known without a device ------------------------------------------------------------------------------------------
def test_the_constants_are_the_headers():
    text = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "tfx.h")).read()
    assert re.search(r"#define TFX_PERIOD_MAX \(1 << 20\)", text)
    assert re.search(r"#define TFX_TICK_MAX \(0x7fffffff - TFX_PERIOD_MAX\)", text)
    from gym_traffic import _native as nat
    assert nat.TICK_MAX == TICK_MAX and nat.PERIOD_MAX == PERIOD_MAX
    # the largest sum of the header's derivation stays an int32
    assert TICK_MAX + PERIOD_MAX - 1 <= 0x7fffffff and TICK_MAX + 2 <= 0x7fffffff


def test_late_case_lists_cover_what_they_must():
    for cls in CLASSES:
        cases = LATE_CASES[cls]
        assert len(cases) == len(set(cases)) and 7 <= len(cases) <= 8, cls
        assert {p for p, _, _ in cases} == set(H.PREFIXES), cls
        assert {c for _, _, c in cases} == set(H.CONTS), cls
        assert {"M1", "M2", "M5"} <= {m for _, m, _ in cases}, cls
        assert {(p, m) for p, m, _ in cases} <= {(p, m) for p, m, _ in H.CASES}, cls
    assert {m for cls in CLASSES for _, m, _ in LATE_CASES[cls]} == set(H.MUTATORS)


def test_shift_is_exact():
    rng = np.random.RandomState(1)
    w = rng.randint(0, 50, size=1000).astype(np.float32)
    for D in (0, W24 - 70, W24 - 3, 3 * W24 - 63, TICK_MAX - 100):
        want = np.array([float(np.float32(int(t) + D)) for t in w])          # Python int -> binary64 (exact) -> float32
        assert np.array_equal(shift_w(w, D, False).astype(np.float64), want), D
        assert np.array_equal(shift_w(w, D, True), np.array([(int(t) + D) % W24 for t in w], np.float32)), D
    # ties go to even: 2^24 + 1 -> 2^24, 2^24 + 3 -> 2^24 + 4
    assert shift_w(np.float32([1, 3]), W24, False).tolist() == [float(W24), float(W24 + 4)]
    m = ClockMap(5, False)
    assert m.stamp(np.array([0, 1, 77])).tolist() == [0, 6, 82]
    ops = [dict(op="load", tick=60, w=np.float32([3, 4])), dict(op="set_tick", to=60), dict(op="set_tick", rel=1), dict(op="halves")]
    got = shift_ops(ops, 100, True)
    assert got[0]["tick"] == 160 and got[0]["w"].tolist() == [103.0, 104.0] and got[1]["to"] == 160 and got[2] == ops[2]
    assert ops[0]["tick"] == 60 and ops[0]["w"].tolist() == [3.0, 4.0]          # (the low ops are left as they were)


def rebase_cases():
    """tests/golden/regress/rebase_rounds_once.json: (spawn, shift, want) - float32(spawn + shift) with ONE rounding"""
    import json
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "regress", "rebase_rounds_once.json")
    return json.load(open(path))["cases"]


def test_rebase_rounds_once_in_the_numpy_definition():
    """devrng.put_cars, the NumPy statement of tfx_put_cars: a spawn_shift float32 does not hold is added with one rounding
    (the record holds ten cases in which wa + (float)shift rounds twice and ends 2 to 128 ticks off)"""
    from gym_traffic import devrng
    cases = rebase_cases()
    assert sum(c["want"] != c["rounded_twice"] for c in cases) >= 10
    Cc = 6
    for c in cases:
        assert c["want"] == int(np.float32(c["spawn"] + c["shift"])) == int(shift_w(np.float32([c["spawn"]]), c["shift"], False)[0])
        z = np.zeros((1, 1, Cc), np.float32)
        out = devrng.put_cars(z, z, z, None, np.ones((1, 1), np.int32), np.ones((1, 1), np.int32), Cc, np.array([0, 1]),
                              np.float32([[5.0, 1.0]]), None, np.float32([c["spawn"]]), spawn_shift=c["shift"])
        assert int(out[2][0, 0, 2]) == c["want"], c


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("geom", sorted(H.GEOMS))
def test_the_classes_are_where_they_say(geom, cls):
    """the clocks a case of the class runs through, from the ops alone"""
    for triple in LATE_CASES[cls]:
        p = triple[0]
        D = shift_of(cls, p)
        side = DatedOracle(H.World(geom, "plain"))
        pre, mut, cont = case_ops(geom, triple)
        first_call = next(op for op in pre if op["op"] in ("step", "agent"))
        side.run(pre)
        top = side.tick
        side.run(mut).run(cont)
        top = max(top, side.tick)
        assert top - H.T0[p] <= MOST_TICKS, (triple, top)
        assert D >= 0 and H.T0[p] + D >= 0 and top + D <= TICK_MAX, (cls, triple)
        if cls == "BELOW24":
            assert top + D <= W24 - 1, (triple, top + D)
        elif cls in BOUNDARY:
            t0 = H.T0[p] + D
            assert 2 <= BOUNDARY[cls] - t0 <= 8 and t0 + first_call["n"] >= BOUNDARY[cls], (triple, t0)
            assert top + D > BOUNDARY[cls], (triple, top + D)
        else:
            assert TICK_MAX - 64 <= side.tick + D <= TICK_MAX, (triple, side.tick + D)


@pytest.mark.parametrize("kind", ["validate", "het"])
@pytest.mark.parametrize("geom", sorted(H.GEOMS))
def test_late_cases_are_not_vacuous(geom, kind):
    """With the oracle alone, per class: trips that begin before the boundary and end at or behind it; live cars at the
    end whose shifted spawn tick lies on the other side of the boundary from the clock; on single-archetype handles trip
    times that the float32 formula changes at 3 * 2^24 (and at the top), none that it changes below 2^24; after P4 an env
    with an overflow stamp and one without; at least half of the envs live at every hand-over."""
    w = H.World(geom, kind)
    for cls in CLASSES:
        crossing = wrapped = changed = trips = 0
        for triple in LATE_CASES[cls]:
            p, m, c = triple
            D = shift_of(cls, p)
            B = BOUNDARY.get(cls)
            pre, mut, cont = case_ops(geom, triple)
            side = DatedOracle(w).run(pre)
            if p == "P4":
                stamped = side.done.astype(bool)              # (the decision's overflows: done_tick = tick + 1 + D != 0 there)
                assert stamped.any() and not stamped.all(), (cls, triple)
            side.run(mut)
            assert 2 * H.live_envs(side.done) >= w.E, ("live at the hand-over", cls, triple, side.done)
            side.run(cont)
            cmap = ClockMap(D, w.het, side.dated())
            o = side.orc
            for k in range(w.E):
                n = int(o.n_trips[k])
                assert n <= o.trip_cap
                low = o.trip_times[k, :n]
                spawn, pop = cmap.spawn_of(k, low)
                trips += n
                late = ClockMap(D, False, cmap.pops).trips(k, low)       # (the single-archetype formula, whatever the kind)
                if cls == "BELOW24":
                    assert np.array_equal(late, low), ("the trip map is the identity below 2^24", triple, k)
                changed += int((late != low).sum())
                if B is not None:
                    crossing += int(((spawn + D < B) & (pop + D >= B)).sum())
                    live = live_mask(o.leading[k], o.lastcar[k], o.C)
                    born = _ticks_of(o.planes(k)[2][live]) + D
                    wrapped += int(((born < B) != (side.tick + D < B)).sum())
        print("%s/%s %s: %d trips, %d begin before the boundary and end behind it, %d live cars across the boundary from "
              "the clock, %d trip times the float32 formula changes" % (geom, kind, cls, trips, crossing, wrapped, changed))
        assert trips > 0, cls
        if cls in BOUNDARY:
            assert crossing >= 1 and wrapped >= 1, (cls, crossing, wrapped)
        if cls in ("CROSS3x24", "TOP"):
            assert changed >= 1, (cls, "the quantised formula is not exercised")
        if cls == "BELOW24":
            assert changed == 0
