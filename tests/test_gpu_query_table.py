"""What every device query of the engine shares (gym_traffic.core.QUERIES), checked row by row on the device: the default
tensors are made once per (query, key) and reused, every member of a caller's out= is held to the row's dtype and shape before
anything is launched, and the engine computes the same afterwards.  The same for the other checked inputs (frames(out=),
trip_stats(cursor=), demand_counts(out=), set_demand(profile_of_env=)) and for the launch reports."""
import numpy as np
import pytest

from test_gpu_clone import make

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from gym_traffic import _native as nat  # noqa: E402
from gym_traffic.core import QUERIES, CarList  # noqa: E402

E, CAP, PX, SENTINEL = 3, 64, 8, 0x5A
INF = float("inf")
TRIP_EDGES = {0: None, 1: [0, 1000], 2: [0, 40, 1000]}
CELL_EDGES = {1: [-INF, INF], 2: [-INF, 60.0, INF]}
# per row: the call as (engine, key, out) and the keys to use - the first is the one the out= checks run at (no dimension
# of 1 there: a view with a stride over such a dimension still counts as contiguous)
CALLS = dict(
    road_measures=(lambda eng, key, out: eng.road_measures(out=out), (None,)),
    road_following=(lambda eng, key, out: eng.road_following(2.0, 0.1, 3.0, out=out), (None,)),
    road_ends=(lambda eng, key, out: eng.road_ends(k=key, out=out), (2, 3)),
    car_ages=(lambda eng, key, out: eng.car_ages(out=out), (None,)),
    trip_stats=(lambda eng, key, out: eng.trip_stats(edges=TRIP_EDGES[key], out=out), (2, 1, 0)),
    road_cells=(lambda eng, key, out: eng.road_cells(CELL_EDGES[key], out=out), (2, 1)),
    car_list=(lambda eng, key, out: eng.car_list(max_cars=key, out=out), (CAP,)),
)
assert sorted(CALLS) == sorted(QUERIES)                # (a new row brings its call here)
WRONG = ("dtype", "dim", "strided", "host")


def driven(kind):
    """3 envs on the 2x2 grid, 24 roads of capacity 10, a car every 4 ticks on every entry road for 20 ticks"""
    eng = make("pertick", E, kind, m=2, n=2, capacity=10)
    assert eng.R == 24
    eng.reset(np.zeros((E, eng.I), np.int32))
    eng.set_actions(np.zeros((E, eng.I), np.int32))
    eng.set_spawns(period=4)
    eng.step(20)
    return eng


def launch_reports(eng):
    return dict(measure=eng.measure_launch(), follow=eng.follow_launch(), ends=eng.ends_launch(2), car_list=eng.car_list_launch(E),
                put=eng.put_launch(E), ages=eng.ages_launch(), cells=eng.cells_launch(2), frames=eng.frames_launch(E, PX))


@pytest.fixture(scope="module")
def engines():
    val, plain = driven("validate"), driven("plain")
    assert val.P == 3 and plain.P == 2
    cars = val.road_measures().n_cars
    assert int(cars.sum()) > 0 and bool((cars == 0).any())
    return dict(val=val, plain=plain, reports=launch_reports(val))


def wrong(form, dtype, shape, dev):
    """a tensor that misses (dtype, shape, contiguous, on the device) in exactly one way; `dim` gives one per dimension"""
    if form == "dtype":
        return [torch.zeros(shape, dtype=torch.float32 if dtype == torch.int32 else torch.int32, device=dev)]
    if form == "dim":
        return [torch.zeros(shape[:d] + (shape[d] + 1,) + shape[d + 1:], dtype=dtype, device=dev) for d in range(len(shape))]
    if form == "strided":
        t = torch.zeros(shape[:-1] + (2 * shape[-1],), dtype=dtype, device=dev)[..., ::2]
        assert tuple(t.shape) == tuple(shape) and not t.is_contiguous()
        return [t]
    return [torch.zeros(shape, dtype=dtype)]


def refused(call, dtype, shape, dev, word=None):
    """call(tensor) raises ValueError (naming `word`) for every wrong form of the tensor -> how many were tried"""
    n = 0
    for form in WRONG:
        for bad in wrong(form, dtype, tuple(shape), dev):
            with pytest.raises(ValueError) as err:
                call(bad)
            assert word is None or word in str(err.value), (form, str(err.value))
            n += 1
    return n


def valid(eng, q, key, fill=0):
    return [None if shape(eng, key) is None else torch.full(shape(eng, key), fill, dtype=dtype, device=eng.device)
            for dtype, shape, _ in q.planes]


# ---- (a) the default tensors are made once per (query, key) ---------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CALLS))
def test_cache_reuse(engines, name):
    eng, (call, keys) = engines["val"], CALLS[name]
    first = call(eng, keys[0], None)
    again = call(eng, keys[0], None)
    if name == "car_list":                                              # never cached: fresh planes per call
        assert isinstance(first, CarList) and all(a is not b for a, b in zip(first, again))
        return
    assert isinstance(first, QUERIES[name].tuple)
    assert all(a is b for a, b in zip(first, again))
    seen = {id(t) for t in first if t is not None}
    for key in keys[1:]:
        other = call(eng, key, None)
        assert all(a is b for a, b in zip(other, call(eng, key, None)))
        for field, (_, shape, _), t in zip(other._fields, QUERIES[name].planes, other):
            assert (t is None) == (shape(eng, key) is None), (field, key)
            assert t is None or (id(t) not in seen and tuple(t.shape) == shape(eng, key)), (field, key)
        seen |= {id(t) for t in other if t is not None}
    assert all(a is b for a, b in zip(first, call(eng, keys[0], None)))
    if name == "trip_stats":
        assert first.hist is not None and call(eng, 0, None).hist is None


# ---- (b), (c) every member of out= is checked before the launch; the engine computes the same afterwards -----------------
@pytest.mark.parametrize("name", sorted(CALLS))
def test_bad_out_members_are_refused(engines, name):
    eng, q, (call, keys) = engines["val"], QUERIES[name], CALLS[name]
    key, dev = keys[0], engines["val"].device
    want = [t.clone() if t is not None else None for t in call(eng, key, None)]
    watch = valid(eng, q, key, SENTINEL)
    tried = 0
    for i, (field, (dtype, shape, _)) in enumerate(zip(q.tuple._fields, q.planes)):
        def one(bad):
            call(eng, key, [bad if j == i else None for j in range(len(q.planes))])
        tried += refused(one, dtype, shape(eng, key), dev, word=field)
    assert tried == sum(3 + len(shape(eng, key)) for _, shape, _ in q.planes)
    torch.cuda.synchronize()
    for field, t in zip(q.tuple._fields, watch):
        assert bool((t == SENTINEL).all()), field
    mine = valid(eng, q, key)
    got = call(eng, key, mine)
    planes = got[2:] if name == "car_list" else got
    assert all(a is b for a, b in zip(planes, mine))
    assert len(got) == len(want)
    for field, g, w in zip(type(got)._fields, got, want):
        assert torch.equal(g, w), field
    again = call(eng, key, None)
    for field, g, w in zip(type(again)._fields, again, want):
        assert torch.equal(g, w), field


# ---- (d) the engine without a side plane -----------------------------------------------------------------------------------
def test_plain_engine(engines):
    plain = engines["plain"]
    cl = plain.car_list(max_cars=CAP)
    assert cl.spawn is None and cl.xv is not None and cl.road is not None and cl.row is not None
    with pytest.raises(ValueError) as err:
        plain.car_list(out=[None, None, None, torch.zeros((CAP,), dtype=torch.float32, device=plain.device)])
    assert "spawn" in str(err.value)
    with pytest.raises(nat.TfxError):
        plain.car_ages()
    # the caller's other planes still go through
    mine = [torch.zeros((CAP, 2), dtype=torch.float32, device=plain.device), None, None, None]
    assert torch.equal(plain.car_list(out=mine).xv, cl.xv)


# ---- (e) the other checked inputs ------------------------------------------------------------------------------------------
def test_other_checked_inputs(engines):
    val, plain = engines["val"], engines["plain"]
    dev = val.device
    H, W = val.frame_size(PX)
    picture = val.frames(px=PX).clone()
    assert refused(lambda t: val.frames(px=PX, out=t), torch.uint8, (E, H, W, 4), dev) == 7
    mine = torch.zeros((E, H, W, 4), dtype=torch.uint8, device=dev)
    assert val.frames(px=PX, out=mine) is mine and torch.equal(mine, picture)
    assert val.frames(px=PX) is val.frames(px=PX) and val.frames(px=PX) is not val.frames([0, 2], px=PX)

    stats = [t.clone() for t in val.trip_stats()[:4]]
    assert refused(lambda t: val.trip_stats(cursor=t), torch.int32, (E,), dev) == 4
    cursor = torch.zeros((E,), dtype=torch.int32, device=dev)
    assert all(torch.equal(a, b) for a, b in zip(val.trip_stats(cursor=cursor)[:4], stats))
    assert torch.equal(cursor, val.n_trips)

    plain.set_demand([[2.0]], seed=3)
    counts = plain.demand_counts(5, 4).clone()
    assert refused(lambda t: plain.demand_counts(5, 4, out=t), torch.int32, (4, E, plain.n_entry), dev) == 6
    assert refused(lambda t: plain.set_demand([[2.0]], seed=3, profile_of_env=t), torch.int32, (E,), dev) == 4
    mine = torch.zeros((4, E, plain.n_entry), dtype=torch.int32, device=dev)
    assert plain.demand_counts(5, 4, out=mine) is mine and torch.equal(mine, counts) and int(counts.sum()) > 0
    prof = torch.zeros((E,), dtype=torch.int32, device=dev)
    plain.set_demand([[2.0]], seed=3, profile_of_env=prof)
    assert plain.demand_profile is prof and torch.equal(plain.demand_counts(5, 4), counts)


# ---- (f) the launch reports -------------------------------------------------------------------------------------------------
def test_launch_reports(engines):
    now = launch_reports(engines["val"])
    assert sorted(now) == sorted(engines["reports"]) and len(now) == 8
    for name, pair in now.items():
        assert len(pair) == 2 and all(type(v) is int and v > 0 for v in pair), (name, pair)
        assert pair == engines["reports"][name], name
