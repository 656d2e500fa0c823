"""The table of the engine's device queries (gym_traffic.core.QUERIES) against include/tfx.h, without a GPU: every struct of
output planes in the header has a row, and the row's namedtuple, ctypes struct, element types and shapes are the header's.
A torch dtype that is not the C member's element type would let a kernel write past a tensor and pass every other host
test."""
import re
import types

import pytest
import torch

from test_measures_host import HEADER

from gym_traffic import core

# the C struct each row fills
STRUCT_OF = dict(road_measures="tfx_measure_buffers", road_cells="tfx_cell_buffers", car_ages="tfx_age_buffers",
                 trip_stats="tfx_trip_stat_buffers", road_following="tfx_follow_buffers", road_ends="tfx_ends_buffers",
                 car_list="tfx_car_list_buffers")
DTYPE_OF = {"float": torch.float32, "int32_t": torch.int32, "int64_t": torch.int64, "uint8_t": torch.uint8}
# an engine and a key with sizes that differ from each other and from every literal dimension
ENGINE = types.SimpleNamespace(E=3, R=5, P=3)
KEY = 7
DIMS = dict(E=ENGINE.E, R=ENGINE.R, k=KEY, n_cells=KEY, n_bins=KEY)


def header_structs():
    """{name: [(element type, member, comment or None)]} of every `tfx_*_buffers` struct whose members are all pointers the
    library writes through (no const, no scalar member) and that a call takes as its `out` argument"""
    text = open(HEADER).read()
    calls = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    found = {}
    for body, name in re.findall(r"typedef struct(?: \w+)? \{([^{}]*)\} (tfx_\w+_buffers);", text, re.S):
        members = re.findall(r"([^;/]+);[ \t]*(?:/\*(.*?)\*/)?", body, re.S)
        decl = [re.fullmatch(r"\s*(\w+)\s*\*\s*(\w+)\s*", d) for d, _ in members]
        if all(decl) and re.search(r"const\s+%s\s*\*\s*out\b" % name, calls):
            found[name] = [(m.group(1), m.group(2), c or None) for m, (_, c) in zip(decl, members)]
    return found


STRUCTS = header_structs()


def test_every_struct_of_output_planes_has_a_row():
    assert sorted(STRUCTS) == sorted(STRUCT_OF.values())
    assert sorted(core.QUERIES) == sorted(STRUCT_OF)
    for name, q in core.QUERIES.items():
        assert q.name == name
    assert len({q.struct for q in core.QUERIES.values()}) == len(core.QUERIES)


@pytest.mark.parametrize("name", sorted(STRUCT_OF))
def test_row_is_the_header_struct(name):
    q = core.QUERIES[name]
    members = STRUCTS[STRUCT_OF[name]]
    assert list(q.tuple._fields) == [f for f, _ in q.struct._fields_] == [m for _, m, _ in members]
    assert len(q.planes) == len(members)
    for (ctype, member, comment), (dtype, shape, fill) in zip(members, q.planes):
        assert dtype == DTYPE_OF[ctype], member
        got = shape(ENGINE, KEY)
        assert isinstance(got, tuple) and all(isinstance(d, int) for d in got), member
        dims = re.match(r"\s*((?:\[\w+\])+)", comment or "")
        if dims:                                                    # the header states the shape: [E][R][k][2]
            want = tuple(int(d) if d.isdigit() else DIMS[d] for d in re.findall(r"\[(\w+)\]", dims.group(1)))
            assert got == want, member
        assert fill == (float("inf") if member in ("gap_min", "ttc_min") else 0), member


def test_shapes_without_a_comment_are_the_documented_ones():
    """the members the header leaves without a shape comment of their own: [E, R] by road id (the first member's comment
    says so), [E] for the trip statistics, [cap] and [cap, 2] for the car list"""
    E, R = ENGINE.E, ENGINE.R
    for name in ("road_measures", "road_following", "car_ages"):
        assert all(shape(ENGINE, KEY) == (E, R) for _, shape, _ in core.QUERIES[name].planes), name
    assert [shape(ENGINE, KEY) for _, shape, _ in core.QUERIES["trip_stats"].planes] == [(E,)] * 4 + [(E, KEY)]
    assert [shape(ENGINE, KEY) for _, shape, _ in core.QUERIES["car_list"].planes] == [(KEY, 2), (KEY,), (KEY,), (KEY,)]


def test_absent_planes():
    """no histogram without bins, no spawn plane on an engine that keeps two planes - and nothing else is ever absent"""
    plain = types.SimpleNamespace(E=3, R=5, P=2)
    for name, q in core.QUERIES.items():
        for field, (_, shape, _) in zip(q.tuple._fields, q.planes):
            assert (shape(plain, KEY) is None) == ((name, field) == ("car_list", "spawn")), (name, field)
            assert (shape(ENGINE, 0) is None) == ((name, field) == ("trip_stats", "hist")), (name, field)


def test_public_tuples_keep_their_fields():
    assert core.RoadMeasures._fields == ("n_cars", "n_halted", "queue", "speed_sum")
    assert core.RoadCells._fields == ("n_cars", "speed_sum")
    assert core.CarAges._fields == ("n_cars", "age_sum", "age_max")
    assert core.TripStats._fields == ("count", "tick_sum", "tick_max", "lost", "hist")
    assert core.RoadFollowing._fields == ("n_cars", "n_pairs", "n_joined", "n_overlap", "gap_sum", "gap_min", "n_hw", "hw_sum",
                                          "n_conflict", "ttc_min", "drac_max")
    assert core.RoadEnds._fields == ("n_cars", "n_heads", "heads", "head_rows", "tail", "tail_row")
    assert core.CarList._fields == ("n", "offsets", "xv", "road", "row", "spawn")
    for t in (core.RoadMeasures, core.RoadCells, core.CarAges, core.TripStats, core.RoadFollowing, core.RoadEnds, core.CarList):
        assert t.__module__ == "gym_traffic.core" and getattr(core, t.__name__) is t


def test_the_predicate_without_a_device():
    """what can be told on the host: a host tensor, another dtype or shape, a view with holes and a non-tensor are refused"""
    ok = dict(dtype=torch.int32, shape=(3, 5))
    assert not core._is_plane(torch.zeros((3, 5), dtype=torch.int32), **ok)              # (right, but on the host)
    assert not core._is_plane(None, **ok) and not core._is_plane([[0] * 5] * 3, **ok)
