"""The four read-only road kernels on ONE state that combines the hazards of their shared walk (csrc/tfx_walk.hpp; the
state: tests/test_walk_host.py): columns of up to 55 cars that start a row down after a two-tick pass, counts on
both sides of a multiple of eight, a partial second tile, empty roads, and - TFX_MEASURE_GRID=1 - one workgroup whose four
wavefronts each take a second item.  Every query equals its NumPy definition (gym_traffic.devrng) on the image
tfx_export_ring produces, the queries agree with each other, both layouts give the same bytes, and a second accumulated
call gives exactly twice the integers."""
import numpy as np
import pytest

from test_gpu_parity import same_bits
from test_gpu_fused import engine_with
from test_gpu_clone import PATHS
from test_walk_host import CALLS, E_WALK, GRID, NOW, initial_state, oracle_walk, scenario
import test_gpu_cells as cells
import test_gpu_frames as frames
import test_gpu_measures as measures
import test_gpu_travel as travel

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from gym_traffic.devrng import cell_edges  # noqa: E402

HALT = 0.1
X_FROMS = (None, 300.0)
N_CELLS = (8, 11, 32)             # one per instantiation of k_cells
PX = 13
IDS = [2, -1, 0, E_WALK, 1]       # ten (frame, tile) items: three rounds, env ids outside [0, E) between shown ones


def walk_engine(path):
    layout = "ring" if path == "ring" else "transposed"
    eng = engine_with(dict(PATHS[path], TFX_MEASURE_GRID="1"), E_WALK, layout=layout, planes=3, validate=True, **GRID)
    eng.reset(np.zeros((E_WALK, eng.I), np.int32))
    eng.set_tick(NOW)
    x, v, w, ld, lc = initial_state()
    eng.load_state(x, v, ld, lc, w=w)
    for act, cnt in scenario(eng.I, eng.n_entry):
        eng.set_actions(act)
        eng.set_spawns(counts=cnt, per_tick=True)
        eng.step(cnt.shape[0])
    return eng


@pytest.fixture(scope="module")
def engines():
    return {path: walk_engine(path) for path in ("pairs_tail", "ring")}


def test_the_state_combines_the_hazards(engines):
    s = oracle_walk()
    for path, eng in engines.items():
        # one workgroup: its four wavefronts share the six (env, tile) items, and the ten (frame, tile) items of IDS
        assert eng.measure_launch() == eng.ages_launch() == eng.cells_launch(8) == eng.frames_launch(len(IDS), PX) == (1, 4)
        assert eng.R == 80 and eng.C == 66 and eng.tick == NOW + sum(CALLS)
        # HIP equals the oracle bit for bit, so what tests/test_walk_host.py found of the oracle's state holds here
        assert np.array_equal(eng.leading.cpu().numpy(), s["leading"]) and np.array_equal(eng.lastcar.cpu().numpy(), s["lastcar"]), path
    eng = engines["pairs_tail"]
    hb, cars = eng.head_rows(), eng.cars_on_roads_flat().cpu().numpy()
    assert eng.pair_ticks() > 0 and hb.any() and not engines["ring"].head_rows().any()
    for t in s["tiles"]:
        assert (cars[:, t][hb[:, t] > 0] >= 9).any()            # a column of nine cars or more below empty rows, in both tiles
        assert (cars[:, t] > 0).any(axis=1).all()               # both tiles hold live roads
    assert (cars == 0).any()


def queries(eng, twice=False):
    """every output of the four queries as host arrays, by name; twice: of a second, accumulated call into the tensors of
    the first"""
    def ask(call, **kw):
        out = call(**kw)
        return call(accumulate=True, **kw) if twice else out

    out = {}
    for x_from in X_FROMS:
        for name, t in zip(measures.NAMES, measures.host(ask(eng.road_measures, halt_speed=HALT, x_from=x_from))):
            out["measures", x_from, name] = t
    for B in N_CELLS:
        for name, t in zip(("n_cars", "speed_sum"), cells.host(ask(eng.road_cells, edges=cell_edges(GRID["length"], B)))):
            out["cells", B, name] = t
    for name, t in zip(travel.CarAges._fields, travel.host(ask(eng.car_ages))):
        out["ages", name] = t
    return out


def test_queries_equal_their_definitions_and_each_other(engines):
    got = {}
    for path, eng in engines.items():
        got[path] = q = queries(eng)
        for x_from in X_FROMS:
            measures.assert_measures([q["measures", x_from, n] for n in measures.NAMES], measures.model_of(eng, HALT, x_from),
                                     (path, x_from))                   # (speed_sum: bit for bit)
        for B in N_CELLS:
            cells.assert_cells([q["cells", B, "n_cars"], q["cells", B, "speed_sum"]],
                               cells.model_of(eng, cell_edges(GRID["length"], B)), (path, B))
        travel.assert_fields([q["ages", n] for n in travel.CarAges._fields], travel.ages_model(eng), travel.CarAges._fields, path)
        cars = eng.cars_on_roads_flat().cpu().numpy()
        assert np.array_equal(q["measures", None, "n_cars"], cars) and np.array_equal(q["ages", "n_cars"], cars), path
        for B in N_CELLS:
            assert np.array_equal(q["cells", B, "n_cars"].sum(axis=-1), cars), (path, B)
        assert (q["measures", 300.0, "n_cars"] < cars).any() and q["ages", "age_max"].max() > 150
    a, b = got["pairs_tail"], got["ring"]
    assert a.keys() == b.keys()
    for key in a:
        assert a[key].tobytes() == b[key].tobytes(), key


def test_a_second_accumulated_call_doubles_the_integers(engines):
    for path, eng in engines.items():
        once = queries(eng)
        twice = queries(eng, twice=True)
        for key, one in once.items():
            if key[-1] == "age_max":
                assert np.array_equal(twice[key], one), (path, key)
            elif one.dtype != np.float32:
                assert np.array_equal(twice[key], 2 * one), (path, key)
            else:
                assert same_bits(twice[key], (one + one).astype(np.float32)), (path, key)     # one float32 add per word


def test_frames_equal_the_definitions_picture(engines):
    pictures = {}
    for path, eng in engines.items():
        every = frames.check(eng, PX, path)
        some = frames.check(eng, PX, path, ids=IDS)
        assert frames.n_blue(every) > 500
        assert (some[1] == 255).all() and (some[3] == 255).all() and np.array_equal(some[0], every[2])
        pictures[path] = every.tobytes() + some.tobytes()
    assert pictures["pairs_tail"] == pictures["ring"]
