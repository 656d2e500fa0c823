"""Switching the spawn rule on ONE handle (tfx_set_poisson / tfx_set_demand / tfx_set_regular / tfx_set_spawns): each
setter releases the arrival stream the handle had and binds its own, so after every switch the long-lived engine must
compute, env for env and bit for bit, what a fresh engine computes that was only ever given that rule - under the same
seed and the same calls.  A pointer into a released buffer, a spawn_stride or an archetype-row binding left over from
the rule before, or a captured graph replayed with the old rule's arguments would show here."""
import numpy as np
import pytest

from oracle.oracle import live_mask
from test_gpu_fused import engine_with
from test_gpu_clone import assert_env_equal, snapshot
from test_gpu_demand import DEMAND, E, GRID, OFF, PATHS, PROFILE, SEED, cars, plain_engine, weights

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from gym_traffic import _native as nat  # noqa: E402

N_ENTRY = 6
ACT = np.random.RandomState(21).randint(2, size=(E, 4)).astype(np.int32)              # one fixed action table
COUNTS = (np.random.RandomState(22).rand(7, E, N_ENTRY) < 0.3).astype(np.int32)       # per-tick counts, a row per tick of step(7)
ARCH2 = np.array([[11.11, 4.0, 3.0, 4.0, 13.89, 6.0, 2.0, 1.0], [8.0, 7.5, 1.5, 3.0, 11.0, 4.0, 2.5, 2.0]], np.float32)


def give_poisson(eng):
    eng.set_poisson(0.9, seed=SEED)


def give_regular(eng):
    eng.set_regular(0.5, seed=SEED + 1)


def give_demand(eng):
    prof = torch.as_tensor(np.asarray(PROFILE, np.int32)).to(eng.device)
    eng.set_demand(seed=SEED, profile_of_env=prof, weights=weights(eng.n_entry), **DEMAND)


def give_counts(eng):
    eng.set_spawns(counts=COUNTS, per_tick=True)


def run_calls(eng):
    """reset, the action table, step(7), then - through the captured graph - agent_step(4); the decision's outputs"""
    eng.reset(np.zeros((eng.E, eng.I), np.int32))
    eng.set_actions(ACT)
    eng.step(7)
    mid = snapshot(eng)
    out = [t.cpu().numpy().copy() for t in eng.agent_step(4)]
    return mid, out


def walk(path, stages, fresh_engine):
    eng = fresh_engine()
    assert eng.n_entry == N_ENTRY and eng.I == ACT.shape[1]
    for k, give in enumerate(stages):
        where = (path, k, give.__name__)
        give(eng)
        ref = fresh_engine()
        give(ref)
        mid, out = run_calls(eng)
        rmid, rout = run_calls(ref)
        end, rend = snapshot(eng), snapshot(ref)
        for e in range(E):
            assert_env_equal(mid, e, rmid, e, where + ("step",))
            assert_env_equal(end, e, rend, e, where + ("agent_step",))
        for u, v, name in zip(out, rout, ("aobs", "areward", "adone")):
            assert np.array_equal(u.view(np.uint8), v.view(np.uint8)), where + (name,)
        assert eng.tick == 11 and cars(eng) > 5, where
        yield eng, give, end


@pytest.mark.parametrize("path", ["resident", "pairs", "pertick"])
def test_switching_rules_equals_a_fresh_engine(path):
    stages = [give_poisson, give_demand, give_regular, give_counts, give_demand, give_poisson]
    seen = []
    for eng, give, _ in walk(path, stages, lambda: plain_engine(PATHS[path])):
        seen.append(give.__name__)
        if give is give_counts:         # the demand went with its buffer
            with pytest.raises(nat.TfxError, match="tfx error -2"):
                eng.demand_counts(0, 1)
            assert eng.demand is None
        if give is give_demand:
            assert eng.demand_counts(0, 1).shape == (1, E, N_ENTRY)
    assert len(seen) == 6
    assert (eng.fused_ticks()[0] > 0) == (path == "resident")


@pytest.mark.parametrize("path", ["pairs", "pertick"])
def test_switching_rules_rebinds_the_archetype_rows(path):
    """Heterogeneous cars: the Poisson stream draws every car's archetype row into its own buffer, the regular stream
    draws none (every car is row 0) - the row buffer must be unbound and bound again with the stream."""
    def fresh_engine():
        return engine_with(PATHS[path], E, planes=3, layout="transposed", archetypes=ARCH2, env_id_offset=OFF, **GRID)

    for eng, give, (s, C) in walk(path, [give_poisson, give_regular, give_poisson], fresh_engine):
        rows = np.concatenate([s["arch"][e][live_mask(s["leading"][e], s["lastcar"][e], C)] for e in range(E)])
        assert rows.size > 5 and rows.max() == (0 if give is give_regular else 1), (path, give.__name__)
