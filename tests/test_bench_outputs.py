"""bench.py's plain run and `--dump-outputs DIR`: what a plain run measures (one timed region of --steps ticks and
nothing else), and the arrays it leaves for comparing two builds output for output."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

torch = pytest.importorskip("torch")

NAMES = ("obs", "rewards", "done", "leading", "lastcar", "x", "v")


class _Engine(object):
    """The attributes of a TfxEngine that bench.dump_outputs reads, on the CPU."""

    def __init__(self, E=40, R=6, C=5, I=2, seed=1):
        rng = np.random.RandomState(seed)
        self.E, self.R, self.C, self.I, self.obs_len = E, R, C, I, 2 * (R - 2) + 2 * I
        self.device = torch.device("cpu")
        self.xv = torch.as_tensor(rng.uniform(1, 9, (E, R, C, 2)).astype(np.float32))
        self.leading = torch.as_tensor(rng.randint(1, C, (E, R)).astype(np.int32))
        self.lastcar = torch.as_tensor(rng.randint(1, C, (E, R)).astype(np.int32))
        self.obs = torch.as_tensor(rng.randint(0, 99, (E, self.obs_len)).astype(np.int32))
        self.rewards = torch.as_tensor(rng.uniform(-1, 1, (E, I)).astype(np.float32))
        self.done = torch.as_tensor(rng.randint(0, 2, E).astype(np.uint8))

    def drop_staging(self):
        pass


def _load(d, suffix=""):
    return {n: np.load(os.path.join(str(d), n + suffix + ".npy")) for n in NAMES}


def test_dump_outputs_whole_batch_and_seeded_sample(tmp_path):
    import bench
    from oracle.oracle import live_mask
    eng = _Engine()
    assert bench.dump_outputs(eng, str(tmp_path / "all"), 1 << 30) == eng.E
    z = _load(tmp_path / "all")
    assert {n: a.dtype for n, a in z.items()} == {"obs": np.float64, "rewards": np.float32, "done": np.float64,
                                                  "leading": np.float64, "lastcar": np.float64,
                                                  "x": np.float32, "v": np.float32}
    assert np.array_equal(z["obs"], eng.obs.numpy()) and np.array_equal(z["rewards"], eng.rewards.numpy())
    assert np.array_equal(z["done"], eng.done.numpy()) and np.array_equal(z["lastcar"], eng.lastcar.numpy())
    # slots that hold a car (the oracle's ring convention) keep x and v; every other slot reads 0
    xv = eng.xv.numpy()
    for e in range(eng.E):
        live = live_mask(eng.leading[e].numpy(), eng.lastcar[e].numpy(), eng.C)
        assert np.array_equal(z["x"][e], np.where(live, xv[e, ..., 0], 0)), e
        assert np.array_equal(z["v"][e], np.where(live, xv[e, ..., 1], 0)), e
    assert 0 < int((z["x"] != 0).sum()) < z["x"].size
    # a budget of 7 envs: the same sorted seeded draw every time, and within the budget
    per_env = 8 * (eng.obs_len + 1 + 2 * eng.R) + 4 * (eng.I + 2 * eng.R * eng.C)
    for d in ("s1", "s2"):
        assert bench.dump_outputs(eng, str(tmp_path / d), 7 * per_env + 5, "_rank1") == 7
    a, b = _load(tmp_path / "s1", "_rank1"), _load(tmp_path / "s2", "_rank1")
    assert all(np.array_equal(a[n], b[n]) for n in NAMES)
    assert sum(os.path.getsize(str(tmp_path / "s1" / (n + "_rank1.npy"))) for n in NAMES) <= 7 * per_env + 7 * 128
    idx = np.sort(np.random.RandomState(bench.DUMP_SEED).choice(eng.E, 7, replace=False))
    assert np.array_equal(a["obs"], eng.obs.numpy()[idx]) and np.array_equal(a["x"], z["x"][idx])


@pytest.mark.gpu
def test_plain_run_times_the_steps_it_is_given_and_dumps_the_same_outputs(tmp_path):
    """A plain run: one timed region of exactly --steps ticks, the contract fields, none of what --full adds; two runs
    with the same arguments write the same outputs, within the size limit."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    lines = []
    for d in ("a", "b"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "3",
                            "--envs", "512", "--dump-outputs", str(tmp_path / d)], env=env, stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, universal_newlines=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        out = [ln for ln in r.stdout.splitlines() if ln.strip()]
        assert len(out) == 1
        lines.append(json.loads(out[0]))
    for out in lines:
        assert out["metric"] == "vehicle_updates_per_sec" and out["unit"] == "vehicle-updates/s"
        assert out["higher_is_better"] is True and out["dtype"] == "f32" and out["value"] > 0
        assert out["steps"] == 7 and out["warmup"] == 3 and out["repeats"] == 1 and len(out["regions"]) == 1
        assert abs(out["ms_per_step"] - out["regions"][0]["ms"] / 7) <= 1e-9 * out["ms_per_step"]
        assert "roofline" not in out and "cpu_baseline" not in out and out["agent_decisions_timed"] == 0
    assert lines[0]["regions"][0]["vehicle_updates"] == lines[1]["regions"][0]["vehicle_updates"]
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sum(os.path.getsize(str(tmp_path / "a" / (n + ".npy"))) for n in NAMES) <= 64 * 10 ** 6
    assert a["obs"].shape[0] < 512 and a["x"].ndim == 3 and int((a["x"] != 0).sum()) > 1000
    for n in NAMES:
        assert a[n].dtype in (np.float32, np.float64) and np.array_equal(a[n], b[n]), n
