"""tfx_frames on the device (include/tfx.h, csrc/tfx_frames.hpp) against its definition in NumPy (devrng.frames) applied
to the engine's own export_ring image, ring indices and light words - byte for byte: on the driven scenario of
tests/test_frames_host.py on several step paths (and against the CPU oracle's picture of the same scenario), on three grids
under both layouts after step(1), step(2), step(7), graph-replayed agent steps, between move_cars and the advance, after
a clone and after a ring import, on validate-mode and heterogeneous handles; plus: env_ids in any order, repeated and out
of range, the roads-only form, more items than wavefronts, the call writes nothing, argument errors are codes, and it
feeds TrafficVecEnv.frames / render and tools/frames_demo.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_gpu_fused import engine_with
from test_gpu_clone import ARCH, GRID, PATHS, Inputs, assert_env_equal, drive, make, snapshot
from test_gpu_measures import SEQUENCE, load_random, same_snapshot
from test_frames_host import BAD_ARGS, BLUE, driven_calls, driven_frames, driven_with_lights, owned_pixels
from test_measures_host import E_DRIVEN

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from gym_traffic import _native as nat  # noqa: E402
from gym_traffic.devrng import frames  # noqa: E402

PXS = (8, 13, 32)
# the archetype table of tests/test_gpu_clone.py with car lengths 4, 12 and 7.5
ARCH_LEN = ARCH.copy()
ARCH_LEN[:, 1] = (4.0, 12.0, 7.5)


def model_of(eng, px, ids=None, plain_length=False):
    """the definition applied to the image tfx_export_ring produces right now"""
    x, _, _ = eng.planes_numpy()
    het = eng.het and not plain_length
    return frames(x, eng.leading.cpu().numpy(), eng.lastcar.cpu().numpy(), eng.current_phase.cpu().numpy(),
                  eng.elapsed.cpu().numpy(), eng.m, eng.n, px, float(eng.cfg.length), yellow_ticks=int(eng.cfg.yellow_ticks),
                  car_l=float(eng.cfg.car_l), rows=eng.arch.cpu().numpy() if het else None,
                  lengths=eng.archetypes[:, 1] if het else None, env_ids=ids)


def assert_frames(got, want, where):
    assert got.dtype == np.uint8 and got.shape == want.shape, (where, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere((got != want).any(axis=-1))
        raise AssertionError((where, len(bad), [(b.tolist(), got[tuple(b)].tolist(), want[tuple(b)].tolist()) for b in bad[:5]]))


def check(eng, px, where, ids=None):
    got = eng.frames(ids, px=px).cpu().numpy()
    assert_frames(got, model_of(eng, px, ids), (where, px))
    return got


def check_all(eng, where):
    return [check(eng, px, where) for px in PXS][-1]


def n_blue(img):
    return int((img == BLUE).all(axis=-1).sum())


# ---- 1. the driven scenario, against the CPU oracle's picture of it ---------------------------------------------------------
@pytest.mark.parametrize("path", ["resident", "pertick", "pairs_tail", "pairs_split", "ring", "ring_resident"])
def test_driven_scenario(path):
    eng = make(path, E_DRIVEN)
    eng.reset(np.zeros((eng.E, eng.I), np.int32))
    for act, cnt in driven_calls(eng.I, eng.n_entry):
        eng.set_actions(act)
        eng.set_spawns(counts=cnt, per_tick=True)
        eng.step(cnt.shape[0])
    if path.startswith("pairs"):
        # the run ended on a two-tick pass: columns that start a row or two down are really drawn
        assert eng.pair_ticks() > 0 and eng.head_rows().any()
    s = driven_with_lights()
    for px in PXS:
        got = check(eng, px, path)
        # HIP equals the oracle bit for bit, so its picture is the oracle's
        assert_frames(got, driven_frames(s, px), (path, "oracle", px))
    assert n_blue(got) > 1000 and not n_blue(got[0])


# ---- 2. three grids, both layouts, every kind of call --------------------------------------------------------------------------
def call_inputs(rng, eng, n, density=0.2):
    act = rng.randint(2, size=(eng.E, eng.I)).astype(np.int32)
    cnt = ((rng.rand(n, eng.E, eng.n_entry) < density) * rng.randint(1, 3, size=(n, eng.E, eng.n_entry))).astype(np.int32)
    eng.set_actions(act)
    eng.set_spawns(counts=cnt, per_tick=True)


@pytest.mark.parametrize("path", ["pairs_tail", "ring"])
@pytest.mark.parametrize("m,n,capacity,E", [(2, 2, 10, 5), (3, 2, 14, 3), (4, 4, 14, 3)])
def test_grids_layouts_and_calls(path, m, n, capacity, E):
    """2 x 2 with ten ring slots: rings wrap; 3 x 2: m != n; 4 x 4: 80 roads, two tiles per env.  64 ticks of warm-up fill
    the roads (on the CPU oracle this run has wrapped and full rings on every grid by then)."""
    eng = make(path, E, m=m, n=n, capacity=capacity)
    assert eng.frame_size(13) == ((m + 1) * 13 + 1, (n + 1) * 13 + 1)
    rng = np.random.RandomState(100 * m + n)
    eng.reset(np.zeros((E, eng.I), np.int32))
    for _ in range(8):
        call_inputs(rng, eng, 8)
        eng.step(8)
    head_rows = False
    for kind, ticks in (("step", 1), ("step", 2), ("step", 7), ("agent", 6), ("agent", 6), ("step", 2)):
        call_inputs(rng, eng, ticks)
        (eng.agent_step if kind == "agent" else eng.step)(ticks)          # (the second agent step replays the captured graph)
        head_rows |= bool(eng.head_rows().any())
        got = check_all(eng, (path, m, n, kind, ticks))
        assert n_blue(got) > 50
    ld, lc = eng.leading.cpu().numpy(), eng.lastcar.cpu().numpy()
    cars = eng.cars_on_roads_flat().cpu().numpy()
    assert (ld > lc).any() and (cars == capacity - 2).any() and (cars == 0).any()
    if path != "ring" and (m, n) == (2, 2):
        assert head_rows
    # between tfx_move_cars and tfx_advance_finished_cars: heads past the road's end clamp to its last pixel
    call_inputs(rng, eng, 1)
    eng.move_cars()
    check_all(eng, (path, m, n, "after move_cars"))
    eng.advance_finished_cars()
    check_all(eng, (path, m, n, "after the advance"))
    # after a clone: the last env becomes env 0, env 1 becomes the last
    src = np.full(E, -1, np.int32)
    src[1], src[0] = E - 1, -1
    before = eng.frames([E - 1], px=13).cpu().numpy()
    eng.clone_envs(src)
    got = check_all(eng, (path, m, n, "after clone_envs"))
    assert np.array_equal(eng.frames([1], px=13).cpu().numpy(), before)
    # after tfx_import_ring + tfx_refresh: unsorted x, empty, wrapped and full rings
    count = load_random(eng, 7 * m + n)
    got = check_all(eng, (path, m, n, "after the ring import"))
    assert n_blue(got) > count.sum() // 4


@pytest.mark.parametrize("path", ["ring", "pertick"])
def test_cars_past_the_road_end_are_drawn_clamped(path):
    """One car half a metre before the end of every road at 10 m/s: tfx_move_cars takes those whose way is free - the exit
    roads' at the least, nothing ever stops them - past the road's end, and until the advance the ring image holds them
    there (ring layout; the transposed layout moves them to the outbox at once - there the picture follows the image)."""
    E = 3
    eng = make(path, E)
    eng.reset(np.zeros((E, eng.I), np.int32))
    length = float(eng.cfg.length)
    x = np.zeros((E, eng.R, eng.C), np.float32)
    v = np.zeros((E, eng.R, eng.C), np.float32)
    x[..., 2], v[..., 2] = length - 0.5, 10.0
    eng.load_state(x, v, np.ones((E, eng.R), np.int32), np.full((E, eng.R), 2, np.int32))
    eng.set_actions(np.zeros((E, eng.I), np.int32))
    eng.set_spawns(counts=np.zeros((E, eng.n_entry), np.int32))
    check(eng, 32, "before")
    eng.move_cars()
    head = eng.planes_numpy()[0][..., 2]
    if path == "ring":
        assert (head[:, eng.r:] > length + 4.0).all()                       # front and back of the car are past the end
    for px in PXS:
        got = check(eng, px, (path, "after move_cars"))
    if path == "ring":
        roads, _, _ = owned_pixels(eng.m, eng.n, PXS[-1])
        for e in range(eng.r, eng.R):                                      # a and b clamp to the road's last pixel
            line = [tuple(got[1, r_, c_]) == BLUE for c_, r_ in roads[e]]
            assert line == [False] * (len(line) - 1) + [True], e
    eng.advance_finished_cars()
    check_all(eng, (path, "after the advance"))


# ---- 3. validate-mode and heterogeneous handles ------------------------------------------------------------------------------------
@pytest.mark.parametrize("path,kind", [("pertick", "validate"), ("pairs_tail", "validate"), ("ring", "validate"),
                                       ("pertick", "het"), ("pairs_tail", "het")])
def test_validate_and_heterogeneous_handles(path, kind):
    E = 4
    if kind == "het":
        eng = engine_with(PATHS[path], E, layout="transposed", planes=3, validate=True, archetypes=ARCH_LEN, **GRID)
        assert eng.het
    else:
        eng = make(path, E, kind)
    load_random(eng, 11)
    check_all(eng, (path, kind, "random rings"))
    eng.reset(np.zeros((E, eng.I), np.int32))
    inp = Inputs(eng, 5)
    for call in [("step", 8)] * 5 + [("step", 1), ("step", 2), ("agent", 6), ("agent", 6), ("step", 7), ("step", 4)]:
        drive(eng, inp, call)
    got = check_all(eng, (path, kind, "driven"))
    assert n_blue(got) > 50
    if kind == "het":
        from oracle.oracle import live_mask
        ld, lc = eng.leading.cpu().numpy(), eng.lastcar.cpu().numpy()
        rows = eng.arch.cpu().numpy()
        live = np.stack([live_mask(ld[k], lc[k], eng.C) for k in range(E)])
        assert {0, 1} <= set(rows[live].tolist())                        # cars of length 4 and of length 12 are on the roads
        # ... and the picture depends on them: with every car as long as car_l it is another one
        assert not np.array_equal(got, model_of(eng, 32, plain_length=True))


# ---- 4. env_ids ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["pairs_tail", "ring"])
def test_env_ids(path):
    E = 5
    eng = make(path, E, m=2, n=2, capacity=10)
    load_random(eng, 21)
    whole = check(eng, 13, "every env")
    assert len({f.tobytes() for f in whole}) == E                            # the envs look different
    for ids in ([3, 1, 4], [2, 2, 0, 2], [-1, 0, E, 1, 7, -5], [4]):
        got = check(eng, 13, ids, ids=ids)
        for f, k in zip(got, ids):
            assert np.array_equal(f, whole[k]) if 0 <= k < E else (f == 255).all()
    # an int32 tensor on the device, a NumPy array
    dev = torch.tensor([4, 0, 3], dtype=torch.int32, device=eng.device)
    assert np.array_equal(eng.frames(dev, px=13).cpu().numpy(), whole[[4, 0, 3]])
    assert np.array_equal(eng.frames(np.array([1, 2]), px=13).cpu().numpy(), whole[[1, 2]])
    # the engine's tensor per (n, px) is rewritten roads only from its second use on: a frame whose id is out of range
    # then loses the picture the call before left in it
    assert n_blue(eng.frames([0, 1], px=8).cpu().numpy()[1]) > 0
    got = check(eng, 8, "an id out of range after a picture", ids=[0, -1])
    assert (got[1] == 255).all() and n_blue(got[0]) > 0
    # NULL env_ids through the C call: envs 0 .. n_frames - 1
    H, W = eng.frame_size(13)
    out = torch.zeros((3, H, W, 4), dtype=torch.uint8, device=eng.device)
    nat.check(nat.lib().tfx_frames(eng.h, None, 3, 13, C.c_void_p(out.data_ptr()), 0, eng._stream()))
    assert np.array_equal(out.cpu().numpy(), whole[:3])


# ---- 5. roads only --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["pairs_tail", "ring"])
def test_roads_only(path):
    E = 3
    eng = make(path, E, m=2, n=2, capacity=10)
    load_random(eng, 22)
    px = 13
    H, W = eng.frame_size(px)
    want = model_of(eng, px, [2, 0])
    roads, _, _ = owned_pixels(2, 2, px)
    rc, rr = roads[5][3]                                                     # a road pixel ...
    assert (want[1, 0, 0] == 255).all() and (want[0, 0, 0] == 255).all()    # ... and a background one: the corner
    mine = torch.zeros((2, H, W, 4), dtype=torch.uint8, device=eng.device)
    assert eng.frames([2, 0], px=px, out=mine) is mine
    assert_frames(mine.cpu().numpy(), want, "out=")
    sentinel = torch.tensor([1, 2, 3, 4], dtype=torch.uint8, device=eng.device)
    mine[1, 0, 0] = sentinel
    mine[1, rr, rc] = sentinel
    eng.frames([2, 0], px=px, out=mine, roads_only=True)
    got = mine.cpu().numpy()
    assert got[1, 0, 0].tolist() == [1, 2, 3, 4]                             # the background is not written ...
    assert np.array_equal(got[1, rr, rc], want[1, rr, rc])                   # ... the road pixel is
    got[1, 0, 0] = 255
    assert_frames(got, want, "roads only")
    eng.frames([2, 0], px=px, out=mine)                                      # without the flag the background comes back
    assert_frames(mine.cpu().numpy(), want, "background again")
    # the engine's own tensor per (n, px) takes the flag by itself from its second use on
    own = eng.frames([2, 0], px=px)
    assert own is not mine and eng.frames([1, 0], px=px) is own and eng.frames([2, 0], px=8) is not own
    eng.frames([2, 0], px=px)
    own[1, 0, 0] = sentinel
    own[1, rr, rc] = sentinel
    assert eng.frames([2, 0], px=px) is own
    got = own.cpu().numpy()
    assert got[1, 0, 0].tolist() == [1, 2, 3, 4] and np.array_equal(got[1, rr, rc], want[1, rr, rc])
    got[1, 0, 0] = 255
    assert_frames(got, want, "the cached tensor")
    # the cars move, the cached tensor follows
    call_inputs(np.random.RandomState(1), eng, 3)
    eng.step(3)
    got = eng.frames([2, 0], px=px).cpu().numpy()
    got[1, 0, 0] = 255
    assert_frames(got, model_of(eng, px, [2, 0]), "the cached tensor, later")
    with pytest.raises(ValueError):
        eng.frames([2, 0], px=px, out=torch.zeros((2, H, W, 3), dtype=torch.uint8, device=eng.device))
    with pytest.raises(ValueError):
        eng.frames([2, 0], px=7)


# ---- 6. later rounds of the stride loop ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["transposed", "ring"])
def test_stride_loop(layout):
    """Seven frames of the 4 x 4 grid (80 roads: two tiles per env) are 14 (frame, tile) items - no multiple of the four
    wavefronts of the ONE workgroup TFX_GRID_CAP=1 leaves the launch: every wavefront takes three or four items, and
    clears and refills its bitset as often."""
    cfg = dict(m=4, n=4, length=120.0, capacity=14, rate=0.5)
    ids = [4, 0, 2, 2, 1, 3, 0]
    plain = engine_with({"TFX_RESIDENT": "0"}, 5, layout=layout, **cfg)
    assert plain.frames_launch(len(ids), 13) == (4, 16) and plain.frames_launch(1, 13) == (1, 4)
    eng = engine_with({"TFX_RESIDENT": "0", "TFX_GRID_CAP": "1"}, 5, layout=layout, **cfg)
    grid, waves = eng.frames_launch(len(ids), 13)
    items = len(ids) * ((eng.R + 63) // 64)
    assert (grid, waves) == (1, 4) and items == 14 and items > waves and items % 4
    capped = engine_with({"TFX_RESIDENT": "0", "TFX_MEASURE_GRID": "2"}, 5, layout=layout, **cfg)
    assert capped.frames_launch(len(ids), 13) == (2, 8)
    count = load_random(eng, 9)
    assert count.any(axis=1).all()
    for px in PXS:
        got = check(eng, px, layout, ids=ids)
        assert all(n_blue(f) > 0 for f in got)
    check(eng, 13, layout)                                                  # five frames: ten items


# ---- 7. read-only -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["resident", "pairs_tail", "pairs_split", "pertick", "ring"])
def test_twin_that_is_never_drawn(path):
    """An engine drawn between every call of a mixed step / agent_step sequence (repeats replay captured graphs) stays
    bit-identical to one that never is, outputs included."""
    E = E_DRIVEN
    eng, ref = make(path, E), make(path, E)
    rng = np.random.RandomState(31)
    for e_ in (eng, ref):
        e_.reset(np.zeros((E, eng.I), np.int32))
    blue = 0
    for kind, n in SEQUENCE:
        act = rng.randint(2, size=(E, eng.I)).astype(np.int32)
        cnt = ((rng.rand(n, E, eng.n_entry) < 0.15) * rng.randint(1, 3, size=(n, E, eng.n_entry))).astype(np.int32)
        eng.frames(px=8)
        eng.frames([5, 1, 1], px=32)
        outs = []
        for e_ in (eng, ref):
            e_.set_actions(act)
            e_.set_spawns(counts=cnt, per_tick=True)
            out = (e_.agent_step if kind == "agent" else e_.step)(n)
            outs.append([t.cpu().numpy().copy() for t in out] if kind == "agent" else [])
        for a, b in zip(*outs):
            assert a.tobytes() == b.tobytes(), (path, kind, n)
        blue = n_blue(check(eng, 13, (path, kind, n)))
        sa, sb = snapshot(eng), snapshot(ref)
        for k in range(E):
            assert_env_equal(sa, k, sb, k, (path, kind, n))
        assert np.array_equal(eng.head_rows(), ref.head_rows())
    assert blue > 0


def test_the_launch_is_not_counted_by_fail_after():
    eng = make("pertick", 3)
    load_random(eng, 2)
    lib = nat.lib()
    nat.check(lib.tfx_debug_fail_after(eng.h, 1))                            # the NEXT counted launch fails
    for _ in range(3):
        check(eng, 13, "frames under fail_after")                          # (tfx_export_ring is not counted either)
    before = snapshot(eng)
    with pytest.raises(nat.TfxError, match="injected"):
        eng.clone_envs(np.array([-1, 0, -1], np.int32))
    nat.check(lib.tfx_debug_fail_after(eng.h, 0))
    same_snapshot(before, snapshot(eng))
    check(eng, 13, "after the injected failure")


# ---- 8. errors ---------------------------------------------------------------------------------------------------------------------------
def test_errors_are_codes_and_the_handle_stays_usable():
    lib = nat.lib()
    eng = make("pertick", 3)
    load_random(eng, 4)
    H, W = eng.frame_size(32)
    out_t = torch.zeros((4, H, W, 4), dtype=torch.uint8, device=eng.device)
    ids_t = torch.tensor([0, 1], dtype=torch.int32, device=eng.device)
    out, ids, st = C.c_void_p(out_t.data_ptr()), C.c_void_p(ids_t.data_ptr()), eng._stream()
    # before tfx_bind_buffers
    h = C.c_void_p()
    nat.check(lib.tfx_create(C.byref(eng.cfg), C.byref(h)))
    assert lib.tfx_frames(h, ids, 2, 32, out, 0, st) == -2
    assert b"tfx_bind_buffers" in lib.tfx_last_error()
    hh, ww = C.c_int32(), C.c_int32()
    assert lib.tfx_frame_size(h, 32, C.byref(hh), C.byref(ww)) == 0 and (hh.value, ww.value) == (H, W)
    nat.check(lib.tfx_destroy(h))
    for args, msg in BAD_ARGS(ids, out):
        assert lib.tfx_frames(eng.h, *args, st) == -1, msg
        assert msg in lib.tfx_last_error(), (msg, lib.tfx_last_error())
    assert lib.tfx_frames(None, ids, 2, 32, out, 0, st) == -1 and b"null handle" in lib.tfx_last_error()
    assert lib.tfx_frames(eng.h, None, 4, 32, out, 0, st) == -1 and b"env_ids is null" in lib.tfx_last_error()
    assert lib.tfx_frames(eng.h, None, 3, 32, out, 0, st) == 0               # n_frames == E is fine
    torch.cuda.synchronize()
    got = out_t.cpu().numpy()
    assert not got[3].any()                                                  # the refused calls wrote nothing
    assert_frames(got[:3], model_of(eng, 32), "after the errors")
    with pytest.raises(ValueError):
        eng.frames([], px=32)
    eng.step(3)
    check(eng, 32, "after a step")


# ---- 9. TrafficVecEnv.frames / render ---------------------------------------------------------------------------------------------------
def test_vec_env_frames_and_render():
    from gym_traffic.envs.vec_env import TrafficVecEnv
    from gym_traffic.wrappers.vec import VecRemiRepeater
    E, m, n = 5, 3, 3
    venv = TrafficVecEnv(E, m, n, 120.0, capacity=14, spawn='periodic', spawn_period=3, seed=3)
    wrapped = VecRemiRepeater(venv, 5)
    wrapped.reset()
    eng = venv.engine
    rng = np.random.RandomState(4)
    for d in range(9):
        wrapped.step(torch.as_tensor(rng.randint(2, size=(E, eng.I)).astype(np.int32)).to(eng.device))
    want = model_of(eng, 32)
    every = wrapped.frames()                                                 # through VecWrapper.__getattr__
    assert every.dtype == torch.uint8 and tuple(every.shape) == (E, 4 * 32 + 1, 4 * 32 + 1, 4) and every.is_cuda
    assert_frames(every.cpu().numpy(), want, "every env")
    assert n_blue(want) > 20
    for envs in ([3, 0], np.array([3, 0]), torch.tensor([3, 0], dtype=torch.int32, device=eng.device)):
        assert_frames(venv.frames(envs).cpu().numpy(), want[[3, 0]], type(envs))
    for k in (0, 4):
        img = venv.render(env=k)
        assert isinstance(img, np.ndarray) and img.dtype == np.uint8 and img.shape == (129, 129, 3)
        assert np.array_equal(img, venv.frames([k])[0, ..., :3].cpu().numpy()) and np.array_equal(img, want[k, ..., :3])
    assert venv.render(env=2, px=13).shape == (53, 53, 3)
    with pytest.raises(NotImplementedError, match="frames"):
        venv.render(mode='human')


# ---- 10. the demo -------------------------------------------------------------------------------------------------------------------------
def test_frames_demo_writes_its_pngs(tmp_path):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "frames_demo.py"), "--envs", "8", "--m", "3", "--n", "3",
                          "--length", "120", "--capacity", "14", "--decisions", "5", "--ticks", "6", "--show", "0", "5",
                          "--px", "16", "--out", str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    print(out.stdout)
    names = sorted(os.listdir(str(tmp_path)))
    assert names == ["env%d_%03d.png" % (k, d) for k in (0, 5) for d in range(5)]
    from PIL import Image
    img = np.asarray(Image.open(os.path.join(str(tmp_path), names[-1])))
    assert img.shape == (65, 65, 3) and (img[0, 0] == 255).all() and (img != 255).any()
