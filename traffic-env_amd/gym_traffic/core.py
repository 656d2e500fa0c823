"""TfxEngine: E batched traffic envs resident on one MI355X.

Owns the device buffers (PyTorch-ROCm tensors - used for memory and streams only) and drives the
HIP kernels through the C ABI (include/tfx.h, csrc/tfx_hip.hip).  Both front-ends sit on top of it:
`TrafficEnv` (the reference's single-env gym object, NumPy in / NumPy out) and `TrafficVecEnv`
(tensors in / tensors out for batched RL rollouts).

State layout = the reference's arrays with a leading env dimension (traffic_env.py:361-382):
    xv [E,R,C,2] f32 ((x, v) per ring slot; `x`/`v` are views)   w [E,R,C] f32 (planes == 3 only)
    With layout='transposed' (the default when w is not carried) the kernels keep the cars in a
    position-major array instead (csrc/tfx_move_t.hpp); `xv`/`x`/`v` then are a ring-layout staging
    copy that is refreshed from the device on access and pushed back by refresh()/load_state().
    leading/lastcar [E,R] i32   obs [E,2r+2I] i32   rewards [E,I] f32   waiting [E,r] i32
    passed_dst [E,I] u8   done_tick [E] i32
"""
import collections
import ctypes as C
import os

import numpy as np
import torch

from . import _native as nat

# the single archetype of the reference (traffic_env.py:35-43)
ARCHETYPE = dict(car_v=11.11, car_l=4.0, car_a=3.0, car_delta=4.0, car_v0=13.89, car_b=6.0,
                 car_T=2.0, car_s0=1.0)
# module constants of the reference (traffic_env.py:17-25)
CONSTANTS = dict(yellow_ticks=6, thresh=0.2, detect_dist=10.0, overflow_penalty=10.0, eps=1e-8)


# One row per device query that writes into a struct of output planes (include/tfx.h).  `tuple` is what the query returns
# and takes as out=; its fields are those of the ctypes struct `struct`.  `planes` holds per field (torch dtype: the element
# type of the C member, shape, fill of a fresh tensor); a shape is a function of the engine and the query's key - what the
# shapes depend on beyond the engine: road_ends' k, the number of bins or cells, car_list's length - and gives None where
# the engine or the call has no such plane.
Query = collections.namedtuple("Query", "name tuple struct planes")


def _query(name, tuple_name, struct, **planes):
    fields = [f for f, _ in struct._fields_]
    if set(fields) != set(planes):
        raise TypeError("%s: the planes %s are not the fields of %s" % (name, sorted(planes), struct.__name__))
    return Query(name, collections.namedtuple(tuple_name, fields), struct, tuple(planes[f] for f in fields))


def _e(eng, key):
    return (eng.E,)


def _er(eng, key):
    return (eng.E, eng.R)


def _erk(eng, key):
    return (eng.E, eng.R, key)


def _cap(eng, key):
    return (key,)


_I32, _I64, _F32, _U8, _INF = torch.int32, torch.int64, torch.float32, torch.uint8, float("inf")
QUERIES = {q.name: q for q in (
    _query("road_measures", "RoadMeasures", nat.TfxMeasureBuffers,
           n_cars=(_I32, _er, 0), n_halted=(_I32, _er, 0), queue=(_I32, _er, 0), speed_sum=(_F32, _er, 0)),
    _query("road_following", "RoadFollowing", nat.TfxFollowBuffers,
           n_cars=(_I32, _er, 0), n_pairs=(_I32, _er, 0), n_joined=(_I32, _er, 0), n_overlap=(_I32, _er, 0),
           gap_sum=(_F32, _er, 0), gap_min=(_F32, _er, _INF), n_hw=(_I32, _er, 0), hw_sum=(_F32, _er, 0),
           n_conflict=(_I32, _er, 0), ttc_min=(_F32, _er, _INF), drac_max=(_F32, _er, 0)),
    _query("road_ends", "RoadEnds", nat.TfxEndsBuffers,
           n_cars=(_I32, _er, 0), n_heads=(_I32, _er, 0), heads=(_F32, lambda eng, k: (eng.E, eng.R, k, 2), 0),
           head_rows=(_U8, _erk, 0), tail=(_F32, lambda eng, k: (eng.E, eng.R, 2), 0), tail_row=(_U8, _er, 0)),
    _query("car_ages", "CarAges", nat.TfxAgeBuffers, n_cars=(_I32, _er, 0), age_sum=(_I64, _er, 0), age_max=(_I32, _er, 0)),
    _query("trip_stats", "TripStats", nat.TfxTripStatBuffers,
           count=(_I32, _e, 0), tick_sum=(_I64, _e, 0), tick_max=(_I32, _e, 0), lost=(_I32, _e, 0),
           hist=(_I32, lambda eng, B: (eng.E, B) if B else None, 0)),
    _query("road_cells", "RoadCells", nat.TfxCellBuffers, n_cars=(_I32, _erk, 0), speed_sum=(_F32, _erk, 0)),
    # (never cached: car_list makes fresh planes of the call's length; CarList puts n and offsets in front of them)
    _query("car_list", "CarPlanes", nat.TfxCarListBuffers,
           xv=(_F32, lambda eng, cap: (cap, 2), 0), road=(_I32, _cap, 0), row=(_U8, _cap, 0),
           spawn=(_F32, lambda eng, cap: (cap,) if eng.P == 3 else None, 0)),
)}
# road_measures(), road_following(), car_ages(): [E, R] device tensors by road id; road_ends(): heads [E, R, k, 2], head_rows
# [E, R, k], tail [E, R, 2]; trip_stats(): [E], hist [E, n_bins] or None; road_cells(): [E, R, B] by road id and cell
RoadMeasures, RoadFollowing, RoadEnds, CarAges, TripStats, RoadCells = [
    QUERIES[q].tuple for q in ("road_measures", "road_following", "road_ends", "car_ages", "trip_stats", "road_cells")]
# what car_list() returns: n int32 scalar (the total N) and offsets int32 [n_sel * R + 1], then the planes of max_cars (or N)
# entries: xv [.., 2], road, row, spawn (None on engines without a spawn plane) - device tensors
CarList = collections.namedtuple("CarList", ("n", "offsets") + QUERIES["car_list"].tuple._fields)


def _is_plane(t, dtype, shape):
    """t is a contiguous device tensor of this dtype and shape"""
    return isinstance(t, torch.Tensor) and t.dtype == dtype and tuple(t.shape) == tuple(shape) and t.is_contiguous() \
        and t.is_cuda


def _buffers(q, out):
    """the ctypes struct of query `q` that points at the tensors of `out` (a member None: a null pointer)"""
    return q.struct(*[_ptr(t) for t in out])


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


class HostMirror(object):
    def __init__(self, device, tensors):
        self.device = device
        self.dev = list(tensors)
        self.host = [torch.empty(t.shape, dtype=t.dtype).pin_memory() for t in self.dev]
        self.views = [h.numpy() for h in self.host]

    def pull(self):
        for h, t in zip(self.host, self.dev):
            h.copy_(t, non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()
        return self.views


class PackedMirror(object):
    """Pinned host copy of ONE contiguous device byte buffer that several tensors are views of: one
    device-to-host copy and one stream synchronisation bring all of them over.  `views` maps a name
    to (byte offset, dtype, shape); pull() returns {name: NumPy view} (valid until the next pull)."""

    def __init__(self, device, buf, views):
        self.device = device
        self.dev = buf
        self.host = torch.empty(buf.shape, dtype=torch.uint8).pin_memory()
        raw = self.host.numpy()
        self.views = {}
        for name, (off, dtype, shape) in views.items():
            n = int(np.prod(shape)) * np.dtype(dtype).itemsize
            self.views[name] = raw[off:off + n].view(dtype).reshape(shape)

    def start(self):
        """Queue the copy only (a later pull() / synchronisation on the same stream completes it)."""
        self.host.copy_(self.dev, non_blocking=True)
        return self.views

    def pull(self):
        self.host.copy_(self.dev, non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()
        return self.views


class TfxEngine(object):
    def __init__(self, m, n, length, capacity, n_envs=1, rate=0.5, learn_switch=False,
                 validate=False, entry_spec=0, planes=None, trip_cap=4096, device=None, env_id_offset=0,
                 layout=None, archetypes=None, constants=None):
        """constants: entries of CONSTANTS to override (yellow_ticks, thresh, detect_dist, overflow_penalty, eps); the
        engine keeps the full set as `constants`.
        archetypes: rows (v, l, a, delta, v0, b, T, s0) of the reference's `archetypes` table
        (traffic_env.py:35-43) when there is more than its single default row, or a delta other than 4
        ("heterogeneous cars": needs planes = 3 and the transposed layout; every car keeps its row, see
        set_spawns(..., rows=) and the `arch` property).  One ordinary row (delta = 4) IS the engine's single archetype:
        `car` (the car_* values in use) and cfg.car_* then hold that row, not ARCHETYPE."""
        if not torch.cuda.is_available():
            raise nat.TfxError("no GPU visible: the traffic env step runs on MI355X only (no CPU fallback)")
        self.lib = nat.lib()
        self.device = torch.device(device if device is not None else "cuda:%d" % torch.cuda.current_device())
        self.m, self.n, self.C, self.E = int(m), int(n), int(capacity), int(n_envs)
        arch = None if archetypes is None else np.asarray(archetypes, np.float32).reshape(-1, 8)
        self.het = arch is not None and (len(arch) > 1 or float(arch[0, 3]) != 4.0)
        self.archetypes = arch
        self.P = int(planes) if planes else (3 if (validate or self.het) else 2)
        cfg = nat.TfxConfig()
        cfg.m, cfg.n, cfg.capacity, cfg.n_envs, cfg.planes = self.m, self.n, self.C, self.E, self.P
        cfg.length, cfg.rate = float(length), float(rate)
        self.car = dict(ARCHETYPE)
        if arch is not None and not self.het:
            self.car = dict(zip(("car_v", "car_l", "car_a", "car_delta", "car_v0", "car_b", "car_T", "car_s0"),
                                [float(t) for t in arch[0]]))
        for k, v in self.car.items():
            setattr(cfg, k, v)
        if arch is not None:
            if len(arch) > nat.MAX_ARCH:
                raise ValueError("at most %d archetype rows" % nat.MAX_ARCH)
            cfg.n_archetypes = len(arch)
            for a, row in enumerate(arch):
                for j in range(8):
                    cfg.arch[a][j] = float(row[j])
        unknown = set(constants or {}) - set(CONSTANTS)
        if unknown:
            raise ValueError("unknown constants: %s (known: %s)" % (sorted(unknown), sorted(CONSTANTS)))
        self.constants = dict(CONSTANTS, **(constants or {}))
        self.constants["yellow_ticks"] = int(self.constants["yellow_ticks"])
        for k, v in self.constants.items():
            setattr(cfg, k, v)
        cfg.learn_switch, cfg.validate = int(bool(learn_switch)), int(bool(validate))
        cfg.entry_spec = int(entry_spec)
        cfg.env_id_offset = int(env_id_offset)
        if layout is None:
            layout = os.environ.get("TFX_LAYOUT") or "transposed"
        if layout not in ("ring", "transposed"):
            raise ValueError("layout must be 'ring' or 'transposed'")
        self.layout = layout
        cfg.layout = 1 if layout == "transposed" else 0
        self.cfg = cfg
        self.validate = bool(validate)
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            nat.check(self.lib.tfx_create(C.byref(cfg), C.byref(h)))
        self.h = h
        dims = [C.c_int32() for _ in range(4)]
        nat.check(self.lib.tfx_dims(h, *[C.byref(d) for d in dims]))
        self.I, self.r, self.R, self.n_entry = [int(d.value) for d in dims]
        self.obs_len = 2 * self.r + 2 * self.I
        self.dest = np.zeros(self.R, np.int32)
        self.phases = np.zeros(self.R, np.int32)
        self.nexts = np.zeros(self.R, np.int32)
        self.entrypoints = np.zeros(max(1, self.n_entry), np.int32)
        nat.check(self.lib.tfx_tables(h, *[a.ctypes.data_as(C.c_void_p) for a in
                                           (self.dest, self.phases, self.nexts, self.entrypoints)]))
        self.entrypoints = self.entrypoints[:self.n_entry]
        self.entry_index = {int(rd): j for j, rd in enumerate(self.entrypoints)}

        E, R, P, Cc, I, r = self.E, self.R, self.P, self.C, self.I, self.r
        dev = self.device
        # zeros, not empty: the reference leaves these to np.empty garbage; a defined start keeps
        # runs reproducible (dead slots are never read)
        if self.layout == "transposed":
            pairs = C.c_int64()
            nat.check(self.lib.tfx_xv_pairs(h, C.byref(pairs)))
            self._t = torch.zeros((int(pairs.value), 2), dtype=torch.float32, device=dev)
            # the ring-shaped staging copy behind `xv` / `x` / `v` / `w` / load_state is made on first
            # use: a rollout that never looks at the cars does not pay a second copy of them
            self._ring = None
            self._ringw = None
            self._ringa = None
            self._tw = torch.zeros((self._t.shape[0],), dtype=torch.float32, device=dev) if P == 3 else None
        else:
            self._t = None
            self._ring = torch.zeros((E, R, Cc, 2), dtype=torch.float32, device=dev)
            # spawn ticks (validate mode): ring-shaped like the cars
            self._ringw = torch.zeros((E, R, Cc), dtype=torch.float32, device=dev) if P == 3 else None
            self._ringa = None
            self._tw = None
        # transposed handles: `_epoch` counts calls that move the cars; the staging copy mirrors the
        # device state only while `_stage_epoch` equals it
        self._epoch = 0
        self._stage_epoch = -1
        self.leading = torch.ones((E, R), dtype=torch.int32, device=dev)
        self.lastcar = torch.ones((E, R), dtype=torch.int32, device=dev)
        # what a caller reads back after a step lives in ONE buffer (obs | rewards | done_tick | n_trips |
        # done) so that the single-env surface needs one device-to-host copy per step
        self.trip_cap = int(trip_cap)
        lay, off = {}, 0
        for name, dtype, shape in (("obs", np.int32, (E, self.obs_len)), ("rewards", np.float32, (E, I)),
                                   ("done_tick", np.int32, (E,)), ("n_trips", np.int32, (E,)),
                                   ("done", np.uint8, (E,))):
            lay[name] = (off, dtype, shape)
            off += int(np.prod(shape)) * np.dtype(dtype).itemsize
        self._out = torch.zeros(((off + 15) // 16 * 16,), dtype=torch.uint8, device=dev)
        self._out_layout = lay

        def view(name, tdtype):
            o, dtype, shape = lay[name]
            n = int(np.prod(shape)) * np.dtype(dtype).itemsize
            return self._out[o:o + n].view(tdtype).view(*shape)
        self.obs = view("obs", torch.int32)
        self.rewards = view("rewards", torch.float32)
        self.done_tick = view("done_tick", torch.int32)
        self.done = view("done", torch.uint8)
        self.n_trips = view("n_trips", torch.int32) if validate else None
        self.waiting = torch.zeros((E, r), dtype=torch.int32, device=dev)
        self.passed_dst = torch.zeros((E, I), dtype=torch.uint8, device=dev)
        self.trip_times = torch.zeros((E, self.trip_cap), dtype=torch.float32, device=dev) if validate else None
        self._cars = torch.zeros((E, R), dtype=torch.int32, device=dev)
        # the queries' default tensors, made on first use: (query, key) -> its tuple of QUERIES; ("frames", (frames, px)) ->
        # the picture, which holds the background after that
        self._planes = {}
        b = nat.TfxBuffers()
        b.xv = _ptr(self._t if self._t is not None else self._ring)
        b.w = _ptr(self._tw if self._tw is not None else self._ringw)
        b.leading, b.lastcar = _ptr(self.leading), _ptr(self.lastcar)
        b.obs, b.rewards, b.waiting = _ptr(self.obs), _ptr(self.rewards), _ptr(self.waiting)
        b.passed_dst, b.done_tick = _ptr(self.passed_dst), _ptr(self.done_tick)
        b.trip_times, b.n_trips, b.trip_cap = _ptr(self.trip_times), _ptr(self.n_trips), self.trip_cap
        nat.check(self.lib.tfx_bind_buffers(h, C.byref(b)))
        self._action_buf = None
        self._spawn_buf = None
        self._held_action = None
        self._held_spawn = None
        self._action_bound = None
        self._spawn_bound = None
        self._rows_key = None       # (pointer, S, per_tick) of the spawn-row buffer bound last (heterogeneous cars)
        self._stages = {}
        self.tick = 0
        # episodes on the device (set_episodes): None while off
        self.ep_return = self.ep_len = self.final_return = self.final_len = self.truncated = self.ep_index = None
        self.episode_pool = None    # the engine restarts clone from (set_episode_pool)
        # demand profiles (set_demand): None while another spawn rule is bound
        self._clear_demand()
        # views with the reference's attribute names (traffic_env.py:372-376)
        self.passed = self.obs[:, :r]
        self.detected = self.obs[:, r:2 * r]
        self.current_phase = self.obs[:, 2 * r:2 * r + I]
        self.elapsed = self.obs[:, 2 * r + I:]

    # ---- car state in the reference's ring layout -----------------------------------------------
    def _staging(self):
        if self._ring is None:
            self._ring = torch.zeros((self.E, self.R, self.C, 2), dtype=torch.float32, device=self.device)
            if self.P == 3:
                self._ringw = torch.zeros((self.E, self.R, self.C), dtype=torch.float32, device=self.device)
            if self.het:
                self._ringa = torch.zeros((self.E, self.R, self.C), dtype=torch.uint8, device=self.device)

    def drop_staging(self):
        """Free the ring-shaped staging copy of a transposed handle (it comes back on the next access)."""
        if self._t is not None:
            self._ring = None
            self._ringw = None
            self._ringa = None
            self._stage_epoch = -1

    def _export(self):
        if self._t is not None:
            self._staging()
            with torch.cuda.device(self.device):
                nat.check(self.lib.tfx_export_ring(self.h, _ptr(self._ring), _ptr(self._ringw), _ptr(self._ringa),
                                                   self._stream()))
            self._stage_epoch = self._epoch

    @property
    def xv(self):
        """[E,R,C,2] (x, v) by ring slot.  Ring layout: the live device array.  Transposed layout: a
        staging copy brought up to date by this access; write to it, then call refresh()."""
        self._export()
        return self._ring

    @property
    def w(self):
        """[E,R,C] spawn tick by ring slot (None unless planes == 3); same staging rule as `xv`."""
        if self.P != 3:
            return None
        self._export()
        return self._ringw

    @property
    def arch(self):
        """[E,R,C] uint8: row of the archetype table each ring slot's car was spawned from (None unless the
        engine has heterogeneous cars); same staging rule as `xv`."""
        if not self.het:
            return None
        self._export()
        return self._ringa

    @property
    def x(self):
        return self.xv[..., 0]

    @property
    def v(self):
        return self.xv[..., 1]

    def __del__(self):
        h, self.h = getattr(self, "h", None), None
        if h:
            try:
                self.lib.tfx_destroy(h)
            except Exception:
                pass

    # ---- stream plumbing: kernels go on torch's current stream --------------------------------
    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    # ---- the reference's operations ----------------------------------------------------------
    def reset(self, phase_init):
        """TrafficEnv._reset (traffic_env.py:259-272); phase_init int[E,I] or [I]."""
        ph = torch.as_tensor(np.array(np.broadcast_to(
            np.asarray(phase_init, np.int32), (self.E, self.I)))).to(self.device)
        with torch.cuda.device(self.device):
            nat.check(self.lib.tfx_reset(self.h, _ptr(ph), self._stream()))
        self._epoch += 1
        self._keep = ph
        self.tick = 0
        self.done.zero_()

    def reset_envs(self, mask, phase_init):
        """_reset for the envs selected by `mask` (bool/uint8 [E], tensor or array) only - the episode
        boundary of a batched rollout; phase_init int [E,I] (rows of unselected envs are ignored)."""
        m = mask if isinstance(mask, torch.Tensor) else torch.as_tensor(np.asarray(mask))
        m = m.to(device=self.device, dtype=torch.uint8).contiguous()
        ph = phase_init if isinstance(phase_init, torch.Tensor) else torch.as_tensor(
            np.array(np.broadcast_to(np.asarray(phase_init, np.int32), (self.E, self.I))))
        ph = ph.to(device=self.device, dtype=torch.int32).contiguous()
        with torch.cuda.device(self.device):
            nat.check(self.lib.tfx_reset_envs(self.h, _ptr(ph), _ptr(m), self._stream()))
        self._epoch += 1
        self._keep = (ph, m)
        self.done.masked_fill_(m.bool(), 0)

    def set_episodes(self, max_decisions=None, seed=0, enabled=True):
        """Episodes on the device (tfx_set_episodes, include/tfx.h): from now on every agent_step restarts the envs
        whose last decision ended their episode (phases drawn on the device; devrng.episode_phases mirrors the draw),
        runs the ticks, then accounts for the decision - all inside the decision's one submission.  max_decisions: the
        time limit in decisions (None or 0: episodes end on overflow only).  Allocates (zeroed) and exposes
            ep_return f32 [E,I], ep_len i32 [E]        the running episode
            final_return f32 [E,I], final_len i32 [E]  the episode that ended last (valid where adone | truncated)
            truncated u8 [E]                           the last decision hit the time limit (and did not overflow)
            ep_index i32 [E]                           episodes ended so far = number of the running one
        The observation agent_step returns for an env that ended is its terminal one; the env restarts at the
        beginning of the NEXT decision, under that decision's action.  In validate mode the trip log of an ended
        episode therefore stays readable until the next decision begins.  reset() / reset_envs() abandon the episode
        of the envs they reset: accumulators cleared, ep_index unmoved.  enabled=False switches the feature off again
        (the tensors are dropped)."""
        E, I, dev = self.E, self.I, self.device
        if not enabled:
            with torch.cuda.device(dev):
                nat.check(self.lib.tfx_set_episodes(self.h, 0, 0, 0, None))
            self.ep_return = self.ep_len = self.final_return = self.final_len = self.truncated = self.ep_index = None
            self._ep_keep = None
            return
        limit = 0 if max_decisions is None else int(max_decisions)
        if limit < 0:
            raise ValueError("max_decisions must be >= 0 (None / 0: no time limit)")
        self.ep_return = torch.zeros((E, I), dtype=torch.float32, device=dev)
        self.final_return = torch.zeros((E, I), dtype=torch.float32, device=dev)
        self.ep_len = torch.zeros((E,), dtype=torch.int32, device=dev)
        self.final_len = torch.zeros((E,), dtype=torch.int32, device=dev)
        self.ep_index = torch.zeros((E,), dtype=torch.int32, device=dev)
        self.truncated = torch.zeros((E,), dtype=torch.uint8, device=dev)
        b = nat.TfxEpisodeBuffers()
        b.ep_return, b.ep_len = _ptr(self.ep_return), _ptr(self.ep_len)
        b.final_return, b.final_len = _ptr(self.final_return), _ptr(self.final_len)
        b.truncated, b.ep_index = _ptr(self.truncated), _ptr(self.ep_index)
        with torch.cuda.device(dev):
            nat.check(self.lib.tfx_set_episodes(self.h, 1, limit, int(seed) & 0xFFFFFFFFFFFFFFFF, C.byref(b)))
        self._ep_keep = b

    def set_episode_pool(self, pool):
        """Warm restarts (tfx_set_episode_pool, include/tfx.h): while episodes are on, an env that ended restarts as a
        clone of an env of `pool` - another engine of the same world, warmed up by the caller - instead of empty; which
        one is rule 3 (devrng.episode_pool_slots).  The restart is clone_envs(..., streams=False, episodes=False) for the
        envs that ended, inside the decision's submission; the pool is read when the restart runs, never written.  None
        detaches.  The engine keeps a reference to the pool while it is attached."""
        with torch.cuda.device(self.device):
            nat.check(self.lib.tfx_set_episode_pool(self.h, None if pool is None else pool.h))
        self.episode_pool = pool

    def clone_envs(self, src_of_env, source=None, streams=False, episodes=False):
        """Env e becomes a copy of env src_of_env[e] of `source` (another engine of the same world; default: this
        one), -1 leaves env e alone: tfx_clone_envs (include/tfx.h), one launch on the current stream, no host
        synchronisation.  src_of_env: int [E], tensor (stays on the device) or array.  streams: the clone also
        continues the source's on-device arrival stream (set_poisson / set_regular) - same cars on the same roads from
        then on; episodes: the running episode's accounting travels too (set_episodes).  In place a source must not
        itself be overwritten: envs that break the rule (or whose index is out of range) are left untouched and
        counted, see clone_skipped() and devrng.clone_plan.  Returns the index tensor as bound."""
        src = self if source is None else source
        idx = src_of_env if isinstance(src_of_env, torch.Tensor) else torch.as_tensor(np.asarray(src_of_env, np.int32))
        idx = idx.to(device=self.device, dtype=torch.int32).contiguous()
        if idx.numel() != self.E:
            raise ValueError("src_of_env must hold one index per env (%d), got %d" % (self.E, idx.numel()))
        flags = (nat.CLONE_STREAM if streams else 0) | (nat.CLONE_EPISODE if episodes else 0)
        with torch.cuda.device(self.device):
            nat.check(self.lib.tfx_clone_envs(self.h, src.h, _ptr(idx), flags, self._stream()))
        self._epoch += 1
        self._clone_keep = idx
        # the Python-side done flags of the envs that were cloned: those of their sources
        s = idx.long()
        ok = (s >= 0) & (s < src.E)
        sc = s.clamp(0, src.E - 1)
        if src is self:
            t = s[sc]
            ok &= (t == -1) | (t == s)
        self.done.copy_(torch.where(ok, src.done[sc], self.done))
        return idx

    def clone_skipped(self):
        """Envs earlier clone_envs() calls left untouched against the caller's wish since the last call of this
        (tfx_clone_skipped: returns and clears the device counter; synchronises the stream)."""
        n = C.c_uint64()
        with torch.cuda.device(self.device):
            nat.check(self.lib.tfx_clone_skipped(self.h, C.byref(n), self._stream()))
        return int(n.value)

    # ---- what the device queries share (one row of QUERIES each) ----------------------------------------------------
    def _tensors(self, q, key, out):
        """The tensors one call of query `q` writes, as q.tuple.  out None: those the engine allocates on first use of
        (q, key) - filled as the row says - and reuses; otherwise the caller's, every member that is not None checked
        against the row: a contiguous device tensor of the plane's dtype and shape."""
        if out is None:
            out = self._planes.get((q.name, key))
            if out is None:
                out = self._planes[(q.name, key)] = self._fresh(q, key)
            return out
        out = q.tuple(*out)
        for name, (dtype, shape, _), t in zip(q.tuple._fields, q.planes, out):
            if t is not None:
                shape = shape(self, key)
                if shape is None:
                    raise ValueError("%s(out=): %s is a plane this engine or call does not have" % (q.name, name))
                if not _is_plane(t, dtype, shape):
                    raise ValueError("%s(out=): %s must be a contiguous %s %s device tensor" % (q.name, name, dtype, list(shape)))
        return out

    def _fresh(self, q, key):
        """new tensors for every plane of query `q` that this engine has at `key`, filled as the row says"""
        planes = []
        for dtype, shape, fill in q.planes:
            shape = shape(self, key)
            if shape is None:
                planes.append(None)
            elif fill == 0:
                planes.append(torch.zeros(shape, dtype=dtype, device=self.device))
            else:
                planes.append(torch.full(shape, fill, dtype=dtype, device=self.device))
        return q.tuple(*planes)

    def _launch_report(self, fn, *ints):
        """(workgroups, wavefronts) as one of the library's tfx_*_launch calls reports them for this engine"""
        g, w = C.c_int32(), C.c_int32()
        nat.check(fn(self.h, *ints, C.byref(g), C.byref(w)))
        return int(g.value), int(w.value)

    def _env_ids(self, env_ids):
        """a caller's env numbers - a list, an array or a device tensor; None: every env in order - as (int32 device
        tensor or None, number of selections)"""
        if env_ids is None:
            return None, self.E
        if not torch.is_tensor(env_ids):
            env_ids = torch.as_tensor(np.ascontiguousarray(np.asarray(env_ids, np.int32).reshape(-1)))
        ids = env_ids.to(device=self.device, dtype=torch.int32).reshape(-1).contiguous()
        return ids, int(ids.shape[0])

    def _road_mask(self, roads, who):
        """a caller's uint8 / bool mask [R] by road id (None: every road) as a uint8 device tensor or None"""
        if roads is None:
            return None
        if not torch.is_tensor(roads):
            roads = torch.as_tensor(np.ascontiguousarray(np.asarray(roads).reshape(-1) != 0))
        mask = (roads.to(device=self.device).reshape(-1) != 0).to(torch.uint8).contiguous()
        if int(mask.shape[0]) != self.R:
            raise ValueError("%s: roads must have %d entries, one per road id" % (who, self.R))
        return mask

    def road_measures(self, halt_speed=0.1, x_from=None, accumulate=False, out=None):
        """The standard traffic measures per road, from one read-only launch over the live cars (tfx_road_measures,
        include/tfx.h; gym_traffic.devrng.road_measures states the definition in NumPy): -> RoadMeasures(n_cars,
        n_halted, queue, speed_sum), [E, R] device tensors by road id (int32 x 3, float32).  A car is in range iff
        x >= x_from (None: every car); halted iff in range and v < halt_speed; queue: the halted in-range platoon at
        the head of the road; speed_sum: float32 sum of v over the cars in range, in car order.  accumulate: added to
        the tensors instead of overwriting them (integrate over decisions by measuring between calls).  out: the
        caller's RoadMeasures (any member None: not computed); default: tensors the engine allocates once, zeroed,
        and reuses.  No host synchronisation; nothing of the env state is written."""
        q = QUERIES["road_measures"]
        out = self._tensors(q, None, out)
        b = _buffers(q, out)
        with torch.cuda.device(self.device):
            nat.check(self.lib.tfx_road_measures(self.h, float(halt_speed), float("-inf") if x_from is None else float(x_from),
                                                 C.byref(b), nat.MEASURE_ACCUMULATE if accumulate else 0, self._stream()))
        return out

    def measure_launch(self):
        """(workgroups, wavefronts) of the road_measures launch of this engine (tfx_measure_launch; tests)."""
        return self._launch_report(self.lib.tfx_measure_launch)

    def road_following(self, platoon_gap, v_min, ttc_crit, x_from=None, out=None, accumulate=False):
        """The car-following measures per road, from one read-only launch over the live cars (tfx_road_following,
        include/tfx.h; gym_traffic.devrng.road_following states the definition in NumPy): -> RoadFollowing, eleven [E, R]
        device tensors by road id - int32 counters, float32 gap_sum, gap_min, hw_sum, ttc_min, drac_max.  Car j >= 1 of
        a road pairs with its leader j-1; with g = (x_L - x_F) - l_L and dv = v_F - v_L, over the pairs whose follower has
        x >= x_from (None: every car): n_pairs; n_joined (g <= platoon_gap: platoons = n_cars - n_joined); n_overlap
        (g < 0); gap_sum, gap_min; n_hw, hw_sum (g / v_F where v_F >= v_min > 0); n_conflict (dv > 0, g > 0 and g / dv <
        ttc_crit), ttc_min and drac_max ((dv * dv) / (g + g)) over the closing pairs; n_cars: the cars in range.
        accumulate: counters and sums are added to, minima and the maximum combined with what is there, instead of
        overwritten.  out: the caller's RoadFollowing (any member None: not computed; for accumulate the caller starts
        gap_min / ttc_min at +inf and the rest at 0); default: tensors the engine allocates once - zeros, gap_min and
        ttc_min +inf - and reuses.  No host synchronisation; nothing of the env state is written."""
        q = QUERIES["road_following"]
        out = self._tensors(q, None, out)
        p = nat.TfxFollowParams(float("-inf") if x_from is None else float(x_from), float(platoon_gap), float(v_min),
                                float(ttc_crit))
        b = _buffers(q, out)
        with torch.cuda.device(self.device):
            nat.check(self.lib.tfx_road_following(self.h, C.byref(p), C.byref(b),
                                                  nat.FOLLOW_ACCUMULATE if accumulate else 0, self._stream()))
        return out

    def follow_launch(self):
        """(workgroups, wavefronts) of the road_following launch of this engine (tfx_follow_launch; tests)."""
        return self._launch_report(self.lib.tfx_follow_launch)

    def road_ends(self, k=4, pad_dist=float("inf"), pad_v=0.0, pad_tail_x=float("inf"), out=None):
        """The two ends of every road, from one read-only launch (tfx_road_ends, include/tfx.h; gym_traffic.devrng.road_ends
        states the definition in NumPy): -> RoadEnds(n_cars, n_heads int32 [E, R]; heads float32 [E, R, k, 2]; head_rows
        uint8 [E, R, k]; tail float32 [E, R, 2]; tail_row uint8 [E, R]), device tensors by road id.  heads[..., j, :] is
        (length - x, v) of car j from the head, in ring order, for j < min(n, k) and (pad_dist, pad_v) beyond; tail is
        (x, v) of the road's last car, (pad_tail_x, pad_v) on an empty road; the rows are the cars' archetype rows (0 on
        single-archetype engines), 255 where there is no car.  k: 1 .. 16.  out: the caller's RoadEnds (any member None:
        not computed); default: tensors the engine allocates once per k and reuses.  No host synchronisation; nothing of
        the env state is written."""
        k = int(k)
        if not 1 <= k <= nat.MAX_HEADS:
            raise ValueError("road_ends: k %d is outside 1..%d" % (k, nat.MAX_HEADS))
        q = QUERIES["road_ends"]
        out = self._tensors(q, k, out)
        p = nat.TfxEndsParams(k, float(pad_dist), float(pad_v), float(pad_tail_x))
        b = _buffers(q, out)
        with torch.cuda.device(self.device):
            nat.check(self.lib.tfx_road_ends(self.h, C.byref(p), C.byref(b), 0, self._stream()))
        return out

    def ends_launch(self, k):
        """(workgroups, wavefronts) of the road_ends launch of this engine for k cars a road (tfx_ends_launch; tests)."""
        return self._launch_report(self.lib.tfx_ends_launch, int(k))

    def car_list(self, env_ids=None, roads=None, max_cars=None, out=None):
        """Every live car of chosen envs as one flat run, from one read-only launch (tfx_car_list, include/tfx.h;
        gym_traffic.devrng.car_list states the definition in NumPy): -> CarList(n, offsets, xv, road, row, spawn), device
        tensors.  env_ids: a list, an array or an int32 device tensor of env numbers (None: every env in order; repeats are
        fine; an id outside [0, E) contributes no cars); roads: a uint8 / bool mask [R] by road id (None: every road).
        offsets int32 [n_sel * R + 1] is the exclusive prefix sum of the road counts in (selection s, road id) order - taken
        here in torch from leading / lastcar with tile_road's clamp - and n = offsets[-1] the total, a device scalar.  Car
        j from the head of (s, road), in ring order, is entry offsets[s * R + road] + j: xv float32 [.., 2] its (x, v), road
        int32 its key s * R + road id, row uint8 its archetype row (0 on single-archetype engines), spawn float32 its spawn
        tick (None on engines without a spawn plane).
        max_cars = an int: the planes have that length and nothing synchronises with the host; entries from min(n, max_cars)
        on are not written (fresh tensors are zeroed).  max_cars = None: n is read back once - ONE host synchronisation -
        and the planes are sized exactly.  out: the caller's (xv, road, row, spawn) of one length, any member None: not
        computed; then max_cars is that length.  Nothing of the env state is written."""
        q, E, R, dev = QUERIES["car_list"], self.E, self.R, self.device
        ld, lc = self.leading, self.lastcar
        count = (lc - ld + (ld > lc).to(torch.int32) * (self.C - 1)).clamp_(0, self.C - 1)
        ids, n_sel = self._env_ids(env_ids)
        if n_sel < 1:
            raise ValueError("car_list: no env chosen")
        if ids is not None:
            shown = (ids >= 0) & (ids < E)
            count = count.index_select(0, torch.where(shown, ids, torch.zeros_like(ids)).long()) * shown[:, None]
        mask = self._road_mask(roads, "car_list")
        if mask is not None:
            count = count * mask[None, :]
        if n_sel * R + 1 > 2 ** 31 - 1:
            raise ValueError("car_list: %d selections of %d roads do not fit int32 offsets" % (n_sel, R))
        offsets = torch.zeros((n_sel * R + 1,), dtype=torch.int32, device=dev)
        torch.cumsum(count.reshape(-1), 0, dtype=torch.int32, out=offsets[1:])
        n = offsets[-1]
        if out is not None:
            planes = list(out)
            sizes = {int(t.shape[0]) for t in planes if t is not None}
            if len(planes) != 4 or len(sizes) != 1:
                raise ValueError("car_list(out=): (xv, road, row, spawn) of one length are needed, any of them None")
            cap = sizes.pop() if max_cars is None else int(max_cars)
            # (refused: a length that is not max_cars; spawn on an engine that keeps no spawn ticks, planes == 2)
            planes = self._tensors(q, cap, planes)
        else:
            cap = int(n) if max_cars is None else int(max_cars)      # int(n): the one host synchronisation
            if cap < 0:
                raise ValueError("car_list: max_cars %d is negative" % cap)
            planes = self._fresh(q, cap)
        if cap > 2 ** 31 - 1:
            raise ValueError("car_list: %d entries do not fit int32 offsets" % cap)
        b = _buffers(q, planes)
        with torch.cuda.device(dev):
            nat.check(self.lib.tfx_car_list(self.h, _ptr(ids), n_sel, _ptr(mask), _ptr(offsets), cap, C.byref(b), 0,
                                            self._stream()))
        return CarList(n, offsets, *planes)

    def car_list_launch(self, n_sel):
        """(workgroups, wavefronts) of the car_list launch of this engine for n_sel chosen envs (tfx_car_list_launch;
        tests)."""
        return self._launch_report(self.lib.tfx_car_list_launch, int(n_sel))

    def digest_parts(self):
        """every TFX_DIGEST_* part this engine has: all of them, without SPAWN where there is no side plane (planes == 2)
        and without ROWS where there is no archetype table (every row is 0)"""
        parts = nat.DIGEST_CARS | nat.DIGEST_RING | nat.DIGEST_LIGHTS | nat.DIGEST_OBS
        if self.het:
            parts |= nat.DIGEST_ROWS
        if self.P == 3:
            parts |= nat.DIGEST_SPAWN
        return parts

    def state_digest(self, envs=None, parts=None, roads=None, per_road=False, out=None):
        """A 64-bit fingerprint of the state of chosen envs, from one read-only launch over their live cars
        (tfx_state_digest, include/tfx.h, which states the rule; gym_traffic.devrng.state_digest is the definition in
        NumPy) -> int64 [n_sel] device tensor holding the bits of the uint64 digests; per_road=True: (env, road int64
        [n_sel, R]), a digest per road id as well.  Two envs - of this engine or of any other, whatever its layout, E
        or sharding - whose chosen parts hold the same bits have equal digests; a fingerprint, not a cryptographic hash.
        envs: a list, an array or an int32 device tensor of env numbers (None: every env in order; repeats are fine; an id
        outside [0, E) gives 0); parts: a sum of nat.DIGEST_CARS | ROWS | SPAWN | RING | LIGHTS | OBS (None: every part
        this engine has, digest_parts()); roads: a uint8 / bool mask [R] by road id (None: every road; a masked-out road
        enters no digest and its road word is 0).  out: the caller's int64 tensor [n_sel], or with per_road the pair
        (env, road); default: tensors the engine keeps per (n_sel, per_road) and reuses - clone() what must last.  No
        host synchronisation when envs is None or a device tensor; nothing of the env state is written."""
        ids, n_sel = self._env_ids(envs)
        if n_sel < 1:
            raise ValueError("state_digest: no env chosen")
        parts = self.digest_parts() if parts is None else int(parts)
        if parts <= 0 or parts & ~nat.DIGEST_ALL:
            raise ValueError("state_digest: parts 0x%x is empty or has unknown bits" % parts)
        if parts & nat.DIGEST_SPAWN and self.P != 3:
            raise ValueError("state_digest: DIGEST_SPAWN needs the spawn plane (planes == 3: validate mode or heterogeneous cars)")
        mask = self._road_mask(roads, "state_digest")
        key = ("state_digest", (n_sel, bool(per_road)))
        if out is None:
            out = self._planes.get(key)
            if out is None:
                out = self._planes[key] = (
                    torch.zeros((n_sel,), dtype=torch.int64, device=self.device),
                    torch.zeros((n_sel, self.R), dtype=torch.int64, device=self.device) if per_road else None)
            env, road = out
        else:
            env, road = tuple(out) if per_road else (out, None)
            if not _is_plane(env, torch.int64, (n_sel,)) or (per_road and not _is_plane(road, torch.int64, (n_sel, self.R))):
                raise ValueError("state_digest(out=): contiguous int64 device tensors [%d]%s are needed"
                                 % (n_sel, " and [%d, %d]" % (n_sel, self.R) if per_road else ""))
        with torch.cuda.device(self.device):
            nat.check(self.lib.tfx_state_digest(self.h, _ptr(ids), n_sel, _ptr(mask), parts, _ptr(env), _ptr(road), 0,
                                                self._stream()))
        return (env, road) if per_road else env

    def digest_launch(self, n_sel):
        """(workgroups, wavefronts) of the state_digest launch of this engine for n_sel chosen envs (tfx_digest_launch;
        tests)."""
        return self._launch_report(self.lib.tfx_digest_launch, int(n_sel))

    def _dev(self, who, a, dtype, np_dtype, shape, what):
        """argument `what` of method `who` - a caller's tensor or array-like - as a contiguous device tensor of this dtype
        and shape (None stays None)"""
        if a is None:
            return None
        if not torch.is_tensor(a):
            a = torch.as_tensor(np.ascontiguousarray(np.asarray(a, np_dtype)))
        a = a.to(device=self.device, dtype=dtype).contiguous()
        if tuple(a.shape) != tuple(shape):
            raise ValueError("%s: %s must have shape %s, not %s" % (who, what, list(shape), list(a.shape)))
        return a

    def put_cars(self, offsets, xv=None, row=None, spawn=None, env_ids=None, roads=None, leading=None, lead_x=None,
                 spawn_shift=0, count_lost=False):
        """The cars of chosen envs written from one flat run, in one launch and with no host synchronisation - the inverse
        of car_list (tfx_put_cars, include/tfx.h; gym_traffic.devrng.put_cars states the definition in NumPy).  offsets
        int32 [n_sel * R + 1], xv float32 [cap, 2], row uint8 [cap] (None: row 0), spawn float32 [cap] (None: tick 0; ignored
        by engines without a spawn plane) are a list as car_list returns it - device tensors or array-likes; a CarList may
        be passed whole as the first argument.  Road `road` of env env_ids[s] (None: env s) then holds the cars at
        offsets[s * R + road] .. offsets[s * R + road + 1], head first, at most C - 2 of them and none from outside [0, cap).
        roads: a uint8 / bool mask [R] (None: every road) - the others keep their cars; leading int32 [n_sel, R]: the roads'
        new `leading` (None or no ring index: unchanged); lead_x float32 [n_sel, R]: the x the leader's slot shows (None:
        +inf, as after a reset); spawn_shift: added to every spawn tick (a list taken at another clock).  env_ids must be
        distinct: a host-side list with repeats raises.  count_lost: cars that did not fit are added to the counter
        put_lost() reads.  Nothing else of the engine's state changes and no refresh() is needed."""
        if isinstance(offsets, CarList):
            cl = offsets
            offsets, xv = cl.offsets, cl.xv if xv is None else xv
            row = cl.row if row is None else row
            spawn = cl.spawn if spawn is None else spawn
        if xv is None:
            raise ValueError("put_cars: xv is needed")
        R, dev = self.R, self.device
        if not torch.is_tensor(offsets):
            offsets = torch.as_tensor(np.ascontiguousarray(np.asarray(offsets, np.int32).reshape(-1)))
        offsets = offsets.to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
        n_keys = int(offsets.shape[0]) - 1
        if n_keys < R or n_keys % R:
            raise ValueError("put_cars: offsets must hold n_sel * %d + 1 entries, not %d" % (R, n_keys + 1))
        n_sel = n_keys // R
        if env_ids is not None and not torch.is_tensor(env_ids):
            env_ids = np.asarray(env_ids, np.int64).reshape(-1)
            shown = env_ids[(env_ids >= 0) & (env_ids < self.E)]
            if len(np.unique(shown)) != len(shown):
                raise ValueError("put_cars: env_ids must be distinct")
        ids, n_ids = self._env_ids(env_ids)
        if ids is not None and n_ids != n_sel:
            raise ValueError("put_cars: %d env ids for offsets of %d selections" % (n_ids, n_sel))
        if ids is None and n_sel > self.E:
            raise ValueError("put_cars: offsets of %d selections for %d envs" % (n_sel, self.E))
        mask = self._road_mask(roads, "put_cars")
        if not torch.is_tensor(xv):
            xv = torch.as_tensor(np.ascontiguousarray(np.asarray(xv, np.float32).reshape(-1, 2)))
        xv = xv.to(device=dev, dtype=torch.float32).contiguous()
        cap = int(xv.shape[0])
        if xv.dim() != 2 or xv.shape[1] != 2 or cap > 2 ** 31 - 1:
            raise ValueError("put_cars: xv must be [cap, 2] with cap below 2^31")
        row = self._dev("put_cars", row, torch.uint8, np.uint8, (cap,), "row")
        spawn = self._dev("put_cars", spawn, torch.float32, np.float32, (cap,), "spawn") if self.P == 3 else None
        leading = self._dev("put_cars", None if leading is None else leading.reshape(-1) if torch.is_tensor(leading)
                            else np.asarray(leading).reshape(-1), torch.int32, np.int32, (n_keys,), "leading")
        lead_x = self._dev("put_cars", None if lead_x is None else lead_x.reshape(-1) if torch.is_tensor(lead_x)
                           else np.asarray(lead_x).reshape(-1), torch.float32, np.float32, (n_keys,), "lead_x")
        if count_lost and getattr(self, "_put_lost", None) is None:
            self._put_lost = torch.zeros((1,), dtype=torch.int64, device=dev)
        if cap == 0:
            xv = torch.zeros((1, 2), dtype=torch.float32, device=dev)      # (a pointer to pass: no entry of it is read)
        b = nat.TfxPutBuffers(_ptr(xv), _ptr(row), _ptr(spawn), _ptr(leading), _ptr(lead_x))
        self._epoch += 1
        with torch.cuda.device(dev):
            nat.check(self.lib.tfx_put_cars(self.h, _ptr(ids), n_sel, _ptr(mask), _ptr(offsets), cap, C.byref(b),
                                            int(spawn_shift), _ptr(self._put_lost) if count_lost else None, 0,
                                            self._stream()))
        # (the launch reads these after the call returns: the caching allocator hands a freed block out again to work on
        # the same stream only, which is ordered behind the launch)
        self._put_keep = (ids, mask, offsets, xv, row, spawn, leading, lead_x)

    def put_lost(self):
        """Cars earlier put_cars(count_lost=True) calls could not place - runs longer than a road holds or cut by the
        planes' length - since the last call of this: reads and clears the device counter; synchronises."""
        t = getattr(self, "_put_lost", None)
        if t is None:
            return 0
        n = int(t.item())
        t.zero_()
        return n

    # the bound per-env rows pack_envs gathers by index
    _PACK_ROWS = ("obs", "rewards", "waiting", "passed_dst", "done_tick", "done")

    def pack_envs(self, envs):
        """Everything a caller can see of the chosen envs as a plain dict of device tensors: the car list (offsets, xv,
        row, spawn) with the roads' `leading`, the rows of obs, rewards, waiting, passed_dst, done_tick and done, with a
        trip log its rows and n_trips, and the clock (`tick`), grid and capacity it was taken at.  One car_list launch plus
        torch indexing; the total number of cars is read back once.  The arrival stream's position, the greedy
        controller's held action and the episode accounting are not in it (they travel through clone_envs only)."""
        if not torch.is_tensor(envs):
            envs = torch.as_tensor(np.ascontiguousarray(np.asarray(envs, np.int64).reshape(-1)))
        idx = envs.to(device=self.device, dtype=torch.int64).reshape(-1)
        cl = self.car_list(env_ids=idx.to(torch.int32))
        packed = dict(offsets=cl.offsets, xv=cl.xv, row=cl.row, spawn=cl.spawn, leading=self.leading[idx].clone(),
                      tick=int(self.tick), grid=(self.m, self.n, float(self.cfg.length)), capacity=self.C)
        for k in self._PACK_ROWS:
            packed[k] = getattr(self, k)[idx].clone()
        if self.n_trips is not None:
            packed["n_trips"] = self.n_trips[idx].clone()
            packed["trip_times"] = self.trip_times[idx].clone()
        return packed

    def unpack_envs(self, envs, packed):
        """envs[s] of this engine receives selection s of what pack_envs returned - of this engine or of another one on the
        same grid, whatever its E and capacity: one put_cars launch plus torch index writes, no host synchronisation.
        Cars that do not fit are counted in put_lost(); spawn ticks and the done_tick stamp are rebased by the difference
        of the two clocks; the trip log is cut to this engine's trip_cap.  envs must be distinct.  -> the ids as an int64
        device tensor."""
        grid = (self.m, self.n, float(self.cfg.length))
        if tuple(packed["grid"]) != grid:
            raise ValueError("unpack_envs: packed on grid %r, this engine is %r" % (tuple(packed["grid"]), grid))
        host_ids = None if torch.is_tensor(envs) else np.asarray(envs, np.int64).reshape(-1)
        idx = (envs if host_ids is None else torch.as_tensor(np.ascontiguousarray(host_ids))).to(
            device=self.device, dtype=torch.int64).reshape(-1)
        if int(idx.shape[0]) != int(packed["leading"].shape[0]):
            raise ValueError("unpack_envs: %d envs for %d packed ones" % (int(idx.shape[0]), int(packed["leading"].shape[0])))
        dt = int(self.tick) - int(packed["tick"])
        self.put_cars(packed["offsets"], packed["xv"], row=packed["row"], spawn=packed["spawn"],
                      env_ids=host_ids if host_ids is not None else idx.to(torch.int32), leading=packed["leading"],
                      spawn_shift=dt, count_lost=True)
        for k in self._PACK_ROWS:
            src = packed[k].to(self.device)
            if k == "done_tick":
                src = torch.where(src != 0, src + dt, src)      # (a stamp: tick + 1 of a past tick, 0 = never)
            getattr(self, k)[idx] = src
        if self.n_trips is not None and "n_trips" in packed:
            n = min(self.trip_cap, int(packed["trip_times"].shape[1]))
            self.n_trips[idx] = packed["n_trips"].to(self.device)
            self.trip_times[idx, :n] = packed["trip_times"].to(self.device)[:, :n]
        return idx

    def put_launch(self, n_sel):
        """(workgroups, wavefronts) of the put_cars launch of this engine for n_sel chosen envs (tfx_put_launch; tests)."""
        return self._launch_report(self.lib.tfx_put_launch, int(n_sel))

    def car_ages(self, accumulate=False, out=None):
        """How long every live car has been on the map, per road, from one read-only launch over the side plane
        (tfx_car_ages, include/tfx.h; gym_traffic.devrng.car_ages states the definition in NumPy): -> CarAges(n_cars
        int32, age_sum int64, age_max int32), [E, R] device tensors by road id.  Ages are in ticks at the engine's device
        clock - twice the seconds advance_hack would log if the car left the map now.  accumulate: n_cars and age_sum
        are added to and age_max is maxed instead of overwritten.  out: the caller's CarAges (any member None: not
        computed); default: tensors the engine allocates once, zeroed, and reuses.  Needs the side plane (planes == 3:
        validate mode or heterogeneous cars).  No host synchronisation; nothing of the env state is written."""
        q = QUERIES["car_ages"]
        out = self._tensors(q, None, out)
        b = _buffers(q, out)
        with torch.cuda.device(self.device):
            nat.check(self.lib.tfx_car_ages(self.h, C.byref(b), nat.TRAVEL_ACCUMULATE if accumulate else 0, self._stream()))
        return out

    def ages_launch(self):
        """(workgroups, wavefronts) of the car_ages launch of this engine (tfx_ages_launch; tests)."""
        return self._launch_report(self.lib.tfx_ages_launch)

    def trip_stats(self, edges=None, cursor=None, accumulate=False, out=None):
        """The finished trips of every env, reduced on the device where they are logged (tfx_trip_stats, include/tfx.h;
        gym_traffic.devrng.trip_stats states the rule in NumPy): -> TripStats(count int32, tick_sum int64, tick_max
        int32, lost int32 [E], hist int32 [E, n_bins] or None).  Trips count in ticks (seconds * 2).  edges: n_bins + 1
        non-decreasing ints in ticks (host), 1 .. 32 bins; None: no histogram.  cursor: the caller's int32 [E] device
        tensor - only the log entries from cursor[e] on are taken and cursor[e] becomes n_trips[e]; an env whose log is
        shorter than its cursor is read from the start; zero the cursor of the envs you reset.  None: the whole log.
        lost: trips that happened but fell off the end of the log (trip_cap).  accumulate: sums and counts are added to
        and tick_max is maxed.  out: the caller's TripStats (any member None: not computed); default: tensors the engine
        allocates once per n_bins, zeroed, and reuses.  Needs validate mode.  No host synchronisation."""
        e = None if edges is None else np.ascontiguousarray(np.asarray(edges, np.int32).reshape(-1))
        B = 0 if e is None else len(e) - 1
        if e is not None and not 1 <= B <= nat.MAX_TRIP_BINS:
            raise ValueError("trip_stats: %d edges - 2 .. %d make 1 .. %d bins" % (len(e), nat.MAX_TRIP_BINS + 1,
                                                                                  nat.MAX_TRIP_BINS))
        q = QUERIES["trip_stats"]
        out = self._tensors(q, B, out)
        if cursor is not None and not _is_plane(cursor, torch.int32, (self.E,)):
            raise ValueError("trip_stats(cursor=): a contiguous int32 [%d] device tensor is needed" % self.E)
        b = _buffers(q, out)
        ep = None if e is None else e.ctypes.data_as(C.POINTER(C.c_int32))
        with torch.cuda.device(self.device):
            nat.check(self.lib.tfx_trip_stats(self.h, ep, B, _ptr(cursor), C.byref(b),
                                              nat.TRAVEL_ACCUMULATE if accumulate else 0, self._stream()))
        return out

    def road_cells(self, edges, accumulate=False, out=None):
        """Cars and speeds per cell of road, from one read-only launch over the live cars (tfx_road_cells, include/tfx.h;
        gym_traffic.devrng.road_cells states the definition in NumPy): -> RoadCells(n_cars int32, speed_sum float32),
        [E, R, B] device tensors by road id and cell.  edges: B + 1 strictly ascending float32 values (host; -inf / +inf
        allowed at the ends, devrng.cell_edges makes uniform ones); a car is in cell b iff edges[b] <= x < edges[b + 1];
        speed_sum: float32 sum of v over the cell's cars, in car order.  accumulate: added to the tensors instead of
        overwriting them.  out: the caller's RoadCells (a member None: not computed); default: tensors the engine
        allocates once per B, zeroed, and reuses.  No host synchronisation; nothing of the env state is written."""
        e = np.ascontiguousarray(np.asarray(edges, np.float32).reshape(-1))
        B = len(e) - 1
        if not 1 <= B <= nat.MAX_CELLS:
            raise ValueError("road_cells: %d edges - 2 .. %d make 1 .. %d cells" % (len(e), nat.MAX_CELLS + 1, nat.MAX_CELLS))
        q = QUERIES["road_cells"]
        out = self._tensors(q, B, out)
        b = _buffers(q, out)
        with torch.cuda.device(self.device):
            nat.check(self.lib.tfx_road_cells(self.h, e.ctypes.data_as(C.POINTER(C.c_float)), B, C.byref(b),
                                              nat.CELLS_ACCUMULATE if accumulate else 0, self._stream()))
        return out

    def cells_launch(self, n_cells):
        """(workgroups, wavefronts) of the road_cells launch of this engine for n_cells cells (tfx_cells_launch; tests)."""
        return self._launch_report(self.lib.tfx_cells_launch, int(n_cells))

    def frame_size(self, px=32):
        """(H, W) of a frame at px pixels per road length (tfx_frame_size): ((m + 1) * px + 1, (n + 1) * px + 1)."""
        hh, ww = C.c_int32(), C.c_int32()
        nat.check(self.lib.tfx_frame_size(self.h, int(px), C.byref(hh), C.byref(ww)))
        return int(hh.value), int(ww.value)

    def frames(self, env_ids=None, px=32, out=None, roads_only=False):
        """Top-view pictures of chosen envs, from one read-only launch over their live cars (tfx_frames, include/tfx.h;
        gym_traffic.devrng.frames states the definition in NumPy) -> uint8 [n, H, W, 4] device tensor, bytes R, G, B, A
        ([..., :3] is RGB): white background, every road in its light's colour, every car a blue bar.  env_ids: a list,
        an array or an int32 device tensor of env numbers (None: every env; an id outside [0, E) gives a white frame;
        repeats are fine); px: pixels per road length, 8 .. 256.  out: the caller's tensor of that shape; roads_only:
        `out` already holds the background of an earlier call with the same px, write the road pixels only.  Default:
        a tensor the engine keeps per (n, px) and reuses - from its second use on only the road pixels are written.
        No host synchronisation when env_ids is None or a device tensor; nothing of the env state is written."""
        ids, n = self._env_ids(env_ids)
        px = int(px)
        if not nat.FRAME_PX_MIN <= px <= nat.FRAME_PX_MAX:
            raise ValueError("frames: px must be in %d .. %d" % (nat.FRAME_PX_MIN, nat.FRAME_PX_MAX))
        if n < 1:
            raise ValueError("frames: no env to draw")
        shape = (n,) + self.frame_size(px) + (4,)
        if out is None:
            roads_only = ("frames", (n, px)) in self._planes
            if not roads_only:
                self._planes[("frames", (n, px))] = torch.empty(shape, dtype=torch.uint8, device=self.device)
            out = self._planes[("frames", (n, px))]
        elif not _is_plane(out, torch.uint8, shape):
            raise ValueError("frames(out=): a contiguous uint8 [%d, %d, %d, 4] device tensor is needed" % shape[:3])
        with torch.cuda.device(self.device):
            nat.check(self.lib.tfx_frames(self.h, _ptr(ids), n, px, _ptr(out), nat.FRAMES_ROADS_ONLY if roads_only else 0,
                                          self._stream()))
        return out

    def frames_launch(self, n_frames, px=32):
        """(workgroups, wavefronts) of the frames launch of this engine for n_frames frames (tfx_frames_launch; tests)."""
        return self._launch_report(self.lib.tfx_frames_launch, int(n_frames), int(px))

    def head_rows(self):
        """uint8 [E,R] (host): rows at the top of each road's column that hold no car (tfx_debug_head_rows; tests)."""
        out = np.zeros((self.E, self.R), np.uint8)
        with torch.cuda.device(self.device):
            nat.check(self.lib.tfx_debug_head_rows(self.h, out.ctypes.data_as(C.c_void_p), self._stream()))
        return out

    def refresh(self, cars=None):
        """After writing xv / leading / lastcar from outside: push the ring-layout staging copy to
        the device layout (transposed handles) and rebuild the tail cache.  This route copies every ring slot of the
        whole batch; put_cars() writes the cars of chosen envs from a flat list and needs no refresh().

        The staging copy mirrors the device only until the cars move again.  A caller that kept a
        reference to `xv` / `x` / `v` / `w` across a step and wrote into it holds a STALE image: pushing
        it would overwrite the live cars, dropping it would silently lose the edit - so that raises.
        Take `eng.xv` again after the step (the access refreshes it), then write, then refresh().
        cars=False: rebuild the tail cache only (the caller changed leading / lastcar alone and wants
        the k-th car of a road to stay its k-th car); ring semantics for such a write need `_export()`
        BEFORE it (the env's DeviceViews do that)."""
        with torch.cuda.device(self.device):
            if self._t is not None and self._ring is not None and cars is not False:
                if self._stage_epoch != self._epoch:
                    raise nat.TfxError("refresh(): the ring-layout staging copy behind xv / x / v / w is stale (the cars "
                                       "moved since it was exported); read eng.xv again before editing it, call "
                                       "drop_staging() to discard it, or refresh(cars=False) to rebuild the tails only")
                nat.check(self.lib.tfx_import_ring(self.h, _ptr(self._ring), _ptr(self._ringw), _ptr(self._ringa),
                                                   self._stream()))
            nat.check(self.lib.tfx_refresh(self.h, self._stream()))

    def set_poisson(self, cars_per_tick, seed=0):
        """On-device Poisson arrivals (the reference's generator, traffic_env.py:160-164, with a
        counter-based RNG): cars_per_tick = cars_per_sec * rate for the whole env.  Heterogeneous cars: the
        stream draws every car's archetype row too (rule 1 of include/tfx.h; devrng.PoissonMirror mirrors it)."""
        from gym_traffic.devrng import gap_table
        cdf = gap_table(cars_per_tick)
        nat.check(self.lib.tfx_set_poisson(self.h, float(cars_per_tick), int(seed),
                                           cdf.ctypes.data_as(C.c_void_p), int(cdf.size)))
        self._clear_demand()
        self._spawn_bound = None
        self._rows_buf, self._rows_key = None, None

    def set_regular(self, cars_per_tick, seed=0):
        """On-device form of the reference's `regular` generator (traffic_env.py:167-176): ceil(cars_per_tick) cars
        every round(1 / cars_per_tick) ticks (Python's round, as the reference computes it), each on an entry road drawn
        from the env's Philox stream; cars_per_tick = cars_per_sec * rate for the whole env."""
        import math
        every, burst = round(1 / cars_per_tick), math.ceil(cars_per_tick)
        nat.check(self.lib.tfx_set_regular(self.h, int(every), int(burst), int(seed)))
        self._clear_demand()
        self._spawn_bound = None
        self._rows_buf, self._rows_key = None, None   # (heterogeneous cars: every car is row 0, traffic_env.py:174)

    def _clear_demand(self):
        """No demand is bound (any more): what set_demand exposes goes"""
        self.demand = self.demand_profile = self.demand_tables = None
        self.demand_row_cdf = self.demand_rows_per_road = None

    def set_demand(self, means, weights=None, seg_ticks=1, tick_offset=0, seed=0, profile_of_env=None, n_cdf=None,
                   row_weights=None):
        """Demand profiles on the device (tfx_set_demand, rule 4 of include/tfx.h): a true per-tick Poisson process whose
        mean changes over time, weighs the entry roads and differs from env to env.  means: [K][S] cars per env per tick
        of profile k in segment s (K <= 16, S <= 64 segments of seg_ticks ticks; the clock tick t is in segment
        floormod(t + tick_offset, S * seg_ticks) // seg_ticks); weights: [K][S][n_entry] (or [n_entry]) weights of the
        entry roads in entry-index order, None: equal.  profile_of_env: int32 [E] device tensor, read whenever arrivals
        are drawn - rewrite it between calls at will; None: one of zeros is made.  It is exposed as `demand_profile`, the
        tables as `demand_tables` (devrng.demand_counts mirrors the rule from them).  Replaces any earlier spawn rule.
        Heterogeneous cars (an archetype table): every car's row is drawn as well (tfx_set_demand_mixed, rule 5), by
        row_weights [K][S][n_archetypes] (or [n_archetypes]; None: equal) - the truck share of profile k in segment s;
        the table is exposed as `demand_row_cdf`, the rows kept per road and tick as `demand_rows_per_road`
        (devrng.demand_rows mirrors the rule from them).  A single-archetype engine takes no row_weights."""
        from gym_traffic.devrng import demand_row_table, demand_tables
        if row_weights is not None and not self.het:
            raise ValueError("row_weights need an engine with an archetype table (archetypes=)")
        tables = demand_tables(means, weights, n_cdf=n_cdf, n_entry=self.n_entry)
        K, S, n = tables.count_cdf.shape
        n_arch = max(1, int(self.cfg.n_archetypes))
        row_cdf = np.ascontiguousarray(demand_row_table(row_weights, K, S, n_arch), np.uint32) if self.het else None
        if profile_of_env is None:
            profile_of_env = torch.zeros((self.E,), dtype=torch.int32, device=self.device)
        prof = profile_of_env
        if not _is_plane(prof, torch.int32, (self.E,)):
            raise ValueError("profile_of_env must be a contiguous int32 [%d] device tensor" % self.E)
        cc = np.ascontiguousarray(tables.count_cdf, np.uint32)
        rc = np.ascontiguousarray(tables.road_cdf, np.uint32)
        dm = nat.TfxDemand()
        dm.n_profiles, dm.n_segments, dm.seg_ticks, dm.tick_offset, dm.n_cdf = K, S, int(seg_ticks), int(tick_offset), n
        dm.count_cdf, dm.road_cdf = cc.ctypes.data_as(C.c_void_p), rc.ctypes.data_as(C.c_void_p)
        dm.profile_of_env = _ptr(prof)
        dm.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        per_road = C.c_int32()
        with torch.cuda.device(self.device):
            if row_cdf is None:
                nat.check(self.lib.tfx_set_demand(self.h, C.byref(dm)))
            else:
                nat.check(self.lib.tfx_set_demand_mixed(self.h, C.byref(dm), row_cdf.ctypes.data_as(C.c_void_p), n_arch))
                nat.check(self.lib.tfx_demand_rows_per_road(self.h, C.byref(per_road)))
        self._clear_demand()
        self.demand_profile, self.demand_tables = prof, tables
        if row_cdf is not None:
            self.demand_row_cdf, self.demand_rows_per_road = row_cdf, int(per_road.value)
        self.demand = dict(seg_ticks=int(seg_ticks), tick_offset=int(tick_offset), seed=int(seed))
        self._spawn_bound = None
        self._rows_buf, self._rows_key = None, None

    def demand_counts(self, tick0, n_ticks, out=None):
        """int32 [n_ticks, E, n_entry] device tensor: the cars rule 4 gives every env on every entry road in clock ticks
        tick0 .. tick0 + n_ticks - 1 under the demand_profile as it stands (tfx_demand_counts: one read-only launch, no
        host synchronisation) - a preview of the demand, and what devrng.demand_counts computes on the host."""
        shape = (int(n_ticks), self.E, self.n_entry)
        if out is None:
            out = torch.empty(shape, dtype=torch.int32, device=self.device)
        elif not _is_plane(out, torch.int32, shape):
            raise ValueError("demand_counts(out=): a contiguous int32 [%d, %d, %d] device tensor" % shape)
        if shape[0] == 0:
            return out                  # (an empty tensor has no address to hand over)
        with torch.cuda.device(self.device):
            nat.check(self.lib.tfx_demand_counts(self.h, int(tick0), int(n_ticks), _ptr(out), self._stream()))
        return out

    def demand_rows(self, tick0, n_ticks, out=None):
        """(counts int32 [n_ticks, E, n_entry], rows uint8 [n_ticks, E, n_entry, demand_rows_per_road]) device tensors:
        rules 4 and 5 for clock ticks tick0 .. tick0 + n_ticks - 1 under the demand_profile as it stands
        (tfx_demand_rows: one read-only launch, no host synchronisation) - what devrng.demand_rows computes on the host
        for j < min(count, demand_rows_per_road); the entries past a road's cars are 0 here too (the tensor starts as
        zeros, the launch leaves them alone).  out: the caller's (counts, rows) pair of those shapes, rows as the caller
        left them past the cars.  TfxError -2 without a demand that draws rows."""
        if self.demand_rows_per_road is None:
            raise nat.TfxError("tfx error -2: demand: no demand that draws archetype rows is bound (set_demand on an "
                               "engine with an archetype table)")
        shape = (int(n_ticks), self.E, self.n_entry, self.demand_rows_per_road)
        if out is None:
            counts = torch.empty(shape[:3], dtype=torch.int32, device=self.device)
            rows = torch.zeros(shape, dtype=torch.uint8, device=self.device)
        else:
            counts, rows = out
            if not (_is_plane(counts, torch.int32, shape[:3]) and _is_plane(rows, torch.uint8, shape)):
                raise ValueError("demand_rows(out=): contiguous device tensors int32 [%d, %d, %d] and uint8 [%d, %d, %d, %d]"
                                 % (shape[:3] + shape))
        if rows.numel() == 0:           # (no ticks, or n_cdf = 1: no cars at all - an empty tensor has no address)
            return self.demand_counts(tick0, n_ticks, out=counts), rows
        with torch.cuda.device(self.device):
            nat.check(self.lib.tfx_demand_rows(self.h, int(tick0), int(n_ticks), _ptr(counts), _ptr(rows), self._stream()))
        return counts, rows

    def set_greedy(self, spacing=3):
        """On-device greedy controller (algorithms/greedy.py:14-16), a decision every `spacing` ticks."""
        key = ("greedy", int(spacing))
        if self._action_bound != key:
            nat.check(self.lib.tfx_set_actions(self.h, nat.ACTION_GREEDY, None, int(spacing), 0))
            self._action_bound = key

    def set_actions(self, actions=None, cycle_period=None, per_tick=False):
        """actions: int tensor/array [E,I] (or [I] broadcast; with per_tick a leading n_ticks
        dim), or cycle_period for the on-device fixed cycle.  Host arrays go through a pinned staging
        buffer into a device buffer the engine keeps per shape, held device tensors are copied into
        one, so the bound pointer - and any captured graph - stays valid from call to call; a
        per-tick device tensor is bound as it is (zero copy)."""
        if cycle_period is not None:
            key = ("cycle", int(cycle_period))
            if self._action_bound != key:      # an unchanged rule keeps the captured agent-step graph
                nat.check(self.lib.tfx_set_actions(self.h, nat.ACTION_CYCLE, None, int(cycle_period), 0))
                self._action_bound = key
            return
        a, owned = self._as_dev_i32(actions, "act_pt" if per_tick else "act")
        if per_tick:
            mode = nat.ACTION_BROADCAST if a.dim() == 2 else nat.ACTION_BUFFER
            key = ("per_tick", mode, a.data_ptr())
        else:
            mode = nat.ACTION_BROADCAST if a.dim() == 1 else nat.ACTION_BUFFER
            if not owned:
                if self._held_action is None or self._held_action.shape != a.shape:
                    self._held_action = torch.empty_like(a)
                self._held_action.copy_(a)
                a = self._held_action
            key = ("held", mode, a.data_ptr())
        self._action_buf = a
        if self._action_bound != key:
            nat.check(self.lib.tfx_set_actions(self.h, mode, _ptr(a), 0, 1 if per_tick else 0))
            self._action_bound = key

    def set_spawns(self, counts=None, period=None, per_tick=False, rows=None):
        """counts: int [E,n_entry] (with per_tick: [n_ticks,E,n_entry]); period: on-device
        one-car-every-`period`-ticks per entry road; neither: no spawns.  Buffers as in set_actions.
        rows (heterogeneous cars): uint8 [E,n_entry,S] (per_tick: [n_ticks,E,n_entry,S]) - the archetype-table
        row of the j-th car each entry road receives this tick (cars past S, or all without `rows`: row 0)."""
        if self.het and counts is not None:
            if rows is None:
                nat.check(self.lib.tfx_set_spawn_archetypes(self.h, None, 0, 0))
                self._rows_buf, self._rows_key = None, None
            else:
                r8 = torch.as_tensor(np.ascontiguousarray(rows, np.uint8)).to(self.device) if not isinstance(rows, torch.Tensor) \
                    else rows.to(device=self.device, dtype=torch.uint8).contiguous()
                self._rows_buf = r8
                key = (r8.data_ptr(), int(r8.shape[-1]), bool(per_tick))
                if self._rows_key != key:  # (an unchanged binding keeps the captured agent-step graph)
                    nat.check(self.lib.tfx_set_spawn_archetypes(self.h, _ptr(r8), int(r8.shape[-1]), 1 if per_tick else 0))
                    self._rows_key = key
        if period is not None:
            key = ("periodic", int(period))
            if self._spawn_bound != key:
                self._clear_demand()
                nat.check(self.lib.tfx_set_spawns(self.h, nat.SPAWN_PERIODIC, None, int(period), 0))
                self._spawn_bound = key
        elif counts is not None:
            c, owned = self._as_dev_i32(counts, "spawn_pt" if per_tick else "spawn")
            if per_tick:
                key = ("per_tick", c.data_ptr())
            else:
                if not owned:
                    if self._held_spawn is None or self._held_spawn.shape != c.shape:
                        self._held_spawn = torch.empty_like(c)
                    self._held_spawn.copy_(c)
                    c = self._held_spawn
                key = ("held", c.data_ptr())
            self._spawn_buf = c
            if self._spawn_bound != key:
                self._clear_demand()
                nat.check(self.lib.tfx_set_spawns(self.h, nat.SPAWN_COUNTS, _ptr(c), 0, 1 if per_tick else 0))
                self._spawn_bound = key
        elif self._spawn_bound != ("none",):
            self._clear_demand()
            nat.check(self.lib.tfx_set_spawns(self.h, nat.SPAWN_NONE, None, 0, 0))
            self._spawn_bound = ("none",)

    def set_spawn_rows(self, rows, per_tick=False):
        """Heterogeneous cars: uint8 [E,n_entry,S] (per_tick: [n_ticks,E,n_entry,S]) archetype-table row of the j-th
        car each entry road receives (tfx_set_spawn_archetypes); pairs with the count buffer already bound."""
        r8 = torch.as_tensor(np.ascontiguousarray(rows, np.uint8)).to(self.device) if not isinstance(rows, torch.Tensor) \
            else rows.to(device=self.device, dtype=torch.uint8).contiguous()
        self._rows_buf, self._rows_key = r8, None
        nat.check(self.lib.tfx_set_spawn_archetypes(self.h, _ptr(r8), int(r8.shape[-1]), 1 if per_tick else 0))

    def _as_dev_i32(self, a, key):
        """-> (int32 device tensor, owned).  Device tensors pass through (owned False).  Host arrays
        are written to a pinned staging buffer and copied asynchronously into a device buffer kept
        per (key, shape): `owned` True - the engine may bind that buffer itself."""
        if isinstance(a, torch.Tensor):
            return a.to(device=self.device, dtype=torch.int32).contiguous(), False
        a = np.ascontiguousarray(a, dtype=np.int32)
        slot = self._stages.get((key, a.shape))
        if slot is None:
            slot = [torch.empty(a.shape, dtype=torch.int32).pin_memory(),
                    torch.empty(a.shape, dtype=torch.int32, device=self.device), torch.cuda.Event(), False]
            self._stages[(key, a.shape)] = slot
        pin, dev, ev, used = slot
        if used:
            ev.synchronize()            # the previous upload from this staging buffer has left the host
        pin.numpy()[...] = a
        dev.copy_(pin, non_blocking=True)
        ev.record(torch.cuda.current_stream(self.device))
        slot[3] = True
        return dev, True

    def out_mirror(self):
        """Pinned mirror of the read-back buffer: pull() -> {'obs', 'rewards', 'done_tick', 'n_trips',
        'done'} as NumPy views, one copy + one synchronisation."""
        return PackedMirror(self.device, self._out, self._out_layout)

    def agent_mirror(self):
        """Pinned mirror of the fused decision's outputs: pull() -> {'aobs', 'areward'}."""
        if getattr(self, "_aobs", None) is None:
            raise nat.TfxError("agent_mirror() needs one agent_step() first")
        na = self.E * (2 * self.r + self.I)
        lay = {"aobs": (0, np.float32, (self.E, 2 * self.r + self.I)),
               "areward": (4 * na, np.float32, (self.E, self.I))}
        return PackedMirror(self.device, self._aout.view(torch.uint8), lay)

    def stage_inputs(self, actions, counts, per_tick=False):
        """Light actions int [E,I] and arrival counts int [E,n_entry] (per_tick: [n,E,n_entry]) from host
        arrays through ONE pinned staging buffer and ONE host-to-device copy; binds both inputs."""
        actions = np.asarray(actions, np.int32).reshape(self.E, self.I)
        counts = np.asarray(counts, np.int32)
        na = self.E * self.I
        key = ("inp", counts.shape)
        slot = self._stages.get(key)
        if slot is None:
            slot = [torch.empty((na + counts.size,), dtype=torch.int32).pin_memory(),
                    torch.empty((na + counts.size,), dtype=torch.int32, device=self.device), torch.cuda.Event(), False]
            self._stages[key] = slot
        pin, dev, ev, used = slot
        if used:
            ev.synchronize()
        h = pin.numpy()
        h[:na] = actions.ravel()
        h[na:] = counts.ravel()
        dev.copy_(pin, non_blocking=True)
        ev.record(torch.cuda.current_stream(self.device))
        slot[3] = True
        a, c = dev[:na], dev[na:]
        ka = ("held", nat.ACTION_BUFFER, a.data_ptr())
        if self._action_bound != ka:
            nat.check(self.lib.tfx_set_actions(self.h, nat.ACTION_BUFFER, _ptr(a), 0, 0))
            self._action_bound = ka
        ks = ("per_tick" if per_tick else "held", c.data_ptr())
        if self._spawn_bound != ks:
            self._clear_demand()
            nat.check(self.lib.tfx_set_spawns(self.h, nat.SPAWN_COUNTS, _ptr(c), 0, 1 if per_tick else 0))
            self._spawn_bound = ks
        self._action_buf, self._spawn_buf = a, c

    def host_mirror(self, *tensors):
        """Pinned host copies of small device tensors, refreshed together with ONE stream
        synchronisation: mirror.pull() -> list of NumPy views (valid until the next pull)."""
        return HostMirror(self.device, tensors)

    def step(self, n_ticks=1, update_done=True):
        """n_ticks x TrafficEnv._step (traffic_env.py:224-248) with the inputs set by
        set_actions / set_spawns.  Updates `done` (overflow in any of these ticks) unless the caller
        derives it from `done_tick` itself (update_done=False saves a launch)."""
        first = self.tick
        self._clock_room(int(n_ticks), "step")
        self._epoch += 1
        with torch.cuda.device(self.device):
            nat.check(self.lib.tfx_step(self.h, int(n_ticks), self._stream()))
            self.tick += int(n_ticks)
            if update_done:
                nat.check(self.lib.tfx_done(self.h, _ptr(self.done), first, self._stream()))

    def agent_step(self, n_ticks=10, remi=True):
        """One agent decision fused on the device (Repeater + Remi of traffic_test.py:27-64) with the
        inputs set by set_actions / set_spawns.  Returns (aobs f32 [E,2r+I], areward f32 [E,I],
        adone u8 [E]) - buffers owned by the engine and overwritten by the next call."""
        if getattr(self, "_aobs", None) is None:
            na, nr = self.E * (2 * self.r + self.I), self.E * self.I
            self._aout = torch.zeros((na + nr,), dtype=torch.float32, device=self.device)   # aobs | areward
            self._aobs = self._aout[:na].view(self.E, 2 * self.r + self.I)
            self._arew = self._aout[na:].view(self.E, self.I)
            # the decision's done flags ARE the engine's `done` (what reset_done() defaults to)
            self._adone = self.done
        self._clock_room(int(n_ticks), "agent_step")
        self._epoch += 1
        with torch.cuda.device(self.device):
            nat.check(self.lib.tfx_agent_step(self.h, int(n_ticks), int(bool(remi)), _ptr(self._aobs),
                                              _ptr(self._arew), _ptr(self._adone), self._stream()))
        self.tick += int(n_ticks)
        return self._aobs, self._arew, self._adone

    def move_cars(self):
        self._clock_room(1, "move_cars")
        self._epoch += 1
        with torch.cuda.device(self.device):
            nat.check(self.lib.tfx_move_cars(self.h, self._stream()))

    def advance_finished_cars(self):
        first = self.tick
        self._clock_room(1, "advance_finished_cars")
        self._epoch += 1
        with torch.cuda.device(self.device):
            nat.check(self.lib.tfx_advance_finished_cars(self.h, self._stream()))
            self.tick += 1
            nat.check(self.lib.tfx_done(self.h, _ptr(self.done), first, self._stream()))

    def remi_reward(self):
        with torch.cuda.device(self.device):
            nat.check(self.lib.tfx_remi(self.h, self._stream()))
        return self.rewards

    def cars_on_roads_flat(self):
        with torch.cuda.device(self.device):
            nat.check(self.lib.tfx_cars_on_roads(self.h, _ptr(self._cars), self._stream()))
        return self._cars

    def cars_on_roads(self):
        """[E, m, n, 4] as TrafficEnv.cars_on_roads (traffic_env.py:255-257)."""
        flat = self.cars_on_roads_flat()[:, :self.r]
        return flat.reshape(self.E, 4, self.m, self.n).permute(0, 2, 3, 1)

    def set_tick(self, tick):
        """The clock's domain is 0 .. nat.TICK_MAX (include/tfx.h); checked here as well: the C ABI takes an int32, and
        ctypes would wrap a Python int that does not fit one."""
        if not 0 <= int(tick) <= nat.TICK_MAX:
            raise nat.TfxError("tfx error %d: tick %d is outside the clock's domain 0 .. TFX_TICK_MAX = %d"
                               % (nat.EINVAL, int(tick), nat.TICK_MAX))
        nat.check(self.lib.tfx_set_tick(self.h, int(tick)))
        self.tick = int(tick)

    def _clock_room(self, n, call):
        """the handle's own check (csrc/tfx_handle.hpp:clock_room) on the mirror `tick`: nothing is enqueued, nothing
        changes when a call would run a tick past the clock's domain"""
        if self.tick + n > nat.TICK_MAX:
            raise nat.TfxError("tfx error %d: %s: the clock stands at %d and %d more tick(s) would take it past "
                               "TFX_TICK_MAX = %d (set_tick or reset move it back)" % (nat.ESTATE, call, self.tick, n, nat.TICK_MAX))

    def vehicle_updates(self):
        out = C.c_uint64()
        nat.check(self.lib.tfx_vehicle_updates(self.h, C.byref(out), self._stream()))
        return int(out.value)

    def reset_counters(self):
        nat.check(self.lib.tfx_reset_counters(self.h, self._stream()))

    def profile(self, max_ticks):
        """Record HIP events around the kernels of the next `max_ticks` ticks (0 = off)."""
        nat.check(self.lib.tfx_profile(self.h, int(max_ticks)))

    def profile_read(self):
        mv, ad, n = C.c_double(), C.c_double(), C.c_int32()
        nat.check(self.lib.tfx_profile_read(self.h, C.byref(mv), C.byref(ad), C.byref(n)))
        return dict(move_ms=mv.value, advance_ms=ad.value, ticks=n.value)

    def fastdiv_status(self):
        en, bad = C.c_int32(), C.c_uint64()
        nat.check(self.lib.tfx_fastdiv_status(self.h, C.byref(en), C.byref(bad)))
        return dict(enabled=bool(en.value), mismatches=int(bad.value))

    def fused_ticks(self):
        """(ticks run so far by the LDS-resident multi-tick kernel k_res, whether this handle's envs fit it)."""
        n, cap = C.c_int64(), C.c_int32()
        nat.check(self.lib.tfx_fused_ticks(self.h, C.byref(n), C.byref(cap)))
        return int(n.value), bool(cap.value)

    def pair_ticks(self):
        """Ticks run so far as two-tick passes (k_move_tt + k_edge; tfx_pair_ticks)."""
        n = C.c_int64()
        nat.check(self.lib.tfx_pair_ticks(self.h, C.byref(n)))
        return int(n.value)

    def tail_ticks(self):
        """Ticks of those whose pair was finished by ONE launch, a workgroup per env (k_tail; tfx_tail_ticks)."""
        n = C.c_int64()
        nat.check(self.lib.tfx_tail_ticks(self.h, C.byref(n)))
        return int(n.value)

    def slow_pairs(self):
        """Env-pairs of fused decisions that ran one tick at a time because the first tick could overflow (tfx_slow_pairs)."""
        n = C.c_uint64()
        nat.check(self.lib.tfx_slow_pairs(self.h, C.byref(n), self._stream()))
        return int(n.value)

    def split_ticks(self):
        """Ticks of step() calls that ran as two halves of the env range on two streams (tfx_split_ticks)."""
        n = C.c_int64()
        nat.check(self.lib.tfx_split_ticks(self.h, C.byref(n)))
        return int(n.value)

    def step_kernel(self):
        """Name of the kernel that moved the cars in the last tick ('k_move_t', 'k_res', ...)."""
        return self.lib.tfx_step_kernel(self.h).decode()

    def launch_info(self):
        v = [C.c_int32() for _ in range(3)]
        nat.check(self.lib.tfx_launch_info(self.h, *[C.byref(x) for x in v]))
        return dict(grid=v[0].value, block=v[1].value, waves_per_road=v[2].value)

    def planes_numpy(self):
        """(x, v, w) as NumPy [E,R,C] copies (w is zeros when it is not carried)."""
        ring = self.xv.cpu().numpy()
        x, v = ring[..., 0], ring[..., 1]
        w = self._ringw.cpu().numpy() if self.P == 3 else np.zeros_like(x)   # (exported with xv)
        return x, v, w

    # ---- bulk state import (tests, checkpoint restore) ----------------------------------------
    def load_state(self, x, v, leading, lastcar, w=None, arch=None):
        """x, v[, w][, arch]: [E,R,C]; leading/lastcar: [E,R].  Rebuilds the kernel's tail cache."""
        self._staging()
        self._stage_epoch = self._epoch
        if self._ringa is not None and arch is not None:
            self._ringa.copy_(torch.as_tensor(np.asarray(arch, np.uint8)).to(self.device))
        self._ring[..., 0].copy_(torch.as_tensor(np.asarray(x, np.float32)).to(self.device))
        self._ring[..., 1].copy_(torch.as_tensor(np.asarray(v, np.float32)).to(self.device))
        if self._ringw is not None and w is not None:
            self._ringw.copy_(torch.as_tensor(np.asarray(w, np.float32)).to(self.device))
        self.leading.copy_(torch.as_tensor(np.asarray(leading, np.int32)).to(self.device))
        self.lastcar.copy_(torch.as_tensor(np.asarray(lastcar, np.int32)).to(self.device))
        self.refresh()
