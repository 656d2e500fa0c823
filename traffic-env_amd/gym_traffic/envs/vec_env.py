"""TrafficVecEnv: E independent traffic envs stepped together on one MI355X, tensors in/out.

This is the batched form of the reference's TrafficEnv (traffic_env.py:221-394) for RL rollouts:
the same tick semantics per env, every env's arrays stacked along a leading dimension, no host
round trip inside `step`.  Spawns come either from per-env replicas of the reference's seeded
generators (`spawn='poisson'|'regular'`: host RandomState schedules, bit-identical per env to a
reference env seeded `seed + env_id`), from the on-device form of the reference's Poisson generator
(`spawn='device'`: Philox streams keyed by (seed, global env id), no host work per tick - the one to
use for throughput), from the on-device form of its `regular` generator (`spawn='regular_device'`: the reference's car
counts per tick, entry roads from the same Philox streams), from the on-device fixed-rate rule (`spawn='periodic'`) or
from demand profiles on the device (`spawn='demand'`, rule 4 of include/tfx.h: a true per-tick Poisson process - not the
reference's rounded-gap generator - whose mean changes over time, weighs the entry roads and differs from env to env:
`demand=dict(means=[K][S], weights=[K][S][n_entry] or None, seg_ticks=, tick_offset=0)`, the profile of every env in the
device tensor `demand_profile`, int32 [E], zeros at first and the user's to rewrite between calls; with `archetypes` the
dict also takes `row_weights=[K][S][n]`, the share of every table row among the cars of profile k in segment s).
Sharding across GPUs is by env id (gym_traffic/distributed.py); envs share nothing.

Mixed cars: `archetypes` takes the reference's `archetypes` table (traffic_env.py:35-43) as rows (v, l, a, delta, v0, b,
T, s0) - the order of TfxEngine - and every car the envs make is a row of it, kept through every handoff (planes = 3,
the transposed layout).  `poisson` replays the reference's `archetypes[random.randint(n)]` per car on each env's
RandomState (env k equals a single-env TrafficEnv with the same table seeded `seed + k`); `device` draws the rows on the
device by rule 1 of include/tfx.h (gym_traffic/devrng.py mirrors it); `demand` draws them on the device by rule 5, by
the demand's `row_weights` (devrng.demand_rows mirrors it); `regular`, `regular_device` and `periodic` make
every car row 0, as the reference's `regular` generator does (traffic_env.py:174).

Episodes: with `autoreset=True` the envs keep their episodes on the device (tfx_set_episodes, include/tfx.h).  Every
`agent_step` first restarts the envs whose previous decision ended their episode - by overflow (`adone`) or by the time
limit `episode_len` in decisions (`truncated`; the reference's algorithms run FLAGS.episode_len decisions per episode,
algorithms/greedy.py:13) - with phases drawn on the device, and accounts for the decision at its end: `episode_return`,
`episode_length` (running), `final_return`, `final_length` (of the episode that just ended; valid where
`adone | truncated`).  The observation returned for an env that ended is its terminal one; its new episode starts with
the next decision.  No host work per decision; `reset_done()` is not to be called in this mode.

Warm restarts: every env of the reference's training setup is `Repeater -> WarmupWrapper(FLAGS.warmup_lights) -> Remi`
(traffic_test.py:84-86) - reset() runs warmup_lights decisions under sampled actions before the agent sees anything, so
no episode starts on an empty map.  `make_warm_pool` pays that warm-up once, for a small second TrafficVecEnv, and
`set_warm_pool` attaches it: from then on a restart on the device is a clone of one of the pool's envs (which one: rule 3
of include/tfx.h, devrng.episode_pool_slots) instead of an empty map, still inside the decision's one submission;
`reset(warm=True)` starts episode 0 the same way.

Travel times: in validate mode `travel_times()` keeps mean travel time on the device - the finished trips of every env's
log reduced from a cursor on (tfx_trip_stats) and the ages of the cars still on the map (tfx_car_ages), running across
resets and restarts, with no host round trip; `trip_times()` remains the host copy of the log.
"""
import collections

import numpy as np
import torch

from gym_traffic import devrng
from gym_traffic.core import ARCHETYPE, TfxEngine, TripStats
from gym_traffic.envs.roadgraph import GridRoad
from gym_traffic.spawner import ArrivalStreams


# what TrafficVecEnv.measures() returns: the engine's four per-road tensors and the views derived from them
VecMeasures = collections.namedtuple("VecMeasures", "n_cars n_halted queue speed_sum halted cars mean_speed pressure")
# what TrafficVecEnv.following() returns: the engine's eleven per-road tensors and the views derived from them
VecFollowing = collections.namedtuple("VecFollowing", "n_cars n_pairs n_joined n_overlap gap_sum gap_min n_hw hw_sum n_conflict "
                                                      "ttc_min drac_max pairs mean_gap min_gap platoons mean_platoon_size "
                                                      "mean_headway_s min_ttc_s conflicts max_drac overlaps")
# what TrafficVecEnv.stop_lines() returns: the engine's six road-end tensors and the views derived from them
VecEnds = collections.namedtuple("VecEnds", "n_cars n_heads heads head_rows tail tail_row approach eta_s entry_room "
                                            "downstream_room cross_gap")
# what TrafficVecEnv.cars() returns: the engine's car list and the per-car views derived from it
VecCars = collections.namedtuple("VecCars", "n offsets xv road row spawn sel road_id rank dist age_ticks valid")
# what TrafficVecEnv.cell_obs() returns: the engine's two per-cell tensors and the image a convolutional policy reads
VecCells = collections.namedtuple("VecCells", "n_cars speed_sum image")
# what TrafficVecEnv.travel_times() returns: per-env travel-time figures, finished trips and cars still on the map
VecTravel = collections.namedtuple("VecTravel", "finished finished_s mean_trip_s max_trip_s hist lost unfinished "
                                                "unfinished_s oldest_s mean_incl_unfinished_s")


class TrafficVecEnv(object):
    def __init__(self, num_envs, m, n, length, capacity=20, rate=0.5, local_cars_per_sec=0.12,
                 spawn='poisson', spawn_period=8, entry_spec=0, learn_switch=False, validate=False,
                 seed=0, env_id_offset=0, device=None, archetypes=None, autoreset=False, episode_len=None, demand=None,
                 constants=None, trip_cap=4096):
        """constants: entries of gym_traffic.core.CONSTANTS to override (the reference's module constants: yellow_ticks,
        thresh, detect_dist, overflow_penalty, eps), handed to the engine.
        archetypes: None (the reference's single archetype) or float [n, 8] rows (v, l, a, delta, v0, b, T, s0) of
        the archetype table, n <= 64 - every spawn mode then makes mixed cars as the module docstring says.
        autoreset / episode_len: episodes on the device, see the module docstring (episode_len needs autoreset; in
        validate mode the trip log of an ended episode stays readable until the next decision begins).
        demand: with spawn='demand', the keyword arguments of TfxEngine.set_demand other than the seed - means, weights,
        seg_ticks, tick_offset, n_cdf and, with `archetypes`, row_weights (None: every row equally likely).
        trip_cap: validate mode, the trips every env's log holds between two restarts (later ones are counted, not
        kept: travel_times().lost)."""
        if episode_len is not None and not autoreset:
            raise ValueError("episode_len needs autoreset=True (the time limit is kept on the device)")
        self.num_envs = int(num_envs)
        # how this env was made (snapshot() makes another one like it)
        self._ctor = dict(m=m, n=n, length=length, capacity=capacity, rate=rate, local_cars_per_sec=local_cars_per_sec,
                          spawn=spawn, spawn_period=spawn_period, entry_spec=entry_spec, learn_switch=learn_switch,
                          validate=validate, seed=seed, env_id_offset=env_id_offset, device=device,
                          archetypes=archetypes, autoreset=autoreset, episode_len=episode_len, demand=demand,
                          constants=constants, trip_cap=trip_cap)
        self.graph = GridRoad(m, n, length)
        self.graph.generate_entrypoints(entry_spec)
        tab = None if archetypes is None else np.asarray(archetypes, np.float32).reshape(-1, 8)
        self.engine = TfxEngine(m, n, length, capacity, n_envs=num_envs, rate=rate,
                                learn_switch=learn_switch, validate=validate,
                                entry_spec=entry_spec, device=device, env_id_offset=env_id_offset,
                                archetypes=tab, constants=constants, trip_cap=trip_cap,
                                **({} if tab is None else dict(planes=3, layout="transposed")))
        self.archetypes = tab
        self.constants = self.engine.constants
        self.rate = float(rate)
        open_sides = 4 - bin(int(entry_spec) & 15).count('1')
        self.cars_per_sec = local_cars_per_sec * m * open_sides
        self.spawn = spawn
        self.env_id_offset = int(env_id_offset)
        eng = self.engine
        if spawn in ('poisson', 'regular'):
            # env k of this shard is global env (env_id_offset + k): its stream does not depend on
            # how the envs are sharded over GPUs
            # (replayed in C for all envs at once: reference-identical arrivals at any batch size)
            # (heterogeneous cars: the rows of every tick's cars too, S = capacity - 2 per road; bound next to the
            # counts through a device buffer kept per tick count)
            self._arrivals = ArrivalStreams([seed + self.env_id_offset + k for k in range(self.num_envs)],
                                            spawn == 'poisson', self.graph.entrypoints, eng.entry_index,
                                            max(1, eng.n_entry), self.cars_per_sec * self.rate,
                                            **(dict(n_archetypes=len(tab), per_road=eng.C - 2) if eng.het else {}))
            self._rows_dev = {}
        elif spawn == 'device':
            eng.set_poisson(self.cars_per_sec * self.rate, seed=seed)
        elif spawn == 'regular_device':
            eng.set_regular(self.cars_per_sec * self.rate, seed=seed)
        elif spawn == 'demand':
            if not isinstance(demand, dict) or "means" not in demand:
                raise ValueError("spawn='demand' needs demand=dict(means=..., weights=..., seg_ticks=..., tick_offset=0)")
            unknown = set(demand) - {"means", "weights", "seg_ticks", "tick_offset", "n_cdf", "row_weights"}
            if unknown:
                raise ValueError("demand: unknown keys %s" % sorted(unknown))
            eng.set_demand(seed=seed, **demand)
            self.demand_profile = eng.demand_profile
        elif spawn == 'periodic':
            eng.set_spawns(period=spawn_period)
        elif spawn in (None, 'none'):
            eng.set_spawns()
        else:
            raise ValueError("spawn must be poisson|regular|device|regular_device|demand|periodic|none")
        if demand is not None and spawn != 'demand':
            raise ValueError("demand= needs spawn='demand'")
        self._phase_rng = np.random.RandomState(seed + 7919 + self.env_id_offset)
        self.obs, self.rewards, self.done = eng.obs, eng.rewards, eng.done
        self.autoreset = bool(autoreset)
        self.episode_len = None if episode_len is None else int(episode_len)
        if self.autoreset:
            eng.set_episodes(max_decisions=self.episode_len, seed=seed)
            self.truncated = eng.truncated
            self.episode_return, self.episode_length = eng.ep_return, eng.ep_len
            self.final_return, self.final_length = eng.final_return, eng.final_len
            self.episode_index = eng.ep_index
        self._travel = None     # travel_times(): the cursor and the running tensors, made on first use
        # validate mode with autoreset: ep_index as it stood when the last decision began (a reset, a clone: as it stands
        # with nothing pending).  Where ep_index has moved since, the episode ended in that decision and the NEXT decision
        # begins by restarting the env - which clears its trip log (_begin_decision)
        self._ep_before = eng.ep_index.clone() if (self.autoreset and eng.n_trips is not None) else None

    @property
    def observation_shape(self):
        return (self.num_envs, self.engine.obs_len)

    def reset(self, phase_init=None, warm=False):
        """warm: with a pool attached (set_warm_pool), after the plain reset every env becomes a clone of the pool env
        devrng.episode_pool_slots(seed, global env ids, episode_index, pool size) names - rule 3 with the episode numbers
        the reset left (0 after construction) - so the first episode starts as warm as the later ones; the envs keep
        their own arrival streams and accounting."""
        eng = self.engine
        if phase_init is None:
            phase_init = self._phase_rng.randint(2, size=(eng.E, eng.I)).astype(np.int32)
        eng.reset(phase_init)
        self._travel_forget()
        if self._ep_before is not None:
            self._ep_before.copy_(eng.ep_index)     # (the reset clears the restart marks; ep_index does not move)
        if warm:
            pool = self.warm_pool
            if pool is None:
                raise RuntimeError("reset(warm=True) needs a pool of warmed-up envs: set_warm_pool(make_warm_pool(...))")
            ids = np.arange(self.num_envs) + self.env_id_offset
            slots = devrng.episode_pool_slots(self._ctor["seed"], ids, self.episode_index.cpu().numpy(), pool.num_envs)
            self.clone_envs(slots, source=pool, streams=False, episodes=False)
        return eng.obs

    # ---- warm restarts (tfx_set_episode_pool, include/tfx.h) ---------------------------------------------------------
    warm_pool = None
    # global env ids from here on are the pools' (make_warm_pool's default): their arrival streams stay apart from the
    # live envs' however those are sharded, and every shard that builds its pool with the default builds the same one
    POOL_ENV_ID_OFFSET = 1 << 30

    def set_warm_pool(self, pool):
        """Attach `pool` (a TrafficVecEnv of the same world, e.g. from make_warm_pool; None detaches): the envs that end
        restart on the device as clones of its envs instead of empty.  The pool is read at the time of each restart and
        never written - step it between decisions to keep it fresh.  Kept alive by this env while attached."""
        if not self.autoreset:
            raise RuntimeError("set_warm_pool() needs autoreset=True (the restarts it warms are those on the device)")
        self.engine.set_episode_pool(None if pool is None else pool.engine)
        self.warm_pool = pool

    def make_warm_pool(self, n_pool, decisions, n_ticks=10, cycle_period=None, seed=None, env_id_offset=None):
        """A TrafficVecEnv of n_pool envs of this env's construction (autoreset off), reset and run through `decisions`
        agent decisions of n_ticks ticks - WarmupWrapper's reset (wrappers/warmup.py:8-13): actions sampled per light from
        a torch generator on the device seeded `seed` (default: this env's seed), or the fixed cycle with cycle_period.
        env_id_offset (default POOL_ENV_ID_OFFSET = 2**30) keeps the pool's arrival streams apart from the live envs'.
        Raises RuntimeError("Episode completed during warmup") if an env overflowed, as the reference asserts.  In
        validate mode the pool's n_trips are zeroed: warm-up trips do not enter the live envs' logs.  Returns the pool;
        attach it with set_warm_pool."""
        ctor = dict(self._ctor, autoreset=False, episode_len=None,
                    env_id_offset=self.POOL_ENV_ID_OFFSET if env_id_offset is None else int(env_id_offset))
        pool = TrafficVecEnv(int(n_pool), **ctor)
        pool.reset()
        eng = pool.engine
        gen = torch.Generator(device=eng.device)
        gen.manual_seed(int(self._ctor["seed"] if seed is None else seed))
        over = torch.zeros_like(eng.done)
        for _ in range(int(decisions)):
            if cycle_period is not None:
                out = pool.agent_step(n_ticks=n_ticks, cycle_period=cycle_period)
            else:
                act = torch.randint(0, 2, (eng.E, eng.I), generator=gen, device=eng.device, dtype=torch.int32)
                out = pool.agent_step(act, n_ticks=n_ticks)
            over |= out[2]
        if bool(over.any()):
            raise RuntimeError("Episode completed during warmup")
        if eng.n_trips is not None:
            eng.n_trips.zero_()
        return pool

    def reset_done(self, done=None, phase_init=None):
        """Start a new episode in the envs that are done (default: the `done` flags of the last step
        or decision), leaving the others running; returns the mask that was reset."""
        eng = self.engine
        if self.autoreset:
            raise RuntimeError("reset_done() with autoreset=True would reset the envs twice: the next agent_step "
                               "restarts the envs that ended (adone | truncated) on the device")
        mask = eng.done.clone() if done is None else done      # (reset_envs clears eng.done of those envs)
        if phase_init is None:
            phase_init = self._phase_rng.randint(2, size=(eng.E, eng.I)).astype(np.int32)
        eng.reset_envs(mask, phase_init)
        self._travel_forget(mask)
        return mask

    def step(self, actions=None, n_ticks=1, cycle_period=None):
        """actions: int tensor [E, I] on the device (held for n_ticks, like the Repeater wrapper,
        traffic_test.py:48-49) or None with cycle_period for the on-device fixed-cycle controller.
        Returns live device tensors (obs int32 [E,2r+2I], rewards f32 [E,I], done u8 [E])."""
        eng = self.engine
        if cycle_period is not None:
            eng.set_actions(cycle_period=cycle_period)
        elif actions is not None:
            eng.set_actions(actions)
        if self.spawn in ('poisson', 'regular'):
            self._bind_arrivals(int(n_ticks))
        eng.step(int(n_ticks))
        return eng.obs, eng.rewards, eng.done

    def agent_step(self, actions=None, n_ticks=10, remi=True, cycle_period=None):
        """One agent decision for every env as ONE device submission: the Repeater (+ Remi) wrappers
        of the reference (traffic_test.py:27-64) fused in tfx_agent_step.  Returns device tensors
        (aobs f32 [E,2r+I], areward f32 [E,I], adone u8 [E]) owned by the engine.  An env that
        overflows stands still for the rest of the decision (`if done: break`); with host-side
        arrival schedules the arrivals drawn for its remaining ticks are dropped."""
        eng, n = self.engine, int(n_ticks)
        if cycle_period is not None:
            eng.set_actions(cycle_period=cycle_period)
        elif actions is not None:
            eng.set_actions(actions)
        if self.spawn in ('poisson', 'regular'):
            self._bind_arrivals(n)
        if self._ep_before is not None:
            self._begin_decision()
        return eng.agent_step(n, remi=remi)

    def _begin_decision(self):
        """Validate mode with autoreset, on the device: the envs whose episode ended in the previous decision restart as
        this one begins, which clears their trip logs - travel_times() reads those from the start again."""
        ep = self.engine.ep_index
        if self._travel is not None:
            self._travel["cursor"].masked_fill_(ep != self._ep_before, 0)
        self._ep_before.copy_(ep)

    def _restart_pending(self):
        """int32 [E] on the device: 1 where the env's last decision ended its episode and no decision has begun since"""
        if self._ep_before is None:
            return torch.zeros((self.num_envs,), dtype=torch.int32, device=self.engine.device)
        return (self.engine.ep_index != self._ep_before).to(torch.int32)

    def _bind_arrivals(self, n):
        """The host streams' next n ticks as the engine's per-tick spawn counts (and, heterogeneous cars, rows)."""
        eng = self.engine
        if not eng.het:
            counts, _ = self._arrivals.next_ticks(n)
            eng.set_spawns(counts=counts, per_tick=True)
            return
        counts, _, rows = self._arrivals.next_ticks(n)
        dev = self._rows_dev.get(n)
        if dev is None:
            dev = self._rows_dev[n] = torch.empty(rows.shape, dtype=torch.uint8, device=eng.device)
        dev.copy_(torch.from_numpy(rows))
        eng.set_spawns(counts=counts, per_tick=True, rows=dev)

    def remi_reward(self):
        return self.engine.remi_reward()

    # ---- branch, snapshot, restore (tfx_clone_envs, include/tfx.h) -------------------------------------------------
    def clone_envs(self, src_of_env, source=None, streams=True, episodes=True):
        """Env e becomes a copy of env src_of_env[e] of `source` (another TrafficVecEnv of the same world; default: this
        one); -1 leaves env e alone.  One device launch, no host synchronisation (TfxEngine.clone_envs).  streams: the
        clone also continues its source's arrival stream - on the device for spawn='device' | 'regular_device' | 'demand'
        (a demand env also takes its source's demand_profile entry, gathered on the device from the index tensor), and for
        the host-replayed modes ('poisson' | 'regular') by copying the source envs' generator states, so env e replays
        what its source would have replayed; both envs must use the same spawn mode.  episodes: with autoreset on in
        both, the running episode's return / length / index travel too.  In place a source must not itself be
        overwritten (devrng.clone_plan); such envs are left alone and counted in engine.clone_skipped()."""
        other = self if source is None else source
        eng = self.engine
        on_device = self.spawn in ('device', 'regular_device', 'demand')
        if streams and self.spawn != other.spawn:
            raise ValueError("clone_envs(streams=True) needs the same spawn mode in both envs (%r / %r)"
                             % (self.spawn, other.spawn))
        with_episodes = bool(episodes and self.autoreset and other.autoreset)
        idx = eng.clone_envs(src_of_env, source=other.engine, streams=bool(streams and on_device), episodes=with_episodes)
        demand = streams and self.spawn == 'demand'
        if demand or self._travel is not None or (with_episodes and self._ep_before is not None):
            # the envs the clone applied to (devrng.clone_plan's rule, on the device)
            s = idx.long()
            ok = (s >= 0) & (s < other.num_envs)
            sc = s.clamp(0, other.num_envs - 1)
            if other is self:
                t = s[sc]
                ok &= (t == -1) | (t == s)
            if demand:      # ... take their sources' profiles
                self.demand_profile.copy_(torch.where(ok, other.demand_profile[sc], self.demand_profile))
            if self._travel is not None:
                # ... and their sources' trip logs: travel_times() goes on from the end of what was cloned, so the
                # source's finished trips do not enter the clone's running figures
                cur = self._travel["cursor"]
                cur.copy_(torch.where(ok, eng.n_trips, cur))
            if with_episodes and self._ep_before is not None:
                # ... and, with the episode accounting, their sources' restart marks
                self._ep_before.copy_(torch.where(ok, eng.ep_index - other._restart_pending()[sc], self._ep_before))
        if streams and self.spawn in ('poisson', 'regular'):
            from gym_traffic.devrng import clone_plan
            host = idx.cpu().numpy()
            applied, _ = clone_plan(host, None if other is self else other.num_envs)
            self._arrivals.copy_streams(np.where(applied, host, -1), other._arrivals)
        return idx

    def snapshot(self):
        """A new TrafficVecEnv of the same construction holding a clone of every env (streams and episodes included)."""
        snap = TrafficVecEnv(self.num_envs, **self._ctor)
        snap.reset(np.zeros((self.num_envs, self.engine.I), np.int32))
        snap.clone_envs(torch.arange(self.num_envs, dtype=torch.int32), source=self)
        return snap

    def restore(self, snap):
        """Every env back to the state `snap` (from snapshot()) holds.  travel_times() reads the restored logs from the
        start: its running figures go on, and the trips the snapshot's logs hold are added to them (clear the running
        figures before restoring if they counted those trips once already)."""
        idx = self.clone_envs(torch.arange(self.num_envs, dtype=torch.int32), source=snap)
        self._travel_forget()
        return idx

    # ---- validate-mode metrics, batched (reference: traffic_test.py:41-46, traffic_env.py:139-157, util.py:91-92) ----
    def light_times(self, actions):
        """float32 [E, I]: for every light the action flips, the seconds it had been in its phase -
        (elapsed + 1) * xor(current_phase, action) / 2, what the Repeater reports per decision as
        info['light_times'] in validate mode (traffic_test.py:41-46); 0 where the action flips nothing.  Call it
        BEFORE the decision's step, like the reference does.  The single-env list is `t[k][t[k] != 0]`."""
        eng = self.engine
        a = actions if isinstance(actions, torch.Tensor) else torch.as_tensor(np.asarray(actions))
        a = a.to(eng.device)
        flips = (eng.current_phase != 0) != (a != 0)
        return ((eng.elapsed + 1) * flips).to(torch.float32) / 2

    def unfinished(self):
        """int64 [E]: cars still on the train roads, `np.sum(env.cars_on_roads())` per env (util.py:92)."""
        eng = self.engine
        return eng.cars_on_roads_flat()[:, :eng.r].sum(dim=1)

    def trip_times(self, env=None):
        """Trip times (seconds) of the cars that left the map since the last reset, in the order advance_hack logs
        them (traffic_env.py:153-154): a list of float32 arrays, one per env - or env `env`'s array.  Needs
        validate=True."""
        eng = self.engine
        if eng.n_trips is None:
            raise RuntimeError("trip times are recorded in validate mode only (TrafficVecEnv(..., validate=True))")
        n = eng.n_trips.cpu().numpy()
        tt = eng.trip_times.cpu().numpy()
        if env is not None:
            return tt[env, :min(int(n[env]), eng.trip_cap)].copy()
        return [tt[k, :min(int(n[k]), eng.trip_cap)].copy() for k in range(eng.E)]

    def _travel_forget(self, mask=None):
        """The trip logs of the envs in `mask` (None: all) start again: travel_times() reads them from the start."""
        if self._travel is None:
            return
        cur = self._travel["cursor"]
        if mask is None:
            cur.zero_()
        else:
            m = mask if isinstance(mask, torch.Tensor) else torch.as_tensor(np.asarray(mask))
            cur.masked_fill_(m.to(cur.device).bool(), 0)

    def travel_times(self, edges_s=None, clear=False):
        """Travel times of every env, on the device, with no host synchronisation: one launch over the trip logs
        (TfxEngine.trip_stats / tfx_trip_stats) and one over the live cars' spawn ticks (TfxEngine.car_ages /
        tfx_car_ages, include/tfx.h) plus a few torch expressions.  Needs validate=True.  The env keeps a cursor into every
        env's log and RUNNING tensors: each call adds the trips logged since the previous one, across resets and
        restarts, so a rollout reads "mean travel time so far" at any decision.  -> VecTravel, all [E]:
            finished      int64    trips read from the logs so far
            finished_s    float64  the sum of their trip seconds (ticks / 2, as the reference logs them)
            mean_trip_s   float64  finished_s / finished, 0 where no trip finished
            max_trip_s    float64  the longest of them
            hist          int64 [E, n_bins]: trips per bin of edges_s (seconds, n_bins + 1 non-decreasing values, rounded
                          to ticks; at most 32 bins), None without edges_s; changing the edges restarts the histogram
            lost          int64    trips that happened but fell off the end of a log (trip_cap): counted in no other figure
            unfinished    int64    cars on the map NOW, on all R roads - exit roads too: a car logs its trip only when it
                          leaves the map
            unfinished_s  float64  the seconds those cars have spent on the map so far
            oldest_s      float64  the longest of those
            mean_incl_unfinished_s  float64  (finished_s + unfinished_s) / (finished + unfinished), 0 where that is 0 / 0 -
                          the figure that does not flatter a policy whose cars never arrive
        clear=True zeroes the running tensors after the read (per-episode or per-window figures).
        reset(), reset_done(mask) and restore() zero the cursor of the envs they reset; clone_envs() sets the cursor of a
        cloned env to the end of the log it received.  With autoreset=True call travel_times() ONCE PER DECISION, after
        it: an ended episode's log stays readable only until the next decision begins; agent_step() zeroes the cursor
        of every env whose episode ended in the previous decision as it begins the next one, because the restart clears
        that log (a snapshot carries which envs are about to restart, so this holds across snapshot() / restore() too).
        Calls between two decisions add nothing twice.  A warm pool's n_trips must be zero for the log of a restart to
        start empty: make_warm_pool leaves it so, a pool that is stepped afterwards must be re-zeroed by the caller."""
        eng = self.engine
        if eng.n_trips is None:
            raise RuntimeError("travel times are recorded in validate mode only (TrafficVecEnv(..., validate=True))")
        E, dev = eng.E, eng.device
        ed = None if edges_s is None else tuple(int(round(2.0 * float(t))) for t in np.asarray(edges_s).reshape(-1))
        tv = self._travel
        if tv is None:
            tv = self._travel = dict(cursor=torch.zeros((E,), dtype=torch.int32, device=dev),
                                     count=torch.zeros((E,), dtype=torch.int32, device=dev),
                                     tick_sum=torch.zeros((E,), dtype=torch.int64, device=dev),
                                     tick_max=torch.zeros((E,), dtype=torch.int32, device=dev),
                                     lost=torch.zeros((E,), dtype=torch.int32, device=dev), hist=None, edges=None)
        if ed != tv["edges"]:
            tv["edges"] = ed
            tv["hist"] = None if ed is None else torch.zeros((E, len(ed) - 1), dtype=torch.int32, device=dev)
        eng.trip_stats(edges=ed, cursor=tv["cursor"], accumulate=True,
                       out=TripStats(tv["count"], tv["tick_sum"], tv["tick_max"], tv["lost"], tv["hist"]))
        ages = eng.car_ages()
        finished = tv["count"].long()
        finished_s = tv["tick_sum"].double() / 2
        zero = torch.zeros_like(finished_s)
        unfinished = ages.n_cars.sum(dim=1, dtype=torch.int64)
        unfinished_s = ages.age_sum.sum(dim=1).double() / 2
        both = finished + unfinished
        out = VecTravel(finished, finished_s, torch.where(finished > 0, finished_s / finished.clamp(min=1), zero),
                        tv["tick_max"].double() / 2, None if tv["hist"] is None else tv["hist"].long(), tv["lost"].long(),
                        unfinished, unfinished_s, ages.age_max.max(dim=1).values.double() / 2,
                        torch.where(both > 0, (finished_s + unfinished_s) / both.clamp(min=1), zero))
        if clear:
            for k in ("count", "tick_sum", "tick_max", "lost", "hist"):
                if tv[k] is not None:
                    tv[k].zero_()
        return out

    def measures(self, halt_speed=0.1, x_from=None, accumulate=False):
        """The standard traffic measures of signal control for every env, on the device, with no host synchronisation:
        one read-only launch over the live cars (TfxEngine.road_measures / tfx_road_measures, include/tfx.h) plus a few
        torch expressions over its four words per road.  -> VecMeasures:
            n_cars, n_halted, queue  int32 [E, R], speed_sum float32 [E, R] - per road id: cars with x >= x_from (None:
                        all), those of them with v < halt_speed, the halted platoon at the head of the road, the sum of
                        the speeds; the engine's tensors, overwritten by the next call - or, accumulate=True, added to
                        (halted vehicle-decisions as a delay figure: measure once per decision)
            halted, cars int64 [E] - sums of n_halted / n_cars over the train roads
            mean_speed  float64 [E] - sum of speed_sum over the train roads / cars, 0 where there are no cars
            pressure    int64 [E, I, 2] - max-pressure's quantity: for phase p the sum over the approach roads e of the
                        intersection with graph.phases[e] == p of n_cars[e] - n_cars[graph.nexts[e]]
        With accumulate=True the derived views are those of the accumulated tensors."""
        eng = self.engine
        rm = eng.road_measures(halt_speed=halt_speed, x_from=x_from, accumulate=accumulate)
        r = eng.r
        if getattr(self, "_pressure_idx", None) is None:
            g = self.graph
            self._pressure_idx = (torch.as_tensor(g.nexts[:r].astype(np.int64)).to(eng.device),
                                  torch.as_tensor(g.dest[:r].astype(np.int64) * 2 + g.phases[:r]).to(eng.device))
        nxt, cell = self._pressure_idx
        n = rm.n_cars.long()
        cars = n[:, :r].sum(dim=1)
        halted = rm.n_halted[:, :r].sum(dim=1, dtype=torch.int64)
        speed = rm.speed_sum[:, :r].sum(dim=1, dtype=torch.float64)
        mean_speed = torch.where(cars > 0, speed / cars.clamp(min=1), torch.zeros_like(speed))
        pressure = torch.zeros((eng.E, 2 * eng.I), dtype=torch.int64, device=eng.device)
        pressure.index_add_(1, cell, n[:, :r] - n[:, nxt])
        return VecMeasures(rm.n_cars, rm.n_halted, rm.queue, rm.speed_sum, halted, cars, mean_speed,
                           pressure.view(eng.E, eng.I, 2))

    def following(self, platoon_gap=10.0, v_min=0.5, ttc_crit=3.0, x_from=None, accumulate=False):
        """The car-following measures of every env, on the device, with no host synchronisation: one read-only launch
        over the live cars (TfxEngine.road_following / tfx_road_following, include/tfx.h) plus a few torch expressions
        over its eleven words per road.  A car pairs with the car ahead of it on its road; g is the net gap to that
        leader's rear bumper, dv the closing speed.  -> VecFollowing:
            n_cars .. drac_max  the engine's RoadFollowing tensors [E, R] per road id, overwritten by the next call - or,
                        accumulate=True, combined with it (measure once per decision: conflicts per car-decision)
        and over the train roads:
            pairs       int64 [E] - pairs whose follower has x >= x_from (None: all)
            mean_gap    float64 [E] - sum of gap_sum / pairs, in metres; nan without pairs
            min_gap     float32 [E] - the smallest g; +inf without pairs
            platoons    int64 [E, R] - n_cars - n_joined per road (every road): the groups of cars no further than
                        platoon_gap apart; mean_platoon_size float64 [E] - cars / platoons, nan without cars
            mean_headway_s float64 [E] - sum of hw_sum / sum of n_hw: mean of g / v_F over the followers with v_F >= v_min;
                        nan without such pairs
            min_ttc_s   float32 [E] - the smallest g / dv over the closing pairs (dv > 0, g > 0); +inf without
            conflicts   int64 [E] - closing pairs with g / dv < ttc_crit
            max_drac    float32 [E] - the largest dv^2 / 2g over the closing pairs, 0 without
            overlaps    int64 [E] - pairs with g < 0: followers past their leader's rear bumper
        With accumulate=True the derived views are those of the accumulated tensors."""
        eng = self.engine
        rf = eng.road_following(platoon_gap, v_min, ttc_crit, x_from=x_from, accumulate=accumulate)
        r = eng.r
        nan = torch.full((eng.E,), float("nan"), dtype=torch.float64, device=eng.device)

        def total(t):
            return t[:, :r].sum(dim=1, dtype=torch.int64)

        def ratio(num, den):
            return torch.where(den > 0, num / den.clamp(min=1), nan)
        pairs = total(rf.n_pairs)
        platoons = rf.n_cars.long() - rf.n_joined.long()
        return VecFollowing(*rf, pairs,
                            ratio(rf.gap_sum[:, :r].sum(dim=1, dtype=torch.float64), pairs),
                            rf.gap_min[:, :r].min(dim=1).values,
                            platoons, ratio(total(rf.n_cars).double(), platoons[:, :r].sum(dim=1)),
                            ratio(rf.hw_sum[:, :r].sum(dim=1, dtype=torch.float64), total(rf.n_hw)),
                            rf.ttc_min[:, :r].min(dim=1).values, total(rf.n_conflict),
                            rf.drac_max[:, :r].max(dim=1).values, total(rf.n_overlap))

    def stop_lines(self, k=4, v_min=0.5):
        """The cars at every stop line and the room at every road's entrance, on the device, with no host
        synchronisation: one read-only launch that reads the first k cars and the last car of every road
        (TfxEngine.road_ends / tfx_road_ends, include/tfx.h) plus a few torch expressions.  -> VecEnds:
            n_cars, n_heads int32 [E, R]; heads float32 [E, R, k, 2]; head_rows uint8 [E, R, k]; tail float32 [E, R, 2];
                        tail_row uint8 [E, R] - per road id: the engine's tensors for this k, overwritten by the next
                        call with the same k.  heads[..., j, :] is (distance to the stop line, speed) of car j from the
                        head, (+inf, 0) where the road has fewer cars; tail is (x, v) of the last car, (+inf, 0) on an
                        empty road; the rows are archetype rows, 255 where there is no car
            approach    float32 [E, m, n, 4, k, 2] - heads of the train roads in cars_on_roads()' order: [:, row, col, d]
                        is the approach of direction d into intersection (row, col), what a per-intersection policy reads
            eta_s       float32 [E, r, k] - distance / max(speed, v_min): seconds to the stop line at the car's current
                        speed (never faster than a car of speed v_min); +inf where padded
            entry_room  float32 [E, R] - tail x - l, l the last car's length (its archetype row's; the single
                        archetype's otherwise): the free road behind the last car, +inf on an empty road
            downstream_room float32 [E, r] - entry_room of the road a train road's cars drive into (graph.nexts), +inf
                        where there is none
            cross_gap   float32 [E, r] - heads[..., 0, 0] + downstream_room: the net gap from the head car across the
                        stop line to the last car of the next road - the pair following() leaves out; +inf where either
                        side has no car"""
        eng = self.engine
        if not float(v_min) > 0:
            raise ValueError("stop_lines: v_min %r is not above 0" % (v_min,))
        re_ = eng.road_ends(k=k)
        E, r, m, n, K = eng.E, eng.r, eng.m, eng.n, int(k)
        if getattr(self, "_ends_idx", None) is None:
            nxt = self.graph.nexts[:r].astype(np.int64)
            lengths = eng.archetypes[:, 1] if eng.het else np.array([float(eng.cfg.car_l)], np.float32)
            self._ends_idx = (torch.as_tensor(np.maximum(nxt, 0)).to(eng.device), torch.as_tensor(nxt >= 0).to(eng.device),
                              torch.as_tensor(np.asarray(lengths, np.float32)).to(eng.device))
        nxt, has_next, lengths = self._ends_idx
        inf = torch.full((), float("inf"), dtype=torch.float32, device=eng.device)
        heads = re_.heads[:, :r]
        approach = heads.reshape(E, 4, m, n, K, 2).permute(0, 2, 3, 1, 4, 5)
        listed = torch.arange(K, device=eng.device) < re_.n_heads[:, :r, None]
        eta_s = torch.where(listed, heads[..., 0] / heads[..., 1].clamp(min=float(v_min)), inf)
        some = re_.n_cars > 0
        row = re_.tail_row.long() if eng.het else torch.zeros_like(re_.n_cars, dtype=torch.int64)
        length = lengths[torch.where(some, row, torch.zeros_like(row))]
        entry_room = torch.where(some, re_.tail[..., 0] - length, inf)
        downstream_room = torch.where(has_next, entry_room[:, nxt], inf)
        both = some[:, :r] & has_next & some[:, nxt]
        cross_gap = torch.where(both, heads[:, :, 0, 0] + downstream_room, inf)
        return VecEnds(*re_, approach, eta_s, entry_room, downstream_room, cross_gap)

    def cars(self, envs=None, roads=None, max_cars=None):
        """Every car of chosen envs as one flat, ragged (CSR) list on the device: floating-car data for logging, the
        input of a vehicle-level policy, or a look into a few envs of a big batch - one read-only launch that stores the
        live cars compacted (TfxEngine.car_list / tfx_car_list, include/tfx.h) plus a few torch expressions.  envs: a
        list, an array or an int32 device tensor of env numbers (None: every env; repeats are fine; an id outside [0, E)
        has no cars); roads: a uint8 / bool mask [R] by road id, e.g. arterial(...) (None: every road); max_cars: the
        length of the per-car tensors - with an int nothing synchronises with the host, with None the total is read
        back once and the tensors are sized exactly.  -> VecCars:
            n           int32 scalar - the cars of the chosen envs and roads (may exceed max_cars: then the list is cut)
            offsets     int32 [n_sel * R + 1] - cars of (selection s, road) are entries offsets[s * R + road] ..
                        offsets[s * R + road + 1], head first, in ring order
            xv          float32 [L, 2] (x, v); road int32 [L] the key s * R + road id; row uint8 [L] the archetype row;
                        spawn float32 [L] the spawn tick, None unless the env is validate or heterogeneous
            sel, road_id int64 [L] - road // R and road % R; rank int64 [L] - the car's place from the head of its road
            dist        float32 [L] - length - x, the distance to the stop line
            age_ticks   int32 [L] - ticks since the car was spawned (TfxEngine.car_ages' rule), None where spawn is
            valid       bool [L] - arange(L) < n: entries that hold a car; the others are zero"""
        eng = self.engine
        cl = eng.car_list(env_ids=envs, roads=roads, max_cars=max_cars)
        L, R = int(cl.xv.shape[0]), eng.R
        at = torch.arange(L, device=eng.device)
        valid = at < cl.n
        key = cl.road.long()
        sel, road_id = key // R, key % R
        rank = torch.where(valid, at - cl.offsets[:-1][key].long(), torch.zeros_like(at))
        dist = float(eng.cfg.length) - cl.xv[:, 0]
        age = None
        if cl.spawn is not None:
            if eng.het:
                age = (int(eng.tick) - cl.spawn.to(torch.int64)).bitwise_and(0xFFFFFF).to(torch.int32)
            else:
                age = (torch.full((), float(int(eng.tick)), dtype=torch.float32, device=eng.device) - cl.spawn).to(torch.int32)
            age = torch.where(valid, age, torch.zeros_like(age))
        return VecCars(*cl, sel, road_id, rank, dist, age, valid)

    def set_cars(self, cars, envs=None, roads=None, leading=None, spawn_shift=0):
        """Write a car list back: what cars() returned, or an edited copy of it (any object with offsets, xv, row and
        spawn - a VecCars, a CarList, a namedtuple's _replace(...)), becomes the cars of the chosen envs in one launch
        with no host synchronisation (TfxEngine.put_cars / tfx_put_cars, include/tfx.h).  Road `road` of env envs[s] (None:
        env s) then holds entries offsets[s * R + road] .. offsets[s * R + road + 1] of the planes, head first: stall a car
        by zeroing its v, delete or insert cars by rebuilding offsets and planes in torch.  roads: a uint8 / bool mask [R] -
        roads outside it keep their cars (pass the mask cars() was given); leading int32 [n_sel, R]: the roads' new ring
        position (None: each road keeps its own, the head car takes the slot behind it); spawn_shift: added to every
        spawn tick (a list taken at another clock).  envs must be distinct: a host-side list with repeats raises.  A road
        holds at most capacity - 2 cars: the excess is dropped and counted in engine.put_lost().  Counters, lights,
        rewards and the trip log are not touched - see pack_envs / unpack_envs for whole envs."""
        self.engine.put_cars(cars.offsets, cars.xv, row=cars.row, spawn=cars.spawn, env_ids=envs, roads=roads,
                             leading=leading, spawn_shift=spawn_shift, count_lost=True)

    def pack_envs(self, envs):
        """Everything a caller can see of the chosen envs as a plain dict of device tensors - for a scenario library, for
        torch.save, for a send to another rank (TfxEngine.pack_envs): the car list (offsets, xv, row, spawn) with the
        roads' `leading`, the bound per-env rows gathered by index in torch (obs, rewards, waiting, passed_dst, done_tick,
        done), on validate envs the trip-log rows and n_trips, and the clock (`tick`), grid and capacity it was taken at.
        One read-only launch plus torch indexing; the total number of cars is read back once.  envs: a list, an array or a
        device tensor of env numbers.  What the handle alone owns - the position of an arrival stream, the greedy
        controller's held action, the episode accounting - is NOT in the dict: tfx.h lets those travel through clone_envs
        only."""
        return self.engine.pack_envs(envs)

    def unpack_envs(self, envs, packed):
        """Write what pack_envs returned into envs of this batch or of another one on the same grid - E and capacity may
        differ: envs[s] receives selection s of the dict (TfxEngine.unpack_envs).  One launch for the cars plus torch index
        writes for the per-env rows; no host synchronisation.  A road whose cars do not fit this batch's capacity keeps the
        first capacity - 2 and the excess shows in engine.put_lost(); `leading` is kept where it is a ring index here.
        Spawn ticks and the done_tick stamp are rebased by the difference of the two clocks, as clone_envs does across
        handles, so ages and trip times go on correctly; travel_times() goes on from the end of the log an env received.
        envs must be distinct.  The arrival stream's position, the greedy controller's held action and the episode
        accounting do NOT travel this way (tfx.h: clone_envs alone carries them): a written env goes on with its own."""
        eng = self.engine
        idx = eng.unpack_envs(envs, packed)
        if self._travel is not None and eng.n_trips is not None:
            self._travel["cursor"][idx] = eng.n_trips[idx]

    # ---- state digests (tfx_state_digest, include/tfx.h) -----------------------------------------------------------
    def digest_parts(self, parts='state'):
        """The TFX_DIGEST_* bits of a named set (an int passes through):
            'cars'   CARS | ROWS - the cars alone: counts, (x, v) bits and archetype rows, wherever the ring stands
            'state'  CARS | ROWS | RING | LIGHTS | OBS - everything the next tick depends on that a caller can see, except
                     the clock-relative spawn ticks.  The next tick reads `detected` (through the observation), and the
                     library hands out the counters as ONE part, so 'state' takes OBS whole: passed, waiting, passed_dst,
                     rewards and done_tick ride along.  Two envs that differ only in those accumulated counters are
                     different under 'state'; done_tick is a clock stamp where an env has overflowed (0 otherwise)
            'all'    'state' plus SPAWN, where the envs keep spawn ticks (validate or heterogeneous): equal only at the
                     same clock, spawn ticks are absolute
        ROWS is dropped where there is no archetype table (every row is 0 there)."""
        from gym_traffic import _native as nat
        if not isinstance(parts, str):
            return int(parts)
        eng = self.engine
        rows = nat.DIGEST_ROWS if eng.het else 0
        state = nat.DIGEST_CARS | rows | nat.DIGEST_RING | nat.DIGEST_LIGHTS | nat.DIGEST_OBS
        sets = dict(cars=nat.DIGEST_CARS | rows, state=state, all=state | (nat.DIGEST_SPAWN if eng.P == 3 else 0))
        if parts not in sets:
            raise ValueError("digest: parts must be 'cars', 'state', 'all' or a sum of DIGEST_* bits, not %r" % (parts,))
        return sets[parts]

    def digest(self, envs=None, parts='state', per_road=False):
        """A 64-bit fingerprint of every chosen env's state, on the device, with no host synchronisation: one read-only
        launch over the live cars (TfxEngine.state_digest / tfx_state_digest, include/tfx.h) -> int64 [len(envs)] device
        tensor (the uint64 bits); per_road=True: (env, road int64 [len(envs), R]).  Envs whose chosen parts hold the same
        bits have equal digests - within this batch, across batches, layouts, shards and snapshots: a transposition key
        for tree search, an 8-byte-per-env check of a sharded run.  A fingerprint, not a cryptographic hash.  envs: a
        list, an array or an int32 device tensor of env numbers (None: every env); parts: see digest_parts.  The engine
        keeps one tensor per (len(envs), per_road): the next such call overwrites it - clone() what must last."""
        return self.engine.state_digest(envs, parts=self.digest_parts(parts), per_road=per_road)

    def same_state(self, src_of_env, source=None, parts='state'):
        """bool [E] device tensor: entry e is True iff env e's digest equals that of env src_of_env[e] of `source`
        (another TrafficVecEnv of the same world; default: this one) - the argument shape of clone_envs, so
        `same_state(idx)` after `clone_envs(idx)` checks the clone for every env at once.  -1 (or any index outside the
        source) gives False.  Two launches, no host synchronisation when src_of_env is a device tensor."""
        other = self if source is None else source
        eng = self.engine
        idx = src_of_env if isinstance(src_of_env, torch.Tensor) else torch.as_tensor(np.asarray(src_of_env, np.int32))
        idx = idx.to(device=eng.device, dtype=torch.int32).reshape(-1).contiguous()
        if idx.numel() != eng.E:
            raise ValueError("src_of_env must hold one index per env (%d), got %d" % (eng.E, idx.numel()))
        bits = self.digest_parts(parts)
        if bits != other.digest_parts(parts):
            raise ValueError("same_state: the two envs do not have the same parts for %r" % (parts,))
        mine = torch.empty((eng.E,), dtype=torch.int64, device=eng.device)
        theirs = torch.empty((eng.E,), dtype=torch.int64, device=other.engine.device)
        eng.state_digest(None, parts=bits, out=mine)
        other.engine.state_digest(idx.to(other.engine.device), parts=bits, out=theirs)
        ok = (idx >= 0) & (idx < other.num_envs)
        return ok & (mine == theirs.to(eng.device))

    def arterial(self, row_or_col, direction):
        """uint8 [R] road mask of one arterial: the chain of roads a car of `direction` (0 eastbound, 1 westbound - along
        row `row_or_col`; 2 towards higher rows, 3 towards lower rows - along column `row_or_col`) drives through, from
        its entry road to the exit road, found by following the GridRoad `nexts` table.  For cars(roads=...)."""
        g = self.graph
        m, n, v = g.m, g.n, g.m * g.n
        i, d = int(row_or_col), int(direction)
        if d not in (0, 1, 2, 3) or not 0 <= i < (m if d < 2 else n):
            raise ValueError("arterial: direction %r / index %r is not on the %d x %d grid" % (direction, row_or_col, m, n))
        road = (i * n, v + i * n + n - 1, 2 * v + i, 3 * v + (m - 1) * n + i)[d]
        mask = np.zeros(g.roads, np.uint8)
        while road >= 0:
            mask[road] = 1
            road = int(g.nexts[road])
        return mask

    def cell_obs(self, n_cells=8, edges=None, v_scale=None, accumulate=False):
        """The discrete traffic state encoding of every env, on the device, with no host synchronisation: every approach
        cut into cells along its length, each cell with its car count and its mean speed - one read-only launch over the
        live cars (TfxEngine.road_cells / tfx_road_cells, include/tfx.h) plus a few torch expressions.  -> VecCells:
            n_cars int32, speed_sum float32 [E, R, B] - per road id and cell; the engine's tensors, overwritten by the
                        next call with the same B - or, accumulate=True, added to
            image       float32 [E, 2, 4, B, m, n]; image.view(E, 8 * B, m, n) is the channels-first form.  Plane 0: the
                        count of train road d * m * n + row * n + col - the approach of direction d into intersection
                        (row, col) - at [:, 0, d, b, row, col]; plane 1: that cell's mean speed / v_scale, 0 where the
                        cell is empty
        edges: B + 1 ascending float32 values (default: devrng.cell_edges(length, n_cells) - B equal cells, no car left
        out); v_scale: default the archetype's v0 (with an archetype table: the largest v0 of its rows)."""
        eng = self.engine
        if edges is None:
            edges = devrng.cell_edges(float(eng.cfg.length), n_cells)
        if v_scale is None:
            v_scale = ARCHETYPE["car_v0"] if self.archetypes is None else float(self.archetypes[:, 4].max())
        rc = eng.road_cells(edges, accumulate=accumulate)
        E, B, m, n = eng.E, rc.n_cars.shape[2], eng.m, eng.n
        cnt = rc.n_cars[:, :eng.r].view(E, 4, m, n, B).permute(0, 1, 4, 2, 3)
        tot = rc.speed_sum[:, :eng.r].view(E, 4, m, n, B).permute(0, 1, 4, 2, 3)
        image = torch.empty((E, 2, 4, B, m, n), dtype=torch.float32, device=eng.device)
        image[:, 0] = cnt
        image[:, 1] = torch.where(cnt > 0, tot / cnt.clamp(min=1) / float(v_scale), torch.zeros_like(tot))
        return VecCells(rc.n_cars, rc.speed_sum, image)

    def frames(self, envs=None, px=32):
        """Top-view pictures of chosen envs, on the device, with no host synchronisation (TfxEngine.frames / tfx_frames,
        include/tfx.h) -> uint8 [len(envs), H, W, 4] device tensor, H = (m + 1) * px + 1, W = (n + 1) * px + 1, bytes R, G,
        B, A: [..., :3] is the RGB picture a video logger keeps, [..., :3].permute(0, 3, 1, 2) the channels-first image
        an agent reads - white background, roads in their lights' colours, cars as blue bars.  envs: a list, an array or
        an int32 device tensor of env numbers (None: every env).  The engine keeps one tensor per (len(envs), px): the
        next call with the same two overwrites it - clone() what must last."""
        return self.engine.frames(envs, px=px)

    def render(self, env=0, mode='rgb_array', px=32):
        """One env's picture on the host -> uint8 NumPy [H, W, 3] (synchronises; frames() is the batched, device-side
        form)."""
        if mode != 'rgb_array':
            raise NotImplementedError("TrafficVecEnv.render draws mode='rgb_array' only - there is no window for mode=%r; "
                                      "take frames(envs, px) and show or save the images yourself" % (mode,))
        return self.frames([int(env)], px=px)[0, ..., :3].cpu().numpy()

    def cars_on_roads(self):
        return self.engine.cars_on_roads()
