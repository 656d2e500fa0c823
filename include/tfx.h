/*
 * tfx.h - C ABI of the MI355X-native IDM traffic-env step ("tfx" = traffic step).
 *
 * This is the drop-in boundary for the hot path of samanklesaria/traffic-env.  The reference has
 * no FFI of its own: the boundary it offers is the set of numba-typed kernels in
 * gym_traffic/envs/traffic_env.py (each @jit signature is a C-like contract: typed, in-place,
 * caller-owned arrays) plus the TrafficEnv methods that sequence them.  Every entry point below
 * cites the reference interface it replaces.  All arrays gain a leading E (batched env)
 * dimension; E = 1 reproduces the reference object.
 *
 * Conventions
 *   - plain C, no torch/HIP types in signatures: device pointers are `void*`-compatible raw
 *     pointers, the stream is a `void*` holding a hipStream_t (NULL = default stream);
 *   - every call returns 0 on success, a negative TFX_E* code on failure; the message for the
 *     calling thread is available from tfx_last_error(); nothing throws, nothing calls exit();
 *   - all state arrays are owned by the caller (the Python env keeps them as PyTorch-ROCm
 *     tensors) and are mutated in place, exactly like the reference's NumPy arrays
 *     (traffic_env.py:361-382); the handle owns only static road tables and per-road scratch;
 *   - no global mutable state: handles are independent and may be driven from different host
 *     threads (the reference's kernels are nogil and A3C steps envs from threads, a3c.py:69-72).
 *
 * Device data layout (all little-endian, C-contiguous)
 *   xv         float32 [E][R][C][2]   (x, v) of the car in ring slot s of road e = the reference's
 *                                     state[e, xi, s], state[e, vi, s] (traffic_env.py:34,364),
 *                                     interleaved so a road's live cars are ONE contiguous span
 *                                     and a car is one 8-byte access.  16-byte aligned.
 *   w          float32 [E][R][C]      state[e, wi, s], the spawn tick (validate-mode trip times);
 *                                     present when tfx_config.planes == 3, else NULL.
 *                                     The other 7 per-car parameters are per-archetype constants
 *                                     (traffic_env.py:35-43) and live in tfx_config.
 *   leading    int32   [E][R]         slot of the fake leader  (README.md:14-23 of the reference)
 *   lastcar    int32   [E][R]         slot of the last car; == leading when the road is empty
 *   obs        int32   [E][2r+2I]     passed | detected | current_phase | elapsed (traffic_env.py:370-376)
 *   rewards    float32 [E][I]
 *   waiting    int32   [E][r]
 *   passed_dst uint8   [E][I]
 *   done_tick  int32   [E]            tick index (+1) of the last tick in which the env overflowed
 */
#ifndef TFX_H
#define TFX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TFX_ABI_VERSION 13
#define TFX_KP 2 /* popped cars carried per road per tick on the parallel path; more -> exact serial path */
#define TFX_MAX_ARCH 64 /* rows of the archetype table (traffic_env.py:35-43 ships one); a power of two */
/* The clock's domain: 0 <= tick <= TFX_TICK_MAX, for the handle's clock between calls and for every tick a call runs.
 * tfx_set_tick refuses anything else (TFX_EINVAL); a call that would run a tick past it - tfx_step, tfx_agent_step
 * with clock + n_ticks > TFX_TICK_MAX, tfx_move_cars and tfx_advance_finished_cars at TFX_TICK_MAX - returns TFX_ESTATE
 * with a message naming the clock, before anything is enqueued: the handle, its clock and the bound buffers stay as
 * they are, and tfx_set_tick or tfx_reset make it usable again.  The handle checks a host mirror of the device clock
 * (csrc/tfx_handle.hpp).  The pure previews tfx_demand_counts / tfx_demand_rows take any int32 tick0.
 *
 * Where the bound comes from - every int32 expression in csrc/ that adds to a tick t of the domain:
 *   t + 1            tick stamps, 0 = never (done_tick, the handle's serial-advance and risk stamps, k_res's overflow and
 *                    serial stamps), the greedy controller's (t + 1) % spacing, k_tail's second tick
 *   t + 2, t + u     k_tail (u < 2) and the clock a pair leaves; k_res's tick0 + tt and tick0 + n_ticks: all at most the
 *                    clock the call ends on, which the check keeps at or below TFX_TICK_MAX; k_tail's risk stamp for the
 *                    pair that follows in the same call, (t + 2) + 1: at most that clock, too
 *   t + (env + env_id_offset) % period     TFX_ACTION_CYCLE: at most t + TFX_PERIOD_MAX - 1 (tfx_set_actions refuses a
 *                    longer cycle), the largest of them all: TFX_TICK_MAX + TFX_PERIOD_MAX - 1 = INT32_MAX - 1
 *   s + (tick(dst) - tick(src))            tfx_clone_envs rebasing a stamp s <= tick(src) + 1: at most tick(dst) + 1
 *   spawn tick + (tick(dst) - tick(src))   rebasing a heterogeneous side word (tfx_clone_envs, tfx_put_cars' spawn_shift): a
 *                    24-bit tick plus up to TFX_TICK_MAX passes INT32_MAX - added as unsigned, kept modulo 2^24
 *   t + tick_offset, first + row           the demand rule: in 64 bits / unsigned, any int32
 * t % period (periodic spawns) and (float)t (spawn ticks) add nothing; a negative t would break the first (C's % is
 * negative then) and the stamps (a stamp of tick -1 is 0, "never"), hence the lower bound. */
#define TFX_PERIOD_MAX (1 << 20)                  /* the longest TFX_ACTION_CYCLE period */
#define TFX_TICK_MAX (0x7fffffff - TFX_PERIOD_MAX) /* 2146435071 */

enum {
  TFX_OK = 0,
  TFX_EINVAL = -1,   /* bad argument / unsupported configuration */
  TFX_ESTATE = -2,   /* call order (e.g. step before bind_buffers) */
  TFX_EDEVICE = -3,  /* HIP runtime error (message has the HIP error string) */
  TFX_ENOMEM = -4
};

/* how the per-tick light action is obtained (TrafficEnv._step(action), traffic_env.py:224-232) */
enum {
  TFX_ACTION_BUFFER = 0,    /* int32 [n_ticks or 1][E][I] device buffer */
  TFX_ACTION_BROADCAST = 1, /* int32 [n_ticks or 1][I]: same action for every env */
  TFX_ACTION_CYCLE = 2,     /* on-device fixed cycle: a = ((tick + env % period) / period) & 1
                               (algorithms/fixed.py:6-7 with spacing = period, env-staggered) */
  TFX_ACTION_GREEDY = 3     /* on-device greedy controller (algorithms/greedy.py:14-16): every `period`
                               ticks phase 1 iff N-S approaches hold more cars than E-W ones */
};

/* how cars enter (TrafficEnv.add_new_cars, traffic_env.py:274-283) */
enum {
  TFX_SPAWN_NONE = 0,
  TFX_SPAWN_COUNTS = 1,  /* int32 [n_ticks or 1][E][n_entry]: cars to add to entry road j this tick
                            (host replays the reference's RandomState schedule) */
  TFX_SPAWN_PERIODIC = 2 /* on-device fixed rate: entry road e gets one car when
                            tick % period == e % period */
};

typedef struct tfx_config {
  int32_t m, n;          /* GridRoad(m, n, l): I = m*n, r = 4I, R = r + 2m + 2n (roadgraph.py:26-33) */
  int32_t capacity;      /* CAPACITY, slots per road incl. slot 0 and the fake leader (traffic_env.py:24) */
  int32_t n_envs;        /* E */
  int32_t planes;        /* 2: (x, v) only; 3: the w array is carried too */
  float length;          /* graph.len */
  float rate;            /* FLAGS.rate, seconds per tick (traffic_env.py:12) */
  /* the archetype, traffic_env.py:35-43 */
  float car_v, car_l, car_a, car_delta, car_v0, car_b, car_T, car_s0;
  int32_t yellow_ticks;  /* YELLOW_TICKS (traffic_env.py:21) */
  float thresh;          /* THRESH (traffic_env.py:17) */
  float detect_dist;     /* the 10 of `length - 10` (traffic_env.py:201) */
  float overflow_penalty;/* OVERFLOW_PENALTY (traffic_env.py:23) */
  float eps;             /* EPS (traffic_env.py:25) */
  int32_t learn_switch;  /* FLAGS.learn_switch (traffic_env.py:15,225-230) */
  int32_t validate;      /* FLAGS.mode == 'validate': advance_hack records trip times (traffic_env.py:240-242) */
  uint32_t entry_spec;   /* generate_entrypoints(spec) bit mask (roadgraph.py:42-51) */
  int32_t env_id_offset; /* global id of env 0 of this handle (env-sharded multi-GPU runs): the
                            on-device controllers use env + offset, so results do not depend on the
                            sharding */
  int32_t layout;        /* 0: xv is the ring layout above; 1: transposed layout - xv is T[tile][k][64][2]:
                            the k-th car behind the fake leader of the road in storage slot (64*tile + j)
                            at T[tile][k][j] (with planes = 3, w is T[tile][k][64] likewise);
                            tfx_xv_pairs gives the size, tfx_export_ring / tfx_import_ring convert to
                            and from the ring layout.  Between calls a column may start one or two rows
                            down (the handle remembers where: two-tick passes, tfx_pair_ticks), so T is
                            meaningful only together with its handle - snapshot and restore envs with
                            tfx_clone_envs, edit the cars through tfx_export_ring / tfx_import_ring, never
                            through T itself */
  /* The reference's `archetypes` TABLE (traffic_env.py:35-43: float32 [n][10]; add_new_cars draws a row per car,
   * :164).  n_archetypes <= 1: the single archetype of the car_* fields above (the reference's default), and the
   * table is ignored.  n_archetypes in 2..TFX_MAX_ARCH, or one row whose delta is not 4: "heterogeneous cars" -
   * every car carries the row it was spawned from through handoffs; needs layout = 1 and planes = 3 (the per-car
   * side word then holds (spawn tick mod 2^24) << 6 | row as integer bits; the envs never run LDS-resident), and takes the rows of spawned
   * cars from tfx_set_spawn_archetypes.  (v/v0)**delta: for an integer delta in 1..8 the binary64 product chain of
   * oracle/idm_oracle.c powi_cr rounded once (for 4: the same value as the single-archetype path); for any other delta
   * in (0, 64] the binary64 log2 / exp2 sequence of include/tfx_pow.h rounded once - both shared bit for bit with the
   * oracle, both within 1 ulp of NumPy's float32 power, which is what the reference runs (traffic_env.py:56).
   * Row layout: v (spawn speed), l, a, delta, v0, b, T, s0. */
  int32_t n_archetypes;
  float arch[TFX_MAX_ARCH][8];
} tfx_config;

typedef struct tfx_buffers {
  float *xv;
  float *w;
  int32_t *leading;
  int32_t *lastcar;
  int32_t *obs;
  float *rewards;
  int32_t *waiting;
  uint8_t *passed_dst;
  int32_t *done_tick;
  float *trip_times;   /* [E][trip_cap] or NULL; (tick - w)/2 of cars leaving the map (traffic_env.py:154) */
  int32_t *n_trips;    /* [E] or NULL */
  int32_t trip_cap;
} tfx_buffers;

typedef struct tfx_handle_s *tfx_handle;

int tfx_abi_version(void);
const char *tfx_last_error(void);

/* TrafficEnv.set_graph (traffic_env.py:361-382) + GridRoad tables (roadgraph.py:26-64): builds
 * dest/phases/nexts/entrypoints for the grid on the device.  */
int tfx_create(const tfx_config *cfg, tfx_handle *out);
int tfx_destroy(tfx_handle h);
/* sizes for the caller's allocations */
int tfx_dims(tfx_handle h, int32_t *I, int32_t *r, int32_t *R, int32_t *n_entry);
/* copies the int32[R] tables (host pointers, any may be NULL); entrypoints is int32[n_entry] */
int tfx_tables(tfx_handle h, int32_t *dest, int32_t *phases, int32_t *nexts, int32_t *entrypoints);
int tfx_bind_buffers(tfx_handle h, const tfx_buffers *b);

/* TrafficEnv._reset (traffic_env.py:259-272).  phase_init: device int32 [E][I] (replaces
 * action_space.sample()).  detected / rewards are left stale, as in the reference. */
int tfx_reset(tfx_handle h, const int32_t *phase_init, void *stream);
/* The batched form's episode boundary: _reset for the envs whose byte in `mask` (device uint8 [E]) is
 * non-zero, the others untouched; phase_init (device int32 [E][I]) is read for those envs only.  The
 * device clock is shared by the batch and keeps running (the reference's `steps` only feeds the
 * spawn-tick stamps, whose differences are what trip times use). */
int tfx_reset_envs(tfx_handle h, const int32_t *phase_init, const uint8_t *mask, void *stream);
/* Call after writing state/leading/lastcar from outside (tests, checkpoint restore): rebuilds the
 * per-road tail cache the light kernel reads. */
int tfx_refresh(tfx_handle h, void *stream);

/* period: TFX_ACTION_CYCLE's cycle, 1 .. TFX_PERIOD_MAX (the bound TFX_TICK_MAX is derived from: the rule adds up to
 * period - 1 to the clock), and TFX_ACTION_GREEDY's spacing, >= 1; anything else is TFX_EINVAL. */
int tfx_set_actions(tfx_handle h, int32_t mode, const int32_t *dev, int32_t period, int32_t per_tick);
int tfx_set_spawns(tfx_handle h, int32_t mode, const int32_t *dev, int32_t period, int32_t per_tick);
/* On-device form of the reference's Poisson generator (traffic_env.py:160-164): per env, gaps of
 * round(Exp(1/cars_per_tick)) ticks between cars, each car on a uniformly drawn entry road; Philox
 * streams keyed by (seed, global env id).  `cdf` (host pointer, n_cdf entries) holds
 * P(gap <= k) * 2^32 for k = 0.. (the last entry must be 0xFFFFFFFF); gym_traffic/devrng.py builds it
 * and mirrors the stream on the host.
 *
 * Heterogeneous handles (tfx_config.n_archetypes): the stream also draws the archetype-table row of every car
 * (`archetypes[random.randint(n)]`, traffic_env.py:164) and binds those rows as the spawn rows (in place of any
 * tfx_set_spawn_archetypes buffer).  Rule 1: take car j (0-based) that the stream puts on entry index ej of global env
 * g in a tick, and let s be the number of cars the stream has put on that entry road of that env before this tick
 * (every car made counts, overflowed ones included; an env that stands still in an agent step makes none).  Its row is
 *     row = (u0 * n_archetypes) >> 32,  u = philox4x32(ctr = {s + j, g, TAG_ARCH, ej}, key = seed)
 * with TAG_ARCH = 0x41524348 (the gap and road draws use 0x47415021 / 0x524F4144 and keep their indices; rules 2 - 5 use
 * 0x45504953, 0x504F4F4C, 0x44434E54 / 0x44524F44 and 0x44524F57: the counts
 * are those of a single-archetype handle with the same seed).  Rows are stored for j < S = C - 2 only: no road takes
 * more cars in one tick (add_car, traffic_env.py:97-114; the cars past it overflow), so no car past it reaches a road.
 * The stream's rows stay bound until a later tfx_set_spawns (which unbinds them: cars get row 0 unless a
 * tfx_set_spawn_archetypes buffer is bound after it), tfx_set_spawn_archetypes (its buffer replaces them) or
 * tfx_set_regular / tfx_set_poisson. */
int tfx_set_poisson(tfx_handle h, double cars_per_tick, uint64_t seed, const uint32_t *cdf, int32_t n_cdf);
/* On-device form of the reference's `regular` generator (traffic_env.py:167-176): with cars_per_tick =
 * cars_per_sec * rate, `burst` = ceil(cars_per_tick) cars in every tick i of the env's generator with
 * i % every == 0, `every` = round(1 / cars_per_tick) (Python's round: half to even; every == 0 means every tick) -
 * the caller passes the two integers; each car on a uniformly drawn entry road (rand.choice(entrypoints), :280) from the
 * Philox stream keyed by (seed, global env id), car c using the same draw index as car c of tfx_set_poisson's stream.
 * The per-tick car COUNTS are exactly the reference's; gym_traffic/devrng.py mirrors the road draws on the host.
 * Heterogeneous handles: every car is archetypes[0] (:174); the call unbinds the rows of an earlier tfx_set_poisson. */
int tfx_set_regular(tfx_handle h, int32_t every, int32_t burst, uint64_t seed);
/* Heterogeneous cars only: the archetype row of every car the count buffer of tfx_set_spawns adds
 * (`archetypes[random.randint(archetypes.shape[0])]`, traffic_env.py:164): device uint8
 * [n_ticks or 1][E][n_entry][per_road], entry j of a road = its j-th car of the tick in creation order (cars
 * beyond per_road, and every car while no buffer is bound or under TFX_SPAWN_PERIODIC - the reference's `regular`
 * generator yields archetypes[0], :174 - get row 0).  The buffer replaces the rows a tfx_set_poisson stream bound. */
int tfx_set_spawn_archetypes(tfx_handle h, const uint8_t *dev, int32_t per_road, int32_t per_tick);

/* Demand profiles on the device: arrivals that change over time (a rush hour, tidal flow), that weigh the entry roads
 * (an arterial against side streets) and whose level differs from env to env of one batch, with no host work per
 * decision.  This is a TRUE per-tick Poisson process - the car count of every tick is Poisson distributed and the ticks
 * are independent - NOT the reference's generator, whose gaps between cars are round(Exp) whole ticks
 * (traffic_env.py:160-164): that one stays tfx_set_poisson.  The rule is stateless: there is no stream position to
 * freeze, clone or rebase, and the rows of any tick can be asked for at any time (tfx_demand_counts).
 *
 * A demand has K = n_profiles (1..16) profiles of S = n_segments (1..64) segments of seg_ticks >= 1 ticks each - the
 * period is P = S * seg_ticks, which must fit an int32 - a tick_offset, and two HOST tables of uint32 thresholds
 * (copied by the call; gym_traffic/devrng.py demand_tables builds them):
 *   count_cdf[K][S][n_cdf], n_cdf in 1..256: count_cdf[k][s][c] = min(floor(P(N <= c) * 2^32), 0xFFFFFFFF) for
 *     N ~ Poisson(mean[k][s]); the last entry is 0xFFFFFFFF: at most n_cdf - 1 cars per env per tick
 *   road_cdf[K][S][n_entry]: the cumulative weights of the entry roads scaled the same way, the last entry 0xFFFFFFFF
 * and profile_of_env, a DEVICE int32 [E] the caller owns: it is read when the arrivals are drawn, so it may be rewritten
 * between calls (a curriculum, domain randomisation) with no re-capture; NULL: profile 0 everywhere.
 *
 * Rule 4.  For the tick whose device clock value is t, env `env` with stream id g (env + env_id_offset until a clone
 * with TFX_CLONE_STREAM hands over its source's id):
 *     k  = profile_of_env[env]                 (outside [0, K): the env gets no cars in this tick)
 *     s  = floormod(t + tick_offset, P) / seg_ticks          (64-bit, floor modulo)
 *     u  = philox4x32(ctr = {t, g, TAG_DCNT, 0}, key = seed)
 *     N  = #{c in 0 .. n_cdf-2 : u0 >= count_cdf[k][s][c]}
 *     car c (0 <= c < N):  w = word (c & 3) of philox4x32(ctr = {t, g, TAG_DROAD, c >> 2}, key = seed)
 *                          ej = #{j in 0 .. n_entry-2 : w >= road_cdf[k][s][j]}
 *     counts[env][ej] += 1
 * with TAG_DCNT = 0x44434E54 and TAG_DROAD = 0x44524F44 (the other draws use 0x47415021, 0x524F4144, 0x41524348,
 * 0x45504953, 0x504F4F4C and, rule 5, 0x44524F57).  Comparisons and integer adds only: the device (k_demand, csrc/tfx_demand.hpp), the host
 * mirror (devrng.demand_counts) and any sharding of the envs over handles agree to the bit.  Cars beyond what a road
 * takes in a tick overflow, as with any count buffer.  The rule reads the handle's clock, like TFX_ACTION_CYCLE and
 * TFX_SPAWN_PERIODIC: it is an input of the handle, nothing about it is reset by tfx_reset, tfx_reset_envs or an episode
 * restart, and a clone on a handle whose clock differs follows that handle's clock.  An env that stands still in an
 * agent step gets no cars for the ticks it skips - what a per-tick count buffer gives it.
 *
 * tfx_step and tfx_agent_step draw the rows of a call up front, in one launch (tfx_step: per chunk of the rows the
 * handle's count buffer holds; a decision must fit it: 64 ticks, fewer beyond 32 MB of counts), and run from there on
 * exactly as they do for a bound per-tick count buffer.
 *
 * tfx_set_demand replaces any earlier spawn rule, as tfx_set_poisson does; a later tfx_set_spawns / tfx_set_poisson /
 * tfx_set_regular replaces it.  TFX_EINVAL, naming the field: a null struct or null tables, sizes out of range, a
 * period that does not fit an int32, a table row that is not non-decreasing or does not end in 0xFFFFFFFF, no entry
 * roads or more than 2048, a heterogeneous handle (rule 4 draws no archetype rows: tfx_set_demand_mixed, below, draws
 * them).  TFX_ESTATE before tfx_bind_buffers.  A refused call changes nothing.
 *
 * tfx_clone_envs with TFX_CLONE_STREAM between two demand handles copies the stream id, so source and clone receive the
 * same cars from then on (under the same profile_of_env entries, which are the caller's); it needs an equal seed, sizes,
 * tick_offset and tables, else TFX_EINVAL, as it is between a demand handle and a Poisson or regular one. */
typedef struct tfx_demand {
  int32_t n_profiles, n_segments, seg_ticks, tick_offset, n_cdf;
  const uint32_t *count_cdf, *road_cdf;   /* HOST */
  const int32_t *profile_of_env;          /* DEVICE [E] or NULL */
  uint64_t seed;
} tfx_demand;
int tfx_set_demand(tfx_handle h, const tfx_demand *dm);
/* The rows rule 4 makes for clock ticks tick0 .. tick0 + n_ticks - 1, into the caller's device buffer int32
 * [n_ticks][E][n_entry]: a preview for users (what will arrive in the next hour?) and the direct test handle on
 * k_demand.  Read-only, one launch on `stream`, no host synchronisation; captured graphs stay valid and
 * tfx_debug_fail_after does not count the launch.  TFX_EINVAL: a NULL handle, NULL `out`, a negative n_ticks;
 * TFX_ESTATE before tfx_bind_buffers or without a demand. */
int tfx_demand_counts(tfx_handle h, int32_t tick0, int32_t n_ticks, int32_t *out, void *stream);

/* Demand profiles for heterogeneous handles (tfx_config.n_archetypes): rule 4's cars, each with an archetype-table row
 * drawn by (profile, segment) weights - a truck share that follows the time of day and differs from env to env.
 * row_cdf is a third HOST table (copied by the call; devrng.demand_row_table builds it) in the format of road_cdf:
 *   row_cdf[K][S][n_rows], n_rows = the handle's n_archetypes: the cumulative weights of the rows scaled by 2^32, every
 *   row of the table non-decreasing, its last entry 0xFFFFFFFF.  A row of weight zero is not drawn.
 *
 * Rule 5.  Take car c (0 <= c < N) of rule 4's item (clock tick t, stream id g, profile k, segment s), and let ej be the
 * entry road rule 4 gives it:
 *     v   = word (c & 3) of philox4x32(ctr = {t, g, TAG_DROW, c >> 2}, key = seed)
 *     row = #{i in 0 .. n_rows-2 : v >= row_cdf[k][s][i]}
 *     j   = #{c' < c : ej(c') == ej}           (creation order on a road = car-index order)
 *     rows[tick][env][ej][j] = row             if j < S,   S = min(C - 2, n_cdf - 1)
 * with TAG_DROW = 0x44524F57.  Comparisons and integer adds only; the counts are exactly rule 4's, and the new draws use
 * a tag of their own: a single-archetype handle with the same seed sees the same cars.  S loses nothing: no road takes
 * more than C - 2 cars in a tick (the cars past it overflow) and no env receives more than n_cdf - 1.  Entries of a road
 * past min(count, S) are unspecified (nobody reads them; the mirror, devrng.demand_rows, returns 0 there).  Like rule 4
 * the rule is stateless: restarts, warm pools, clones and clocks need nothing new, and an env that stops in a decision
 * does not consume the later rows.
 *
 * The call makes every check tfx_set_demand makes, and returns TFX_EINVAL, naming the field, for a null row_cdf, n_rows
 * other than the handle's n_archetypes, a row_cdf row that decreases or does not end in 0xFFFFFFFF, and a handle that is
 * not heterogeneous (that one takes tfx_set_demand); TFX_ESTATE before tfx_bind_buffers.  A refused call changes nothing.
 * It replaces any earlier spawn rule and binds the rows it draws as the spawn rows, per tick like the counts, wherever
 * the cars move (tfx_step, tfx_agent_step, tfx_move_cars); a later tfx_set_spawns, tfx_set_poisson, tfx_set_regular,
 * tfx_set_demand or tfx_set_spawn_archetypes does what it does after a tfx_set_poisson stream's rows.  A decision must
 * fit the rows the handle's buffer holds: counts and archetype rows share one chunk (64 ticks, fewer beyond 32 MB of
 * counts or 256 MB of rows: 16 at 4096 envs x 64 entry roads x S = 64).  tfx_demand_counts works as on a plain demand.
 * tfx_clone_envs with TFX_CLONE_STREAM compares row_cdf with the other tables ("demand tables"). */
int tfx_set_demand_mixed(tfx_handle h, const tfx_demand *dm, const uint32_t *row_cdf, int32_t n_rows);
/* Rules 4 and 5 together for clock ticks tick0 .. tick0 + n_ticks - 1, into the caller's device buffers: counts int32
 * [n_ticks][E][n_entry] (what tfx_demand_counts gives) and rows uint8 [n_ticks][E][n_entry][S] (entry j of a road is
 * written for j < min(count, S), the rest is left as it was).  Read-only, one launch on `stream`, no host
 * synchronisation; captured graphs stay valid and tfx_debug_fail_after does not count the launch.  TFX_EINVAL: a NULL
 * handle or buffer, a negative n_ticks; TFX_ESTATE before tfx_bind_buffers or without a mixed demand. */
int tfx_demand_rows(tfx_handle h, int32_t tick0, int32_t n_ticks, int32_t *counts, uint8_t *rows, void *stream);
/* S of rule 5 for the mixed demand the handle holds.  TFX_ESTATE without one. */
int tfx_demand_rows_per_road(tfx_handle h, int32_t *per_road);

/* TrafficEnv._step (traffic_env.py:224-248), n_ticks times: phase/elapsed update, spawns,
 * move_cars, advance_finished_cars | advance_hack, steps += 1. */
int tfx_step(tfx_handle h, int32_t n_ticks, void *stream);
/* The two halves on their own, for kernel-level parity tests:
 * move_cars (traffic_env.py:187-212, incl. update_lights :81-94; also applies the phase update and
 * the spawns of the current tick) and advance_finished_cars / advance_hack (:117-157). */
int tfx_move_cars(tfx_handle h, void *stream);
int tfx_advance_finished_cars(tfx_handle h, void *stream);

/* One agent decision = the Repeater (+ Remi) wrappers of traffic_test.py:27-64 fused on the device:
 * n_ticks x _step with the held action; `passed` accumulates, `detected` keeps the last tick, an
 * env that overflows stops for the rest of the step (`if done: break`); then, with remi != 0,
 * remi_reward() (else the rewards are the sum over the ticks).  Outputs (device pointers, any may
 * be NULL): aobs float32 [E][2r+I] = [sum passed | last detected | elapsed/100*(2*phase-1)],
 * areward float32 [E][I], adone uint8 [E].  The launch sequence is captured into a HIP graph on
 * first use and replayed afterwards.  Needs ONE action for the whole step (a held buffer, the cycle
 * rule or the greedy controller); any spawn rule works, a per-tick count buffer must hold at least
 * n_ticks rows (row t feeds tick t of the step; rows after an env's overflow are not consumed). */
int tfx_agent_step(tfx_handle h, int32_t n_ticks, int32_t remi, float *aobs, float *areward,
                   uint8_t *adone, void *stream);

/* Episodes on the device (default off: tfx_agent_step then does what it always did, launch for launch).  Every
 * algorithm of the reference runs episodes of FLAGS.episode_len decisions and resets (`for i in range(FLAGS.episode_len)`,
 * algorithms/greedy.py:13, fixed.py:16, spacedgreedy.py:16; traffic_test.py:20: 600 s / 5 s = 120 decisions) and prints
 * each episode's return (print_running_stats(episode_reward(...))).  With enabled != 0 tfx_agent_step does three more
 * things inside the same submission (and the same captured graph):
 *
 *   1. begin of the decision - masked restart: every env whose previous decision ended its episode is reset exactly as
 *      tfx_reset_envs would reset it, its phases drawn on the device.  Rule 2: the phase of intersection i in episode
 *      number n (ep_index: 0 for the episode the caller's tfx_reset started, 1 for the first restart, ...) of global env
 *      g = env + env_id_offset is
 *          phase = u0 & 1,  u = philox4x32(ctr = {n, g, TAG_EPISODE, i}, key = seed)
 *      with TAG_EPISODE = 0x45504953 (the arrival streams use 0x47415021, 0x524F4144 and 0x41524348); it depends on
 *      nothing else, so not on how envs are sharded over handles.  gym_traffic/devrng.py episode_phases mirrors it.
 *      This is "next-step auto-reset": the observation a decision returns for an env that ended is its terminal one; the
 *      new episode starts with the next decision, under that decision's action - the state sequence of the loop
 *      `tfx_agent_step(); tfx_reset_envs(phases, terminated | truncated)`.  Arrival streams run on across a restart, as
 *      they do under tfx_reset_envs.  Validate mode: the trip log of an ended episode stays readable until the next
 *      decision begins (the restart clears n_trips).
 *   2. the ticks, untouched.
 *   3. end of the decision - accounting, per env, in decision order (float32 adds, so exactly reproducible):
 *        ep_return[env][:] += areward;  ep_len[env] += 1
 *        terminated = adone (overflow since the decision began);
 *        truncated[env] = !terminated && max_decisions > 0 && ep_len[env] == max_decisions
 *        where terminated | truncated:  final_return[env][:] = ep_return, final_len[env] = ep_len, both accumulators
 *        cleared, ep_index[env] += 1, and the env is marked for the restart of step 1.
 *      final_return / final_len keep the last ended episode's values elsewhere.
 *
 * tfx_reset and tfx_reset_envs clear ep_return, ep_len and the restart mark of the envs they reset (they abandon an
 * episode; ep_index does not move).  The buffers are the caller's (device pointers, all required when enabled; the
 * caller zeroes them): ep_return / final_return float32 [E][I], ep_len / final_len / ep_index int32 [E], truncated
 * uint8 [E].  tfx_set_episodes itself clears the restart marks.  enabled == 0: `b` may be NULL, max_decisions and seed
 * are ignored.  TFX_EINVAL for a negative max_decisions or a missing buffer, TFX_ESTATE before tfx_bind_buffers.
 * max_decisions == 0: no time limit (episodes end on overflow only). */
typedef struct tfx_episode_buffers {
  float *ep_return;
  int32_t *ep_len;
  float *final_return;
  int32_t *final_len;
  uint8_t *truncated;
  int32_t *ep_index;
} tfx_episode_buffers;
int tfx_set_episodes(tfx_handle h, int32_t enabled, int32_t max_decisions, uint64_t seed, const tfx_episode_buffers *b);

/* Warm restarts: while episodes are on (tfx_set_episodes), an env whose previous decision ended its episode restarts as
 * a clone of an env of `pool` instead of empty.  pool == NULL detaches.  Every env of the reference's training setup is
 * `Repeater -> WarmupWrapper(FLAGS.warmup_lights) -> Remi` (traffic_test.py:84-86): reset() runs warmup_lights decisions
 * under sampled actions before the agent sees anything, so no episode starts on an empty map.  Here the warm-up is paid
 * once, for the envs of a second handle (the pool), and a restart copies one of them.
 *
 * Rule 3 (the pool slot): global env g = env + env_id_offset, starting its episode number n (ep_index[env] as step 3 of
 * the previous decision left it - the n of rule 2), takes env
 *     slot = (u0 * n_pool) >> 32,  u = philox4x32(ctr = {n, g, TAG_POOL, 0}, key = seed)
 * of the pool, n_pool = the pool handle's n_envs, seed = the one given to tfx_set_episodes, TAG_POOL = 0x504F4F4C (the
 * other draws use 0x47415021, 0x524F4144, 0x41524348 and 0x45504953).  It depends on nothing else, so not on how envs
 * are sharded over handles.  gym_traffic/devrng.py episode_pool_slots mirrors it.
 *
 * With a pool attached, step 1 of a decision does for every marked env exactly what tfx_clone_envs(h, pool, src, 0,
 * stream) does with src[env] = slot (-1 for the other envs), in the decision's own submission and with no launch more
 * than an episodes-on decision makes anyway: cars, counters, lights, the whole obs row (current_phase / elapsed are the
 * pool env's: rule 2 is not drawn), caches and, in validate mode, the trip log arrive from the pool env, ticks rebased by
 * tick(h) - tick(pool) read on the device.  The env keeps its own arrival stream and position (arrival streams run on
 * across a restart) and its own ep_* accounting; the clone_skipped counter is not touched (a slot is always valid).
 * Steps 2 and 3 are what they were.
 *
 * The pool is read, never written, and read when the restart runs: it is a pointer, not a snapshot - a caller may keep
 * it fresh by stepping it between decisions on the same stream; work on the pool pending on ANOTHER stream is the
 * caller's to order, as for tfx_clone_envs.  The caller keeps the pool alive (and its buffers bound) while it is
 * attached.  Both handles bound (else TFX_ESTATE), on the same device, with the same world as tfx_clone_envs asks of
 * dst != src (else TFX_EINVAL with a message naming the field; n_envs and env_id_offset may differ); pool == h is
 * TFX_EINVAL.  A refused call changes nothing.  Attaching and detaching are allowed before or after tfx_set_episodes
 * (the pool is inert while episodes are off) and re-capture the agent-step graph.  tfx_debug_fail_after counts the
 * restart's launch like the other launches of the decision. */
int tfx_set_episode_pool(tfx_handle h, tfx_handle pool);

/* remi (traffic_env.py:64-78) via TrafficEnv.remi_reward (:384-387) */
int tfx_remi(tfx_handle h, void *stream);
/* cars_on_roads (traffic_env.py:214-218): out device int32 [E][R] */
int tfx_cars_on_roads(tfx_handle h, int32_t *out, void *stream);
/* done flag of _step (traffic_env.py:246-248): out[k] = env k overflowed in a tick >= since_tick */
int tfx_done(tfx_handle h, uint8_t *out, int32_t since_tick, void *stream);

int tfx_get_tick(tfx_handle h, int32_t *tick);              /* TrafficEnv.steps */
/* also clears the per-env overflow stamps; TFX_EINVAL (nothing changes) outside 0 .. TFX_TICK_MAX */
int tfx_set_tick(tfx_handle h, int32_t tick);
/* live cars advanced by move_cars since the last tfx_reset_counters (synchronises the stream) */
int tfx_vehicle_updates(tfx_handle h, uint64_t *out, void *stream);
int tfx_reset_counters(tfx_handle h, void *stream);
/* Per-kernel timing for the roofline report: with max_ticks > 0 the next tfx_step calls record HIP
 * events on the launch stream around the move and advance kernels of up to max_ticks ticks;
 * tfx_profile_read waits for them and returns (and clears) the summed durations. 0 disables. */
int tfx_profile(tfx_handle h, int32_t max_ticks);
int tfx_profile_read(tfx_handle h, double *move_ms, double *advance_ms, int32_t *n_ticks);
/* (x, v) pairs the caller's xv buffer must hold for this handle's layout (and, with planes = 3 on the
 * transposed layout, floats its w buffer must hold) */
int tfx_xv_pairs(tfx_handle h, int64_t *pairs);
/* Transposed-layout handles: copy the cars to / from ring-layout arrays (device pointers): ring_xv
 * float32 [E][R][C][2] with the fake leader's x in slot `leading` as the reference keeps it, ring_w
 * float32 [E][R][C] (spawn ticks; may be NULL, ignored unless planes = 3), ring_a uint8 [E][R][C] (archetype
 * row per car; may be NULL, ignored unless the handle has heterogeneous cars).  After an import call
 * tfx_refresh. */
int tfx_export_ring(tfx_handle h, float *ring_xv, float *ring_w, uint8_t *ring_a, void *stream);
int tfx_import_ring(tfx_handle h, const float *ring_xv, const float *ring_w, const uint8_t *ring_a, void *stream);
/* What the next call depends on.  The results of the next tfx_step / tfx_agent_step / tfx_move_cars +
 * tfx_advance_finished_cars depend on four things only: the ring image (the cars as tfx_export_ring shows them, leading,
 * lastcar), the other bound buffers (obs, rewards, waiting, passed_dst, done_tick, the trip log), the clock
 * (tfx_get_tick) and the inputs bound for the call.  A handle that has run anything before and a new one that was
 * given the same four (tfx_reset, the buffers copied, tfx_import_ring + tfx_refresh, tfx_set_tick, then done_tick -
 * tfx_set_tick clears it) compute the same bits from then on; importing a handle's own export changes nothing.  Three
 * things the handle owns and the caller cannot export travel through tfx_clone_envs alone: the position of an on-device
 * arrival stream (TFX_CLONE_STREAM), the greedy controller's held action, and the episode marks and accounting
 * (TFX_CLONE_EPISODE).  Everything else a handle keeps between calls - row offsets of the two-tick pass, tail and
 * record caches, the stamps of overflows, of the serial advance and of the risk bound, the second stream's clock, its
 * captured graphs - is rebuilt or ignored: a stamp left by an earlier call may cost time (an env takes the exact serial
 * or one-tick form once more), it never changes a result.  tests/test_gpu_transplant.py holds every step path to this. */

/* Two of the IDM's three divisions have a constant divisor (2*sqrt(a*b) and v0).  At tfx_create the
 * library checks on the device, exhaustively over the admitted numerator range, that the
 * reciprocal form it would like to use is bit-identical to IEEE division for these constants;
 * `enabled` reports whether it is in use, `mismatches` the count found (0 when enabled). */
int tfx_fastdiv_status(tfx_handle h, int32_t *enabled, uint64_t *mismatches);
/* launch geometry of the move kernel, for the roofline report */
int tfx_launch_info(tfx_handle h, int32_t *grid, int32_t *block, int32_t *waves_per_road);
/* Ticks of this handle that ran in the LDS-resident multi-tick kernel (k_res: every tick of a tfx_step
 * or tfx_agent_step call in ONE launch, the envs' cars held in a compute unit's LDS) since tfx_create,
 * and whether the handle's envs fit it at all (`capable`: two lanes per road - or one - within 512
 * lanes and 160 KB of rings per workgroup: cfg0, cfg1, the reference's 3x3 default do; cfg2 and cfg4
 * do not).  A capable handle takes k_res on its own unless trip times are recorded (validate mode);
 * every input rule runs inside it (held / per-tick buffers, fixed cycle, periodic arrivals, the
 * on-device Poisson stream, the greedy controller) and tfx_agent_step's remi / observation / done tail
 * too; results are bit-identical either way.  Environment switches read by tfx_bind_buffers:
 * TFX_RESIDENT=0 turns it off, TFX_RES_LPR=1 forces one lane per road, TFX_RES_EPB=n packs n envs per
 * workgroup, TFX_RES_MIN_TICKS=n leaves calls shorter than n ticks to the per-tick kernels. */
int tfx_fused_ticks(tfx_handle h, int64_t *ticks, int32_t *capable);
/* Ticks of this handle that ran as two-tick passes since tfx_create (transposed layout: k_move_tt takes every
 * car but the head of each road through TWO ticks per trip through HBM, k_edge finishes the second tick for
 * the heads and the cars that joined a road in between - csrc/tfx_move_tt.hpp; launches that leave wave slots empty
 * split every tile's walk over 2, 4 or 8 wavefronts: k_move_tts, csrc/tfx_move_tts.hpp).  tfx_step and tfx_agent_step
 * use them on their own for calls of two ticks or more of every handle whose envs do not fit k_res - heterogeneous
 * cars from 4 tiles of 64 roads per compute unit on; results are
 * bit-identical to the tick-by-tick kernels.  TFX_PAIRS=0 turns them off, TFX_PAIRS=2 forces them at any size. */
int tfx_pair_ticks(tfx_handle h, int64_t *ticks);
/* ... of which the rest of the pair - advance_finished_cars of the first tick (traffic_env.py:117-135), the road
 * heads' second tick, advance_finished_cars of the second - ran as ONE launch with a workgroup per env (k_tail,
 * csrc/tfx_tail.hpp) instead of three: tfx_step does so on its own from one env per compute unit on, unless the
 * second tick's inputs are produced on the device in between (tfx_set_poisson, TFX_ACTION_GREEDY).  TFX_TAIL=0
 * turns it off, TFX_TAIL=2 forces it at any batch size; results are bit-identical. */
int tfx_tail_ticks(tfx_handle h, int64_t *ticks);
/* Inside tfx_agent_step a pair of ticks runs as ONE pass over the cars only for envs in which the pair's first tick
 * provably cannot overflow a ring (a bound on how far a car can move, csrc/tfx_move_tt.hpp risk_lane); the others take
 * the pair one tick at a time, which is what `if done: break` (traffic_test.py:55) needs.  pairs = env-pairs that took
 * that slower, equally exact path since tfx_create (synchronises the stream). */
int tfx_slow_pairs(tfx_handle h, uint64_t *pairs, void *stream);
/* Ticks of tfx_step calls that ran as two halves of the env range, the second half on a stream the handle owns
 * (forked from and joined to the caller's stream with events, so the call keeps its stream semantics): the
 * latency-bound per-road launch of one half then runs under the other half's pass over the cars.  Used for calls
 * of pairs whose halves still fill the chip, never while tfx_profile is timing kernels.  TFX_SPLIT=0 turns it off,
 * TFX_SPLIT=2 forces it at any batch size; results are bit-identical (envs share nothing, traffic_env.py:361-382). */
int tfx_split_ticks(tfx_handle h, int64_t *ticks);
/* name of the kernel that moved the cars in the handle's last tick ("k_move_tt", "k_move_tts", "k_move_t", "k_move_ts",
 * "k_res", "k_move_dma", ...), for the roofline report; "" before the first step */
const char *tfx_step_kernel(tfx_handle h);

/* Error-path testing: the n-th kernel launch a later tfx_step / tfx_agent_step / tfx_move_cars /
 * tfx_advance_finished_cars call would make (counted from this call, over calls) is not made and that call returns
 * TFX_EDEVICE instead.  The handle stays usable: its second stream is joined back, nothing a sequence changes in the
 * handle while it enqueues stays changed; the envs' state is then somewhere inside the failed call (reset or reload
 * it).  0 switches the injection off. */
int tfx_debug_fail_after(tfx_handle h, int32_t n_launches);

/* Clone env states on the device: env e of `dst` becomes a copy of env src_of_env[e] of `src`; -1 leaves env e
 * untouched.  src_of_env is a DEVICE int32 [dst E] (a planner computes it with an argmax on the device).  One launch
 * on `stream`, no host synchronisation, no bound pointer changes: captured agent-step / step graphs stay valid.  This is
 * what lookahead controllers (K candidate light settings from the state an env is in), population methods with common
 * random numbers, and snapshot / restore need; the reference has no counterpart (its env is one Python object,
 * copy.deepcopy would do).
 *
 * dst != src (snapshot / branch: the second handle is the stash or the branch pool): both bound, on the same device,
 *   with the same world - m, n, capacity, planes, layout, length, rate, validate, learn_switch, entry_spec, the same
 *   archetype table, the same kinds ordering of storage slots, and the same per-tick constants (yellow_ticks, thresh,
 *   detect_dist, overflow_penalty, eps); anything else is TFX_EINVAL with a message naming the field.  n_envs and
 *   env_id_offset may differ.  An index outside [-1, src E) leaves env e untouched and is counted.  The launch is
 *   ordered on `stream` only: work of `src` still pending on ANOTHER stream must be ordered before it by the caller
 *   (an event, or a synchronisation).
 * dst == src (in place, no staging buffer): a source must not itself be overwritten - env e is cloned only if
 *   s = src_of_env[e] has src_of_env[s] == -1 or == s.  An env that breaks the rule, or whose index is outside
 *   [-1, E), is LEFT UNTOUCHED and counted in a device counter that tfx_clone_skipped returns (and clears).  No index
 *   array has undefined behaviour.  gym_traffic/devrng.py clone_plan states the rule in NumPy.
 *
 * What a clone always carries: the live cars (x, v; with planes == 3 the side word: spawn tick, and for heterogeneous
 * cars the table row), leading, lastcar, the whole obs row, rewards, waiting, passed_dst, done_tick, in validate mode
 * n_trips and the logged trip_times, the greedy controller's held decision, and every handle-owned word a later kernel
 * reads for that env (the column offsets a two-tick pass leaves, tail and leader caches, road records, outboxes).
 * After a clone ANY sequence of calls gives env e the bits it would give its source under the same inputs - also
 * between two two-tick passes, without tfx_refresh.
 *
 * Clocks: every handle has its own device clock.  Across handles everything stored as a tick is rebased by
 * tick(dst) - tick(src), read on the device: spawn ticks (the plain float, and modulo 2^24 inside the heterogeneous
 * side word), non-zero done_tick stamps, and the handle's own per-env tick stamps (which env takes the serial advance
 * or a pair of ticks one at a time - copied and rebased rather than cleared, so that a clone taken between
 * tfx_move_cars and tfx_advance_finished_cars continues as its source does); trip times of a cloned env are then
 * those of its source.  Input rules that read the clock (TFX_ACTION_CYCLE, TFX_SPAWN_PERIODIC) are inputs of the
 * DESTINATION handle and are not cloned: a clone on a handle whose clock differs follows that handle's cycle.
 *
 * TFX_CLONE_STREAM: the clone also continues its source's on-device arrival stream (tfx_set_poisson / tfx_set_regular):
 *   position (gap_left, draws, the per-entry car counters `seq` of rule 1) AND identity.  Every env has a stream id - a
 *   handle-owned uint32, set to env + env_id_offset by tfx_set_poisson / tfx_set_regular - that keys its gap, road and
 *   archetype-row draws (the `g` of rule 1); the flag copies id and position, so source and clone receive the same cars
 *   on the same roads with the same rows from then on.  Needs the same stream in both handles (kind, seed, rate /
 *   `every`, `burst`), else TFX_EINVAL.  Without the flag a clone keeps its own stream and position: same world,
 *   independent arrivals.  Rule 2 (episode phases) stays keyed by the env's own global id.
 * TFX_CLONE_EPISODE: with episodes on in both handles (tfx_set_episodes) ep_return, ep_len, ep_index and the restart mark
 *   are copied too (final_* and truncated describe past decisions and are not).  Episodes off in both: the flag is
 *   ignored; on in exactly one: TFX_EINVAL.  Without the flag the destination's accounting is left alone.
 * tfx_debug_fail_after counts the clone's launch on `dst`. */
enum { TFX_CLONE_STREAM = 1, TFX_CLONE_EPISODE = 2 };
int tfx_clone_envs(tfx_handle dst, tfx_handle src, const int32_t *src_of_env, int32_t flags, void *stream);
/* envs tfx_clone_envs calls on `h` (as dst) left untouched against the caller's wish since the last call of this
 * (synchronises the stream, clears the counter) */
int tfx_clone_skipped(tfx_handle h, uint64_t *skipped, void *stream);   /* synchronises the stream */
/* Road measures on the device: the standard traffic measures of signal control - cars halted per approach, the queue at
 * the stop line, speeds - as four words per road, from one read-only pass over the live cars (k_measure,
 * csrc/tfx_measure.hpp).  The reference has no counterpart beyond cars_on_roads (traffic_env.py:214-218); without this
 * call the route is tfx_export_ring of every ring slot and array code over the image.
 *
 * Definition, as a function of the image tfx_export_ring would produce at that moment (on a ring-layout handle: of xv
 * itself) - so it is defined in every state a handle can be in: between two-tick passes, after a clone, after
 * tfx_import_ring + tfx_refresh, between tfx_move_cars and tfx_advance_finished_cars.  For road e of env k take its cars
 * in order from the head, j = 0 .. n-1: car j sits in ring slot wrap(leading + 1 + j) (wrap: a slot past C - 1 is slot
 * 1, traffic_env.py:46-47), n is the count tfx_cars_on_roads returns; the fake leader is not a car.
 *   in range    x >= x_from (x_from = -INFINITY: every car; a NaN x is out of range)
 *   n_cars      the number of cars in range (x_from = -INFINITY: what tfx_cars_on_roads returns)
 *   n_halted    the number of cars in range with v < halt_speed - float32, exact, strict
 *   queue       the largest q such that cars 0 .. q-1 are all in range and all have v < halt_speed: the platoon
 *               standing at the head of the road
 *   speed_sum   the float32 sum of v over the cars in range: s = 0.0f, then s = s + v car by car in ascending j, one
 *               rounding per add, never reassociated - the same bits on both layouts and from a host loop
 * Outputs are device pointers, [E][R] by the reference's road id (like `leading`); any may be NULL, at least one must not
 * be.  Without TFX_MEASURE_ACCUMULATE every bound output is overwritten (a road with no cars gets 0); with it
 * out = out + value: integer adds, and ONE float32 add of the road's sum - a caller integrates over decisions (halted
 * vehicle-ticks as a delay figure) by measuring between calls.
 *
 * One launch on `stream`, no host synchronisation; nothing in the handle or in the caller's bound state is written:
 * captured step / agent-step graphs stay valid, and tfx_debug_fail_after does not count the launch.  TFX_EINVAL: a NULL
 * handle, a NULL `out`, all four pointers NULL, unknown flag bits, a NaN halt_speed or x_from (infinities are fine);
 * TFX_ESTATE before tfx_bind_buffers.  gym_traffic/devrng.py road_measures states the definition in NumPy.
 * TFX_MEASURE_GRID=n (read by tfx_create) caps the launch at n workgroups. */
typedef struct tfx_measure_buffers {
  int32_t *n_cars;     /* cars in range */
  int32_t *n_halted;   /* cars in range with v < halt_speed */
  int32_t *queue;      /* standing queue at the head of the road */
  float *speed_sum;    /* sum of v over the cars in range */
} tfx_measure_buffers;
enum { TFX_MEASURE_ACCUMULATE = 1 };
int tfx_road_measures(tfx_handle h, float halt_speed, float x_from, const tfx_measure_buffers *out, int32_t flags,
                      void *stream);
/* Test support: the launch geometry tfx_road_measures uses for this handle - workgroups, and wavefronts (one per
 * (env, tile) item at a time; more items than wavefronts: every wavefront strides over several). */
int tfx_measure_launch(tfx_handle h, int32_t *grid, int32_t *waves);
/* Road cells on the device: the discrete traffic state encoding - every road cut into n_cells cells along its length,
 * each with its car count and the sum of its cars' speeds - from one read-only pass over the live cars (k_cells,
 * csrc/tfx_cells.hpp).  tfx_road_measures generalised from four words per road to n_cells cells per road; without this
 * call the route is tfx_export_ring of every ring slot and array code over the image.
 *
 * Definition, as a function of the image tfx_export_ring would produce at that moment (on a ring-layout handle: of xv
 * itself), so it is defined in every state a handle can be in, as the measures are.  `edges` is a HOST array of
 * n_cells + 1 float32 values, strictly ascending; -INFINITY is allowed as the first and +INFINITY as the last.  For road
 * e of env k take its cars in order from the head, j = 0 .. n-1: car j sits in ring slot wrap(leading + 1 + j), n is the
 * count tfx_cars_on_roads returns.
 *   in range     edges[0] <= x < edges[n_cells]; a NaN x is in no cell
 *   its cell     b = #{k in 1 .. n_cells-1 : x >= edges[k]} - comparisons only, no arithmetic on x, so there is nothing
 *                for contraction or reciprocal forms to change; a car exactly on an edge belongs to the upper cell
 *   n_cars[b]    the number of cars of cell b
 *   speed_sum[b] s = 0.0f, then s = s + v over the cars of cell b in ascending j, one rounding per add, never
 *                reassociated - the same bits on both layouts and from a host loop
 * Outputs are device pointers, [E][R][n_cells] by the reference's road id; either may be NULL, not both.  Without
 * TFX_CELLS_ACCUMULATE every bound output is overwritten (an empty cell gets 0); with it out = out + value: an integer add,
 * and ONE float32 add per cell.  With n_cells = 1 and edges = {x_from, +INFINITY} the two planes are tfx_road_measures'
 * n_cars and speed_sum, bit for bit.
 *
 * One launch on `stream`, no host synchronisation (the edges travel by value); nothing in the handle or in the caller's
 * bound state is written: captured step / agent-step graphs stay valid, and tfx_debug_fail_after does not count the
 * launch.  TFX_MEASURE_GRID caps this launch too.  TFX_EINVAL: a NULL handle, NULL `edges`, NULL `out`, both pointers
 * NULL, n_cells outside 1 .. TFX_MAX_CELLS, a NaN edge, edges not strictly ascending, unknown flag bits; TFX_ESTATE before
 * tfx_bind_buffers.  gym_traffic/devrng.py road_cells states the definition in NumPy, cell_edges makes uniform edges. */
#define TFX_MAX_CELLS 32
typedef struct tfx_cell_buffers {
  int32_t *n_cars;     /* [E][R][n_cells] by road id; may be NULL */
  float *speed_sum;    /* [E][R][n_cells]; may be NULL */
} tfx_cell_buffers;
enum { TFX_CELLS_ACCUMULATE = 1 };
int tfx_road_cells(tfx_handle h, const float *edges, int32_t n_cells, const tfx_cell_buffers *out, int32_t flags,
                   void *stream);
/* Test support: the launch geometry tfx_road_cells uses for this handle and n_cells - workgroups, and wavefronts. */
int tfx_cells_launch(tfx_handle h, int32_t n_cells, int32_t *grid, int32_t *waves);
/* Top-view frames on the device: chosen envs of the batch drawn as RGBA images - the picture TrafficEnv.render() gives of
 * one env, and the vehicle-position image signal-control agents read - from one read-only pass over the live cars of
 * those envs (k_frames, csrc/tfx_frames.hpp).  The cost follows the envs drawn, not the batch; without this call the
 * route is tfx_export_ring of every ring slot of every env and a host loop over the cars.
 *
 * Definition, as a function of the image tfx_export_ring would produce at that moment (on a ring-layout handle: of xv
 * itself), of leading / lastcar and of the light words inside obs - so it is defined in every state a handle can be in,
 * as the measures are.  It is integer geometry; the only float step is one float32 multiply per car end.
 *   size      px = S pixels per road length, TFX_FRAME_PX_MIN <= S <= TFX_FRAME_PX_MAX.  A frame is H x W pixels of 4
 *             bytes R, G, B, A; W = (n + 1) * S + 1, H = (m + 1) * S + 1 (tfx_frame_size).  The image row is the grid's
 *             row coordinate (row 0 at the top); intersection (row, col) has its centre at pixel (cx, cy) =
 *             ((col + 1) * S, (row + 1) * S), (column, row) of the image.
 *   roads     every road is one pixel wide and lies one pixel beside the centre line, on the side where
 *             GridRoad._unit_segments (roadgraph.py) puts its eps.  With t the pixel along the road from its start, the
 *             train road of direction block d into intersection (row, col) has its pixel t at
 *               d = 0: (cx - S + t, cy - 1)    d = 1: (cx + S - t, cy + 1)
 *               d = 2: (cx + 1, cy - S + t)    d = 3: (cx - 1, cy + S - t)
 *             An exit road continues the road it follows, away from the grid, from the centre of that road's
 *             intersection on: the four exit blocks, in _unit_segments' order, continue d = 3 out of row 0 ((cx - 1,
 *             cy - t)), d = 0 out of the last column ((cx + t, cy - 1)), d = 2 out of the last row ((cx + 1, cy + t)) and
 *             d = 1 out of column 0 ((cx - t, cy + 1)).
 *   owned     a road owns the pixels t = 2 .. S - 2 only, S - 3 of them: it stays out of the 3 x 3 box round each
 *             intersection.  No two roads share a pixel and every owned pixel lies inside the frame.
 *   colours   every byte outside a road's own pixels is 0xFF (white, alpha 255).  A road's own pixels take its light's
 *             colour (update_colors, traffic_env.py:335-346; gym_traffic.render.light_colours): with phase(e) = 1 for d <
 *             2, else 0, and the words current_phase / elapsed of the road's intersection, yellow (255,255,0) iff phase(e)
 *             == current_phase and elapsed < yellow_ticks; red (255,0,0) iff phase(e) == current_phase and not so fresh,
 *             or the other phase and fresh; green (0,255,0) otherwise, and on every exit road.  Alpha is 255.
 *   cars      take road e's cars from the head, as the measures do.  A car's length l is that of the archetype row it
 *             carries (a single-archetype handle: car_l).  With k = float32(S - 3) / float32(length), computed once on
 *             the host, a car whose x is NaN is not drawn; otherwise
 *               a = clamp(floorf(x * k), 0, S - 4)    b = clamp(floorf((x - l) * k), 0, S - 4)
 *             clamped in float before the conversion, and the car turns pixels t = 2 + b .. 2 + a of its road blue
 *             (0,0,255).  Neither expression has a form a compiler could contract; the clamp makes the rule total: x >
 *             length (between tfx_move_cars and the advance), x - l < 0, infinities.
 * Every pixel has one writer and one value: the device stores each road pixel once, with its final value.
 *
 * env_ids: device int32 [n_frames], frame f shows env env_ids[f]; NULL: envs 0 .. n_frames - 1 (then n_frames <= E).
 * An id outside [0, E) is no error: that frame is all background, nothing is read for it.  An env may appear in several
 * frames.  out: device memory, [n_frames][H][W][4] bytes.  TFX_FRAMES_ROADS_ONLY: the background is not written, only the
 * road pixels are - the caller promises that `out` holds the background of an earlier call with the same px (a video
 * logger that reuses one tensor); a frame whose id is out of range then has its road pixels written white.
 *
 * At most one memset (the background) and one launch on `stream`, no host synchronisation; nothing in the handle or in
 * the caller's bound state is written: captured step / agent-step graphs stay valid, and tfx_debug_fail_after does not
 * count the launch.  TFX_MEASURE_GRID and TFX_GRID_CAP cap the launch as they cap the cells'.  The arguments are checked
 * before the handle.  TFX_EINVAL: NULL `out`, n_frames < 1, px outside TFX_FRAME_PX_MIN .. TFX_FRAME_PX_MAX, unknown
 * flag bits, a NULL handle, n_frames > E with env_ids NULL, a frame of 2^31 pixels or more; TFX_ESTATE before
 * tfx_bind_buffers.  gym_traffic/devrng.py frames states the definition in NumPy, frame_geometry the roads' pixels. */
#define TFX_FRAME_PX_MIN 8
#define TFX_FRAME_PX_MAX 256
enum { TFX_FRAMES_ROADS_ONLY = 1 };
int tfx_frame_size(tfx_handle h, int32_t px, int32_t *height, int32_t *width);
int tfx_frames(tfx_handle h, const int32_t *env_ids, int32_t n_frames, int32_t px, uint8_t *out, int32_t flags,
               void *stream);
/* Test support: the launch geometry tfx_frames uses for this handle, n_frames and px - workgroups, and wavefronts (one
 * per (frame, tile) item at a time). */
int tfx_frames_launch(tfx_handle h, int32_t n_frames, int32_t px, int32_t *grid, int32_t *waves);
/* Travel times on the device.  Mean travel time is the headline figure of signal control and the one thing the
 * reference's validate mode prints (advance_hack, traffic_env.py:139-157).  Two read-only launches (k_ages, k_trips,
 * csrc/tfx_travel.hpp) give it with no host round trip: the ages of the cars still on the map, and the finished trips
 * reduced where they are logged.  Without them the route is a copy of the whole [E][trip_cap] log, and tfx_export_ring of
 * every ring slot for the spawn ticks - and a mean over finished trips alone flatters the policy that leaves its cars in
 * a jam.
 *
 * tfx_car_ages: how long every live car has been on the map.  Definition, as a function of the image tfx_export_ring
 * would produce at that moment, with the cars and the car order of tfx_road_measures.  `now` is the handle's device
 * clock, read on the device when the launch runs (the way tfx_clone_envs reads it): the value tfx_get_tick returns once
 * the stream has drained.  The age of a car is int32(side_age(now, side word)) (csrc/tfx_common.hpp) - TWICE the trip time
 * in seconds advance_hack would log if the car left the map in this tick:
 *   single-archetype handles   (int32)((float)now - w)               w: the spawn tick, a float
 *   heterogeneous handles      (now - spawn tick) & 0xFFFFFF          spawn ticks are kept modulo 2^24
 * Late clocks.  A single-archetype handle stores the spawn tick as a float32: (float)tick at the spawn, one rounding to
 * nearest even, and a logged trip time is ((float)pop tick - w) / 2 in float32.  While the clock is at most 2^24 both
 * are exact integers and ages and trip times are exact.  Beyond 2^24 they are the values of these formulas and no more:
 * between 2^24 and 2^25 ticks are kept to the even ones, up to 2^26 to multiples of 4, ... and of 128 at the top of the
 * clock's domain; an age or a doubled trip time is then off by up to that step.  Heterogeneous handles keep integers
 * modulo 2^24 and are exact at any clock of the domain for trips (and ages) shorter than 2^24 ticks.  Rebasing
 * (tfx_clone_envs, tfx_put_cars' spawn_shift) gives a single-archetype spawn tick (float)(w + dt), rounded once.
 * Per road:
 *   n_cars    the cars on the road, what tfx_cars_on_roads returns
 *   age_sum   the int64 sum of their ages
 *   age_max   the largest of their ages, 0 on an empty road
 * Integer arithmetic: order-free, the same bits on both layouts and from a host loop (gym_traffic/devrng.py car_ages).
 * Outputs are device pointers, [E][R] by the reference's road id; any may be NULL, at least one must not be.  Without
 * TFX_TRAVEL_ACCUMULATE every bound output is overwritten; with it n_cars and age_sum are added to and age_max is maxed.
 *
 * One launch on `stream`, no host synchronisation; nothing in the handle or in the caller's bound state is written:
 * captured step / agent-step graphs stay valid, and tfx_debug_fail_after does not count the launch.  TFX_MEASURE_GRID and
 * TFX_GRID_CAP cap the launch as they cap the measures'.  TFX_EINVAL: a NULL `out`, a NULL handle, all three pointers
 * NULL, unknown flag bits; TFX_ESTATE before tfx_bind_buffers, or on a handle that carries no side plane (planes == 2).
 * A refused call launches nothing. */
typedef struct tfx_age_buffers {
  int32_t *n_cars;     /* [E][R] by road id; may be NULL */
  int64_t *age_sum;
  int32_t *age_max;
} tfx_age_buffers;
enum { TFX_TRAVEL_ACCUMULATE = 1 };
int tfx_car_ages(tfx_handle h, const tfx_age_buffers *out, int32_t flags, void *stream);
/* Test support: the launch geometry tfx_car_ages uses for this handle - workgroups, and wavefronts (one per (env, tile)
 * item at a time), like tfx_measure_launch. */
int tfx_ages_launch(tfx_handle h, int32_t *grid, int32_t *waves);
/* tfx_trip_stats: the finished trips of every env, reduced on the device.  Needs a validate handle with trip_times and
 * n_trips bound.  edges: a HOST array of n_bins + 1 non-decreasing int32 values in ticks, copied into the kernel's
 * arguments; n_bins is 1..32.  cursor: a DEVICE int32 [E] the caller owns, or NULL.  Outputs: device pointers, [E], hist
 * [E][n_bins]; any may be NULL, at least one must not be; with hist NULL, edges may be NULL and n_bins 0.
 *
 * Rule, for env e, with cap = trip_cap:
 *   n = n_trips[e];  c = cursor[e] if cursor is given and 0 <= cursor[e] <= n, else 0 (a log shorter than its cursor was
 *   cleared by a reset or a restart: it is read from the start)
 *   the entries taken are i in [min(c, cap), min(n, cap)); entry i counts t_i = (int32)(trip_times[e][i] * 2.0f) ticks -
 *   exact, the log holds age / 2.0f of an integer age
 *   count     the number of entries taken
 *   tick_sum  the int64 sum of t_i (seconds: / 2, as the reference has them)
 *   tick_max  their maximum, 0 if none were taken
 *   lost      max(n, cap) - max(c, cap): the trips that happened but fell off the end of the log
 *   hist[b]   the number of i with edges[b] <= t_i < edges[b + 1] (equal neighbours: an empty bin)
 *   afterwards, if cursor is given, cursor[e] = n
 * Without TFX_TRAVEL_ACCUMULATE the outputs are overwritten; with it sums and counts are added to and tick_max is maxed.
 * Everything is integer, so nothing depends on the order.  gym_traffic/devrng.py trip_stats states the rule in NumPy.
 *
 * The rule cannot see one case: a log that was cleared and then grew back past the old cursor before the next call looks
 * like a log that only grew.  The caller zeroes the cursor of the envs it resets (TrafficVecEnv.travel_times does).
 *
 * One launch on `stream`, no host synchronisation; nothing in the handle or in its bound state is written (the cursor and
 * the outputs are the caller's): captured graphs stay valid, tfx_debug_fail_after does not count the launch.  TFX_EINVAL:
 * a NULL `out`, a NULL handle, all outputs NULL, unknown flag bits, n_bins out of range, hist given without edges, edges
 * that decrease; TFX_ESTATE before tfx_bind_buffers, or on a handle that is not in validate mode.  A refused call
 * launches nothing. */
typedef struct tfx_trip_stat_buffers {
  int32_t *count;      /* [E]; may be NULL */
  int64_t *tick_sum;
  int32_t *tick_max;
  int32_t *lost;
  int32_t *hist;       /* [E][n_bins]; may be NULL */
} tfx_trip_stat_buffers;
int tfx_trip_stats(tfx_handle h, const int32_t *edges, int32_t n_bins, int32_t *cursor, const tfx_trip_stat_buffers *out,
                   int32_t flags, void *stream);
/* Car-following measures on the device: what relates a car to its leader - net gaps, time headways, closing speeds with
 * time to collision (TTC) and the deceleration rate to avoid a crash (DRAC), platoon joins, overlaps - as eleven words per
 * road, from one read-only pass over the live cars (k_follow, csrc/tfx_follow.hpp).  The surrogate safety figures of a
 * signal policy, platoon counts per approach, what a loop detector measures as headways, and a counter of followers the
 * Jacobi IDM update pushed past their leader's rear bumper.  The reference has no counterpart; without this call the
 * route is tfx_export_ring of every ring slot and array code over the image.
 *
 * Definition, as a function of the image tfx_export_ring would produce at that moment (on a ring-layout handle: of xv
 * itself), so it is defined in every state a handle can be in, as the measures are.  For road e of env k take its cars in
 * order from the head, j = 0 .. n-1: car j sits in ring slot wrap(leading + 1 + j), n is the count tfx_cars_on_roads
 * returns; the fake leader is not a car.  Car j >= 1 forms a PAIR with its leader, car j-1 (F: the follower j, L: the
 * leader).  The head car forms none: its leader is the light or a car of the next road - a stop-line or cross-road pair
 * is out of scope of this call.  All arithmetic is float32, every operation rounded once in the order written, never
 * contracted, divisions correctly rounded:
 *   in range    the follower's x >= x_from (x_from = -INFINITY: every car; a NaN x is out of range); n_cars tests the
 *               head car the same way.  A leader out of range still leads.
 *   g           (x_L - x_F) - l_L: the net gap in IDM's own expression order (traffic_env.py:55).  l_L is the LEADER's
 *               length: car_l, or on heterogeneous handles the l of the table row in the leader's side word
 *   dv          v_F - v_L: the closing speed
 * Per road, every counter counting pairs in range only:
 *   n_cars      cars in range (tfx_road_measures' n_cars for the same x_from)
 *   n_pairs     pairs in range
 *   n_joined    pairs with g <= platoon_gap: the platoons on the road are n_cars - n_joined
 *   n_overlap   pairs with g < 0
 *   gap_sum     s = 0.0f, then s = s + g pair by pair in ascending j
 *   gap_min     m = +INFINITY, then m = g < m ? g : m (a NaN g is never taken)
 *   n_hw        pairs with v_F >= v_min
 *   hw_sum      s = 0.0f, then s = s + g / v_F over those pairs in ascending j: the sum of the time headways
 *   n_conflict  pairs with dv > 0 && g > 0 && g / dv < ttc_crit
 *   ttc_min     m = +INFINITY, then m = t < m ? t : m over t = g / dv of the pairs with dv > 0 && g > 0
 *   drac_max    m = 0.0f, then m = a > m ? a : m over a = (dv * dv) / (g + g) of the same pairs
 * Minima and maxima are comparisons and selects, so a NaN is never taken.  A road without such pairs gets 0 / +INFINITY /
 * 0 as its sums / minima / maximum.
 *
 * Outputs are device pointers, [E][R] by the reference's road id; any may be NULL, at least one must not be.  Without
 * TFX_FOLLOW_ACCUMULATE every bound output is overwritten.  With it: integers add; each float sum takes ONE float32 add
 * of the road's value (out = out + value); gap_min and ttc_min become value < out ? value : out; drac_max becomes value >
 * out ? value : out.  The caller initialises an accumulating buffer: 0 for the counters, the sums and drac_max, +INFINITY
 * for gap_min and ttc_min.
 *
 * One launch on `stream`, no host synchronisation; nothing in the handle or in the caller's bound state is written:
 * captured step / agent-step graphs stay valid, and tfx_debug_fail_after does not count the launch.  TFX_MEASURE_GRID and
 * TFX_GRID_CAP cap the launch as they cap the measures'.  TFX_EINVAL: a NULL handle, a NULL `p` or `out`, all eleven
 * pointers NULL, unknown flag bits, a NaN in any field of `p` (infinities are fine), v_min <= 0 (the headway is never a
 * division by zero); TFX_ESTATE before tfx_bind_buffers.  A refused call launches nothing.  gym_traffic/devrng.py
 * road_following states the definition in NumPy. */
typedef struct tfx_follow_params {
  float x_from;        /* followers (and, for n_cars, cars) with x >= x_from are in range */
  float platoon_gap;   /* g <= platoon_gap: the follower belongs to its leader's platoon */
  float v_min;         /* > 0: slower followers have no time headway */
  float ttc_crit;      /* g / dv < ttc_crit: a conflict */
} tfx_follow_params;
typedef struct tfx_follow_buffers {
  int32_t *n_cars;     /* [E][R] by road id; any may be NULL */
  int32_t *n_pairs;
  int32_t *n_joined;
  int32_t *n_overlap;
  float *gap_sum;
  float *gap_min;
  int32_t *n_hw;
  float *hw_sum;
  int32_t *n_conflict;
  float *ttc_min;
  float *drac_max;
} tfx_follow_buffers;
enum { TFX_FOLLOW_ACCUMULATE = 1 };
int tfx_road_following(tfx_handle h, const tfx_follow_params *p, const tfx_follow_buffers *out, int32_t flags,
                       void *stream);
/* Test support: the launch geometry tfx_road_following uses for this handle - workgroups, and wavefronts (one per
 * (env, tile) item at a time), like tfx_measure_launch. */
int tfx_follow_launch(tfx_handle h, int32_t *grid, int32_t *waves);
/* Road ends on the device: the first K cars at every stop line and the last car of every road, from one read-only launch
 * (k_ends, csrc/tfx_ends.hpp).  Every other road call reduces a road to a few numbers; this one hands out the cars
 * themselves, where a policy looks: the nearest vehicles of an approach as (distance to the stop line, speed) - what an
 * attention-style or an actuated signal controller reads - and where the last car of a road stands, which is the room
 * left at its entrance.  The head car against the stop line and against the last car of the road it drives into are the
 * pairs tfx_road_following leaves out.  The launch reads at most K + 2 rows of a tile and one more for the tails, whatever
 * the density.  Without this call the route is tfx_export_ring of every ring slot.
 *
 * Definition, as a function of the image tfx_export_ring would produce at that moment (on a ring-layout handle: of xv
 * itself): between two-tick passes, after a clone, between tfx_move_cars and tfx_advance_finished_cars.  For road e of env
 * k: n = ring_count(leading, lastcar) clamped to 0 .. C-1, what tfx_cars_on_roads returns; car j (0 <= j < n) sits in ring
 * slot wrap(leading + 1 + j).  Cars are listed in ring order, head first, as exported - NOT sorted by x: an unsorted ring
 * and a car past the road end give what their slots hold.  With k = K in 1 .. TFX_MAX_HEADS:
 *   n_cars     int32 [E][R]         n
 *   n_heads    int32 [E][R]         min(n, K)
 *   heads      float32 [E][R][K][2] entry j < min(n, K): (length - x_j, v_j) - ONE float32 subtraction from
 *                                   tfx_config.length, negative for a car past the road end; the others (pad_dist, pad_v)
 *   head_rows  uint8 [E][R][K]      the archetype row of car j (the low 6 bits of its side word's integer bits) on
 *                                   heterogeneous handles, 0 on single-archetype handles; TFX_ENDS_NO_CAR in padded entries
 *   tail       float32 [E][R][2]    (x, v) of car n - 1; (pad_tail_x, pad_v) on an empty road
 *   tail_row   uint8 [E][R]         the row of car n - 1, TFX_ENDS_NO_CAR on an empty road
 * All by the reference's road id, over all R roads.  The pads may be any float32, infinities and NaN included: they are
 * stored bit for bit.  Outputs are device pointers (heads and tail 8-byte aligned); any may be NULL and is then skipped.
 * Lists do not add: there is no accumulate form, flags must be 0.  Ages of the listed cars (tfx_car_ages has the per-road
 * figures), a range filter (callers mask by distance) and sorting by x are out of scope.
 *
 * One launch on `stream`, no host synchronisation; nothing in the handle or in the caller's bound state is written:
 * captured step / agent-step graphs stay valid, and tfx_debug_fail_after does not count the launch.  TFX_MEASURE_GRID and
 * TFX_GRID_CAP cap the launch as they cap the measures'.  TFX_EINVAL: a NULL handle, a NULL `p` or `out`, k outside
 * 1 .. TFX_MAX_HEADS, flags other than 0; TFX_ESTATE before tfx_bind_buffers.  A refused call launches nothing.
 * gym_traffic/devrng.py road_ends states the definition in NumPy. */
#define TFX_MAX_HEADS 16
#define TFX_ENDS_NO_CAR 255
typedef struct tfx_ends_params {
  int32_t k;           /* cars listed from the head of every road, 1 .. TFX_MAX_HEADS */
  float pad_dist;      /* distance of a padded heads entry */
  float pad_v;         /* speed of a padded heads entry and of the tail of an empty road */
  float pad_tail_x;    /* x of the tail of an empty road */
} tfx_ends_params;
typedef struct tfx_ends_buffers {
  int32_t *n_cars;     /* [E][R] by road id; any may be NULL */
  int32_t *n_heads;
  float *heads;        /* [E][R][k][2] */
  uint8_t *head_rows;  /* [E][R][k] */
  float *tail;         /* [E][R][2] */
  uint8_t *tail_row;   /* [E][R] */
} tfx_ends_buffers;
int tfx_road_ends(tfx_handle h, const tfx_ends_params *p, const tfx_ends_buffers *out, int32_t flags, void *stream);
/* Test support: the launch geometry tfx_road_ends uses for this handle and k - workgroups, and wavefronts (one per
 * (env, tile) item at a time), like tfx_follow_launch. */
int tfx_ends_launch(tfx_handle h, int32_t k, int32_t *grid, int32_t *waves);
/* Car lists on the device: every live car of chosen envs as one flat run, from one read-only launch (k_cars,
 * csrc/tfx_cars.hpp).  The other road calls reduce a road to a few numbers and tfx_road_ends hands out at most
 * TFX_MAX_HEADS cars a road; this one hands out all of them, compacted: floating-car data of a few envs per tick, a ragged
 * (CSR) list for a vehicle-level policy, or chosen envs of a big batch without a whole-batch tfx_export_ring.
 *
 * Definition, as a function of the image tfx_export_ring would produce at that moment (on a ring-layout handle: of xv
 * itself): between two-tick passes, after a clone, between tfx_move_cars and tfx_advance_finished_cars.
 *   Selection  env_ids holds n_sel env numbers (NULL: selection s is env s, n_sel <= E); repeats are allowed; an id outside
 *              [0, E) contributes no cars.
 *   Road filter road_mask is uint8 [R] by road id or NULL; a road whose byte is 0 contributes no cars.
 *   Counts     count[s][e] = ring_count(leading, lastcar) of road e of env env_ids[s] clamped to 0 .. C-1 - what
 *              tfx_cars_on_roads returns - and 0 for masked-out roads and for envs that are not shown.
 *   Offsets    int32 [n_sel * R + 1]: the exclusive prefix sum of the counts in (s, road id) order; offsets[n_sel * R] is
 *              the total N.  The CALLER computes them (the prefix sum of the tfx_cars_on_roads counts of the chosen envs,
 *              zeroed where masked or not shown) and passes them in; the library launches no scan.
 *   Order      car j from the head of (s, e), in ring order (slot wrap(leading + 1 + j); NOT sorted by x), has index
 *              i = offsets[s * R + e] + j.
 *   Planes, for every i < min(N, cap):
 *     xv     float32 [cap][2]  (x, v) of the car, moved bit for bit
 *     road   int32 [cap]       s * R + e
 *     row    uint8 [cap]       the car's archetype row; 0 on single-archetype handles
 *     spawn  float32 [cap]     the car's spawn tick exactly as tfx_export_ring gives it in ring_w; handles with
 *                              planes == 3 only
 *   Entries at i >= min(N, cap) are never written.  There is no arithmetic: everything is reproducible byte for byte.
 * Any plane may be NULL and is then skipped (xv 8-byte aligned).  Memory safety does not depend on the offsets: entry j of
 * key k = s * R + e is stored only if j < offsets[k + 1] - offsets[k] and offsets[k] + j lies in [0, cap), so offsets that
 * do not match the counts lose or overlap cars but never send a store outside the planes.
 *
 * One launch on `stream`, no host synchronisation; nothing in the handle or in the caller's bound state is written:
 * captured step / agent-step graphs stay valid, and tfx_debug_fail_after does not count the launch.  TFX_MEASURE_GRID and
 * TFX_GRID_CAP cap the launch as they cap the measures'.  TFX_EINVAL: a NULL handle, `out` or `offsets`, n_sel <= 0,
 * n_sel > E with env_ids NULL, n_sel * R + 1 beyond int32, cap < 0, flags other than 0, `spawn` on a planes == 2 handle;
 * TFX_ESTATE before tfx_bind_buffers.  cap == 0 is a valid call that launches nothing, as does a refused call.
 * gym_traffic/devrng.py car_list states the definition in NumPy. */
typedef struct { float *xv; int32_t *road; uint8_t *row; float *spawn; } tfx_car_list_buffers;  /* any member NULL: skipped */
int tfx_car_list(tfx_handle h, const int32_t *env_ids /*device, NULL: all*/, int32_t n_sel, const uint8_t *road_mask /*device [R] or NULL*/,
                 const int32_t *offsets /*device [n_sel*R+1]*/, int32_t cap, const tfx_car_list_buffers *out, int32_t flags, void *stream);
/* Test support: the launch geometry tfx_car_list uses for this handle and n_sel chosen envs - workgroups, and wavefronts
 * (one per (selected env, tile) item at a time), like tfx_frames_launch. */
int tfx_car_list_launch(tfx_handle h, int32_t n_sel, int32_t *grid, int32_t *waves);
/* Car lists back in: the cars of chosen envs written from one flat run, in one launch (k_put, csrc/tfx_put.hpp) - the
 * inverse of tfx_car_list.  Edit a list and write it back, restart chosen envs from a library of lists, move envs between
 * batches of another E or capacity: a list is plain data, a handle is not.
 *
 * Definition, on the image tfx_export_ring would produce afterwards (on a ring-layout handle: xv itself), for every
 * selection s whose env = env_ids[s] lies in [0, E) (NULL: selection s is env s, n_sel <= E) and every road e whose
 * road_mask byte is non-zero (NULL: every road), with key = s * R + e:
 *   Run        base = offsets[key], run = max(0, offsets[key + 1] - base); the entries offered are those of
 *              [base, base + run) that lie in [0, cap): first = max(base, 0), fit = max(0, min(base + run, cap) - first).
 *   Count      the road afterwards holds n = min(fit, C - 2) cars - a ring of C - 1 slots, one of them the leader's, holds
 *              no more (with C - 1 the ring words would read as an empty road); on the transposed layout also n <= the
 *              tile's rows.  tfx_cars_on_roads then returns n.
 *   Cars       car j < n from the head is entry first + j of the planes: (x, v) moved bit for bit; the side word built as
 *              tfx_import_ring builds it from (spawn, row) - on planes == 2 handles spawn is ignored - with spawn_shift
 *              added to every spawn tick as tfx_clone_envs adds the difference of two clocks (a list recorded at another
 *              clock is rebased; on heterogeneous handles modulo 2^24).
 *   Ring words leading' = leading[key] where that is a ring index of this handle (1 .. C-1), otherwise - or with
 *              `leading` NULL - the road's current one; lastcar' = the slot of car n - 1 (leading' + n under the ring's
 *              wrap), leading' itself when n == 0.  Slot leading' shows lead_x[key] (NULL: +INFINITY, what a reset writes).
 *              The value is for the image only: the next tick's light update rewrites it on every road that has a light,
 *              and on exit roads the model's leader is +INFINITY always - pass that there.
 *   Lost       the first n cars offered are taken; run - n is added to *lost (device, may be NULL) with one atomicAdd per
 *              road that loses cars, and nothing else happens.
 *   Untouched  roads that are masked out, envs that are not selected and selections whose id lies outside [0, E) keep their
 *              cars, ring words and caches bit for bit.  Slots or rows of a written road that hold no car afterwards are
 *              unspecified.
 *   Caches     the launch writes every per-road word tfx_import_ring followed by tfx_refresh would leave for the road - the
 *              row offset of the two-tick pass (0), the leader's x, the tail caches with tfx_refresh's values, empty roads
 *              and the ring layout included - so no tfx_refresh is needed.  Everything else the handle keeps (records,
 *              stamps, graphs) is left alone: by "What the next call depends on" above such residue never changes a result.
 * env_ids must be distinct.  With repeats the launch is still memory-safe and the env's ring words stay ring indices, but
 * which of the offered runs a road's words and car rows come from is unspecified.  Memory safety does not depend on the
 * offsets: entry i of a plane is read only if 0 <= i < cap, and stores go to the selected envs' own columns and words only.
 *
 * One launch on `stream`, no host synchronisation; no pointer changes, so captured step / agent-step graphs stay valid;
 * tfx_debug_fail_after does not count the launch and TFX_GRID_CAP caps it.  The call belongs between whole ticks: between
 * tfx_move_cars and tfx_advance_finished_cars the outbox of a written road is stale and the advance would hand on cars
 * that are no longer there - the handle does not track that state, so this is the caller's rule, not an error code.
 * TFX_EINVAL: a NULL handle, `in`, `in->xv` or `offsets`, n_sel <= 0, n_sel > E with env_ids NULL, n_sel * R + 1 beyond
 * int32, cap < 0, flags other than 0; TFX_ESTATE before tfx_bind_buffers.  cap == 0 is valid and empties the selected
 * roads.  gym_traffic/devrng.py put_cars states the definition in NumPy. */
typedef struct {
  const float   *xv;      /* [cap][2] (x, v); required */
  const uint8_t *row;     /* [cap] archetype row; NULL: row 0 */
  const float   *spawn;   /* [cap] spawn tick as tfx_car_list / ring_w give it; NULL: 0 */
  const int32_t *leading; /* [n_sel*R] new `leading` per (selection, road); NULL or a value that is no valid ring index of this handle: the road keeps its current one */
  const float   *lead_x;  /* [n_sel*R] the x the image shows in slot `leading`; NULL: +INFINITY (what a reset writes) */
} tfx_put_buffers;
int tfx_put_cars(tfx_handle h, const int32_t *env_ids /*device, NULL: selection s is env s*/, int32_t n_sel,
                 const uint8_t *road_mask /*device [R] or NULL*/, const int32_t *offsets /*device [n_sel*R+1]*/,
                 int32_t cap, const tfx_put_buffers *in, int32_t spawn_shift, uint64_t *lost /*device, may be NULL*/,
                 int32_t flags, void *stream);
/* Test support: the launch geometry tfx_put_cars uses for this handle and n_sel chosen envs, like tfx_car_list_launch. */
int tfx_put_launch(tfx_handle h, int32_t n_sel, int32_t *grid, int32_t *waves);
/* State digests on the device: a 64-bit fingerprint per chosen env, and optionally one per road, from one read-only
 * launch over the live cars (k_digest, csrc/tfx_digest.hpp).  "Are these two env states the same bits?" as 8 bytes per
 * env: a check of what tfx_clone_envs, tfx_put_cars or a sharded run claim, for every env at once; a transposition key
 * for tree search.  A FINGERPRINT, NOT A CRYPTOGRAPHIC HASH: equal states always give equal digests; unequal states give
 * different digests except by accident (about 2^-64 per pair of unrelated states), and an adversary can construct
 * collisions.
 *
 * Definition, integer arithmetic only, on the image tfx_export_ring would produce at that moment (on a ring-layout handle:
 * on xv itself) and on the bound buffers - so it is also defined between two-tick passes, after a clone, between
 * tfx_move_cars and tfx_advance_finished_cars, and it is equal across layouts, shardings and handles.  All arithmetic is
 * uint64 modulo 2^64.
 *   mix(z)     the splitmix64 finaliser, in this order: z ^= z >> 30; z *= 0xbf58476d1ce4e5b9; z ^= z >> 27;
 *              z *= 0x94d049bb133111eb; z ^= z >> 31.
 *   G          0x9e3779b97f4a7c15.
 *   Parts      `parts` is a non-zero sum of the TFX_DIGEST_* bits below and nothing else:
 *     CARS   = 1   the count and every car's (x, v) bit patterns
 *     ROWS   = 2   every car's archetype row, as tfx_car_list gives `row` (0 on single-archetype handles)
 *     SPAWN  = 4   every car's spawn tick: the bit pattern of the float tfx_car_list gives in `spawn`; handles with
 *                  planes == 3 only, else TFX_EINVAL
 *     RING   = 8   `leading` of every road (the wrapped-ring branch of the model makes the ring position part of what
 *                  the next tick depends on)
 *     LIGHTS = 16  current_phase[I] and elapsed[I] from obs
 *     OBS    = 32  passed[r], detected[r], waiting[r], passed_dst[I], the bit patterns of rewards[I], done_tick
 *   Selection  env_ids holds n_sel env numbers (NULL: selection s is env s, n_sel <= E); repeats are allowed.
 *   Per road   For road e of a shown env whose road_mask byte is non-zero (NULL: every road), with n the count as
 *              tfx_cars_on_roads clamps it and car j the j-th from the head in ring order - tfx_car_list's order:
 *                A_j = xbits | vbits << 32,   B_j = spawnbits | row << 32   (a half of B_j is 0 where its part is off)
 *                road = mix(1 + n)
 *                     + [RING]           mix((2 << 56) | leading)
 *                     + [CARS]           sum over j of mix(A_j + (2j + 1) * G)
 *                     + [ROWS or SPAWN]  sum over j of mix(B_j + (2j + 2) * G)
 *              With none of CARS, ROWS, SPAWN and RING set no road term enters the env digest at all, road_digest is 0
 *              and no car row is loaded.  Float bit patterns are hashed as they are: -0.0 differs from 0.0, NaNs differ
 *              by payload.
 *   Per word   Sections s = 1 current_phase, 2 elapsed (LIGHTS), 3 passed, 4 detected, 5 waiting, 6 passed_dst,
 *              7 rewards, 8 done_tick (OBS): index i and 32-bit value val give mix((s << 56) | (i << 32) | val); a uint8
 *              is zero-extended, an int32 or a float contributes its bit pattern.
 *   Per env    env = sum over the unmasked roads e of mix(road_e + (e + 1) * G) + the word terms of the chosen sections.
 *              road_digest[s][e] = road_e, 0 for masked-out roads.  A selection whose id lies outside [0, E) has env = 0
 *              and every road_digest = 0; nothing of the handle's state is read for it.
 * Every combination is a sum, so any evaluation order gives the same bits.  Spawn ticks are clock-relative: compare envs
 * taken at different clocks without SPAWN (done_tick, inside OBS, is a clock stamp too where it is not 0).  What only the
 * handle owns - caches, arrival-stream positions, episode accounting - is not caller-visible state and is not hashed.
 *
 * One memset of env_digest and one launch on `stream`, no host synchronisation; nothing in the handle or in the caller's
 * bound state is written: captured step / agent-step graphs stay valid, and tfx_debug_fail_after does not count the
 * launch.  TFX_MEASURE_GRID and TFX_GRID_CAP cap the launch as they cap the measures'.  TFX_EINVAL: a NULL handle or
 * env_digest, n_sel <= 0, n_sel > E with env_ids NULL, n_sel * R beyond int32, parts 0 or with unknown bits, SPAWN on a
 * planes == 2 handle, flags other than 0; TFX_ESTATE before tfx_bind_buffers.  A refused call launches nothing.
 * gym_traffic/devrng.py state_digest states the definition in NumPy. */
#define TFX_DIGEST_CARS 1
#define TFX_DIGEST_ROWS 2
#define TFX_DIGEST_SPAWN 4
#define TFX_DIGEST_RING 8
#define TFX_DIGEST_LIGHTS 16
#define TFX_DIGEST_OBS 32
int tfx_state_digest(tfx_handle h, const int32_t *env_ids /*device, NULL: selection s is env s*/, int32_t n_sel,
                     const uint8_t *road_mask /*device [R] or NULL*/, int32_t parts,
                     uint64_t *env_digest /*device [n_sel], required*/, uint64_t *road_digest /*device [n_sel][R] or NULL*/,
                     int32_t flags /*0*/, void *stream);
/* Test support: the launch geometry tfx_state_digest uses for this handle and n_sel chosen envs, like tfx_car_list_launch. */
int tfx_digest_launch(tfx_handle h, int32_t n_sel, int32_t *grid, int32_t *waves);
/* Test support: out (HOST uint8 [E][R]) receives, per road, the rows at the top of its column that hold no car - what a
 * two-tick pass leaves between calls on the transposed layout (0 everywhere on the ring layout).  Synchronises the stream. */
int tfx_debug_head_rows(tfx_handle h, uint8_t *out, void *stream);

/* Host-side replay of the reference's seeded arrival generators for many envs (no GPU involved): one
 * stream per env holds a legacy numpy RandomState's MT19937 state (`RandomState.get_state()[1:3]`)
 * plus the generator's own state - `gap`: whole ticks left before the next Poisson car (-1 = draw a
 * new gap), `tick`: the regular generator's tick counter.  tfx_arrivals_replay advances every stream
 * by n_ticks exactly as traffic_env.py:160-176 + :274-283 would (poisson != 0: round(Exp(mean_gap))
 * empty ticks between cars; else `burst` cars every `every` ticks), drawing each car's entry road
 * with rand.choice over n_choices entry points.  counts int32 [n_ticks][n_streams][n_columns] receives
 * the cars per entry road (choice c -> column column_of_choice[c]), made int32 [n_ticks][n_streams]
 * (may be NULL) the cars created.
 *
 * tfx_arrivals_replay_rows is the same replay for a table of n_archetypes rows (1..TFX_MAX_ARCH): every Poisson car
 * draws randint(n_archetypes) where SpawnSchedule._poisson_tick does (after its gap, before its entry road; nothing is
 * drawn for one row), the regular generator draws no row (archetypes[0], traffic_env.py:174).  rows uint8
 * [n_ticks][n_streams][n_columns][S] receives the row of the j-th car of each column in the tick, in creation order,
 * for j < S (the bytes past a column's cars are left as they were); with n_archetypes = 1 the counts, made and the
 * streams' final states are those of tfx_arrivals_replay. */
typedef struct tfx_arrival_stream {
  uint32_t mt[624];
  int32_t pos;
  int32_t gap;
  int64_t tick;
} tfx_arrival_stream;
int tfx_arrivals_replay(tfx_arrival_stream *streams, int32_t n_streams, int32_t n_ticks, int32_t poisson,
                        double mean_gap, int32_t every, int32_t burst, int32_t n_choices,
                        const int32_t *column_of_choice, int32_t n_columns, int32_t *counts, int32_t *made);
int tfx_arrivals_replay_rows(tfx_arrival_stream *streams, int32_t n_streams, int32_t n_ticks, int32_t poisson,
                             double mean_gap, int32_t every, int32_t burst, int32_t n_choices,
                             const int32_t *column_of_choice, int32_t n_columns, int32_t *counts, int32_t *made,
                             int32_t n_archetypes, int32_t S, uint8_t *rows);

#ifdef __cplusplus
}
#endif
#endif /* TFX_H */
