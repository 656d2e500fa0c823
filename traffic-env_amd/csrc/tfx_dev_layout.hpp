// tfx_dev_layout.hpp - the parameter blocks every kernel takes by value (Dev, EpDev) and the ONE description of the
// device arrays behind a Dev, as host arithmetic: for_each_env_array names every array that holds something per env -
// sub_dev (the halves of a split call, run_ticks) and graph_key's pointer lists (tfx_hip.hip) are written on it;
// carve_arena names every region of the handle's scratch arena once, to size the arena and to bind its pointers
// (tfx_create).  Nothing here is device code, dereferences a device pointer or needs a device: tfx_common.hpp adds the
// arithmetic the kernels share, tests/dev_layout_check.cpp checks the tables on the host alone.
#pragma once
#include <hip/hip_vector_types.h>

#include <cstddef>
#include <cstdint>
#include <type_traits>

#include "tfx.h"

namespace tfx {

constexpr int KP = TFX_KP;
// The vehicle-update counter is spread over VEH_SLOTS words, one cache line apart (veh_add, tfx_common.hpp)
constexpr int VEH_SLOTS = 256, VEH_STRIDE = 8;

// Everything a kernel needs, passed by value.
struct Dev {
  int I, r, R, C, E, n_entry, obs_len;
  int yellow, learn_switch, validate, env_off;
  // fused agent step (Repeater + Remi, traffic_test.py:27-64): `passed` (and, without Remi, the
  // rewards) accumulate over the ticks of the step; an env that overflowed in an earlier tick of
  // the step stands still for the rest of it (`if done: break`, traffic_test.py:55)
  int agent_mode, accum_rewards;
  const int *agent_first;  // tick at which the current agent step began
  float length, rate, car_v, car_l, car_a, car_v0, car_b, car_T, car_s0;
  float risk_a;                  // the largest acceleration any car can have (k_risk's movement bound): car_a, or the table's maximum
  float two_sab, eps, thresh, near_end, ovf_pen;
  float r_two_sab, r_v0;  // correctly rounded reciprocals of the two constant divisors
  int fastdiv;            // the reciprocal form of those divisions was verified exact (div_selftest)
  int fastmax;            // v_max_f32 orders +0 above -0 in either operand order (k_max_selftest)
  // caller-owned state
  float2 *xv;  // [E][R][C] (x, v) per ring slot
  float *w;    // [E][R][C] spawn tick per ring slot, or nullptr
  int *leading, *lastcar, *obs;
  // phase | elapsed of env k's intersections: lights + k * lights_stride (= obs + 2r, obs_len: the words inside obs
  // - or a workgroup's LDS copy with stride 0, k_tail)
  int *lights;
  int lights_stride;
  float *rewards;
  int *waiting;
  uint8_t *passed_dst;
  int *done_tick;
  float *trip_times;
  int *n_trips;
  int trip_cap;
  // handle-owned tables + scratch
  const int *nexts, *pred, *entry_idx;
  // transposed layout: road e of an env lives in storage slot road_slot[e] (tile = slot / 64, lane =
  // slot % 64, G tiles per env); slot_road is the inverse (-1 = padding lane)
  const int *road_slot, *slot_road;
  int G;
  int trows;  // rows (of 64 (x, v) pairs) a tile occupies in T: >= C - 2
  int4 *rec;      // per road: {pops k | head slot << 16, spawn overflows | uncompacted << 30, bits of post-move tail x, live cars}
  // transposed layout: rows at the top of a road's column that hold no car (0..TFX_KP; see rec_hb) - a byte per road
  // of its own since round 4: the pass reads one byte instead of a 16-byte record, k_tail writes one back
  uint8_t *hb;
  // k_tail<AGENT> only (LDS): 0 = the road's head cannot reach the road's end in the next tick - what edge_tile saw while
  // it held the head's new state - so that the bound for the next pair (risk_lane) need not load the road's first rows
  uint8_t *riskhint;
  // "road state word": leading | lastcar << 9 | hb << 18 of a road, 4 bytes.  Between the pairs of ONE tfx_step call
  // (plain cars, outside agent steps) k_tail writes this word instead of leading, lastcar and hb (9 bytes) and the next
  // pass reads it instead of them (its RSW form); the call's last k_tail brings the reference's arrays up to date, its
  // first pass reads those - nobody else looks at them in between.
  int *rsw;
  // per road, two-tick pass only (tfx_move_tt.hpp): what the pass hands to the edge work of the second tick, 12 bytes
  // (round 3: one 16-byte record): {v of the tail after the first tick, x of the tail after the second} and the
  // waiting (both ticks so far) | detected (second tick so far) | detected (first tick) counts (rec2c_pack)
  float2 *rec2f;
  int *rec2c;
  // A two-tick pass that k_tail follows (its CREC form) writes its road record in 8 bytes instead of rec's 16 - {packed
  // integers (crec_pack), bits of the tail's x} - and the count of spawn overflows, when there are any, to ovf_cnt; k_tail expands it into its LDS copy
  // of rec, so the phase code reads what it always read
  int2 *crec;
  int *ovf_cnt;
  // transposed layout only (tfx_config.layout = 1): xv is T[tile][k][64]; the first TFX_KP = 2 cars that
  // left a road this tick wait in its outbox column outb[tile][j][64], j < KP - a road that pops more
  // stays uncompacted for the tick and its env takes the serial advance; the fake leader's x has no
  // slot of its own and lives in leadx
  float2 *outb;
  float *outw;  // outbox of the spawn-tick plane (planes = 3)
  float *leadx;
  int layout;
  float *tailx;   // per road: x of the last car after the advance (what update_lights reads)
  int *env_flag;  // == tick+1 when the env must take the serial advance this tick
  // == tick+1 when the env takes the pair of ticks starting at `tick` one tick at a time (k_risk).  Two planes, used in
  // turn by the pairs of a call (risk_word): k_tail stamps the NEXT pair's plane while the launches behind it still read
  // the current pair's
  int *env_risk;
  int risk_stride;  // words from one plane to the other (the whole handle's E, also inside the half of a split call)
  int *risk_any;  // [2], one per plane of env_risk: == tick+1 when any env is marked for the pair starting at `tick`
  unsigned long long *veh;
  unsigned long long *slow_pairs;  // env-pairs of agent steps that k_tail took one tick at a time (tfx_slow_pairs)
  int *tickA, *tickB;
  // per-tick inputs
  const int *action;
  int action_mode, action_period;
  long action_stride;
  const int *spawn;
  int spawn_mode, spawn_period;
  long spawn_stride;
  // greedy controller (algorithms/greedy.py:14-16): > 0 = the advance of tick t writes the action of tick t + 1
  // whenever (t + 1) % greedy_spacing == 0
  int greedy_spacing;
  int *greedy_act;               // [E][I]
  // heterogeneous cars (tfx_config.n_archetypes): every car's side word w holds (spawn tick mod 2^24) << 6 | table row as integer bits
  int het;
  const float *arch_tab;         // [TFX_MAX_ARCH][ARCH_W]: l, a, v0, T, s0, 2 sqrt(a b), delta, spawn speed
  int *taila;                    // per road: table row of its last car (next to tailx)
  const uint8_t *spawn_arch;     // rows of the cars the count buffer adds: [tick][E][n_entry][spawn_arch_S]
  int spawn_arch_S;
  long spawn_arch_stride;
};

// Episodes on the device (tfx_set_episodes, include/tfx.h), a parameter block of its own: only the kernels that begin
// and end a decision (and k_reset) see it, every other kernel's arguments are what they were.  The caller's
// accumulators, and two bytes per env of the handle's own - mark: the env's last decision ended its episode (the next
// decision restarts it), last: the decision under way is the last one the time limit allows (k_episode_begin writes
// it, the decision's tail reads it: nothing in a tail reads a word another lane of the same launch writes).
struct EpDev {
  int on, max;
  unsigned seed_lo, seed_hi;
  float *ep_return, *final_return;
  int *ep_len, *final_len, *ep_index;
  uint8_t *trunc, *mark, *last;
};

// A new member of Dev does not compile until someone has decided what it is: an array with something per env (without
// a line in for_each_env_array the second half of a split call works on the first half's memory), a region of the
// scratch arena (carve_arena), both, or neither.  Then update the size.
static_assert(sizeof(Dev) == 584, "Dev changed: see for_each_env_array and carve_arena");

// whose an array is: the caller's through tfx_bind_buffers | a per-tick input a setter bound (the caller's, an arrival
// stream's, the greedy controller's) | a region of the handle's scratch arena
enum ArrayKind { ARR_BOUND, ARR_INPUT, ARR_SCRATCH };

// (x, v) pairs of an env's cars: T[tile][k][64] or [R][C]
inline size_t env_car_pairs(const Dev &d) {
  return d.layout == 1 ? (size_t)d.G * (size_t)d.trows * 64 : (size_t)d.R * (size_t)d.C;
}

// f(d.member, elements per env, kind) for every per-env array of d, in the modes d is in: env k's part of an array
// begins k * elements into it.  An array may be null.  (lights points into obs: env_lights.)
template <class D, class F>
void for_each_env_array(D &d, F f) {
  auto each = [&f](size_t per_env, ArrayKind kind, auto &...member) { (f(member, per_env, kind), ...); };
  const size_t R = (size_t)d.R, I = (size_t)d.I, n_entry = (size_t)d.n_entry, one = 1;
  each(env_car_pairs(d), ARR_BOUND, d.xv, d.w);
  each(R, ARR_BOUND, d.leading, d.lastcar);
  each((size_t)d.obs_len, ARR_BOUND, d.obs);
  each(I, ARR_BOUND, d.rewards, d.passed_dst);
  each((size_t)d.r, ARR_BOUND, d.waiting);
  each(one, ARR_BOUND, d.done_tick, d.n_trips);
  each((size_t)d.trip_cap, ARR_BOUND, d.trip_times);
  // (a broadcast action row and the other spawn rules hold nothing per env)
  if (d.action_mode == TFX_ACTION_BUFFER) each(I, ARR_INPUT, d.action);
  if (d.spawn_mode == TFX_SPAWN_COUNTS) each(n_entry, ARR_INPUT, d.spawn);
  each(n_entry * (size_t)d.spawn_arch_S, ARR_INPUT, d.spawn_arch);
  each(I, ARR_INPUT, d.greedy_act);
  each(R, ARR_SCRATCH, d.rec, d.rec2f, d.rec2c, d.crec, d.ovf_cnt, d.rsw, d.tailx, d.leadx, d.taila, d.hb);
  each((size_t)d.G * KP * 64, ARR_SCRATCH, d.outb, d.outw);
  each(one, ARR_SCRATCH, d.env_flag, d.env_risk);  // (env_risk: either plane - risk_stride stays the whole handle's E)
}

// phase | elapsed of an env's intersections are words inside its obs row
inline int *env_lights(const Dev &d) { return d.obs + 2 * d.r; }

// The envs [lo, lo + n) of a Dev as a Dev of their own: every per-env array starts at env lo (a null one stays null),
// the global env id offset moves along (on-device rules are functions of the global id), everything else - the
// vehicle-update counter too - is shared.  clock: the three clock words of a range that runs on a stream of its own.
inline Dev sub_dev(const Dev &whole, int lo, int n, int *clock) {
  Dev s = whole;
  s.E = n;
  s.env_off = whole.env_off + lo;
  for_each_env_array(s, [lo](auto *&p, size_t per_env, ArrayKind) { p = p ? p + (size_t)lo * per_env : p; });
  s.lights = env_lights(s);
  if (clock) {
    s.tickA = clock;
    s.tickB = clock + 1;
    s.risk_any = clock + 2;
  }
  return s;
}

// The small words of the scratch arena, the 64-bit ones first: 8-aligned in a 256-aligned region
struct MiscWords {
  unsigned long long selftest;       // k_div_selftest's and k_max_selftest's mismatch count (tfx_create; zero afterwards)
  unsigned long long slow_pairs;     // Dev::slow_pairs
  unsigned long long clone_skipped;  // envs tfx_clone_envs left untouched (tfx_clone_skipped)
  int tickA, tickB, agent_first, risk_any[2];
  int clock2[4];  // tickA, tickB, risk_any[2] of the second half of a split call (sub_dev's clock)
};

// The handle's scratch arena: every region named once - what points at it, its elements (none where its condition is
// false), whether the pointer is null then (kernels and sub_dev ask those) - in the arena's order, 256-aligned.  Returns
// the arena's bytes; base != nullptr: binds the regions, Dev's small words and risk_stride to an arena there as well.
// Besides Dev's own: the episode bytes (mark | last, one per env each: tfx_set_episodes), the device copy of the
// episode block, the small words.  (d.E, R, G, layout and het are set by then.)
inline size_t carve_arena(Dev &d, EpDev &ep, EpDev *&dev_ep, MiscWords *&misc, int planes, char *base) {
  size_t off = 0;
  auto region = [&](auto *&p, size_t count, bool null_if_empty = false) {
    using T = std::remove_pointer_t<std::remove_reference_t<decltype(p)>>;
    if (base) p = (null_if_empty && count == 0) ? nullptr : reinterpret_cast<T *>(base + off);
    off = (off + count * sizeof(T) + 255) / 256 * 256;
  };
  const size_t E = (size_t)d.E, ER = E * (size_t)d.R;
  const size_t T = d.layout == 1 ? 1 : 0;               // the transposed layout's own regions
  const size_t outbox = T * E * (size_t)d.G * KP * 64;  // TFX_KP rows per tile (the cars a road hands over in a tick)
  region(d.rec, ER);
  region(d.rec2f, T * ER);
  region(d.rec2c, T * ER);
  region(d.crec, T * ER, true);
  region(d.ovf_cnt, T * ER, true);
  region(d.rsw, T * ER, true);
  region(d.tailx, ER);
  region(d.env_flag, E);
  region(d.env_risk, 2 * E);  // two planes (risk_word)
  region(d.outb, outbox);
  region(d.outw, planes == 3 ? outbox : 0);
  region(d.leadx, ER);
  region(d.taila, d.het ? ER : 0);
  region(d.hb, T * ER, true);
  region(ep.mark, 2 * E);
  region(dev_ep, 1);
  region(misc, 1);
  region(d.veh, (size_t)VEH_SLOTS * VEH_STRIDE);
  if (!base) return off;
  ep.last = ep.mark + E;
  d.tickA = &misc->tickA;
  d.tickB = &misc->tickB;
  d.agent_first = &misc->agent_first;
  d.risk_any = misc->risk_any;
  d.slow_pairs = &misc->slow_pairs;
  d.risk_stride = d.E;
  return off;
}

}  // namespace tfx
