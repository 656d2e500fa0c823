// tfx_tile.hpp - the vocabulary of the tile walkers: what every device function that walks a tile of 64 roads, lane per
// road, on the transposed layout shares with the others - k_move_t (tfx_move_t.hpp), k_move_ts (tfx_move_ts.hpp),
// move_tt_tile / edge_tile / risk_lane (tfx_move_tt.hpp) and move_tt_tile_seg (tfx_move_tts.hpp); the read-only walk
// (tfx_walk.hpp) takes wave_max from here.  Device only, everything inlined.  The rule for using a piece: the walker keeps
// the registers, LDS, scratch and barriers it had with the piece written out (tools/kernel_regs.py is the check) - the
// passes sit close to their register lines, and a spelling that is the same arithmetic can move them.  Where one did,
// the site keeps its own copy and says so: the lane's road in k_move_ts, move_tt_tile and move_tt_tile_seg, the tile's
// longest road in move_tt_tile_seg, the heterogeneous arrivals in edge_tile, the one-tick outputs inside the two pair
// walkers (there interleaved with the pair's record).
//
// Several pieces are rules of the reference that must be bit-identical wherever they apply, and each stands here once:
//   * het_spawns: add_car (:97-114) car by car for heterogeneous cars;
//   * kq_of / count_car: the waiting count's wrapped-ring quirk (:210) and the `detected` test;
//   * idm_plain: the single-archetype IDM step under the wave-wide fast-division domain test;
//   * store_tick_outputs: what one tick of a road leaves behind for the advance and the observation.
#pragma once
#include "tfx_common.hpp"

namespace tfx {

typedef float f2v __attribute__((ext_vector_type(2)));

// the largest v of the wavefront's 64 lanes, wave-uniform
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const int q = __shfl_xor(v, off, 64);
    v = q > v ? q : v;
  }
  return __builtin_amdgcn_readfirstlane(v);
}

// One (x, v) row entry, non-temporal: every byte of the car rows is touched once per pass.  NT = false: default caching.
template <bool NT = true>
__device__ __forceinline__ float2 ld_nt(const float2 *ptr) {
  if (!NT) return *ptr;
  const f2v t = __builtin_nontemporal_load(reinterpret_cast<const f2v *>(ptr));
  return make_float2(t.x, t.y);
}
template <bool NT = true>
__device__ __forceinline__ void st_nt(float2 *ptr, float a, float b) {
  if (!NT) {
    *ptr = make_float2(a, b);
    return;
  }
  f2v t;
  t.x = a;
  t.y = b;
  __builtin_nontemporal_store(t, reinterpret_cast<f2v *>(ptr));
}

// sim (:50-62) for a single-archetype car: idm_step_fast where the handle passed the division self-test and EVERY lane
// that calls is inside its domain (one wave-wide test), idm_step otherwise - bit-identical either way.  (The two-car
// step of the two-tick passes tests both cars' speeds with one ballot and keeps its own selection.)
__device__ __forceinline__ void idm_plain(const Dev &d, float x, float v, float xl, float vl, float ll, float &xn, float &vn) {
  const bool off_domain = __builtin_amdgcn_ballot_w64(!idm_fast_domain(v)) != 0ull;
  if (d.fastdiv && !off_domain) idm_step_fast(d, x, v, xl, vl, ll, xn, vn);
  else idm_step(d, x, v, xl, vl, ll, xn, vn);
}

// Heterogeneous cars spawned this tick, add_car :97-114 car by car: each queues behind the road's tail at the moment it
// is created - the tail's OWN length and minimum gap - and brings the row add_new_cars drew for it (:164; row 0 where
// the handle has no draws).  step(k, x, v, side word) for cars n_old .. n_old + n_sp - 1; smax: the loop bound (the
// wavefront's largest n_sp where step needs the lanes together).  arch: the LDS copy of the archetype table.
template <class Step>
__device__ __forceinline__ void het_spawns(const Dev &d, const RoadPrep &p, int id, int env, int e, int tick, int tidx,
                                           int n_old, int n_sp, int smax, const float *arch, Step &&step) {
  int lc = ring_adv(p.ld, n_old, d.C);
  float tx = d.tailx[id];
  int ta = d.taila[id];
  const int ej = d.entry_idx[e];
  const uint8_t *rows = (d.spawn_arch && d.spawn_mode == TFX_SPAWN_COUNTS && ej >= 0)
                            ? d.spawn_arch + (size_t)tidx * d.spawn_arch_stride +
                                  ((size_t)env * d.n_entry + ej) * d.spawn_arch_S
                            : nullptr;
  for (int s = 0; s < smax; ++s)
    if (s < n_sp) {
      const int row = (rows && s < d.spawn_arch_S) ? (rows[s] & (TFX_MAX_ARCH - 1)) : 0;
      const float start = (lc != p.ld) ? (tx - arch[ta * ARCH_W + AR_L]) - arch[ta * ARCH_W + AR_S0] : INFINITY;
      const float xs = (start < 0.0f) ? start : 0.0f;
      step(n_old + s, xs, arch[row * ARCH_W + AR_V], side_pack(tick, row));
      lc = wrap1(lc + 1, d.C);
      tx = xs;
      ta = row;
    }
}

// Wrapped ring: the waiting count tests x, not v, on ring slots 1..lastcar (:210) = the cars from index kq on (counted
// from the head); an unwrapped ring has no such car.
__device__ __forceinline__ int kq_of(const RoadPrep &p, int C) { return (p.ld > p.lc) ? C - 1 - p.ld : 0x7fffffff; }
// car k's new state (xn, vn) into the road's waiting and detected counts
__device__ __forceinline__ void count_car(const Dev &d, int k, int kq, float xn, float vn, int &n_wait, int &n_det) {
  const float wq = (k >= kq) ? xn : vn;
  n_wait += (wq < d.thresh) ? 1 : 0;
  n_det += (xn > d.near_end) ? 1 : 0;
}

// What a lane knows of its road of a tile (road) and where that road's cars are (columns); either half can be used alone.
struct TileLane {
  int e_slot;  // the slot's road id, -1: the slot holds no road
  bool valid;
  int e, id;   // road id and [env][road id] - road 0 where the slot holds none
  float2 *col, *ocol;   // T[k] of this road = col[k * 64]; its outbox column (KP rows)
  float *wcol, *owcol;  // W: the side words - same rows as the cars
  __device__ __forceinline__ void road(const Dev &d, long tile, int env, int lane) {
    e_slot = d.slot_road[(int)(tile - (long)env * d.G) * 64 + lane];
    valid = e_slot >= 0;
    e = valid ? e_slot : 0;
    id = env * d.R + e;
  }
  template <bool W>
  __device__ __forceinline__ void columns(const Dev &d, long tile, int lane) {
    col = d.xv + ((size_t)tile * d.trows) * 64 + lane;
    ocol = d.outb + ((size_t)tile * KP) * 64 + lane;
    wcol = W ? d.w + ((size_t)tile * d.trows) * 64 + lane : nullptr;
    owcol = W ? d.outw + ((size_t)tile * KP) * 64 + lane : nullptr;
  }
};

// the tick's phase of the periodic spawner (spawn_count's tick_mod_period)
__device__ __forceinline__ int spawn_phase(const Dev &d, int tick) {
  return (d.spawn_mode == TFX_SPAWN_PERIODIC) ? tick % d.spawn_period : 0;
}

// The end of a walker kernel: the wavefront's vehicle-updates into the counter, the tick into the second clock word.
// reduce = false (wave-uniform): a wavefront that counted nothing by construction (k_move_ts's later segments).
__device__ __forceinline__ void finish_walk(const Dev &d, int lane, unsigned long long my_updates, int tick, bool reduce = true) {
  if (reduce) {
    for (int off = 32; off > 0; off >>= 1) my_updates += __shfl_down(my_updates, off);
    if (lane == 0 && my_updates) veh_add(d.veh, my_updates);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) *d.tickB = tick;
}

// "Phase W" of a road that took ONE tick: its waiting / detected / passed words, the 16-byte record the advance
// consumes, the stamp that sends the env to the serial advance, the fake leader's x for tfx_export_ring.
//   accumulate: `passed` adds up (the later ticks of an agent step) instead of being overwritten
//   tail_row: heterogeneous cars - table row of the road's tail after the move (rec.w), otherwise 0
//   serial: a car ran through a whole road, or more than TFX_KP cars left (the caller's `far || kpop > KP`)
__device__ __forceinline__ void store_tick_outputs(const Dev &d, const RoadPrep &p, int env, int e, int id, int tick, int n_tot,
                                                   int n_wait, int n_det, int kpop, float tail_x, int tail_row, bool serial,
                                                   bool accumulate) {
  if (e < d.r) {
    int *ob = d.obs + (size_t)env * d.obs_len;
    if (n_tot > 0) {  // `detected` keeps its last value while a road is empty (:199-201)
      d.waiting[(size_t)env * d.r + e] += n_wait;
      ob[d.r + e] = n_det;
    }
    ob[e] = accumulate ? ob[e] + kpop : kpop;
    if (kpop > 0) d.passed_dst[(size_t)env * d.I + e % d.I] = 1;
  }
  d.rec[id] = make_int4(rec_pack(kpop, p.ld, d.C), rec_y(p.ovf_sp, kpop > KP), __float_as_int(tail_x), n_tot | (tail_row << 16));
  if (serial) d.env_flag[env] = tick + 1;
  d.leadx[id] = p.xL;
}

}  // namespace tfx
