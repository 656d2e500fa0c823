// tfx_put.hpp - k_put: the cars of chosen envs written from one flat run (tfx_put_cars, include/tfx.h) - the mirror
// image of k_cars (tfx_cars.hpp).  Road e of selected env s receives the cars at offsets[s * R + e] ..
// offsets[s * R + e + 1] of the caller's planes, head first, and with them every per-road word tfx_import_ring followed by
// tfx_refresh would leave: leading, lastcar, hb = 0, leadx, tailx, taila.  No other state of the handle is written.
//
// k_cars' and k_clone's decomposition: a wavefront per (selected env, tile) item, four to a workgroup, striding over the
// n_sel * G items, a lane per road through slot_road.
//   * The env of an item comes from env_ids[s]; of an id outside [0, E) nothing is read or written.  A road whose mask
//     byte is 0 is left alone altogether.
//   * The road's run is cut to the entries the planes have - [max(base, 0), min(base + run, cap)) - and to the cars a ring
//     holds (C - 2; trows on the transposed layout); what does not fit is added to *lost, one atomicAdd per such road.
//     No entry outside [0, cap) is read whatever the offsets hold, and stores go to the item's own columns and words only.
//   * Transposed layout: a lane loading its own cars from base + j would scatter the 64 loads of a row over 64 runs.  So
//     per block of WALK_P rows the lanes run over (road of the tile, u) pairs - k_cars' flush reversed: base and count
//     come across the wavefront by __shfl, a road's up to 8 cars of the block arrive as one contiguous 64-byte run of xv
//     with the matching runs of row and spawn, and land in the wavefront's [WALK_P][64] LDS planes under ends_word<8>'s
//     rotation; then every lane takes its own column out of LDS and rows k0 .. k0 + WALK_P - 1 leave as full-width row
//     stores, a lane storing rows < n of its road only.  Rounds in which no road has a car are skipped (uniform).
//   * Ring layout: each lane writes its road's slots from leading' + 1 under wrap1 and lead_x into slot leading'.
//   * The side word is k_import_ring's: side_pack(tick, row) on heterogeneous handles, the tick otherwise, the tick moved
//     by spawn_shift as clone_side moves it.
// NT: non-temporal row stores, as k_clone's - tfx_put_cars takes them on handles whose cars do not fit the Infinity Cache
// (DESIGN.md 7m has the figures).
// LDS: 4 wavefronts x (4 KB + 2 KB) = 24 KB per workgroup; no workgroup barrier, no atomics besides `lost`.
#pragma once
#include "tfx_clone.hpp"
#include "tfx_common.hpp"
#include "tfx_ends.hpp"
#include "tfx_walk.hpp"

namespace tfx {

struct PutArgs {
  const int *env_ids;        // [n_sel] on the device; null: selection s is env s
  const uint8_t *road_mask;  // [R] on the device; null: every road
  const int *offsets;        // [n_sel * R + 1] on the device
  int n_sel;
  int cap;                   // entries the planes hold
  const f2v *xv;             // [cap] (x, v)
  const uint8_t *row;        // [cap] archetype row; null: row 0
  const float *spawn;        // [cap] spawn tick; null: 0
  const int *leading;        // [n_sel * R] new leading; null or no ring index: the road keeps its own
  const float *lead_x;       // [n_sel * R] x shown in slot leading; null: +inf
  int spawn_shift;
  unsigned long long *lost;  // cars that did not fit, or null
};

// the side word of a listed car (k_import_ring's) under the clock spawn_shift ticks on (clone_side's rule)
__device__ __forceinline__ float put_side(const Dev &d, float tk, int row, int shift) {
  const float w = d.het ? side_pack((int)tk, row & (TFX_MAX_ARCH - 1)) : tk;
  return clone_side(d, w, shift);
}

template <bool NT>
__global__ __launch_bounds__(256) void k_put(const Dev d, const PutArgs a) {
  __shared__ f2v s_xv[4][WALK_P * 64];
  __shared__ float s_sw[4][WALK_P * 64];
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int G = d.G, R = d.R, C = d.C;
  const long items = (long)a.n_sel * G;
  const long nw = (long)gridDim.x * 4;
  const bool side = d.w != nullptr;
  f2v *pxv = s_xv[wv];
  float *psw = s_sw[wv];

  for (long item = (long)blockIdx.x * 4 + wv; item < items; item += nw) {
    const int s = (int)(item / G);
    const int g = (int)(item - (long)s * G);
    const int env = __builtin_amdgcn_readfirstlane(a.env_ids ? a.env_ids[s] : s);
    if (env < 0 || env >= d.E) continue;  // (uniform) not one of the handle's envs: nothing is written
    const int e_slot = d.slot_road[g * 64 + lane];
    const bool live = e_slot >= 0 && (!a.road_mask || a.road_mask[e_slot] != 0);
    const int e = e_slot >= 0 ? e_slot : 0;
    const size_t id = (size_t)env * R + e;
    const size_t key = (size_t)s * R + e;

    // the road's run, cut to the planes and to the ring
    int base = 0, n = 0, ld = 1;
    if (live) {
      const long b0 = a.offsets[key];
      long run = (long)a.offsets[key + 1] - b0;
      if (run < 0) run = 0;
      const long lo = b0 < 0 ? 0 : b0;
      long hi = b0 + run;
      if (hi > (long)a.cap) hi = a.cap;
      long fit = hi - lo;
      if (fit < 0) fit = 0;
      int room = C - 2;
      if (d.layout == 1 && room > d.trows) room = d.trows;
      if (room < 0) room = 0;
      if (fit > room) fit = room;
      base = (int)lo;
      n = (int)fit;
      if (run > fit && a.lost) atomicAdd(a.lost, (unsigned long long)(run - fit));
      ld = a.leading ? a.leading[key] : 0;
      if (ld < 1 || ld > C - 1) ld = d.leading[id];
      if (ld < 1 || ld > C - 1) ld = 1;  // (never on a handle that was reset: no store leaves the road's slots regardless)
    }
    const float lead_x = (live && a.lead_x) ? a.lead_x[key] : __builtin_inff();
    float tail_x = 0.0f;  // x of car n - 1
    float tail_w = 0.0f;  // its side word

    if (d.layout == 1) {
      const int kmax = wave_max(n);
      const size_t col = ((size_t)env * G + g) * (size_t)d.trows * 64 + lane;
      f2v *dx = reinterpret_cast<f2v *>(d.xv + col);
      float *dw = side ? d.w + col : nullptr;
      for (int k0 = 0; k0 < kmax; k0 += WALK_P) {
        // lanes over (road of the tile, u) pairs: a road's cars of the block are one contiguous run of the planes
        for (int it = 0; it < WALK_P; ++it) {
          const int rl = it * (64 / WALK_P) + lane / WALK_P;  // the tile's road ...
          const int u = lane % WALK_P;                        // ... and its car of the block
          const int j = k0 + u;
          const long at = (long)__shfl(base, rl, 64) + j;
          const bool mine = j < __shfl(n, rl, 64) && at >= 0 && at < (long)a.cap;
          if (__builtin_amdgcn_ballot_w64(mine) == 0ull) continue;  // (uniform) no road of this round has a car
          if (mine) {
            const int word = ends_word<WALK_P>(u, rl);
            pxv[word] = a.xv[at];
            if (side) psw[word] = put_side(d, a.spawn ? a.spawn[at] : 0.0f, a.row ? a.row[at] : 0, a.spawn_shift);
          }
        }
        // the planes change hands: written per (road, u) pair, read per lane
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
        for (int u = 0; u < WALK_P; ++u) {
          if (k0 + u < n) {
            const int word = ends_word<WALK_P>(u, lane);
            const f2v c = pxv[word];
            tail_x = c.x;
            if (NT) __builtin_nontemporal_store(c, dx + (size_t)(k0 + u) * 64);
            else dx[(size_t)(k0 + u) * 64] = c;
            if (side) {
              tail_w = psw[word];
              if (NT) __builtin_nontemporal_store(tail_w, dw + (size_t)(k0 + u) * 64);
              else dw[(size_t)(k0 + u) * 64] = tail_w;
            }
          }
        }
        // ... and back, before the pairs fill them with the next block
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      }
    } else if (live) {
      float2 *rx = d.xv + id * C;
      int slot = ld;
      for (int j = 0; j < n; ++j) {
        slot = wrap1(slot + 1, C);
        const f2v c = a.xv[base + j];
        rx[slot] = make_float2(c.x, c.y);
        tail_x = c.x;
        if (side) d.w[id * C + slot] = put_side(d, a.spawn ? a.spawn[base + j] : 0.0f, a.row ? a.row[base + j] : 0, a.spawn_shift);
      }
      rx[ld].x = lead_x;
    }

    // ---- the per-road words: what tfx_import_ring + tfx_refresh would leave ---------------------------------
    if (live) {
      const int lc = ring_adv(ld, n, C);
      d.leading[id] = ld;
      d.lastcar[id] = lc;
      if (d.layout == 1) {
        d.hb[id] = 0;
        d.leadx[id] = lead_x;
        d.tailx[id] = n > 0 ? tail_x : 0.0f;
        if (d.het) d.taila[id] = n > 0 ? side_arch(tail_w) : 0;
      } else {
        d.tailx[id] = n > 0 ? tail_x : lead_x;  // (k_refresh: the x in slot lastcar)
      }
    }
  }
}

}  // namespace tfx
