// tfx_ends.hpp - k_ends: the two ends of every road (tfx_road_ends, include/tfx.h) - its first K cars as (distance to
// the stop line, speed) pairs with their archetype rows, and its last car - the one road kernel that hands out cars
// instead of sums over them.
//
// Read-only, on the shared walk of the road kernels (tfx_walk.hpp) over the (x, v) plane and, in heterogeneous handles,
// the side plane (a car's row is the low bits of its side word; plain and validate handles never load it).
//   * The walk is cut short: the TileRoad's count is clamped to K before walk_cars sees it, so a lane loads rows
//     hb .. hb + min(n, K) - 1 of its column and the tile's deepest row is at most K + 2 (hb is 0 to 2), whatever the
//     density.  On the ring layout a lane takes the first min(n, K) slots behind its leading slot.
//   * The last car is one more load per lane - row hb + n - 1 of the lane's column, bounded by trows as the walk bounds
//     its rows; on the ring layout slot lastcar - issued ahead of the walk, so it is in flight with the walk's rows.
//     Lanes of empty roads load nothing.
//   * A lane's K pairs cannot be registers (a dynamically indexed register array goes to scratch, as k_cells found).
//     They are staged in LDS, [j][lane] per wavefront - a plane of (distance, speed) pairs and a byte plane of rows,
//     filled with the pads first; a lane writes only its own column, so there are no atomics.  Row j is rotated by
//     (32 / KMAX) * j lanes, as k_cells rotates its cells: without it the store pass would read a road's K entries from
//     one bank.
//   * After a tile the wavefront stores 64 * K entries per plane: lanes run over (road, j) pairs, so every road's K
//     entries leave as one contiguous run at [env][road id][0 .. K) - k_cells' store pass.  The four per-road values
//     (n_cars, n_heads, tail, tail_row) are stored per lane at [env][road id].  Lanes of slots without a road store
//     nothing.  A plane whose pointer is null is skipped everywhere.
//   * float32: one subtraction per listed car (length - x); everything else is moved, pads included, bit for bit.
// Instantiated on the bound of K (4, 8, 16: 9, 18, 36 KB of LDS per workgroup), so that a short list keeps its occupancy.
#pragma once
#include "tfx_common.hpp"
#include "tfx_walk.hpp"

namespace tfx {

struct EndsOut {
  int *n_cars, *n_heads;  // [E][R] by road id; null = not wanted
  f2v *heads;             // [E][R][K] (distance, speed)
  uint8_t *head_rows;     // [E][R][K]
  f2v *tail;              // [E][R] (x, v)
  uint8_t *tail_row;      // [E][R]
};

// entry of (car j, lane l) in a wavefront's [KMAX][64] plane: row j rotated by (32 / KMAX) * j lanes
template <int KMAX>
__device__ __forceinline__ int ends_word(int j, int l) {
  return j * 64 + ((l + (32 / KMAX) * j) & 63);
}

// a wavefront per (env, tile), four to a workgroup, striding over the E * G items; K <= KMAX cars from the head
template <int KMAX>
__global__ __launch_bounds__(256) void k_ends(const Dev d, const tfx_ends_params p, const EndsOut o) {
  __shared__ f2v s_xv[4][KMAX * 64];
  __shared__ uint8_t s_row[4][KMAX * 64];
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int G = d.G, R = d.R, K = p.k;
  const long items = (long)d.E * G;
  const long nw = (long)gridDim.x * 4;
  const bool want_h = o.heads != nullptr, want_r = o.head_rows != nullptr;
  const bool want_t = o.tail != nullptr || o.tail_row != nullptr;
  const bool side = d.het && (want_r || o.tail_row != nullptr);
  const int div_k = (65536 + K - 1) / K;  // q / K == (q * div_k) >> 16 for q < 1024, K <= 16 (error q / 65536 < 1 / 16)
  const f2v pad{p.pad_dist, p.pad_v};

  for (long item = (long)blockIdx.x * 4 + wv; item < items; item += nw) {
    const int env = (int)(item / G);
    const TileRoad r = tile_road(d, env, (int)(item - (long)env * G), lane);
    const int e_slot = r.e_slot;
    const size_t id = r.id;

    // the last car, ahead of the walk
    f2v tl{p.pad_tail_x, p.pad_v};
    float tsw = 0.0f;
    if (want_t && r.n > 0) {
      size_t at;
      if (d.layout == 1) {
        const int hb = d.hb[id];
        const int rows = r.n + hb > d.trows ? d.trows : r.n + hb;
        at = (r.tile * (size_t)d.trows + (size_t)(rows - 1)) * 64 + lane;
      } else {
        // wrap1 taken n times from the leading slot: lastcar, by the count's own definition - and inside the ring
        // whatever the two words hold
        const int slot = r.leading + r.n;
        at = id * d.C + (slot >= d.C ? slot - (d.C - 1) : slot);
      }
      tl = reinterpret_cast<const f2v *>(d.xv)[at];
      if (side) tsw = d.w[at];
    }

    if (want_h || want_r) {
      for (int j = 0; j < K; ++j) {
        if (want_h) s_xv[wv][ends_word<KMAX>(j, lane)] = pad;
        if (want_r) s_row[wv][ends_word<KMAX>(j, lane)] = TFX_ENDS_NO_CAR;
      }
      TileRoad rk = r;
      rk.n = r.n < K ? r.n : K;
      int j = 0;
      walk_cars<2, true, false>(d, rk, lane, side && want_r, [&](bool, f2v c, float sw) {
        if (want_h) s_xv[wv][ends_word<KMAX>(j, lane)] = f2v{d.length - c.x, c.y};
        if (want_r) s_row[wv][ends_word<KMAX>(j, lane)] = (uint8_t)(d.het ? side_arch(sw) : 0);
        ++j;
      });
    }

    if (r.live) {
      if (o.n_cars) o.n_cars[id] = r.n;
      if (o.n_heads) o.n_heads[id] = r.n < K ? r.n : K;
      if (o.tail) o.tail[id] = tl;
      if (o.tail_row) o.tail_row[id] = (uint8_t)(r.n > 0 ? (d.het ? side_arch(tsw) : 0) : TFX_ENDS_NO_CAR);
    }

    if (want_h || want_r) {
      // the planes change hands: written per lane, read per (road, j) pair
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      for (int it = 0; it < K; ++it) {
        const int q = it * 64 + lane;
        const int rl = (q * div_k) >> 16;  // the tile's road q / K ...
        const int j = q - rl * K;          // ... and its car
        const int e_r = __shfl(e_slot, rl, 64);
        if (e_r >= 0) {
          const size_t at = ((size_t)env * R + e_r) * (size_t)K + j;
          if (want_h) o.heads[at] = s_xv[wv][ends_word<KMAX>(j, rl)];
          if (want_r) o.head_rows[at] = s_row[wv][ends_word<KMAX>(j, rl)];
        }
      }
      // ... and back, before the next item's lanes fill them with the pads
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
  }
}

}  // namespace tfx
