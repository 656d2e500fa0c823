// tfx_cells.hpp - k_cells: car count and speed sum per CELL of every road (tfx_road_cells, include/tfx.h) - the discrete
// traffic state encoding - from ONE read of the live cars.  k_measure (tfx_measure.hpp) generalised from four words per
// road to B cells per road; read-only like it, and on the same walk (tfx_walk.hpp) in its uniform form: every lane takes
// part in every step up to the tile's longest road, because a step uses ballot and cross-lane reads.
//
// What is new:
//   * B running values per lane cannot be registers (a dynamically indexed register array goes to scratch).  The two
//     planes live in LDS, [cell][lane] per wavefront, 2 * BMAX * 64 words; a lane touches only its own column of them
//     while it walks, so there are no atomics.  Row b is rotated by (32 / BMAX) * b lanes: lanes that are in the same
//     cell - the usual case, cars come from the head down - fall on 32 different banks, and so do the reads of the store
//     pass below (without the rotation that pass would put a road's B cells on ONE bank; padding the rows instead would
//     take the 32-cell instantiation past 64 KB).
//   * A lane keeps the cell it is in - index, [lo, hi), count and sum - in registers and goes to LDS only when a car
//     falls outside [lo, hi): write the old cell back, find the new one, fetch its values.  x is almost always
//     non-increasing down a road, so that happens about B times per road, but nothing relies on the order: any x is
//     binned by the definition's own expression, b = #{k in 1..B-1 : x >= edges[k]} - comparisons against edges held in
//     scalar registers (kernel argument by value, padded with +inf from k = B on), run for the whole wavefront when any
//     lane needs it; lo / hi of the new cell come by a cross-lane read from the lanes that hold edge k in a register.
//   * After a tile the wavefront stores 64 * B words per plane: lanes run over (road, cell) pairs, so every road's B
//     values leave as one contiguous run at [env][road id][0 .. B); with the accumulate flag the same pass reads, adds
//     and writes.  Lanes of slots without a road store nothing.  A plane whose pointer is null is skipped everywhere.
// Instantiated on the cell bound (8, 16, 32: 16, 32, 64 KB of LDS per workgroup), so that few cells keep their occupancy.
#pragma once
#include "tfx_common.hpp"
#include "tfx_walk.hpp"

namespace tfx {

struct CellEdges {
  float lo, hi;                  // edges[0], edges[B]: in range iff lo <= x < hi
  float inner[TFX_MAX_CELLS];    // inner[k] = edges[k] for k = 1 .. B-1, +inf from k = B on; inner[0] unused
};

struct CellOut {
  int *n_cars;       // [E][R][B] by road id; null = not wanted
  float *speed_sum;
  int accumulate;    // out = out + value instead of out = value
};

// word of (cell b, lane l) in a wavefront's [BMAX][64] plane: row b rotated by (32 / BMAX) * b lanes
template <int BMAX>
__device__ __forceinline__ int cell_word(int b, int l) {
  return b * 64 + ((l + (32 / BMAX) * b) & 63);
}

// A lane's walk over its road's cars: the cell it is in lives in registers, the others in the wavefront's LDS planes.
template <int BMAX>
struct CellWalk {
  int *cnt;      // this wavefront's planes
  float *sum;
  int lane;
  float edge;    // lane k holds edges[k] for the cross-lane read: -inf in lane 0, +inf from lane B on
  bool want_n, want_s;
  int cur = -1;  // no cell yet: [lo, hi) is empty and the first car in range misses
  float lo = INFINITY, hi = -INFINITY;
  int rc = 0;
  float rs = 0.0f;

  __device__ __forceinline__ void put_back() {
    if (cur >= 0) {
      if (want_n) cnt[cell_word<BMAX>(cur, lane)] = rc;
      if (want_s) sum[cell_word<BMAX>(cur, lane)] = rs;
    }
  }

  // every lane of the wavefront calls this together; `live`: this lane has a car (x, v)
  __device__ __forceinline__ void take(const CellEdges &ed, bool live, float x, float v) {
    const bool in = live && x >= ed.lo && x < ed.hi;
    const bool miss = in && !(x >= lo && x < hi);
    if (__builtin_amdgcn_ballot_w64(miss) != 0ull) {
      int b = 0;
#pragma unroll
      for (int k = 1; k < BMAX; ++k) b += x >= ed.inner[k] ? 1 : 0;
      const float nlo = __shfl(edge, b, 64), nhi = __shfl(edge, b + 1, 64);
      if (miss) {
        put_back();
        cur = b;
        lo = nlo;
        hi = nhi;
        rc = want_n ? cnt[cell_word<BMAX>(b, lane)] : 0;
        rs = want_s ? sum[cell_word<BMAX>(b, lane)] : 0.0f;
      }
    }
    rc += in ? 1 : 0;
    rs = in ? rs + v : rs;
  }
};

// a wavefront per (env, tile), four to a workgroup, striding over the E * G items; B <= BMAX cells
template <int BMAX>
__global__ __launch_bounds__(256) void k_cells(const Dev d, const CellEdges ed, const int B, const CellOut o) {
  __shared__ int s_cnt[4][BMAX * 64];
  __shared__ float s_sum[4][BMAX * 64];
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int G = d.G, R = d.R;
  const long items = (long)d.E * G;
  const long nw = (long)gridDim.x * 4;
  const bool want_n = o.n_cars != nullptr, want_s = o.speed_sum != nullptr;
  const int div_b = (65536 + B - 1) / B;  // p / B == (p * div_b) >> 16 for p < 2048, B <= 32 (error p / 65536 < 1 / 32)

  float edge = lane == 0 ? -INFINITY : INFINITY;
#pragma unroll
  for (int k = 1; k < BMAX; ++k) edge = lane == k ? ed.inner[k] : edge;

  for (long item = (long)blockIdx.x * 4 + wv; item < items; item += nw) {
    const int env = (int)(item / G);
    const TileRoad r = tile_road(d, env, (int)(item - (long)env * G), lane);
    const int e_slot = r.e_slot;

    CellWalk<BMAX> w{s_cnt[wv], s_sum[wv], lane, edge, want_n, want_s};
    for (int b = 0; b < B; ++b) {
      if (want_n) s_cnt[wv][cell_word<BMAX>(b, lane)] = 0;
      if (want_s) s_sum[wv][cell_word<BMAX>(b, lane)] = 0.0f;
    }

    walk_cars<2, false, true>(d, r, lane, false, [&](bool live, f2v c, float) { w.take(ed, live, c.x, c.y); });
    w.put_back();

    // the planes change hands: written per lane, read per (road, cell) pair
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    for (int it = 0; it < B; ++it) {
      const int p = it * 64 + lane;
      const int rl = (p * div_b) >> 16;  // the tile's road p / B ...
      const int b = p - rl * B;          // ... and its cell
      const int e_r = __shfl(e_slot, rl, 64);
      if (e_r >= 0) {
        const size_t at = ((size_t)env * R + e_r) * (size_t)B + b;
        if (want_n) {
          const int val = s_cnt[wv][cell_word<BMAX>(b, rl)];
          o.n_cars[at] = o.accumulate ? o.n_cars[at] + val : val;
        }
        if (want_s) {
          const float val = s_sum[wv][cell_word<BMAX>(b, rl)];
          o.speed_sum[at] = o.accumulate ? o.speed_sum[at] + val : val;
        }
      }
    }
    // ... and back, before the next item's lanes clear them
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
}

}  // namespace tfx
