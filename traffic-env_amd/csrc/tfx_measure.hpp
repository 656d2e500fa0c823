// tfx_measure.hpp - k_measure: the standard traffic measures per road (tfx_road_measures, include/tfx.h) - cars in
// range, cars halted, the standing queue at the head of the road, the sum of the speeds - from ONE read of the live cars.
//
// Read-only, and shaped like k_clone (tfx_clone.hpp) and k_move_t (tfx_move_t.hpp): one wavefront per (env, tile), lane
// per road.
//   * the lane of storage slot 64 * tile + j loads its road's leading / lastcar / hb; the wavefront reduces the tile's
//     deepest live row;
//   * rows 0 .. kmax-1 of the tile are walked as 64 x 8 B row loads, coalesced, MEAS_P rows in flight; a lane loads the
//     rows its own road has cars in and no others (not the rows a two-tick pass left empty at the top of the column,
//     not the rows past the road's count), so a sparse env costs less than a full one;
//   * every lane consumes its own road's cars from the head to the tail, four running values in registers: the count,
//     the halted count, the queue with its "prefix still unbroken" flag, the speed sum - one float32 add per car in
//     range, in car order, which is what makes the sum reproducible bit for bit and equal on both layouts;
//   * the four words are stored (or, TFX_MEASURE_ACCUMULATE, added) per lane at [env][road id].
// Only (x, v) is read: the side plane (spawn ticks, table rows) plays no part.
// Ring layout (tfx_config.layout = 0, the non-default one): the same decomposition, each lane walks the ring slots of
// its road from leading + 1 with wrap1.
#pragma once
#include "tfx_common.hpp"
#include "tfx_move_t.hpp"

namespace tfx {

constexpr int MEAS_P = 8;  // rows in flight per wavefront

struct MeasureOut {
  int *n_cars, *n_halted, *queue;  // [E][R] by road id; null = not wanted
  float *speed_sum;
  int accumulate;                  // out += value instead of out = value
};

// a road's running values; take() is the definition of include/tfx.h for one car, cars taken from the head on
struct MeasureAcc {
  int cars = 0, halted = 0, queue = 0;
  bool open = true;  // every car so far was in range and halted: the queue still grows
  float sum = 0.0f;
  __device__ __forceinline__ void take(float x, float v, float halt, float x_from) {
    const bool in = x >= x_from;
    const bool still = in && v < halt;
    cars += in ? 1 : 0;
    halted += still ? 1 : 0;
    open = open && still;
    queue += open ? 1 : 0;
    sum = in ? sum + v : sum;
  }
};

// a wavefront per (env, tile), four to a workgroup, striding over the E * G items
__global__ __launch_bounds__(256) void k_measure(const Dev d, const float halt, const float x_from, const MeasureOut o) {
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int G = d.G, R = d.R, C = d.C;
  const long items = (long)d.E * G;
  const long nw = (long)gridDim.x * 4;

  for (long item = (long)blockIdx.x * 4 + wv; item < items; item += nw) {
    const int env = (int)(item / G);
    const int g = (int)(item - (long)env * G);
    const int e_slot = d.slot_road[g * 64 + lane];
    const bool valid = e_slot >= 0;
    const size_t id = (size_t)env * R + (valid ? e_slot : 0);
    const int ld = d.leading[id];
    int n = valid ? ring_count(ld, d.lastcar[id], C) : 0;
    n = n < 0 ? 0 : (n > C - 1 ? C - 1 : n);
    MeasureAcc a;

    if (d.layout == 1) {
      const int hb = d.hb[id];  // rows a two-tick pass left empty at the top of the column (tfx_move_tt.hpp)
      int rows = valid ? n + hb : 0;
      rows = rows > d.trows ? d.trows : rows;
      int kmax = rows;
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        const int q = __shfl_xor(kmax, off, 64);
        kmax = q > kmax ? q : kmax;
      }
      kmax = __builtin_amdgcn_readfirstlane(kmax);
      const f2v *col = reinterpret_cast<const f2v *>(d.xv + ((size_t)env * G + g) * (size_t)d.trows * 64 + lane);
      for (int k0 = 0; k0 < kmax; k0 += MEAS_P) {
        f2v c[MEAS_P];
#pragma unroll
        for (int u = 0; u < MEAS_P; ++u)
          if (k0 + u >= hb && k0 + u < rows) c[u] = col[(size_t)(k0 + u) * 64];
#pragma unroll
        for (int u = 0; u < MEAS_P; ++u)
          if (k0 + u >= hb && k0 + u < rows) a.take(c[u].x, c[u].y, halt, x_from);
      }
    } else {
      const float2 *row = d.xv + id * C;
      int slot = ld;
      for (int k = 0; k < n; ++k) {
        slot = wrap1(slot + 1, C);
        const float2 c = row[slot];
        a.take(c.x, c.y, halt, x_from);
      }
    }

    if (valid) {
      if (o.accumulate) {
        if (o.n_cars) o.n_cars[id] += a.cars;
        if (o.n_halted) o.n_halted[id] += a.halted;
        if (o.queue) o.queue[id] += a.queue;
        if (o.speed_sum) o.speed_sum[id] = o.speed_sum[id] + a.sum;
      } else {
        if (o.n_cars) o.n_cars[id] = a.cars;
        if (o.n_halted) o.n_halted[id] = a.halted;
        if (o.queue) o.queue[id] = a.queue;
        if (o.speed_sum) o.speed_sum[id] = a.sum;
      }
    }
  }
}

}  // namespace tfx
