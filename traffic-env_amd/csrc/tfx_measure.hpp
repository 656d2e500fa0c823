// tfx_measure.hpp - k_measure: the standard traffic measures per road (tfx_road_measures, include/tfx.h) - cars in
// range, cars halted, the standing queue at the head of the road, the sum of the speeds - from ONE read of the live cars.
//
// Read-only: the shared walk of the road kernels (tfx_walk.hpp) over the (x, v) plane; the side plane (spawn ticks, table
// rows) plays no part.
//   * every lane consumes its own road's cars from the head to the tail, four running values in registers: the count,
//     the halted count, the queue with its "prefix still unbroken" flag, the speed sum - one float32 add per car in
//     range, in car order, which is what makes the sum reproducible bit for bit and equal on both layouts;
//   * the four words are stored (or, TFX_MEASURE_ACCUMULATE, added) per lane at [env][road id].
#pragma once
#include "tfx_common.hpp"
#include "tfx_walk.hpp"

namespace tfx {

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
  const int G = d.G;
  const long items = (long)d.E * G;
  const long nw = (long)gridDim.x * 4;

  for (long item = (long)blockIdx.x * 4 + wv; item < items; item += nw) {
    const int env = (int)(item / G);
    const TileRoad r = tile_road(d, env, (int)(item - (long)env * G), lane);
    const size_t id = r.id;
    MeasureAcc a;
    walk_cars<2, false, false>(d, r, lane, false, [&](bool, f2v c, float) { a.take(c.x, c.y, halt, x_from); });

    if (r.live) {
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
