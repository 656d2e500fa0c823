// tfx_follow.hpp - k_follow: the car-following measures per road (tfx_road_following, include/tfx.h) - net gaps, time
// headways, closing speeds with time to collision and DRAC, platoon joins, overlaps - from ONE read of the live cars.
//
// Read-only, on the shared walk of the road kernels (tfx_walk.hpp) over the (x, v) plane and, in heterogeneous handles,
// the side plane (the leader's length is that of the table row in ITS side word; the table is a workgroup's LDS copy,
// as in k_frames).  Plain and validate handles never load the side plane.
//   * The walk hands a road's cars to visit from the head to the tail, so a car's leader is the car visited just before
//     it, on both layouts.  This is the one road kernel that carries state from one visited car to the next: the lane
//     keeps its leader's x, v, l and a have-leader flag next to the eleven running values, all in registers.  The carry
//     lives outside the walk, so it survives the walk's blocks of WALK_P rows and the rows a two-tick pass left empty at
//     the top of the column (visit is not called for those); it is constructed inside the stride loop, so nothing
//     carries from one item to the next.
//   * float32 throughout, one rounding per operation in the order include/tfx.h writes them; min and max are compares
//     and selects (a NaN is never taken); two IEEE divisions per pair.
//   * the bound words are stored (or, TFX_FOLLOW_ACCUMULATE, combined) per lane at [env][road id].
#pragma once
#include "tfx_common.hpp"
#include "tfx_walk.hpp"

namespace tfx {

struct FollowOut {
  int *n_cars, *n_pairs, *n_joined, *n_overlap;  // [E][R] by road id; null = not wanted
  float *gap_sum, *gap_min;
  int *n_hw;
  float *hw_sum;
  int *n_conflict;
  float *ttc_min, *drac_max;
  int accumulate;                                // out (+)= value, min or max instead of out = value
};

// a road's running values; take() is the definition of include/tfx.h for one car, cars taken from the head on
struct FollowAcc {
  float lx = 0.0f, lv = 0.0f, ll = 0.0f;  // the leader: the car taken just before
  bool have = false;                      // ... if there was one
  int cars = 0, pairs = 0, joined = 0, overlap = 0, hw = 0, conflict = 0;
  float gap_sum = 0.0f, gap_min = INFINITY, hw_sum = 0.0f, ttc_min = INFINITY, drac_max = 0.0f;
  __device__ __forceinline__ void take(float x, float v, float l, const tfx_follow_params &p) {
    const bool in = x >= p.x_from;
    const bool pair = have && in;
    const float g = (lx - x) - ll;
    const float dv = v - lv;
    cars += in ? 1 : 0;
    pairs += pair ? 1 : 0;
    joined += (pair && g <= p.platoon_gap) ? 1 : 0;
    overlap += (pair && g < 0.0f) ? 1 : 0;
    gap_sum = pair ? gap_sum + g : gap_sum;
    gap_min = (pair && g < gap_min) ? g : gap_min;
    const bool timed = pair && v >= p.v_min;
    hw += timed ? 1 : 0;
    hw_sum = timed ? hw_sum + g / v : hw_sum;
    const bool closing = pair && dv > 0.0f && g > 0.0f;
    const float ttc = g / dv;
    const float drac = (dv * dv) / (g + g);
    conflict += (closing && ttc < p.ttc_crit) ? 1 : 0;
    ttc_min = (closing && ttc < ttc_min) ? ttc : ttc_min;
    drac_max = (closing && drac > drac_max) ? drac : drac_max;
    lx = x;
    lv = v;
    ll = l;
    have = true;
  }
};

// a wavefront per (env, tile), four to a workgroup, striding over the E * G items
__global__ __launch_bounds__(256) void k_follow(const Dev d, const tfx_follow_params p, const FollowOut o) {
  __shared__ float s_arch[TFX_MAX_ARCH * ARCH_W];
  if (d.het) load_arch(d, s_arch);
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int G = d.G;
  const long items = (long)d.E * G;
  const long nw = (long)gridDim.x * 4;

  for (long item = (long)blockIdx.x * 4 + wv; item < items; item += nw) {
    const int env = (int)(item / G);
    const TileRoad r = tile_road(d, env, (int)(item - (long)env * G), lane);
    const size_t id = r.id;
    FollowAcc a;
    walk_cars<2, true, false>(d, r, lane, d.het, [&](bool, f2v c, float sw) {
      a.take(c.x, c.y, d.het ? s_arch[side_arch(sw) * ARCH_W + AR_L] : d.car_l, p);
    });

    if (r.live) {
      if (o.accumulate) {
        if (o.n_cars) o.n_cars[id] += a.cars;
        if (o.n_pairs) o.n_pairs[id] += a.pairs;
        if (o.n_joined) o.n_joined[id] += a.joined;
        if (o.n_overlap) o.n_overlap[id] += a.overlap;
        if (o.gap_sum) o.gap_sum[id] = o.gap_sum[id] + a.gap_sum;
        if (o.gap_min) { const float m = o.gap_min[id]; o.gap_min[id] = a.gap_min < m ? a.gap_min : m; }
        if (o.n_hw) o.n_hw[id] += a.hw;
        if (o.hw_sum) o.hw_sum[id] = o.hw_sum[id] + a.hw_sum;
        if (o.n_conflict) o.n_conflict[id] += a.conflict;
        if (o.ttc_min) { const float m = o.ttc_min[id]; o.ttc_min[id] = a.ttc_min < m ? a.ttc_min : m; }
        if (o.drac_max) { const float m = o.drac_max[id]; o.drac_max[id] = a.drac_max > m ? a.drac_max : m; }
      } else {
        if (o.n_cars) o.n_cars[id] = a.cars;
        if (o.n_pairs) o.n_pairs[id] = a.pairs;
        if (o.n_joined) o.n_joined[id] = a.joined;
        if (o.n_overlap) o.n_overlap[id] = a.overlap;
        if (o.gap_sum) o.gap_sum[id] = a.gap_sum;
        if (o.gap_min) o.gap_min[id] = a.gap_min;
        if (o.n_hw) o.n_hw[id] = a.hw;
        if (o.hw_sum) o.hw_sum[id] = a.hw_sum;
        if (o.n_conflict) o.n_conflict[id] = a.conflict;
        if (o.ttc_min) o.ttc_min[id] = a.ttc_min;
        if (o.drac_max) o.drac_max[id] = a.drac_max;
      }
    }
  }
}

}  // namespace tfx
