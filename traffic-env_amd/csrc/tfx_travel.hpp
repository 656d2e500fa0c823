// tfx_travel.hpp - travel times on the device (tfx_car_ages, tfx_trip_stats, include/tfx.h): two read-only kernels.
//
// k_ages: how long every live car has been on the map, per road - the count, the int64 sum and the maximum of
// side_age(now, side word), `now` read from the handle's device clock as k_clone reads it.  The shared walk of the road
// kernels (tfx_walk.hpp) over the SIDE plane only - 64 x 4 B row loads; xv is never read - with three running integers
// per lane, stored (or, TFX_TRAVEL_ACCUMULATE, added / maxed) at [env][road id].
// Integer arithmetic throughout: the order of the cars does not matter, both layouts and a host loop give the same bits.
//
// k_trips: the finished trips, reduced where advance_hack's device forms log them (trip_times / n_trips of the bound
// buffers).  One wavefront per env, four to a workgroup, striding over the envs; the lanes stride the span
// [min(c, cap), min(n, cap)) of the env's log in coalesced 256 B rows with per-lane integer accumulators, bin every entry
// into a per-wavefront LDS histogram, a wave reduction closes the sums and one lane per output stores.  Entries count in
// ticks, t = (int)(trip_time * 2.0f): exact, the log holds age / 2.0f of an integer age.
//
// The cursor rule (c = cursor[e] if 0 <= cursor[e] <= n, else 0: a log shorter than its cursor was cleared) cannot see
// one case: a log that was cleared and grew back PAST the old cursor before the next call looks like a log that only
// grew, and its first `cursor` entries are skipped.  The caller zeroes the cursor of the envs it resets
// (TrafficVecEnv.travel_times does).
#pragma once
#include "tfx_common.hpp"
#include "tfx_walk.hpp"

namespace tfx {

struct AgeOut {
  int *n_cars;          // [E][R] by road id; null = not wanted
  long long *age_sum;
  int *age_max;
  int accumulate;       // sums += value, max = max(max, value) instead of out = value
};

// a wavefront per (env, tile), four to a workgroup, striding over the E * G items
__global__ __launch_bounds__(256) void k_ages(const Dev d, const AgeOut o) {
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int G = d.G;
  const long items = (long)d.E * G;
  const long nw = (long)gridDim.x * 4;
  const int now = *d.tickA;

  for (long item = (long)blockIdx.x * 4 + wv; item < items; item += nw) {
    const int env = (int)(item / G);
    const TileRoad r = tile_road(d, env, (int)(item - (long)env * G), lane);
    const size_t id = r.id;
    const int n = r.n;
    int amax = 0;
    long long asum = 0;
    walk_cars<0, true, false>(d, r, lane, true, [&](bool, f2v, float sw) {
      const int a = (int)side_age(d, now, sw);
      asum += a;
      amax = a > amax ? a : amax;
    });

    if (r.live) {
      if (o.accumulate) {
        if (o.n_cars) o.n_cars[id] += n;
        if (o.age_sum) o.age_sum[id] += asum;
        if (o.age_max) {
          const int old = o.age_max[id];
          o.age_max[id] = amax > old ? amax : old;
        }
      } else {
        if (o.n_cars) o.n_cars[id] = n;
        if (o.age_sum) o.age_sum[id] = asum;
        if (o.age_max) o.age_max[id] = amax;
      }
    }
  }
}

constexpr int TRIP_BINS = 32;  // the most bins tfx_trip_stats takes

struct TripEdges {
  int e[TRIP_BINS + 1];  // e[0 .. n_bins], non-decreasing; by value, so the call needs no copy
};

struct TripOut {
  int *count;           // [E]; null = not wanted
  long long *tick_sum;
  int *tick_max;
  int *lost;
  int *hist;            // [E][n_bins]
  int accumulate;
};

// a wavefront per env, four to a workgroup, striding over the envs (the four wavefronts of a workgroup make the same
// number of rounds: the barriers round the LDS histogram are uniform)
__global__ __launch_bounds__(256) void k_trips(const Dev d, const TripEdges ed, const int n_bins, int *cursor,
                                               const TripOut o) {
  __shared__ int s_hist[4][TRIP_BINS];
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int cap = d.trip_cap;
  const bool binned = o.hist != nullptr;

  for (long base = (long)blockIdx.x * 4; base < d.E; base += (long)gridDim.x * 4) {
    const long env = base + wv;
    const bool live = env < d.E;
    int n = 0, c = 0;
    if (live) {
      n = d.n_trips[env];
      c = cursor ? cursor[env] : 0;
      if (c < 0 || c > n) c = 0;  // a log shorter than its cursor was cleared: read it from the start
    }
    const int lo = c < cap ? c : cap;
    const int hi = n < cap ? n : cap;
    if (binned) {
      if (lane < TRIP_BINS) s_hist[wv][lane] = 0;
      __syncthreads();
    }
    long long sum = 0;
    int mx = 0;
    if (live) {
      const float *log = d.trip_times + (size_t)env * cap;
      for (int i = lo + lane; i < hi; i += 64) {
        const int t = (int)(log[i] * 2.0f);
        sum += t;
        mx = t > mx ? t : mx;
        if (binned && t >= ed.e[0]) {
          int b = 0;
          bool in = false;
#pragma unroll
          for (int k = 1; k <= TRIP_BINS; ++k) {
            if (k < n_bins) b += t >= ed.e[k] ? 1 : 0;
            if (k == n_bins) in = t < ed.e[k];
          }
          if (in) atomicAdd(&s_hist[wv][b], 1);
        }
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      sum += __shfl_xor(sum, off, 64);
      const int q = __shfl_xor(mx, off, 64);
      mx = q > mx ? q : mx;
    }
    if (binned) __syncthreads();
    if (live) {
      const int cnt = hi > lo ? hi - lo : 0;
      const int lost = (n > cap ? n : cap) - (c > cap ? c : cap);
      if (binned && lane < n_bins) {
        int *hp = o.hist + (size_t)env * n_bins + lane;
        *hp = o.accumulate ? *hp + s_hist[wv][lane] : s_hist[wv][lane];
      }
      if (lane == 0) {
        if (o.accumulate) {
          if (o.count) o.count[env] += cnt;
          if (o.tick_sum) o.tick_sum[env] += sum;
          if (o.tick_max) {
            const int old = o.tick_max[env];
            o.tick_max[env] = mx > old ? mx : old;
          }
          if (o.lost) o.lost[env] += lost;
        } else {
          if (o.count) o.count[env] = cnt;
          if (o.tick_sum) o.tick_sum[env] = sum;
          if (o.tick_max) o.tick_max[env] = mx;
          if (o.lost) o.lost[env] = lost;
        }
        if (cursor) cursor[env] = n;
      }
    }
    if (binned) __syncthreads();  // the next round clears the histogram
  }
}

}  // namespace tfx
