// tfx_demand.hpp - k_demand: the arrivals of rule 4 of include/tfx.h (tfx_set_demand) - time-varying, per-env, weighted,
// a true per-tick Poisson process - for n_ticks consecutive clock ticks of every env in ONE launch.
//
// The cars of an env in a tick are a pure function of (seed, stream id, clock tick) and two small threshold tables, so
// the (tick row, env) items share nothing: where k_poisson (tfx_misc.hpp) walks a serial chain per env - a gap decides
// where the next car falls - this kernel has n_ticks * E independent items.  Decomposition:
//   * a wavefront per item, four to a workgroup, a stride loop over the items (item_grid, tfx_launch.hpp);
//   * the car count N of the item: one Philox block for the whole wavefront (every lane computes it: no LDS, no
//     broadcast), lane l compares it with thresholds l, l + 64, ... of the item's count_cdf row (at most four: n_cdf <=
//     256) and the ballots' population counts add up to N = #{c <= n_cdf - 2 : u0 >= count_cdf[c]};
//   * N == 0, or a profile outside [0, K): the row is zeros, nothing else is read;
//   * otherwise the item's road_cdf row and an n_entry histogram sit in the wavefront's slice of the dynamic LDS; lane l
//     takes cars l, l + 64, ...: car c draws word c & 3 of Philox block c >> 2 (four neighbouring lanes evaluate the
//     same block - a car costs one block either way, and no cross-lane traffic) and finds its entry road by a binary
//     search over the row - the rows are non-decreasing (tfx_set_demand checks), so the first j with w < road_cdf[j] IS
//     #{j <= n_entry - 2 : w >= road_cdf[j]} - then one integer LDS atomic; the order of the adds cannot matter;
//   * the row leaves coalesced, lane j to word j.
// Comparisons and integer adds only: the host mirror (gym_traffic/devrng.py demand_counts) and any sharding of the envs
// over handles agree with it to the bit.  Inside tfx_step / tfx_agent_step the clock is read on the device (use_clock),
// which keeps the launch capturable; the preview (tfx_demand_counts) names its first tick.  Nothing but `out` is written.
//
// k_demand<true> (tfx_set_demand_mixed, rule 5): the archetype row of every car as well, into rows_out
// [n_ticks][E][n_entry][S].  Same decomposition; the cars go 64 at a time in car-index order (every lane of the wavefront
// takes every round, so the barriers inside are uniform), and a car adds
//   * its rank j on its road: the road's histogram value BEFORE the round's adds plus the lower lanes of the round with
//     the same ej - a ballot per distinct road of the round, v_mbcnt of the mask; a wavefront fence/barrier between the
//     round's reads of the histogram and its adds, another before the next round reads.  That is car-index order exactly;
//   * its row: one more Philox block per four cars (TAG_DROW), a count over the n_rows - 1 thresholds of the item's
//     row_cdf row - the same address in every lane;
//   * one byte store, if j < S.  Bytes past a road's min(count, S) are never written; an item of no cars writes none.
// The LDS slice is the one the counts need.  Nothing but `out` and `rows_out` is written.
#pragma once
#include "tfx_common.hpp"
#include "tfx_misc.hpp"

namespace tfx {

constexpr unsigned TAG_DCNT = 0x44434E54u;   // rule 4 of include/tfx.h: the car count of (tick, stream id)
constexpr unsigned TAG_DROAD = 0x44524F44u;  // ... and the entry roads of its cars
constexpr unsigned TAG_DROW = 0x44524F57u;   // rule 5: the archetype rows of its cars
constexpr int DEMAND_MAX_PROFILES = 16, DEMAND_MAX_SEGMENTS = 64, DEMAND_MAX_CDF = 256;
// road_cdf row + histogram of four wavefronts within the 64 KB every kernel has without asking
constexpr int DEMAND_MAX_ENTRY = 2048;

struct DemandDev {
  const unsigned *count_cdf;  // [K][S][n_cdf]
  const unsigned *road_cdf;   // [K][S][n_entry]
  const unsigned *sid;        // [E] stream ids (env + env_id_offset until a clone with TFX_CLONE_STREAM)
  const int *profile;         // [E] the caller's, read when the arrivals are drawn; null: profile 0 everywhere
  int K, S, seg_ticks, tick_offset, n_cdf;
  unsigned seed_lo, seed_hi;
};

// rule 5: what k_demand<true> reads besides (tfx_set_demand_mixed); row_cdf == nullptr: a plain demand
struct DemandRows {
  const unsigned *row_cdf;  // [K][S][n_rows]
  int n_rows;               // the handle's n_archetypes
  int S;                    // rows kept per road and tick: min(C - 2, n_cdf - 1)
};

// segment of clock tick t: floormod(t + tick_offset, P) / seg_ticks in 64 bits (P = S * seg_ticks fits an int32)
__device__ __forceinline__ int demand_segment(const DemandDev &dm, int t) {
  const long long P = (long long)dm.S * dm.seg_ticks;
  long long r = ((long long)t + dm.tick_offset) % P;
  if (r < 0) r += P;
  return (int)(r / dm.seg_ticks);
}

// out [n_ticks][E][n_entry]; row i holds clock tick (use_clock ? *d.tickA : tick0) + i.  ROWS: rows_out as well
template <bool ROWS>
__global__ __launch_bounds__(256) void k_demand(const Dev d, const DemandDev dm, const int use_clock, const int tick0,
                                                const int n_ticks, int *out, const DemandRows dr, uint8_t *rows_out) {
  extern __shared__ __attribute__((aligned(16))) unsigned s_dm[];  // per wavefront: road_cdf row | histogram
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int ne = d.n_entry;
  unsigned *s_cdf = s_dm + (size_t)wv * 2 * ne;
  int *s_hist = (int *)(s_cdf + ne);
  const unsigned first = (unsigned)(use_clock ? *d.tickA : tick0);
  const long items = (long)n_ticks * d.E;
  const long nw = (long)gridDim.x * 4;

  for (long item = (long)blockIdx.x * 4 + wv; item < items; item += nw) {
    const int row = (int)(item / d.E);
    const int env = (int)(item - (long)row * d.E);
    const int t = (int)(first + (unsigned)row);  // (the clock is an int32 that wraps)
    int *dst = out + (size_t)item * ne;
    const int k = dm.profile ? dm.profile[env] : 0;
    int N = 0, s = 0;
    unsigned g = 0;
    if (k >= 0 && k < dm.K) {  // (uniform over the wavefront, like everything up to the cars)
      s = demand_segment(dm, t);
      g = dm.sid[env];
      unsigned u[4];
      philox4x32((unsigned)t, g, TAG_DCNT, 0u, dm.seed_lo, dm.seed_hi, u);
      const unsigned *cc = dm.count_cdf + ((size_t)k * dm.S + s) * dm.n_cdf;
      for (int c0 = 0; c0 < dm.n_cdf - 1; c0 += 64) {
        const int c = c0 + lane;
        const bool over = c < dm.n_cdf - 1 && u[0] >= cc[c];
        N += __builtin_popcountll(__builtin_amdgcn_ballot_w64(over));
      }
    }
    if (N == 0) {
      for (int j = lane; j < ne; j += 64) dst[j] = 0;
      continue;
    }
    const unsigned *rc = dm.road_cdf + ((size_t)k * dm.S + s) * ne;
    for (int j = lane; j < ne; j += 64) {
      s_cdf[j] = rc[j];
      s_hist[j] = 0;
    }
    // the slice changes hands: written lane by lane, read and added to by whichever lane a car falls to
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if constexpr (ROWS) {
      const unsigned *rw = dr.row_cdf + ((size_t)k * dm.S + s) * dr.n_rows;
      uint8_t *rdst = rows_out + (size_t)item * ne * dr.S;
      for (int c0 = 0; c0 < N; c0 += 64) {  // (uniform: every lane takes every round)
        const int c = c0 + lane;
        const bool car = c < N;
        const int q = c & 3;
        int ej = -1, before = 0, row = 0;
        if (car) {
          unsigned u[4];
          philox4x32((unsigned)t, g, TAG_DROAD, (unsigned)(c >> 2), dm.seed_lo, dm.seed_hi, u);
          const unsigned w = q == 0 ? u[0] : (q == 1 ? u[1] : (q == 2 ? u[2] : u[3]));
          int lo = 0, hi = ne - 1;
          while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (w >= s_cdf[mid]) lo = mid + 1;
            else hi = mid;
          }
          ej = lo;
          before = s_hist[ej];  // the cars of the rounds before on this road
          philox4x32((unsigned)t, g, TAG_DROW, (unsigned)(c >> 2), dm.seed_lo, dm.seed_hi, u);
          const unsigned v = q == 0 ? u[0] : (q == 1 ? u[1] : (q == 2 ? u[2] : u[3]));
          for (int i = 0; i < dr.n_rows - 1; ++i) row += v >= rw[i] ? 1 : 0;
        }
        // the lower lanes of the round on the same road: a ballot per distinct road, the first lane left names it
        int lower = 0;
        for (unsigned long long left = __builtin_amdgcn_ballot_w64(car); left;) {
          const int e = __builtin_amdgcn_readlane(ej, __builtin_ctzll(left));
          const unsigned long long same = __builtin_amdgcn_ballot_w64(ej == e);
          if (ej == e) lower = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(same >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)same, 0u));
          left &= ~same;
        }
        // every lane has read the histogram before any lane adds to it ...
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (car) {
          atomicAdd(&s_hist[ej], 1);
          const int j = before + lower;
          if (j < dr.S) rdst[(size_t)ej * dr.S + j] = (uint8_t)row;
        }
        // ... and the adds are in before the next round reads it
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      }
    } else {
      for (int c = lane; c < N; c += 64) {
        unsigned u[4];
        philox4x32((unsigned)t, g, TAG_DROAD, (unsigned)(c >> 2), dm.seed_lo, dm.seed_hi, u);
        const int q = c & 3;
        const unsigned w = q == 0 ? u[0] : (q == 1 ? u[1] : (q == 2 ? u[2] : u[3]));
        // first j in [0, ne - 1] with w < s_cdf[j], ne - 1 when there is none (the last threshold is not compared)
        int lo = 0, hi = ne - 1;
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (w >= s_cdf[mid]) lo = mid + 1;
          else hi = mid;
        }
        atomicAdd(&s_hist[lo], 1);
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    for (int j = lane; j < ne; j += 64) dst[j] = s_hist[j];
    // ... and back, before the next item's lanes fill the slice
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
}

}  // namespace tfx
