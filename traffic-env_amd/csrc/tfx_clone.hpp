// tfx_clone.hpp - k_clone: env e of a destination handle becomes a copy of env src_of_env[e] of a source handle
// (tfx_clone_envs, include/tfx.h): branch, snapshot and restore envs without leaving the device.
//
// The state of an env (DESIGN.md "What an env's state consists of") is G whole tiles of cars, a handful of words per
// road and a handful per env; envs share nothing (traffic_env.py:361-382).  One wavefront per (destination env, tile),
// lane per road as in k_move_t (tfx_move_t.hpp):
//   * the wavefront reads the env's source index (one word; -1: nothing else happens), checks the in-place rule, loads
//     the source roads' leading / lastcar / hb and reduces the tile's deepest live row;
//   * rows 0 .. kmax-1 of the source tile stream to the destination tile - 64 x 8 B per row, coalesced, non-temporal
//     (every byte is touched once), CLONE_P rows in flight; a lane moves the rows its own road has cars in and no others,
//     so a sparse env costs less than a full one; the side plane (spawn ticks / table rows) likewise, spawn ticks
//     rebased by the difference of the two handles' clocks;
//   * then the per-road words (ring indices, hb, the road records, tail and leader caches, the outbox rows);
//   * the per-env arrays (the obs row, rewards, waiting, ...) are spread over the env's G wavefronts, lane 0 of the
//     env's first tile writes the per-env scalars.
// Ring layout (tfx_config.layout = 0, the non-default one): the same decomposition, each lane copies the C slots of
// its road.
// k_clone<true> (PICK) is the masked restart of a decision with a pool of warmed-up envs attached (tfx_set_episode_pool,
// include/tfx.h): no index array - the wavefront reads the env's restart mark (none: it leaves on a wave-uniform branch,
// so a decision in which nobody restarts costs one nearly empty launch) and draws the pool env by rule 3; it also does
// k_episode_begin's other job, the `last` flags, so the decision makes no launch more than it makes without a pool.
// A source is never written by the launch that reads it: across handles because the handles differ, in place because an
// env whose source is itself a destination is left alone and counted (clone_plan in gym_traffic/devrng.py states the rule).
#pragma once
#include "tfx_common.hpp"
#include "tfx_misc.hpp"
#include "tfx_walk.hpp"

namespace tfx {

constexpr int CLONE_P = 8;  // rows in flight per wavefront

// what travels on request (TFX_CLONE_STREAM / TFX_CLONE_EPISODE) or when both handles have it; null / 0 = not copied
struct CloneOpt {
  int same;                          // dst == src: the in-place rule applies
  int stream;                        // the arrival stream's identity and position
  int *d_gap, *s_gap;                // PoissonDev::gap_left
  unsigned *d_draws, *s_draws;       // PoissonDev::draws
  unsigned *d_sid, *s_sid;           // PoissonDev::sid
  unsigned *d_seq, *s_seq;           // PoissonRows::seq [E][n_entry] (heterogeneous cars), or null
  int episode;                       // the running episode's accounting
  EpDev d_ep, s_ep;                  // (PICK: d_ep is the destination's block whatever `episode` says - mark, ep_index, last)
  int *d_greedy, *s_greedy;          // the greedy controller's held decision [E][I], or null
  unsigned long long *skipped;       // destination handle: envs left untouched against the caller's wish
};

// a tick stamp (tick + 1 of some past tick; 0 = never) under the destination's clock
// (a destination clock far behind the source's can take a stamp to 0 or below: every reader compares a stamp with the
// current clock - tick + 1 of a tick still to come, or "later than the decision began" - so such a stamp reads as
// what it is, one of a tick long past)
__device__ __forceinline__ int clone_stamp(int s, int dt) { return s ? s + dt : 0; }

// a side word under the destination's clock: the spawn tick moves by dt, the table row stays
__device__ __forceinline__ float clone_side(const Dev &d, float wa, int dt) {
  if (dt == 0) return wa;
  if (d.het) {
    const int b = __float_as_int(wa);
    // (unsigned: a spawn tick below 2^24 plus a clock difference up to TFX_TICK_MAX passes INT32_MAX; only the low 24 bits count)
    return side_pack((int)((unsigned)(b >> ARCH_BITS) + (unsigned)dt), b & (TFX_MAX_ARCH - 1));
  }
  // ONE rounding of spawn tick + dt, what a car spawned at that tick of the destination's clock holds ((float)tick).
  // (float)dt is exact up to 2^24; past it wa + (float)dt would round twice - a clock difference of 2^31 - 2^20 is a
  // multiple of 128 only by chance - and the sum of a float below 2^31 and an int32 is exact in binary64.
  const float fd = (float)dt;
  return (double)fd == (double)dt ? wa + fd : (float)((double)wa + (double)dt);
}

// words [0, n) of a per-env array, shared out over the env's G wavefronts
template <typename T>
__device__ __forceinline__ void clone_span(T *dst, const T *src, int n, int g, int G, int lane) {
  for (int i = g * 64 + lane; i < n; i += G * 64) dst[i] = src[i];
}

// may env `env` of the destination take source index s?  (wave-uniform)
__device__ __forceinline__ bool clone_allowed(const int *src_of_env, int env, int s, int E_src, bool same) {
  if (s < 0 || s >= E_src) return false;
  if (!same || s == env) return true;
  const int t = src_of_env[s];
  return t == -1 || t == s;
}

// PICK: the source of env `env` is `mark[env] ? rule 3 : -1` instead of src_of_env[env] (null then), sd the pool handle's
// block; reads mark, ep_len and ep_index and writes none of them
template <bool PICK>
__global__ __launch_bounds__(256) void k_clone(const Dev dd, const Dev sd, const int *src_of_env, const CloneOpt o) {
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int G = dd.G, R = dd.R, C = dd.C;
  const long items = (long)dd.E * G;
  const long nw = (long)gridDim.x * 4;
  const int dt = *dd.tickA - *sd.tickA;

  for (long item = (long)blockIdx.x * 4 + wv; item < items; item += nw) {
    const int env = (int)(item / G);
    const int g = (int)(item - (long)env * G);
    int s;
    if (PICK) {
      const EpDev &ep = o.d_ep;
      // (every env learns whether the decision under way is the last one its time limit allows, as in k_episode_begin)
      if (g == 0 && lane == 0) ep.last[env] = (ep.max > 0 && ep.ep_len[env] + 1 == ep.max) ? 1 : 0;
      if (__builtin_amdgcn_readfirstlane((int)ep.mark[env]) == 0) continue;
      s = __builtin_amdgcn_readfirstlane(episode_pool_slot(ep, env, (unsigned)(env + dd.env_off), sd.E));  // always in [0, sd.E)
    } else {
      s = __builtin_amdgcn_readfirstlane(src_of_env[env]);
      if (s == -1) continue;
      if (!clone_allowed(src_of_env, env, s, sd.E, o.same != 0)) {
        if (g == 0 && lane == 0) atomicAdd(o.skipped, 1ull);
        continue;
      }
      if (o.same && s == env) continue;  // a copy of itself
    }

    const int e_slot = dd.slot_road[g * 64 + lane];
    const bool valid = e_slot >= 0;
    const int e = valid ? e_slot : 0;
    const size_t did = (size_t)env * R + e, sid = (size_t)s * R + e;

    // ---- the cars ----------------------------------------------------------------------------------------
    const int ld = sd.leading[sid], lc = sd.lastcar[sid];
    if (dd.layout == 1) {
      const int hb = sd.hb[sid];
      int rows = valid ? ring_count(ld, lc, C) + hb : 0;  // rows of the column that hold (or lead up to) cars
      rows = rows < 0 ? 0 : (rows > dd.trows ? dd.trows : rows);
      const int kmax = wave_max(rows);
      const size_t scol = ((size_t)s * G + g) * (size_t)sd.trows * 64 + lane;
      const size_t dcol = ((size_t)env * G + g) * (size_t)dd.trows * 64 + lane;
      const f2v *sx = reinterpret_cast<const f2v *>(sd.xv + scol);
      f2v *dx = reinterpret_cast<f2v *>(dd.xv + dcol);
      const float *sw = sd.w ? sd.w + scol : nullptr;
      float *dw = dd.w ? dd.w + dcol : nullptr;
      for (int k0 = 0; k0 < kmax; k0 += CLONE_P) {
        f2v c[CLONE_P];
        float cw[CLONE_P];
#pragma unroll
        for (int u = 0; u < CLONE_P; ++u) {
          if (k0 + u < rows) {
            c[u] = __builtin_nontemporal_load(sx + (size_t)(k0 + u) * 64);
            if (sw) cw[u] = __builtin_nontemporal_load(sw + (size_t)(k0 + u) * 64);
          }
        }
#pragma unroll
        for (int u = 0; u < CLONE_P; ++u) {
          if (k0 + u < rows) {
            __builtin_nontemporal_store(c[u], dx + (size_t)(k0 + u) * 64);
            if (sw) __builtin_nontemporal_store(clone_side(dd, cw[u], dt), dw + (size_t)(k0 + u) * 64);
          }
        }
      }
      if (valid) {
        // the cars a road handed over in its last tick (read between move_cars and advance_finished_cars)
        const size_t so = ((size_t)s * G + g) * (size_t)KP * 64 + lane, dO = ((size_t)env * G + g) * (size_t)KP * 64 + lane;
#pragma unroll
        for (int j = 0; j < KP; ++j) {
          dd.outb[dO + (size_t)j * 64] = sd.outb[so + (size_t)j * 64];
          if (sw) dd.outw[dO + (size_t)j * 64] = clone_side(dd, sd.outw[so + (size_t)j * 64], dt);
        }
        dd.hb[did] = (uint8_t)hb;
        dd.rec2f[did] = sd.rec2f[sid];
        dd.rec2c[did] = sd.rec2c[sid];
        dd.crec[did] = sd.crec[sid];
        dd.ovf_cnt[did] = sd.ovf_cnt[sid];
        dd.rsw[did] = sd.rsw[sid];
      }
    } else if (valid) {
      const float2 *sx = sd.xv + sid * C;
      float2 *dx = dd.xv + did * C;
      for (int k = 0; k < C; ++k) dx[k] = sx[k];
      if (sd.w)
        for (int k = 0; k < C; ++k) dd.w[did * C + k] = clone_side(dd, sd.w[sid * C + k], dt);
    }

    // ---- the per-road words --------------------------------------------------------------------------------
    if (valid) {
      dd.leading[did] = ld;
      dd.lastcar[did] = lc;
      dd.rec[did] = sd.rec[sid];
      dd.tailx[did] = sd.tailx[sid];
      dd.leadx[did] = sd.leadx[sid];
      if (dd.het) dd.taila[did] = sd.taila[sid];
    }

    // ---- the per-env arrays, shared out over the env's wavefronts ----------------------------------------
    clone_span(dd.obs + (size_t)env * dd.obs_len, sd.obs + (size_t)s * sd.obs_len, dd.obs_len, g, G, lane);
    clone_span(dd.rewards + (size_t)env * dd.I, sd.rewards + (size_t)s * dd.I, dd.I, g, G, lane);
    clone_span(dd.waiting + (size_t)env * dd.r, sd.waiting + (size_t)s * dd.r, dd.r, g, G, lane);
    clone_span(dd.passed_dst + (size_t)env * dd.I, sd.passed_dst + (size_t)s * dd.I, dd.I, g, G, lane);
    if (o.d_greedy) clone_span(o.d_greedy + (size_t)env * dd.I, o.s_greedy + (size_t)s * dd.I, dd.I, g, G, lane);
    if (dd.n_trips && sd.n_trips && dd.trip_times && sd.trip_times) {
      int nt = sd.n_trips[s];
      nt = nt < sd.trip_cap ? nt : sd.trip_cap;
      nt = nt < dd.trip_cap ? nt : dd.trip_cap;
      clone_span(dd.trip_times + (size_t)env * dd.trip_cap, sd.trip_times + (size_t)s * sd.trip_cap, nt, g, G, lane);
    }
    if (o.stream && o.d_seq)
      clone_span(o.d_seq + (size_t)env * dd.n_entry, o.s_seq + (size_t)s * dd.n_entry, dd.n_entry, g, G, lane);
    if (o.episode)
      clone_span(o.d_ep.ep_return + (size_t)env * dd.I, o.s_ep.ep_return + (size_t)s * dd.I, dd.I, g, G, lane);

    // ---- the per-env scalars ---------------------------------------------------------------------------------
    if (g == 0 && lane == 0) {
      dd.done_tick[env] = clone_stamp(sd.done_tick[s], dt);
      // (stamps of past ticks: they stay as stale under the destination's clock as they are under the source's)
      dd.env_flag[env] = clone_stamp(sd.env_flag[s], dt);
      dd.env_risk[env] = clone_stamp(sd.env_risk[s], dt);
      dd.env_risk[(size_t)dd.risk_stride + env] = clone_stamp(sd.env_risk[(size_t)sd.risk_stride + s], dt);
      if (dd.n_trips && sd.n_trips) dd.n_trips[env] = sd.n_trips[s];
      if (o.stream) {
        o.d_gap[env] = o.s_gap[s];
        o.d_draws[env] = o.s_draws[s];
        o.d_sid[env] = o.s_sid[s];
      }
      if (o.episode) {
        o.d_ep.ep_len[env] = o.s_ep.ep_len[s];
        o.d_ep.ep_index[env] = o.s_ep.ep_index[s];
        o.d_ep.mark[env] = o.s_ep.mark[s];
      }
    }
  }
}

}  // namespace tfx
