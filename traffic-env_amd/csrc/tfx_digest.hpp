// tfx_digest.hpp - k_digest: 64-bit fingerprints of chosen envs' states, one word per env and optionally one per road
// (tfx_state_digest, include/tfx.h, which states the rule).  "Are these two env states the same bits?" answered on the
// device by one read-only pass, instead of an export of every car and a comparison on the host.
//
// Read-only, on the shared walk of the road kernels (tfx_walk.hpp) over the n_sel * G (selected env, tile) items, a
// wavefront per item, four to a workgroup, lane per road - k_cars' launch.  What is new:
//   * The hot path is integer: per car one or two splitmix64 finalisers (dg_mix: two 64-bit multiplies, three shifts
//     and xors each) over the car's bit patterns, keyed by its place from the head.  The key (2j + 1) * G advances by an
//     add per car, so the multiplies of the rule's keys never run.  A lane keeps one 64-bit running sum; there is no LDS.
//   * FORM picks the walk (uniform over the launch, so an instantiation each): 0 - no car row is loaded, only the ring
//     words (or nothing of the roads at all); 1 - (x, v) pairs; 2 - (x, v) pairs and the B word of a car (row, spawn
//     tick), with the side plane where the handle has one and the parts need it; 3 - the B word alone: the walk over the
//     side plane only, or over no plane where the B word is 0 for every car.
//   * Every combination is a wrapping 64-bit sum, so no order matters: the lanes of a wavefront are summed by a butterfly
//     of __shfl_xor on the two halves, and one lane adds the wavefront's share to env_digest[s] with one 64-bit atomic
//     add - the host zeroed the words on the same stream.  Which wavefront arrives first changes nothing.
//   * The wavefront of tile 0 of a selection also takes the env's words (lights, counters, rewards), lanes striding over
//     I and r.
//   * Of an id outside [0, E) nothing of the handle's state is read; its env word keeps the memset's 0 and its road words
//     are stored as 0, as are those of masked-out roads.
#pragma once
#include "tfx_common.hpp"
#include "tfx_walk.hpp"

namespace tfx {

constexpr unsigned long long DG_G = 0x9e3779b97f4a7c15ull;
constexpr int DG_ROAD_PARTS = TFX_DIGEST_CARS | TFX_DIGEST_ROWS | TFX_DIGEST_SPAWN | TFX_DIGEST_RING;
constexpr int DG_ALL_PARTS = DG_ROAD_PARTS | TFX_DIGEST_LIGHTS | TFX_DIGEST_OBS;

struct DigestArgs {
  const int *env_ids;               // [n_sel] on the device; null: selection s is env s
  const uint8_t *road_mask;         // [R] on the device; null: every road
  int n_sel;
  int parts;                        // TFX_DIGEST_* bits
  unsigned long long *env_digest;   // [n_sel], zeroed by the host on the launch's stream
  unsigned long long *road_digest;  // [n_sel][R] or null
};

// the splitmix64 finaliser
__device__ __forceinline__ unsigned long long dg_mix(unsigned long long z) {
  z ^= z >> 30;
  z *= 0xbf58476d1ce4e5b9ull;
  z ^= z >> 27;
  z *= 0x94d049bb133111ebull;
  z ^= z >> 31;
  return z;
}

// the term of 32-bit value `val` at index i of section s (1..8) of the env's words
__device__ __forceinline__ unsigned long long dg_word(int s, int i, unsigned val) {
  return dg_mix(((unsigned long long)s << 56) | ((unsigned long long)(unsigned)i << 32) | val);
}

// the sum of a 64-bit value over the wavefront's lanes (wrapping), in every lane
__device__ __forceinline__ unsigned long long dg_wave_sum(unsigned long long t) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)t, m, 64);
    const unsigned hi = (unsigned)__shfl_xor((int)(unsigned)(t >> 32), m, 64);
    t += ((unsigned long long)hi << 32) | lo;
  }
  return t;
}

// a wavefront per (selected env, tile), four to a workgroup, striding over the n_sel * G items
template <int FORM>
__global__ __launch_bounds__(256) void k_digest(const Dev d, const DigestArgs a) {
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int G = d.G, R = d.R;
  const long items = (long)a.n_sel * G;
  const long nw = (long)gridDim.x * 4;
  const int parts = a.parts;
  const bool roads_on = (parts & DG_ROAD_PARTS) != 0;
  const bool rows_on = (parts & TFX_DIGEST_ROWS) != 0 && d.het;  // a single-archetype car's row is 0
  const bool spawn_on = (parts & TFX_DIGEST_SPAWN) != 0;
  const bool want_side = d.w != nullptr && (rows_on || spawn_on);

  for (long item = (long)blockIdx.x * 4 + wv; item < items; item += nw) {
    const int s = (int)(item / G);
    const int g = (int)(item - (long)s * G);
    const int env = a.env_ids ? a.env_ids[s] : s;
    const bool shown = env >= 0 && env < d.E;  // (uniform)
    const int e_slot = d.slot_road[g * 64 + lane];
    unsigned long long *rd = (a.road_digest && e_slot >= 0) ? a.road_digest + ((size_t)s * R + e_slot) : nullptr;
    if (!shown || !roads_on) {
      // not one of the handle's envs, or no part of the roads is asked for: the road words are 0 and no road term enters
      if (rd) *rd = 0ull;
      if (!shown) continue;
    }

    unsigned long long term = 0ull;  // the lane's share of the env word
    if (roads_on) {
      TileRoad r = tile_road(d, env, g, lane);
      if (r.live && a.road_mask && a.road_mask[r.e_slot] == 0) {
        r.live = false;  // masked out: no row of the road is loaded
        r.n = 0;
      }
      unsigned long long sum = dg_mix(1ull + (unsigned long long)r.n);
      if (parts & TFX_DIGEST_RING) sum += dg_mix((2ull << 56) | (unsigned long long)(unsigned)r.leading);
      unsigned long long key = DG_G;  // (2j + 1) * G of the lane's next car
      if (FORM == 1) {
        walk_cars<2, false, false>(d, r, lane, false, [&](bool, f2v c, float) {
          sum += dg_mix(((unsigned long long)__float_as_uint(c.x) | ((unsigned long long)__float_as_uint(c.y) << 32)) + key);
          key += 2ull * DG_G;
        });
      } else if (FORM == 2) {
        walk_cars<2, true, false>(d, r, lane, want_side, [&](bool, f2v c, float sw) {
          const unsigned sp = spawn_on ? __float_as_uint(side_tick(d, sw)) : 0u;
          const unsigned row = rows_on ? (unsigned)side_arch(sw) : 0u;
          sum += dg_mix(((unsigned long long)__float_as_uint(c.x) | ((unsigned long long)__float_as_uint(c.y) << 32)) + key);
          sum += dg_mix(((unsigned long long)sp | ((unsigned long long)row << 32)) + (key + DG_G));
          key += 2ull * DG_G;
        });
      } else if (FORM == 3) {
        walk_cars<0, true, false>(d, r, lane, want_side, [&](bool, f2v, float sw) {
          const unsigned sp = spawn_on ? __float_as_uint(side_tick(d, sw)) : 0u;
          const unsigned row = rows_on ? (unsigned)side_arch(sw) : 0u;
          sum += dg_mix(((unsigned long long)sp | ((unsigned long long)row << 32)) + (key + DG_G));
          key += 2ull * DG_G;
        });
      }
      if (rd) *rd = r.live ? sum : 0ull;
      if (r.live) term = dg_mix(sum + (unsigned long long)(r.e_slot + 1) * DG_G);
    }

    if (g == 0 && (parts & (TFX_DIGEST_LIGHTS | TFX_DIGEST_OBS))) {
      // the env's words: obs is passed | detected | current_phase | elapsed
      const int *ob = d.obs + (size_t)env * d.obs_len;
      const int I = d.I, nr = d.r;
      if (parts & TFX_DIGEST_LIGHTS) {
        for (int i = lane; i < I; i += 64) {
          term += dg_word(1, i, (unsigned)ob[2 * nr + i]);
          term += dg_word(2, i, (unsigned)ob[2 * nr + I + i]);
        }
      }
      if (parts & TFX_DIGEST_OBS) {
        for (int i = lane; i < nr; i += 64) {
          term += dg_word(3, i, (unsigned)ob[i]);
          term += dg_word(4, i, (unsigned)ob[nr + i]);
          term += dg_word(5, i, (unsigned)d.waiting[(size_t)env * nr + i]);
        }
        for (int i = lane; i < I; i += 64) {
          term += dg_word(6, i, (unsigned)d.passed_dst[(size_t)env * I + i]);
          term += dg_word(7, i, __float_as_uint(d.rewards[(size_t)env * I + i]));
        }
        if (lane == 0) term += dg_word(8, 0, (unsigned)d.done_tick[env]);
      }
    }

    const unsigned long long total = dg_wave_sum(term);
    if (lane == 0 && total != 0ull) atomicAdd(a.env_digest + s, total);
  }
}

}  // namespace tfx
