// tfx_cars.hpp - k_cars: every live car of chosen envs as one flat run (tfx_car_list, include/tfx.h) - the cars of
// (selected env s, road e) at offsets[s * R + e] .. offsets[s * R + e + 1], head first, as (x, v) pairs with the planes
// that go with them: the road key s * R + e, the archetype row and the spawn tick.  Where k_ends lists at most K cars a
// road into a dense [E][R][K] block, this one compacts all of them into the ragged (CSR) list the caller's offsets
// describe.
//
// Read-only, on the shared walk of the road kernels (tfx_walk.hpp) over the n_sel * G (selected env, tile) items: the
// (x, v) plane and - only where `row` (heterogeneous handles) or `spawn` is wanted - the side plane.
//   * The env of an item comes from a device array (env_ids[s]) as in k_frames; of an id outside [0, E) nothing of the
//     handle's state is read and nothing is stored.  A road whose mask byte is 0 is handed to the walk without cars: none
//     of its rows is loaded.
//   * A lane storing its own car to offsets[road] + j would scatter the 64 eight-byte stores of a row over 64 runs.  So the
//     walk runs in its uniform form, the wavefront in lockstep, and every lane appends its cars of a block of WALK_P
//     visits to the wavefront's [WALK_P][64] LDS planes - (x, v) pairs and side words - at row u = cars it has in the
//     block so far, rotated as k_ends rotates its rows (ends_word<8>).  A lane writes only its own column: no atomics.
//   * After every block of WALK_P visits, and after the last partial one, the lanes run over (road of the tile, u) pairs:
//     the road's block count, the rank of its first car of the block, its base offset and its run length come across the
//     wavefront by __shfl, and the up to 8 cars a road has in the block leave as one contiguous 64-byte run of xv with the
//     matching runs of the other planes.  Rounds of the pass in which no road has a car are skipped (uniform).
//   * Memory safety does not rest on the caller's offsets: entry j of road key k is stored only if
//     j < offsets[k + 1] - offsets[k] and offsets[k] + j lies in [0, cap).  Offsets that do not match the counts lose or
//     overlap cars; they never send a store outside the planes.  A plane whose pointer is null is skipped everywhere.
//   * Nothing is computed: (x, v) is moved bit for bit, the row is the low bits of the side word, the spawn tick is what
//     tfx_export_ring writes to ring_w (side_tick).
// LDS: 4 wavefronts x (4 KB + 2 KB) = 24 KB per workgroup; no workgroup barrier, no cross-workgroup traffic.
#pragma once
#include "tfx_common.hpp"
#include "tfx_ends.hpp"
#include "tfx_walk.hpp"

namespace tfx {

struct CarsArgs {
  const int *env_ids;        // [n_sel] on the device; null: selection s is env s
  const uint8_t *road_mask;  // [R] on the device; null: every road
  const int *offsets;        // [n_sel * R + 1] on the device
  int n_sel;
  int cap;                   // entries the planes hold
  f2v *xv;                   // [cap] (x, v); any plane null = not wanted
  int *road;                 // [cap] s * R + road id
  uint8_t *row;              // [cap] archetype row
  float *spawn;              // [cap] spawn tick
};

// a wavefront per (selected env, tile), four to a workgroup, striding over the n_sel * G items
__global__ __launch_bounds__(256) void k_cars(const Dev d, const CarsArgs a) {
  __shared__ f2v s_xv[4][WALK_P * 64];
  __shared__ float s_sw[4][WALK_P * 64];
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int G = d.G, R = d.R;
  const long items = (long)a.n_sel * G;
  const long nw = (long)gridDim.x * 4;
  const bool want_xv = a.xv != nullptr;
  const bool want_side = d.w != nullptr && ((d.het && a.row != nullptr) || a.spawn != nullptr);
  f2v *pxv = s_xv[wv];
  float *psw = s_sw[wv];

  for (long item = (long)blockIdx.x * 4 + wv; item < items; item += nw) {
    const int s = (int)(item / G);
    const int g = (int)(item - (long)s * G);
    const int env = a.env_ids ? a.env_ids[s] : s;
    if (env < 0 || env >= d.E) continue;  // (uniform) not one of the handle's envs: no cars
    TileRoad r = tile_road(d, env, g, lane);
    if (r.live && a.road_mask && a.road_mask[r.e_slot] == 0) {
      r.live = false;  // masked out: no row of the road is loaded
      r.n = 0;
    }
    // the road's run in the planes, from the caller's offsets: base and length bound every store below
    const int key = s * R + (r.e_slot >= 0 ? r.e_slot : 0);
    int base = 0, len = 0;
    if (r.n > 0) {
      base = a.offsets[key];
      const long run = (long)a.offsets[key + 1] - base;  // whatever the two words hold: 0 .. the road's count
      len = run < 0 ? 0 : (run > r.n ? r.n : (int)run);
    }

    int j0 = 0;      // rank of the lane's first car of the block
    int cnt = 0;     // cars the lane has in the block
    int visits = 0;  // (uniform) visits of the block so far

    // the block leaves: lanes run over (road of the tile, u) pairs, a road's cars of the block are one contiguous run
    auto flush = [&]() __attribute__((always_inline)) {
      // the planes change hands: written per lane, read per (road, u) pair
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      for (int it = 0; it < WALK_P; ++it) {
        const int rl = it * (64 / WALK_P) + lane / WALK_P;  // the tile's road ...
        const int u = lane % WALK_P;                        // ... and its car of the block
        const int cnt_r = __shfl(cnt, rl, 64);
        const int j = __shfl(j0, rl, 64) + u;
        const int len_r = __shfl(len, rl, 64);
        const long at = (long)__shfl(base, rl, 64) + j;
        const int key_r = __shfl(key, rl, 64);
        const bool mine = u < cnt_r && j < len_r && at >= 0 && at < (long)a.cap;
        if (__builtin_amdgcn_ballot_w64(mine) == 0ull) continue;  // (uniform) no road of this round has a car
        if (mine) {
          const int word = ends_word<WALK_P>(u, rl);
          if (want_xv) a.xv[at] = pxv[word];
          if (a.road) a.road[at] = key_r;
          if (want_side) {
            const float sw = psw[word];
            if (a.row) a.row[at] = (uint8_t)(d.het ? side_arch(sw) : 0);
            if (a.spawn) a.spawn[at] = side_tick(d, sw);
          } else if (a.row) {
            a.row[at] = 0;
          }
        }
      }
      // ... and back, before the lanes fill them with the next block
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      j0 += cnt;
      cnt = 0;
      visits = 0;
    };

    walk_cars<2, true, true>(d, r, lane, want_side, [&](bool mine, f2v c, float sw) {
      if (mine) {
        const int word = ends_word<WALK_P>(cnt, lane);
        if (want_xv) pxv[word] = c;
        if (want_side) psw[word] = sw;
        ++cnt;
      }
      if (++visits == WALK_P) flush();
    });
    if (visits > 0) flush();
  }
}

}  // namespace tfx
