// tfx_frames.hpp - k_frames: top-view RGBA frames of chosen envs (tfx_frames, include/tfx.h) from ONE read of their live
// cars.  Read-only like k_measure and k_cells, and on their walk (tfx_walk.hpp) over the n_frames * G (frame, tile)
// items: x of every car and, in heterogeneous handles, its side word.
//
// What is new:
//   * The env of an item comes from a device array (env_ids[frame]); for an id outside [0, E) nothing of the handle's
//     state is read: the item is skipped and its frame keeps the background the memset gave it - or, roads only, where
//     no memset ran, its road pixels are painted white.
//   * A lane keeps its road's occupancy - one bit per pixel the road owns, S - 3 <= 253 of them - as a bitset in LDS,
//     [word][lane] per wavefront (8 x 64 words = 2 KB); it touches only its own column of them, so there are no
//     atomics.  A car sets bits b .. a (the definition's clamped floors): usually one word, never more than eight.
//   * After a tile the lanes run over (road, pixel) pairs: every pixel a road owns is stored ONCE with its final value
//     - the car colour where the bit is set, the road's light colour otherwise - as a full 32-bit store.  Roads that run
//     along an image row leave as contiguous runs of dwords; roads that run down a column are strided stores.  Start
//     pixel, step and colour are per-road values the lanes hold in registers and read across the wavefront.
//   * Heterogeneous handles read the side-word plane next to the cars: the car's table row is in its low 6 bits, its
//     length in the table (a workgroup's LDS copy).
#pragma once
#include "tfx_common.hpp"
#include "tfx_walk.hpp"

namespace tfx {

constexpr int FRAME_WORDS = 8;  // (TFX_FRAME_PX_MAX - 3 + 31) / 32
static_assert(FRAME_WORDS * 32 >= TFX_FRAME_PX_MAX - 3, "a road's pixels fit its bitset");
// bytes R, G, B, A of a pixel, as the little-endian word a lane stores
constexpr unsigned PX_GREEN = 0xFF00FF00u, PX_RED = 0xFF0000FFu, PX_YELLOW = 0xFF00FFFFu, PX_CAR = 0xFFFF0000u,
                   PX_WHITE = 0xFFFFFFFFu;

struct FrameArgs {
  const int *env_ids;  // [n_frames] on the device; null: frame f shows env f
  unsigned *out;       // [n_frames][H][W] pixels
  int n_frames;
  int roads_only;      // TFX_FRAMES_ROADS_ONLY: no memset ran, the frames hold an earlier call's picture
  int m, n, S, W, H;
  float k;             // float32(S - 3) / float32(length): pixels a road owns per unit of x
};

// index, within a frame, of the pixel at t = 0 of road e, and the step to the pixel at t + 1 (include/tfx.h)
__device__ __forceinline__ void frame_road(const FrameArgs &f, const int e, int &start, int &step) {
  const int m = f.m, n = f.n, v = m * n, S = f.S, W = f.W;
  int row, col, dir;  // the intersection the road runs into (train roads) or away from (exit roads)
  bool exit_road = false;
  if (e < 4 * v) {
    dir = e / v;
    const int c = e - dir * v;
    row = c / n;
    col = c - row * n;
  } else {
    // the four exit blocks, in GridRoad._unit_segments' order: each continues the train roads of one direction
    const int q = e - 4 * v;
    exit_road = true;
    if (q < n) { dir = 3; row = 0; col = q; }
    else if (q < n + m) { dir = 0; row = q - n; col = n - 1; }
    else if (q < 2 * n + m) { dir = 2; row = m - 1; col = q - n - m; }
    else { dir = 1; row = q - 2 * n - m; col = 0; }
  }
  const int cx = (col + 1) * S, cy = (row + 1) * S;
  const int back = exit_road ? 0 : S;  // a train road starts S pixels before the centre, an exit road at the centre
  int sx, sy, dx, dy;
  switch (dir) {
    case 0: sx = cx - back; sy = cy - 1; dx = 1; dy = 0; break;
    case 1: sx = cx + back; sy = cy + 1; dx = -1; dy = 0; break;
    case 2: sx = cx + 1; sy = cy - back; dx = 0; dy = 1; break;
    default: sx = cx - 1; sy = cy + back; dx = 0; dy = -1; break;
  }
  start = sy * W + sx;
  step = dy * W + dx;
}

// clamp(floorf(t), 0, top) in float, before the conversion (a NaN gives 0)
__device__ __forceinline__ int frame_pixel(const float t, const float top) {
  const float fl = floorf(t);
  return (int)(!(fl >= 0.0f) ? 0.0f : (fl > top ? top : fl));
}

// a car at x of length l sets bits b .. a of the lane's column of the wavefront's bitset
__device__ __forceinline__ void frame_mark(unsigned *bits, const int lane, const float x, const float l, const float k,
                                           const float top) {
  if (x != x) return;  // a NaN x is not drawn
  const int a = frame_pixel(x * k, top);
  const int b = frame_pixel((x - l) * k, top);
  for (int w = b >> 5; w <= (a >> 5); ++w) {
    const int lo = w == (b >> 5) ? (b & 31) : 0, hi = w == (a >> 5) ? (a & 31) : 31;
    bits[w * 64 + lane] |= (0xFFFFFFFFu >> (31 - hi)) & (0xFFFFFFFFu << lo);
  }
}

// a wavefront per (frame, tile), four to a workgroup, striding over the n_frames * G items
__global__ __launch_bounds__(256) void k_frames(const Dev d, const FrameArgs f) {
  __shared__ unsigned s_bits[4][FRAME_WORDS * 64];
  __shared__ float s_arch[TFX_MAX_ARCH * ARCH_W];
  if (d.het) load_arch(d, s_arch);
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int G = d.G;
  const long items = (long)f.n_frames * G;
  const long nw = (long)gridDim.x * 4;
  const int npix = f.S - 3;                 // pixels a road owns: t = 2 .. S - 2
  const int nwords = (npix + 31) >> 5;
  const float top = (float)(npix - 1);
  const unsigned div = (unsigned)((0x100000000ull + (unsigned)npix - 1) / (unsigned)npix);  // p / npix == umulhi(p, div) for p * npix < 2^32
  const size_t frame_px = (size_t)f.H * f.W;
  unsigned *bits = s_bits[wv];

  for (long item = (long)blockIdx.x * 4 + wv; item < items; item += nw) {
    const int frame = (int)(item / G);
    const int g = (int)(item - (long)frame * G);
    const int env = f.env_ids ? f.env_ids[frame] : frame;
    // (uniform over the wavefront) An id outside [0, E): nothing of the handle's state is read, the frame is background -
    // what the memset left, or, roads only, its road pixels painted white over whatever an earlier call drew there
    const bool shown = env >= 0 && env < d.E;
    if (!shown && !f.roads_only) continue;
    const TileRoad r = tile_road(d, env, g, lane, shown);
    const int e_slot = r.e_slot;
    const bool valid = e_slot >= 0, live = r.live;

    // the road's light colour (update_colors, traffic_env.py:335-346), start pixel and step
    unsigned colour = shown ? PX_GREEN : PX_WHITE;
    int start = 0, step = 0;
    if (valid) frame_road(f, e_slot, start, step);
    if (live && e_slot < d.r) {
      const int dir = e_slot / d.I, i = e_slot - dir * d.I;
      const int *lw = d.lights + (size_t)env * d.lights_stride;
      const bool mine = ((dir < 2) ? 1 : 0) == lw[i];  // roadgraph.py:36
      const bool fresh = lw[d.I + i] < d.yellow;
      colour = mine ? (fresh ? PX_YELLOW : PX_RED) : (fresh ? PX_RED : PX_GREEN);
    }
    start += 2 * step;  // the first pixel the road owns

    for (int w = 0; w < nwords; ++w) bits[w * 64 + lane] = 0u;

    walk_cars<1, true, false>(d, r, lane, d.het, [&](bool, f2v c, float sw) {
      frame_mark(bits, lane, c.x, d.het ? s_arch[side_arch(sw) * ARCH_W + AR_L] : d.car_l, f.k, top);
    });

    // the bitset changes hands: written per lane, read per (road, pixel) pair
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const unsigned long long have = __builtin_amdgcn_ballot_w64(valid);
    const int total = (64 - __builtin_clzll(have | 1ull)) * npix;  // pairs up to the tile's last road
    unsigned *px = f.out + (size_t)frame * frame_px;
    for (int p0 = 0; p0 < total; p0 += 64) {
      const int p = p0 + lane;
      const int rl = (int)__umulhi((unsigned)p, div);  // the tile's road p / npix ...
      const int j = p - rl * npix;                     // ... and its pixel
      const int e_r = __shfl(e_slot, rl, 64);
      const int at = __shfl(start, rl, 64) + j * __shfl(step, rl, 64);
      const unsigned c_r = __shfl((int)colour, rl, 64);
      if (p < total && e_r >= 0) px[at] = ((bits[(j >> 5) * 64 + rl] >> (j & 31)) & 1u) ? PX_CAR : c_r;
    }
    // ... and back, before the next item's lanes clear it
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
}

}  // namespace tfx
