// tfx_walk.hpp - the one walk of the live cars that the read-only road kernels share: k_measure (tfx_measure.hpp),
// k_cells (tfx_cells.hpp), k_ages (tfx_travel.hpp), k_frames (tfx_frames.hpp), k_follow (tfx_follow.hpp) and k_ends
// (tfx_ends.hpp, which cuts the walk short: it hands in a TileRoad whose count is clamped to its K).  Device only.
//
// The kernels take one wavefront per (env or frame, tile) item, four to a workgroup, striding over the items, lane per
// road as in k_move_t (tfx_move_t.hpp):
//   * tile_road: the lane of storage slot 64 * tile + j finds its road through slot_road and loads its leading /
//     lastcar; the count is clamped to [0, C-1].  Lanes past the last road of a partial tile hold no road (`live` false,
//     no cars), and so does every lane of an env that is not shown: of such an env nothing but slot_road is read.
//     Everything a lane knows of its item is in the TileRoad it gets here, so nothing carries over from one item of the
//     stride loop to the next.
//   * walk_cars, transposed layout: the wavefront reduces the tile's deepest live row, kmax (wave_max, which the move
//     kernels' tile walkers share: tfx_tile.hpp); rows 0 .. kmax-1 are walked as coalesced row loads (64 x 8 B of
//     (x, v), 64 x 4 B of side words), WALK_P rows in flight, default caching.  A lane loads rows hb <= k < hb + n of
//     its own column and no others - not the rows a two-tick pass left empty at the top of the column (hb,
//     tfx_move_tt.hpp), not the rows past the road's count - so a sparse env costs less than a full one.
//   * walk_cars, ring layout (tfx_config.layout = 0, the non-default one): each lane walks the ring slots of its road
//     from leading + 1 with wrap1.
//   * Either way `visit` sees a road's cars from the head to the tail: float32 sums taken in that order are
//     reproducible bit for bit and equal on both layouts.  The car visited just before a car is its leader: k_follow
//     carries that car's (x, v, l) from one visit to the next, in state of its own that lives outside the walk - the
//     walk keeps nothing between visits, neither across its blocks of WALK_P rows nor over the rows it skips.
#pragma once
#include "tfx_common.hpp"
#include "tfx_move_t.hpp"

namespace tfx {

constexpr int WALK_P = 8;  // rows in flight per wavefront

// what a lane knows of its road of an item
struct TileRoad {
  int e_slot;   // the slot's road id, -1: the slot holds no road
  bool live;    // a road of an env that is shown
  size_t id;    // [env][road id] - road 0 where the slot holds none; 0 if the env is not shown
  size_t tile;  // [env][tile]; tile g of env 0 if the env is not shown (no row of it is loaded)
  int leading;
  int n;        // live cars, 0 if not live
};

// shown = false: the env id is not one of the handle's (k_frames); uniform over the wavefront
__device__ __forceinline__ TileRoad tile_road(const Dev &d, int env, int g, int lane, bool shown = true) {
  TileRoad r;
  r.e_slot = d.slot_road[g * 64 + lane];
  r.live = r.e_slot >= 0 && shown;
  r.id = shown ? (size_t)env * d.R + (r.e_slot >= 0 ? r.e_slot : 0) : 0;
  r.tile = (size_t)(shown ? env : 0) * d.G + g;
  r.leading = shown ? d.leading[r.id] : 1;
  const int n = r.live ? ring_count(r.leading, d.lastcar[r.id], d.C) : 0;
  r.n = n < 0 ? 0 : (n > d.C - 1 ? d.C - 1 : n);
  return r;
}

// visit(live, xv, side word) for the cars of the lane's road, from the head to the tail.
//   XV         words of a car's (x, v) pair that are loaded: 0 (xv is never read), 1 (x only) or 2
//   SIDE       the side plane is loaded - where side_wanted says so too (uniform) - otherwise never read
//   UNIFORM    every lane of the wavefront calls visit together, as often as the tile's longest road has cars (and
//              empty rows above them), with live = false and zeros where it has no car: visit may use ballot and
//              __shfl.  Otherwise visit runs on lanes that have a car only.
// A plane that was not asked for reaches visit as 0.
template <int XV, bool SIDE, bool UNIFORM, class Visit>
__device__ __forceinline__ void walk_cars(const Dev &d, const TileRoad &r, int lane, bool side_wanted, Visit &&visit) {
  static_assert(XV >= 0 && XV <= 2, "words of (x, v)");
  const bool side = SIDE && side_wanted;
  // A word is zeroed ahead of the loads where visit can see it unloaded: every word in the uniform form (lanes without a
  // car) and with XV == 1 (the half pair, and the side word where side_wanted is false); a plane never asked for
  // otherwise.  Words that every visited car loads are not: the zero would only wait for the loads of the round before
  // (profiles/r06_query_walk.txt has the figures).  A side plane the template takes but side_wanted declines (k_follow on
  // a single-archetype handle) is zeroed as well.
  constexpr bool ZERO_XV = UNIFORM || XV != 2, ZERO_SIDE = UNIFORM || XV == 1 || !SIDE;
  if (d.layout == 1) {
    const int hb = r.live ? d.hb[r.id] : 0;  // rows a two-tick pass left empty at the top of the column
    const int rows = r.n + hb > d.trows ? d.trows : r.n + hb;
    const int kmax = wave_max(rows);
    const size_t at = r.tile * (size_t)d.trows * 64 + lane;
    const float2 *col = d.xv + at;
    const float *wcol = side ? d.w + at : nullptr;  // the side words travel with the cars
    for (int k0 = 0; k0 < kmax; k0 += WALK_P) {
      f2v c[WALK_P];
      float sw[WALK_P];
#pragma unroll
      for (int u = 0; u < WALK_P; ++u) {
        if (ZERO_XV) c[u] = f2v{0.0f, 0.0f};
        if (ZERO_SIDE || !side) sw[u] = 0.0f;
        if (k0 + u >= hb && k0 + u < rows) {
          if (XV == 2) c[u] = reinterpret_cast<const f2v *>(col)[(size_t)(k0 + u) * 64];
          if (XV == 1) c[u].x = col[(size_t)(k0 + u) * 64].x;
          if (side) sw[u] = wcol[(size_t)(k0 + u) * 64];
        }
      }
#pragma unroll
      for (int u = 0; u < WALK_P; ++u) {
        const bool mine = k0 + u >= hb && k0 + u < rows;
        if (UNIFORM ? k0 + u < kmax : mine) visit(mine, c[u], sw[u]);
      }
    }
  } else {
    const int nmax = UNIFORM ? wave_max(r.n) : r.n;
    int slot = r.leading;
    for (int k = 0; k < nmax; ++k) {
      f2v c{0.0f, 0.0f};
      float sw = 0.0f;
      const bool mine = k < r.n;
      if (mine) {
        slot = wrap1(slot + 1, d.C);
        const size_t at = r.id * d.C + slot;
        if (XV == 2) c = f2v{d.xv[at].x, d.xv[at].y};
        if (XV == 1) c.x = d.xv[at].x;
        if (side) sw = d.w[at];
      }
      visit(mine, c, sw);
    }
  }
}

}  // namespace tfx
