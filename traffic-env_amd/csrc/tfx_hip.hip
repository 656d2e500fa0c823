// tfx_hip.hip - MI355X (gfx950 / CDNA4) implementation of the IDM traffic-env tick behind the
// C ABI of include/tfx.h.  Written for wave64; no other target is supported.
//
// One tick (reference: gym_traffic/envs/traffic_env.py:224-248, TrafficEnv._step) is
//   * for envs that fit a compute unit's LDS: part of ONE launch per tfx_step / tfx_agent_step call -
//     k_res (tfx_resident.hpp), the cars resident on chip for all the ticks of the call;
//   * otherwise per-tick kernels, from two ticks on as PAIRS:
//       k_move_tt (tfx_move_tt.hpp)   the cars through two ticks per trip through HBM
//       k_tail (tfx_tail.hpp)         advance of tick t, the deferred cars' tick t+1, advance of t+1: a workgroup per env
//     with the env range in two halves on two streams (validate mode: the W forms of both kernels, heterogeneous cars:
//     the HET forms); small launches and the ring layout: k_move_t / k_move_ts / k_move_dma / k_move<WPR> + k_advance.
//     Plain calls and agent steps enqueue them through ONE sequence (tfx_sequence.hpp: pair, single, run_ticks), which
//     lists where the two differ.
// This file is the C ABI itself; the handle is in tfx_handle.hpp, kernel choice, grid sizing and launches in tfx_launch.hpp,
// the cold kernels in tfx_misc.hpp, the table of an env's device arrays - the scratch arena tfx_create carves, the halves
// of a split call (sub_dev), the pointer lists of graph_key - in tfx_dev_layout.hpp.  tfx_step and tfx_agent_step read alike: size the grids, decide, run the body
// (step_body / agent_sequence) on the caller's stream or replay its capture (run_captured).
#include <cmath>
#include <initializer_list>
#include <memory>
#include <new>

#include "tfx_cells.hpp"
#include "tfx_follow.hpp"
#include "tfx_ends.hpp"
#include "tfx_cars.hpp"
#include "tfx_digest.hpp"
#include "tfx_put.hpp"
#include "tfx_frames.hpp"
#include "tfx_clone.hpp"
#include "tfx_measure.hpp"
#include "tfx_sequence.hpp"
#include "tfx_travel.hpp"

namespace {

// A graph key is the values themselves, one after the other: every field has a fixed width, and the fields that come
// and go (an array per mode, the pool's block) follow the modes and the pool pointer that announce them
template <class... T>
void key_put(std::string &key, const T &...v) {
  (key.append(reinterpret_cast<const char *>(&v), sizeof v), ...);
}
void key_put_arrays(std::string &key, const Dev &d) {
  for_each_env_array(d, [&key](const void *p, size_t, ArrayKind) { key_put(key, p); });
}

// The arrival stream's part of that key: k_poisson's / k_res's and k_demand's arguments - the kind, the seeds, the tables'
// sizes, the caller's profile_of_env and the stream's buffer
void stream_key(const ArrivalStream &a, std::string &key) {
  const PoissonDev &p = a.ps;
  const DemandDev &m = a.dm;
  key_put(key, a.kind, p.seed_lo, p.seed_hi, p.n_cdf, p.regular, p.every, p.burst, m.K, m.S, m.seg_ticks, m.tick_offset, m.n_cdf,
          m.seed_lo, m.seed_hi, m.profile, a.drow.n_rows, a.drow.S, a.buf);
}

// Everything a captured launch sequence bakes into its kernel arguments (a stale graph is never replayed, even when a
// re-allocated buffer lands on the address the old one had: input_gen): the scalars and the caller's outputs, every
// per-env array of the handle (for_each_env_array), the episode block, the pool's arrays, the stream
std::string graph_key(tfx_handle h, int n_ticks, int remi, const void *aobs, const void *areward, const void *adone) {
  const Dev &d = h->d;
  static_assert(std::has_unique_object_representations_v<EpDev>, "the key takes the episode block byte for byte");
  std::string key;
  key.reserve(1024);
  key_put(key, h->input_gen, h->greedy, h->greedy_spacing, n_ticks, remi, aobs, areward, adone, d.action, d.action_mode,
          d.action_period, d.action_stride, d.spawn, d.spawn_mode, d.spawn_period, d.spawn_stride, h->pool);
  key_put_arrays(key, d);
  key_put(key, h->ep);  // (no padding: four words, eight pointers)
  // warm restarts (tfx_set_episode_pool): the pool's block is baked into the restart's arguments - whatever of it a
  // caller can re-bind (the rest lives as long as the pool handle does)
  if (const tfx_handle p = h->pool) {
    key_put_arrays(key, p->d);
    key_put(key, p->d.trip_cap, p->d.action_mode, p->d.spawn_mode);
  }
  stream_key(h->stream, key);
  return key;
}


// One captured sequence through its whole cycle: capture `body` (which enqueues on the stream it is given) when the key
// differs from that of the graph at hand, then replay the graph on `st`.  The grids were sized at the API entry: no
// occupancy query or function attribute may run between the begin and the end of a capture (size_grids).
// Counting: a body adds the ticks it enqueues to the handle's counters, as it does when it runs eagerly.  A capture ran
// no kernel, so what the body added is taken back, kept as the sequence's per-replay addition, and every replay -
// the first included - adds it again and reports the capture's last mover.
template <class Body>
int run_captured(tfx_handle h, CapturedSeq &c, const std::string &key, hipStream_t st, Body body) {
  if (!c.exec || c.key != key) {
    if (c.exec) { (void)hipGraphExecDestroy(c.exec); c.exec = nullptr; }
    if (c.graph) { (void)hipGraphDestroy(c.graph); c.graph = nullptr; }
    if (!h->ag_stream) HIPCHK(hipStreamCreateWithFlags(&h->ag_stream, hipStreamNonBlocking));
    const long long fused0 = h->fused_ticks, pair0 = h->pair_ticks, tail0 = h->tail_ticks;
    HIPCHK(hipStreamBeginCapture(h->ag_stream, hipStreamCaptureModeThreadLocal));
    const int rc = body(h->ag_stream);
    hipGraph_t g = nullptr;
    const hipError_t ce = hipStreamEndCapture(h->ag_stream, &g);
    c.fused = h->fused_ticks - fused0;
    c.pair = h->pair_ticks - pair0;
    c.tail = h->tail_ticks - tail0;
    c.step_kernel = h->step_kernel;
    h->fused_ticks = fused0;
    h->pair_ticks = pair0;
    h->tail_ticks = tail0;
    if (rc != TFX_OK) { if (g) (void)hipGraphDestroy(g); return rc; }
    if (ce != hipSuccess) return fail(TFX_EDEVICE, "hipStreamEndCapture: %s", hipGetErrorString(ce));
    c.graph = g;
    HIPCHK(hipGraphInstantiate(&c.exec, g, nullptr, nullptr, 0));
    c.key = key;
  }
  HIPCHK(hipGraphLaunch(c.exec, st));
  h->fused_ticks += c.fused;
  h->pair_ticks += c.pair;
  h->tail_ticks += c.tail;
  h->step_kernel = c.step_kernel;
  return TFX_OK;
}

}  // namespace

extern "C" int tfx_agent_step(tfx_handle h, int32_t n_ticks, int32_t remi, float *aobs, float *areward,
                              uint8_t *adone, void *stream) {
  if (int rc = check_handle(h, true)) return rc;
  if (n_ticks < 1) return fail(TFX_EINVAL, "n_ticks < 1");
  if (h->action_per_tick)
    return fail(TFX_EINVAL, "the fused agent step holds ONE action for all its ticks (bind the action buffer "
                            "with per_tick = 0)");
  if (h->stream.upfront() && n_ticks > h->stream.rows)
    return fail(TFX_EINVAL, "n_ticks = %d: a decision's arrivals are drawn up front and the demand's count buffer holds %d "
                            "rows at this batch size", n_ticks, h->stream.rows);
  if (int rc = clock_room(h, n_ticks, "tfx_agent_step")) return rc;
  ClockAdvance advanced{h, n_ticks};
  hipStream_t st = (hipStream_t)stream;
  if (!res_usable(h, n_ticks)) {
    if (int rc = size_grids(h, true, n_ticks)) return rc;
  }
  // a batch whose halves still fill the chip: two halves on two streams (k_tail of one under the pass of the other),
  // run eagerly; every other decision replays a captured graph
  const bool split = split_usable(h, n_ticks, true);
  if (split) {
    if (int rc = ensure_split(h, st)) return rc;
  }
  const bool capture = h->use_graph && !split;
  auto body = [&](hipStream_t s) { return agent_sequence(h, n_ticks, remi, aobs, areward, adone, s, split); };
  if (!capture) return body(st);
  // one graph per distinct launch sequence: everything baked into kernel arguments is in the key
  return run_captured(h, h->captured[SEQ_AGENT], graph_key(h, n_ticks, remi, aobs, areward, adone), st, body);
}

namespace {

// The handle's arrival stream goes: its rows stop feeding the move kernels - the counts, and the archetype rows it drew
// (rows bound through tfx_set_spawn_archetypes stay) - and its buffer is freed.  Nothing of the handle keeps pointing
// into it: a caller that fails after this leaves a handle without spawns.
void drop_stream(tfx_handle h) {
  ArrivalStream &s = h->stream;
  if (!s.drawn()) return;
  Dev &d = h->d;
  if (d.spawn_arch && d.spawn_arch == s.prow.rows) {
    d.spawn_arch = nullptr;
    d.spawn_arch_S = 0;
    d.spawn_arch_stride = 0;
  }
  d.spawn = nullptr;
  d.spawn_stride = 0;
  d.spawn_mode = TFX_SPAWN_NONE;
  h->spawn_per_tick = 0;
  (void)hipFree(s.buf);
  s = ArrivalStream{};
}

// A new stream of `kind` for the handle's envs, staged WITHOUT touching the handle (a call that fails here has changed
// nothing): the buffer (stream_layout), cleared - tick counters, car indices and seq start at 0, a Poisson stream's
// gap at -1: first gap not drawn yet -, every env's stream keyed by its global id (tfx_clone_envs with
// TFX_CLONE_STREAM copies ids), the kind's tables uploaded one behind the other.  The setter adds the kind's scalars.
struct HostTable { const uint32_t *words; size_t n; };
int stage_stream(tfx_handle h, StreamKind kind, uint64_t seed, std::initializer_list<HostTable> tables, ArrivalStream *out,
                 int demand_rows = 0) {
  const Dev &d = h->d;
  const bool demand = kind == STREAM_DEMAND;
  size_t n_tables = 0;
  for (const HostTable &t : tables) n_tables += t.n;
  // heterogeneous cars: the Poisson stream draws every car's archetype row (the regular stream's cars are row 0), a mixed
  // demand demand_rows of them per road and tick - with no car counters to keep (rule 5 is stateless)
  const int S = kind == STREAM_POISSON && h->het ? d.C - 2 : (demand ? demand_rows : 0);
  const StreamLayout l = stream_layout(d.E, d.n_entry, n_tables, S, demand);
  ArrivalStream s;
  if (hipMalloc(&s.buf, l.bytes) != hipSuccess) {
    const hipError_t e = hipGetLastError();
    return demand ? fail(TFX_ENOMEM, "demand: hipMalloc(%zu bytes) failed", l.bytes)
                  : fail(TFX_EDEVICE, "hipMalloc(arrival stream, %zu bytes): %s", l.bytes, hipGetErrorString(e));
  }
  char *base = (char *)s.buf;
  s.kind = kind;
  s.rows = l.rows;
  s.counts = (int *)(base + l.counts);
  s.gap = (int *)(base + l.gap);
  s.draws = (unsigned *)(base + l.draws);
  s.sid = (unsigned *)(base + l.sid);
  s.tables = (unsigned *)(base + l.tables);
  std::vector<unsigned> ids((size_t)d.E);
  for (int e = 0; e < d.E; ++e) ids[(size_t)e] = (unsigned)(e + d.env_off);
  bool ok = hipMemset(s.buf, 0, l.bytes) == hipSuccess &&
            (kind != STREAM_POISSON || hipMemset(s.gap, 0xff, (size_t)d.E * 4) == hipSuccess) &&
            hipMemcpy(s.sid, ids.data(), ids.size() * 4, hipMemcpyHostToDevice) == hipSuccess;
  unsigned *to = s.tables;
  for (const HostTable &t : tables) {
    ok = ok && (t.n == 0 || hipMemcpy(to, t.words, t.n * 4, hipMemcpyHostToDevice) == hipSuccess);
    to += t.n;
  }
  if (!ok) {
    const hipError_t e = hipGetLastError();
    (void)hipFree(s.buf);
    return fail(TFX_EDEVICE, demand ? "demand: uploading the tables failed: %s" : "uploading the arrival stream failed: %s",
                hipGetErrorString(e));
  }
  if (demand) {
    s.dm.sid = s.sid;
    s.dm.seed_lo = (unsigned)seed;
    s.dm.seed_hi = (unsigned)(seed >> 32);
  } else {
    s.ps.counts = s.counts;
    s.ps.gap_left = s.gap;
    s.ps.draws = s.draws;
    s.ps.sid = s.sid;
    s.ps.seed_lo = (unsigned)seed;
    s.ps.seed_hi = (unsigned)(seed >> 32);
  }
  if (S > 0) {
    s.prow.seq = demand ? nullptr : (unsigned *)(base + l.seq);
    s.prow.rows = (uint8_t *)(base + l.arch);
    s.prow.S = S;
    s.prow.n_arch = h->n_arch;
  }
  *out = std::move(s);
  return TFX_OK;
}

// The staged stream replaces whatever spawn rule the handle had.  What the move kernels see: a count buffer of the
// handle's own - per tick for rule 4, whose callers draw their rows up front; one row for rule 1 (tfx_step's chunks set
// the strides of theirs, for_stream_chunks) - and the stream's archetype rows or, where it draws none (every car of the
// regular stream is archetypes[0], traffic_env.py:174), no rows at all.  The rows of a mixed demand are per tick like
// its counts: the stride holds wherever the move kernels run - decisions and tfx_move_cars as well as tfx_step's chunks.
void install_stream(tfx_handle h, ArrivalStream &&s) {
  Dev &d = h->d;
  ++h->input_gen;
  drop_stream(h);
  h->stream = std::move(s);
  const ArrivalStream &a = h->stream;
  d.spawn = a.counts;
  d.spawn_stride = a.upfront() ? (long)d.E * d.n_entry : 0;
  d.spawn_mode = TFX_SPAWN_COUNTS;
  h->spawn_per_tick = a.upfront() ? 1 : 0;
  d.spawn_arch = a.prow.rows;
  d.spawn_arch_S = a.prow.S;
  d.spawn_arch_stride = a.upfront() ? d.spawn_stride * a.prow.S : 0;
}

// a threshold table's row: non-decreasing, the last one 0xFFFFFFFF (k_demand's binary search relies on the order).
// 0: fine; c < n: the row decreases at c; n: it does not end in 0xFFFFFFFF
int bad_cdf_row(const uint32_t *row, int n) {
  for (int c = 1; c < n; ++c)
    if (row[c] < row[c - 1]) return c;
  return row[n - 1] != 0xFFFFFFFFu ? n : 0;
}

// tfx_set_demand (mixed false: rule 4 alone) and tfx_set_demand_mixed (rule 5 as well: row_cdf [K][S][n_rows]).
// (the arguments first, as tfx_road_cells checks them: each cause is named whatever state the handle is in)
int set_demand(tfx_handle h, const tfx_demand *dm, bool mixed, const uint32_t *row_cdf, int32_t n_rows) {
  if (!dm) return fail(TFX_EINVAL, "demand: dm is null");
  if (!dm->count_cdf) return fail(TFX_EINVAL, "demand: count_cdf is null");
  if (!dm->road_cdf) return fail(TFX_EINVAL, "demand: road_cdf is null");
  if (mixed && !row_cdf) return fail(TFX_EINVAL, "demand: row_cdf is null");
  const int K = dm->n_profiles, S = dm->n_segments, n_cdf = dm->n_cdf;
  if (K < 1 || K > DEMAND_MAX_PROFILES) return fail(TFX_EINVAL, "demand: n_profiles %d is outside 1..%d", K, DEMAND_MAX_PROFILES);
  if (S < 1 || S > DEMAND_MAX_SEGMENTS) return fail(TFX_EINVAL, "demand: n_segments %d is outside 1..%d", S, DEMAND_MAX_SEGMENTS);
  if (dm->seg_ticks < 1) return fail(TFX_EINVAL, "demand: seg_ticks %d is below 1", dm->seg_ticks);
  if (n_cdf < 1 || n_cdf > DEMAND_MAX_CDF) return fail(TFX_EINVAL, "demand: n_cdf %d is outside 1..%d", n_cdf, DEMAND_MAX_CDF);
  if ((long long)S * dm->seg_ticks > 0x7fffffffLL)
    return fail(TFX_EINVAL, "demand: the period n_segments * seg_ticks = %lld does not fit an int32", (long long)S * dm->seg_ticks);
  for (int ks = 0; ks < K * S; ++ks)
    if (const int c = bad_cdf_row(dm->count_cdf + (size_t)ks * n_cdf, n_cdf))
      return fail(TFX_EINVAL, c < n_cdf ? "demand: count_cdf row (%d, %d) decreases at %d" : "demand: count_cdf row (%d, %d) does not end in 0xFFFFFFFF",
                  ks / S, ks % S, c);
  if (int rc = check_handle(h, false)) return rc;
  Dev &d = h->d;
  if (h->het && !mixed)
    return fail(TFX_EINVAL, "demand: heterogeneous handles (tfx_config.n_archetypes) are not supported - rule 4 draws no archetype rows: "
                            "tfx_set_demand_mixed draws them (rule 5)");
  if (mixed && !h->het)
    return fail(TFX_EINVAL, "demand: tfx_set_demand_mixed needs a heterogeneous handle (tfx_config.n_archetypes); this one has a "
                            "single archetype: tfx_set_demand");
  if (mixed && n_rows != h->n_arch)
    return fail(TFX_EINVAL, "demand: n_rows %d is not the handle's n_archetypes %d", n_rows, h->n_arch);
  if (d.n_entry < 1) return fail(TFX_EINVAL, "demand: no entry roads");
  if (d.n_entry > DEMAND_MAX_ENTRY) return fail(TFX_EINVAL, "demand: more than %d entry roads", DEMAND_MAX_ENTRY);
  const int ne = d.n_entry;
  for (int ks = 0; ks < K * S; ++ks)
    if (const int c = bad_cdf_row(dm->road_cdf + (size_t)ks * ne, ne))
      return fail(TFX_EINVAL, c < ne ? "demand: road_cdf row (%d, %d) decreases at %d" : "demand: road_cdf row (%d, %d) does not end in 0xFFFFFFFF",
                  ks / S, ks % S, c);
  for (int ks = 0; mixed && ks < K * S; ++ks)
    if (const int c = bad_cdf_row(row_cdf + (size_t)ks * n_rows, n_rows))
      return fail(TFX_EINVAL, c < n_rows ? "demand: row_cdf row (%d, %d) decreases at %d" : "demand: row_cdf row (%d, %d) does not end in 0xFFFFFFFF",
                  ks / S, ks % S, c);
  if (int rc = check_handle(h, true)) return rc;
  const size_t n_cc = (size_t)K * S * n_cdf, n_rc = (size_t)K * S * ne, n_rw = mixed ? (size_t)K * S * n_rows : 0;
  // rule 5 keeps S rows per road and tick: no road takes more than C - 2 cars in a tick, no env receives more than n_cdf - 1
  const int per_road = mixed ? (d.C - 2 < n_cdf - 1 ? d.C - 2 : n_cdf - 1) : 0;
  ArrivalStream s;
  if (int rc = stage_stream(h, STREAM_DEMAND, dm->seed, {{dm->count_cdf, n_cc}, {dm->road_cdf, n_rc}, {row_cdf, n_rw}}, &s, per_road))
    return rc;
  s.count_cdf.assign(dm->count_cdf, dm->count_cdf + n_cc);
  s.road_cdf.assign(dm->road_cdf, dm->road_cdf + n_rc);
  DemandDev &m = s.dm;
  m.count_cdf = s.tables;
  m.road_cdf = s.tables + n_cc;
  m.profile = dm->profile_of_env;
  m.K = K; m.S = S; m.seg_ticks = dm->seg_ticks; m.tick_offset = dm->tick_offset; m.n_cdf = n_cdf;
  if (mixed) {
    s.row_cdf.assign(row_cdf, row_cdf + n_rw);
    s.drow.row_cdf = s.tables + n_cc + n_rc;
    s.drow.n_rows = n_rows;
    s.drow.S = per_road;
  }
  install_stream(h, std::move(s));
  return TFX_OK;
}

// The ticks of a call under an arrival stream whose rows are drawn up front: in chunks of the rows the count buffer
// holds, ONE launch each (they depend on nothing but the stream and, rule 4, the clock the chunk before left; a launch
// per tick was the longest one of a cfg4 tick), then body(chunk).  A chunk's kernels count ticks from 0 - row t of the
// count buffer, and of the stream's archetype rows (heterogeneous cars), is the chunk's tick t; a per-tick ACTION buffer
// is indexed by the tick of the whole call, so its base moves along with the chunks.  Everything is put back on exit.
template <class Body>
int for_stream_chunks(tfx_handle h, int n_ticks, hipStream_t st, Body body) {
  Dev &d = h->d;
  const ArrivalStream &s = h->stream;
  const int *const act0 = d.action;
  const long stride0 = d.spawn_stride, arch_stride0 = d.spawn_arch_stride;
  const bool rows = s.prow.rows && d.spawn_arch == s.prow.rows;
  int rc = TFX_OK;
  for (int done = 0; done < n_ticks && rc == TFX_OK; done += s.rows) {
    const int chunk = n_ticks - done < s.rows ? n_ticks - done : s.rows;
    rc = launch_stream(h, chunk, st);
    d.spawn_stride = (long)d.E * d.n_entry;
    if (rows) d.spawn_arch_stride = d.spawn_stride * s.prow.S;
    if (act0 && h->action_per_tick) d.action = act0 + (size_t)done * d.action_stride;
    if (rc == TFX_OK) rc = body(chunk);
    d.spawn_stride = stride0;
    d.spawn_arch_stride = arch_stride0;
    d.action = act0;
  }
  return rc;
}

// the launches of a tfx_step call on the per-tick kernels, on `st`
int step_body(tfx_handle h, int n_ticks, hipStream_t st) {
  // a call's ticks, or one chunk of them: two halves on two streams where that pays (a chunk that splits is not captured)
  auto ticks = [&](int n) {
    const bool split = split_usable(h, n);
    if (split) {
      if (int rc = ensure_split(h, st)) return rc;
    }
    return run_ticks(h, n, st, false, split);
  };
  if (int rc = launch_greedy(h, st)) return rc;  // (the decision of the call's first tick; later ones: advance_item)
  return h->stream.drawn() && n_ticks > 0 ? for_stream_chunks(h, n_ticks, st, ticks) : ticks(n_ticks);
}

// ---- tfx_create's three steps -----------------------------------------------------------------------------
// the archetype rows a configuration describes: v, l, a, delta, v0, b, T, s0
struct ArchRows {
  int n = 1;
  bool het = false;  // several rows, or an exponent other than 4
  float row[TFX_MAX_ARCH][8] = {};
};

// Step 1: the configuration is one this library runs; its archetype rows
int check_config(const tfx_config &cfg, ArchRows &ar) {
  if (cfg.m < 1 || cfg.n < 1) return fail(TFX_EINVAL, "grid must be at least 1x1");
  if (cfg.capacity < 3) return fail(TFX_EINVAL, "capacity must be >= 3 (slot 0 + fake leader + 1 car)");
  if (cfg.capacity - 2 > 256) return fail(TFX_EINVAL, "capacity-2 > 256 cars per road is not supported");
  if (cfg.n_envs < 1) return fail(TFX_EINVAL, "n_envs must be >= 1");
  if (cfg.planes != 2 && cfg.planes != 3) return fail(TFX_EINVAL, "planes must be 2 (x,v) or 3 (x,v,w)");
  if (cfg.validate && cfg.planes != 3) return fail(TFX_EINVAL, "validate mode needs planes = 3 (spawn tick w)");
  if (cfg.layout != 0 && cfg.layout != 1) return fail(TFX_EINVAL, "layout must be 0 (ring) or 1 (transposed)");
  ar.n = cfg.n_archetypes <= 1 ? 1 : cfg.n_archetypes;
  if (ar.n > TFX_MAX_ARCH) return fail(TFX_EINVAL, "at most %d archetype rows", TFX_MAX_ARCH);
  ar.het = ar.n > 1;
  for (int a = 0; a < ar.n; ++a) {
    const float single[8] = {cfg.car_v, cfg.car_l, cfg.car_a, cfg.car_delta, cfg.car_v0, cfg.car_b, cfg.car_T, cfg.car_s0};
    memcpy(ar.row[a], cfg.n_archetypes >= 1 ? cfg.arch[a] : single, sizeof single);
    const float delta = ar.row[a][3];
    if (!(delta > 0.0f) || !(delta <= 64.0f))
      return fail(TFX_EINVAL, "archetype %d: delta = %g - the exponent must be in (0, 64]", a, delta);
    if (delta != 4.0f) ar.het = true;
    if (!(ar.row[a][2] > 0.0f) || !(ar.row[a][5] > 0.0f) || !(ar.row[a][4] > 0.0f))
      return fail(TFX_EINVAL, "archetype %d: a, b and v0 must be > 0", a);
  }
  if (ar.het && (cfg.layout != 1 || cfg.planes != 3))
    return fail(TFX_EINVAL, "heterogeneous cars (several archetypes, or delta != 4) need layout = 1 and planes = 3");
  if (!(cfg.length > 0.0f) || !(cfg.rate > 0.0f)) return fail(TFX_EINVAL, "length and rate must be > 0");
  return TFX_OK;
}

// Step 2: the host side of the handle - the road tables and storage slots, the environment knobs, the device the handle
// lives on, the scalars of the device block
int init_host(tfx_handle_s *h, const tfx_config &given, const ArchRows &ar) {
  h->cfg = given;
  h->het = ar.het;
  h->n_arch = ar.n;
  if (!ar.het && given.n_archetypes == 1) {  // one ordinary row given through the table: it IS the archetype
    h->cfg.car_v = ar.row[0][0]; h->cfg.car_l = ar.row[0][1]; h->cfg.car_a = ar.row[0][2];
    h->cfg.car_delta = ar.row[0][3]; h->cfg.car_v0 = ar.row[0][4]; h->cfg.car_b = ar.row[0][5];
    h->cfg.car_T = ar.row[0][6]; h->cfg.car_s0 = ar.row[0][7];
  }
  const tfx_config *cfg = &h->cfg;
  build_tables(h);
  build_slots(h);
  if (const char *mv = getenv("TFX_MOVE_VARIANT")) h->move_variant = atoi(mv);
  if (const char *gr = getenv("TFX_GRAPH")) h->use_graph = atoi(gr) != 0;
  if (const char *pv = getenv("TFX_PAIRS")) h->pairs = atoi(pv);
  if (const char *tv = getenv("TFX_TAIL")) h->tail = atoi(tv);
  if (const char *sv = getenv("TFX_SPLIT")) h->split = atoi(sv);
  if (const char *gv = getenv("TFX_TT_SEG")) h->tt_seg = atoi(gv);
  if (const char *gv = getenv("TFX_TT_SEGS")) h->tt_segs = atoi(gv);
  if (const char *gv = getenv("TFX_MEASURE_GRID")) h->measure_grid = atoi(gv);
  if (const char *gv = getenv("TFX_GRID_CAP")) h->grid_cap = atoi(gv) > 0 ? atoi(gv) : 0;
  if (const char *pc = getenv("TFX_MOVE_BLOCKS_PER_CU")) h->move_blocks_per_cu = atoi(pc);
  if (const char *sv = getenv("TFX_STAGGER")) h->stagger = atoi(sv) != 0;
  int dev = 0;
  hipDeviceProp_t prop;
  if (hipGetDevice(&dev) == hipSuccess) h->device = dev;
  if (hipGetDeviceProperties(&prop, dev) == hipSuccess)
    h->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;

  Dev &d = h->d;
  memset(&d, 0, sizeof d);
  d.I = cfg->m * cfg->n;
  d.r = 4 * d.I;
  d.R = d.r + 2 * cfg->m + 2 * cfg->n;
  d.C = cfg->capacity;
  d.E = cfg->n_envs;
  d.n_entry = (int)h->h_entry.size();
  d.obs_len = 2 * d.r + 2 * d.I;
  d.yellow = cfg->yellow_ticks;
  d.learn_switch = cfg->learn_switch;
  d.validate = cfg->validate;
  d.env_off = cfg->env_id_offset;
  d.layout = cfg->layout;
  d.length = cfg->length;
  d.rate = cfg->rate;
  d.car_v = cfg->car_v; d.car_l = cfg->car_l; d.car_a = cfg->car_a; d.car_v0 = cfg->car_v0;
  d.car_b = cfg->car_b; d.car_T = cfg->car_T; d.car_s0 = cfg->car_s0;
  d.risk_a = cfg->car_a;
  if (ar.het)
    for (int a = 0; a < ar.n; ++a) d.risk_a = a == 0 ? ar.row[0][2] : fmaxf(d.risk_a, ar.row[a][2]);
  d.two_sab = 2.0f * sqrtf(cfg->car_a * cfg->car_b);  // 2 * np.sqrt(a*b) (traffic_env.py:54)
  d.eps = cfg->eps;
  d.r_two_sab = 1.0f / d.two_sab;
  d.r_v0 = 1.0f / cfg->car_v0;
  d.thresh = cfg->thresh;
  d.near_end = cfg->length - cfg->detect_dist;
  d.ovf_pen = cfg->overflow_penalty;
  if ((long)d.E * d.R > 0x7fffffffL / 4) return fail(TFX_EINVAL, "E*R too large");
  d.G = h->tiles_per_env;
  d.trows = d.C - 2;  // (padding the tile stride off the power of two was measured: slightly slower)
  d.het = ar.het ? 1 : 0;
  const int cars = d.C - 2;
  h->wpr = cars <= 64 ? 1 : (cars <= 128 ? 2 : 4);
  d.action_mode = TFX_ACTION_CYCLE;
  d.action_period = 20;
  d.spawn_mode = TFX_SPAWN_NONE;
  d.spawn_period = 8;
  return TFX_OK;
}

// Step 3: the device side - the road tables, the scratch arena (carve_arena, tfx_dev_layout.hpp: one list sizes it and
// binds its pointers), the archetype table, the self-tests of the fast paths
int init_device(tfx_handle_s *h, const ArchRows &ar) {
  Dev &d = h->d;
  const size_t R = (size_t)d.R;
  const size_t n_slots = h->h_slot_road.size();
  if (hipMalloc((void **)&h->dev_tables, (4 * R + n_slots) * sizeof(int)) != hipSuccess)
    return fail(TFX_ENOMEM, "hipMalloc(tables) failed");
  if (hipMemcpy(h->dev_tables, h->h_nexts.data(), R * sizeof(int), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(h->dev_tables + R, h->h_pred.data(), R * sizeof(int), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(h->dev_tables + 2 * R, h->h_entry_idx.data(), R * sizeof(int), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(h->dev_tables + 3 * R, h->h_road_slot.data(), R * sizeof(int), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(h->dev_tables + 4 * R, h->h_slot_road.data(), n_slots * sizeof(int), hipMemcpyHostToDevice) != hipSuccess)
    return fail(TFX_EDEVICE, "uploading the road tables failed");
  d.nexts = h->dev_tables;
  d.pred = h->dev_tables + R;
  d.entry_idx = h->dev_tables + 2 * R;
  d.road_slot = h->dev_tables + 3 * R;
  d.slot_road = h->dev_tables + 4 * R;

  // the scratch arena: sized, allocated and cleared, bound
  const size_t bytes = carve_arena(d, h->ep, h->dev_ep, h->misc, h->cfg.planes, nullptr);
  if (hipMalloc(&h->dev_scratch, bytes) != hipSuccess) return fail(TFX_ENOMEM, "hipMalloc(scratch, %zu bytes) failed", bytes);
  if (hipMemset(h->dev_scratch, 0, bytes) != hipSuccess) return fail(TFX_EDEVICE, "clearing the scratch failed");
  carve_arena(d, h->ep, h->dev_ep, h->misc, h->cfg.planes, (char *)h->dev_scratch);
  if (ar.het) {
    float tab[TFX_MAX_ARCH][ARCH_W] = {};
    for (int a = 0; a < ar.n; ++a) {
      const float *r = ar.row[a];
      tab[a][AR_L] = r[1]; tab[a][AR_A] = r[2]; tab[a][AR_V0] = r[4]; tab[a][AR_T] = r[6]; tab[a][AR_S0] = r[7];
      tab[a][AR_2SAB] = 2.0f * sqrtf(r[2] * r[5]);  // 2 * np.sqrt(a*b) (traffic_env.py:54)
      tab[a][AR_DELTA] = r[3]; tab[a][AR_V] = r[0];
    }
    if (hipMalloc((void **)&h->dev_arch, sizeof tab) != hipSuccess ||
        hipMemcpy(h->dev_arch, tab, sizeof tab, hipMemcpyHostToDevice) != hipSuccess)
      return fail(TFX_ENOMEM, "uploading the archetype table failed");
    d.arch_tab = h->dev_arch;
  }
  // reciprocal division is used only if it is exact for this handle's constants on the whole
  // admitted numerator domain (2 x ~2^31 quotients, a few milliseconds; TFX_FASTDIV=0 disables)
  d.fastdiv = 0;
  {
    const char *fd = getenv("TFX_FASTDIV");
    if (!fd || atoi(fd) != 0) {
      unsigned long long *bad = &h->misc->selftest;  // zero at this point
      hipLaunchKernelGGL(k_div_selftest, dim3(h->n_cu * 8), dim3(256), 0, 0, d.two_sab, d.r_two_sab,
                         TFX_FASTDIV_A_LO, TFX_FASTDIV_A_HI, bad);
      hipLaunchKernelGGL(k_div_selftest, dim3(h->n_cu * 8), dim3(256), 0, 0, h->cfg.car_v0, d.r_v0,
                         TFX_FASTDIV_V_LO, TFX_FASTDIV_V_HI, bad);
      unsigned long long nbad = 1;
      if (hipMemcpy(&nbad, bad, sizeof nbad, hipMemcpyDeviceToHost) == hipSuccess && nbad == 0) d.fastdiv = 1;
      (void)hipMemset(bad, 0, sizeof nbad);
      h->div_mismatches = nbad;
    }
  }
  {
    unsigned *bad = reinterpret_cast<unsigned *>(&h->misc->selftest);  // (cleared again above)
    hipLaunchKernelGGL(k_max_selftest, dim3(1), dim3(1), 0, 0, bad, 0.0f, -0.0f);
    unsigned nbad = 1;
    if (hipMemcpy(&nbad, bad, sizeof nbad, hipMemcpyDeviceToHost) == hipSuccess && nbad == 0) d.fastmax = 1;
    (void)hipMemset(bad, 0, 8);
  }
  return TFX_OK;
}

}  // namespace

extern "C" {

int tfx_abi_version(void) { return TFX_ABI_VERSION; }
const char *tfx_last_error(void) { return g_err.c_str(); }

int tfx_create(const tfx_config *cfg, tfx_handle *out) {
  if (!cfg || !out) return fail(TFX_EINVAL, "null argument");
  ArchRows ar;
  if (int rc = check_config(*cfg, ar)) return rc;
  int ndev = 0;
  HIPCHK(hipGetDeviceCount(&ndev));
  if (ndev < 1) return fail(TFX_EDEVICE, "no HIP device");
  // the half-built handle is released through tfx_destroy, which tolerates every member being null: a failure below
  // is a plain return
  std::unique_ptr<tfx_handle_s, int (*)(tfx_handle)> h(new (std::nothrow) tfx_handle_s(), tfx_destroy);
  if (!h) return fail(TFX_ENOMEM, "out of host memory");
  if (int rc = init_host(h.get(), *cfg, ar)) return rc;
  if (int rc = init_device(h.get(), ar)) return rc;
  *out = h.release();
  return TFX_OK;
}

int tfx_destroy(tfx_handle h) {
  if (!h) return TFX_OK;
  for (hipEvent_t e : h->ev) (void)hipEventDestroy(e);
  for (CapturedSeq &c : h->captured) {
    if (c.exec) (void)hipGraphExecDestroy(c.exec);
    if (c.graph) (void)hipGraphDestroy(c.graph);
  }
  if (h->ag_stream) (void)hipStreamDestroy(h->ag_stream);
  if (h->split_stream) {
    (void)hipStreamSynchronize(h->split_stream);
    (void)hipStreamDestroy(h->split_stream);
    (void)hipEventDestroy(h->split_fork);
    (void)hipEventDestroy(h->split_join);
    (void)hipEventDestroy(h->split_stagger);
  }
  drop_stream(h);
  if (h->dev_greedy) (void)hipFree(h->dev_greedy);
  if (h->dev_tables) (void)hipFree(h->dev_tables);
  if (h->dev_scratch) (void)hipFree(h->dev_scratch);
  if (h->dev_arch) (void)hipFree(h->dev_arch);
  delete h;
  return TFX_OK;
}

int tfx_dims(tfx_handle h, int32_t *I, int32_t *r, int32_t *R, int32_t *n_entry) {
  if (int rc = check_handle(h, false)) return rc;
  if (I) *I = h->d.I;
  if (r) *r = h->d.r;
  if (R) *R = h->d.R;
  if (n_entry) *n_entry = h->d.n_entry;
  return TFX_OK;
}

int tfx_tables(tfx_handle h, int32_t *dest, int32_t *phases, int32_t *nexts, int32_t *entrypoints) {
  if (int rc = check_handle(h, false)) return rc;
  const size_t R = (size_t)h->d.R;
  if (dest) memcpy(dest, h->h_dest.data(), R * sizeof(int32_t));
  if (phases) memcpy(phases, h->h_phases.data(), R * sizeof(int32_t));
  if (nexts) memcpy(nexts, h->h_nexts.data(), R * sizeof(int32_t));
  if (entrypoints) memcpy(entrypoints, h->h_entry.data(), h->h_entry.size() * sizeof(int32_t));
  return TFX_OK;
}

int tfx_bind_buffers(tfx_handle h, const tfx_buffers *b) {
  if (int rc = check_handle(h, false)) return rc;
  if (!b) return fail(TFX_EINVAL, "null buffers");
  if (!b->xv || !b->leading || !b->lastcar || !b->obs || !b->rewards || !b->waiting ||
      !b->passed_dst || !b->done_tick)
    return fail(TFX_EINVAL, "xv, leading, lastcar, obs, rewards, waiting, passed_dst and done_tick are required");
  if (h->cfg.planes == 3 && !b->w) return fail(TFX_EINVAL, "planes = 3 needs the w buffer");
  if (((uintptr_t)b->xv & 15u) != 0) return fail(TFX_EINVAL, "xv must be 16-byte aligned");
  if (h->cfg.validate && (!b->n_trips || (b->trip_times && b->trip_cap < 1)))
    return fail(TFX_EINVAL, "validate mode needs n_trips (and trip_cap >= 1 with trip_times)");
  Dev &d = h->d;
  d.xv = reinterpret_cast<float2 *>(b->xv); d.w = b->w;
  d.leading = b->leading; d.lastcar = b->lastcar; d.obs = b->obs;
  d.lights = env_lights(d); d.lights_stride = d.obs_len;
  d.rewards = b->rewards; d.waiting = b->waiting; d.passed_dst = b->passed_dst;
  d.done_tick = b->done_tick; d.trip_times = b->trip_times; d.n_trips = b->n_trips;
  d.trip_cap = b->trip_cap;
  h->bound = true;
  ++h->input_gen;
  return d.w ? res_configure<true>(h) : res_configure<false>(h);
}

int tfx_reset(tfx_handle h, const int32_t *phase_init, void *stream) {
  if (int rc = check_handle(h, true)) return rc;
  if (!phase_init) return fail(TFX_EINVAL, "phase_init is required");
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(hipMemsetAsync(h->d.tickA, 0, sizeof(int), st));
  HIPCHK(hipMemsetAsync(h->d.tickB, 0, sizeof(int), st));
  h->clock = 0;
  hipLaunchKernelGGL(k_reset, dim3(grid_for(h, (long)h->d.E * h->d.R)), dim3(256), 0, st, h->d, phase_init,
                     (const uint8_t *)nullptr, h->ep);
  HIPCHK(hipGetLastError());
  return TFX_OK;
}

int tfx_reset_envs(tfx_handle h, const int32_t *phase_init, const uint8_t *mask, void *stream) {
  if (int rc = check_handle(h, true)) return rc;
  if (!phase_init || !mask) return fail(TFX_EINVAL, "phase_init and mask are required");
  hipLaunchKernelGGL(k_reset, dim3(grid_for(h, (long)h->d.E * h->d.R)), dim3(256), 0, (hipStream_t)stream,
                     h->d, phase_init, mask, h->ep);
  HIPCHK(hipGetLastError());
  return TFX_OK;
}

int tfx_set_episodes(tfx_handle h, int32_t enabled, int32_t max_decisions, uint64_t seed, const tfx_episode_buffers *b) {
  if (enabled) {  // (arguments first: they are checked even where no handle can exist)
    if (max_decisions < 0) return fail(TFX_EINVAL, "max_decisions must be >= 0 (0: no time limit)");
    if (!b) return fail(TFX_EINVAL, "null episode buffers");
    if (!b->ep_return || !b->ep_len || !b->final_return || !b->final_len || !b->truncated || !b->ep_index)
      return fail(TFX_EINVAL, "ep_return, ep_len, final_return, final_len, truncated and ep_index are required");
  }
  if (int rc = check_handle(h, true)) return rc;
  EpDev &ep = h->ep;
  HIPCHK(hipDeviceSynchronize());  // (decisions under way still read the marks)
  HIPCHK(hipMemset(ep.mark, 0, 2 * (size_t)h->d.E));
  ++h->input_gen;
  ep.on = enabled ? 1 : 0;
  ep.max = enabled ? max_decisions : 0;
  ep.seed_lo = enabled ? (unsigned)seed : 0u;
  ep.seed_hi = enabled ? (unsigned)(seed >> 32) : 0u;
  ep.ep_return = enabled ? b->ep_return : nullptr;
  ep.ep_len = enabled ? b->ep_len : nullptr;
  ep.final_return = enabled ? b->final_return : nullptr;
  ep.final_len = enabled ? b->final_len : nullptr;
  ep.trunc = enabled ? b->truncated : nullptr;
  ep.ep_index = enabled ? b->ep_index : nullptr;
  HIPCHK(hipMemcpy(h->dev_ep, &ep, sizeof ep, hipMemcpyHostToDevice));
  HIPCHK(hipDeviceSynchronize());
  return TFX_OK;
}

int tfx_refresh(tfx_handle h, void *stream) {
  if (int rc = check_handle(h, true)) return rc;
  hipLaunchKernelGGL(k_refresh, dim3(grid_for(h, (long)h->d.E * h->d.R)), dim3(256), 0,
                     (hipStream_t)stream, h->d);
  HIPCHK(hipGetLastError());
  return TFX_OK;
}

int tfx_set_actions(tfx_handle h, int32_t mode, const int32_t *dev, int32_t period, int32_t per_tick) {
  if (int rc = check_handle(h, false)) return rc;
  Dev &d = h->d;
  ++h->input_gen;
  h->greedy = false;
  d.greedy_spacing = 0;
  d.greedy_act = nullptr;
  if (mode == TFX_ACTION_GREEDY) {
    if (period < 1) return fail(TFX_EINVAL, "greedy spacing must be >= 1");
    if (!h->dev_greedy) {
      HIPCHK(hipMalloc((void **)&h->dev_greedy, (size_t)d.E * d.I * sizeof(int)));
      HIPCHK(hipMemset(h->dev_greedy, 0, (size_t)d.E * d.I * sizeof(int)));
    }
    h->greedy = true;
    h->greedy_spacing = period;
    d.greedy_spacing = period;
    d.greedy_act = h->dev_greedy;
    d.action = h->dev_greedy;
    d.action_stride = 0;
    d.action_mode = TFX_ACTION_BUFFER;
    h->action_per_tick = 0;
    return TFX_OK;
  }
  if (mode == TFX_ACTION_CYCLE) {
    if (period < 1 || period > TFX_PERIOD_MAX)
      return fail(TFX_EINVAL, "cycle period must be >= 1 and <= TFX_PERIOD_MAX = %d", TFX_PERIOD_MAX);
    d.action_period = period;
  } else if (mode == TFX_ACTION_BUFFER || mode == TFX_ACTION_BROADCAST) {
    if (!dev) return fail(TFX_EINVAL, "action buffer is null");
    d.action = dev;
    d.action_stride = per_tick ? (mode == TFX_ACTION_BUFFER ? (long)d.E * d.I : (long)d.I) : 0;
  } else {
    return fail(TFX_EINVAL, "unknown action mode %d", mode);
  }
  d.action_mode = mode;
  h->action_per_tick = per_tick;
  return TFX_OK;
}

int tfx_set_spawns(tfx_handle h, int32_t mode, const int32_t *dev, int32_t period, int32_t per_tick) {
  if (int rc = check_handle(h, false)) return rc;
  Dev &d = h->d;
  ++h->input_gen;
  drop_stream(h);  // (its rows were bound as a count buffer of the handle's own: a failing call below leaves no spawns)
  if (mode == TFX_SPAWN_PERIODIC) {
    if (period < 1) return fail(TFX_EINVAL, "spawn period must be >= 1");
    d.spawn_period = period;
  } else if (mode == TFX_SPAWN_COUNTS) {
    if (!dev) return fail(TFX_EINVAL, "spawn buffer is null");
    d.spawn = dev;
    d.spawn_stride = per_tick ? (long)d.E * d.n_entry : 0;
  } else if (mode != TFX_SPAWN_NONE) {
    return fail(TFX_EINVAL, "unknown spawn mode %d", mode);
  }
  d.spawn_mode = mode;
  h->spawn_per_tick = per_tick;
  return TFX_OK;
}

int tfx_set_spawn_archetypes(tfx_handle h, const uint8_t *dev, int32_t per_road, int32_t per_tick) {
  if (int rc = check_handle(h, false)) return rc;
  if (!h->het) return fail(TFX_ESTATE, "the handle has a single archetype");
  if (dev && per_road < 1) return fail(TFX_EINVAL, "per_road must be >= 1");
  Dev &d = h->d;
  ++h->input_gen;
  d.spawn_arch = dev;
  d.spawn_arch_S = dev ? per_road : 0;
  d.spawn_arch_stride = (dev && per_tick) ? (long)d.E * d.n_entry * per_road : 0;
  return TFX_OK;
}

int tfx_set_poisson(tfx_handle h, double cars_per_tick, uint64_t seed, const uint32_t *cdf, int32_t n_cdf) {
  if (int rc = check_handle(h, false)) return rc;
  if (!(cars_per_tick > 0.0)) return fail(TFX_EINVAL, "cars_per_tick must be > 0");
  if (!cdf || n_cdf < 1 || n_cdf > 65536) return fail(TFX_EINVAL, "gap table missing or too long");
  Dev &d = h->d;
  if (d.n_entry < 1) return fail(TFX_EINVAL, "no entry roads");
  ArrivalStream s;
  if (int rc = stage_stream(h, STREAM_POISSON, seed, {{cdf, (size_t)n_cdf}}, &s)) return rc;
  s.ps.cdf = s.tables;
  s.ps.n_cdf = n_cdf;
  s.rate = cars_per_tick;
  install_stream(h, std::move(s));
  return TFX_OK;
}

int tfx_set_regular(tfx_handle h, int32_t every, int32_t burst, uint64_t seed) {
  if (int rc = check_handle(h, false)) return rc;
  if (every < 0 || burst < 1) return fail(TFX_EINVAL, "every must be >= 0 and burst >= 1");
  Dev &d = h->d;
  if (d.n_entry < 1) return fail(TFX_EINVAL, "no entry roads");
  ArrivalStream s;
  if (int rc = stage_stream(h, STREAM_REGULAR, seed, {}, &s)) return rc;
  s.ps.regular = 1;
  s.ps.every = every;
  s.ps.burst = burst;
  install_stream(h, std::move(s));
  return TFX_OK;
}

int tfx_set_demand(tfx_handle h, const tfx_demand *dm) { return set_demand(h, dm, false, nullptr, 0); }

int tfx_set_demand_mixed(tfx_handle h, const tfx_demand *dm, const uint32_t *row_cdf, int32_t n_rows) {
  return set_demand(h, dm, true, row_cdf, n_rows);
}

int tfx_demand_counts(tfx_handle h, int32_t tick0, int32_t n_ticks, int32_t *out, void *stream) {
  if (!out) return fail(TFX_EINVAL, "demand: out is null");
  if (n_ticks < 0) return fail(TFX_EINVAL, "demand: n_ticks %d is negative", n_ticks);
  if (int rc = check_handle(h, true)) return rc;
  if (!h->stream.upfront()) return fail(TFX_ESTATE, "demand: tfx_set_demand has not been called (or another spawn rule replaced it)");
  if (n_ticks == 0) return TFX_OK;
  // Not counted by tfx_debug_fail_after, nothing in the handle changes: captured graphs stay valid.
  return launch_demand(h, 0, tick0, n_ticks, out, nullptr, (hipStream_t)stream);
}

int tfx_demand_rows(tfx_handle h, int32_t tick0, int32_t n_ticks, int32_t *counts, uint8_t *rows, void *stream) {
  if (!counts) return fail(TFX_EINVAL, "demand: counts is null");
  if (!rows) return fail(TFX_EINVAL, "demand: rows is null");
  if (n_ticks < 0) return fail(TFX_EINVAL, "demand: n_ticks %d is negative", n_ticks);
  if (int rc = check_handle(h, true)) return rc;
  if (!h->stream.mixed())
    return fail(TFX_ESTATE, "demand: tfx_set_demand_mixed has not been called (or another spawn rule replaced it)");
  if (n_ticks == 0) return TFX_OK;
  // Not counted by tfx_debug_fail_after, nothing in the handle changes: captured graphs stay valid.
  return launch_demand(h, 0, tick0, n_ticks, counts, h->stream.drow.S > 0 ? rows : nullptr, (hipStream_t)stream);
}

int tfx_demand_rows_per_road(tfx_handle h, int32_t *per_road) {
  if (!per_road) return fail(TFX_EINVAL, "demand: per_road is null");
  if (int rc = check_handle(h, true)) return rc;
  if (!h->stream.mixed())
    return fail(TFX_ESTATE, "demand: tfx_set_demand_mixed has not been called (or another spawn rule replaced it)");
  *per_road = h->stream.drow.S;
  return TFX_OK;
}

int tfx_step(tfx_handle h, int32_t n_ticks, void *stream) {
  if (int rc = check_handle(h, true)) return rc;
  if (n_ticks < 0) return fail(TFX_EINVAL, "n_ticks < 0");
  if (int rc = clock_room(h, n_ticks, "tfx_step")) return rc;
  ClockAdvance advanced{h, n_ticks};
  hipStream_t st = (hipStream_t)stream;
  // envs that fit a compute unit's LDS: all the ticks of the call in one launch (tfx_resident.hpp)
  if (n_ticks > 0 && res_usable(h, n_ticks)) {
    auto fused = [&](int n) {
      TickTimer timer(h);
      if (int rc = timer.begin(st)) return rc;
      if (int rc = launch_res(h, n, st)) return rc;
      h->fused_ticks += n;
      if (int rc = timer.mid(st)) return rc;
      return timer.end(st, n);
    };
    // demand profiles: k_res reads the rows as a bound per-tick count buffer - drawn up front, chunk by chunk.  The draw
    // stays outside the timed region (tfx_profile), as it does on the per-tick path: an entry per chunk.  (Rule 1: k_res
    // draws inside its launch.)
    return h->stream.upfront() ? for_stream_chunks(h, n_ticks, st, fused) : fused(n_ticks);
  }
  if (int rc = size_grids(h, false, n_ticks)) return rc;
  // Launch-bound handles (a few thousand tiles: cfg4 x 16, a 16x16 grid x 256 envs) replay the call's launches as a HIP
  // graph, like the fused agent step does: at cfg4 x 16 the kernels of a tick add up to 59 us of its 65.6
  // (profiles/r04_cfg4_closed_loop_trace.txt).  Not while kernels are timed, not for calls that split over two streams.
  const Dev &d = h->d;
  const bool capture = h->use_graph && !h->prof && n_ticks >= 4 && d.layout == 1 &&
                       (long)d.E * d.G <= (long)h->n_cu * 24 && !split_usable(h, n_ticks);
  auto body = [&](hipStream_t s) { return step_body(h, n_ticks, s); };
  if (!capture) return body(st);
  // captured once per distinct sequence (graph_key), replayed afterwards
  return run_captured(h, h->captured[SEQ_STEP], graph_key(h, n_ticks, -1, nullptr, nullptr, nullptr), st, body);
}

int tfx_move_cars(tfx_handle h, void *stream) {
  if (int rc = check_handle(h, true)) return rc;
  if (int rc = clock_room(h, 1, "tfx_move_cars")) return rc;  // (the advance that completes the tick moves the clock)
  if (int rc = size_grids(h, false, 1)) return rc;
  if (int rc = launch_greedy(h, (hipStream_t)stream)) return rc;
  // (rule 4: the row of the tick the clock stands at)
  if (int rc = h->stream.upfront() ? launch_stream(h, 1, (hipStream_t)stream) : launch_inputs(h, (hipStream_t)stream)) return rc;
  return (pairs_usable(h) && !single_tick_ts(h)) ? launch_move_tt(h, false, false, 0, (hipStream_t)stream) : launch_move(h, 0, (hipStream_t)stream);
}

int tfx_advance_finished_cars(tfx_handle h, void *stream) {
  if (int rc = check_handle(h, true)) return rc;
  if (int rc = clock_room(h, 1, "tfx_advance_finished_cars")) return rc;
  if (int rc = size_grids(h, false, 1)) return rc;
  ClockAdvance advanced{h, 1};
  return launch_advance(h, 0, (hipStream_t)stream);
}

int tfx_remi(tfx_handle h, void *stream) {
  if (int rc = check_handle(h, true)) return rc;
  hipLaunchKernelGGL(k_remi, dim3(grid_for(h, (long)h->d.E * h->d.I)), dim3(256), 0,
                     (hipStream_t)stream, h->d);
  HIPCHK(hipGetLastError());
  return TFX_OK;
}

int tfx_cars_on_roads(tfx_handle h, int32_t *out, void *stream) {
  if (int rc = check_handle(h, true)) return rc;
  if (!out) return fail(TFX_EINVAL, "out is null");
  hipLaunchKernelGGL(k_cars_on_roads, dim3(grid_for(h, (long)h->d.E * h->d.R)), dim3(256), 0,
                     (hipStream_t)stream, h->d, out);
  HIPCHK(hipGetLastError());
  return TFX_OK;
}

int tfx_done(tfx_handle h, uint8_t *out, int32_t since_tick, void *stream) {
  if (int rc = check_handle(h, true)) return rc;
  if (!out) return fail(TFX_EINVAL, "out is null");
  hipLaunchKernelGGL(k_done, dim3(grid_for(h, h->d.E)), dim3(256), 0, (hipStream_t)stream, h->d,
                     out, since_tick);
  HIPCHK(hipGetLastError());
  return TFX_OK;
}

int tfx_get_tick(tfx_handle h, int32_t *tick) {
  if (int rc = check_handle(h, false)) return rc;
  if (!tick) return fail(TFX_EINVAL, "tick is null");
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(tick, h->d.tickA, sizeof(int), hipMemcpyDeviceToHost));
  return TFX_OK;
}

int tfx_set_tick(tfx_handle h, int32_t tick) {
  if (int rc = check_handle(h, false)) return rc;
  if (tick < 0 || tick > TFX_TICK_MAX)
    return fail(TFX_EINVAL, "tick %d is outside the clock's domain 0 .. TFX_TICK_MAX = %d", tick, TFX_TICK_MAX);
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(h->d.tickA, &tick, sizeof(int), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(h->d.tickB, &tick, sizeof(int), hipMemcpyHostToDevice));
  h->clock = tick;
  // tick stamps taken under the old clock must not alias ticks of the new one
  HIPCHK(hipMemset(h->d.env_flag, 0, (size_t)h->d.E * sizeof(int)));
  if (h->bound) HIPCHK(hipMemset(h->d.done_tick, 0, (size_t)h->d.E * sizeof(int)));
  return TFX_OK;
}

int tfx_vehicle_updates(tfx_handle h, uint64_t *out, void *stream) {
  if (int rc = check_handle(h, false)) return rc;
  if (!out) return fail(TFX_EINVAL, "out is null");
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  std::vector<unsigned long long> slots((size_t)VEH_SLOTS * VEH_STRIDE);
  HIPCHK(hipMemcpy(slots.data(), h->d.veh, slots.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  unsigned long long v = 0;
  for (int i = 0; i < VEH_SLOTS; ++i) v += slots[(size_t)i * VEH_STRIDE];
  *out = (uint64_t)v;
  return TFX_OK;
}

int tfx_reset_counters(tfx_handle h, void *stream) {
  if (int rc = check_handle(h, false)) return rc;
  HIPCHK(hipMemsetAsync(h->d.veh, 0, (size_t)VEH_SLOTS * VEH_STRIDE * sizeof(unsigned long long), (hipStream_t)stream));
  return TFX_OK;
}

int tfx_profile(tfx_handle h, int32_t max_ticks) {
  if (int rc = check_handle(h, false)) return rc;
  for (hipEvent_t e : h->ev) (void)hipEventDestroy(e);
  h->ev.clear();
  h->ev_ticks = 0;
  h->ev_used = 0;
  h->prof = max_ticks > 0;
  if (!h->prof) return TFX_OK;
  h->ev.resize((size_t)max_ticks * 3);
  h->ev_weight.assign((size_t)max_ticks, 1);
  for (hipEvent_t &e : h->ev) HIPCHK(hipEventCreate(&e));
  h->ev_ticks = max_ticks;
  return TFX_OK;
}

int tfx_profile_read(tfx_handle h, double *move_ms, double *advance_ms, int32_t *n_ticks) {
  if (int rc = check_handle(h, false)) return rc;
  double mv = 0.0, ad = 0.0;
  int ticks = 0;
  for (int i = 0; i < h->ev_used; ++i) {
    float a = 0.f, b = 0.f;
    HIPCHK(hipEventSynchronize(h->ev[(size_t)i * 3 + 2]));
    HIPCHK(hipEventElapsedTime(&a, h->ev[(size_t)i * 3], h->ev[(size_t)i * 3 + 1]));
    HIPCHK(hipEventElapsedTime(&b, h->ev[(size_t)i * 3 + 1], h->ev[(size_t)i * 3 + 2]));
    mv += a;
    ad += b;
    ticks += h->ev_weight[i];
  }
  if (move_ms) *move_ms = mv;
  if (advance_ms) *advance_ms = ad;
  if (n_ticks) *n_ticks = ticks;
  h->ev_used = 0;
  return TFX_OK;
}

int tfx_xv_pairs(tfx_handle h, int64_t *pairs) {
  if (int rc = check_handle(h, false)) return rc;
  if (!pairs) return fail(TFX_EINVAL, "pairs is null");
  *pairs = (int64_t)h->d.E * (int64_t)env_car_pairs(h->d);
  return TFX_OK;
}

int tfx_export_ring(tfx_handle h, float *ring_xv, float *ring_w, uint8_t *ring_a, void *stream) {
  if (int rc = check_handle(h, true)) return rc;
  if (h->d.layout != 1) return fail(TFX_ESTATE, "the handle already uses the ring layout");
  if (!ring_xv) return fail(TFX_EINVAL, "ring_xv is null");
  hipLaunchKernelGGL(k_export_ring, dim3(grid_for(h, (long)h->d.E * h->d.R)), dim3(256), 0,
                     (hipStream_t)stream, h->d, reinterpret_cast<float2 *>(ring_xv), ring_w, ring_a);
  HIPCHK(hipGetLastError());
  return TFX_OK;
}

int tfx_import_ring(tfx_handle h, const float *ring_xv, const float *ring_w, const uint8_t *ring_a, void *stream) {
  if (int rc = check_handle(h, true)) return rc;
  if (h->d.layout != 1) return fail(TFX_ESTATE, "the handle already uses the ring layout");
  if (!ring_xv) return fail(TFX_EINVAL, "ring_xv is null");
  hipLaunchKernelGGL(k_import_ring, dim3(grid_for(h, (long)h->d.E * h->d.R)), dim3(256), 0,
                     (hipStream_t)stream, h->d, reinterpret_cast<const float2 *>(ring_xv), ring_w, ring_a);
  HIPCHK(hipGetLastError());
  return TFX_OK;
}

int tfx_fastdiv_status(tfx_handle h, int32_t *enabled, uint64_t *mismatches) {
  if (int rc = check_handle(h, false)) return rc;
  if (enabled) *enabled = h->d.fastdiv;
  if (mismatches) *mismatches = h->div_mismatches;
  return TFX_OK;
}

int tfx_fused_ticks(tfx_handle h, int64_t *ticks, int32_t *capable) {
  if (int rc = check_handle(h, false)) return rc;
  if (ticks) *ticks = h->fused_ticks;
  if (capable) *capable = h->res_epb > 0 ? 1 : 0;
  return TFX_OK;
}

int tfx_pair_ticks(tfx_handle h, int64_t *ticks) {
  if (int rc = check_handle(h, false)) return rc;
  if (ticks) *ticks = h->pair_ticks;
  return TFX_OK;
}

int tfx_tail_ticks(tfx_handle h, int64_t *ticks) {
  if (int rc = check_handle(h, false)) return rc;
  if (ticks) *ticks = h->tail_ticks;
  return TFX_OK;
}

int tfx_slow_pairs(tfx_handle h, uint64_t *pairs, void *stream) {
  if (int rc = check_handle(h, false)) return rc;
  if (!pairs) return fail(TFX_EINVAL, "pairs is null");
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  unsigned long long v = 0;
  HIPCHK(hipMemcpy(&v, h->d.slow_pairs, sizeof v, hipMemcpyDeviceToHost));
  *pairs = (uint64_t)v;
  return TFX_OK;
}

int tfx_split_ticks(tfx_handle h, int64_t *ticks) {
  if (int rc = check_handle(h, false)) return rc;
  if (ticks) *ticks = h->split_ticks;
  return TFX_OK;
}

const char *tfx_step_kernel(tfx_handle h) { return h ? h->step_kernel : ""; }

}  // extern "C"

namespace {

// Two handles a clone can go between (tfx_clone_envs with dst != src, tfx_set_episode_pool): the same device and the
// same world; anything else is TFX_EINVAL with a message naming the field, led by `what`
int same_world(tfx_handle dst, tfx_handle src, const char *what) {
  const tfx_config &a = dst->cfg, &b = src->cfg;
  if (dst->device != src->device)
    return fail(TFX_EINVAL, "%s: the handles live on different devices (device %d / %d)", what, dst->device, src->device);
#define TFX_SAME(field, fmt)                                                                                         \
  if (a.field != b.field) return fail(TFX_EINVAL, "%s: the handles differ in " #field " (" fmt " / " fmt ")", what, a.field, b.field)
  TFX_SAME(m, "%d"); TFX_SAME(n, "%d"); TFX_SAME(capacity, "%d"); TFX_SAME(planes, "%d"); TFX_SAME(layout, "%d");
  TFX_SAME(length, "%g"); TFX_SAME(rate, "%g"); TFX_SAME(validate, "%d"); TFX_SAME(learn_switch, "%d");
  TFX_SAME(entry_spec, "%u");
  // (the constants every tick reads: a clone continues as its source does only under the same ones)
  TFX_SAME(yellow_ticks, "%d"); TFX_SAME(thresh, "%g"); TFX_SAME(detect_dist, "%g"); TFX_SAME(overflow_penalty, "%g");
  TFX_SAME(eps, "%g");
#undef TFX_SAME
  if (dst->het != src->het || dst->n_arch != src->n_arch)
    return fail(TFX_EINVAL, "%s: the handles differ in n_archetypes (%d / %d rows)", what, dst->n_arch, src->n_arch);
  const bool table = a.n_archetypes >= 1;
  if (table != (b.n_archetypes >= 1) ||
      (table ? memcmp(a.arch, b.arch, (size_t)dst->n_arch * sizeof a.arch[0]) != 0
             : (a.car_v != b.car_v || a.car_l != b.car_l || a.car_a != b.car_a || a.car_delta != b.car_delta ||
                a.car_v0 != b.car_v0 || a.car_b != b.car_b || a.car_T != b.car_T || a.car_s0 != b.car_s0)))
    return fail(TFX_EINVAL, "%s: the handles differ in the archetype table (arch)", what);
  if (dst->h_slot_road != src->h_slot_road)
    return fail(TFX_EINVAL, "%s: the handles differ in the kinds ordering of their storage slots (TFX_KINDS)", what);
  return TFX_OK;
}

// Two handles whose envs can follow each other's arrival streams (TFX_CLONE_STREAM): the same kind of stream under the
// same parameters (and, same_world, on the same archetype table: both draw rows, or neither does)
int streams_compatible(tfx_handle dst, tfx_handle src) {
  const ArrivalStream &a = dst->stream, &b = src->stream;
  if (a.upfront() != b.upfront())
    return fail(TFX_EINVAL, "clone: the handles differ in the stream kind (demand profiles in one handle only)");
  if (a.upfront()) {
    // rule 4 has no position: the stream id alone makes source and clone receive the same cars - under the same
    // seed, sizes, offset and tables (the host copies)
    const DemandDev &p = a.dm, &q = b.dm;
    if (p.seed_lo != q.seed_lo || p.seed_hi != q.seed_hi) return fail(TFX_EINVAL, "clone: the handles differ in the demand seed");
    if (p.K != q.K || p.S != q.S || p.seg_ticks != q.seg_ticks || p.n_cdf != q.n_cdf)
      return fail(TFX_EINVAL, "clone: the handles differ in the demand sizes (n_profiles, n_segments, seg_ticks, n_cdf)");
    if (p.tick_offset != q.tick_offset) return fail(TFX_EINVAL, "clone: the handles differ in the demand tick_offset");
    // (a mixed and a plain demand handle: one row_cdf is empty - and same_world refused them before: n_archetypes)
    if (a.count_cdf != b.count_cdf || a.road_cdf != b.road_cdf || a.row_cdf != b.row_cdf)
      return fail(TFX_EINVAL, "clone: the handles differ in the demand tables (count_cdf / road_cdf / row_cdf)");
    return TFX_OK;
  }
  if (!a.drawn() || !b.drawn())
    return fail(TFX_EINVAL, "clone: TFX_CLONE_STREAM needs an on-device arrival stream (tfx_set_poisson / tfx_set_regular / "
                            "tfx_set_demand) in both handles");
  const PoissonDev &p = a.ps, &q = b.ps;
  if (p.regular != q.regular) return fail(TFX_EINVAL, "clone: the handles differ in the stream kind (poisson / regular)");
  if (p.seed_lo != q.seed_lo || p.seed_hi != q.seed_hi) return fail(TFX_EINVAL, "clone: the handles differ in the stream seed");
  if (p.regular ? (p.every != q.every) : (a.rate != b.rate || p.n_cdf != q.n_cdf))
    return fail(TFX_EINVAL, "clone: the handles differ in the stream rate");
  if (p.burst != q.burst) return fail(TFX_EINVAL, "clone: the handles differ in the stream burst");
  return TFX_OK;
}

}  // namespace

extern "C" {

int tfx_clone_envs(tfx_handle dst, tfx_handle src, const int32_t *src_of_env, int32_t flags, void *stream) {
  if (flags & ~(TFX_CLONE_STREAM | TFX_CLONE_EPISODE)) return fail(TFX_EINVAL, "unknown clone flags 0x%x", flags);
  if (!src_of_env) return fail(TFX_EINVAL, "src_of_env is null");
  if (int rc = check_handle(dst, true)) return rc;
  if (int rc = check_handle(src, true)) return rc;
  if (dst != src) {
    if (int rc = same_world(dst, src, "clone")) return rc;
  }
  CloneOpt o{};
  o.same = dst == src ? 1 : 0;
  o.skipped = &dst->misc->clone_skipped;
  if (flags & TFX_CLONE_STREAM) {
    if (int rc = streams_compatible(dst, src)) return rc;
    const ArrivalStream &p = dst->stream, &q = src->stream;
    o.stream = 1;
    o.d_gap = p.gap; o.s_gap = q.gap;
    o.d_draws = p.draws; o.s_draws = q.draws;
    o.d_sid = p.sid; o.s_sid = q.sid;
    o.d_seq = p.prow.seq; o.s_seq = q.prow.seq;
  }
  if (flags & TFX_CLONE_EPISODE) {
    if (dst->ep.on != src->ep.on)
      return fail(TFX_EINVAL, "clone: TFX_CLONE_EPISODE with episodes on in one handle only (tfx_set_episodes)");
    if (dst->ep.on) {
      o.episode = 1;
      o.d_ep = dst->ep;
      o.s_ep = src->ep;
    }
  }
  if (dst->d.greedy_act && src->d.greedy_act) {
    o.d_greedy = dst->d.greedy_act;
    o.s_greedy = src->d.greedy_act;
  }
  TFX_INJECT(dst);
  hipLaunchKernelGGL(k_clone<false>, dim3((unsigned)tile_grid(dst)), dim3(256), 0, (hipStream_t)stream, dst->d, src->d,
                     (const int *)src_of_env, o);
  HIPCHK(hipGetLastError());
  return TFX_OK;
}

int tfx_set_episode_pool(tfx_handle h, tfx_handle pool) {
  if (int rc = check_handle(h, false)) return rc;
  if (pool == h) return fail(TFX_EINVAL, "episode pool: a handle cannot be its own pool");
  if (int rc = check_handle(h, true)) return rc;
  if (pool) {
    if (int rc = check_handle(pool, true)) return rc;
    if (int rc = same_world(h, pool, "episode pool")) return rc;
  }
  // (nothing on the device changes: decisions under way keep the arguments they were enqueued with)
  h->pool = pool;
  ++h->input_gen;  // the captured agent-step graph holds the other form of the restart
  return TFX_OK;
}

int tfx_clone_skipped(tfx_handle h, uint64_t *skipped, void *stream) {
  if (int rc = check_handle(h, false)) return rc;
  if (!skipped) return fail(TFX_EINVAL, "skipped is null");
  // read and cleared ON the stream, behind the clones enqueued there and ahead of the next one
  unsigned long long v = 0;
  HIPCHK(hipMemcpyAsync(&v, &h->misc->clone_skipped, sizeof v, hipMemcpyDeviceToHost, (hipStream_t)stream));
  HIPCHK(hipMemsetAsync(&h->misc->clone_skipped, 0, sizeof v, (hipStream_t)stream));
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  *skipped = (uint64_t)v;
  return TFX_OK;
}

int tfx_road_measures(tfx_handle h, float halt_speed, float x_from, const tfx_measure_buffers *out, int32_t flags,
                      void *stream) {
  if (!out) return fail(TFX_EINVAL, "out is null");
  if (int rc = check_handle(h, false)) return rc;
  if (!out->n_cars && !out->n_halted && !out->queue && !out->speed_sum)
    return fail(TFX_EINVAL, "measures: every output pointer is null");
  if (flags & ~TFX_MEASURE_ACCUMULATE) return fail(TFX_EINVAL, "unknown measure flags 0x%x", flags);
  if (std::isnan(halt_speed) || std::isnan(x_from)) return fail(TFX_EINVAL, "measures: halt_speed / x_from is NaN");
  if (int rc = check_handle(h, true)) return rc;
  MeasureOut o{};
  o.n_cars = out->n_cars;
  o.n_halted = out->n_halted;
  o.queue = out->queue;
  o.speed_sum = out->speed_sum;
  o.accumulate = (flags & TFX_MEASURE_ACCUMULATE) ? 1 : 0;
  return launch_query(k_measure, tile_grid(h, true), stream, h->d, halt_speed, x_from, o);
}

int tfx_measure_launch(tfx_handle h, int32_t *grid, int32_t *waves) {
  if (int rc = check_handle(h, false)) return rc;
  return report_launch(tile_grid(h, true), grid, waves);
}

int tfx_road_following(tfx_handle h, const tfx_follow_params *p, const tfx_follow_buffers *out, int32_t flags,
                       void *stream) {
  if (!p) return fail(TFX_EINVAL, "following: p is null");
  if (!out) return fail(TFX_EINVAL, "following: out is null");
  if (int rc = check_handle(h, false)) return rc;
  if (!out->n_cars && !out->n_pairs && !out->n_joined && !out->n_overlap && !out->gap_sum && !out->gap_min && !out->n_hw &&
      !out->hw_sum && !out->n_conflict && !out->ttc_min && !out->drac_max)
    return fail(TFX_EINVAL, "following: every output pointer is null");
  if (flags & ~TFX_FOLLOW_ACCUMULATE) return fail(TFX_EINVAL, "unknown following flags 0x%x", flags);
  if (std::isnan(p->x_from) || std::isnan(p->platoon_gap) || std::isnan(p->v_min) || std::isnan(p->ttc_crit))
    return fail(TFX_EINVAL, "following: x_from / platoon_gap / v_min / ttc_crit is NaN");
  if (!(p->v_min > 0.0f)) return fail(TFX_EINVAL, "following: v_min %g is not above 0", (double)p->v_min);
  if (int rc = check_handle(h, true)) return rc;
  FollowOut o{};
  o.n_cars = out->n_cars;
  o.n_pairs = out->n_pairs;
  o.n_joined = out->n_joined;
  o.n_overlap = out->n_overlap;
  o.gap_sum = out->gap_sum;
  o.gap_min = out->gap_min;
  o.n_hw = out->n_hw;
  o.hw_sum = out->hw_sum;
  o.n_conflict = out->n_conflict;
  o.ttc_min = out->ttc_min;
  o.drac_max = out->drac_max;
  o.accumulate = (flags & TFX_FOLLOW_ACCUMULATE) ? 1 : 0;
  return launch_query(k_follow, tile_grid(h, true), stream, h->d, *p, o);
}

int tfx_follow_launch(tfx_handle h, int32_t *grid, int32_t *waves) {
  if (int rc = check_handle(h, false)) return rc;
  return report_launch(tile_grid(h, true), grid, waves);
}

int tfx_road_ends(tfx_handle h, const tfx_ends_params *p, const tfx_ends_buffers *out, int32_t flags, void *stream) {
  if (!p) return fail(TFX_EINVAL, "ends: p is null");
  if (!out) return fail(TFX_EINVAL, "ends: out is null");
  if (int rc = check_handle(h, false)) return rc;
  if (p->k < 1 || p->k > TFX_MAX_HEADS) return fail(TFX_EINVAL, "ends: k %d is outside 1..%d", p->k, TFX_MAX_HEADS);
  if (flags) return fail(TFX_EINVAL, "unknown ends flags 0x%x (lists do not accumulate)", flags);
  if (int rc = check_handle(h, true)) return rc;
  EndsOut o{};
  o.n_cars = out->n_cars;
  o.n_heads = out->n_heads;
  o.heads = reinterpret_cast<f2v *>(out->heads);
  o.head_rows = out->head_rows;
  o.tail = reinterpret_cast<f2v *>(out->tail);
  o.tail_row = out->tail_row;
  // k_measure's launch (tile_grid), instantiated on the bound of k
  const int K = p->k;
  return launch_query(K <= 4 ? k_ends<4> : K <= 8 ? k_ends<8> : k_ends<16>, tile_grid(h, true), stream, h->d, *p, o);
}

int tfx_ends_launch(tfx_handle h, int32_t k, int32_t *grid, int32_t *waves) {
  if (int rc = check_handle(h, false)) return rc;
  if (k < 1 || k > TFX_MAX_HEADS) return fail(TFX_EINVAL, "ends: k %d is outside 1..%d", k, TFX_MAX_HEADS);
  return report_launch(tile_grid(h, true), grid, waves);
}

// the n_sel of the two car-list calls: at least one selection, and keys s * R + road id that fit an int32
static int car_list_sel_ok(tfx_handle h, int32_t n_sel) {
  if (n_sel < 1) return fail(TFX_EINVAL, "car list: n_sel %d is less than 1", n_sel);
  if ((long long)n_sel * h->d.R + 1 > 0x7fffffffll)
    return fail(TFX_EINVAL, "car list: %d selections of %d roads do not fit int32 offsets", n_sel, h->d.R);
  return TFX_OK;
}

int tfx_car_list(tfx_handle h, const int32_t *env_ids, int32_t n_sel, const uint8_t *road_mask, const int32_t *offsets,
                 int32_t cap, const tfx_car_list_buffers *out, int32_t flags, void *stream) {
  if (!out) return fail(TFX_EINVAL, "car list: out is null");
  if (!offsets) return fail(TFX_EINVAL, "car list: offsets is null");
  if (cap < 0) return fail(TFX_EINVAL, "car list: cap %d is negative", cap);
  if (flags) return fail(TFX_EINVAL, "unknown car list flags 0x%x", flags);
  if (int rc = check_handle(h, false)) return rc;
  if (int rc = car_list_sel_ok(h, n_sel)) return rc;
  if (!env_ids && n_sel > h->d.E)
    return fail(TFX_EINVAL, "car list: n_sel %d is more than the handle's %d envs and env_ids is null", n_sel, h->d.E);
  if (out->spawn && h->cfg.planes != 3)
    return fail(TFX_EINVAL, "car list: the handle carries no side plane (planes == 2): spawn ticks are not kept");
  if (int rc = check_handle(h, true)) return rc;
  if (cap == 0) return TFX_OK;  // no entry may be written
  CarsArgs a{};
  a.env_ids = env_ids;
  a.road_mask = road_mask;
  a.offsets = offsets;
  a.n_sel = n_sel;
  a.cap = cap;
  a.xv = reinterpret_cast<f2v *>(out->xv);
  a.road = out->road;
  a.row = out->row;
  a.spawn = out->spawn;
  if (!a.xv && !a.road && !a.row && !a.spawn) return TFX_OK;  // nothing wanted
  // k_frames' launch: (selected env, tile) items
  return launch_query(k_cars, tile_grid(h, true, n_sel), stream, h->d, a);
}

int tfx_car_list_launch(tfx_handle h, int32_t n_sel, int32_t *grid, int32_t *waves) {
  if (int rc = check_handle(h, false)) return rc;
  if (int rc = car_list_sel_ok(h, n_sel)) return rc;
  return report_launch(tile_grid(h, true, n_sel), grid, waves);
}

int tfx_put_cars(tfx_handle h, const int32_t *env_ids, int32_t n_sel, const uint8_t *road_mask, const int32_t *offsets,
                 int32_t cap, const tfx_put_buffers *in, int32_t spawn_shift, uint64_t *lost, int32_t flags, void *stream) {
  if (!in) return fail(TFX_EINVAL, "put cars: in is null");
  if (!in->xv) return fail(TFX_EINVAL, "put cars: in->xv is null");
  if (!offsets) return fail(TFX_EINVAL, "put cars: offsets is null");
  if (cap < 0) return fail(TFX_EINVAL, "put cars: cap %d is negative", cap);
  if (flags) return fail(TFX_EINVAL, "unknown put cars flags 0x%x", flags);
  if (int rc = check_handle(h, false)) return rc;
  if (int rc = car_list_sel_ok(h, n_sel)) return rc;
  if (!env_ids && n_sel > h->d.E)
    return fail(TFX_EINVAL, "put cars: n_sel %d is more than the handle's %d envs and env_ids is null", n_sel, h->d.E);
  if (int rc = check_handle(h, true)) return rc;
  PutArgs a{};
  a.env_ids = env_ids;
  a.road_mask = road_mask;
  a.offsets = offsets;
  a.n_sel = n_sel;
  a.cap = cap;  // (0: every selected road is emptied)
  a.xv = reinterpret_cast<const f2v *>(in->xv);
  a.row = in->row;
  a.spawn = h->cfg.planes == 3 ? in->spawn : nullptr;
  a.leading = in->leading;
  a.lead_x = in->lead_x;
  a.spawn_shift = spawn_shift;
  a.lost = reinterpret_cast<unsigned long long *>(lost);
  // k_cars' items: (selected env, tile) pairs.  Not counted by tfx_debug_fail_after; no pointer of the handle changes, so
  // captured graphs stay valid
  const long grid = tile_grid(h, false, n_sel);
  // Non-temporal row stores where the mover uses them (pick_move_t: the handle's cars do not fit the Infinity Cache, so
  // the next tick finds none of them there anyway): 1113 -> 1029 us for xv of all 4096 envs of cfg2, 75.9 -> 65.8 us for
  // 256 envs, no difference below (profiles/put_cars.txt).  TFX_PUT_NT=0 / 1, read per call, forces a form
  // (tools/time_put_cars.py measures both on one handle).
  const char *ntv = getenv("TFX_PUT_NT");
  const bool nt = ntv ? atoi(ntv) != 0 : (size_t)h->d.E * env_car_pairs(h->d) * sizeof(float2) > ((size_t)448 << 20);
  return nt ? launch_query(k_put<true>, grid, stream, h->d, a) : launch_query(k_put<false>, grid, stream, h->d, a);
}

int tfx_put_launch(tfx_handle h, int32_t n_sel, int32_t *grid, int32_t *waves) {
  if (int rc = check_handle(h, false)) return rc;
  if (int rc = car_list_sel_ok(h, n_sel)) return rc;
  return report_launch(tile_grid(h, false, n_sel), grid, waves);
}

// the n_sel of the two digest calls: at least one selection, and road words s * R + road id that fit an int32
static int digest_sel_ok(tfx_handle h, int32_t n_sel) {
  if (n_sel < 1) return fail(TFX_EINVAL, "digest: n_sel %d is less than 1", n_sel);
  if ((long long)n_sel * h->d.R > 0x7fffffffll)
    return fail(TFX_EINVAL, "digest: %d selections of %d roads do not fit int32", n_sel, h->d.R);
  return TFX_OK;
}

int tfx_state_digest(tfx_handle h, const int32_t *env_ids, int32_t n_sel, const uint8_t *road_mask, int32_t parts,
                     uint64_t *env_digest, uint64_t *road_digest, int32_t flags, void *stream) {
  // (the arguments first, as tfx_road_cells checks them: each cause is named whatever state the handle is in)
  if (!env_digest) return fail(TFX_EINVAL, "digest: env_digest is null");
  if (flags) return fail(TFX_EINVAL, "unknown digest flags 0x%x", flags);
  if (parts == 0 || (parts & ~DG_ALL_PARTS)) return fail(TFX_EINVAL, "digest: parts 0x%x is empty or has unknown bits", parts);
  if (int rc = check_handle(h, false)) return rc;
  if (int rc = digest_sel_ok(h, n_sel)) return rc;
  if (!env_ids && n_sel > h->d.E)
    return fail(TFX_EINVAL, "digest: n_sel %d is more than the handle's %d envs and env_ids is null", n_sel, h->d.E);
  if ((parts & TFX_DIGEST_SPAWN) && h->cfg.planes != 3)
    return fail(TFX_EINVAL, "digest: the handle carries no side plane (planes == 2): spawn ticks are not kept");
  if (int rc = check_handle(h, true)) return rc;
  DigestArgs a{};
  a.env_ids = env_ids;
  a.road_mask = road_mask;
  a.n_sel = n_sel;
  a.parts = parts;
  a.env_digest = reinterpret_cast<unsigned long long *>(env_digest);
  a.road_digest = reinterpret_cast<unsigned long long *>(road_digest);
  // the env words are sums of the wavefronts' shares: they start at 0, as tfx_frames' background starts white
  HIPCHK(hipMemsetAsync(env_digest, 0, (size_t)n_sel * sizeof(uint64_t), (hipStream_t)stream));
  // k_cars' launch: (selected env, tile) items.  The walk by the parts (tfx_digest.hpp)
  const bool cars = (parts & TFX_DIGEST_CARS) != 0, bword = (parts & (TFX_DIGEST_ROWS | TFX_DIGEST_SPAWN)) != 0;
  const long grid = tile_grid(h, true, n_sel);
  if (cars && bword) return launch_query(k_digest<2>, grid, stream, h->d, a);
  if (cars) return launch_query(k_digest<1>, grid, stream, h->d, a);
  if (bword) return launch_query(k_digest<3>, grid, stream, h->d, a);
  return launch_query(k_digest<0>, grid, stream, h->d, a);
}

int tfx_digest_launch(tfx_handle h, int32_t n_sel, int32_t *grid, int32_t *waves) {
  if (int rc = check_handle(h, false)) return rc;
  if (int rc = digest_sel_ok(h, n_sel)) return rc;
  return report_launch(tile_grid(h, true, n_sel), grid, waves);
}

int tfx_car_ages(tfx_handle h, const tfx_age_buffers *out, int32_t flags, void *stream) {
  if (!out) return fail(TFX_EINVAL, "ages: out is null");
  if (int rc = check_handle(h, false)) return rc;
  if (!out->n_cars && !out->age_sum && !out->age_max) return fail(TFX_EINVAL, "ages: every output pointer is null");
  if (flags & ~TFX_TRAVEL_ACCUMULATE) return fail(TFX_EINVAL, "unknown travel flags 0x%x", flags);
  if (int rc = check_handle(h, true)) return rc;
  if (!h->d.w) return fail(TFX_ESTATE, "ages: the handle carries no side plane (planes == 2): spawn ticks are not kept");
  AgeOut o{};
  o.n_cars = out->n_cars;
  o.age_sum = reinterpret_cast<long long *>(out->age_sum);
  o.age_max = out->age_max;
  o.accumulate = (flags & TFX_TRAVEL_ACCUMULATE) ? 1 : 0;
  return launch_query(k_ages, tile_grid(h, true), stream, h->d, o);
}

int tfx_ages_launch(tfx_handle h, int32_t *grid, int32_t *waves) {
  if (int rc = check_handle(h, false)) return rc;
  return report_launch(tile_grid(h, true), grid, waves);
}

int tfx_trip_stats(tfx_handle h, const int32_t *edges, int32_t n_bins, int32_t *cursor, const tfx_trip_stat_buffers *out,
                   int32_t flags, void *stream) {
  // (the arguments first, as tfx_road_cells checks them: each cause is named whatever state the handle is in)
  if (!out) return fail(TFX_EINVAL, "trips: out is null");
  if (int rc = check_handle(h, false)) return rc;
  if (!out->count && !out->tick_sum && !out->tick_max && !out->lost && !out->hist)
    return fail(TFX_EINVAL, "trips: every output pointer is null");
  if (flags & ~TFX_TRAVEL_ACCUMULATE) return fail(TFX_EINVAL, "unknown travel flags 0x%x", flags);
  if (n_bins < 0 || n_bins > TRIP_BINS || (out->hist && n_bins < 1))
    return fail(TFX_EINVAL, "trips: n_bins %d is outside 1..%d", n_bins, TRIP_BINS);
  TripEdges ed{};
  if (out->hist) {
    if (!edges) return fail(TFX_EINVAL, "trips: hist is given but edges is null");
    for (int k = 0; k < n_bins; ++k)
      if (edges[k] > edges[k + 1])
        return fail(TFX_EINVAL, "trips: edges decrease at %d (%d, %d)", k, edges[k], edges[k + 1]);
    for (int k = 0; k <= TRIP_BINS; ++k) ed.e[k] = edges[k <= n_bins ? k : n_bins];
  }
  if (int rc = check_handle(h, true)) return rc;
  if (!h->d.validate || !h->d.trip_times || !h->d.n_trips)
    return fail(TFX_ESTATE, "trips: the handle is not in validate mode with trip_times and n_trips bound: no trip log is kept");
  TripOut o{};
  o.count = out->count;
  o.tick_sum = reinterpret_cast<long long *>(out->tick_sum);
  o.tick_max = out->tick_max;
  o.lost = out->lost;
  o.hist = out->hist;
  o.accumulate = (flags & TFX_TRAVEL_ACCUMULATE) ? 1 : 0;
  // a wavefront per env; of the caller's memory the cursor is written next to the outputs
  return launch_query(k_trips, item_grid(h, h->d.E), stream, h->d, ed, out->hist ? n_bins : 0, cursor, o);
}

int tfx_road_cells(tfx_handle h, const float *edges, int32_t n_cells, const tfx_cell_buffers *out, int32_t flags,
                   void *stream) {
  // (the arguments first, as tfx_road_measures does with `out`: each cause is named whatever state the handle is in)
  if (!edges) return fail(TFX_EINVAL, "cells: edges is null");
  if (!out) return fail(TFX_EINVAL, "cells: out is null");
  if (!out->n_cars && !out->speed_sum) return fail(TFX_EINVAL, "cells: every output pointer is null");
  if (n_cells < 1 || n_cells > TFX_MAX_CELLS)
    return fail(TFX_EINVAL, "cells: n_cells %d is outside 1..%d", n_cells, TFX_MAX_CELLS);
  if (flags & ~TFX_CELLS_ACCUMULATE) return fail(TFX_EINVAL, "unknown cell flags 0x%x", flags);
  for (int k = 0; k <= n_cells; ++k)
    if (std::isnan(edges[k])) return fail(TFX_EINVAL, "cells: edge %d is NaN", k);
  for (int k = 0; k < n_cells; ++k)
    if (!(edges[k] < edges[k + 1]))
      return fail(TFX_EINVAL, "cells: edges are not strictly ascending at %d (%g, %g)", k, edges[k], edges[k + 1]);
  if (int rc = check_handle(h, true)) return rc;
  CellEdges ed;
  ed.lo = edges[0];
  ed.hi = edges[n_cells];
  for (int k = 0; k < TFX_MAX_CELLS; ++k) ed.inner[k] = (k >= 1 && k < n_cells) ? edges[k] : INFINITY;
  CellOut o{};
  o.n_cars = out->n_cars;
  o.speed_sum = out->speed_sum;
  o.accumulate = (flags & TFX_CELLS_ACCUMULATE) ? 1 : 0;
  // k_measure's launch (tile_grid), instantiated on the cell bound
  const int B = n_cells;
  return launch_query(B <= 8 ? k_cells<8> : B <= 16 ? k_cells<16> : k_cells<32>, tile_grid(h, true), stream, h->d, ed, B, o);
}

int tfx_cells_launch(tfx_handle h, int32_t n_cells, int32_t *grid, int32_t *waves) {
  if (int rc = check_handle(h, false)) return rc;
  if (n_cells < 1 || n_cells > TFX_MAX_CELLS)
    return fail(TFX_EINVAL, "cells: n_cells %d is outside 1..%d", n_cells, TFX_MAX_CELLS);
  return report_launch(tile_grid(h, true), grid, waves);
}

// the px of the three frame calls
static int frame_px_ok(int32_t px) {
  if (px < TFX_FRAME_PX_MIN || px > TFX_FRAME_PX_MAX)
    return fail(TFX_EINVAL, "frames: px %d is outside %d..%d", px, TFX_FRAME_PX_MIN, TFX_FRAME_PX_MAX);
  return TFX_OK;
}

int tfx_frame_size(tfx_handle h, int32_t px, int32_t *height, int32_t *width) {
  if (int rc = frame_px_ok(px)) return rc;
  if (int rc = check_handle(h, false)) return rc;
  if (height) *height = (h->cfg.m + 1) * px + 1;
  if (width) *width = (h->cfg.n + 1) * px + 1;
  return TFX_OK;
}

int tfx_frames(tfx_handle h, const int32_t *env_ids, int32_t n_frames, int32_t px, uint8_t *out, int32_t flags,
               void *stream) {
  // (the arguments first, as tfx_road_cells checks them: each cause is named whatever state the handle is in)
  if (!out) return fail(TFX_EINVAL, "frames: out is null");
  if (n_frames < 1) return fail(TFX_EINVAL, "frames: n_frames %d is less than 1", n_frames);
  if (int rc = frame_px_ok(px)) return rc;
  if (flags & ~TFX_FRAMES_ROADS_ONLY) return fail(TFX_EINVAL, "unknown frame flags 0x%x", flags);
  if (int rc = check_handle(h, false)) return rc;
  if (!env_ids && n_frames > h->d.E)
    return fail(TFX_EINVAL, "frames: n_frames %d is more than the handle's %d envs and env_ids is null", n_frames, h->d.E);
  const long long W = (long long)(h->cfg.n + 1) * px + 1, H = (long long)(h->cfg.m + 1) * px + 1;
  if (W * H > 0x7fffffffll) return fail(TFX_EINVAL, "frames: a frame of %lld x %lld pixels is too large", H, W);
  if (int rc = check_handle(h, true)) return rc;
  FrameArgs f{};
  f.env_ids = env_ids;
  f.out = reinterpret_cast<unsigned *>(out);
  f.n_frames = n_frames;
  f.roads_only = (flags & TFX_FRAMES_ROADS_ONLY) ? 1 : 0;
  f.m = h->cfg.m;
  f.n = h->cfg.n;
  f.S = px;
  f.W = (int)W;
  f.H = (int)H;
  f.k = (float)(px - 3) / h->cfg.length;  // one float32 division, on the host
  if (!(flags & TFX_FRAMES_ROADS_ONLY))
    HIPCHK(hipMemsetAsync(out, 0xFF, (size_t)n_frames * (size_t)(W * H) * 4, (hipStream_t)stream));
  return launch_query(k_frames, tile_grid(h, true, n_frames), stream, h->d, f);
}

int tfx_frames_launch(tfx_handle h, int32_t n_frames, int32_t px, int32_t *grid, int32_t *waves) {
  if (n_frames < 1) return fail(TFX_EINVAL, "frames: n_frames %d is less than 1", n_frames);
  if (int rc = frame_px_ok(px)) return rc;
  if (int rc = check_handle(h, false)) return rc;
  return report_launch(tile_grid(h, true, n_frames), grid, waves);
}

int tfx_debug_head_rows(tfx_handle h, uint8_t *out, void *stream) {
  if (int rc = check_handle(h, true)) return rc;
  if (!out) return fail(TFX_EINVAL, "out is null");
  const size_t n = (size_t)h->d.E * h->d.R;
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  if (h->d.layout != 1) {
    memset(out, 0, n);
    return TFX_OK;
  }
  HIPCHK(hipMemcpy(out, h->d.hb, n, hipMemcpyDeviceToHost));
  return TFX_OK;
}

int tfx_debug_fail_after(tfx_handle h, int32_t n_launches) {
  if (int rc = check_handle(h, false)) return rc;
  h->fail_after = n_launches > 0 ? n_launches : 0;
  return TFX_OK;
}

int tfx_launch_info(tfx_handle h, int32_t *grid, int32_t *block, int32_t *waves_per_road) {
  if (int rc = check_handle(h, false)) return rc;
  if (h->grid_move == 0) return fail(TFX_ESTATE, "no move kernel has been launched yet");
  if (grid) *grid = h->grid_move;
  if (block) *block = 256;
  if (waves_per_road) *waves_per_road = h->wpr;
  return TFX_OK;
}

}  // extern "C"

// host-only: replay of the reference's seeded arrival generators for many envs
#include "tfx_arrivals.cpp"
