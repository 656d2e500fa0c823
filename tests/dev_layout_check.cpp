// Stand-alone host check of csrc/tfx_dev_layout.hpp: the one table of an env's device arrays - the visitor over the
// per-env arrays, sub_dev (the halves of a split call), the carving of the scratch arena and its small words.  Built
// with -fsanitize=address,undefined and run by tests/test_dev_layout.py; it needs no device and dereferences no array.
// What it expects is restated here and NOT taken from the header under test: old_sub_dev is the body sub_dev had when
// it listed the arrays by hand, expected_regions the sizes and conditions tfx_create wrote out in its offset block.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "tfx_dev_layout.hpp"

using namespace tfx;

static int failures = 0;
#define CHECK(cond)                                                                         \
  do {                                                                                      \
    if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
  } while (0)

struct Shape { int m, n, C, E; };
struct Case { Shape s; int layout, planes, het; };

// the scalars of a handle's device block, as tfx_create derives them from the configuration
static Dev dev_scalars(const Case &c) {
  Dev d;
  std::memset(&d, 0, sizeof d);
  d.I = c.s.m * c.s.n;
  d.r = 4 * d.I;
  d.R = d.r + 2 * c.s.m + 2 * c.s.n;
  d.C = c.s.C;
  d.E = c.s.E;
  d.n_entry = 2 * (c.s.m + c.s.n);
  d.obs_len = 2 * d.r + 2 * d.I;
  d.env_off = 7;
  d.layout = c.layout;
  d.G = (d.R + 63) / 64;
  d.trows = d.C - 2;
  d.het = c.het;
  d.action_mode = TFX_ACTION_CYCLE;
  d.spawn_mode = TFX_SPAWN_NONE;
  return d;
}

// ---- the arena ------------------------------------------------------------------------------------------
struct Region { const char *name; uintptr_t at; size_t bytes; bool expect_null; };

// the offset block of tfx_create, region by region: bytes, and whether the pointer is null when there are none
static std::vector<Region> expected_regions(const Dev &d, const EpDev &ep, const EpDev *dev_ep, const MiscWords *misc, int planes) {
  const size_t E = (size_t)d.E, ER = E * (size_t)d.R;
  const bool T = d.layout == 1;
  const size_t n_opairs = E * d.G * TFX_KP * 64;
  auto at = [](const void *p) { return (uintptr_t)p; };
  return {
      {"rec", at(d.rec), ER * 16, false},
      {"rec2f", at(d.rec2f), T ? ER * 8 : 0, false},
      {"rec2c", at(d.rec2c), T ? ER * 4 : 0, false},
      {"crec", at(d.crec), T ? ER * 8 : 0, !T},
      {"ovf_cnt", at(d.ovf_cnt), T ? ER * 4 : 0, !T},
      {"rsw", at(d.rsw), T ? ER * 4 : 0, !T},
      {"tailx", at(d.tailx), ER * 4, false},
      {"env_flag", at(d.env_flag), E * 4, false},
      {"env_risk", at(d.env_risk), 2 * E * 4, false},
      {"outb", at(d.outb), T ? n_opairs * 8 : 0, false},
      {"outw", at(d.outw), T && planes == 3 ? n_opairs * 4 : 0, false},
      {"leadx", at(d.leadx), ER * 4, false},
      {"taila", at(d.taila), d.het ? ER * 4 : 0, false},
      {"hb", at(d.hb), T ? ER : 0, !T},
      {"ep", at(ep.mark), 2 * E, false},
      {"dev_ep", at(dev_ep), sizeof(EpDev), false},
      {"misc", at(misc), sizeof(MiscWords), false},
      {"veh", at(d.veh), (size_t)256 * 8 * 8, false},
  };
}

static void check_arena(const Case &c) {
  Dev d = dev_scalars(c);
  EpDev ep{};
  EpDev *dev_ep = nullptr;
  MiscWords *misc = nullptr;
  const Dev before = d;
  const size_t bytes = carve_arena(d, ep, dev_ep, misc, c.planes, nullptr);
  CHECK(std::memcmp(&d, &before, sizeof d) == 0);  // sizing binds nothing
  CHECK(!ep.mark && !ep.last && !dev_ep && !misc);
  CHECK(bytes % 256 == 0);
  char *base = static_cast<char *>(std::aligned_alloc(256, bytes));
  CHECK(carve_arena(d, ep, dev_ep, misc, c.planes, base) == bytes);
  CHECK(ep.last == ep.mark + d.E);
  const uintptr_t lo = (uintptr_t)base, hi = lo + bytes;

  // the regions in the arena's order: each begins where the one before it, rounded up to 256 bytes, ends
  const std::vector<Region> want = expected_regions(d, ep, dev_ep, misc, c.planes);
  size_t sum = 0;
  for (size_t i = 0; i < want.size(); ++i) {
    const Region &r = want[i];
    if (!r.expect_null) CHECK(r.at == lo + sum);
    sum += (r.bytes + 255) / 256 * 256;
    if (r.expect_null) {
      CHECK(r.at == 0 && r.bytes == 0);
      continue;
    }
    CHECK(r.at != 0);
    CHECK(r.at % 256 == 0);
    CHECK(r.at >= lo && r.at + r.bytes <= hi);
    for (size_t j = 0; j < i; ++j) {  // pairwise disjoint (a region without bytes overlaps nothing)
      const Region &q = want[j];
      if (q.expect_null || q.bytes == 0 || r.bytes == 0) continue;
      CHECK(r.at + r.bytes <= q.at || q.at + q.bytes <= r.at);
    }
  }
  CHECK(sum == bytes);  // a region whose condition is false takes no space

  // the small words: distinct, the 64-bit ones 8-aligned, all inside the misc region
  const uintptr_t m_lo = (uintptr_t)misc, m_hi = m_lo + sizeof(MiscWords);
  struct Word { uintptr_t at; size_t bytes; };
  const Word words[] = {
      {(uintptr_t)&misc->selftest, 8},   {(uintptr_t)d.slow_pairs, 8},     {(uintptr_t)&misc->clone_skipped, 8},
      {(uintptr_t)d.tickA, 4},             {(uintptr_t)d.tickB, 4},          {(uintptr_t)d.agent_first, 4},
      {(uintptr_t)d.risk_any, 4},          {(uintptr_t)(d.risk_any + 1), 4}, {(uintptr_t)misc->clock2, 4},
      {(uintptr_t)(misc->clock2 + 1), 4}, {(uintptr_t)(misc->clock2 + 2), 4}, {(uintptr_t)(misc->clock2 + 3), 4}};
  const size_t n_words = sizeof words / sizeof words[0];
  for (size_t i = 0; i < n_words; ++i) {
    CHECK(words[i].at % words[i].bytes == 0);
    CHECK(words[i].at >= m_lo && words[i].at + words[i].bytes <= m_hi);
    for (size_t j = 0; j < i; ++j)
      CHECK(words[i].at + words[i].bytes <= words[j].at || words[j].at + words[j].bytes <= words[i].at);
  }
  CHECK(d.risk_stride == d.E);
  std::free(base);
}

// ---- the halves -----------------------------------------------------------------------------------------
// sub_dev as it was when it listed the arrays by hand (tfx_launch.hpp before the table), with h->d as `d`
static Dev old_sub_dev(const Dev &d, int lo, int n, int *clock) {
  Dev s = d;
  const size_t R = (size_t)d.R, I = (size_t)d.I, r = (size_t)d.r, L = (size_t)lo;
  s.E = n;
  s.env_off = d.env_off + lo;
  const size_t tile_pairs = (size_t)d.G * (size_t)d.trows * 64, out_pairs = (size_t)d.G * TFX_KP * 64;
  s.xv = d.xv + L * (d.layout == 1 ? tile_pairs : R * d.C);
  if (d.w) s.w = d.w + L * (d.layout == 1 ? tile_pairs : R * d.C);
  s.leading = d.leading + L * R;
  s.lastcar = d.lastcar + L * R;
  s.obs = d.obs + L * (size_t)d.obs_len;
  s.lights = s.obs + 2 * d.r;
  s.rewards = d.rewards + L * I;
  s.waiting = d.waiting + L * r;
  s.passed_dst = d.passed_dst + L * I;
  s.done_tick = d.done_tick + L;
  if (d.trip_times) s.trip_times = d.trip_times + L * (size_t)d.trip_cap;
  if (d.n_trips) s.n_trips = d.n_trips + L;
  s.rec = d.rec + L * R;
  s.rec2f = d.rec2f + L * R;
  if (d.rsw) s.rsw = d.rsw + L * R;
  if (d.crec) {
    s.crec = d.crec + L * R;
    s.ovf_cnt = d.ovf_cnt + L * R;
  }
  s.rec2c = d.rec2c + L * R;
  if (d.hb) s.hb = d.hb + L * R;
  s.tailx = d.tailx + L * R;
  if (d.taila) s.taila = d.taila + L * R;
  if (d.spawn_arch) s.spawn_arch = d.spawn_arch + L * (size_t)d.n_entry * (size_t)d.spawn_arch_S;
  s.leadx = d.leadx + L * R;
  s.outb = d.outb + L * out_pairs;
  if (d.outw) s.outw = d.outw + L * out_pairs;
  s.env_flag = d.env_flag + L;
  s.env_risk = d.env_risk + L;
  if (d.action_mode == TFX_ACTION_BUFFER && d.action) s.action = d.action + L * I;
  if (d.greedy_act) s.greedy_act = d.greedy_act + L * I;
  if (d.spawn_mode == TFX_SPAWN_COUNTS && d.spawn) s.spawn = d.spawn + L * (size_t)d.n_entry;
  if (clock) {
    s.tickA = clock;
    s.tickB = clock + 1;
    s.risk_any = clock + 2;
  }
  return s;
}

// distinct synthetic addresses, far enough apart for any array of these shapes; never dereferenced
static uintptr_t next_base = (uintptr_t)1 << 32;
template <class T>
static void fake(T *&p) {
  p = reinterpret_cast<T *>(next_base);
  next_base += (uintptr_t)1 << 28;
}

// A bound handle's Dev: the arena carved at a synthetic base, the caller's buffers as tfx_bind_buffers binds them;
// optional: the arrays a handle may or may not have (the side plane where planes = 3 only)
static Dev bound_dev(const Case &c, bool optional, int action_mode, int spawn_mode) {
  Dev d = dev_scalars(c);
  EpDev ep{};
  EpDev *dev_ep = nullptr;
  MiscWords *misc = nullptr;
  char *arena = nullptr;
  fake(arena);
  carve_arena(d, ep, dev_ep, misc, c.planes, arena);
  fake(d.xv); fake(d.leading); fake(d.lastcar); fake(d.obs); fake(d.rewards); fake(d.waiting); fake(d.passed_dst);
  fake(d.done_tick);
  d.lights = d.obs + 2 * d.r;
  d.lights_stride = d.obs_len;
  if (c.planes == 3) fake(d.w);
  if (optional) {
    fake(d.trip_times); fake(d.n_trips); fake(d.greedy_act);
    d.trip_cap = 11;
    if (c.het) {
      fake(d.spawn_arch);
      d.spawn_arch_S = 3;
    }
  } else {
    d.taila = nullptr;  // (with the other optional arrays of the arena null at layout 0: crec, ovf_cnt, rsw, hb)
  }
  d.action_mode = action_mode;
  if (action_mode != TFX_ACTION_CYCLE) fake(d.action);
  d.spawn_mode = spawn_mode;
  if (spawn_mode == TFX_SPAWN_COUNTS) fake(d.spawn);
  return d;
}

struct Arr { uintptr_t at; size_t env_bytes; ArrayKind kind; };
static std::vector<Arr> arrays_of(const Dev &d) {
  std::vector<Arr> v;
  for_each_env_array(d, [&](auto *p, size_t per_env, ArrayKind k) { v.push_back({(uintptr_t)p, per_env * sizeof(*p), k}); });
  return v;
}

static void check_halves(const Case &c, bool optional, int action_mode, int spawn_mode) {
  const Dev whole = bound_dev(c, optional, action_mode, spawn_mode);
  const int E = whole.E, n0 = E / 2;
  int clock_words[4];
  int *const clock = clock_words;
  const Dev a = sub_dev(whole, 0, n0, nullptr), b = sub_dev(whole, n0, E - n0, clock);

  CHECK(a.E == n0 && b.E == E - n0);
  CHECK(a.env_off == whole.env_off && b.env_off == whole.env_off + n0);
  CHECK(a.tickA == whole.tickA && a.tickB == whole.tickB && a.risk_any == whole.risk_any);
  CHECK(b.tickA == clock && b.tickB == clock + 1 && b.risk_any == clock + 2);
  CHECK(a.risk_stride == E && b.risk_stride == E);
  CHECK(a.lights == a.obs + 2 * whole.r && b.lights == b.obs + 2 * whole.r);
  CHECK(a.veh == whole.veh && b.veh == whole.veh && b.agent_first == whole.agent_first && b.slow_pairs == whole.slow_pairs);

  // the two halves tile every visited array exactly
  const std::vector<Arr> w = arrays_of(whole), va = arrays_of(a), vb = arrays_of(b);
  CHECK(va.size() == w.size() && vb.size() == w.size());
  bool bound = false, input = false, scratch = false;
  for (size_t i = 0; i < w.size() && i < va.size() && i < vb.size(); ++i) {
    CHECK(va[i].env_bytes == w[i].env_bytes && vb[i].env_bytes == w[i].env_bytes && va[i].kind == w[i].kind);
    bound |= w[i].kind == ARR_BOUND;
    input |= w[i].kind == ARR_INPUT;
    scratch |= w[i].kind == ARR_SCRATCH;
    if (w[i].at == 0) {
      CHECK(va[i].at == 0 && vb[i].at == 0);
      continue;
    }
    CHECK(va[i].at == w[i].at);
    CHECK(vb[i].at == w[i].at + (size_t)n0 * w[i].env_bytes);
    CHECK(vb[i].at + (size_t)(E - n0) * w[i].env_bytes == w[i].at + (size_t)E * w[i].env_bytes);
  }
  CHECK(bound && input && scratch);

  // the per-tick inputs move only in the modes that hold something per env
  const size_t I = (size_t)whole.I, ne = (size_t)whole.n_entry;
  if (action_mode == TFX_ACTION_BUFFER) CHECK(b.action == whole.action + (size_t)n0 * I);
  else CHECK(b.action == whole.action);
  if (spawn_mode == TFX_SPAWN_COUNTS) CHECK(b.spawn == whole.spawn + (size_t)n0 * ne);
  else CHECK(b.spawn == whole.spawn);
  // what the second half of a split call works on, array by array
  CHECK(b.xv == whole.xv + (size_t)n0 * (c.layout == 1 ? (size_t)whole.G * whole.trows * 64 : (size_t)whole.R * whole.C));
  CHECK(b.obs == whole.obs + (size_t)n0 * whole.obs_len);
  CHECK(b.done_tick == whole.done_tick + n0 && b.env_flag == whole.env_flag + n0 && b.env_risk == whole.env_risk + n0);
  CHECK(b.outb == whole.outb + (size_t)n0 * whole.G * TFX_KP * 64);
  if (!optional) {
    CHECK(!b.trip_times && !b.n_trips && !b.taila && !b.spawn_arch && !b.greedy_act);
    if (c.planes == 2) CHECK(!b.w);
    if (c.layout == 0) CHECK(!b.crec && !b.ovf_cnt && !b.rsw && !b.hb);
  } else {
    CHECK(b.trip_times == whole.trip_times + (size_t)n0 * 11);
    if (c.het) CHECK(b.spawn_arch == whole.spawn_arch + (size_t)n0 * ne * 3);
  }

  // the unchanged rule: byte for byte what the hand-written list gave
  const int los[] = {0, 1, E / 2, E - 1};
  for (int lo : los) {
    if (lo >= E) continue;
    for (int *ck : {(int *)nullptr, clock}) {
      const Dev got = sub_dev(whole, lo, E - lo, ck), want = old_sub_dev(whole, lo, E - lo, ck);
      CHECK(std::memcmp(&got, &want, sizeof(Dev)) == 0);
    }
  }
}

int main() {
  // 1x1, the smallest; 2x3 with an odd batch (unequal halves); 16x16 with 128-car rings: 17 tiles per env, trows = 128
  const Shape shapes[] = {{1, 1, 3, 1}, {2, 3, 10, 5}, {16, 16, 130, 3}};
  int n_cases = 0;
  for (const Shape &s : shapes)
    for (int layout = 0; layout < 2; ++layout)
      for (int planes = 2; planes <= 3; ++planes)
        for (int het = 0; het < 2; ++het) {
          if (het && (layout != 1 || planes != 3)) continue;  // (tfx_create admits heterogeneous cars there only)
          const Case c{s, layout, planes, het};
          check_arena(c);
          for (int optional = 0; optional < 2; ++optional) {
            check_halves(c, optional != 0, TFX_ACTION_BUFFER, TFX_SPAWN_COUNTS);
            check_halves(c, optional != 0, TFX_ACTION_BROADCAST, TFX_SPAWN_PERIODIC);
            check_halves(c, optional != 0, TFX_ACTION_CYCLE, TFX_SPAWN_NONE);
          }
          ++n_cases;
        }
  CHECK(n_cases == 15);
  {  // the shapes are the ones meant
    const Dev d = dev_scalars({shapes[2], 1, 3, 0});
    CHECK(d.G == 17 && d.trows == 128 && d.R == 1088);
  }
  std::printf(failures ? "%d checks failed\n" : "dev layout ok\n", failures);
  return failures ? EXIT_FAILURE : EXIT_SUCCESS;
}
