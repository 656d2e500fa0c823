// Stand-alone host check of stream_layout (csrc/tfx_stream_layout.hpp), the carving of an arrival stream's one device
// allocation.  Built with -fsanitize=address,undefined and run by tests/test_stream_layout.py; it needs no device.
// The rows formulas below restate, setter by setter, what tfx_set_poisson, tfx_set_regular and tfx_set_demand computed
// when each carved a buffer of its own - they are NOT taken from the header under test.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "tfx_stream_layout.hpp"

static int failures = 0;
#define CHECK(cond)                                                                         \
  do {                                                                                      \
    if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
  } while (0)

static long clamp64(long rows) { return rows < 1 ? 1 : (rows > 64 ? 64 : rows); }

// tfx_set_poisson: 32 MB of counts; heterogeneous cars: and 64 MB of E x n_entry x S archetype rows
static long rows_poisson(long E, long ne, bool het, long S) {
  long rows = ((long)32 << 20) / (E * ne * 4);
  if (het) {
    const long arows = ((long)64 << 20) / (E * ne * S);
    if (arows < rows) rows = arows;
  }
  return clamp64(rows);
}
// tfx_set_regular, tfx_set_demand: the counts alone
static long rows_regular(long E, long ne) { return clamp64(((long)32 << 20) / (E * ne * 4)); }
static long rows_demand(long E, long ne) {
  long rows = ((long)32 << 20) / (E * ne * 4);
  rows = rows < 1 ? 1 : (rows > 64 ? 64 : rows);
  return rows;
}

struct Region { const char *name; size_t off, len; };

// the regions in order, disjoint, 4-byte aligned, inside `bytes`, and together exactly `bytes`
static void check_regions(const StreamLayout &l, long E, long ne, size_t n_tables, int S) {
  const size_t per_tick = (size_t)E * ne;
  const std::vector<Region> regions = {
      {"counts", l.counts, (size_t)l.rows * per_tick * 4}, {"gap", l.gap, (size_t)E * 4},
      {"draws", l.draws, (size_t)E * 4},                   {"sid", l.sid, (size_t)E * 4},
      {"tables", l.tables, n_tables * 4},                  {"seq", l.seq, S > 0 ? per_tick * 4 : 0},
      {"arch", l.arch, S > 0 ? (size_t)l.rows * per_tick * S : 0}};
  size_t end = 0;
  for (const Region &r : regions) {
    CHECK(r.off % 4 == 0);
    CHECK(r.off >= end);  // (in order: no region begins inside the one before)
    CHECK(r.off + r.len <= l.bytes);
    end = r.off + r.len;
  }
  CHECK(end == l.bytes);
  CHECK(l.counts == 0);
}

int main() {
  const long Es[] = {1, 5, 4096}, nes[] = {6, 64};
  const int S = 64;  // capacity 66: the cars a road holds
  for (long E : Es)
    for (long ne : nes) {
      // Poisson, one archetype and several: the gap table of a rate (some hundred thresholds)
      for (int het = 0; het < 2; ++het) {
        const size_t n_cdf = 137;
        const StreamLayout l = stream_layout(E, ne, n_cdf, het ? S : 0);
        CHECK(l.rows == rows_poisson(E, ne, het != 0, S));
        check_regions(l, E, ne, n_cdf, het ? S : 0);
        const size_t n_counts = (size_t)l.rows * E * ne, n_seq = het ? (size_t)E * ne : 0;
        CHECK(l.bytes == (n_counts + 3 * (size_t)E + n_cdf + n_seq) * 4 + (het ? (size_t)l.rows * E * ne * S : 0));
      }
      {  // regular: no tables
        const StreamLayout l = stream_layout(E, ne, 0, 0);
        CHECK(l.rows == rows_regular(E, ne));
        check_regions(l, E, ne, 0, 0);
        CHECK(l.bytes == ((size_t)l.rows * E * ne + 3 * (size_t)E) * 4);
      }
      {  // demand: K x S x n_cdf count thresholds and K x S x n_entry road thresholds
        const size_t n_cc = (size_t)2 * 3 * 137, n_rc = (size_t)2 * 3 * ne;
        const StreamLayout l = stream_layout(E, ne, n_cc + n_rc, 0);
        CHECK(l.rows == rows_demand(E, ne));
        check_regions(l, E, ne, n_cc + n_rc, 0);
        CHECK(l.bytes == ((size_t)l.rows * E * ne + 3 * (size_t)E + n_cc + n_rc) * 4);
      }
    }
  // the caps bite: 4096 envs x 64 entry roads hold 32 rows of counts, 4 with archetype rows; one env holds 64
  CHECK(stream_layout(4096, 64, 0, 0).rows == 32);
  CHECK(stream_layout(4096, 64, 0, S).rows == 4);
  CHECK(stream_layout(1, 6, 0, S).rows == 64);
  std::printf(failures ? "%d checks failed\n" : "stream layout ok\n", failures);
  return failures ? EXIT_FAILURE : EXIT_SUCCESS;
}
