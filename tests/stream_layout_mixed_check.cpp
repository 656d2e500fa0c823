// Stand-alone host check of stream_layout's up-front form (csrc/tfx_stream_layout.hpp): the one allocation of a mixed
// demand (tfx_set_demand_mixed) - counts and archetype rows share a chunk, no per-entry car counters.  Built with
// -fsanitize=address,undefined and run by tests/test_stream_layout_mixed.py; it needs no device.  The rows rule below
// restates what tfx.h promises - it is NOT taken from the header under test.
#include <cstdio>
#include <cstdlib>

#include "tfx_stream_layout.hpp"

static int failures = 0;
#define CHECK(cond)                                                                         \
  do {                                                                                      \
    if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
  } while (0)

// 64 rows, fewer beyond 32 MB of counts or 256 MB of archetype rows, never below one
static long rows_mixed(long E, long ne, long S) {
  long rows = ((long)32 << 20) / (E * ne * 4);
  const long arows = ((long)256 << 20) / (E * ne * S);
  if (arows < rows) rows = arows;
  return rows < 1 ? 1 : (rows > 64 ? 64 : rows);
}

int main() {
  const long Es[] = {1, 5, 4096, 65536}, nes[] = {6, 64}, Ss[] = {1, 4, 13, 16, 35, 64};
  for (long E : Es)
    for (long ne : nes)
      for (long S : Ss) {
        const size_t n_tables = (size_t)2 * 3 * (137 + ne + 3);  // count_cdf | road_cdf | row_cdf
        const StreamLayout l = stream_layout(E, ne, n_tables, (int)S, true);
        const size_t per_tick = (size_t)E * ne;
        CHECK(l.rows == rows_mixed(E, ne, S));
        CHECK(l.counts == 0);
        CHECK(l.gap == (size_t)l.rows * per_tick * 4);
        CHECK(l.draws == l.gap + (size_t)E * 4 && l.sid == l.draws + (size_t)E * 4 && l.tables == l.sid + (size_t)E * 4);
        CHECK(l.seq == l.tables + n_tables * 4);
        CHECK(l.arch == l.seq);  // no seq words: rule 5 keeps no position
        CHECK(l.arch % 4 == 0);
        CHECK(l.bytes == l.arch + (size_t)l.rows * per_tick * S);
        // what the other streams get is what they got
        const StreamLayout p = stream_layout(E, ne, n_tables, (int)S), q = stream_layout(E, ne, n_tables, (int)S, false);
        CHECK(p.rows == q.rows && p.bytes == q.bytes && p.arch == q.seq + per_tick * 4);
      }
  // a 10-tick decision of 4096 envs x 64 entry roads fits at every S the capacity of 66 allows
  CHECK(stream_layout(4096, 64, 0, 13, true).rows == 32);
  CHECK(stream_layout(4096, 64, 0, 16, true).rows == 32);
  CHECK(stream_layout(4096, 64, 0, 35, true).rows == 29);
  CHECK(stream_layout(4096, 64, 0, 64, true).rows == 16);
  CHECK(stream_layout(4096, 64, 0, 64).rows == 4);
  std::printf(failures ? "%d checks failed\n" : "mixed stream layout ok\n", failures);
  return failures ? EXIT_FAILURE : EXIT_SUCCESS;
}
