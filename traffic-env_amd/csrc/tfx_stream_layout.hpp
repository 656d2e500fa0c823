// tfx_stream_layout.hpp - how the ONE device allocation of a handle's arrival stream (ArrivalStream, tfx_handle.hpp) is
// carved: counts | gap | draws | sid | tables | seq | archetype rows.  Plain C++ without a device, so the arithmetic can
// be checked on the host alone (tests/stream_layout_check.cpp).
#pragma once
#include <cstddef>

struct StreamLayout {
  int rows;  // ticks of arrival counts the buffer holds: a longer call is drawn in chunks of this many
  // byte offsets of the regions: counts int [rows][E][n_entry]; gap int [E], draws and sid unsigned [E] (the words a
  // clone with TFX_CLONE_STREAM copies); the kind's tables, n_tables words; heterogeneous cars: seq unsigned
  // [E][n_entry] and the archetype rows uint8 [rows][E][n_entry][S], last because they are bytes
  size_t counts, gap, draws, sid, tables, seq, arch;
  size_t bytes;
};

// Rows of E x n_entry counts: at most 64, at most ~32 MB; with S > 0 archetype rows per entry road and tick also
// E x n_entry x S of those per tick within ~64 MB (cfg2: 17 MB per tick) - one chunk serves counts and archetype rows
// together.  upfront: a mixed demand (tfx_set_demand_mixed).  Rule 5 is stateless: no per-entry car counters (seq); and
// a whole decision must fit the chunk, where rule 1 draws a decision tick by tick: ~256 MB of archetype rows (4096 envs
// x 64 entry roads hold 16 ticks at S = 64, the most their capacity of 66 allows, and the 32 of the counts up to S = 32).
inline StreamLayout stream_layout(long E, long n_entry, size_t n_tables, int S, bool upfront = false) {
  long rows = ((long)32 << 20) / (E * n_entry * 4);
  if (S > 0) {
    const long arows = ((long)(upfront ? 256 : 64) << 20) / (E * n_entry * S);
    if (arows < rows) rows = arows;
  }
  StreamLayout l{};
  l.rows = (int)(rows < 1 ? 1 : (rows > 64 ? 64 : rows));
  const size_t env = (size_t)E * 4, per_tick = (size_t)E * n_entry;
  l.counts = 0;
  l.gap = l.counts + (size_t)l.rows * per_tick * 4;
  l.draws = l.gap + env;
  l.sid = l.draws + env;
  l.tables = l.sid + env;
  l.seq = l.tables + n_tables * 4;
  l.arch = l.seq + (S > 0 && !upfront ? per_tick * 4 : 0);
  l.bytes = l.arch + (S > 0 ? (size_t)l.rows * per_tick * S : 0);
  return l;
}
