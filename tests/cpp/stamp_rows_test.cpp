// CPU test of bourse_amd/csrc/stamp_rows.hpp (tests/test_stamp_rows_cpu.py compiles and runs it): the rank rule of the
// stamp compaction applied to the pools of <pools file>, printed to <out file> for the test to compare with a plain sort
// (tests/stamp_model.py); here: applying it twice changes nothing more, and the host's room accounting.
//   pools: n_pools, then per pool: seq_ctr n_slots, then one line per slot: live seq
//   out:   per pool one line: the new counter, then the n_slots new stamps
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "../../bourse_amd/csrc/stamp_rows.hpp"

using namespace bkd::stamps;

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  std::FILE* in = std::fopen(argv[1], "r");
  std::FILE* out = std::fopen(argv[2], "w");
  if (!in || !out) return 2;
  uint32_t n_pools = 0;
  if (std::fscanf(in, "%" SCNu32, &n_pools) != 1) return 2;
  for (uint32_t p = 0; p < n_pools; ++p) {
    uint32_t ctr = 0, n = 0;
    if (std::fscanf(in, "%" SCNu32 " %" SCNu32, &ctr, &n) != 2) return 2;
    std::vector<uint8_t> live(n);
    std::vector<uint32_t> seq(n), once(n), twice(n);
    for (uint32_t i = 0; i < n; ++i) {
      uint32_t l = 0;
      if (std::fscanf(in, "%" SCNu32 " %" SCNu32, &l, &seq[i]) != 2) return 2;
      live[i] = static_cast<uint8_t>(l);
    }
    const uint32_t c1 = compact(ctr, n, live.data(), seq.data(), once.data());
    const uint32_t c2 = compact(c1, n, live.data(), once.data(), twice.data());
    if (c2 != c1 || twice != once) {  // a fixed point
      std::printf("pool %" PRIu32 ": a second compaction changed the stamps\n", p);
      return 1;
    }
    std::fprintf(out, "%" PRIu32, c1);
    for (uint32_t v : once) std::fprintf(out, " %" PRIu32, v);
    std::fprintf(out, "\n");
  }
  std::fclose(out);
  // ages wrap: the counter just past 0, a stamp just below 2^32
  if (age(2u, 0xFFFFFFFEu) != 4u || age(2u, 1u) != 1u) return 1;
  if (older(2u, 1u, 0xFFFFFFFEu) != 1u || older(2u, 0xFFFFFFFEu, 1u) != 0u || older(2u, 1u, 1u) != 0u) return 1;
  // the room: H_SEQ may reach the limit and not pass it
  Room room;
  if (room.limit != 0xFFFFFFFFull || room.bound != 0 || room.needs_compaction(0xFFFFFFFFull) || !room.needs_compaction(0x100000000ull))
    return 1;
  room.spend(0xFFFFFFF0ull);
  if (room.needs_compaction(15) || !room.needs_compaction(16)) return 1;
  room.compacted(512);
  if (room.bound != 512 || room.after_compaction(512) != 0xFFFFFFFFull - 512) return 1;
  room.raise(100);
  if (room.bound != 512) return 1;
  room.raise(0xFFFFFFFBull);  // a reset to a snapshot taken at a larger bound
  if (room.bound != 0xFFFFFFFBull || room.needs_compaction(4) || !room.needs_compaction(5)) return 1;
  Room small;
  small.limit = 64 + 300;
  if (small.after_compaction(64) != 300 || small.after_compaction(512) != 0) return 1;
  std::printf("stamp_rows ok %" PRIu32 " pools\n", n_pools);
  return 0;
}
