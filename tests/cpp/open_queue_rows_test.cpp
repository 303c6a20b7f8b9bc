// CPU test of bourse_amd/csrc/open_queue_rows.hpp (tests/test_open_queue_cpu.py compiles and runs it): the row arithmetic of
// the queue table - the empty row, where a live order stands relative to a listed one, adding one order to a row, the
// row's words - applied to the pools of <pools file> the way open_queue.hpp applies it (a first walk over the live slots
// finds the listed order's stamp by its id, a second adds every live slot to the row; an id that is not live keeps the empty
// row), printed to <rows file> for the test to compare with tests/open_queue_model.py.
//   pools: n_pools, then per pool: n_slots n_entries, then one line per slot: live id price vol side_is_bid seq, then one
//          line per entry: order_id price side_is_bid
//   rows:  per pool and entry one line: the row's eight words
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "../../bourse_amd/csrc/open_queue_rows.hpp"

using namespace bkd::open_queue;

struct Slot {
  uint32_t live, id, price, vol, side, seq;
};
struct Listed {
  uint32_t id, price, side;
};

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  std::FILE* in = std::fopen(argv[1], "r");
  std::FILE* out = std::fopen(argv[2], "w");
  if (!in || !out) return 2;
  uint32_t n_pools = 0;
  if (std::fscanf(in, "%" SCNu32, &n_pools) != 1) return 2;
  for (uint32_t p = 0; p < n_pools; ++p) {
    uint32_t n_slots = 0, n_entries = 0;
    if (std::fscanf(in, "%" SCNu32 " %" SCNu32, &n_slots, &n_entries) != 2) return 2;
    std::vector<Slot> pool(n_slots);
    for (Slot& s : pool)
      if (std::fscanf(in, "%" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32, &s.live, &s.id, &s.price, &s.vol,
                      &s.side, &s.seq) != 6)
        return 2;
    for (uint32_t e = 0; e < n_entries; ++e) {
      Listed o;
      if (std::fscanf(in, "%" SCNu32 " %" SCNu32 " %" SCNu32, &o.id, &o.price, &o.side) != 3) return 2;
      uint32_t stamp = 0;
      bool found = false;
      for (const Slot& s : pool)
        if (s.live && o.id != 0xFFFFFFFFu && s.id == o.id) stamp = s.seq, found = true;
      Row row = empty_row();
      for (const Slot& s : pool)
        if (s.live) add_order(row, found ? place(o.side, o.price, stamp, s.side, s.price, s.seq) : 0u, s.vol);
      uint32_t w[8];
      row_words(row, w);
      for (uint32_t v : w) std::fprintf(out, "%" PRIu32 " ", v);
      std::fprintf(out, "\n");
    }
  }
  std::fclose(out);
  // the empty row is what the header documents, an order is level with itself and not ahead of itself
  const Row e = empty_row();
  if (e.ahead_vol || e.level_ahead_vol || e.level_vol || e.ahead_orders || e.level_ahead_orders) return 1;
  if (place(1, 100, 7, 1, 100, 7) != LEVEL || place(0, 100, 7, 0, 100, 7) != LEVEL) return 1;
  if (place(1, 100, 7, 0, 100, 3) != 0u || place(0, 100, 7, 1, 99, 3) != 0u) return 1;  // the other side never counts
  if (sizeof(Row) != 32) return 1;
  std::printf("open_queue_rows ok %" PRIu32 " pools\n", n_pools);
  return 0;
}
