// CPU test of bourse_amd/csrc/open_order_rows.hpp (tests/test_open_orders_cpu.py compiles and runs it): the row arithmetic
// of the open-order tables - adding one resting order to a summary, the empty row and entry, packing an entry, the row's
// words - applied to the pools of <pools file> the way open_orders.hpp applies it (slots in pool order, an entry's place =
// the number of the trader's slots with a smaller id), printed to <rows file> for the test to compare with
// tests/open_orders_model.py.
//   pools: n_pools, then per pool: n_slots n_traders depth, then one line per slot: live id price vol side_is_bid trader
//   rows:  per pool and trader one line: the summary's eight words, then depth x {order_id price vol side_is_bid}
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "../../bourse_amd/csrc/open_order_rows.hpp"

using namespace bkd::open_orders;

struct Slot {
  uint32_t live, id, price, vol, side, trader;
};

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  std::FILE* in = std::fopen(argv[1], "r");
  std::FILE* out = std::fopen(argv[2], "w");
  if (!in || !out) return 2;
  uint32_t n_pools = 0;
  if (std::fscanf(in, "%" SCNu32, &n_pools) != 1) return 2;
  for (uint32_t p = 0; p < n_pools; ++p) {
    uint32_t n_slots = 0, n_traders = 0, depth = 0;
    if (std::fscanf(in, "%" SCNu32 " %" SCNu32 " %" SCNu32, &n_slots, &n_traders, &depth) != 3) return 2;
    std::vector<Slot> pool(n_slots);
    for (Slot& s : pool)
      if (std::fscanf(in, "%" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32, &s.live, &s.id, &s.price, &s.vol,
                      &s.side, &s.trader) != 6)
        return 2;
    for (uint32_t x = 0; x < n_traders; ++x) {
      Summary sum = empty_summary();
      std::vector<Entry> list(depth, empty_entry());
      for (const Slot& s : pool) {
        if (!s.live || s.trader != x) continue;
        add_order(sum, s.side, s.price, s.vol);
        uint32_t rank = 0;
        for (const Slot& o : pool) rank += o.live && o.trader == x && o.id < s.id ? 1u : 0u;
        if (rank < depth) list[rank] = pack_entry(s.id, s.price, s.vol, s.side);
      }
      for (uint32_t k = entries_used(sum, depth); k < depth; ++k)
        if (list[k].order_id != NO_ORDER) return 1;  // the used entries are the first ones
      uint32_t w[8];
      summary_words(sum, w);
      for (uint32_t v : w) std::fprintf(out, "%" PRIu32 " ", v);
      for (const Entry& e : list) std::fprintf(out, "%" PRIu32 " %" PRIu32 " %" PRIu32 " %" PRIu32 " ", e.order_id, e.price, e.vol, e.side_is_bid);
      std::fprintf(out, "\n");
    }
  }
  std::fclose(out);
  // the empty row and entry are what the header documents
  const Summary e = empty_summary();
  if (e.bid_vol || e.ask_vol || e.n_bid || e.n_ask || e.best_bid || e.best_ask != 0xFFFFFFFFu) return 1;
  const Entry n = empty_entry();
  if (n.order_id != 0xFFFFFFFFu || n.price || n.vol || n.side_is_bid) return 1;
  if (sizeof(Summary) != 32 || sizeof(Entry) != 16) return 1;
  std::printf("open_order_rows ok %" PRIu32 " pools\n", n_pools);
  return 0;
}
