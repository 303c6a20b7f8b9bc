// CPU test of bourse_amd/csrc/quote_rows.hpp (tests/test_quotes_cpu.py compiles and runs it): the per-position decision of
// bk_submit_quotes - the keepers of a trader's list, an entry slot's element, a side's new order - applied to the traders of
// <cases file> the way quotes_ingress.hpp applies it (every grid position walks the trader's list in order up to the first
// unused entry, then makes its own element), printed to <grid file> for the test to compare with tests/quotes_model.py.
//   cases: n_cases, then per case: depth, one line per entry: order_id price vol side_is_bid, then the quote row's four words
//   grid:  per case and grid position one line: action side vol price order_id
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "../../bourse_amd/csrc/quote_rows.hpp"

using namespace bkd::quotes;

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  std::FILE* in = std::fopen(argv[1], "r");
  std::FILE* out = std::fopen(argv[2], "w");
  if (!in || !out) return 2;
  uint32_t n_cases = 0;
  if (std::fscanf(in, "%" SCNu32, &n_cases) != 1) return 2;
  for (uint32_t c = 0; c < n_cases; ++c) {
    uint32_t depth = 0;
    if (std::fscanf(in, "%" SCNu32, &depth) != 1) return 2;
    std::vector<Entry> list(depth);
    for (Entry& e : list)
      if (std::fscanf(in, "%" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32, &e.order_id, &e.price, &e.vol, &e.side_is_bid) != 4) return 2;
    Quote q;
    if (std::fscanf(in, "%" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32, &q.bid_price, &q.bid_vol, &q.ask_price, &q.ask_vol) != 4) return 2;
    for (uint32_t at = 0; at < depth + 2u; ++at) {
      Keepers keep = no_keepers();
      Entry mine = {NO_ORDER, 0u, 0u, 0u};
      for (uint32_t k = 0; k < depth; ++k) {
        if (list[k].order_id == NO_ORDER) break;
        see_entry(keep, q, k, list[k]);
        if (k == at) mine = list[k];
      }
      const Element x = at < depth ? entry_element(keep, q, at, mine) : new_element(keep, q, at == depth ? 1u : 0u);
      std::fprintf(out, "%" PRIu32 " %" PRIu32 " %" PRIu32 " %" PRIu32 " %" PRIu32 "\n", x.action, x.side, x.vol, x.price, x.order_id);
    }
  }
  std::fclose(out);
  // the constants the kernel and the header's callers rely on
  if (KEEP != 0xFFFFFFFFu || ACT_MODIFY != 0x80000003u || SIDE_HAS_VOL != 4u) return 1;
  if (sizeof(Quote) != 16 || sizeof(Entry) != 16) return 1;
  const Element none = no_element();
  if (none.action || none.side || none.vol || none.price || none.order_id) return 1;
  std::printf("quote_rows ok %" PRIu32 " cases\n", n_cases);
  return 0;
}
