// CPU test of bourse_amd/csrc/account_fold.hpp (tests/test_accounts_cpu.py compiles and runs it): the per-record
// arithmetic of the trader accounts - who buys, the signed deltas, the 32 x 32 -> 64-bit product - folded over the records
// of <records file> and compared with the rows of <expected file>, which tests/accounts_model.py printed.
//   records:  n_traders n_records, then one line per record: side_is_bid price vol active_trader passive_trader
//   expected: one line per trader: position cash volume fills, each as an unsigned 64-bit word (two's complement)
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "../../bourse_amd/csrc/account_fold.hpp"

using namespace bkd::accounts;

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  std::FILE* in = std::fopen(argv[1], "r");
  std::FILE* ex = std::fopen(argv[2], "r");
  if (!in || !ex) return 2;
  uint32_t n_traders = 0;
  uint64_t n_records = 0;
  if (std::fscanf(in, "%" SCNu32 " %" SCNu64, &n_traders, &n_records) != 2) return 2;
  std::vector<Delta> rows(n_traders, Delta{0, 0, 0, 0});
  for (uint64_t i = 0; i < n_records; ++i) {
    uint32_t side = 0, price = 0, vol = 0, ta = 0, tp = 0;
    if (std::fscanf(in, "%" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32 " %" SCNu32, &side, &price, &vol, &ta, &tp) != 5) return 2;
    const Parties p = parties(side, ta, tp);
    if (p.buyer < n_traders) add(rows[p.buyer], buyer_delta(price, vol));
    if (p.seller < n_traders) add(rows[p.seller], seller_delta(price, vol));
  }
  int bad = 0;
  for (uint32_t t = 0; t < n_traders; ++t) {
    uint64_t w[4] = {0, 0, 0, 0};
    if (std::fscanf(ex, "%" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64, &w[0], &w[1], &w[2], &w[3]) != 4) return 2;
    const Delta& r = rows[t];
    if (r.position != w[0] || r.cash != w[1] || r.volume != w[2] || r.fills != w[3]) {
      if (bad++ < 8)
        std::printf("trader %u: {%" PRIu64 ", %" PRIu64 ", %" PRIu64 ", %" PRIu64 "} vs {%" PRIu64 ", %" PRIu64 ", %" PRIu64 ", %" PRIu64
                    "}\n", t, r.position, r.cash, r.volume, r.fills, w[0], w[1], w[2], w[3]);
    }
  }
  if (bad) return 1;
  // the product is the full 64-bit one, and the signs are the buyer's and the seller's
  if (notional(0xFFFFFFFFu, 0xFFFFFFFFu) != 0xFFFFFFFE00000001ull) return 1;
  if (buyer_delta(3, 5).cash != 0ull - 15ull || seller_delta(3, 5).position != 0ull - 5ull) return 1;
  std::printf("account_fold ok %" PRIu64 " records %u traders\n", n_records, n_traders);
  return 0;
}
