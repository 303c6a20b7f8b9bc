// CPU test of bourse_amd/csrc/trade_bar_fold.hpp (tests/test_trade_bars_cpu.py compiles and runs it): the per-record
// arithmetic of the trade bars - which side the aggressor took, the 32 x 32 -> 64-bit notional - and the combination of
// partial bars, over the steps of <records file>, compared with the rows of <expected file>, which
// tests/trade_bars_model.py printed.
//   records:  n_steps, then per step one line "n_records n_cuts cut_1 .. cut_n_cuts" (0 < cut_1 < .. < n_records: where the
//             step's records are split into partial bars) and one line per record: side_is_bid price vol
//   expected: one line per step: open high low close buy_vol sell_vol notional n_buy n_sell
// A step's partial bars are each folded record by record (of_record, extend) and then combined twice, from the left and
// from the right: both must give the expected row.  A step without a record is idle(close of the step before it).
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "../../bourse_amd/csrc/trade_bar_fold.hpp"

using namespace bkd::trade_bars;

static bool same(const Bar& r, const uint64_t w[9]) {
  return r.open == w[0] && r.high == w[1] && r.low == w[2] && r.close == w[3] && r.buy_vol == w[4] && r.sell_vol == w[5] &&
         r.notional == w[6] && r.n_buy == w[7] && r.n_sell == w[8];
}

static void show(const char* how, uint64_t step, const Bar& r, const uint64_t w[9]) {
  std::printf("step %" PRIu64 " (%s): {%u, %u, %u, %u, %" PRIu64 ", %" PRIu64 ", %" PRIu64 ", %u, %u} vs {%" PRIu64 ", %" PRIu64
              ", %" PRIu64 ", %" PRIu64 ", %" PRIu64 ", %" PRIu64 ", %" PRIu64 ", %" PRIu64 ", %" PRIu64 "}\n",
              step, how, r.open, r.high, r.low, r.close, r.buy_vol, r.sell_vol, r.notional, r.n_buy, r.n_sell, w[0], w[1], w[2],
              w[3], w[4], w[5], w[6], w[7], w[8]);
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  std::FILE* in = std::fopen(argv[1], "r");
  std::FILE* ex = std::fopen(argv[2], "r");
  if (!in || !ex) return 2;
  uint64_t n_steps = 0, n_total = 0, n_partials = 0;
  if (std::fscanf(in, "%" SCNu64, &n_steps) != 1) return 2;
  int bad = 0;
  uint32_t prev_close = 0;
  for (uint64_t s = 0; s < n_steps; ++s) {
    uint64_t n = 0, n_cuts = 0;
    if (std::fscanf(in, "%" SCNu64 " %" SCNu64, &n, &n_cuts) != 2) return 2;
    std::vector<uint64_t> cuts(n_cuts);
    for (uint64_t& c : cuts)
      if (std::fscanf(in, "%" SCNu64, &c) != 1) return 2;
    cuts.push_back(n);
    std::vector<Bar> partial;
    uint64_t next_cut = 0;
    bool open_partial = false;
    for (uint64_t i = 0; i < n; ++i) {
      uint32_t side = 0, price = 0, vol = 0;
      if (std::fscanf(in, "%" SCNu32 " %" SCNu32 " %" SCNu32, &side, &price, &vol) != 3) return 2;
      const Bar one = of_record(price, vol, side);
      if (open_partial)
        partial.back() = extend(partial.back(), one);
      else
        partial.push_back(one);
      open_partial = true;
      if (i + 1 == cuts[next_cut]) open_partial = false, ++next_cut;
    }
    n_total += n, n_partials += partial.size();
    Bar left = idle(prev_close), right = left;
    if (!partial.empty()) {
      left = partial.front();
      for (size_t p = 1; p < partial.size(); ++p) left = extend(left, partial[p]);
      right = partial.back();
      for (size_t p = partial.size() - 1; p-- > 0;) right = extend(partial[p], right);
    }
    uint64_t w[9];
    for (uint64_t& x : w)
      if (std::fscanf(ex, "%" SCNu64, &x) != 1) return 2;
    if (!same(left, w) && bad++ < 8) show("from the left", s, left, w);
    if (!same(right, w) && bad++ < 8) show("from the right", s, right, w);
    prev_close = left.close;
  }
  if (bad) return 1;
  // the product is the full 64-bit one, side_is_bid == 0 is the aggressor buying, and the row's words lie as bk_trade_bar's
  if (notional(0xFFFFFFFFu, 0xFFFFFFFFu) != 0xFFFFFFFE00000001ull) return 1;
  if (!is_buy(0) || is_buy(1) || of_record(7, 5, 0).buy_vol != 5 || of_record(7, 5, 1).sell_vol != 5) return 1;
  Bar r = of_record(1, 2, 0);
  r.high = 3, r.low = 4, r.close = 5, r.buy_vol = 0x700000006ull, r.sell_vol = 0x900000008ull, r.notional = 0xB0000000Aull;
  r.n_buy = 12, r.n_sell = 13;
  uint32_t w[12];
  words(r, w);
  const uint32_t want[12] = {1, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13};
  for (int i = 0; i < 12; ++i)
    if (w[i] != want[i]) return 1;
  std::printf("trade_bar_fold ok %" PRIu64 " steps %" PRIu64 " records %" PRIu64 " partial bars\n", n_steps, n_total, n_partials);
  return 0;
}
