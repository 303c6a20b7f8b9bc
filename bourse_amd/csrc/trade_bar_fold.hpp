// trade_bar_fold.hpp - what ONE trade record adds to a book's bar of the step, and how the bar of a later run of records
// extends the bar of an earlier one (bk_trade_bars_enable).
//
// Compiled by the device fold (trade_bars.hpp) and by a CPU test (tests/cpp/trade_bar_fold_test.cpp): no HIP type, no
// intrinsic.  A record is {price, vol, side_is_bid}; side_is_bid is the PASSIVE order's side, read as account_fold.hpp
// reads it:
//   side_is_bid == 0   the passive order was an ask: the AGGRESSOR bought  -> buy_vol, n_buy;
//   side_is_bid != 0   the passive order was a bid:  the aggressor sold    -> sell_vol, n_sell.
// The 64-bit words are sums modulo 2^64; vol * price is the full 32 x 32 -> 64-bit product; the counts wrap modulo 2^32.
// A Bar always covers at least one record: a step without one has the carried bar of idle().
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BKD_BAR_HD __host__ __device__ inline
#else
#define BKD_BAR_HD inline
#endif

namespace bkd {
namespace trade_bars {

struct Bar {  // bk_trade_bar, field by field
  uint32_t open, high, low, close;
  uint64_t buy_vol, sell_vol;
  uint64_t notional;
  uint32_t n_buy, n_sell;
};

BKD_BAR_HD bool is_buy(uint32_t side_is_bid) { return side_is_bid == 0u; }

BKD_BAR_HD uint64_t notional(uint32_t price, uint32_t vol) { return static_cast<uint64_t>(price) * static_cast<uint64_t>(vol); }

// the bar of one record
BKD_BAR_HD Bar of_record(uint32_t price, uint32_t vol, uint32_t side_is_bid) {
  const bool buy = is_buy(side_is_bid);
  Bar r;
  r.open = r.high = r.low = r.close = price;
  r.buy_vol = buy ? vol : 0u;
  r.sell_vol = buy ? 0u : vol;
  r.notional = notional(price, vol);
  r.n_buy = buy ? 1u : 0u;
  r.n_sell = buy ? 0u : 1u;
  return r;
}

// the bar of the records of `a` followed by the records of `b`
BKD_BAR_HD Bar extend(const Bar& a, const Bar& b) {
  Bar r;
  r.open = a.open;
  r.high = a.high > b.high ? a.high : b.high;
  r.low = a.low < b.low ? a.low : b.low;
  r.close = b.close;
  r.buy_vol = a.buy_vol + b.buy_vol;
  r.sell_vol = a.sell_vol + b.sell_vol;
  r.notional = a.notional + b.notional;
  r.n_buy = a.n_buy + b.n_buy;
  r.n_sell = a.n_sell + b.n_sell;
  return r;
}

// the bar of a step without a record: the previous step's close carried, every other word zero
BKD_BAR_HD Bar idle(uint32_t prev_close) {
  Bar r;
  r.open = r.high = r.low = r.close = prev_close;
  r.buy_vol = r.sell_vol = r.notional = 0u;
  r.n_buy = r.n_sell = 0u;
  return r;
}

// the row's twelve little-endian 32-bit words, three 16-byte vectors
BKD_BAR_HD void words(const Bar& r, uint32_t w[12]) {
  w[0] = r.open, w[1] = r.high, w[2] = r.low, w[3] = r.close;
  w[4] = static_cast<uint32_t>(r.buy_vol), w[5] = static_cast<uint32_t>(r.buy_vol >> 32);
  w[6] = static_cast<uint32_t>(r.sell_vol), w[7] = static_cast<uint32_t>(r.sell_vol >> 32);
  w[8] = static_cast<uint32_t>(r.notional), w[9] = static_cast<uint32_t>(r.notional >> 32);
  w[10] = r.n_buy, w[11] = r.n_sell;
}

}  // namespace trade_bars
}  // namespace bkd
