// open_order_rows.hpp - the rows of bk_open_orders_enable's tables, one resting order at a time.
//
// Compiled by the device refresh (open_orders.hpp) and by a CPU test (tests/cpp/open_order_rows_test.cpp): no HIP type, no
// intrinsic.  A trader's summary row is {bid_vol, ask_vol, n_bid, n_ask, best_bid, best_ask} (bk_open_summary, 32 B); an
// entry is {order_id, price, vol, side_is_bid} (bk_open_order, 16 B).  The volume sums are modulo 2^64 and cannot wrap: a
// pool holds at most 512 orders of at most 2^32 - 1 each.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BKD_OPEN_HD __host__ __device__ inline
#else
#define BKD_OPEN_HD inline
#endif

namespace bkd {
namespace open_orders {

constexpr uint32_t NO_ORDER = 0xFFFFFFFFu;  // order_id of an unused entry
constexpr uint32_t NO_ASK = 0xFFFFFFFFu;    // best_ask of a trader without a resting ask (best_bid: 0)

struct Summary {
  uint64_t bid_vol, ask_vol;
  uint32_t n_bid, n_ask, best_bid, best_ask;
};

struct Entry {
  uint32_t order_id, price, vol, side_is_bid;
};

// the row of a trader with no resting order
BKD_OPEN_HD Summary empty_summary() {
  Summary s;
  s.bid_vol = 0, s.ask_vol = 0;
  s.n_bid = 0, s.n_ask = 0;
  s.best_bid = 0, s.best_ask = NO_ASK;
  return s;
}

// one more resting order of the row's trader: its side, current price and remaining volume
BKD_OPEN_HD void add_order(Summary& s, uint32_t side_is_bid, uint32_t price, uint32_t vol) {
  if (side_is_bid) {
    s.bid_vol += vol;
    s.n_bid += 1u;
    s.best_bid = price > s.best_bid ? price : s.best_bid;
  } else {
    s.ask_vol += vol;
    s.n_ask += 1u;
    s.best_ask = price < s.best_ask ? price : s.best_ask;
  }
}

// every slot of a trader's list behind the used ones
BKD_OPEN_HD Entry empty_entry() {
  Entry e;
  e.order_id = NO_ORDER, e.price = 0, e.vol = 0, e.side_is_bid = 0;
  return e;
}

BKD_OPEN_HD Entry pack_entry(uint32_t order_id, uint32_t price, uint32_t vol, uint32_t side_is_bid) {
  Entry e;
  e.order_id = order_id, e.price = price, e.vol = vol, e.side_is_bid = side_is_bid ? 1u : 0u;
  return e;
}

// the row's eight little-endian words as they lie in memory
BKD_OPEN_HD void summary_words(const Summary& s, uint32_t (&w)[8]) {
  w[0] = static_cast<uint32_t>(s.bid_vol), w[1] = static_cast<uint32_t>(s.bid_vol >> 32);
  w[2] = static_cast<uint32_t>(s.ask_vol), w[3] = static_cast<uint32_t>(s.ask_vol >> 32);
  w[4] = s.n_bid, w[5] = s.n_ask, w[6] = s.best_bid, w[7] = s.best_ask;
}

// how many entries of a trader's list are used
BKD_OPEN_HD uint32_t entries_used(const Summary& s, uint32_t depth) {
  const uint32_t n = s.n_bid + s.n_ask;
  return n < depth ? n : depth;
}

}  // namespace open_orders
}  // namespace bkd
