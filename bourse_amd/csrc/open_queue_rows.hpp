// open_queue_rows.hpp - the rows of bk_open_queue_enable's table, one resting order at a time.
//
// Compiled by the device refresh (open_queue.hpp) and by a CPU test (tests/cpp/open_queue_rows_test.cpp): no HIP type, no
// intrinsic.  The row of a listed order o is {ahead_vol, level_ahead_vol, level_vol, ahead_orders, level_ahead_orders}
// (bk_open_queue, 32 B): what rests on o's side with priority over it, the part of that at o's own price, and everything at
// that price, o included.  Priority is the matching engine's: the better price, then the smaller pool stamp (seq).  The
// volume sums are modulo 2^64 and cannot wrap: a pool holds at most 512 orders of at most 2^32 - 1 each.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BKD_QUEUE_HD __host__ __device__ inline
#else
#define BKD_QUEUE_HD inline
#endif

namespace bkd {
namespace open_queue {

constexpr uint32_t AHEAD = 1u;  // place(): r trades before o
constexpr uint32_t LEVEL = 2u;  // place(): r rests at o's price, on o's side (o itself does)

struct Row {
  uint64_t ahead_vol, level_ahead_vol, level_vol;
  uint32_t ahead_orders, level_ahead_orders;
};

// the row of an unused entry, and of an entry whose order is not live in the pool
BKD_QUEUE_HD Row empty_row() {
  Row w;
  w.ahead_vol = 0, w.level_ahead_vol = 0, w.level_vol = 0;
  w.ahead_orders = 0, w.level_ahead_orders = 0;
  return w;
}

// where the live order r stands relative to the listed order o: AHEAD when r is on o's side at a better price (higher for
// a bid, lower for an ask) or at o's price with an earlier stamp, LEVEL when it is on o's side at o's price.  o itself is
// LEVEL and not AHEAD (its stamp is not earlier than itself).
BKD_QUEUE_HD uint32_t place(uint32_t o_is_bid, uint32_t o_price, uint32_t o_seq, uint32_t r_is_bid, uint32_t r_price,
                            uint32_t r_seq) {
  if ((o_is_bid != 0u) != (r_is_bid != 0u)) return 0u;
  const bool level = r_price == o_price;
  const bool better = o_is_bid ? r_price > o_price : r_price < o_price;
  const bool ahead = better || (level && r_seq < o_seq);
  return (ahead ? AHEAD : 0u) | (level ? LEVEL : 0u);
}

// one more live order of the pool, with its place() and remaining volume
BKD_QUEUE_HD void add_order(Row& w, uint32_t where, uint32_t vol) {
  const bool ahead = (where & AHEAD) != 0u, level = (where & LEVEL) != 0u;
  w.ahead_vol += ahead ? vol : 0u;
  w.ahead_orders += ahead ? 1u : 0u;
  w.level_ahead_vol += ahead && level ? vol : 0u;
  w.level_ahead_orders += ahead && level ? 1u : 0u;
  w.level_vol += level ? vol : 0u;
}

// the row's eight little-endian words as they lie in memory
BKD_QUEUE_HD void row_words(const Row& w, uint32_t (&v)[8]) {
  v[0] = static_cast<uint32_t>(w.ahead_vol), v[1] = static_cast<uint32_t>(w.ahead_vol >> 32);
  v[2] = static_cast<uint32_t>(w.level_ahead_vol), v[3] = static_cast<uint32_t>(w.level_ahead_vol >> 32);
  v[4] = static_cast<uint32_t>(w.level_vol), v[5] = static_cast<uint32_t>(w.level_vol >> 32);
  v[6] = w.ahead_orders, v[7] = w.level_ahead_orders;
}

}  // namespace open_queue
}  // namespace bkd
