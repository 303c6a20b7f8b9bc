// bin_fold.hpp - which bin ONE level-2 record raises in each channel of a book's bin table, where the record a span reaches
// back to stands, and how the carry moves on (bk_bins_enable).
//
// Compiled by the device fold (bins.hpp) and by a CPU test (tests/cpp/bin_fold_test.cpp): no HIP type, no intrinsic.
// Of a record only trade_vol, bid_price and ask_price are read (words 0 .. 2); an empty side reads bid_price == 0 /
// ask_price == 0xFFFFFFFF.  A record's WORD {two, m} is the lag table's (lag_fold.hpp): bit 63 set and m = bid + ask (twice
// the mid) in the low bits if it is two-sided, the whole word 0 if it is not or if the step lies in front of the table's
// start.  With B bins, S spans k_0 .. k_{S-1} and C = S + 2 channels, step s raises one count in
//   channel j < S  if two_s && two_{s-k_j}:  bin clamp(floor((m_s - m_{s-k_j}) / ret_width) + B / 2, 0, B - 1);
//   channel S      if two_s:                 bin min((ask - bid) / spread_width, B - 1), the difference a wrapping u32;
//   channel S + 1  always:                   bin min(trade_vol / vol_width, B - 1).
// The carry holds Kmax = max k_j words: entry i is the word of step bins_seen - 1 - i.
#pragma once
#include <stdint.h>

#include "hist_cursor.hpp"  // ring::slot_of
#include "lag_fold.hpp"     // lags::word_of, lags::TWO, lags::M_BITS (and series::two_sided behind them)

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BKD_BINS_HD __host__ __device__ inline
#else
#define BKD_BINS_HD inline
#endif

namespace bkd {
namespace bins {

constexpr uint32_t MAX_BINS = 256u, MAX_SPANS = 4u, MAX_SPAN = 64u;
constexpr uint32_t MAX_CHANNELS = MAX_SPANS + 2u;
using lags::M_BITS;
using lags::TWO;
using lags::word_of;
using ring::slot_of;  // the ring slot of step i of a fold whose first step stands at slot0

// floor(h / w) for w >= 1: below zero it is -ceil(|h| / w)
BKD_BINS_HD int64_t floor_div(int64_t h, uint32_t w) {
  if (h >= 0) return static_cast<int64_t>(static_cast<uint64_t>(h) / w);
  const uint64_t a = 0ull - static_cast<uint64_t>(h);
  return -static_cast<int64_t>((a + (w - 1u)) / w);
}

// the return's bin: cur and at_k are the words of steps s and s - k, both two-sided
BKD_BINS_HD uint32_t ret_bin(uint64_t cur, uint64_t at_k, uint32_t width, uint32_t B) {
  const int64_t h = static_cast<int64_t>((cur & M_BITS) - (at_k & M_BITS));
  const int64_t q = floor_div(h, width) + static_cast<int64_t>(B / 2u);
  return q < 0 ? 0u : q > static_cast<int64_t>(B - 1u) ? B - 1u : static_cast<uint32_t>(q);
}

BKD_BINS_HD uint32_t top_bin(uint32_t x, uint32_t width, uint32_t B) {
  const uint32_t q = x / width;
  return q < B - 1u ? q : B - 1u;
}
BKD_BINS_HD uint32_t spread_bin(uint32_t bid, uint32_t ask, uint32_t width, uint32_t B) { return top_bin(ask - bid, width, B); }
BKD_BINS_HD uint32_t vol_bin(uint32_t trade_vol, uint32_t width, uint32_t B) { return top_bin(trade_vol, width, B); }

// Where the record of step lo + i - k stands for step i of a fold that starts at lo = bins_seen: in the ring as step
// i - k of the fold while i >= k - the fold's own range, which the lost-step check guarantees is retained - else in the
// carry, entry k - 1 - i
struct Where {
  bool in_ring;
  uint32_t at;  // the fold's step index, or the carry's entry
};
BKD_BINS_HD Where partner(uint32_t i, uint32_t k) { return i >= k ? Where{true, i - k} : Where{false, k - 1u - i}; }

// ... and where entry i of the carry BEHIND a fold of n steps comes from: the record of step lo + n - 1 - i
BKD_BINS_HD Where next_carry(uint32_t n, uint32_t i) { return i < n ? Where{true, n - 1u - i} : Where{false, i - n}; }

}  // namespace bins
}  // namespace bkd
