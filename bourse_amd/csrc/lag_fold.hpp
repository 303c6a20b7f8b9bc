// lag_fold.hpp - what ONE level-2 record adds to ONE row of a book's lag table, the window word of a record, and where the
// carry and the steps of a fold stand in the window (bk_lags_enable).
//
// Compiled by the device fold (lags.hpp) and by a CPU test (tests/cpp/lag_fold_test.cpp): no HIP type, no intrinsic.
// Of a record only bid_price and ask_price are read; an empty side reads bid_price == 0 / ask_price == 0xFFFFFFFF.  A record
// becomes one WORD {two, m}: bit 63 set and m = bid + ask (twice the mid) in the low bits if it is two-sided, the whole word
// 0 if it is not or if the step lies in front of the table's start.  Row k - 1 of step s, from four words - those of steps
// s, s - 1, s - k and s - k - 1:
//   SPAN k  two_s && two_{s-k}:  h = m_s - m_{s-k}, a = |h|: n_h, sum_h, sum_abs_h, sum_h2 (a * a mod 2^64), sum_h4 (a^4 mod
//           2^128, a 128-bit pair), max_abs_h;
//   LAG k   r_s && r_{s-k}, where r_t = two_t && two_{t-1} and d_t = m_t - m_{t-1}:  n_pairs, sum_dd (d_s * d_{s-k}, two's
//           complement), sum_abs_dd.
// All 64-bit words are sums modulo 2^64; signed words are two's complement.
#pragma once
#include <stdint.h>

#include "series_fold.hpp"  // two_sided, abs_i64, pow4_mod128

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BKD_LAGS_HD __host__ __device__ inline
#else
#define BKD_LAGS_HD inline
#endif

namespace bkd {
namespace lags {

enum Word : uint32_t {  // bk_lag_row, word by word
  N_PAIRS = 0, SUM_DD, SUM_ABS_DD, N_H, SUM_H, SUM_ABS_H, SUM_H2, SUM_H4_LO, SUM_H4_HI, MAX_ABS_H, ROW_WORDS
};
static_assert(ROW_WORDS == 10, "bk_lag_row is 10 words");

constexpr uint32_t MAX_LAGS = 64u;  // K, rows per book
constexpr uint32_t CHUNK = 64u;     // steps the window takes in at a time
constexpr uint64_t TWO = 1ull << 63, M_BITS = TWO - 1ull;

struct Row {
  uint64_t w[ROW_WORDS];
};

// the window word of a record
BKD_LAGS_HD uint64_t word_of(uint32_t bid, uint32_t ask) {
  return series::two_sided(bid, ask) ? TWO | (static_cast<uint64_t>(bid) + ask) : 0ull;
}

// The window of a fold at K lags: K + 1 carry words in front - carry entry j (the record of step lags_seen - 1 - j) at
// carry_at(K, j), so the window reads forward in time - then up to CHUNK steps; step i of the chunk at step_at(K, i).
// Lag k of that step reads the words at step_at(K, i) - k and one in front of it: never below 0.
constexpr uint32_t WINDOW_WORDS = MAX_LAGS + 1u + CHUNK;
BKD_LAGS_HD uint32_t carry_at(uint32_t K, uint32_t j) { return K - j; }
BKD_LAGS_HD uint32_t step_at(uint32_t K, uint32_t i) { return K + 1u + i; }

// r += the two terms of step s at one lag k: cur, prev = the words of steps s, s - 1; at_k, before_k = those of s - k, s - k - 1
BKD_LAGS_HD void add(Row& r, uint64_t cur, uint64_t prev, uint64_t at_k, uint64_t before_k) {
  if (!(cur & TWO)) return;
  const uint64_t m = cur & M_BITS;
  if (at_k & TWO) {  // the span: only its two end points must be two-sided
    const int64_t h = static_cast<int64_t>(m - (at_k & M_BITS));
    const uint64_t a = series::abs_i64(h);
    uint64_t lo, hi;
    series::pow4_mod128(a, lo, hi);
    r.w[N_H] += 1u;
    r.w[SUM_H] += static_cast<uint64_t>(h);
    r.w[SUM_ABS_H] += a;
    r.w[SUM_H2] += a * a;
    r.w[SUM_H4_LO] += lo;
    r.w[SUM_H4_HI] += hi + (r.w[SUM_H4_LO] < lo ? 1u : 0u);
    r.w[MAX_ABS_H] = series::umax64(r.w[MAX_ABS_H], a);
    if ((prev & TWO) && (before_k & TWO)) {  // the lag: a return at both ends
      const int64_t d = static_cast<int64_t>(m - (prev & M_BITS));
      const int64_t dk = static_cast<int64_t>((at_k & M_BITS) - (before_k & M_BITS));
      r.w[N_PAIRS] += 1u;
      r.w[SUM_DD] += static_cast<uint64_t>(d) * static_cast<uint64_t>(dk);
      r.w[SUM_ABS_DD] += series::abs_i64(d) * series::abs_i64(dk);
    }
  }
}

// r = the row of r's steps followed by part's
BKD_LAGS_HD void merge(Row& r, const Row& part) {
  r.w[N_PAIRS] += part.w[N_PAIRS], r.w[SUM_DD] += part.w[SUM_DD], r.w[SUM_ABS_DD] += part.w[SUM_ABS_DD];
  r.w[N_H] += part.w[N_H], r.w[SUM_H] += part.w[SUM_H], r.w[SUM_ABS_H] += part.w[SUM_ABS_H], r.w[SUM_H2] += part.w[SUM_H2];
  r.w[SUM_H4_LO] += part.w[SUM_H4_LO];
  r.w[SUM_H4_HI] += part.w[SUM_H4_HI] + (r.w[SUM_H4_LO] < part.w[SUM_H4_LO] ? 1u : 0u);  // (after the low word's sum)
  r.w[MAX_ABS_H] = series::umax64(r.w[MAX_ABS_H], part.w[MAX_ABS_H]);
}

}  // namespace lags
}  // namespace bkd
