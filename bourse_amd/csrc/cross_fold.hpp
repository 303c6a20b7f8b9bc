// cross_fold.hpp - what ONE step adds to ONE row of a market's cross table, where the carry and the steps of a fold stand in
// an asset's window, and which row a unit of the fold owns (bk_cross_enable).
//
// Compiled by the device fold (cross.hpp) and by a CPU test (tests/cpp/cross_fold_test.cpp): no HIP type, no intrinsic.
// The window word of a record is the lag table's (lags::word_of, lag_fold.hpp): bit 63 set and m = bid + ask (twice the mid)
// in the low bits if the record is two-sided, the whole word 0 if it is not or if the step lies in front of the table's
// start, a clear or a reset.  Row (j, a, b) - the ORDERED pair asset a against asset b at span h = spans[j] - of step s, from
// five words - a's of steps s and s - h, b's of steps s, s - h and s - 2h:
//   CONTEMPORANEOUS  two_a(s) && two_a(s-h) && two_b(s) && two_b(s-h):  x = m_a(s) - m_a(s-h), y = m_b(s) - m_b(s-h):
//                    n, sum_x, sum_y, sum_xx, sum_yy, sum_xy;
//   LEAD             two_a(s) && two_a(s-h) && two_b(s-h) && two_b(s-2h) (b's word of step s is NOT asked for):
//                    z = m_b(s-h) - m_b(s-2h): n_lead, sum_lead (x * z).
// All words are sums modulo 2^64; signed words are two's complement, products are 64-bit products of them.
#pragma once
#include <stdint.h>

#include "lag_fold.hpp"  // lags::word_of, TWO, M_BITS (and series_fold.hpp through it)

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BKD_CROSS_HD __host__ __device__ inline
#else
#define BKD_CROSS_HD inline
#endif

namespace bkd {
namespace cross {

enum Word : uint32_t {  // bk_cross_row, word by word
  N = 0, SUM_X, SUM_Y, SUM_XX, SUM_YY, SUM_XY, N_LEAD, SUM_LEAD, ROW_WORDS
};
static_assert(ROW_WORDS == 8, "bk_cross_row is 8 words");

constexpr uint32_t MAX_SPANS = 4u, MAX_SPAN = 64u;  // S spans of 1 .. 64 steps each
constexpr uint32_t MAX_ASSETS = 8u;                 // A, books per market
constexpr uint32_t MAX_UNITS = MAX_SPANS * MAX_ASSETS * MAX_ASSETS;  // U = S * A * A <= 256: four rounds of 64 lanes
constexpr uint32_t CHUNK = 64u;                     // steps the windows take in at a time

using lags::M_BITS;
using lags::TWO;
using lags::word_of;

struct Row {
  uint64_t w[ROW_WORDS];
};

// The window of ONE asset at a longest span Hmax: 2 * Hmax carry words in front - carry entry j (the record of step
// seen - 2 * Hmax + j: the carry reads forward in time, as the window does) at carry_at(j) = j - then up to CHUNK steps;
// step i of the chunk at step_at(Hmax, i).  Span h <= Hmax of that step reads the words h and 2 * h in front of it: never
// below 0.  A market's windows stand one behind the other, asset a's at window_at(Hmax, a).
BKD_CROSS_HD uint32_t carry_words(uint32_t Hmax) { return 2u * Hmax; }
BKD_CROSS_HD uint32_t window_words(uint32_t Hmax) { return 2u * Hmax + CHUNK; }
BKD_CROSS_HD uint32_t window_at(uint32_t Hmax, uint32_t a) { return a * window_words(Hmax); }
BKD_CROSS_HD uint32_t carry_at(uint32_t j) { return j; }
BKD_CROSS_HD uint32_t step_at(uint32_t Hmax, uint32_t i) { return 2u * Hmax + i; }
// between two chunks (and behind the last) the window's last 2 * Hmax words become its front: word front_from(cnt, j) -> j
BKD_CROSS_HD uint32_t front_from(uint32_t cnt, uint32_t j) { return cnt + j; }

// unit u = j * A * A + a * A + b  <->  row (j, a, b)
struct Unit {
  uint32_t j, a, b;
};
BKD_CROSS_HD uint32_t units(uint32_t S, uint32_t A) { return S * A * A; }
BKD_CROSS_HD uint32_t unit_of(uint32_t A, uint32_t j, uint32_t a, uint32_t b) { return (j * A + a) * A + b; }
BKD_CROSS_HD Unit unit_at(uint32_t A, uint32_t u) {
  const uint32_t ja = u / A;
  return {ja / A, ja % A, u % A};
}

// r += the two terms of step s of one unit: a_s, a_h = asset a's words of steps s, s - h; b_s, b_h, b_2h = asset b's of
// steps s, s - h, s - 2h
BKD_CROSS_HD void add(Row& r, uint64_t a_s, uint64_t a_h, uint64_t b_s, uint64_t b_h, uint64_t b_2h) {
  if (!(a_s & a_h & b_h & TWO)) return;  // both terms need a's return and b's word of step s - h
  const uint64_t x = (a_s & M_BITS) - (a_h & M_BITS);
  if (b_s & TWO) {
    const uint64_t y = (b_s & M_BITS) - (b_h & M_BITS);
    r.w[N] += 1u;
    r.w[SUM_X] += x;
    r.w[SUM_Y] += y;
    r.w[SUM_XX] += x * x;
    r.w[SUM_YY] += y * y;
    r.w[SUM_XY] += x * y;
  }
  if (b_2h & TWO) {
    const uint64_t z = (b_h & M_BITS) - (b_2h & M_BITS);
    r.w[N_LEAD] += 1u;
    r.w[SUM_LEAD] += x * z;
  }
}

// r = the row of r's steps followed by part's
BKD_CROSS_HD void merge(Row& r, const Row& part) {
  for (uint32_t i = 0; i < ROW_WORDS; ++i) r.w[i] += part.w[i];
}

}  // namespace cross
}  // namespace bkd
