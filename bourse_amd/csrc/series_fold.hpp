// series_fold.hpp - what ONE level-2 record adds to a book's row of series moments, given the two values in front of it, how
// those two values move on, and the row's 24 words (bk_series_enable).
//
// Compiled by the device fold (series.hpp) and by a CPU test (tests/cpp/series_fold_test.cpp): no HIP type, no intrinsic.
// A record is the first five words of a level-2 record, {trade_vol, bid_price, ask_price, ask_vol, bid_vol}; an empty side
// reads bid_price == 0 / ask_price == 0xFFFFFFFF.  With m = bid + ask (twice the mid) of a two-sided record:
//   a RETURN d = m - m_prev exists between two CONSECUTIVE two-sided records, a PAIR d * d_prev over three;
//   the values in front of a record are Prev {have_m, m, have_d, d}: m of the record before it if that one was two-sided,
//   d of that record if it had a return.  A word whose have_ bit is clear is 0, so Prev is a function of the two records in
//   front (and of one bit of the third) - which is what lets every lane of the device fold build its own.
// All 64-bit words are sums modulo 2^64, sum_d4 a sum modulo 2^128 of a^4 modulo 2^128; signed words are two's complement.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BKD_SERIES_HD __host__ __device__ inline
#else
#define BKD_SERIES_HD inline
#endif

namespace bkd {
namespace series {

enum Word : uint32_t {  // bk_series_row, word by word
  N_STEPS = 0, N_TWO_SIDED, SUM_M, SUM_SPREAD, SUM_SPREAD_SQ, SUM_BID_VOL, SUM_ASK_VOL, SUM_TRADE_VOL, SUM_TRADE_VOL_SQ,
  N_TRADE_STEPS, N_RET, SUM_D, SUM_ABS_D, SUM_D2, SUM_D4_LO, SUM_D4_HI, MAX_ABS_D, N_PAIRS, SUM_DD, SUM_ABS_DD, MIN_M, MAX_M,
  CARRY_M, CARRY_D, ROW_WORDS
};
static_assert(ROW_WORDS == 24, "bk_series_row is 24 words");

constexpr uint32_t NO_ASK = 0xFFFFFFFFu;
constexpr uint64_t HAVE_M = 1ull << 63, HAVE_D = 1ull << 62, M_BITS = HAVE_D - 1ull;

struct Row {
  uint64_t w[ROW_WORDS];
};

// the values in front of a record
struct Prev {
  uint32_t have_m, have_d;
  uint64_t m;
  int64_t d;
};

// what one record contributes
struct Term {
  uint64_t tv, tv_sq, bid_vol, ask_vol;
  uint32_t traded, two, ret, pair;
  uint64_t m, spread, spread_sq;  // two
  int64_t d;                      // ret
  uint64_t a, d2, d4_lo, d4_hi;   // ret: |d|, a^2 mod 2^64, a^4 mod 2^128
  uint64_t dd, abs_dd;            // pair: d * d_prev (two's complement), a * |d_prev|
};

BKD_SERIES_HD bool two_sided(uint32_t bid, uint32_t ask) { return bid != 0u && ask != NO_ASK; }

// the full 64 x 64 -> 128-bit product from 32-bit limbs
BKD_SERIES_HD void mul_64x64(uint64_t x, uint64_t y, uint64_t& lo, uint64_t& hi) {
  const uint64_t x0 = x & 0xFFFFFFFFull, x1 = x >> 32, y0 = y & 0xFFFFFFFFull, y1 = y >> 32;
  const uint64_t p00 = x0 * y0, p01 = x0 * y1, p10 = x1 * y0, p11 = x1 * y1;
  const uint64_t mid = (p00 >> 32) + (p01 & 0xFFFFFFFFull) + (p10 & 0xFFFFFFFFull);
  lo = (p00 & 0xFFFFFFFFull) | (mid << 32);
  hi = p11 + (p01 >> 32) + (p10 >> 32) + (mid >> 32);
}

// a^4 modulo 2^128: a * a may need more than 64 bits (a < 2^33), so it is squared as a 128-bit word
BKD_SERIES_HD void pow4_mod128(uint64_t a, uint64_t& lo, uint64_t& hi) {
  uint64_t l, h;
  mul_64x64(a, a, l, h);
  mul_64x64(l, l, lo, hi);
  hi += 2ull * l * h;  // (2 * l * h * 2^64; h * h * 2^128 vanishes)
}

BKD_SERIES_HD uint64_t abs_i64(int64_t d) { return d < 0 ? 0ull - static_cast<uint64_t>(d) : static_cast<uint64_t>(d); }

BKD_SERIES_HD Term term(uint32_t tv, uint32_t bid, uint32_t ask, uint32_t ask_vol, uint32_t bid_vol, const Prev& p) {
  Term t{};
  t.tv = tv;
  t.tv_sq = static_cast<uint64_t>(tv) * tv;
  t.bid_vol = bid_vol;
  t.ask_vol = ask_vol;
  t.traded = tv > 0u ? 1u : 0u;
  t.two = two_sided(bid, ask) ? 1u : 0u;
  if (t.two) {
    t.m = static_cast<uint64_t>(bid) + ask;
    t.spread = static_cast<uint32_t>(ask - bid);
    t.spread_sq = t.spread * t.spread;
  }
  t.ret = t.two && p.have_m ? 1u : 0u;
  if (t.ret) {
    t.d = static_cast<int64_t>(t.m - p.m);
    t.a = abs_i64(t.d);
    t.d2 = t.a * t.a;
    pow4_mod128(t.a, t.d4_lo, t.d4_hi);
  }
  t.pair = t.ret && p.have_d ? 1u : 0u;
  if (t.pair) {
    t.dd = static_cast<uint64_t>(t.d) * static_cast<uint64_t>(p.d);
    t.abs_dd = t.a * abs_i64(p.d);
  }
  return t;
}

// the carry update: the values in front of the NEXT record
BKD_SERIES_HD Prev next(const Term& t) {
  Prev p;
  p.have_m = t.two;
  p.m = t.two ? t.m : 0ull;
  p.have_d = t.ret;
  p.d = t.ret ? t.d : 0;
  return p;
}

// the values in front of a record from the quotes of the record before it and what was in front of THAT one (of which
// only have_m and m are read)
BKD_SERIES_HD Prev prev_of(uint32_t bid1, uint32_t ask1, const Prev& before1) { return next(term(0u, bid1, ask1, 0u, 0u, before1)); }

// have_m and m of one record alone (what prev_of reads of its last argument)
BKD_SERIES_HD Prev quotes_only(uint32_t bid, uint32_t ask) {
  Prev p;
  p.have_m = two_sided(bid, ask) ? 1u : 0u;
  p.m = p.have_m ? static_cast<uint64_t>(bid) + ask : 0ull;
  p.have_d = 0u;
  p.d = 0;
  return p;
}

// a row without a record
BKD_SERIES_HD Row cleared() {
  Row r{};
  r.w[MIN_M] = ~0ull;
  return r;
}

BKD_SERIES_HD uint64_t umin64(uint64_t x, uint64_t y) { return x < y ? x : y; }
BKD_SERIES_HD uint64_t umax64(uint64_t x, uint64_t y) { return x > y ? x : y; }

// r += t: the sums and the extremes (the carry words are not touched: pack() writes them once)
BKD_SERIES_HD void add(Row& r, const Term& t) {
  r.w[N_STEPS] += 1u;
  r.w[SUM_TRADE_VOL] += t.tv;
  r.w[SUM_TRADE_VOL_SQ] += t.tv_sq;
  r.w[N_TRADE_STEPS] += t.traded;
  r.w[SUM_BID_VOL] += t.bid_vol;
  r.w[SUM_ASK_VOL] += t.ask_vol;
  if (t.two) {
    r.w[N_TWO_SIDED] += 1u;
    r.w[SUM_M] += t.m;
    r.w[SUM_SPREAD] += t.spread;
    r.w[SUM_SPREAD_SQ] += t.spread_sq;
    r.w[MIN_M] = umin64(r.w[MIN_M], t.m);
    r.w[MAX_M] = umax64(r.w[MAX_M], t.m);
  }
  if (t.ret) {
    r.w[N_RET] += 1u;
    r.w[SUM_D] += static_cast<uint64_t>(t.d);
    r.w[SUM_ABS_D] += t.a;
    r.w[SUM_D2] += t.d2;
    r.w[SUM_D4_LO] += t.d4_lo;
    r.w[SUM_D4_HI] += t.d4_hi + (r.w[SUM_D4_LO] < t.d4_lo ? 1u : 0u);
    r.w[MAX_ABS_D] = umax64(r.w[MAX_ABS_D], t.a);
  }
  if (t.pair) {
    r.w[N_PAIRS] += 1u;
    r.w[SUM_DD] += t.dd;
    r.w[SUM_ABS_DD] += t.abs_dd;
  }
}

// r = the row of r's records followed by part's: sums added, extremes combined; the carry words stay r's
BKD_SERIES_HD void merge(Row& r, const Row& part) {
  r.w[N_STEPS] += part.w[N_STEPS], r.w[N_TWO_SIDED] += part.w[N_TWO_SIDED], r.w[SUM_M] += part.w[SUM_M];
  r.w[SUM_SPREAD] += part.w[SUM_SPREAD], r.w[SUM_SPREAD_SQ] += part.w[SUM_SPREAD_SQ];
  r.w[SUM_BID_VOL] += part.w[SUM_BID_VOL], r.w[SUM_ASK_VOL] += part.w[SUM_ASK_VOL];
  r.w[SUM_TRADE_VOL] += part.w[SUM_TRADE_VOL], r.w[SUM_TRADE_VOL_SQ] += part.w[SUM_TRADE_VOL_SQ];
  r.w[N_TRADE_STEPS] += part.w[N_TRADE_STEPS], r.w[N_RET] += part.w[N_RET], r.w[SUM_D] += part.w[SUM_D];
  r.w[SUM_ABS_D] += part.w[SUM_ABS_D], r.w[SUM_D2] += part.w[SUM_D2], r.w[SUM_D4_LO] += part.w[SUM_D4_LO];
  r.w[N_PAIRS] += part.w[N_PAIRS], r.w[SUM_DD] += part.w[SUM_DD], r.w[SUM_ABS_DD] += part.w[SUM_ABS_DD];
  r.w[SUM_D4_HI] += part.w[SUM_D4_HI] + (r.w[SUM_D4_LO] < part.w[SUM_D4_LO] ? 1u : 0u);  // (after the low word's sum)
  r.w[MAX_ABS_D] = umax64(r.w[MAX_ABS_D], part.w[MAX_ABS_D]);
  r.w[MIN_M] = umin64(r.w[MIN_M], part.w[MIN_M]);
  r.w[MAX_M] = umax64(r.w[MAX_M], part.w[MAX_M]);
}

// the row's two carry words from the values in front of the next record, and back
BKD_SERIES_HD void pack(Row& r, const Prev& p) {
  r.w[CARRY_M] = (p.have_m ? HAVE_M | (p.m & M_BITS) : 0ull) | (p.have_d ? HAVE_D : 0ull);
  r.w[CARRY_D] = p.have_d ? static_cast<uint64_t>(p.d) : 0ull;
}
BKD_SERIES_HD Prev unpack(uint64_t carry_m, uint64_t carry_d) {
  Prev p;
  p.have_m = carry_m & HAVE_M ? 1u : 0u;
  p.have_d = carry_m & HAVE_D ? 1u : 0u;
  p.m = p.have_m ? carry_m & M_BITS : 0ull;
  p.d = p.have_d ? static_cast<int64_t>(carry_d) : 0;
  return p;
}

}  // namespace series
}  // namespace bkd
