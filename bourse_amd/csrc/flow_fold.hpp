// flow_fold.hpp - the plain rules of a book's flow table (bk_flow_enable): the window word of a trade record,
// what one record adds to the base words and one pair of records to a lag row, which indices of a fold can be read, how a
// run of unreadable indices moves the carry, and the carry a fold leaves.
//
// Compiled by the device fold (flow.hpp) and by a CPU test (tests/cpp/flow_fold_test.cpp): no HIP type, no intrinsic.
// A record is {price, vol, side_is_bid}; side_is_bid is the PASSIVE order's side as trade_bar_fold.hpp reads it, so the
// aggressor bought iff side_is_bid == 0: s = +1, otherwise s = -1.  Records are numbered per book as the header counts them
// (H_TRADES the next index, H_TRADE_BASE the first retained one).  A record becomes one WORD: bit 63 valid, bit 62 buy, the
// price in the low 32 bits; the whole word is 0 for an index that could not be read or lies in front of the table's start.
// A pair (i, i - k), 1 <= k <= K, counts iff both words are valid - whatever lies between them - with dp = p_i - p_{i-k}:
//   n_pairs += 1, sum_ss += s_i s_{i-k}, sum_resp += s_{i-k} dp, sum_back += s_i dp, sum_abs_dp += |dp|, sum_dp2 += dp^2.
// All words are sums modulo 2^64 (max_vol a maximum); signed words are two's complement.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BKD_FLOW_HD __host__ __device__ inline
#else
#define BKD_FLOW_HD inline
#endif

namespace bkd {
namespace flow {

enum BaseWord : uint32_t { N_TRADES = 0, N_BUY, SUM_VOL, BUY_VOL, SUM_VOL_SQ, NOTIONAL, MAX_VOL, N_LOST, BASE_WORDS };
enum LagWord : uint32_t { N_PAIRS = 0, SUM_SS, SUM_RESP, SUM_BACK, SUM_ABS_DP, SUM_DP2, LAG_WORDS };
static_assert(BASE_WORDS == 8 && LAG_WORDS == 6, "a book's table is uint64_t[8 + 6 K]");

constexpr uint32_t MAX_LAGS = 64u;  // K, lag rows per book
constexpr uint32_t CHUNK = 64u;     // records the window takes in at a time
constexpr uint64_t VALID = 1ull << 63, BUY = 1ull << 62, PRICE_BITS = 0xFFFFFFFFull;

struct Base {
  uint64_t w[BASE_WORDS];
};
struct LagRow {
  uint64_t w[LAG_WORDS];
};

BKD_FLOW_HD uint32_t table_words(uint32_t K) { return BASE_WORDS + LAG_WORDS * K; }

// the window word of a record that was read
BKD_FLOW_HD uint64_t word_of(uint32_t price, uint32_t side_is_bid) { return VALID | (side_is_bid == 0u ? BUY : 0ull) | price; }

// r += one record that was read
BKD_FLOW_HD void add_record(Base& r, uint32_t price, uint32_t vol, uint32_t side_is_bid) {
  const bool buy = side_is_bid == 0u;
  r.w[N_TRADES] += 1u;
  r.w[N_BUY] += buy ? 1u : 0u;
  r.w[SUM_VOL] += vol;
  r.w[BUY_VOL] += buy ? vol : 0u;
  r.w[SUM_VOL_SQ] += static_cast<uint64_t>(vol) * vol;
  r.w[NOTIONAL] += static_cast<uint64_t>(vol) * price;
  r.w[MAX_VOL] = r.w[MAX_VOL] > vol ? r.w[MAX_VOL] : vol;
}

// r = the base words of r's records followed by part's
BKD_FLOW_HD void merge(Base& r, const Base& part) {
  for (uint32_t i = 0; i < BASE_WORDS; ++i)
    if (i != MAX_VOL) r.w[i] += part.w[i];
  r.w[MAX_VOL] = r.w[MAX_VOL] > part.w[MAX_VOL] ? r.w[MAX_VOL] : part.w[MAX_VOL];
}

// r += the pair of the record with word `cur` and the one k records in front of it with word `at_k`
BKD_FLOW_HD void add_pair(LagRow& r, uint64_t cur, uint64_t at_k) {
  if (!(cur & at_k & VALID)) return;
  const uint64_t dp = (cur & PRICE_BITS) - (at_k & PRICE_BITS);  // two's complement, |dp| < 2^32
  const uint64_t neg = 0ull - dp;
  const uint64_t a = static_cast<int64_t>(dp) < 0 ? neg : dp;
  r.w[N_PAIRS] += 1u;
  r.w[SUM_SS] += ((cur ^ at_k) & BUY) ? ~0ull : 1ull;
  r.w[SUM_RESP] += (at_k & BUY) ? dp : neg;
  r.w[SUM_BACK] += (cur & BUY) ? dp : neg;
  r.w[SUM_ABS_DP] += a;
  r.w[SUM_DP2] += a * a;
}

BKD_FLOW_HD void merge(LagRow& r, const LagRow& part) {
  for (uint32_t i = 0; i < LAG_WORDS; ++i) r.w[i] += part.w[i];
}

// The indices a fold covers are [seen, total).  Index i can be read iff base <= i < total and i - base < capacity (base,
// total as the fold read them from the header): the readable ones are the run [lo, hi), in front of it lo - seen lost
// indices - consumed before the table saw them - and behind it total - hi - dropped beyond the capacity.
struct Plan {
  uint64_t lo, hi;               // seen <= lo <= hi <= total
  uint64_t lost_front, lost_back;
};
BKD_FLOW_HD Plan plan(uint64_t seen, uint64_t total, uint64_t base, uint64_t capacity) {
  if (seen > total) seen = total;  // (a cursor ahead of the book: nothing rewinds a book without a clear, so never)
  Plan p;
  p.lo = base > seen ? base : seen;
  if (p.lo > total) p.lo = total;
  const uint64_t since_base = total > base ? total - base : 0ull;
  const uint64_t end = capacity < since_base ? base + capacity : total;  // min(total, base + capacity)
  p.hi = end > p.lo ? end : p.lo;
  p.lost_front = p.lo - seen;
  p.lost_back = total - p.hi;
  return p;
}

// The carry: entry j is the word of index seen - 1 - j, j < K.  After `gap` unreadable indices entry j is invalid for
// j < gap and the old entry j - gap behind them - a gap of K or more invalidates all of it and is never walked.
// carry_src: the old entry that entry j holds after the gap, or NO_ENTRY: invalid.
constexpr uint32_t NO_ENTRY = 0xFFFFFFFFu;
BKD_FLOW_HD uint32_t carry_src(uint32_t K, uint64_t gap, uint32_t j) {
  return gap >= K || j < gap ? NO_ENTRY : j - static_cast<uint32_t>(gap);
}

// The window of a fold at K lags: K carry words in front - carry entry j at carry_at(K, j), so the window reads forward in
// time - then up to CHUNK records; record i of the chunk at rec_at(K, i).  Lag k of it reads rec_at(K, i) - k: never below 0.
constexpr uint32_t WINDOW_WORDS = MAX_LAGS + CHUNK;
BKD_FLOW_HD uint32_t carry_at(uint32_t K, uint32_t j) { return K - 1u - j; }
BKD_FLOW_HD uint32_t rec_at(uint32_t K, uint32_t i) { return K + i; }

}  // namespace flow
}  // namespace bkd
