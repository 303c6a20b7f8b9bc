// depth_fold.hpp - what ONE level of ONE level-2 record adds to its row of a book's depth table, what the record adds to
// the table's header, and which lane of the device fold reads which (step, level) (bk_depth_enable).
//
// Compiled by the device fold (depth.hpp) and by a CPU test (tests/cpp/depth_fold_test.cpp): no HIP type, no intrinsic.
// A record is {trade_vol, bid_price, ask_price, ask_vol, bid_vol} and then L levels of {bid_vol, bid_n, ask_vol, ask_n};
// an empty side reads bid_price == 0 / ask_price == 0xFFFFFFFF.  A record's WORD {two, m} is the lag table's
// (lag_fold.hpp).  With I_q = sum_{i <= q} bid_vol_i - sum_{i <= q} ask_vol_i of a record (|I_q| < 2^38), level q of step s
// adds to row q
//   always:            bid_vol, ask_vol, their squares, bid_n, ask_n, and one count per occupied side;
//   if two_s:          I_q, I_q^2 (modulo 2^64) and |I_q|;
//   if two_s, two_s-1: the PAIR's terms from J = I_q(s - 1) and d = m_s - m_{s-1}.
// The header counts the steps, the sides and the pairs' moves.  The carry is I_q of the last folded step per level and,
// behind them, that step's word: a cleared carry (all zeros) is a step that is not two-sided, so it forms no pair.
// All 64-bit words are sums modulo 2^64; signed words are two's complement.
#pragma once
#include <stdint.h>

#include "lag_fold.hpp"  // lags::word_of, lags::TWO, lags::M_BITS (and series::two_sided, abs_i64, NO_ASK behind them)

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BKD_DEPTH_HD __host__ __device__ inline
#else
#define BKD_DEPTH_HD inline
#endif

namespace bkd {
namespace depth {

enum Word : uint32_t {  // a level's row, word by word
  SUM_BID_VOL = 0, SUM_ASK_VOL, SUM_BID_VOL_SQ, SUM_ASK_VOL_SQ, SUM_BID_ORDERS, SUM_ASK_ORDERS, N_BID_STEPS, N_ASK_STEPS,
  SUM_IMB, SUM_IMB_SQ, N_SIGNED, SUM_SIGN_D, N_AGREE, SUM_IMB_D, N_MOVE, SUM_ABS_IMB, ROW_WORDS
};
enum HeaderWord : uint32_t {  // row L
  N_STEPS = 0, N_TWO_SIDED, N_PAIRS, SUM_D, SUM_ABS_D, N_UP, N_DOWN, N_BID_SIDE, N_ASK_SIDE, HEADER_WORDS
};
static_assert(ROW_WORDS == 16 && HEADER_WORDS <= ROW_WORDS, "a row of the depth table is 16 words, 128 B");

constexpr uint32_t MAX_LEVELS = 64u;
constexpr uint32_t REC_HEAD = 5u, LEVEL_WORDS = 4u;  // a record: five words, then four per level
using lags::M_BITS;
using lags::TWO;
using lags::word_of;

struct Row {
  uint64_t w[ROW_WORDS];
};

BKD_DEPTH_HD Row cleared() { return Row{}; }

// How the 64 lanes of a wave divide into (step, level): Lp is the power of two at or above L, a pass covers G = 64 / Lp
// consecutive steps, lane g * Lp + q reads level q of step pass * G + g
struct Lanes {
  uint32_t Lp, shift, G;  // Lp == 1 << shift
};
BKD_DEPTH_HD Lanes lanes_of(uint32_t L) {
  uint32_t shift = 0u;
  while ((1u << shift) < L) ++shift;
  return Lanes{1u << shift, shift, 64u >> shift};
}
BKD_DEPTH_HD uint32_t passes_of(const Lanes& a, uint32_t n) { return (n + a.G - 1u) >> (6u - a.shift); }
BKD_DEPTH_HD uint32_t level_of(const Lanes& a, uint32_t lane) { return lane & (a.Lp - 1u); }
BKD_DEPTH_HD uint32_t group_of(const Lanes& a, uint32_t lane) { return lane >> a.shift; }
BKD_DEPTH_HD uint32_t step_of(const Lanes& a, uint32_t pass, uint32_t lane) { return pass * a.G + group_of(a, lane); }
// the lane that holds level q of the fold's last step, n - 1, in the last pass
BKD_DEPTH_HD uint32_t last_lane(const Lanes& a, uint32_t n, uint32_t q) { return (((n - 1u) & (a.G - 1u)) << a.shift) + q; }
// the lane whose I_q is J for this lane one pass on, if this lane is of group 0: the last group's
BKD_DEPTH_HD uint32_t tail_lane(const Lanes& a, uint32_t q) { return ((a.G - 1u) << a.shift) + q; }

// where level q of a record starts, in words
BKD_DEPTH_HD uint32_t level_at(uint32_t q) { return REC_HEAD + LEVEL_WORDS * q; }

// a pair: the words of steps s and s - 1 are both two-sided; its move d = m_s - m_{s-1}
BKD_DEPTH_HD bool pair_of(uint64_t cur, uint64_t prev) { return (cur & prev & TWO) != 0ull; }
BKD_DEPTH_HD int64_t move_of(uint64_t cur, uint64_t prev) { return static_cast<int64_t>((cur & M_BITS) - (prev & M_BITS)); }

// r += level q of step s: its four words, I = I_q(s), J = I_q(s - 1), and the words of steps s, s - 1
BKD_DEPTH_HD void add_level(Row& r, uint32_t bv, uint32_t bn, uint32_t av, uint32_t an, int64_t I, int64_t J, uint64_t cur,
                            uint64_t prev) {
  r.w[SUM_BID_VOL] += bv;
  r.w[SUM_ASK_VOL] += av;
  r.w[SUM_BID_VOL_SQ] += static_cast<uint64_t>(bv) * bv;
  r.w[SUM_ASK_VOL_SQ] += static_cast<uint64_t>(av) * av;
  r.w[SUM_BID_ORDERS] += bn;
  r.w[SUM_ASK_ORDERS] += an;
  r.w[N_BID_STEPS] += bn > 0u ? 1u : 0u;
  r.w[N_ASK_STEPS] += an > 0u ? 1u : 0u;
  if (cur & TWO) {
    const uint64_t u = static_cast<uint64_t>(I);
    r.w[SUM_IMB] += u;
    r.w[SUM_IMB_SQ] += u * u;
    r.w[SUM_ABS_IMB] += series::abs_i64(I);
  }
  if (pair_of(cur, prev)) {
    const int64_t d = move_of(cur, prev);
    const uint64_t ud = static_cast<uint64_t>(d);
    const uint64_t sd = J > 0 ? ud : J < 0 ? 0ull - ud : 0ull;  // sgn(J) * d
    r.w[N_SIGNED] += J != 0 ? 1u : 0u;
    r.w[SUM_SIGN_D] += sd;
    r.w[N_AGREE] += static_cast<int64_t>(sd) > 0 ? 1u : 0u;
    r.w[SUM_IMB_D] += static_cast<uint64_t>(J) * ud;
    r.w[N_MOVE] += J != 0 && d != 0 ? 1u : 0u;
  }
}

// h += step s: its quotes, and the words of steps s, s - 1 (once per step, not once per level)
BKD_DEPTH_HD void add_header(Row& h, uint32_t bid, uint32_t ask, uint64_t cur, uint64_t prev) {
  h.w[N_STEPS] += 1u;
  h.w[N_TWO_SIDED] += cur & TWO ? 1u : 0u;
  h.w[N_BID_SIDE] += bid != 0u ? 1u : 0u;
  h.w[N_ASK_SIDE] += ask != series::NO_ASK ? 1u : 0u;
  if (pair_of(cur, prev)) {
    const int64_t d = move_of(cur, prev);
    h.w[N_PAIRS] += 1u;
    h.w[SUM_D] += static_cast<uint64_t>(d);
    h.w[SUM_ABS_D] += series::abs_i64(d);
    h.w[N_UP] += d > 0 ? 1u : 0u;
    h.w[N_DOWN] += d < 0 ? 1u : 0u;
  }
}

// r = the row of r's steps followed by part's (levels and header alike)
BKD_DEPTH_HD void merge(Row& r, const Row& part) {
  for (uint32_t k = 0; k < ROW_WORDS; ++k) r.w[k] += part.w[k];
}

}  // namespace depth
}  // namespace bkd
