// candle_fold.hpp - which bar and slot of a book's candle table a step belongs to, which bars a fold skips, when a slot's row
// is continued and when restarted, what ONE level-2 record adds to its bar, how two partial bars merge, and which lanes of
// the device fold form one bar's segment (bk_candles_enable).
//
// Compiled by the device fold (candles.hpp) and by a CPU test (tests/cpp/candle_fold_test.cpp): no HIP type, no intrinsic.
// Of a record only trade_vol, bid_price and ask_price are read (words 0 .. 2); an empty side reads bid_price == 0 /
// ask_price == 0xFFFFFFFF.  A record's WORD {two, m} is the lag table's (lag_fold.hpp).  With bars of W steps and N slots a
// book, absolute step s belongs to bar j = s / W, which lives in slot j % N.  A bar's row is a PART: the sixteen words below
// over a run of consecutive steps of one bar; a part without a step (n_steps == 0) is the merge's identity.  Step s adds
//   always:            one step, trade_vol, and one count if it traded;
//   if two_s:          m = bid + ask as open / high / low / close and to sum_m, (ask - bid) as a wrapping u32;
//   if two_s, two_s-1: the return d = m_s - m_{s-1} - the step before may lie in the bar before, or come from the carry.
// The carry is the word of the last folded step: a cleared carry (0) is a step that is not two-sided, so it forms no return.
// All 64-bit words are sums modulo 2^64; sum_d is two's complement.
#pragma once
#include <stdint.h>

#include "lag_fold.hpp"  // lags::word_of, lags::TWO, lags::M_BITS (and series::abs_i64, umax64, umin64 behind them)

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BKD_CANDLES_HD __host__ __device__ inline
#else
#define BKD_CANDLES_HD inline
#endif

namespace bkd {
namespace candles {

enum Word : uint32_t {  // a bar's row, word by word
  FIRST_STEP = 0, N_STEPS, N_TWO_SIDED, OPEN_M, HIGH_M, LOW_M, CLOSE_M, SUM_M, SUM_SPREAD, SUM_TRADE_VOL, N_TRADE_STEPS,
  N_RET, SUM_D, SUM_ABS_D, SUM_D2, MAX_ABS_D, ROW_WORDS
};
static_assert(ROW_WORDS == 16, "a row of the candle table is 16 words, 128 B");

constexpr uint32_t MAX_WIDTH = 1u << 20, MAX_CANDLES = 1u << 16;
using lags::M_BITS;
using lags::TWO;
using lags::word_of;

struct Part {
  uint64_t w[ROW_WORDS];
};

BKD_CANDLES_HD Part cleared() { return Part{}; }

// the bar of an absolute step, its first step, and the slot it lives in
BKD_CANDLES_HD uint64_t bar_of(uint64_t step, uint32_t W) { return step / W; }
BKD_CANDLES_HD uint64_t bar_start(uint64_t bar, uint32_t W) { return bar * W; }
BKD_CANDLES_HD uint32_t slot_of_bar(uint64_t bar, uint32_t N) { return static_cast<uint32_t>(bar % N); }

// a fold whose last step lies in bar `last` does not write bar j at all if its slot belongs to a later bar of the same fold
BKD_CANDLES_HD bool skipped(uint64_t bar, uint64_t last, uint32_t N) { return bar + N <= last; }

// the row a slot holds is bar j's own (and is continued) if it holds a step and its first step lies in bar j - without a
// division: first_step - j W, as a wrapping difference, is below W; otherwise the slot is restarted
BKD_CANDLES_HD bool continues(const Part& row, uint64_t bar, uint32_t W) {
  return row.w[N_STEPS] != 0ull && row.w[FIRST_STEP] - bar_start(bar, W) < W;
}

// the part of ONE step: `step` is absolute, cur and prev the words of steps s and s - 1 (prev: 0 behind a cut)
BKD_CANDLES_HD Part term(uint64_t step, uint32_t trade_vol, uint32_t bid, uint32_t ask, uint64_t cur, uint64_t prev) {
  Part p{};
  p.w[FIRST_STEP] = step;
  p.w[N_STEPS] = 1u;
  p.w[SUM_TRADE_VOL] = trade_vol;
  p.w[N_TRADE_STEPS] = trade_vol > 0u ? 1u : 0u;
  if (cur & TWO) {
    const uint64_t m = cur & M_BITS;
    p.w[N_TWO_SIDED] = 1u;
    p.w[OPEN_M] = p.w[HIGH_M] = p.w[LOW_M] = p.w[CLOSE_M] = p.w[SUM_M] = m;
    p.w[SUM_SPREAD] = static_cast<uint32_t>(ask - bid);
    if (prev & TWO) {
      const int64_t d = static_cast<int64_t>(m - (prev & M_BITS));
      const uint64_t a = series::abs_i64(d);
      p.w[N_RET] = 1u;
      p.w[SUM_D] = static_cast<uint64_t>(d);
      p.w[SUM_ABS_D] = a;
      p.w[SUM_D2] = a * a;
      p.w[MAX_ABS_D] = a;
    }
  }
  return p;
}

// the part of a's steps followed by b's, both of the same bar: open is the first two-sided step's, close the last's, the
// low is not polluted by the zeros of a side without a two-sided step (a two-sided m is >= 1, so the high cannot be)
BKD_CANDLES_HD Part merge(const Part& a, const Part& b) {
  Part r;
  const bool a2 = a.w[N_TWO_SIDED] != 0ull, b2 = b.w[N_TWO_SIDED] != 0ull;
  r.w[FIRST_STEP] = a.w[N_STEPS] != 0ull ? a.w[FIRST_STEP] : b.w[FIRST_STEP];  // (the only word an empty part would spoil)
  r.w[N_STEPS] = a.w[N_STEPS] + b.w[N_STEPS];
  r.w[N_TWO_SIDED] = a.w[N_TWO_SIDED] + b.w[N_TWO_SIDED];
  r.w[OPEN_M] = a2 ? a.w[OPEN_M] : b.w[OPEN_M];
  r.w[HIGH_M] = series::umax64(a.w[HIGH_M], b.w[HIGH_M]);
  r.w[LOW_M] = !a2 ? b.w[LOW_M] : !b2 ? a.w[LOW_M] : series::umin64(a.w[LOW_M], b.w[LOW_M]);
  r.w[CLOSE_M] = b2 ? b.w[CLOSE_M] : a.w[CLOSE_M];
  r.w[SUM_M] = a.w[SUM_M] + b.w[SUM_M];
  r.w[SUM_SPREAD] = a.w[SUM_SPREAD] + b.w[SUM_SPREAD];
  r.w[SUM_TRADE_VOL] = a.w[SUM_TRADE_VOL] + b.w[SUM_TRADE_VOL];
  r.w[N_TRADE_STEPS] = a.w[N_TRADE_STEPS] + b.w[N_TRADE_STEPS];
  r.w[N_RET] = a.w[N_RET] + b.w[N_RET];
  r.w[SUM_D] = a.w[SUM_D] + b.w[SUM_D];
  r.w[SUM_ABS_D] = a.w[SUM_ABS_D] + b.w[SUM_ABS_D];
  r.w[SUM_D2] = a.w[SUM_D2] + b.w[SUM_D2];
  r.w[MAX_ABS_D] = series::umax64(a.w[MAX_ABS_D], b.w[MAX_ABS_D]);
  return r;
}

// what a slot holds once `part` of bar j is folded into it
BKD_CANDLES_HD Part merged_row(const Part& row, const Part& part, uint64_t bar, uint32_t W) {
  return continues(row, bar, W) ? merge(row, part) : part;
}

// Where a pass of 64 consecutive steps stands: the bar of its first step, that step's phase inside the bar, the bar's slot.
// The host gives the first pass's (seen / W, seen % W, (seen / W) % N); every later one follows by 32-bit arithmetic.
struct Pass {
  uint64_t bar;
  uint32_t phase, slot;
};
BKD_CANDLES_HD Pass first_pass(uint64_t step, uint32_t W, uint32_t N) {
  const uint64_t bar = bar_of(step, W);
  return Pass{bar, static_cast<uint32_t>(step - bar_start(bar, W)), slot_of_bar(bar, N)};
}
BKD_CANDLES_HD Pass next_pass(const Pass& p, uint32_t W, uint32_t N) {
  const uint32_t x = p.phase + 64u, adv = x / W;  // adv <= 64
  return Pass{p.bar + adv, x - adv * W, (p.slot + adv % N) % N};
}

// The lane-to-segment mapping: lane l of a pass holds the step `l` behind the pass's first.  The lanes of one bar are a
// contiguous range; its HEAD is the lane of phase 0, or lane 0; its TAIL the lane of phase W - 1, or lane 63, or the lane
// of the fold's last step.  The tail merges the segment into the bar's row.
struct Seg {
  uint32_t rel;    // bars behind the pass's first
  uint32_t phase;  // of this lane's step inside its bar
  uint32_t slot;
  bool head;
};
BKD_CANDLES_HD Seg seg_of(const Pass& p, uint32_t lane, uint32_t W, uint32_t N) {
  const uint32_t x = p.phase + lane, rel = x / W, phase = x - rel * W;  // x < 2^20 + 64, rel <= 64
  return Seg{rel, phase, (p.slot + rel % N) % N, phase == 0u || lane == 0u};
}
// i: the lane's step inside the fold of n steps (i < n)
BKD_CANDLES_HD bool tail_of(const Seg& s, uint32_t lane, uint32_t i, uint32_t n, uint32_t W) {
  return s.phase == W - 1u || lane == 63u || i == n - 1u;
}

// One round of the head-flagged segmented scan, for the lane that has fetched (below, below_head) from `off` lanes down:
// a lane whose segment started at or behind lane - off + 1 keeps its own
BKD_CANDLES_HD void scan_round(Part& mine, bool& head, const Part& below, bool below_head, uint32_t lane, uint32_t off) {
  if (lane >= off && !head) {
    mine = merge(below, mine);
    head = below_head;
  }
}

}  // namespace candles
}  // namespace bkd
