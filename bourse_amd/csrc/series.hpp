// series.hpp - bk_series_*: one row of integer series moments per book, folded on the device from the level-2 history ring.
//
// The reference has no counterpart (its users fold Env::level_2_data's history on the host).  The env keeps series[n_books]
// rows of 192 B, twelve 16-byte vectors (bk_series_row; the words and what one record adds are series_fold.hpp's), and a
// host cursor series_seen: the steps below it are folded.  k_fold runs on the env's stream when bk_series_fold (or a reset,
// or a masked clear) asks for it, over the steps [lo, lo + n) that the stepping kernels have written to the ring -
// DESIGN.md 2.22:
//   * one wave per book, FOLD_WAVES waves per block (the last block may hold fewer books);
//   * one lane per STEP: the lane of step s loads the first five words of its own record and bid, ask of the records of
//     steps s - 1 and s - 2 - from the ring while those steps are >= lo, from the row's carry words (the values in front of
//     step lo) otherwise - so its term is self-contained and no lane waits for a neighbour;
//   * a fold of more than 64 steps has every lane accumulate its steps s, s + 64, .. in 64-bit registers (series::add);
//   * ONE reduction at the end: the sums from wrapping u32 wave sums of 16-bit limbs (64 x 65 535 fits a u32) recombined
//     modulo 2^64 (the 128-bit pair: eight limbs, modulo 2^128), the three extremes by wave_umax / wave_umin on halves;
//   * lane 0 adds to the row it reads, takes the carry from the lane of the last step, and writes the twelve vectors.
// k_clear clears the rows of the masked books, or with carry_only just their two carry words (the resets' cut).
// Plain C++, no LDS, no scratch, no atomics, vector loads and stores only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "book_device.hpp"
#include "hist_ring.hpp"
#include "series_fold.hpp"

namespace bkd {
namespace series {

constexpr int FOLD_WAVES = 4;      // waves (books) per block of k_fold / k_clear
constexpr uint32_t ROW_VECS = 12u;  // 16-byte vectors per row

using ring::vec_hi;
using ring::vec_lo;
using ring::vec_of;

struct FoldArgs {
  ring::Span ring;
  bk_u32x4* rows;  // [n_books][12]
};

// (wave_sum_u32 / wave_sum_u64, the wave's exact and modulo-2^64 sums, stand beside wave_add in book_device.hpp)
// the sum of the wave's 64 word pairs modulo 2^128: the low word's sum is exact (70 bits), its carry goes to the high word
__device__ __forceinline__ void wave_sum_u128(uint64_t lo, uint64_t hi, uint64_t& out_lo, uint64_t& out_hi) {
  const uint64_t s0 = wave_sum_u32(static_cast<uint32_t>(lo));        // < 2^38
  const uint64_t s1 = wave_sum_u32(static_cast<uint32_t>(lo >> 32));  // < 2^38, weighs 2^32
  out_lo = s0 + (s1 << 32);
  const uint64_t carry = (s1 >> 32) + (out_lo < s0 ? 1u : 0u);
  out_hi = wave_sum_u64(hi) + carry;
}

// the wave's largest / smallest 64-bit word: the high halves first, then the low halves of the lanes that hold that high half
__device__ __forceinline__ uint64_t wave_umax64(uint64_t x) {
  const uint32_t hi = wave_umax(static_cast<uint32_t>(x >> 32));
  const uint32_t lo = wave_umax(static_cast<uint32_t>(x >> 32) == hi ? static_cast<uint32_t>(x) : 0u);
  return mk64(lo, hi);
}
__device__ __forceinline__ uint64_t wave_umin64(uint64_t x) {
  const uint32_t hi = wave_umin(static_cast<uint32_t>(x >> 32));
  const uint32_t lo = wave_umin(static_cast<uint32_t>(x >> 32) == hi ? static_cast<uint32_t>(x) : 0xFFFFFFFFu);
  return mk64(lo, hi);
}

__device__ __forceinline__ uint64_t rdl64(uint64_t v, uint32_t lane) {
  return mk64(rdl(static_cast<uint32_t>(v), lane), rdl(static_cast<uint32_t>(v >> 32), lane));
}

__global__ __launch_bounds__(64 * FOLD_WAVES) void k_fold(FoldArgs g) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t b = rfl(blockIdx.x * FOLD_WAVES + (threadIdx.x >> 6));
  if (b >= g.ring.n_books) return;
  bk_u32x4* row = g.rows + static_cast<size_t>(b) * ROW_VECS;
  const bk_u32x4 cv = row[CARRY_M / 2];  // {carry_m, carry_d}: the values in front of step lo
  const Prev carry = unpack(mk64(rfl(cv.x), rfl(cv.y)), mk64(rfl(cv.z), rfl(cv.w)));
  const uint64_t cap = g.ring.hist_cap;

  Row acc = cleared();
  Prev last = carry;  // the values behind this lane's latest step
  for (uint32_t i = lane; i < g.ring.n; i += 64u) {  // step lo + i; i, slot0 < cap: no division
    const uint64_t slot = ring::slot_of(g.ring.slot0, i, cap);
    const uint32_t* rec = ring::record(g.ring, slot, b);
    const uint32_t tv = rec[0], bid = rec[1], ask = rec[2], ask_vol = rec[3], bid_vol = rec[4];
    Prev p = carry;
    if (i >= 1u) {
      const uint64_t slot1 = slot == 0u ? cap - 1u : slot - 1u;
      const uint32_t* rec1 = ring::record(g.ring, slot1, b);
      Prev before1 = carry;  // (step lo - 1: only have_m and m are read)
      if (i >= 2u) {
        const uint64_t slot2 = slot1 == 0u ? cap - 1u : slot1 - 1u;
        const uint32_t* rec2 = ring::record(g.ring, slot2, b);
        before1 = quotes_only(rec2[1], rec2[2]);
      }
      p = prev_of(rec1[1], rec1[2], before1);
    }
    const Term t = term(tv, bid, ask, ask_vol, bid_vol, p);
    add(acc, t);
    last = next(t);
  }

  // one reduction: every lane takes part (a lane without a step holds the cleared row)
  Row sum = cleared();
  sum.w[N_STEPS] = g.ring.n;
  sum.w[N_TWO_SIDED] = wave_sum_u32(static_cast<uint32_t>(acc.w[N_TWO_SIDED]));  // (a lane's counts are below 2^26)
  sum.w[N_TRADE_STEPS] = wave_sum_u32(static_cast<uint32_t>(acc.w[N_TRADE_STEPS]));
  sum.w[N_RET] = wave_sum_u32(static_cast<uint32_t>(acc.w[N_RET]));
  sum.w[N_PAIRS] = wave_sum_u32(static_cast<uint32_t>(acc.w[N_PAIRS]));
  sum.w[SUM_M] = wave_sum_u64(acc.w[SUM_M]);
  sum.w[SUM_SPREAD] = wave_sum_u64(acc.w[SUM_SPREAD]);
  sum.w[SUM_SPREAD_SQ] = wave_sum_u64(acc.w[SUM_SPREAD_SQ]);
  sum.w[SUM_BID_VOL] = wave_sum_u64(acc.w[SUM_BID_VOL]);
  sum.w[SUM_ASK_VOL] = wave_sum_u64(acc.w[SUM_ASK_VOL]);
  sum.w[SUM_TRADE_VOL] = wave_sum_u64(acc.w[SUM_TRADE_VOL]);
  sum.w[SUM_TRADE_VOL_SQ] = wave_sum_u64(acc.w[SUM_TRADE_VOL_SQ]);
  sum.w[SUM_D] = wave_sum_u64(acc.w[SUM_D]);
  sum.w[SUM_ABS_D] = wave_sum_u64(acc.w[SUM_ABS_D]);
  sum.w[SUM_D2] = wave_sum_u64(acc.w[SUM_D2]);
  wave_sum_u128(acc.w[SUM_D4_LO], acc.w[SUM_D4_HI], sum.w[SUM_D4_LO], sum.w[SUM_D4_HI]);
  sum.w[SUM_DD] = wave_sum_u64(acc.w[SUM_DD]);
  sum.w[SUM_ABS_DD] = wave_sum_u64(acc.w[SUM_ABS_DD]);
  sum.w[MAX_ABS_D] = wave_umax64(acc.w[MAX_ABS_D]);
  sum.w[MIN_M] = wave_umin64(acc.w[MIN_M]);
  sum.w[MAX_M] = wave_umax64(acc.w[MAX_M]);
  // the carry is the last step's: its lane's latest
  const uint32_t owner = (g.ring.n - 1u) & 63u;
  Prev tail;
  tail.have_m = rdl(last.have_m, owner);
  tail.have_d = rdl(last.have_d, owner);
  tail.m = rdl64(last.m, owner);
  tail.d = static_cast<int64_t>(rdl64(static_cast<uint64_t>(last.d), owner));

  if (lane == 0) {
    Row r;
#pragma unroll
    for (uint32_t v = 0; v < ROW_VECS - 1u; ++v) {
      const bk_u32x4 x = row[v];
      r.w[2 * v] = vec_lo(x), r.w[2 * v + 1] = vec_hi(x);
    }
    merge(r, sum);
    pack(r, tail);
#pragma unroll
    for (uint32_t v = 0; v < ROW_VECS; ++v) row[v] = vec_of(r.w[2 * v], r.w[2 * v + 1]);
  }
}

struct ClearArgs {
  ring::Masked books;
  uint32_t carry_only;  // 1: only the two carry words (no return spans a reset; the sums go on)
  bk_u32x4* rows;
};

__global__ __launch_bounds__(64 * FOLD_WAVES) void k_clear(ClearArgs g) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t b = ring::masked_book(g.books, FOLD_WAVES);
  if (b == ring::NO_BOOK) return;
  bk_u32x4* row = g.rows + static_cast<size_t>(b) * ROW_VECS;
  // cleared(): all zeros except min_m, the low word of its vector
  static_assert(MIN_M % 2 == 0 && CARRY_M % 2 == 0 && CARRY_D == CARRY_M + 1, "the vectors of min_m and of the carry");
  if (lane < ROW_VECS && (!g.carry_only || lane == CARRY_M / 2)) row[lane] = vec_of(lane == MIN_M / 2 ? ~0ull : 0ull, 0ull);
}

}  // namespace series
}  // namespace bkd
