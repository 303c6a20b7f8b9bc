// bins.hpp - bk_bins_*: per book C = S + 2 rows of B counts, folded on the device from the level-2 history ring: the
// distribution of the mid's change over S spans of k_j <= 64 steps, of the spread and of the traded volume per step.
//
// The reference has no counterpart (its users fold Env::level_2_data's history on the host).  The env keeps the table
// bins[n_books][C][B] of u64 counts (which bin a record raises is bin_fold.hpp's), a carry bins_carry[n_books][Kmax] of
// window words - entry i the record of step bins_seen - 1 - i, Kmax the longest span - and a host cursor bins_seen: the
// steps below it are folded.  k_fold runs on the env's stream when bk_bins_fold (or a reset, or a masked clear) asks for it,
// over the steps [lo, lo + n) that the stepping kernels have written to the ring - DESIGN.md 2.25:
//   * one wave per book, FOLD_WAVES waves per block (the last block may hold fewer books), one block of C x B u32 counters
//     in dynamic LDS per wave, zeroed first;
//   * one lane per STEP (a fold of more than 64 steps: steps s, s + 64, ..): the lane loads trade_vol, bid, ask of its own
//     record and, per span, bid and ask of the record k_j steps back - from the ring while that step belongs to the fold,
//     from the carry otherwise - and raises one LDS counter per channel with atomicAdd;
//   * behind a wave fence the lanes stride over the C x B counters and add the non-zero ones to the u64 rows: the wave owns
//     its book, so no global atomic is needed, and a bin the fold did not raise is neither read nor written;
//   * lane i < Kmax then builds carry entry i from the ring or from the old carry; every read stands before the fence,
//     every write behind it.
// Integer adds only: the result does not depend on the order in which the counters are raised.
// k_clear clears the rows and carry of the masked books, or with carry_only just their carry (the resets' cut).
// Plain C++, no scratch, no global atomics, vector loads and stores only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bin_fold.hpp"
#include "book_device.hpp"
#include "hist_ring.hpp"

namespace bkd {
namespace bins {

constexpr int FOLD_WAVES = 4;  // waves (books) per block of k_fold / k_clear

using ring::wave_sync;

struct FoldArgs {
  ring::Span ring;
  uint32_t B, S, Kmax;
  uint32_t spans;  // k_j in byte j (a register shift, not an indexed argument)
  uint32_t ret_width, spread_width, vol_width;
  uint64_t* rows;   // [n_books][S + 2][B]
  uint64_t* carry;  // [n_books][Kmax]
};

// LDS bytes of one block of k_fold
inline size_t fold_lds_bytes(uint32_t S, uint32_t B) { return static_cast<size_t>(FOLD_WAVES) * (S + 2u) * B * sizeof(uint32_t); }

// the window word of step `at` of the fold
__device__ __forceinline__ uint64_t ring_word(const FoldArgs& g, uint32_t b, uint32_t at) {
  const uint32_t* rec = ring::record(g.ring, slot_of(g.ring.slot0, at, g.ring.hist_cap), b);
  return word_of(rec[1], rec[2]);
}

__global__ __launch_bounds__(64 * FOLD_WAVES) void k_fold(FoldArgs g) {
  extern __shared__ uint32_t counters[];  // [FOLD_WAVES][S + 2][B]
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = rfl(threadIdx.x >> 6);
  const uint32_t b = rfl(blockIdx.x * FOLD_WAVES + wave);
  if (b >= g.ring.n_books) return;  // (no block-wide barrier below: a wave is on its own)
  const uint32_t B = g.B, S = g.S, CB = (S + 2u) * B;
  uint32_t* cnt = counters + wave * CB;
  uint64_t* carry = g.carry + static_cast<size_t>(b) * g.Kmax;
  for (uint32_t v = lane; v < CB; v += 64u) cnt[v] = 0u;
  wave_sync();

  for (uint32_t i = lane; i < g.ring.n; i += 64u) {  // step lo + i
    const uint32_t* rec = ring::record(g.ring, slot_of(g.ring.slot0, i, g.ring.hist_cap), b);
    const uint32_t tv = rec[0], bid = rec[1], ask = rec[2];
    const uint64_t cur = word_of(bid, ask);
    atomicAdd(&cnt[(S + 1u) * B + vol_bin(tv, g.vol_width, B)], 1u);
    if (cur & TWO) {
      atomicAdd(&cnt[S * B + spread_bin(bid, ask, g.spread_width, B)], 1u);
      for (uint32_t j = 0; j < S; ++j) {
        const Where w = partner(i, (g.spans >> (8u * j)) & 0xFFu);
        const uint64_t at_k = w.in_ring ? ring_word(g, b, w.at) : carry[w.at];
        if (at_k & TWO) atomicAdd(&cnt[j * B + ret_bin(cur, at_k, g.ret_width, B)], 1u);
      }
    }
  }
  wave_sync();

  uint64_t* rows = g.rows + static_cast<size_t>(b) * CB;
  for (uint32_t v = lane; v < CB; v += 64u) {
    const uint32_t c = cnt[v];
    if (c) rows[v] += c;
  }

  // the carry behind the fold: every entry is read (ring or old carry) before any is written
  uint64_t mine = 0ull;
  if (lane < g.Kmax) {
    const Where w = next_carry(g.ring.n, lane);
    mine = w.in_ring ? ring_word(g, b, w.at) : carry[w.at];
  }
  wave_sync();
  if (lane < g.Kmax) carry[lane] = mine;
}

struct ClearArgs {
  ring::Masked books;
  uint32_t CB;          // counts per book, (S + 2) * B
  uint32_t Kmax;
  uint32_t carry_only;  // 1: only the carry (no span reaches over a reset; the counts go on)
  uint64_t* rows;
  uint64_t* carry;
};

__global__ __launch_bounds__(64 * FOLD_WAVES) void k_clear(ClearArgs g) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t b = ring::masked_book(g.books, FOLD_WAVES);
  if (b == ring::NO_BOOK) return;
  uint64_t* carry = g.carry + static_cast<size_t>(b) * g.Kmax;
  if (lane < g.Kmax) carry[lane] = 0ull;
  if (g.carry_only) return;
  uint64_t* rows = g.rows + static_cast<size_t>(b) * g.CB;
  for (uint32_t v = lane; v < g.CB; v += 64u) rows[v] = 0ull;
}

}  // namespace bins
}  // namespace bkd
