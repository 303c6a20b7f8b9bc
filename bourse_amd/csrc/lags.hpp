// lags.hpp - bk_lags_*: K rows of integer sums per book, one per lag k = 1 .. K <= 64, folded on the device from the
// level-2 history ring: the autocovariance of the mid's step-to-step change and of its magnitude at lag k, and the moments of
// the change over a span of k steps.
//
// The reference has no counterpart (its users fold Env::level_2_data's history on the host).  The env keeps rows
// lags[n_books][K] of 80 B, five 16-byte vectors (bk_lag_row; the words and what one record adds are lag_fold.hpp's), a
// carry lag_carry[n_books][K + 1] of window words - entry j the record of step lags_seen - 1 - j - and a host cursor
// lags_seen: the steps below it are folded.  k_fold runs on the env's stream when bk_lags_fold (or a reset, or a masked
// clear) asks for it, over the steps [lo, lo + n) that the stepping kernels have written to the ring - DESIGN.md 2.24:
//   * one wave per book, FOLD_WAVES waves per block (the last block may hold fewer books), one window of
//     WINDOW_WORDS 8-byte words in LDS per wave, which opens with the K + 1 carry words;
//   * per chunk of up to 64 steps, one lane per STEP loads bid, ask of its record and appends their word to the window;
//   * the wave then walks the chunk's steps in order with one lane per LAG: the words of steps s and s - 1 are wave-uniform
//     (a readlane of the lane that loaded s), lane k - 1 reads those of s - k and s - k - 1 from the window - neighbouring
//     lanes neighbouring words - and adds its two terms to its own ten accumulators (lags::add);
//   * the window's last K + 1 words move to its front for the next chunk, and at the end to the carry;
//   * NO cross-lane reduction: lane k - 1 adds its accumulators to the row it reads and writes the five vectors.
// k_clear clears the rows and carry of the masked books, or with carry_only just their carry (the resets' cut).
// Plain C++, no scratch, no atomics, vector loads and stores only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "book_device.hpp"
#include "hist_ring.hpp"
#include "lag_fold.hpp"

namespace bkd {
namespace lags {

constexpr int FOLD_WAVES = 4;      // waves (books) per block of k_fold / k_clear
constexpr uint32_t ROW_VECS = 5u;  // 16-byte vectors per row

using ring::vec_hi;
using ring::vec_lo;
using ring::vec_of;
using ring::wave_sync;

struct FoldArgs {
  ring::Span ring;
  uint32_t K;       // lags, 1 .. MAX_LAGS
  bk_u32x4* rows;   // [n_books][K][5]
  uint64_t* carry;  // [n_books][K + 1]
};

__global__ __launch_bounds__(64 * FOLD_WAVES) void k_fold(FoldArgs g) {
  __shared__ uint64_t windows[FOLD_WAVES][WINDOW_WORDS];
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = rfl(threadIdx.x >> 6);
  const uint32_t b = rfl(blockIdx.x * FOLD_WAVES + wave);
  if (b >= g.ring.n_books) return;  // (no block-wide barrier below: a wave is on its own)
  const uint32_t K = g.K;
  uint64_t* win = windows[wave];
  uint64_t* carry = g.carry + static_cast<size_t>(b) * (K + 1u);
  for (uint32_t j = lane; j <= K; j += 64u) win[carry_at(K, j)] = carry[j];
  const uint64_t cap = g.ring.hist_cap;

  Row acc{};
  for (uint32_t base = 0; base < g.ring.n; base += CHUNK) {
    const uint32_t cnt = g.ring.n - base < CHUNK ? g.ring.n - base : CHUNK;  // this chunk's steps: wave-uniform
    uint64_t mine = 0;
    if (lane < cnt) {  // step lo + base + lane; base + lane < n <= cap, slot0 < cap: no division
      const uint32_t* rec = ring::record(g.ring, ring::slot_of(g.ring.slot0, base + lane, cap), b);
      mine = word_of(rec[1], rec[2]);
      win[step_at(K, lane)] = mine;
    }
    wave_sync();
    uint64_t prev = win[carry_at(K, 0)];  // the step in front of the chunk (every lane reads the same word)
    for (uint32_t i = 0; i < cnt; ++i) {
      const uint64_t cur = mk64(rdl(static_cast<uint32_t>(mine), i), rdl(static_cast<uint32_t>(mine >> 32), i));
      if (lane < K) {
        const uint32_t at = step_at(K, i) - (lane + 1u);  // >= 1: the word in front of it exists
        add(acc, cur, prev, win[at], win[at - 1u]);
      }
      prev = cur;
    }
    // the window's last K + 1 words become its front: words [cnt, cnt + K] -> [0, K] (read by all before any is written)
    wave_sync();
    const uint64_t front = lane <= K ? win[cnt + lane] : 0ull;
    const uint64_t front64 = K == MAX_LAGS && lane == 0u ? win[cnt + MAX_LAGS] : 0ull;  // (K + 1 = 65 words, 64 lanes)
    wave_sync();
    if (lane <= K) win[lane] = front;
    if (K == MAX_LAGS && lane == 0u) win[MAX_LAGS] = front64;
    wave_sync();
  }

  if (lane < K) {  // lane k - 1 owns row k - 1
    bk_u32x4* row = g.rows + (static_cast<size_t>(b) * K + lane) * ROW_VECS;
    Row r;
#pragma unroll
    for (uint32_t v = 0; v < ROW_VECS; ++v) {
      const bk_u32x4 x = row[v];
      r.w[2 * v] = vec_lo(x), r.w[2 * v + 1] = vec_hi(x);
    }
    merge(r, acc);
#pragma unroll
    for (uint32_t v = 0; v < ROW_VECS; ++v) row[v] = vec_of(r.w[2 * v], r.w[2 * v + 1]);
  }
  for (uint32_t j = lane; j <= K; j += 64u) carry[j] = win[carry_at(K, j)];
}

struct ClearArgs {
  ring::Masked books;
  uint32_t K;
  uint32_t carry_only;  // 1: only the carry (no span or pair reaches over a reset; the sums go on)
  bk_u32x4* rows;
  uint64_t* carry;
};

__global__ __launch_bounds__(64 * FOLD_WAVES) void k_clear(ClearArgs g) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t b = ring::masked_book(g.books, FOLD_WAVES);
  if (b == ring::NO_BOOK) return;
  uint64_t* carry = g.carry + static_cast<size_t>(b) * (g.K + 1u);
  for (uint32_t j = lane; j <= g.K; j += 64u) carry[j] = 0ull;
  if (g.carry_only) return;
  bk_u32x4* rows = g.rows + static_cast<size_t>(b) * g.K * ROW_VECS;
  for (uint32_t v = lane; v < g.K * ROW_VECS; v += 64u) rows[v] = vec_of(0ull, 0ull);
}

}  // namespace lags
}  // namespace bkd
