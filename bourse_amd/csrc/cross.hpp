// cross.hpp - bk_cross_*: S * A * A rows of integer sums per MARKET of an env of markets (A = assets >= 2 books each), one per
// span h = spans[j] (S <= 4 of them, 1 .. 64 steps) and ORDERED pair of assets (a, b), folded on the device from the level-2
// history ring: the moments behind the covariance of the two assets' changes of the mid over h steps, and the product of
// a's change with b's PREVIOUS one (who leads whom).
//
// The reference has no counterpart (its users fold Env::level_2_data's history on the host).  The env keeps rows
// cross_rows[n_markets][S][A][A] of 64 B, four 16-byte vectors (bk_cross_row; the words and what one step adds are
// cross_fold.hpp's), a carry cross_carry[n_markets][A][2 * Hmax] of window words - Hmax the longest span, entry j of an asset
// the record of step cross_seen - 2 * Hmax + j - and a host cursor: the steps below it are folded.  k_fold runs on the env's
// stream when bk_cross_fold (or a reset, or a masked clear) asks for it, over the steps [lo, lo + n) that the stepping
// kernels have written to the ring - DESIGN.md 2.29:
//   * one wave per MARKET, FOLD_WAVES waves per block (the last block may hold fewer markets), A windows of
//     2 * Hmax + 64 8-byte words in dynamic LDS per wave, each of which opens with the asset's 2 * Hmax carry words;
//   * per chunk of up to 64 steps, one lane per STEP loads bid, ask of each of the market's A records - a wave-uniform loop
//     over the assets - and appends their words to the windows;
//   * the wave then walks the chunk's steps in order with one lane per UNIT u = j * A * A + a * A + b < U = S * A * A <= 256:
//     lane l owns units l, l + 64, l + 128, l + 192 - up to four rounds, each with its own eight accumulators in registers
//     and a wave-uniform test of whether the round exists - and reads its five words of the step from the two windows
//     (cross::add);
//   * the windows' last 2 * Hmax words move to their front for the next chunk, and at the end to the carry;
//   * NO cross-lane reduction: a lane adds its accumulators to the rows it owns, read and written as four vectors each.
// k_clear clears the rows and carry of the masked markets, or with carry_only just their carry (the resets' cut).
// Plain C++, no scratch, no atomics, vector loads and stores only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "book_device.hpp"
#include "cross_fold.hpp"
#include "hist_ring.hpp"

namespace bkd {
namespace cross {

constexpr int FOLD_WAVES = 4;      // waves (markets) per block of k_fold / k_clear
constexpr uint32_t ROW_VECS = 4u;  // 16-byte vectors per row
static_assert(MAX_UNITS == 4u * 64u, "a lane owns at most four units: k_fold keeps four sets of accumulators");

using ring::vec_hi;
using ring::vec_lo;
using ring::vec_of;
using ring::wave_sync;

struct FoldArgs {
  ring::Span ring;   // (n_books = n_markets * A)
  uint32_t A, S, Hmax;
  uint32_t spans;    // h_j in byte j (a register shift, not an indexed argument)
  bk_u32x4* rows;    // [n_markets][S][A][A][4]
  uint64_t* carry;   // [n_markets][A][2 * Hmax]
};

// LDS bytes of one block of k_fold: FOLD_WAVES markets of A windows
inline size_t fold_lds_bytes(uint32_t A, uint32_t Hmax) {
  return static_cast<size_t>(FOLD_WAVES) * A * window_words(Hmax) * sizeof(uint64_t);
}

// what a lane knows of one of its units: where the two assets' windows stand, and the span (0: the lane has no such unit)
struct Mine {
  uint32_t at_a, at_b, h;
};

__device__ __forceinline__ Mine mine_of(const FoldArgs& g, uint32_t u) {
  if (u >= units(g.S, g.A)) return {0u, 0u, 0u};
  const Unit q = unit_at(g.A, u);
  return {window_at(g.Hmax, q.a), window_at(g.Hmax, q.b), (g.spans >> (8u * q.j)) & 0xFFu};
}

// acc += step `at` (a window position, >= 2 * Hmax) of the unit
__device__ __forceinline__ void add_step(Row& acc, const uint64_t* win, const Mine& q, uint32_t at) {
  if (!q.h) return;
  const uint64_t* wa = win + q.at_a + at;
  const uint64_t* wb = win + q.at_b + at;
  add(acc, wa[0], wa[-static_cast<int>(q.h)], wb[0], wb[-static_cast<int>(q.h)], wb[-2 * static_cast<int>(q.h)]);
}

// row += acc, as four vectors read and four written
__device__ __forceinline__ void add_to_row(bk_u32x4* row, const Row& acc) {
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

__global__ __launch_bounds__(64 * FOLD_WAVES) void k_fold(FoldArgs g) {
  extern __shared__ uint64_t windows[];  // [FOLD_WAVES][A][2 * Hmax + CHUNK]
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = rfl(threadIdx.x >> 6);
  const uint32_t m = rfl(blockIdx.x * FOLD_WAVES + wave);
  const uint32_t A = g.A, Hmax = g.Hmax;
  if (m >= g.ring.n_books / A) return;  // (no block-wide barrier below: a wave is on its own)
  const uint32_t U = units(g.S, A), C = carry_words(Hmax);
  uint64_t* win = windows + wave * A * window_words(Hmax);
  uint64_t* carry = g.carry + static_cast<size_t>(m) * A * C;
  for (uint32_t a = 0; a < A; ++a)
    for (uint32_t j = lane; j < C; j += 64u) win[window_at(Hmax, a) + carry_at(j)] = carry[a * C + j];
  const uint64_t cap = g.ring.hist_cap;

  const Mine q0 = mine_of(g, lane), q1 = mine_of(g, lane + 64u), q2 = mine_of(g, lane + 128u), q3 = mine_of(g, lane + 192u);
  Row acc0{}, acc1{}, acc2{}, acc3{};
  for (uint32_t base = 0; base < g.ring.n; base += CHUNK) {
    const uint32_t cnt = g.ring.n - base < CHUNK ? g.ring.n - base : CHUNK;  // this chunk's steps: wave-uniform
    if (lane < cnt) {  // step lo + base + lane; base + lane < n <= cap, slot0 < cap: no division
      const uint64_t slot = ring::slot_of(g.ring.slot0, base + lane, cap);
      for (uint32_t a = 0; a < A; ++a) {
        const uint32_t* rec = ring::record(g.ring, slot, m * A + a);
        win[window_at(Hmax, a) + step_at(Hmax, lane)] = word_of(rec[1], rec[2]);
      }
    }
    wave_sync();
    for (uint32_t i = 0; i < cnt; ++i) {
      const uint32_t at = step_at(Hmax, i);
      add_step(acc0, win, q0, at);
      if (U > 64u) add_step(acc1, win, q1, at);  // (wave-uniform: the round exists)
      if (U > 128u) add_step(acc2, win, q2, at);
      if (U > 192u) add_step(acc3, win, q3, at);
    }
    // every window's last 2 * Hmax words become its front: words [cnt, cnt + C) -> [0, C), C <= 128 - two a lane, read by
    // all before any is written (the windows of two assets do not overlap)
    wave_sync();
    for (uint32_t a = 0; a < A; ++a) {
      uint64_t* w = win + window_at(Hmax, a);
      const uint64_t lo = lane < C ? w[front_from(cnt, lane)] : 0ull;
      const uint64_t hi = lane + 64u < C ? w[front_from(cnt, lane + 64u)] : 0ull;
      wave_sync();
      if (lane < C) w[lane] = lo;
      if (lane + 64u < C) w[lane + 64u] = hi;
    }
    wave_sync();
  }

  bk_u32x4* rows = g.rows + static_cast<size_t>(m) * U * ROW_VECS;  // lane l owns rows l, l + 64, l + 128, l + 192
  if (q0.h) add_to_row(rows + static_cast<size_t>(lane) * ROW_VECS, acc0);
  if (q1.h) add_to_row(rows + static_cast<size_t>(lane + 64u) * ROW_VECS, acc1);
  if (q2.h) add_to_row(rows + static_cast<size_t>(lane + 128u) * ROW_VECS, acc2);
  if (q3.h) add_to_row(rows + static_cast<size_t>(lane + 192u) * ROW_VECS, acc3);
  for (uint32_t a = 0; a < A; ++a)
    for (uint32_t j = lane; j < C; j += 64u) carry[a * C + j] = win[window_at(Hmax, a) + carry_at(j)];
}

struct ClearArgs {
  ring::Masked markets;  // (one mask byte per market: M = 1, n_books = n_markets)
  uint32_t U;            // rows per market, S * A * A
  uint32_t carry_words;  // A * 2 * Hmax
  uint32_t carry_only;   // 1: only the carry (no span or lead reaches over a reset; the sums go on)
  bk_u32x4* rows;
  uint64_t* carry;
};

__global__ __launch_bounds__(64 * FOLD_WAVES) void k_clear(ClearArgs g) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t m = ring::masked_book(g.markets, FOLD_WAVES);
  if (m == ring::NO_BOOK) return;
  uint64_t* carry = g.carry + static_cast<size_t>(m) * g.carry_words;
  for (uint32_t j = lane; j < g.carry_words; j += 64u) carry[j] = 0ull;
  if (g.carry_only) return;
  bk_u32x4* rows = g.rows + static_cast<size_t>(m) * g.U * ROW_VECS;
  for (uint32_t v = lane; v < g.U * ROW_VECS; v += 64u) rows[v] = vec_of(0ull, 0ull);
}

}  // namespace cross
}  // namespace bkd
