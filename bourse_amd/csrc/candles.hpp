// candles.hpp - bk_candles_*: per book a ring of the last N bars of W steps each, sixteen u64 words a bar, folded on the
// device from words 0 .. 2 of the level-2 history ring's records: OHLC of twice the mid, the sums behind the time-weighted
// mid and spread, the traded volume and the realised variance of every bar - the PATH the series moments collapse.
//
// The reference has no counterpart (its users fold Env::level_2_data's history on the host).  The table is the series
// moments' companion, not a table of its own: it has no cursor, it is folded, cleared and cut by the series' launches
// (bourse_amd.hip launch_series_fold / launch_series_clear) over the same span and mask.  The env keeps
// candle_rows[n_books][N][16] and a carry candle_carry[n_books]: the word of the last folded step.  Bars are aligned to the
// env's absolute step count, the same for every book: step s is of bar s / W in slot (s / W) % N.  What one step adds, how
// two parts of a bar merge, when a slot is continued and which lanes form a bar are candle_fold.hpp's - DESIGN.md 2.28:
//   * one wave per book, FOLD_WAVES waves per block (the last block may hold fewer books), 64 steps a pass, a lane a step;
//   * a lane loads words 0 .. 2 of its record and takes the word of the step before from the lane below - lane 0 from the
//     last lane of the pass before, for the fold's first step from the carry - and forms its step's part;
//   * the lanes of one bar are a contiguous range of any length (W need not be a power of two, the fold need not start a
//     bar): a head-flagged segmented inclusive scan over ds_bpermute, six rounds, leaves the bar's part in its tail lane;
//   * the tail lane reads the slot's row, continues or restarts it, and writes it back - unless the bar is one the fold
//     skips, its slot being a later bar's of the same fold: the bars written in one pass then stand in different slots;
//   * a bar that spans passes is continued from its row: the wave's fence stands between a pass's stores and the next's loads;
//   * the carry is read in front of the first pass and written behind the last.
// The host passes where the fold's first step stands (seen / W, seen % W, (seen / W) % N) and the bar of its last step: no
// lane divides 64-bit words.
// k_clear clears the rows and carry of the masked books, or with carry_only just their carry (the resets' cut).
// Plain C++ and builtins, no LDS allocation, no scratch, no global atomics, vector loads and stores only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "book_device.hpp"
#include "candle_fold.hpp"
#include "hist_ring.hpp"

namespace bkd {
namespace candles {

constexpr int FOLD_WAVES = 4;                  // waves (books) per block of k_fold / k_clear
constexpr uint32_t ROW_VECS = ROW_WORDS / 2u;  // 16-byte vectors per row

using ring::slot_of;
using ring::vec_hi;
using ring::vec_lo;
using ring::vec_of;
using ring::wave_sync;

struct FoldArgs {
  ring::Span ring;
  uint32_t W, N;      // steps a bar, bars a book
  uint64_t bar;       // of the fold's first step: seen / W
  uint32_t phase;     // seen % W
  uint32_t slot;      // (seen / W) % N
  uint64_t last_bar;  // of the fold's last step: (seen + n - 1) / W
  bk_u32x4* rows;     // [n_books][N][8]
  uint64_t* carry;    // [n_books]
};

// lane `from`'s x (every lane of the wave takes part)
__device__ __forceinline__ uint64_t lane_get(uint64_t x, uint32_t from) {
  const int at = static_cast<int>((from & 63u) << 2);
  const uint32_t lo = static_cast<uint32_t>(__builtin_amdgcn_ds_bpermute(at, static_cast<int>(static_cast<uint32_t>(x))));
  const uint32_t hi = static_cast<uint32_t>(__builtin_amdgcn_ds_bpermute(at, static_cast<int>(static_cast<uint32_t>(x >> 32))));
  return mk64(lo, hi);
}

__device__ __forceinline__ Part load_row(const bk_u32x4* row) {
  Part r;
#pragma unroll
  for (uint32_t v = 0; v < ROW_VECS; ++v) {
    const bk_u32x4 x = row[v];
    r.w[2 * v] = vec_lo(x), r.w[2 * v + 1] = vec_hi(x);
  }
  return r;
}

__device__ __forceinline__ void store_row(bk_u32x4* row, const Part& r) {
#pragma unroll
  for (uint32_t v = 0; v < ROW_VECS; ++v) row[v] = vec_of(r.w[2 * v], r.w[2 * v + 1]);
}

__global__ __launch_bounds__(64 * FOLD_WAVES) void k_fold(FoldArgs g) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t b = rfl(blockIdx.x * FOLD_WAVES + (threadIdx.x >> 6));
  if (b >= g.ring.n_books) return;
  const uint32_t W = g.W, N = g.N, n = g.ring.n;
  const uint64_t cap = g.ring.hist_cap;
  bk_u32x4* rows = g.rows + static_cast<size_t>(b) * N * ROW_VECS;

  uint64_t tail = g.carry[b];  // the word of the step in front of the pass
  uint64_t cur = 0ull;
  Pass at{g.bar, g.phase, g.slot};
  const uint32_t passes = (n + 63u) >> 6;
  for (uint32_t pass = 0; pass < passes; ++pass) {
    const uint32_t i = pass * 64u + lane;  // step lo + i
    const bool has = i < n;
    const Seg s = seg_of(at, lane, W, N);
    const uint64_t bar = at.bar + s.rel;
    uint32_t tv = 0u, bid = 0u, ask = 0u;
    if (has) {
      const uint32_t* rec = ring::record(g.ring, slot_of(g.ring.slot0, i, cap), b);
      tv = rec[0], bid = rec[1], ask = rec[2];
    }
    cur = has ? word_of(bid, ask) : 0ull;
    const uint64_t below = lane_get(cur, lane - 1u);
    const uint64_t prev = lane == 0u ? tail : below;
    tail = lane_get(cur, 63u);

    // the bar's part in its tail lane: lanes without a step are segments of their own and hold the identity
    Part p = has ? term(bar_start(bar, W) + s.phase, tv, bid, ask, cur, prev) : cleared();
    bool head = s.head || !has;
    for (uint32_t off = 1u; off < 64u; off <<= 1) {
      Part q;
#pragma unroll
      for (uint32_t k = 0; k < ROW_WORDS; ++k) q.w[k] = lane_get(p.w[k], lane - off);
      const bool q_head = __builtin_amdgcn_ds_bpermute(static_cast<int>(((lane - off) & 63u) << 2), head ? 1 : 0) != 0;
      scan_round(p, head, q, q_head, lane, off);
    }

    if (has && tail_of(s, lane, i, n, W) && !skipped(bar, g.last_bar, N)) {
      bk_u32x4* row = rows + static_cast<size_t>(s.slot) * ROW_VECS;
      store_row(row, merged_row(load_row(row), p, bar, W));
    }
    wave_sync();  // the next pass may continue this pass's last bar from another lane
    at = next_pass(at, W, N);
  }

  // the carry behind the fold is the word of its last step (read above, in front of the first pass)
  const uint64_t next_word = lane_get(cur, (n - 1u) & 63u);
  if (lane == 0u) g.carry[b] = next_word;
}

struct ClearArgs {
  ring::Masked books;
  uint32_t N;
  uint32_t carry_only;  // 1: only the carry (no return reaches over a reset; the bars go on)
  bk_u32x4* rows;
  uint64_t* carry;
};

__global__ __launch_bounds__(64 * FOLD_WAVES) void k_clear(ClearArgs g) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t b = ring::masked_book(g.books, FOLD_WAVES);
  if (b == ring::NO_BOOK) return;
  if (lane == 0u) g.carry[b] = 0ull;
  if (g.carry_only) return;
  const uint32_t vecs = g.N * ROW_VECS;  // <= 2^19
  bk_u32x4* rows = g.rows + static_cast<size_t>(b) * vecs;
  for (uint32_t v = lane; v < vecs; v += 64u) rows[v] = vec_of(0ull, 0ull);
}

}  // namespace candles
}  // namespace bkd
