// depth.hpp - bk_depth_*: per book L + 1 rows of sixteen u64 words, folded on the device from the LADDER of the level-2
// history ring - the 4 L words {bid_vol, bid_n, ask_vol, ask_n} per level that the series moments do not read: per level the
// moments of the resting volume and order count, the moments of the cumulative imbalance I_q and its response to the next
// move of the mid; in row L the header.
//
// The reference has no counterpart (its users fold Env::level_2_data's history on the host).  The table is the series
// moments' companion, not a table of its own: it has no cursor, it is folded, cleared and cut by the series' launches
// (bourse_amd.hip launch_series_fold / launch_series_clear) over the same span and mask.  The env keeps
// depth_rows[n_books][L + 1][16] and a carry depth_carry[n_books][L + 1]: I_q of the last folded step per level, then that
// step's window word.  What one (step, level) adds and which lane reads it are depth_fold.hpp's - DESIGN.md 2.27:
//   * one wave per book, FOLD_WAVES waves per block (the last block may hold fewer books);
//   * a lane owns a (step, level): with Lp the power of two at or above L a pass covers G = 64 / Lp consecutive steps, lane
//     g * Lp + q reads level q of step pass * G + g; lanes with q >= L, and groups behind the fold's last step, carry zeros;
//   * per pass a segmented inclusive scan of bid_vol - ask_vol (64-bit) over the Lp lanes by ds_bpermute gives I_q; I_q of
//     the step before comes from lane - Lp, for group 0 from the last group of the pass before, for the fold's first step
//     from the carry; the word of the step before comes from the ring, for the fold's first step from the carry;
//   * sixteen 64-bit sums per lane in registers, and the header's nine (only the lanes of level 0 are read in the end);
//   * behind the last pass the G groups are added by log2(G) xor-shuffles, the lanes of group 0 add to their book's rows -
//     the wave owns the book, no atomics - lane 0 adds the header, and L + 1 lanes write the carry: every read of the carry
//     stands before the fence, every write behind it.
// A record is 5 + 4 L words and its base only 4-byte aligned: the levels are read through const uint32_t*.
// k_clear clears the rows and carry of the masked books, or with carry_only just their carry (the resets' cut).
// Plain C++ and builtins, no LDS allocation, no scratch, no global atomics, vector loads and stores only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "book_device.hpp"
#include "depth_fold.hpp"
#include "hist_ring.hpp"

namespace bkd {
namespace depth {

constexpr int FOLD_WAVES = 4;              // waves (books) per block of k_fold / k_clear
constexpr uint32_t ROW_VECS = ROW_WORDS / 2u;  // 16-byte vectors per row

using ring::slot_of;
using ring::vec_hi;
using ring::vec_lo;
using ring::vec_of;
using ring::wave_sync;

struct FoldArgs {
  ring::Span ring;
  uint32_t L;
  bk_u32x4* rows;   // [n_books][L + 1][8]
  uint64_t* carry;  // [n_books][L + 1]
};

// lane `from`'s x (every lane of the wave takes part)
__device__ __forceinline__ uint64_t lane_get(uint64_t x, uint32_t from) {
  const int at = static_cast<int>((from & 63u) << 2);
  const uint32_t lo = static_cast<uint32_t>(__builtin_amdgcn_ds_bpermute(at, static_cast<int>(static_cast<uint32_t>(x))));
  const uint32_t hi = static_cast<uint32_t>(__builtin_amdgcn_ds_bpermute(at, static_cast<int>(static_cast<uint32_t>(x >> 32))));
  return mk64(lo, hi);
}

// row += r, eight vectors read, added and written
__device__ __forceinline__ void add_to(bk_u32x4* row, const Row& r) {
#pragma unroll
  for (uint32_t v = 0; v < ROW_VECS; ++v) {
    const bk_u32x4 x = row[v];
    row[v] = vec_of(vec_lo(x) + r.w[2 * v], vec_hi(x) + r.w[2 * v + 1]);
  }
}

__global__ __launch_bounds__(64 * FOLD_WAVES) void k_fold(FoldArgs g) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t b = rfl(blockIdx.x * FOLD_WAVES + (threadIdx.x >> 6));
  if (b >= g.ring.n_books) return;
  const uint32_t L = g.L, n = g.ring.n;
  const Lanes a = lanes_of(L);
  const uint32_t q = level_of(a, lane), grp = group_of(a, lane);
  const bool live = q < L;
  const uint64_t cap = g.ring.hist_cap;
  uint64_t* carry = g.carry + static_cast<size_t>(b) * (L + 1u);

  // the step in front of the fold: I_q of it in the lanes of every group (group 0 reads it), and its word
  int64_t tail = live ? static_cast<int64_t>(carry[q]) : 0;
  const uint64_t carry_word = carry[L];

  Row acc = cleared(), hdr = cleared();
  int64_t I = 0;
  uint64_t cur = 0ull;
  const uint32_t passes = passes_of(a, n);
  for (uint32_t pass = 0; pass < passes; ++pass) {
    const uint32_t i = step_of(a, pass, lane);  // step lo + i
    const bool has = i < n;
    uint32_t bid = 0u, ask = 0u, bv = 0u, bn = 0u, av = 0u, an = 0u;
    uint64_t prev = 0ull;
    if (has) {
      const uint64_t slot = slot_of(g.ring.slot0, i, cap);
      const uint32_t* rec = ring::record(g.ring, slot, b);
      bid = rec[1], ask = rec[2];
      if (live) {
        const uint32_t* lv = rec + level_at(q);
        bv = lv[0], bn = lv[1], av = lv[2], an = lv[3];
      }
      prev = carry_word;
      if (i >= 1u) {
        const uint32_t* rec1 = ring::record(g.ring, slot == 0u ? cap - 1u : slot - 1u, b);
        prev = word_of(rec1[1], rec1[2]);
      }
    }
    cur = has ? word_of(bid, ask) : 0ull;
    // I_q: the inclusive scan of bid_vol - ask_vol inside the group's Lp lanes
    I = static_cast<int64_t>(static_cast<uint64_t>(bv) - static_cast<uint64_t>(av));
    for (uint32_t off = 1u; off < a.Lp; off <<= 1) {
      const uint64_t below = lane_get(static_cast<uint64_t>(I), lane - off);
      if (q >= off) I += static_cast<int64_t>(below);
    }
    // I_q of the step before: the group below, or what the pass before (or the carry) left for group 0
    const uint64_t up = lane_get(static_cast<uint64_t>(I), lane - a.Lp);
    const int64_t J = grp == 0u ? tail : static_cast<int64_t>(up);
    tail = static_cast<int64_t>(lane_get(static_cast<uint64_t>(I), tail_lane(a, q)));
    if (has) {
      add_level(acc, bv, bn, av, an, I, J, cur, prev);
      add_header(hdr, bid, ask, cur, prev);
    }
  }

  // the carry behind the fold is the last step's: its group's lanes of the last pass
  const uint32_t from = last_lane(a, n, q);
  const uint64_t next_I = lane_get(static_cast<uint64_t>(I), from);
  const uint64_t next_word = lane_get(cur, from);

  // the G groups' sums -> group 0
  for (uint32_t off = a.Lp; off < 64u; off <<= 1) {
#pragma unroll
    for (uint32_t k = 0; k < ROW_WORDS; ++k) acc.w[k] += lane_get(acc.w[k], lane ^ off);
#pragma unroll
    for (uint32_t k = 0; k < HEADER_WORDS; ++k) hdr.w[k] += lane_get(hdr.w[k], lane ^ off);
  }

  bk_u32x4* rows = g.rows + static_cast<size_t>(b) * (L + 1u) * ROW_VECS;
  if (grp == 0u && live) add_to(rows + static_cast<size_t>(q) * ROW_VECS, acc);
  if (lane == 0u) add_to(rows + static_cast<size_t>(L) * ROW_VECS, hdr);  // (words 9 .. 15 stay 0)
  wave_sync();
  if (grp == 0u && live) carry[q] = next_I;
  if (lane == 0u) carry[L] = next_word;
}

struct ClearArgs {
  ring::Masked books;
  uint32_t L;
  uint32_t carry_only;  // 1: only the carry (no pair reaches over a reset; the sums go on)
  bk_u32x4* rows;
  uint64_t* carry;
};

__global__ __launch_bounds__(64 * FOLD_WAVES) void k_clear(ClearArgs g) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t b = ring::masked_book(g.books, FOLD_WAVES);
  if (b == ring::NO_BOOK) return;
  uint64_t* carry = g.carry + static_cast<size_t>(b) * (g.L + 1u);
  for (uint32_t v = lane; v < g.L + 1u; v += 64u) carry[v] = 0ull;
  if (g.carry_only) return;
  const uint32_t vecs = (g.L + 1u) * ROW_VECS;
  bk_u32x4* rows = g.rows + static_cast<size_t>(b) * vecs;
  for (uint32_t v = lane; v < vecs; v += 64u) rows[v] = vec_of(0ull, 0ull);
}

}  // namespace depth
}  // namespace bkd
