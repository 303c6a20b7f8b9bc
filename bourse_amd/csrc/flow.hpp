// flow.hpp - bk_flow_*: per book the sums of its TRADE RECORDS in record order - the base words (counts, volumes, notional)
// and K <= 64 lag rows in trade time: the autocorrelation of the trade sign, the response function, the variogram of the price.
//
// The reference has no counterpart (its users fold Env::get_trades on the host).  The env keeps table[n_books][8 + 6 K] u64
// words - four 16-byte vectors of base words, then three per lag row; the words and what a record and a pair add are
// flow_fold.hpp's - a carry flow_carry[n_books][K] of window words, entry j the record of index flow_seen - 1 - j, and one
// cursor per book, flow_seen[n_books]: the records below it are folded.  k_fold runs on the env's stream when bk_flow_fold,
// a step of the device ingress, a reset or a masked clear asks for it - DESIGN.md 2.26:
//   * one wave per book, FOLD_WAVES waves per block (the last block may hold fewer books), one window of WINDOW_WORDS
//     8-byte words in LDS per wave;
//   * the wave loads H_TRADES, H_TRADE_BASE (four header words) and its cursor; with nothing new - most of a launch behind
//     a step - it returns at once (a consuming fold first moves H_TRADE_BASE);
//   * the indices [seen, total) are lost_front unreadable ones, the readable run [lo, hi), lost_back unreadable ones
//     (flow::plan).  The window opens with the carry moved by lost_front invalid words; a gap of K or more invalidates all
//     of it and is never walked;
//   * per chunk of up to 64 records, one lane per RECORD loads the 32-byte record as two 16-byte vectors, appends its word to
//     the window and adds the record to its own base sums in registers;
//   * the wave then walks the chunk's records in order with one lane per LAG: the record's word is wave-uniform (a readlane
//     of the lane that loaded it), lane k - 1 reads the word k records in front of it from the window - neighbouring lanes
//     neighbouring words - and adds the pair to its own six accumulators (flow::add_pair): no cross-lane reduction;
//   * the window's last K words move to its front for the next chunk, and at the end - behind lost_back invalid words - to
//     the carry;
//   * the base sums take ONE reduction at the end and lane 0 adds them to the four vectors it reads; lane k - 1 adds its
//     accumulators to its own 48-byte row;
//   * the cursor moves to H_TRADES behind a wave fence; with `consume` the wave ends by H_TRADE_BASE = H_TRADES, as
//     bk_clear_trades does (the host passes it to the LAST fold of a step only).
// k_clear moves the masked books' cursors to their H_TRADES and invalidates their carry - the resets' cut - and unless
// carry_only zeroes their rows as well.  Plain C++, no scratch, no atomics, vector loads and stores only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "book_device.hpp"
#include "flow_fold.hpp"
#include "hist_ring.hpp"  // ring::Masked, masked_book, wave_sync, vec_of

namespace bkd {
namespace flow {

constexpr int FOLD_WAVES = 4;        // waves (books) per block of k_fold / k_clear
constexpr uint32_t BASE_VECS = 4u;   // 16-byte vectors of base words
constexpr uint32_t LAG_VECS = 3u;    // 16-byte vectors per lag row

using ring::vec_hi;
using ring::vec_lo;
using ring::vec_of;
using ring::wave_sync;

__host__ __device__ inline size_t book_vecs(uint32_t K) { return BASE_VECS + static_cast<size_t>(LAG_VECS) * K; }

struct FoldArgs {
  uint32_t* state;  // [n_books][stride]
  uint32_t stride, n_books;
  const bk_u32x4* trades;  // [n_books][trade_cap][2]
  uint32_t trade_cap;
  uint32_t K;                // lags, 1 .. MAX_LAGS
  bk_u32x4* table;           // [n_books][4 + 3 K]
  uint64_t* carry;           // [n_books][K]
  unsigned long long* seen;  // [n_books]
  uint32_t consume;
};

__global__ __launch_bounds__(64 * FOLD_WAVES) void k_fold(FoldArgs g) {
  __shared__ uint64_t windows[FOLD_WAVES][WINDOW_WORDS];
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = rfl(threadIdx.x >> 6);
  const uint32_t b = rfl(blockIdx.x * FOLD_WAVES + wave);
  if (b >= g.n_books) return;  // (no block-wide barrier below: a wave is on its own)
  uint32_t* h = g.state + static_cast<size_t>(b) * g.stride;
  const uint64_t total = mk64(rfl(h[H_TRADES_LO]), rfl(h[H_TRADES_HI]));
  const uint64_t base = mk64(rfl(h[H_TRADE_BASE_LO]), rfl(h[H_TRADE_BASE_HI]));
  const unsigned long long seen_raw = g.seen[b];
  const uint64_t seen = mk64(rfl(static_cast<uint32_t>(seen_raw)), rfl(static_cast<uint32_t>(seen_raw >> 32)));
  // Nothing new.  (seen > total - a cursor ahead of the book - cannot be: whatever puts H_TRADES back, the resets and a
  // checkpoint load, ends with k_clear, which moves the cursor to the new count, and bk_load_book is refused.  An entry
  // that rewinds a book without that cut would leave the table waiting here, cursor unmoved, until the count passes it.)
  if (seen >= total) {
    if (lane == 0 && g.consume && base != total) {
      h[H_TRADE_BASE_LO] = static_cast<uint32_t>(total);
      h[H_TRADE_BASE_HI] = static_cast<uint32_t>(total >> 32);
    }
    return;
  }

  const uint32_t K = g.K;
  const Plan p = plan(seen, total, base, g.trade_cap);
  uint64_t* win = windows[wave];
  uint64_t* carry = g.carry + static_cast<size_t>(b) * K;
  if (lane < K) {
    const uint32_t src = carry_src(K, p.lost_front, lane);
    win[carry_at(K, lane)] = src == NO_ENTRY ? 0ull : carry[src];
  }
  wave_sync();

  Base mine_sum{};  // this lane's records
  LagRow acc{};     // this lane's lag
  const bk_u32x4* recs = g.trades + static_cast<size_t>(b) * g.trade_cap * 2;
  for (uint64_t c = p.lo; c < p.hi; c += CHUNK) {
    const uint32_t cnt = p.hi - c < CHUNK ? static_cast<uint32_t>(p.hi - c) : CHUNK;  // this chunk's records: wave-uniform
    uint64_t mine = 0;
    if (lane < cnt) {  // index c + lane in [lo, hi): base <= it and it - base < trade_cap
      const bk_u32x4* rec = recs + (c + lane - base) * 2;
      const bk_u32x4 r0 = rec[0], r1 = rec[1];  // {t_lo, t_hi, price, vol} {active, passive, side_is_bid, pad}
      mine = word_of(r0.z, r1.z);
      add_record(mine_sum, r0.z, r0.w, r1.z);
      win[rec_at(K, lane)] = mine;
    }
    wave_sync();
    for (uint32_t i = 0; i < cnt; ++i) {
      const uint64_t cur = mk64(rdl(static_cast<uint32_t>(mine), i), rdl(static_cast<uint32_t>(mine >> 32), i));
      if (lane < K) add_pair(acc, cur, win[rec_at(K, i) - (lane + 1u)]);
    }
    // the window's last K words become its front: words [cnt, cnt + K) -> [0, K) (read by all before any is written)
    wave_sync();
    const uint64_t front = lane < K ? win[cnt + lane] : 0ull;
    wave_sync();
    if (lane < K) win[lane] = front;
    wave_sync();
  }

  // the base words: one reduction, lane 0 adds to the four vectors
  Base sum;
  sum.w[N_TRADES] = wave_sum_u32(static_cast<uint32_t>(mine_sum.w[N_TRADES]));  // (a lane's counts are below 2^32: trade_cap is)
  sum.w[N_BUY] = wave_sum_u32(static_cast<uint32_t>(mine_sum.w[N_BUY]));
  sum.w[SUM_VOL] = wave_sum_u64(mine_sum.w[SUM_VOL]);
  sum.w[BUY_VOL] = wave_sum_u64(mine_sum.w[BUY_VOL]);
  sum.w[SUM_VOL_SQ] = wave_sum_u64(mine_sum.w[SUM_VOL_SQ]);
  sum.w[NOTIONAL] = wave_sum_u64(mine_sum.w[NOTIONAL]);
  sum.w[MAX_VOL] = wave_umax(static_cast<uint32_t>(mine_sum.w[MAX_VOL]));
  sum.w[N_LOST] = p.lost_front + p.lost_back;
  bk_u32x4* tab = g.table + static_cast<size_t>(b) * book_vecs(K);
  if (lane == 0) {
    Base r;
#pragma unroll
    for (uint32_t v = 0; v < BASE_VECS; ++v) {
      const bk_u32x4 x = tab[v];
      r.w[2 * v] = vec_lo(x), r.w[2 * v + 1] = vec_hi(x);
    }
    merge(r, sum);
#pragma unroll
    for (uint32_t v = 0; v < BASE_VECS; ++v) tab[v] = vec_of(r.w[2 * v], r.w[2 * v + 1]);
  }
  if (lane < K) {  // lane k - 1 owns row k - 1
    bk_u32x4* row = tab + BASE_VECS + static_cast<size_t>(lane) * LAG_VECS;
    LagRow r;
#pragma unroll
    for (uint32_t v = 0; v < LAG_VECS; ++v) {
      const bk_u32x4 x = row[v];
      r.w[2 * v] = vec_lo(x), r.w[2 * v + 1] = vec_hi(x);
    }
    merge(r, acc);
#pragma unroll
    for (uint32_t v = 0; v < LAG_VECS; ++v) row[v] = vec_of(r.w[2 * v], r.w[2 * v + 1]);
    const uint32_t src = carry_src(K, p.lost_back, lane);  // the window's front holds the carry in front of that gap
    carry[lane] = src == NO_ENTRY ? 0ull : win[carry_at(K, src)];
  }
  wave_sync();  // rows and carry stand before the cursor says so
  if (lane == 0) {
    g.seen[b] = total;
    if (g.consume) {
      h[H_TRADE_BASE_LO] = static_cast<uint32_t>(total);
      h[H_TRADE_BASE_HI] = static_cast<uint32_t>(total >> 32);
    }
  }
}

struct ClearArgs {
  ring::Masked books;
  const uint32_t* state;
  uint32_t stride;
  uint32_t K;
  uint32_t carry_only;  // 1: only carry and cursor (no pair reaches over a reset; the sums go on)
  bk_u32x4* table;
  uint64_t* carry;
  unsigned long long* seen;
};

__global__ __launch_bounds__(64 * FOLD_WAVES) void k_clear(ClearArgs g) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t b = ring::masked_book(g.books, FOLD_WAVES);
  if (b == ring::NO_BOOK) return;
  if (lane < g.K) g.carry[static_cast<size_t>(b) * g.K + lane] = 0ull;
  if (lane == 0) {
    const uint32_t* h = g.state + static_cast<size_t>(b) * g.stride;
    g.seen[b] = mk64(h[H_TRADES_LO], h[H_TRADES_HI]);
  }
  if (g.carry_only) return;
  bk_u32x4* tab = g.table + static_cast<size_t>(b) * book_vecs(g.K);
  const uint32_t n = static_cast<uint32_t>(book_vecs(g.K));
  for (uint32_t v = lane; v < n; v += 64u) tab[v] = vec_of(0ull, 0ull);
}

}  // namespace flow
}  // namespace bkd
