// trade_bars.hpp - bk_trade_bars_*: a ring of per-step OHLCV bars for every book of a DEVICE-INGRESS env, kept on the device.
//
// The reference has no counterpart (its users fold Env::get_trades on the host).  The env keeps bars[n_books][window] rows of
// 48 B, three 16-byte vectors {open, high, low, close} {buy_vol, sell_vol} {notional, n_buy, n_sell} (bk_trade_bar), and one
// cursor per book, bars_seen[n_books]: the number of the book's trade records already folded.  k_fold runs on the env's
// stream behind every step's event kernel, in front of accounts::k_fold where both are on - DESIGN.md 2.21:
//   * one wave per book, FOLD_WAVES waves per block (the last block may hold fewer books);
//   * the wave loads H_TRADES, H_TRADE_BASE (four header words), its cursor and the first vector of the previous step's
//     slot, whose fourth word is the close a step without a trade carries;
//   * with nothing new - most of a launch - it writes the carried bar, three 16-byte stores, and returns: no loop;
//   * otherwise it walks the new records 64 at a time, one lane per record, the 32-byte record as two 16-byte vectors.  A
//     bar is a pure reduction across the wave: high / low by wave_umax / wave_umin (a lane without a record contributes
//     the identity), open / close by a readlane of the first / last lane that holds a record, the counts from ballots, and
//     the 64-bit sums from wrapping u32 wave sums of 16-bit limbs (64 x 65 535 fits a u32) recombined modulo 2^64.  The
//     chunk's bar extends the running one in registers (trade_bar_fold.hpp), and lane 0 writes the row once;
//   * a record that cannot be read - dropped beyond trade_capacity - is stepped over: the bar is that of the records read,
//     and the book carries FLAG_TRADE_OVERFLOW from the step's kernel already (no flag bit of the bars' own);
//   * the cursor moves to H_TRADES; with `consume` the wave ends by H_TRADE_BASE = H_TRADES, as bk_clear_trades does (the
//     host passes it to the LAST fold of a step only, so no fold hides a record from the other).
// k_clear zeroes the rows of the masked books and moves their cursors to the books' H_TRADES (bk_trade_bars_enable,
// bk_trade_bars_clear*, and the tail of bk_ingress_reset_books*).  Plain C++, no LDS, no scratch, vector loads and stores only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "book_device.hpp"
#include "trade_bar_fold.hpp"

namespace bkd {
namespace trade_bars {

constexpr int FOLD_WAVES = 4;                  // waves (books) per block of k_fold / k_clear
constexpr uint32_t MAX_WINDOW = 1024u;
constexpr uint32_t ROW_VECS = 3u;              // 16-byte vectors per row

struct FoldArgs {
  uint32_t* state;  // [n_books][stride]
  uint32_t stride, n_books;
  const bk_u32x4* trades;  // [n_books][trade_cap][2]
  uint32_t trade_cap;
  bk_u32x4* bars;  // [n_books][window][3]
  uint32_t window;
  uint32_t slot, prev_slot;  // this step's slot k % window, and (k - 1) % window
  unsigned long long* seen;  // [n_books]
  uint32_t consume;
};

// (wave_sum_u32 / wave_sum_u64, the wave's exact and modulo-2^64 sums, stand beside wave_add in book_device.hpp)
// one 48-byte row by the calling lane
__device__ __forceinline__ void store_bar(bk_u32x4* row, const Bar& r) {
  uint32_t w[12];
  words(r, w);
  bk_u32x4 v0, v1, v2;
  v0.x = w[0], v0.y = w[1], v0.z = w[2], v0.w = w[3];
  v1.x = w[4], v1.y = w[5], v1.z = w[6], v1.w = w[7];
  v2.x = w[8], v2.y = w[9], v2.z = w[10], v2.w = w[11];
  row[0] = v0;
  row[1] = v1;
  row[2] = v2;
}

__global__ __launch_bounds__(64 * FOLD_WAVES) void k_fold(FoldArgs g) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t b = rfl(blockIdx.x * FOLD_WAVES + (threadIdx.x >> 6));
  if (b >= g.n_books) return;
  uint32_t* h = g.state + static_cast<size_t>(b) * g.stride;
  bk_u32x4* rows = g.bars + static_cast<size_t>(b) * g.window * ROW_VECS;
  const bk_u32x4 prev = rows[static_cast<size_t>(g.prev_slot) * ROW_VECS];  // read before the write: window 1 reuses the slot
  const uint64_t total = mk64(rfl(h[H_TRADES_LO]), rfl(h[H_TRADES_HI]));
  const uint64_t base = mk64(rfl(h[H_TRADE_BASE_LO]), rfl(h[H_TRADE_BASE_HI]));
  const unsigned long long seen_raw = g.seen[b];
  uint64_t seen = mk64(rfl(static_cast<uint32_t>(seen_raw)), rfl(static_cast<uint32_t>(seen_raw >> 32)));
  const uint32_t prev_close = rfl(prev.w);
  bk_u32x4* row = rows + static_cast<size_t>(g.slot) * ROW_VECS;
  if (seen == total) {  // a step without a trade: the slot is being reused, so it is written all the same
    if (lane == 0) {
      store_bar(row, idle(prev_close));
      if (g.consume && base != total) {
        h[H_TRADE_BASE_LO] = static_cast<uint32_t>(total);
        h[H_TRADE_BASE_HI] = static_cast<uint32_t>(total >> 32);
      }
    }
    return;
  }

  if (seen > total) seen = total;  // (a cursor ahead of the book: nothing rewinds a book without k_clear, so never)
  Bar run = idle(prev_close);
  bool have = false;  // `run` covers a record
  for (uint64_t c = seen; c < total; c += 64u) {
    const uint64_t i = c + lane;
    const uint64_t pos = i - base;  // (i < base wraps far beyond trade_cap)
    const bool ok = i < total && i >= base && pos < g.trade_cap;
    uint32_t price = 0, vol = 0, side_is_bid = 0;
    if (ok) {
      const bk_u32x4* rec = g.trades + (static_cast<size_t>(b) * g.trade_cap + pos) * 2;
      const bk_u32x4 r0 = rec[0], r1 = rec[1];  // {t_lo, t_hi, price, vol} {active, passive, side_is_bid, pad}
      price = r0.z, vol = r0.w, side_is_bid = r1.z;
    }
    const unsigned long long have_rec = __ballot(ok);
    if (have_rec == 0ull) continue;  // (wave-uniform: the reductions below run with every lane)
    const bool buy = ok && is_buy(side_is_bid);
    const unsigned long long buys = __ballot(buy);
    Bar ch;
    ch.open = rdl(price, static_cast<uint32_t>(__builtin_ctzll(have_rec)));
    ch.close = rdl(price, 63u - static_cast<uint32_t>(__builtin_clzll(have_rec)));
    ch.high = wave_umax(ok ? price : 0u);
    ch.low = wave_umin(ok ? price : 0xFFFFFFFFu);
    ch.buy_vol = wave_sum_u32(buy ? vol : 0u);
    ch.sell_vol = wave_sum_u32(ok && !buy ? vol : 0u);
    ch.notional = wave_sum_u64(ok ? notional(price, vol) : 0ull);
    ch.n_buy = static_cast<uint32_t>(__builtin_popcountll(buys));
    ch.n_sell = static_cast<uint32_t>(__builtin_popcountll(have_rec & ~buys));
    run = have ? extend(run, ch) : ch;
    have = true;
  }
  if (lane == 0) {
    store_bar(row, run);  // (no record could be read: the carried bar)
    g.seen[b] = total;
    if (g.consume) {
      h[H_TRADE_BASE_LO] = static_cast<uint32_t>(total);
      h[H_TRADE_BASE_HI] = static_cast<uint32_t>(total >> 32);
    }
  }
}

struct ClearArgs {
  const uint8_t* mask;  // [n_books / M] device memory; nullptr: every book
  uint32_t M;           // books per mask byte (bk_ingress_reset_books*' units are markets)
  const uint32_t* state;
  uint32_t stride, n_books;
  bk_u32x4* bars;
  uint32_t window;
  unsigned long long* seen;
};

__global__ __launch_bounds__(64 * FOLD_WAVES) void k_clear(ClearArgs g) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t b = rfl(blockIdx.x * FOLD_WAVES + (threadIdx.x >> 6));
  if (b >= g.n_books) return;
  if (g.mask && rfl(static_cast<uint32_t>(g.mask[b / g.M])) == 0u) return;
  bk_u32x4* rows = g.bars + static_cast<size_t>(b) * g.window * ROW_VECS;
  const uint32_t n = g.window * ROW_VECS;
  const bk_u32x4 zero = {0u, 0u, 0u, 0u};
  for (uint32_t v = lane; v < n; v += 64u) rows[v] = zero;
  if (lane == 0) {
    const uint32_t* h = g.state + static_cast<size_t>(b) * g.stride;
    g.seen[b] = mk64(h[H_TRADES_LO], h[H_TRADES_HI]);
  }
}

}  // namespace trade_bars
}  // namespace bkd
