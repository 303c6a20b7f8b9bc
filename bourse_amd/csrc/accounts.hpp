// accounts.hpp - bk_accounts_*: per-trader position, cash, volume and fill count of a DEVICE-INGRESS env, kept on the device.
//
// The reference has no counterpart (its users join Env::get_trades with Env::get_orders on the host).  The env
// keeps acct[n_books][n_traders] rows of 32 B {position, cash, volume, fills} (bk_account) and one cursor per book,
// acct_seen[n_books]: the number of the book's trade records already folded.  k_fold runs on the env's stream behind every
// step's event kernel - DESIGN.md 2.16:
//   * one wave per book, FOLD_WAVES waves per block (the last block may hold fewer books);
//   * the wave loads H_TRADES, H_TRADE_BASE (four header words) and its cursor; with nothing new it returns - most of a
//     launch takes this path, so it holds those loads and nothing else;
//   * otherwise it walks the new records 64 at a time, one lane per record: the 32-byte record as two 16-byte vectors, the
//     traders of its two orders from dorders[book][id][0].y, the deltas of buyer and seller from account_fold.hpp;
//   * many lanes share a trader, and one wave owns the book's rows, so conflicts are resolved inside the wave with no
//     atomic and no cross-lane reduction: trader x belongs to lane x % 64; the chunk's records are walked in order with
//     their words broadcast from their lanes (readlane), and the owning lane adds the party's delta in its registers; after
//     the walk the lanes that hold a trader read, add and write their rows at once - the rows are distinct, 32 B each, two
//     16-byte vectors.  Two traders of one chunk on one lane (only with n_traders > 64) take a further pass over the
//     records left.  Sums are integers modulo 2^64: the order chosen cannot show.  (The first form, a butterfly of wave
//     shuffles per distinct trader of the chunk - 43 ds_bpermute each - added 371 us to a step of 65 536 books x 26
//     trades where this one adds 112, and 380 against 71 with 512 traders per book: DESIGN.md 2.16);
//   * a record that cannot be folded - dropped beyond trade_capacity (or consumed by bk_clear_trades before the fold saw it),
//     or with an order id >= max_orders - sets FLAG_ACCOUNTS_INEXACT in the book's H_FLAGS and is stepped over;
//   * the cursor moves to H_TRADES; with consume_trades the wave ends by H_TRADE_BASE = H_TRADES, as bk_clear_trades does.
// k_clear zeroes the rows of the masked books and moves their cursors to the books' H_TRADES (bk_accounts_clear*, and the
// tail of bk_ingress_reset_books*).  Plain C++, no LDS, no scratch, vector loads and stores only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "account_fold.hpp"
#include "book_device.hpp"

namespace bkd {
namespace accounts {

constexpr int FOLD_WAVES = 4;                      // waves (books) per block of k_fold / k_clear
constexpr uint32_t FLAG_ACCOUNTS_INEXACT = 512u;   // BK_FLAG_ACCOUNTS_INEXACT
constexpr uint32_t MAX_TRADERS = 65536u;
constexpr uint32_t NO_TRADER = 0xFFFFFFFFu;

struct FoldArgs {
  uint32_t* state;  // [n_books][stride]
  uint32_t stride, n_books;
  const bk_u32x4* trades;  // [n_books][trade_cap][2]
  uint32_t trade_cap;
  const uint4* dorders;  // [n_books][max_orders][2]
  uint32_t max_orders;
  bk_u32x4* acct;  // [n_books][n_traders][2]
  uint32_t n_traders;
  unsigned long long* seen;  // [n_books]
  uint32_t consume;
};

// row += d: one 32-byte read-modify-write by the calling lane
__device__ __forceinline__ void add_row(bk_u32x4* row, const Delta& d) {
  const bk_u32x4 a = row[0], b = row[1];
  const uint64_t position = mk64(a.x, a.y) + d.position, cash = mk64(a.z, a.w) + d.cash;
  const uint64_t volume = mk64(b.x, b.y) + d.volume, fills = mk64(b.z, b.w) + d.fills;
  bk_u32x4 o0, o1;
  o0.x = static_cast<uint32_t>(position), o0.y = static_cast<uint32_t>(position >> 32);
  o0.z = static_cast<uint32_t>(cash), o0.w = static_cast<uint32_t>(cash >> 32);
  o1.x = static_cast<uint32_t>(volume), o1.y = static_cast<uint32_t>(volume >> 32);
  o1.z = static_cast<uint32_t>(fills), o1.w = static_cast<uint32_t>(fills >> 32);
  row[0] = o0;
  row[1] = o1;
}

__global__ __launch_bounds__(64 * FOLD_WAVES) void k_fold(FoldArgs g) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t b = rfl(blockIdx.x * FOLD_WAVES + (threadIdx.x >> 6));
  if (b >= g.n_books) return;
  uint32_t* h = g.state + static_cast<size_t>(b) * g.stride;
  const uint64_t total = mk64(rfl(h[H_TRADES_LO]), rfl(h[H_TRADES_HI]));
  const uint64_t base = mk64(rfl(h[H_TRADE_BASE_LO]), rfl(h[H_TRADE_BASE_HI]));
  const unsigned long long seen_raw = g.seen[b];
  uint64_t seen = mk64(rfl(static_cast<uint32_t>(seen_raw)), rfl(static_cast<uint32_t>(seen_raw >> 32)));
  if (seen == total && (!g.consume || base == total)) return;

  bool lost = false;  // this lane met a record it could not fold
  if (seen > total) {  // (a cursor ahead of the book: nothing rewinds a book without k_clear, so never - but never silent)
    lost = true;
    seen = total;
  }
  bk_u32x4* rows = g.acct + static_cast<size_t>(b) * g.n_traders * 2;
  for (uint64_t c = seen; c < total; c += 64u) {
    const uint64_t i = c + lane;
    const uint64_t pos = i - base;  // (i < base wraps far beyond trade_cap)
    const bool valid = i < total;
    bool ok = valid && i >= base && pos < g.trade_cap;
    uint32_t price = 0, vol = 0, act = 0, pas = 0, side_is_bid = 0;
    if (ok) {
      const bk_u32x4* rec = g.trades + (static_cast<size_t>(b) * g.trade_cap + pos) * 2;
      const bk_u32x4 r0 = rec[0], r1 = rec[1];  // {t_lo, t_hi, price, vol} {active, passive, side_is_bid, pad}
      price = r0.z, vol = r0.w, act = r1.x, pas = r1.y, side_is_bid = r1.z;
      ok = act < g.max_orders && pas < g.max_orders;
    }
    uint32_t t_act = 0xFFFFFFFFu, t_pas = 0xFFFFFFFFu;
    if (ok) {  // {start_vol, trader, price, bid}
      const uint4* d = g.dorders + static_cast<size_t>(b) * g.max_orders * 2;
      t_act = d[static_cast<size_t>(act) * 2].y;
      t_pas = d[static_cast<size_t>(pas) * 2].y;
    }
    lost |= valid && !ok;
    const Parties p = parties(side_is_bid, t_act, t_pas);
    const bool pend_b = ok && p.buyer < g.n_traders, pend_s = ok && p.seller < g.n_traders;
    // Conflicts are resolved inside the wave.  Trader x belongs to lane x % 64 for the whole launch.  A pass walks the
    // records that still have a pending party, in order, with the record's words broadcast from its lane (readlane); the
    // owning lane takes the party if it holds no trader yet in this pass, or this one - then it adds the delta in its
    // registers - and leaves it pending otherwise (two traders of the chunk on one lane: only with n_traders > 64).  After
    // the pass the lanes that hold a trader read, add and write their rows at once: the rows are distinct.  A pass always
    // takes its first party, so the passes end; a trader's parties are all taken in the same pass.
    unsigned long long todo_b = __ballot(pend_b), todo_s = __ballot(pend_s);
    while ((todo_b | todo_s) != 0ull) {
      uint32_t own = NO_TRADER;
      Delta mine{0, 0, 0, 0};
      unsigned long long walk = todo_b | todo_s;
      while (walk != 0ull) {
        const int r = __builtin_ctzll(walk);
        walk &= walk - 1ull;
        const uint32_t r_price = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(price), r));
        const uint32_t r_vol = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(vol), r));
        if ((todo_b >> r) & 1ull) {
          const uint32_t x = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(p.buyer), r));
          const bool take = lane == (x & 63u) && (own == NO_TRADER || own == x);
          if (take) {
            own = x;
            add(mine, buyer_delta(r_price, r_vol));
          }
          if (__ballot(take) != 0ull) todo_b &= ~(1ull << r);
        }
        if ((todo_s >> r) & 1ull) {
          const uint32_t x = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(p.seller), r));
          const bool take = lane == (x & 63u) && (own == NO_TRADER || own == x);
          if (take) {
            own = x;
            add(mine, seller_delta(r_price, r_vol));
          }
          if (__ballot(take) != 0ull) todo_s &= ~(1ull << r);
        }
      }
      if (own != NO_TRADER) add_row(rows + static_cast<size_t>(own) * 2, mine);
    }
  }
  const bool any_lost = __ballot(lost) != 0ull;
  if (lane == 0) {
    if (any_lost) h[H_FLAGS] |= FLAG_ACCOUNTS_INEXACT;
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
  bk_u32x4* acct;
  uint32_t n_traders;
  unsigned long long* seen;
};

__global__ __launch_bounds__(64 * FOLD_WAVES) void k_clear(ClearArgs g) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t b = rfl(blockIdx.x * FOLD_WAVES + (threadIdx.x >> 6));
  if (b >= g.n_books) return;
  if (g.mask && rfl(static_cast<uint32_t>(g.mask[b / g.M])) == 0u) return;
  bk_u32x4* rows = g.acct + static_cast<size_t>(b) * g.n_traders * 2;
  const uint32_t n = g.n_traders * 2u;
  const bk_u32x4 zero = {0u, 0u, 0u, 0u};
  for (uint32_t v = lane; v < n; v += 64u) rows[v] = zero;
  if (lane == 0) {
    const uint32_t* h = g.state + static_cast<size_t>(b) * g.stride;
    g.seen[b] = mk64(h[H_TRADES_LO], h[H_TRADES_HI]);
  }
}

}  // namespace accounts
}  // namespace bkd
