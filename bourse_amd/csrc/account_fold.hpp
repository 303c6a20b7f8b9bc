// account_fold.hpp - what ONE trade record adds to the accounts of its two parties (bk_accounts_enable).
//
// Compiled by the device fold (accounts.hpp) and by a CPU test (tests/cpp/account_fold_test.cpp): no HIP type, no
// intrinsic.  A record is {price, vol, side_is_bid} with the traders of its active and passive orders; the price is the
// record's own, which is the passive order's (orderbook.rs match_orders).  side_is_bid is the PASSIVE order's side:
//   side_is_bid == 1   the passive order was a bid: its trader buys, the active order's trader sells;
//   side_is_bid == 0   the passive order was an ask: the active order's trader buys, the passive one's sells.
// All arithmetic is modulo 2^64 (two's complement for the signed words); vol * price is the full 32 x 32 -> 64-bit product.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BKD_ACCT_HD __host__ __device__ inline
#else
#define BKD_ACCT_HD inline
#endif

namespace bkd {
namespace accounts {

struct Delta {  // added word by word (mod 2^64) to a bk_account row {position, cash, volume, fills}
  uint64_t position, cash, volume, fills;
};

struct Parties {
  uint32_t buyer, seller;  // trader ids
};

BKD_ACCT_HD Parties parties(uint32_t side_is_bid, uint32_t active_trader, uint32_t passive_trader) {
  Parties p;
  p.buyer = side_is_bid ? passive_trader : active_trader;
  p.seller = side_is_bid ? active_trader : passive_trader;
  return p;
}

BKD_ACCT_HD uint64_t notional(uint32_t price, uint32_t vol) { return static_cast<uint64_t>(price) * static_cast<uint64_t>(vol); }

// the buyer's row gains vol and pays vol * price
BKD_ACCT_HD Delta buyer_delta(uint32_t price, uint32_t vol) {
  Delta d;
  d.position = static_cast<uint64_t>(vol);
  d.cash = 0ull - notional(price, vol);
  d.volume = vol;
  d.fills = 1;
  return d;
}

// the seller's row loses vol and receives vol * price
BKD_ACCT_HD Delta seller_delta(uint32_t price, uint32_t vol) {
  Delta d;
  d.position = 0ull - static_cast<uint64_t>(vol);
  d.cash = notional(price, vol);
  d.volume = vol;
  d.fills = 1;
  return d;
}

BKD_ACCT_HD void add(Delta& a, const Delta& b) {
  a.position += b.position;
  a.cash += b.cash;
  a.volume += b.volume;
  a.fills += b.fills;
}

}  // namespace accounts
}  // namespace bkd
