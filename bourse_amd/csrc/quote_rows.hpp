// quote_rows.hpp - one trader's row of bk_submit_quotes' table against that trader's listed entries, one grid position at a
// time.
//
// Compiled by the device kernel (quotes_ingress.hpp) and by a CPU test (tests/cpp/quote_rows_test.cpp): no HIP type, no
// intrinsic.  A quote row is {bid_price, bid_vol, ask_price, ask_vol} (bk_quote, 16 B); an entry is {order_id, price, vol,
// side_is_bid} (bk_open_order, 16 B), unused with order_id == 0xFFFFFFFF.  A trader's batch is G = depth + 2 grid positions:
// position k < depth is entry k's element (a cancellation, a volume-only modification or nothing), position depth the new
// bid and position depth + 1 the new ask (a new limit order or nothing).
//
// Per side S with the target (P, V): the KEEPER is the first used entry of side S whose price is P.  V == KEEP leaves the
// side alone, V == 0 cancels every listed order of it; otherwise every listed order of the side but the keeper is cancelled,
// a keeper that holds more than V is reduced to V in place, one that holds less is left and a new order (P, V - held) queues
// behind it, and without a keeper the new order is (P, V).  No sum is formed: V - held is taken only where held < V.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BKD_QUOTE_HD __host__ __device__ inline
#else
#define BKD_QUOTE_HD inline
#endif

namespace bkd {
namespace quotes {

constexpr uint32_t KEEP = 0xFFFFFFFFu;           // == BK_QUOTE_KEEP, as a side's vol
constexpr uint32_t NO_ORDER = 0xFFFFFFFFu;       // order_id of an unused entry (open_order_rows.hpp)
constexpr uint32_t ACT_NONE = 0u, ACT_NEW = 1u, ACT_CANCEL = 2u, ACT_MODIFY = 0x80000003u;  // k_ingest's actions
constexpr uint32_t SIDE_HAS_VOL = 4u;            // BK_ACTION_MODIFY's side bit 2: the element carries a new volume

struct Quote {
  uint32_t bid_price, bid_vol, ask_price, ask_vol;
};

struct Entry {
  uint32_t order_id, price, vol, side_is_bid;
};

// the keepers of both sides as far as the trader's list has been read
struct Keepers {
  uint32_t bid_at, bid_vol, ask_at, ask_vol;  // *_at: the entry's index in the list, NO_ORDER while none is found
};

// one element of the dense instruction grid (the trader is the row's)
struct Element {
  uint32_t action, side, vol, price, order_id;
};

BKD_QUOTE_HD Keepers no_keepers() {
  Keepers k;
  k.bid_at = NO_ORDER, k.bid_vol = 0u, k.ask_at = NO_ORDER, k.ask_vol = 0u;
  return k;
}

// entry `at` of the trader's list, taken in ascending index
BKD_QUOTE_HD void see_entry(Keepers& k, const Quote& q, uint32_t at, const Entry& e) {
  if (e.order_id == NO_ORDER) return;
  if (e.side_is_bid) {
    if (k.bid_at == NO_ORDER && e.price == q.bid_price) k.bid_at = at, k.bid_vol = e.vol;
  } else {
    if (k.ask_at == NO_ORDER && e.price == q.ask_price) k.ask_at = at, k.ask_vol = e.vol;
  }
}

BKD_QUOTE_HD Element no_element() {
  Element x;
  x.action = ACT_NONE, x.side = 0u, x.vol = 0u, x.price = 0u, x.order_id = 0u;
  return x;
}

// grid position `at` < depth: what happens to entry `at`, given the keepers of the WHOLE list
BKD_QUOTE_HD Element entry_element(const Keepers& k, const Quote& q, uint32_t at, const Entry& e) {
  Element x = no_element();
  if (e.order_id == NO_ORDER) return x;
  const uint32_t want = e.side_is_bid ? q.bid_vol : q.ask_vol;
  const uint32_t keeper = e.side_is_bid ? k.bid_at : k.ask_at;
  if (want == KEEP) return x;
  if (want == 0u || keeper != at) {
    x.action = ACT_CANCEL, x.order_id = e.order_id;
  } else if (e.vol > want) {
    x.action = ACT_MODIFY, x.side = SIDE_HAS_VOL, x.vol = want, x.order_id = e.order_id;
  }
  return x;
}

// grid position depth (side_is_bid = 1) or depth + 1 (side_is_bid = 0): the side's new order, given the keepers of the list
BKD_QUOTE_HD Element new_element(const Keepers& k, const Quote& q, uint32_t side_is_bid) {
  Element x = no_element();
  const uint32_t want = side_is_bid ? q.bid_vol : q.ask_vol, price = side_is_bid ? q.bid_price : q.ask_price;
  const uint32_t keeper = side_is_bid ? k.bid_at : k.ask_at, held = side_is_bid ? k.bid_vol : k.ask_vol;
  if (want == KEEP || want == 0u) return x;
  if (keeper != NO_ORDER && held >= want) return x;
  x.action = ACT_NEW, x.side = side_is_bid ? 1u : 0u, x.price = price;
  x.vol = keeper != NO_ORDER ? want - held : want;
  return x;
}

}  // namespace quotes
}  // namespace bkd
