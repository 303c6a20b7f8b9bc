// open_orders.hpp - bk_open_orders_*: every trader's resting orders per book of a DEVICE-INGRESS env, kept on the device.
//
// The reference has no counterpart (its users join Env::get_orders with the book on the host).  The env keeps two tables,
// summary[n_books][n_traders] rows of 32 B (bk_open_summary) and entries[n_books][n_traders][depth] rows of 16 B
// (bk_open_order), and k_refresh<R> recomputes a book's rows from its pool - the state block as the last step left it - and
// the order records' trader ids (dorders[book][id][0].y).  It is stateless: no cursor, nothing in a snapshot.  DESIGN.md 2.17:
//   * one wave per book, REFRESH_WAVES waves per block (the last block may hold fewer books); with a mask (the tail of
//     bk_ingress_reset_books*) the wave of an unmasked unit returns at once;
//   * lane l holds slot r * 64 + l of every pool register r: price, vol, id and meta, and - for a live slot whose id has a
//     record (id < max_orders) - the trader, gathered from dorders; a trader >= n_traders counts as no trader;
//   * the traders are taken 64 at a time (trader x belongs to chunk x / 64; one chunk for n_traders <= 64).  Inside a chunk
//     the wave loops over the distinct traders present: the first pending slot's trader by readlane, the matching slots by
//     one ballot per register, then ONE walk over the matched slots with their volume, price, side and id broadcast by
//     readlane - the summary accumulates in scalar arithmetic (open_order_rows.hpp) and every lane bumps the rank of its own
//     slots whose id is above the broadcast one.  Matched lanes with rank < depth store their 16-byte entry at
//     entries[book][x][rank] (ascending order id), the lanes behind the used ones store the empty entry, lanes 0 and 1 the
//     two halves of the summary row;
//   * the chunk's traders with no resting order get the empty row from the lane x % 64 and the empty entries from one
//     flat, coalesced pass over the chunk's entries.  Every row of the book is written exactly once per launch.
// Plain C++, no LDS, no scratch, no atomic, vector loads and stores only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "book_device.hpp"
#include "open_order_rows.hpp"

namespace bkd {
namespace open_orders {

constexpr int REFRESH_WAVES = 4;  // waves (books) per block of k_refresh
constexpr uint32_t MAX_TRADERS = 65536u, MAX_DEPTH = 64u;
constexpr uint32_t NO_TRADER = 0xFFFFFFFFu;

struct RefreshArgs {
  const uint8_t* mask;  // [n_books / M] device memory; nullptr: every book
  uint32_t M;           // books per mask byte (bk_ingress_reset_books*' units are markets)
  const uint32_t* state;  // [n_books][stride]
  uint32_t stride, n_books;
  const uint32_t* dorders;  // [n_books][max_orders][2] x 4 words: word 1 of a record is the order's trader
  uint32_t max_orders;
  bk_u32x4* summary;  // [n_books][n_traders][2]
  bk_u32x4* entries;  // [n_books][n_traders][depth]; nullptr with depth == 0
  uint32_t n_traders, depth;
  uint32_t depth_inv;  // ceil(2^24 / depth): e / depth == (e * depth_inv) >> 24 for e < 4096 (host_math.hpp-style, depth <= 64)
};

__device__ __forceinline__ bk_u32x4 entry_vec(const Entry& e) {
  bk_u32x4 v = {e.order_id, e.price, e.vol, e.side_is_bid};
  return v;
}

template <int R>
__global__ __launch_bounds__(64 * REFRESH_WAVES) void k_refresh(RefreshArgs g) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t b = rfl(blockIdx.x * REFRESH_WAVES + (threadIdx.x >> 6));
  if (b >= g.n_books) return;
  if (g.mask && rfl(static_cast<uint32_t>(g.mask[b / g.M])) == 0u) return;

  const uint32_t* pool = g.state + static_cast<size_t>(b) * g.stride + HDR_DW;
  const uint32_t* recs = g.dorders + static_cast<size_t>(b) * g.max_orders * 8;
  uint32_t price[R], vol[R], id[R], side[R], trader[R], rank[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const uint32_t* p = pool + r * POOL_FIELDS * 64;
    price[r] = p[lane];
    vol[r] = p[64 + lane];
    id[r] = p[128 + lane];
    const uint32_t meta = p[256 + lane];
    side[r] = (meta >> 1) & 1u;
    // (an id at or beyond max_orders has no record: never read, the order is left out - its book carries ORDER_LOG_FULL)
    const bool known = (meta & 1u) != 0u && id[r] < g.max_orders;
    uint32_t t = NO_TRADER;
    if (known) t = recs[static_cast<size_t>(id[r]) * 8 + 1];
    trader[r] = t < g.n_traders ? t : NO_TRADER;
  }

  const uint32_t depth = g.depth;
  bk_u32x4* rows = g.summary + static_cast<size_t>(b) * g.n_traders * 2;
  bk_u32x4* ents = depth ? g.entries + static_cast<size_t>(b) * g.n_traders * depth : nullptr;
  const bk_u32x4 none = entry_vec(empty_entry());
  const uint32_t n_chunks = (g.n_traders + 63u) >> 6;
  for (uint32_t c = 0; c < n_chunks; ++c) {
    unsigned long long todo[R], any = 0ull;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      todo[r] = __ballot((trader[r] >> 6) == c);  // (NO_TRADER >> 6 is beyond the last chunk)
      any |= todo[r];
    }
    unsigned long long present = 0ull;  // bit x % 64: trader x of this chunk rests an order
    while (any != 0ull) {
      uint32_t x = NO_TRADER;
#pragma unroll
      for (int r = R - 1; r >= 0; --r)
        if (todo[r] != 0ull) x = rdl(trader[r], static_cast<uint32_t>(__builtin_ctzll(todo[r])));
      unsigned long long match[R];
      any = 0ull;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        match[r] = __ballot(trader[r] == x);
        todo[r] &= ~match[r];
        any |= todo[r];
        rank[r] = 0u;
      }
      present |= 1ull << (x & 63u);
      Summary s = empty_summary();
#pragma unroll
      for (int r = 0; r < R; ++r) {
        unsigned long long walk = match[r];
        while (walk != 0ull) {
          const uint32_t l = static_cast<uint32_t>(__builtin_ctzll(walk));
          walk &= walk - 1ull;
          add_order(s, rdl(side[r], l), rdl(price[r], l), rdl(vol[r], l));
          if (depth) {
            const uint32_t w_id = rdl(id[r], l);
#pragma unroll
            for (int q = 0; q < R; ++q) rank[q] += w_id < id[q] ? 1u : 0u;
          }
        }
      }
      uint32_t w[8];
      summary_words(s, w);
      if (lane < 2u) {
        bk_u32x4 half;
        half.x = lane ? w[4] : w[0], half.y = lane ? w[5] : w[1], half.z = lane ? w[6] : w[2], half.w = lane ? w[7] : w[3];
        rows[static_cast<size_t>(x) * 2 + lane] = half;
      }
      if (depth) {
        bk_u32x4* list = ents + static_cast<size_t>(x) * depth;
#pragma unroll
        for (int r = 0; r < R; ++r)
          if (lane_bit(match[r]) && rank[r] < depth) list[rank[r]] = entry_vec(pack_entry(id[r], price[r], vol[r], side[r]));
        const uint32_t k = entries_used(s, depth) + lane;  // the slots behind the used ones (depth <= 64: one pass)
        if (k < depth) list[k] = none;
      }
    }
    // the chunk's traders with no resting order
    const uint32_t x0 = c << 6, x = x0 + lane;
    if (x < g.n_traders && !lane_bit(present)) {
      uint32_t w[8];
      summary_words(empty_summary(), w);
      bk_u32x4 h0 = {w[0], w[1], w[2], w[3]}, h1 = {w[4], w[5], w[6], w[7]};
      rows[static_cast<size_t>(x) * 2] = h0;
      rows[static_cast<size_t>(x) * 2 + 1] = h1;
    }
    if (depth) {
      const uint32_t in_chunk = g.n_traders - x0 < 64u ? g.n_traders - x0 : 64u;
      const uint32_t n_e = in_chunk * depth;  // <= 4096
      bk_u32x4* list = ents + static_cast<size_t>(x0) * depth;
      for (uint32_t e = lane; e < n_e; e += 64u) {
        const uint32_t t = (e * g.depth_inv) >> 24;  // e / depth
        if (((present >> t) & 1ull) == 0ull) list[e] = none;
      }
    }
  }
}

}  // namespace open_orders
}  // namespace bkd
