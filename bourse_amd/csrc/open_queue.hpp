// open_queue.hpp - bk_open_queue_*: the queue position of every listed resting order of a DEVICE-INGRESS env, kept on the device.
//
// The companion of open_orders.hpp's entries: queue[n_books][n_traders][depth] rows of 32 B (bk_open_queue), one per entry, and
// k_refresh<R> recomputes a book's rows from its pool - price, vol, id, seq and meta of every slot - and the entries the
// open-order refresh in front of it on the stream wrote.  It reads pool facts only, never the order records: every live slot
// counts, whoever owns it.  It is stateless: no cursor, nothing in a snapshot.  DESIGN.md 2.19:
//   * one wave per book, REFRESH_WAVES waves per block (the last block may hold fewer books); with a mask (the tail of
//     bk_ingress_reset_books*) the wave of an unmasked unit returns at once;
//   * lane l holds slot r * 64 + l of every pool register r; the live slots are one ballot per register;
//   * the book's entries are taken 64 at a time, one per lane.  A pass with no used entry stores its empty rows and walks
//     nothing.  Otherwise a first walk over the live slots broadcasts each one's id and seq by readlane and the lane whose
//     entry has that id keeps the stamp; a second walk broadcasts each live slot's side, price, stamp and volume, and every
//     lane adds it to its own row when it is ahead of, or level with, its entry (open_queue_rows.hpp);
//   * every lane stores its 32-byte row, two 16-byte vectors at consecutive addresses.  Every row of the book is written
//     exactly once per launch.
// Plain C++, no LDS, no scratch, no atomic, no cross-lane reduction, vector loads and stores only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "book_device.hpp"
#include "open_queue_rows.hpp"

namespace bkd {
namespace open_queue {

constexpr int REFRESH_WAVES = 4;  // waves (books) per block of k_refresh
constexpr uint32_t NO_ORDER = 0xFFFFFFFFu;  // order_id of an unused entry (open_order_rows.hpp)

struct RefreshArgs {
  const uint8_t* mask;  // [n_books / M] device memory; nullptr: every book
  uint32_t M;           // books per mask byte (bk_ingress_reset_books*' units are markets)
  const uint32_t* state;  // [n_books][stride]
  uint32_t stride, n_books;
  const bk_u32x4* entries;  // [n_books][n_entries]: {order_id, price, vol, side_is_bid} as open_orders::k_refresh left them
  bk_u32x4* queue;          // [n_books][n_entries][2]
  uint32_t n_entries;       // n_traders * depth, > 0
};

template <int R>
__global__ __launch_bounds__(64 * REFRESH_WAVES) void k_refresh(RefreshArgs g) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t b = rfl(blockIdx.x * REFRESH_WAVES + (threadIdx.x >> 6));
  if (b >= g.n_books) return;
  if (g.mask && rfl(static_cast<uint32_t>(g.mask[b / g.M])) == 0u) return;

  const uint32_t* pool = g.state + static_cast<size_t>(b) * g.stride + HDR_DW;
  uint32_t price[R], vol[R], id[R], seq[R], side[R];
  unsigned long long live[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const uint32_t* p = pool + r * POOL_FIELDS * 64;
    price[r] = p[lane];
    vol[r] = p[64 + lane];
    id[r] = p[128 + lane];
    seq[r] = p[192 + lane];
    const uint32_t meta = p[256 + lane];
    side[r] = (meta >> 1) & 1u;
    live[r] = __ballot((meta & 1u) != 0u);
  }

  const bk_u32x4* ents = g.entries + static_cast<size_t>(b) * g.n_entries;
  bk_u32x4* rows = g.queue + static_cast<size_t>(b) * g.n_entries * 2;
  for (uint32_t e0 = 0; e0 < g.n_entries; e0 += 64u) {
    const uint32_t e = e0 + lane;
    const bool in = e < g.n_entries;  // (the lanes behind the last entry stay in the walks: readlane wants the whole wave)
    bk_u32x4 ent = {NO_ORDER, 0u, 0u, 0u};
    if (in) ent = ents[e];
    const bool used = ent.x != NO_ORDER;
    Row row = empty_row();
    if (__ballot(used) != 0ull) {
      // the stamp of every lane's entry
      uint32_t stamp = 0u;
      bool found = false;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        unsigned long long walk = live[r];
        while (walk != 0ull) {
          const uint32_t l = static_cast<uint32_t>(__builtin_ctzll(walk));
          walk &= walk - 1ull;
          const bool mine = used && rdl(id[r], l) == ent.x;
          stamp = mine ? rdl(seq[r], l) : stamp;
          found = found || mine;
        }
      }
      // every live slot against every lane's entry (an entry whose id is not live keeps the empty row)
#pragma unroll
      for (int r = 0; r < R; ++r) {
        unsigned long long walk = live[r];
        while (walk != 0ull) {
          const uint32_t l = static_cast<uint32_t>(__builtin_ctzll(walk));
          walk &= walk - 1ull;
          const uint32_t where = place(ent.w, ent.y, stamp, rdl(side[r], l), rdl(price[r], l), rdl(seq[r], l));
          add_order(row, found ? where : 0u, rdl(vol[r], l));
        }
      }
    }
    uint32_t w[8];
    row_words(row, w);
    const bk_u32x4 h0 = {w[0], w[1], w[2], w[3]}, h1 = {w[4], w[5], w[6], w[7]};
    if (in) {
      rows[static_cast<size_t>(e) * 2] = h0;
      rows[static_cast<size_t>(e) * 2 + 1] = h1;
    }
  }
}

}  // namespace open_queue
}  // namespace bkd
