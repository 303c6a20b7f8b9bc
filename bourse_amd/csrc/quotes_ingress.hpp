// quotes_ingress.hpp - bk_submit_quotes*: a dense table of target quotes, one row per trader of the open-order view, turned
// into the book's cancellations, in-place reductions and new orders and queued on the device.
//
// The reference has no counterpart.  The call is DEFINED as a dense instruction batch: book b's batch is the grid
// n_traders x G, G = depth + 2, trader-major - positions 0 .. depth - 1 of a trader are its entry slots (action 2 with the
// entry's id, BK_ACTION_MODIFY with side bit 2, the new volume and the entry's id, or action 0), position depth is the new
// bid and depth + 1 the new ask (action 1 or 0); quote_rows.hpp makes each position's element.  k_submit queues that grid
// exactly as k_ingest (book_device.hpp) queues the same grid from six arrays with book_offsets[b] = b * n_traders * G:
//   * one wave per market (per book when assets == 1), lanes hold grid positions, 64 per pass - k_ingest's passes over the
//     same grid, so a bad price, a full queue or an exhausted id space cuts at the same element with the same code;
//   * each pass is k_ingest's pass: ballots for bad price, room and new orders, lane_rank for queue position and id,
//     write_new_order for the records, one header and qlen write per book / market.  It is a COPY of k_ingest's pass, not
//     shared code: k_ingest must keep compiling instruction for instruction, and its elements come from six arrays by index
//     where these come from registers;
//   * how a lane learns its trader's keepers: it loads the trader's quote row (16 B) and walks the trader's entries in list
//     order with 16-byte loads, feeding quote_rows.hpp's see_entry.  The lanes of one trader read the same addresses in the
//     same iteration, so a trader's G lanes share every load; the entries of a list are packed (open_orders::k_refresh puts
//     the used ones first), so a lane leaves the walk at the first unused entry.  No LDS pre-pass: with G = depth + 2 lanes
//     per trader a pre-pass with lanes as traders would use 64 / G of the wave and needs the same loads.
// It reads the quote rows, the entries table, the header words k_ingest reads (H_NEXT_ID, H_T_LO / HI) and the queue length:
// no pool word, hence no pool-size template.  Plain C++, no LDS, no scratch, no atomic, vector loads and stores only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "book_device.hpp"
#include "quote_rows.hpp"

namespace bkd {
namespace quotes {

struct SubmitArgs {
  const bk_u32x4* quotes;   // [n_books][n_traders] {bid_price, bid_vol, ask_price, ask_vol}
  const bk_u32x4* entries;  // [n_books][n_traders][depth] as open_orders::k_refresh left them
  uint32_t n_traders, depth;  // depth > 0
  unsigned long long* out_ids;  // nullable: [n_books][n_traders][2] id of the new bid / ask this call created, else u64::MAX
  uint32_t* status;             // nullable: [2 * n_books] {code (bk_status), grid positions of the book's batch applied}
  uint4* q;                     // [n_markets][qcap] event records (HostEvent layout)
  uint32_t* qlen;               // [n_markets]
  uint32_t qcap;
  uint4* dorders;               // [n_books][log_cap][2] immutable halves (write_new_order)
  uint32_t* mods_flag;          // nullable: k_ingest's hint word (IngestArgs::mods_flag)
};

__global__ __launch_bounds__(64) void k_submit(DevArgs a, SubmitArgs g) {
  const uint32_t lane = threadIdx.x;
  const uint32_t mkt = blockIdx.x, M = a.assets;
  const uint32_t depth = g.depth, G = depth + 2u, n = g.n_traders * G;  // (<= 65536 * 66: no wrap)
  uint32_t qn = g.qlen[mkt];
  uint4* q = g.q + (size_t)mkt * g.qcap;
  for (uint32_t asset = 0; asset < M; ++asset) {
    const uint32_t book = mkt * M + asset;
    uint32_t* hdr = a.state + (size_t)book * a.state_stride;
    const uint32_t tick = a.asset_tick[asset];
    uint32_t next_id = rfl(hdr[H_NEXT_ID]);
    const NewOrderRecords rec{g.dorders, a.order_log, book, a.log_cap, rfl(hdr[H_T_LO]), rfl(hdr[H_T_HI])};
    const bk_u32x4* quotes = g.quotes + (size_t)book * g.n_traders;
    const bk_u32x4* entries = g.entries + (size_t)book * g.n_traders * depth;
    uint32_t code = ING_OK, applied = 0;
    for (uint32_t base = 0; base < n && code == ING_OK; base += 64u) {
      const uint32_t p = base + lane;
      const bool in = p < n;
      const uint32_t trader = in ? p / G : 0u, at = p - trader * G;
      // this position's element
      Element x = no_element();
      if (in) {
        const bk_u32x4 qv = quotes[trader];
        const Quote qt = {qv.x, qv.y, qv.z, qv.w};
        const bk_u32x4* list = entries + (size_t)trader * depth;
        Keepers keep = no_keepers();
        Entry mine = {NO_ORDER, 0u, 0u, 0u};
        for (uint32_t k = 0; k < depth; ++k) {
          const bk_u32x4 ev = list[k];
          if (ev.x == NO_ORDER) break;  // (the used entries come first)
          const Entry e = {ev.x, ev.y, ev.z, ev.w};
          see_entry(keep, qt, k, e);
          if (k == at) mine = e;
        }
        x = at < depth ? entry_element(keep, qt, at, mine) : new_element(keep, qt, at == depth ? 1u : 0u);
      }
      const uint32_t act = x.action, sd = x.side, vol = x.vol, price = x.price;
      // from here on: k_ingest's pass
      const bool is_new = act == ACT_NEW, is_ev = act != ACT_NONE;
      if (g.mods_flag && __ballot(in && act == ACT_MODIFY) && lane == 0u) *g.mods_flag = 1u;
      // the first bad price of the chunk stops the book's batch (earlier elements are applied)
      const uint64_t badm = __ballot(is_new && price % tick != 0u);
      uint32_t cut = badm ? (uint32_t)__builtin_ctzll(badm) : 64u;
      if (badm) code = ING_PRICE;
      // ... so does a full queue / an exhausted id space (BK_CAPACITY)
      uint64_t evm = __ballot(in && is_ev && lane < cut);
      const uint32_t room = g.qcap - qn;
      if ((uint32_t)__builtin_popcountll(evm) > room) {
        uint64_t m = evm;  // the events that do not fit: all but the first `room`
        for (uint32_t r = 0; r < room; ++r) m &= m - 1ull;
        cut = (uint32_t)__builtin_ctzll(m);
        code = ING_CAPACITY;
        evm = __ballot(in && is_ev && lane < cut);
      }
      if ((uint64_t)next_id + 64u >= 0xFFFFFFFFull) {  // ids are u32 on the device: refuse the chunk
        cut = 0;
        code = ING_CAPACITY;
        evm = 0;
      }
      const bool valid = in && lane < cut;
      const uint64_t newm = __ballot(valid && is_new);
      const uint32_t rank_ev = lane_rank(evm);
      const uint32_t rank_new = lane_rank(newm);
      const uint32_t id = next_id + rank_new;
      if (valid && is_ev) {
        uint4 e;
        if (is_new) {
          e = make_uint4(0u | ((sd & 1u) << 8) | (asset << 16), id, price, vol);
        } else if (act == ACT_CANCEL) {
          e = make_uint4(1u | (asset << 16), x.order_id, 0u, 0u);
        } else {  // a volume-only modification
          e = make_uint4(2u | (1u << 10) | (asset << 16), x.order_id, 0u, vol);
        }
        q[qn + rank_ev] = e;
      }
      if (valid && is_new) write_new_order(rec, id, vol, trader, price, sd & 1u);
      if (valid && g.out_ids && at >= depth)
        g.out_ids[((size_t)book * g.n_traders + trader) * 2 + (at - depth)] = is_new ? (unsigned long long)id : ~0ull;
      next_id += (uint32_t)__builtin_popcountll(newm);
      qn += (uint32_t)__builtin_popcountll(evm);
      applied += cut < 64u ? cut : (n - base < 64u ? n - base : 64u);
    }
    if (lane == 0u) {
      hdr[H_NEXT_ID] = next_id;
      if (g.status) {
        g.status[2 * book] = code;
        g.status[2 * book + 1] = applied;
      }
    }
  }
  if (lane == 0u) g.qlen[mkt] = qn;
}

}  // namespace quotes
}  // namespace bkd
