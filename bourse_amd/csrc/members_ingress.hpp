// members_ingress.hpp - agents.update(env, rng) of an AgentSet with NoiseAgent / MomentumAgent members (with or without
// RandomAgents members, in declaration order: crates/macros/src/lib.rs:57-73) into the device-resident ingress queues
// (bk_update_members).  The members and the submitted instructions of one env share every book's queue, its id counter and
// its RNG, as the reference's background agents and a user's own agent share one `Env` and one `rng` (env.rs:116-219,
// runner.rs:53-68).  The step itself is k_step_events' over that queue, unchanged.
//
// Restated semantics (paths relative to the reference repo):
//   common::cancel_live_orders            crates/step_sim/src/agents/common.rs:56-75
//   NoiseAgent::update                    crates/step_sim/src/agents/noise_agent.rs:127-176
//   MomentumAgent::update                 crates/step_sim/src/agents/momentum_agent.rs:146-208
//   RandomAgents::update                  crates/step_sim/src/agents/random_agent.rs:85-119
// with the draws, thresholds and f64 routines of mixed_update_and_shuffle (mixed_agents.hpp) - the same MixedDesc
// records, the same pm_math.hpp functions, no FMA contraction.
//
// One wave per book.  The walk over a member's list and its traders is the book's serial RNG stream - wave-uniform, the RNG
// in scalar registers; everything else is lane-parallel:
//   * a member's `orders` vector is a row of ids in device memory, in insertion (= ascending id) order.  The filter of
//     cancel_live_orders takes 64 entries per pass into lanes.  Status::Active of an entry = its id rests in the book's pool
//     right now: ONE SWEEP over the pool's ids per pass - every live register's 64 ids are broadcast in turn (v_readlane)
//     and compared with all 64 entries at once.  That is 3 instructions per pool slot and pass whatever the list holds;
//     R ballots per entry cost the same at a full pass but sit inside the serial walk, and an LDS table of the live ids
//     needs the same 64 R compares per pass behind an LDS round trip.  Registers of the pool that hold nothing live are
//     skipped.  An order queued earlier in the same step is New (not yet in the pool), a filled or cancelled one has left
//     it: both are dropped without a draw - the order log is not read;
//   * the draws that follow are one next_u32 per Active entry, in list order; the kept ids go back compacted (lane_rank), the
//     cancellation records to the queue in list order;
//   * the traders' loop collects its New orders in lanes (v_writelane), 64 at a time, and writes their records, their
//     `dorders` halves, their first order-log entries (k_ingest's: write_new_order) and the list's new entries
//     lane-parallel in event order;
//   * a RandomAgents member keeps its agents' held ids (AGENT_HELD_NONE = None) in the same row and walks them with
//     k_update_agents' pass (agents_ingress.hpp: random_agent, random_pass_end);
//   * MomentumAgent's momentum / last_price / "has a last price" live in an array of their own (the header's H_GST words
//     belong to bk_run's kernels); the RNG words, H_NEXT_ID, the flags and the queue length are written once per book.
// Capacity: an event beyond the queue's room, or a New order once the u32 id space is exhausted, is dropped and the book
// flagged FLAG_EVENT_OVERFLOW (the draws are taken all the same; a dropped New consumes no id and enters no list).  A list
// row has 64 R + max n_agents entries: after the filter it holds Active orders only (at most the pool's slots), and one
// update pushes at most n_agents more.
#pragma once
#include "agents_ingress.hpp"
#include "mixed_agents.hpp"

#pragma clang fp contract(off)

namespace bkd {
namespace ingress {

struct MembersIngressArgs {
  IngressArgs io;
  uint32_t n_members;
  uint32_t tick;            // the book's tick size (create_order's check)
  const MixedDesc* descs;   // member j of book b: descs[b * d_stride + j] (the per-book table; d_stride 0 = one row for all)
  const uint32_t* id_start; // ... and its first trader id, id_start[b * d_stride + j]
  uint32_t d_stride;
  uint32_t list_cap;        // entries per row
  uint32_t* lists;          // [n_books][n_members][list_cap] order ids
  uint32_t* lens;           // [n_books][n_members]
  uint64_t* mstate;         // [n_books][n_members][2] momentum, last_price (f64 bits)
  uint32_t* mflags;         // [n_books] bit j: member j has a last price
};

// rows this size never overflow (see above); the host sizes them with it
constexpr uint32_t members_list_cap(uint32_t R, uint32_t max_n_agents) { return 64u * R + max_n_agents; }
static_assert(members_list_cap(8, 0xFFFFu) == 512u + 65535u, "a row holds the pool's slots and one update's pushes");

// one MixedDesc record (128 bytes) through the scalar cache: a wave-uniform address, written by the host only
__device__ __forceinline__ MixedDesc sload_desc(const MixedDesc* p) {
  bk_u32x16 a, b;
  asm volatile("s_load_dwordx16 %0, %2, 0x0\n\ts_load_dwordx16 %1, %2, 0x40\n\ts_waitcnt lgkmcnt(0)"
               : "=&s"(a), "=&s"(b)
               : "s"(p));
  MixedDesc D;
  D.type = a[0], D.n = a[1], D.thr = a[2], D.tick_lo = a[3], D.tick_rng = a[4], D.tick_zone = a[5], D.vol_lo = a[6];
  D.vol_rng = a[7], D.vol_zone = a[8], D.tick_size = a[9], D.thr_limit = a[10], D.thr_market = a[11];
  D.keep_thr = (int32_t)a[12], D.trade_vol = a[13], D.slot_base = a[14], D.pad = a[15];
  D.mu = pm::from_bits(mk64(b[0], b[1])), D.sigma = pm::from_bits(mk64(b[2], b[3]));
  D.decay = pm::from_bits(mk64(b[4], b[5])), D.demand = pm::from_bits(mk64(b[6], b[7]));
  D.scale = pm::from_bits(mk64(b[8], b[9])), D.order_ratio = pm::from_bits(mk64(b[10], b[11]));
  D.n_f = pm::from_bits(mk64(b[12], b[13])), D.tick_f = pm::from_bits(mk64(b[14], b[15]));
  return D;
}

// New orders collected in lanes, in event order: lane k holds the k-th of the batch (ids id0 + k)
struct NewBatch {
  uint32_t price, trader;  // per lane
  uint64_t bidm, limm;     // bid side; limit orders (they enter the member's list)
  uint32_t cnt, id0, ev0;
};

// the batch's records, dorders halves and first log entries (write_new_order), and the limit orders' ids onto the list
// (`tag`: random_pass_end's)
__device__ __forceinline__ void flush_new(const Walk& W, NewBatch& N, uint32_t vol, uint32_t* list, uint32_t& len,
                                          uint32_t list_cap, int lane, uint32_t tag) {
  if (N.cnt == 0) return;
  const bool mine = (uint32_t)lane < N.cnt;
  const uint32_t id = N.id0 + (uint32_t)lane;
  const uint32_t bid = lane_bit(N.bidm) ? 1u : 0u;
  if (mine) {
    W.q[W.q0 + N.ev0 + (uint32_t)lane] = make_uint4((bid << 8) | tag, id, N.price, vol);
    write_new_order(W.rec, id, vol, N.trader, N.price, bid);
  }
  const uint32_t rank = lane_rank(N.limm);
  if (lane_bit(N.limm) && len + rank < list_cap) list[len + rank] = id;
  len += (uint32_t)__builtin_popcountll(N.limm);
  N.cnt = 0;
  N.bidm = N.limm = 0;
}

// Env::place_order from a Noise / Momentum trader: the id and the New event (dropped and flagged beyond the queue's room
// or the id space); a limit price off the book's tick grid is flagged and creates nothing (mixed_create's rule,
// mixed_agents.hpp); a market order carries the extreme price of its side (orderbook.rs:595) and takes no check
__device__ __forceinline__ void place_new(Walk& W, NewBatch& N, bool limit, bool is_bid, uint32_t price, uint32_t trader,
                                          uint32_t tick, uint32_t vol, uint32_t* list, uint32_t& len, uint32_t list_cap,
                                          int lane, uint32_t tag) {
  if (limit && price % tick != 0) {
    W.flags |= FLAG_PRICE_TICK;
    return;
  }
  if (!(W.n_ev < W.room && W.next_id < AGENT_HELD_NONE - 1u)) {
    W.flags |= FLAG_EVENT_OVERFLOW;
    return;
  }
  if (N.cnt == 64u) flush_new(W, N, vol, list, len, list_cap, lane, tag);
  if (N.cnt == 0) {
    N.id0 = W.next_id;
    N.ev0 = W.n_ev;
  }
  const uint64_t bit = 1ull << N.cnt;
  N.price = wrl(price, N.cnt, N.price);
  N.trader = wrl(trader, N.cnt, N.trader);
  N.bidm |= is_bid ? bit : 0ull;
  N.limm |= limit ? bit : 0ull;
  N.cnt += 1;
  W.n_ev += 1;
  W.next_id += 1;
}

template <int R>
__global__ __launch_bounds__(64) void k_update_members(MembersIngressArgs g) {
  const int lane = threadIdx.x;
  const uint32_t book = blockIdx.x;
  uint32_t* st = g.io.state + (size_t)book * g.io.state_stride;
  const uint32_t hdr = st[lane];
  uint64_t live[R];
#pragma unroll
  for (int r = 0; r < R; ++r) live[r] = mk64(rdl(hdr, H_LIVE0 + 2 * r), rdl(hdr, H_LIVE0 + 2 * r + 1));
  uint32_t pid[R];  // the pool's ids; AGENT_HELD_NONE where nothing rests (no order has that id)
  double mid;       // OrderBook::mid_price (orderbook.rs:272-276) of the book as it stands: updates only queue events
  {
    uint32_t mb = 0u, mk = 0xFFFFFFFFu;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const uint32_t* p = st + HDR_DW + r * POOL_FIELDS * 64;
      const uint32_t price = p[0 * 64 + lane], meta = p[4 * 64 + lane];
      pid[r] = sel(live[r], p[2 * 64 + lane], AGENT_HELD_NONE);
      const bool is_bid = (meta & 2u) != 0;
      mb = max(mb, (lane_bit(live[r]) && is_bid) ? price : 0u);
      mk = min(mk, (lane_bit(live[r]) && !is_bid) ? price : 0xFFFFFFFFu);
    }
    const uint32_t bid = wave_umax(mb), ask = wave_umin(mk);
    mid = static_cast<double>(bid) + 0.5 * static_cast<double>(ask - bid);
  }
  Walk W = walk_begin(g.io, book, hdr);
  Rng& rng = W.rng;
  const MixedDesc* row = g.descs + (size_t)book * g.d_stride;
  const uint32_t* id_start = g.id_start + (size_t)book * g.d_stride;
  uint32_t mflags = rfl(g.mflags[book]);

  for (uint32_t j = 0; j < g.n_members; ++j) {
#define BK_MU_UNIT book
#define BK_MU_TICK g.tick
#define BK_MU_TAG 0u
#include "members_update_body.inc"
#undef BK_MU_UNIT
#undef BK_MU_TICK
#undef BK_MU_TAG
  }
  walk_end(W, g.io, st, hdr, lane);
  if (lane == 0) g.mflags[book] = mflags;
}

}  // namespace ingress
}  // namespace bkd
