// market_ingress.hpp - RandomMarketAgents::update (random_agent.rs:204-245) and MarketAgent::update of a MarketAgentSet
// (NoiseMarketAgent noise_agent.rs:226-340, MomentumMarketAgent momentum_agent.rs:282-397, members in declaration order)
// into the device-resident ingress queue of every MARKET (bk_update_market_agents / bk_update_market_members).  The agents
// and the submitted instructions of one env share the market's queue, its books' id counters and its RNG, as the
// reference's background MarketAgents and a user's own agent share one MarketEnv and one rng (runner.rs:108-131).  The
// step itself is k_step_events<.., MKT>'s over that queue, unchanged.  DESIGN.md 2.18.
//
// One wave per market.  The walk is the market's serial RNG stream, wave-uniform in scalar registers, and it is
// agents_ingress.hpp's and members_ingress.hpp's: Walk, random_agent, random_pass_end, members_update_body.inc.  What a market adds:
//   * a group or member of asset a trades book market * assets + a: Active is tested against THAT pool (its ids are
//     loaded pre-masked where the pass or the member begins - the pools do not change during an update), ids come from
//     that book's counter, prices lie around that book's mid, records go to that book's rows (write_new_order);
//   * the walk's id counter and flags are those of the asset in hand.  The books' H_NEXT_ID, H_FLAGS and clock words
//     ride in vector registers, lane a = asset a (AssetWords): v_readlane where an asset is entered, v_writelane where it
//     is left, so groups may return to an asset; nothing is indexed in scalar registers and nothing spills;
//   * events carry asset << 16 in their first word (k_ingest's layout) and go to the market's queue in call order;
//   * a 64-agent pass serves one book (random_pass_end numbers its ids from one counter): market_walk.hpp cuts the
//     passes where the asset changes;
//   * every book of a market holds a copy of the market's RNG words and k_step_events shuffles with each book's own
//     copy, so the advanced state is written to all `assets` headers.
// Capacity is 2.12's drop rule on the market's queue; FLAG_EVENT_OVERFLOW / FLAG_PRICE_TICK go to the book of the asset
// whose event was dropped or refused.  No LDS, no scratch, no atomics, plain vector stores.
#pragma once
#include "market_walk.hpp"
#include "members_ingress.hpp"

#pragma clang fp contract(off)

namespace bkd {
namespace ingress {

struct MarketAgentsArgs {
  IngressArgs io;          // (q and qlen are per market)
  uint32_t assets;         // books per market
  uint32_t n_agents, n_groups;
  const Group* groups;     // group k of market m: groups[m * g_stride + k] (the per-market table; g_stride 0 = one row for all)
  uint32_t g_stride;
  uint32_t* held;          // [n_markets][n_agents] held order ids
};

struct MarketMembersArgs {
  IngressArgs io;
  uint32_t assets;
  uint32_t asset_tick[MAX_ASSETS];  // the books' tick sizes (create_order's check)
  uint64_t member_assets;           // member j trades asset (member_assets >> 8 j) & 0xFF
  uint32_t n_members;
  const MixedDesc* descs;           // member j of market m: descs[m * d_stride + j] (d_stride 0 = one row for all)
  const uint32_t* id_start;         // ... and its first trader id, id_start[m * d_stride + j]
  uint32_t d_stride;
  uint32_t list_cap;                // entries per row
  uint32_t* lists;                  // [n_markets][n_members][list_cap] order ids of the member's asset
  uint32_t* lens;                   // [n_markets][n_members]
  uint64_t* mstate;                 // [n_markets][n_members][2] momentum, last_price (f64 bits)
  uint32_t* mflags;                 // [n_markets] bit j: member j has a last price
};
static_assert(MAX_INGRESS_MEMBERS * 8 <= 64 && MAX_ASSETS <= 256, "the members' assets pack into one word");

// per lane: lane a < assets holds these header words of book market * assets + a
struct AssetWords {
  uint32_t next_id, flags, t_lo, t_hi;
};

// the market's RNG (book 0's copy: all copies are equal between kernels), its queue's room, its books' words
__device__ __forceinline__ Walk market_begin(const IngressArgs& g, uint32_t mkt, uint32_t M, AssetWords& A, int lane) {
  const uint32_t* st0 = g.state + (size_t)mkt * M * g.state_stride;
  const uint32_t* mine = st0 + (size_t)((uint32_t)lane < M ? lane : 0) * g.state_stride;
  A.next_id = mine[H_NEXT_ID], A.flags = mine[H_FLAGS], A.t_lo = mine[H_T_LO], A.t_hi = mine[H_T_HI];
  const uint32_t hdr = st0[lane];
  Walk W;
  W.rng.s0 = mk64(rdl(hdr, H_S0_LO), rdl(hdr, H_S0_HI));
  W.rng.s1 = mk64(rdl(hdr, H_S1_LO), rdl(hdr, H_S1_HI));
  W.next_id = W.flags = 0;
  W.rec = NewOrderRecords{g.dorders, g.order_log, mkt * M, g.log_cap, 0u, 0u};
  W.q0 = rfl(g.qlen[mkt]);
  W.room = g.qcap > W.q0 ? g.qcap - W.q0 : 0u;
  W.n_ev = 0;
  W.q = g.q + (size_t)mkt * g.qcap;
  return W;
}

// the walk takes the id counter, the flags and the record rows of asset a's book ...
__device__ __forceinline__ void enter_asset(Walk& W, const AssetWords& A, uint32_t book, uint32_t a) {
  W.next_id = rdl(A.next_id, a), W.flags = rdl(A.flags, a);
  W.rec.book = book, W.rec.t_lo = rdl(A.t_lo, a), W.rec.t_hi = rdl(A.t_hi, a);
}
// ... and hands them back
__device__ __forceinline__ void leave_asset(const Walk& W, AssetWords& A, uint32_t a) {
  A.next_id = wrl(W.next_id, a, A.next_id);
  A.flags = wrl(W.flags, a, A.flags);
}

// the advanced RNG into every book's copy, each book's id counter and flags, the queue's length
__device__ __forceinline__ void market_end(const Walk& W, const AssetWords& A, const IngressArgs& g, uint32_t mkt, uint32_t M,
                                           int lane) {
  uint32_t* st0 = g.state + (size_t)mkt * M * g.state_stride;
  uint32_t w = 0;
  w = wrl((uint32_t)W.rng.s0, H_S0_LO, w);
  w = wrl((uint32_t)(W.rng.s0 >> 32), H_S0_HI, w);
  w = wrl((uint32_t)W.rng.s1, H_S1_LO, w);
  w = wrl((uint32_t)(W.rng.s1 >> 32), H_S1_HI, w);
  const bool rng_word = lane == H_S0_LO || lane == H_S0_HI || lane == H_S1_LO || lane == H_S1_HI;
  for (uint32_t a = 0; a < M; ++a)
    if (rng_word) st0[(size_t)a * g.state_stride + lane] = w;
  if ((uint32_t)lane < M) {
    uint32_t* mine = st0 + (size_t)lane * g.state_stride;
    mine[H_NEXT_ID] = A.next_id;
    mine[H_FLAGS] = A.flags;
  }
  if (lane == 0) g.qlen[mkt] = W.q0 + W.n_ev;
}

template <int R>
__global__ __launch_bounds__(64) void k_update_market_agents(MarketAgentsArgs g) {
  const int lane = threadIdx.x;
  const uint32_t mkt = blockIdx.x, M = g.assets;
  AssetWords A;
  Walk W = market_begin(g.io, mkt, M, A, lane);
  uint32_t* held = g.held + (size_t)mkt * g.n_agents;
  const Group* gt = g.groups + (size_t)mkt * g.g_stride;
  const auto n_of = [gt](uint32_t k) { return rfl(gt[k].n); };
  const auto asset_of = [gt](uint32_t k) { return rfl(gt[k].asset); };
  PassCursor c;
  MarketPass p;
  while (next_pass(c, g.n_groups, n_of, asset_of, p)) {
    const uint32_t a = p.asset, book = mkt * M + a;
    const uint32_t* st = g.io.state + (size_t)book * g.io.state_stride;
    const uint32_t hdr = st[lane];
    uint32_t pid[R];  // the pool's ids; AGENT_HELD_NONE where nothing rests (no order has that id)
#pragma unroll
    for (int r = 0; r < R; ++r) pid[r] = st[HDR_DW + r * POOL_FIELDS * 64 + 2 * 64 + lane];
#pragma unroll
    for (int r = 0; r < R; ++r)
      pid[r] = sel(mk64(rdl(hdr, H_LIVE0 + 2 * r), rdl(hdr, H_LIVE0 + 2 * r + 1)), pid[r], AGENT_HELD_NONE);
    enter_asset(W, A, book, a);
    const bool in = (uint32_t)lane < p.len;
    const uint32_t h = in ? held[p.first + lane] : AGENT_HELD_NONE;
    RandomPass S(W);
    uint32_t gi = p.group, t = p.trader0;
    Group G = sload_group(gt + gi);
    for (uint32_t l = 0; l < p.len; ++l, ++t) {
      while (t >= G.n) {  // the next group that has an agent: the same asset (market_walk.hpp)
        ++gi;
        G = sload_group(gt + gi);
        t = 0;
      }
      random_agent<R>(W, S, G, pid, h, l, t);  // TraderId = the agent's index in its group
    }
    const uint32_t now = random_pass_end(W, S, h, a << 16);
    if (in) held[p.first + lane] = now;
    leave_asset(W, A, a);
  }
  market_end(W, A, g.io, mkt, M, lane);
}

// the live bits of a book's pool registers, the pool's ids (AGENT_HELD_NONE where nothing rests: no order has that id)
// and OrderBook::mid_price (orderbook.rs:272-276) as the book stands - what k_update_members loads once for its book
template <int R>
__device__ __forceinline__ void load_pool(const uint32_t* st, uint32_t hdr, int lane, uint64_t (&live)[R], uint32_t (&pid)[R],
                                          double& mid) {
  uint32_t mb = 0u, mk = 0xFFFFFFFFu;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    live[r] = mk64(rdl(hdr, H_LIVE0 + 2 * r), rdl(hdr, H_LIVE0 + 2 * r + 1));
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

template <int R>
__global__ __launch_bounds__(64) void k_update_market_members(MarketMembersArgs g) {
  const int lane = threadIdx.x;
  const uint32_t mkt = blockIdx.x, M = g.assets;
  AssetWords A;
  Walk W = market_begin(g.io, mkt, M, A, lane);
  Rng& rng = W.rng;
  const MixedDesc* row = g.descs + (size_t)mkt * g.d_stride;
  const uint32_t* id_start = g.id_start + (size_t)mkt * g.d_stride;
  uint32_t mflags = rfl(g.mflags[mkt]);
  uint32_t a = 0;
  // (a RandomAgents member leaves the body by `continue`: the walk hands the asset's words back in the loop's step)
  for (uint32_t j = 0; j < g.n_members; leave_asset(W, A, a), ++j) {
    a = (uint32_t)(g.member_assets >> (8u * j)) & 0xFFu;
    const uint32_t book = mkt * M + a;
    const uint32_t* st = g.io.state + (size_t)book * g.io.state_stride;
    uint64_t live[R];
    uint32_t pid[R];
    double mid;
    load_pool<R>(st, st[lane], lane, live, pid, mid);
    enter_asset(W, A, book, a);
#define BK_MU_UNIT mkt
#define BK_MU_TICK g.asset_tick[a]
#define BK_MU_TAG (a << 16)
#include "members_update_body.inc"
#undef BK_MU_UNIT
#undef BK_MU_TICK
#undef BK_MU_TAG
  }
  market_end(W, A, g.io, mkt, M, lane);
  if (lane == 0) g.mflags[mkt] = mflags;
}

}  // namespace ingress
}  // namespace bkd
