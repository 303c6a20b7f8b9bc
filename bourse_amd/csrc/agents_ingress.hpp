// agents_ingress.hpp - RandomAgents::update (random_agent.rs:85-119) into the device-resident ingress queues
// (bk_update_agents): the on-device agents and the submitted instructions of one env share every book's queue, its id
// counter and its RNG, as the reference's background agents and a user's own agent share one `Env` and one `rng`
// (env.rs:116-219, runner.rs:53-68).  The step itself is k_step_events' over that queue, unchanged.
//
// One wave per book.  The walk over the agents is the book's serial RNG stream - wave-uniform, in scalar registers, the
// RandomAgents branch of mixed_update_and_shuffle on held ids instead of fixed pool slots; everything else is lane-parallel:
//   * lane l of pass p holds agent 64 p + l's held id (u32, AGENT_HELD_NONE = None) and, after the walk, the fields of its
//     new order (written into its lane with v_writelane);
//   * Status::Active of a held id = it rests in the book's pool right now: one ballot compare of the id against every pool
//     register, whose lanes hold AGENT_HELD_NONE where the header's live bit is clear.  An order queued earlier in the same
//     step is New (not yet in the pool); a filled or cancelled order has left it - the order log is not read;
//   * the pass's events go to the queue in agent order, compacted with lane_rank, with k_ingest's records and log entries
//     (write_new_order); the RNG words, H_NEXT_ID, the flags and the queue length are written once per book.
// Capacity: an event beyond the queue's room, or a New order once the u32 id space is exhausted, is dropped and the book
// flagged FLAG_EVENT_OVERFLOW (the draws are taken all the same; a dropped New consumes no id).  The agent then holds None.
//
// The walk's state (Walk, walk_begin, walk_end) and the pass over 64 RandomAgents (RandomPass, random_agent,
// random_pass_end) are shared with k_update_members (members_ingress.hpp), whose RandomAgents members take the same pass.
#pragma once

namespace bkd {

constexpr uint32_t AGENT_HELD_NONE = 0xFFFFFFFFu;

// what every kernel that queues a book's events is handed (bk_env::ingress_args)
struct IngressArgs {
  uint32_t* state;
  uint32_t state_stride, log_cap, qcap;
  uint4* q;              // [n_books][qcap] event records (k_ingest's layout)
  uint32_t* qlen;        // [n_books]
  uint4* dorders;        // [n_books][log_cap][2] immutable halves
  DevOrderLog* order_log;
};

struct AgentsIngressArgs {
  IngressArgs io;
  uint32_t n_agents;
  const Group* groups;   // group g of book b: groups[b * g_stride + g] (the per-book table; g_stride 0 = one row for all)
  uint32_t g_stride;
  uint32_t* held;        // [n_books][n_agents] held order ids
};

// what one book's update carries from pass to pass and from member to member
struct Walk {
  Rng rng;
  uint32_t next_id, flags, n_ev, room, q0;
  uint4* q;  // the book's queue
  NewOrderRecords rec;
};

// the book's RNG, id counter, flags and clock from its header quad (lane w holds header word w); the queue's room
__device__ __forceinline__ Walk walk_begin(const IngressArgs& g, uint32_t book, uint32_t hdr) {
  Walk W;
  W.rng.s0 = mk64(rdl(hdr, H_S0_LO), rdl(hdr, H_S0_HI));
  W.rng.s1 = mk64(rdl(hdr, H_S1_LO), rdl(hdr, H_S1_HI));
  W.next_id = rdl(hdr, H_NEXT_ID), W.flags = rdl(hdr, H_FLAGS);
  W.rec = NewOrderRecords{g.dorders, g.order_log, book, g.log_cap, rdl(hdr, H_T_LO), rdl(hdr, H_T_HI)};
  W.q0 = rfl(g.qlen[book]);
  W.room = g.qcap > W.q0 ? g.qcap - W.q0 : 0u;
  W.n_ev = 0;
  W.q = g.q + (size_t)book * g.qcap;
  return W;
}

// the header words the update changed: the RNG, the id counter, the flags; then the queue's length
__device__ __forceinline__ void walk_end(const Walk& W, const IngressArgs& g, uint32_t* st, uint32_t hdr, int lane) {
  uint32_t w = hdr;
  w = wrl((uint32_t)W.rng.s0, H_S0_LO, w);
  w = wrl((uint32_t)(W.rng.s0 >> 32), H_S0_HI, w);
  w = wrl((uint32_t)W.rng.s1, H_S1_LO, w);
  w = wrl((uint32_t)(W.rng.s1 >> 32), H_S1_HI, w);
  w = wrl(W.next_id, H_NEXT_ID, w);
  w = wrl(W.flags, H_FLAGS, w);
  if ((lane >= H_S0_LO && lane <= H_NEXT_ID) || lane == H_FLAGS) st[lane] = w;
  if (lane == 0) g.qlen[W.rec.book] = W.q0 + W.n_ev;
}

// One pass of RandomAgents::update over up to 64 agents, agent l in lane l: who cancels, who places (on which side), whose
// event was dropped; the new orders' fields in their agents' lanes; the walk's counters as the pass found them
struct RandomPass {
  uint64_t canm = 0, newm = 0, bidm = 0, dropm = 0;
  uint32_t price = 0, vol = 0, trader = 0;  // per lane
  uint32_t ev0, id0;
  __device__ __forceinline__ explicit RandomPass(const Walk& W) : ev0(W.n_ev), id0(W.next_id) {}
};

// Agent l of the pass (random_agent.rs:91-111) with the parameters P of its group (a Group) or member (a MixedDesc); `h`
// holds the pass's held ids, `pid` the pool's ids with AGENT_HELD_NONE where nothing rests (no order has that id)
template <int R, class Params>
__device__ __forceinline__ void random_agent(Walk& W, RandomPass& S, const Params& P, const uint32_t (&pid)[R], uint32_t h,
                                             uint32_t l, uint32_t trader) {
  const uint32_t x = W.rng.next_u32();  // p = gen::<f32>()  (random_agent.rs:91)
  if ((x >> 8) >= P.thr) return;        // inactive: keeps what it holds
  const uint64_t bit = 1ull << l;
  const uint32_t hl = rdl(h, l);
  uint64_t act = 0;
  if (hl != AGENT_HELD_NONE) {
#pragma unroll
    for (int r = 0; r < R; ++r) act |= __ballot(pid[r] == hl);
  }
  if (act) {  // holds an Active order: env.cancel_order (:95-97)
    if (W.n_ev < W.room) {
      S.canm |= bit;
      W.n_ev += 1;
    } else {
      S.dropm |= bit;
      W.flags |= FLAG_EVENT_OVERFLOW;
    }
    return;
  }
  // env.place_order with side, tick, vol drawn in this order (:99-111)
  const uint32_t side = W.rng.below(2u, 0x7FFFFFFFu);  // [Ask, Bid].choose: 0 = Ask, 1 = Bid
  const uint32_t tick = P.tick_lo + W.rng.below(P.tick_rng, P.tick_zone);
  const uint32_t vol = P.vol_lo + W.rng.below(P.vol_rng, P.vol_zone);
  if (W.n_ev < W.room && W.next_id < AGENT_HELD_NONE - 1u) {
    S.newm |= bit;
    S.bidm |= side ? bit : 0ull;
    S.price = wrl(tick * P.tick_size, l, S.price);
    S.vol = wrl(vol, l, S.vol);
    S.trader = wrl(trader, l, S.trader);
    W.n_ev += 1;
    W.next_id += 1;
  } else {
    S.dropm |= bit;
    W.flags |= FLAG_EVENT_OVERFLOW;
  }
}

// the pass's records, in agent order; returns what the lane's agent holds now (`h` for an inactive one).  `tag`: what a
// market's queue carries in the event word beside the kind, asset << 16 (k_ingest's layout; 0 on independent books)
__device__ __forceinline__ uint32_t random_pass_end(const Walk& W, const RandomPass& S, uint32_t h, uint32_t tag = 0u) {
  const uint32_t at = W.q0 + S.ev0 + lane_rank(S.canm | S.newm), id = S.id0 + lane_rank(S.newm);
  const bool is_new = lane_bit(S.newm), is_can = lane_bit(S.canm);
  const uint32_t bid = lane_bit(S.bidm) ? 1u : 0u;
  const uint32_t now = is_new ? id : (is_can || lane_bit(S.dropm)) ? AGENT_HELD_NONE : h;
  if (is_can) W.q[at] = make_uint4(1u | tag, h, 0u, 0u);
  if (is_new) {
    W.q[at] = make_uint4((bid << 8) | tag, id, S.price, S.vol);
    write_new_order(W.rec, id, S.vol, S.trader, S.price, bid);
  }
  return now;
}

template <int R>
__global__ __launch_bounds__(64) void k_update_agents(AgentsIngressArgs g) {
  const int lane = threadIdx.x;
  const uint32_t book = blockIdx.x;
  uint32_t* st = g.io.state + (size_t)book * g.io.state_stride;
  const uint32_t hdr = st[lane];
  uint32_t pid[R];
#pragma unroll
  for (int r = 0; r < R; ++r) pid[r] = st[HDR_DW + r * POOL_FIELDS * 64 + 2 * 64 + lane];
#pragma unroll
  for (int r = 0; r < R; ++r)
    pid[r] = sel(mk64(rdl(hdr, H_LIVE0 + 2 * r), rdl(hdr, H_LIVE0 + 2 * r + 1)), pid[r], AGENT_HELD_NONE);
  Walk W = walk_begin(g.io, book, hdr);
  uint32_t* held = g.held + (size_t)book * g.n_agents;
  const Group* gt = g.groups + (size_t)book * g.g_stride;
  uint32_t gi = 0, gbeg = 0;
  Group G = sload_group(gt);
  uint32_t gend = G.n;
  for (uint32_t base = 0; base < g.n_agents; base += 64) {
    const uint32_t n_here = min(64u, g.n_agents - base);
    const bool in = (uint32_t)lane < n_here;
    const uint32_t h = in ? held[base + lane] : AGENT_HELD_NONE;
    RandomPass S(W);
    for (uint32_t l = 0; l < n_here; ++l) {
      const uint32_t n = base + l;
      while (n >= gend) {  // groups in declaration order (a group of 0 agents is skipped)
        ++gi;
        G = sload_group(gt + gi);
        gbeg = gend;
        gend += G.n;
      }
      random_agent<R>(W, S, G, pid, h, l, n - gbeg);  // TraderId = the agent's index in its group
    }
    const uint32_t now = random_pass_end(W, S, h);
    if (in) held[base + lane] = now;
  }
  walk_end(W, g.io, st, hdr, lane);
}

}  // namespace bkd
