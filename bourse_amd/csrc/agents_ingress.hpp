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
//     register, masked by the live bits of the header.  An order queued earlier in the same step is New (not yet in the
//     pool); a filled or cancelled order has left it - the order log is not read;
//   * the pass's events go to the queue in agent order, compacted with mbcnt, with k_ingest's records and log entries
//     (immutable half, status New, provisional key, the book's clock as arrival time); the RNG words, H_NEXT_ID, the flags
//     and the queue length are written once per book.
// Capacity: an event beyond the queue's room, or a New order once the u32 id space is exhausted, is dropped and the book
// flagged FLAG_EVENT_OVERFLOW (the draws are taken all the same; a dropped New consumes no id).  The agent then holds None.
#pragma once

namespace bkd {

constexpr uint32_t AGENT_HELD_NONE = 0xFFFFFFFFu;

struct AgentsIngressArgs {
  uint32_t* state;
  uint32_t state_stride, n_agents, log_cap, qcap;
  const Group* groups;   // group g of book b: groups[b * g_stride + g] (the per-book table; g_stride 0 = one row for all)
  uint32_t g_stride;
  uint32_t* held;        // [n_books][n_agents] held order ids
  uint4* q;              // [n_books][qcap] event records (k_ingest's layout)
  uint32_t* qlen;        // [n_books]
  uint4* dorders;        // [n_books][log_cap][2] immutable halves
  DevOrderLog* order_log;
};

template <int R>
__global__ __launch_bounds__(64) void k_update_agents(AgentsIngressArgs g) {
  const int lane = threadIdx.x;
  const uint32_t book = blockIdx.x;
  uint32_t* st = g.state + (size_t)book * g.state_stride;
  const uint32_t hdr = st[lane];
  uint32_t pid[R];
#pragma unroll
  for (int r = 0; r < R; ++r) pid[r] = st[HDR_DW + r * POOL_FIELDS * 64 + 2 * 64 + lane];
  uint64_t live[R];
#pragma unroll
  for (int r = 0; r < R; ++r) live[r] = mk64(rdl(hdr, H_LIVE0 + 2 * r), rdl(hdr, H_LIVE0 + 2 * r + 1));
  Rng rng;
  rng.s0 = mk64(rdl(hdr, H_S0_LO), rdl(hdr, H_S0_HI));
  rng.s1 = mk64(rdl(hdr, H_S1_LO), rdl(hdr, H_S1_HI));
  uint32_t next_id = rdl(hdr, H_NEXT_ID), flags = rdl(hdr, H_FLAGS);
  const uint32_t t_lo = rdl(hdr, H_T_LO), t_hi = rdl(hdr, H_T_HI);
  const uint32_t q0 = rfl(g.qlen[book]);
  const uint32_t room = g.qcap > q0 ? g.qcap - q0 : 0u;
  uint4* q = g.q + (size_t)book * g.qcap;
  uint32_t* held = g.held + (size_t)book * g.n_agents;
  const Group* gt = g.groups + (size_t)book * g.g_stride;
  uint32_t n_ev = 0;  // events this call queued
  uint32_t gi = 0, gbeg = 0;
  Group G = sload_group(gt);
  uint32_t gend = G.n;
  for (uint32_t base = 0; base < g.n_agents; base += 64) {
    const uint32_t n_here = min(64u, g.n_agents - base);
    const bool in = (uint32_t)lane < n_here;
    const uint32_t h = in ? held[base + lane] : AGENT_HELD_NONE;
    const uint32_t ev0 = n_ev, id0 = next_id;
    uint64_t canm = 0, newm = 0, bidm = 0, dropm = 0;
    uint32_t e_price = 0, e_vol = 0, e_trader = 0;
    for (uint32_t l = 0; l < n_here; ++l) {
      const uint32_t n = base + l;
      while (n >= gend) {  // groups in declaration order (a group of 0 agents is skipped)
        ++gi;
        G = sload_group(gt + gi);
        gbeg = gend;
        gend += G.n;
      }
      const uint32_t x = rng.next_u32();  // p = gen::<f32>()  (random_agent.rs:91)
      if ((x >> 8) >= G.thr) continue;    // inactive: keeps what it holds
      const uint64_t bit = 1ull << l;
      const uint32_t hl = rdl(h, l);
      uint64_t act = 0;
      if (hl != AGENT_HELD_NONE) {
#pragma unroll
        for (int r = 0; r < R; ++r) act |= __ballot(pid[r] == hl) & live[r];
      }
      if (act) {  // holds an Active order: env.cancel_order (:95-97)
        if (n_ev < room) {
          canm |= bit;
          n_ev += 1;
        } else {
          dropm |= bit;
          flags |= FLAG_EVENT_OVERFLOW;
        }
        continue;
      }
      // env.place_order with side, tick, vol drawn in this order (:99-111)
      const uint32_t side = rng.below(2u, 0x7FFFFFFFu);  // [Ask, Bid].choose: 0 = Ask, 1 = Bid
      const uint32_t tick = G.tick_lo + rng.below(G.tick_rng, G.tick_zone);
      const uint32_t vol = G.vol_lo + rng.below(G.vol_rng, G.vol_zone);
      if (n_ev < room && next_id < AGENT_HELD_NONE - 1u) {
        newm |= bit;
        bidm |= side ? bit : 0ull;
        e_price = wrl(tick * G.tick_size, l, e_price);
        e_vol = wrl(vol, l, e_vol);
        e_trader = wrl(n - gbeg, l, e_trader);  // TraderId = the agent's index in its group
        n_ev += 1;
        next_id += 1;
      } else {
        dropm |= bit;
        flags |= FLAG_EVENT_OVERFLOW;
      }
    }
    // the pass's records, in agent order
    const uint64_t evm = canm | newm;
    const uint32_t rank_ev = __builtin_amdgcn_mbcnt_hi((uint32_t)(evm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)evm, 0u));
    const uint32_t rank_new = __builtin_amdgcn_mbcnt_hi((uint32_t)(newm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)newm, 0u));
    const bool is_new = lane_bit(newm), is_can = lane_bit(canm);
    const uint32_t id = id0 + rank_new;
    const uint32_t bid = lane_bit(bidm) ? 1u : 0u;
    if (is_can) q[q0 + ev0 + rank_ev] = make_uint4(1u, h, 0u, 0u);
    if (is_new) {
      q[q0 + ev0 + rank_ev] = make_uint4(bid << 8, id, e_price, e_vol);
      if (id < g.log_cap) {
        uint4* d = g.dorders + ((size_t)book * g.log_cap + id) * 2;
        d[0] = make_uint4(e_vol, e_trader, e_price, bid);
        d[1] = make_uint4(t_lo, t_hi, 0u, 0u);
        // initial order-log entry: status New, nothing traded, provisional key (price, 0) (orderbook.rs:388-391)
        uint4* lg = reinterpret_cast<uint4*>(g.order_log + (size_t)book * g.log_cap + id);
        lg[0] = make_uint4(0u, e_vol, e_price, e_price);
        lg[1] = make_uint4(t_lo, t_hi, 0xFFFFFFFFu, 0xFFFFFFFFu);
        lg[2] = make_uint4(0u, 0u, 0u, 0u);
      }
    }
    if (in) held[base + lane] = is_new ? id : (is_can || lane_bit(dropm)) ? AGENT_HELD_NONE : h;
  }
  // the header words this call changed: the RNG, the id counter, the flags; then the queue's length
  uint32_t w = hdr;
  w = wrl((uint32_t)rng.s0, H_S0_LO, w);
  w = wrl((uint32_t)(rng.s0 >> 32), H_S0_HI, w);
  w = wrl((uint32_t)rng.s1, H_S1_LO, w);
  w = wrl((uint32_t)(rng.s1 >> 32), H_S1_HI, w);
  w = wrl(next_id, H_NEXT_ID, w);
  w = wrl(flags, H_FLAGS, w);
  if ((lane >= H_S0_LO && lane <= H_NEXT_ID) || lane == H_FLAGS) st[lane] = w;
  if (lane == 0) g.qlen[book] = q0 + n_ev;
}

}  // namespace bkd
