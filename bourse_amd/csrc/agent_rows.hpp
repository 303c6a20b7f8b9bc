// agent_rows.hpp - ONE entry of an agent table: a bk_random_agents into a Group record, a bk_agent_desc into a MixedDesc
// record, each with the install's checks and the install's status code.  One text for the host installs
// (agent_table.hpp make_groups / make_mixed_descs), the host retunes (bk_retune_random_agents / bk_retune_agents) and the
// retune kernels (retune.hpp): under hipcc it compiles for both sides (BKD_HOST_DEVICE, host_math.hpp).  Plain C++17, no
// HIP; tests/cpp/agent_rows_test.cpp compiles it with g++ against the table builders.
//
// The thresholds go through double: ceil / floor of a float times 2^24 are exact there, on the device as on the host.
#pragma once
#include <cstdint>

#include "../../include/bourse_amd.h"
#include "host_math.hpp"

namespace bkd {

struct Group {  // RandomAgents::new, host-preprocessed
  uint32_t n;          // agents in the group
  uint32_t thr;        // activity: (u32 >> 8) < thr  <=>  f32 draw < activity_rate (exact, see host)
  uint32_t tick_lo, tick_rng, tick_zone;
  uint32_t vol_lo, vol_rng, vol_zone;
  uint32_t tick_size;  // the agents' tick size
  uint32_t asset;      // RandomMarketAgents: the asset (book of the market) the group trades
  uint32_t pad[2];
};
static_assert(sizeof(Group) == 48, "Group: 48-byte records (the per-unit table is read as three 16-byte loads)");

struct MixedDesc {
  uint32_t type;  // 0 RandomAgents, 1 NoiseAgent, 2 MomentumAgent
  uint32_t n;
  uint32_t thr, tick_lo, tick_rng, tick_zone, vol_lo, vol_rng, vol_zone, tick_size;  // RandomAgents (see Group)
  uint32_t thr_limit, thr_market;  // NoiseAgent: (u32 >> 8) < thr  <=>  gen::<f32>() < p
  int32_t keep_thr;                // cancel_live_orders keeps an order iff (u32 >> 8) > keep_thr  <=>  gen::<f32>() > p_cancel
  uint32_t trade_vol;
  uint32_t slot_base;              // RandomAgents: first fixed slot
  uint32_t pad;
  double mu, sigma, decay, demand, scale, order_ratio, n_f, tick_f;
};
static_assert(sizeof(MixedDesc) == 128, "MixedDesc layout");

static_assert(sizeof(bk_random_agents) == 28, "bk_random_agents: 28-byte rows (RANDOM_AGENTS_DTYPE)");
static_assert(sizeof(bk_agent_desc) == 104, "bk_agent_desc: 104-byte rows (AGENT_DESC_DTYPE)");

namespace agent_rows {

// why an entry was refused (the installs turn it into their message; the kernels report the status alone)
enum Why : uint32_t {
  WHY_NONE = 0,
  WHY_EMPTY_RANGE,    // group: tick_lo >= tick_hi or vol_lo >= vol_hi
  WHY_ASSET,          // group: its asset is no book of the market
  WHY_TICK_MULTIPLE,  // tick_size no (non-zero) multiple of the asset's tick
  WHY_PRICE_BOUND,    // group: tick_lo == 0 or (tick_hi - 1) * tick_size >= u32::MAX
  WHY_RANDOM_RANGES,  // RandomAgents member: any of the range checks
  WHY_N_U16,          // Noise / Momentum: n_agents is a u16 in the reference
  WHY_LOGNORMAL,      // Noise / Momentum: LogNormal::new(mu, sigma) needs finite mu and sigma >= 0
  WHY_TYPE,           // unknown agent type
};

BKD_HOST_DEVICE inline bool finite_f64(double x) { return __builtin_isfinite(x); }

// One RandomAgents group.  asset_tick: the tick size of the asset's book, or 0 when the asset is no book of the market
// (no book has tick 0: bk_env_create and bk_set_tick_sizes refuse it).  On BK_OK *out is the whole record.
BKD_HOST_DEVICE inline int group_row(const bk_random_agents& r, uint32_t asset, uint32_t asset_tick, Group* out,
                                     uint32_t* why) {
  if (r.tick_lo >= r.tick_hi || r.vol_lo >= r.vol_hi) {  // gen_range asserts low < high
    *why = WHY_EMPTY_RANGE;
    return BK_INVALID_ARGUMENT;
  }
  if (asset_tick == 0) {
    *why = WHY_ASSET;
    return BK_INVALID_ARGUMENT;
  }
  // every sampled price tick * tick_size must pass create_order's tick check (else `.unwrap()` panics,
  // random_agent.rs:103-110)
  if (r.tick_size % asset_tick != 0) {
    *why = WHY_TICK_MULTIPLE;
    return BK_PRICE_NOT_TICK_MULTIPLE;
  }
  if (static_cast<uint64_t>(r.tick_hi - 1) * r.tick_size >= 0xFFFFFFFFull || r.tick_lo == 0) {
    *why = WHY_PRICE_BOUND;
    return BK_INVALID_ARGUMENT;
  }
  Group G{};
  G.n = r.n_agents;
  G.thr = activity_threshold(r.activity_rate);
  G.tick_lo = r.tick_lo;
  G.tick_rng = r.tick_hi - r.tick_lo;
  G.tick_zone = sample_zone(G.tick_rng);
  G.vol_lo = r.vol_lo;
  G.vol_rng = r.vol_hi - r.vol_lo;
  G.vol_zone = sample_zone(G.vol_rng);
  G.tick_size = r.tick_size;
  G.asset = asset;
  *out = G;
  *why = WHY_NONE;
  return BK_OK;
}

// One member of an AgentSet.  asset_tick: the tick size of the member's book; slot_base: the fixed RandomAgents slots the
// members before it take on that book (what a RandomAgents member's record holds).  On BK_OK *out is the whole record.
BKD_HOST_DEVICE inline int mixed_row(const bk_agent_desc& m, uint32_t asset_tick, uint32_t slot_base, MixedDesc* out,
                                     uint32_t* why) {
  MixedDesc D{};
  D.type = m.type;
  D.n = m.n_agents;
  if (m.tick_size == 0 || m.tick_size % asset_tick != 0) {
    *why = WHY_TICK_MULTIPLE;
    return BK_PRICE_NOT_TICK_MULTIPLE;
  }
  if (m.type == BK_AGENT_RANDOM) {
    if (m.tick_lo >= m.tick_hi || m.vol_lo >= m.vol_hi || m.tick_lo == 0 ||
        static_cast<uint64_t>(m.tick_hi - 1) * m.tick_size >= 0xFFFFFFFFull) {
      *why = WHY_RANDOM_RANGES;
      return BK_INVALID_ARGUMENT;
    }
    D.thr = activity_threshold(m.activity_rate);
    D.tick_lo = m.tick_lo;
    D.tick_rng = m.tick_hi - m.tick_lo;
    D.tick_zone = sample_zone(D.tick_rng);
    D.vol_lo = m.vol_lo;
    D.vol_rng = m.vol_hi - m.vol_lo;
    D.vol_zone = sample_zone(D.vol_rng);
    D.tick_size = m.tick_size;
    D.slot_base = slot_base;
  } else if (m.type == BK_AGENT_NOISE || m.type == BK_AGENT_MOMENTUM) {
    if (m.n_agents > 0xFFFFu) {
      *why = WHY_N_U16;
      return BK_INVALID_ARGUMENT;
    }
    if (!(m.price_dist_sigma >= 0.0) || !finite_f64(m.price_dist_sigma) || !finite_f64(m.price_dist_mu)) {  // .unwrap()
      *why = WHY_LOGNORMAL;
      return BK_INVALID_ARGUMENT;
    }
    D.thr_limit = activity_threshold(m.p_limit);
    D.thr_market = activity_threshold(m.p_market);
    D.keep_thr = keep_threshold(m.p_cancel);
    D.trade_vol = m.trade_vol;
    D.mu = m.price_dist_mu;
    D.sigma = m.price_dist_sigma;
    D.decay = m.decay;
    D.demand = m.demand;
    D.scale = m.scale;
    D.order_ratio = m.order_ratio;
    D.n_f = static_cast<double>(m.n_agents);
    D.tick_f = static_cast<double>(m.tick_size);
  } else {
    *why = WHY_TYPE;
    return BK_INVALID_ARGUMENT;
  }
  *out = D;
  *why = WHY_NONE;
  return BK_OK;
}

// ---- a retune's further checks: the fields the pool layout, the kernels' loop lengths and the trader ids depend on stay
// what the install wrote.  `cur`: the installed record.  Run after the install's checks, on an entry that passed them.
BKD_HOST_DEVICE inline int group_fixed_ok(const Group& next, const Group& cur) {
  return next.n == cur.n ? BK_OK : BK_INVALID_ARGUMENT;
}
BKD_HOST_DEVICE inline int mixed_fixed_ok(const MixedDesc& next, const MixedDesc& cur, uint32_t id_start,
                                          uint32_t installed_id_start) {
  return next.type == cur.type && next.n == cur.n && id_start == installed_id_start ? BK_OK : BK_INVALID_ARGUMENT;
}

}  // namespace agent_rows
}  // namespace bkd
