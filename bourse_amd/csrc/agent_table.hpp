// agent_table.hpp - agent sets as the kernels read them (plain C++17, no HIP):
//   * RandomAgents groups: the Group record, the host preprocessing of a bk_random_agents row into Group records (the
//     checks, activity_threshold, sample_zone) and the per-unit table of bk_set_random_agents_per_book;
//   * AgentSets with Noise / Momentum members: the MixedDesc record, the preprocessing of a bk_agent_desc row into
//     MixedDesc records (the checks, the thresholds, the zones and the f64 fields) and the per-unit table of
//     bk_set_agents_per_book.
// The uniform calls and the tables build their records here, so a table row is exactly what the uniform call would
// install; tests/test_per_book_table_cpu.py and tests/test_members_per_book_cpu.py check it on the CPU.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

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

// FNV-1a of n records (the checkpoint header's agent-set hash)
inline uint64_t groups_hash(const Group* g, size_t n) {
  const unsigned char* c = reinterpret_cast<const unsigned char*>(g);
  uint64_t h = 1469598103934665603ull;
  for (size_t i = 0; i < n * sizeof(Group); ++i) h = (h ^ c[i]) * 1099511628211ull;
  return h;
}

// One row of groups: n_groups records into out[0 .. n_groups), their agents into *total.  asset_tick: the M books' tick
// sizes; assets: the group's book of the market (null: all 0).  Returns BK_OK or the status of the first failing group,
// with its message in *msg (prefixed by `where`).  Capacity against max_live_orders is the caller's check.
inline int make_groups(const bk_random_agents* rows, uint32_t n_groups, const uint32_t* assets, uint32_t M,
                       const uint32_t* asset_tick, Group* out, uint64_t* total, std::string* msg,
                       const std::string& where = std::string()) {
  *total = 0;
  auto fail = [&](int code, uint32_t g, const char* m) {
    *msg = where.empty() ? std::string(m) : where + "group " + std::to_string(g) + ": " + m;
    return code;
  };
  for (uint32_t g = 0; g < n_groups; ++g) {
    const bk_random_agents& r = rows[g];
    if (r.tick_lo >= r.tick_hi || r.vol_lo >= r.vol_hi)
      return fail(BK_INVALID_ARGUMENT, g, "empty tick/vol range");  // gen_range asserts low < high
    // every sampled price tick * tick_size must pass create_order's tick check (else `.unwrap()` panics,
    // random_agent.rs:103-110)
    const uint32_t asset = assets ? assets[g] : 0u;
    if (asset >= M) return fail(BK_INVALID_ARGUMENT, g, "group asset index out of range");
    if (r.tick_size % asset_tick[asset] != 0)
      return fail(BK_PRICE_NOT_TICK_MULTIPLE, g, "agent tick_size must be a multiple of the env tick_size");
    if (static_cast<uint64_t>(r.tick_hi - 1) * r.tick_size >= 0xFFFFFFFFull || r.tick_lo == 0)
      return fail(BK_INVALID_ARGUMENT, g, "limit prices must lie in (0, u32::MAX)");
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
    *total += r.n_agents;
    out[g] = G;
  }
  return BK_OK;
}

constexpr const char* CAPACITY_MSG = "sum of n_agents exceeds max_live_orders (one pool slot per agent)";

// The per-unit table: rows[u * n_groups + g] is group g of unit u < n_units.  Every row is checked as make_groups checks
// one (the message names the unit and the group), n_agents must be the same in every unit (the pool layout is shared),
// and the agents of a unit must fit max_live_orders.  On success `out` holds n_units x n_groups records, unit-major.
inline int make_group_table(const bk_random_agents* rows, uint32_t n_units, uint32_t n_groups, const uint32_t* assets,
                            uint32_t M, const uint32_t* asset_tick, uint32_t max_live_orders, std::vector<Group>& out,
                            uint64_t* total, std::string* msg) {
  std::vector<Group> t(static_cast<size_t>(n_units) * n_groups);
  *total = 0;
  for (uint32_t u = 0; u < n_units; ++u) {
    const std::string where = "unit " + std::to_string(u) + ", ";
    uint64_t tot = 0;
    const size_t row = static_cast<size_t>(u) * n_groups;
    if (int rc = make_groups(rows + row, n_groups, assets, M, asset_tick, t.data() + row, &tot, msg, where)) return rc;
    for (uint32_t g = 0; g < n_groups; ++g)
      if (t[row + g].n != t[g].n) {
        *msg = where + "group " + std::to_string(g) + ": n_agents differs from unit 0's (every unit shares the pool layout)";
        return BK_INVALID_ARGUMENT;
      }
    if (tot > max_live_orders) {
      *msg = where + CAPACITY_MSG;
      return BK_CAPACITY;
    }
    *total = tot;
  }
  out.swap(t);
  return BK_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// AgentSets with Noise / Momentum members (mixed_agents.hpp, wave_mixed.hpp)
constexpr int MAX_MEMBERS = 4;
// ... and on an env with the device ingress, whose update kernels (members_ingress.hpp, market_ingress.hpp) walk the
// members row by row and keep nothing per member in registers: bk_run's kernels, which hold MAX_MEMBERS, never run there
constexpr int MAX_INGRESS_MEMBERS = 8;
constexpr int MAX_ASSETS = 8;  // books per market (MarketEnv<ASSETS>)

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

// FNV-1a over bytes, continuing from h
inline uint64_t fnv1a_bytes(const void* p, size_t n, uint64_t h = 1469598103934665603ull) {
  const unsigned char* c = static_cast<const unsigned char*>(p);
  for (size_t i = 0; i < n; ++i) h = (h ^ c[i]) * 1099511628211ull;
  return h;
}
// the checkpoint header's agent-set hash of n MixedDesc records and the members' assets (member_asset[MAX_MEMBERS])
// (member_asset[MAX_INGRESS_MEMBERS]; the assets of members beyond MAX_MEMBERS are hashed only where there are such members)
inline uint64_t mixed_hash(const uint32_t* member_asset, const MixedDesc* d, size_t n, uint32_t n_members = 0) {
  uint64_t h = fnv1a_bytes(member_asset, MAX_MEMBERS * sizeof(uint32_t), fnv1a_bytes(d, n * sizeof(MixedDesc)));
  if (n_members > static_cast<uint32_t>(MAX_MEMBERS))
    h = fnv1a_bytes(member_asset + MAX_MEMBERS, (MAX_INGRESS_MEMBERS - MAX_MEMBERS) * sizeof(uint32_t), h);
  return h;
}

// One row of members: n_members records into out[0 .. n_members), the fixed RandomAgents slots of each asset's books into
// fixed_a[MAX_ASSETS] (zeroed here).  asset_tick: the M books' tick sizes; assets: the member's book of the market (null:
// all 0; the caller checks them against M).  Returns BK_OK or the status of the first failing member, with its message in
// *msg (prefixed by `where`).  Capacity against max_live_orders is the caller's check (mixed_capacity_ok).
inline int make_mixed_descs(const bk_agent_desc* members, uint32_t n_members, const uint32_t* assets,
                            const uint32_t* asset_tick, MixedDesc* out, uint32_t* fixed_a, std::string* msg,
                            const std::string& where = std::string()) {
  for (int as = 0; as < MAX_ASSETS; ++as) fixed_a[as] = 0;
  auto fail = [&](int code, uint32_t i, const char* m) {
    *msg = where.empty() ? std::string(m) : where + "member " + std::to_string(i) + ": " + m;
    return code;
  };
  for (uint32_t i = 0; i < n_members; ++i) {
    const uint32_t as = assets ? assets[i] : 0u;
    uint32_t& fixed = fixed_a[as];  // fixed RandomAgents slots are counted per book
    const bk_agent_desc& m = members[i];
    MixedDesc D;
    std::memset(&D, 0, sizeof(D));
    D.type = m.type;
    D.n = m.n_agents;
    if (m.tick_size == 0 || m.tick_size % asset_tick[as] != 0)
      return fail(BK_PRICE_NOT_TICK_MULTIPLE, i, "member tick_size must be a non-zero multiple of the env tick_size");
    if (m.type == BK_AGENT_RANDOM) {
      if (m.tick_lo >= m.tick_hi || m.vol_lo >= m.vol_hi || m.tick_lo == 0 ||
          static_cast<uint64_t>(m.tick_hi - 1) * m.tick_size >= 0xFFFFFFFFull)
        return fail(BK_INVALID_ARGUMENT, i, "bad RandomAgents ranges");
      D.thr = activity_threshold(m.activity_rate);
      D.tick_lo = m.tick_lo;
      D.tick_rng = m.tick_hi - m.tick_lo;
      D.tick_zone = sample_zone(D.tick_rng);
      D.vol_lo = m.vol_lo;
      D.vol_rng = m.vol_hi - m.vol_lo;
      D.vol_zone = sample_zone(D.vol_rng);
      D.tick_size = m.tick_size;
      D.slot_base = fixed;
      fixed += m.n_agents;
    } else if (m.type == BK_AGENT_NOISE || m.type == BK_AGENT_MOMENTUM) {
      if (m.n_agents > 0xFFFFu) return fail(BK_INVALID_ARGUMENT, i, "n_agents is a u16 in the reference");
      if (!(m.price_dist_sigma >= 0.0) || !std::isfinite(m.price_dist_sigma) || !std::isfinite(m.price_dist_mu))
        return fail(BK_INVALID_ARGUMENT, i, "LogNormal::new(mu, sigma) needs finite mu and sigma >= 0");  // .unwrap()
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
      return fail(BK_INVALID_ARGUMENT, i, "unknown agent type");
    }
    out[i] = D;
  }
  return BK_OK;
}

constexpr const char* MIXED_CAPACITY_MSG = "RandomAgents members leave no pool slots for the other members' orders";
inline bool mixed_capacity_ok(const uint32_t* fixed_a, uint32_t M, uint32_t max_live_orders) {
  for (uint32_t as = 0; as < M; ++as)
    if (fixed_a[as] >= max_live_orders) return false;
  return true;
}

// The per-unit table: members[u * n_members + i] is member i of unit u < n_units.  Every row is checked as
// make_mixed_descs checks one (the message names the unit and the member); type and n_agents must be the same in every
// unit (the members' kinds, loop lengths and pool layout are shared; the assets are one array for all units).  On success
// `out` holds n_units x n_members records, unit-major, and fixed_a the fixed slots every unit shares.
inline int make_mixed_table(const bk_agent_desc* members, uint32_t n_units, uint32_t n_members, const uint32_t* assets,
                            uint32_t M, const uint32_t* asset_tick, uint32_t max_live_orders, std::vector<MixedDesc>& out,
                            uint32_t* fixed_a, std::string* msg) {
  std::vector<MixedDesc> t(static_cast<size_t>(n_units) * n_members);
  for (uint32_t u = 0; u < n_units; ++u) {
    const std::string where = "unit " + std::to_string(u) + ", ";
    const size_t row = static_cast<size_t>(u) * n_members;
    if (int rc = make_mixed_descs(members + row, n_members, assets, asset_tick, t.data() + row, fixed_a, msg, where))
      return rc;
    for (uint32_t i = 0; i < n_members; ++i) {
      const char* what = t[row + i].type != t[i].type ? "type differs from unit 0's"
                         : t[row + i].n != t[i].n   ? "n_agents differs from unit 0's"
                                                    : nullptr;
      if (what) {
        *msg = where + "member " + std::to_string(i) + ": " + what + " (every unit shares the members' kinds and pool layout)";
        return BK_INVALID_ARGUMENT;
      }
    }
  }
  if (!mixed_capacity_ok(fixed_a, M, max_live_orders)) {
    *msg = std::string("unit 0, ") + MIXED_CAPACITY_MSG;
    return BK_CAPACITY;
  }
  out.swap(t);
  return BK_OK;
}

}  // namespace bkd
