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
#include "agent_rows.hpp"  // Group, MixedDesc and the checks and arithmetic of one entry (shared with retune.hpp)
#include "host_math.hpp"

namespace bkd {

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
    const uint32_t asset = assets ? assets[g] : 0u;
    Group G;
    uint32_t why = 0;
    if (int rc = agent_rows::group_row(r, asset, asset < M ? asset_tick[asset] : 0u, &G, &why)) {  // (agent_rows.hpp)
      const char* m = why == agent_rows::WHY_EMPTY_RANGE     ? "empty tick/vol range"
                      : why == agent_rows::WHY_ASSET         ? "group asset index out of range"
                      : why == agent_rows::WHY_TICK_MULTIPLE ? "agent tick_size must be a multiple of the env tick_size"
                                                       : "limit prices must lie in (0, u32::MAX)";
      return fail(rc, g, m);
    }
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
    uint32_t why = 0;
    if (int rc = agent_rows::mixed_row(m, asset_tick[as], fixed, &D, &why)) {  // (agent_rows.hpp)
      const char* t = why == agent_rows::WHY_TICK_MULTIPLE   ? "member tick_size must be a non-zero multiple of the env tick_size"
                      : why == agent_rows::WHY_RANDOM_RANGES ? "bad RandomAgents ranges"
                      : why == agent_rows::WHY_N_U16         ? "n_agents is a u16 in the reference"
                      : why == agent_rows::WHY_LOGNORMAL     ? "LogNormal::new(mu, sigma) needs finite mu and sigma >= 0"
                                                       : "unknown agent type";
      return fail(rc, i, t);
    }
    if (m.type == BK_AGENT_RANDOM) fixed += m.n_agents;
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
