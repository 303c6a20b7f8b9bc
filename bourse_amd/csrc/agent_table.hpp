// agent_table.hpp - RandomAgents groups as the kernels read them (plain C++17, no HIP): the Group record, the host
// preprocessing of a bk_random_agents row into Group records (the checks, activity_threshold, sample_zone) and the
// per-unit table of bk_set_random_agents_per_book.  bk_set_random_market_agents and bk_set_random_agents_per_book both
// build their records here, so a table row is exactly what the uniform call would install;
// tests/test_per_book_table_cpu.py checks it on the CPU.
#pragma once
#include <cstdint>
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

}  // namespace bkd
