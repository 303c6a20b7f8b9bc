// market_walk.hpp - the pass schedule of RandomMarketAgents::update (random_agent.rs:204-245) on one market.
//
// Compiled by the device update (market_ingress.hpp) and by a CPU test (tests/cpp/market_walk_test.cpp): no HIP type, no
// intrinsic.  The groups of a market are walked in declaration order, their agents numbered 0 .. sum(n) - 1 across the
// groups; a PASS is up to 64 consecutive agents that trade the same asset, agent `first + l` in lane l.  One pass serves
// one book only (its new ids are numbered from one counter), so a pass ends
//   * after 64 agents, or
//   * where the next agent belongs to a group of another asset (a group of 0 agents has no agent and ends nothing), or
//   * with the last agent.
// A pass may hold several groups of one asset; the trader id of an agent is its index in its group, so the pass carries
// the group of its first agent and that agent's index in it, and whoever walks the pass moves on to the next non-empty
// group where the index reaches the group's size.  Groups may return to an asset an earlier pass has served.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BKD_WALK_HD __host__ __device__ inline
#else
#define BKD_WALK_HD inline
#endif

namespace bkd {
namespace ingress {

constexpr uint32_t PASS_AGENTS = 64;  // one agent per lane

struct MarketPass {
  uint32_t first;    // the pass's first agent (its number across the groups)
  uint32_t len;      // 1 .. 64 agents
  uint32_t asset;    // the book of the market all of them trade
  uint32_t trader0;  // the first agent's index in its group
  uint32_t group;    // ... and that group
};

// where the walk stands: the next agent, the group it is looked for in and that group's first agent
struct PassCursor {
  uint32_t next = 0, group = 0, gbeg = 0;
};

// The next pass of a row of n_groups groups, group g with n_of(g) agents on asset asset_of(g); false once every agent
// has been served.  Both functions are called with g < n_groups only.
template <class SizeOf, class AssetOf>
BKD_WALK_HD bool next_pass(PassCursor& c, uint32_t n_groups, SizeOf n_of, AssetOf asset_of, MarketPass& p) {
  while (c.group < n_groups && c.next >= c.gbeg + n_of(c.group)) {
    c.gbeg += n_of(c.group);
    c.group += 1;
  }
  if (c.group >= n_groups) return false;
  p.first = c.next;
  p.group = c.group;
  p.trader0 = c.next - c.gbeg;
  p.asset = asset_of(c.group);
  p.len = 0;
  uint32_t g = c.group, gend = c.gbeg + n_of(c.group);
  for (;;) {
    const uint32_t left = gend - (p.first + p.len), want = PASS_AGENTS - p.len;
    p.len += left < want ? left : want;
    if (p.len == PASS_AGENTS) break;
    do ++g; while (g < n_groups && n_of(g) == 0);  // the next group that has an agent
    if (g >= n_groups || asset_of(g) != p.asset) break;
    gend += n_of(g);
  }
  c.next = p.first + p.len;
  return true;
}

}  // namespace ingress
}  // namespace bkd
