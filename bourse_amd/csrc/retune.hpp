// retune.hpp - bk_retune_*: the parameter records of chosen units of the installed per-unit table, rewritten in place on
// the device.  The reference's counterpart is an assignment to the fields of a unit's agent objects between
// two `update` calls; here the records are what every PB kernel reads at its next launch, so one small kernel on the env's
// stream is the whole of it.  Nothing but the records is touched: books, RNG states, held ids, member lists and momentum
// state stay.
//   * eight lanes per unit, eight units per wave: lane 8 i + j holds entry j (group / member) of the wave's unit i
//     (MAX_GROUPS = MAX_INGRESS_MEMBERS = 8); UNITS_PER_BLOCK units per block;
//   * a lane loads its input row and the installed record's fixed fields (n, asset / type, slot_base, and the installed
//     first trader id of a member) and builds the record in registers with the install's own text (agent_rows.hpp);
//   * the unit's verdict is its byte of one ballot of "failed"; the first failing entry is the byte's lowest set bit, and
//     that lane - which holds the status - writes the unit's status pair {code, entry};
//   * a unit whose byte is clear is applied: every lane stores its record as 16-byte vectors (3 per Group, 8 per
//     MixedDesc); a unit with any failing entry keeps its whole row;
//   * refused units are counted with one atomic add per wave, by one lane; idle lanes (entry >= width, unit >= n_units,
//     mask clear) load and store nothing, but entry 0 of an unmasked unit writes its {BK_OK, 0}.
// Plain C++ and builtins, no LDS, no scratch, vector stores only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "agent_rows.hpp"
#include "book_device.hpp"

namespace bkd {
namespace retune {

constexpr int WAVES = 4;                          // waves per block
constexpr uint32_t UNITS_PER_BLOCK = WAVES * 8u;  // 8 lanes per unit
constexpr uint32_t WIDTH = 8;                     // entries per unit at most

struct Args {
  const void* rows;     // [n_units][width] bk_random_agents / bk_agent_desc
  void* table;          // [n_units][width] Group / MixedDesc: the installed per-unit table
  const uint8_t* mask;  // [n_units]; nullptr: every unit
  uint32_t* status;     // [n_units][2] {bk_status, first failing entry}; nullptr: not reported
  unsigned long long* rejected;  // the env's count of refused units
  const uint32_t* id_start;      // members: [n_units][width] the installed first trader ids
  uint32_t n_units, width;
  uint32_t asset_tick[8];  // the tick size of every asset's book
  uint64_t member_assets;  // members: byte j = member j's asset
};

// the tick of `asset` (< 8) without an indexed read of the kernel arguments (which would go through scratch)
__device__ __forceinline__ uint32_t tick_of(const Args& g, uint32_t asset) {
  uint32_t t = g.asset_tick[0];
#pragma unroll
  for (uint32_t k = 1; k < 8; ++k) t = asset == k ? g.asset_tick[k] : t;
  return t;
}

// the verdicts of one wave: the status pairs and the count of refused units.  Returns whether this lane's unit is applied.
__device__ __forceinline__ bool verdict(const Args& g, uint32_t lane, uint32_t unit, bool live, bool chosen, int st) {
  const uint32_t i = lane >> 3, j = lane & 7u;
  const unsigned long long failed = __ballot(live && st != BK_OK);
  const uint32_t byte = static_cast<uint32_t>(failed >> (8u * i)) & 0xFFu;
  const uint32_t first = byte ? static_cast<uint32_t>(__builtin_ctz(byte)) : 0u;
  if (g.status && unit < g.n_units) {
    if (byte ? j == first : j == 0u) {  // (an unmasked unit's byte is clear: {BK_OK, 0})
      uint32_t* s = g.status + static_cast<size_t>(unit) * 2;
      s[0] = byte ? static_cast<uint32_t>(st) : static_cast<uint32_t>(BK_OK);
      s[1] = first;
    }
  }
  unsigned long long m = failed;  // one bit per refused unit
  m |= m >> 4;
  m |= m >> 2;
  m |= m >> 1;
  m &= 0x0101010101010101ull;
  if (m != 0ull && lane == 0u) atomicAdd(g.rejected, static_cast<unsigned long long>(__builtin_popcountll(m)));
  return chosen && byte == 0u;
}

__global__ __launch_bounds__(64 * WAVES) void k_groups(Args g) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t unit = blockIdx.x * UNITS_PER_BLOCK + (threadIdx.x >> 3);
  const uint32_t j = lane & 7u;
  const bool chosen = unit < g.n_units && (!g.mask || g.mask[unit] != 0);
  const bool live = chosen && j < g.width;
  const size_t e = static_cast<size_t>(unit) * g.width + j;
  uint4* rec = reinterpret_cast<uint4*>(static_cast<Group*>(g.table) + e);
  Group G{};
  int st = BK_OK;
  if (live) {
    const bk_random_agents r = static_cast<const bk_random_agents*>(g.rows)[e];
    const uint4 c0 = rec[0];  // {n, thr, tick_lo, tick_rng}
    const uint4 c2 = rec[2];  // {tick_size, asset, pad, pad}
    Group cur{};
    cur.n = c0.x;
    cur.asset = c2.y;
    uint32_t why;
    st = agent_rows::group_row(r, cur.asset, tick_of(g, cur.asset & 7u), &G, &why);
    if (st == BK_OK) st = agent_rows::group_fixed_ok(G, cur);
  }
  if (verdict(g, lane, unit, live, chosen, st) && live) {
    rec[0] = make_uint4(G.n, G.thr, G.tick_lo, G.tick_rng);
    rec[1] = make_uint4(G.tick_zone, G.vol_lo, G.vol_rng, G.vol_zone);
    rec[2] = make_uint4(G.tick_size, G.asset, 0u, 0u);
  }
}

__device__ __forceinline__ uint4 pack(double a, double b) {
  const unsigned long long x = static_cast<unsigned long long>(__double_as_longlong(a));
  const unsigned long long y = static_cast<unsigned long long>(__double_as_longlong(b));
  return make_uint4(static_cast<uint32_t>(x), static_cast<uint32_t>(x >> 32), static_cast<uint32_t>(y),
                    static_cast<uint32_t>(y >> 32));
}

__global__ __launch_bounds__(64 * WAVES) void k_members(Args g) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t unit = blockIdx.x * UNITS_PER_BLOCK + (threadIdx.x >> 3);
  const uint32_t j = lane & 7u;
  const bool chosen = unit < g.n_units && (!g.mask || g.mask[unit] != 0);
  const bool live = chosen && j < g.width;
  const size_t e = static_cast<size_t>(unit) * g.width + j;
  uint4* rec = reinterpret_cast<uint4*>(static_cast<MixedDesc*>(g.table) + e);
  MixedDesc D{};
  int st = BK_OK;
  if (live) {
    const bk_agent_desc m = static_cast<const bk_agent_desc*>(g.rows)[e];
    const uint4 c0 = rec[0];  // {type, n, thr, tick_lo}
    const uint4 c3 = rec[3];  // {keep_thr, trade_vol, slot_base, pad}
    MixedDesc cur{};
    cur.type = c0.x;
    cur.n = c0.y;
    cur.slot_base = c3.z;
    const uint32_t asset = static_cast<uint32_t>(g.member_assets >> (8u * j)) & 7u;
    uint32_t why;
    st = agent_rows::mixed_row(m, tick_of(g, asset), cur.slot_base, &D, &why);
    if (st == BK_OK) st = agent_rows::mixed_fixed_ok(D, cur, m.agent_id_start, g.id_start[e]);
  }
  if (verdict(g, lane, unit, live, chosen, st) && live) {
    rec[0] = make_uint4(D.type, D.n, D.thr, D.tick_lo);
    rec[1] = make_uint4(D.tick_rng, D.tick_zone, D.vol_lo, D.vol_rng);
    rec[2] = make_uint4(D.vol_zone, D.tick_size, D.thr_limit, D.thr_market);
    rec[3] = make_uint4(static_cast<uint32_t>(D.keep_thr), D.trade_vol, D.slot_base, 0u);
    rec[4] = pack(D.mu, D.sigma);
    rec[5] = pack(D.decay, D.demand);
    rec[6] = pack(D.scale, D.order_ratio);
    rec[7] = pack(D.n_f, D.tick_f);
  }
}

}  // namespace retune
}  // namespace bkd
