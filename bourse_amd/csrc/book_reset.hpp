// book_reset.hpp - bk_reset_books*: chosen books go back to a device-resident snapshot between two bk_run calls.
//
// The reference has no counterpart (an Env is rebuilt, never rewound).  A book's whole simulation state on the
// on-device order flow is its block of `state` (stride = 64 + R * 5 * 64 dwords) and its row of `l2_last` (W = 5 + 4 *
// levels dwords) - what bk_checkpoint_* carries - so a reset is a masked copy of those two from the snapshot's arrays, with
// four header words set on the way:
//   * H_TRADE_BASE = the snapshot's H_TRADES: no trade record of the abandoned run stays retained (k_book_service op 0, as
//     after bk_checkpoint_load);
//   * H_FLAGS = the snapshot's | the book's current ones: a sticky flag is never lost by a reset (bk_clear_flags clears);
//   * H_TRADING = the env's current flag (bk_enable_trading is env-wide, and so is its host mirror);
//   * with `seeds`: H_S0 / H_S1 = seed_from_u64(seeds[u]) in every book of the unit, as bk_env_create writes them
//     (host_math.hpp: one text for the host and the device).
// Every other dword - clock, id and sequence counters, step / event counters, trade volume, live masks, pool, the members'
// owner tags - returns to the snapshot's value.
//
// ONE WAVE PER UNIT u: a book, or with assets = M > 1 the market of books u * M .. u * M + M - 1 (which share one RNG
// stream).  A wave whose mask byte is 0 leaves after that one load.  A masked wave moves each block as 16-byte vectors
// (stride * 4 = 256 + 1280 R is a multiple of 16, the blocks are contiguous and the arrays come from hipMalloc) with every
// load of the block issued before its first store - R = 8: 656 vectors, 11 per lane, 44 VGPRs - and the level-2 row dword by
// dword (W is odd).  The header is the block's first 16 vectors, so lane l < 16 holds header dwords 4 l .. 4 l + 3 in its
// first vector and sets its own words there before the store: one store per dword.  No LDS, no scratch, vector stores only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "book_device.hpp"
#include "host_math.hpp"

namespace bkd {
namespace reset {

struct ResetArgs {
  uint32_t* state;             // [n_units * M][stride]
  uint32_t* l2_last;           // [n_units * M][W]
  const uint32_t* snap_state;  // the snapshot's copies of the two
  const uint32_t* snap_l2;
  uint32_t stride, W, M, n_units;
  const uint8_t* mask;    // [n_units], device memory: non-zero = reset the unit
  const uint64_t* seeds;  // [n_units], device memory, nullable: the units' new RNG seeds
  uint32_t trading;       // the env's current trading flag
};

constexpr int WAVES = 4;  // units per block

// header dword `dw` lives in component dw & 3 of the first vector of lane dw >> 2
__device__ __forceinline__ void set_hdr(bk_u32x4& v, uint32_t lane, int dw, uint32_t value) {
  if (lane == static_cast<uint32_t>(dw >> 2)) v[dw & 3] = value;
}

template <int R>
__global__ __launch_bounds__(64 * WAVES) void k_reset_books(ResetArgs g) {
  constexpr uint32_t NVEC = (HDR_DW + R * POOL_FIELDS * 64) / 4;  // 16-byte vectors of one block
  constexpr int PER_LANE = (NVEC + 63) / 64;
  static_assert((HDR_DW + R * POOL_FIELDS * 64) % 4 == 0 && HDR_DW == 64, "the block is whole vectors, the header the first 16");
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t u = rfl(blockIdx.x * WAVES + (threadIdx.x >> 6));
  if (u >= g.n_units) return;
  if (g.mask[u] == 0) return;
  uint64_t s0 = 0, s1 = 0;
  const bool reseed = g.seeds != nullptr;
  if (reseed) seed_from_u64(g.seeds[u], s0, s1);
  for (uint32_t a = 0; a < g.M; ++a) {
    const size_t b = static_cast<size_t>(u) * g.M + a;
    const uint32_t* src = g.snap_state + b * g.stride;
    uint32_t* dst = g.state + b * g.stride;
    const bk_u32x4* src4 = reinterpret_cast<const bk_u32x4*>(src);
    bk_u32x4* dst4 = reinterpret_cast<bk_u32x4*>(dst);
    bk_u32x4 v[PER_LANE];
#pragma unroll
    for (int i = 0; i < PER_LANE; ++i) {
      const uint32_t k = i * 64 + lane;
      if (k < NVEC) v[i] = src4[k];
    }
    const uint32_t flags_now = dst[H_FLAGS];  // (the same address in every lane; read before the vector that holds it is stored)
    // the snapshot's trade count, for the lane that holds H_TRADE_BASE (H_TRADES sits in another lane's vector)
    const uint32_t trades_lo = src[H_TRADES_LO], trades_hi = src[H_TRADES_HI];
    // the level-2 row: up to 4 dwords per lane in flight
    const uint32_t* l2s = g.snap_l2 + b * g.W;
    uint32_t* l2d = g.l2_last + b * g.W;
    for (uint32_t base = 0; base < g.W; base += 256) {
      uint32_t t[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const uint32_t k = base + i * 64 + lane;
        if (k < g.W) t[i] = l2s[k];
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const uint32_t k = base + i * 64 + lane;
        if (k < g.W) l2d[k] = t[i];
      }
    }
    set_hdr(v[0], lane, H_TRADE_BASE_LO, trades_lo);
    set_hdr(v[0], lane, H_TRADE_BASE_HI, trades_hi);
    if (lane == static_cast<uint32_t>(H_FLAGS >> 2)) v[0][H_FLAGS & 3] |= flags_now;
    set_hdr(v[0], lane, H_TRADING, g.trading);
    if (reseed) {
      set_hdr(v[0], lane, H_S0_LO, static_cast<uint32_t>(s0));
      set_hdr(v[0], lane, H_S0_HI, static_cast<uint32_t>(s0 >> 32));
      set_hdr(v[0], lane, H_S1_LO, static_cast<uint32_t>(s1));
      set_hdr(v[0], lane, H_S1_HI, static_cast<uint32_t>(s1 >> 32));
    }
#pragma unroll
    for (int i = 0; i < PER_LANE; ++i) {
      const uint32_t k = i * 64 + lane;
      if (k < NVEC) dst4[k] = v[i];
    }
  }
}

}  // namespace reset
}  // namespace bkd
