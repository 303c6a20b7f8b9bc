// ingress_reset.hpp - bk_ingress_reset_books*: chosen books of a DEVICE-INGRESS env go back to a device-resident snapshot.
//
// The reference has no counterpart (an Env is rebuilt, never rewound).  A device-ingress env keeps more per
// book than the state block and the level-2 row that reset::k_reset_books (book_reset.hpp) moves - DESIGN.md 2.15:
//   * the unit's queue length dqlen[u]                                   -> 0 (what was queued since the last step is dropped);
//   * the order records dorders[b][id][2] (32 B) and order_log[b][id] (48 B), id < keep_b = min(the snapshot's
//     H_NEXT_ID of b, max_orders)                                        -> the snapshot's (stored as [n_books][n_keep], n_keep =
//     the largest keep_b); records at ids >= the snapshot's H_NEXT_ID need nothing: every reader stops at H_NEXT_ID, and
//     they are overwritten as the ids are handed out again;
//   * bk_update_agents' / bk_update_market_agents' agent_held[u][n_agents] -> the snapshot's row, or None (0xFFFFFFFF) in every
//     entry if the env had not made the buffer at the save (u: the unit - the book, or the market);
//   * bk_update_members' / bk_update_market_members' member_lists[u][n_members][list_cap], member_lens[u][n_members],
//     member_state[u][n_members][2], member_flags[u]                     -> the snapshot's rows, or the state of a first
//     update (lengths 0, state 0, flags 0, every list entry None);
//   * wcache: NOTHING.  WaveDecoder::load_cache validates the cached record against the book's RNG words, which rewind
//     (or are re-seeded) with the state block, so a stale record is rejected and decoded again.
//
// The bytes per masked book are data-dependent (hundreds of KB at a few thousand orders against the block's 1.5 - 10 KB),
// so the copy is NOT one wave per unit:
//   k_collect_units  one lane per unit reads its mask byte; a wave ballot + one atomicAdd per wave appends the masked
//                    units to `list` (its order is not deterministic; nothing depends on it); the same lane writes the
//                    unit's small fixed-size rows: dqlen, lengths, member state, flags.
//   k_reset_records  a fixed grid (sized from the CU count, never from the mask) whose waves stride over (list entry x
//                    segment) work items: an all-zero mask costs one load of the counter per wave, whatever n_keep is, and
//                    one masked book's records are shared by as many waves as they have segments.  A segment of the order
//                    records is 64 lanes x SEG_VECS 16-byte vectors (4 KiB at SEG_VECS = 4, the measured choice - DESIGN.md
//                    2.15), every load of the segment issued before its first store as in k_reset_books; the dword rows
//                    (agent_held, member_lists: their row lengths are no multiple of 4) move as 64 x 4 dwords.
// The same kernel run with list == nullptr takes every unit and is how bk_ingress_snapshot_save packs the records into
// the slot (source and destination strides swapped).  No LDS, no scratch, vector stores and ordinary atomicAdd only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "book_device.hpp"

#ifndef BKD_RESET_SEG_VECS
#define BKD_RESET_SEG_VECS 4
#endif

namespace bkd {
namespace reset {

constexpr int SEG_VECS = BKD_RESET_SEG_VECS;  // 16-byte vectors per lane and segment of the order records
constexpr uint32_t SEG_V = 64u * SEG_VECS;    // vectors per segment
constexpr uint32_t SEG_DW = 64u * 4u;         // dwords per segment of a dword row
constexpr int RECORD_WAVES = 4;               // waves per block of k_reset_records
constexpr uint32_t ORD_V = 2, LOG_V = 3;      // 16-byte vectors per order id in dorders / order_log
static_assert(sizeof(DevOrderLog) == LOG_V * 16, "an order_log record is three vectors");

constexpr uint32_t segs(uint32_t n, uint32_t per) { return (n + per - 1) / per; }

struct CollectArgs {
  const uint8_t* mask;  // [n_units], device memory
  uint32_t n_units, M;
  uint32_t* list;   // [n_units] the masked units, appended
  uint32_t* count;  // zeroed in front of the launch
  uint32_t* dqlen;  // [n_units]
  // bk_update_members' small rows (n_members = 0: none); snap_* == nullptr: the state of a first update
  uint32_t n_members;
  uint32_t* lens;
  uint64_t* mstate;
  uint32_t* mflags;
  const uint32_t* snap_lens;
  const uint64_t* snap_mstate;
  const uint32_t* snap_mflags;
};

__global__ __launch_bounds__(256) void k_collect_units(CollectArgs g) {
  const uint32_t u = blockIdx.x * 256u + threadIdx.x;
  const bool in = u < g.n_units;
  const bool on = in && g.mask[u] != 0;
  const unsigned long long bal = __ballot(on);
  if (bal == 0ull) return;
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t base = 0;
  if (lane == 0) base = atomicAdd(g.count, static_cast<uint32_t>(__popcll(bal)));
  base = rfl(base);
  if (!on) return;
  g.list[base + static_cast<uint32_t>(__popcll(bal & ((1ull << lane) - 1ull)))] = u;
  g.dqlen[u] = 0u;
  if (g.n_members) {  // (the members' rows are per unit: a book, or a market)
    for (uint32_t j = 0; j < g.n_members; ++j) {
      const size_t row = static_cast<size_t>(u) * g.n_members + j;
      g.lens[row] = g.snap_lens ? g.snap_lens[row] : 0u;
      g.mstate[2 * row] = g.snap_mstate ? g.snap_mstate[2 * row] : 0ull;
      g.mstate[2 * row + 1] = g.snap_mstate ? g.snap_mstate[2 * row + 1] : 0ull;
    }
    g.mflags[u] = g.snap_mflags ? g.snap_mflags[u] : 0u;
  }
}

// the largest keep_b = min(H_NEXT_ID of b, max_orders) of the env's books (bk_ingress_snapshot_save: *out zeroed in front)
__global__ __launch_bounds__(256) void k_max_keep(const uint32_t* state, uint32_t stride, uint32_t n_books, uint32_t max_orders,
                                                  uint32_t* out) {
  const uint32_t b = blockIdx.x * 256u + threadIdx.x;
  uint32_t keep = 0;
  if (b < n_books) keep = min(state[static_cast<size_t>(b) * stride + H_NEXT_ID], max_orders);
  for (int off = 32; off > 0; off >>= 1) keep = max(keep, static_cast<uint32_t>(__shfl_xor(static_cast<int>(keep), off)));
  if ((threadIdx.x & 63u) == 0 && keep) atomicMax(out, keep);
}

struct RecordArgs {
  const uint32_t* list;   // the masked units; nullptr: every unit, in order (the save)
  const uint32_t* count;  // entries of `list`
  uint32_t n_units, M;
  const uint32_t* keep_state;  // [n_books][stride]: keep_b is read from its H_NEXT_ID (the snapshot's blocks)
  uint32_t stride, max_orders, n_keep;
  // the order records: rows of dst_ids / src_ids ids per book (max_orders in the env, n_keep in a slot)
  bk_u32x4* dst_orders;
  const bk_u32x4* src_orders;
  bk_u32x4* dst_log;
  const bk_u32x4* src_log;
  uint32_t dst_ids, src_ids;
  // bk_update_agents' held ids (n_agents = 0: none); snap_held == nullptr: None in every entry
  uint32_t n_agents;
  uint32_t* held;
  const uint32_t* snap_held;
  // bk_update_members' lists (n_members = 0: none); snap_lists == nullptr: None in every entry.  Of a Noise / Momentum
  // member's row the snapshot's length moves (snap_lens), of a RandomAgents member's (bit j of random_mask) the whole
  // row of its agents' held ids (member_n[j])
  uint32_t n_members, list_cap, random_mask;
  uint32_t member_n[MAX_INGRESS_MEMBERS];
  uint32_t* lists;
  const uint32_t* snap_lists;
  const uint32_t* snap_lens;
};

// n vectors from src to dst, this segment: every load before the first store
__device__ __forceinline__ void move_vectors(bk_u32x4* dst, const bk_u32x4* src, uint32_t first, uint32_t n, uint32_t lane) {
  bk_u32x4 v[SEG_VECS];
#pragma unroll
  for (int i = 0; i < SEG_VECS; ++i) {
    const uint32_t k = first + i * 64u + lane;
    if (k < n) v[i] = src[k];
  }
#pragma unroll
  for (int i = 0; i < SEG_VECS; ++i) {
    const uint32_t k = first + i * 64u + lane;
    if (k < n) dst[k] = v[i];
  }
}

// n dwords of a row, this segment; src == nullptr: None
__device__ __forceinline__ void move_dwords(uint32_t* dst, const uint32_t* src, uint32_t first, uint32_t n, uint32_t lane) {
  uint32_t t[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint32_t k = first + i * 64u + lane;
    t[i] = (src && k < n) ? src[k] : 0xFFFFFFFFu;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint32_t k = first + i * 64u + lane;
    if (k < n) dst[k] = t[i];
  }
}

__global__ __launch_bounds__(64 * RECORD_WAVES) void k_reset_records(RecordArgs g) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = rfl(blockIdx.x * RECORD_WAVES + (threadIdx.x >> 6));
  const uint32_t n_waves = gridDim.x * RECORD_WAVES;
  const uint32_t n_list = g.list ? rfl(*g.count) : g.n_units;
  // the segments of one unit, in this order: dorders and order_log of each of its M books, then the unit's agent_held
  // row and its members' lists (the host checks that n_units * s_unit fits 32 bits)
  const uint32_t s_ord = segs(g.n_keep * ORD_V, SEG_V), s_log = segs(g.n_keep * LOG_V, SEG_V);
  const uint32_t s_held = segs(g.n_agents, SEG_DW), s_row = segs(g.list_cap, SEG_DW);
  const uint32_t s_book = s_ord + s_log;
  const uint32_t s_unit = g.M * s_book + s_held + g.n_members * s_row;
  if (s_unit == 0) return;
  const uint32_t total = n_list * s_unit;
  for (uint32_t w = wave; w < total; w += n_waves) {
    const uint32_t e = w / s_unit, r = w - e * s_unit;
    const uint32_t u = g.list ? rfl(g.list[e]) : e;
    uint32_t s = r;
    if (r < g.M * s_book) {
      const uint32_t a = r / s_book;
      s = r - a * s_book;
      const size_t b = static_cast<size_t>(u) * g.M + a;
      const uint32_t keep = min(rfl(g.keep_state[b * g.stride + H_NEXT_ID]), g.max_orders);
      if (s < s_ord) {
        move_vectors(g.dst_orders + b * g.dst_ids * ORD_V, g.src_orders + b * g.src_ids * ORD_V, s * SEG_V, keep * ORD_V, lane);
      } else {
        s -= s_ord;
        move_vectors(g.dst_log + b * g.dst_ids * LOG_V, g.src_log + b * g.src_ids * LOG_V, s * SEG_V, keep * LOG_V, lane);
      }
      continue;
    }
    s -= g.M * s_book;
    const size_t un = u;
    if (s < s_held) {
      move_dwords(g.held + un * g.n_agents, g.snap_held ? g.snap_held + un * g.n_agents : nullptr, s * SEG_DW, g.n_agents, lane);
      continue;
    }
    s -= s_held;
    const uint32_t j = s / s_row;
    s -= j * s_row;
    const size_t row = un * g.n_members + j;
    uint32_t n = g.list_cap;  // (None in every entry)
    if (g.snap_lists) n = (g.random_mask >> j) & 1u ? g.member_n[j] : min(rfl(g.snap_lens[row]), g.list_cap);
    move_dwords(g.lists + row * g.list_cap, g.snap_lists ? g.snap_lists + row * g.list_cap : nullptr, s * SEG_DW, n, lane);
  }
}

}  // namespace reset
}  // namespace bkd
