// stamp_compact.hpp - k_compact<R>: the stamp compaction of every book of an env (stamp_rows.hpp has the rule and why).
//
// Queued by the host library on the env's stream in front of a launch that could take a book's H_SEQ past its limit, and
// after bk_checkpoint_load; never part of a step.  DESIGN.md 7:
//   * one wave per book, COMPACT_WAVES waves per block (the last block may hold fewer books);
//   * lane l holds the stamp of slot r * 64 + l of every pool register r and the book's H_SEQ; the live slots are one
//     ballot per register;
//   * one walk over the live slots broadcasts each one's stamp by readlane, and every lane adds stamps::older() to the
//     rank of each of its own R slots;
//   * a lane stores the rank over the stamp of its live slots only (dead slots keep their words), lane 0 the live count
//     over H_SEQ.  A book with no live order only has its counter set to 0.
// Plain C++, no LDS, no scratch, no atomic, vector loads and stores only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "book_device.hpp"
#include "stamp_rows.hpp"

namespace bkd {
namespace stamps {

constexpr int COMPACT_WAVES = 4;  // waves (books) per block of k_compact

template <int R>
__global__ __launch_bounds__(64 * COMPACT_WAVES) void k_compact(uint32_t* state, uint32_t stride, uint32_t n_books) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t b = rfl(blockIdx.x * COMPACT_WAVES + (threadIdx.x >> 6));
  if (b >= n_books) return;

  uint32_t* hdr = state + static_cast<size_t>(b) * stride;
  uint32_t* pool = hdr + HDR_DW;
  const uint32_t seq_ctr = hdr[H_SEQ];  // (the same address in every lane)
  uint32_t seq[R], rank[R];
  unsigned long long live[R];
  uint32_t n_live = 0;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const uint32_t* p = pool + r * POOL_FIELDS * 64;
    seq[r] = p[192 + lane];
    live[r] = __ballot((p[256 + lane] & 1u) != 0u);
    n_live += static_cast<uint32_t>(__builtin_popcountll(live[r]));
    rank[r] = 0u;
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    unsigned long long walk = live[r];
    while (walk != 0ull) {
      const uint32_t l = static_cast<uint32_t>(__builtin_ctzll(walk));
      walk &= walk - 1ull;
      const uint32_t other = rdl(seq[r], l);
#pragma unroll
      for (int q = 0; q < R; ++q) rank[q] += older(seq_ctr, seq[q], other);
    }
  }
#pragma unroll
  for (int r = 0; r < R; ++r)
    if ((live[r] >> lane) & 1ull) pool[r * POOL_FIELDS * 64 + 192 + lane] = rank[r];
  if (lane == 0u) hdr[H_SEQ] = n_live;
}

}  // namespace stamps
}  // namespace bkd
