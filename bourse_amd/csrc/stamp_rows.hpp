// stamp_rows.hpp - the rank rule of the stamp compaction, one live order at a time.
//
// Compiled by the device kernel (stamp_compact.hpp), by the host library's accounting and by a CPU test
// (tests/cpp/stamp_rows_test.cpp): no HIP type, no intrinsic.  Every resting order carries a u32 arrival stamp (pool field
// 3) taken from the book's counter H_SEQ, and time priority inside a price level is "smaller stamp first" - compared RAW by
// the event-by-event loop, the queue view and bk_live_orders.  That is right as long as the live stamps of a book never
// straddle a wrap of the counter, and the compaction keeps it so, off the hot path: a live order's new stamp is its RANK,
// the number of live orders of the book that are older by the wrapping age H_SEQ - stamp, and the new H_SEQ is the live
// count - the state bk_load_book builds.  The wrapping age orders the live stamps correctly as long as fewer than 2^32
// orders have rested since the oldest live stamp was handed out (or since the last compaction), which is what the host's
// accounting (Room below) guarantees.  Stamps are unique per book, so no two live orders share a rank; dead slots keep
// their words.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BKD_STAMP_HD __host__ __device__ inline
#else
#define BKD_STAMP_HD inline
#endif

namespace bkd {
namespace stamps {

// how many orders have rested since `seq` was handed out, the order itself included (modulo 2^32; never 0 for a live order
// under the invariant above, since the counter is past every live stamp)
BKD_STAMP_HD uint32_t age(uint32_t seq_ctr, uint32_t seq) { return seq_ctr - seq; }

// 1 when the live order stamped `other` is older than the one stamped `mine`
BKD_STAMP_HD uint32_t older(uint32_t seq_ctr, uint32_t mine, uint32_t other) {
  return age(seq_ctr, other) > age(seq_ctr, mine) ? 1u : 0u;
}

// The rule over one whole pool, as the kernel applies it: seq[i] of every live slot becomes its rank, the return value
// is the new counter.  `out` may not alias `seq`.
inline uint32_t compact(uint32_t seq_ctr, uint32_t n_slots, const uint8_t* live, const uint32_t* seq, uint32_t* out) {
  uint32_t n_live = 0;
  for (uint32_t i = 0; i < n_slots; ++i) {
    out[i] = seq[i];
    if (!live[i]) continue;
    n_live += 1;
    uint32_t rank = 0;
    for (uint32_t j = 0; j < n_slots; ++j)
      if (live[j]) rank += older(seq_ctr, seq[i], seq[j]);
    out[i] = rank;
  }
  return n_live;
}

// The host's accounting: an upper bound of the largest H_SEQ among an env's books.  Before a launch in which a book can
// rest at most `rests` orders the caller asks needs_compaction(rests); when it says so the compaction is queued in front
// of the launch and compacted(pool_slots) recorded; then spend(rests).  H_SEQ itself then never passes `limit`, so it
// never wraps while an order rests.
struct Room {
  uint64_t limit = 0xFFFFFFFFull;  // the largest value H_SEQ may reach (BOURSE_AMD_STAMP_ROOM lowers it)
  uint64_t bound = 0;              // H_SEQ <= bound in every book

  bool needs_compaction(uint64_t rests) const { return bound + rests > limit; }
  // the most rests a launch may make after a compaction of pools of `pool_slots` slots
  uint64_t after_compaction(uint32_t pool_slots) const { return limit > pool_slots ? limit - pool_slots : 0; }
  void compacted(uint32_t pool_slots) { bound = pool_slots; }
  void spend(uint64_t rests) { bound += rests; }
  void raise(uint64_t other_bound) { bound = other_bound > bound ? other_bound : bound; }
};

}  // namespace stamps
}  // namespace bkd
