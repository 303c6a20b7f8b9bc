// hist_cursor.hpp - what a table folded from the level-2 history ring owes (plain C++17, no HIP): the rule of the host
// cursor that the series moments, the lag table and the bin table share.
//
// The ring keeps the last `cap` steps, or those since the last bk_clear_history (hist_base).  A table's cursor `seen` says
// that the steps below it are folded.  Of the steps [seen, steps_done) either some are no longer retained - the fold is
// refused - or there are none, or all of them stand in the ring: n <= cap of them from slot seen % cap on.
// bourse_amd.hip asks it for every fold, masked clear and reset; tests/cpp/hist_cursor_test.cpp checks it on the CPU.
#pragma once
#include <algorithm>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BKD_RING_HD __host__ __device__ inline
#else
#define BKD_RING_HD inline
#endif

namespace bkd {
namespace ring {

// first retained step of the history ring: the last cap steps, or since the last bk_clear_history()
inline uint64_t first_retained(uint64_t steps_done, uint64_t hist_base, uint64_t cap) {
  return std::max(steps_done > cap ? steps_done - cap : 0, hist_base);
}

enum CursorKind { CURSOR_LOST, CURSOR_NOTHING, CURSOR_FOLD };
struct Cursor {
  CursorKind kind;
  uint64_t first;  // CURSOR_LOST: steps [seen, first) are gone, first - seen of them
  uint32_t slot0;  // CURSOR_FOLD: the slot of step seen, seen % cap as a 64-bit remainder
  uint32_t n;      // CURSOR_FOLD: steps to fold, 1 .. cap (a ring's capacity is a u32, so both fit)
};

inline Cursor cursor(uint64_t seen, uint64_t steps_done, uint64_t hist_base, uint64_t cap) {
  const uint64_t first = first_retained(steps_done, hist_base, cap);
  if (seen < first) return {CURSOR_LOST, first, 0u, 0u};
  if (seen >= steps_done) return {CURSOR_NOTHING, first, 0u, 0u};  // (cap == 0 ends above: first == steps_done)
  return {CURSOR_FOLD, first, static_cast<uint32_t>(seen % cap), static_cast<uint32_t>(steps_done - seen)};
}

// the ring slot of step i of a fold whose first step stands at slot0: slot0 < cap, i < cap - one conditional subtract
// (the one function here that the fold kernels compile too, through hist_ring.hpp)
BKD_RING_HD uint64_t slot_of(uint32_t slot0, uint32_t i, uint64_t cap) {
  const uint64_t slot = static_cast<uint64_t>(slot0) + i;
  return slot >= cap ? slot - cap : slot;
}

}  // namespace ring
}  // namespace bkd
