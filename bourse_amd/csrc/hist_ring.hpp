// hist_ring.hpp - what the kernels of the three tables folded from the level-2 history ring share (series.hpp, lags.hpp,
// bins.hpp): the span of the ring a fold reads and where its records stand, which book a wave of k_clear
// clears, the wave's fence, and a 16-byte vector from and to two 8-byte words.
// Plain C++ and the builtins of book_device.hpp; no kernel of its own.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "book_device.hpp"
#include "hist_cursor.hpp"  // ring::slot_of

namespace bkd {
namespace ring {

// what every fold reads: steps [lo, lo + n) of every book (the host fills it from ring::cursor's answer)
struct Span {
  const uint32_t* hist;  // [hist_cap][n_books][W]
  uint32_t hist_cap, n_books, W;
  uint32_t slot0;  // lo % hist_cap
  uint32_t n;      // steps to fold, 1 .. hist_cap
};

// the record of `book` in ring slot `slot`
__device__ __forceinline__ const uint32_t* record(const Span& s, uint64_t slot, uint32_t book) {
  return s.hist + (static_cast<size_t>(slot) * s.n_books + book) * s.W;
}

// the books a k_clear clears
struct Masked {
  const uint8_t* mask;  // [n_books / M] device memory; nullptr: every book
  uint32_t M;           // books per mask byte (the resets' units are markets)
  uint32_t n_books;
};

// the book of this wave of a k_clear with `waves` waves per block, or NO_BOOK: past the end, or not in the mask
constexpr uint32_t NO_BOOK = 0xFFFFFFFFu;
__device__ __forceinline__ uint32_t masked_book(const Masked& g, uint32_t waves) {
  const uint32_t b = rfl(blockIdx.x * waves + (threadIdx.x >> 6));
  if (b >= g.n_books) return NO_BOOK;
  if (g.mask && rfl(static_cast<uint32_t>(g.mask[b / g.M])) == 0u) return NO_BOOK;
  return b;
}

// what one wave's LDS and global accesses must reach before its other lanes' later ones
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ uint64_t vec_lo(const bk_u32x4& v) { return mk64(v.x, v.y); }
__device__ __forceinline__ uint64_t vec_hi(const bk_u32x4& v) { return mk64(v.z, v.w); }
__device__ __forceinline__ bk_u32x4 vec_of(uint64_t lo, uint64_t hi) {
  bk_u32x4 v;
  v.x = static_cast<uint32_t>(lo), v.y = static_cast<uint32_t>(lo >> 32);
  v.z = static_cast<uint32_t>(hi), v.w = static_cast<uint32_t>(hi >> 32);
  return v;
}

}  // namespace ring
}  // namespace bkd
