// wave_mixed.hpp — k_agents_mixed_wave: agents.update of an AgentSet of NoiseAgent / MomentumAgent members + the shuffle
// of Env::step with ONE WAVE PER BOOK and the book's xoroshiro128** stream decoded 64 draws at a time.
//
// Why: the lane-per-book members' update (k_agents_mixed_lanes) walks ~1 500 dependent draws per book-step on ONE wave
// per 64 books - at C5 as written (8 192 books x 256 momentum + 256 noise agents) that is 128 waves on a chip of 1 024
// SIMDs, 532 us per step, 11 % lane utilisation (profiles/r02/pmc_c5m.json).  The members' streams are regular between
// hits, so they decode like RandomAgents' (wave_agents.hpp), only simpler - NOTHING a trader draws depends on the book:
//
//   * common::cancel_live_orders (ref crates/step_sim/src/agents/common.rs:54-76): one f32 draw per Active order of the
//     member, in list (= order id) order.  The member's `orders` list is kept per book (pool slots in creation order,
//     book-major so that a wave reads 64 entries with one load); entry i of a 64-entry chunk is lane i's: live test, draw
//     index = ballot prefix count, keep / cancel, in-place compaction - 64 orders per iteration.  An entry whose order
//     died is dropped in its member's own pass; slots are only handed out if they were free at the START of the step, so
//     a stale entry can never meet a re-used slot (no "listed" masks as in the lane-per-book kernel).
//   * the traders' loop (noise_agent.rs:132-174, momentum_agent.rs:163-203): a trader's turn starting at stream position
//     q ends at F(q), a function of the draws at q.. only (threshold tests, gen_bool, the ziggurat's length).  Every lane
//     evaluates F for its own position of the 64-draw window, the positions actually visited are the orbit of the
//     window's entry point under F (pointer doubling, 5 rounds), and the visited lanes that hit place their orders ALL AT
//     ONCE: ziggurat, exp, tick rounding are per-lane f64 code across the window's orders instead of scalar code per order.
//   * order ids are dense in creation order (ballot prefix counts), the k-th order created in a step takes the k-th free
//     slot (a rank table in LDS), and is written straight into the book's pool block with its pend bit - what
//     k_step_batch<R, false, POOLPEND> (book_device.hpp) expects.
//   * the shuffle is wave_agents.hpp's, on the same stream (the lane states are handed over).
//
// Semantics restated from (paths relative to the reference repo): agents/common.rs:21-141, noise_agent.rs:127-176,
// momentum_agent.rs:146-208, rand 0.8.5 / rand_distr 0.4.3 sampling as in mixed_agents.hpp (PARITY UNPINNED against
// Rust, bit-exact against the oracle through pm_math.hpp).  Independent books only (assets == 1; markets keep the
// lane-per-book update); a RandomAgents member of such a set is walked draw by draw on the scalar path.
#pragma once
#include "mixed_agents.hpp"
#include "wave_agents.hpp"

#pragma clang fp contract(off)

namespace bkd {

#ifndef BOURSE_AMD_TWO_ROUND
#define BOURSE_AMD_TWO_ROUND 1
#endif
constexpr uint32_t FLAG_DECODE_LOOKAHEAD = 256u;  // a ziggurat ran past the decode's look-ahead (p < 2^-90): flagged
constexpr uint32_t MW_RING = 512;                 // generated u64 draws kept in LDS
constexpr uint32_t MW_LOOK = 192;                 // a window's draws + look-ahead: positions [w0, w0 + MW_LOOK)
// books (waves) per workgroup: 8 (69.7 KB of LDS per workgroup since round 5's 64-entry price queue, two per CU = four waves
// per SIMD).  Until the event kernel's launches got 40 % shorter (the top-anchored key window, book_device.hpp
// keys_begin_wide) this kernel's occupancy did not matter - halving it cost 5 % -; since then the four parts' decode launches
// queue for LDS and halving it costs 13 %.  NINE waves per workgroup (76.8 KB, 18 waves per CU, 80 VGPRs) was tried: 36.0
// against 39.8 M - 228 workgroups per 2 048-book launch leave 28 CUs without one (docs/EXPERIMENTS.md).
#ifndef BOURSE_AMD_MW_WPB
#define BOURSE_AMD_MW_WPB 8
#endif
constexpr int MW_WPB = BOURSE_AMD_MW_WPB;

// per wave: the u64 ring | event list, free-slot table (u16 x 64 R each; the table's memory becomes the shuffle's swap
// targets) | orbit marks (72) + the pool's live words (16) + pad | deferred-price queue: 64 x f64 argument + 64 x u16
// {slot, side} - marks + live words + queue are 1 KB together, which becomes the shuffle's buckets
constexpr uint32_t MW_QCAP = 64;
static_assert(96 * 4 + MW_QCAP * 8 + MW_QCAP * 2 >= 64 * 8 * 2, "the shuffle's buckets (u16 x 512) alias marks + live words + queue");
constexpr uint32_t mw_wave_dwords(int R) { return 2 * MW_RING + 2 * 32 * R + 96 + 2 * MW_QCAP + MW_QCAP / 2; }
constexpr uint32_t MW_SHARED_DW = 2048 + 2 * 514 + 4;  // T^256 table, ziggurat x / f tables (257 doubles each), pad
constexpr size_t mixed_wave_lds_bytes(int R) { return (size_t)(MW_SHARED_DW + MW_WPB * mw_wave_dwords(R)) * 4; }

// xoroshiro128** on 32-bit halves, full 64-bit output word
__device__ __forceinline__ uint64_t rnglane_next_u64(RngLane& t) {
  const uint64_t s0 = mk64(t.a0, t.a1);
  uint64_t r = s0 * 5ull;
  r = (r << 7) | (r >> 57);
  r *= 9ull;
  t.advance();
  return r;
}

// The generator side of the decode: same block structure and cache record as WaveDecoder (wave_agents.hpp) - lane j
// holds the state 4 j draws into the 256-draw block - so the two kernels hand a book over through its record.
struct Stream64 {
  const uint4* tab;
  uint64_t* ring;  // ring[q & (MW_RING - 1)] = draw q of this launch's stream
  uint4* wcs;
  int lane;
  uint4 cs;
  uint32_t gen_end, pos;

  __device__ __forceinline__ void load_cache(const uint32_t* wc, uint32_t s0l, uint32_t s0h, uint32_t s1l, uint32_t s1h,
                                             const uint4* jt_lane) {
    const uint32_t wch = wc[lane];
    cs = reinterpret_cast<const uint4*>(wc + WC_HDR)[lane];
    pos = rdl(wch, WC_OFF);
    const bool cached = rdl(wch, WC_TAG) == WC_MAGIC && rdl(wch, WC_S0_LO) == s0l && rdl(wch, WC_S0_HI) == s0h &&
                        rdl(wch, WC_S1_LO) == s1l && rdl(wch, WC_S1_HI) == s1h && pos < WV_BLOCK;
    if (!cached) {
      cs = make_uint4(s0l, s0h, s1l, s1h);
      for (int b = 0; b < 6; ++b) {
        const uint4 j = wv_jump(jt_lane + b * 512, cs);
        const bool take = (lane >> b) & 1;
        cs.x = take ? j.x : cs.x;
        cs.y = take ? j.y : cs.y;
        cs.z = take ? j.z : cs.z;
        cs.w = take ? j.w : cs.w;
      }
      pos = 0;
    }
    gen_end = 0;
  }
  __device__ __forceinline__ void gen_block() {
    if (gen_end != 0) {
      wcs[lane] = cs;
      cs = wv_jump(tab, cs);
    }
    RngLane t{cs.x, cs.y, cs.z, cs.w};
    uint64_t x[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) x[k] = rnglane_next_u64(t);
    uint4* dst = reinterpret_cast<uint4*>(ring + ((gen_end + 4u * (uint32_t)lane) & (MW_RING - 1)));
    dst[0] = make_uint4((uint32_t)x[0], (uint32_t)(x[0] >> 32), (uint32_t)x[1], (uint32_t)(x[1] >> 32));
    dst[1] = make_uint4((uint32_t)x[2], (uint32_t)(x[2] >> 32), (uint32_t)x[3], (uint32_t)(x[3] >> 32));
    gen_end += WV_BLOCK;
    wave_sync();
  }
  __device__ __forceinline__ void ensure(uint32_t upto) {
    while (gen_end < upto) gen_block();
  }
  __device__ __forceinline__ uint64_t at(uint32_t q) const { return ring[q & (MW_RING - 1)]; }
};

// out[k] = the k-th slot of `mask` in slot order; returns the number of slots
template <int R>
__device__ __forceinline__ uint32_t rank_slots(const uint64_t (&mask)[R], uint16_t* out, int lane) {
  uint32_t acc = 0;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const uint32_t lr = acc + lane_rank(mask[r]);
    if (lane_bit(mask[r])) out[lr] = (uint16_t)(64u * r + (uint32_t)lane);
    acc += (uint32_t)__builtin_popcountll(mask[r]);
  }
  wave_sync();
  return acc;
}

// the members' `orders` lists of the wave-per-book update: pool slots in creation (= id) order, per book
struct WaveLists {
  uint16_t* list;  // [n_books][MAX_MEMBERS][cap]
  uint32_t* len;   // [n_books][MAX_MEMBERS]
  uint32_t cap;    // entries per member = pool size
};

// rand_distr StandardNormal (256-layer ziggurat) read from the generated stream starting at q0; len = draws consumed.
// `lim`: first position NOT available; running into it sets `over` (the caller flags the book).
__device__ __forceinline__ double zig_from_stream(const Stream64& S, const double* zx, const double* zf, uint32_t q0,
                                                  uint32_t lim, uint32_t& len, bool& over) {
  uint32_t q = q0;
  double out = 0.0;
  for (;;) {
    if (q >= lim) {
      over = true;
      break;
    }
    const uint64_t bits = S.at(q++);
    const uint32_t i = (uint32_t)bits & 0xffu;
    const double u = pm::from_bits(0x4000000000000000ull | (bits >> 12)) - 3.0;
    const double x = u * zx[i];
    if (pm::fabs_(x) < zx[i + 1]) {
      out = x;
      break;
    }
    if (i == 0) {
      const double Rz = 3.654152885361008796;
      double xx = 1.0, yy = 0.0;
      bool bad = false;
      while (-2.0 * yy < xx * xx) {
        if (q + 2u > lim) {
          bad = true;
          break;
        }
        const double x_ = pm::from_bits(0x3FF0000000000000ull | (S.at(q) >> 12)) - (1.0 - 2.220446049250313e-16 / 2.0);
        const double y_ = pm::from_bits(0x3FF0000000000000ull | (S.at(q + 1u) >> 12)) - (1.0 - 2.220446049250313e-16 / 2.0);
        q += 2u;
        xx = pm::log(x_) / Rz;
        yy = pm::log(y_);
      }
      if (bad) {
        over = true;
        break;
      }
      out = (u < 0.0) ? xx - Rz : Rz - xx;
      break;
    }
    if (q >= lim) {
      over = true;
      break;
    }
    const double f = static_cast<double>(S.at(q++) >> 11) * (1.0 / 9007199254740992.0);
    const double lhs = zf[i + 1] + (zf[i] - zf[i + 1]) * f;
    if (lhs < pm::exp(-x * x / 2.0)) {
      out = x;
      break;
    }
  }
  len = q - q0;
  return out;
}

template <int R>
__global__ __launch_bounds__(64 * MW_WPB, MW_WPB > 8 ? 5 : 4) void k_agents_mixed_wave(DevArgs a, MixedArgs ma, WaveArgs wa, WaveLists wl) {
#define BK_PB 0
#include "wave_mixed_body.inc"
#undef BK_PB
}

// PB (bk_set_agents_per_book): the members' records come from the book's row of the per-unit table
template <int R, bool PB>
__global__ __launch_bounds__(64 * MW_WPB, MW_WPB > 8 ? 5 : 4) void k_agents_mixed_wave(DevArgs a, MixedArgs ma, WaveArgs wa, WaveLists wl,
                                                                                  const MixedDesc* table) {
  static_assert(PB, "the uniform form is k_agents_mixed_wave<R>(DevArgs, MixedArgs, WaveArgs, WaveLists)");
#define BK_PB 1
#include "wave_mixed_body.inc"
#undef BK_PB
}

// (Re)build the wave-per-book lists from the pool after another pipeline (or a restore / a fresh set of agents): live
// slots tagged with the member, oldest order (smallest id) first.  One wave per book.
template <int R>
__global__ __launch_bounds__(256) void k_wave_lists_rebuild(DevArgs a, MixedArgs ma, WaveLists wl) {
  const int lane = threadIdx.x & 63;
  const uint32_t book = rfl(blockIdx.x * 4 + (threadIdx.x >> 6));
  if (book >= a.n_books) return;
  const uint32_t* st = a.state + (size_t)book * a.state_stride;
  uint32_t id[R], meta[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    id[r] = st[HDR_DW + r * POOL_FIELDS * 64 + 2 * 64 + lane];
    meta[r] = st[HDR_DW + r * POOL_FIELDS * 64 + 4 * 64 + lane];
  }
  for (uint32_t j = 0; j < MAX_MEMBERS; ++j) {
    uint64_t mask[R];
    uint64_t any = 0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      mask[r] = j < ma.n_desc ? __ballot((meta[r] & 1u) && ((meta[r] >> 8) & 0xFFu) == j + 1) : 0ull;
      any |= mask[r];
    }
    uint16_t* my = wl.list + ((size_t)book * MAX_MEMBERS + j) * wl.cap;
    uint32_t n = 0;
    while (any) {
      uint32_t m = 0xFFFFFFFFu;
#pragma unroll
      for (int r = 0; r < R; ++r) m = min(m, sel(mask[r], id[r], 0xFFFFFFFFu));
      const uint32_t idmin = wave_umin(m);
      int slot = 0;
      any = 0;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const uint64_t hit = mask[r] & __ballot(id[r] == idmin);
        if (hit) slot = r * 64 + (int)__builtin_ctzll(hit);
        mask[r] &= ~hit;
        any |= mask[r];
      }
      if (lane == 0) my[n] = (uint16_t)slot;
      n += 1;
    }
    if (lane == 0) wl.len[(size_t)book * MAX_MEMBERS + j] = n;
  }
}

}  // namespace bkd
