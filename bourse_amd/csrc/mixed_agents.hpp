// mixed_agents.hpp — gfx950 kernel for AgentSets that contain NoiseAgent / MomentumAgent members
// (SURVEY §8f rank 1), alone or together with RandomAgents groups, in declaration order.
//
//   k_run_mixed<R>: one wave per book, n_steps x { every member's update(env, rng); Env::step(rng) } with the
//   book in registers across the launch (like k_run_random).  The members' logic is strictly sequential in the
//   book's RNG stream, so it runs as wave-uniform control flow; the f64 price arithmetic (log-normal offsets around
//   the mid, rounding to ticks, tanh of the momentum) is evaluated redundantly on every lane.
//
// Restated semantics (paths relative to the reference repo):
//   agents::common::{cancel_live_orders, place_*_limit_order, round_price_*}  crates/step_sim/src/agents/common.rs:21-141
//   NoiseAgent::update      crates/step_sim/src/agents/noise_agent.rs:127-176
//   MomentumAgent::update   crates/step_sim/src/agents/momentum_agent.rs:146-208
//   rand / rand_distr sampling (Standard f64, Bernoulli(0.5), Open01, StandardNormal ziggurat, LogNormal): third-party,
//   restated — PARITY UNPINNED against Rust; exp/ln/tanh from pm_math.hpp so that the CPU oracle, which uses the
//   same restatement, can be matched bit-for-bit.
//
// Device representation: every order a member creates gets a pool slot at creation (pending until its New event is
// processed; released again if it never rests), RandomAgents members keep their fixed slot == agent mapping in
// [0, n_fixed); a member's `orders` list is "live slots tagged with the member", iterated in ascending order id
// (= the list's insertion order).
#pragma once
#include "book_device.hpp"
#include "pm_math.hpp"

// every f64 expression below must round exactly like the oracle's (no FMA contraction): file-scope switch
#pragma clang fp contract(off)

namespace bkd {

constexpr int H_GFLAGS = 30;  // bit j: member j has a last_price
constexpr int H_GST = 48;     // member j: dwords 48+4j.. = momentum (lo, hi), last_price (lo, hi)

// (MixedDesc, MAX_MEMBERS: agent_table.hpp)

struct MixedArgs {
  const MixedDesc* descs;
  uint32_t n_desc;
  uint32_t n_fixed;  // pool slots reserved for RandomAgents members
  // MarketEnv mode (NoiseMarketAgent / MomentumMarketAgent / RandomMarketAgents members): the asset each member trades
  // and the fixed slots reserved in each asset's book
  uint32_t asset[MAX_MEMBERS];
  uint32_t n_fixed_a[MAX_ASSETS];
};

#define ZIG_TABLE_BEGIN(name) __constant__ const double name[257] = {
#define ZIG_TABLE_END };
#include "zig_norm_tables.inc"
#undef ZIG_TABLE_BEGIN
#undef ZIG_TABLE_END

// pin a wave-uniform 64-bit value to scalar registers (the f64 code around the generator otherwise drags the RNG
// arithmetic onto the vector unit: v_mad_u64_u32 chains instead of s_mul / s_lshl)
__device__ __forceinline__ uint64_t pin_scalar(uint64_t x) {
  return mk64(rfl((uint32_t)x), rfl((uint32_t)(x >> 32)));
}
__device__ __forceinline__ uint64_t next_u64(Rng& rng) {
  rng.s0 = pin_scalar(rng.s0);
  rng.s1 = pin_scalar(rng.s1);
  uint64_t r = rng.s0 * 5ull;
  r = (r << 7) | (r >> 57);
  r *= 9ull;
  const uint64_t t1 = rng.s1 ^ rng.s0;
  rng.s0 = ((rng.s0 << 24) | (rng.s0 >> 40)) ^ t1 ^ (t1 << 16);
  rng.s1 = (t1 << 37) | (t1 >> 27);
  return r;
}
// wave-uniform double out of the VALU back into scalar registers (keeps later control flow uniform)
__device__ __forceinline__ double uni(double x) {
  const uint64_t b = pm::to_bits(x);
  return pm::from_bits(mk64(rfl((uint32_t)b), rfl((uint32_t)(b >> 32))));
}
__device__ __forceinline__ double gen_f64(Rng& rng) {  // rand Standard f64
  return static_cast<double>(next_u64(rng) >> 11) * (1.0 / 9007199254740992.0);
}
__device__ __forceinline__ double gen_open01(Rng& rng) {  // rand Open01 f64
  const double v = pm::from_bits(0x3FF0000000000000ull | (next_u64(rng) >> 12));
  return v - (1.0 - 2.220446049250313e-16 / 2.0);
}
// rand_distr StandardNormal: 256-layer ziggurat (utils.rs ziggurat, symmetric)
__device__ __forceinline__ double sample_standard_normal(Rng& rng) {
  for (;;) {
    const uint64_t bits = next_u64(rng);
    const uint32_t i = (uint32_t)bits & 0xffu;
    const double u = pm::from_bits(0x4000000000000000ull | (bits >> 12)) - 3.0;
    const double x = uni(u * ZIG_NORM_X[i]);
    if (pm::fabs_(x) < ZIG_NORM_X[i + 1]) return x;
    if (i == 0) {
      const double R = 3.654152885361008796;
      double xx = 1.0, yy = 0.0;
      while (-2.0 * yy < xx * xx) {
        const double x_ = gen_open01(rng);
        const double y_ = gen_open01(rng);
        xx = uni(pm::log(x_) / R);
        yy = uni(pm::log(y_));
      }
      return (u < 0.0) ? xx - R : R - xx;
    }
    const double lhs = uni(ZIG_NORM_F[i + 1] + (ZIG_NORM_F[i] - ZIG_NORM_F[i + 1]) * gen_f64(rng));
    if (lhs < uni(pm::exp(-x * x / 2.0))) return x;
  }
}
__device__ __forceinline__ uint32_t price_from_f64(double p) {  // clamp(0, u32::MAX) as u32 (NaN -> 0)
  if (!(p == p)) return 0u;
  if (p < 0.0) p = 0.0;
  if (p > 4294967295.0) p = 4294967295.0;
  return static_cast<uint32_t>(p);
}
__device__ __forceinline__ uint32_t round_price_up(double p, double tick) {  // common.rs:21-25
  return price_from_f64(pm::ceil_(p / tick) * tick);
}
__device__ __forceinline__ uint32_t round_price_down(double p, double tick) {  // common.rs:36-40
  return price_from_f64(pm::floor_(p / tick) * tick);
}
// `gen::<f64>() < p` as an integer threshold on the 53 random bits: k * 2^-53 < p  <=>  k < ceil(p * 2^53)
__device__ __forceinline__ uint64_t thr53(double p) {
  if (!(p > 0.0)) return 0ull;
  if (p >= 1.0) return 9007199254740992ull;
  return static_cast<uint64_t>(static_cast<int64_t>(pm::ceil_(p * 9007199254740992.0)));
}

template <int R>
struct MixedCtx {
  uint32_t ev[R];     // event list (slot indices)
  uint32_t owner[R];  // member index + 1 of the limit order resting / pending in the slot, 0 = none
  uint32_t n_fixed;   // slots [0, n_fixed) belong to RandomAgents members; the rest is allocated dynamically
  uint32_t tick;      // the book's tick size (create_order's check)
  uint32_t n_ev;
};

// Env::place_order from a member: id assignment + New event; the order is parked in a free pool slot
template <int R>
__device__ __forceinline__ void mixed_create(Book<R>& B, MixedCtx<R>& C, int lane, bool is_bid, uint32_t price,
                                             uint32_t vol, uint32_t owner_tag) {
  // create_order's tick check (orderbook.rs:367-382); the reference `.unwrap()`s the Err (common.rs:107,140), i.e.
  // panics: flagged, and like an Err nothing is created (no id, no event).  Reachable when a log-normal offset drives
  // the price to the u32::MAX clamp on a book whose tick does not divide it.  Market orders carry no price.
  if (owner_tag != 0 && price % C.tick != 0) {
    B.flags |= FLAG_PRICE_TICK;
    return;
  }
  const uint32_t id = B.next_id;
  B.next_id += 1;  // create_order consumes the id (orderbook.rs:363)
  int slot = -1;
#pragma unroll
  for (int r = R - 1; r >= 0; --r) {
    // dynamic slots of this register: index >= n_fixed (rebuilt here: 2R fewer live SGPRs than a mask array)
    const uint32_t lo = C.n_fixed > 64u * r ? C.n_fixed - 64u * r : 0u;
    const uint64_t dyn = lo >= 64u ? 0ull : (~0ull << lo);
    const uint64_t fr = ~(B.live[r] | B.pend[r]) & dyn;
    if (fr) slot = r * 64 + (int)__builtin_ctzll(fr);
  }
  if (slot < 0) {
    B.flags |= FLAG_POOL_OVERFLOW;  // reported, never silent: the order (and its event) is dropped
    return;
  }
  slot_write<R>(B.price, slot, price);
  slot_write<R>(B.vol, slot, vol);
  slot_write<R>(B.id, slot, id);
  slot_write<R>(C.owner, slot, owner_tag);
  mask_set<R>(B.bid, slot, is_bid);
  mask_set<R>(B.pend, slot, true);
  slot_write<R>(C.ev, C.n_ev, (uint32_t)slot);
  C.n_ev += 1;
  (void)lane;
}

// common::cancel_live_orders (common.rs:54-76): the member's Active orders in list (= id) order, one f32 draw each;
// `draw > p_cancel` keeps the order, otherwise its cancellation is queued
template <int R>
__device__ __forceinline__ void mixed_cancel_live(Book<R>& B, MixedCtx<R>& C, Rng& rng, int lane, uint32_t tag,
                                                  int32_t keep_thr) {
  uint64_t mask[R];
  uint64_t any = 0;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    mask[r] = B.live[r] & __ballot(C.owner[r] == tag);
    any |= mask[r];
  }
  while (any) {
    uint32_t m = 0xFFFFFFFFu;
#pragma unroll
    for (int r = 0; r < R; ++r) m = min(m, sel(mask[r], B.id[r], 0xFFFFFFFFu));
    const uint32_t idmin = wave_umin(m);
    int slot = 0;
    any = 0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const uint64_t hit = mask[r] & __ballot(B.id[r] == idmin);
      if (hit) slot = r * 64 + (int)__builtin_ctzll(hit);
      mask[r] &= ~hit;
      any |= mask[r];
    }
    const uint32_t x = rng.next_u32();
    if (!((int32_t)(x >> 8) > keep_thr)) {  // not kept -> env.cancel_order(id)
      slot_write<R>(C.ev, C.n_ev, (uint32_t)slot);
      C.n_ev += 1;
    }
  }
  (void)lane;
}

// member state that lives across steps: momentum / last mid price per member (momentum_agent.rs:108-117)
struct MixedState {
  uint32_t gflags;
  double g_mom[MAX_MEMBERS], g_last[MAX_MEMBERS];
};
__device__ __forceinline__ void mixed_load_state(MixedState& S, const uint32_t* st, int lane) {
  const uint32_t hdr = st[lane];
  S.gflags = rdl(hdr, H_GFLAGS);
#pragma unroll
  for (int j = 0; j < MAX_MEMBERS; ++j) {
    S.g_mom[j] = pm::from_bits(mk64(rdl(hdr, H_GST + 4 * j), rdl(hdr, H_GST + 4 * j + 1)));
    S.g_last[j] = pm::from_bits(mk64(rdl(hdr, H_GST + 4 * j + 2), rdl(hdr, H_GST + 4 * j + 3)));
  }
}
// after store_book: member state into the header, owner tags (+ live / bid / pend bits) into the pool's meta words
template <int R>
__device__ __forceinline__ void mixed_store_state(const MixedState& S, const Book<R>& B, const MixedCtx<R>& C,
                                                  uint32_t* st, int lane) {
  uint32_t h2 = st[lane];
  auto put = [&](int idx, uint32_t v) { h2 = (lane == idx) ? v : h2; };
  put(H_GFLAGS, S.gflags);
#pragma unroll
  for (int j = 0; j < MAX_MEMBERS; ++j) {
    const uint64_t mb = pm::to_bits(S.g_mom[j]), lb = pm::to_bits(S.g_last[j]);
    put(H_GST + 4 * j, (uint32_t)mb);
    put(H_GST + 4 * j + 1, (uint32_t)(mb >> 32));
    put(H_GST + 4 * j + 2, (uint32_t)lb);
    put(H_GST + 4 * j + 3, (uint32_t)(lb >> 32));
  }
  st[lane] = h2;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    uint32_t* p = st + HDR_DW + r * POOL_FIELDS * 64 + 4 * 64;
    p[lane] = (lane_bit(B.live[r]) ? 1u : 0u) | (lane_bit(B.bid[r]) ? 2u : 0u) | (lane_bit(B.pend[r]) ? 4u : 0u) |
              (C.owner[r] << 8);
  }
}
template <int R>
__device__ __forceinline__ void mixed_load_ctx(MixedCtx<R>& C, const uint32_t* st, const MixedArgs& ma, int lane) {
#pragma unroll
  for (int r = 0; r < R; ++r) {
    C.ev[r] = 0;
    C.owner[r] = (st[HDR_DW + r * POOL_FIELDS * 64 + 4 * 64 + lane] >> 8) & 0xFFu;
  }
  C.n_fixed = ma.n_fixed;
  C.n_ev = 0;
}

// One step's agents.update(env, rng) for every member in declaration order (crates/macros/src/lib.rs:57-73) followed
// by transactions.shuffle(rng) (env.rs:121): fills C.ev / C.n_ev and parks the new orders in the pool.
template <int R>
__device__ __forceinline__ void mixed_update_and_shuffle(Book<R>& B, MixedCtx<R>& C, Rng& rng, const MixedArgs& ma,
                                                         MixedState& S, int lane) {
  C.n_ev = 0;
  // OrderBook::mid_price (orderbook.rs:272-276) of the book as the agents see it (updates only queue events)
  double mid;
  {
    uint32_t mb = 0u, mk = 0xFFFFFFFFu;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      mb = max(mb, sel(B.live[r] & B.bid[r], B.price[r], 0u));
      mk = min(mk, sel(B.live[r] & ~B.bid[r], B.price[r], 0xFFFFFFFFu));
    }
    const uint32_t bid = wave_umax(mb), ask = wave_umin(mk);
    mid = static_cast<double>(bid) + 0.5 * static_cast<double>(ask - bid);
  }
  for (uint32_t j = 0; j < ma.n_desc; ++j) {
    const MixedDesc D = ma.descs[j];
    if (D.type == 0) {
      // ---- RandomAgents::update (random_agent.rs:85-119), fixed slots [slot_base, slot_base + n)
      for (uint32_t i = 0; i < D.n; ++i) {
        const uint32_t n = D.slot_base + i;
        const uint32_t x = rng.next_u32();
        if ((x >> 8) < D.thr) {
          slot_write<R>(C.ev, C.n_ev, n);
          C.n_ev += 1;
          if (!mask_test<R>(B.live, n)) {
            const uint32_t side = rng.below(2u, 0x7FFFFFFFu);
            const uint32_t tick = D.tick_lo + rng.below(D.tick_rng, D.tick_zone);
            const uint32_t vol = D.vol_lo + rng.below(D.vol_rng, D.vol_zone);
            slot_write<R>(B.price, n, tick * D.tick_size);
            slot_write<R>(B.vol, n, vol);
            slot_write<R>(B.id, n, B.next_id);
            B.next_id += 1;
            mask_set<R>(B.bid, n, side != 0);
            mask_set<R>(B.pend, n, true);
          }
        }
      }
    } else {
      const uint32_t tag = j + 1;
      mixed_cancel_live<R>(B, C, rng, lane, tag, D.keep_thr);
      if (D.type == 1) {
        // ---- NoiseAgent::update (noise_agent.rs:127-176)
        for (uint32_t t = 0; t < D.n; ++t) {
          if ((rng.next_u32() >> 8) < D.thr_limit) {                // gen::<f32>() < p_limit
            const bool buy = next_u64(rng) < 0x8000000000000000ull;  // gen_bool(0.5)
            const double dist = pm::fabs_(uni(pm::exp(D.mu + D.sigma * sample_standard_normal(rng))));
            const uint32_t price =
                rfl(buy ? round_price_down(mid - dist, D.tick_f) : round_price_up(mid + dist, D.tick_f));
            mixed_create<R>(B, C, lane, buy, price, D.trade_vol, tag);
          }
          if ((rng.next_u32() >> 8) < D.thr_market) {                // gen::<f32>() < p_market
            const bool buy = next_u64(rng) < 0x8000000000000000ull;
            mixed_create<R>(B, C, lane, buy, buy ? 0xFFFFFFFFu : 0u, D.trade_vol, 0u);
          }
        }
      } else {
        // ---- MomentumAgent::update (momentum_agent.rs:146-208)
        double m = 0.0, p_market = 0.0;
        if ((S.gflags >> j) & 1u) {
          double gm = S.g_mom[0], gl = S.g_last[0];
#pragma unroll
          for (int q = 1; q < MAX_MEMBERS; ++q) {
            gm = ((uint32_t)q == j) ? S.g_mom[q] : gm;
            gl = ((uint32_t)q == j) ? S.g_last[q] : gl;
          }
          m = uni(gm * (1.0 - D.decay) + D.decay * (mid - gl));
          p_market = uni(D.demand * pm::tanh(D.scale * m) / D.n_f);
        }
        uint64_t thr_l, thr_m;
        {
          const double p_limit = D.order_ratio * p_market;
          thr_l = thr53(p_limit);
          thr_m = thr53(p_market);
          thr_l = mk64(rfl((uint32_t)thr_l), rfl((uint32_t)(thr_l >> 32)));
          thr_m = mk64(rfl((uint32_t)thr_m), rfl((uint32_t)(thr_m >> 32)));
        }
        const int sgn = (m > 0.0) ? 1 : ((m < 0.0) ? -1 : 0);
        for (uint32_t t = 0; t < D.n; ++t) {
          if ((next_u64(rng) >> 11) < thr_l) {  // gen::<f64>() < p_limit
            if (sgn != 0) {
              const double dist = pm::fabs_(uni(pm::exp(D.mu + D.sigma * sample_standard_normal(rng))));
              const uint32_t price =
                  rfl(sgn > 0 ? round_price_down(mid - dist, D.tick_f) : round_price_up(mid + dist, D.tick_f));
              mixed_create<R>(B, C, lane, sgn > 0, price, D.trade_vol, tag);
            }
          }
          if ((next_u64(rng) >> 11) < thr_m) {  // gen::<f64>() < p_market
            if (sgn != 0) mixed_create<R>(B, C, lane, sgn > 0, sgn > 0 ? 0xFFFFFFFFu : 0u, D.trade_vol, 0u);
          }
        }
#pragma unroll
        for (int q = 0; q < MAX_MEMBERS; ++q) {
          if ((uint32_t)q == j) {
            S.g_mom[q] = m;
            S.g_last[q] = mid;
          }
        }
        S.gflags |= 1u << j;
      }
    }
  }
  // ---- Env::step's shuffle (env.rs:121)
  for (uint32_t i = C.n_ev; i-- > 1;) {
    const uint32_t jx = rng.below(i + 1);
    const uint32_t ai = slot_read<R>(C.ev, i), aj = slot_read<R>(C.ev, jx);
    slot_write<R>(C.ev, i, aj);
    slot_write<R>(C.ev, jx, ai);
  }
}

// fused: n_steps x { members' update + shuffle; event loop + snapshot } with the book in registers (small batches)
template <int R>
__global__ __launch_bounds__(256) void k_run_mixed(DevArgs a, MixedArgs ma, uint64_t first_step, uint32_t n_steps) {
#define BK_PB 0
#include "run_mixed_body.inc"
#undef BK_PB
}

// split: one step's members' update + shuffle per book; the new orders stay parked in the pool (pend bit in the
// stored meta word), the shuffled event list goes to the book's step batch for k_step_batch<R, false, true>.
template <int R>
__global__ __launch_bounds__(256) void k_agents_mixed(DevArgs a, MixedArgs ma) {
#define BK_PB 0
#include "agents_mixed_body.inc"
#undef BK_PB
}

// PB (bk_set_agents_per_book): the members' parameters are the book's row of the per-unit table, table[book * n_desc + j]
template <int R, bool PB>
__global__ __launch_bounds__(256) void k_run_mixed(DevArgs a, MixedArgs ma, uint64_t first_step, uint32_t n_steps,
                                                   const MixedDesc* table) {
  static_assert(PB, "the uniform form is k_run_mixed<R>(DevArgs, MixedArgs, uint64_t, uint32_t)");
#define BK_PB 1
#include "run_mixed_body.inc"
#undef BK_PB
}

template <int R, bool PB>
__global__ __launch_bounds__(256) void k_agents_mixed(DevArgs a, MixedArgs ma, const MixedDesc* table) {
  static_assert(PB, "the uniform form is k_agents_mixed<R>(DevArgs, MixedArgs)");
#define BK_PB 1
#include "agents_mixed_body.inc"
#undef BK_PB
}

// ==================================================================================
// Lane-per-book members' update (the split pipeline's default for these AgentSets): 64 books per wave, every lane runs
// its book's agents.update + shuffle as ordinary per-lane code — the RNG stream, the ziggurat / exp / tanh arithmetic and
// the order creation are all SIMT across books instead of scalar code on one wave per book.  What a lane needs of its
// book: the touch prices (mid price) from the last level-2 record, the pool's live masks (one 64-byte line of the
// header), and the member's `orders` list, kept in creation order in an aux buffer laid out [member][entry][book] so
// that the lanes' accesses coalesce.  New orders are written straight into free pool slots with their pend bit; the
// event kernel is k_step_batch<R, false, true>.
//
// A slot counts as free when it is neither live, nor pending, nor still referenced by some member's list (`inl` masks):
// a dead order's entry is purged at its member's next update, so "live bit set" alone identifies a list entry's order.
// ==================================================================================
struct MixedLists {
  uint16_t* list;  // [MAX_MEMBERS][cap][n_books]: pool slots of the member's orders, oldest first
  uint32_t* len;   // [MAX_MEMBERS][n_books]
  uint32_t* inl;   // [2R][n_books]: slots referenced by the lists, 32 per word
  uint32_t cap;    // entries per member = pool size
  uint32_t n_books;
  uint32_t n_units;  // lists are per market (= book when assets == 1)
};

struct LaneRng {  // xoroshiro128** per lane
  uint64_t s0, s1;
  __device__ __forceinline__ uint64_t next_u64() {
    uint64_t r = s0 * 5ull;
    r = (r << 7) | (r >> 57);
    r *= 9ull;
    const uint64_t t1 = s1 ^ s0;
    s0 = ((s0 << 24) | (s0 >> 40)) ^ t1 ^ (t1 << 16);
    s1 = (t1 << 37) | (t1 >> 27);
    return r;
  }
  __device__ __forceinline__ uint32_t next_u32() { return (uint32_t)next_u64(); }
  __device__ __forceinline__ uint32_t below(uint32_t range, uint32_t zone) {
    for (;;) {
      const uint64_t m = (uint64_t)next_u32() * range;
      if ((uint32_t)m <= zone) return (uint32_t)(m >> 32);
    }
  }
  __device__ __forceinline__ double f64() { return static_cast<double>(next_u64() >> 11) * (1.0 / 9007199254740992.0); }
  __device__ __forceinline__ double open01() {
    const double v = pm::from_bits(0x3FF0000000000000ull | (next_u64() >> 12));
    return v - (1.0 - 2.220446049250313e-16 / 2.0);
  }
  // rand_distr StandardNormal (256-layer ziggurat), as above; zx / zf = the tables (staged in LDS by the caller: a
  // lane's index is its own, and a table miss would be a full memory round trip in a latency-bound kernel)
  __device__ __forceinline__ double std_normal(const double* zx, const double* zf) {
    for (;;) {
      const uint64_t bits = next_u64();
      const uint32_t i = (uint32_t)bits & 0xffu;
      const double u = pm::from_bits(0x4000000000000000ull | (bits >> 12)) - 3.0;
      const double x = u * zx[i];
      if (pm::fabs_(x) < zx[i + 1]) return x;
      if (i == 0) {
        const double Rz = 3.654152885361008796;
        double xx = 1.0, yy = 0.0;
        while (-2.0 * yy < xx * xx) {
          const double x_ = open01();
          const double y_ = open01();
          xx = pm::log(x_) / Rz;
          yy = pm::log(y_);
        }
        return (u < 0.0) ? xx - Rz : Rz - xx;
      }
      const double lhs = zf[i + 1] + (zf[i] - zf[i + 1]) * f64();
      if (lhs < pm::exp(-x * x / 2.0)) return x;
    }
  }
};

// MKT: the lane owns a MARKET (books [b*M, b*M + M)): one RNG stream, one event queue; member j trades asset
// ma.asset[j] (NoiseMarketAgent / MomentumMarketAgent / RandomMarketAgents: noise_agent.rs:281-339,
// momentum_agent.rs:328-396, random_agent.rs:204-247); event entries carry the asset in bits 12..14.
constexpr int MLQ_CAP = 128;  // deferred-price queue of k_agents_mixed_lanes: drained at 64, at most 64 more per agent turn
                               // (2 x 80.9 KB of LDS still fit a CU at R = 8)
constexpr size_t mixed_lanes_lds_bytes(int R, bool mkt) {
  return (size_t)(32 * R * 64 + 2 * (2 * R * 64) + 2 * (mkt ? MAX_ASSETS * 64 : 64)) * 4 + 2 * 257 * sizeof(double) +
         MLQ_CAP * (2 * sizeof(double) + 4);
}

template <int R, bool MKT>
__global__ __launch_bounds__(64) void k_agents_mixed_lanes(DevArgs a, MixedArgs ma, MixedLists ml) {
#define BK_PB 0
#include "mixed_lanes_body.inc"
#undef BK_PB
}

// PB (bk_set_agents_per_book): one member's record of the lane's unit, the fields its kind reads - D holds the shared ones
// (type, n, slot_base, n_f) already.  Per lane these are vector registers: a whole 128-byte record would not stay in them.
__device__ __forceinline__ void lane_desc(MixedDesc& D, const MixedDesc* e) {
  if (D.type == 0) {
    D.thr = e->thr;
    D.tick_lo = e->tick_lo;
    D.tick_rng = e->tick_rng;
    D.tick_zone = e->tick_zone;
    D.vol_lo = e->vol_lo;
    D.vol_rng = e->vol_rng;
    D.vol_zone = e->vol_zone;
    D.tick_size = e->tick_size;
    return;
  }
  D.keep_thr = e->keep_thr;
  D.trade_vol = e->trade_vol;
  D.mu = e->mu;
  D.sigma = e->sigma;
  D.tick_f = e->tick_f;
  if (D.type == 1) {
    D.thr_limit = e->thr_limit;
    D.thr_market = e->thr_market;
  } else {
    D.decay = e->decay;
    D.demand = e->demand;
    D.scale = e->scale;
    D.order_ratio = e->order_ratio;
  }
}
// + the per-lane ticks of the deferred-price queue (independent books only; 2 x 81.4 KB still fit a CU at R = 8)
constexpr size_t mixed_lanes_pb_lds_bytes(int R, bool mkt) { return mixed_lanes_lds_bytes(R, mkt) + (mkt ? 0 : 64 * sizeof(double)); }
static_assert(2 * mixed_lanes_pb_lds_bytes(8, false) <= 160 * 1024, "two workgroups per CU at R = 8");

template <int R, bool MKT, bool PB>
__global__ __launch_bounds__(64) void k_agents_mixed_lanes(DevArgs a, MixedArgs ma, MixedLists ml, const MixedDesc* table) {
  static_assert(PB, "the uniform form is k_agents_mixed_lanes<R, MKT>(DevArgs, MixedArgs, MixedLists)");
#define BK_PB 1
#include "mixed_lanes_body.inc"
#undef BK_PB
}

// (Re)build the members' lists from the pool after the wave-per-book kernels (or a restore) have run: live slots
// tagged with the member, oldest order first.  One wave per book.
template <int R>
__global__ __launch_bounds__(256) void k_mixed_lists_rebuild(DevArgs a, MixedArgs ma, MixedLists ml) {
  const int lane = threadIdx.x & 63;
  const uint32_t book = rfl(blockIdx.x * 4 + (threadIdx.x >> 6));
  if (book >= a.n_books) return;
  const uint32_t* st = a.state + (size_t)book * a.state_stride;
  const size_t NB = ml.n_books, NU = ml.n_units;
  const uint32_t unit = book / a.assets, my_asset = book - unit * a.assets;  // assets == 1: unit == book
  uint32_t id[R], meta[R];
  uint64_t listed[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    id[r] = st[HDR_DW + r * POOL_FIELDS * 64 + 2 * 64 + lane];
    meta[r] = st[HDR_DW + r * POOL_FIELDS * 64 + 4 * 64 + lane];
    listed[r] = 0;
  }
  for (uint32_t j = 0; j < ma.n_desc; ++j) {
    if (a.assets > 1 && ma.asset[j] != my_asset) continue;  // the member trades another asset of the market
    uint64_t mask[R];
    uint64_t any = 0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      mask[r] = __ballot((meta[r] & 1u) && ((meta[r] >> 8) & 0xFFu) == j + 1);
      any |= mask[r];
      listed[r] |= mask[r];
    }
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
      if (lane == 0) ml.list[((size_t)j * ml.cap + n) * NU + unit] = (uint16_t)slot;
      n += 1;
    }
    if (lane == 0) ml.len[(size_t)j * NU + unit] = n;
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    if (lane == 0) {
      ml.inl[(size_t)(2 * r) * NB + book] = (uint32_t)listed[r];
      ml.inl[(size_t)(2 * r + 1) * NB + book] = (uint32_t)(listed[r] >> 32);
    }
  }
}

// pm_math.hpp routines on the device, element-wise (tests only)
__global__ void k_selftest_math(int op, const double* in, double* out, uint64_t n) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double x = in[i];
  out[i] = op == 0 ? pm::exp(x) : (op == 1 ? pm::log(x) : pm::tanh(x));
}

}  // namespace bkd
