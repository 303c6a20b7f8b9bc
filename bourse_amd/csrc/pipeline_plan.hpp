// pipeline_plan.hpp - which kernels a bk_run launches (plain C++17, no HIP): the auto rule, the request modes' fall-backs and
// every per-pipeline choice of the launch code, as one function of the env's shape and settings.  bourse_amd.hip launches
// from it and bk_get_pipeline reports from it; tests/test_pipeline_plan.py checks it on the CPU over a grid of shapes.
#pragma once
#include <algorithm>
#include <cstdint>

namespace bkd {

// AgentSets of Noise / Momentum members on independent books: from this many books the members' update runs one WAVE per
// book with the stream decoded 64 draws at a time (k_agents_mixed_wave, wave_mixed.hpp) in front of the event kernel
constexpr uint32_t MIXED_WAVE_MIN_BOOKS = 512;
// The auto rule for RandomAgents books, derived from the SHAPE (pool registers R = pool / 64) instead of a book count
// swept at one shape (scripts/shape_sweep.py, profiles/r03/shape_sweep.txt: C2 R = 1, C3 R = 2, a 256-slot pool R = 4,
// C5 R = 8, 1 024 .. 65 536 books):
//   * `wave` (k_run_wave: decode + events fused, book in registers across the launch) while the batch fits the chip in
//     ONE residency round of that kernel - asked of the runtime (hipOccupancyMaxActiveBlocksPerMultiprocessor x 8 books
//     per workgroup x CUs: 6 144 books at R <= 2, 4 096 at R = 4, 2 048 at R = 8); one book more and a second round at a
//     fraction of the occupancy costs more than the split form's launches (C3: 103 M at 6 144, 94 M at 7 168 books).
//     64-slot pools are the exception: their book-step is so short that the persistent kernel wins up to the lane split's
//     take-over (C2: 195 M vs 170 M at 8 192, 216 vs 206 at 16 384);
//   * `wave_split` (k_agents_wave + k_step_batch, three parts) from there;
//   * `split` (lane-per-book k_agents_fsm + k_step_batch, four parts) from lane_split_min_books(R): its 125 us chain
//     per step needs that many books to be hidden.  Crossovers re-measured at the end of round 4, after the decode and
//     both event loops got faster (profiles/r04/shape_sweep_crossovers.txt, twice: the second sweep after the decode's last
//     trims and the event waves' priority rule): 26 k / 26.4 - 27.9 k (two boxes) / 25.3 k / 26.5 k books for R = 1, 2, 4, 8 (round 3: 23 k /
//     24.5 k / 18 k / 24.5 k - the 256-slot pools' wave_split gained most: 53 -> 76 M).
// behind the wave-parallel decode the event waves run at priority 1 from this many books (book_device.hpp k_step_batch).  Re-swept
// at the end of round 4: pools of <= 128 slots gain from 8 192 books now (132.5 -> 135.3 M there, +1 % at 12 288; round 3: -2 %
// at 8 192), the 512-slot pools still lose below 16 384 (C5 stand-in 32.0 -> 31.4 M at 8 192)
constexpr uint32_t wave_step_prio_books(int R) { return R <= 2 ? 8192u : 16384u; }
constexpr uint32_t lane_split_min_books(int R) { return R == 4 ? 25600u : (R == 2 ? 27648u : 26624u); }

struct PlanInput {                // what the rule reads of an env
  int R = 1;                      // pool registers per book (pool / 64)
  uint32_t n_books = 0, M = 1;    // M: books per market, 1 = independent books
  bool groups = false;            // RandomAgents groups installed
  uint32_t n_mixed = 0;           // AgentSet members installed
  // the caller's request (bk_set_pipeline / BOURSE_AMD_PIPELINE): 0 auto, 1 fused, 2 split, 3 split with wave-per-book
  // AgentSet members, 4 wave_split, 5 wave; a request the env's agents cannot take (e.g. "wave" for a market) falls back
  int request = 0;
  int n_parts = 4, wave_parts = 0;  // bk_set_split_parts / bk_set_wave_options (wave_parts 0: by the rule)
  uint32_t min_part = 4096;
  uint32_t fused_resident = 0;    // books one residency round of k_run_wave<R> holds on this device (0 = not asked yet)
  uint32_t stagger_us = ~0u;      // BOURSE_AMD_STAGGER_US, ~0 = the default rule
  bool warming = false, step_decode = false;  // bk_warm's scratch steps; BOURSE_AMD_STEP_DECODE
  bool order_log = false;         // bk_set_agent_order_log: the agents' orders are logged (only the split kinds can)
  bool per_book = false;          // bk_set_random_agents_per_book: the groups' parameters come from a per-unit table
  bool members_per_book = false;  // bk_set_agents_per_book: the AgentSet members' parameters come from a per-unit table
};

enum PlanKind {
  PL_FUSED_RANDOM,  // k_run_random: one wave per book, all phases, n_steps per launch (also: no agents = plain steps)
  PL_FUSED_WAVE,    // k_run_wave: wave-parallel decode + events, persistent
  PL_SPLIT_LANES,   // k_agents_fsm (one lane per book / market) + k_step_batch
  PL_SPLIT_WAVE,    // k_agents_wave (one wave per book, stream decoded 64 draws at a time) + k_step_batch
  PL_MIXED_FUSED,   // k_run_mixed: AgentSet members, fused
  PL_MIXED_WAVE,    // k_agents_mixed_wave + k_step_batch<POOLPEND>
  PL_MIXED_LANES,   // k_agents_mixed_lanes + k_step_batch<POOLPEND> (markets' only pipeline; on request otherwise)
  PL_MIXED_WPB,     // k_agents_mixed (one wave per book, scalar) + k_step_batch<POOLPEND> (mode 3, on request)
};

// the agents kernel of a split kind, in front of k_step_batch: none (the fused kinds), k_agents_fsm, k_agents_wave,
// k_agents_mixed_lanes<R, false / true>, k_agents_mixed_wave, k_agents_mixed
enum PlanAgents { AG_NONE, AG_FSM, AG_WAVE, AG_MIXED_LANES, AG_MIXED_LANES_MKT, AG_MIXED_WAVE, AG_MIXED_WPB };

struct Plan {  // every choice the launch code makes; the fused kinds leave all but `kind` at the defaults
  PlanKind kind = PL_FUSED_RANDOM;
  int parts = 1;                 // contiguous parts of the batch, each on a stream of its own from two
  PlanAgents agents = AG_NONE;
  bool step_mkt = false, step_poolpend = false;  // k_step_batch<R, MKT, POOLPEND>
  uint32_t stagger_us = 0;       // parts start i x stagger_us apart; 0 = one agents kernel apart (by events)
  bool step_prio = false;        // the event waves run at priority 1
  bool write_last = false;       // every step writes the latest level-2 record (otherwise only a launch's last one)
  bool step_decode = false;      // k_step_decode<R> takes a part's inner steps: events of step s + decode of step s + 1
  bool step_log = false;         // k_step_batch_log<R, MKT> instead of k_step_batch<R, MKT>: the order log is written
  bool agents_per_book = false;  // the agents kernel (or k_run_wave) is the <R, PB = true> form that reads the per-unit table
  bool members_per_book = false;  // the members' kernel (k_run_mixed or a mixed agents kernel) is its PB form that reads
                                  // the members' per-unit table
};

inline bool is_split(PlanKind k) { return k != PL_FUSED_RANDOM && k != PL_FUSED_WAVE && k != PL_MIXED_FUSED; }

// RandomAgents on independent books: the kinds whose limits depend on fused_resident
inline bool random_books(const PlanInput& in) { return !in.n_mixed && in.M == 1 && in.groups; }

// the last book count k_run_wave takes in auto mode
inline uint32_t wave_fused_max(const PlanInput& in) {
  if (in.R == 1) return lane_split_min_books(1) - 1u;
  const uint32_t res = in.fused_resident ? in.fused_resident : (in.R == 8 ? 2048u : 6144u);
  // (256-slot pools: a round holds 6 144 books like the 128-slot ones, but the split form is already ahead at 5 120 -
  // 37.7 vs 33.8 M - and level at 4 096)
  // (512-slot pools: two workgroups per CU fit since round 4 - 4 096 books - but the split form is 4 % ahead there: 25.4 vs 24.4 M)
  return in.R >= 8 ? std::min(res, 2048u) : (in.R >= 4 ? std::min(res, 4096u) : res);
}

// split pipeline: the batch is cut into n_parts contiguous parts, each on its own stream and started one k_agents_fsm apart,
// so the latency-bound lane-per-book kernel of one part runs under the issue-bound wave-per-book kernel of another
inline int lane_parts(const PlanInput& in) {
  const uint32_t units = in.n_books / in.M;
  return static_cast<int>(std::max(1u, std::min(static_cast<uint32_t>(in.n_parts), units / in.min_part)));
}

inline int wave_parts(const PlanInput& in) {
  if (in.wave_parts > 0)  // set explicitly (tests, sweeps): any batch of >= 64 books per part
    return static_cast<int>(std::max(1u, std::min(static_cast<uint32_t>(in.wave_parts), in.n_books / 64u)));
  // One part per hardware queue (four) once a part holds 2 048 books.  Re-swept in round 4, after the event loops got
  // faster (scripts/exp_c5p.sh): C5 as written 32.3 / 32.8 / 34.0 / 21.9 M in 2 / 3 / 4 / 5 parts (round 3: two parts), C5
  // stand-in 26.1 / 27.0 / 19.3 M in 3 / 4 / 5, the C3 shards 116.7 / 117.7 M (8 192 books) and 140.0 / 139.7 M (16 384) in
  // 3 / 4; a fifth part shares a queue and halves the rate.
  return static_cast<int>(std::max(1u, std::min(4u, in.n_books / 2048u)));
}

inline PlanKind plan_kind(const PlanInput& in) {
  const int mode = in.request;
  if (in.n_mixed) {
    if (in.M == 1 && (mode == 4 || (mode == 0 && in.n_books >= MIXED_WAVE_MIN_BOOKS))) return PL_MIXED_WAVE;
    if (mode == 2 || in.M > 1) return PL_MIXED_LANES;
    if (mode == 3) return PL_MIXED_WPB;
    return PL_MIXED_FUSED;
  }
  if (random_books(in)) {
    if (mode == 5 || (mode == 0 && in.n_books <= wave_fused_max(in))) return PL_FUSED_WAVE;
    if (mode == 4 || (mode == 0 && in.n_books < lane_split_min_books(in.R))) return PL_SPLIT_WAVE;
  }
  // (auto with RandomAgents on independent books never gets here below lane_split_min_books: the wave forms take it)
  if ((mode >= 2 && mode != 5) || in.M > 1 || (mode == 0 && random_books(in))) return PL_SPLIT_LANES;
  return PL_FUSED_RANDOM;
}

inline Plan make_plan(const PlanInput& in) {
  Plan p;
  p.kind = plan_kind(in);
  // the order log of the agents' orders is written by the split forms' event kernel only: a RandomAgents env that logs
  // takes the split form of the fused kind the rule picked (k_run_wave -> wave_split, k_run_random -> split)
  if (in.order_log && in.groups && !in.n_mixed) {
    if (p.kind == PL_FUSED_WAVE) p.kind = PL_SPLIT_WAVE;
    if (p.kind == PL_FUSED_RANDOM) p.kind = PL_SPLIT_LANES;
  }
  // a per-unit parameter table is read by the PB forms of k_run_wave, k_agents_wave and k_agents_fsm; k_run_random (which
  // auto picks only on a "fused" request) has none and takes the lane split instead.  k_step_batch reads only the groups'
  // sizes and assets, which every unit shares.  (bk_warm's scratch steps run the same decoders.)
  p.agents_per_book = in.per_book && in.groups && !in.n_mixed;
  if (p.agents_per_book && p.kind == PL_FUSED_RANDOM) p.kind = PL_SPLIT_LANES;
  // the members' per-unit table: every mixed kind has a PB form, so nothing else of the plan changes
  p.members_per_book = in.members_per_book && in.n_mixed > 0;
  if (!is_split(p.kind)) return p;
  const bool mixed = p.kind != PL_SPLIT_LANES && p.kind != PL_SPLIT_WAVE;
  const bool wave = p.kind == PL_SPLIT_WAVE || p.kind == PL_MIXED_WAVE;  // (both on independent books only)
  p.parts = wave ? wave_parts(in) : lane_parts(in);
  switch (p.kind) {
    case PL_SPLIT_LANES: p.agents = AG_FSM; break;
    case PL_SPLIT_WAVE: p.agents = AG_WAVE; break;
    case PL_MIXED_LANES: p.agents = in.M > 1 ? AG_MIXED_LANES_MKT : AG_MIXED_LANES; break;
    case PL_MIXED_WAVE: p.agents = AG_MIXED_WAVE; break;
    default: p.agents = AG_MIXED_WPB; break;
  }
  p.step_mkt = in.M > 1;
  p.step_poolpend = mixed;
  // by time: i x stagger_us.  The lane split's parts cycle through a ~180 us agents kernel and a ~140 us event kernel; one
  // agents kernel apart (the round-1 rule) puts part 2 at 360 us = almost in phase with part 0 again.  Measured at C3
  // (driver's 20-step regions): 60 us apart 186-189 M first region / 199-201 M later ones against 182 / 192-195 M
  // (BOURSE_AMD_STAGGER_US overrides; other pipelines keep the event-based stagger)
  // (round 3, 20-step regions, first / median of five: 0 us 226 / 229 M, 20 us 240 / 246, 35 us 238 / 244, 50 us 241 / 242,
  // 70 us 235 / 238; no difference over 200 steps)
  p.stagger_us = in.stagger_us != ~0u ? in.stagger_us : ((p.kind == PL_SPLIT_LANES && p.parts >= 3) ? 30u : 0u);
  p.step_prio = wave && in.n_books / in.M >= wave_step_prio_books(in.R);
  // the lane-per-book members' update reads the touches from the latest level-2 record: keep it current
  p.write_last = p.kind == PL_MIXED_LANES || p.kind == PL_MIXED_WAVE;
  // (experiment, docs/EXPERIMENTS.md: BOURSE_AMD_STEP_DECODE=1 runs a part's inner steps of the wave_split pipeline as ONE
  // launch each - k_step_decode = events of step s + decode of step s + 1)
  // (bk_warm's scratch steps leave the log alone: they run the log-less kernel and the books are put back)
  p.step_log = in.order_log && !in.warming;
  p.step_decode = in.step_decode && p.kind == PL_SPLIT_WAVE && !in.warming && !p.step_log && !p.agents_per_book;
  return p;
}

}  // namespace bkd
