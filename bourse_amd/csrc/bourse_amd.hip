// bourse_amd.hip — C ABI (include/bourse_amd.h) over the gfx950 kernels in book_device.hpp.
//
// Host side of the drop-in boundary: owns the device state of B independent books, keeps the
// host-visible half of `bourse_de::Env` (order creation, id assignment, the per-step event
// queue — crates/step_sim/src/env.rs:166-219) and launches the step kernels.  There is no CPU
// execution path: without a usable GPU every entry point fails with BK_NO_DEVICE.  Which kernels a bk_run launches is
// decided in pipeline_plan.hpp (make_plan); the launch code here only follows that plan.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <atomic>
#include <condition_variable>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "../../include/bourse_amd.h"
#include "book_device.hpp"
// k_agents_fsm is compiled in its own unit (fsm_unit.hip: another machine-scheduler strategy); only declared here
namespace bkd {
extern template __global__ void k_agents_fsm<1>(DevArgs);
extern template __global__ void k_agents_fsm<2>(DevArgs);
extern template __global__ void k_agents_fsm<4>(DevArgs);
extern template __global__ void k_agents_fsm<8>(DevArgs);
extern template __global__ void k_agents_fsm<1, true>(DevArgs, const Group*);
extern template __global__ void k_agents_fsm<2, true>(DevArgs, const Group*);
extern template __global__ void k_agents_fsm<4, true>(DevArgs, const Group*);
extern template __global__ void k_agents_fsm<8, true>(DevArgs, const Group*);
}  // namespace bkd
#include "host_math.hpp"
#include "agent_table.hpp"
#include "host_pool.hpp"
#include "hist_cursor.hpp"
#include "pipeline_plan.hpp"
#include "mixed_agents.hpp"
#include "wave_agents.hpp"
#include "wave_mixed.hpp"
#include "step_events.hpp"
#include "agents_ingress.hpp"
#include "members_ingress.hpp"
#include "market_ingress.hpp"
#include "book_reset.hpp"
#include "ingress_reset.hpp"
#include "accounts.hpp"
#include "trade_bars.hpp"
#include "depth.hpp"
#include "candles.hpp"
#include "series.hpp"
#include "open_orders.hpp"
#include "open_queue.hpp"
#include "quotes_ingress.hpp"
#include "retune.hpp"
#include "stamp_compact.hpp"
#include "lags.hpp"
#include "bins.hpp"
#include "cross.hpp"
#include "flow.hpp"

using namespace bkd;

static_assert(sizeof(DevStats) == sizeof(bk_stats), "bk_stats layout");
static_assert(sizeof(OutTrade) == sizeof(bk_trade), "bk_trade layout");
static_assert(sizeof(bk_config) == 72 && sizeof(bk_random_agents) == 28 && sizeof(bk_trade) == 40 &&
                  sizeof(bk_order) == 48,
              "C ABI struct layout (mirrored by bourse_amd/_lib.py)");
static_assert(sizeof(bk_agent_desc) == 104, "bk_agent_desc layout (mirrored by bourse_amd/_lib.py)");
static_assert(sizeof(bk_account) == 32 && sizeof(bk_account) == 2 * sizeof(bk_u32x4) &&
                  accounts::FLAG_ACCOUNTS_INEXACT == BK_FLAG_ACCOUNTS_INEXACT,
              "bk_account layout / flag (accounts.hpp)");
static_assert(sizeof(bk_trade_bar) == 48 && sizeof(bk_trade_bar) == trade_bars::ROW_VECS * sizeof(bk_u32x4),
              "bk_trade_bar layout (trade_bars.hpp)");
static_assert(sizeof(bk_series_row) == 192 && sizeof(bk_series_row) == series::ROW_VECS * sizeof(bk_u32x4) &&
                  sizeof(bk_series_row) == series::ROW_WORDS * 8 && offsetof(bk_series_row, carry_m) == series::CARRY_M * 8 &&
                  offsetof(bk_series_row, min_m) == series::MIN_M * 8 && offsetof(bk_series_row, sum_d4_lo) == series::SUM_D4_LO * 8,
              "bk_series_row layout (series_fold.hpp)");
static_assert(sizeof(bk_lag_row) == 80 && sizeof(bk_lag_row) == lags::ROW_VECS * sizeof(bk_u32x4) &&
                  sizeof(bk_lag_row) == lags::ROW_WORDS * 8 && offsetof(bk_lag_row, n_h) == lags::N_H * 8 &&
                  offsetof(bk_lag_row, sum_h4_lo) == lags::SUM_H4_LO * 8 && offsetof(bk_lag_row, max_abs_h) == lags::MAX_ABS_H * 8,
              "bk_lag_row layout (lag_fold.hpp)");
static_assert(BK_FLOW_BASE_WORDS == flow::BASE_WORDS && BK_FLOW_LAG_WORDS == flow::LAG_WORDS && BK_FLOW_N_LOST == flow::N_LOST &&
                  BK_FLOW_SUM_DP2 == flow::SUM_DP2 && flow::BASE_WORDS * 8 == flow::BASE_VECS * sizeof(bk_u32x4) &&
                  flow::LAG_WORDS * 8 == flow::LAG_VECS * sizeof(bk_u32x4),
              "the flow table's words (flow_fold.hpp)");
static_assert(sizeof(bk_bins_config) == 36 && offsetof(bk_bins_config, spans) == 8 && offsetof(bk_bins_config, ret_width) == 24 &&
                  sizeof(static_cast<bk_bins_config*>(nullptr)->spans) == bins::MAX_SPANS * 4,
              "bk_bins_config layout (bin_fold.hpp)");
static_assert(sizeof(bk_cross_row) == 64 && sizeof(bk_cross_row) == cross::ROW_VECS * sizeof(bk_u32x4) &&
                  sizeof(bk_cross_row) == cross::ROW_WORDS * 8 && offsetof(bk_cross_row, sum_xx) == cross::SUM_XX * 8 &&
                  offsetof(bk_cross_row, sum_xy) == cross::SUM_XY * 8 && offsetof(bk_cross_row, sum_lead) == cross::SUM_LEAD * 8,
              "bk_cross_row layout (cross_fold.hpp)");
static_assert(sizeof(bk_cross_config) == 20 && offsetof(bk_cross_config, spans) == 4 &&
                  sizeof(static_cast<bk_cross_config*>(nullptr)->spans) == cross::MAX_SPANS * 4 && static_cast<int>(cross::MAX_ASSETS) == MAX_ASSETS,
              "bk_cross_config layout / the assets of a market (cross_fold.hpp)");
static_assert(sizeof(bk_open_summary) == 32 && sizeof(bk_open_summary) == 2 * sizeof(bk_u32x4) &&
                  sizeof(bk_open_order) == 16 && sizeof(bk_open_order) == sizeof(bk_u32x4) &&
                  sizeof(open_orders::Summary) == sizeof(bk_open_summary) && sizeof(open_orders::Entry) == sizeof(bk_open_order),
              "bk_open_summary / bk_open_order layout (open_orders.hpp)");
static_assert(sizeof(bk_open_queue) == 32 && sizeof(bk_open_queue) == 2 * sizeof(bk_u32x4) &&
                  sizeof(open_queue::Row) == sizeof(bk_open_queue) && open_queue::NO_ORDER == open_orders::NO_ORDER,
              "bk_open_queue layout (open_queue.hpp)");
static_assert(sizeof(bk_quote) == 16 && sizeof(bk_quote) == sizeof(bk_u32x4) && sizeof(quotes::Quote) == sizeof(bk_quote) &&
                  quotes::KEEP == BK_QUOTE_KEEP && quotes::ACT_MODIFY == BK_ACTION_MODIFY && quotes::ACT_MODIFY == ING_ACTION_MODIFY &&
                  quotes::NO_ORDER == open_orders::NO_ORDER,
              "bk_quote layout / constants (quote_rows.hpp)");
static_assert(sizeof(DevTrade) == 32 && sizeof(DevOrderLog) == 48 && sizeof(uint4) == 16, "device record layout");

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

#define HIPCHK(expr)                                                                              \
  do {                                                                                            \
    hipError_t _e = (expr);                                                                       \
    if (_e != hipSuccess)                                                                         \
      return fail(BK_HIP_ERROR, std::string(#expr) + ": " + hipGetErrorString(_e));               \
  } while (0)

struct HostOrder {  // immutable half of an order, fixed at create_order (orderbook.rs:356-396)
  uint8_t bid;
  uint32_t start_vol, price, trader;
  uint64_t create_time;
};
struct HostEvent {
  uint32_t word, id, price, vol;
};
static_assert(sizeof(HostEvent) == 16, "HostEvent is uploaded as one uint4 per event");
struct BookHost {
  std::vector<HostOrder> orders;
  std::vector<HostEvent> queue;
  std::vector<DevOrderLog> log_cache;
  uint64_t n_uploaded = 0;  // orders whose New event has reached the device
  uint64_t time_offset = 0;  // set by bk_set_time: book time = start_time + steps_done * step_size + time_offset (wrapping)
  bool log_fresh = false;
  uint64_t mirror_epoch = ~0ull;  // device-resident ingress: `orders` mirrors the device's records as of this ingest epoch
};

template <class T>
struct DevBuf {
  T* p = nullptr;
  size_t n = 0;
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
  hipError_t alloc(size_t count) {
    if (p) (void)hipFree(p);
    p = nullptr;
    n = count;
    if (count == 0) return hipSuccess;
    return hipMalloc(reinterpret_cast<void**>(&p), count * sizeof(T));
  }
  // Replace this buffer by a freshly made one: `other` leaves with the previous block and frees it at its scope's exit.
  void swap(DevBuf& other) {
    std::swap(p, other.p);
    std::swap(n, other.n);
  }
};

// A host table on its way to a kernel of the env's stream: caller -> pinned block (before the call returns) -> device block
// (on the stream).  `copied` is recorded behind every upload: once it has passed, the pinned block may be written again.
struct HostStage {
  DevBuf<unsigned char> dev;
  unsigned char* pin = nullptr;
  size_t bytes = 0;  // of either block
  hipEvent_t copied = nullptr;
  ~HostStage() {
    if (pin) (void)hipHostFree(pin);
    if (copied) (void)hipEventDestroy(copied);
  }
  // Room for n bytes in both blocks, the pinned one free to write.  Blocks that are too small are replaced (they only grow);
  // `drain`: an earlier call's kernel on `stream` may still read the device block replaced here, so wait for the stream.
  int reserve(size_t n, hipStream_t stream, bool drain) {
    if (n <= bytes) {
      HIPCHK(hipEventSynchronize(copied));  // the call before this one has been uploaded: the pinned rows are free
      return BK_OK;
    }
    if (copied) HIPCHK(hipEventSynchronize(copied));
    if (drain) HIPCHK(hipStreamSynchronize(stream));
    DevBuf<unsigned char> fresh;
    HIPCHK(fresh.alloc(n));
    void* fresh_pin = nullptr;
    HIPCHK(hipHostMalloc(&fresh_pin, n, hipHostMallocDefault));
    if (!copied && hipEventCreateWithFlags(&copied, hipEventDisableTiming) != hipSuccess) {
      (void)hipHostFree(fresh_pin);
      return fail(BK_HIP_ERROR, "hipEventCreateWithFlags failed");
    }
    if (pin) (void)hipHostFree(pin);
    pin = static_cast<unsigned char*>(fresh_pin);
    bytes = n;
    dev.swap(fresh);
    return BK_OK;
  }
  // the first n bytes of the pinned block -> the device block, on `stream`
  int upload(size_t n, hipStream_t stream) {
    HIPCHK(hipMemcpyAsync(dev.p, pin, n, hipMemcpyHostToDevice, stream));
    HIPCHK(hipEventRecord(copied, stream));
    return BK_OK;
  }
};

}  // namespace

// One table folded from the level-2 history ring by a host cursor - the series moments, the lag table, the bin table, and
// beside those three per-book tables the per-market cross table.  What they share is written once over this struct (the
// cursor's rule is hist_cursor.hpp's); what differs is how a table's fold over a span of the ring and its clear are launched.
struct HistTable {
  const char* noun;     // in the lost steps' message: "of the <noun> were lost"
  const char* name;     // in the guard's: "this env has no <name>"
  const char* article;  // in bk_load_book's refusal: "with <article><name>"
  const char* prefix;   // its entries are bk_<prefix>_enable, bk_<prefix>_clear, ..
  void (*fold)(bk_env*, const ring::Span&);  // steps [seen, seen + n) of every book, all retained
  // rows (and carry) of the masked books (one mask byte per M books; nullptr: every book) -> cleared, or only their carry
  void (*clear)(bk_env*, const uint8_t* mask_dev, uint32_t M, bool carry_only);
  bool on = false;
  uint64_t seen = 0;     // steps below it are folded (a host integer, as steps_done)
  DevBuf<uint8_t> mask;  // bk_<prefix>_clear: device staging of the host mask [n_books / clear_M]
  uint32_t clear_M = 1;  // books per mask byte of bk_<prefix>_clear[_device] (the cross table's unit is the market: env->M)
};
enum { T_SERIES, T_LAGS, T_BINS, N_HIST_TABLES };
enum { T_CROSS = N_HIST_TABLES };  // the per-market table: bk_env::cross_table, beside the three per-book tables[]
static void launch_series_fold(bk_env*, const ring::Span&);
static void launch_series_clear(bk_env*, const uint8_t*, uint32_t, bool);
static void launch_lags_fold(bk_env*, const ring::Span&);
static void launch_lags_clear(bk_env*, const uint8_t*, uint32_t, bool);
static void launch_bins_fold(bk_env*, const ring::Span&);
static void launch_bins_clear(bk_env*, const uint8_t*, uint32_t, bool);
static void launch_cross_fold(bk_env*, const ring::Span&);
static void launch_cross_clear(bk_env*, const uint8_t*, uint32_t, bool);

struct bk_env {
  bk_config cfg{};
  int R = 1;
  uint32_t M = 1;  // books per market (MarketEnv<ASSETS>): cfg.assets, 1 = independent books
  uint32_t asset_tick[MAX_ASSETS] = {0, 0, 0, 0, 0, 0, 0, 0};
  uint32_t W = 0, stride = 0;
  hipStream_t stream = nullptr;
  DevBuf<uint32_t> state, l2_last, hist, ev_off, batch;
  DevBuf<uint4> ev;               // this step's events, 16 B each (HostEvent layout), CSR by book / market
  HostEvent* ev_stage = nullptr;  // pinned staging of the same (uploaded at link speed)
  uint32_t* off_stage = nullptr;
  uint32_t batch_stride = 0;
  int pipeline = 0;  // the caller's request, 0 auto .. 5 (pipeline_plan.hpp PlanInput::request)
  DevBuf<uint32_t> warm_snap;         // bk_warm: state + L2 copy of the scratch steps
  bool warming = false;               // bk_warm's scratch steps: no history slots, no trade records
  // bk_snapshot_save: device-resident copies of state + l2_last that bk_reset_books* put chosen books back to, each with
  // the ckpt_header words (shape, agent set) of the env as it was saved
  struct Snapshot {
    DevBuf<uint32_t> buf;
    bool used = false;
    uint64_t shape[4] = {0, 0, 0, 0};  // ckpt_header h[2..5]
    uint64_t stamp_bound = 0;          // the env's stamp_room.bound as it was saved
  } snaps[BK_MAX_SNAPSHOTS];
  DevBuf<uint8_t> reset_mask;    // bk_reset_books: device staging of the host mask / seeds [n_units]
  DevBuf<uint64_t> reset_seeds;
  // bk_ingress_snapshot_save: slots of their own for a device-ingress env - the two arrays above, the order records of the
  // ids the books had handed out ([n_books][n_keep] of dorders and order_log) and the agents' / members' per-book rows
  // (ingress_reset.hpp), with the env's shape, its agent set and the count of bk_set_*agents* calls as it was saved
  struct IngressSnapshot {
    DevBuf<uint32_t> buf;
    DevBuf<uint4> orders, log;
    uint32_t n_keep = 0, keep_cap = 0;  // ids per book held / allocated
    DevBuf<uint32_t> held, lists, lens, mflags;
    DevBuf<uint64_t> mstate;
    bool held_saved = false, members_saved = false;  // false: the env had not made these buffers yet (every agent holds None)
    bool used = false;
    uint64_t shape[4] = {0, 0, 0, 0};  // ckpt_header h[2..5]
    uint64_t installs = 0;
    uint64_t bytes = 0;
    uint64_t stamp_bound = 0;  // the env's stamp_room.bound as it was saved
  } isnaps[BK_MAX_SNAPSHOTS];
  DevBuf<uint32_t> reset_list;  // [n_units] the masked units of one ingress reset, then its counter (k_collect_units)
  int reset_blocks = 0;         // k_reset_records' fixed grid: 4 blocks of 4 waves per CU
  // bk_accounts_enable: per-trader rows [n_books][acct_traders] of 32 B and the per-book cursors (accounts.hpp)
  DevBuf<bk_u32x4> acct;
  DevBuf<unsigned long long> acct_seen;
  DevBuf<uint8_t> acct_mask;  // bk_accounts_clear: device staging of the host mask [n_books]
  uint32_t acct_traders = 0;  // 0: no accounts
  bool acct_consume = false;
  // bk_trade_bars_enable: per-step bars [n_books][bars_window] of 48 B and the per-book cursors (trade_bars.hpp)
  DevBuf<bk_u32x4> bars;
  DevBuf<unsigned long long> bars_seen;
  DevBuf<uint8_t> bars_mask;  // bk_trade_bars_clear: device staging of the host mask [n_books]
  uint32_t bars_window = 0;   // 0: no bars
  bool bars_consume = false;
  // bk_flow_enable: 8 + 6 flow_lags words per book [n_books][4 + 3 K] vectors, the carry [n_books][K] and the per-book
  // cursors (flow.hpp)
  DevBuf<bk_u32x4> flow_table;
  DevBuf<uint64_t> flow_carry;
  DevBuf<unsigned long long> flow_seen;
  DevBuf<uint8_t> flow_mask;  // bk_flow_clear: device staging of the host mask [n_books]
  uint32_t flow_lags = 0;     // 0: no flow table
  bool flow_consume = false;
  // the three per-book tables folded from the history ring (HistTable above), the per-market one beside
  // them (2.29), and what each keeps on the device:
  HistTable tables[N_HIST_TABLES] = {
      {"series", "series moments", "", "series", launch_series_fold, launch_series_clear},
      {"lag table", "lag table", "a ", "lags", launch_lags_fold, launch_lags_clear},
      {"bin table", "bin table", "a ", "bins", launch_bins_fold, launch_bins_clear}};
  HistTable cross_table = {"cross table", "cross table", "a ", "cross", launch_cross_fold, launch_cross_clear};
  // bk_series_enable: one row of series moments per book [n_books] of 192 B (series.hpp)
  DevBuf<bk_u32x4> series_rows;
  // bk_depth_enable: the series' companion over the ladder, (levels + 1) rows of 128 B per book [n_books][L + 1][8] vectors
  // and the carry [n_books][L + 1] (depth.hpp); folded, cleared and cut by the series' two launches, with no cursor of its own
  DevBuf<bk_u32x4> depth_rows;
  DevBuf<uint64_t> depth_carry;
  // bk_candles_enable: the series' other companion, the last candle_n bars of candle_width steps per book [n_books][N][8]
  // vectors of 128 B a bar and the carry [n_books] (candles.hpp); folded, cleared and cut by the series' two launches too
  DevBuf<bk_u32x4> candle_rows;
  DevBuf<uint64_t> candle_carry;
  uint32_t candle_width = 0, candle_n = 0;
  // bk_lags_enable: n_lags rows per book [n_books][n_lags] of 80 B and the carry [n_books][n_lags + 1] (lags.hpp)
  DevBuf<bk_u32x4> lag_rows;
  DevBuf<uint64_t> lag_carry;
  uint32_t n_lags = 0;
  // bk_bins_enable: (n_spans + 2) rows of n_bins counts per book [n_books][C][B] and the carry [n_books][bins_kmax] (bins.hpp)
  DevBuf<uint64_t> bin_rows;
  DevBuf<uint64_t> bins_carry;
  bk_bins_config bins_cfg{};
  uint32_t bins_kmax = 0;  // the longest span
  // bk_cross_enable: n_spans * assets * assets rows per MARKET [n_markets][S][A][A] of 64 B and the carry
  // [n_markets][A][2 * cross_hmax] (cross.hpp)
  DevBuf<bk_u32x4> cross_rows;
  DevBuf<uint64_t> cross_carry;
  bk_cross_config cross_cfg{};
  uint32_t cross_hmax = 0;  // the longest span
  // bk_open_orders_enable: every trader's resting orders per book, recomputed from the pool behind every step (open_orders.hpp)
  DevBuf<bk_u32x4> open_summary;  // [n_books][open_traders][2]
  DevBuf<bk_u32x4> open_entries;  // [n_books][open_traders][open_depth]; empty with open_depth == 0
  uint32_t open_traders = 0, open_depth = 0;  // open_traders == 0: no view
  // bk_open_queue_enable: the queue position of every entry above, recomputed right behind them (open_queue.hpp)
  DevBuf<bk_u32x4> open_queue;  // [n_books][open_traders][open_depth][2]; empty: no queue view
  // bk_submit_quotes: the host table's staging, [n_books][open_traders] rows, made at the first call
  HostStage quote_stage;
  // bk_retune_*: the count of refused units (device), the members' installed first trader ids as the kernel compares them
  // (uploaded by the per-unit install, synchronously like its table), and the host forms' staging: rows then mask, made at the
  // first call and grown only by a wider table
  DevBuf<unsigned long long> retune_count;
  DevBuf<uint32_t> retune_id0;  // [units][n_mixed], uploaded by bk_set_agents_per_book beside the table
  HostStage retune_stage;
  uint64_t agent_installs = 0;  // bk_set_*agents* calls: each marks the held ids / the members' lists stale
  DevBuf<uint4> jump_tabs;      // k_agents_wave: T^256 (block jump) then T^(4 << b), b = 0..5 (lane offsets): 7 x 8 KB
  DevBuf<uint32_t> wcache;      // k_agents_wave: per-book lane states of the RNG block in progress
  uint32_t wave_lookahead = 64;
  uint32_t stagger_us = ~0u;    // parts of a split launch start i x stagger_us apart; ~0 = default rule, 0 = by events
  int wave_parts = 0;           // bk_set_wave_options: 0 = by the rule (pipeline_plan.hpp wave_parts)
  // AgentSets with Noise / Momentum members on independent books: wave-parallel decode of the members' update
  bool wl_valid = false;    // the wave-per-book members' lists (wl_list) describe the pools as of steps_done
  DevBuf<uint16_t> wl_list;    // [n_books][MAX_MEMBERS][pool]: k_agents_mixed_wave's lists, book-major
  DevBuf<uint32_t> wl_len;
  bool mw_attr_set = false;
  uint32_t fused_resident = 0;   // books one residency round of k_run_wave<R> holds on this device (0 = not asked yet)
  bool step_decode = false;      // BOURSE_AMD_STEP_DECODE (pipeline_plan.hpp)
  bool fsm_compiled_loop = false;  // BOURSE_AMD_FSM_LOOP=compiled: k_agents_fsm<R> runs its C++ draw loop, not fsm_asm.hpp's
  // split pipeline geometry (pipeline_plan.hpp lane_parts)
  int n_parts = 4;  // one per hardware queue (part_streams)
  uint32_t min_part = 4096;  // books (markets) per part below which the batch is cut in fewer parts
  static constexpr int MAX_PARTS = 8;
  hipStream_t part_stream[MAX_PARTS] = {};
  hipEvent_t ev_fork = nullptr, ev_first[MAX_PARTS] = {}, ev_join[MAX_PARTS] = {};
  DevBuf<DevTrade> trades;
  DevBuf<DevOrderLog> order_log;
  DevBuf<DevStats> stats;
  DevBuf<OutTrade> tr_dense;           // bk_trades_compact: dense record stream + CSR offsets
  DevBuf<unsigned long long> tr_off;
  uint64_t tr_total = 0;
  DevBuf<MixedDesc> mixed_descs;  // AgentSets with Noise/Momentum members (k_run_mixed)
  // bk_set_agents_per_book: the per-unit table of the members (unit u = book u, or market u), mtable[u * n_mixed + i], on
  // the host (the hash) and on the device (the PB kernels); mixed_descs then holds unit 0's row, whose kinds, sizes and
  // assets every unit shares (what k_mixed_lists_rebuild / k_wave_lists_rebuild read)
  std::vector<MixedDesc> mtable;
  DevBuf<MixedDesc> dmtable;
  uint32_t n_mixed = 0, n_fixed = 0;
  // lane-per-book members' update (k_agents_mixed_lanes): the members' order lists, [member][entry][book]
  DevBuf<uint16_t> ml_list;
  DevBuf<uint32_t> ml_len, ml_inl;
  bool lds_attr_set = false;  // hipFuncAttributeMaxDynamicSharedMemorySize applied on this env's device
  DevBuf<uint64_t> gather_buf;  // n_books u64: gather_header()
  bool fsm_attr_set = false;  // same for k_agents_fsm (its LDS is dynamic: book_device.hpp)
  bool ml_valid = false;  // the lists describe the pool as of steps_done (false after a wave-per-book launch / restore)
  uint32_t member_asset[MAX_INGRESS_MEMBERS] = {0, 0, 0, 0, 0, 0, 0, 0};
  uint32_t n_fixed_a[MAX_ASSETS] = {0, 0, 0, 0, 0, 0, 0, 0};
  MixedLists lists() const {
    return MixedLists{ml_list.p, ml_len.p, ml_inl.p, static_cast<uint32_t>(R) * 64u, cfg.n_books, cfg.n_books / M};
  }
  MixedArgs margs() const {
    MixedArgs ma{};
    ma.descs = mixed_descs.p;
    ma.n_desc = n_mixed;
    ma.n_fixed = n_fixed;
    for (int i = 0; i < MAX_MEMBERS; ++i) ma.asset[i] = member_asset[i];
    for (int i = 0; i < MAX_ASSETS; ++i) ma.n_fixed_a[i] = n_fixed_a[i];
    return ma;
  }
  std::vector<BookHost> books;
  std::unique_ptr<HostPool> pool;  // host threads for large host-driven batches (created on first use)
  HostPool& host_pool() {
    if (!pool) {
      unsigned nt = std::min<unsigned>(std::max(1u, std::thread::hardware_concurrency()), 16u);
      if (const char* e = std::getenv("BOURSE_AMD_HOST_THREADS")) nt = static_cast<unsigned>(std::max(1, std::atoi(e)));
      pool.reset(new HostPool(nt - 1));
    }
    return *pool;
  }
  std::vector<Group> groups;
  // bk_set_random_agents_per_book: the per-unit table (unit u = book u, or market u), table[u * n_groups + g], on the host
  // (the hash) and on the device (the PB kernels); `groups` then holds unit 0's row, whose sizes and assets every unit shares
  std::vector<Group> table;
  DevBuf<Group> dtable;
  uint32_t n_agents_total = 0;
  uint64_t agents_hash = 0;   // FNV-1a of the installed agent set (checkpoint compatibility)
  // device-resident instruction ingress (bk_device_ingress_enable): the queues, the id counters and the immutable halves of
  // the orders live on the device; the per-order host entries are refused, the readers mirror on demand
  bool device_ingress = false;
  uint32_t qcap = 0;               // events per book (market) and step
  DevBuf<uint4> dq, dorders;       // [n_markets][qcap] event records; [n_books][max_orders][2] immutable halves
  DevBuf<uint32_t> dqlen;          // [n_markets] queue lengths
  uint64_t ingest_epoch = 0;       // bumped by every submit / step: invalidates the readers' mirrors
  // bk_update_agents: the RandomAgents' held order ids [n_books][n_agents_total] and, for the uniform set, its groups on the
  // device; re-made (all None) at the first bk_update_agents after a bk_set_random_agents* call
  DevBuf<uint32_t> agent_held;
  DevBuf<Group> agent_groups;
  bool agent_held_stale = true;
  // bk_update_members: the members' `orders` lists [n_books][n_mixed][member_list_cap] (a RandomAgents member's row holds its
  // agents' held ids) with their lengths, MomentumAgent's momentum / last_price [n_books][n_mixed][2] and "has a last
  // price" bits [n_books], the members' first trader ids as the kernel reads them; re-made (empty lists, no momentum
  // state) at the first bk_update_members after a bk_set_agents* call
  DevBuf<uint32_t> member_lists, member_lens, member_flags, member_id0_dev;
  DevBuf<uint64_t> member_state;
  std::vector<uint32_t> member_id0;    // [units or 1][n_mixed] agent_id_start, as installed
  std::vector<uint32_t> member_type, member_n;  // [n_mixed] kinds and sizes (every unit shares them)
  uint32_t member_list_cap = 0;
  bool member_lists_stale = true;
  // bk_set_agent_order_log: bk_run's RandomAgents record their orders in dorders / order_log (k_step_batch_log); the
  // readers mirror them like the device ingress's
  bool agent_log = false;
  // HOST arrays through the device ingress (bk_submit_instructions_host): two slots of pinned + device staging, the
  // upload of ticket t + 1 on a copy stream of its own under the step kernel of ticket t, ids / status back on a third
  struct HostIngress {
    static constexpr int SLOTS = 2;
    size_t cap = 0;                 // elements per slot
    char* pin[SLOTS] = {nullptr, nullptr};
    char* dev[SLOTS] = {nullptr, nullptr};
    hipStream_t in = nullptr, out = nullptr;
    hipEvent_t e_h2d[SLOTS] = {}, e_ing[SLOTS] = {}, e_done[SLOTS] = {};
    uint64_t ticket_of[SLOTS] = {~0ull, ~0ull};  // the ticket whose arrays / results a slot holds
    uint64_t n_elem[SLOTS] = {0, 0};
    uint64_t next_ticket = 0;
    // pinned blocks a growth replaced: a view of their tickets' results (bk_submit_result_view) stays valid until two more
    // submits, so they are freed only then (they were freed at once and the views dangled)
    struct Retired {
      char* pin;
      uint64_t free_from_ticket;  // freed by the submit that takes this ticket (or by bk_env_destroy)
    };
    std::vector<Retired> retired;
    // one slot = [offsets (B + 1) u64 | order_id cap u64 | out_ids cap u64 | status 2 B u32 | action | vol | trader | price
    // cap u32 each | side cap u8], the same layout in pinned and in device memory
    size_t o_off = 0, o_oid = 0, o_out = 0, o_st = 0, o_act = 0, o_vol = 0, o_trd = 0, o_prc = 0, o_side = 0, bytes = 0;
    void layout(size_t B, size_t c) {
      cap = c;
      o_off = 0;
      o_oid = o_off + (B + 1) * 8;
      o_out = o_oid + c * 8;
      o_st = o_out + c * 8;
      o_act = o_st + B * 8;
      o_vol = o_act + c * 4;
      o_trd = o_vol + c * 4;
      o_prc = o_trd + c * 4;
      o_side = o_prc + c * 4;
      bytes = (o_side + c + 63) & ~size_t(63);
    }
  } hi;
  bool ev_seq_shuffle = false;  // measurement knobs of k_step_events' shuffle, from the environment at bk_env_create:
  int ev_shuffle_min = -1;      // draw by draw always / the queue length the wave-parallel form starts at (-1: the rule)
  std::atomic<bool> ev_mods_seen{false};  // a modification was submitted to this env (sticky): k_step_events<.., MODS = true> from then on
  uint32_t* mods_flag_host = nullptr;     // device ingress: k_ingest's hint word in mapped host memory, and its device address
  uint32_t* mods_flag_dev = nullptr;
  bool device_flow = false;   // bk_run has stepped this env with on-device agents: host-driven orders are refused
  uint64_t steps_done = 0, hist_base = 0;
  // the books' arrival stamps (H_SEQ, pool field 3) never straddle a wrap: the host's upper bound of the largest H_SEQ,
  // raised before every launch by the most orders one book can rest in it, and the compaction queued in front of a launch
  // that could pass the limit (stamp_rows.hpp; reserve_stamps)
  bkd::stamps::Room stamp_room;
  uint64_t stamp_compactions = 0;  // launches of the compaction so far (bk_stamp_compactions)
  uint32_t trading = 1;
  size_t ev_capacity = 0;
  // profiling
  int profile = 0;       // 0 off, N: HIP-event-time the kernels of every Nth step
  uint64_t prof_tick = 0;  // steps seen while profiling
  bool prof_now = false;
  struct ProfEv {
    hipEvent_t a, b;
    int kind;
  };
  std::vector<ProfEv> prof_events;
  double prof_bracket_ms = 0;  // what two events recorded back to back on a stream read (calibrated, subtracted)
  std::vector<hipEvent_t> prof_pool;  // events created ahead of the launches that use them
  hipEvent_t prof_event() {
    hipEvent_t e = nullptr;
    if (!prof_pool.empty()) {
      e = prof_pool.back();
      prof_pool.pop_back();
    } else if (hipEventCreate(&e) != hipSuccess) {
      e = nullptr;
    }
    return e;
  }
  // per kernel kind: 0 the fused kernels, 1 the agents kernel of a split pipeline, 2 k_step_batch, 3 k_step_events
  static constexpr int PROF_KINDS = 4;
  double prof_ms[PROF_KINDS] = {0, 0, 0, 0};
  uint64_t prof_launches[PROF_KINDS] = {0, 0, 0, 0};

  DevArgs args() const {
    DevArgs a{};
    a.n_books = cfg.n_books;
    a.levels = cfg.levels;
    a.tick_size = cfg.tick_size;
    a.n_groups = static_cast<uint32_t>(groups.size());
    a.step_lo = static_cast<uint32_t>(cfg.step_size);
    a.step_hi = static_cast<uint32_t>(cfg.step_size >> 32);
    a.state_stride = stride;
    a.l2_width = W;
    a.trade_cap = warming ? 0u : cfg.trade_capacity;
    a.hist_cap = warming ? 0u : cfg.history_capacity;
    a.hist_slot0 = a.hist_cap ? static_cast<uint32_t>(steps_done % cfg.history_capacity) : 0u;
    a.step_prio = 0;
    a.n_agents_total = n_agents_total;
    a.log_cap = cfg.max_orders;
    a.state = state.p;
    a.l2_last = l2_last.p;
    a.hist = hist.p;
    a.trades = trades.p;
    a.order_log = order_log.p;
    a.ev_off = ev_off.p;
    a.ev = device_ingress ? dq.p : ev.p;
    a.ev_len = device_ingress ? dqlen.p : nullptr;
    a.ev_stride = qcap;
    a.fsm_loop = fsm_compiled_loop ? 1u : 0u;
    a.batch = batch.p;
    a.batch_stride = batch_stride;
    a.book_begin = 0;
    a.book_end = cfg.n_books / M;
    a.assets = M;
    for (int i = 0; i < MAX_ASSETS; ++i) a.asset_tick[i] = asset_tick[i];
    auto dv = [](uint32_t d) {
      const HostUDiv h = make_udiv(d ? d : 1u);
      return UDiv{h.m, h.sh1, h.sh2, h.d};
    };
    a.tick_div = dv(cfg.tick_size);
    for (int i = 0; i < MAX_ASSETS; ++i) a.asset_div[i] = dv(asset_tick[i]);
    for (size_t g = 0; g < groups.size(); ++g) a.groups[g] = groups[g];
    return a;
  }
  // the queues and order records bk_update_agents' and bk_update_members' kernels write into
  IngressArgs ingress_args() const {
    return IngressArgs{state.p, stride, cfg.max_orders, qcap, dq.p, dqlen.p, dorders.p, order_log.p};
  }
};

namespace {

int use_device(bk_env* env) {
  HIPCHK(hipSetDevice(env->cfg.device));
  return BK_OK;
}

struct ProfScope {  // HIP events around a launch on the env's stream
  bk_env* env;
  int kind;
  hipStream_t st;
  hipEvent_t a = nullptr, b = nullptr;
  ProfScope(bk_env* e, int k, hipStream_t s = nullptr) : env(e), kind(k), st(s ? s : e->stream) {
    if (env->prof_now && hipEventCreate(&a) == hipSuccess && hipEventCreate(&b) == hipSuccess)
      (void)hipEventRecord(a, st);
  }
  ~ProfScope() {
    if (a && b) {
      (void)hipEventRecord(b, st);
      env->prof_events.push_back({a, b, kind});
    }
  }
};

// A launch of the multi-stream pipelines, timed - when it is sampled - by two events recorded on its stream.
template <typename K, typename... Args>
void launch_timed(bk_env* env, int kind, K kernel, dim3 grid, dim3 block, uint32_t lds, hipStream_t st, Args... args) {
  hipEvent_t a = nullptr, b = nullptr;
  // Sampling whole STEPS (round 1) was biased once four parts overlapped: the sampled step's launches reach the GPU late
  // (six event creations on the launch path), overlap less and run 10 % faster than the rest - in the kernel trace
  // itself, scripts/kt_check.sh.  Events attached to the dispatch (hipExtLaunchKernelGGL) read 4-11 % long on these
  // 35-140 us kernels.  So: single launches are sampled, one in
  // (2 x profile + 1), which with 2 x parts launches per step walks through every part and both kernels; the events come
  // from a pool created when profiling is switched on, not from hipEventCreate on the launch path.
  const uint64_t every = env->profile == 1 ? 1u : 2u * static_cast<uint64_t>(env->profile) + 1u;  // odd: walks all parts
  const bool sample = env->profile > 0 && (env->prof_tick++ % every) == 0;
  if (sample && (a = env->prof_event()) && (b = env->prof_event())) {
    (void)hipEventRecord(a, st);
    hipLaunchKernelGGL(kernel, grid, block, lds, st, args...);
    (void)hipEventRecord(b, st);
    env->prof_events.push_back({a, b, kind});
  } else {
    hipLaunchKernelGGL(kernel, grid, block, lds, st, args...);
  }
}

// f(std::integral_constant<int, R>{}) for the env's pool registers per book R = 1, 2, 4, anything else 8: the one place a
// runtime R picks a kernel instantiation
template <typename F>
auto by_R(int R, F&& f) {
  switch (R) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 4: return f(std::integral_constant<int, 4>{});
    default: return f(std::integral_constant<int, 8>{});
  }
}

// A table kernel that gives every book one wave, `waves` of them per block, on the env's stream (g: its argument struct)
template <typename K, typename A>
void launch_wave_per_book(bk_env* env, K kernel, uint32_t waves, uint32_t n_books, const A& g) {
  hipLaunchKernelGGL(kernel, dim3((n_books + waves - 1) / waves), dim3(64 * waves), 0, env->stream, g);
}
template <typename K, typename A>
void launch_wave_per_book(bk_env* env, K kernel, uint32_t waves, const A& g) {
  launch_wave_per_book(env, kernel, waves, g.n_books, g);
}

// stamps::k_compact over every book, on the env's stream: every live stamp becomes its rank, H_SEQ the live count
int compact_stamps(bk_env* env) {
  const uint32_t B = env->cfg.n_books;
  const dim3 grid((B + bkd::stamps::COMPACT_WAVES - 1) / bkd::stamps::COMPACT_WAVES), block(64 * bkd::stamps::COMPACT_WAVES);
  by_R(env->R, [&](auto r) {
    hipLaunchKernelGGL(bkd::stamps::k_compact<decltype(r)::value>, grid, block, 0, env->stream, env->state.p, env->stride, B);
  });
  HIPCHK(hipGetLastError());
  env->stamp_room.compacted(static_cast<uint32_t>(env->R) * 64u);
  env->stamp_compactions += 1;
  return BK_OK;
}

// Before a launch in which one book can rest up to `rests` orders: queues the stamp compaction on the env's stream (for
// the multi-part pipelines that is in front of the fork) when the launch could take a book's H_SEQ past the limit.
int reserve_stamps(bk_env* env, uint64_t rests) {
  if (rests == 0) return BK_OK;
  if (env->stamp_room.needs_compaction(rests))
    if (int rc = compact_stamps(env)) return rc;
  env->stamp_room.spend(rests);
  return BK_OK;
}

int wave_args(bk_env* env, WaveArgs* wva);
template <int R>
int launch_events(bk_env* env, const DevArgs& a, uint64_t step_index, uint32_t max_queue) {
  env->prof_now = env->profile > 0;
  ProfScope ps(env, 3);
  uint32_t perm_bytes = ((max_queue + 63u) & ~63u) * 2u + 128u;  // u16 permutation of the longest queue
  if (perm_bytes < ev_lds_bytes(R)) perm_bytes = ev_lds_bytes(R);  // ... the wave-parallel shuffle's and the keyed form's lists (step_events.hpp)
  // a queue longer than the pool runs the keyed form chunk by chunk (round 6): its work area sits BEHIND the permutation
  if (max_queue > 64u * R) perm_bytes = std::max(perm_bytes, ((max_queue + 63u) & ~63u) * 2u + ev_keyed_lds_bytes(R));
  // the shuffle borrows the decode's jump tables and per-book lane-state cache (BOURSE_AMD_EV_SEQ_SHUFFLE=1: the draw-by-draw
  // loop, for measurements)
  // (both knobs are read ONCE, when the env is created - bk_env_create -: a getenv per launch raced with another thread's
  // setenv; a test sets them before it creates its env)
  const bool seq_shuffle = env->ev_seq_shuffle;
  // (its fixed cost - the cache record, a block of draws, a resolution over all 64 R positions - pays from a queue length that
  // grows with the pool: docs/EXPERIMENTS.md; BOURSE_AMD_EV_WAVE_SHUFFLE_MIN overrides, for measurements)
  const int min_env = env->ev_shuffle_min;
  const uint32_t shuffle_min = min_env >= 0 ? static_cast<uint32_t>(min_env) : (12u * R > 32u ? 12u * R : 32u);  // (measured: 256 slots 24 events -3 %, 48 +5 %; 512 slots 48 -7 %, 96 +3 %)
  // the lane-state cache (1 280 B per book) and the jump tables exist only once a step CAN take the wave-parallel shuffle: no
  // queue of this launch reaches its threshold -> wcache stays null and the kernel draws one by one (every env's
  // first bk_step allocated 84 MB at 65 536 books whether or not it ever shuffled that way)
  WaveArgs wva{};
  if (!seq_shuffle && max_queue >= shuffle_min && max_queue >= 2u)
    if (int rc = wave_args(env, &wva)) return rc;
  const bool chunks = max_queue > 64u * R;  // a queue longer than the pool: the instantiation whose keyed form runs chunk by chunk
  const dim3 grid(env->cfg.n_books), block(64);
  // 512-slot pools: the kernel WITH the keyed modifications only once this env has seen one (step_events.hpp k_step_events: the
  // clean launch is 13 % faster without that code).  Sticky; k_ingest's hint may lag by a step - that step's modifications then
  // run event by event, with the same results.
  if (env->mods_flag_host && *static_cast<volatile uint32_t*>(env->mods_flag_host)) env->ev_mods_seen.store(true, std::memory_order_relaxed);
  if constexpr (R == 8) {
    if (!chunks && !env->ev_mods_seen.load(std::memory_order_relaxed)) {
      if (env->M == 1)
        hipLaunchKernelGGL((k_step_events<R, false, false, false>), grid, block, perm_bytes, env->stream, a, wva, step_index, shuffle_min, perm_bytes);
      else
        hipLaunchKernelGGL((k_step_events<R, true, false, false>), grid, block, perm_bytes, env->stream, a, wva, step_index, shuffle_min, perm_bytes);
      HIPCHK(hipGetLastError());
      return BK_OK;
    }
  }
  if (env->M == 1 && !chunks)
    hipLaunchKernelGGL((k_step_events<R, false, false>), grid, block, perm_bytes, env->stream, a, wva, step_index, shuffle_min, perm_bytes);
  else if (env->M == 1)
    hipLaunchKernelGGL((k_step_events<R, false, true>), grid, block, perm_bytes, env->stream, a, wva, step_index, shuffle_min, perm_bytes);
  else if (!chunks)
    hipLaunchKernelGGL((k_step_events<R, true, false>), grid, block, perm_bytes, env->stream, a, wva, step_index, shuffle_min, perm_bytes);
  else
    hipLaunchKernelGGL((k_step_events<R, true, true>), grid, block, perm_bytes, env->stream, a, wva, step_index, shuffle_min, perm_bytes);
  HIPCHK(hipGetLastError());
  return BK_OK;
}

// jump tables (T^256, then T^(4 << b)) and the per-book lane-state cache of the wave-parallel decode, on first use
int wave_args(bk_env* env, WaveArgs* wva) {
  if (!env->jump_tabs.p) {
    std::vector<uint32_t> all;
    for (int t = 0; t < 7; ++t) {
      const std::vector<uint32_t> tab = xoroshiro_jump_table(t == 0 ? WV_BLOCK : static_cast<uint64_t>(WV_K) << (t - 1));
      all.insert(all.end(), tab.begin(), tab.end());
    }
    HIPCHK(env->jump_tabs.alloc(all.size() / 4));
    HIPCHK(env->wcache.alloc(static_cast<size_t>(env->cfg.n_books) * WC_STRIDE));
    // on the ENV's stream (a hipStreamNonBlocking stream is not ordered behind the null stream), and waited for: `all` is a local
    HIPCHK(hipMemcpyAsync(env->jump_tabs.p, all.data(), all.size() * 4, hipMemcpyHostToDevice, env->stream));
    HIPCHK(hipMemsetAsync(env->wcache.p, 0, static_cast<size_t>(env->cfg.n_books) * WC_STRIDE * 4, env->stream));
    HIPCHK(hipStreamSynchronize(env->stream));
  }
  wva->jt_block = env->jump_tabs.p;
  wva->jt_lane = env->jump_tabs.p + 512;
  wva->wcache = env->wcache.p;
  wva->lookahead = env->wave_lookahead;
  return BK_OK;
}

// The parts' streams: one process-wide set per device, every member PROBED to sit on a hardware queue of its own.
// HIP multiplexes streams onto GPU_MAX_HW_QUEUES (4) hardware queues - a new stream joins the least-referenced queue
// once four exist - and two parts that share a queue run back to back: the pipeline loses its overlap (C3 220 -> 124 M
// book-steps/s with a second env that had created its own streams first, 216 -> 119 M under torch.distributed.run, where
// RCCL's streams come first).  Which queue a stream got cannot be asked, but it can be measured: two 300 us spin kernels
// on two streams take 300 us on different queues and 600 us on one.  Eight candidates are created, a mutually
// concurrent subset of up to four is kept (greedy), the rest destroyed; every env on the device uses that set for all
// its parts (the caller's stream only forks and joins), envs sharing it just interleave.  CU-masked streams, which do
// get a queue each, were measured and are not an option (98 M).  ~10 ms once per process and device.
const std::vector<hipStream_t>& part_streams(int device) {
  static std::mutex mu;
  static std::map<int, std::vector<hipStream_t>> pool;
  std::lock_guard<std::mutex> lk(mu);
  auto it = pool.find(device);
  if (it != pool.end()) return it->second;
  std::vector<hipStream_t> cand, chosen;
  // BOURSE_AMD_PART_STREAMS=N (1..8): take N fresh streams WITHOUT probing.  For launchers that start many ranks at once
  // (one process per GPU: each rank would otherwise run its 8 x 300 us probe kernels at start-up, all at the same time,
  // next to RCCL's communicator set-up), and for boxes where the host-clock probe is unreliable.  Default: probe.
  if (const char* e = std::getenv("BOURSE_AMD_PART_STREAMS")) {
    const int want = std::atoi(e);
    if (want >= 1 && want <= 8) {
      for (int k = 0; k < want; ++k) {
        hipStream_t st = nullptr;
        if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) break;
        chosen.push_back(st);
      }
      (void)hipGetLastError();
      if (getenv("BOURSE_AMD_VERBOSE"))
        fprintf(stderr, "bourse_amd: device %d: %zu part streams taken unprobed (BOURSE_AMD_PART_STREAMS)\n", device, chosen.size());
      return pool.emplace(device, std::move(chosen)).first->second;
    }
  }
  for (int k = 0; k < 8; ++k) {
    hipStream_t st = nullptr;
    if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) break;
    hipLaunchKernelGGL(k_delay, dim3(1), dim3(64), 0, st, 1u);  // first use: the stream takes its hardware queue now
    cand.push_back(st);
  }
  (void)hipDeviceSynchronize();  // the probe times kernels: nothing of ours may still be running
  constexpr uint32_t SPIN_US = 300;
  auto concurrent = [&](hipStream_t x, hipStream_t y) {
    for (int attempt = 0; attempt < 2; ++attempt) {  // a slow pair is measured twice (someone else's work on the GPU)
      const auto t0 = std::chrono::steady_clock::now();
      hipLaunchKernelGGL(k_delay, dim3(1), dim3(64), 0, x, SPIN_US * 100u);
      hipLaunchKernelGGL(k_delay, dim3(1), dim3(64), 0, y, SPIN_US * 100u);
      (void)hipStreamSynchronize(x);
      (void)hipStreamSynchronize(y);
      const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
      if (us < 1.6 * SPIN_US) return true;
    }
    return false;
  };
  for (hipStream_t c : cand) {
    bool ok = chosen.size() < 4;
    for (size_t j = 0; ok && j < chosen.size(); ++j) ok = concurrent(c, chosen[j]);
    if (ok)
      chosen.push_back(c);
    else
      (void)hipStreamDestroy(c);
  }
  (void)hipGetLastError();
  if (getenv("BOURSE_AMD_VERBOSE"))
    fprintf(stderr, "bourse_amd: device %d: %zu of %zu candidate streams on hardware queues of their own\n", device,
            chosen.size(), cand.size());
  // fewer than four: the parts of a split launch share queues and run back to back (C3 220 -> 124 M book-steps/s when
  // every part sat on one queue).  Results are unaffected; say so once instead of being silently slow.
  if (chosen.size() < 4 && !cand.empty())
    fprintf(stderr, "bourse_amd: warning: device %d: only %zu of %zu candidate streams run concurrently (busy GPU or serialised "
            "kernels?): multi-part launches will overlap less; BOURSE_AMD_PART_STREAMS=4 skips the probe\n", device,
            chosen.size(), cand.size());
  return pool.emplace(device, std::move(chosen)).first->second;
}

// The per-kind set-up of a bk_run launch: dynamic-LDS attributes, the members' lists (allocated on first use, rebuilt from
// the owner tags when another pipeline changed the pools) and which of them still describe the pools, the wave decode's tables
template <int R>
int prepare_launch(bk_env* env, const Plan& pl, const DevArgs& a0, WaveArgs* wva) {
  switch (pl.kind) {
    case PL_FUSED_RANDOM: break;
    case PL_SPLIT_LANES:
    case PL_SPLIT_WAVE:
      if (!env->fsm_attr_set) {
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_agents_fsm<R>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   static_cast<int>(fsm_lds_bytes(R))));
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_agents_fsm<R, true>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(fsm_lds_bytes(R))));
        env->fsm_attr_set = true;
      }
      if (pl.kind == PL_SPLIT_WAVE) return wave_args(env, wva);
      break;
    case PL_FUSED_WAVE: return wave_args(env, wva);
    case PL_MIXED_LANES: {
      const size_t NB = env->cfg.n_books, cap = static_cast<size_t>(R) * 64, NU = NB / env->M;
      if (!env->ml_list.p) {
        HIPCHK(env->ml_list.alloc(MAX_MEMBERS * cap * NU));
        HIPCHK(env->ml_len.alloc(MAX_MEMBERS * NU));
        HIPCHK(env->ml_inl.alloc(2 * static_cast<size_t>(R) * NB));
        env->ml_valid = false;
      }
      if (!env->lds_attr_set) {  // allow > 64 KB of dynamic LDS (160 KB per workgroup on MI355X); the attribute is per device
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_agents_mixed_lanes<R, true>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(mixed_lanes_lds_bytes(R, true))));
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_agents_mixed_lanes<R, false>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(mixed_lanes_lds_bytes(R, false))));
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_agents_mixed_lanes<R, true, true>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(mixed_lanes_pb_lds_bytes(R, true))));
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_agents_mixed_lanes<R, false, true>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(mixed_lanes_pb_lds_bytes(R, false))));
        env->lds_attr_set = true;
      }
      if (!env->ml_valid) {
        hipLaunchKernelGGL(k_mixed_lists_rebuild<R>, dim3((env->cfg.n_books + 3) / 4), dim3(256), 0, env->stream, a0, env->margs(),
                           env->lists());
        HIPCHK(hipGetLastError());
        env->ml_valid = true;
      }
      env->wl_valid = false;  // (the wave-per-book lists no longer describe the pools)
      break;
    }
    case PL_MIXED_WPB:
    case PL_MIXED_FUSED:
      env->ml_valid = false;
      env->wl_valid = false;
      break;
    case PL_MIXED_WAVE:
      if (int rc = wave_args(env, wva)) return rc;
      if (!env->mw_attr_set) {  // > 64 KB of dynamic LDS at R = 8 (160 KB per workgroup on MI355X); per device
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_agents_mixed_wave<R>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   static_cast<int>(mixed_wave_lds_bytes(R))));
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_agents_mixed_wave<R, true>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(mixed_wave_lds_bytes(R))));
        env->mw_attr_set = true;
      }
      if (!env->wl_list.p) {
        HIPCHK(env->wl_list.alloc(static_cast<size_t>(env->cfg.n_books) * MAX_MEMBERS * R * 64));
        HIPCHK(env->wl_len.alloc(static_cast<size_t>(env->cfg.n_books) * MAX_MEMBERS));
        env->wl_valid = false;
      }
      if (!env->wl_valid) {  // another pipeline (or a restore / a fresh env) changed the pools: lists from the owner tags
        hipLaunchKernelGGL(k_wave_lists_rebuild<R>, dim3((env->cfg.n_books + 3) / 4), dim3(256), 0, env->stream, a0, env->margs(),
                           WaveLists{env->wl_list.p, env->wl_len.p, static_cast<uint32_t>(R) * 64u});
        HIPCHK(hipGetLastError());
        env->wl_valid = true;
      }
      env->ml_valid = false;
      break;
  }
  return BK_OK;
}

// The streams and fork / join events of a multi-part launch, on first use
int prepare_parts(bk_env* env) {
  if (env->ev_fork) return BK_OK;
  const std::vector<hipStream_t>& ps = part_streams(env->cfg.device);
  if (ps.empty()) return fail(BK_HIP_ERROR, "could not create the parts' streams");
  for (int i = 0; i < bk_env::MAX_PARTS; ++i) {
    env->part_stream[i] = ps[static_cast<size_t>(i) % ps.size()];  // more parts than queues: they share
    if (!env->ev_first[i]) HIPCHK(hipEventCreateWithFlags(&env->ev_first[i], hipEventDisableTiming));
    if (!env->ev_join[i]) HIPCHK(hipEventCreateWithFlags(&env->ev_join[i], hipEventDisableTiming));
  }
  // last: ev_fork doubles as "the parts' streams and events are set up" (a failure above leaves it unset, so the
  // next bk_run tries again instead of launching on null streams)
  HIPCHK(hipEventCreateWithFlags(&env->ev_fork, hipEventDisableTiming));
  return BK_OK;
}

// fused kinds: all n_steps in one launch on the env's stream
template <int R>
int launch_fused(bk_env* env, const Plan& pl, const DevArgs& a, const WaveArgs& wva, uint64_t first_step, uint32_t n_steps) {
  const uint32_t nb = env->cfg.n_books;
  env->prof_now = env->profile > 0;
  ProfScope ps(env, 0);
  if (pl.kind == PL_MIXED_FUSED && pl.members_per_book)
    hipLaunchKernelGGL((k_run_mixed<R, true>), dim3((nb + 3) / 4), dim3(256), 0, env->stream, a, env->margs(), first_step, n_steps,
                       static_cast<const MixedDesc*>(env->dmtable.p));
  else if (pl.kind == PL_MIXED_FUSED)
    hipLaunchKernelGGL(k_run_mixed<R>, dim3((nb + 3) / 4), dim3(256), 0, env->stream, a, env->margs(), first_step, n_steps);
  else if (pl.kind == PL_FUSED_WAVE && pl.agents_per_book)
    hipLaunchKernelGGL((k_run_wave<R, true>), dim3((nb + 7) / 8), dim3(512), 0, env->stream, a, wva, first_step, n_steps,
                       static_cast<const Group*>(env->dtable.p));
  else if (pl.kind == PL_FUSED_WAVE)
    hipLaunchKernelGGL(k_run_wave<R>, dim3((nb + 7) / 8), dim3(512), 0, env->stream, a, wva, first_step, n_steps);
  else
    hipLaunchKernelGGL(k_run_random<R>, dim3((nb + 3) / 4), dim3(256), 0, env->stream, a, first_step, n_steps);
  HIPCHK(hipGetLastError());
  return BK_OK;
}

// split kinds: per step and per part one agents launch (the RNG-serial phases) + one wave-per-book event launch
template <int R>
int launch_split(bk_env* env, const Plan& pl, const DevArgs& a0, const WaveArgs& wva, uint64_t first_step, uint32_t n_steps) {
  const MixedArgs ma = env->margs();
  const MixedLists ml = env->lists();
  const uint32_t M = env->M;
  const uint32_t B = env->cfg.n_books / M;  // units the parts are cut in: books, or markets of M books
  const Group* table = env->dtable.p;        // (pl.agents_per_book: the per-unit table)
  const MixedDesc* mtable = env->dmtable.p;  // (pl.members_per_book: the members' per-unit table)
  const int P = pl.parts;  // (small batches: one part on the caller's stream)
  if (P > 1) {
    if (int rc = prepare_parts(env)) return rc;
    HIPCHK(hipEventRecord(env->ev_fork, env->stream));
    for (int i = 0; i < P; ++i) HIPCHK(hipStreamWaitEvent(env->part_stream[i], env->ev_fork, 0));
  }
  for (uint32_t s = 0; s < n_steps; ++s) {
    env->prof_now = false;  // (launch_timed samples single launches)
    for (int i = 0; i < P; ++i) {
      DevArgs a = a0;
      a.book_begin = static_cast<uint32_t>(static_cast<uint64_t>(B) * i / P) & ~3u;
      a.book_end = (i + 1 == P) ? B : (static_cast<uint32_t>(static_cast<uint64_t>(B) * (i + 1) / P) & ~3u);
      a.hist_slot0 = a.hist_cap ? static_cast<uint32_t>((first_step + s) % a.hist_cap) : 0u;
      a.step_prio = pl.step_prio ? 1u : 0u;
      const uint32_t nb = a.book_end - a.book_begin;
      hipStream_t st = P > 1 ? env->part_stream[i] : env->stream;
      if (P > 1 && s == 0 && i > 0) {  // stagger the parts: by time, or by one agents kernel each
        if (pl.stagger_us > 0)
          hipLaunchKernelGGL(k_delay, dim3(1), dim3(64), 0, st, static_cast<uint32_t>(i) * pl.stagger_us * 100u);
        else
          HIPCHK(hipStreamWaitEvent(st, env->ev_first[i - 1], 0));
      }
      const uint64_t step_no = first_step + s;
      if (pl.agents == AG_MIXED_WAVE && pl.members_per_book)
        launch_timed(env, 1, &k_agents_mixed_wave<R, true>, dim3((nb + MW_WPB - 1) / MW_WPB), dim3(64 * MW_WPB),
                     static_cast<uint32_t>(mixed_wave_lds_bytes(R)), st, a, ma, wva,
                     WaveLists{env->wl_list.p, env->wl_len.p, static_cast<uint32_t>(R) * 64u}, mtable);
      else if (pl.agents == AG_MIXED_WAVE)
        launch_timed(env, 1, &k_agents_mixed_wave<R>, dim3((nb + MW_WPB - 1) / MW_WPB), dim3(64 * MW_WPB),
                     static_cast<uint32_t>(mixed_wave_lds_bytes(R)), st, a, ma, wva,
                     WaveLists{env->wl_list.p, env->wl_len.p, static_cast<uint32_t>(R) * 64u});
      else if (pl.agents == AG_MIXED_LANES_MKT && pl.members_per_book)
        launch_timed(env, 1, &k_agents_mixed_lanes<R, true, true>, dim3((nb + 63) / 64), dim3(64), mixed_lanes_pb_lds_bytes(R, true),
                     st, a, ma, ml, mtable);
      else if (pl.agents == AG_MIXED_LANES && pl.members_per_book)
        launch_timed(env, 1, &k_agents_mixed_lanes<R, false, true>, dim3((nb + 63) / 64), dim3(64),
                     mixed_lanes_pb_lds_bytes(R, false), st, a, ma, ml, mtable);
      else if (pl.agents == AG_MIXED_WPB && pl.members_per_book)
        launch_timed(env, 1, &k_agents_mixed<R, true>, dim3((nb + 3) / 4), dim3(256), 0u, st, a, ma, mtable);
      else if (pl.agents == AG_MIXED_LANES_MKT)
        launch_timed(env, 1, &k_agents_mixed_lanes<R, true>, dim3((nb + 63) / 64), dim3(64), mixed_lanes_lds_bytes(R, true), st, a,
                     ma, ml);
      else if (pl.agents == AG_MIXED_LANES)
        launch_timed(env, 1, &k_agents_mixed_lanes<R, false>, dim3((nb + 63) / 64), dim3(64), mixed_lanes_lds_bytes(R, false), st,
                     a, ma, ml);
      else if (pl.agents == AG_MIXED_WPB)
        launch_timed(env, 1, &k_agents_mixed<R>, dim3((nb + 3) / 4), dim3(256), 0u, st, a, ma);
      else if (pl.agents == AG_WAVE && pl.step_decode && s > 0)
        ;  // (the previous step's k_step_decode has decoded this step already)
      else if (pl.agents == AG_WAVE && pl.agents_per_book)
        launch_timed(env, 1, &k_agents_wave<R, true>, dim3((nb + 3) / 4), dim3(256), 0u, st, a, wva, table);
      else if (pl.agents == AG_WAVE)
        launch_timed(env, 1, &k_agents_wave<R>, dim3((nb + 3) / 4), dim3(256), 0u, st, a, wva);
      else if (pl.agents_per_book)
        launch_timed(env, 1, &k_agents_fsm<R, true>, dim3((nb + 63) / 64), dim3(64), fsm_lds_bytes(R), st, a, table);
      else
        launch_timed(env, 1, &k_agents_fsm<R>, dim3((nb + 63) / 64), dim3(64), fsm_lds_bytes(R), st, a);
      if (P > 1 && s == 0) HIPCHK(hipEventRecord(env->ev_first[i], st));
      const uint32_t write_last = (s + 1 == n_steps || a.hist_cap == 0 || pl.write_last) ? 1u : 0u;
      if (pl.step_log && pl.step_mkt)
        launch_timed(env, 2, &k_step_batch_log<R, true>, dim3(nb * M), dim3(64), 0u, st, a, step_no, write_last, env->dorders.p);
      else if (pl.step_log)
        launch_timed(env, 2, &k_step_batch_log<R, false>, dim3(nb), dim3(64), 0u, st, a, step_no, write_last, env->dorders.p);
      else if (pl.step_poolpend && pl.step_mkt)
        launch_timed(env, 2, &k_step_batch<R, true, true>, dim3(nb * M), dim3(64), 0u, st, a, step_no, write_last);
      else if (pl.step_poolpend)
        launch_timed(env, 2, &k_step_batch<R, false, true>, dim3(nb), dim3(64), 0u, st, a, step_no, write_last);
      else if (pl.step_mkt)
        launch_timed(env, 2, &k_step_batch<R, true>, dim3(nb * M), dim3(64), 0u, st, a, step_no, write_last);
      else if (pl.step_decode && s + 1 < n_steps)  // (the decode half belongs to the NEXT step; nothing in it reads the history slot)
        launch_timed(env, 2, &k_step_decode<R>, dim3((nb + 3) / 4), dim3(256), 0u, st, a, wva, step_no, write_last);
      else
        launch_timed(env, 2, &k_step_batch<R, false>, dim3(nb), dim3(64), 0u, st, a, step_no, write_last);
    }
  }
  HIPCHK(hipGetLastError());
  if (P > 1) {
    for (int i = 0; i < P; ++i) {
      HIPCHK(hipEventRecord(env->ev_join[i], env->part_stream[i]));
      HIPCHK(hipStreamWaitEvent(env->stream, env->ev_join[i], 0));
    }
  }
  return BK_OK;
}

// make `later` wait for the work queued on `earlier` so far
int order_after(hipStream_t later, hipStream_t earlier) {
  hipEvent_t ev = nullptr;
  HIPCHK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  hipError_t e = hipEventRecord(ev, earlier);
  if (e == hipSuccess) e = hipStreamWaitEvent(later, ev, 0);
  (void)hipEventDestroy(ev);  // released once the wait has been satisfied
  if (e != hipSuccess) return fail(BK_HIP_ERROR, std::string("stream ordering: ") + hipGetErrorString(e));
  return BK_OK;
}

// Host-driven orders on an env whose books are populated by on-device agents would restart the order ids at 0 (colliding
// with the agents' ids) and could take an agent's pool slot: one env runs ONE of the two flows.
int host_flow_ok(bk_env* env) {
  if (env->device_ingress)
    return fail(BK_INVALID_ARGUMENT, "this env takes its instructions from device memory (bk_device_ingress_enable): "
                                     "per-order host calls would collide with the ids assigned on the device");
  if (env->device_flow)
    return fail(BK_INVALID_ARGUMENT, "host-driven orders cannot be mixed with bk_run's on-device agents on the same env");
  return BK_OK;
}

int check_book(bk_env* env, uint32_t book) {
  if (!env) return fail(BK_INVALID_ARGUMENT, "null env");
  if (book >= env->cfg.n_books) return fail(BK_INVALID_ARGUMENT, "book index out of range");
  return BK_OK;
}

// books [first_book, first_book + n_books) of the readers: all of them exist (an empty range may start behind the last)
int book_range_ok(const bk_env* env, uint32_t first_book, uint32_t n_books) {
  if (first_book > env->cfg.n_books || n_books > env->cfg.n_books - first_book)
    return fail(BK_INVALID_ARGUMENT, "book range out of bounds");
  return BK_OK;
}

// The rows of a book range of an enabled per-book table -> host, behind the table's own check: range, null, device, a wait
// for the env's stream, then one copy per table (`book_bytes` each book; only the first `out` is required, a null or
// empty one behind it is left out).
struct BookRows {
  const void* table;
  size_t book_bytes;
  void* out;
};
int get_book_rows(bk_env* env, uint32_t first_book, uint32_t n_books, std::initializer_list<BookRows> tables) {
  if (int rc = book_range_ok(env, first_book, n_books)) return rc;
  if (n_books && !tables.begin()->out) return fail(BK_INVALID_ARGUMENT, "null argument");
  if (int rc = use_device(env)) return rc;
  HIPCHK(hipStreamSynchronize(env->stream));
  for (const BookRows& t : tables)
    if (n_books && t.out && t.book_bytes)
      HIPCHK(hipMemcpy(t.out, static_cast<const char*>(t.table) + first_book * t.book_bytes, n_books * t.book_bytes,
                       hipMemcpyDeviceToHost));
  return BK_OK;
}

int refresh_log(bk_env* env, uint32_t book) {
  BookHost& bh = env->books[book];
  if (bh.log_fresh) return BK_OK;
  const uint64_t n = std::min<uint64_t>(bh.n_uploaded, env->cfg.max_orders);
  bh.log_cache.resize(n);
  if (n) {
    HIPCHK(hipStreamSynchronize(env->stream));
    HIPCHK(hipMemcpy(bh.log_cache.data(), env->order_log.p + static_cast<size_t>(book) * env->cfg.max_orders,
                     n * sizeof(DevOrderLog), hipMemcpyDeviceToHost));
  }
  bh.log_fresh = true;
  return BK_OK;
}

// Device-resident ingress and logged on-device agents: the readers' view of one book's orders.  The immutable halves
// written by k_ingest / k_step_batch_log and the book's id counter are fetched into the same BookHost fields the
// host-driven path fills at bk_place_order, so every reader below works unchanged; valid until the next submit / step /
// bk_run (ingest_epoch).
int mirror_orders(bk_env* env, uint32_t book) {
  if (!env->device_ingress && !env->agent_log) return BK_OK;
  BookHost& bh = env->books[book];
  if (bh.mirror_epoch == env->ingest_epoch) return BK_OK;
  HIPCHK(hipSetDevice(env->cfg.device));
  HIPCHK(hipStreamSynchronize(env->stream));
  uint32_t count = 0;
  HIPCHK(hipMemcpy(&count, env->state.p + static_cast<size_t>(book) * env->stride + H_NEXT_ID, 4, hipMemcpyDeviceToHost));
  const uint64_t logged = std::min<uint64_t>(count, env->cfg.max_orders);
  std::vector<uint4> rows(logged * 2);
  if (logged)
    HIPCHK(hipMemcpy(rows.data(), env->dorders.p + static_cast<size_t>(book) * env->cfg.max_orders * 2, logged * 32,
                     hipMemcpyDeviceToHost));
  bh.orders.assign(count, HostOrder{0, 0, 0, 0, 0});
  for (uint64_t id = 0; id < logged; ++id) {
    const uint4 a = rows[2 * id], b = rows[2 * id + 1];
    bh.orders[id] = HostOrder{static_cast<uint8_t>(a.w & 1u), a.x, a.z, a.y, (static_cast<uint64_t>(b.y) << 32) | b.x};
  }
  bh.n_uploaded = count;  // every order has had a log entry since k_ingest / k_step_batch_log created it
  bh.log_fresh = false;
  bh.mirror_epoch = env->ingest_epoch;
  return BK_OK;
}

int prof_collect(bk_env* env) {
  HIPCHK(hipStreamSynchronize(env->stream));
  for (auto& pr : env->prof_events) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, pr.a, pr.b) == hipSuccess) {
      env->prof_ms[pr.kind] += std::max(0.0, static_cast<double>(ms) - env->prof_bracket_ms);
      env->prof_launches[pr.kind] += 1;
    }
    env->prof_pool.push_back(pr.a);
    env->prof_pool.push_back(pr.b);
  }
  env->prof_events.clear();
  return BK_OK;
}

void fill_order(const bk_env* env, const BookHost& bh, uint64_t id, bk_order* o) {
  const HostOrder& h = bh.orders[id];
  std::memset(o, 0, sizeof(*o));
  o->side_is_bid = h.bid;
  o->start_vol = h.start_vol;
  o->trader_id = h.trader;
  o->order_id = id;
  if (id < bh.n_uploaded && id < bh.log_cache.size()) {
    const DevOrderLog& d = bh.log_cache[id];
    o->status = static_cast<uint8_t>(d.status);
    o->vol = d.vol;
    o->price = d.price;
    o->arr_time = (static_cast<uint64_t>(d.arr_hi) << 32) | d.arr_lo;
    o->end_time = (static_cast<uint64_t>(d.end_hi) << 32) | d.end_lo;
  } else {  // created, New event still queued (or beyond the log capacity)
    o->status = 0;
    o->vol = h.start_vol;
    o->price = h.price;
    o->arr_time = h.create_time;
    o->end_time = ~0ull;
  }
  (void)env;
}

}  // namespace

extern "C" {

const char* bk_last_error(void) { return g_err.c_str(); }

int bk_hip_versions(int* built, int* runtime) {
  int v = 0;
  if (hipRuntimeGetVersion(&v) != hipSuccess) v = 0;
  if (built) *built = HIP_VERSION;
  if (runtime) *runtime = v;
  return BK_OK;
}

int bk_device_count(int* out) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) n = 0;
  if (out) *out = n;
  return BK_OK;
}

int bk_env_create(const bk_config* cfg, bk_env** out) {
  if (!cfg || !out) return fail(BK_INVALID_ARGUMENT, "null argument");
  *out = nullptr;
  if (cfg->n_books == 0) return fail(BK_INVALID_ARGUMENT, "n_books must be >= 1");
  if (cfg->tick_size == 0) return fail(BK_INVALID_ARGUMENT, "tick_size must be > 0");  // orderbook.rs:159
  if (cfg->levels == 0 || cfg->levels > 64) return fail(BK_INVALID_ARGUMENT, "levels must be in 1..64");
  const uint32_t M = cfg->assets ? cfg->assets : 1u;
  if (M > MAX_ASSETS || cfg->n_books % M != 0)
    return fail(BK_INVALID_ARGUMENT, "assets must be <= 8 and divide n_books");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(BK_NO_DEVICE, "no HIP device available: bourse_amd has no CPU execution path");
  if (cfg->device < 0 || cfg->device >= ndev) return fail(BK_INVALID_ARGUMENT, "device ordinal out of range");

  std::unique_ptr<bk_env> env(new bk_env());
  env->cfg = *cfg;
  env->M = M;
  for (uint32_t i = 0; i < MAX_ASSETS; ++i) env->asset_tick[i] = cfg->tick_size;
  uint32_t pool = cfg->max_live_orders ? cfg->max_live_orders : 128;
  int R = 1;
  while (R * 64u < pool) R *= 2;
  if (R > 8) return fail(BK_INVALID_ARGUMENT, "max_live_orders must be <= 512");
  env->R = R;
  env->cfg.max_live_orders = R * 64;
  env->W = 5 + 4 * cfg->levels;
  env->stride = HDR_DW + R * POOL_FIELDS * 64;
  env->trading = cfg->trading ? 1 : 0;
  HIPCHK(hipSetDevice(cfg->device));

  const size_t B = cfg->n_books;
  HIPCHK(env->state.alloc(B * env->stride));
  HIPCHK(env->l2_last.alloc(B * env->W));
  HIPCHK(env->hist.alloc(static_cast<size_t>(cfg->history_capacity) * B * env->W));
  HIPCHK(env->trades.alloc(B * cfg->trade_capacity));
  HIPCHK(env->order_log.alloc(B * cfg->max_orders));
  HIPCHK(env->stats.alloc(2));  // [0] the record, [1] its reset template
  {
    DevStats init{};
    init.min_bid = 0xFFFFFFFFu;
    init.min_ask = 0xFFFFFFFFu;
    HIPCHK(hipMemcpy(env->stats.p + 1, &init, sizeof(init), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(env->stats.p, &init, sizeof(init), hipMemcpyHostToDevice));
  }
  env->batch_stride = 64 + 160 * R;
  HIPCHK(env->batch.alloc(B * env->batch_stride));
  HIPCHK(hipMemset(env->batch.p, 0, B * env->batch_stride * sizeof(uint32_t)));
  if (const char* pm = std::getenv("BOURSE_AMD_PIPELINE")) {
    if (std::strcmp(pm, "fused") == 0) env->pipeline = 1;
    if (std::strcmp(pm, "split") == 0) env->pipeline = 2;
    if (std::strcmp(pm, "wave_split") == 0) env->pipeline = 4;
    if (std::strcmp(pm, "wave") == 0) env->pipeline = 5;
  }
  if (const char* np = std::getenv("BOURSE_AMD_SPLIT_PARTS")) {
    const int v = std::atoi(np);
    if (v >= 1 && v <= bk_env::MAX_PARTS) env->n_parts = v;
  }
  if (const char* sq = std::getenv("BOURSE_AMD_EV_SEQ_SHUFFLE")) env->ev_seq_shuffle = *sq == '1';
  if (const char* sm = std::getenv("BOURSE_AMD_EV_WAVE_SHUFFLE_MIN")) env->ev_shuffle_min = std::atoi(sm);
  if (const char* su = std::getenv("BOURSE_AMD_STAGGER_US")) env->stagger_us = static_cast<uint32_t>(std::max(0, std::atoi(su)));
  if (const char* sd = std::getenv("BOURSE_AMD_STEP_DECODE")) env->step_decode = std::atoi(sd) != 0;
  if (const char* fl = std::getenv("BOURSE_AMD_FSM_LOOP")) env->fsm_compiled_loop = std::strcmp(fl, "compiled") == 0;
  if (const char* mp = std::getenv("BOURSE_AMD_MIN_PART")) {
    const int v = std::atoi(mp);
    if (v >= 64) env->min_part = static_cast<uint32_t>(v);
  }
  // diagnostic knobs of the stamps: the value every fresh book's H_SEQ starts at, and the room a compaction leaves (so
  // that tests reach the wrap, and the compaction, within a few steps)
  uint32_t seq_start = 0;
  if (const char* ss = std::getenv("BOURSE_AMD_SEQ_START")) seq_start = static_cast<uint32_t>(std::strtoull(ss, nullptr, 0));
  if (const char* sr = std::getenv("BOURSE_AMD_STAMP_ROOM")) {
    const unsigned long long v = std::strtoull(sr, nullptr, 0);
    if (v >= 1) env->stamp_room.limit = std::min<uint64_t>(env->stamp_room.limit, static_cast<uint64_t>(R) * 64u + v);
  }
  env->stamp_room.bound = seq_start;
  HIPCHK(env->ev_off.alloc(B + 1));
  HIPCHK(hipMemset(env->ev_off.p, 0, (B + 1) * sizeof(uint32_t)));

  // initial device state: empty books, per-book RNG streams, Env::new's empty-book snapshot
  std::vector<uint32_t> st(B * env->stride, 0u), l2(B * env->W, 0u);
  for (size_t b = 0; b < B; ++b) {
    uint32_t* h = st.data() + b * env->stride;
    uint64_t s0, s1;
    seed_from_u64(cfg->seed + cfg->book_offset + b / M, s0, s1);  // one stream per market (runner.rs:115)
    h[H_T_LO] = static_cast<uint32_t>(cfg->start_time);
    h[H_T_HI] = static_cast<uint32_t>(cfg->start_time >> 32);
    h[H_S0_LO] = static_cast<uint32_t>(s0);
    h[H_S0_HI] = static_cast<uint32_t>(s0 >> 32);
    h[H_S1_LO] = static_cast<uint32_t>(s1);
    h[H_S1_HI] = static_cast<uint32_t>(s1 >> 32);
    h[H_TRADING] = env->trading;
    h[H_SEQ] = seq_start;
    uint32_t* l = l2.data() + b * env->W;
    l[1] = 0u;           // bid touch of an empty side (side.rs:194-196)
    l[2] = 0xFFFFFFFFu;  // ask touch of an empty side (side.rs:99-104)
  }
  HIPCHK(hipMemcpy(env->state.p, st.data(), st.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(env->l2_last.p, l2.data(), l2.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
  env->books.resize(B);
  *out = env.release();
  return BK_OK;
}

void bk_env_destroy(bk_env* env) {
  if (!env) return;
  (void)hipSetDevice(env->cfg.device);
  (void)hipStreamSynchronize(env->stream);
  for (auto& pr : env->prof_events) {
    (void)hipEventDestroy(pr.a);
    (void)hipEventDestroy(pr.b);
  }
  for (hipEvent_t e : env->prof_pool) (void)hipEventDestroy(e);
  if (env->ev_stage) (void)hipHostFree(env->ev_stage);
  if (env->off_stage) (void)hipHostFree(env->off_stage);
  if (env->hi.in) (void)hipStreamSynchronize(env->hi.in);
  if (env->hi.out) (void)hipStreamSynchronize(env->hi.out);
  if (env->mods_flag_host) (void)hipHostFree(env->mods_flag_host);
  for (auto& r : env->hi.retired) (void)hipHostFree(r.pin);
  env->hi.retired.clear();
  for (int i = 0; i < bk_env::HostIngress::SLOTS; ++i) {
    if (env->hi.pin[i]) (void)hipHostFree(env->hi.pin[i]);
    if (env->hi.dev[i]) (void)hipFree(env->hi.dev[i]);
    for (hipEvent_t e : {env->hi.e_h2d[i], env->hi.e_ing[i], env->hi.e_done[i]})
      if (e) (void)hipEventDestroy(e);
  }
  if (env->hi.in) (void)hipStreamDestroy(env->hi.in);
  if (env->hi.out) (void)hipStreamDestroy(env->hi.out);
  if (env->ev_fork) (void)hipEventDestroy(env->ev_fork);
  for (int i = 0; i < bk_env::MAX_PARTS; ++i) {
    if (env->part_stream[i]) (void)hipStreamSynchronize(env->part_stream[i]);  // shared (part_streams): not destroyed
    if (env->ev_first[i]) (void)hipEventDestroy(env->ev_first[i]);
    if (env->ev_join[i]) (void)hipEventDestroy(env->ev_join[i]);
  }
  delete env;
}

int bk_env_set_stream(bk_env* env, void* hip_stream) {
  if (!env) return fail(BK_INVALID_ARGUMENT, "null env");
  env->stream = static_cast<hipStream_t>(hip_stream);
  return BK_OK;
}

int bk_env_sync(bk_env* env) {
  if (!env) return fail(BK_INVALID_ARGUMENT, "null env");
  if (int rc = use_device(env)) return rc;
  HIPCHK(hipStreamSynchronize(env->stream));
  return BK_OK;
}

// ------------------------------------------------------------------ host-driven order flow
int bk_place_order(bk_env* env, uint32_t book, int bid, uint32_t vol, uint32_t trader_id, int has_price,
                   uint32_t price, uint64_t* out_order_id) {
  if (int rc = check_book(env, book)) return rc;
  if (int rc = host_flow_ok(env)) return rc;
  const uint32_t asset = book % env->M, tick = env->asset_tick[asset];
  if (has_price && price % tick != 0)  // create_order's tick check, orderbook.rs:367-382
    return fail(BK_PRICE_NOT_TICK_MULTIPLE,
                "Price " + std::to_string(price) + " was not a multiple of tick-size " + std::to_string(tick));
  BookHost& bh = env->books[book];
  BookHost& qh = env->books[book - asset];  // the queue is the market's (market_env.rs:58)
  const uint64_t id = bh.orders.size();  // current_order_id, orderbook.rs:327-329
  if (id >= 0xFFFFFFFFull) return fail(BK_CAPACITY, "order id space exhausted");
  const uint32_t p = has_price ? price : (bid ? 0xFFFFFFFFu : 0u);  // market sentinels, types.rs:168,221
  const uint64_t now = env->cfg.start_time + env->steps_done * env->cfg.step_size + bh.time_offset;
  bh.orders.push_back(HostOrder{static_cast<uint8_t>(bid ? 1 : 0), vol, p, trader_id, now});
  qh.queue.push_back(HostEvent{0u | (bid ? 1u << 8 : 0u) | (asset << 16), static_cast<uint32_t>(id), p, vol});
  if (out_order_id) *out_order_id = id;
  return BK_OK;
}

int bk_cancel_order(bk_env* env, uint32_t book, uint64_t order_id) {
  if (int rc = check_book(env, book)) return rc;
  if (int rc = host_flow_ok(env)) return rc;
  // an id that was never created panics only when the event is PROCESSED (orderbook.rs:642): checked in bk_step
  const uint32_t asset = book % env->M;
  env->books[book - asset].queue.push_back(
      HostEvent{1u | (asset << 16), static_cast<uint32_t>(std::min<uint64_t>(order_id, 0xFFFFFFFFull)), 0u, 0u});
  return BK_OK;
}

int bk_modify_order(bk_env* env, uint32_t book, uint64_t order_id, int has_price, uint32_t new_price, int has_vol,
                    uint32_t new_vol) {
  if (int rc = check_book(env, book)) return rc;
  if (int rc = host_flow_ok(env)) return rc;
  const uint32_t asset = book % env->M;
  const uint32_t w = 2u | (has_price ? 1u << 9 : 0u) | (has_vol ? 1u << 10 : 0u) | (asset << 16);
  env->ev_mods_seen.store(true, std::memory_order_relaxed);  // (launch_events: the k_step_events form with the keyed modifications)
  env->books[book - asset].queue.push_back(
      HostEvent{w, static_cast<uint32_t>(std::min<uint64_t>(order_id, 0xFFFFFFFFull)), new_price, new_vol});
  return BK_OK;
}

int bk_submit_instructions(bk_env* env, uint32_t book, size_t n, const uint32_t* action, const uint8_t* side,
                           const uint32_t* vol, const uint32_t* trader_id, const uint32_t* price,
                           const uint64_t* order_id, uint64_t* out_ids, size_t* n_done) {
  if (int rc = check_book(env, book)) return rc;
  if (n_done) *n_done = 0;
  if (n && (!action || !side || !vol || !trader_id || !price || !order_id))
    return fail(BK_INVALID_ARGUMENT, "null instruction array");
  for (size_t i = 0; i < n; ++i) {
    uint64_t id = ~0ull;  // usize::MAX for non-new instructions (step_sim_numpy.rs:255-268)
    if (action[i] == 1) {
      // (bit 0 is the side on EVERY entry - k_ingest reads `side & 1`; bits 1 / 2 belong to BK_ACTION_MODIFY: ADVICE r5)
      int rc = bk_place_order(env, book, (side[i] & 1) != 0, vol[i], trader_id[i], 1, price[i], &id);
      if (rc != BK_OK) return rc;  // earlier elements stay created and queued (:167-177)
    } else if (action[i] == 2) {
      int rc = bk_cancel_order(env, book, order_id[i]);
      if (rc != BK_OK) return rc;
    } else if (action[i] == BK_ACTION_MODIFY) {  // the extension both entries share (k_ingest); anything else: no-op (:266)
      int rc = bk_modify_order(env, book, order_id[i], (side[i] & 2) != 0, price[i], (side[i] & 4) != 0, vol[i]);
      if (rc != BK_OK) return rc;
    }
    if (out_ids) out_ids[i] = id;
    if (n_done) *n_done = i + 1;
  }
  return BK_OK;
}

// The same for EVERY book in one call (SURVEY §8b "batched SoA ops"): the instructions of book b are elements
// [book_offsets[b], book_offsets[b + 1]) of the arrays.  Semantics per book as bk_submit_instructions; stops at the first
// bad price of any book (*n_done = index of the offending element, earlier elements stay queued).
int bk_submit_instructions_csr(bk_env* env, const uint64_t* book_offsets, const uint32_t* action, const uint8_t* side,
                               const uint32_t* vol, const uint32_t* trader_id, const uint32_t* price,
                               const uint64_t* order_id, uint64_t* out_ids, size_t* n_done) {
  if (!env || !book_offsets) return fail(BK_INVALID_ARGUMENT, "null argument");
  const uint32_t B = env->cfg.n_books, M = env->M, NM = B / M;
  if (n_done) *n_done = 0;
  if (book_offsets[B] > book_offsets[0] && (!action || !side || !vol || !trader_id || !price || !order_id))
    return fail(BK_INVALID_ARGUMENT, "null instruction array");
  for (uint32_t b = 0; b < B; ++b)
    if (book_offsets[b + 1] < book_offsets[b]) return fail(BK_INVALID_ARGUMENT, "book_offsets must be non-decreasing");
  // The host half of Env (tick check, id assignment, queueing) is independent per book (per market: the queue is the
  // market's): large batches are spread over host threads, each owning a contiguous range of markets.
  auto work = [&](uint32_t m_lo, uint32_t m_hi, int* rc_out, size_t* done_out, std::string* err) {
    *rc_out = BK_OK;
    for (uint32_t b = m_lo * M; b < m_hi * M; ++b) {
      const uint64_t lo = book_offsets[b], hi = book_offsets[b + 1];
      if (hi == lo) continue;
      size_t done = 0;
      const int rc = bk_submit_instructions(env, b, hi - lo, action + lo, side + lo, vol + lo, trader_id + lo, price + lo,
                                            order_id + lo, out_ids ? out_ids + lo : nullptr, &done);
      if (rc != BK_OK) {
        *rc_out = rc;
        *done_out = lo + done;
        *err = bk_last_error();  // thread-local in the worker
        return;
      }
    }
    *done_out = book_offsets[static_cast<size_t>(m_hi) * M];
  };
  const uint64_t total = book_offsets[B];
  unsigned nt = 1;
  if (total >= 65536 && NM >= 64) nt = std::min<unsigned>(env->host_pool().threads(), NM);
  std::vector<int> rcs(nt, BK_OK);
  std::vector<size_t> dones(nt, 0);
  std::vector<std::string> errs(nt);
  auto task = [&](unsigned t) {
    work(static_cast<uint32_t>(static_cast<uint64_t>(NM) * t / nt),
         static_cast<uint32_t>(static_cast<uint64_t>(NM) * (t + 1) / nt), &rcs[t], &dones[t], &errs[t]);
  };
  if (nt == 1)
    task(0);
  else if (!env->host_pool().run(nt, task))
    return fail(BK_CAPACITY, "host pool: too many tasks");
  for (unsigned t = 0; t < nt; ++t) {  // the first failing range in book order decides (books after it may be queued too)
    if (rcs[t] != BK_OK) {
      if (n_done) *n_done = dones[t];
      return fail(rcs[t], errs[t]);
    }
  }
  if (n_done) *n_done = total;
  return BK_OK;
}

int bk_enable_trading(bk_env* env, int enabled) {
  if (!env) return fail(BK_INVALID_ARGUMENT, "null env");
  if (int rc = use_device(env)) return rc;
  env->trading = enabled ? 1 : 0;
  const uint32_t B = env->cfg.n_books;
  hipLaunchKernelGGL(k_book_service, dim3((B + 255) / 256), dim3(256), 0, env->stream, env->state.p, env->stride, B, 1,
                     env->trading);
  HIPCHK(hipGetLastError());
  return BK_OK;
}

int bk_step(bk_env* env) {
  if (!env) return fail(BK_INVALID_ARGUMENT, "null env");
  if (env->device_ingress) {  // the queues are on the device already: launch, then wait as this entry always has
    if (int rc = bk_step_async(env)) return rc;
    HIPCHK(hipStreamSynchronize(env->stream));
    return BK_OK;
  }
  if (int rc = host_flow_ok(env)) return rc;
  if (int rc = use_device(env)) return rc;
  const size_t B = env->cfg.n_books, M = env->M, NM = B / M;
  // CSR offsets of the queues (one row per market; a market of one book when assets == 1)
  std::vector<uint32_t> off(NM + 1, 0u);
  size_t total = 0;
  uint32_t max_queue = 0;
  for (size_t m = 0; m < NM; ++m) {
    const size_t q = env->books[m * M].queue.size();
    if (q > EV_LDS_CAP) return fail(BK_CAPACITY, "more than 8192 events queued for one book (market) in one step");
    off[m] = static_cast<uint32_t>(total);
    total += q;
    max_queue = std::max(max_queue, static_cast<uint32_t>(q));
  }
  off[NM] = static_cast<uint32_t>(total);
  HIPCHK(hipStreamSynchronize(env->stream));  // previous step may still read the event buffers
  if (total > env->ev_capacity || !env->off_stage) {
    const size_t cap = std::max<size_t>(total * 2, 1024);
    HIPCHK(env->ev.alloc(cap));
    if (env->ev_stage) HIPCHK(hipHostFree(env->ev_stage));
    env->ev_stage = nullptr;
    HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&env->ev_stage), cap * sizeof(HostEvent), hipHostMallocDefault));
    if (!env->off_stage)
      HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&env->off_stage), (B + 1) * sizeof(uint32_t), hipHostMallocDefault));
    env->ev_capacity = cap;
  }
  // validate (an id that was never created: orderbook.rs:642) and flatten straight into pinned memory: one 16-byte
  // record per event, uploaded at link speed.  Markets are independent: large batches are spread over the host threads.
  unsigned nt = 1;
  if (total >= 32768 && NM >= 64) nt = std::min<unsigned>(env->host_pool().threads(), static_cast<unsigned>(NM));
  std::vector<size_t> bad_market(nt, NM);
  std::vector<uint32_t> bad_id(nt, 0u);
  auto task = [&](unsigned t) {
    const size_t m_lo = NM * t / nt, m_hi = NM * (t + 1) / nt;
    for (size_t m = m_lo; m < m_hi; ++m) {
      const std::vector<HostEvent>& q = env->books[m * M].queue;
      for (const HostEvent& e : q)
        if ((e.word & 0xFFu) != 0 && e.id >= env->books[m * M + ((e.word >> 16) & 0xFFu)].orders.size()) {
          bad_market[t] = m;
          bad_id[t] = e.id;
          return;
        }
      if (!q.empty()) std::memcpy(env->ev_stage + off[m], q.data(), q.size() * sizeof(HostEvent));
    }
  };
  if (nt == 1)
    task(0);
  else if (!env->host_pool().run(nt, task))
    return fail(BK_CAPACITY, "host pool: too many tasks");
  for (unsigned t = 0; t < nt; ++t)  // the first offender in market order; nothing has been uploaded or cleared
    if (bad_market[t] != NM) return fail(BK_UNKNOWN_ORDER_ID, "No order with id " + std::to_string(bad_id[t]) + " exists");
  std::memcpy(env->off_stage, off.data(), (NM + 1) * sizeof(uint32_t));
  HIPCHK(hipMemcpyAsync(env->ev_off.p, env->off_stage, (NM + 1) * 4, hipMemcpyHostToDevice, env->stream));
  if (total)
    HIPCHK(hipMemcpyAsync(env->ev.p, env->ev_stage, total * sizeof(HostEvent), hipMemcpyHostToDevice, env->stream));
  if (int rc = reserve_stamps(env, max_queue)) return rc;  // (a New or a re-keying modification takes one stamp)
  const DevArgs a = env->args();
  const int rc = by_R(env->R, [&](auto r) { return launch_events<decltype(r)::value>(env, a, env->steps_done, max_queue); });
  if (rc != BK_OK) return rc;
  env->steps_done += 1;
  for (size_t b = 0; b < B; ++b) {
    BookHost& bh = env->books[b];
    bh.queue.clear();
    bh.n_uploaded = bh.orders.size();
    bh.log_fresh = false;
  }
  HIPCHK(hipStreamSynchronize(env->stream));
  return BK_OK;
}

// ------------------------------------------------------------------ device-resident instruction ingress
// (rust/src/step_sim_numpy.rs:233-275 submit_instructions + env.rs:166-219, for every book, with no host in the loop)
int bk_device_ingress_enable(bk_env* env, uint32_t queue_capacity) {
  if (!env) return fail(BK_INVALID_ARGUMENT, "null env");
  if (env->device_ingress) {
    if (queue_capacity != env->qcap) return fail(BK_INVALID_ARGUMENT, "device ingress is already enabled with another queue capacity");
    return BK_OK;
  }
  if (queue_capacity == 0 || queue_capacity > EV_LDS_CAP)
    return fail(BK_INVALID_ARGUMENT, "queue_capacity must be in 1..8192 events per book (market) and step");
  if (env->device_flow || env->n_mixed || !env->groups.empty() || env->agent_log)
    return fail(BK_INVALID_ARGUMENT, "an env runs ONE order flow: on-device agents (bk_run) or submitted instructions");
  for (const BookHost& bh : env->books)
    if (!bh.queue.empty() || !bh.orders.empty())
      return fail(BK_INVALID_ARGUMENT, "enable the device ingress before any order is placed through the host entries");
  if (int rc = use_device(env)) return rc;
  const size_t NM = env->cfg.n_books / env->M;
  HIPCHK(env->dq.alloc(NM * queue_capacity));
  HIPCHK(env->dqlen.alloc(NM));
  HIPCHK(hipMemsetAsync(env->dqlen.p, 0, NM * 4, env->stream));
  HIPCHK(env->dorders.alloc(static_cast<size_t>(env->cfg.n_books) * env->cfg.max_orders * 2));
  // k_ingest's "a modification was submitted" hint: one word of mapped host memory (launch_events reads it without a copy)
  if (!env->mods_flag_host) {
    void* hp = nullptr;
    if (hipHostMalloc(&hp, 64, hipHostMallocMapped) == hipSuccess) {
      *static_cast<uint32_t*>(hp) = 0u;
      void* dp = nullptr;
      if (hipHostGetDevicePointer(&dp, hp, 0) == hipSuccess) {
        env->mods_flag_host = static_cast<uint32_t*>(hp);
        env->mods_flag_dev = static_cast<uint32_t*>(dp);
      } else {
        (void)hipHostFree(hp);
      }
    }
    (void)hipGetLastError();
    if (!env->mods_flag_host) env->ev_mods_seen.store(true);  // (no hint available: always the full kernel)
  }
  env->qcap = queue_capacity;
  env->device_ingress = true;
  return BK_OK;
}

int bk_submit_instructions_device(bk_env* env, const uint64_t* book_offsets_dev, const uint32_t* action_dev, const uint8_t* side_dev,
                                  const uint32_t* vol_dev, const uint32_t* trader_dev, const uint32_t* price_dev,
                                  const uint64_t* order_id_dev, uint64_t* out_ids_dev, uint32_t* status_dev) {
  if (!env) return fail(BK_INVALID_ARGUMENT, "null env");
  if (!env->device_ingress) return fail(BK_INVALID_ARGUMENT, "call bk_device_ingress_enable first");
  if (!book_offsets_dev || !action_dev || !side_dev || !vol_dev || !trader_dev || !price_dev || !order_id_dev)
    return fail(BK_INVALID_ARGUMENT, "null instruction array");
  if (int rc = use_device(env)) return rc;
  IngestArgs g{};
  g.off = reinterpret_cast<const unsigned long long*>(book_offsets_dev);
  g.action = action_dev;
  g.side = side_dev;
  g.vol = vol_dev;
  g.trader = trader_dev;
  g.price = price_dev;
  g.order_id = reinterpret_cast<const unsigned long long*>(order_id_dev);
  g.out_ids = reinterpret_cast<unsigned long long*>(out_ids_dev);
  g.status = status_dev;
  g.q = env->dq.p;
  g.qlen = env->dqlen.p;
  g.qcap = env->qcap;
  g.dorders = env->dorders.p;
  g.mods_flag = env->mods_flag_dev;
  const DevArgs a = env->args();
  hipLaunchKernelGGL(k_ingest, dim3(env->cfg.n_books / env->M), dim3(64), 0, env->stream, a, g);
  HIPCHK(hipGetLastError());
  env->ingest_epoch += 1;
  return BK_OK;
}

// ==================================================================================
// HOST arrays through the device ingress (round 5; VERDICT r4 "missing" #2).  A `BaseNumpyAgent`-style caller
// (src/bourse/step_sim/agents/base_agent.py:67-116, runner.py:103-112) hands over HOST numpy arrays; rounds 1-4 walked them
// through the host half of Env (tick check, ids and queues on CPU threads, 16 B per event uploaded: 3.2 M book-steps/s at
// 8 192 books x 48 instructions).  Here the SAME six arrays (rust/src/step_sim_numpy.rs:233-275) go pinned staging ->
// one async upload per array on a copy stream -> k_ingest on the env's stream -> ids / per-book status back on a second copy
// stream.  Two slots: the upload of ticket t + 1 runs under the step kernel of ticket t; a ticket's results stay
// readable until two more submits.  Same per-book semantics as every other submit entry (k_ingest: dense ids in element
// order, a book's batch stops at its first bad price with the earlier elements applied, other books unaffected).
// ==================================================================================
namespace {
int hi_ensure(bk_env* env, size_t n_elem) {
  bk_env::HostIngress& h = env->hi;
  if (!h.in) {
    HIPCHK(hipStreamCreateWithFlags(&h.in, hipStreamNonBlocking));
    HIPCHK(hipStreamCreateWithFlags(&h.out, hipStreamNonBlocking));
    for (int i = 0; i < bk_env::HostIngress::SLOTS; ++i) {
      HIPCHK(hipEventCreateWithFlags(&h.e_h2d[i], hipEventDisableTiming));
      HIPCHK(hipEventCreateWithFlags(&h.e_ing[i], hipEventDisableTiming));
      HIPCHK(hipEventCreateWithFlags(&h.e_done[i], hipEventDisableTiming));
    }
  }
  if (n_elem <= h.cap && h.pin[0] && h.pin[1]) return BK_OK;
  // grow: everything in flight must have landed first; the results the slots hold (ids + status of the last two tickets - a
  // caller that fetches one submit late has not read them yet) move into the new staging
  HIPCHK(hipStreamSynchronize(h.in));
  HIPCHK(hipStreamSynchronize(env->stream));
  HIPCHK(hipStreamSynchronize(h.out));
  const size_t cap = std::max<size_t>((n_elem + n_elem / 4 + 1023) & ~size_t(1023), 1024);
  // BOTH new slots are allocated before anything of the old staging is given up: a failed allocation leaves the env as it was
  bk_env::HostIngress lay = h;
  lay.layout(env->cfg.n_books, cap);
  char *npin[bk_env::HostIngress::SLOTS] = {}, *ndev[bk_env::HostIngress::SLOTS] = {};
  for (int i = 0; i < bk_env::HostIngress::SLOTS; ++i) {
    if (hipHostMalloc(reinterpret_cast<void**>(&npin[i]), lay.bytes, hipHostMallocDefault) != hipSuccess) npin[i] = nullptr;
    if (npin[i] && hipMalloc(reinterpret_cast<void**>(&ndev[i]), lay.bytes) != hipSuccess) ndev[i] = nullptr;
    if (!npin[i] || !ndev[i]) {
      (void)hipGetLastError();
      for (int j = 0; j <= i; ++j) {
        if (npin[j]) (void)hipHostFree(npin[j]);
        if (ndev[j]) (void)hipFree(ndev[j]);
      }
      return fail(BK_CAPACITY, "bk_submit_instructions_host: out of pinned / device memory for the staging");
    }
  }
  const bk_env::HostIngress old = h;
  h.layout(env->cfg.n_books, cap);
  for (int i = 0; i < bk_env::HostIngress::SLOTS; ++i) {
    h.pin[i] = npin[i];
    h.dev[i] = ndev[i];
    if (old.pin[i] && old.ticket_of[i] != ~0ull) {
      std::memcpy(h.pin[i] + h.o_out, old.pin[i] + old.o_out, old.n_elem[i] * 8);
      std::memcpy(h.pin[i] + h.o_st, old.pin[i] + old.o_st, static_cast<size_t>(env->cfg.n_books) * 8);
    }
    // a view into the old pinned block (of a ticket < next_ticket) is valid until two more submits: the block goes when the
    // submit of ticket next_ticket + 1 starts.  The device block has no outside references (every stream was drained above).
    if (old.pin[i]) h.retired.push_back({old.pin[i], h.next_ticket + 1});
    if (old.dev[i]) HIPCHK(hipFree(old.dev[i]));
  }
  return BK_OK;
}
void hi_release_retired(bk_env* env, bool all) {
  auto& r = env->hi.retired;
  for (size_t i = 0; i < r.size();) {
    if (all || env->hi.next_ticket >= r[i].free_from_ticket) {
      (void)hipHostFree(r[i].pin);
      r[i] = r.back();
      r.pop_back();
    } else {
      ++i;
    }
  }
}

// The staging copies: the calling thread alone below 1 MB, else FOUR threads of the env's pool claiming 256 KB pieces one at a
// time.  Measured on three boxes at 9.8 MB per step (scripts/host_driven_rate.py, `tickets`): one thread 0.30 - 0.40 ms (the copy
// then bounds the step: 15 M book-steps/s), sixteen threads 0.19 ms on a quiet box (24.6 M) but 0.9 ms on a busy one (a parallel
// copy is as fast as its slowest worker gets scheduled, and sixteen runnable threads meet the container's CPU quota), four
// threads with pieces claimed dynamically: see docs/EXPERIMENTS.md.
struct HiSeg {
  void* dst;
  const void* src;
  size_t bytes;
};
void hi_copy(bk_env* env, const HiSeg* segs, int n_segs) {
  constexpr size_t PIECE = 256u << 10, PARALLEL_FROM = 1u << 20;
  size_t total = 0;
  for (int i = 0; i < n_segs; ++i)
    if (segs[i].dst != segs[i].src) total += segs[i].bytes;  // (dst == src: the caller filled the staging array in place)
  if (total < PARALLEL_FROM) {
    for (int i = 0; i < n_segs; ++i)
      if (segs[i].dst != segs[i].src && segs[i].bytes) std::memcpy(segs[i].dst, segs[i].src, segs[i].bytes);
    return;
  }
  struct Piece {
    char* d;
    const char* s;
    size_t n;
  };
  std::vector<Piece> pieces;
  for (int i = 0; i < n_segs; ++i) {
    const HiSeg& g = segs[i];
    if (g.dst == g.src) continue;
    for (size_t o = 0; o < g.bytes; o += PIECE)
      pieces.push_back({static_cast<char*>(g.dst) + o, static_cast<const char*>(g.src) + o, std::min(PIECE, g.bytes - o)});
  }
  std::atomic<size_t> next{0};
  auto worker = [&](unsigned) {
    for (size_t k = next.fetch_add(1); k < pieces.size(); k = next.fetch_add(1)) std::memcpy(pieces[k].d, pieces[k].s, pieces[k].n);
  };
  const unsigned nt = std::min<unsigned>(4u, env->host_pool().threads());
  if (nt <= 1 || !env->host_pool().run(nt, worker)) worker(0);
}
}  // namespace

int bk_ingress_staging(bk_env* env, uint64_t min_elements, bk_ingress_arrays* out) {
  if (!env || !out) return fail(BK_INVALID_ARGUMENT, "null argument");
  if (!env->device_ingress) return fail(BK_INVALID_ARGUMENT, "call bk_device_ingress_enable first");
  if (int rc = use_device(env)) return rc;
  if (int rc = hi_ensure(env, min_elements)) return rc;
  bk_env::HostIngress& h = env->hi;
  const int s = static_cast<int>(h.next_ticket % bk_env::HostIngress::SLOTS);
  // the slot's previous ticket (two submits ago) must have been consumed before the caller writes into its arrays
  if (h.ticket_of[s] != ~0ull) HIPCHK(hipEventSynchronize(h.e_done[s]));
  char* p = h.pin[s];
  out->capacity = h.cap;
  out->book_offsets = reinterpret_cast<uint64_t*>(p + h.o_off);
  out->action = reinterpret_cast<uint32_t*>(p + h.o_act);
  out->side = reinterpret_cast<uint8_t*>(p + h.o_side);
  out->vol = reinterpret_cast<uint32_t*>(p + h.o_vol);
  out->trader_id = reinterpret_cast<uint32_t*>(p + h.o_trd);
  out->price = reinterpret_cast<uint32_t*>(p + h.o_prc);
  out->order_id = reinterpret_cast<uint64_t*>(p + h.o_oid);
  return BK_OK;
}

int bk_submit_instructions_host(bk_env* env, const uint64_t* book_offsets, const uint32_t* action, const uint8_t* side,
                                const uint32_t* vol, const uint32_t* trader_id, const uint32_t* price,
                                const uint64_t* order_id, uint64_t* out_ticket) {
  if (!env || !book_offsets) return fail(BK_INVALID_ARGUMENT, "null argument");
  if (!env->device_ingress) return fail(BK_INVALID_ARGUMENT, "call bk_device_ingress_enable first");
  const size_t B = env->cfg.n_books;
  const uint64_t n = book_offsets[B];
  if (book_offsets[0] != 0) return fail(BK_INVALID_ARGUMENT, "book_offsets[0] must be 0");
  for (size_t b = 0; b < B; ++b)
    if (book_offsets[b + 1] < book_offsets[b]) return fail(BK_INVALID_ARGUMENT, "book_offsets must be non-decreasing");
  if (n && (!action || !side || !vol || !trader_id || !price || !order_id))
    return fail(BK_INVALID_ARGUMENT, "null instruction array");
  if (int rc = use_device(env)) return rc;
  if (int rc = hi_ensure(env, n)) return rc;
  hi_release_retired(env, false);  // (pinned blocks replaced by a growth two submits ago: their tickets' views have expired)
  bk_env::HostIngress& h = env->hi;
  const uint64_t ticket = h.next_ticket;
  const int s = static_cast<int>(ticket % bk_env::HostIngress::SLOTS);
  if (h.ticket_of[s] != ~0ull) HIPCHK(hipEventSynchronize(h.e_done[s]));  // slot free: its upload, ingest and download are over
  char *pp = h.pin[s], *dd = h.dev[s];
  const HiSeg segs[7] = {{pp + h.o_off, book_offsets, (B + 1) * 8}, {pp + h.o_oid, order_id, n * 8}, {pp + h.o_act, action, n * 4},
                         {pp + h.o_vol, vol, n * 4},     {pp + h.o_trd, trader_id, n * 4}, {pp + h.o_prc, price, n * 4},
                         {pp + h.o_side, side, n}};
  auto up = [&](size_t off, size_t bytes) -> hipError_t {
    return bytes ? hipMemcpyAsync(dd + off, pp + off, bytes, hipMemcpyHostToDevice, h.in) : hipSuccess;
  };
  // Large batches in three groups of ~a third of the bytes, each uploaded as soon as it is staged: the link works on group g
  // while the host copies group g + 1 (a caller that fetches the ids before every step - the reference's call shape - waits
  // for copy + upload + k_ingest + download in sequence: 0.25 + 0.2 ms of it at 8 192 books x 48 instructions were these two).
  const bool grouped = n * 27 >= (3u << 20);
  if (!grouped) hi_copy(env, segs, 7);
  if (grouped) hi_copy(env, segs + 0, 2);
  HIPCHK(up(h.o_off, (B + 1) * 8));
  HIPCHK(up(h.o_oid, n * 8));
  if (grouped) hi_copy(env, segs + 2, 2);
  HIPCHK(up(h.o_act, n * 4));
  HIPCHK(up(h.o_vol, n * 4));
  if (grouped) hi_copy(env, segs + 4, 3);
  HIPCHK(up(h.o_trd, n * 4));
  HIPCHK(up(h.o_prc, n * 4));
  HIPCHK(up(h.o_side, n));
  HIPCHK(hipEventRecord(h.e_h2d[s], h.in));
  HIPCHK(hipStreamWaitEvent(env->stream, h.e_h2d[s], 0));
  if (n) {
    // (k_ingest leaves out_ids alone from a book's failing element on: those read u64::MAX here, not a stale ticket's ids)
    HIPCHK(hipMemsetAsync(dd + h.o_out, 0xFF, n * 8, env->stream));
    if (int rc = bk_submit_instructions_device(
            env, reinterpret_cast<const uint64_t*>(dd + h.o_off), reinterpret_cast<const uint32_t*>(dd + h.o_act),
            reinterpret_cast<const uint8_t*>(dd + h.o_side), reinterpret_cast<const uint32_t*>(dd + h.o_vol),
            reinterpret_cast<const uint32_t*>(dd + h.o_trd), reinterpret_cast<const uint32_t*>(dd + h.o_prc),
            reinterpret_cast<const uint64_t*>(dd + h.o_oid), reinterpret_cast<uint64_t*>(dd + h.o_out),
            reinterpret_cast<uint32_t*>(dd + h.o_st)))
      return rc;
  } else {
    HIPCHK(hipMemsetAsync(dd + h.o_st, 0, B * 8, env->stream));  // no element for any book: every status {OK, 0}
  }
  HIPCHK(hipEventRecord(h.e_ing[s], env->stream));
  HIPCHK(hipStreamWaitEvent(h.out, h.e_ing[s], 0));
  if (n) HIPCHK(hipMemcpyAsync(pp + h.o_out, dd + h.o_out, n * 8, hipMemcpyDeviceToHost, h.out));
  HIPCHK(hipMemcpyAsync(pp + h.o_st, dd + h.o_st, B * 8, hipMemcpyDeviceToHost, h.out));
  HIPCHK(hipEventRecord(h.e_done[s], h.out));
  h.ticket_of[s] = ticket;
  h.n_elem[s] = n;
  h.next_ticket = ticket + 1;
  if (out_ticket) *out_ticket = ticket;
  return BK_OK;
}

int bk_submit_result_view(bk_env* env, uint64_t ticket, const uint64_t** out_ids, const uint32_t** status,
                          uint32_t* first_failed_book) {
  if (!env) return fail(BK_INVALID_ARGUMENT, "null env");
  bk_env::HostIngress& h = env->hi;
  const int s = static_cast<int>(ticket % bk_env::HostIngress::SLOTS);
  if (ticket >= h.next_ticket || h.ticket_of[s] != ticket)
    return fail(BK_INVALID_ARGUMENT, "unknown or expired ticket (a ticket's results stay readable until two more submits)");
  if (int rc = use_device(env)) return rc;
  HIPCHK(hipEventSynchronize(h.e_done[s]));
  const size_t B = env->cfg.n_books;
  const uint32_t* st = reinterpret_cast<const uint32_t*>(h.pin[s] + h.o_st);
  if (out_ids) *out_ids = reinterpret_cast<const uint64_t*>(h.pin[s] + h.o_out);
  if (status) *status = st;
  if (first_failed_book) {
    *first_failed_book = 0xFFFFFFFFu;
    for (size_t b = 0; b < B; ++b)
      if (st[2 * b] != BK_OK) {
        *first_failed_book = static_cast<uint32_t>(b);
        break;
      }
  }
  return BK_OK;
}

int bk_submit_result(bk_env* env, uint64_t ticket, uint64_t* out_ids, uint32_t* status, uint32_t* first_failed_book) {
  if (!env) return fail(BK_INVALID_ARGUMENT, "null env");
  bk_env::HostIngress& h = env->hi;
  const int s = static_cast<int>(ticket % bk_env::HostIngress::SLOTS);
  if (ticket >= h.next_ticket || h.ticket_of[s] != ticket)
    return fail(BK_INVALID_ARGUMENT, "unknown or expired ticket (a ticket's results stay readable until two more submits)");
  if (int rc = use_device(env)) return rc;
  HIPCHK(hipEventSynchronize(h.e_done[s]));
  const size_t B = env->cfg.n_books;
  const uint32_t* st = reinterpret_cast<const uint32_t*>(h.pin[s] + h.o_st);
  if (out_ids) {
    const HiSeg seg{out_ids, h.pin[s] + h.o_out, h.n_elem[s] * 8};
    hi_copy(env, &seg, 1);
  }
  if (status) std::memcpy(status, st, B * 8);
  if (first_failed_book) {
    *first_failed_book = 0xFFFFFFFFu;
    for (size_t b = 0; b < B; ++b)
      if (st[2 * b] != BK_OK) {
        *first_failed_book = static_cast<uint32_t>(b);
        break;
      }
  }
  return BK_OK;
}

// Env::step over the device-resident queues, asynchronous on the env's stream (bk_step = this + a wait)
static void launch_accounts_fold(bk_env* env) {
  accounts::FoldArgs g{};
  g.state = env->state.p;
  g.stride = env->stride;
  g.n_books = env->cfg.n_books;
  g.trades = reinterpret_cast<const bk_u32x4*>(env->trades.p);
  g.trade_cap = env->cfg.trade_capacity;
  g.dorders = env->dorders.p;
  g.max_orders = env->cfg.max_orders;
  g.acct = env->acct.p;
  g.n_traders = env->acct_traders;
  g.seen = env->acct_seen.p;
  // (the last fold of a step consumes for all: the flow's and the bars' folds run in front of this one and leave the records alone)
  g.consume = env->acct_consume || env->bars_consume || env->flow_consume ? 1u : 0u;
  launch_wave_per_book(env, accounts::k_fold, accounts::FOLD_WAVES, g);
}

// the step the env's counter reads k -> slot k % window of every book; in front of the accounts' fold, which then consumes
static void launch_bars_fold(bk_env* env) {
  trade_bars::FoldArgs g{};
  g.state = env->state.p;
  g.stride = env->stride;
  g.n_books = env->cfg.n_books;
  g.trades = reinterpret_cast<const bk_u32x4*>(env->trades.p);
  g.trade_cap = env->cfg.trade_capacity;
  g.bars = env->bars.p;
  g.window = env->bars_window;
  g.slot = static_cast<uint32_t>(env->steps_done % env->bars_window);
  g.prev_slot = (g.slot + env->bars_window - 1u) % env->bars_window;
  g.seen = env->bars_seen.p;
  g.consume = !env->acct_traders && (env->bars_consume || env->flow_consume) ? 1u : 0u;
  launch_wave_per_book(env, trade_bars::k_fold, trade_bars::FOLD_WAVES, g);
}

// the flow table: every book's records [its cursor, H_TRADES); `consume`: the fold ends by H_TRADE_BASE = H_TRADES
static void launch_flow_fold(bk_env* env, bool consume) {
  flow::FoldArgs g{};
  g.state = env->state.p;
  g.stride = env->stride;
  g.n_books = env->cfg.n_books;
  g.trades = reinterpret_cast<const bk_u32x4*>(env->trades.p);
  g.trade_cap = env->cfg.trade_capacity;
  g.K = env->flow_lags;
  g.table = env->flow_table.p;
  g.carry = env->flow_carry.p;
  g.seen = env->flow_seen.p;
  g.consume = consume ? 1u : 0u;
  launch_wave_per_book(env, flow::k_fold, flow::FOLD_WAVES, g);
}

// carry of the masked books (one mask byte per M books; nullptr: every book) -> invalid, their cursors -> the books'
// H_TRADES; unless carry_only their words -> 0 as well
static void launch_flow_clear(bk_env* env, const uint8_t* mask_dev, uint32_t M, bool carry_only) {
  flow::ClearArgs g{};
  g.books = ring::Masked{mask_dev, M, env->cfg.n_books};
  g.state = env->state.p;
  g.stride = env->stride;
  g.K = env->flow_lags;
  g.carry_only = carry_only ? 1u : 0u;
  g.table = env->flow_table.p;
  g.carry = env->flow_carry.p;
  g.seen = env->flow_seen.p;
  launch_wave_per_book(env, flow::k_clear, flow::FOLD_WAVES, g.books.n_books, g);
}

// rows of the masked books (one mask byte per M books; nullptr: every book) -> 0, their cursors -> the books' H_TRADES
static void launch_bars_clear(bk_env* env, const uint8_t* mask_dev, uint32_t M) {
  trade_bars::ClearArgs g{};
  g.mask = mask_dev;
  g.M = M;
  g.state = env->state.p;
  g.stride = env->stride;
  g.n_books = env->cfg.n_books;
  g.bars = env->bars.p;
  g.window = env->bars_window;
  g.seen = env->bars_seen.p;
  launch_wave_per_book(env, trade_bars::k_clear, trade_bars::FOLD_WAVES, g);
}

// rows of the masked books (one mask byte per M books; nullptr: every book) -> 0, their cursors -> the books' H_TRADES
static void launch_accounts_clear(bk_env* env, const uint8_t* mask_dev, uint32_t M) {
  accounts::ClearArgs g{};
  g.mask = mask_dev;
  g.M = M;
  g.state = env->state.p;
  g.stride = env->stride;
  g.n_books = env->cfg.n_books;
  g.acct = env->acct.p;
  g.n_traders = env->acct_traders;
  g.seen = env->acct_seen.p;
  launch_wave_per_book(env, accounts::k_clear, accounts::FOLD_WAVES, g);
}

// the open-order rows of the masked books (one mask byte per M books; nullptr: every book) from their pools as they are at
// this point of the env's stream: one launch, no allocation, no stream wait, no host read
static void launch_open_orders_refresh(bk_env* env, const uint8_t* mask_dev, uint32_t M) {
  open_orders::RefreshArgs g{};
  g.mask = mask_dev;
  g.M = M;
  g.state = env->state.p;
  g.stride = env->stride;
  g.n_books = env->cfg.n_books;
  g.dorders = reinterpret_cast<const uint32_t*>(env->dorders.p);
  g.max_orders = env->cfg.max_orders;
  g.summary = env->open_summary.p;
  g.entries = env->open_entries.p;
  g.n_traders = env->open_traders;
  g.depth = env->open_depth;
  g.depth_inv = g.depth ? ((1u << 24) + g.depth - 1u) / g.depth : 0u;
  by_R(env->R, [&](auto r) { launch_wave_per_book(env, open_orders::k_refresh<decltype(r)::value>, open_orders::REFRESH_WAVES, g); });
}

// the queue rows of the masked books from their pools and the entries the open-order refresh in front of it wrote: one
// launch, no allocation, no stream wait, no host read
static void launch_open_queue_refresh(bk_env* env, const uint8_t* mask_dev, uint32_t M) {
  open_queue::RefreshArgs g{};
  g.mask = mask_dev;
  g.M = M;
  g.state = env->state.p;
  g.stride = env->stride;
  g.n_books = env->cfg.n_books;
  g.entries = env->open_entries.p;
  g.queue = env->open_queue.p;
  g.n_entries = env->open_traders * env->open_depth;  // (<= 65536 * 64)
  by_R(env->R, [&](auto r) { launch_wave_per_book(env, open_queue::k_refresh<decltype(r)::value>, open_queue::REFRESH_WAVES, g); });
}

// both tables of the open-order view: the rows, then - for an env with the queue view - their queue positions
static void launch_open_refresh(bk_env* env, const uint8_t* mask_dev, uint32_t M) {
  launch_open_orders_refresh(env, mask_dev, M);
  if (env->open_queue.p) launch_open_queue_refresh(env, mask_dev, M);
}

int bk_step_async(bk_env* env) {
  if (!env) return fail(BK_INVALID_ARGUMENT, "null env");
  if (!env->device_ingress) return fail(BK_INVALID_ARGUMENT, "bk_step_async steps the device-resident queues: call bk_device_ingress_enable first");
  if (int rc = use_device(env)) return rc;
  if (int rc = reserve_stamps(env, env->qcap)) return rc;  // (the queues' lengths are known on the device only)
  const DevArgs a = env->args();
  // (the shuffle permutation's LDS is sized for a full queue: the host does not know the queues' lengths - nothing of this
  // step has been on the host)
  const int rc = by_R(env->R, [&](auto r) { return launch_events<decltype(r)::value>(env, a, env->steps_done, env->qcap); });
  if (rc != BK_OK) return rc;
  if (env->flow_lags) {  // the flow table: this step's new trade records, right behind the event kernel; it consumes only alone
    launch_flow_fold(env, env->flow_consume && !env->bars_window && !env->acct_traders);
    HIPCHK(hipGetLastError());
  }
  if (env->bars_window) {  // trade bars: the same records
    launch_bars_fold(env);
    HIPCHK(hipGetLastError());
  }
  if (env->acct_traders) {  // trader accounts: the same records
    launch_accounts_fold(env);
    HIPCHK(hipGetLastError());
  }
  if (env->open_traders) {  // open orders: the pools as this step left them
    launch_open_refresh(env, nullptr, 1);
    HIPCHK(hipGetLastError());
  }
  HIPCHK(hipMemsetAsync(env->dqlen.p, 0, static_cast<size_t>(env->cfg.n_books / env->M) * 4, env->stream));
  env->steps_done += 1;
  env->ingest_epoch += 1;
  return BK_OK;
}

// The held ids of the installed RandomAgents, one row per unit (book, or market when assets > 1), made at the first update
// after an install: every agent holds None; the old orders stay on the books, unowned.
static int make_agent_held(bk_env* env) {
  if (!env->agent_held_stale) return BK_OK;
  const size_t n = static_cast<size_t>(env->cfg.n_books / env->M) * env->n_agents_total;
  HIPCHK(hipStreamSynchronize(env->stream));  // (an earlier launch may still read the buffers replaced here)
  HIPCHK(env->agent_held.alloc(n));
  if (n) HIPCHK(hipMemset(env->agent_held.p, 0xFF, n * 4));
  if (env->table.empty()) {
    HIPCHK(env->agent_groups.alloc(env->groups.size()));
    HIPCHK(hipMemcpy(env->agent_groups.p, env->groups.data(), env->groups.size() * sizeof(Group), hipMemcpyHostToDevice));
  } else {
    HIPCHK(env->agent_groups.alloc(0));
  }
  env->agent_held_stale = false;
  return BK_OK;
}

// The members' lists, lengths and momentum state, one row per unit and member, made at the first update after an install:
// empty lists, no momentum state; the old orders stay, unowned.
static int make_member_rows(bk_env* env) {
  if (!env->member_lists_stale) return BK_OK;
  const size_t units = env->cfg.n_books / env->M;
  HIPCHK(hipStreamSynchronize(env->stream));  // (an earlier launch may still read the buffers replaced here)
  uint32_t max_n = 0;
  for (uint32_t n : env->member_n) max_n = std::max(max_n, n);
  env->member_list_cap = bkd::ingress::members_list_cap(static_cast<uint32_t>(env->R), max_n);
  const size_t rows = units * env->n_mixed;
  HIPCHK(env->member_lists.alloc(rows * env->member_list_cap));
  HIPCHK(env->member_lens.alloc(rows));
  HIPCHK(env->member_state.alloc(rows * 2));
  HIPCHK(env->member_flags.alloc(units));
  HIPCHK(env->member_id0_dev.alloc(env->member_id0.size()));
  HIPCHK(hipMemset(env->member_lists.p, 0xFF, rows * env->member_list_cap * 4));  // (a RandomAgents member's agents hold None)
  HIPCHK(hipMemset(env->member_lens.p, 0, rows * 4));
  HIPCHK(hipMemset(env->member_state.p, 0, rows * 16));
  HIPCHK(hipMemset(env->member_flags.p, 0, units * 4));
  HIPCHK(hipMemcpy(env->member_id0_dev.p, env->member_id0.data(), env->member_id0.size() * 4, hipMemcpyHostToDevice));
  env->member_lists_stale = false;
  return BK_OK;
}

// agents.update(env, rng) (random_agent.rs:85-119) of the installed RandomAgents for every book, into the device-resident
// queues at this point of the book's stream (agents_ingress.hpp k_update_agents), asynchronous on the env's stream.  The
// agents only place and cancel: they never queue a modification, so k_ingest's hint for k_step_events stays as it is.
int bk_update_agents(bk_env* env) {
  if (!env) return fail(BK_INVALID_ARGUMENT, "null env");
  if (!env->device_ingress)
    return fail(BK_INVALID_ARGUMENT, "bk_update_agents queues the agents' orders in the device-resident queues: call "
                                     "bk_device_ingress_enable first");
  if (env->M > 1) return fail(BK_INVALID_ARGUMENT, "bk_update_agents runs RandomAgents on independent books (assets == 1)");
  if (env->n_mixed)
    return fail(BK_INVALID_ARGUMENT, "bk_update_agents runs RandomAgents only: this env has an AgentSet with Noise / "
                                     "Momentum members");
  if (env->groups.empty()) return fail(BK_INVALID_ARGUMENT, "no RandomAgents groups installed (bk_set_random_agents)");
  if (int rc = use_device(env)) return rc;
  const uint32_t B = env->cfg.n_books, NA = env->n_agents_total;
  if (int rc = make_agent_held(env)) return rc;
  AgentsIngressArgs g{};
  g.io = env->ingress_args();
  g.n_agents = NA;
  g.groups = env->table.empty() ? env->agent_groups.p : env->dtable.p;
  g.g_stride = env->table.empty() ? 0u : static_cast<uint32_t>(env->groups.size());
  g.held = env->agent_held.p;
  by_R(env->R, [&](auto r) {
    hipLaunchKernelGGL(k_update_agents<decltype(r)::value>, dim3(B), dim3(64), 0, env->stream, g);
    return 0;
  });
  HIPCHK(hipGetLastError());
  env->ingest_epoch += 1;
  return BK_OK;
}

// agents.update(env, rng) of the installed AgentSet - NoiseAgent / MomentumAgent members (noise_agent.rs:127-176,
// momentum_agent.rs:146-208, common.rs:56-75), with or without RandomAgents members, in declaration order - for every book
// into the device-resident queues at this point of the book's stream (members_ingress.hpp k_update_members), asynchronous
// on the env's stream.  The members only place and cancel: k_ingest's hint for k_step_events stays as it is.
int bk_update_members(bk_env* env) {
  if (!env) return fail(BK_INVALID_ARGUMENT, "null env");
  if (!env->device_ingress)
    return fail(BK_INVALID_ARGUMENT, "bk_update_members queues the members' orders in the device-resident queues: call "
                                     "bk_device_ingress_enable first");
  if (env->M > 1) return fail(BK_INVALID_ARGUMENT, "bk_update_members runs an AgentSet on independent books (assets == 1)");
  if (!env->n_mixed) {
    if (!env->groups.empty())
      return fail(BK_INVALID_ARGUMENT, "this env has RandomAgents groups only (bk_set_random_agents*): they are run by "
                                       "bk_update_agents");
    return fail(BK_INVALID_ARGUMENT, "no AgentSet installed (bk_set_agents / bk_set_agents_per_book)");
  }
  if (int rc = use_device(env)) return rc;
  const uint32_t B = env->cfg.n_books, NM = env->n_mixed;
  if (int rc = make_member_rows(env)) return rc;
  bkd::ingress::MembersIngressArgs g{};
  g.io = env->ingress_args();
  g.n_members = NM;
  g.tick = env->cfg.tick_size;
  g.descs = env->mtable.empty() ? env->mixed_descs.p : env->dmtable.p;
  g.id_start = env->member_id0_dev.p;
  g.d_stride = env->mtable.empty() ? 0u : NM;
  g.list_cap = env->member_list_cap;
  g.lists = env->member_lists.p;
  g.lens = env->member_lens.p;
  g.mstate = env->member_state.p;
  g.mflags = env->member_flags.p;
  by_R(env->R, [&](auto r) {
    hipLaunchKernelGGL(bkd::ingress::k_update_members<decltype(r)::value>, dim3(B), dim3(64), 0, env->stream, g);
    return 0;
  });
  HIPCHK(hipGetLastError());
  env->ingest_epoch += 1;
  return BK_OK;
}

// RandomMarketAgents::update (random_agent.rs:204-245) of the groups installed by bk_set_random_market_agents or the
// per-market table of bk_set_random_agents_per_book, for every market, into the market's device-resident queue at this
// point of its stream (market_ingress.hpp k_update_market_agents), asynchronous on the env's stream.  An env of one asset
// is a market of one book: there this entry and bk_update_agents share the held ids and are interchangeable step by step.
int bk_update_market_agents(bk_env* env) {
  if (!env) return fail(BK_INVALID_ARGUMENT, "null env");
  if (!env->device_ingress)
    return fail(BK_INVALID_ARGUMENT, "bk_update_market_agents queues the agents' orders in the device-resident queues: call "
                                     "bk_device_ingress_enable first");
  if (env->n_mixed)
    return fail(BK_INVALID_ARGUMENT, "bk_update_market_agents runs RandomMarketAgents only: this env has a set with Noise / "
                                     "Momentum members, which bk_update_market_members runs");
  if (env->groups.empty())
    return fail(BK_INVALID_ARGUMENT, "no RandomMarketAgents groups installed (bk_set_random_market_agents)");
  if (int rc = use_device(env)) return rc;
  if (int rc = make_agent_held(env)) return rc;
  bkd::ingress::MarketAgentsArgs g{};
  g.io = env->ingress_args();
  g.assets = env->M;
  g.n_agents = env->n_agents_total;
  g.n_groups = static_cast<uint32_t>(env->groups.size());
  g.groups = env->table.empty() ? env->agent_groups.p : env->dtable.p;
  g.g_stride = env->table.empty() ? 0u : g.n_groups;
  g.held = env->agent_held.p;
  by_R(env->R, [&](auto r) {
    hipLaunchKernelGGL(bkd::ingress::k_update_market_agents<decltype(r)::value>, dim3(env->cfg.n_books / env->M), dim3(64), 0,
                       env->stream, g);
    return 0;
  });
  HIPCHK(hipGetLastError());
  env->ingest_epoch += 1;
  return BK_OK;
}

// MarketAgent::update of the set installed by bk_set_market_agents or bk_set_agents_per_book - NoiseMarketAgent
// (noise_agent.rs:226-340), MomentumMarketAgent (momentum_agent.rs:282-397) and RandomMarketAgents members, in declaration
// order - for every market, into the market's device-resident queue at this point of its stream (market_ingress.hpp
// k_update_market_members), asynchronous on the env's stream.  On an env of one asset it shares the lists and the
// momentum state with bk_update_members.
int bk_update_market_members(bk_env* env) {
  if (!env) return fail(BK_INVALID_ARGUMENT, "null env");
  if (!env->device_ingress)
    return fail(BK_INVALID_ARGUMENT, "bk_update_market_members queues the members' orders in the device-resident queues: call "
                                     "bk_device_ingress_enable first");
  if (!env->n_mixed) {
    if (!env->groups.empty())
      return fail(BK_INVALID_ARGUMENT, "this env has RandomMarketAgents groups only (bk_set_random_market_agents*): they are "
                                       "run by bk_update_market_agents");
    return fail(BK_INVALID_ARGUMENT, "no MarketAgentSet installed (bk_set_market_agents / bk_set_agents_per_book)");
  }
  if (int rc = use_device(env)) return rc;
  if (int rc = make_member_rows(env)) return rc;
  bkd::ingress::MarketMembersArgs g{};
  g.io = env->ingress_args();
  g.assets = env->M;
  for (int i = 0; i < MAX_ASSETS; ++i) g.asset_tick[i] = env->asset_tick[i];
  for (uint32_t j = 0; j < env->n_mixed; ++j) g.member_assets |= static_cast<uint64_t>(env->member_asset[j]) << (8u * j);
  g.n_members = env->n_mixed;
  g.descs = env->mtable.empty() ? env->mixed_descs.p : env->dmtable.p;
  g.id_start = env->member_id0_dev.p;
  g.d_stride = env->mtable.empty() ? 0u : env->n_mixed;
  g.list_cap = env->member_list_cap;
  g.lists = env->member_lists.p;
  g.lens = env->member_lens.p;
  g.mstate = env->member_state.p;
  g.mflags = env->member_flags.p;
  by_R(env->R, [&](auto r) {
    hipLaunchKernelGGL(bkd::ingress::k_update_market_members<decltype(r)::value>, dim3(env->cfg.n_books / env->M), dim3(64), 0,
                       env->stream, g);
    return 0;
  });
  HIPCHK(hipGetLastError());
  env->ingest_epoch += 1;
  return BK_OK;
}

// Member `member`'s `orders` vector of one book as the device holds it after the last bk_update_members (the ids a
// RandomAgents member's agents hold, u64::MAX for None): *n_out = its length, the first min(cap, length) ids in out_ids.
int bk_member_orders(bk_env* env, uint32_t book, uint32_t member, uint32_t cap, uint64_t* out_ids, uint32_t* n_out) {
  if (int rc = check_book(env, book)) return rc;
  if (!env->device_ingress || !env->n_mixed)
    return fail(BK_INVALID_ARGUMENT, "bk_member_orders reads the lists of bk_update_members: no AgentSet on a device-ingress env");
  if (member >= env->n_mixed) return fail(BK_INVALID_ARGUMENT, "member index out of range");
  if (cap && !out_ids) return fail(BK_INVALID_ARGUMENT, "null argument");
  if (int rc = use_device(env)) return rc;
  const bool random = env->member_type[member] == BK_AGENT_RANDOM;
  uint32_t n = random ? env->member_n[member] : 0u;
  std::vector<uint32_t> ids(n, AGENT_HELD_NONE);
  if (!env->member_lists_stale) {  // (stale: installed and not yet updated - empty lists, every agent holds None)
    HIPCHK(hipStreamSynchronize(env->stream));
    const size_t row = static_cast<size_t>(book / env->M) * env->n_mixed + member;  // (a market's rows: ids of the member's asset)
    if (!random) HIPCHK(hipMemcpy(&n, env->member_lens.p + row, 4, hipMemcpyDeviceToHost));
    n = std::min(n, env->member_list_cap);
    ids.resize(n);
    if (n) HIPCHK(hipMemcpy(ids.data(), env->member_lists.p + row * env->member_list_cap, n * 4ull, hipMemcpyDeviceToHost));
  }
  for (uint32_t i = 0; i < n && i < cap; ++i) out_ids[i] = ids[i] == AGENT_HELD_NONE ? ~0ull : ids[i];
  if (n_out) *n_out = n;
  return BK_OK;
}

int bk_order_status(bk_env* env, uint32_t book, uint64_t order_id, uint8_t* out_status) {
  if (int rc = check_book(env, book)) return rc;
  if (int rc = mirror_orders(env, book)) return rc;
  BookHost& bh = env->books[book];
  if (order_id >= bh.orders.size())
    return fail(BK_UNKNOWN_ORDER_ID, "No order with id " + std::to_string(order_id) + " exists");
  if (env->cfg.max_orders == 0) return fail(BK_INVALID_ARGUMENT, "order log disabled (max_orders == 0)");
  if (order_id >= env->cfg.max_orders) return fail(BK_CAPACITY, "order id beyond the order-log capacity");
  if (int rc = use_device(env)) return rc;
  if (int rc = refresh_log(env, book)) return rc;
  bk_order o;
  fill_order(env, bh, order_id, &o);
  if (out_status) *out_status = o.status;
  return BK_OK;
}

int bk_order_count(bk_env* env, uint32_t book, uint64_t* out) {
  if (int rc = check_book(env, book)) return rc;
  if (int rc = mirror_orders(env, book)) return rc;
  if (out) *out = env->books[book].orders.size();
  return BK_OK;
}

int bk_get_orders(bk_env* env, uint32_t book, uint64_t first, uint64_t n, bk_order* out) {
  if (int rc = check_book(env, book)) return rc;
  if (int rc = mirror_orders(env, book)) return rc;
  BookHost& bh = env->books[book];
  if (first > bh.orders.size() || n > bh.orders.size() - first) return fail(BK_INVALID_ARGUMENT, "order range out of bounds");
  if (n && !out) return fail(BK_INVALID_ARGUMENT, "null argument");
  if (bh.orders.size() > env->cfg.max_orders && env->cfg.max_orders > 0 && bh.n_uploaded > env->cfg.max_orders)
    return fail(BK_CAPACITY, "order log capacity exceeded");
  if (int rc = use_device(env)) return rc;
  if (env->cfg.max_orders)
    if (int rc = refresh_log(env, book)) return rc;
  for (uint64_t i = 0; i < n; ++i) fill_order(env, bh, first + i, out + i);
  return BK_OK;
}

// ------------------------------------------------------------------ on-device order flow
int bk_set_random_market_agents(bk_env* env, uint32_t n_groups, const bk_random_agents* groups,
                                const uint32_t* assets) {
  if (!env || (!groups && n_groups)) return fail(BK_INVALID_ARGUMENT, "null argument");
  if (n_groups > MAX_GROUPS) return fail(BK_INVALID_ARGUMENT, "at most 8 agent groups");
  std::vector<Group> gs(n_groups);
  uint64_t total = 0;
  std::string msg;
  if (int rc = make_groups(groups, n_groups, assets, env->M, env->asset_tick, gs.data(), &total, &msg))  // (agent_table.hpp)
    return fail(rc, msg);
  if (total > env->cfg.max_live_orders) return fail(BK_CAPACITY, CAPACITY_MSG);
  env->groups = gs;
  env->n_agents_total = static_cast<uint32_t>(total);
  env->n_mixed = 0;
  env->table.clear();  // (replaces a per-unit table)
  (void)env->dtable.alloc(0);
  env->mtable.clear();  // (and a members' table)
  (void)env->dmtable.alloc(0);
  env->agents_hash = gs.empty() ? 0 : groups_hash(gs.data(), gs.size());
  env->agent_held_stale = true;  // (a new RandomAgents::new: the agents hold nothing)
  env->agent_installs += 1;
  return BK_OK;
}

// RandomAgents groups whose parameters differ per unit (book, or market when assets > 1): every row is checked and
// preprocessed as bk_set_random_market_agents does one (agent_table.hpp make_group_table); the table goes to the device,
// where the PB forms of k_agents_fsm / k_agents_wave / k_run_wave read unit u's row.  Nothing changes on a failure.
int bk_set_random_agents_per_book(bk_env* env, uint32_t n_groups, const bk_random_agents* groups, const uint32_t* assets) {
  if (!env || (!groups && n_groups)) return fail(BK_INVALID_ARGUMENT, "null argument");
  if (n_groups == 0) return fail(BK_INVALID_ARGUMENT, "a per-unit table needs at least one group");
  if (n_groups > MAX_GROUPS) return fail(BK_INVALID_ARGUMENT, "at most 8 agent groups");
  const uint32_t n_units = env->cfg.n_books / env->M;
  std::vector<Group> t;
  uint64_t total = 0;
  std::string msg;
  if (int rc = make_group_table(groups, n_units, n_groups, assets, env->M, env->asset_tick, env->cfg.max_live_orders, t, &total, &msg))
    return fail(rc, msg);
  if (int rc = use_device(env)) return rc;
  DevBuf<Group> d;
  HIPCHK(d.alloc(t.size()));
  HIPCHK(hipMemcpy(d.p, t.data(), t.size() * sizeof(Group), hipMemcpyHostToDevice));
  env->dtable.swap(d);  // (the previous table, if any, is freed with `d`)
  env->groups.assign(t.begin(), t.begin() + n_groups);
  env->table.swap(t);
  env->n_agents_total = static_cast<uint32_t>(total);
  env->n_mixed = 0;
  env->mtable.clear();
  (void)env->dmtable.alloc(0);
  env->agents_hash = groups_hash(env->table.data(), env->table.size());
  env->agent_held_stale = true;
  env->agent_installs += 1;
  return BK_OK;
}

int bk_set_random_agents(bk_env* env, uint32_t n_groups, const bk_random_agents* groups) {
  return bk_set_random_market_agents(env, n_groups, groups, nullptr);  // every group on asset 0
}

int bk_set_tick_sizes(bk_env* env, uint32_t n, const uint32_t* tick_sizes) {
  if (!env || !tick_sizes) return fail(BK_INVALID_ARGUMENT, "null argument");
  if (n != env->M) return fail(BK_INVALID_ARGUMENT, "one tick size per asset");
  if (env->steps_done || !env->groups.empty()) return fail(BK_INVALID_ARGUMENT, "set the tick sizes before anything else");
  for (const BookHost& bh : env->books)
    if (!bh.orders.empty()) return fail(BK_INVALID_ARGUMENT, "set the tick sizes before anything else");
  for (uint32_t i = 0; i < n; ++i)
    if (tick_sizes[i] == 0) return fail(BK_INVALID_ARGUMENT, "tick_size must be > 0");  // orderbook.rs:159
  for (uint32_t i = 0; i < n; ++i) env->asset_tick[i] = tick_sizes[i];
  return BK_OK;
}

static int set_agents_impl(bk_env* env, uint32_t n_members, const bk_agent_desc* members, const uint32_t* assets);
// bk_run's kernels hold MAX_MEMBERS members; on an env with the device ingress, where only bk_update_members /
// bk_update_market_members run the set, MAX_INGRESS_MEMBERS
static int member_count_ok(const bk_env* env, uint32_t n_members) {
  if (n_members <= static_cast<uint32_t>(MAX_MEMBERS)) return BK_OK;
  if (!env->device_ingress) return fail(BK_INVALID_ARGUMENT, "at most 4 members in a set with Noise/Momentum agents");
  if (n_members > static_cast<uint32_t>(MAX_INGRESS_MEMBERS))
    return fail(BK_INVALID_ARGUMENT, "at most 8 members in a set with Noise/Momentum agents on a device-ingress env");
  return BK_OK;
}
static int install_members(bk_env* env, const std::vector<MixedDesc>& ds, uint32_t n_members, const uint32_t* assets,
                           const uint32_t* fixed_a, std::vector<MixedDesc> table);

int bk_set_agents(bk_env* env, uint32_t n_members, const bk_agent_desc* members) {
  if (!env || (!members && n_members)) return fail(BK_INVALID_ARGUMENT, "null argument");
  if (env->M > 1) return fail(BK_INVALID_ARGUMENT, "markets (assets > 1) take bk_set_market_agents");
  return set_agents_impl(env, n_members, members, nullptr);
}

// A MarketAgentSet of RandomMarketAgents / NoiseMarketAgent / MomentumMarketAgent members (random_agent.rs:164-247,
// noise_agent.rs:226-340, momentum_agent.rs:282-397): member i trades asset assets[i] of every market.
int bk_set_market_agents(bk_env* env, uint32_t n_members, const bk_agent_desc* members, const uint32_t* assets) {
  if (!env || (!members && n_members) || (!assets && n_members)) return fail(BK_INVALID_ARGUMENT, "null argument");
  for (uint32_t i = 0; i < n_members; ++i)
    if (assets[i] >= env->M) return fail(BK_INVALID_ARGUMENT, "member asset index out of range");
  return set_agents_impl(env, n_members, members, assets);
}

static int set_agents_impl(bk_env* env, uint32_t n_members, const bk_agent_desc* members, const uint32_t* assets) {
  bool all_random = true;
  for (uint32_t i = 0; i < n_members; ++i) all_random = all_random && members[i].type == BK_AGENT_RANDOM;
  if (all_random) {
    std::vector<bk_random_agents> g(n_members);
    for (uint32_t i = 0; i < n_members; ++i)
      g[i] = bk_random_agents{members[i].n_agents, members[i].tick_lo, members[i].tick_hi, members[i].vol_lo,
                              members[i].vol_hi, members[i].tick_size, members[i].activity_rate};
    return bk_set_random_market_agents(env, n_members, g.data(), assets);
  }
  if (int rc = member_count_ok(env, n_members)) return rc;
  if (env->agent_log)
    return fail(BK_INVALID_ARGUMENT, "the agents' order log (bk_set_agent_order_log) records RandomAgents only: "
                                     "a set with Noise / Momentum members cannot be installed on a logging env");
  if (int rc = use_device(env)) return rc;
  std::vector<MixedDesc> ds(n_members);
  uint32_t fixed_a[MAX_ASSETS];
  std::string msg;
  if (int rc = make_mixed_descs(members, n_members, assets, env->asset_tick, ds.data(), fixed_a, &msg))  // (agent_table.hpp)
    return fail(rc, msg);
  if (!mixed_capacity_ok(fixed_a, env->M, env->cfg.max_live_orders)) return fail(BK_CAPACITY, MIXED_CAPACITY_MSG);
  if (int rc = install_members(env, ds, n_members, assets, fixed_a, {})) return rc;
  env->member_id0.resize(n_members);
  for (uint32_t i = 0; i < n_members; ++i) env->member_id0[i] = members[i].agent_id_start;
  return BK_OK;
}

// The members' records into the env: `ds` = the (shared) row every unit's kernels and the list rebuilds read, `table` =
// the per-unit table of bk_set_agents_per_book (empty: the uniform set).  Replaces whatever agents were installed.
static int install_members(bk_env* env, const std::vector<MixedDesc>& ds, uint32_t n_members, const uint32_t* assets,
                           const uint32_t* fixed_a, std::vector<MixedDesc> table) {
  DevBuf<MixedDesc> dt;
  if (!table.empty()) {
    HIPCHK(dt.alloc(table.size()));
    HIPCHK(hipMemcpy(dt.p, table.data(), table.size() * sizeof(MixedDesc), hipMemcpyHostToDevice));
  }
  uint32_t fixed = fixed_a[0];
  HIPCHK(env->mixed_descs.alloc(n_members));
  HIPCHK(hipMemcpy(env->mixed_descs.p, ds.data(), ds.size() * sizeof(MixedDesc), hipMemcpyHostToDevice));
  env->n_mixed = n_members;
  env->n_fixed = fixed;
  env->member_type.resize(n_members);
  env->member_n.resize(n_members);
  for (uint32_t i = 0; i < n_members; ++i) env->member_type[i] = ds[i].type, env->member_n[i] = ds[i].n;
  env->member_lists_stale = true;  // (a new AgentSet: empty lists, no momentum state; bk_update_members)
  env->agent_installs += 1;
  env->wl_valid = false;
  for (uint32_t i = 0; i < MAX_INGRESS_MEMBERS; ++i) env->member_asset[i] = (assets && i < n_members) ? assets[i] : 0u;
  for (uint32_t as = 0; as < MAX_ASSETS; ++as) env->n_fixed_a[as] = fixed_a[as];
  env->ml_valid = false;
  env->groups.clear();
  env->table.clear();
  (void)env->dtable.alloc(0);
  env->n_agents_total = 0;
  env->dmtable.swap(dt);  // (the previous table, if any, is freed with `dt`)
  env->mtable.swap(table);
  env->agents_hash = env->mtable.empty() ? mixed_hash(env->member_asset, ds.data(), ds.size(), n_members)
                                         : mixed_hash(env->member_asset, env->mtable.data(), env->mtable.size(), n_members);
  return BK_OK;
}

// Noise / Momentum (and RandomAgents) members whose parameters differ per unit (book, or market when assets > 1): every
// row is checked and preprocessed as set_agents_impl does one (agent_table.hpp make_mixed_table); unit 0's row is the
// env's shared row (the members' kinds, sizes and assets, which every unit shares), the table goes to the device, where
// the PB forms of k_run_mixed / k_agents_mixed / k_agents_mixed_wave / k_agents_mixed_lanes read unit u's row.  An
// all-RandomAgents table is bk_set_random_agents_per_book's.  Nothing changes on a failure.
int bk_set_agents_per_book(bk_env* env, uint32_t n_members, const bk_agent_desc* members, const uint32_t* assets) {
  if (!env || (!members && n_members)) return fail(BK_INVALID_ARGUMENT, "null argument");
  if (n_members == 0) return fail(BK_INVALID_ARGUMENT, "a per-unit table needs at least one member");
  if (env->M > 1 && !assets) return fail(BK_INVALID_ARGUMENT, "markets (assets > 1) need the members' assets");
  for (uint32_t i = 0; assets && i < n_members; ++i)
    if (assets[i] >= env->M) return fail(BK_INVALID_ARGUMENT, "member asset index out of range");
  const uint32_t n_units = env->cfg.n_books / env->M;
  const size_t n = static_cast<size_t>(n_units) * n_members;
  bool all_random = true;
  for (size_t k = 0; k < n; ++k) all_random = all_random && members[k].type == BK_AGENT_RANDOM;
  if (all_random) {
    std::vector<bk_random_agents> g(n);
    for (size_t k = 0; k < n; ++k)
      g[k] = bk_random_agents{members[k].n_agents, members[k].tick_lo, members[k].tick_hi, members[k].vol_lo,
                              members[k].vol_hi, members[k].tick_size, members[k].activity_rate};
    return bk_set_random_agents_per_book(env, n_members, g.data(), assets);
  }
  if (int rc = member_count_ok(env, n_members)) return rc;
  if (env->agent_log)
    return fail(BK_INVALID_ARGUMENT, "the agents' order log (bk_set_agent_order_log) records RandomAgents only: "
                                     "a set with Noise / Momentum members cannot be installed on a logging env");
  std::vector<MixedDesc> t;
  uint32_t fixed_a[MAX_ASSETS];
  std::string msg;
  if (int rc = make_mixed_table(members, n_units, n_members, assets, env->M, env->asset_tick, env->cfg.max_live_orders, t,
                                fixed_a, &msg))
    return fail(rc, msg);
  if (int rc = use_device(env)) return rc;
  const std::vector<MixedDesc> row0(t.begin(), t.begin() + n_members);
  if (int rc = install_members(env, row0, n_members, assets, fixed_a, std::move(t))) return rc;
  env->member_id0.resize(n);
  for (size_t k = 0; k < n; ++k) env->member_id0[k] = members[k].agent_id_start;
  // ... and on the device for bk_retune_agents*, which compare a row's agent_id_start with them (member_id0_dev is the
  // ingress path's own copy, made only at a device-ingress env's first update)
  HIPCHK(env->retune_id0.alloc(n));
  HIPCHK(hipMemcpy(env->retune_id0.p, env->member_id0.data(), n * 4, hipMemcpyHostToDevice));
  return BK_OK;
}

// ------------------------------------------------------------------ retune: the installed per-unit table, in place
// bk_retune_*: the parameter records of the masked units of the installed per-unit table are replaced on the device
// (retune.hpp).  Books, RNG states, held ids, member lists, momentum state, the stale marks,
// agent_installs and agents_hash stay: the hash goes on naming the install, whose shape a retune cannot change, so
// checkpoints and snapshot slots taken on either side of a retune stay usable - they hold no parameters.  The host's
// table / mtable keep the INSTALLED records: they are read for emptiness, for the hash and for the fixed fields only.
static int retune_ok(bk_env* env, const void* rows, bool members, uint32_t width) {
  if (!env || !rows) return fail(BK_INVALID_ARGUMENT, "null argument");
  if (members) {
    if (env->mtable.empty())
      return fail(BK_INVALID_ARGUMENT, env->n_mixed ? "a retune rewrites the per-unit table: install the members with "
                                                      "bk_set_agents_per_book (a table of identical rows costs nothing)"
                                                    : "no per-unit table of members installed (bk_set_agents_per_book; an "
                                                      "all-RandomAgents table is bk_retune_random_agents')");
    if (width != env->n_mixed) return fail(BK_INVALID_ARGUMENT, "n_members differs from the installed table's");
  } else {
    if (env->table.empty())
      return fail(BK_INVALID_ARGUMENT, !env->groups.empty() ? "a retune rewrites the per-unit table: install the groups with "
                                                              "bk_set_random_agents_per_book (a table of identical rows costs "
                                                              "nothing)"
                                                            : "no per-unit table of RandomAgents groups installed "
                                                              "(bk_set_random_agents_per_book)");
    if (width != env->groups.size()) return fail(BK_INVALID_ARGUMENT, "n_groups differs from the installed table's");
  }
  return BK_OK;
}

// the one launch; the counter is made at the first call, everything else at the install
static int launch_retune(bk_env* env, bool members, uint32_t width, const void* rows_dev, const uint8_t* mask_dev,
                         uint32_t* status_dev) {
  if (reinterpret_cast<uintptr_t>(rows_dev) & (members ? 7u : 3u))
    return fail(BK_INVALID_ARGUMENT, members ? "rows must be 8-byte aligned" : "rows must be 4-byte aligned");
  if (reinterpret_cast<uintptr_t>(status_dev) & 3u) return fail(BK_INVALID_ARGUMENT, "status must be 4-byte aligned");
  if (int rc = use_device(env)) return rc;
  if (!env->retune_count.p) {
    HIPCHK(env->retune_count.alloc(1));
    HIPCHK(hipMemsetAsync(env->retune_count.p, 0, 8, env->stream));
  }
  retune::Args g{};
  g.rows = rows_dev;
  g.table = members ? static_cast<void*>(env->dmtable.p) : static_cast<void*>(env->dtable.p);
  g.mask = mask_dev;
  g.status = status_dev;
  g.rejected = env->retune_count.p;
  g.id_start = env->retune_id0.p;
  g.n_units = env->cfg.n_books / env->M;
  g.width = width;
  for (int i = 0; i < MAX_ASSETS; ++i) g.asset_tick[i] = env->asset_tick[i] ? env->asset_tick[i] : env->asset_tick[0];
  for (uint32_t j = 0; j < width && members; ++j) g.member_assets |= static_cast<uint64_t>(env->member_asset[j]) << (8u * j);
  const dim3 grid((g.n_units + retune::UNITS_PER_BLOCK - 1) / retune::UNITS_PER_BLOCK), block(64 * retune::WAVES);
  if (members)
    hipLaunchKernelGGL(retune::k_members, grid, block, 0, env->stream, g);
  else
    hipLaunchKernelGGL(retune::k_groups, grid, block, 0, env->stream, g);
  HIPCHK(hipGetLastError());
  return BK_OK;
}

// Hold NO host synchronisation and, after the first call, no allocation: one launch on the env's stream.
int bk_retune_random_agents_device(bk_env* env, uint32_t n_groups, const bk_random_agents* rows_dev, const uint8_t* mask_dev,
                                   uint32_t* status_dev) {
  if (int rc = retune_ok(env, rows_dev, false, n_groups)) return rc;
  return launch_retune(env, false, n_groups, rows_dev, mask_dev, status_dev);
}

int bk_retune_agents_device(bk_env* env, uint32_t n_members, const bk_agent_desc* rows_dev, const uint8_t* mask_dev,
                            uint32_t* status_dev) {
  if (int rc = retune_ok(env, rows_dev, true, n_members)) return rc;
  return launch_retune(env, true, n_members, rows_dev, mask_dev, status_dev);
}

// the host forms' rows (and mask) through the env's pinned and device staging into the same kernel
static int retune_from_host(bk_env* env, bool members, uint32_t width, const void* rows, size_t row_bytes, const uint8_t* mask) {
  if (int rc = use_device(env)) return rc;
  const size_t n_units = env->cfg.n_books / env->M;
  const size_t rows_bytes = (n_units * width * row_bytes + 15u) & ~size_t(15);
  const size_t bytes = rows_bytes + n_units;
  HostStage& st = env->retune_stage;
  if (int rc = st.reserve(bytes, env->stream, true)) return rc;  // (an earlier retune may still read the staging it replaces)
  std::memcpy(st.pin, rows, n_units * width * row_bytes);  // the caller's table may be reused on return
  if (mask) std::memcpy(st.pin + rows_bytes, mask, n_units);
  if (int rc = st.upload(mask ? bytes : rows_bytes, env->stream)) return rc;
  return launch_retune(env, members, width, st.dev.p, mask ? st.dev.p + rows_bytes : nullptr, nullptr);
}

// The masked units are checked on the host first, with the installs' row builders: on the first failure nothing changes.
int bk_retune_random_agents(bk_env* env, uint32_t n_groups, const bk_random_agents* rows, const uint8_t* mask) {
  if (int rc = retune_ok(env, rows, false, n_groups)) return rc;
  const uint32_t n_units = env->cfg.n_books / env->M;
  uint32_t assets[MAX_GROUPS];
  for (uint32_t g = 0; g < n_groups; ++g) assets[g] = env->groups[g].asset;
  std::vector<Group> rec(n_groups);
  std::string msg;
  for (uint32_t u = 0; u < n_units; ++u) {
    if (mask && !mask[u]) continue;
    const std::string where = "unit " + std::to_string(u) + ", ";
    uint64_t total = 0;
    const size_t row = static_cast<size_t>(u) * n_groups;
    if (int rc = make_groups(rows + row, n_groups, assets, env->M, env->asset_tick, rec.data(), &total, &msg, where))
      return fail(rc, msg);
    for (uint32_t g = 0; g < n_groups; ++g)
      if (int rc = agent_rows::group_fixed_ok(rec[g], env->table[row + g]))
        return fail(rc, where + "group " + std::to_string(g) + ": n_agents differs from the installed value (a retune keeps the pool layout)");
  }
  return retune_from_host(env, false, n_groups, rows, sizeof(bk_random_agents), mask);
}

int bk_retune_agents(bk_env* env, uint32_t n_members, const bk_agent_desc* rows, const uint8_t* mask) {
  if (int rc = retune_ok(env, rows, true, n_members)) return rc;
  const uint32_t n_units = env->cfg.n_books / env->M;
  std::vector<MixedDesc> rec(n_members);
  uint32_t fixed_a[MAX_ASSETS];
  std::string msg;
  for (uint32_t u = 0; u < n_units; ++u) {
    if (mask && !mask[u]) continue;
    const std::string where = "unit " + std::to_string(u) + ", ";
    const size_t row = static_cast<size_t>(u) * n_members;
    if (int rc = make_mixed_descs(rows + row, n_members, env->member_asset, env->asset_tick, rec.data(), fixed_a, &msg, where))
      return fail(rc, msg);
    for (uint32_t i = 0; i < n_members; ++i)
      if (int rc = agent_rows::mixed_fixed_ok(rec[i], env->mtable[row + i], rows[row + i].agent_id_start, env->member_id0[row + i]))
        return fail(rc, where + "member " + std::to_string(i) +
                            ": type, n_agents or agent_id_start differs from the installed value (a retune keeps the members' kinds, "
                            "pool layout and trader ids)");
  }
  return retune_from_host(env, true, n_members, rows, sizeof(bk_agent_desc), mask);
}

int bk_retune_rejected(bk_env* env, uint64_t* out) {
  if (!env || !out) return fail(BK_INVALID_ARGUMENT, "null argument");
  *out = 0;
  if (!env->retune_count.p) return BK_OK;  // (no retune yet)
  if (int rc = use_device(env)) return rc;
  HIPCHK(hipStreamSynchronize(env->stream));
  unsigned long long n = 0;
  HIPCHK(hipMemcpy(&n, env->retune_count.p, 8, hipMemcpyDeviceToHost));
  *out = n;
  return BK_OK;
}

// books one residency round of the fused wave kernel holds (the auto rule's `wave` limit): asked of the runtime once
static void query_fused_resident(bk_env* env) {
  if (hipSetDevice(env->cfg.device) != hipSuccess) return;
  int blocks = 0, cus = 0;
  hipError_t e = by_R(env->R, [&](auto r) {
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, k_run_wave<decltype(r)::value>, 512, 0);
  });
  if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, env->cfg.device);
  if (e == hipSuccess && blocks > 0 && cus > 0) env->fused_resident = static_cast<uint32_t>(blocks) * 8u * static_cast<uint32_t>(cus);
  (void)hipGetLastError();
  if (getenv("BOURSE_AMD_VERBOSE"))
    fprintf(stderr, "bourse_amd: k_run_wave<%d>: %d workgroups per CU x %d CUs -> one round holds %u books\n", env->R, blocks, cus,
            env->fused_resident);
}

// THE pipeline choice (pipeline_plan.hpp): bk_run launches from it, bk_get_pipeline reports it
static Plan env_plan(bk_env* env) {
  PlanInput in{env->R, env->cfg.n_books, env->M, !env->groups.empty(), env->n_mixed, env->pipeline, env->n_parts, env->wave_parts,
               env->min_part, env->fused_resident, env->stagger_us, env->warming, env->step_decode, env->agent_log,
               !env->table.empty(), !env->mtable.empty()};
  if (!in.fused_resident && random_books(in)) {
    query_fused_resident(env);
    in.fused_resident = env->fused_resident;
  }
  return make_plan(in);
}

int bk_run(bk_env* env, uint64_t n_steps) {
  if (!env) return fail(BK_INVALID_ARGUMENT, "null env");
  if (n_steps == 0) return BK_OK;
  const Plan pl = env_plan(env);
  if (n_steps > 0xFFFFFFFFull) return fail(BK_INVALID_ARGUMENT, "n_steps too large for one launch");
  if (int rc = use_device(env)) return rc;
  if (env->device_ingress) return fail(BK_INVALID_ARGUMENT, "bk_run cannot be mixed with submitted instructions on the same env");
  for (const BookHost& bh : env->books)
    if (!bh.queue.empty() || !bh.orders.empty())
      return fail(BK_INVALID_ARGUMENT, "bk_run cannot be mixed with host-driven orders on the same env");
  {  // stamps: every agent places at most one order per step.  A run longer than the room holds goes in pieces.
    uint64_t per_step = env->n_agents_total;
    if (env->n_mixed) {
      per_step = 0;
      for (uint32_t n : env->member_n) per_step += n;
    }
    if (per_step && env->stamp_room.needs_compaction(n_steps * per_step)) {
      const uint64_t most = std::max<uint64_t>(1, env->stamp_room.after_compaction(static_cast<uint32_t>(env->R) * 64u) / per_step);
      if (n_steps > most) {
        for (uint64_t left = n_steps; left;) {
          const uint64_t c = std::min(left, most);
          if (int rc = bk_run(env, c)) return rc;
          left -= c;
        }
        return BK_OK;
      }
    }
    if (int rc = reserve_stamps(env, n_steps * per_step)) return rc;
  }
  DevArgs a = env->args();
  if (a.n_groups == 0) {  // no agents: plain steps
    a.groups[0] = Group{};
    a.n_agents_total = 0;
  }
  const uint32_t ns = static_cast<uint32_t>(n_steps);
  if (env->n_mixed || a.n_groups) env->device_flow = true;
  // Which kernels (pipeline_plan.hpp - the rule itself is documented there and in DESIGN.md 2.1):
  //  * the fused kernels keep a book in registers across all steps of the launch but run the RNG-serial phases on the
  //    scalar unit of ONE wave per book; the split forms move them to one lane per book (>= 64 books per wave to pay off)
  //    or decode the stream wave-parallel, in front of the lean event kernel, the batch cut in parts that overlap;
  //  * markets always take a split form: the market's RNG-serial phase is one lane, its books are M waves;
  //  * the lane-per-book members' update keeps a filled order's pool slot reserved until its member's next update, so a
  //    pool the wave-per-book kernels just fit can overflow there (flagged): it is only ever taken on request (mode 2) or
  //    for markets, where the other kernels do not exist - nothing of the library's choosing is left to guard.
  const int rc = by_R(env->R, [&](auto r) -> int {
    constexpr int R = decltype(r)::value;
    WaveArgs wva{};
    if (int rc = prepare_launch<R>(env, pl, a, &wva)) return rc;
    return is_split(pl.kind) ? launch_split<R>(env, pl, a, wva, env->steps_done, ns)
                             : launch_fused<R>(env, pl, a, wva, env->steps_done, ns);
  });
  if (rc != BK_OK) return rc;
  env->steps_done += n_steps;
  if (env->agent_log) env->ingest_epoch += 1;  // the agents created and changed orders: the readers mirror again
  return BK_OK;
}

int bk_set_agent_order_log(bk_env* env, int on) {
  if (!env) return fail(BK_INVALID_ARGUMENT, "null env");
  if (!on) {
    if (env->agent_log) return fail(BK_INVALID_ARGUMENT, "the agents' order log cannot be switched off once it is on");
    return BK_OK;
  }
  if (env->agent_log) return BK_OK;
  if (env->cfg.max_orders == 0)
    return fail(BK_INVALID_ARGUMENT, "the agents' order log needs max_orders > 0 (its capacity per book)");
  if (env->steps_done || env->device_flow)
    return fail(BK_INVALID_ARGUMENT, "switch the agents' order log on before the env's first bk_run: it could not hold "
                                     "the orders created before");
  if (env->device_ingress)
    return fail(BK_INVALID_ARGUMENT, "this env takes its instructions from device memory (bk_device_ingress_enable), which "
                                     "logs its orders already");
  if (env->n_mixed)
    return fail(BK_INVALID_ARGUMENT, "the agents' order log records RandomAgents only: this env has an AgentSet with "
                                     "Noise / Momentum members");
  for (const BookHost& bh : env->books)
    if (!bh.orders.empty() || !bh.queue.empty())
      return fail(BK_INVALID_ARGUMENT, "the agents' order log is for bk_run's on-device agents: this env holds host-driven orders");
  if (int rc = use_device(env)) return rc;
  HIPCHK(env->dorders.alloc(static_cast<size_t>(env->cfg.n_books) * env->cfg.max_orders * 2));
  env->agent_log = true;
  env->ingest_epoch += 1;
  return BK_OK;
}

// Warm-up without side effects: n_steps of THIS env's own kernels (same agents, same pipeline, same streams) on its own
// books, then everything put back - state blocks, level-2 records, step counter; the scratch steps write no history slot
// and no trade record.  Why it exists: an MI355X drops its clocks within milliseconds of idling and needs ~15 ms of load
// to come back, and the first launch of a pipeline also pays one-off set-up (the parts' streams, dynamic-LDS
// attributes, the decode's lane-state cache); a latency-sensitive caller - a short bk_run after host-side work - calls
// this first.  Asynchronous on the env's stream like bk_run (two device-to-device copies around the steps).
int bk_warm(bk_env* env, uint64_t n_steps) {
  if (!env) return fail(BK_INVALID_ARGUMENT, "null env");
  if (n_steps == 0) return BK_OK;
  if (int rc = use_device(env)) return rc;
  const size_t sb = static_cast<size_t>(env->cfg.n_books) * env->stride, lb = static_cast<size_t>(env->cfg.n_books) * env->W;
  if (!env->warm_snap.p) HIPCHK(env->warm_snap.alloc(sb + lb));
  HIPCHK(hipMemcpyAsync(env->warm_snap.p, env->state.p, sb * 4, hipMemcpyDeviceToDevice, env->stream));
  HIPCHK(hipMemcpyAsync(env->warm_snap.p + sb, env->l2_last.p, lb * 4, hipMemcpyDeviceToDevice, env->stream));
  const uint64_t steps0 = env->steps_done;
  const bool flow0 = env->device_flow;
  const uint64_t stamps0 = env->stamp_room.bound;  // (the books come back as they are now, their H_SEQ with them)
  env->warming = true;
  const int rc = bk_run(env, n_steps);
  env->warming = false;
  env->steps_done = steps0;
  env->device_flow = flow0;
  env->stamp_room.bound = stamps0;
  env->wl_valid = false;  // the wave-per-book lists described the scratch steps' pools
  env->ml_valid = false;  // the members' lists described the scratch steps' pool
  // put the books back WHATEVER bk_run returned: a launch that failed half-way (an event record / wait between two kernel
  // launches) has already stepped some parts, and the step counter above is rolled back either way.  bk_run's own error
  // (and its message) wins over one of the restore copies.
  std::string run_err = rc != BK_OK ? g_err : std::string();
  if (rc != BK_OK)  // (a failed multi-part launch never reached its join: the parts' streams may still be stepping)
    for (int i = 0; i < bk_env::MAX_PARTS; ++i)
      if (env->part_stream[i]) (void)hipStreamSynchronize(env->part_stream[i]);
  const hipError_t e1 = hipMemcpyAsync(env->state.p, env->warm_snap.p, sb * 4, hipMemcpyDeviceToDevice, env->stream);
  const hipError_t e2 = hipMemcpyAsync(env->l2_last.p, env->warm_snap.p + sb, lb * 4, hipMemcpyDeviceToDevice, env->stream);
  if (rc != BK_OK) return fail(rc, run_err);
  HIPCHK(e1);
  HIPCHK(e2);
  return BK_OK;
}

// ------------------------------------------------------------------ readers
uint32_t bk_l2_width(const bk_env* env) { return env ? env->W : 0; }

int bk_level2(bk_env* env, uint32_t first_book, uint32_t n_books, uint32_t* out) {
  if (!env || !out) return fail(BK_INVALID_ARGUMENT, "null argument");
  if (int rc = book_range_ok(env, first_book, n_books)) return rc;
  if (int rc = use_device(env)) return rc;
  HIPCHK(hipStreamSynchronize(env->stream));
  HIPCHK(hipMemcpy(out, env->l2_last.p + static_cast<size_t>(first_book) * env->W,
                   static_cast<size_t>(n_books) * env->W * 4, hipMemcpyDeviceToHost));
  return BK_OK;
}

// first retained step of the history ring: the last history_capacity steps, or since the last bk_clear_history()
static uint64_t hist_first(const bk_env* env) {
  return ring::first_retained(env->steps_done, env->hist_base, env->cfg.history_capacity);
}

int bk_history_len(bk_env* env, uint64_t* first_step, uint64_t* n_steps) {
  if (!env) return fail(BK_INVALID_ARGUMENT, "null env");
  const uint64_t f = hist_first(env);
  if (first_step) *first_step = f;
  if (n_steps) *n_steps = env->cfg.history_capacity ? env->steps_done - f : 0;
  return BK_OK;
}

// copy steps [first_step, first_step + n_steps) of the ring to `out` (handles the wrap); async if cs != nullptr
static int hist_copy(bk_env* env, uint64_t first_step, uint64_t n_steps, uint32_t first_book, uint32_t n_books,
                     uint32_t* out, hipStream_t cs, bool async) {
  if (!env || !out) return fail(BK_INVALID_ARGUMENT, "null argument");
  if (!env->cfg.history_capacity || first_step < hist_first(env) || first_step > env->steps_done ||
      n_steps > env->steps_done - first_step)
    return fail(BK_INVALID_ARGUMENT, "step range not retained (history is a ring of history_capacity steps)");
  if (int rc = book_range_ok(env, first_book, n_books)) return rc;
  if (int rc = use_device(env)) return rc;
  const size_t W = env->W, B = env->cfg.n_books, cap = env->cfg.history_capacity;
  const size_t row = static_cast<size_t>(n_books) * W * 4;
  uint64_t done = 0;
  while (done < n_steps) {
    const uint64_t slot = (first_step + done) % cap;
    const uint64_t n = std::min<uint64_t>(n_steps - done, cap - slot);
    const uint32_t* src = env->hist.p + (slot * B + first_book) * W;
    uint32_t* dst = out + done * static_cast<size_t>(n_books) * W;
    if (async && n_books == B)  // whole rows are contiguous: one linear copy
      HIPCHK(hipMemcpyAsync(dst, src, row * n, hipMemcpyDeviceToHost, cs));
    else if (async)
      HIPCHK(hipMemcpy2DAsync(dst, row, src, B * W * 4, row, n, hipMemcpyDeviceToHost, cs));
    else
      HIPCHK(hipMemcpy2D(dst, row, src, B * W * 4, row, n, hipMemcpyDeviceToHost));
    done += n;
  }
  return BK_OK;
}

int bk_history(bk_env* env, uint64_t first_step, uint64_t n_steps, uint32_t first_book, uint32_t n_books,
               uint32_t* out) {
  if (!env) return fail(BK_INVALID_ARGUMENT, "null env");
  if (int rc = use_device(env)) return rc;
  HIPCHK(hipStreamSynchronize(env->stream));
  return hist_copy(env, first_step, n_steps, first_book, n_books, out, nullptr, false);
}

// Egress overlapped with stepping: the copy is ordered after the work queued on the env's stream so far and runs on
// `copy_stream`; the caller keeps stepping and must not let the ring wrap onto the steps being copied
// (history_capacity >= 2 x chunk), then waits with bk_stream_sync(copy_stream).  `out` should be pinned
// (bk_pinned_alloc) for the copy to be truly asynchronous.
int bk_history_copy_async(bk_env* env, uint64_t first_step, uint64_t n_steps, uint32_t first_book, uint32_t n_books,
                          uint32_t* out, void* copy_stream) {
  if (!env || !copy_stream) return fail(BK_INVALID_ARGUMENT, "null argument");
  if (int rc = use_device(env)) return rc;
  hipStream_t cs = static_cast<hipStream_t>(copy_stream);
  if (int rc = order_after(cs, env->stream)) return rc;
  return hist_copy(env, first_step, n_steps, first_book, n_books, out, cs, true);
}

int bk_stream_create(void** out) {
  if (!out) return fail(BK_INVALID_ARGUMENT, "null argument");
  hipStream_t s;
  HIPCHK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  *out = s;
  return BK_OK;
}
int bk_stream_sync(void* stream) {
  HIPCHK(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
  return BK_OK;
}
int bk_stream_destroy(void* stream) {
  HIPCHK(hipStreamDestroy(static_cast<hipStream_t>(stream)));
  return BK_OK;
}
int bk_pinned_alloc(uint64_t nbytes, void** out) {
  if (!out) return fail(BK_INVALID_ARGUMENT, "null argument");
  HIPCHK(hipHostMalloc(out, nbytes, hipHostMallocDefault));
  return BK_OK;
}
int bk_pinned_free(void* p) {
  HIPCHK(hipHostFree(p));
  return BK_OK;
}

int bk_clear_history(bk_env* env) {
  if (!env) return fail(BK_INVALID_ARGUMENT, "null env");
  env->hist_base = env->steps_done;
  return BK_OK;
}

// ------------------------------------------------------------------ the tables folded from the level-2 history ring
// No counterpart in the reference.  Per book: series_rows[n_books] rows of 24 u64 words (series.hpp),
// lag_rows[n_books][n_lags] rows of 10 u64 words and lag_carry[n_books][n_lags + 1] (lags.hpp, 2.24), and
// bin_rows[n_books][n_spans + 2][n_bins] u64 counts and bins_carry[n_books][bins_kmax] (bins.hpp, 2.25); per market:
// cross_rows[n_markets][n_spans][A][A] rows of 8 u64 words and cross_carry[n_markets][A][2 * cross_hmax] (cross.hpp, 2.29) -
// each folded by its k_fold on the env's stream when its bk_*_fold, a masked clear or a reset asks.  The eight launches
// first, then the one contract over HistTable (2.21a).
static ring::Masked masked_books(const bk_env* env, const uint8_t* mask_dev, uint32_t M) { return {mask_dev, M, env->cfg.n_books}; }

static void launch_series_fold(bk_env* env, const ring::Span& span) {
  series::FoldArgs g{};
  g.ring = span;
  g.rows = env->series_rows.p;
  launch_wave_per_book(env, series::k_fold, series::FOLD_WAVES, span.n_books, g);
  if (env->depth_rows.p) {  // the ladder's companion table: the same span, right behind
    depth::FoldArgs d{};
    d.ring = span;
    d.L = env->cfg.levels;
    d.rows = env->depth_rows.p;
    d.carry = env->depth_carry.p;
    launch_wave_per_book(env, depth::k_fold, depth::FOLD_WAVES, span.n_books, d);
  }
  if (env->candle_rows.p) {  // the bars' companion table: the same span; its first step is the series' cursor, not yet advanced
    const uint64_t seen = env->tables[T_SERIES].seen;
    candles::FoldArgs c{};
    c.ring = span;
    c.W = env->candle_width;
    c.N = env->candle_n;
    const candles::Pass at = candles::first_pass(seen, c.W, c.N);
    c.bar = at.bar, c.phase = at.phase, c.slot = at.slot;
    c.last_bar = candles::bar_of(seen + span.n - 1u, c.W);
    c.rows = env->candle_rows.p;
    c.carry = env->candle_carry.p;
    launch_wave_per_book(env, candles::k_fold, candles::FOLD_WAVES, span.n_books, c);
  }
}

static void launch_series_clear(bk_env* env, const uint8_t* mask_dev, uint32_t M, bool carry_only) {
  series::ClearArgs g{};
  g.books = masked_books(env, mask_dev, M);
  g.carry_only = carry_only ? 1u : 0u;
  g.rows = env->series_rows.p;
  launch_wave_per_book(env, series::k_clear, series::FOLD_WAVES, g.books.n_books, g);
  if (env->depth_rows.p) {
    depth::ClearArgs d{};
    d.books = g.books;
    d.L = env->cfg.levels;
    d.carry_only = g.carry_only;
    d.rows = env->depth_rows.p;
    d.carry = env->depth_carry.p;
    launch_wave_per_book(env, depth::k_clear, depth::FOLD_WAVES, d.books.n_books, d);
  }
  if (env->candle_rows.p) {
    candles::ClearArgs c{};
    c.books = g.books;
    c.N = env->candle_n;
    c.carry_only = g.carry_only;
    c.rows = env->candle_rows.p;
    c.carry = env->candle_carry.p;
    launch_wave_per_book(env, candles::k_clear, candles::FOLD_WAVES, c.books.n_books, c);
  }
}

static void launch_lags_fold(bk_env* env, const ring::Span& span) {
  lags::FoldArgs g{};
  g.ring = span;
  g.K = env->n_lags;
  g.rows = env->lag_rows.p;
  g.carry = env->lag_carry.p;
  launch_wave_per_book(env, lags::k_fold, lags::FOLD_WAVES, span.n_books, g);
}

static void launch_lags_clear(bk_env* env, const uint8_t* mask_dev, uint32_t M, bool carry_only) {
  lags::ClearArgs g{};
  g.books = masked_books(env, mask_dev, M);
  g.K = env->n_lags;
  g.carry_only = carry_only ? 1u : 0u;
  g.rows = env->lag_rows.p;
  g.carry = env->lag_carry.p;
  launch_wave_per_book(env, lags::k_clear, lags::FOLD_WAVES, g.books.n_books, g);
}

static void launch_bins_fold(bk_env* env, const ring::Span& span) {
  const bk_bins_config& c = env->bins_cfg;
  bins::FoldArgs g{};
  g.ring = span;
  g.B = c.n_bins;
  g.S = c.n_spans;
  g.Kmax = env->bins_kmax;
  g.spans = c.spans[0] | c.spans[1] << 8 | c.spans[2] << 16 | c.spans[3] << 24;
  g.ret_width = c.ret_width, g.spread_width = c.spread_width, g.vol_width = c.vol_width;
  g.rows = env->bin_rows.p;
  g.carry = env->bins_carry.p;
  // (a launch of its own: the wave-per-book helper passes no dynamic LDS)
  hipLaunchKernelGGL(bins::k_fold, dim3((span.n_books + bins::FOLD_WAVES - 1) / bins::FOLD_WAVES), dim3(64 * bins::FOLD_WAVES),
                     bins::fold_lds_bytes(g.S, g.B), env->stream, g);
}

static void launch_bins_clear(bk_env* env, const uint8_t* mask_dev, uint32_t M, bool carry_only) {
  bins::ClearArgs g{};
  g.books = masked_books(env, mask_dev, M);
  g.CB = (env->bins_cfg.n_spans + 2u) * env->bins_cfg.n_bins;
  g.Kmax = env->bins_kmax;
  g.carry_only = carry_only ? 1u : 0u;
  g.rows = env->bin_rows.p;
  g.carry = env->bins_carry.p;
  launch_wave_per_book(env, bins::k_clear, bins::FOLD_WAVES, g.books.n_books, g);
}

static void launch_cross_fold(bk_env* env, const ring::Span& span) {
  const bk_cross_config& c = env->cross_cfg;
  cross::FoldArgs g{};
  g.ring = span;
  g.A = env->M;
  g.S = c.n_spans;
  g.Hmax = env->cross_hmax;
  g.spans = c.spans[0] | c.spans[1] << 8 | c.spans[2] << 16 | c.spans[3] << 24;
  g.rows = env->cross_rows.p;
  g.carry = env->cross_carry.p;
  // one wave per MARKET (a launch of its own: the wave-per-book helper passes no dynamic LDS)
  const uint32_t markets = span.n_books / env->M;
  hipLaunchKernelGGL(cross::k_fold, dim3((markets + cross::FOLD_WAVES - 1) / cross::FOLD_WAVES), dim3(64 * cross::FOLD_WAVES),
                     cross::fold_lds_bytes(g.A, g.Hmax), env->stream, g);
}

// (mask_dev holds one byte per MARKET from either caller - a reset's M is env->M, and so is the table's own clear_M)
static void launch_cross_clear(bk_env* env, const uint8_t* mask_dev, uint32_t, bool carry_only) {
  cross::ClearArgs g{};
  g.markets = ring::Masked{mask_dev, 1u, env->cfg.n_books / env->M};
  g.U = cross::units(env->cross_cfg.n_spans, env->M);
  g.carry_words = env->M * cross::carry_words(env->cross_hmax);
  g.carry_only = carry_only ? 1u : 0u;
  g.rows = env->cross_rows.p;
  g.carry = env->cross_carry.p;
  launch_wave_per_book(env, cross::k_clear, cross::FOLD_WAVES, g.markets.n_books, g);
}

// a step of [seen, steps_done) that the ring no longer retains refuses; nothing is launched or changed
// (`at`: where the cursor's answer goes for a caller that folds next)
static int table_lost_check(bk_env* env, const HistTable& t, ring::Cursor* at = nullptr) {
  const ring::Cursor c = ring::cursor(t.seen, env->steps_done, env->hist_base, env->cfg.history_capacity);
  if (at) *at = c;
  if (c.kind != ring::CURSOR_LOST) return BK_OK;
  char msg[224];
  std::snprintf(msg, sizeof msg,
                "%llu step(s) of the %s were lost: steps [%llu, %llu) are no longer retained by the history ring "
                "(history_capacity steps, or since bk_clear_history) - fold at least every history_capacity steps; "
                "bk_%s_clear(env, NULL) starts again",
                static_cast<unsigned long long>(c.first - t.seen), t.noun, static_cast<unsigned long long>(t.seen),
                static_cast<unsigned long long>(c.first), t.prefix);
  return fail(BK_INVALID_ARGUMENT, msg);
}

// fold what is outstanding (nothing: no launch); lost steps refuse, the table, its carry and its cursor unchanged
static int table_fold_outstanding(bk_env* env, HistTable& t) {
  ring::Cursor c;
  if (int rc = table_lost_check(env, t, &c)) return rc;
  if (c.kind != ring::CURSOR_FOLD) return BK_OK;
  if (int rc = use_device(env)) return rc;
  t.fold(env, ring::Span{env->hist.p, env->cfg.history_capacity, env->cfg.n_books, env->W, c.slot0, c.n});
  HIPCHK(hipGetLastError());
  t.seen = env->steps_done;
  return BK_OK;
}

// the full clear of an enable or a bk_*_clear(env, NULL): every row starts again at this step, lost steps are forgotten
static void table_start_again(bk_env* env, HistTable& t) {
  t.seen = env->steps_done;
  t.clear(env, nullptr, 1, false);
}

// What a bk_*_enable ends with once the table's blocks and shape stand in the env.  A clear that cannot be launched leaves
// the table off: the caller then takes its blocks back out.
static int table_commit_enable(bk_env* env, HistTable& t) {
  t.on = true;
  table_start_again(env, t);
  const hipError_t launched = hipGetLastError();
  if (launched == hipSuccess) return BK_OK;
  t.on = false;
  return fail(BK_HIP_ERROR, std::string("bk_") + t.prefix + "_enable: the clear could not be launched: " + hipGetErrorString(launched));
}

static int read_hdr(bk_env* env, uint32_t book, int first_dw, int n_dw, uint32_t* out) {
  if (int rc = use_device(env)) return rc;
  HIPCHK(hipStreamSynchronize(env->stream));
  HIPCHK(hipMemcpy(out, env->state.p + static_cast<size_t>(book) * env->stride + first_dw, n_dw * 4,
                   hipMemcpyDeviceToHost));
  return BK_OK;
}

int bk_trade_count(bk_env* env, uint32_t book, uint64_t* total, uint64_t* first_retained) {
  if (int rc = check_book(env, book)) return rc;
  uint32_t h[HDR_DW];
  if (int rc = read_hdr(env, book, 0, HDR_DW, h)) return rc;
  if (total) *total = (static_cast<uint64_t>(h[H_TRADES_HI]) << 32) | h[H_TRADES_LO];
  if (first_retained) *first_retained = (static_cast<uint64_t>(h[H_TRADE_BASE_HI]) << 32) | h[H_TRADE_BASE_LO];
  return BK_OK;
}

// one header counter of every book -> host (stream-ordered gather into a contiguous device array, one copy)
int gather_header(bk_env* env, uint32_t word, uint32_t n_words, uint64_t* totals) {
  const uint32_t NB = env->cfg.n_books;
  if (!env->gather_buf.p) HIPCHK(env->gather_buf.alloc(NB));
  hipLaunchKernelGGL(k_gather_header, dim3((NB + 255) / 256), dim3(256), 0, env->stream, env->state.p, env->stride, word, n_words,
                     NB, reinterpret_cast<unsigned long long*>(env->gather_buf.p));
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(totals, env->gather_buf.p, static_cast<size_t>(NB) * 8, hipMemcpyDeviceToHost, env->stream));
  HIPCHK(hipStreamSynchronize(env->stream));
  return BK_OK;
}

int bk_trade_counts(bk_env* env, uint64_t* totals) {
  if (!env || !totals) return fail(BK_INVALID_ARGUMENT, "null argument");
  if (int rc = use_device(env)) return rc;
  return gather_header(env, H_TRADES_LO, 2, totals);
}

int bk_get_trades(bk_env* env, uint32_t book, uint64_t first, uint64_t n, bk_trade* out) {
  if (int rc = check_book(env, book)) return rc;
  uint64_t total = 0, base = 0;
  if (int rc = bk_trade_count(env, book, &total, &base)) return rc;
  if (first < base || first > total || n > total - first) return fail(BK_INVALID_ARGUMENT, "trade range not retained");
  if (n && !out) return fail(BK_INVALID_ARGUMENT, "null argument");
  if (first + n - base > env->cfg.trade_capacity)
    return fail(BK_CAPACITY, "trade records beyond trade_capacity were dropped");
  if (n == 0) return BK_OK;
  std::vector<DevTrade> tmp(n);
  HIPCHK(hipMemcpy(tmp.data(), env->trades.p + static_cast<size_t>(book) * env->cfg.trade_capacity + (first - base),
                   n * sizeof(DevTrade), hipMemcpyDeviceToHost));
  for (uint64_t i = 0; i < n; ++i) {
    const DevTrade& d = tmp[i];
    bk_trade& t = out[i];
    t.t = (static_cast<uint64_t>(d.t_hi) << 32) | d.t_lo;
    t.side_is_bid = d.side_is_bid;
    t.price = d.price;
    t.vol = d.vol;
    t.reserved = 0;
    t.active_order_id = d.active;
    t.passive_order_id = d.passive;
  }
  return BK_OK;
}

// Trade egress at scale (Env::get_trades for every book at once): gather every book's retained
// records into ONE dense device buffer in the bk_trade layout with CSR offsets (book b owns [off[b], off[b+1])), and mark
// them consumed (as bk_clear_trades).  Returns the number of records; fetch them with bk_trades_compact_copy_async.
int bk_trades_compact(bk_env* env, uint64_t* out_total) {
  if (!env) return fail(BK_INVALID_ARGUMENT, "null env");
  if (int rc = use_device(env)) return rc;
  const uint32_t B = env->cfg.n_books;
  if (!env->tr_off.p) HIPCHK(env->tr_off.alloc(static_cast<size_t>(B) + 1));
  hipLaunchKernelGGL(k_trade_scan, dim3(1), dim3(1024), 0, env->stream, env->state.p, env->stride, B,
                     env->cfg.trade_capacity, env->tr_off.p);
  HIPCHK(hipGetLastError());
  unsigned long long total = 0;
  HIPCHK(hipMemcpyAsync(&total, env->tr_off.p + B, 8, hipMemcpyDeviceToHost, env->stream));
  HIPCHK(hipStreamSynchronize(env->stream));
  if (total > env->tr_dense.n) HIPCHK(env->tr_dense.alloc(std::max<size_t>(total + total / 4, 1024)));
  hipLaunchKernelGGL(k_trade_gather, dim3((B + 3) / 4), dim3(256), 0, env->stream, env->state.p, env->stride, B,
                     env->cfg.trade_capacity, env->trades.p, env->tr_off.p, env->tr_dense.p);
  HIPCHK(hipGetLastError());
  env->tr_total = total;
  if (out_total) *out_total = total;
  return BK_OK;
}

// Copy the stream made by the last bk_trades_compact: `records` (tr_total x bk_trade) and `offsets` (n_books + 1) to
// host memory on `copy_stream` (ordered after the compaction; NULL = the env's stream, synchronous).  Pinned
// destinations (bk_pinned_alloc) make the copy overlap the next bk_run.
int bk_trades_compact_copy_async(bk_env* env, bk_trade* records, uint64_t* offsets, void* copy_stream) {
  if (!env || !offsets || (env->tr_total && !records)) return fail(BK_INVALID_ARGUMENT, "null argument");
  if (!env->tr_off.p) return fail(BK_INVALID_ARGUMENT, "call bk_trades_compact first");
  if (int rc = use_device(env)) return rc;
  hipStream_t cs = copy_stream ? static_cast<hipStream_t>(copy_stream) : env->stream;
  if (copy_stream)
    if (int rc = order_after(cs, env->stream)) return rc;
  HIPCHK(hipMemcpyAsync(offsets, env->tr_off.p, (static_cast<size_t>(env->cfg.n_books) + 1) * 8, hipMemcpyDeviceToHost, cs));
  if (env->tr_total)
    HIPCHK(hipMemcpyAsync(records, env->tr_dense.p, env->tr_total * sizeof(bk_trade), hipMemcpyDeviceToHost, cs));
  if (!copy_stream) HIPCHK(hipStreamSynchronize(cs));
  return BK_OK;
}

int bk_clear_trades(bk_env* env) {
  if (!env) return fail(BK_INVALID_ARGUMENT, "null env");
  if (int rc = use_device(env)) return rc;
  const uint32_t B = env->cfg.n_books;
  hipLaunchKernelGGL(k_book_service, dim3((B + 255) / 256), dim3(256), 0, env->stream, env->state.p, env->stride, B, 0,
                     0u);
  HIPCHK(hipGetLastError());
  return BK_OK;
}

// OrderEntry.key of orders [first, first + n) (orderbook.rs:34-39): the price and time the order's priority key was
// last set with.  key = (side, price_key(key_price), key_time); price_key = u32::MAX - price for bids (side.rs:300-302).
int bk_get_order_keys(bk_env* env, uint32_t book, uint64_t first, uint64_t n, uint32_t* key_price,
                      uint64_t* key_time) {
  if (int rc = check_book(env, book)) return rc;
  if (int rc = mirror_orders(env, book)) return rc;
  BookHost& bh = env->books[book];
  if (first > bh.orders.size() || n > bh.orders.size() - first) return fail(BK_INVALID_ARGUMENT, "order range out of bounds");
  if (env->cfg.max_orders == 0) return fail(BK_INVALID_ARGUMENT, "order log disabled (max_orders == 0)");
  if (bh.n_uploaded > env->cfg.max_orders) return fail(BK_CAPACITY, "order log capacity exceeded");
  if (int rc = use_device(env)) return rc;
  if (int rc = refresh_log(env, book)) return rc;
  for (uint64_t i = 0; i < n; ++i) {
    const uint64_t id = first + i;
    if (id < bh.n_uploaded && id < bh.log_cache.size()) {
      const DevOrderLog& d = bh.log_cache[id];
      if (key_price) key_price[i] = d.key_price;
      if (key_time) key_time[i] = (static_cast<uint64_t>(d.key_hi) << 32) | d.key_lo;
    } else {  // created, New event still queued: provisional key (orderbook.rs:388-391)
      if (key_price) key_price[i] = bh.orders[id].price;
      if (key_time) key_time[i] = 0;
    }
  }
  return BK_OK;
}

// Replace one book's state with a snapshot (OrderBook::load_json -> TryFrom<OrderBookState>, orderbook.rs:827-918):
// clock, per-step trade volume, every order ever created (with its key) and every trade.  Active orders go back into
// the pool in key order, the level-2 record is rebuilt from them.  The book must have no queued events.
int bk_load_book(bk_env* env, uint32_t book, uint64_t t, uint32_t trade_vol, uint64_t n_orders, const bk_order* orders,
                 const uint32_t* key_price, const uint64_t* key_time, uint64_t n_trades, const bk_trade* trades) {
  if (int rc = check_book(env, book)) return rc;
  if (env->acct_traders)
    return fail(BK_INVALID_ARGUMENT, "loading a book into an env with trader accounts (bk_accounts_enable) is not supported: "
                                     "its trade records would have no order records to look the traders up in");
  if (env->bars_window)
    return fail(BK_INVALID_ARGUMENT, "loading a book into an env with trade bars (bk_trade_bars_enable) is not supported: "
                                     "its trade records would pass as the next step's");
  if (env->flow_lags)
    return fail(BK_INVALID_ARGUMENT, "loading a book into an env with a flow table (bk_flow_enable) is not supported: the "
                                     "book's trade records would pass as the successors of the replaced book's");
  for (const HistTable* t : {&env->tables[T_SERIES], &env->tables[T_LAGS], &env->tables[T_BINS], &env->cross_table})
    if (t->on)
      return fail(BK_INVALID_ARGUMENT, std::string("loading a book into an env with ") + t->article + t->name + " (bk_" + t->prefix +
                                           "_enable) is not supported: the book's next record would pass as the successor of "
                                           "the replaced book's last");
  if ((n_orders && (!orders || !key_price || !key_time)) || (n_trades && !trades))
    return fail(BK_INVALID_ARGUMENT, "null argument");
  // (the agents' log holds what k_step_batch_log wrote for every id below the book's counter: a loaded book's orders
  // would be mirrored from rows nothing wrote)
  if (env->agent_log)
    return fail(BK_INVALID_ARGUMENT, "loading a book into an env with the agents' order log (bk_set_agent_order_log) is not "
                                     "supported");
  BookHost& bh = env->books[book];
  if (!env->books[book - book % env->M].queue.empty())
    return fail(BK_INVALID_ARGUMENT, "events are queued for this book (market)");
  if (n_orders > env->cfg.max_orders) return fail(BK_CAPACITY, "snapshot holds more orders than max_orders");
  if (n_trades > env->cfg.trade_capacity) return fail(BK_CAPACITY, "snapshot holds more trades than trade_capacity");
  if (n_orders >= 0xFFFFFFFFull) return fail(BK_CAPACITY, "order id space exhausted");
  std::vector<uint64_t> act;  // Active orders, to be ranked by key time (price-time priority within a price)
  for (uint64_t i = 0; i < n_orders; ++i) {
    if (orders[i].order_id != i) return fail(BK_INVALID_ARGUMENT, "orders must be listed by id");
    if (orders[i].status > 4) return fail(BK_INVALID_ARGUMENT, "bad order status");
    if (orders[i].status == 1) act.push_back(i);
  }
  const uint32_t pool = static_cast<uint32_t>(env->R) * 64u;
  if (act.size() > pool) return fail(BK_CAPACITY, "snapshot holds more Active orders than max_live_orders");
  if (int rc = use_device(env)) return rc;
  HIPCHK(hipStreamSynchronize(env->stream));
  std::stable_sort(act.begin(), act.end(), [&](uint64_t a, uint64_t b) { return key_time[a] < key_time[b]; });

  const uint32_t L = env->cfg.levels, W = env->W, tick = env->asset_tick[book % env->M];
  std::vector<uint32_t> st(env->stride, 0u), l2(W, 0u);
  uint32_t* hdr = st.data();
  HIPCHK(hipMemcpy(hdr, env->state.p + static_cast<size_t>(book) * env->stride, HDR_DW * 4, hipMemcpyDeviceToHost));
  hdr[H_T_LO] = static_cast<uint32_t>(t);
  hdr[H_T_HI] = static_cast<uint32_t>(t >> 32);
  hdr[H_NEXT_ID] = static_cast<uint32_t>(n_orders);
  hdr[H_SEQ] = static_cast<uint32_t>(act.size());
  env->stamp_room.raise(act.size());
  hdr[H_TRADES_LO] = static_cast<uint32_t>(n_trades);
  hdr[H_TRADES_HI] = static_cast<uint32_t>(n_trades >> 32);
  hdr[H_TRADE_BASE_LO] = hdr[H_TRADE_BASE_HI] = 0;
  hdr[H_FLAGS] = 0;
  hdr[H_TRADE_VOL] = trade_vol;
  hdr[H_LAST_NTRADES] = hdr[H_LAST_NEVENTS] = 0;
  for (int r = 0; r < 8; ++r) hdr[H_LIVE0 + 2 * r] = hdr[H_LIVE0 + 2 * r + 1] = 0;
  uint32_t bid_best = 0, ask_best = 0xFFFFFFFFu, bid_vol = 0, ask_vol = 0;
  for (size_t k = 0; k < act.size(); ++k) {
    const bk_order& o = orders[act[k]];
    const uint32_t r = static_cast<uint32_t>(k) / 64u, lane = static_cast<uint32_t>(k) % 64u;
    uint32_t* p = st.data() + HDR_DW + r * POOL_FIELDS * 64;
    p[0 * 64 + lane] = o.price;
    p[1 * 64 + lane] = o.vol;
    p[2 * 64 + lane] = static_cast<uint32_t>(o.order_id);
    p[3 * 64 + lane] = static_cast<uint32_t>(k);  // seq: rank in key-time order
    p[4 * 64 + lane] = 1u | (o.side_is_bid ? 2u : 0u);
    hdr[H_LIVE0 + 2 * r + (lane >> 5)] |= 1u << (lane & 31);
    if (o.side_is_bid) {
      bid_best = std::max(bid_best, o.price);
      bid_vol += o.vol;
    } else {
      ask_best = std::min(ask_best, o.price);
      ask_vol += o.vol;
    }
  }
  // level-2 record of the loaded book (orderbook.rs:229-264): [trade_vol, bid, ask, ask_vol, bid_vol, levels...]
  l2[0] = trade_vol;
  l2[1] = bid_best;
  l2[2] = ask_best;
  l2[3] = ask_vol;
  l2[4] = bid_vol;
  // (level q is the price touch -/+ q * tick with a wrapping u32 multiply: with a huge tick several levels may alias)
  for (uint64_t i : act) {
    const bk_order& o = orders[i];
    const uint32_t d = o.side_is_bid ? bid_best - o.price : o.price - ask_best;
    for (uint32_t q = 0; q < L; ++q) {
      if (q * tick == d) {
        l2[5 + 4 * q + (o.side_is_bid ? 0 : 2)] += o.vol;
        l2[5 + 4 * q + (o.side_is_bid ? 1 : 3)] += 1;
      }
    }
  }
  std::vector<DevOrderLog> log(n_orders);
  bh.orders.clear();
  for (uint64_t i = 0; i < n_orders; ++i) {
    const bk_order& o = orders[i];
    bh.orders.push_back(HostOrder{static_cast<uint8_t>(o.side_is_bid ? 1 : 0), o.start_vol, o.price, o.trader_id,
                                  o.arr_time});
    DevOrderLog& d = log[i];
    std::memset(&d, 0, sizeof(d));
    d.status = o.status;
    d.vol = o.vol;
    d.price = o.price;
    d.key_price = key_price[i];
    d.arr_lo = static_cast<uint32_t>(o.arr_time);
    d.arr_hi = static_cast<uint32_t>(o.arr_time >> 32);
    d.end_lo = static_cast<uint32_t>(o.end_time);
    d.end_hi = static_cast<uint32_t>(o.end_time >> 32);
    d.key_lo = static_cast<uint32_t>(key_time[i]);
    d.key_hi = static_cast<uint32_t>(key_time[i] >> 32);
  }
  std::vector<DevTrade> tr(n_trades);
  for (uint64_t i = 0; i < n_trades; ++i) {
    const bk_trade& x = trades[i];
    tr[i] = DevTrade{static_cast<uint32_t>(x.t), static_cast<uint32_t>(x.t >> 32), x.price, x.vol,
                     static_cast<uint32_t>(x.active_order_id), static_cast<uint32_t>(x.passive_order_id),
                     x.side_is_bid ? 1u : 0u, 0u};
  }
  HIPCHK(hipMemcpy(env->state.p + static_cast<size_t>(book) * env->stride, st.data(), st.size() * 4,
                   hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(env->l2_last.p + static_cast<size_t>(book) * W, l2.data(), W * 4, hipMemcpyHostToDevice));
  if (n_orders)
    HIPCHK(hipMemcpy(env->order_log.p + static_cast<size_t>(book) * env->cfg.max_orders, log.data(),
                     n_orders * sizeof(DevOrderLog), hipMemcpyHostToDevice));
  if (n_trades)
    HIPCHK(hipMemcpy(env->trades.p + static_cast<size_t>(book) * env->cfg.trade_capacity, tr.data(),
                     n_trades * sizeof(DevTrade), hipMemcpyHostToDevice));
  env->ml_valid = false;
  env->wl_valid = false;
  bh.n_uploaded = n_orders;
  bh.log_fresh = false;
  bh.time_offset = t - (env->cfg.start_time + env->steps_done * env->cfg.step_size);
  return BK_OK;
}

// OrderBook::set_time (crates/order_book/src/orderbook.rs:183-185) for one book (host-driven path)
int bk_set_time(bk_env* env, uint32_t book, uint64_t t) {
  if (int rc = check_book(env, book)) return rc;
  if (int rc = use_device(env)) return rc;
  HIPCHK(hipStreamSynchronize(env->stream));
  const uint32_t w[2] = {static_cast<uint32_t>(t), static_cast<uint32_t>(t >> 32)};
  HIPCHK(hipMemcpy(env->state.p + static_cast<size_t>(book) * env->stride + H_T_LO, w, 8, hipMemcpyHostToDevice));
  env->books[book].time_offset = t - (env->cfg.start_time + env->steps_done * env->cfg.step_size);
  return BK_OK;
}

int bk_time(bk_env* env, uint32_t book, uint64_t* out) {
  if (int rc = check_book(env, book)) return rc;
  uint32_t h[2];
  if (int rc = read_hdr(env, book, H_T_LO, 2, h)) return rc;
  if (out) *out = (static_cast<uint64_t>(h[1]) << 32) | h[0];
  return BK_OK;
}

int bk_trade_vol(bk_env* env, uint32_t book, uint32_t* out) {
  if (int rc = check_book(env, book)) return rc;
  if (!out) return fail(BK_INVALID_ARGUMENT, "null argument");
  return read_hdr(env, book, H_TRADE_VOL, 1, out);
}

int bk_steps_done(bk_env* env, uint64_t* out) {
  if (!env) return fail(BK_INVALID_ARGUMENT, "null env");
  if (out) *out = env->steps_done;
  return BK_OK;
}

int bk_book_flags(bk_env* env, uint32_t* out) {
  if (!env || !out) return fail(BK_INVALID_ARGUMENT, "null argument");
  if (int rc = use_device(env)) return rc;
  std::vector<uint64_t> v(env->cfg.n_books);
  if (int rc = gather_header(env, H_FLAGS, 1, v.data())) return rc;
  for (size_t b = 0; b < v.size(); ++b) out[b] = static_cast<uint32_t>(v[b]);
  return BK_OK;
}

// Clear sticky flag bits of every book (the caller has seen and handled them: e.g. after draining the trade records that
// overflowed, or after reporting a capacity error once)
int bk_clear_flags(bk_env* env, uint32_t mask) {
  if (!env) return fail(BK_INVALID_ARGUMENT, "null env");
  if (int rc = use_device(env)) return rc;
  const uint32_t B = env->cfg.n_books;
  hipLaunchKernelGGL(k_book_service, dim3((B + 255) / 256), dim3(256), 0, env->stream, env->state.p, env->stride, B, 2, mask);
  HIPCHK(hipGetLastError());
  return BK_OK;
}

// What a strict caller polls after every step: the OR of all books' sticky flags and the largest number of trade
// records any book retains (towards trade_capacity) - one small reduction + an 8-byte copy instead of n_books words.
int bk_flags_summary(bk_env* env, uint32_t* flags_or, uint64_t* max_retained_trades) {
  if (!env) return fail(BK_INVALID_ARGUMENT, "null env");
  if (int rc = use_device(env)) return rc;
  const uint32_t B = env->cfg.n_books;
  if (!env->gather_buf.p) HIPCHK(env->gather_buf.alloc(B));
  uint32_t* out = reinterpret_cast<uint32_t*>(env->gather_buf.p);
  HIPCHK(hipMemsetAsync(out, 0, 8, env->stream));
  hipLaunchKernelGGL(k_flags_summary, dim3((B + 255) / 256), dim3(256), 0, env->stream, env->state.p, env->stride, B, out);
  HIPCHK(hipGetLastError());
  uint32_t res[2] = {0, 0};
  HIPCHK(hipMemcpyAsync(res, out, 8, hipMemcpyDeviceToHost, env->stream));
  HIPCHK(hipStreamSynchronize(env->stream));
  if (flags_or) *flags_or = res[0];
  if (max_retained_trades) *max_retained_trades = res[1];
  return BK_OK;
}

int bk_rng_state(bk_env* env, uint32_t book, uint64_t out_state[2]) {
  if (int rc = check_book(env, book)) return rc;
  if (!out_state) return fail(BK_INVALID_ARGUMENT, "null argument");
  uint32_t h[4];
  if (int rc = read_hdr(env, book, H_S0_LO, 4, h)) return rc;
  out_state[0] = (static_cast<uint64_t>(h[1]) << 32) | h[0];
  out_state[1] = (static_cast<uint64_t>(h[3]) << 32) | h[2];
  return BK_OK;
}

int bk_live_orders(bk_env* env, uint32_t book, uint32_t cap, bk_order* out, uint32_t* n_out) {
  if (int rc = check_book(env, book)) return rc;
  if (cap && !out) return fail(BK_INVALID_ARGUMENT, "null argument");
  std::vector<uint32_t> st(env->stride);
  if (int rc = read_hdr(env, book, 0, static_cast<int>(env->stride), st.data())) return rc;
  struct Live {
    uint32_t price, vol, id, seq, bid;
  };
  std::vector<Live> v;
  for (int r = 0; r < env->R; ++r) {
    const uint32_t* p = st.data() + HDR_DW + r * POOL_FIELDS * 64;
    for (int l = 0; l < 64; ++l)
      if (p[4 * 64 + l] & 1u) v.push_back(Live{p[l], p[64 + l], p[128 + l], p[192 + l], (p[4 * 64 + l] >> 1) & 1u});
  }
  std::sort(v.begin(), v.end(), [](const Live& x, const Live& y) {
    if (x.bid != y.bid) return x.bid > y.bid;  // bids first
    if (x.price != y.price) return x.bid ? x.price > y.price : x.price < y.price;
    return x.seq < y.seq;
  });
  if (n_out) *n_out = static_cast<uint32_t>(v.size());
  for (size_t i = 0; i < v.size() && i < cap; ++i) {
    std::memset(&out[i], 0, sizeof(bk_order));
    out[i].side_is_bid = static_cast<uint8_t>(v[i].bid);
    out[i].status = 1;
    out[i].vol = v[i].vol;
    out[i].price = v[i].price;
    out[i].order_id = v[i].id;
    out[i].end_time = ~0ull;
  }
  return BK_OK;
}

// ------------------------------------------------------------------ stats
int bk_stats_compute(bk_env* env, bk_stats* out_host) {
  if (!env) return fail(BK_INVALID_ARGUMENT, "null env");
  if (int rc = use_device(env)) return rc;
  // reset the record from the template kept next to it: a device-to-device copy in stream order, so that queueing the
  // reduction never waits for the stepping kernels in front of it (the per-launch all-gather of a sharded run)
  HIPCHK(hipMemcpyAsync(env->stats.p, env->stats.p + 1, sizeof(DevStats), hipMemcpyDeviceToDevice, env->stream));
  const uint32_t B = env->cfg.n_books;
  const uint32_t blocks = std::min<uint32_t>((B + 255) / 256, 1024);
  hipLaunchKernelGGL(k_stats, dim3(blocks), dim3(256), 0, env->stream, env->state.p, env->stride, env->l2_last.p,
                     env->W, B, env->stats.p);
  HIPCHK(hipGetLastError());
  if (out_host) {
    HIPCHK(hipStreamSynchronize(env->stream));
    HIPCHK(hipMemcpy(out_host, env->stats.p, sizeof(bk_stats), hipMemcpyDeviceToHost));
  }
  return BK_OK;
}

int bk_stats_device_ptr(bk_env* env, void** out) {
  if (!env || !out) return fail(BK_INVALID_ARGUMENT, "null argument");
  *out = env->stats.p;
  return BK_OK;
}

// the latest level-2 records on the device: u32[n_books][bk_l2_width()], for on-device consumers (e.g. the optional
// per-book L1 all-gather across GPUs); valid until the env is destroyed, contents as of the work queued so far
int bk_level2_device_ptr(bk_env* env, void** out) {
  if (!env || !out) return fail(BK_INVALID_ARGUMENT, "null argument");
  *out = env->l2_last.p;
  return BK_OK;
}

// ------------------------------------------------------------------ measurement
int bk_profile_enable(bk_env* env, int on) {
  if (!env) return fail(BK_INVALID_ARGUMENT, "null env");
  env->profile = on < 0 ? 0 : on;
  env->prof_tick = 0;
  env->prof_now = false;
  if (env->profile > 0 && use_device(env) == BK_OK) {
    while (env->prof_pool.size() < 256) {
      hipEvent_t e = nullptr;
      if (hipEventCreate(&e) != hipSuccess) break;
      env->prof_pool.push_back(e);
    }
    // Two events recorded on a stream bracket the launch gap as well as the kernel (the first fires when the previous
    // kernel of the stream ends): ~4 us, 3 % of a 135 us launch and 12 % of a 35 us one against the kernel trace
    // (scripts/kt_check.sh).  The reading of two events recorded back to back, calibrated once per env, is subtracted
    // from every sample.
    if (env->prof_bracket_ms == 0 && env->prof_pool.size() >= 2) {
      HIPCHK(hipStreamSynchronize(env->stream));
      std::vector<float> v;
      for (int i = 0; i < 9; ++i) {
        hipLaunchKernelGGL(k_delay, dim3(1), dim3(64), 0, env->stream, 1u);  // something for the first event to follow
        (void)hipEventRecord(env->prof_pool[0], env->stream);
        (void)hipEventRecord(env->prof_pool[1], env->stream);
        (void)hipStreamSynchronize(env->stream);
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, env->prof_pool[0], env->prof_pool[1]) == hipSuccess) v.push_back(ms);
      }
      if (!v.empty()) {
        std::sort(v.begin(), v.end());
        env->prof_bracket_ms = v[v.size() / 2];
      }
      if (getenv("BOURSE_AMD_VERBOSE")) fprintf(stderr, "bourse_amd: two events back to back read %.1f us\n", env->prof_bracket_ms * 1e3);
    }
  }
  return BK_OK;
}

int bk_profile_read(bk_env* env, double* total_ms, uint64_t* n_launches, int reset) {
  if (!env) return fail(BK_INVALID_ARGUMENT, "null env");
  if (int rc = use_device(env)) return rc;
  if (int rc = prof_collect(env)) return rc;
  double ms = 0;
  uint64_t n = 0;
  for (int k = 0; k < bk_env::PROF_KINDS; ++k) {
    ms += env->prof_ms[k];
    n += env->prof_launches[k];
    if (reset) {
      env->prof_ms[k] = 0.0;
      env->prof_launches[k] = 0;
    }
  }
  if (total_ms) *total_ms = ms;
  if (n_launches) *n_launches = n;
  return BK_OK;
}

int bk_profile_read_kind(bk_env* env, int kind, double* total_ms, uint64_t* n_launches) {
  if (!env || kind < 0 || kind >= bk_env::PROF_KINDS) return fail(BK_INVALID_ARGUMENT, "bad argument");
  if (int rc = use_device(env)) return rc;
  if (int rc = prof_collect(env)) return rc;
  if (total_ms) *total_ms = env->prof_ms[kind];
  if (n_launches) *n_launches = env->prof_launches[kind];
  return BK_OK;
}

int bk_get_pipeline(bk_env* env, int* split, int* n_parts) {
  if (!env) return fail(BK_INVALID_ARGUMENT, "null env");
  const Plan pl = env_plan(env);  // the same plan bk_run launches from
  // by PlanKind: 0 fused, 1 split (lane-per-book agents), 2 wave_split, 3 wave
  static constexpr int code[] = {0, 3, 1, 2, 0, 2, 1, 1};
  static_assert(PL_MIXED_WPB == 7, "one code per PlanKind");
  if (split) *split = code[pl.kind];
  if (n_parts) *n_parts = pl.parts;
  return BK_OK;
}

int bk_set_pipeline(bk_env* env, int mode) {
  if (!env || mode < 0 || mode > 5)
    return fail(BK_INVALID_ARGUMENT,
                "pipeline mode must be 0 (auto), 1 (fused), 2 (split), 3 (split, wave-per-book AgentSet members), 4 (wave_split: "
                "wave-parallel RNG decode kernel + event kernel) or 5 (wave: both fused in one persistent kernel)");
  env->pipeline = mode;
  return BK_OK;
}

// DEPRECATED (kept so that clients built against rounds 1-3 still link): those rounds rolled a launch of the library's
// own pipeline choice back when it overflowed a pool the other kernels fit; no such launch exists any more.  Always 0.
int bk_pipeline_fallbacks(bk_env* env, uint64_t* out) {
  if (!env || !out) return fail(BK_INVALID_ARGUMENT, "null argument");
  *out = 0;
  return BK_OK;
}

// k_agents_wave knobs: look-ahead of the vector path (1..64 draws; small values force the scalar slow path - tests),
// parts the wave pipeline cuts the batch in (0 = as the lane split)
int bk_set_wave_options(bk_env* env, uint32_t lookahead, int parts) {
  if (!env || lookahead < 1 || lookahead > 64 || parts < 0 || parts > bk_env::MAX_PARTS)
    return fail(BK_INVALID_ARGUMENT, "lookahead must be in 1..64 and parts in 0..8");
  env->wave_lookahead = lookahead;
  env->wave_parts = parts;
  return BK_OK;
}

// split pipeline geometry: the batch is cut in min(n_parts, units / min_part) contiguous parts on separate streams
int bk_set_split_parts(bk_env* env, int n_parts, uint32_t min_part) {
  if (!env || n_parts < 1 || n_parts > bk_env::MAX_PARTS || min_part < 64)
    return fail(BK_INVALID_ARGUMENT, "n_parts must be in 1..8 and min_part >= 64");
  env->n_parts = n_parts;
  env->min_part = min_part;
  return BK_OK;
}

int bk_get_split_parts(bk_env* env, int* n_parts, uint32_t* min_part) {
  if (!env) return fail(BK_INVALID_ARGUMENT, "null env");
  if (n_parts) *n_parts = env->n_parts;
  if (min_part) *min_part = env->min_part;
  return BK_OK;
}

// orders created so far per book by the on-device agents (OrderBook::current_order_id, orderbook.rs:327-329)
int bk_order_counts(bk_env* env, uint64_t* totals) {
  if (!env || !totals) return fail(BK_INVALID_ARGUMENT, "null argument");
  if (int rc = use_device(env)) return rc;
  return gather_header(env, H_NEXT_ID, 1, totals);
}

int bk_event_steps_keyed(bk_env* env, uint64_t* counts) {
  if (!env || !counts) return fail(BK_INVALID_ARGUMENT, "null argument");
  if (int rc = use_device(env)) return rc;
  return gather_header(env, H_EV_KEYED, 1, counts);
}

int bk_stamp_compactions(bk_env* env, uint64_t* out) {
  if (!env || !out) return fail(BK_INVALID_ARGUMENT, env ? "null argument" : "null env");
  *out = env->stamp_compactions;
  return BK_OK;
}

// ---------------------------------------------------------------- checkpoint / resume (on-device order flow)
// The reference cannot resume a running simulation (Env, agents and RNG are not serialisable);
// here the whole simulation state IS the per-book device block (pool, clock, counters, RNG), so a checkpoint
// is one device-to-host copy.  Host-driven envs (order log + host order table) are not covered.
// header: 8 x u64 = {magic "BKCKPT02", steps_done, n_books << 32 | stride (pool size), levels width W << 32 | assets,
// number of Noise/Momentum members << 32 | RandomAgents groups, hash of the installed agent set, trading flag, 0}
constexpr uint64_t CKPT_MAGIC = 0x3230545043434B42ull;  // "BKCKPT02" little-endian
constexpr size_t CKPT_HDR = 8;                            // u64 words
static void ckpt_header(const bk_env* env, uint64_t* h) {
  h[0] = CKPT_MAGIC;
  h[1] = env->steps_done;
  h[2] = (static_cast<uint64_t>(env->cfg.n_books) << 32) | env->stride;
  h[3] = (static_cast<uint64_t>(env->W) << 32) | env->M;
  h[4] = (static_cast<uint64_t>(env->n_mixed) << 32) | static_cast<uint32_t>(env->groups.size());
  h[5] = env->agents_hash;
  h[6] = env->trading;
  h[7] = 0;
}
uint64_t bk_checkpoint_bytes(const bk_env* env) {
  // header + per-book state blocks + the latest level-2 records (Env::level_2_data; the lane-per-book members' update
  // reads the touches from there)
  return env ? CKPT_HDR * 8 + static_cast<uint64_t>(env->cfg.n_books) * (env->stride + env->W) * 4 : 0;
}

int bk_checkpoint_save(bk_env* env, void* out, uint64_t nbytes) {
  if (!env || !out) return fail(BK_INVALID_ARGUMENT, "null argument");
  if (nbytes < bk_checkpoint_bytes(env)) return fail(BK_INVALID_ARGUMENT, "checkpoint buffer too small");
  if (env->device_ingress) return fail(BK_INVALID_ARGUMENT, "checkpointing a host-driven env is not supported");
  if (env->agent_log)
    return fail(BK_INVALID_ARGUMENT, "checkpointing an env with the agents' order log (bk_set_agent_order_log) is not supported");
  for (const BookHost& bh : env->books)
    if (!bh.orders.empty()) return fail(BK_INVALID_ARGUMENT, "checkpointing a host-driven env is not supported");
  if (int rc = use_device(env)) return rc;
  HIPCHK(hipStreamSynchronize(env->stream));
  uint64_t* h = static_cast<uint64_t*>(out);
  ckpt_header(env, h);
  const size_t sb = static_cast<size_t>(env->cfg.n_books) * env->stride * 4;
  HIPCHK(hipMemcpy(h + CKPT_HDR, env->state.p, sb, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(reinterpret_cast<char*>(h + CKPT_HDR) + sb, env->l2_last.p,
                   static_cast<size_t>(env->cfg.n_books) * env->W * 4, hipMemcpyDeviceToHost));
  return BK_OK;
}

int bk_checkpoint_load(bk_env* env, const void* in, uint64_t nbytes) {
  if (!env || !in) return fail(BK_INVALID_ARGUMENT, "null argument");
  // (a restored book's id counter would cover orders the agents' log never saw: their rows are unwritten)
  if (env->agent_log)
    return fail(BK_INVALID_ARGUMENT, "restoring a checkpoint into an env with the agents' order log (bk_set_agent_order_log) is "
                                     "not supported");
  const uint64_t* h = static_cast<const uint64_t*>(in);
  if (nbytes < CKPT_HDR * 8 || h[0] != CKPT_MAGIC)
    return fail(BK_INVALID_ARGUMENT, "not a bourse_amd checkpoint of this version (bad magic)");
  uint64_t want[CKPT_HDR];
  ckpt_header(env, want);
  if (nbytes < bk_checkpoint_bytes(env) || h[2] != want[2] || h[3] != want[3])
    return fail(BK_INVALID_ARGUMENT, "checkpoint does not match this env (n_books / pool size / levels / assets)");
  if (h[4] != want[4] || h[5] != want[5])
    return fail(BK_INVALID_ARGUMENT, "checkpoint was taken with a different agent set: install the same agents first");
  if (int rc = use_device(env)) return rc;
  HIPCHK(hipStreamSynchronize(env->stream));
  const size_t sb = static_cast<size_t>(env->cfg.n_books) * env->stride * 4;
  HIPCHK(hipMemcpy(env->state.p, h + CKPT_HDR, sb, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(env->l2_last.p, reinterpret_cast<const char*>(h + CKPT_HDR) + sb,
                   static_cast<size_t>(env->cfg.n_books) * env->W * 4, hipMemcpyHostToDevice));
  env->ml_valid = false;
  env->wl_valid = false;
  env->steps_done = h[1];
  env->hist_base = h[1];  // retained history/trade records restart at the restored step
  env->trading = h[6] ? 1u : 0u;  // the host mirror of the books' trading flag (H_TRADING travels in the state blocks)
  // an image is only ever taken from an on-device-order-flow env: the restored books hold the agents' orders and ids, so
  // host-driven orders (whose ids would restart at 0) are refused from here on, exactly as after a bk_run
  if (env->n_mixed || !env->groups.empty() || h[1] > 0) env->device_flow = true;
  const uint32_t B = env->cfg.n_books;
  hipLaunchKernelGGL(k_book_service, dim3((B + 255) / 256), dim3(256), 0, env->stream, env->state.p, env->stride, B, 0,
                     0u);
  HIPCHK(hipGetLastError());
  // the image's stamps are whatever its env had reached: compacted here, the bound starts again at the pool size
  if (int rc = compact_stamps(env)) return rc;
  // the tables folded from the history ring are no part of a checkpoint: every row starts again at the restored step
  for (HistTable& t : env->tables) {
    if (!t.on) continue;
    t.clear(env, nullptr, 1, false);
    HIPCHK(hipGetLastError());
    t.seen = env->steps_done;
  }
  if (env->cross_table.on) {  // ... and the per-market one
    launch_cross_clear(env, nullptr, 1, false);
    HIPCHK(hipGetLastError());
    env->cross_table.seen = env->steps_done;
  }
  if (env->flow_lags) {  // nor is the flow table: every word starts again, the cursors at the restored counts
    launch_flow_clear(env, nullptr, 1, false);
    HIPCHK(hipGetLastError());
  }
  HIPCHK(hipStreamSynchronize(env->stream));
  return BK_OK;
}

// ---------------------------------------------------------------- per-book reset to a device-resident snapshot
// No counterpart in the reference (an Env is rebuilt, never rewound).  What is moved is what a checkpoint carries - the
// books' state blocks and level-2 records - but device to device, and back only for the units a mask names
// (book_reset.hpp).
uint64_t bk_snapshot_bytes(const bk_env* env) {
  return env ? static_cast<uint64_t>(env->cfg.n_books) * (env->stride + env->W) * 4 : 0;
}

// the env kinds bk_checkpoint_save refuses, refused here for the same reasons (a device-ingress env has entries of its
// own, bk_ingress_snapshot_save / bk_ingress_reset_books* below, which rewind what it keeps beside the state blocks)
static int snapshot_env_ok(bk_env* env, uint32_t slot) {
  if (!env) return fail(BK_INVALID_ARGUMENT, "null env");
  if (slot >= BK_MAX_SNAPSHOTS) return fail(BK_INVALID_ARGUMENT, "snapshot slot out of range (BK_MAX_SNAPSHOTS = 4)");
  if (env->device_ingress)
    return fail(BK_INVALID_ARGUMENT, "snapshots of a host-driven env (bk_device_ingress_enable) are not supported, as its "
                                     "checkpoints are not: the queues, the order records and the agents' held ids would "
                                     "have to be rewound as well");
  if (env->agent_log)
    return fail(BK_INVALID_ARGUMENT, "snapshots of an env with the agents' order log (bk_set_agent_order_log) are not "
                                     "supported, as its checkpoints are not: the log would keep the abandoned run's orders");
  if (!env->device_flow)  // (an env bk_run has stepped with agents holds no host-placed order: host_flow_ok)
    for (const BookHost& bh : env->books)
      if (!bh.orders.empty())
        return fail(BK_INVALID_ARGUMENT, "snapshots of a host-driven env (host-placed orders) are not supported, as its "
                                         "checkpoints are not: the host's order table is not part of the books' state");
  return BK_OK;
}

int bk_snapshot_save(bk_env* env, uint32_t slot) {
  if (int rc = snapshot_env_ok(env, slot)) return rc;
  if (int rc = use_device(env)) return rc;
  bk_env::Snapshot& s = env->snaps[slot];
  const size_t sb = static_cast<size_t>(env->cfg.n_books) * env->stride, lb = static_cast<size_t>(env->cfg.n_books) * env->W;
  if (!s.buf.p) HIPCHK(s.buf.alloc(sb + lb));
  s.used = false;
  HIPCHK(hipMemcpyAsync(s.buf.p, env->state.p, sb * 4, hipMemcpyDeviceToDevice, env->stream));
  HIPCHK(hipMemcpyAsync(s.buf.p + sb, env->l2_last.p, lb * 4, hipMemcpyDeviceToDevice, env->stream));
  uint64_t h[CKPT_HDR];
  ckpt_header(env, h);
  for (int i = 0; i < 4; ++i) s.shape[i] = h[2 + i];
  s.stamp_bound = env->stamp_room.bound;
  s.used = true;
  return BK_OK;
}

int bk_snapshot_drop(bk_env* env, uint32_t slot) {
  if (!env) return fail(BK_INVALID_ARGUMENT, "null env");
  if (slot >= BK_MAX_SNAPSHOTS) return fail(BK_INVALID_ARGUMENT, "snapshot slot out of range (BK_MAX_SNAPSHOTS = 4)");
  if (int rc = use_device(env)) return rc;
  bk_env::Snapshot& s = env->snaps[slot];
  if (s.buf.p) HIPCHK(hipStreamSynchronize(env->stream));  // (a reset from the slot may still be queued)
  s.used = false;
  HIPCHK(s.buf.alloc(0));
  return BK_OK;
}

// a slot's ckpt_header words (h[2..5], as its save kept them) against the env as it is now
static int snapshot_shape_ok(bk_env* env, const uint64_t (&shape)[4]) {
  uint64_t h[CKPT_HDR];
  ckpt_header(env, h);
  if (shape[0] != h[2] || shape[1] != h[3])
    return fail(BK_INVALID_ARGUMENT, "snapshot does not match this env (n_books / pool size / levels / assets)");
  if (shape[2] != h[4] || shape[3] != h[5])
    return fail(BK_INVALID_ARGUMENT, "snapshot was taken with a different agent set: install the same agents first");
  return BK_OK;
}

// every refusal, before anything is enqueued
static int reset_ok(bk_env* env, uint32_t slot, const void* mask) {
  if (int rc = snapshot_env_ok(env, slot)) return rc;
  if (!mask) return fail(BK_INVALID_ARGUMENT, "null mask");
  const bk_env::Snapshot& s = env->snaps[slot];
  if (!s.used) return fail(BK_INVALID_ARGUMENT, "snapshot slot is empty: call bk_snapshot_save first");
  return snapshot_shape_ok(env, s.shape);
}

// A host mask of n entries (and seeds, when given) into lazily allocated device buffers, for the _device form of the
// caller: waits for the env's stream, so the caller's arrays are free when it returns
// (`seeds` is required when `seeds_host` is given; bk_accounts_clear has neither)
static int stage_mask(bk_env* env, size_t n, const uint8_t* mask_host, DevBuf<uint8_t>& mask,
                      const uint64_t* seeds_host = nullptr, DevBuf<uint64_t>* seeds = nullptr) {
  if (!mask.p) HIPCHK(mask.alloc(n));
  HIPCHK(hipMemcpyAsync(mask.p, mask_host, n, hipMemcpyHostToDevice, env->stream));
  if (seeds_host) {
    if (!seeds->p) HIPCHK(seeds->alloc(n));
    HIPCHK(hipMemcpyAsync(seeds->p, seeds_host, n * 8, hipMemcpyHostToDevice, env->stream));
  }
  HIPCHK(hipStreamSynchronize(env->stream));
  return BK_OK;
}

// The host form of a table's masked clear behind the table's own check: no mask is the _device form's business, a mask
// (one byte per book) goes through the table's `staging` into it.
static int clear_from_host(bk_env* env, const uint8_t* mask_host, DevBuf<uint8_t>& staging,
                           int (*device_form)(bk_env*, const uint8_t*), uint32_t books_per_byte = 1) {
  if (!mask_host) return device_form(env, nullptr);
  if (int rc = use_device(env)) return rc;
  if (int rc = stage_mask(env, env->cfg.n_books / books_per_byte, mask_host, staging)) return rc;
  return device_form(env, staging.p);
}

// The host form of either reset behind its refusals: mask and seeds (one per unit) through the env's staging into the _device form.
static int reset_from_host(bk_env* env, uint32_t slot, const uint8_t* mask_host, const uint64_t* seeds_host,
                           int (*device_form)(bk_env*, uint32_t, const uint8_t*, const uint64_t*)) {
  if (int rc = use_device(env)) return rc;
  const size_t n_units = env->cfg.n_books / env->M;
  if (int rc = stage_mask(env, n_units, mask_host, env->reset_mask, seeds_host, &env->reset_seeds)) return rc;
  return device_form(env, slot, env->reset_mask.p, seeds_host ? env->reset_seeds.p : nullptr);
}

// reset::k_reset_books<R> for the units the mask names, from `snap` = [state | l2_last] of a slot, on the env's stream
static void launch_reset_books(bk_env* env, const uint32_t* snap, const uint8_t* mask_dev, const uint64_t* seeds_dev) {
  const size_t sb = static_cast<size_t>(env->cfg.n_books) * env->stride;
  reset::ResetArgs g{};
  g.state = env->state.p;
  g.l2_last = env->l2_last.p;
  g.snap_state = snap;
  g.snap_l2 = snap + sb;
  g.stride = env->stride;
  g.W = env->W;
  g.M = env->M;
  g.n_units = env->cfg.n_books / env->M;
  g.mask = mask_dev;
  g.seeds = seeds_dev;
  g.trading = env->trading;
  const dim3 grid((g.n_units + reset::WAVES - 1) / reset::WAVES), block(64 * reset::WAVES);
  by_R(env->R, [&](auto r) { hipLaunchKernelGGL(reset::k_reset_books<decltype(r)::value>, grid, block, 0, env->stream, g); });
}

// What both resets open with, on the env's stream: the masked units' books go back to `snap` = [state | l2_last] of a slot
// whose save kept `stamp_bound`.
static int reset_books_from(bk_env* env, const uint32_t* snap, uint64_t stamp_bound, const uint8_t* mask_dev,
                            const uint64_t* seeds_dev) {
  // the tables folded from the history ring: lost steps of any of them refuse the reset before one of them launches anything
  // (checked bins, lags, series, cross and launched series, lags, bins, cross: the order decides whose message is seen when two
  // have lost steps)
  for (int i = N_HIST_TABLES - 1; i >= 0; --i)
    if (env->tables[i].on)
      if (int rc = table_lost_check(env, env->tables[i])) return rc;
  if (env->cross_table.on)
    if (int rc = table_lost_check(env, env->cross_table)) return rc;
  // ... then the steps so far belong to the old episode, and no return, span or pair reaches over the reset: cut the carry
  for (HistTable& t : env->tables) {
    if (!t.on) continue;
    if (int rc = table_fold_outstanding(env, t)) return rc;
    t.clear(env, mask_dev, env->M, true);
    HIPCHK(hipGetLastError());
  }
  if (env->cross_table.on) {  // the per-market table: the reset's mask is already one byte per market
    if (int rc = table_fold_outstanding(env, env->cross_table)) return rc;
    launch_cross_clear(env, mask_dev, env->M, true);
    HIPCHK(hipGetLastError());
  }
  if (env->flow_lags) {  // the flow table: the records so far belong to the old episode
    launch_flow_fold(env, env->flow_consume);
    HIPCHK(hipGetLastError());
  }
  launch_reset_books(env, snap, mask_dev, seeds_dev);
  HIPCHK(hipGetLastError());
  if (env->flow_lags) {  // ... the reset put H_TRADES back: the cursors follow, and no pair reaches over the reset
    launch_flow_clear(env, mask_dev, env->M, true);
    HIPCHK(hipGetLastError());
  }
  env->stamp_room.raise(stamp_bound);  // (the reset books' H_SEQ is the snapshot's again)
  return BK_OK;
}

// Holds NO host synchronisation: one launch on the env's stream - no stream wait, no host read of the mask, no allocation.
int bk_reset_books_device(bk_env* env, uint32_t slot, const uint8_t* mask_dev, const uint64_t* seeds_dev) {
  if (int rc = reset_ok(env, slot, mask_dev)) return rc;
  if (int rc = use_device(env)) return rc;
  if (int rc = reset_books_from(env, env->snaps[slot].buf.p, env->snaps[slot].stamp_bound, mask_dev, seeds_dev)) return rc;
  // which books changed is known on the device only: the members' lists of every book are rebuilt from the owner tags
  env->ml_valid = false;
  env->wl_valid = false;
  return BK_OK;
}

int bk_reset_books(bk_env* env, uint32_t slot, const uint8_t* mask_host, const uint64_t* seeds_host) {
  if (int rc = reset_ok(env, slot, mask_host)) return rc;
  return reset_from_host(env, slot, mask_host, seeds_host, bk_reset_books_device);
}

// ---------------------------------------------------------------- the same for a device-ingress env
// No counterpart in the reference.  A device-ingress env keeps more per book than the two arrays above: its queue length,
// the order records of the ids it has handed out, the held ids of bk_update_agents and the lists and momentum state of
// bk_update_members - all rewound here, on the device (ingress_reset.hpp).  The slots are the env's
// isnaps, apart from bk_snapshot_save's.
static bool held_active(const bk_env* env) { return !env->n_mixed && !env->groups.empty(); }
static bool members_active(const bk_env* env) { return env->n_mixed != 0; }

static int ingress_slot_ok(bk_env* env, uint32_t slot) {
  if (!env) return fail(BK_INVALID_ARGUMENT, "null env");
  if (slot >= BK_MAX_SNAPSHOTS) return fail(BK_INVALID_ARGUMENT, "snapshot slot out of range (BK_MAX_SNAPSHOTS = 4)");
  if (!env->device_ingress)
    return fail(BK_INVALID_ARGUMENT, "bk_ingress_snapshot_* / bk_ingress_reset_books* serve an env with the device ingress "
                                     "(bk_device_ingress_enable): this env's entries are bk_snapshot_save / bk_reset_books");
  return BK_OK;
}

// k_reset_records' arguments for this env's agents and members (the rows a reset moves); false: its work items would
// not fit the kernel's 32-bit index
static bool ingress_record_args(const bk_env* env, uint32_t n_keep, reset::RecordArgs& g) {
  g.n_units = env->cfg.n_books / env->M;
  g.M = env->M;
  g.stride = env->stride;
  g.max_orders = env->cfg.max_orders;
  g.n_keep = n_keep;
  uint32_t max_n = 0;
  if (held_active(env)) g.n_agents = env->n_agents_total;
  if (members_active(env)) {
    g.n_members = env->n_mixed;
    for (uint32_t j = 0; j < env->n_mixed; ++j) {
      g.member_n[j] = env->member_n[j];
      max_n = std::max(max_n, env->member_n[j]);
      if (env->member_type[j] == BK_AGENT_RANDOM) g.random_mask |= 1u << j;
    }
    g.list_cap = bkd::ingress::members_list_cap(static_cast<uint32_t>(env->R), max_n);  // (as bk_update_members sizes a row)
  }
  // (the order records are rows per book, the agents' and members' rows per unit)
  const uint64_t s_book = uint64_t(reset::segs(n_keep * reset::ORD_V, reset::SEG_V)) + reset::segs(n_keep * reset::LOG_V, reset::SEG_V);
  const uint64_t s_rows = reset::segs(g.n_agents, reset::SEG_DW) + uint64_t(g.n_members) * reset::segs(g.list_cap, reset::SEG_DW);
  return (s_book * env->M + s_rows) * g.n_units < 0xFFFFFFFFull;
}

uint64_t bk_ingress_snapshot_bytes(const bk_env* env, uint32_t slot) {
  return env && slot < BK_MAX_SNAPSHOTS && env->isnaps[slot].used ? env->isnaps[slot].bytes : 0;
}

// May synchronise (a reset may not): the number of ids to keep per book is read back from a small device reduction, and
// the slot's record arrays are sized by it.
int bk_ingress_snapshot_save(bk_env* env, uint32_t slot) {
  if (int rc = ingress_slot_ok(env, slot)) return rc;
  if (int rc = use_device(env)) return rc;
  bk_env::IngressSnapshot& s = env->isnaps[slot];
  const size_t B = env->cfg.n_books, n_units = B / env->M;
  const size_t sb = B * env->stride, lb = B * env->W;
  HIPCHK(hipStreamSynchronize(env->stream));  // (a reset from the slot may still be queued: its arrays may be replaced)
  if (!env->reset_list.p) {
    HIPCHK(env->reset_list.alloc(n_units + 1));
    int cus = 0;
    HIPCHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, env->cfg.device));
    env->reset_blocks = std::max(cus, 1) * 4;
  }
  uint32_t* counter = env->reset_list.p + n_units;
  uint32_t n_keep = 0;
  HIPCHK(hipMemsetAsync(counter, 0, 4, env->stream));
  hipLaunchKernelGGL(reset::k_max_keep, dim3((B + 255) / 256), dim3(256), 0, env->stream, env->state.p, env->stride,
                     static_cast<uint32_t>(B), env->cfg.max_orders, counter);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(&n_keep, counter, 4, hipMemcpyDeviceToHost, env->stream));
  HIPCHK(hipStreamSynchronize(env->stream));
  reset::RecordArgs g{};
  if (!ingress_record_args(env, n_keep, g))
    return fail(BK_CAPACITY, "bk_ingress_snapshot_save: books x order records exceed what one reset launch indexes");
  s.used = false;
  if (!s.buf.p) HIPCHK(s.buf.alloc(sb + lb));
  if (n_keep > s.keep_cap) {
    HIPCHK(s.orders.alloc(B * n_keep * reset::ORD_V));
    HIPCHK(s.log.alloc(B * n_keep * reset::LOG_V));
    s.keep_cap = n_keep;
  }
  s.n_keep = n_keep;
  HIPCHK(hipMemcpyAsync(s.buf.p, env->state.p, sb * 4, hipMemcpyDeviceToDevice, env->stream));
  HIPCHK(hipMemcpyAsync(s.buf.p + sb, env->l2_last.p, lb * 4, hipMemcpyDeviceToDevice, env->stream));
  if (n_keep) {  // the records of ids < keep_b, packed to rows of n_keep ids: k_reset_records over every unit
    g.n_agents = g.n_members = 0;
    g.keep_state = env->state.p;
    g.dst_orders = reinterpret_cast<bk_u32x4*>(s.orders.p);
    g.src_orders = reinterpret_cast<const bk_u32x4*>(env->dorders.p);
    g.dst_log = reinterpret_cast<bk_u32x4*>(s.log.p);
    g.src_log = reinterpret_cast<const bk_u32x4*>(env->order_log.p);
    g.dst_ids = n_keep;
    g.src_ids = env->cfg.max_orders;
    hipLaunchKernelGGL(reset::k_reset_records, dim3(env->reset_blocks), dim3(64 * reset::RECORD_WAVES), 0, env->stream, g);
    HIPCHK(hipGetLastError());
  }
  s.bytes = (sb + lb) * 4 + B * s.keep_cap * (reset::ORD_V + reset::LOG_V) * 16;
  s.held_saved = held_active(env) && !env->agent_held_stale;
  if (s.held_saved) {
    const size_t n = n_units * env->n_agents_total;
    if (s.held.n != n) HIPCHK(s.held.alloc(n));
    if (n) HIPCHK(hipMemcpyAsync(s.held.p, env->agent_held.p, n * 4, hipMemcpyDeviceToDevice, env->stream));
    s.bytes += n * 4;
  }
  s.members_saved = members_active(env) && !env->member_lists_stale;
  if (s.members_saved) {
    const size_t rows = n_units * env->n_mixed, nl = rows * env->member_list_cap;
    if (s.lists.n != nl) HIPCHK(s.lists.alloc(nl));
    if (s.lens.n != rows) HIPCHK(s.lens.alloc(rows));
    if (s.mstate.n != rows * 2) HIPCHK(s.mstate.alloc(rows * 2));
    if (s.mflags.n != n_units) HIPCHK(s.mflags.alloc(n_units));
    HIPCHK(hipMemcpyAsync(s.lists.p, env->member_lists.p, nl * 4, hipMemcpyDeviceToDevice, env->stream));
    HIPCHK(hipMemcpyAsync(s.lens.p, env->member_lens.p, rows * 4, hipMemcpyDeviceToDevice, env->stream));
    HIPCHK(hipMemcpyAsync(s.mstate.p, env->member_state.p, rows * 16, hipMemcpyDeviceToDevice, env->stream));
    HIPCHK(hipMemcpyAsync(s.mflags.p, env->member_flags.p, n_units * 4, hipMemcpyDeviceToDevice, env->stream));
    s.bytes += nl * 4 + rows * 20 + n_units * 4;
  }
  uint64_t h[CKPT_HDR];
  ckpt_header(env, h);
  for (int i = 0; i < 4; ++i) s.shape[i] = h[2 + i];
  s.installs = env->agent_installs;
  s.stamp_bound = env->stamp_room.bound;
  s.used = true;
  return BK_OK;
}

int bk_ingress_snapshot_drop(bk_env* env, uint32_t slot) {
  if (int rc = ingress_slot_ok(env, slot)) return rc;
  if (int rc = use_device(env)) return rc;
  bk_env::IngressSnapshot& s = env->isnaps[slot];
  if (s.buf.p) HIPCHK(hipStreamSynchronize(env->stream));  // (a reset from the slot may still be queued)
  s.used = false;
  s.n_keep = s.keep_cap = 0;
  s.bytes = 0;
  HIPCHK(s.buf.alloc(0));
  HIPCHK(s.orders.alloc(0));
  HIPCHK(s.log.alloc(0));
  HIPCHK(s.held.alloc(0));
  HIPCHK(s.lists.alloc(0));
  HIPCHK(s.lens.alloc(0));
  HIPCHK(s.mstate.alloc(0));
  HIPCHK(s.mflags.alloc(0));
  return BK_OK;
}

// every refusal, before anything is enqueued
static int ingress_reset_ok(bk_env* env, uint32_t slot, const void* mask) {
  if (int rc = ingress_slot_ok(env, slot)) return rc;
  const bk_env::IngressSnapshot& s = env->isnaps[slot];
  if (!s.used) return fail(BK_INVALID_ARGUMENT, "snapshot slot is empty: call bk_ingress_snapshot_save first");
  if (!mask) return fail(BK_INVALID_ARGUMENT, "null mask");
  if (int rc = snapshot_shape_ok(env, s.shape)) return rc;
  if (s.installs != env->agent_installs)
    return fail(BK_INVALID_ARGUMENT, "agents were installed again (bk_set_*agents*) since the snapshot was taken: their held "
                                     "ids and lists start empty at the next update, which a reset cannot restore - call "
                                     "bk_ingress_snapshot_save again");
  return BK_OK;
}

// Holds NO host synchronisation: a memset and three launches on the env's stream - no stream wait, no host read, no
// allocation (the list of masked units was allocated by the first save).
int bk_ingress_reset_books_device(bk_env* env, uint32_t slot, const uint8_t* mask_dev, const uint64_t* seeds_dev) {
  if (int rc = ingress_reset_ok(env, slot, mask_dev)) return rc;
  if (int rc = use_device(env)) return rc;
  const bk_env::IngressSnapshot& s = env->isnaps[slot];
  const uint32_t n_units = env->cfg.n_books / env->M;
  if (int rc = reset_books_from(env, s.buf.p, s.stamp_bound, mask_dev, seeds_dev)) return rc;
  uint32_t* counter = env->reset_list.p + n_units;
  HIPCHK(hipMemsetAsync(counter, 0, 4, env->stream));
  // (after a bk_set_*agents* call and before the next update the env's own rows are stale and are re-made by that update;
  // the install count has refused every slot that holds rows by then)
  const bool held = held_active(env) && !env->agent_held_stale, members = members_active(env) && !env->member_lists_stale;
  reset::CollectArgs c{};
  c.mask = mask_dev;
  c.n_units = n_units;
  c.M = env->M;
  c.list = env->reset_list.p;
  c.count = counter;
  c.dqlen = env->dqlen.p;
  if (members) {
    c.n_members = env->n_mixed;
    c.lens = env->member_lens.p;
    c.mstate = env->member_state.p;
    c.mflags = env->member_flags.p;
    if (s.members_saved) c.snap_lens = s.lens.p, c.snap_mstate = s.mstate.p, c.snap_mflags = s.mflags.p;
  }
  hipLaunchKernelGGL(reset::k_collect_units, dim3((n_units + 255) / 256), dim3(256), 0, env->stream, c);
  HIPCHK(hipGetLastError());
  reset::RecordArgs g{};
  ingress_record_args(env, s.n_keep, g);  // (checked at the save)
  if (!held) g.n_agents = 0;
  if (!members) g.n_members = g.list_cap = 0;
  g.list = env->reset_list.p;
  g.count = counter;
  g.keep_state = s.buf.p;
  g.dst_orders = reinterpret_cast<bk_u32x4*>(env->dorders.p);
  g.src_orders = reinterpret_cast<const bk_u32x4*>(s.orders.p);
  g.dst_log = reinterpret_cast<bk_u32x4*>(env->order_log.p);
  g.src_log = reinterpret_cast<const bk_u32x4*>(s.log.p);
  g.dst_ids = env->cfg.max_orders;
  g.src_ids = s.n_keep;
  g.held = env->agent_held.p;
  g.snap_held = s.held_saved ? s.held.p : nullptr;
  g.lists = env->member_lists.p;
  g.snap_lists = s.members_saved ? s.lists.p : nullptr;
  g.snap_lens = s.members_saved ? s.lens.p : nullptr;
  hipLaunchKernelGGL(reset::k_reset_records, dim3(env->reset_blocks), dim3(64 * reset::RECORD_WAVES), 0, env->stream, g);
  HIPCHK(hipGetLastError());
  if (env->acct_traders) {  // trader accounts are not part of a snapshot: a reset book counts from its reset
    launch_accounts_clear(env, mask_dev, env->M);
    HIPCHK(hipGetLastError());
  }
  if (env->bars_window) {  // trade bars are not part of a snapshot either: zero rows, the cursor at the restored count
    launch_bars_clear(env, mask_dev, env->M);
    HIPCHK(hipGetLastError());
  }
  // the flow table's sums go on across episodes: only the cut, the cursor at the restored count.  (reset_books_from has made
  // this cut already, with the same mask, and nothing between there and here moves H_TRADES: the launch is kept beside the
  // bars' and the accounts' as the place where whatever this entry later restores of a book's trade count is followed.)
  if (env->flow_lags) {
    launch_flow_clear(env, mask_dev, env->M, true);
    HIPCHK(hipGetLastError());
  }
  if (env->open_traders) {  // the reset books show the snapshot's resting orders before their next step
    launch_open_refresh(env, mask_dev, env->M);
    HIPCHK(hipGetLastError());
  }
  env->ingest_epoch += 1;  // the readers' mirrors of the orders and the log fetch from the device again
  return BK_OK;
}

int bk_ingress_reset_books(bk_env* env, uint32_t slot, const uint8_t* mask_host, const uint64_t* seeds_host) {
  if (int rc = ingress_reset_ok(env, slot, mask_host)) return rc;
  return reset_from_host(env, slot, mask_host, seeds_host, bk_ingress_reset_books_device);
}

// ------------------------------------------------------------------ trader accounts of a device-ingress env
// No counterpart in the reference.  acct[n_books][n_traders] rows {position, cash, volume, fills} folded from each step's
// new trade records by accounts::k_fold behind the step's event kernel (bk_step_async); accounts.hpp, DESIGN.md 2.16.
int bk_accounts_enable(bk_env* env, uint32_t n_traders, int consume_trades) {
  if (!env) return fail(BK_INVALID_ARGUMENT, "null env");
  if (!env->device_ingress)
    return fail(BK_INVALID_ARGUMENT, "trader accounts serve an env with the device ingress (bk_device_ingress_enable): only "
                                     "there are the orders' trader ids in device memory");
  if (env->acct_traders) return fail(BK_INVALID_ARGUMENT, "trader accounts are already enabled on this env");
  if (n_traders == 0 || n_traders > accounts::MAX_TRADERS)
    return fail(BK_INVALID_ARGUMENT, "n_traders must be in 1..65536");
  if (env->cfg.max_orders == 0)
    return fail(BK_INVALID_ARGUMENT, "trader accounts need max_orders > 0: a trade record's traders are looked up in the "
                                     "order records");
  if (env->steps_done != 0 || env->ingest_epoch != 0)
    return fail(BK_INVALID_ARGUMENT, "enable trader accounts before the first instruction, update or step");
  for (const bk_env::IngressSnapshot& s : env->isnaps)
    if (s.used) return fail(BK_INVALID_ARGUMENT, "enable trader accounts while no ingress snapshot slot is held");
  if (int rc = use_device(env)) return rc;
  const size_t B = env->cfg.n_books;
  DevBuf<bk_u32x4> rows;
  DevBuf<unsigned long long> seen;
  HIPCHK(rows.alloc(B * n_traders * 2));
  HIPCHK(seen.alloc(B));
  env->acct.swap(rows);
  env->acct_seen.swap(seen);
  env->acct_traders = n_traders;
  env->acct_consume = consume_trades != 0;
  launch_accounts_clear(env, nullptr, 1);
  HIPCHK(hipGetLastError());
  return BK_OK;
}

static int accounts_ok(bk_env* env) {
  if (!env) return fail(BK_INVALID_ARGUMENT, "null env");
  if (!env->acct_traders) return fail(BK_INVALID_ARGUMENT, "this env has no trader accounts: call bk_accounts_enable first");
  return BK_OK;
}

int bk_accounts_device_ptr(bk_env* env, void** out) {
  if (int rc = accounts_ok(env)) return rc;
  if (!out) return fail(BK_INVALID_ARGUMENT, "null argument");
  *out = env->acct.p;
  return BK_OK;
}

int bk_get_accounts(bk_env* env, uint32_t first_book, uint32_t n_books, bk_account* out) {
  if (int rc = accounts_ok(env)) return rc;
  return get_book_rows(env, first_book, n_books, {{env->acct.p, env->acct_traders * sizeof(bk_account), out}});
}

int bk_accounts_clear_device(bk_env* env, const uint8_t* mask_dev) {
  if (int rc = accounts_ok(env)) return rc;
  if (int rc = use_device(env)) return rc;
  launch_accounts_clear(env, mask_dev, 1);
  HIPCHK(hipGetLastError());
  return BK_OK;
}

int bk_accounts_clear(bk_env* env, const uint8_t* mask_host) {
  if (int rc = accounts_ok(env)) return rc;
  return clear_from_host(env, mask_host, env->acct_mask, bk_accounts_clear_device);
}

// ------------------------------------------------------------------ trade bars of a device-ingress env
// No counterpart in the reference.  bars[n_books][window] rows {open, high, low, close, buy_vol, sell_vol, notional, n_buy,
// n_sell}: the bar of step k in slot k % window, folded from the step's new trade records by trade_bars::k_fold behind the
// step's event kernel (bk_step_async); trade_bars.hpp, DESIGN.md 2.21.
int bk_trade_bars_enable(bk_env* env, uint32_t window, int consume_trades) {
  if (!env) return fail(BK_INVALID_ARGUMENT, "null env");
  if (!env->device_ingress)
    return fail(BK_INVALID_ARGUMENT, "trade bars serve an env with the device ingress (bk_device_ingress_enable): they are "
                                     "folded behind bk_step_async");
  if (env->bars_window) return fail(BK_INVALID_ARGUMENT, "trade bars are already enabled on this env");
  if (window == 0 || window > trade_bars::MAX_WINDOW) return fail(BK_INVALID_ARGUMENT, "window must be in 1..1024 steps");
  if (int rc = use_device(env)) return rc;
  const size_t B = env->cfg.n_books;
  DevBuf<bk_u32x4> rows;
  DevBuf<unsigned long long> seen;
  HIPCHK(rows.alloc(B * window * trade_bars::ROW_VECS));
  HIPCHK(seen.alloc(B));
  env->bars.swap(rows);
  env->bars_seen.swap(seen);
  env->bars_window = window;
  env->bars_consume = consume_trades != 0;
  launch_bars_clear(env, nullptr, 1);
  HIPCHK(hipGetLastError());
  return BK_OK;
}

static int trade_bars_ok(bk_env* env) {
  if (!env) return fail(BK_INVALID_ARGUMENT, "null env");
  if (!env->bars_window) return fail(BK_INVALID_ARGUMENT, "this env has no trade bars: call bk_trade_bars_enable first");
  return BK_OK;
}

int bk_trade_bars_device_ptr(bk_env* env, void** out) {
  if (int rc = trade_bars_ok(env)) return rc;
  if (!out) return fail(BK_INVALID_ARGUMENT, "null argument");
  *out = env->bars.p;
  return BK_OK;
}

int bk_trade_bars_slot(bk_env* env, uint32_t* out) {
  if (int rc = trade_bars_ok(env)) return rc;
  if (!out) return fail(BK_INVALID_ARGUMENT, "null argument");
  *out = static_cast<uint32_t>((env->steps_done % env->bars_window + env->bars_window - 1u) % env->bars_window);
  return BK_OK;
}

int bk_get_trade_bars(bk_env* env, uint32_t first_book, uint32_t n_books, bk_trade_bar* out) {
  if (int rc = trade_bars_ok(env)) return rc;
  return get_book_rows(env, first_book, n_books, {{env->bars.p, env->bars_window * sizeof(bk_trade_bar), out}});
}

int bk_trade_bars_clear_device(bk_env* env, const uint8_t* mask_dev) {
  if (int rc = trade_bars_ok(env)) return rc;
  if (int rc = use_device(env)) return rc;
  launch_bars_clear(env, mask_dev, 1);
  HIPCHK(hipGetLastError());
  return BK_OK;
}

int bk_trade_bars_clear(bk_env* env, const uint8_t* mask_host) {
  if (int rc = trade_bars_ok(env)) return rc;
  return clear_from_host(env, mask_host, env->bars_mask, bk_trade_bars_clear_device);
}

// ------------------------------------------------------------------ the flow table of the trade records
// No counterpart in the reference.  table[n_books][8 + 6 K] u64 words - the base words, then K lag rows in trade time -
// folded from each book's trade records by flow::k_fold from a per-book device cursor; flow.hpp, DESIGN.md 2.26.
int bk_flow_enable(bk_env* env, uint32_t n_lags, int consume_trades) {
  if (!env) return fail(BK_INVALID_ARGUMENT, "null env");
  if (!env->cfg.trade_capacity)
    return fail(BK_INVALID_ARGUMENT, "the flow table is folded from the trade records: trade_capacity must be > 0");
  if (n_lags == 0 || n_lags > flow::MAX_LAGS) return fail(BK_INVALID_ARGUMENT, "n_lags must be in 1..64");
  if (env->flow_lags) return fail(BK_INVALID_ARGUMENT, "the flow table is already enabled on this env");
  if (int rc = use_device(env)) return rc;
  const size_t B = env->cfg.n_books;
  DevBuf<bk_u32x4> table;
  DevBuf<uint64_t> carry;
  DevBuf<unsigned long long> seen;
  HIPCHK(table.alloc(B * flow::book_vecs(n_lags)));
  HIPCHK(carry.alloc(B * n_lags));
  HIPCHK(seen.alloc(B));
  env->flow_table.swap(table);
  env->flow_carry.swap(carry);
  env->flow_seen.swap(seen);
  env->flow_lags = n_lags;
  env->flow_consume = consume_trades != 0;
  launch_flow_clear(env, nullptr, 1, false);
  const hipError_t launched = hipGetLastError();
  if (launched == hipSuccess) return BK_OK;
  env->flow_table.swap(table);  // the env stays without the table: the new blocks leave with the locals
  env->flow_carry.swap(carry);
  env->flow_seen.swap(seen);
  env->flow_lags = 0;
  env->flow_consume = false;
  return fail(BK_HIP_ERROR, std::string("bk_flow_enable: the clear could not be launched: ") + hipGetErrorString(launched));
}

static int flow_ok(bk_env* env) {
  if (!env) return fail(BK_INVALID_ARGUMENT, "null env");
  if (!env->flow_lags) return fail(BK_INVALID_ARGUMENT, "this env has no flow table: call bk_flow_enable first");
  return BK_OK;
}

int bk_flow_fold(bk_env* env) {
  if (int rc = flow_ok(env)) return rc;
  if (int rc = use_device(env)) return rc;
  launch_flow_fold(env, env->flow_consume);
  HIPCHK(hipGetLastError());
  return BK_OK;
}

int bk_flow_clear_device(bk_env* env, const uint8_t* mask_dev) {
  if (int rc = flow_ok(env)) return rc;
  if (int rc = use_device(env)) return rc;
  if (mask_dev) {  // (without a mask nothing is folded: every book starts again at its H_TRADES)
    launch_flow_fold(env, env->flow_consume);
    HIPCHK(hipGetLastError());
  }
  launch_flow_clear(env, mask_dev, 1, false);
  HIPCHK(hipGetLastError());
  return BK_OK;
}

int bk_flow_clear(bk_env* env, const uint8_t* mask_host) {
  if (int rc = flow_ok(env)) return rc;
  return clear_from_host(env, mask_host, env->flow_mask, bk_flow_clear_device);
}

int bk_flow_device_ptr(bk_env* env, void** out) {
  if (int rc = flow_ok(env)) return rc;
  if (!out) return fail(BK_INVALID_ARGUMENT, "null argument");
  *out = env->flow_table.p;
  return BK_OK;
}

int bk_flow_lags(bk_env* env, uint32_t* out) {
  if (int rc = flow_ok(env)) return rc;
  if (!out) return fail(BK_INVALID_ARGUMENT, "null argument");
  *out = env->flow_lags;
  return BK_OK;
}

int bk_get_flow(bk_env* env, uint32_t first_book, uint32_t n_books, uint64_t* out) {
  if (int rc = flow_ok(env)) return rc;
  return get_book_rows(env, first_book, n_books, {{env->flow_table.p, flow::table_words(env->flow_lags) * sizeof(uint64_t), out}});
}

// carry and cursors of books [first_book, first_book + n_books): what a test compares between differently cut folds
int bk_get_flow_state(bk_env* env, uint32_t first_book, uint32_t n_books, uint64_t* carry, uint64_t* seen) {
  if (int rc = flow_ok(env)) return rc;
  if (!seen) return fail(BK_INVALID_ARGUMENT, "null argument");
  return get_book_rows(env, first_book, n_books, {{env->flow_seen.p, sizeof(uint64_t), seen},
                                                  {env->flow_carry.p, env->flow_lags * sizeof(uint64_t), carry}});
}

// ------------------------------------------------------------------ the tables folded from the history ring: the entries
// (the launches, the lost-step check and the fold of what is outstanding stand with the history ring above)
// table `which`: one of the three per-book tables, or T_CROSS, the per-market one beside them
static HistTable& table_at(bk_env* env, int which) { return which == T_CROSS ? env->cross_table : env->tables[which]; }

// the guard of every entry but the enable
static int table_ok(bk_env* env, int which) {
  if (!env) return fail(BK_INVALID_ARGUMENT, "null env");
  const HistTable& t = table_at(env, which);
  if (!t.on) return fail(BK_INVALID_ARGUMENT, std::string("this env has no ") + t.name + ": call bk_" + t.prefix + "_enable first");
  return BK_OK;
}

static int table_fold(bk_env* env, int which) {
  if (int rc = table_ok(env, which)) return rc;
  return table_fold_outstanding(env, table_at(env, which));
}

static int table_clear_device(bk_env* env, int which, const uint8_t* mask_dev) {
  if (int rc = table_ok(env, which)) return rc;
  if (int rc = use_device(env)) return rc;
  HistTable& t = table_at(env, which);
  if (mask_dev) {
    if (int rc = table_fold_outstanding(env, t)) return rc;
    t.clear(env, mask_dev, t.clear_M, false);
  } else {
    table_start_again(env, t);  // nothing is folded
  }
  HIPCHK(hipGetLastError());
  return BK_OK;
}

static int table_clear(bk_env* env, int which, const uint8_t* mask_host, int (*device_form)(bk_env*, const uint8_t*)) {
  if (int rc = table_ok(env, which)) return rc;
  if (mask_host)
    if (int rc = table_lost_check(env, table_at(env, which))) return rc;  // (refused before the mask is staged)
  return clear_from_host(env, mask_host, table_at(env, which).mask, device_form, table_at(env, which).clear_M);
}

// ------------------------------------------------------------------ per-book series moments
int bk_series_enable(bk_env* env) {
  if (!env) return fail(BK_INVALID_ARGUMENT, "null env");
  if (!env->cfg.history_capacity)
    return fail(BK_INVALID_ARGUMENT, "the series moments are folded from the level-2 history ring: history_capacity must be > 0");
  if (env->tables[T_SERIES].on) return fail(BK_INVALID_ARGUMENT, "the series moments are already enabled on this env");
  if (int rc = use_device(env)) return rc;
  DevBuf<bk_u32x4> rows;
  HIPCHK(rows.alloc(static_cast<size_t>(env->cfg.n_books) * series::ROW_VECS));
  env->series_rows.swap(rows);
  const int rc = table_commit_enable(env, env->tables[T_SERIES]);
  if (rc) env->series_rows.swap(rows);  // the env stays without the table: the new block leaves with `rows`
  return rc;
}

int bk_series_fold(bk_env* env) { return table_fold(env, T_SERIES); }
int bk_series_clear_device(bk_env* env, const uint8_t* mask_dev) { return table_clear_device(env, T_SERIES, mask_dev); }
int bk_series_clear(bk_env* env, const uint8_t* mask_host) { return table_clear(env, T_SERIES, mask_host, bk_series_clear_device); }

int bk_series_device_ptr(bk_env* env, void** out) {
  if (int rc = table_ok(env, T_SERIES)) return rc;
  if (!out) return fail(BK_INVALID_ARGUMENT, "null argument");
  *out = env->series_rows.p;
  return BK_OK;
}

int bk_get_series(bk_env* env, uint32_t first_book, uint32_t n_books, bk_series_row* out) {
  if (int rc = table_ok(env, T_SERIES)) return rc;
  return get_book_rows(env, first_book, n_books, {{env->series_rows.p, sizeof(bk_series_row), out}});
}

// ------------------------------------------------------------------ per-book depth table, the series' companion
// No counterpart in the reference.  depth_rows[n_books][levels + 1] rows of 16 u64 words and depth_carry[n_books][levels + 1]
// (depth.hpp): no HistTable of its own - the series' cursor, fold, clear and cut act on both tables.
static int depth_ok(bk_env* env) {
  if (!env) return fail(BK_INVALID_ARGUMENT, "null env");
  if (!env->depth_rows.p) return fail(BK_INVALID_ARGUMENT, "this env has no depth table: call bk_depth_enable first");
  return BK_OK;
}

int bk_depth_enable(bk_env* env) {
  if (!env) return fail(BK_INVALID_ARGUMENT, "null env");
  if (!env->tables[T_SERIES].on)
    return fail(BK_INVALID_ARGUMENT, "the depth table is the series moments' companion and shares their cursor: call bk_series_enable first");
  if (env->depth_rows.p) return fail(BK_INVALID_ARGUMENT, "the depth table is already enabled on this env");
  static_assert(depth::MAX_LEVELS == 64, "cfg.levels is 1..64");
  // the series' outstanding steps first (lost steps refuse, the env unchanged): both tables then stand at steps_done
  if (int rc = table_fold(env, T_SERIES)) return rc;
  if (int rc = use_device(env)) return rc;
  const size_t rows_per_book = env->cfg.levels + 1u;
  DevBuf<bk_u32x4> rows;
  DevBuf<uint64_t> carry;
  HIPCHK(rows.alloc(static_cast<size_t>(env->cfg.n_books) * rows_per_book * depth::ROW_VECS));
  HIPCHK(carry.alloc(static_cast<size_t>(env->cfg.n_books) * rows_per_book));
  depth::ClearArgs d{};
  d.books = masked_books(env, nullptr, 1);
  d.L = env->cfg.levels;
  d.carry_only = 0u;
  d.rows = rows.p;
  d.carry = carry.p;
  launch_wave_per_book(env, depth::k_clear, depth::FOLD_WAVES, d.books.n_books, d);
  const hipError_t launched = hipGetLastError();
  if (launched != hipSuccess)  // the env stays without the table: the new blocks leave with `rows` and `carry`
    return fail(BK_HIP_ERROR, std::string("bk_depth_enable: the clear could not be launched: ") + hipGetErrorString(launched));
  env->depth_rows.swap(rows);
  env->depth_carry.swap(carry);
  return BK_OK;
}

int bk_depth_device_ptr(bk_env* env, void** out) {
  if (int rc = depth_ok(env)) return rc;
  if (!out) return fail(BK_INVALID_ARGUMENT, "null argument");
  *out = env->depth_rows.p;
  return BK_OK;
}

int bk_get_depth(bk_env* env, uint32_t first_book, uint32_t n_books, uint64_t* out) {
  if (int rc = depth_ok(env)) return rc;
  return get_book_rows(env, first_book, n_books,
                       {{env->depth_rows.p, (env->cfg.levels + 1u) * static_cast<size_t>(depth::ROW_WORDS) * sizeof(uint64_t), out}});
}

// ------------------------------------------------------------------ per-book candle table, the series' companion
// No counterpart in the reference.  candle_rows[n_books][candle_n] rows of 16 u64 words and candle_carry[n_books]
// (candles.hpp): no HistTable of its own - the series' cursor, fold, clear and cut act on it too.
static int candles_ok(bk_env* env) {
  if (!env) return fail(BK_INVALID_ARGUMENT, "null env");
  if (!env->candle_rows.p) return fail(BK_INVALID_ARGUMENT, "this env has no candle table: call bk_candles_enable first");
  return BK_OK;
}

int bk_candles_enable(bk_env* env, uint32_t width, uint32_t n_candles) {
  if (!env) return fail(BK_INVALID_ARGUMENT, "null env");
  if (!env->tables[T_SERIES].on)
    return fail(BK_INVALID_ARGUMENT, "the candle table is the series moments' companion and shares their cursor: call bk_series_enable first");
  if (env->candle_rows.p) return fail(BK_INVALID_ARGUMENT, "the candle table is already enabled on this env");
  if (width < 1u || width > candles::MAX_WIDTH) return fail(BK_INVALID_ARGUMENT, "width must be in 1..1048576 steps a bar");
  if (n_candles < 1u || n_candles > candles::MAX_CANDLES) return fail(BK_INVALID_ARGUMENT, "n_candles must be in 1..65536 bars a book");
  // the series' outstanding steps first (lost steps refuse, the env unchanged): both tables then stand at steps_done
  if (int rc = table_fold(env, T_SERIES)) return rc;
  if (int rc = use_device(env)) return rc;
  DevBuf<bk_u32x4> rows;
  DevBuf<uint64_t> carry;
  HIPCHK(rows.alloc(static_cast<size_t>(env->cfg.n_books) * n_candles * candles::ROW_VECS));
  HIPCHK(carry.alloc(static_cast<size_t>(env->cfg.n_books)));
  candles::ClearArgs c{};
  c.books = masked_books(env, nullptr, 1);
  c.N = n_candles;
  c.carry_only = 0u;
  c.rows = rows.p;
  c.carry = carry.p;
  launch_wave_per_book(env, candles::k_clear, candles::FOLD_WAVES, c.books.n_books, c);
  const hipError_t launched = hipGetLastError();
  if (launched != hipSuccess)  // the env stays without the table: the new blocks leave with `rows` and `carry`
    return fail(BK_HIP_ERROR, std::string("bk_candles_enable: the clear could not be launched: ") + hipGetErrorString(launched));
  env->candle_rows.swap(rows);
  env->candle_carry.swap(carry);
  env->candle_width = width;
  env->candle_n = n_candles;
  return BK_OK;
}

int bk_candles_config_get(bk_env* env, uint32_t out[2]) {
  if (int rc = candles_ok(env)) return rc;
  if (!out) return fail(BK_INVALID_ARGUMENT, "null argument");
  out[0] = env->candle_width, out[1] = env->candle_n;
  return BK_OK;
}

int bk_candles_device_ptr(bk_env* env, void** out) {
  if (int rc = candles_ok(env)) return rc;
  if (!out) return fail(BK_INVALID_ARGUMENT, "null argument");
  *out = env->candle_rows.p;
  return BK_OK;
}

int bk_get_candles(bk_env* env, uint32_t first_book, uint32_t n_books, uint64_t* out) {
  if (int rc = candles_ok(env)) return rc;
  return get_book_rows(env, first_book, n_books,
                       {{env->candle_rows.p, env->candle_n * static_cast<size_t>(candles::ROW_WORDS) * sizeof(uint64_t), out}});
}

// ------------------------------------------------------------------ per-book lag table
int bk_lags_enable(bk_env* env, uint32_t n_lags) {
  if (!env) return fail(BK_INVALID_ARGUMENT, "null env");
  if (!env->cfg.history_capacity)
    return fail(BK_INVALID_ARGUMENT, "the lag table is folded from the level-2 history ring: history_capacity must be > 0");
  if (n_lags == 0 || n_lags > lags::MAX_LAGS) return fail(BK_INVALID_ARGUMENT, "n_lags must be in 1..64");
  if (env->tables[T_LAGS].on) return fail(BK_INVALID_ARGUMENT, "the lag table is already enabled on this env");
  if (int rc = use_device(env)) return rc;
  DevBuf<bk_u32x4> rows;
  DevBuf<uint64_t> carry;
  HIPCHK(rows.alloc(static_cast<size_t>(env->cfg.n_books) * n_lags * lags::ROW_VECS));
  HIPCHK(carry.alloc(static_cast<size_t>(env->cfg.n_books) * (n_lags + 1u)));
  env->lag_rows.swap(rows);
  env->lag_carry.swap(carry);
  env->n_lags = n_lags;
  const int rc = table_commit_enable(env, env->tables[T_LAGS]);
  if (rc) {  // the env stays without the table: the new blocks leave with `rows` and `carry`
    env->lag_rows.swap(rows);
    env->lag_carry.swap(carry);
    env->n_lags = 0;
  }
  return rc;
}

int bk_lags_fold(bk_env* env) { return table_fold(env, T_LAGS); }
int bk_lags_clear_device(bk_env* env, const uint8_t* mask_dev) { return table_clear_device(env, T_LAGS, mask_dev); }
int bk_lags_clear(bk_env* env, const uint8_t* mask_host) { return table_clear(env, T_LAGS, mask_host, bk_lags_clear_device); }

int bk_lags_device_ptr(bk_env* env, void** out) {
  if (int rc = table_ok(env, T_LAGS)) return rc;
  if (!out) return fail(BK_INVALID_ARGUMENT, "null argument");
  *out = env->lag_rows.p;
  return BK_OK;
}

int bk_get_lags(bk_env* env, uint32_t first_book, uint32_t n_books, bk_lag_row* out) {
  if (int rc = table_ok(env, T_LAGS)) return rc;
  return get_book_rows(env, first_book, n_books, {{env->lag_rows.p, env->n_lags * sizeof(bk_lag_row), out}});
}

// ------------------------------------------------------------------ per-book bin table
static const char* bins_config_fault(const bk_bins_config& c) {
  if (c.n_bins < 2u || c.n_bins > bins::MAX_BINS || c.n_bins % 2u) return "n_bins must be even and in 2..256";
  if (c.n_spans < 1u || c.n_spans > bins::MAX_SPANS) return "n_spans must be in 1..4";
  for (uint32_t j = 0; j < c.n_spans; ++j)
    if (c.spans[j] < 1u || c.spans[j] > bins::MAX_SPAN) return "every used span must be in 1..64";
  if (!c.ret_width || !c.spread_width || !c.vol_width) return "ret_width, spread_width and vol_width must be >= 1";
  return nullptr;
}

int bk_bins_enable(bk_env* env, const bk_bins_config* cfg) {
  if (!env) return fail(BK_INVALID_ARGUMENT, "null env");
  if (!cfg) return fail(BK_INVALID_ARGUMENT, "null argument");
  if (!env->cfg.history_capacity)
    return fail(BK_INVALID_ARGUMENT, "the bin table is folded from the level-2 history ring: history_capacity must be > 0");
  if (const char* why = bins_config_fault(*cfg)) return fail(BK_INVALID_ARGUMENT, why);
  if (env->tables[T_BINS].on) return fail(BK_INVALID_ARGUMENT, "the bin table is already enabled on this env");
  if (int rc = use_device(env)) return rc;
  bk_bins_config c = *cfg;
  uint32_t kmax = 0;
  for (uint32_t j = 0; j < bins::MAX_SPANS; ++j) {
    if (j >= c.n_spans) c.spans[j] = 0u;
    kmax = std::max(kmax, c.spans[j]);
  }
  DevBuf<uint64_t> rows, carry;
  HIPCHK(rows.alloc(static_cast<size_t>(env->cfg.n_books) * (c.n_spans + 2u) * c.n_bins));
  HIPCHK(carry.alloc(static_cast<size_t>(env->cfg.n_books) * kmax));
  env->bin_rows.swap(rows);
  env->bins_carry.swap(carry);
  env->bins_cfg = c;
  env->bins_kmax = kmax;
  const int rc = table_commit_enable(env, env->tables[T_BINS]);
  if (rc) {  // the env stays without the table: the new blocks leave with `rows` and `carry`
    env->bin_rows.swap(rows);
    env->bins_carry.swap(carry);
    env->bins_cfg = bk_bins_config{};
    env->bins_kmax = 0;
  }
  return rc;
}

int bk_bins_config_get(bk_env* env, bk_bins_config* out) {
  if (int rc = table_ok(env, T_BINS)) return rc;
  if (!out) return fail(BK_INVALID_ARGUMENT, "null argument");
  *out = env->bins_cfg;
  return BK_OK;
}

int bk_bins_fold(bk_env* env) { return table_fold(env, T_BINS); }
int bk_bins_clear_device(bk_env* env, const uint8_t* mask_dev) { return table_clear_device(env, T_BINS, mask_dev); }
int bk_bins_clear(bk_env* env, const uint8_t* mask_host) { return table_clear(env, T_BINS, mask_host, bk_bins_clear_device); }

int bk_bins_device_ptr(bk_env* env, void** out) {
  if (int rc = table_ok(env, T_BINS)) return rc;
  if (!out) return fail(BK_INVALID_ARGUMENT, "null argument");
  *out = env->bin_rows.p;
  return BK_OK;
}

int bk_get_bins(bk_env* env, uint32_t first_book, uint32_t n_books, uint64_t* out) {
  if (int rc = table_ok(env, T_BINS)) return rc;
  const size_t per_book = static_cast<size_t>(env->bins_cfg.n_spans + 2u) * env->bins_cfg.n_bins * sizeof(uint64_t);
  return get_book_rows(env, first_book, n_books, {{env->bin_rows.p, per_book, out}});
}

// ------------------------------------------------------------------ per-market cross table
static const char* cross_config_fault(const bk_cross_config& c) {
  if (c.n_spans < 1u || c.n_spans > cross::MAX_SPANS) return "n_spans must be in 1..4";
  for (uint32_t j = 0; j < c.n_spans; ++j)
    if (c.spans[j] < 1u || c.spans[j] > cross::MAX_SPAN) return "every used span must be in 1..64";
  return nullptr;
}

int bk_cross_enable(bk_env* env, const bk_cross_config* cfg) {
  if (!env) return fail(BK_INVALID_ARGUMENT, "null env");
  if (!cfg) return fail(BK_INVALID_ARGUMENT, "null argument");
  if (!env->cfg.history_capacity)
    return fail(BK_INVALID_ARGUMENT, "the cross table is folded from the level-2 history ring: history_capacity must be > 0");
  if (env->M < 2u)
    return fail(BK_INVALID_ARGUMENT, "the cross table couples the assets of a market: it needs an env of markets with assets >= 2, "
                                     "not an env of independent books (assets == 1)");
  if (const char* why = cross_config_fault(*cfg)) return fail(BK_INVALID_ARGUMENT, why);
  if (env->cross_table.on) return fail(BK_INVALID_ARGUMENT, "the cross table is already enabled on this env");
  if (int rc = use_device(env)) return rc;
  bk_cross_config c = *cfg;
  uint32_t hmax = 0;
  for (uint32_t j = 0; j < cross::MAX_SPANS; ++j) {
    if (j >= c.n_spans) c.spans[j] = 0u;
    hmax = std::max(hmax, c.spans[j]);
  }
  const size_t markets = env->cfg.n_books / env->M;
  DevBuf<bk_u32x4> rows;
  DevBuf<uint64_t> carry;
  HIPCHK(rows.alloc(markets * cross::units(c.n_spans, env->M) * cross::ROW_VECS));
  HIPCHK(carry.alloc(markets * env->M * cross::carry_words(hmax)));
  env->cross_rows.swap(rows);
  env->cross_carry.swap(carry);
  env->cross_cfg = c;
  env->cross_hmax = hmax;
  env->cross_table.clear_M = env->M;  // its own clear's mask holds one byte per market, as a reset's
  const int rc = table_commit_enable(env, env->cross_table);
  if (rc) {  // the env stays without the table: the new blocks leave with `rows` and `carry`
    env->cross_rows.swap(rows);
    env->cross_carry.swap(carry);
    env->cross_cfg = bk_cross_config{};
    env->cross_hmax = 0;
    env->cross_table.clear_M = 1;
  }
  return rc;
}

int bk_cross_config_get(bk_env* env, bk_cross_config* out) {
  if (int rc = table_ok(env, T_CROSS)) return rc;
  if (!out) return fail(BK_INVALID_ARGUMENT, "null argument");
  *out = env->cross_cfg;
  return BK_OK;
}

int bk_cross_fold(bk_env* env) { return table_fold(env, T_CROSS); }
int bk_cross_clear_device(bk_env* env, const uint8_t* mask_dev) { return table_clear_device(env, T_CROSS, mask_dev); }
int bk_cross_clear(bk_env* env, const uint8_t* mask_host) { return table_clear(env, T_CROSS, mask_host, bk_cross_clear_device); }

int bk_cross_device_ptr(bk_env* env, void** out) {
  if (int rc = table_ok(env, T_CROSS)) return rc;
  if (!out) return fail(BK_INVALID_ARGUMENT, "null argument");
  *out = env->cross_rows.p;
  return BK_OK;
}

// the rows of markets [first_market, first_market + n_markets) -> host (an empty range may start behind the last market)
int bk_get_cross(bk_env* env, uint32_t first_market, uint32_t n_markets, bk_cross_row* out) {
  if (int rc = table_ok(env, T_CROSS)) return rc;
  const uint32_t markets = env->cfg.n_books / env->M;
  if (first_market > markets || n_markets > markets - first_market) return fail(BK_INVALID_ARGUMENT, "market range out of bounds");
  if (n_markets && !out) return fail(BK_INVALID_ARGUMENT, "null argument");
  if (int rc = use_device(env)) return rc;
  HIPCHK(hipStreamSynchronize(env->stream));
  const size_t market_bytes = static_cast<size_t>(cross::units(env->cross_cfg.n_spans, env->M)) * sizeof(bk_cross_row);
  if (n_markets)
    HIPCHK(hipMemcpy(out, reinterpret_cast<const char*>(env->cross_rows.p) + first_market * market_bytes, n_markets * market_bytes,
                     hipMemcpyDeviceToHost));
  return BK_OK;
}

// ------------------------------------------------------------------ open orders of a device-ingress env
// No counterpart in the reference.  summary[n_books][n_traders] and entries[n_books][n_traders][depth]: every trader's resting
// orders per book, recomputed from the pool by open_orders::k_refresh behind every step's event kernel (bk_step_async) and
// behind bk_ingress_reset_books*; open_orders.hpp, DESIGN.md 2.17.
int bk_open_orders_enable(bk_env* env, uint32_t n_traders, uint32_t depth) {
  if (!env) return fail(BK_INVALID_ARGUMENT, "null env");
  if (!env->device_ingress)
    return fail(BK_INVALID_ARGUMENT, "the open-order view serves an env with the device ingress (bk_device_ingress_enable): "
                                     "only there are the orders' trader ids in device memory");
  if (env->open_traders) return fail(BK_INVALID_ARGUMENT, "the open-order view is already enabled on this env");
  if (n_traders == 0 || n_traders > open_orders::MAX_TRADERS)
    return fail(BK_INVALID_ARGUMENT, "n_traders must be in 1..65536");
  if (depth > open_orders::MAX_DEPTH) return fail(BK_INVALID_ARGUMENT, "depth must be in 0..64 entries per trader and book");
  if (env->cfg.max_orders == 0)
    return fail(BK_INVALID_ARGUMENT, "the open-order view needs max_orders > 0: a resting order's trader is looked up in the "
                                     "order records");
  if (int rc = use_device(env)) return rc;
  const size_t rows = static_cast<size_t>(env->cfg.n_books) * n_traders;
  DevBuf<bk_u32x4> summary, entries;
  HIPCHK(summary.alloc(rows * 2));
  HIPCHK(entries.alloc(rows * depth));
  env->open_summary.swap(summary);
  env->open_entries.swap(entries);
  env->open_traders = n_traders;
  env->open_depth = depth;
  launch_open_refresh(env, nullptr, 1);
  HIPCHK(hipGetLastError());
  return BK_OK;
}

static int open_orders_ok(bk_env* env) {
  if (!env) return fail(BK_INVALID_ARGUMENT, "null env");
  if (!env->open_traders)
    return fail(BK_INVALID_ARGUMENT, "this env has no open-order view: call bk_open_orders_enable first");
  return BK_OK;
}

int bk_open_orders_refresh(bk_env* env) {
  if (int rc = open_orders_ok(env)) return rc;
  if (int rc = use_device(env)) return rc;
  launch_open_refresh(env, nullptr, 1);
  HIPCHK(hipGetLastError());
  return BK_OK;
}

int bk_open_orders_device_ptrs(bk_env* env, void** summary, void** entries) {
  if (int rc = open_orders_ok(env)) return rc;
  if (!summary || !entries) return fail(BK_INVALID_ARGUMENT, "null argument");
  *summary = env->open_summary.p;
  *entries = env->open_entries.p;  // (nullptr with depth == 0)
  return BK_OK;
}

int bk_get_open_orders(bk_env* env, uint32_t first_book, uint32_t n_books, bk_open_summary* summary_out,
                       bk_open_order* entries_out) {
  if (int rc = open_orders_ok(env)) return rc;
  const size_t entries = static_cast<size_t>(env->open_traders) * env->open_depth;  // (per book; none with depth == 0)
  return get_book_rows(env, first_book, n_books, {{env->open_summary.p, env->open_traders * sizeof(bk_open_summary), summary_out},
                                                  {env->open_entries.p, entries * sizeof(bk_open_order), entries_out}});
}

// ------------------------------------------------------------------ queue positions of the open orders
// No counterpart in the reference.  queue[n_books][n_traders][depth], one row per entry of the open-order view: the volume and
// the orders with priority over it, recomputed from the pool by open_queue::k_refresh right behind open_orders::k_refresh
// wherever that runs; open_queue.hpp, DESIGN.md 2.19.
int bk_open_queue_enable(bk_env* env) {
  if (!env) return fail(BK_INVALID_ARGUMENT, "null env");
  if (!env->open_traders)
    return fail(BK_INVALID_ARGUMENT, "the queue view has one row per entry of the open-order view: call bk_open_orders_enable first");
  if (env->open_depth == 0)
    return fail(BK_INVALID_ARGUMENT, "the queue view needs depth > 0: the open-order view of this env keeps no entries");
  if (env->open_queue.p) return fail(BK_INVALID_ARGUMENT, "the queue view is already enabled on this env");
  if (int rc = use_device(env)) return rc;
  DevBuf<bk_u32x4> queue;
  HIPCHK(queue.alloc(static_cast<size_t>(env->cfg.n_books) * env->open_traders * env->open_depth * 2));
  env->open_queue.swap(queue);
  launch_open_refresh(env, nullptr, 1);
  HIPCHK(hipGetLastError());
  return BK_OK;
}

static int open_queue_ok(bk_env* env) {
  if (!env) return fail(BK_INVALID_ARGUMENT, "null env");
  if (!env->open_queue.p) return fail(BK_INVALID_ARGUMENT, "this env has no queue view: call bk_open_queue_enable first");
  return BK_OK;
}

int bk_open_queue_device_ptr(bk_env* env, void** out) {
  if (int rc = open_queue_ok(env)) return rc;
  if (!out) return fail(BK_INVALID_ARGUMENT, "null argument");
  *out = env->open_queue.p;
  return BK_OK;
}

int bk_get_open_queue(bk_env* env, uint32_t first_book, uint32_t n_books, bk_open_queue* out) {
  if (int rc = open_queue_ok(env)) return rc;
  const size_t entries = static_cast<size_t>(env->open_traders) * env->open_depth;
  return get_book_rows(env, first_book, n_books, {{env->open_queue.p, entries * sizeof(bk_open_queue), out}});
}

// ------------------------------------------------------------------ quotes through the device ingress
// No counterpart in the reference.  quotes[n_books][n_traders], one target row per trader of the open-order view, joined with
// the view's entries and queued as cancellations, volume-only modifications and new orders by quotes::k_submit - k_ingest's
// passes over the dense grid n_traders x (depth + 2); quotes_ingress.hpp, DESIGN.md 2.20.
static int submit_quotes_ok(bk_env* env, const void* quotes) {
  if (!env) return fail(BK_INVALID_ARGUMENT, "null env");
  if (!quotes) return fail(BK_INVALID_ARGUMENT, "null quotes");
  if (!env->device_ingress) return fail(BK_INVALID_ARGUMENT, "call bk_device_ingress_enable first");
  if (!env->open_traders)
    return fail(BK_INVALID_ARGUMENT, "a quote row is joined with the trader's listed orders: call bk_open_orders_enable first");
  if (env->open_depth == 0)
    return fail(BK_INVALID_ARGUMENT, "quotes need depth > 0: the open-order view of this env keeps no entries");
  return BK_OK;
}

int bk_submit_quotes_device(bk_env* env, const bk_quote* quotes_dev, uint64_t* out_ids_dev, uint32_t* status_dev) {
  if (int rc = submit_quotes_ok(env, quotes_dev)) return rc;
  if (reinterpret_cast<uintptr_t>(quotes_dev) & 15u) return fail(BK_INVALID_ARGUMENT, "quotes must be 16-byte aligned");
  if (int rc = use_device(env)) return rc;
  quotes::SubmitArgs g{};
  g.quotes = reinterpret_cast<const bk_u32x4*>(quotes_dev);
  g.entries = env->open_entries.p;
  g.n_traders = env->open_traders;
  g.depth = env->open_depth;
  g.out_ids = reinterpret_cast<unsigned long long*>(out_ids_dev);
  g.status = status_dev;
  g.q = env->dq.p;
  g.qlen = env->dqlen.p;
  g.qcap = env->qcap;
  g.dorders = env->dorders.p;
  g.mods_flag = env->mods_flag_dev;
  const DevArgs a = env->args();
  hipLaunchKernelGGL(quotes::k_submit, dim3(env->cfg.n_books / env->M), dim3(64), 0, env->stream, a, g);
  HIPCHK(hipGetLastError());
  env->ingest_epoch += 1;
  return BK_OK;
}

int bk_submit_quotes(bk_env* env, const bk_quote* quotes, uint64_t* out_ids_dev, uint32_t* status_dev) {
  if (int rc = submit_quotes_ok(env, quotes)) return rc;
  if (int rc = use_device(env)) return rc;
  const size_t bytes = static_cast<size_t>(env->cfg.n_books) * env->open_traders * sizeof(bk_quote);
  HostStage& st = env->quote_stage;
  // (the view's shape is fixed once enabled: one size for the env's life, so no block in use is ever replaced)
  if (int rc = st.reserve(bytes, env->stream, false)) return rc;
  std::memcpy(st.pin, quotes, bytes);  // the caller's table may be reused on return
  if (int rc = st.upload(bytes, env->stream)) return rc;
  return bk_submit_quotes_device(env, reinterpret_cast<const bk_quote*>(st.dev.p), out_ids_dev, status_dev);
}

uint64_t bk_state_bytes_per_book(const bk_env* env) { return env ? static_cast<uint64_t>(env->stride) * 4 : 0; }

// DPP reduction self-test (tests only): in[n_waves*64] -> out[n_waves*4] = {min, max, sum, sel-sum}
int bk_selftest_reduce(const uint32_t* in_host, uint32_t n_waves, uint32_t* out_host) {
  if (!in_host || !out_host) return fail(BK_INVALID_ARGUMENT, "null argument");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(BK_NO_DEVICE, "no HIP device available");
  DevBuf<uint32_t> in, out;
  HIPCHK(in.alloc(static_cast<size_t>(n_waves) * 64));
  HIPCHK(out.alloc(static_cast<size_t>(n_waves) * 4));
  HIPCHK(hipMemcpy(in.p, in_host, static_cast<size_t>(n_waves) * 64 * 4, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_selftest_reduce, dim3(n_waves), dim3(64), 0, nullptr, in.p, out.p);
  HIPCHK(hipGetLastError());
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(out_host, out.p, static_cast<size_t>(n_waves) * 4 * 4, hipMemcpyDeviceToHost));
  return BK_OK;
}

// pm_math.hpp on the device (tests only): out[i] = f(in[i]), op 0 pm::exp, 1 pm::log, 2 pm::tanh - the routines the
// Noise/Momentum members' log-normal offsets and momentum signal go through (agents/common.rs:104,137;
// momentum_agent.rs:156); tests compare them with the host build of the same header bit for bit and with libm in ulps
int bk_selftest_math(int op, const double* in_host, uint64_t n, double* out_host) {
  if (!in_host || !out_host || op < 0 || op > 2) return fail(BK_INVALID_ARGUMENT, "bad argument");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(BK_NO_DEVICE, "no HIP device available");
  DevBuf<double> in, out;
  HIPCHK(in.alloc(n));
  HIPCHK(out.alloc(n));
  HIPCHK(hipMemcpy(in.p, in_host, n * sizeof(double), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_selftest_math, dim3(static_cast<uint32_t>((n + 255) / 256)), dim3(256), 0, nullptr, op, in.p, out.p, n);
  HIPCHK(hipGetLastError());
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(out_host, out.p, n * sizeof(double), hipMemcpyDeviceToHost));
  return BK_OK;
}

}  // extern "C"
