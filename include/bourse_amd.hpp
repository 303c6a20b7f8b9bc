// bourse_amd.hpp — C++17 host-side mirror of the reference's Rust surface over the C ABI (bourse_amd.h).
//
// The reference's host language is Rust; the build image has no cargo/rustc, so the compiled-language mirror of
// `bourse_de::Env`, the `Agent` trait and `sim_runner` is this header (INTEGRATION.md shows the equivalent Rust shim).
// Names, argument meaning and error behaviour follow the reference (paths relative to the reference repository):
//   Env            crates/step_sim/src/env.rs:58-295        -> bourse_amd::Env (one book of a ManyEnv)
//   OrderError     crates/order_book/src/orderbook.rs:127-142 -> bourse_amd::OrderError (the Result's Err, thrown)
//   Agent          crates/step_sim/src/agents/mod.rs:46-55   -> bourse_amd::Agent
//   sim_runner     crates/step_sim/src/runner.rs:46-69       -> bourse_amd::sim_runner
// Header-only; link libbourse_amd.so.  No CPU fallback: without a GPU the ManyEnv constructor throws.
#pragma once
#include <cstdint>
#include <optional>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "bourse_amd.h"

namespace bourse_amd {

using OrderId = uint64_t;  // usize
using Nanos = uint64_t;
using Price = uint32_t;
using Vol = uint32_t;
using TraderId = uint32_t;
using OrderCount = uint32_t;
enum class Side : uint8_t { Bid, Ask };                                   // types.rs:26-47
enum class Status : uint8_t { New, Active, Filled, Cancelled, Rejected };  // types.rs:51-75

struct OrderError : std::runtime_error {  // OrderError::PriceError { price, tick_size }
  using std::runtime_error::runtime_error;
};
struct Error : std::runtime_error {  // everything the reference would panic on / device capacities / HIP errors
  int code;
  Error(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};
inline void check(int rc) {
  if (rc == BK_OK) return;
  if (rc == BK_PRICE_NOT_TICK_MULTIPLE) throw OrderError(bk_last_error());
  throw Error(rc, bk_last_error());
}

struct Trade {  // types.rs:103-118
  Nanos t;
  Side side;
  Price price;
  Vol vol;
  OrderId active_order_id, passive_order_id;
};
struct Order {  // types.rs:79-99
  Side side;
  Status status;
  Nanos arr_time, end_time;
  Vol vol, start_vol;
  Price price;
  TraderId trader_id;
  OrderId order_id;
};
struct Level2Data {  // types.rs:272-285 with LEVELS a run-time value
  Price bid_price, ask_price;
  Vol bid_vol, ask_vol;
  std::vector<std::pair<Vol, OrderCount>> bid_price_levels, ask_price_levels;
};

class ManyEnv;

// One book of a ManyEnv with the method set of `bourse_de::Env`.  A cheap view: copy freely.
class Env {
 public:
  Env(bk_env* h, uint32_t book, uint32_t levels) : h_(h), book_(book), levels_(levels) {}
  // Env::place_order (env.rs:166-176): Err(PriceError) -> throws OrderError, nothing created or queued
  OrderId place_order(Side side, Vol vol, TraderId trader_id, std::optional<Price> price) {
    uint64_t id = 0;
    check(bk_place_order(h_, book_, side == Side::Bid, vol, trader_id, price.has_value(), price.value_or(0), &id));
    return id;
  }
  void cancel_order(OrderId id) { check(bk_cancel_order(h_, book_, id)); }  // env.rs:189-191
  void modify_order(OrderId id, std::optional<Price> new_price, std::optional<Vol> new_vol) {  // env.rs:208-219
    check(bk_modify_order(h_, book_, id, new_price.has_value(), new_price.value_or(0), new_vol.has_value(),
                          new_vol.value_or(0)));
  }
  Status order_status(OrderId id) const {  // env.rs:288-290
    uint8_t s = 0;
    check(bk_order_status(h_, book_, id, &s));
    return static_cast<Status>(s);
  }
  Level2Data level_2_data() const {  // env.rs:293-295 (the end-of-step snapshot)
    std::vector<uint32_t> w(5 + 4 * levels_);
    check(bk_level2(h_, book_, 1, w.data()));
    Level2Data d{w[1], w[2], w[4], w[3], {}, {}};
    for (uint32_t i = 0; i < levels_; ++i) {
      d.bid_price_levels.emplace_back(w[5 + 4 * i], w[6 + 4 * i]);
      d.ask_price_levels.emplace_back(w[7 + 4 * i], w[8 + 4 * i]);
    }
    return d;
  }
  Vol last_trade_vol() const {  // get_trade_vols().last()
    std::vector<uint32_t> w(5 + 4 * levels_);
    check(bk_level2(h_, book_, 1, w.data()));
    return w[0];
  }
  std::vector<Trade> get_trades() const {  // env.rs:277-280
    uint64_t total = 0, base = 0;
    check(bk_trade_count(h_, book_, &total, &base));
    std::vector<bk_trade> raw(total - base);
    if (!raw.empty()) check(bk_get_trades(h_, book_, base, raw.size(), raw.data()));
    std::vector<Trade> out;
    for (const bk_trade& t : raw)
      out.push_back(Trade{t.t, t.side_is_bid ? Side::Bid : Side::Ask, t.price, t.vol, t.active_order_id, t.passive_order_id});
    return out;
  }
  std::vector<Order> get_orders() const {  // env.rs:262-264
    uint64_t n = 0;
    check(bk_order_count(h_, book_, &n));
    std::vector<bk_order> raw(n);
    if (n) check(bk_get_orders(h_, book_, 0, n, raw.data()));
    std::vector<Order> out;
    for (const bk_order& o : raw)
      out.push_back(Order{o.side_is_bid ? Side::Bid : Side::Ask, static_cast<Status>(o.status), o.arr_time, o.end_time, o.vol,
                          o.start_vol, o.price, o.trader_id, o.order_id});
    return out;
  }
  Nanos time() const {
    uint64_t t = 0;
    check(bk_time(h_, book_, &t));
    return t;
  }
  uint32_t book() const { return book_; }

 private:
  bk_env* h_;
  uint32_t book_, levels_;
};

// B independent `Env`s stepped in lockstep on one MI355X: `Env::new(start_time, tick_size, step_size, trading)` per book,
// book b seeded seed + book_offset + b.  `env(b)` is book b's Env.
class ManyEnv {
 public:
  ManyEnv(uint32_t n_books, uint64_t seed, Nanos start_time, Price tick_size, Nanos step_size, bool trading = true,
          uint32_t levels = 10, uint32_t max_live_orders = 128, uint32_t max_orders = 1 << 14,
          uint32_t trade_capacity = 1 << 14, uint32_t history_capacity = 0, int device = 0, uint64_t book_offset = 0) {
    bk_config c{};
    c.n_books = n_books;
    c.levels = levels;
    c.start_time = start_time;
    c.tick_size = tick_size;
    c.trading = trading;
    c.step_size = step_size;
    c.seed = seed;
    c.book_offset = book_offset;
    c.max_live_orders = max_live_orders;
    c.max_orders = max_orders;
    c.trade_capacity = trade_capacity;
    c.history_capacity = history_capacity;
    c.device = device;
    check(bk_env_create(&c, &h_));
    n_books_ = n_books;
    levels_ = levels;
  }
  ~ManyEnv() { bk_env_destroy(h_); }
  ManyEnv(const ManyEnv&) = delete;
  ManyEnv& operator=(const ManyEnv&) = delete;

  Env env(uint32_t book) { return Env(h_, book, levels_); }
  uint32_t n_books() const { return n_books_; }
  void step() { check(bk_step(h_)); }                        // Env::step (env.rs:116-135) for every book
  void enable_trading() { check(bk_enable_trading(h_, 1)); }  // env.rs:138-145
  void disable_trading() { check(bk_enable_trading(h_, 0)); }
  // on-device order flow: sim_runner's loop with RandomAgents groups (runner.rs:53-68)
  void set_random_agents(const std::vector<bk_random_agents>& groups) {
    check(bk_set_random_agents(h_, static_cast<uint32_t>(groups.size()), groups.data()));
  }
  // the same with parameters per book: table[b] is book b's groups (n_agents shared by every book; bk_set_random_agents_per_book)
  void set_random_agents_per_book(const std::vector<std::vector<bk_random_agents>>& table) {
    const size_t n_groups = table.empty() ? 0 : table[0].size();
    if (table.size() != n_books_) throw Error(BK_INVALID_ARGUMENT, "the table needs one row of groups per book");
    std::vector<bk_random_agents> flat;
    flat.reserve(table.size() * n_groups);
    for (const auto& row : table) {
      if (row.size() != n_groups) throw Error(BK_INVALID_ARGUMENT, "every row of the table needs the same number of groups");
      flat.insert(flat.end(), row.begin(), row.end());
    }
    check(bk_set_random_agents_per_book(h_, static_cast<uint32_t>(n_groups), flat.data(), nullptr));
  }
  // AgentSet members with parameters per book: table[b] is book b's members (kinds and n_agents shared by every book;
  // bk_set_agents_per_book)
  void set_agents_per_book(const std::vector<std::vector<bk_agent_desc>>& table) {
    const size_t n_members = table.empty() ? 0 : table[0].size();
    if (table.size() != n_books_) throw Error(BK_INVALID_ARGUMENT, "the table needs one row of members per book");
    std::vector<bk_agent_desc> flat;
    flat.reserve(table.size() * n_members);
    for (const auto& row : table) {
      if (row.size() != n_members) throw Error(BK_INVALID_ARGUMENT, "every row of the table needs the same number of members");
      flat.insert(flat.end(), row.begin(), row.end());
    }
    check(bk_set_agents_per_book(h_, static_cast<uint32_t>(n_members), flat.data(), nullptr));
  }
  // retune: the parameters of the books mask[b] != 0 names (empty mask: every book) in the installed per-book table, in
  // place - the agents keep what they hold, nothing else changes (bk_retune_random_agents / bk_retune_agents).  rows is
  // flat, book-major: rows[b * width + j]; on the first bad entry of a masked book nothing changes and Error is thrown.
  void retune_random_agents(uint32_t n_groups, const std::vector<bk_random_agents>& rows, const std::vector<uint8_t>& mask = {}) {
    if (rows.size() != static_cast<size_t>(n_books_) * n_groups || (!mask.empty() && mask.size() != n_books_))
      throw Error(BK_INVALID_ARGUMENT, "retune: n_books x n_groups rows and one mask byte per book are needed");
    check(bk_retune_random_agents(h_, n_groups, rows.data(), mask.empty() ? nullptr : mask.data()));
  }
  void retune_agents(uint32_t n_members, const std::vector<bk_agent_desc>& rows, const std::vector<uint8_t>& mask = {}) {
    if (rows.size() != static_cast<size_t>(n_books_) * n_members || (!mask.empty() && mask.size() != n_books_))
      throw Error(BK_INVALID_ARGUMENT, "retune: n_books x n_members rows and one mask byte per book are needed");
    check(bk_retune_agents(h_, n_members, rows.data(), mask.empty() ? nullptr : mask.data()));
  }
  // ... from device memory, one kernel on the env's stream with no host synchronisation (bk_retune_*_device): a book with
  // a bad entry keeps its row, status_dev (nullable, 2 u32 per book) and retune_rejected() say so
  void retune_random_agents_device(uint32_t n_groups, const bk_random_agents* rows_dev, const uint8_t* mask_dev = nullptr,
                                   uint32_t* status_dev = nullptr) {
    check(bk_retune_random_agents_device(h_, n_groups, rows_dev, mask_dev, status_dev));
  }
  void retune_agents_device(uint32_t n_members, const bk_agent_desc* rows_dev, const uint8_t* mask_dev = nullptr,
                            uint32_t* status_dev = nullptr) {
    check(bk_retune_agents_device(h_, n_members, rows_dev, mask_dev, status_dev));
  }
  uint64_t retune_rejected() {
    uint64_t n = 0;
    check(bk_retune_rejected(h_, &n));
    return n;
  }
  // agents.update(env, rng) of the RandomAgents into the device-resident queues (bk_update_agents; the env has the device
  // ingress, bk_device_ingress_enable(handle(), ..), then the agents): the next step() trades them with the submitted
  // instructions.  Asynchronous on the env's stream.
  void update_agents() { check(bk_update_agents(h_)); }
  // agents.update(env, rng) of an AgentSet with Noise / Momentum members into the same queues (bk_update_members)
  void update_members() { check(bk_update_members(h_)); }
  // RandomMarketAgents::update / MarketAgent::update of the installed set for every market into the market's queue
  // (bk_update_market_agents, bk_update_market_members); an env of one asset is a market of one book
  void update_market_agents() { check(bk_update_market_agents(h_)); }
  void update_market_members() { check(bk_update_market_members(h_)); }
  // member j's `orders` vector of book b after the last update_members (bk_member_orders; UINT64_MAX = None)
  std::vector<uint64_t> member_orders(uint32_t book, uint32_t member) {
    uint32_t n = 0;
    check(bk_member_orders(h_, book, member, 0, nullptr, &n));
    std::vector<uint64_t> ids(n);
    check(bk_member_orders(h_, book, member, n, ids.data(), &n));
    return ids;
  }
  // record the agents' orders (bk_set_agent_order_log; before the first run): env(b).get_orders() answers after run
  void enable_agent_order_log() { check(bk_set_agent_order_log(h_, 1)); }
  void run(uint64_t n_steps) {
    check(bk_run(h_, n_steps));
    check(bk_env_sync(h_));
  }
  // device-resident snapshot of every book (bk_snapshot_save), and chosen books back to it between two runs
  // (bk_reset_books: mask[b] != 0 resets book b; seeds, if any, re-seed the reset books); the reference has no counterpart
  void save_snapshot(uint32_t slot = 0) { check(bk_snapshot_save(h_, slot)); }
  void reset_books(const std::vector<uint8_t>& mask, const uint64_t* seeds = nullptr, uint32_t slot = 0) {
    if (mask.size() != n_books_) throw Error(BK_INVALID_ARGUMENT, "the mask needs one byte per book");
    check(bk_reset_books(h_, slot, mask.data(), seeds));
  }
  // the same for an env with the device ingress (bk_ingress_snapshot_save / bk_ingress_reset_books: order records,
  // held ids and members' lists rewind too, the reset books' queues are emptied); the reference has no counterpart
  void save_ingress_snapshot(uint32_t slot = 0) { check(bk_ingress_snapshot_save(h_, slot)); }
  void drop_ingress_snapshot(uint32_t slot = 0) { check(bk_ingress_snapshot_drop(h_, slot)); }
  void reset_ingress_books(const std::vector<uint8_t>& mask, const uint64_t* seeds = nullptr, uint32_t slot = 0) {
    if (mask.size() != n_books_) throw Error(BK_INVALID_ARGUMENT, "the mask needs one byte per book");
    check(bk_ingress_reset_books(h_, slot, mask.data(), seeds));
  }
  // trader accounts of an env with the device ingress (bk_accounts_enable): position / cash / volume / fills of traders
  // 0 .. n_traders - 1 per book, folded on the device behind every step; the reference has no counterpart
  void enable_accounts(uint32_t n_traders, bool consume_trades = false) {
    check(bk_accounts_enable(h_, n_traders, consume_trades ? 1 : 0));
    n_traders_ = n_traders;
  }
  // rows of books [first_book, first_book + n_books), n_traders each (waits for the env's stream)
  std::vector<bk_account> accounts(uint32_t first_book, uint32_t n_books) {
    std::vector<bk_account> rows(static_cast<size_t>(n_books) * n_traders_);
    check(bk_get_accounts(h_, first_book, n_books, rows.data()));
    return rows;
  }
  std::vector<bk_account> accounts() { return accounts(0, n_books_); }
  // the table in device memory, bk_account[n_books][n_traders]
  bk_account* accounts_device_ptr() {
    void* p = nullptr;
    check(bk_accounts_device_ptr(h_, &p));
    return static_cast<bk_account*>(p);
  }
  // zero the rows of the books with mask[b] != 0 (an empty mask: every book); they count from here
  void clear_accounts(const std::vector<uint8_t>& mask = {}) {
    if (!mask.empty() && mask.size() != n_books_) throw Error(BK_INVALID_ARGUMENT, "the mask needs one byte per book");
    check(bk_accounts_clear(h_, mask.empty() ? nullptr : mask.data()));
  }
  // per-step trade bars of an env with the device ingress (bk_trade_bars_enable): a ring of the last `window` steps' open /
  // high / low / close, buy / sell volume, notional and record counts per book, folded on the device behind every step; the
  // reference has no counterpart
  void enable_trade_bars(uint32_t window = 1, bool consume_trades = false) {
    check(bk_trade_bars_enable(h_, window, consume_trades ? 1 : 0));
    bars_window_ = window;
  }
  // rings of books [first_book, first_book + n_books), window rows each (waits for the env's stream)
  std::vector<bk_trade_bar> trade_bars(uint32_t first_book, uint32_t n_books) {
    std::vector<bk_trade_bar> rows(static_cast<size_t>(n_books) * bars_window_);
    check(bk_get_trade_bars(h_, first_book, n_books, rows.data()));
    return rows;
  }
  std::vector<bk_trade_bar> trade_bars() { return trade_bars(0, n_books_); }
  // the ring in device memory, bk_trade_bar[n_books][window]
  bk_trade_bar* trade_bars_device_ptr() {
    void* p = nullptr;
    check(bk_trade_bars_device_ptr(h_, &p));
    return static_cast<bk_trade_bar*>(p);
  }
  // the slot the latest folded step went to, (steps_done - 1) % window: no wait
  uint32_t trade_bars_slot() {
    uint32_t slot = 0;
    check(bk_trade_bars_slot(h_, &slot));
    return slot;
  }
  // zero all rows of the books with mask[b] != 0 (an empty mask: every book); the carried price starts at 0 again
  void clear_trade_bars(const std::vector<uint8_t>& mask = {}) {
    if (!mask.empty() && mask.size() != n_books_) throw Error(BK_INVALID_ARGUMENT, "the mask needs one byte per book");
    check(bk_trade_bars_clear(h_, mask.empty() ? nullptr : mask.data()));
  }
  // per-book series moments of the level-2 history (bk_series_enable): one row of integer sums per book over its whole
  // series, folded on the device from the history ring (needs history_capacity > 0); the reference has no counterpart
  void enable_series() { check(bk_series_enable(h_)); }
  // queue the fold of the steps run since the last fold (no host wait); throws, naming the count, if steps were lost
  void fold_series() { check(bk_series_fold(h_)); }
  // rows of books [first_book, first_book + n_books) (waits for the env's stream; does not fold)
  std::vector<bk_series_row> series(uint32_t first_book, uint32_t n_books) {
    std::vector<bk_series_row> rows(n_books);
    check(bk_get_series(h_, first_book, n_books, rows.data()));
    return rows;
  }
  std::vector<bk_series_row> series() { return series(0, n_books_); }
  // the table in device memory, bk_series_row[n_books]
  bk_series_row* series_device_ptr() {
    void* p = nullptr;
    check(bk_series_device_ptr(h_, &p));
    return static_cast<bk_series_row*>(p);
  }
  // a mask (one byte per book): fold, then clear those books' rows; an empty mask: clear every row without folding
  void clear_series(const std::vector<uint8_t>& mask = {}) {
    if (!mask.empty() && mask.size() != n_books_) throw Error(BK_INVALID_ARGUMENT, "the mask needs one byte per book");
    check(bk_series_clear(h_, mask.empty() ? nullptr : mask.data()));
  }
  // per-level depth table (bk_depth_enable): the series moments' companion over the ladder of the level-2 records, levels + 1
  // rows of 16 words per book; needs enable_series() and shares its fold, clears and cuts; no counterpart in the reference
  void enable_depth() { check(bk_depth_enable(h_)); }
  // (levels + 1) * 16 words per book of books [first_book, first_book + n_books) (waits for the env's stream; does not fold)
  std::vector<uint64_t> depth(uint32_t first_book, uint32_t n_books) {
    std::vector<uint64_t> rows(static_cast<size_t>(n_books) * (levels_ + 1u) * 16u);
    check(bk_get_depth(h_, first_book, n_books, rows.data()));
    return rows;
  }
  std::vector<uint64_t> depth() { return depth(0, n_books_); }
  // the table in device memory, uint64_t[n_books][levels + 1][16]
  uint64_t* depth_device_ptr() {
    void* p = nullptr;
    check(bk_depth_device_ptr(h_, &p));
    return static_cast<uint64_t*>(p);
  }
  // per-book candle table (bk_candles_enable): the series moments' other companion, a ring of the last n_candles bars of
  // width steps per book, 16 words a bar; needs enable_series() and shares its fold, clears and cuts; no counterpart in the
  // reference
  void enable_candles(uint32_t width, uint32_t n_candles) { check(bk_candles_enable(h_, width, n_candles)); }
  // {width, n_candles} as enabled
  std::pair<uint32_t, uint32_t> candles_config() {
    uint32_t c[2] = {0u, 0u};
    check(bk_candles_config_get(h_, c));
    return {c[0], c[1]};
  }
  // n_candles * 16 words per book of books [first_book, first_book + n_books), slot by slot (waits for the env's stream;
  // does not fold)
  std::vector<uint64_t> candles(uint32_t first_book, uint32_t n_books) {
    std::vector<uint64_t> rows(static_cast<size_t>(n_books) * candles_config().second * 16u);
    check(bk_get_candles(h_, first_book, n_books, rows.data()));
    return rows;
  }
  std::vector<uint64_t> candles() { return candles(0, n_books_); }
  // the table in device memory, uint64_t[n_books][n_candles][16]
  uint64_t* candles_device_ptr() {
    void* p = nullptr;
    check(bk_candles_device_ptr(h_, &p));
    return static_cast<uint64_t*>(p);
  }
  // per-book lag table of the level-2 history (bk_lags_enable): n_lags rows (1 .. 64) of integer sums per book, row k - 1
  // for lag / span k, folded on the device from the history ring (needs history_capacity > 0); no counterpart in the reference
  void enable_lags(uint32_t n_lags) {
    check(bk_lags_enable(h_, n_lags));
    n_lags_ = n_lags;
  }
  // queue the fold of the steps run since the last fold (no host wait); throws, naming the count, if steps were lost
  void fold_lags() { check(bk_lags_fold(h_)); }
  // rows [n_books][n_lags] of books [first_book, first_book + n_books) (waits for the env's stream; does not fold)
  std::vector<bk_lag_row> lags(uint32_t first_book, uint32_t n_books) {
    std::vector<bk_lag_row> rows(static_cast<size_t>(n_books) * n_lags_);
    check(bk_get_lags(h_, first_book, n_books, rows.data()));
    return rows;
  }
  std::vector<bk_lag_row> lags() { return lags(0, n_books_); }
  // the table in device memory, bk_lag_row[n_books][n_lags]
  bk_lag_row* lags_device_ptr() {
    void* p = nullptr;
    check(bk_lags_device_ptr(h_, &p));
    return static_cast<bk_lag_row*>(p);
  }
  // a mask (one byte per book): fold, then clear those books' rows and carry; an empty mask: clear all without folding
  void clear_lags(const std::vector<uint8_t>& mask = {}) {
    if (!mask.empty() && mask.size() != n_books_) throw Error(BK_INVALID_ARGUMENT, "the mask needs one byte per book");
    check(bk_lags_clear(h_, mask.empty() ? nullptr : mask.data()));
  }
  // per-book flow table of the trade records (bk_flow_enable): 8 + 6 n_lags u64 words per book - the base words, then lag rows
  // 1 .. n_lags in trade time (BK_FLOW_*) - folded on the device from each book's trade records (needs trade_capacity > 0);
  // no counterpart in the reference
  void enable_flow(uint32_t n_lags = 16, bool consume_trades = false) {
    check(bk_flow_enable(h_, n_lags, consume_trades ? 1 : 0));
    flow_lags_ = n_lags;
  }
  // queue one launch that folds every book's new trade records (no host wait)
  void fold_flow() { check(bk_flow_fold(h_)); }
  // words [n_books][8 + 6 n_lags] of books [first_book, first_book + n_books) (waits for the env's stream; does not fold)
  std::vector<uint64_t> flow(uint32_t first_book, uint32_t n_books) {
    std::vector<uint64_t> words(static_cast<size_t>(n_books) * (BK_FLOW_BASE_WORDS + BK_FLOW_LAG_WORDS * flow_lags_));
    check(bk_get_flow(h_, first_book, n_books, words.data()));
    return words;
  }
  std::vector<uint64_t> flow() { return flow(0, n_books_); }
  // the table in device memory, uint64_t[n_books][8 + 6 n_lags]
  uint64_t* flow_device_ptr() {
    void* p = nullptr;
    check(bk_flow_device_ptr(h_, &p));
    return static_cast<uint64_t*>(p);
  }
  // a mask (one byte per book): fold, then clear those books' words and carry; an empty mask: clear all without folding
  void clear_flow(const std::vector<uint8_t>& mask = {}) {
    if (!mask.empty() && mask.size() != n_books_) throw Error(BK_INVALID_ARGUMENT, "the mask needs one byte per book");
    check(bk_flow_clear(h_, mask.empty() ? nullptr : mask.data()));
  }
  // per-book bin table of the level-2 history (bk_bins_enable): n_spans + 2 rows of n_bins u64 counts per book - the change
  // of twice the mid over each span, the spread, the traded volume - folded on the device from the history ring (needs
  // history_capacity > 0); no counterpart in the reference
  void enable_bins(const bk_bins_config& cfg) {
    check(bk_bins_enable(h_, &cfg));
    bins_per_book_ = (cfg.n_spans + 2u) * cfg.n_bins;
  }
  bk_bins_config bins_config() {
    bk_bins_config cfg{};
    check(bk_bins_config_get(h_, &cfg));
    return cfg;
  }
  // queue the fold of the steps run since the last fold (no host wait); throws, naming the count, if steps were lost
  void fold_bins() { check(bk_bins_fold(h_)); }
  // counts [n_books][n_spans + 2][n_bins] of books [first_book, first_book + n_books) (waits for the env's stream; does not fold)
  std::vector<uint64_t> bins(uint32_t first_book, uint32_t n_books) {
    std::vector<uint64_t> counts(static_cast<size_t>(n_books) * bins_per_book_);
    check(bk_get_bins(h_, first_book, n_books, counts.data()));
    return counts;
  }
  std::vector<uint64_t> bins() { return bins(0, n_books_); }
  // the table in device memory, uint64_t[n_books][n_spans + 2][n_bins]
  uint64_t* bins_device_ptr() {
    void* p = nullptr;
    check(bk_bins_device_ptr(h_, &p));
    return static_cast<uint64_t*>(p);
  }
  // a mask (one byte per book): fold, then clear those books' counts and carry; an empty mask: clear all without folding
  void clear_bins(const std::vector<uint8_t>& mask = {}) {
    if (!mask.empty() && mask.size() != n_books_) throw Error(BK_INVALID_ARGUMENT, "the mask needs one byte per book");
    check(bk_bins_clear(h_, mask.empty() ? nullptr : mask.data()));
  }
  // per-market cross table of the level-2 history (bk_cross_enable), for an env of markets of `assets` >= 2 books each
  // (book = market * assets + asset): n_spans * assets * assets rows of integer sums per market, row (j, a, b) the ordered pair
  // asset a against asset b at span spans[j] - folded on the device from the history ring (needs history_capacity > 0); no
  // counterpart in the reference
  void enable_cross(const bk_cross_config& cfg, uint32_t assets) {
    check(bk_cross_enable(h_, &cfg));
    cross_markets_ = n_books_ / assets;
    cross_per_market_ = cfg.n_spans * assets * assets;
  }
  bk_cross_config cross_config() {
    bk_cross_config cfg{};
    check(bk_cross_config_get(h_, &cfg));
    return cfg;
  }
  // queue the fold of the steps run since the last fold (no host wait); throws, naming the count, if steps were lost
  void fold_cross() { check(bk_cross_fold(h_)); }
  // rows [n_markets][n_spans][assets][assets] of markets [first_market, first_market + n_markets) (waits for the env's
  // stream; does not fold)
  std::vector<bk_cross_row> cross(uint32_t first_market, uint32_t n_markets) {
    std::vector<bk_cross_row> rows(static_cast<size_t>(n_markets) * cross_per_market_);
    check(bk_get_cross(h_, first_market, n_markets, rows.data()));
    return rows;
  }
  std::vector<bk_cross_row> cross() { return cross(0, cross_markets_); }
  // the table in device memory, bk_cross_row[n_markets][n_spans][assets][assets]
  bk_cross_row* cross_device_ptr() {
    void* p = nullptr;
    check(bk_cross_device_ptr(h_, &p));
    return static_cast<bk_cross_row*>(p);
  }
  // a mask (one byte per MARKET): fold, then clear those markets' rows and carry; an empty mask: clear all without folding
  void clear_cross(const std::vector<uint8_t>& mask = {}) {
    if (!mask.empty() && mask.size() != cross_markets_) throw Error(BK_INVALID_ARGUMENT, "the mask needs one byte per market");
    check(bk_cross_clear(h_, mask.empty() ? nullptr : mask.data()));
  }
  // open orders of an env with the device ingress (bk_open_orders_enable): per book and trader 0 .. n_traders - 1 a summary
  // row and the `depth` oldest resting orders, recomputed on the device behind every step; the reference has no counterpart
  void enable_open_orders(uint32_t n_traders, uint32_t depth = 8) {
    check(bk_open_orders_enable(h_, n_traders, depth));
    open_traders_ = n_traders, open_depth_ = depth;
  }
  void refresh_open_orders() { check(bk_open_orders_refresh(h_)); }
  // rows of books [first_book, first_book + n_books): n_traders summary rows per book and n_traders * depth entries
  // (waits for the env's stream)
  struct OpenOrders {
    std::vector<bk_open_summary> summary;
    std::vector<bk_open_order> entries;
  };
  OpenOrders open_orders(uint32_t first_book, uint32_t n_books) {
    OpenOrders out;
    out.summary.resize(static_cast<size_t>(n_books) * open_traders_);
    out.entries.resize(out.summary.size() * open_depth_);
    check(bk_get_open_orders(h_, first_book, n_books, out.summary.data(), open_depth_ ? out.entries.data() : nullptr));
    return out;
  }
  OpenOrders open_orders() { return open_orders(0, n_books_); }
  // the tables in device memory: bk_open_summary[n_books][n_traders], bk_open_order[n_books][n_traders][depth] (null: depth 0)
  std::pair<bk_open_summary*, bk_open_order*> open_orders_device_ptrs() {
    void *s = nullptr, *e = nullptr;
    check(bk_open_orders_device_ptrs(h_, &s, &e));
    return {static_cast<bk_open_summary*>(s), static_cast<bk_open_order*>(e)};
  }
  // queue positions of the open orders (bk_open_queue_enable): one row per entry of the open-order view - the volume and
  // the orders with priority over it - recomputed on the device right behind those rows; the reference has no counterpart
  void enable_open_queue() { check(bk_open_queue_enable(h_)); }
  // rows of books [first_book, first_book + n_books), n_traders * depth each (waits for the env's stream)
  std::vector<bk_open_queue> open_queue(uint32_t first_book, uint32_t n_books) {
    std::vector<bk_open_queue> rows(static_cast<size_t>(n_books) * open_traders_ * open_depth_);
    check(bk_get_open_queue(h_, first_book, n_books, rows.data()));
    return rows;
  }
  std::vector<bk_open_queue> open_queue() { return open_queue(0, n_books_); }
  // the table in device memory, bk_open_queue[n_books][n_traders][depth]
  bk_open_queue* open_queue_device_ptr() {
    void* p = nullptr;
    check(bk_open_queue_device_ptr(h_, &p));
    return static_cast<bk_open_queue*>(p);
  }
  // quotes (bk_submit_quotes_device): one bk_quote row per book and trader of the open-order view, joined with the view's
  // entries on the device and queued as cancellations, in-place reductions and new orders - the dense grid n_traders x
  // (depth + 2) through the device ingress; out_ids_dev ([n_books][n_traders][2]) and status_dev ([2 * n_books]) are
  // device memory and may be null.  Asynchronous on the env's stream; the reference has no counterpart
  void submit_quotes_device(const bk_quote* quotes_dev, uint64_t* out_ids_dev = nullptr, uint32_t* status_dev = nullptr) {
    check(bk_submit_quotes_device(h_, quotes_dev, out_ids_dev, status_dev));
  }
  // the same from a host table of n_books * n_traders rows (copied through the env's device staging buffer)
  void submit_quotes(const std::vector<bk_quote>& quotes, uint64_t* out_ids_dev = nullptr, uint32_t* status_dev = nullptr) {
    if (quotes.size() != static_cast<size_t>(n_books_) * open_traders_) throw std::invalid_argument("quotes: n_books * n_traders rows");
    check(bk_submit_quotes(h_, quotes.data(), out_ids_dev, status_dev));
  }
  bk_env* handle() { return h_; }

 private:
  bk_env* h_ = nullptr;
  uint32_t n_books_ = 0, levels_ = 10, n_traders_ = 0, open_traders_ = 0, open_depth_ = 0, bars_window_ = 0, n_lags_ = 0, bins_per_book_ = 0, flow_lags_ = 0;
  uint32_t cross_markets_ = 0, cross_per_market_ = 0;
};

// `Agent::update(&mut self, env: &mut Env, rng: &mut R)` (agents/mod.rs:46-55).  The device owns each book's
// xoroshiro128** stream and spends it on the shuffle only; a host-side agent draws from its own generator `Rng`,
// exactly as the reference's Python agents draw from numpy's (src/bourse/step_sim/runner.py:100).
template <class Rng>
struct Agent {
  virtual ~Agent() = default;
  virtual void update(Env& env, Rng& rng) = 0;
};

// `sim_runner(env, agents, seed, n_steps, _)` (runner.rs:46-69) for every book: agents[b] is book b's AgentSet (its
// members in declaration order), rngs[b] its host generator.
template <class Rng>
void sim_runner(ManyEnv& many, std::vector<std::vector<Agent<Rng>*>>& agents, std::vector<Rng>& rngs, uint64_t n_steps) {
  for (uint64_t s = 0; s < n_steps; ++s) {
    for (uint32_t b = 0; b < many.n_books(); ++b) {
      Env e = many.env(b);
      for (Agent<Rng>* a : agents[b]) a->update(e, rngs[b]);
    }
    many.step();
  }
}

}  // namespace bourse_amd
