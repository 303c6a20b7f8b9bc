/* bourse_amd.h — C ABI of the MI355X many-book limit-order-book step simulator.
 *
 * Drop-in boundary for the reference's `bourse_de::Env` hot path (plain pointers and
 * sizes, no torch / C++ types).  One `bk_env` owns B >= 1 INDEPENDENT books on one GPU;
 * book b behaves exactly like one reference `Env` driven by its own
 * `Xoroshiro128StarStar::seed_from_u64(seed + book_offset + b)`.
 *
 * Each entry point cites the reference interface it replaces (paths relative to the
 * reference repository).  INTEGRATION.md shows the Rust `extern "C"` / ctypes bindings.
 *
 * Threads: a `bk_env` is used by ONE host thread at a time (like `&mut Env`); DISTINCT envs may be driven from distinct
 * threads concurrently (every call selects the env's device; bk_last_error() is per thread; the process-wide part streams
 * are created under a lock) - tests/test_gpu_parity.py test_envs_driven_from_concurrent_host_threads.
 *
 * Status codes: every function returns one of these.
 */
#ifndef BOURSE_AMD_H
#define BOURSE_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum bk_status {
  BK_OK = 0,
  BK_PRICE_NOT_TICK_MULTIPLE = 1, /* OrderError::PriceError, crates/order_book/src/orderbook.rs:127-142 */
  BK_UNKNOWN_ORDER_ID = 2,        /* panic! at orderbook.rs:642 / index panic :338,:749 */
  BK_CAPACITY = 3,                /* a fixed device capacity was exceeded (cannot occur in the reference) */
  BK_STEP_SIZE_EXCEEDED = 4,      /* #events in a step >= step_size: (price,t) key collision hazard, SURVEY App. A.9 */
  BK_INVALID_ARGUMENT = 5,
  BK_HIP_ERROR = 6,               /* a HIP runtime call failed; bk_last_error() has the text */
  BK_NO_DEVICE = 7                /* no usable GPU: the product path never falls back to a CPU */
};

/* per-book sticky flag bits reported by bk_book_flags() */
#define BK_FLAG_POOL_OVERFLOW 1u   /* live-order pool full: an order that should rest was dropped */
#define BK_FLAG_TRADE_OVERFLOW 2u  /* trade buffer full: records dropped (counts stay exact) */
#define BK_FLAG_STEP_SIZE 4u       /* a step queued >= step_size events */
#define BK_FLAG_ORDER_LOG_FULL 8u  /* order id beyond the order-log capacity */
#define BK_FLAG_UNKNOWN_ORDER 16u  /* cancel/modify of an id that was never created */
#define BK_FLAG_HIST_OVERFLOW 32u  /* RESERVED, never set (the L2 history is a ring; reading an overwritten step is an
                                     * error of the reader): the bit keeps its place so that the others keep theirs */
#define BK_FLAG_PRICE_TICK 64u     /* a Noise/Momentum agent's limit price (clamped to u32::MAX) was not a tick multiple:
                                     * the reference panics here (`.unwrap()`, common.rs:107,140); the order is not created */
#define BK_FLAG_DECODE_LOOKAHEAD 256u /* the wave-parallel decode of a Noise/Momentum member met a ziggurat rejection loop
                                     * longer than its 128-draw look-ahead (p < 2^-90): results of that book are suspect */
#define BK_FLAG_EVENT_OVERFLOW 128u /* a MARKET with Noise/Momentum members queued more than max_live_orders events in one
                                     * step (its books share one queue of that size): the excess events were dropped */
#define BK_FLAG_ACCOUNTS_INEXACT 512u /* trader accounts (bk_accounts_enable): a trade record of this book could not be folded
                                     * into the rows - dropped beyond trade_capacity, or with an order id >= max_orders */

typedef struct bk_env bk_env;

/* Env::<LEVELS>::new(start_time, tick_size, step_size, trading) — crates/step_sim/src/env.rs:84-95,
 * plus the sizes a fixed-capacity device implementation needs.  Zero-initialise, then set. */
typedef struct bk_config {
  uint32_t n_books;         /* B >= 1 independent books on this GPU */
  uint32_t levels;          /* LEVELS: L2 depth per side (reference default 10; 16/32/64 in the benchmark configs) */
  uint64_t start_time;
  uint32_t tick_size;       /* > 0 (assert at orderbook.rs:159) */
  uint32_t trading;         /* bool */
  uint64_t step_size;
  uint64_t seed;            /* book b is seeded seed + book_offset + b (identity for B = 1) */
  uint64_t book_offset;     /* global index of this GPU's first book (multi-GPU sharding) */
  uint32_t max_live_orders; /* live-order pool per book, rounded up to 64, 128, 256 or 512 (0 = 128; more is refused) */
  uint32_t max_orders;      /* order-log capacity per book: host-driven orders, the device ingress, and bk_run's
                               RandomAgents after bk_set_agent_order_log (0 = no log) */
  uint32_t trade_capacity;  /* trade records retained per book between bk_clear_trades() calls */
  uint32_t history_capacity;/* L2 history ring: the last N steps are retained (0 = keep only the latest record) */
  int32_t device;           /* HIP device ordinal */
  uint32_t assets;          /* MarketEnv<ASSETS> mode (crates/step_sim/src/market_env.rs:46-132): `assets` consecutive books
                             * form a market sharing one clock, ONE RNG stream and ONE shuffled event queue; book =
                             * market * assets + asset; market m is seeded seed + book_offset + m (book_offset counted in
                             * markets).  0 or 1 = independent books (Env).  <= 8, must divide n_books. */
} bk_config;

/* RandomAgents::new(n_agents, tick_range, vol_range, tick_size, activity_rate)
 * — crates/step_sim/src/agents/random_agent.rs:67-81 */
typedef struct bk_random_agents {
  uint32_t n_agents;
  uint32_t tick_lo, tick_hi; /* tick_range (half-open) */
  uint32_t vol_lo, vol_hi;   /* vol_range (half-open) */
  uint32_t tick_size;        /* the AGENTS' tick size: price = tick * tick_size */
  float activity_rate;
} bk_random_agents;

/* One member of a derive(AgentSet) struct (crates/macros/src/lib.rs:57-73): RandomAgents, NoiseAgent
 * (NoiseAgent::new(agent_id_start, n_agents, NoiseAgentParams), crates/step_sim/src/agents/noise_agent.rs:24-123) or
 * MomentumAgent (MomentumAgent::new(agent_id_start, n_agents, MomentumParams), momentum_agent.rs:24-142). */
enum bk_agent_type { BK_AGENT_RANDOM = 0, BK_AGENT_NOISE = 1, BK_AGENT_MOMENTUM = 2 };
typedef struct bk_agent_desc {
  uint32_t type;             /* bk_agent_type */
  uint32_t n_agents;
  uint32_t tick_lo, tick_hi; /* RandomAgents tick_range */
  uint32_t vol_lo, vol_hi;   /* RandomAgents vol_range */
  uint32_t tick_size;        /* the member's tick_size parameter */
  float activity_rate;       /* RandomAgents */
  uint32_t agent_id_start;   /* Noise/Momentum: first trader id */
  float p_limit, p_market;   /* NoiseAgentParams */
  float p_cancel;            /* Noise/Momentum */
  uint32_t trade_vol;        /* Noise/Momentum */
  uint32_t reserved;
  double price_dist_mu, price_dist_sigma;       /* Noise/Momentum: LogNormal(mu, sigma) */
  double decay, demand, scale, order_ratio;     /* MomentumParams */
} bk_agent_desc;

/* Trade — crates/order_book/src/types.rs:103-118; tuple order of PyTrade, rust/src/types.rs:4-15 */
typedef struct bk_trade {
  uint64_t t;
  uint32_t side_is_bid; /* side of the PASSIVE order */
  uint32_t price;
  uint32_t vol;
  uint32_t reserved;
  uint64_t active_order_id;
  uint64_t passive_order_id;
} bk_trade;

/* Order — crates/order_book/src/types.rs:79-99; tuple order of PyOrder, rust/src/types.rs:17-31 */
typedef struct bk_order {
  uint8_t side_is_bid;
  uint8_t status; /* 0 New, 1 Active, 2 Filled, 3 Cancelled, 4 Rejected (types.rs:65-75) */
  uint8_t reserved[6];
  uint64_t arr_time;
  uint64_t end_time;
  uint32_t vol;
  uint32_t start_vol;
  uint32_t price;
  uint32_t trader_id;
  uint64_t order_id;
} bk_order;

/* whole-shard market statistics, modelled on Market's array-valued queries
 * (crates/order_book/src/market.rs:137-216); the unit all-gathered across GPUs (64 bytes) */
typedef struct bk_stats {
  uint64_t n_books;
  uint64_t sum_trade_vol;  /* sum over books of the last step's trade volume */
  uint64_t sum_trades;     /* cumulative trade count over books */
  uint64_t sum_events;     /* cumulative processed events over books */
  uint64_t sum_bid_vol, sum_ask_vol;
  uint32_t min_bid, max_bid, min_ask, max_ask; /* over books with a non-empty side; 0xFFFFFFFF/0 if none */
} bk_stats;

const char* bk_last_error(void);
int bk_device_count(int* out);
/* HIP_VERSION the library was compiled against / hipRuntimeGetVersion() of the runtime this process bound it to (no
 * reference counterpart: diagnostics - a Python process may run the library on PyTorch's bundled runtime, bourse_amd/_lib.py) */
int bk_hip_versions(int* built, int* runtime);

/* ------------------------------------------------------------------ lifetime */
int bk_env_create(const bk_config* cfg, bk_env** out);   /* Env::new, env.rs:84-95 (x B) */
void bk_env_destroy(bk_env* env);
int bk_env_set_stream(bk_env* env, void* hip_stream);    /* run on the caller's hipStream_t (NULL = default) */
int bk_env_sync(bk_env* env);                            /* wait for queued device work */

/* ------------------------------------------- host-driven order flow (per book) */
/* Env::place_order, env.rs:166-176: tick check + id assignment now, New event queued for the next step */
int bk_place_order(bk_env* env, uint32_t book, int bid, uint32_t vol, uint32_t trader_id, int has_price,
                   uint32_t price, uint64_t* out_order_id);
/* Env::cancel_order, env.rs:189-191 */
int bk_cancel_order(bk_env* env, uint32_t book, uint64_t order_id);
/* Env::modify_order, env.rs:208-219 */
int bk_modify_order(bk_env* env, uint32_t book, uint64_t order_id, int has_price, uint32_t new_price, int has_vol,
                    uint32_t new_vol);
/* StepEnvNumpy.submit_instructions, rust/src/step_sim_numpy.rs:233-275: action 0 none / 1 new limit / 2 cancel; every
 * other value is a no-op, as the reference's `_ => Ok(OrderId::MAX)` (:266) - on the host entries AND on the device
 * entry below.  The one extension, the same on all three entries, is BK_ACTION_MODIFY (a code far outside the
 * reference's range, so a reference-written batch can never mean it): Env::modify_order (env.rs:208-219) on
 * order_id[i], side bit 1 = has a new price (price[i]), side bit 2 = has a new volume (vol[i]).
 * out_ids[i] = new id or UINT64_MAX.  Stops at the first bad price (earlier elements stay queued) and
 * returns BK_PRICE_NOT_TICK_MULTIPLE with *n_done = index of the offending element. */
#define BK_ACTION_MODIFY 0x80000003u
int bk_submit_instructions(bk_env* env, uint32_t book, size_t n, const uint32_t* action, const uint8_t* side,
                           const uint32_t* vol, const uint32_t* trader_id, const uint32_t* price,
                           const uint64_t* order_id, uint64_t* out_ids, size_t* n_done);
/* The same for every book in one call: book b's instructions are elements [book_offsets[b], book_offsets[b+1]) of the
 * arrays (CSR over n_books + 1 offsets).  *n_done = global index reached.  Large batches are spread over host threads
 * (one contiguous range of books each; BOURSE_AMD_HOST_THREADS overrides the count); on an error, books after the failing
 * one may already be queued. */
int bk_submit_instructions_csr(bk_env* env, const uint64_t* book_offsets, const uint32_t* action, const uint8_t* side,
                               const uint32_t* vol, const uint32_t* trader_id, const uint32_t* price,
                               const uint64_t* order_id, uint64_t* out_ids, size_t* n_done);
int bk_enable_trading(bk_env* env, int enabled);         /* Env::{enable,disable}_trading, env.rs:138-145 */
/* Env::step, env.rs:116-135, for every book: shuffle + process the queued events, snapshot L2 */
int bk_step(bk_env* env);

/* ------------------------------------------------------------- device-resident instruction ingress
 * For agent layers that already run on the GPU: `submit_instructions` (rust/src/step_sim_numpy.rs:233-275) and the
 * host half of Env::place_order / cancel_order / modify_order (crates/step_sim/src/env.rs:166-219) for EVERY book in one
 * kernel launch, the six SoA arrays taken as DEVICE pointers - nothing of a step passes through host memory.
 * bk_device_ingress_enable: switches a fresh env to this flow (before any order; an env runs one flow: the per-order
 *   host entries and bk_run are refused from then on) and allocates the per-book (per-market) event queues of
 *   `queue_capacity` events per step (1..8192).
 * bk_submit_instructions_device: book b's instructions are elements [book_offsets_dev[b], book_offsets_dev[b+1]) of the
 *   arrays (all in device memory, u64 offsets over n_books + 1).  action 0 = none, 1 = new limit order, 2 = cancel,
 *   anything else a no-op (as the reference's, :266), BK_ACTION_MODIFY = Env::modify_order (the extension of
 *   bk_submit_instructions: side bit 1 = has price, bit 2 = has volume; bit 0 is the bid flag of a new order) - the same
 *   arrays mean the same on the host and on the device entry.  Per book exactly the reference's semantics: ids are dense in element order (an exclusive prefix
 *   sum over action == 1 on the device), the first price that is not a multiple of the book's tick size stops THAT
 *   book's batch - earlier elements stay created and queued (:255-268) - and the other books are unaffected.
 *   out_ids_dev (optional, one u64 per element): the created order's id, u64::MAX otherwise; untouched from the failing
 *   element on.  status_dev (optional, 2 u32 per book): {bk_status code - BK_OK, BK_PRICE_NOT_TICK_MULTIPLE, BK_CAPACITY
 *   (queue full / id space) -, number of the book's elements applied}.  Asynchronous on the env's stream.
 *   A cancel / modify of an id that was never created (the reference panics while processing, orderbook.rs:642; the
 *   host-driven bk_step refuses the step) is dropped at the step and the book flagged BK_FLAG_UNKNOWN_ORDER.
 *   All seven input arrays must be non-null (a step with no instruction for any book: do not call).
 * bk_step_async: Env::step over the device-resident queues without waiting (bk_step on such an env = this + a wait).
 * Readers (bk_get_orders, bk_order_status, bk_get_trades, bk_history ...) work as on the host-driven flow. */
int bk_device_ingress_enable(bk_env* env, uint32_t queue_capacity);
int bk_submit_instructions_device(bk_env* env, const uint64_t* book_offsets_dev, const uint32_t* action_dev,
                                  const uint8_t* side_dev, const uint32_t* vol_dev, const uint32_t* trader_dev,
                                  const uint32_t* price_dev, const uint64_t* order_id_dev, uint64_t* out_ids_dev,
                                  uint32_t* status_dev);
int bk_step_async(bk_env* env);
/* bk_update_agents: agents.update(env, rng) of the installed RandomAgents groups for every book (random_agent.rs:85-119) on
 * an env with the device ingress, so that background agents and submitted instructions trade in one env as in the
 * reference.  For each agent, in declaration order, with the book's own RNG (the one the step shuffles with): draw
 * gen::<f32>(); if active and its held order is Active (resting in the book right now), queue its cancellation and hold
 * nothing; else if active, draw side, tick and volume, create the order (next id of the book, trader id = the agent's
 * index in its group) and queue it.  The events are appended to the same queues as bk_submit_instructions_device's, in
 * call order: update-then-submit and submit-then-update are both valid and each equals the reference called in that
 * order (as do two bk_update_agents in one step).  Every bk_set_random_agents* call resets the held orders to None (the
 * old orders stay on the books, unowned).  A full queue or an exhausted id space drops the event and sets
 * BK_FLAG_EVENT_OVERFLOW.  Asynchronous on the env's stream.  Order: bk_device_ingress_enable, then the agents.
 * BK_INVALID_ARGUMENT (env unchanged): no device ingress, no RandomAgents groups, Noise / Momentum members, assets > 1. */
int bk_update_agents(bk_env* env);
/* bk_update_members: agents.update(env, rng) of the installed AgentSet (bk_set_agents / bk_set_agents_per_book:
 * NoiseAgent and MomentumAgent members, with or without RandomAgents members) for every book on an env with the device
 * ingress - replaces NoiseAgent::update (noise_agent.rs:127-176), MomentumAgent::update (momentum_agent.rs:146-208) with
 * common::cancel_live_orders (common.rs:56-75), and RandomAgents::update (random_agent.rs:85-119), called member by member
 * in declaration order (crates/macros/src/lib.rs:57-73) with the book's own RNG.  A Noise / Momentum member first walks
 * its `orders` list: entries that are not Active (not resting in the book right now) are dropped without a draw, every
 * Active one takes gen::<f32>() and is kept when the draw exceeds p_cancel, else its cancellation is queued; then every
 * trader draws and places its limit order (around the mid price of the book as it stands, next id of the book, trader
 * id agent_id_start + t, remembered in the list) and its market order (price u32::MAX for a bid, 0 for an ask).  A limit
 * price off the book's tick grid sets BK_FLAG_PRICE_TICK and creates nothing.  The events are appended to the same queues
 * as bk_submit_instructions_device's, in call order; a full queue or an exhausted id space drops the event and sets
 * BK_FLAG_EVENT_OVERFLOW.  Every bk_set_agents* call empties the lists and clears the momentum state (the old orders
 * stay on the books, unowned).  Asynchronous on the env's stream.
 * BK_INVALID_ARGUMENT (env unchanged): no device ingress, no AgentSet installed (an all-RandomAgents set is
 * bk_update_agents'), assets > 1. */
int bk_update_members(bk_env* env);
/* bk_update_market_agents: RandomMarketAgents::update (random_agent.rs:204-245) of the groups installed by
 * bk_set_random_market_agents (or the per-market table of bk_set_random_agents_per_book) for every market of an env with
 * the device ingress - background MarketAgents and a user's own agent sharing one MarketEnv and one rng
 * (runner.rs:108-131).  bk_update_agents' semantics with these changes: a group of asset a tests Active against the pool
 * of book market * assets + a, takes that book's next id and records its orders in that book's rows; its events go to the
 * MARKET's queue, tagged with the asset, in call order behind whatever bk_submit_instructions_device or an earlier update
 * queued; the draws come from the market's RNG, whose advanced state every book of the market receives.  A full queue or
 * an exhausted id space drops the event and sets BK_FLAG_EVENT_OVERFLOW on the book of the event's asset.  An env of one
 * asset is a market of one book: there this entry and bk_update_agents share the held ids and may alternate from step to
 * step.  Asynchronous on the env's stream.
 * BK_INVALID_ARGUMENT (env unchanged): no device ingress, no groups installed, Noise / Momentum members (they are
 * bk_update_market_members'). */
int bk_update_market_agents(bk_env* env);
/* bk_update_market_members: MarketAgent::update of the set installed by bk_set_market_agents (or bk_set_agents_per_book) -
 * NoiseMarketAgent (noise_agent.rs:226-340), MomentumMarketAgent (momentum_agent.rs:282-397) and RandomMarketAgents
 * (random_agent.rs:204-245) members, in declaration order, with the market's own RNG - for every market of an env with the
 * device ingress.  bk_update_members' semantics, each member on the book of its asset (that book's pool, mid price, tick
 * size, next id and rows; BK_FLAG_PRICE_TICK and BK_FLAG_EVENT_OVERFLOW on that book), its events in the market's queue
 * as bk_update_market_agents'.  The lists and the momentum state are kept per market; on an env of one asset they are
 * bk_update_members' own.  Asynchronous on the env's stream.
 * BK_INVALID_ARGUMENT (env unchanged): no device ingress, nothing installed, an all-RandomAgents set (it is
 * bk_update_market_agents'). */
int bk_update_market_members(bk_env* env);
/* bk_member_orders: member `member`'s `orders` vector of one book as the device holds it after the last
 * bk_update_members (NoiseAgent.orders / MomentumAgent.orders, noise_agent.rs:104, momentum_agent.rs:114), in list order;
 * for a RandomAgents member the ids its agents hold (RandomAgents.orders, random_agent.rs:49), UINT64_MAX for None.
 * *n_out = the vector's length; the first min(cap, length) ids go to out_ids.  Waits for the env's stream.  On a market
 * (assets > 1, bk_update_market_members) the list is that of market book / assets, and its ids are ids of the member's
 * asset's book. */
int bk_member_orders(bk_env* env, uint32_t book, uint32_t member, uint32_t cap, uint64_t* out_ids, uint32_t* n_out);
/* HOST arrays through the device ingress (a BaseNumpyAgent-style caller: src/bourse/step_sim/agents/base_agent.py:67-116
 * returns host numpy arrays, runner.py:103-112 passes them to submit_instructions, rust/src/step_sim_numpy.rs:233-275).
 * Same arrays, same per-book semantics as bk_submit_instructions_device, but the pointers are HOST memory: the library
 * stages them in pinned memory (host threads), uploads them on a copy stream of its own, runs the ingest kernel on the
 * env's stream and brings ids and per-book status back on a second copy stream.  Asynchronous: returns a ticket at
 * once; two tickets are in flight at most (the upload of one under the step kernel of the other), and
 * bk_submit_result(ticket) waits for that ticket only.  A ticket's results stay readable until two more submits (also
 * across a batch that outgrows the staging: the results move with it).
 *   bk_ingress_staging: OPTIONAL zero-copy - pinned arrays (>= min_elements each; book_offsets n_books + 1) that the NEXT
 *     bk_submit_instructions_host call will upload from: fill them in place and pass these very pointers (any array
 *     passed from elsewhere is copied as usual).  Valid until that submit returns.
 *   bk_submit_result: out_ids (optional, book_offsets[n_books] u64: the created order's id, UINT64_MAX otherwise -
 *     also from a book's failing element on), status (optional, 2 u32 per book: {bk_status code,
 *     elements of the book's batch applied}), first_failed_book (optional: lowest book whose code is not BK_OK, UINT32_MAX
 *     if none - the Python layer raises the reference's ValueError for it). */
typedef struct bk_ingress_arrays {
  uint64_t capacity;       /* elements each instruction array holds */
  uint64_t* book_offsets;  /* n_books + 1 */
  uint32_t* action;
  uint8_t* side;
  uint32_t* vol;
  uint32_t* trader_id;
  uint32_t* price;
  uint64_t* order_id;
} bk_ingress_arrays;
int bk_ingress_staging(bk_env* env, uint64_t min_elements, bk_ingress_arrays* out);
int bk_submit_instructions_host(bk_env* env, const uint64_t* book_offsets, const uint32_t* action, const uint8_t* side,
                                const uint32_t* vol, const uint32_t* trader_id, const uint32_t* price,
                                const uint64_t* order_id, uint64_t* out_ticket);
int bk_submit_result(bk_env* env, uint64_t ticket, uint64_t* out_ids, uint32_t* status, uint32_t* first_failed_book);
/* The same without a copy: pointers INTO the library's pinned staging (ids: book_offsets[n_books] u64; status: 2 u32 per book),
 * valid until two more submits.  For a loop that only looks at the ids (3 MB per step at 8 192 books x 48 instructions). */
int bk_submit_result_view(bk_env* env, uint64_t ticket, const uint64_t** out_ids, const uint32_t** status,
                          uint32_t* first_failed_book);
/* Env::order_status / Env::order, env.rs:283-290 (needs max_orders > 0) */
int bk_order_status(bk_env* env, uint32_t book, uint64_t order_id, uint8_t* out_status);
int bk_order_count(bk_env* env, uint32_t book, uint64_t* out);
int bk_get_orders(bk_env* env, uint32_t book, uint64_t first, uint64_t n, bk_order* out); /* Env::get_orders */
/* OrderEntry.key (crates/order_book/src/orderbook.rs:34-39) of orders [first, first+n): the price and the time the
 * order's priority key (side, price_key, t) was last set with — what OrderBook::save_json serialises beside each order. */
int bk_get_order_keys(bk_env* env, uint32_t book, uint64_t first, uint64_t n, uint32_t* key_price, uint64_t* key_time);
/* OrderBook::load_json -> TryFrom<OrderBookState> (orderbook.rs:827-918): replace one book's state with a snapshot
 * (clock, trade volume, all orders listed by id with their keys, all trades); Active orders re-enter the book in key
 * order and the level-2 record is rebuilt.  Nothing may be queued for the book (its market). */
int bk_load_book(bk_env* env, uint32_t book, uint64_t t, uint32_t trade_vol, uint64_t n_orders, const bk_order* orders,
                 const uint32_t* key_price, const uint64_t* key_time, uint64_t n_trades, const bk_trade* trades);

/* ---------------------------------------------------- on-device order flow */
/* An AgentSet of RandomAgents groups, the same parameters for every book (bk_set_random_agents_per_book: per book),
 * updated in declaration order (crates/macros/src/lib.rs:57-73).  Sum of n_agents <= max_live_orders. */
int bk_set_random_agents(bk_env* env, uint32_t n_groups, const bk_random_agents* groups);
/* Market mode.  Market::new(start_time, tick_size: [Price; ASSETS], trading) — crates/order_book/src/market.rs:74-81:
 * per-asset tick sizes (default: cfg.tick_size for every asset); call before anything else. */
int bk_set_tick_sizes(bk_env* env, uint32_t n_assets, const uint32_t* tick_sizes);
/* A MarketAgentSet of RandomMarketAgents groups (RandomMarketAgents::new(asset, n_agents, tick_range, vol_range,
 * tick_size, activity_rate), random_agent.rs:185-201), the same for every market (per market: bk_set_random_agents_per_book), updated in declaration order with
 * the market's RNG (market_sim_runner, runner.rs:108-131).  assets[g] = the asset group g trades (NULL: all 0).
 * Sum of n_agents <= max_live_orders.  bk_run() then steps every market; host-driven orders use the per-book calls with
 * book = market * assets + asset (MarketEnv::place_order / cancel_order / modify_order, market_env.rs:163-218). */
int bk_set_random_market_agents(bk_env* env, uint32_t n_groups, const bk_random_agents* groups,
                                const uint32_t* assets);
/* RandomAgents groups whose parameters differ per book (per market when assets > 1): groups[u * n_groups + g] is group g
 * of unit u, u < n_books / assets.  n_agents (and assets[g]; NULL = all 0) are shared by every unit.  Unit u steps as the
 * unit of an env given bk_set_random_agents (bk_set_random_market_agents) with row u does, bit for bit.  Every entry is
 * checked as bk_set_random_market_agents checks one, with the same status codes; the message names the first failing
 * unit and group; n_agents[g] differing between units is BK_INVALID_ARGUMENT.  On a failure the installed agents stay.
 * Replaces the installed agent set; a later bk_set_random_agents / bk_set_agents replaces (and frees) the table. */
int bk_set_random_agents_per_book(bk_env* env, uint32_t n_groups, const bk_random_agents* groups, const uint32_t* assets);
/* Any mix of built-in members (at most 4 when a Noise/Momentum member is present), identical for every book.
 * Noise/Momentum members price orders with f64 log-normal offsets: their outputs match the CPU oracle bit for bit
 * but only statistically match a Rust build (third-party sampling + libm). */
int bk_set_agents(bk_env* env, uint32_t n_members, const bk_agent_desc* members);
/* Market mode: a MarketAgentSet of RandomMarketAgents / NoiseMarketAgent / MomentumMarketAgent members
 * (random_agent.rs:164-247, noise_agent.rs:226-340, momentum_agent.rs:282-397); member i trades asset assets[i] of every
 * market and draws from the market's RNG in declaration order. */
int bk_set_market_agents(bk_env* env, uint32_t n_members, const bk_agent_desc* members, const uint32_t* assets);
/* AgentSet (MarketAgentSet) members whose parameters differ per book (per market when assets > 1): members[u * n_members
 * + i] is member i of unit u, u < n_books / assets.  assets[i] as in bk_set_market_agents: NULL on independent books,
 * required on markets.  type, n_agents and assets[i] are shared by every unit; every other field may differ.  Unit u
 * steps as the unit of an env given bk_set_agents (bk_set_market_agents) with row u does, bit for bit.  Every entry is
 * checked as bk_set_agents checks one, with the same status codes; the message names the first failing unit and member;
 * type or n_agents differing between units is BK_INVALID_ARGUMENT.  An all-RandomAgents table is
 * bk_set_random_agents_per_book's.  On a failure the installed agents stay.  Replaces the installed agent set; a later
 * bk_set_agents / bk_set_random_agents / bk_set_random_agents_per_book replaces (and frees) the table. */
int bk_set_agents_per_book(bk_env* env, uint32_t n_members, const bk_agent_desc* members, const uint32_t* assets);
/* RETUNE: replace, for the units a mask names, the parameter records of the installed per-unit table, in place on the
 * device (a unit is a book, or a market when assets > 1).  In the reference's terms the fields of unit u's agent objects
 * are assigned between two `update` calls: the next bk_run, bk_warm, bk_update_agents, bk_update_members or
 * bk_update_market_* queued behind the call steps unit u as the reference would.  NOTHING ELSE CHANGES: the books and
 * the RNG states, the RandomAgents' fixed slots and held ids, the members' order lists, lengths and momentum state
 * (last_price, momentum), the "re-make at the next update" marks of an install, the count of installs and the agent-set
 * hash of checkpoints and snapshot slots all stay.
 *   - Needs an installed per-unit table of the same kind and width: bk_set_random_agents_per_book with the same n_groups
 *     for the RandomAgents entries, bk_set_agents_per_book with the same n_members for the members' (an all-RandomAgents
 *     members table is bk_set_random_agents_per_book's, and so is its retune).  A uniform install is refused with
 *     BK_INVALID_ARGUMENT: install a per-unit table of identical rows, which costs nothing.
 *   - rows[u * width + j] is entry j of unit u, in the install's own structs; rows of unmasked units are not read.
 *     mask: one byte per unit, NULL = every unit.
 *   - Every entry is checked as the install checks one, with the install's status codes (ranges, tick_lo != 0, the price
 *     bound, tick_size a multiple of the asset's tick, finite mu, sigma >= 0).  In addition n_agents - and a member's type
 *     and agent_id_start - must equal the installed values (BK_INVALID_ARGUMENT).  The asset and a RandomAgents member's
 *     first fixed slot are no inputs: they stay what the install wrote.
 *   - All or nothing per unit: a unit with any failing entry keeps its whole row.
 *   - Never silent: status_dev (optional; 2 u32 per unit, as bk_submit_instructions_device's) receives {bk_status, index
 *     of the first failing group / member}, {BK_OK, 0} for an applied or an unmasked unit; and the env counts the refused
 *     units on the device: bk_retune_rejected waits for the env's stream and reads the count, cumulative over the env's life.
 *   - The _device entries are ONE kernel on the env's stream, ordered like bk_reset_books_device: no host synchronisation
 *     and, after the env's first retune (which makes the counter), no allocation.  rows_dev must be 4-byte
 *     (bk_random_agents) / 8-byte (bk_agent_desc) aligned.
 *   - The host entries check the masked units on the host first, with the installs' row builder: on the first failure
 *     nothing at all changes, the status is the install's and bk_last_error() names the unit and the group or member.
 *     Otherwise the rows go through pinned and device staging of the env's own (made at the first call) into the same
 *     kernel; the caller's arrays are free on return.
 *   - Checkpoints and snapshot slots hold no parameters and are not invalidated: a reset or a restore brings no
 *     parameters back (who restores retunes again for the old values), and one taken before a retune is usable after it
 *     and the other way round - the agent-set hash goes on naming the install, whose shape a retune cannot change.
 *     Conversely a checkpoint taken AFTER a retune restores only into an env that repeats the original install (the hash
 *     covers the installed records, thresholds and ranges included), and that env then runs the installed parameters: who
 *     wants to resume with the retuned ones retunes again after bk_checkpoint_load.
 * Refusals (BK_INVALID_ARGUMENT, the env unchanged): null env or rows, no matching per-unit table, a width mismatch, a
 * misaligned device pointer.  Envs with the agents' order log, device-ingress envs, markets and envs with snapshots held
 * all take it.  No counterpart in the reference beyond the assignment itself. */
int bk_retune_random_agents_device(bk_env* env, uint32_t n_groups, const bk_random_agents* rows_dev, const uint8_t* mask_dev,
                                   uint32_t* status_dev);
int bk_retune_random_agents(bk_env* env, uint32_t n_groups, const bk_random_agents* rows, const uint8_t* mask);
int bk_retune_agents_device(bk_env* env, uint32_t n_members, const bk_agent_desc* rows_dev, const uint8_t* mask_dev,
                            uint32_t* status_dev);
int bk_retune_agents(bk_env* env, uint32_t n_members, const bk_agent_desc* rows, const uint8_t* mask);
int bk_retune_rejected(bk_env* env, uint64_t* out);
/* sim_runner's loop body n_steps times for every book: agents.update(env, rng); env.step(rng)
 * (crates/step_sim/src/runner.rs:53-68), sharing each book's RNG between agents and shuffle. */
int bk_run(bk_env* env, uint64_t n_steps);
/* Warm-up without side effects: n_steps of this env's own kernels on its own books (same agents, pipeline and streams),
 * then state blocks, level-2 records and the step counter are put back; the scratch steps write no history slot and no
 * trade record.  For a short bk_run after host-side work: the GPU's clocks fall within milliseconds of idling and take
 * ~15 ms of load to come back, and a pipeline's first launch pays one-off set-up.  Asynchronous like bk_run.  (No
 * counterpart in the reference: a CPU has no launch set-up to hide.) */
int bk_warm(bk_env* env, uint64_t n_steps);
/* Opt-in order log of bk_run's RandomAgents (independent books and markets): every order the agents create is recorded
 * with its trader id (the agent's index within its group), status, remaining volume, arrival / end times and key, so that
 * bk_order_count / bk_get_orders / bk_order_status / bk_get_order_keys answer after bk_run as Env::get_orders /
 * order_status do after sim_runner (env.rs:253-290).  Needs max_orders > 0 (ids beyond it set BK_FLAG_ORDER_LOG_FULL and
 * the readers then return BK_CAPACITY); 80 B per order per book.  Call before the env's first bk_run.  Refused
 * (BK_INVALID_ARGUMENT) on a device-ingress env (which logs already) and with Noise / Momentum members installed
 * (bk_set_agents / bk_set_market_agents then refuse such members); bk_checkpoint_save, bk_checkpoint_load and
 * bk_load_book refuse a logging env (the log holds only the orders its own bk_run steps created).  A
 * logging env runs the split pipelines (split or wave_split in place of the fused ones) with the logging event kernel;
 * bk_warm's scratch steps leave the log and the id counters as they were.  on = 0 leaves an env without the log as it is
 * and is refused once the log is on (it cannot be switched off). */
int bk_set_agent_order_log(bk_env* env, int on);
/* One env runs ONE of the two order flows: once bk_run has stepped it with on-device agents, bk_place_order /
 * bk_cancel_order / bk_modify_order / bk_submit_instructions* / bk_step return BK_INVALID_ARGUMENT (host order ids would
 * restart at 0 and collide with the agents'); and bk_run refuses an env that holds host-placed orders. */

/* ------------------------------------------------------------------ readers */
/* Level-2 record width in u32: 5 + 4*levels, laid out as StepEnvNumpy.level_2_data
 * (rust/src/step_sim_numpy.rs:351-368): [trade_vol, bid_price, ask_price, ask_vol, bid_vol,
 * {bid_vol_i, bid_n_i, ask_vol_i, ask_n_i} for i < levels]. */
uint32_t bk_l2_width(const bk_env* env);
/* Env::level_2_data (end-of-step snapshot) for books [first, first+n): out[n][width] */
int bk_level2(bk_env* env, uint32_t first_book, uint32_t n_books, uint32_t* out);
/* Level2DataRecords + trade_vols (data.rs:9-57, env.rs:64,134): out[n_steps][n_books][width] for retained steps */
int bk_history_len(bk_env* env, uint64_t* first_step, uint64_t* n_steps);
int bk_history(bk_env* env, uint64_t first_step, uint64_t n_steps, uint32_t first_book, uint32_t n_books,
               uint32_t* out);
int bk_clear_history(bk_env* env);
/* Streaming egress: the history buffer is a ring of history_capacity steps; this queues the
 * device-to-host copy of retained steps on `copy_stream`, ordered after the work queued on the env so far, and returns
 * at once, so the next bk_run() overlaps the copy.  Keep history_capacity >= 2 x the chunk being copied; `out` should
 * come from bk_pinned_alloc().  Wait with bk_stream_sync(copy_stream). */
int bk_history_copy_async(bk_env* env, uint64_t first_step, uint64_t n_steps, uint32_t first_book, uint32_t n_books,
                          uint32_t* out, void* copy_stream);
int bk_stream_create(void** out);
int bk_stream_sync(void* stream);
int bk_stream_destroy(void* stream);
int bk_pinned_alloc(uint64_t nbytes, void** out);
int bk_pinned_free(void* p);
/* OrderBook::get_trades, orderbook.rs:800-802 */
int bk_trade_count(bk_env* env, uint32_t book, uint64_t* total, uint64_t* first_retained);
int bk_trade_counts(bk_env* env, uint64_t* totals /* [n_books] */);
int bk_get_trades(bk_env* env, uint32_t book, uint64_t first, uint64_t n, bk_trade* out);
int bk_clear_trades(bk_env* env);
/* Trade egress at scale (Env::get_trades, env.rs:277-280, for every book at once): bk_trades_compact gathers all
 * retained records into one dense device stream in the bk_trade layout with CSR offsets (book b owns
 * [offsets[b], offsets[b+1])) and marks them consumed (like bk_clear_trades); *out_total = number of records.
 * bk_trades_compact_copy_async copies that stream (records: out_total x bk_trade, offsets: n_books + 1) to the host on
 * `copy_stream`, ordered after the compaction (NULL: the env's stream, synchronous), so it overlaps the next bk_run.
 * A book whose records overflowed trade_capacity keeps its BK_FLAG_TRADE_OVERFLOW flag: nothing is dropped silently. */
int bk_trades_compact(bk_env* env, uint64_t* out_total);
int bk_trades_compact_copy_async(bk_env* env, bk_trade* records, uint64_t* offsets, void* copy_stream);
int bk_time(bk_env* env, uint32_t book, uint64_t* out);          /* OrderBook::get_time */
int bk_set_time(bk_env* env, uint32_t book, uint64_t t);         /* OrderBook::set_time, orderbook.rs:183-185 */
int bk_trade_vol(bk_env* env, uint32_t book, uint32_t* out);     /* OrderBook::get_trade_vol (live) */
int bk_steps_done(bk_env* env, uint64_t* out);
int bk_book_flags(bk_env* env, uint32_t* out /* [n_books] */);   /* sticky BK_FLAG_* bits */
/* clear the bits of `mask` in every book's sticky flags (the caller has seen and handled them) */
int bk_clear_flags(bk_env* env, uint32_t mask);
/* what a strict caller polls after a step: OR of every book's flags, and the largest number of trade records any book
 * retains (towards trade_capacity) - two words instead of n_books */
int bk_flags_summary(bk_env* env, uint32_t* flags_or, uint64_t* max_retained_trades);
int bk_rng_state(bk_env* env, uint32_t book, uint64_t out_state[2]);
/* resting (Active) orders of one book in price-time priority per side: bids first, then asks */
int bk_live_orders(bk_env* env, uint32_t book, uint32_t cap, bk_order* out, uint32_t* n_out);

/* ------------------------------------------------------ stats / multi-GPU */
/* reduce this shard's books into one 64-byte record on the device.  out_host != NULL: waits and copies the record to the
 * host.  out_host == NULL: fully asynchronous - the reduction is queued on the env's stream behind the stepping kernels
 * and never synchronises the host (the record is then read on the device through bk_stats_device_ptr, e.g. by an RCCL
 * all-gather on the same stream). */
int bk_stats_compute(bk_env* env, bk_stats* out_host);
/* device address of the 64-byte record (for an RCCL all-gather issued by the caller) */
int bk_stats_device_ptr(bk_env* env, void** out);
/* Device pointer of the latest level-2 records, u32[n_books][bk_l2_width()] (Env::level_2_data of every book), for
 * on-device consumers: the optional per-book L1 all-gather of SURVEY §8e (ii) reads its 9 leading words per book. */
int bk_level2_device_ptr(bk_env* env, void** out);

/* ------------------------------------------------------------- measurement */
/* accumulate HIP-event timings of the step kernels: on = 0 off, N >= 1 time the kernels of every Nth step */
int bk_profile_enable(bk_env* env, int on);
int bk_profile_read(bk_env* env, double* total_ms, uint64_t* n_launches, int reset);
/* per kernel: kind 0 the fused kernels (k_run_random / k_run_wave / k_run_mixed), 1 the agents kernel of a split pipeline
 * (k_agents_fsm / k_agents_wave / k_agents_mixed_*), 2 k_step_batch, 3 k_step_events (host-driven flow) */
int bk_profile_read_kind(bk_env* env, int kind, double* total_ms, uint64_t* n_launches);
/* bk_run kernel pipeline: 0 auto (by shape and batch size), 1 fused (one wave per book, all phases),
 * 2 split (RNG-serial phases one lane per book + event phase one wave per book), 3 split with the members of an AgentSet
 * decoded one wave per book (older form of 4), 4 / 5 below.  Results are identical; only speed differs. */
int bk_set_pipeline(bk_env* env, int mode);
/* Mode 4 on an AgentSet with Noise / Momentum members (independent books): the members' update one WAVE per book with
 * their stream decoded 64 draws at a time (k_agents_mixed_wave) + the event kernel; auto from 512 books.  A RandomAgents
 * member of such a set is walked on that kernel's scalar path (same results).  Markets (assets > 1): as mode 2.
 * Modes 4 ("wave_split") and 5 ("wave") on RandomAgents books: the RNG-serial phases run one WAVE per
 * book with the book's xoroshiro stream decoded 64 draws at a time (jump-ahead lane states + ballot/prefix resolution) -
 * as a kernel of its own in front of the event kernel (4), or fused with the event phase in one persistent kernel that
 * keeps the book in registers across all steps of a bk_run (5).  bk_set_wave_options: look-ahead of the decode's vector
 * path (1..64 draws, default 64; smaller values push placements onto its scalar slow path - a test knob) and the number
 * of parts mode 4 cuts the batch in (0 = default). */
int bk_set_wave_options(bk_env* env, uint32_t lookahead, int parts);
/* DEPRECATED, always *out = 0; kept only so that clients built against rounds 1-3 still link.  (Those rounds rolled an
 * auto-selected launch of the lane-per-book members' update back when it overflowed a pool the other kernels still fit,
 * and counted the roll-backs here; the auto rule has not picked that pipeline since round 3.) */
int bk_pipeline_fallbacks(bk_env* env, uint64_t* out);
/* the pipeline bk_run will use: *split = 0 fused / 1 split (lane-per-book agents) / 2 wave_split / 3 wave; *n_parts =
 * contiguous book parts launched on separate streams */
int bk_get_pipeline(bk_env* env, int* split, int* n_parts);
uint64_t bk_state_bytes_per_book(const bk_env* env);
/* split-pipeline geometry: the batch is cut in min(n_parts, books / min_part) contiguous parts, each on its own HIP
 * stream (defaults 4 - one per hardware queue - and 4096; n_parts in 1..8, min_part >= 64).  Results never depend on it. */
int bk_set_split_parts(bk_env* env, int n_parts, uint32_t min_part);
int bk_get_split_parts(bk_env* env, int* n_parts, uint32_t* min_part); /* the two settings as stored */
/* orders created so far in every book by the on-device agents: OrderBook::current_order_id / orders.len()
 * (crates/order_book/src/orderbook.rs:327-329), totals[n_books] */
int bk_order_counts(bk_env* env, uint64_t* totals /* [n_books] */);
/* A diagnostic of the host-driven / ingress step (bk_step, bk_step_async: Env::step over submitted instructions,
 * crates/step_sim/src/env.rs:116-135): how many of each book's steps ran on the keyed event loop - steps without
 * modifications whose events fit one per pool slot, on a trading book, with prices and arrival stamps inside the key window
 * (bourse_amd/csrc/step_events.hpp step_events_keyed); the others ran the event-by-event loop.  Results never depend on it. */
int bk_event_steps_keyed(bk_env* env, uint64_t* counts /* [n_books] */);
/* A diagnostic of the stamp compaction (bourse_amd/csrc/stamp_rows.hpp): how many times this env has queued
 * it so far - in front of a launch that could have taken a book's arrival-stamp counter past 2^32 - 1 (or past the room
 * BOURSE_AMD_STAMP_ROOM leaves), and once per bk_checkpoint_load.  Results never depend on it.  (No counterpart in the
 * reference.) */
int bk_stamp_compactions(bk_env* env, uint64_t* out);

/* ------------------------------------------------------ checkpoint / resume */
/* Dump / restore the complete simulation state of an on-device-order-flow env (pool, clock, counters, per-book
 * RNG).  The image starts with a versioned header (magic, shape, levels, assets, a hash of the installed agent set):
 * bk_checkpoint_load refuses an image taken from a differently shaped env or with different agents.  The reference has no counterpart: its Env/agents/RNG are not serialisable (only OrderBook JSON snapshots,
 * crates/order_book/src/orderbook.rs:811-832).  A restored env continues bit-identically. */
uint64_t bk_checkpoint_bytes(const bk_env* env);
int bk_checkpoint_save(bk_env* env, void* out, uint64_t nbytes);
int bk_checkpoint_load(bk_env* env, const void* in, uint64_t nbytes);

/* ------------------------------------------------------ per-book reset to a device-resident snapshot */
/* Chosen books of an on-device-order-flow env go back to a snapshot that never leaves the device, while the others carry
 * on: episodes that end at different times per book, a finished parameter row of a sweep started again.  The reference
 * has no counterpart for any of these entries: its Env is rebuilt, never rewound, and one Env is one book.
 * The unit of a reset is a book, or with assets > 1 a market (its books share one RNG stream): n_units = n_books /
 * assets.  Every refusal below is BK_INVALID_ARGUMENT, is checked before anything is enqueued and leaves the env unchanged:
 * slot >= BK_MAX_SNAPSHOTS, and - the conditions bk_checkpoint_save refuses on, for the same reasons - an env with the
 * device ingress (its queues, order records and held ids have to be rewound as well: it has entries of its own,
 * bk_ingress_snapshot_save / bk_ingress_reset_books* below), an env with the agents' order log (the log would keep the
 * abandoned run's orders), an env that holds host-placed orders. */
#define BK_MAX_SNAPSHOTS 4
/* Device bytes one slot costs: n_books * (pool block + level-2 row) * 4.  (No counterpart in the reference.) */
uint64_t bk_snapshot_bytes(const bk_env* env);
/* Device-to-device copy of every book's state block and level-2 record into `slot` (allocated at its first save,
 * overwritten by a later one), with the agent set's hash and the env's shape recorded beside it.  Asynchronous on the
 * env's stream.  (No counterpart in the reference.) */
int bk_snapshot_save(bk_env* env, uint32_t slot);
/* Frees the slot's memory (waits for the env's stream first); dropping an empty slot is not an error; bk_env_destroy
 * drops every slot.  (No counterpart in the reference.) */
int bk_snapshot_drop(bk_env* env, uint32_t slot);
/* Units u with mask_dev[u] != 0 return to their state in `slot`; the others are not touched.  mask_dev [n_units] bytes and
 * seeds_dev [n_units] u64 (nullable) are DEVICE memory written on the env's stream - by the caller's own kernels, for
 * instance.  A reset unit gets back everything its books held at the save (pool, clock, id / step / event counters, trade
 * volume, RNG, the members' state in the block) except: no trade record of the abandoned run stays retained (bk_trade_count
 * = {the snapshot's total, first_retained = the same}); sticky flags are kept (snapshot's | current; bk_clear_flags clears);
 * the trading flag is the env's current one; with seeds_dev, the unit's RNG is seed_from_u64(seeds_dev[u]) as bk_env_create
 * seeds it (in every book of a market).  Not rewound: bk_steps_done, the history ring (a reset book keeps writing its rows
 * at the env's step index), the other books.  Noise / Momentum members' lists are rebuilt from the pools by the next bk_run.
 * HOLDS NO HOST SYNCHRONISATION: one kernel launch on the env's stream - no stream wait, no host read of the mask, no
 * allocation.  Further refusals: empty slot, null mask, a slot saved with another agent set or shape ("install the same
 * agents first", as bk_checkpoint_load).  (No counterpart in the reference.) */
int bk_reset_books_device(bk_env* env, uint32_t slot, const uint8_t* mask_dev, const uint64_t* seeds_dev);
/* The same from HOST arrays: mask and seeds are staged in two env-owned device buffers (allocated at the first call),
 * copied on the env's stream, and the copy is waited for - the caller's arrays are free on return; the reset itself
 * stays asynchronous.  (No counterpart in the reference.) */
int bk_reset_books(bk_env* env, uint32_t slot, const uint8_t* mask_host, const uint64_t* seeds_host);

/* ------------------------------------------------------ per-book reset of a device-ingress env */
/* The same for an env with the device ingress (bk_device_ingress_enable), which the entries above refuse: besides the state
 * block and the level-2 record of its books, a reset unit (book, or market) gets back everything else such an env keeps for
 * it - the order records (bk_get_orders / bk_order_status) of the ids it had handed out at the save, the held ids of
 * bk_update_agents, the lists, lengths, momentum state and flags of bk_update_members - and its queue is EMPTIED: what was
 * submitted or queued by an update for the unit since the last step is dropped, and the ids and statuses already written
 * to the caller's out_ids / status arrays for those instructions are void.  The natural place for a reset is right after
 * a step.  The slots are BK_MAX_SNAPSHOTS of their own, apart from bk_snapshot_save's.  Fix-ups and what is not rewound
 * (bk_steps_done, the history ring, the other units) are bk_reset_books_device's.  Every refusal is BK_INVALID_ARGUMENT,
 * checked before anything is enqueued, and leaves the env unchanged: null env, slot >= BK_MAX_SNAPSHOTS, an env without
 * the device ingress (its entries are bk_snapshot_save / bk_reset_books).  Checkpoints and bk_run of a device-ingress env
 * stay refused. */
/* Device-to-device copy of the above into `slot` (overwritten by a later save; its record arrays grow if the books have
 * handed out more ids since).  If no bk_update_agents / bk_update_members has run since the agents were installed, the
 * slot records that they hold nothing yet, and a reset puts them back there.  MAY SYNCHRONISE: it waits for the env's
 * stream and reads one word back to size the slot.  (No counterpart in the reference.) */
int bk_ingress_snapshot_save(bk_env* env, uint32_t slot);
/* Frees the slot's memory (waits for the env's stream first); dropping an empty slot is not an error.  (No counterpart
 * in the reference.) */
int bk_ingress_snapshot_drop(bk_env* env, uint32_t slot);
/* Device bytes the slot holds; 0 for an empty slot.  This is what is ALLOCATED, not what the last save used: the record
 * arrays grow with a save that finds more ids per book and never shrink, so a slot saved again with fewer ids reports the
 * size of its largest save until it is dropped.  (No counterpart in the reference.) */
uint64_t bk_ingress_snapshot_bytes(const bk_env* env, uint32_t slot);
/* Units u with mask_dev[u] != 0 return to their state in `slot`; mask_dev [n_units] bytes and seeds_dev [n_units] u64
 * (nullable) are DEVICE memory written on the env's stream.  HOLDS NO HOST SYNCHRONISATION: launches on the env's stream
 * only - no stream wait, no host read, no allocation - and an all-zero mask costs a time that does not depend on how many
 * orders the slot holds.  Further refusals: empty slot, null mask, a slot saved with another agent set or shape ("install
 * the same agents first"), and ANY bk_set_*agents* call since the save, the same agents included (it makes the next update
 * start from empty hands, which would wipe what a reset restored: save again).  (No counterpart in the reference.) */
int bk_ingress_reset_books_device(bk_env* env, uint32_t slot, const uint8_t* mask_dev, const uint64_t* seeds_dev);
/* The same from HOST arrays, staged and waited for as bk_reset_books stages them; the reset itself stays asynchronous.
 * (No counterpart in the reference.) */
int bk_ingress_reset_books(bk_env* env, uint32_t slot, const uint8_t* mask_host, const uint64_t* seeds_host);

/* ------------------------------------------------------ trader accounts of a device-ingress env */
/* An opt-in table acct[n_books][n_traders] in DEVICE memory: what each trader bought and sold in each book, folded from
 * the book's new trade records on the env's stream right behind every step's event kernel, with no host synchronisation
 * anywhere on that path (bourse_amd/csrc/accounts.hpp).  A strategy that submits from device memory reads
 * its own fills, inventory and cash there instead of joining bk_get_trades with bk_get_orders on the host.  The reference
 * has no counterpart for any of these entries.
 *
 * Which fills a book's rows record.  The buyer of a trade record is the PASSIVE order's trader when side_is_bid == 1,
 * otherwise the ACTIVE order's trader; the other trader is the seller.  A trader id >= n_traders is skipped without a flag:
 * give background members (bk_set_agents*, bk_set_random_agents*) an agent_id_start above n_traders to keep them out.
 * Markets need nothing special: a book of a market is a book, and the rows are per book (market * assets + asset).
 *
 * Arithmetic.  All of it is modulo 2^64, two's complement; vol * price is the full 32 x 32 -> 64-bit product. */
typedef struct bk_account { /* 32 B, all little-endian 64-bit words */
  int64_t position; /* + vol for every fill as buyer, - vol as seller */
  int64_t cash;     /* - vol * price as buyer, + vol * price as seller (price = the trade record's: the passive order's) */
  uint64_t volume;  /* sum of vol over the trader's fills, either side */
  uint64_t fills;   /* trade records the trader took part in (a self-trade counts twice) */
} bk_account;
/* Enabling.  Accepted only on an env with the device ingress (bk_device_ingress_enable), with max_orders > 0 (the traders
 * of a record's orders are looked up in the order records), before the first instruction, update or step, and while no
 * ingress snapshot slot is held.  Refuses n_traders == 0, n_traders > 65536 and a second call.  A refusal returns
 * BK_INVALID_ARGUMENT, leaves the env unchanged and puts the reason in bk_last_error().
 *
 * The fold and its cursor.  The fold runs after every bk_step_async / bk_step of such an env.  Each book has a cursor
 * (a device array of its own, acct_seen[n_books]; the state block's layout is unchanged) counting the trades already
 * folded.  A record that cannot be folded - it was dropped beyond trade_capacity, or one of its order ids is >= max_orders
 * - sets the sticky flag BK_FLAG_ACCOUNTS_INEXACT on that book and the cursor moves past it: inexact rows are flagged,
 * never silent.  Other books are unaffected.
 *
 * consume_trades.  With consume_trades = 1 the fold ends by setting the book's first retained trade to its trade count
 * (bk_trade_count: first_retained == total), exactly as bk_clear_trades does: trade_capacity then only has to hold ONE
 * step's trades.  With consume_trades = 0 the host's trade readers and bk_trades_compact see what they see today (the
 * fold has run on the stream before any of them can mark a step's records consumed).
 *
 * bk_load_book is refused on an env with accounts.  Behaviour of an env without accounts does not change.
 * (No counterpart in the reference.) */
int bk_accounts_enable(bk_env* env, uint32_t n_traders, int consume_trades);
/* Device pointer of the table, bk_account[n_books][n_traders], for on-device consumers; valid for the env's life, written
 * on the env's stream.  BK_INVALID_ARGUMENT without accounts.  (No counterpart in the reference.) */
int bk_accounts_device_ptr(bk_env* env, void** out);
/* Rows of books [first_book, first_book + n_books) to host memory, n_books * n_traders records.  Waits for the env's
 * stream.  (No counterpart in the reference.) */
int bk_get_accounts(bk_env* env, uint32_t first_book, uint32_t n_books, bk_account* out);
/* Clearing.  Zeroes the rows of the books b with mask[b] != 0 (mask [n_books] bytes; NULL = every book) and sets their
 * cursor to the book's current trade count: a cleared book counts from here.  bk_ingress_reset_books* does the same for
 * the books it resets (every book of a reset market), after its own kernels, on the same stream, using the same device
 * mask: accounts are not part of a snapshot, and a reset book counts from its reset, which is what an episode wants.
 * From a HOST mask: staged on the env's stream and waited for, the clear itself stays asynchronous.  (No counterpart in
 * the reference.) */
int bk_accounts_clear(bk_env* env, const uint8_t* mask_host);
/* The same from DEVICE memory written on the env's stream (NULL = every book).  HOLDS NO HOST SYNCHRONISATION: one launch
 * on the env's stream.  (No counterpart in the reference.) */
int bk_accounts_clear_device(bk_env* env, const uint8_t* mask_dev);

/* ------------------------------------------------------ per-step trade bars of a device-ingress env */
/* An opt-in ring bars[n_books][window] in DEVICE memory: WHAT TRADED in each book in each of the last `window` steps - the
 * first, highest, lowest and last trade price, the volume whose aggressor bought and sold, the notional behind a VWAP and
 * the record counts - folded from the book's new trade records on the env's stream right behind every step's event kernel,
 * with no host synchronisation anywhere on that path (bourse_amd/csrc/trade_bars.hpp).  It is the
 * market-wide counterpart of the per-trader accounts above: a policy that observes and acts in device memory reads signed
 * flow, last price and the step's range there instead of waiting for bk_get_trades.  The reference has no counterpart for
 * any of these entries.
 *
 * Which step goes where.  The step that bk_step_async / bk_step runs while bk_steps_done reads k is folded into slot
 * k % window of every book.  A trade record whose PASSIVE order was an ask (side_is_bid == 0) is a buy, one with
 * side_is_bid == 1 a sell: the aggressor's side, the same reading of the field as the accounts'.  Every record counts,
 * whoever owns its orders; no order record is looked up.  open / close are the prices of the first / last of the step's
 * records in the book's record order, high / low the largest / smallest.  A book-step without a trade overwrites its slot
 * all the same: open = high = low = close = the close of the previous step's slot ((k - 1) % window, read before the write),
 * every other word 0; before a book's first trade since enable, clear or reset that carried price is 0.  Rows are per book,
 * so markets need nothing special (market * assets + asset).
 *
 * Arithmetic.  The 64-bit words are sums modulo 2^64, vol * price the full 32 x 32 -> 64-bit product; the counts wrap
 * modulo 2^32. */
typedef struct bk_trade_bar { /* 48 B, three 16-byte vectors, little-endian */
  uint32_t open, high, low, close; /* prices of the step's trade records, in record order */
  uint64_t buy_vol, sell_vol;      /* volume whose aggressor bought / sold */
  uint64_t notional;               /* sum of vol * price */
  uint32_t n_buy, n_sell;          /* records whose aggressor bought / sold */
} bk_trade_bar;
/* Enabling.  Accepted on an env with the device ingress (bk_device_ingress_enable), at any time - also mid-run and while an
 * ingress snapshot slot is held: the rows are not part of a snapshot.  Zeroes all rows and starts every book's cursor (a
 * device array of its own, bars_seen[n_books]; the state block's layout is unchanged) at its current trade count: steps
 * before the call leave zero rows.  Refuses window outside 1..1024 and a second call.  A refusal - here and in the entries
 * below - returns BK_INVALID_ARGUMENT, leaves the env unchanged and puts the reason in bk_last_error().
 *
 * A record the fold cannot read - dropped beyond trade_capacity - is stepped over: the bar is that of the records that
 * could be read.  Such a book carries BK_FLAG_TRADE_OVERFLOW already (the step's kernel set it when it dropped the record),
 * so an inexact bar is never silent; no flag bit of its own is added.  The fold runs in the same call as the step's
 * kernel, so nothing can consume a step's records before the fold has seen them.
 *
 * consume_trades.  With consume_trades = 1 the folded records are marked consumed as bk_clear_trades does:
 * trade_capacity then only has to hold ONE step's trades.  On an env that also has accounts the bars' fold runs first and
 * the accounts' fold consumes, once, if either feature asked for it: neither fold hides a record from the other.
 *
 * bk_ingress_reset_books* zeroes all `window` rows of the books it resets (every book of a reset market) and moves their
 * cursors to the restored trade count, where it clears the accounts.  bk_load_book is refused on an env with bars.
 * Behaviour of an env without bars does not change.  (No counterpart in the reference.) */
int bk_trade_bars_enable(bk_env* env, uint32_t window, int consume_trades);
/* Device pointer of the ring, bk_trade_bar[n_books][window], for on-device consumers; valid for the env's life, written
 * on the env's stream.  BK_INVALID_ARGUMENT without bars.  (No counterpart in the reference.) */
int bk_trade_bars_device_ptr(bk_env* env, void** out);
/* The slot the latest folded step went to, (bk_steps_done - 1) % window (window - 1 before the first step): a host
 * integer, no wait.  (No counterpart in the reference.) */
int bk_trade_bars_slot(bk_env* env, uint32_t* out);
/* Rows of books [first_book, first_book + n_books) to host memory, n_books * window records.  Waits for the env's
 * stream.  (No counterpart in the reference.) */
int bk_get_trade_bars(bk_env* env, uint32_t first_book, uint32_t n_books, bk_trade_bar* out);
/* Clearing.  Zeroes all rows of the books b with mask[b] != 0 (mask [n_books] bytes; NULL = every book) and sets their
 * cursor to the book's current trade count: the carried price starts at 0 again.  From a HOST mask: staged on the env's
 * stream and waited for, the clear itself stays asynchronous.  (No counterpart in the reference.) */
int bk_trade_bars_clear(bk_env* env, const uint8_t* mask_host);
/* The same from DEVICE memory written on the env's stream (NULL = every book).  HOLDS NO HOST SYNCHRONISATION: one launch
 * on the env's stream.  (No counterpart in the reference.) */
int bk_trade_bars_clear_device(bk_env* env, const uint8_t* mask_dev);

/* ------------------------------------------------------ per-book series moments of the level-2 history */
/* An opt-in table series[n_books] in DEVICE memory: one row of integer sums per book over the book's whole SERIES of
 * level-2 records - what a sweep or a calibration wants back from every book (mean and variance of the spread, moments of
 * the mid-price returns, their lag-1 autocovariance and that of their magnitudes, traded volume, depth) - folded on the
 * env's stream from the history ring that the stepping kernels already write, with no host wait and without the history
 * ever leaving the device (bourse_amd/csrc/series.hpp, series_fold.hpp).  It serves every flow that writes
 * the ring - bk_run on all pipelines, bk_step, the device ingress, markets - and touches no stepping kernel.  The
 * reference has no counterpart for any of these entries.
 *
 * What one record adds.  Of the record of step s and book b only the first five words are read, {trade_vol, bid_price,
 * ask_price, ask_vol, bid_vol}; an empty side reads bid_price == 0 / ask_price == 0xFFFFFFFF, trade_vol is the step's own.
 * The book's carry is {have_m, m_prev, have_d, d_prev}.
 *   always:            n_steps += 1, sum_trade_vol += tv, sum_trade_vol_sq += tv * tv, n_trade_steps += (tv > 0),
 *                      sum_bid_vol += bid_vol, sum_ask_vol += ask_vol;
 *   two-sided (bid != 0 && ask != 0xFFFFFFFF), m = bid + ask (TWICE the mid), sp = ask - bid (u32 wrapping):
 *                      n_two_sided += 1, sum_m += m, sum_spread += sp, sum_spread_sq += sp * sp, min_m, max_m;
 *   two-sided and have_m, d = m - m_prev (signed, |d| < 2^33), a = |d|:
 *                      n_ret += 1, sum_d += d, sum_abs_d += a, sum_d2 += a * a, sum_d4 += a^4 (a 128-bit pair, the power
 *                      exact modulo 2^128), max_abs_d;
 *   and have_d:        n_pairs += 1, sum_dd += d * d_prev (signed), sum_abs_dd += a * |d_prev|;
 *   then the carry:    two-sided: m_prev = m, have_m = 1, and have_d = 1, d_prev = d if there was a return, else have_d = 0;
 *                      one-sided: have_m = have_d = 0.  A word whose have_ bit is clear is 0.
 * A one-sided step breaks the chain: a return exists only between two CONSECUTIVE two-sided steps, a pair only over three.
 * All 64-bit words are sums modulo 2^64, sum_d4 a sum modulo 2^128; signed words are two's complement.  The carry words
 * exist so that folding steps [x, y) and then [y, z) leaves the same row as one fold over [x, z), for every split. */
typedef struct bk_series_row { /* 192 B, twelve 16-byte vectors, little-endian */
  uint64_t n_steps, n_two_sided;
  uint64_t sum_m, sum_spread, sum_spread_sq; /* of two-sided steps; m = bid + ask, twice the mid */
  uint64_t sum_bid_vol, sum_ask_vol;         /* of every step */
  uint64_t sum_trade_vol, sum_trade_vol_sq, n_trade_steps;
  uint64_t n_ret;
  int64_t sum_d;
  uint64_t sum_abs_d, sum_d2, sum_d4_lo, sum_d4_hi, max_abs_d;
  uint64_t n_pairs;
  int64_t sum_dd;
  uint64_t sum_abs_dd;
  uint64_t min_m, max_m; /* 2^64 - 1 and 0 before the first two-sided step */
  uint64_t carry_m;      /* m_prev, bit 63 = have_m, bit 62 = have_d */
  int64_t carry_d;       /* d_prev */
} bk_series_row;
/* Enabling.  Accepted on any env with history_capacity > 0, at any time, once.  Allocates the rows (arrays of their own:
 * the state block, checkpoints and snapshots are unchanged), clears every row - all zeros except min_m = 2^64 - 1 - and
 * sets the env's step cursor series_seen, a host integer as bk_steps_done is, to bk_steps_done: earlier steps are not
 * counted.  A refusal - here and in the entries below: a null env, history_capacity == 0, a second call, any other entry
 * before this one - returns BK_INVALID_ARGUMENT, leaves the env unchanged and puts the reason in bk_last_error().
 *
 * bk_reset_books* and bk_ingress_reset_books* on such an env first fold what is outstanding (and refuse the reset if
 * steps were lost, see bk_series_fold), then zero only the carry words of the books they reset (every book of a masked
 * market): the sums go on across episodes and no return spans a reset; clear by mask if a new row is wanted.
 * bk_checkpoint_load clears every row and sets the cursor to the restored step count.  bk_load_book is refused.  bk_warm
 * writes no history and restores the counter: unaffected.  An env without the table launches nothing new.  (No counterpart
 * in the reference.) */
int bk_series_enable(bk_env* env);
/* Queues, on the env's stream and without any host wait, the fold of steps [series_seen, bk_steps_done) of every book;
 * then series_seen = bk_steps_done.  No new step: no launch.  If a step of that range is no longer retained by the ring -
 * it wrapped (more than history_capacity steps since the last fold), or bk_clear_history was called - returns
 * BK_INVALID_ARGUMENT with the number of lost steps in bk_last_error() and leaves rows and cursor unchanged: a lost step
 * is never silent and needs no flag bit.  bk_series_clear with a NULL mask is the way on.  (No counterpart in the reference.) */
int bk_series_fold(bk_env* env);
/* Clearing.  mask [n_books] bytes, one per BOOK.  With a mask: folds what is outstanding first (refusing as bk_series_fold
 * does), then clears the rows, carry included, of the books b with mask[b] != 0.  NULL: clears every row and sets the
 * cursor to bk_steps_done WITHOUT folding.  From a HOST mask: staged on the env's stream and waited for, the clear itself
 * stays asynchronous.  (No counterpart in the reference.) */
int bk_series_clear(bk_env* env, const uint8_t* mask_host);
/* The same from DEVICE memory written on the env's stream (NULL = every book).  HOLDS NO HOST SYNCHRONISATION: at most
 * two launches on the env's stream.  (No counterpart in the reference.) */
int bk_series_clear_device(bk_env* env, const uint8_t* mask_dev);
/* Device pointer of the table, bk_series_row[n_books], for on-device consumers; valid for the env's life, written on the
 * env's stream.  (No counterpart in the reference.) */
int bk_series_device_ptr(bk_env* env, void** out);
/* Rows of books [first_book, first_book + n_books) to host memory.  Waits for the env's stream; does NOT fold.
 * (No counterpart in the reference.) */
int bk_get_series(bk_env* env, uint32_t first_book, uint32_t n_books, bk_series_row* out);

/* ------------------------------------------------------ per-level depth table, the series moments' companion */
/* An opt-in table depth[n_books][L + 1][16] of uint64_t in DEVICE memory, L = cfg.levels (1..64), 128 B a row: the LADDER
 * half of the series moments.  bk_series_* reads words 0..4 of a level-2 record; this table reads the other 4 L, the levels
 * {bid_vol_i, bid_n_i, ask_vol_i, ask_n_i} as the stepping kernels wrote them - per level the sums behind the average book
 * shape (mean and variance of resting volume and order count, how often the level is occupied) and behind the response of
 * the next move of the mid to the cumulative depth imbalance (bourse_amd/csrc/depth.hpp, depth_fold.hpp).
 * It is no table of its own: it shares the series' cursor, and bk_series_fold, bk_series_clear*, bk_reset_books* and
 * bk_ingress_reset_books* (which cut the carry), bk_checkpoint_load (which clears) act on both tables.  It has no fold or
 * clear entry and adds no flag bit.
 *
 * What one record adds.  Let level q of the record of step s be bv, bn, av, an; two = the step is two-sided (bid != 0 &&
 * ask != 0xFFFFFFFF); m = bid + ask; I_q = sum_{i <= q} bv_i - sum_{i <= q} av_i, an exact integer (|I_q| < 2^38).  A PAIR
 * is two consecutive folded steps s - 1, s, both two-sided, with no cut between them; for a pair d = m_s - m_{s-1} and
 * J = I_q(s - 1).  Row q < L, word by word:
 *    0, 1  sum_bid_vol, sum_ask_vol         sum of bv, of av, over every step
 *    2, 3  sum_bid_vol_sq, sum_ask_vol_sq   sum of bv^2, of av^2
 *    4, 5  sum_bid_orders, sum_ask_orders   sum of bn, of an
 *    6, 7  n_bid_steps, n_ask_steps         steps with bn > 0, with an > 0
 *    8     sum_imb                          sum of I_q over two-sided steps (signed)
 *    9     sum_imb_sq                       sum of I_q^2 over two-sided steps
 *   10     n_signed                         pairs with J != 0
 *   11     sum_sign_d                       sum of sgn(J) * d over pairs (signed)
 *   12     n_agree                          pairs with sgn(J) * d > 0
 *   13     sum_imb_d                        sum of J * d over pairs (signed)
 *   14     n_move                           pairs with J != 0 and d != 0
 *   15     sum_abs_imb                      sum of |I_q| over two-sided steps
 * Row L, the header: 0 n_steps (steps folded since the last clear), 1 n_two_sided, 2 n_pairs, 3 sum_d (signed), 4 sum_abs_d,
 * 5 n_up, 6 n_down (pairs with d > 0, with d < 0), 7 n_bid_side, 8 n_ask_side (steps with bid != 0, with ask != 0xFFFFFFFF),
 * 9..15 zero.  All sums are modulo 2^64; signed words are two's complement.  With a huge tick several levels may alias:
 * that is the record's affair, the table takes the levels as they stand.
 *
 * The carry, uint64_t[n_books][L + 1], is I_q of the last folded step per level and then that step's window word (bit 63
 * set if two-sided, the low bits m).  A cut zeroes the whole carry, so no pair reaches over a reset and the sums go on.
 * Folding steps [x, y) and then [y, z) leaves exactly the rows and carry of one fold over [x, z), for every split.
 *
 * Enabling.  Needs bk_series_enable on the same env (else BK_INVALID_ARGUMENT, bk_last_error() names bk_series_enable);
 * refuses a second call.  First folds the series' outstanding steps - if steps were lost that fold refuses as
 * bk_series_fold does, and so does the enable, the env unchanged - then allocates and clears rows and carry: both tables
 * stand at bk_steps_done and the depth rows count from here.  A clear that cannot be launched leaves the env without the
 * table.  An env without it launches nothing new.  (No counterpart in the reference.) */
int bk_depth_enable(bk_env* env);
/* Device pointer of the table, uint64_t[n_books][L + 1][16], for on-device consumers; valid for the env's life, written on
 * the env's stream.  On an env without the table: BK_INVALID_ARGUMENT, "this env has no depth table: call bk_depth_enable
 * first".  (No counterpart in the reference.) */
int bk_depth_device_ptr(bk_env* env, void** out);
/* Rows of books [first_book, first_book + n_books) to host memory, (L + 1) * 16 words per book.  Waits for the env's
 * stream; does NOT fold (bk_series_fold folds both tables).  (No counterpart in the reference.) */
int bk_get_depth(bk_env* env, uint32_t first_book, uint32_t n_books, uint64_t* out);

/* ------------------------------------------------------ per-book candle table, the series moments' other companion */
/* An opt-in table candles[n_books][N][16] of uint64_t in DEVICE memory, 128 B a row: per book a ring of the last N bars of W
 * steps each - the PATH that bk_series_* collapses to one row: how mid, spread, volume and volatility evolved.  It reads
 * words 0..2 of a level-2 record {trade_vol, bid_price, ask_price} as the stepping kernels wrote them
 * (bourse_amd/csrc/candles.hpp, candle_fold.hpp).  It is no table of its own: it shares the series' cursor,
 * and bk_series_fold, bk_series_clear*, bk_reset_books* and bk_ingress_reset_books* (which cut the carry), bk_checkpoint_load
 * (which clears) act on it too.  It has no fold or clear entry and adds no flag bit.
 *
 * Bars are aligned to the env's absolute step count (bk_steps_done), the same for every book: step s belongs to bar
 * j = s / W, and bar j lives in slot j % N of every book.  The newest folded bar is that of step seen - 1, seen the series'
 * cursor - a host integer.
 *
 * What one record adds.  two = the step is two-sided (bid != 0 && ask != 0xFFFFFFFF); m = bid + ask, twice the mid (up to
 * 33 bits).  A RETURN d = m_s - m_{s-1} exists where steps s - 1 and s are consecutive folded steps, both two-sided, with
 * no cut between them - the series' own rule; it counts in the bar of the LATER step s, the earlier may lie in the bar
 * before.  The row of bar j, word by word:
 *    0  first_step     absolute step of the first record folded into this bar
 *    1  n_steps        records folded into it; 0: the slot holds no bar; < W: a partial bar - the newest, or the first
 *                      behind an enable or a clear
 *    2  n_two_sided    records with two
 *    3  open_m         m of the first two-sided step        (3..6 are 0 while n_two_sided == 0)
 *    4  high_m         the largest m
 *    5  low_m          the smallest m
 *    6  close_m        m of the last two-sided step
 *    7  sum_m          sum of m over two-sided steps; sum_m / (2 n_two_sided) is the time-weighted mid
 *    8  sum_spread     sum of (ask - bid), a wrapping u32, over two-sided steps
 *    9  sum_trade_vol  sum of trade_vol over every step
 *   10  n_trade_steps  steps with trade_vol > 0
 *   11  n_ret          returns whose later step lies in this bar
 *   12  sum_d          sum of d (signed, two's complement)
 *   13  sum_abs_d      sum of |d|
 *   14  sum_d2         sum of d^2; divided by 4 the realised variance in mid-price units
 *   15  max_abs_d      the largest |d|
 * All sums are modulo 2^64.
 *
 * The merge.  The row of slot j % N is CONTINUED if n_steps > 0 and first_step / W == j, else RESTARTED with first_step the
 * first folded step of bar j.  Folding steps [x, y) and then [y, z) leaves exactly the rows and carry of one fold over
 * [x, z), for every split.  A fold may span more bars than N: bar j with j + N <= (the bar of the fold's last step) is then
 * not written, its slot is a later bar's.  The carry, uint64_t[n_books], is the window word of the last folded step (bit
 * 63 set if two-sided, the low bits m); a cut zeroes it, so no return reaches over a reset, and the rows go on.
 *
 * Enabling.  width W in 1..1048576, n_candles N in 1..65536 (else BK_INVALID_ARGUMENT).  Needs bk_series_enable on the same
 * env (else BK_INVALID_ARGUMENT, bk_last_error() names bk_series_enable); refuses a second call.  First folds the series'
 * outstanding steps - if steps were lost that fold refuses as bk_series_fold does, and so does the enable, the env
 * unchanged - then allocates and clears rows and carry: the bars count from bk_steps_done on.  An allocation that fails is
 * BK_HIP_ERROR and leaves the env without the table, as does a clear that cannot be launched.  An env without the table
 * launches nothing new.  bk_depth_enable and this may both be called, in either order.  (No counterpart in the reference.) */
int bk_candles_enable(bk_env* env, uint32_t width, uint32_t n_candles);
/* out[0] = W, out[1] = N as enabled.  One record adds nothing here: the shape is fixed at the enable.  On an env without
 * the table: BK_INVALID_ARGUMENT, "this env has no candle table: call bk_candles_enable first".
 * (No counterpart in the reference.) */
int bk_candles_config_get(bk_env* env, uint32_t out[2]);
/* Device pointer of the table, uint64_t[n_books][N][16], for on-device consumers; valid for the env's life, written on the
 * env's stream: one record adds to the one row of its bar's slot.  (No counterpart in the reference.) */
int bk_candles_device_ptr(bk_env* env, void** out);
/* Rows of books [first_book, first_book + n_books) to host memory, N * 16 words per book, slot by slot: one record has
 * added to the row of slot (s / W) % N.  Waits for the env's stream; does NOT fold (bk_series_fold folds both tables).
 * (No counterpart in the reference.) */
int bk_get_candles(bk_env* env, uint32_t first_book, uint32_t n_books, uint64_t* out);

/* ------------------------------------------------------ per-book lag table of the level-2 history */
/* An opt-in table lags[n_books][n_lags] in DEVICE memory, n_lags = K, 1 <= K <= 64: per book and lag k = 1 .. K the sums
 * behind the autocorrelation of the mid's step-to-step change and of its magnitude at lag k (volatility clustering), and
 * behind the variance and kurtosis of the change over a SPAN of k steps (aggregational Gaussianity, the variance ratio) -
 * the multi-lag sibling of bk_series_*, folded on the env's stream from the same history ring with no host wait
 * (bourse_amd/csrc/lags.hpp, lag_fold.hpp).  It serves every flow that writes the ring - bk_run on all
 * pipelines, bk_step, the device ingress, markets - and touches no stepping kernel.  Neither table needs the other.  The
 * reference has no counterpart for any of these entries.
 *
 * What one record adds.  Of the record of step s and book b only bid_price and ask_price are read (words 1 and 2); an empty
 * side reads bid_price == 0 / ask_price == 0xFFFFFFFF.
 *   two_s = bid != 0 && ask != 0xFFFFFFFF;  m_s = bid + ask (TWICE the mid, a u64);
 *   a step in front of the table's START - the enable, a clear of that book, or a cut by a reset - is not two-sided;
 *   r_s = two_s && two_{s-1};  d_s = m_s - m_{s-1} (signed, |d| < 2^33).
 * Step s adds to row k - 1, for every k in 1 .. K:
 *   SPAN k, if two_s && two_{s-k}, with h = m_s - m_{s-k} and a = |h| (only the two end points must be two-sided):
 *                      n_h += 1, sum_h += h, sum_abs_h += a, sum_h2 += a * a, sum_h4 += a^4 (a 128-bit pair, the power
 *                      exact modulo 2^128), max_abs_h = max(max_abs_h, a);
 *   LAG k, if r_s && r_{s-k}:
 *                      n_pairs += 1, sum_dd += d_s * d_{s-k} (signed), sum_abs_dd += |d_s| * |d_{s-k}|.
 * All 64-bit words are sums modulo 2^64, sum_h4 a sum modulo 2^128; signed words are two's complement; a cleared row is all
 * zeros.  Row 0 is by construction bk_series_row's n_pairs, sum_dd, sum_abs_dd, n_ret, sum_d, sum_abs_d, sum_d2, sum_d4 and
 * max_abs_d over the same steps and cuts.
 *
 * The carry.  d_{s-k} needs m_{s-k-1}: a fold must know the K + 1 records in front of its first step, which the ring may no
 * longer hold.  The env keeps lag_carry[n_books][K + 1] u64, an array of its own beside the table: entry j is the record of
 * step lags_seen - 1 - j - bit 63 = two, the low bits = m - and the whole word is 0 when that step is one-sided or lies in
 * front of the start.  So folding steps [x, y) and then [y, z) leaves the same rows and carry as one fold over [x, z), for
 * every split. */
typedef struct bk_lag_row { /* 80 B, five 16-byte vectors, little-endian */
  uint64_t n_pairs;
  int64_t sum_dd;
  uint64_t sum_abs_dd;
  uint64_t n_h;
  int64_t sum_h;
  uint64_t sum_abs_h, sum_h2, sum_h4_lo, sum_h4_hi, max_abs_h;
} bk_lag_row;
/* Enabling.  Accepted on any env with history_capacity > 0, at any time, once; n_lags in 1 .. 64.  Allocates the rows and
 * the carry (arrays of their own: the state block, checkpoints and snapshots are unchanged), clears both and sets the env's
 * step cursor lags_seen, a host integer as bk_steps_done is and independent of the series' cursor, to bk_steps_done: earlier
 * steps are not counted.  A refusal - here and in the entries below: a null env, history_capacity == 0, n_lags outside
 * 1 .. 64, a second call, any other entry before this one - returns BK_INVALID_ARGUMENT, leaves the env unchanged and puts
 * the reason in bk_last_error().
 *
 * bk_reset_books* and bk_ingress_reset_books* on such an env first fold what is outstanding (and refuse the reset if steps
 * were lost, see bk_lags_fold; with bk_series_enable on the same env both tables are checked before either folds), then
 * zero only the CARRY of the books they reset (every book of a masked market): the sums go on across episodes and no span
 * or pair reaches over a reset; clear by mask if new rows are wanted.  bk_checkpoint_load clears every row and carry and
 * sets the cursor to the restored step count.  bk_load_book is refused.  bk_warm writes no history and restores the counter:
 * unaffected.  An env without the table launches nothing new.  (No counterpart in the reference.) */
int bk_lags_enable(bk_env* env, uint32_t n_lags);
/* Queues, on the env's stream and without any host wait, the fold of steps [lags_seen, bk_steps_done) of every book; then
 * lags_seen = bk_steps_done.  No new step: no launch.  If a step of that range is no longer retained by the ring - it
 * wrapped (more than history_capacity steps since the last fold), or bk_clear_history was called - returns
 * BK_INVALID_ARGUMENT with the number of lost steps in bk_last_error() and leaves rows, carry and cursor unchanged: a lost
 * step is never silent and needs no flag bit.  bk_lags_clear with a NULL mask is the way on.  (No counterpart in the
 * reference.) */
int bk_lags_fold(bk_env* env);
/* Clearing.  mask [n_books] bytes, one per BOOK.  With a mask: folds what is outstanding first (refusing as bk_lags_fold
 * does), then clears the rows and the carry of the books b with mask[b] != 0.  NULL: clears every row and carry and sets the
 * cursor to bk_steps_done WITHOUT folding.  From a HOST mask: staged on the env's stream and waited for, the clear itself
 * stays asynchronous.  (No counterpart in the reference.) */
int bk_lags_clear(bk_env* env, const uint8_t* mask_host);
/* The same from DEVICE memory written on the env's stream (NULL = every book).  HOLDS NO HOST SYNCHRONISATION: at most
 * two launches on the env's stream.  (No counterpart in the reference.) */
int bk_lags_clear_device(bk_env* env, const uint8_t* mask_dev);
/* Device pointer of the table, bk_lag_row[n_books][n_lags], for on-device consumers; valid for the env's life, written on
 * the env's stream.  (No counterpart in the reference.) */
int bk_lags_device_ptr(bk_env* env, void** out);
/* Rows of books [first_book, first_book + n_books) to host memory, n_books * n_lags rows.  Waits for the env's stream; does
 * NOT fold.  (No counterpart in the reference.) */
int bk_get_lags(bk_env* env, uint32_t first_book, uint32_t n_books, bk_lag_row* out);

/* ------------------------------------------------------ per-book bin table of the level-2 history */
/* An opt-in table bins[n_books][C][B] of u64 counts in DEVICE memory: per book the DISTRIBUTION of the mid's change over S
 * spans of k_j steps, of the spread and of the traded volume per step - the tails, quantiles and the share of steps without
 * a trade that the moments of bk_series_* and bk_lags_* do not give.  It is their third sibling, folded on the env's stream
 * from the same history ring with no host wait (bourse_amd/csrc/bins.hpp, bin_fold.hpp).  It serves every
 * flow that writes the ring - bk_run on all pipelines, bk_step, the device ingress, markets - and touches no stepping
 * kernel.  None of the three tables needs another.  The reference has no counterpart for any of these entries.
 *
 * The configuration.  B = n_bins is even and in 2 .. 256; S = n_spans is in 1 .. 4; each used span k_j = spans[j], j < S, is
 * in 1 .. 64, in any order, duplicates allowed (spans[j] for j >= S is ignored and read back as 0); every width is >= 1.
 * C = S + 2 channels per book: channel j < S is the return over k_j steps, channel S the spread, channel S + 1 the traded
 * volume.
 *
 * What one record adds.  Of the record of step s and book b only trade_vol, bid_price and ask_price are read (words 0 .. 2);
 * an empty side reads bid_price == 0 / ask_price == 0xFFFFFFFF.
 *   two_s = bid != 0 && ask != 0xFFFFFFFF;  m_s = bid + ask (TWICE the mid, a u64), as for bk_lags_*;
 *   a step in front of the table's START - the enable, a clear of that book, or a cut by a reset - is not two-sided.
 * Step s adds 1 to one bin of
 *   channel j < S, if two_s && two_{s-k_j} (a one-sided step in between does not matter): with h = m_s - m_{s-k_j} (signed,
 *                  |h| < 2^33) and q = floor(h / ret_width) - a true floor, -ceil(|h| / ret_width) below zero - the bin
 *                  clamp(q + B / 2, 0, B - 1).  Bin i covers [(i - B/2) w, (i - B/2 + 1) w) in units of HALF a price step; the
 *                  two end bins also hold everything beyond them ("at or below", "at or above");
 *   channel S,     if two_s: the bin min((ask - bid) / spread_width, B - 1), the difference a wrapping u32 as
 *                  bk_series_row's sum_spread has it;
 *   channel S + 1, always: the bin min(trade_vol / vol_width, B - 1).
 * Counts are sums modulo 2^64; a cleared table is all zeros.  By construction the total of channel j is bk_lag_row's n_h at
 * span k_j, the total of channel S is bk_series_row's n_two_sided and the total of channel S + 1 its n_steps over the same
 * steps and cuts; with ret_width == 1 and no value clamped, sum_i (i - B/2) * count_i is the lag row's sum_h.
 *
 * The carry.  A fold must know the Kmax = max k_j records in front of its first step, which the ring may no longer hold.  The
 * env keeps bins_carry[n_books][Kmax] u64, an array of its own beside the table: entry i is the record of step
 * bins_seen - 1 - i - bit 63 = two, the low bits = m - and the whole word is 0 when that step is one-sided or lies in front
 * of the start.  So folding steps [x, y) and then [y, z) leaves the same table and carry as one fold over [x, z), for every
 * split. */
typedef struct bk_bins_config { /* 36 B, nine u32 */
  uint32_t n_bins;
  uint32_t n_spans;
  uint32_t spans[4];
  uint32_t ret_width, spread_width, vol_width;
} bk_bins_config;
/* Enabling.  Accepted on any env with history_capacity > 0, at any time, once.  Allocates the table and the carry (arrays of
 * their own: the state block, checkpoints and snapshots are unchanged), clears both and sets the env's step cursor
 * bins_seen, a host integer as bk_steps_done is and independent of the siblings' cursors, to bk_steps_done: earlier steps
 * are not counted.  A refusal - here and in the entries below: a null env or config, history_capacity == 0, a configuration
 * outside the bounds above, a second call, any other entry before this one - returns BK_INVALID_ARGUMENT, leaves the env
 * unchanged and puts the reason in bk_last_error().
 *
 * bk_reset_books* and bk_ingress_reset_books* on such an env first fold what is outstanding (and refuse the reset if steps
 * were lost, see bk_bins_fold; with bk_series_enable or bk_lags_enable on the same env every table is checked before any
 * folds), then zero only the CARRY of the books they reset (every book of a masked market): the counts go on across episodes
 * and no span reaches over a reset; clear by mask if a new table is wanted.  bk_checkpoint_load clears every count and carry
 * and sets the cursor to the restored step count.  bk_load_book is refused.  bk_warm writes no history and restores the
 * counter: unaffected.  An env without the table launches nothing new.  (No counterpart in the reference.) */
int bk_bins_enable(bk_env* env, const bk_bins_config* cfg);
/* The configuration the table was enabled with (spans beyond n_spans read 0).  (No counterpart in the reference.) */
int bk_bins_config_get(bk_env* env, bk_bins_config* out);
/* Queues, on the env's stream and without any host wait, the fold of steps [bins_seen, bk_steps_done) of every book; then
 * bins_seen = bk_steps_done.  No new step: no launch.  If a step of that range is no longer retained by the ring - it
 * wrapped (more than history_capacity steps since the last fold), or bk_clear_history was called - returns
 * BK_INVALID_ARGUMENT with the number of lost steps in bk_last_error() and leaves table, carry and cursor unchanged: a lost
 * step is never silent and needs no flag bit.  bk_bins_clear with a NULL mask is the way on.  (No counterpart in the
 * reference.) */
int bk_bins_fold(bk_env* env);
/* Clearing.  mask [n_books] bytes, one per BOOK.  With a mask: folds what is outstanding first (refusing as bk_bins_fold
 * does), then clears the counts and the carry of the books b with mask[b] != 0.  NULL: clears every count and carry and sets
 * the cursor to bk_steps_done WITHOUT folding.  From a HOST mask: staged on the env's stream and waited for, the clear itself
 * stays asynchronous.  (No counterpart in the reference.) */
int bk_bins_clear(bk_env* env, const uint8_t* mask_host);
/* The same from DEVICE memory written on the env's stream (NULL = every book).  HOLDS NO HOST SYNCHRONISATION: at most
 * two launches on the env's stream.  (No counterpart in the reference.) */
int bk_bins_clear_device(bk_env* env, const uint8_t* mask_dev);
/* Device pointer of the table, uint64_t[n_books][n_spans + 2][n_bins], for on-device consumers; valid for the env's life,
 * written on the env's stream.  (No counterpart in the reference.) */
int bk_bins_device_ptr(bk_env* env, void** out);
/* Counts of books [first_book, first_book + n_books) to host memory, n_books * (n_spans + 2) * n_bins words.  Waits for the
 * env's stream; does NOT fold.  (No counterpart in the reference.) */
int bk_get_bins(bk_env* env, uint32_t first_book, uint32_t n_books, uint64_t* out);

/* ------------------------------------------------------ per-market cross table of the level-2 history */
/* An opt-in table cross[n_markets][S][A][A] in DEVICE memory on an env of markets (A = assets >= 2 books a market,
 * n_markets = n_books / A, book = market * A + asset): per market, span h_j = spans[j] and ORDERED pair of assets (a, b) the
 * sums behind the covariance and correlation of the two assets' changes of the mid over h_j steps - how the correlation
 * grows with the span (the Epps effect) - and behind the product of a's change with b's PREVIOUS one (which asset leads).
 * It is the fourth table folded on the env's stream from the history ring with no host wait (bourse_amd/csrc/cross.hpp,
 * cross_fold.hpp), the only one whose unit is the market and not the book, and needs none of the others.
 * It serves every flow that writes the ring of such an env - bk_run on all pipelines, bk_step, the device ingress - and
 * touches no stepping kernel.  The reference has no counterpart for any of these entries.
 *
 * The configuration.  S = n_spans is in 1 .. 4; each used span h_j = spans[j], j < S, is in 1 .. 64, in any order,
 * duplicates allowed (spans[j] for j >= S is ignored and read back as 0).  Hmax is the longest used span.
 *
 * What one step adds.  Of the record of step s and book market * A + x only bid_price and ask_price are read (words 1 and
 * 2); an empty side reads bid_price == 0 / ask_price == 0xFFFFFFFF.
 *   two_x(s) = bid != 0 && ask != 0xFFFFFFFF;  m_x(s) = bid + ask (TWICE the mid, a u64), as for bk_lags_*;
 *   a step in front of the table's START - the enable, a clear of that market, or a cut by a reset - is not two-sided.
 * Step s adds to row (market, j, a, b), for every j < S and every a, b < A, with h = h_j:
 *   CONTEMPORANEOUS, if two_a(s) && two_a(s-h) && two_b(s) && two_b(s-h), with x = m_a(s) - m_a(s-h) and
 *                    y = m_b(s) - m_b(s-h) (signed, |x|, |y| < 2^33):
 *                      n += 1, sum_x += x, sum_y += y, sum_xx += x * x, sum_yy += y * y, sum_xy += x * y;
 *   LEAD, b's previous window against a's current one, if two_a(s) && two_a(s-h) && two_b(s-h) && two_b(s-2h) (m_b(s) is
 *                    NOT required), with z = m_b(s-h) - m_b(s-2h):
 *                      n_lead += 1, sum_lead += x * z.
 * All words are sums modulo 2^64; signed words are two's complement, and the products are the 64-bit products of the
 * two's-complement values; a cleared row is all zeros.  The definition is pairwise complete: the books are one-sided at
 * different steps, so n of (a, b) is usually below n of (a, a) and of (b, b).  By construction row (., j, a, a) holds in n
 * the n_h, in sum_x and sum_y the sum_h and in sum_xx, sum_yy and sum_xy the sum_h2 of row h_j - 1 of book market * A + a's
 * lag table (bk_lags_*) over the same steps and cuts, at h_j == 1 also its n_pairs in n_lead and its sum_dd in sum_lead; rows
 * (a, b) and (b, a) share n and sum_xy and swap sum_x / sum_y and sum_xx / sum_yy.
 *
 * The carry.  A fold must know the 2 * Hmax records of every asset in front of its first step, which the ring may no longer
 * hold.  The env keeps cross_carry[n_markets][A][2 * Hmax] u64, an array of its own beside the table: entry i of an asset is
 * the record of step cross_seen - 2 * Hmax + i - bit 63 = two, the low bits = m - and the whole word is 0 when that step is
 * one-sided or lies in front of the start.  So folding steps [x, y) and then [y, z) leaves the same rows and carry as one
 * fold over [x, z), for every split - single steps and a ring shorter than 2 * Hmax included. */
typedef struct bk_cross_config { /* 20 B, five u32 */
  uint32_t n_spans;
  uint32_t spans[4];
} bk_cross_config;
typedef struct bk_cross_row { /* 64 B, four 16-byte vectors, little-endian */
  uint64_t n;
  int64_t sum_x, sum_y;
  uint64_t sum_xx, sum_yy;
  int64_t sum_xy;
  uint64_t n_lead;
  int64_t sum_lead;
} bk_cross_row;
/* Enabling.  Accepted on an env of markets (assets >= 2) with history_capacity > 0, at any time, once.  Allocates the rows
 * and the carry (arrays of their own: the state block, checkpoints and snapshots are unchanged), clears both and sets the
 * env's step cursor cross_seen, a host integer as bk_steps_done is and independent of the siblings' cursors, to
 * bk_steps_done: earlier steps are not counted.  A refusal - here and in the entries below: a null env or config,
 * history_capacity == 0, an env of independent books (assets == 1), a configuration outside the bounds above, a second call,
 * any other entry before this one - returns BK_INVALID_ARGUMENT, leaves the env unchanged and puts the reason in
 * bk_last_error().
 *
 * bk_reset_books* and bk_ingress_reset_books* on such an env first fold what is outstanding (and refuse the reset if steps
 * were lost, see bk_cross_fold; every table of the history ring on the same env is checked before any folds), then zero only
 * the CARRY of every asset of the markets they reset: the sums go on across episodes and no span or lead reaches over a
 * reset; clear by mask if new rows are wanted.  bk_checkpoint_load clears every row and carry and sets the cursor to the
 * restored step count.  bk_load_book is refused.  bk_warm writes no history and restores the counter: unaffected.  An env
 * without the table launches nothing new.  (No counterpart in the reference.) */
int bk_cross_enable(bk_env* env, const bk_cross_config* cfg);
/* The configuration the table was enabled with (spans beyond n_spans read 0).  (No counterpart in the reference.) */
int bk_cross_config_get(bk_env* env, bk_cross_config* out);
/* Queues, on the env's stream and without any host wait, the fold of steps [cross_seen, bk_steps_done) of every market; then
 * cross_seen = bk_steps_done.  No new step: no launch.  If a step of that range is no longer retained by the ring - it
 * wrapped (more than history_capacity steps since the last fold), or bk_clear_history was called - returns
 * BK_INVALID_ARGUMENT with the number of lost steps in bk_last_error() and leaves rows, carry and cursor unchanged: a lost
 * step is never silent and needs no flag bit.  bk_cross_clear with a NULL mask is the way on.  (No counterpart in the
 * reference.) */
int bk_cross_fold(bk_env* env);
/* Clearing.  mask [n_markets] bytes, one per MARKET (as the resets' masks).  With a mask: folds what is outstanding first
 * (refusing as bk_cross_fold does), then clears the rows and the carry of the markets m with mask[m] != 0.  NULL: clears
 * every row and carry and sets the cursor to bk_steps_done WITHOUT folding.  From a HOST mask: staged on the env's stream and
 * waited for, the clear itself stays asynchronous.  (No counterpart in the reference.) */
int bk_cross_clear(bk_env* env, const uint8_t* mask_host);
/* The same from DEVICE memory written on the env's stream (NULL = every market).  HOLDS NO HOST SYNCHRONISATION: at most
 * two launches on the env's stream.  (No counterpart in the reference.) */
int bk_cross_clear_device(bk_env* env, const uint8_t* mask_dev);
/* Device pointer of the table, bk_cross_row[n_markets][n_spans][assets][assets], for on-device consumers; valid for the env's
 * life, written on the env's stream.  (No counterpart in the reference.) */
int bk_cross_device_ptr(bk_env* env, void** out);
/* Rows of markets [first_market, first_market + n_markets) to host memory, n_markets * n_spans * assets * assets rows.
 * Waits for the env's stream; does NOT fold.  (No counterpart in the reference.) */
int bk_get_cross(bk_env* env, uint32_t first_market, uint32_t n_markets, bk_cross_row* out);

/* ------------------------------------------------------ per-book flow table of the trade records */
/* An opt-in table flow[n_books][8 + 6 K] of u64 words in DEVICE memory, K = n_lags, 1 <= K <= 64: per book the sums over its
 * TRADE RECORDS in record order - the buy share and the size moments, and at lags k = 1 .. K in TRADE time the sums behind
 * the autocorrelation of the trade sign, the response function <s_i (p_{i+k} - p_i)> and the variogram of the price.  It is
 * folded on the env's stream by one small kernel with no host wait (bourse_amd/csrc/flow.hpp, flow_fold.hpp; DESIGN.md
 * 2.26) and serves every env that writes trade records: bk_run on all pipelines, bk_step, the device ingress, markets,
 * Noise / Momentum members.  It is not one of the tables of the history ring: its cursor is per book and lives in device
 * memory, as the trade bars' and the accounts' do.  The reference has no counterpart for any of these entries.
 *
 * Record i of a book - i counts as bk_trade_count's total does - has the price p_i, the volume v_i and the sign s_i = +1 if
 * the aggressor bought (side_is_bid == 0, the PASSIVE order's side, as for bk_trade_bar) and -1 otherwise.  A record that was
 * read adds to the base words
 *   n_trades += 1, n_buy += [s_i > 0], sum_vol += v_i, buy_vol += [s_i > 0] v_i, sum_vol_sq += v_i^2,
 *   notional += v_i p_i (the full 32 x 32 product), max_vol = max(max_vol, v_i)
 * and, for every k in 1 .. K of which record i - k was read as well - whatever lies between them -, with
 * dp = p_i - p_{i-k} (signed), to lag row k - 1, the words 8 + 6 (k - 1) .. :
 *   n_pairs += 1, sum_ss += s_i s_{i-k}, sum_resp += s_{i-k} dp, sum_back += s_i dp, sum_abs_dp += |dp|, sum_dp2 += dp^2.
 * All words are sums modulo 2^64; signed words are two's complement; a cleared table is all zeros.
 *
 * Lost records.  A fold covers the indices [flow_seen, total).  Index i can be read iff first_retained <= i < total and
 * i - first_retained < trade_capacity (bk_trade_count's words as the fold reads them): a record dropped beyond
 * trade_capacity, or consumed by bk_clear_trades / bk_drain_trades / a consuming fold before this table saw it, cannot.  Such
 * an index adds 1 to n_lost, stands in the window as an invalid word and forms no pair; a pair whose two ends were read
 * still counts at its true lag.  A lost record is never silent and needs no flag bit (a dropped record's book carries
 * BK_FLAG_TRADE_OVERFLOW already).
 *
 * The carry.  The env keeps flow_carry[n_books][K] u64 beside the table: entry j is the record of index flow_seen - 1 - j -
 * bit 63 = it was read, bit 62 = s > 0, the low 32 bits = p - and the whole word is 0 when it was not read or lies in front
 * of the table's start.  So folding [x, y) and then [y, z) leaves the same words and carry as one fold over [x, z), for every
 * split. */
enum { /* the words of one book (one `NAME = N` per line: tools/gen_rust_sys.py reads them) */
  BK_FLOW_N_TRADES = 0,
  BK_FLOW_N_BUY = 1,
  BK_FLOW_SUM_VOL = 2,
  BK_FLOW_BUY_VOL = 3,
  BK_FLOW_SUM_VOL_SQ = 4,
  BK_FLOW_NOTIONAL = 5,
  BK_FLOW_MAX_VOL = 6,
  BK_FLOW_N_LOST = 7,
  BK_FLOW_BASE_WORDS = 8,
  /* of lag row k - 1, from word BK_FLOW_BASE_WORDS + BK_FLOW_LAG_WORDS * (k - 1) */
  BK_FLOW_N_PAIRS = 0,
  BK_FLOW_SUM_SS = 1,
  BK_FLOW_SUM_RESP = 2,
  BK_FLOW_SUM_BACK = 3,
  BK_FLOW_SUM_ABS_DP = 4,
  BK_FLOW_SUM_DP2 = 5,
  BK_FLOW_LAG_WORDS = 6
};
/* Enabling.  Accepted on any env with trade_capacity > 0, at any time, once; n_lags in 1 .. 64.  Allocates the table, the
 * carry and the cursors (arrays of their own: the state block, checkpoints and snapshots are unchanged), clears them and
 * sets every book's cursor to its current trade count: earlier records are not counted.  consume_trades != 0: a fold ends by
 * marking the records consumed, as bk_clear_trades does, so trade_capacity only has to hold what is written between two
 * folds.  A refusal - here and in the entries below: a null env, trade_capacity == 0, n_lags outside 1 .. 64, a second call,
 * any other entry before this one - returns BK_INVALID_ARGUMENT, leaves the env unchanged and puts the reason in
 * bk_last_error().
 *
 * bk_step_async on such an env folds the step's records right behind the event kernel, in front of the trade bars' and the
 * accounts' folds; the LAST fold of the step consumes, once, if any of the three asked.  bk_reset_books* and
 * bk_ingress_reset_books* first fold what is outstanding, then cut the books they reset (every book of a masked market):
 * the carry is invalidated and the cursor follows the restored trade count, so no pair reaches over a reset and the sums go
 * on across episodes; clear by mask if new rows are wanted.  bk_checkpoint_load clears every word and carry and sets the
 * cursors to the restored counts.  bk_load_book is refused.  bk_warm writes no trade record and restores the counts:
 * unaffected.  An env without the table launches nothing new.  (No counterpart in the reference.) */
int bk_flow_enable(bk_env* env, uint32_t n_lags, int consume_trades);
/* Queues, on the env's stream and without any host wait, ONE launch that folds every book's records [flow_seen, total);
 * consumes iff the enable asked.  (No counterpart in the reference.) */
int bk_flow_fold(bk_env* env);
/* Clearing.  mask [n_books] bytes, one per BOOK.  With a mask: folds first, then zeroes the words, invalidates the carry and
 * sets the cursor to the trade count of the books b with mask[b] != 0.  NULL: the same for every book WITHOUT folding.  From a
 * HOST mask: staged on the env's stream and waited for, the clear itself stays asynchronous.  (No counterpart in the
 * reference.) */
int bk_flow_clear(bk_env* env, const uint8_t* mask_host);
/* The same from DEVICE memory written on the env's stream (NULL = every book).  HOLDS NO HOST SYNCHRONISATION: at most
 * two launches on the env's stream.  (No counterpart in the reference.) */
int bk_flow_clear_device(bk_env* env, const uint8_t* mask_dev);
/* Device pointer of the table, uint64_t[n_books][8 + 6 n_lags], for on-device consumers; valid for the env's life, written
 * on the env's stream.  (No counterpart in the reference.) */
int bk_flow_device_ptr(bk_env* env, void** out);
/* The table's n_lags.  (No counterpart in the reference.) */
int bk_flow_lags(bk_env* env, uint32_t* out);
/* Words of books [first_book, first_book + n_books) to host memory, n_books * (8 + 6 n_lags) words.  Waits for the env's
 * stream; does NOT fold.  (No counterpart in the reference.) */
int bk_get_flow(bk_env* env, uint32_t first_book, uint32_t n_books, uint64_t* out);
/* For tests and debugging: the carry [n_books][n_lags] (may be NULL) and the cursors [n_books] of the same books.  Waits for
 * the env's stream; does NOT fold.  (No counterpart in the reference.) */
int bk_get_flow_state(bk_env* env, uint32_t first_book, uint32_t n_books, uint64_t* carry, uint64_t* seen);

/* ------------------------------------------------------ open orders of a device-ingress env */
/* An opt-in pair of tables in DEVICE memory: which orders of each trader rest in each book, at what price and with how much
 * volume left - the one thing a strategy that submits from device memory could not read there (the ids to cancel or
 * modify, the resting volume per side for an exposure limit, its own best bid and ask).  The tables are RECOMPUTED from
 * each book's pool and the order records' trader ids on the env's stream (bourse_amd/csrc/open_orders.hpp):
 * they hold no state of their own - no cursor, nothing in a snapshot - and cannot drift from the book.  The reference has
 * no counterpart for any of these entries.
 *
 * summary[n_books][n_traders], and entries[n_books][n_traders][depth].  "Resting" means live in the pool as the last
 * refresh found it: exactly the set bk_live_orders returns, with the remaining volume and the current price (partial fills
 * and modifications show).  A trader's entries are its resting orders of either side in ascending order id (creation
 * order; ids are u32 on the device); the first min(n_bid + n_ask, depth) are used and every slot behind them holds the
 * empty entry {0xFFFFFFFF, 0, 0, 0}.  A trader that rests more than depth orders has its oldest depth listed and an exact
 * summary: n_bid + n_ask > depth says so.  A trader id >= n_traders is skipped without a flag: give background members
 * (bk_set_agents*, bk_set_random_agents*) an agent_id_start above n_traders to keep them out.  A resting order whose id is
 * >= max_orders has no record to look its trader up in and is left out of the rows; BK_FLAG_ORDER_LOG_FULL is set on that
 * book already.  Rows are per book, so markets need nothing special (market * assets + asset). */
typedef struct bk_open_summary { /* 32 B */
  uint64_t bid_vol, ask_vol;   /* sum of the remaining volume of the trader's resting bids / asks */
  uint32_t n_bid, n_ask;       /* how many rest, ALL of them (not capped by depth) */
  uint32_t best_bid, best_ask; /* highest own bid price (0 if none), lowest own ask price (0xFFFFFFFF if none) */
} bk_open_summary;
typedef struct bk_open_order { /* 16 B */
  uint32_t order_id, price, vol, side_is_bid;
} bk_open_order;
/* Enabling.  Accepted on an env with the device ingress (bk_device_ingress_enable) and max_orders > 0, at any time - also
 * mid-run and while an ingress snapshot slot is held: the tables are a function of the current pools.  depth == 0 keeps
 * the summary rows only (no entry array, no ranking work).  Refuses n_traders == 0, n_traders > 65536, depth > 64 and a
 * second call.  A refusal - here and in the three entries below - returns BK_INVALID_ARGUMENT, is made before anything is
 * allocated or enqueued, leaves the env unchanged and puts the reason in bk_last_error().
 *
 * When the tables are refreshed: at this call (every book); behind every bk_step_async / bk_step, after the event kernel
 * (and after the accounts' fold when both are on); behind bk_ingress_reset_books*, for the reset units only, after the
 * reset's own kernels with the same device mask - a reset book shows the snapshot's resting orders before its next step;
 * and at bk_open_orders_refresh.  Each is one launch on the env's stream: no allocation, no stream wait, no host read.
 * The tables describe the books as of the last refresh: instructions submitted or queued since are not in them.
 * Behaviour of an env without the view does not change.  (No counterpart in the reference.) */
int bk_open_orders_enable(bk_env* env, uint32_t n_traders, uint32_t depth);
/* Refresh the rows of every book now, for callers that changed a pool outside a step.
 * (No counterpart in the reference.) */
int bk_open_orders_refresh(bk_env* env);
/* Device pointers of the two tables, bk_open_summary[n_books][n_traders] and bk_open_order[n_books][n_traders][depth]
 * (*entries = NULL when depth == 0), for on-device consumers; valid for the env's life, written on the env's stream.
 * (No counterpart in the reference.) */
int bk_open_orders_device_ptrs(bk_env* env, void** summary, void** entries);
/* Rows of books [first_book, first_book + n_books) to host memory: n_books * n_traders summary rows and, when entries_out
 * (nullable) is not NULL and depth > 0, n_books * n_traders * depth entries.  Waits for the env's stream.
 * (No counterpart in the reference.) */
int bk_get_open_orders(bk_env* env, uint32_t first_book, uint32_t n_books, bk_open_summary* summary_out,
                       bk_open_order* entries_out);

/* ------------------------------------------------------ queue positions of the open orders */
/* An opt-in companion of the entries above, in DEVICE memory: queue[n_books][n_traders][depth], one row per entry, saying
 * where that resting order stands in its book's queue - how much volume must trade before it is touched, and how much of
 * that rests ahead of it at its own price.  Neither the level-2 ladder (volume per level, nothing inside a level) nor the
 * order ids (a modification that replaces an order keeps its id and takes a fresh place) give it.  The rows are RECOMPUTED
 * from each book's pool on the env's stream (bourse_amd/csrc/open_queue.hpp), right behind the open-order
 * rows wherever those are refreshed; like them they hold no state of their own - no cursor, nothing in a snapshot.  The
 * reference has no counterpart for any of these entries.
 *
 * For the listed order o of side S, price P and pool stamp q (the pool's `seq`, the time priority the matching engine
 * trades by and bk_live_orders sorts by), r ranges over the OTHER live orders of the book on side S: r is better when its
 * price is above P (bids) or below P (asks), level-earlier when its price is P and its stamp is below q.  Every live order
 * counts, whoever owns it: background members and agents, traders >= n_traders, the trader's own other orders, and orders
 * whose id is >= max_orders.  The row of an unused entry (order_id == 0xFFFFFFFF) is all zeros. */
typedef struct bk_open_queue { /* 32 B */
  uint64_t ahead_vol;          /* remaining volume that has priority over this order on its side */
  uint64_t level_ahead_vol;    /* the part of it that rests at this order's own price */
  uint64_t level_vol;          /* all remaining volume at this order's price and side, this order included */
  uint32_t ahead_orders;       /* how many resting orders ahead_vol counts */
  uint32_t level_ahead_orders; /* how many level_ahead_vol counts */
} bk_open_queue;
/* Enabling.  Accepted at any time after bk_open_orders_enable - also mid-run and while an ingress snapshot slot is held.
 * Refuses an env without the open-order view (call bk_open_orders_enable first), one whose view has depth == 0 and a
 * second call.  A refusal - here and in the two entries below - returns BK_INVALID_ARGUMENT, is made before anything is
 * allocated or enqueued, leaves the env unchanged and puts the reason in bk_last_error().  Allocates the table and
 * refreshes both tables for every book, the open-order rows first.
 *
 * When the rows are refreshed: wherever the open-order rows are (bk_open_orders_enable's list), by one more launch on the
 * env's stream right behind that refresh and with the same mask: no allocation, no stream wait, no host read.  Behaviour
 * of an env without the view does not change.  (No counterpart in the reference.) */
int bk_open_queue_enable(bk_env* env);
/* Device pointer of the table, bk_open_queue[n_books][n_traders][depth], for on-device consumers; valid for the env's
 * life, written on the env's stream.  BK_INVALID_ARGUMENT without the queue view.  (No counterpart in the reference.) */
int bk_open_queue_device_ptr(bk_env* env, void** out);
/* Rows of books [first_book, first_book + n_books) to host memory, n_books * n_traders * depth records.  Waits for the
 * env's stream.  (No counterpart in the reference.) */
int bk_get_open_queue(bk_env* env, uint32_t first_book, uint32_t n_books, bk_open_queue* out);

/* ------------------------------------------------------ quotes: requote every trader from one dense table */
/* The action side of an on-device strategy loop: quotes[n_books][n_traders], one row per trader with a row in the
 * open-order view (n_traders and depth are bk_open_orders_enable's; on a market the rows are per book, market * assets +
 * asset), saying "this trader wants this bid and this ask".  The call joins the table with the view's entries on the
 * device (bourse_amd/csrc/quotes_ingress.hpp) and queues the cancellations, in-place reductions and new
 * orders that lead there.  The reference has no counterpart for any of these entries.
 *
 * Per side S of trader t in book b, against the trader's LISTED entries - entries[b][t][0 .. depth-1] in ascending order
 * id, exactly as the last refresh left them:
 *   vol == BK_QUOTE_KEEP   nothing for this side.
 *   vol == 0               every listed order of side S is cancelled.
 *   otherwise (P, V)       the KEEPER is the first listed order of side S whose price equals P; every other listed order of
 *                          side S is cancelled.  With a keeper of remaining volume v: v == V nothing; v > V a volume-only
 *                          modification to V (applied in place, priority kept); v < V a new limit order (P, V - v) - the
 *                          keeper keeps its place and the top-up queues behind it.  Without a keeper: a new limit order
 *                          (P, V).  New orders carry trader id t.
 *
 * The call is DEFINED as a dense instruction batch.  Book b's batch is the grid n_traders x G, G = depth + 2,
 * trader-major: positions 0 .. depth-1 of a trader are its entry slots (action 2 with the entry's id, BK_ACTION_MODIFY with
 * side bit 2, the new volume and the entry's id, or action 0), position depth is the new bid (action 1 or 0) and position
 * depth + 1 the new ask.  For the queue, the ids, the order records, the flags and status_dev the call equals
 * bk_submit_instructions_device given that grid with book_offsets[b] = b * n_traders * G: ids are dense in element order;
 * the first new order whose price the book's tick does not divide stops that book's batch with
 * BK_PRICE_NOT_TICK_MULTIPLE, earlier elements stay queued and other books are unaffected; a full queue or an exhausted
 * id space gives BK_CAPACITY; status_dev (nullable, [2 * n_books]) = {code, grid positions applied}; the events are
 * appended behind whatever was queued earlier in the step, in call order, beside bk_submit_instructions_device,
 * bk_update_agents, bk_update_members and the market updates.  out_ids_dev (nullable, [n_books][n_traders][2] u64) holds
 * the id of the new bid and the new ask the call created, UINT64_MAX otherwise; it is untouched from a book's failing
 * element on.
 *
 * What is the caller's affair:
 *   - The table describes the books as of the last refresh.  Orders submitted since, the trader's orders beyond `depth` and
 *     a second call in one step are not seen: the entries are read as they lie.
 *   - A volume-only modification whose order has meanwhile traded below V is the reference's replace_order.
 *   - Prices are absolute.  Prices relative to the touch are out of scope: the level-2 data's device pointer and one
 *     tensor operation give them.  Market orders are out of scope.
 *   - Nothing is stateful: no snapshot content, nothing to clear. */
typedef struct bk_quote { uint32_t bid_price, bid_vol, ask_price, ask_vol; } bk_quote; /* 16 B */
#define BK_QUOTE_KEEP 0xFFFFFFFFu /* as a side's vol: leave that side's resting orders alone */
/* quotes_dev: DEVICE memory, 16-byte aligned, written on the env's stream.  Asynchronous on the env's stream.  Refuses,
 * with BK_INVALID_ARGUMENT, before anything is enqueued, the env unchanged and the reason in bk_last_error(): a null env
 * or null quotes, an env without the device ingress, one without the open-order view (call bk_open_orders_enable first)
 * and a view with depth == 0.  (No counterpart in the reference.) */
int bk_submit_quotes_device(bk_env* env, const bk_quote* quotes_dev, uint64_t* out_ids_dev, uint32_t* status_dev);
/* The same from a HOST table: copied into pinned staging before the call returns and from there, on the env's stream, into
 * a device staging buffer - both owned by the env and made at the first call; out_ids_dev and status_dev stay device
 * memory.  The host table may be reused on return; a call waits for the upload of the call before it, never for a kernel
 * behind that.  Same refusals.  (No counterpart in the reference.) */
int bk_submit_quotes(bk_env* env, const bk_quote* quotes, uint64_t* out_ids_dev, uint32_t* status_dev);

#ifdef __cplusplus
}
#endif
#endif /* BOURSE_AMD_H */
