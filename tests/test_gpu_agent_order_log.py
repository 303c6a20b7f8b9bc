"""The order log of bk_run's RandomAgents (bk_set_agent_order_log / ManyBookEnv.enable_agent_order_log): after run, the
readers answer for every order the agents created - Env::get_orders / order_status / OrderBook::save_json after
sim_runner (crates/step_sim/src/env.rs:253-290) - bit for bit against the CPU oracle, and the simulation itself is the
one an env without the log runs."""
import numpy as np
import pytest

import oracle_parity as P

pytestmark = pytest.mark.gpu

SEED, STEP, LEVELS = 101, 100_000, 10
MODES = ("auto", "fused", "split", "wave_split", "wave")


def groups_for(pool):
    n = pool // 2
    return [(n, (32, 64), (10, 20), 2, 0.8), (n, (32, 64), (50, 70), 2, 0.2)]


@pytest.fixture(scope="module")
def bk():
    import bourse_amd

    return bourse_amd


def check_book(env, b, view, state=True):
    P.same_book(env, b, view, orders=True, keys=True, state=state)


_refs = {}


def ref_books(oracle, n_books, pool, n_steps=40):
    key = (n_books, pool, n_steps)
    if key not in _refs:
        ref = oracle.ManyBooks(n_books, SEED, 0, 2, STEP, True, LEVELS, groups_for(pool))
        ref.run(n_steps, n_threads=8)
        _refs.clear()
        _refs[key] = ref
    return _refs[key]


def make_env(bk, n_books, pool, max_orders, log=True, strict=True, steps=40):
    env = bk.ManyBookEnv(n_books, SEED, 0, 2, STEP, True, levels=LEVELS, max_live_orders=pool, max_orders=max_orders,
                         trade_capacity=2 * pool * steps, history_capacity=steps, strict=strict)
    env.set_random_agents(groups_for(pool))
    if log:
        env.enable_agent_order_log()
    return env


@pytest.mark.parametrize("pool", [64, 128, 256, 512])
@pytest.mark.parametrize("mode", MODES)
def test_agent_orders_match_the_oracle(bk, oracle, pool, mode):
    B = 512
    env = make_env(bk, B, pool, max_orders=pool * 40)
    env.set_pipeline(mode)
    assert env.pipeline()[0] in ("split", "wave_split"), env.pipeline()  # never a fused kernel with the log
    env.run(15)
    env.run(25)
    ref = ref_books(oracle, B, pool)
    P.no_flags(env)
    P.same_history(env.history(), ref.history())
    assert np.array_equal(env.order_counts(), ref.order_counts())
    # book_state builds one dict per order: every book on the smaller pools, a spread of books on the larger ones
    full = set(range(B)) if pool <= 128 or mode == "split" else set(range(0, B, 37)) | {B - 1}
    for b in range(B):
        check_book(env, b, ref.book(b), state=b in full)
    env.close()


def test_market_agent_orders_match_the_oracle(bk, oracle):
    NM, ticks, n_steps = 300, [1, 2], 40
    groups = [(0, 40, (30, 50), (10, 20), 2, 0.7), (1, 33, (20, 40), (5, 9), 4, 0.9), (0, 20, (30, 50), (50, 70), 2, 0.3)]
    n_agents = sum(g[1] for g in groups)
    env = bk.ManyMarketEnv(NM, SEED, 0, ticks, STEP, True, levels=LEVELS, max_live_orders=128, max_orders=n_agents * n_steps,
                           trade_capacity=2 * n_agents * n_steps, history_capacity=n_steps)
    env.set_random_market_agents(groups)
    env.enable_agent_order_log()
    env.run(15)
    env.run(25)
    ref = oracle.ManyMarkets(NM, SEED, 0, ticks, STEP, True, LEVELS, groups)
    ref.run(n_steps, n_threads=8)
    P.no_flags(env)
    P.same_history(env.history(), ref.history())
    for m in range(NM):
        for a in range(len(ticks)):
            check_book(env, env.book(m, a), ref.book(m, a), state=m % 7 == 0)
    env.close()


@pytest.mark.parametrize("pool,mode", [(64, "auto"), (128, "split"), (256, "wave_split"), (512, "auto")])
def test_logging_changes_nothing_else(bk, pool, mode):
    B = 1024
    outs = []
    for log in (False, True):
        env = make_env(bk, B, pool, max_orders=pool * 40, log=log)
        env.set_pipeline(mode)
        env.run(17)
        env.run(23)
        outs.append(P.snapshot(env))
        env.close()
    P.assert_same(outs[0], outs[1])


def test_markets_logging_changes_nothing_else(bk):
    groups = [(0, 40, (30, 50), (10, 20), 2, 0.7), (1, 60, (20, 40), (5, 9), 4, 0.9)]
    outs = []
    for log in (False, True):
        env = bk.ManyMarketEnv(256, 7, 0, [2, 4], STEP, True, levels=LEVELS, max_live_orders=128, max_orders=4000,
                               trade_capacity=8000, history_capacity=30)
        env.set_random_market_agents(groups)
        if log:
            env.enable_agent_order_log()
        env.run(30)
        outs.append(P.snapshot(env))
        env.close()
    P.assert_same(outs[0], outs[1])


def test_agent_orders_at_scale_on_the_lane_split(bk, oracle):
    B, pool, n_steps = 8192, 128, 20
    env = make_env(bk, B, pool, max_orders=pool * n_steps, steps=n_steps)
    env.set_pipeline("split")
    env.run(n_steps)
    assert env.pipeline()[0] == "split"
    ref = oracle.ManyBooks(B, SEED, 0, 2, STEP, True, LEVELS, groups_for(pool))
    ref.run(n_steps, n_threads=8)
    P.same_history(env.history(), ref.history())
    for b in range(B):
        check_book(env, b, ref.book(b), state=b % 97 == 0)
    env.close()


def test_log_capacity_is_flagged_and_refused(bk):
    B, pool, cap = 256, 128, 200
    plain = make_env(bk, B, pool, max_orders=cap, log=False, strict=False)
    plain.run(40)
    full = make_env(bk, B, pool, max_orders=cap, strict=False)
    full.run(40)
    counts = full.order_counts()
    assert (counts > cap).any()
    fl = full.flags()
    assert np.array_equal((fl & bk._lib.FLAG_ORDER_LOG_FULL) != 0, counts > cap)
    b = int(np.argmax(counts > cap))
    for read in (lambda: full.orders(b), lambda: full.order_keys(b), lambda: full.order_status(b, cap)):
        with pytest.raises(bk._lib.CapacityError):
            read()
    assert full.order_status(b, cap - 1) in (1, 2, 3)  # ids inside the log still answer
    for x in range(B):
        assert np.array_equal(full.trades(x, first=0), plain.trades(x, first=0)), x
    assert np.array_equal(full.history(), plain.history())
    # the strict check reports the overflow like every capacity flag
    strict = make_env(bk, B, pool, max_orders=cap)
    with pytest.raises(bk._lib.CapacityError):
        strict.run(40)
    for e in (plain, full, strict):
        e.close()


def refused(bk, call, match):
    """call() fails with BK_INVALID_ARGUMENT (not merely some error) and a message that names the reason."""
    with pytest.raises(bk._lib.BourseError, match=match) as e:
        call()
    assert e.value.code == bk._lib.BK_INVALID, e.value


def enable_rc(env, on=1):
    return env._L.bk_set_agent_order_log(env._h, on)  # the C ABI's status itself


def test_refusals(bk):
    BK_OK, BK_INVALID = bk._lib.BK_OK, bk._lib.BK_INVALID
    # no log capacity
    env = make_env(bk, 64, 64, max_orders=0, log=False)
    refused(bk, env.enable_agent_order_log, "max_orders")
    assert enable_rc(env) == BK_INVALID
    env.close()
    # after the first run
    env = make_env(bk, 64, 64, max_orders=1000, log=False)
    env.run(1)
    refused(bk, env.enable_agent_order_log, "first bk_run")
    assert enable_rc(env) == BK_INVALID
    env.close()
    # host-driven orders
    env = bk.ManyBookEnv(64, 1, 0, 2, STEP, max_orders=100)
    env.place_order(0, True, 10, 0, 100)
    refused(bk, env.enable_agent_order_log, "host-driven")
    env.close()
    # a device-ingress env logs already; and a logging env cannot take the device ingress
    env = bk.ManyBookEnv(64, 1, 0, 2, STEP, max_orders=100)
    env.enable_device_ingress(16)
    refused(bk, env.enable_agent_order_log, "device memory")
    assert enable_rc(env) == BK_INVALID
    env.close()
    env = bk.ManyBookEnv(64, 1, 0, 2, STEP, max_orders=100)
    env.enable_agent_order_log()
    refused(bk, lambda: env.enable_device_ingress(16), "ONE order flow")
    env.close()
    # Noise / Momentum members: either order
    noise = ("noise", 0, 20, dict(tick_size=2, p_limit=0.2, p_market=0.2, p_cancel=0.1, trade_vol=100, price_dist_mu=0.0,
                                  price_dist_sigma=1.0))
    env = bk.ManyBookEnv(64, 1, 0, 2, STEP, max_orders=100)
    env.set_agents([noise])
    refused(bk, env.enable_agent_order_log, "Noise")
    assert enable_rc(env) == BK_INVALID
    env.close()
    env = bk.ManyBookEnv(64, 1, 0, 2, STEP, max_orders=100)
    env.enable_agent_order_log()
    refused(bk, lambda: env.set_agents([noise]), "Noise")
    env.set_agents([("random", 20, (32, 64), (10, 20), 2, 0.5)])  # RandomAgents-only sets are logged
    env.close()
    # on = 0: nothing to do without the log, refused with it (the log cannot be switched off)
    env = make_env(bk, 64, 64, max_orders=1000, log=False)
    assert enable_rc(env, 0) == BK_OK
    assert enable_rc(env, 1) == BK_OK and enable_rc(env, 1) == BK_OK
    assert enable_rc(env, 0) == BK_INVALID
    env.close()
    # checkpoints: neither saved from nor restored into a logging env (a restored book's id counter would cover orders the
    # log never saw); nor a book loaded into one
    plain = make_env(bk, 64, 64, max_orders=1000, log=False)
    plain.run(3)
    buf = plain.checkpoint()
    env = make_env(bk, 64, 64, max_orders=1000)
    env.run(3)
    refused(bk, env.checkpoint, "checkpoint")
    fresh = make_env(bk, 64, 64, max_orders=1000)
    refused(bk, lambda: fresh.restore(buf), "checkpoint")
    assert fresh.order_counts().sum() == 0 and fresh.order_count(5) == 0 and fresh.steps_done() == 0
    M = bk.env.MAX_PRICE
    state = {"t": 0, "tick_size": 2, "trade_vol": 0, "trading": True, "trades": [],
             "orders": [{"order": {"side": "Bid", "status": "Active", "arr_time": 0, "end_time": 2**64 - 1, "vol": 10,
                                   "start_vol": 10, "price": 100, "trader_id": 0, "order_id": 0},
                         "key": ["Bid", M - 100, 0]}]}
    refused(bk, lambda: fresh.load_book_state(0, state), "loading a book")
    assert fresh.order_count(0) == 0
    for e in (plain, env, fresh):
        e.close()


@pytest.mark.parametrize("mode", ["auto", "split"])
def test_warm_leaves_the_log_alone(bk, mode):
    B, pool = 512, 128
    outs = []
    for warm in (False, True):
        env = make_env(bk, B, pool, max_orders=pool * 40)
        env.set_pipeline(mode)
        if warm:
            env.warm(12)
            assert env.order_counts().sum() == 0 and env.order_count(3) == 0
        env.run(20)
        if warm:
            env.warm(9)
        o = P.snapshot(env)
        o["orders"] = [env.orders(b) for b in range(B)]
        o["keys"] = [np.concatenate([k.astype(np.uint64) for k in env.order_keys(b)]) for b in range(B)]
        outs.append(o)
        env.close()
    P.assert_same(outs[0], outs[1])
