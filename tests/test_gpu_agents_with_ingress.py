"""On-device RandomAgents beside submitted instructions in one env (bk_update_agents): `agents.update(env, rng)`
(ref crates/step_sim/src/agents/random_agent.rs:85-119) queues its placements and cancellations in the device-resident
ingress queues with the book's own RNG, next to the instructions of bk_submit_instructions_device, and the step trades all
of it (env.rs:116-219, runner.rs:53-68).

Every book is checked field by field against one oracle.StepEnv(seed + b) + oracle.RandomAgentSet(groups) called in the
same order: level-2 history, trades, orders with their statuses, order keys and the RNG state after the run."""
import numpy as np
import pytest

import oracle_parity as P
from ingress_support import MOD, SEED, STEP, apply_oracle, check, ingress_env, submit

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bk():
    import bourse_amd

    return bourse_amd


def _groups(pool):
    return [(pool // 2, (32, 64), (10, 20), 2, 0.8), (pool // 4, (30, 66), (50, 70), 2, 0.3)]


@pytest.mark.parametrize("pool", [64, 128, 256, 512])
def test_agents_only_equal_the_oracle(bk, oracle, pool):
    import torch

    B, T = 64, 30
    groups = _groups(pool)
    na = sum(g[0] for g in groups)
    env = ingress_env(bk, torch, B, T, pool, na, na)
    env.set_random_agents(groups)
    refs = [oracle.StepEnv(SEED + b, 0, 2, STEP) for b in range(B)]
    agents = [oracle.RandomAgentSet(groups) for _ in range(B)]
    for _ in range(T):
        env.update_agents(sync=False)
        env.step(sync=False)
        for r, a in zip(refs, agents):
            a.update(r)
            r.step()
    P.no_flags(env)
    check(env, refs)
    assert int(env.trade_counts().sum()) > B * T
    env.close()


def _external(rng, refs, agents, n0, n_max, tick):
    """One step's random instructions for every book: limit and market orders, cancellations and modifications of the
    ids the book had before this step (n0) - half of the targets among the ids the agents hold."""
    B = len(refs)
    n_b = rng.integers(0, n_max + 1, size=B)
    off = np.zeros(B + 1, dtype=np.int64)
    off[1:] = np.cumsum(n_b)
    n = int(off[-1])
    action = rng.choice([1, 2, MOD], size=n, p=[0.55, 0.25, 0.2]).astype(np.uint32)
    bid = rng.integers(0, 2, size=n).astype(np.uint8)
    has_p, has_v = rng.integers(0, 2, size=n).astype(np.uint8), rng.integers(0, 2, size=n).astype(np.uint8)
    side = np.where(action == MOD, (has_p << 1) | (has_v << 2), bid).astype(np.uint8)
    vol = rng.integers(1, 40, size=n).astype(np.uint32)
    trader = rng.integers(1000, 2000, size=n).astype(np.uint32)
    price = (rng.integers(30, 68, size=n) * 2 * tick // 2).astype(np.uint32)
    market = (action == 1) & (rng.random(n) < 0.15)
    price[market] = np.where(bid[market] == 1, 0xFFFFFFFF, 0)  # a market order: the extreme prices (tick 1)
    order_id = np.zeros(n, dtype=np.uint64)
    for b in range(B):
        n_orders = int(n0[b])
        held = np.concatenate([agents[b].held_ids(g) for g in range(len(agents[b].groups))])
        held = held[held < n_orders]
        for i in range(int(off[b]), int(off[b + 1])):
            if action[i] == 1:
                continue
            if n_orders == 0:
                action[i] = 0  # nothing to target yet: a no-op
            elif len(held) and rng.random() < 0.5:
                order_id[i] = held[rng.integers(0, len(held))]
            else:
                order_id[i] = rng.integers(0, n_orders)
    return off, (action, side, vol, trader, price, order_id)


@pytest.mark.parametrize("agents_first", [True, False])
def test_agents_with_external_instructions_equal_the_oracle(bk, oracle, agents_first):
    import torch

    B, T, pool, NX = 64, 24, 256, 6
    groups = [(64, (32, 64), (10, 20), 2, 0.8), (32, (30, 66), (50, 70), 2, 0.3)]
    na = 96
    env = ingress_env(bk, torch, B, T, pool, na, na + NX, tick=1, n_ext=NX)
    env.set_random_agents(groups)
    refs = [oracle.StepEnv(SEED + b, 0, 1, STEP) for b in range(B)]
    agents = [oracle.RandomAgentSet(groups) for _ in range(B)]
    rng = np.random.default_rng(7 + agents_first)
    hits = 0
    for _ in range(T):
        n0 = [r.book.n_orders() for r in refs]
        if agents_first:
            env.update_agents(sync=False)
            for r, a in zip(refs, agents):
                a.update(r)
        off, ins = _external(rng, refs, agents, n0, NX, 1)
        submit(torch, env, off, ins)
        for b, r in enumerate(refs):
            apply_oracle(r, int(off[b]), int(off[b + 1]), ins)
        if not agents_first:
            env.update_agents(sync=False)
            for r, a in zip(refs, agents):
                a.update(r)
        hits += int(((ins[0] == 2) | (ins[0] == MOD)).sum())
        env.step(sync=False)
        for r in refs:
            r.step()
    assert hits > B * T // 2
    P.no_flags(env)
    check(env, refs)
    env.close()


def test_two_updates_in_a_step_no_trading_step_and_a_per_book_table(bk, oracle):
    import torch

    B, T, pool = 64, 16, 512  # (an order placed by the first of two updates and replaced by the second stays, unowned)
    rng = np.random.default_rng(11)
    table = [[(48, (int(lo), int(lo) + int(w)), (int(v), int(v) + 9), 2, float(np.float32(rate))),
              (16, (30, 70), (40, 60), 4, 0.25)]
             for lo, w, v, rate in zip(rng.integers(20, 40, B), rng.integers(5, 40, B), rng.integers(1, 30, B),
                                       rng.uniform(0.1, 0.95, B))]
    na = 64
    env = ingress_env(bk, torch, B, T, pool, 2 * na, 2 * na)
    env.set_random_agents_per_book(table)
    refs = [oracle.StepEnv(SEED + b, 0, 2, STEP) for b in range(B)]
    agents = [oracle.RandomAgentSet(table[b]) for b in range(B)]
    for s in range(T):
        if s == 5:
            env.disable_trading()
            for r in refs:
                r.disable_trading()
        if s == 6:
            env.enable_trading()
            for r in refs:
                r.enable_trading()
        for _ in range(2 if s % 3 == 1 else 1):
            env.update_agents(sync=False)
            for r, a in zip(refs, agents):
                a.update(r)
        env.step(sync=False)
        for r in refs:
            r.step()
    P.no_flags(env)
    check(env, refs)
    env.close()


def test_replaced_agents_forget_their_orders(bk, oracle):
    import torch

    B, T, pool = 64, 20, 256
    g1 = [(64, (32, 64), (10, 20), 2, 0.6)]
    g2 = [(40, (36, 60), (5, 15), 2, 0.9), (24, (30, 70), (20, 30), 2, 0.4)]
    env = ingress_env(bk, torch, B, T, pool, 64, 64)
    env.set_random_agents(g1)
    refs = [oracle.StepEnv(SEED + b, 0, 2, STEP) for b in range(B)]
    agents = [oracle.RandomAgentSet(g1) for _ in range(B)]
    for s in range(T):
        if s == 8:  # a new RandomAgents::new: the old orders stay on the books, unowned
            env.set_random_agents(g2)
            agents = [oracle.RandomAgentSet(g2) for _ in range(B)]
        env.update_agents(sync=False)
        for r, a in zip(refs, agents):
            a.update(r)
        env.step(sync=False)
        for r in refs:
            r.step()
    P.no_flags(env)
    check(env, refs)
    env.close()


def test_update_agents_equals_bk_run_at_8192_books(bk, oracle):
    import torch

    B, T, pool = 8192, 20, 128
    groups = [(64, (32, 64), (10, 20), 2, 0.8), (64, (32, 64), (50, 70), 2, 0.2)]
    dev = ingress_env(bk, torch, B, T, pool, 128, 128, levels=16, n_orders=64 * T)
    dev.set_random_agents(groups)
    run = bk.ManyBookEnv(B, SEED, 0, 2, STEP, levels=16, max_live_orders=pool, max_orders=64 * T,
                         trade_capacity=2 * 64 * T, history_capacity=T)
    run.enable_agent_order_log()
    run.set_random_agents(groups)
    for _ in range(T):
        dev.update_agents(sync=False)
        dev.step(sync=False)
    run.run(T)
    dev.sync()
    assert not dev.flags().any() and not run.flags().any()
    P.same_history(dev.history(), run.history())
    assert np.array_equal(dev.trade_counts(), run.trade_counts())
    for b in sorted(set(range(0, B, 509)) | {B - 1}):
        P.same_records(dev.trades(b, first=0), run.trades(b, first=0), (b,), "trade")
        P.same_records(dev.orders(b), run.orders(b), (b,), "order")
        assert dev.rng_state(b) == run.rng_state(b), b
    dev.close()
    run.close()


NOISE = dict(tick_size=2, p_limit=0.2, p_market=0.2, p_cancel=0.1, trade_vol=100, price_dist_mu=0.0, price_dist_sigma=1.0)


def test_refusals_and_capacity_flags(bk, oracle):
    import torch

    groups = [(32, (32, 64), (10, 20), 2, 0.9)]
    B = 16
    # no device ingress: refused, and the env still runs its own flow
    env = bk.ManyBookEnv(B, SEED, 0, 2, STEP, max_live_orders=64, history_capacity=2)
    env.set_random_agents(groups)
    with pytest.raises(bk.BourseError, match="bk_device_ingress_enable"):
        env.update_agents()
    env.run(2)
    env.close()
    # no groups; then Noise members: refused, the queues still step; bk_run and checkpoints stay refused
    env = ingress_env(bk, torch, B, 4, 64, 32, 32)
    with pytest.raises(bk.BourseError, match="no RandomAgents"):
        env.update_agents()
    env.set_agents([("noise", 0, 8, NOISE)])
    with pytest.raises(bk.BourseError, match="Noise / Momentum"):
        env.update_agents()
    env.step()
    env.set_random_agents(groups)
    env.update_agents()
    env.step()
    with pytest.raises(bk.BourseError, match="bk_run cannot be mixed"):
        env.run(1)
    with pytest.raises(bk.BourseError):
        env.checkpoint()
    refs = [oracle.StepEnv(SEED + b, 0, 2, STEP) for b in range(B)]
    agents = [oracle.RandomAgentSet(groups) for _ in range(B)]
    for r, a in zip(refs, agents):
        r.step()
        a.update(r)
        r.step()
    P.no_flags(env)
    check(env, refs)
    env.close()
    # markets (assets > 1)
    env = bk.ManyBookEnv(2 * B, SEED, 0, 2, STEP, max_live_orders=64, assets=2,
                         stream=torch.cuda.current_stream().cuda_stream)
    env.enable_device_ingress(32)
    env.set_random_market_agents([(0, 16, (32, 64), (10, 20), 2, 0.9)])
    with pytest.raises(bk.BourseError, match="assets == 1"):
        env.update_agents()
    env.step()
    env.close()
    # a queue smaller than the agents' events: flagged, never silent; a strict env raises
    for strict in (True, False):
        env = ingress_env(bk, torch, B, 2, 64, 32, 8, strict=strict)
        env.set_random_agents(groups)
        if strict:
            with pytest.raises(bk.CapacityError, match="EVENT_OVERFLOW"):
                env.update_agents()
        else:
            env.update_agents()
            assert (env.flags() & bk._lib.FLAG_EVENT_OVERFLOW).all()
            assert all(env.order_count(b) <= 8 for b in range(B))
            # the drop rule: a fresh env's first update (nobody holds an id) takes the oracle's draws whether an event fits
            # or not, and queues exactly the first `room` placements, in agent order
            for b in range(B):
                ref = oracle.StepEnv(SEED + b, 0, 2, STEP)
                oracle.RandomAgentSet(groups).update(ref)
                want = ref.book.orders_array()
                assert len(want) > 8, (b, len(want))  # the queue overflows in this book
                assert env.rng_state(b) == tuple(int(x) for x in ref.rng_state()), b
                assert env.order_count(b) == 8, b
                got = env.orders(b)
                for f in ("side", "price", "vol", "trader_id"):
                    assert np.array_equal(got[f], want[f][:8]), (b, f, got[f], want[f][:8])
        env.step()
        env.close()
