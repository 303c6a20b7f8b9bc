"""On-device RandomMarketAgents beside submitted instructions in one market env (bk_update_market_agents):
`RandomMarketAgents::update` (ref crates/step_sim/src/agents/random_agent.rs:204-245) queues its placements and
cancellations in every market's device-resident queue with the market's own RNG, next to the instructions of
bk_submit_instructions_device, and the step trades all of it (market_env.rs, runner.rs:108-131).

Every book (m, a) is checked against oracle.ManyMarkets.book(m, a) - level-2 history, trades, live orders, the order log
and keys - and the RNG words of every book of a market against rng_states()[m] (tests/market_ingress_support.py).
ManyMarkets runs update and step in one call (run(1)), so on real markets the call orders other than submit - update - step
are pinned only through the shared append rule; they are pinned directly on a one-asset env, where the entry runs the same
kernels, against oracle.StepEnv + RandomAgentSet."""
import numpy as np
import pytest

import oracle_parity as P
from ingress_support import SEED, STEP, apply_oracle, check, ingress_env, submit
from market_ingress_support import check_markets, external, many_markets, market_env, submit_markets

pytestmark = pytest.mark.gpu
TICKS = [1, 2, 1]
NM, T = 33, 24


@pytest.fixture(scope="module")
def bk():
    import bourse_amd

    return bourse_amd


def _groups(pool):
    """asset order 0, 1, 2, 0, 2, 1; at 256 slots 70 (two passes) / 5 (a cut inside a wave) / 0 / 20 / 64 / 40 agents"""
    n = [70 * pool // 256, 5 * pool // 256, 0, 20 * pool // 256, 64 * pool // 256, 40 * pool // 256]
    return [(0, n[0], (32, 64), (10, 20), 1, 0.8), (1, n[1], (30, 66), (50, 70), 2, 0.5), (2, n[2], (32, 64), (10, 20), 1, 0.8),
            (0, n[3], (30, 66), (50, 70), 2, 0.3), (2, n[4], (32, 64), (10, 20), 2, 0.8), (1, n[5], (32, 64), (10, 20), 4, 0.7)]


def _env(bk, torch, pool, groups, n_ext=0, nm=NM, steps=T, strict=True, qcap=None):
    na = sum(g[1] for g in groups)
    return market_env(bk, torch, nm, TICKS, steps, pool, na + n_ext if qcap is None else qcap, (na + n_ext) * steps + 16, strict)


def _busy(ref, least_trades):
    """the expected side trades in every book"""
    fewest = min(ref.book(m, a).n_trades() for m in range(ref.n_markets) for a in range(ref.assets))
    assert fewest >= least_trades, fewest


# ------------------------------------------------------------------------------------------------ 1. agents only
@pytest.mark.parametrize("pool", [64, 128, 256, 512])
def test_market_agents_only_equal_the_oracle(bk, oracle, pool):
    import torch

    groups = _groups(pool)
    assert [g[0] for g in groups] == [0, 1, 2, 0, 2, 1] and groups[2][1] == 0
    if pool >= 256:
        assert groups[0][1] > 64 and groups[1][1] < 64
    env = _env(bk, torch, pool, groups)
    env.set_random_market_agents(groups)
    ref = many_markets(oracle, NM, TICKS, groups=groups)
    for _ in range(T):
        env.update_market_agents(sync=False)
        env.step(sync=False)
    ref.run(T)
    _busy(ref, T)  # (a comparison of idle books says nothing)
    P.no_flags(env)
    check_markets(env, lambda m: (ref, m))
    env.close()


# ------------------------------------------------------------------------------------------------ 2. submit, then update
def test_submit_then_update_equals_the_oracle(bk, oracle):
    import torch

    pool, NX = 256, 3
    groups = _groups(pool)
    env = _env(bk, torch, pool, groups, n_ext=NX * len(TICKS))
    env.set_random_market_agents(groups)
    ref = many_markets(oracle, NM, TICKS, groups=groups)
    rng = np.random.default_rng(5)
    targets = 0
    for _ in range(T):
        n0 = [ref.book(b // 3, b % 3).n_orders() for b in range(env.n_books)]
        off, ins, t = external(rng, n0, TICKS, NX)
        targets += t
        submit_markets(torch, env, lambda m: (ref, m), off, ins)
        env.update_market_agents(sync=False)
        env.step(sync=False)
        ref.run(1)
    assert targets > 33 * 24 // 2, targets
    _busy(ref, T)
    P.no_flags(env)
    check_markets(env, lambda m: (ref, m))
    env.close()


# ------------------------------------------------------------------------------------------------ 3. the call orders
@pytest.mark.parametrize("mode", ["alone", "alternated", "submit_between", "twice"])
def test_a_one_asset_env_equals_the_book_oracle_in_every_call_order(bk, oracle, mode):
    """the market entry on a market of one book: on its own, alternated step by step with bk_update_agents (they share
    the held ids), on either side of a submit, and twice in a step"""
    import torch

    B, steps, pool, NX = 64, 18, 512, 4
    groups = [(70, (32, 64), (10, 20), 1, 0.8), (5, (30, 66), (50, 70), 2, 0.3), (0, (32, 64), (10, 20), 1, 0.5),
              (20, (32, 64), (10, 20), 1, 0.7)]
    na = 95
    env = ingress_env(bk, torch, B, steps, pool, 2 * na, 2 * na + NX, tick=1, n_ext=NX)
    env.set_random_agents(groups)
    refs = [oracle.StepEnv(SEED + b, 0, 1, STEP) for b in range(B)]
    agents = [oracle.RandomAgentSet(groups) for _ in range(B)]
    rng = np.random.default_rng(3)

    def update(s):
        (env.update_agents if mode == "alternated" and s % 2 else env.update_market_agents)(sync=False)
        for r, a in zip(refs, agents):
            a.update(r)

    for s in range(steps):
        before = (mode == "submit_between" and s % 2 == 0) or (mode == "twice" and s % 3 == 1)
        if before:
            update(s)
        n0 = [r.book.n_orders() for r in refs]
        off, ins, _ = external(rng, n0, [1], NX, band=(16, 34))
        submit(torch, env, off, ins)
        for b, r in enumerate(refs):
            apply_oracle(r, int(off[b]), int(off[b + 1]), ins)
        if mode == "twice" or not before:
            update(s)
        env.step(sync=False)
        for r in refs:
            r.step()
    assert min(r.book.n_trades() for r in refs) >= steps
    P.no_flags(env)
    check(env, refs)
    env.close()


# ------------------------------------------------------------------------------------------------ 5. a per-market table
def test_a_per_market_table_equals_the_uniform_set_of_each_row(bk, oracle):
    import torch

    pool, steps = 128, 12
    rows = [_groups(pool), [(a, n, (tr[0] + 3, tr[1] + 9), (vr[0] + 5, vr[1] + 30), ts, 0.6) for a, n, tr, vr, ts, _ in _groups(pool)]]
    table = [rows[m % 2 if m != 5 else 0] for m in range(NM)]
    env = _env(bk, torch, pool, rows[0], steps=steps)
    env.set_random_market_agents_per_market(table)
    refs = [many_markets(oracle, 1, TICKS, seed=SEED + m, groups=table[m]) for m in range(NM)]
    for _ in range(steps):
        env.update_market_agents(sync=False)
        env.step(sync=False)
    for r in refs:
        r.run(steps)
        _busy(r, steps // 2)
    P.no_flags(env)
    check_markets(env, lambda m: (refs[m], 0))
    env.close()


# ------------------------------------------------------------------------------------------------ 6. capacity
def test_a_queue_that_runs_out_inside_the_second_asset_flags_that_book(bk, oracle):
    """a fresh market's first update (nobody holds an id): 40 agents of asset 0 at rate 1 take 40 slots of a 50-slot queue,
    the group of asset 1 runs out inside its pass; the draws are taken all the same"""
    import torch

    nm, room = 8, 50
    groups = [(0, 40, (32, 64), (10, 20), 1, 1.0), (1, 40, (32, 64), (10, 20), 2, 1.0), (2, 8, (32, 64), (10, 20), 1, 1.0)]
    env = _env(bk, torch, 128, groups, nm=nm, steps=2, strict=False, qcap=room)
    env.set_random_market_agents(groups)
    env.update_market_agents()
    ref = many_markets(oracle, nm, TICKS, groups=groups)
    ref.set_trading(False)
    ref.run(1)  # (no trading: the oracle's orders all rest, in placement order)
    flags = env.flags().reshape(nm, 3)
    over = np.uint32(bk._lib.FLAG_EVENT_OVERFLOW)
    assert (flags[:, 1] & over).all() and (flags[:, 2] & over).all() and not flags[:, 0].any(), flags
    for m in range(nm):
        want = [ref.book(m, a).orders_array() for a in range(3)]
        # (ManyMarkets' run(1) has shuffled behind the update; while nobody holds an id the walk's draws do not depend on
        # the assets, so the state after the update alone is that of the same groups on one oracle book)
        one = oracle.StepEnv(SEED + m, 0, 1, STEP)
        oracle.RandomAgentSet([g[1:] for g in groups]).update(one)
        want_rng = tuple(int(x) for x in one.rng_state())
        assert [len(w) for w in want] == [40, 40, 8]
        for a, n in enumerate((40, room - 40, 0)):  # exactly `room` events: the oracle's first ones
            b = 3 * m + a
            assert env.order_count(b) == n, (m, a)
            got = env.orders(b)
            for f in ("side", "price", "vol", "trader_id"):
                assert np.array_equal(got[f], want[a][f][:n]), (m, a, f)
            assert env.rng_state(b) == want_rng, (m, a)
    env.step()
    env.close()
    with pytest.raises(bk.CapacityError, match="EVENT_OVERFLOW"):
        env = _env(bk, torch, 128, groups, nm=nm, steps=2, strict=True, qcap=room)
        env.set_random_market_agents(groups)
        try:
            env.update_market_agents()
        finally:
            env.close()


# ------------------------------------------------------------------------------------------------ 7. reset
def test_a_reset_market_rewinds_its_held_ids(bk, oracle):
    """save after 5 steps, 5 more, every other market reset, 5 more: a reset market equals a fresh replay of 5 + 5 steps
    (its agents hold the ids of step 5 again - holding those of the abandoned run, they would cancel other orders or
    none), the others run on"""
    import torch

    pool, n, k = 256, 5, 5
    groups = _groups(pool)
    env = _env(bk, torch, pool, groups, steps=n + 2 * k)
    env.set_random_market_agents(groups)
    refs = [many_markets(oracle, 1, TICKS, seed=SEED + m, groups=groups) for m in range(NM)]

    def run(steps):
        for _ in range(steps):
            env.update_market_agents(sync=False)
            env.step(sync=False)
        for r in refs:
            r.run(steps)

    run(n)
    env.save_ingress_snapshot()
    base = [[r.book(0, a).n_trades() for a in range(3)] for r in refs]
    run(k)
    mask = (np.arange(NM) % 2 == 1).astype(np.uint8)
    env.reset_ingress_markets(mask)
    for m in np.flatnonzero(mask):
        refs[m] = many_markets(oracle, 1, TICKS, seed=SEED + int(m), groups=groups)
        refs[m].run(n)
    run(k)
    env.sync()
    P.no_flags(env)
    hist = env.history()
    for m, ref in enumerate(refs):
        want_hist = ref.history()
        for a in range(3):
            b, view, tag = 3 * m + a, ref.book(0, a), (m, a, "reset" if mask[m] else "kept")
            P.same_history(hist[-k:, b], want_hist[-k:, a], f"{tag}: L2 history tail")
            assert env.rng_state(b) == tuple(int(x) for x in ref.rng_states()[0]), tag
            first = base[m][a] if mask[m] else 0
            assert env.trade_count(b) == (view.n_trades(), first), tag
            P.same_records(env.trades(b), view.trades_array()[first:], tag, "retained trade")
            P.same_live(env, b, view, tag)
            P.same_orders(env, b, view, tag)
            P.same_keys(env, b, view, tag)
    assert min(r.book(0, a).n_trades() for r in refs for a in range(3)) >= n + k
    env.close()


# ------------------------------------------------------------------------------------------------ 8. refusals
def test_refusals_leave_the_env_stepping(bk, oracle):
    import torch

    noise = dict(tick_size=2, p_limit=0.2, p_market=0.2, p_cancel=0.1, trade_vol=100, price_dist_mu=0.0, price_dist_sigma=1.0)
    groups = [(0, 16, (32, 64), (10, 20), 1, 0.9), (1, 16, (32, 64), (10, 20), 2, 0.9)]
    # no device ingress
    env = bk.ManyMarketEnv(4, SEED, 0, [1, 2], STEP, max_live_orders=64, history_capacity=2)
    env.set_random_market_agents(groups)
    with pytest.raises(bk.BourseError, match="bk_device_ingress_enable"):
        env.update_market_agents()
    env.run(2)
    env.close()
    # nothing installed; then Noise / Momentum members: the message names the other entry
    env = market_env(bk, torch, 4, [1, 2], 4, 64, 64, 256)
    with pytest.raises(bk.BourseError, match="no RandomMarketAgents"):
        env.update_market_agents()
    env.step()
    env.set_market_agents([(1, ("noise", 0, 8, noise))])
    with pytest.raises(bk.BourseError, match="bk_update_market_members"):
        env.update_market_agents()
    env.step()
    # the book entry keeps its refusal of markets, word for word
    env.set_random_market_agents(groups)
    with pytest.raises(bk.BourseError, match=r"bk_update_agents runs RandomAgents on independent books \(assets == 1\)"):
        env.update_agents()
    env.update_market_agents()
    env.step()
    ref = many_markets(oracle, 4, [1, 2], groups=groups)
    ref.step()
    ref.step()
    ref.run(1)
    P.no_flags(env)
    check_markets(env, lambda m: (ref, m))
    env.close()
