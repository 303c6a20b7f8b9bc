"""On-device NoiseMarketAgent / MomentumMarketAgent / RandomMarketAgents members beside submitted instructions in one market
env (bk_update_market_members): `MarketAgent::update` of a MarketAgentSet (ref crates/step_sim/src/agents/
noise_agent.rs:226-340, momentum_agent.rs:282-397, random_agent.rs:204-245), members in declaration order with the market's
own RNG, into every market's device-resident queue, next to the instructions of bk_submit_instructions_device.

Every book (m, a) is checked against oracle.ManyMarkets(members=...).book(m, a) and the RNG words of every book of a market
against rng_states()[m] (tests/market_ingress_support.py); busy conditions are counted on the expected side and asserted
before anything is compared.  The call orders are pinned on a one-asset env against oracle.StepEnv + AgentSet."""
import numpy as np
import pytest

import accounts_model as AM
import open_orders_model as OM
import oracle_parity as P
from ingress_support import SEED, STEP, check, members_env, submit, thin_flow
from market_ingress_support import check_markets, external, many_markets, market_env, submit_markets
from members_ingress_cases import MOM, NOISE

pytestmark = pytest.mark.gpu
TICKS = [2, 2, 2]
NM = 33
U64_MAX = 0xFFFFFFFFFFFFFFFF


@pytest.fixture(scope="module")
def bk():
    import bourse_amd

    return bourse_amd


RND = (32, 64), (10, 20), 2
# the set of seven: more members than bk_run's kernels hold (a device-ingress env takes eight), two that return to asset 0,
# members wider than a wave on assets 0 and 2, disjoint trader ranges above the RandomAgents' indices
SEVEN = [(0, ("random", 72, *RND, 0.8)), (1, ("noise", 1000, 20, NOISE)), (0, ("momentum", 2000, 10, MOM)),
         (2, ("random", 5, *RND, 0.8)), (1, ("momentum", 3000, 10, MOM)),
         (2, ("noise", 4000, 70, dict(NOISE, p_limit=0.6, p_market=0.3))), (0, ("noise", 5000, 12, NOISE))]


def _small(pool):
    """a set for the smaller pools: one RandomAgents member, Noise members on assets 0 and 2, a Momentum member behind the
    Noise member of its asset"""
    n = pool // 8
    return [(1, ("random", pool // 2, *RND, 0.8)), (0, ("noise", 1000, n, dict(NOISE, p_cancel=0.4))),
            (0, ("momentum", 2000, 6, dict(MOM, p_cancel=0.5))),
            (2, ("noise", 4000, 6, dict(NOISE, p_limit=0.5, p_market=0.4, p_cancel=0.4)))]


def _events(members):
    """the most events one update queues: an order per RandomAgents agent, two per trader"""
    return sum(m[1] if m[0] == "random" else 2 * m[2] for _, m in members)


def _env(bk, torch, pool, members, steps, n_ext=0, nm=NM, strict=True, qcap=None):
    per = _events(members)
    return market_env(bk, torch, nm, TICKS, steps, pool, (per + 3 * pool + n_ext) if qcap is None else qcap,
                      (per + n_ext) * steps + 16, strict)


def _thin(rng, env):
    """a thin external flow: a few limit orders per book, new orders only (a Momentum member needs a moving mid price)"""
    off, ins, _ = external(rng, [0] * env.n_books, TICKS, 2, new_only=True, band=(10, 15))
    return off, ins


def _busy(ref, members, steps):
    """counted on the expected side: trades in every book, market orders on every asset that has a Noise / Momentum member,
    orders of every member"""
    most_live = 0
    for m in range(ref.n_markets):
        for a in range(ref.assets):
            view = ref.book(m, a)
            assert view.n_trades() > steps, (m, a, view.n_trades())
            o = view.orders_array()
            most_live = max(most_live, int((o["status"] == 1).sum()))
            market = ((o["side"] == 1) & (o["price"] == 0xFFFFFFFF)) | ((o["side"] == 0) & (o["price"] == 0))
            if m == 0:
                if any(ma == a and mem[0] != "random" for ma, mem in members):
                    assert market.any(), (a, "no market order")
                for ma, mem in members:
                    if ma == a:
                        lo, n = (0, mem[1]) if mem[0] == "random" else (mem[1], mem[2])
                        assert ((o["trader_id"] >= lo) & (o["trader_id"] < lo + n)).any(), (a, mem[0], lo)
    return most_live


def _check_member_orders(env, members, markets):
    """every listed id is an order of the member's asset and trader range (the same list from every book of the market)"""
    A = env.assets
    for m in markets:
        for j, (a, mem) in enumerate(members):
            ids = env.member_orders(m * A + a, j)
            assert np.array_equal(ids, env.member_orders(m * A + (a + 1) % A, j)), (m, j)
            ids = ids[ids != U64_MAX]
            lo, n = (0, mem[1]) if mem[0] == "random" else (mem[1], mem[2])
            traders = env.orders(m * A + a)["trader_id"]
            assert (ids < len(traders)).all(), (m, j, ids)
            t = traders[ids.astype(np.int64)]
            assert ((t >= lo) & (t < lo + n)).all(), (m, j, t)
            if mem[0] == "random":
                assert len(env.member_orders(m * A + a, j)) == mem[1], (m, j)


# ------------------------------------------------------------------------------------------------ 4. members
def _run_beside_thin_flow(bk, oracle, torch, pool, members, steps, seed):
    env = _env(bk, torch, pool, members, steps, n_ext=2 * len(TICKS))
    env.set_market_agents(members)
    ref = many_markets(oracle, NM, TICKS, members=members)
    rng = np.random.default_rng(seed)
    for _ in range(steps):
        submit_markets(torch, env, lambda m: (ref, m), *_thin(rng, env))
        env.update_market_members(sync=False)
        env.step(sync=False)
        ref.run(1)
    return env, ref


def test_seven_members_on_three_assets_equal_the_oracle(bk, oracle):
    import torch

    steps = 30
    env, ref = _run_beside_thin_flow(bk, oracle, torch, 512, SEVEN, steps, 41)
    most_live = _busy(ref, SEVEN, steps)
    assert 128 < most_live < 512, most_live  # the pool's upper registers hold orders; nothing is dropped for room
    P.no_flags(env)
    check_markets(env, lambda m: (ref, m))
    _check_member_orders(env, SEVEN, range(0, NM, 8))
    env.close()


@pytest.mark.parametrize("pool", [64, 128, 256])
def test_a_smaller_set_equals_the_oracle_at_every_pool_size(bk, oracle, pool):
    import torch

    steps, members = 24, _small(pool)
    env, ref = _run_beside_thin_flow(bk, oracle, torch, pool, members, steps, 50 + pool)
    most_live = _busy(ref, members, steps // 4)  # (a book trades every fourth step at the least)
    assert most_live < pool, most_live
    P.no_flags(env)
    check_markets(env, lambda m: (ref, m))
    _check_member_orders(env, members, range(0, NM, 8))
    env.close()


# ------------------------------------------------------------------------------------------------ 3. the call orders
@pytest.mark.parametrize("mode", ["alone", "alternated", "twice"])
def test_a_one_asset_env_equals_the_book_oracle_in_every_call_order(bk, oracle, mode):
    """the market entry on a market of one book: on its own, alternated step by step with bk_update_members (they share
    the lists and the momentum state), and twice in a step"""
    import torch

    B, steps, R, NX = 64, 18, 4, 4
    members = [("random", 16, (32, 64), (10, 20), 2, 0.6), ("noise", 16, 10, NOISE), ("momentum", 26, 10, MOM)]
    env = members_env(bk, torch, B, steps, 64 * R, members, 1, n_ext=NX, updates=2)
    env.set_agents(members)
    refs = [oracle.StepEnv(SEED + b, 0, 1, STEP) for b in range(B)]
    sets = [oracle.AgentSet(members) for _ in range(B)]
    rng = np.random.default_rng(29)

    def update(s):
        (env.update_members if mode == "alternated" and s % 2 else env.update_market_members)(sync=False)
        for r, a in zip(refs, sets):
            a.update(r)

    for s in range(steps):
        if mode == "twice" and s % 3 == 1:
            update(s)
        off, ins = thin_flow(rng, B, NX, 1)
        submit(torch, env, off, ins)
        for b, r in enumerate(refs):
            for i in range(int(off[b]), int(off[b + 1])):
                r.place_order(bool(ins[1][i] & 1), int(ins[2][i]), int(ins[3][i]), price=int(ins[4][i]))
        update(s)
        env.step(sync=False)
        for r in refs:
            r.step()
    assert min(r.book.n_trades() for r in refs) > 0 and sum(r.book.n_trades() for r in refs) > B * steps
    P.no_flags(env)
    check(env, refs)
    for b in range(0, B, 7):
        for j, m in enumerate(members):
            if m[0] != "random":
                assert np.array_equal(env.member_orders(b, j), sets[b].order_list(j)), (b, j)
    env.close()


# ------------------------------------------------------------------------------------------------ 5. a per-market table
def test_a_per_market_table_equals_the_uniform_set_of_each_row(bk, oracle):
    import torch

    pool, steps = 128, 16
    rows = [_small(pool), [(a, (m[0], m[1], *m[2:5], 0.5) if m[0] == "random" else
                            (m[0], m[1] + 100, m[2], dict(m[3], trade_vol=60, p_cancel=0.3))) for a, m in _small(pool)]]
    table = [rows[m % 2 if m != 4 else 1] for m in range(NM)]
    env = _env(bk, torch, pool, rows[0], steps, n_ext=2 * len(TICKS))
    env.set_market_agents_per_market(table)
    refs = [many_markets(oracle, 1, TICKS, seed=SEED + m, members=table[m]) for m in range(NM)]
    rng = np.random.default_rng(61)
    for _ in range(steps):
        submit_markets(torch, env, lambda m: (refs[m], 0), *_thin(rng, env))
        env.update_market_members(sync=False)
        env.step(sync=False)
        for r in refs:
            r.run(1)
    assert sum(r.book(0, a).n_trades() for r in refs for a in range(3)) > 3 * NM * steps // 2
    P.no_flags(env)
    check_markets(env, lambda m: (refs[m], 0))
    for m in (0, 1, 4):
        _check_member_orders(env, table[m], [m])
    env.close()


# ------------------------------------------------------------------------------------------------ 6. capacity
def test_a_short_queue_flags_the_book_of_the_dropped_event(bk, oracle):
    """a fresh market's first update: 24 RandomAgents of asset 0 at rate 1 (24 events), then 16 Noise traders of asset 1
    who all place both orders (32 events) in a queue of 40: the room runs out inside the Noise member's loop"""
    import torch

    nm, room = 8, 40
    members = [(0, ("random", 24, *RND, 1.0)), (1, ("noise", 1000, 16, dict(NOISE, p_limit=1.0, p_market=1.0))),
               (2, ("random", 4, *RND, 1.0))]
    env = _env(bk, torch, 128, members, 2, nm=nm, strict=False, qcap=room)
    env.set_market_agents(members)
    env.update_market_members()
    ref = many_markets(oracle, nm, TICKS, members=members)
    ref.set_trading(False)
    ref.run(1)
    flags = env.flags().reshape(nm, 3)
    over = np.uint32(bk._lib.FLAG_EVENT_OVERFLOW)
    assert (flags[:, 1] == over).all() and (flags[:, 2] == over).all() and not flags[:, 0].any(), flags
    for m in range(nm):
        want = [ref.book(m, a).orders_array() for a in range(3)]
        assert [len(w) for w in want] == [24, 32, 4]
        one = oracle.StepEnv(SEED + m, 0, 2, STEP)  # (the draws of a first update do not depend on the assets)
        oracle.AgentSet([mem for _, mem in members]).update(one)
        for a, n in enumerate((24, room - 24, 0)):
            b = 3 * m + a
            assert env.order_count(b) == n, (m, a)  # a dropped New uses no id
            got = env.orders(b)
            for f in ("side", "price", "vol", "trader_id"):
                assert np.array_equal(got[f], want[a][f][:n]), (m, a, f)
            assert env.rng_state(b) == tuple(int(x) for x in one.rng_state()), (m, a)
        listed = env.member_orders(3 * m + 1, 1)
        limit = want[1]["order_id"][:room - 24][~_is_market(want[1][:room - 24])]
        assert np.array_equal(listed, limit), (m, listed, limit)  # ... and enters no list
    env.step()
    env.close()


def _is_market(o):
    return ((o["side"] == 1) & (o["price"] == 0xFFFFFFFF)) | ((o["side"] == 0) & (o["price"] == 0))


# ------------------------------------------------------------------------------------------------ 7. reset
@pytest.mark.parametrize("views", [False, True])
def test_a_reset_market_rewinds_its_lists_and_momentum(bk, oracle, views):
    """save after 5 steps, 5 more, every other market reset, 5 more: a reset market equals a fresh replay of 5 + 5 steps,
    the others run on; with `views`, the trader accounts (tests/accounts_model.py: a reset book counts from its reset) and
    the open orders (tests/open_orders_model.py) of the external traders 0 .. 7 beside update_market_members"""
    import torch

    pool, n, k, NT = 256, 5, 5, 8
    members = _small(pool)
    env = _env(bk, torch, pool, members, n + 2 * k, n_ext=2 * len(TICKS))
    if views:
        env.enable_accounts(NT)
        env.enable_open_orders(NT, depth=4)
    env.set_market_agents(members)
    refs = [many_markets(oracle, 1, TICKS, seed=SEED + m, members=members) for m in range(NM)]
    log = [[] for _ in range(NM)]
    rng = np.random.default_rng(71)

    def run(steps):
        for _ in range(steps):
            off, ins = _thin(rng, env)
            ins[3][:] = ins[3] % NT  # external traders 0 .. NT - 1: the ones with a row
            submit_markets(torch, env, lambda m: (refs[m], 0), off, ins)
            for m in range(NM):
                log[m].append((off[3 * m:3 * m + 4].copy(), ins))
            env.update_market_members(sync=False)
            env.step(sync=False)
            for r in refs:
                r.run(1)

    run(n)
    env.save_ingress_snapshot()
    base = [[r.book(0, a).n_trades() for a in range(3)] for r in refs]
    run(k)
    mask = (np.arange(NM) % 2 == 0).astype(np.uint8)
    env.reset_ingress_markets(mask)
    from market_ingress_support import apply_market

    for m in np.flatnonzero(mask):
        ref = many_markets(oracle, 1, TICKS, seed=SEED + int(m), members=members)
        for off, ins in log[m][:n]:
            for a in range(3):
                apply_market(ref, 0, a, int(off[a]), int(off[a + 1]), ins)
            ref.run(1)
        refs[m] = ref
    run(k)
    env.sync()
    P.no_flags(env)
    hist = env.history()
    acct = env.accounts() if views else None
    opened = env.open_orders() if views else None
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
            if views:
                orders = view.orders_array()
                want = AM.fold(view.trades_array(), orders, NT, first=first)
                assert np.array_equal(acct[b], want), (tag, acct[b], want)
                summary, entries = OM.rows(orders, NT, 4)
                assert np.array_equal(opened[0][b], summary) and np.array_equal(opened[1][b], entries), tag
    assert min(r.book(0, a).n_trades() for r in refs for a in range(3)) > 0
    _check_member_orders(env, members, range(0, NM, 5))
    env.close()


# ------------------------------------------------------------------------------------------------ 8. refusals
def test_refusals_leave_the_env_stepping(bk, oracle):
    import torch

    members = [(1, ("noise", 0, 8, NOISE)), (0, ("random", 8, *RND, 0.9))]
    # no device ingress
    env = bk.ManyMarketEnv(4, SEED, 0, [2, 2], STEP, max_live_orders=64, history_capacity=2)
    env.set_market_agents(members)
    with pytest.raises(bk.BourseError, match="bk_device_ingress_enable"):
        env.update_market_members()
    env.run(2)
    env.close()
    # nothing installed; an all-RandomAgents set: the message names the other entry
    env = market_env(bk, torch, 4, [2, 2], 4, 64, 128, 256)
    with pytest.raises(bk.BourseError, match="no MarketAgentSet"):
        env.update_market_members()
    env.step()
    env.set_market_agents([(0, ("random", 8, *RND, 0.9))])
    with pytest.raises(bk.BourseError, match="bk_update_market_agents"):
        env.update_market_members()
    env.step()
    # the book entry keeps its refusal of markets, word for word
    env.set_market_agents(members)
    with pytest.raises(bk.BourseError, match=r"bk_update_members runs an AgentSet on independent books \(assets == 1\)"):
        env.update_members()
    assert len(env.member_orders(1, 0)) == 0  # installed, not yet updated
    env.update_market_members()
    env.step()
    ref = many_markets(oracle, 4, [2, 2], members=members)
    ref.step()
    ref.step()
    ref.run(1)
    P.no_flags(env)
    check_markets(env, lambda m: (ref, m))
    # more than eight members are refused on a device-ingress env, more than four without it
    nine = [(0, ("noise", 100 * i, 2, NOISE)) for i in range(9)]
    with pytest.raises(bk.BourseError, match="at most 8 members"):
        env.set_market_agents(nine)
    env.close()
    env = bk.ManyMarketEnv(4, SEED, 0, [2, 2], STEP, max_live_orders=64, history_capacity=2)
    with pytest.raises(bk.BourseError, match="at most 4 members"):
        env.set_market_agents(nine[:5])
    env.close()
