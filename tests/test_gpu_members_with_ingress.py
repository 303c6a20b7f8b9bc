"""On-device Noise / Momentum members beside submitted instructions in one env (bk_update_members): `agents.update(env, rng)`
of an AgentSet (ref crates/step_sim/src/agents/noise_agent.rs:127-176, momentum_agent.rs:146-208, common.rs:56-75,
random_agent.rs:85-119) queues its placements and cancellations in the device-resident ingress queues with the book's own
RNG, next to the instructions of bk_submit_instructions_device, and the step trades all of it (env.rs:116-219).

Every book is checked field by field against one oracle.StepEnv(seed + b) + oracle.AgentSet(members) called in the same
order (the harness of tests/test_gpu_agents_with_ingress.py: level-2 history, trades, orders with their statuses, order keys,
the RNG state, one order_status), and env.member_orders(b, j) against the oracle member's `orders` vector.

So that no case passes on idle books, the oracle side is counted while it runs - from its orders, trades and order lists
alone - and the counts are asserted BEFORE the comparison: per Noise / Momentum member a cancellation queued by
cancel_live_orders, a limit order, a market order and a list entry dropped as not Active; more trades than books x steps; a
Momentum member's momentum (the recursion of momentum_agent.rs:152-158 over the oracle's mid prices) both above and below 0.
A Momentum member alone never starts on a book whose mid price stands still (m stays 0), so that set runs beside a thin
flow of submitted new orders; the other sets of the first test run alone."""
import ctypes as C

import numpy as np
import pytest

from members_ingress_cases import CASES, MOM, NOISE, member_set
from ingress_support import (MOD, SEED, STEP, WIDE_STEPS, BusyCounts, apply_oracle, check, ingress_env, submit, thin_flow,
                             wide_flow, wide_set, wide_trading)
from ingress_support import members_env as _make_env

pytestmark = pytest.mark.gpu
U64_MAX = 0xFFFFFFFFFFFFFFFF


@pytest.fixture(scope="module")
def bk():
    import bourse_amd

    return bourse_amd


def _member_ids(oracle, aset, j):
    """member j's `orders` vector (a RandomAgents member: its agents' held ids, u64::MAX = None)"""
    m = aset.members[j]
    if m[0] != "random":
        return aset.order_list(j)
    out = np.zeros(m[1], dtype=np.uint64)
    oracle.lib().orc_agents_held_ids(aset._a, j, out.ctypes.data_as(C.POINTER(C.c_uint64)))
    return out


class Run:
    """B oracle envs with one AgentSet each, and (env given) the device env driven by the same calls."""

    def __init__(self, oracle, members_of, B, tick, env=None, torch=None):
        self.oracle, self.env, self.torch, self.B, self.tick = oracle, env, torch, B, tick
        self.refs = [oracle.StepEnv(SEED + b, 0, tick, STEP) for b in range(B)]
        self.new_sets(members_of)
        self.steps = 0
        self.max_live = 0

    def new_sets(self, members_of):
        """fresh agents (NoiseAgent::new ...) on the running envs"""
        self.sets = [self.oracle.AgentSet(members_of(b)) for b in range(self.B)]
        self.traded = [j for j, m in enumerate(self.sets[0].members) if m[0] != "random"]
        self.busy = BusyCounts(self.sets[0].members)

    def _update_oracle(self, b):
        ref, aset = self.refs[b], self.sets[b]
        before = ref.book.orders_array()
        n0 = len(before)
        lists0 = {j: aset.order_list(j) for j in self.traded}
        mid = ref.book.mid_price()
        aset.update(ref)
        self.busy.note(b, aset.members, before["status"], n0, lists0, {j: aset.order_list(j) for j in self.traded},
                       ref.book.orders_array()[n0:], mid)

    def update(self):
        if self.env is not None:
            self.env.update_members(sync=False)
        for b in range(self.B):
            self._update_oracle(b)

    def submit(self, off, ins):
        if self.env is not None:
            submit(self.torch, self.env, off, ins)
        for b, r in enumerate(self.refs):
            apply_oracle(r, int(off[b]), int(off[b + 1]), ins)

    def trading(self, on):
        if self.env is not None:
            self.env.enable_trading() if on else self.env.disable_trading()
        for r in self.refs:
            r.enable_trading() if on else r.disable_trading()

    def step(self):
        if self.env is not None:
            self.env.step(sync=False)
        for r in self.refs:
            r.step()
            self.max_live = max(self.max_live, int((r.book.orders_array()["status"] == 1).sum()))
        self.steps += 1

    def assert_busy(self, momentum_signs=True):
        """the condition on the oracle side, before any comparison"""
        self.busy.assert_busy(momentum_signs)
        trades = sum(r.book.n_trades() for r in self.refs)
        assert trades > self.B * self.steps, (trades, self.B * self.steps)

    def check(self, books=None):
        check(self.env, self.refs, books)
        for b in (range(self.B) if books is None else books):
            for j in range(len(self.sets[b].members)):
                got, want = self.env.member_orders(b, j), _member_ids(self.oracle, self.sets[b], j)
                assert np.array_equal(got, want), (b, j, got, want)


def _external(rng, run, n0, n_max, tick):
    """tests/test_gpu_agents_with_ingress.py::_external's mix for every book - limit and market orders, cancellations and
    modifications of the ids the book had before this step (n0) - with half of the targets drawn from the members' current
    lists.  Returns (offsets, arrays, targets, targets taken from a list)."""
    B = run.B
    n_b = rng.integers(0, n_max + 1, size=B)
    off = np.zeros(B + 1, dtype=np.int64)
    off[1:] = np.cumsum(n_b)
    n = int(off[-1])
    action = rng.choice([1, 2, MOD], size=n, p=[0.55, 0.25, 0.2]).astype(np.uint32)
    bid = rng.integers(0, 2, size=n).astype(np.uint8)
    has_p, has_v = rng.integers(0, 2, size=n).astype(np.uint8), rng.integers(0, 2, size=n).astype(np.uint8)
    side = np.where(action == MOD, (has_p << 1) | (has_v << 2), bid).astype(np.uint8)
    vol = rng.integers(1, 40, size=n).astype(np.uint32)
    trader = rng.integers(5000, 6000, size=n).astype(np.uint32)
    price = (rng.integers(30, 68, size=n) * tick).astype(np.uint32)
    market = (action == 1) & (rng.random(n) < 0.15)
    price[market] = np.where(bid[market] == 1, 0xFFFFFFFF, 0)  # a market order: the extreme prices (tick 1)
    order_id = np.zeros(n, dtype=np.uint64)
    targets = listed = 0
    for b in range(B):
        n_orders = int(n0[b])
        held = np.concatenate([_member_ids(run.oracle, run.sets[b], j) for j in range(len(run.sets[b].members))])
        held = held[held < n_orders]
        for i in range(int(off[b]), int(off[b + 1])):
            if action[i] == 1:
                continue
            if n_orders == 0:
                action[i] = 0  # nothing to target yet: a no-op
                continue
            targets += 1
            if len(held) and rng.random() < 0.5:
                order_id[i] = held[rng.integers(0, len(held))]
                listed += 1
            else:
                order_id[i] = rng.integers(0, n_orders)
    return off, (action, side, vol, trader, price, order_id), targets, listed


# ------------------------------------------------------------------------------------------------ 1. the sets, every pool
def run_alone(oracle, case, which, env=None, torch=None):
    """case 1 on the oracle (and on `env`): T x { update; step }; the Momentum member alone beside a thin flow of orders"""
    B, T = case["books"], case["steps"]
    members = member_set(case["R"], which)
    run = Run(oracle, lambda b: members, B, 1, env, torch)
    rng = np.random.default_rng(100 + case["R"])
    for s in range(T):
        if which.startswith("mixed") and s < 2:  # the first step without trading: the RandomAgents' orders all rest
            run.trading(s == 1)
        run.update()
        if which == "momentum":
            run.submit(*thin_flow(rng, B, 4, 1))
        run.step()
    return run


@pytest.mark.parametrize("which", ["noise", "momentum", "mixed", "mixed_reversed"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_members_equal_the_oracle(bk, oracle, name, which):
    import torch

    case = CASES[name]
    assert which in case["sets"] and case["unreachable"] is None
    assert case["books"] >= 64 and case["steps"] >= 30
    members = member_set(case["R"], which)
    env = _make_env(bk, torch, case["books"], case["steps"], case["pool"], members, 1, n_ext=4)
    env.set_agents(members)
    run = run_alone(oracle, case, which, env, torch)
    run.assert_busy()
    if which.startswith("mixed") and case["R"] >= 2:  # a bug confined to the pool's upper registers cannot pass unseen
        assert run.max_live > 64 * (case["R"] - 1), run.max_live
    assert not env.flags().any()
    run.check()
    env.close()


# ------------------------------------------------------------------------------------------------ 2. beside instructions
def run_with_external(oracle, case, which, members_first, env=None, torch=None, NX=12):
    B, T = case["books"], case["steps"]
    members = member_set(case["R"], which)
    run = Run(oracle, lambda b: members, B, 1, env, torch)
    rng = np.random.default_rng(7 + members_first + 2 * case["R"])
    targets = listed = 0
    for _ in range(T):
        n0 = [r.book.n_orders() for r in run.refs]
        if members_first:
            run.update()
        off, ins, t, l = _external(rng, run, n0, NX, 1)
        run.submit(off, ins)
        targets, listed = targets + t, listed + l
        if not members_first:
            run.update()
        run.step()
    return run, targets, listed


@pytest.mark.parametrize("members_first", [True, False])
@pytest.mark.parametrize("which", ["noise", "momentum", "mixed", "mixed_reversed"])
@pytest.mark.parametrize("name", ["ingress::k_update_members<4>"])
def test_members_with_external_instructions_equal_the_oracle(bk, oracle, name, which, members_first):
    import torch

    case, NX = CASES[name], 12
    members = member_set(case["R"], which)
    env = _make_env(bk, torch, case["books"], case["steps"], case["pool"], members, 1, n_ext=NX)
    env.set_agents(members)
    run, targets, listed = run_with_external(oracle, case, which, members_first, env, torch, NX)
    run.assert_busy()
    assert targets > case["books"] * case["steps"] // 2 and 3 * listed >= targets, (targets, listed)
    assert not env.flags().any()
    run.check()
    env.close()


# ------------------------------------------------------------------------------------- 2b. members wider than a wave
@pytest.mark.parametrize("pool", [256, 512])
@pytest.mark.parametrize("which", ["noise", "momentum"])
def test_members_wider_than_a_wave_equal_the_oracle(bk, oracle, which, pool):
    """70 Noise traders who all place both orders (140 New events: place_new's flush inside the loop, twice) and 130
    Momentum traders at p_limit, p_market >= 1 (260), with lists of more than 128 Active ids (cancel_live_orders' second
    and third 64-entry pass, compacting in place): tests/ingress_support.py::wide_set.  The same runs are held to the
    model in tests/test_gpu_agents_model.py."""
    import torch

    B, T = 64, WIDE_STEPS
    members = wide_set(which)
    env = _make_env(bk, torch, B, T, pool, members, 1, n_ext=4)
    env.set_agents(members)
    run = Run(oracle, lambda b: members, B, 1, env, torch)
    for s in range(T):
        run.trading(wide_trading(which, s))
        run.update()
        run.submit(*wide_flow(which, pool, s, B, lambda b: run.sets[b].order_list(0)))
        run.step()
    run.assert_busy()
    assert run.busy.longest_list > 128 and run.busy.largest_batch == 2 * members[0][2], (run.busy.longest_list, run.busy.largest_batch)
    assert run.max_live < pool, run.max_live
    assert not env.flags().any()
    run.check()
    env.close()


# ------------------------------------------------------------------------------------------------ 3. the call orders
def test_update_then_submit_submit_then_update_and_two_updates_in_a_step(bk, oracle):
    import torch

    B, T, R, NX = 64, 18, 4, 5
    # (the orders of a step's first update are New at its second one: dropped from the lists and not held by the
    # RandomAgents, who place again - they stay on the books, unowned, so the set is small against the pool)
    members = [("random", 16, (32, 64), (10, 20), 2, 0.6), ("noise", 16, 10, NOISE), ("momentum", 26, 10, MOM)]
    env = _make_env(bk, torch, B, T, 64 * R, members, 1, n_ext=NX, updates=2)
    env.set_agents(members)
    run = Run(oracle, lambda b: members, B, 1, env, torch)
    rng = np.random.default_rng(23)
    for s in range(T):
        n0 = [r.book.n_orders() for r in run.refs]
        kind = s % 3
        if kind != 1:
            run.update()
        off, ins, _, _ = _external(rng, run, n0, NX, 1)
        run.submit(off, ins)
        if kind != 0:
            run.update()  # (kind 2: the second update of the step drops the first one's orders - New - from the lists)
        run.step()
    run.assert_busy(momentum_signs=False)
    assert not env.flags().any()
    run.check()
    env.close()


# ------------------------------------------------------------------------------------------------ 4. a per-book table
def test_a_per_book_table_equals_the_uniform_set_of_each_row(bk, oracle):
    import torch

    B, T, R = 64, 20, 2

    def row(b):
        r = np.random.default_rng(1000 + b)
        return [("noise", 100 * (b % 7), 12, dict(NOISE, p_limit=float(np.float32(r.uniform(0.1, 0.5))),
                                                  p_cancel=float(np.float32(r.uniform(0.05, 0.4))),
                                                  trade_vol=int(r.integers(10, 200)), price_dist_sigma=float(r.uniform(0.5, 3.0)))),
                ("random", 24, (int(r.integers(20, 40)), int(r.integers(50, 80))), (5, int(r.integers(10, 40))), 2,
                 float(np.float32(r.uniform(0.2, 0.9)))),
                ("momentum", 3000 + b, 8, dict(MOM, demand=float(r.uniform(2.0, 12.0)), decay=float(r.uniform(0.3, 1.0)),
                                               p_cancel=float(np.float32(r.uniform(0.05, 0.3)))))]

    table = [row(b) for b in range(B)]
    env = _make_env(bk, torch, B, T, 64 * R, table[0], 1)
    env.set_agents_per_book(table)
    run = Run(oracle, lambda b: table[b], B, 1, env, torch)
    uni_books = (3, B - 1)
    unis = []
    for b0 in uni_books:  # the uniform env given row b0: its book b0 is the table env's
        e = _make_env(bk, torch, B, T, 64 * R, table[b0], 1)
        e.set_agents(table[b0])
        unis.append(e)
    for _ in range(T):
        run.update()
        run.step()
        for e in unis:
            e.update_members(sync=False)
            e.step(sync=False)
    run.assert_busy(momentum_signs=False)
    assert not env.flags().any()
    run.check()
    hist = env.history()
    for b0, e in zip(uni_books, unis):
        e.sync()
        assert np.array_equal(e.history()[:, b0], hist[:, b0]), b0
        assert e.rng_state(b0) == env.rng_state(b0), b0
        for j in range(3):
            assert np.array_equal(e.member_orders(b0, j), env.member_orders(b0, j)), (b0, j)
        e.close()
    env.close()


# ------------------------------------------------------------------------------------------------ 5. capacity
def test_a_short_queue_and_an_off_tick_price_are_flagged(bk, oracle):
    import torch

    B = 16
    # 32 RandomAgents (about 29 place at their first update), then 64 events of a Noise member: the queue's 8 slots run out
    # inside the RandomAgents member
    members = [("random", 32, (32, 64), (10, 20), 2, 0.9), ("noise", 0, 32, dict(NOISE, p_limit=1.0, p_market=1.0))]
    for strict in (True, False):
        env = ingress_env(bk, torch, B, 2, 128, 0, 8, strict=strict, n_orders=256)
        env.set_agents(members)
        if strict:
            with pytest.raises(bk.CapacityError, match="EVENT_OVERFLOW"):
                env.update_members()
        else:
            env.update_members()
            assert (env.flags() & bk._lib.FLAG_EVENT_OVERFLOW).all()
            assert all(env.order_count(b) == 8 for b in range(B))  # a dropped New uses no id
            for b in range(B):
                assert len(env.member_orders(b, 1)) == 0  # ... and enters no list
            # the drop rule: a fresh env's first update (nobody holds an id, the lists are empty) takes the oracle's draws
            # whether an event fits or not, and queues exactly the first `room` placements, in agent order
            for b in range(B):
                ref, aset = oracle.StepEnv(SEED + b, 0, 2, STEP), oracle.AgentSet(members)
                aset.update(ref)
                held, want = _member_ids(oracle, aset, 0), ref.book.orders_array()
                assert int((held != U64_MAX).sum()) > 8, (b, held)  # the queue overflows inside the RandomAgents member
                assert env.rng_state(b) == tuple(int(x) for x in ref.rng_state()), b
                got = env.orders(b)
                for f in ("side", "price", "vol", "trader_id"):
                    assert np.array_equal(got[f], want[f][:8]), (b, f, got[f], want[f][:8])
                # ids 0 .. 7 with the oracle's first 8 placing agents, None with everybody else
                assert np.array_equal(env.member_orders(b, 0), np.where(held < 8, held, U64_MAX)), (b, held)
        env.step()
        env.close()
    # the same queue under a Noise member alone (64 events per update): it runs out inside the member's own loop, with a
    # partly filled batch in place_new / flush_new
    alone = [members[1]]
    env = ingress_env(bk, torch, B, 2, 128, 0, 8, strict=False, n_orders=256)
    env.set_agents(alone)
    env.update_members()
    assert (env.flags() & bk._lib.FLAG_EVENT_OVERFLOW).all()
    for b in range(B):
        ref, aset = oracle.StepEnv(SEED + b, 0, 2, STEP), oracle.AgentSet(alone)
        aset.update(ref)
        want, listed = ref.book.orders_array(), aset.order_list(0)
        assert len(want) > 8, (b, len(want))
        assert env.order_count(b) == 8, b  # a dropped New uses no id
        assert env.rng_state(b) == tuple(int(x) for x in ref.rng_state()), b
        got = env.orders(b)
        for f in ("side", "price", "vol", "trader_id"):
            assert np.array_equal(got[f], want[f][:8]), (b, f, got[f], want[f][:8])
        ids = env.member_orders(b, 0)
        assert 0 < len(ids) <= 8 and np.array_equal(ids, listed[listed < 8]), (b, ids, listed)  # ... and enters no list
    env.step()
    env.close()
    # every sell limit lands on the u32::MAX clamp, which the book's tick 2 does not divide (mixed_create's rule: flagged,
    # nothing created); the oracle creates nothing either, and everything else stays equal
    far = [("noise", 0, 16, dict(NOISE, p_limit=1.0, price_dist_mu=25.0, price_dist_sigma=0.0))]
    T = 6
    env = ingress_env(bk, torch, B, T, 128, 0, 64, strict=False, n_orders=64 * T)
    env.set_agents(far)
    run = Run(oracle, lambda b: far, B, 2, env, torch)
    for _ in range(T):
        run.update()
        run.step()
    env.sync()
    flags = env.flags()
    assert (flags & bk._lib.FLAG_PRICE_TICK).all() and not (flags & ~np.uint32(bk._lib.FLAG_PRICE_TICK)).any(), flags
    for b, r in enumerate(run.refs):
        o = r.book.orders_array()
        assert not ((o["side"] == 0) & (o["price"] != 0)).any(), b  # no sell limit order exists
        assert env.order_count(b) == len(o), b
    run.check()
    env.close()


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals_leave_the_env_stepping(bk, oracle):
    import torch

    B = 16
    members = [("noise", 0, 8, NOISE)]
    # no device ingress
    env = bk.ManyBookEnv(B, SEED, 0, 2, STEP, max_live_orders=64, history_capacity=2)
    env.set_agents(members)
    with pytest.raises(bk.BourseError, match="bk_device_ingress_enable"):
        env.update_members()
    env.run(2)
    env.close()
    # no AgentSet; RandomAgents groups only (bk_update_agents'); then members: bk_update_agents keeps its refusal
    env = ingress_env(bk, torch, B, 4, 64, 0, 64, n_orders=256)
    with pytest.raises(bk.BourseError, match="no AgentSet"):
        env.update_members()
    with pytest.raises(bk.BourseError, match="bk_member_orders"):
        env.member_orders(0, 0)
    env.step()
    env.set_random_agents([(16, (32, 64), (10, 20), 2, 0.9)])
    with pytest.raises(bk.BourseError, match="bk_update_agents"):
        env.update_members()
    env.step()
    env.set_agents(members)
    with pytest.raises(bk.BourseError, match="Noise / Momentum"):
        env.update_agents()
    assert len(env.member_orders(0, 0)) == 0  # installed, not yet updated
    with pytest.raises(bk.BourseError, match="member index"):
        env.member_orders(0, 1)
    env.update_members()
    env.step()
    with pytest.raises(bk.BourseError, match="bk_run cannot be mixed"):
        env.run(1)
    with pytest.raises(bk.BourseError):
        env.checkpoint()
    run = Run(oracle, lambda b: members, B, 2)
    for r in run.refs:
        r.step()
        r.step()
    run.update()
    run.step()
    run.env = env
    assert not env.flags().any()
    run.check()
    env.close()
    # markets (assets > 1)
    env = bk.ManyBookEnv(2 * B, SEED, 0, 2, STEP, max_live_orders=64, assets=2,
                         stream=torch.cuda.current_stream().cuda_stream)
    env.enable_device_ingress(32)
    env.set_market_agents([(0, ("noise", 0, 8, NOISE))])
    with pytest.raises(bk.BourseError, match="assets == 1"):
        env.update_members()
    env.step()
    env.close()


def test_one_install_replaces_the_other(bk, oracle):
    """bk_update_agents and bk_update_members never both run one env: bk_set_random_agents* clears the AgentSet
    (n_mixed), bk_set_agents* clears the groups"""
    import torch

    B = 8
    env = ingress_env(bk, torch, B, 8, 128, 0, 64, n_orders=512)
    groups, members = [(16, (32, 64), (10, 20), 2, 0.9)], [("random", 8, (32, 64), (10, 20), 2, 0.9), ("noise", 8, 8, NOISE)]
    for _ in range(2):
        env.set_random_agents(groups)
        env.update_agents()
        with pytest.raises(bk.BourseError, match="bk_update_agents"):
            env.update_members()
        env.step()
        env.set_agents(members)
        env.update_members()
        with pytest.raises(bk.BourseError, match="Noise / Momentum"):
            env.update_agents()
        env.step()
    # an all-RandomAgents AgentSet is bk_set_random_agents': it stays with bk_update_agents
    env.set_agents([("random", 8, (32, 64), (10, 20), 2, 0.9)])
    with pytest.raises(bk.BourseError, match="bk_update_agents"):
        env.update_members()
    env.update_agents()
    env.step()
    assert not env.flags().any()
    env.close()


# ------------------------------------------------------------------------------------------------ 7. reinstall
def test_reinstalled_members_forget_their_orders_and_their_momentum(bk, oracle):
    import torch

    B, T, R = 64, 24, 2
    first = member_set(R, "mixed")
    second = [("momentum", 900, 12, dict(MOM, demand=8.0)), ("noise", 950, 16, dict(NOISE, p_cancel=0.3)),
              ("random", 40, (30, 66), (5, 25), 2, 0.5)]
    env = _make_env(bk, torch, B, T, 64 * R, first, 1)
    env.set_agents(first)
    run = Run(oracle, lambda b: first, B, 1, env, torch)
    for s in range(T):
        if s == 10:  # NoiseAgent::new / MomentumAgent::new / RandomAgents::new: the old orders stay on the books, unowned
            assert any(len(env.member_orders(b, 1)) for b in range(B))
            env.set_agents(second)
            run.new_sets(lambda b: second)
            for b in range(B):
                assert len(env.member_orders(b, 0)) == 0 and len(env.member_orders(b, 1)) == 0
                assert (env.member_orders(b, 2) == U64_MAX).all()
        run.update()
        run.step()
    run.assert_busy(momentum_signs=False)
    assert not env.flags().any()
    run.check()
    env.close()
