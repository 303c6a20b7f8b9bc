"""The open-order view of a device-ingress env (bk_open_orders_enable; bourse_amd/csrc/open_orders.hpp): per book and trader
a summary row {bid_vol, ask_vol, n_bid, n_ask, best_bid, best_ask} and the `depth` oldest resting orders, recomputed on the
device from the pool behind every step and every reset.

The expected side never shares code with the kernel: tests/open_orders_model.py::rows (plain Python) over the orders of one
oracle.StepEnv(SEED + b) per book (one oracle.ManyMarkets(1, SEED + m) per market) that is given the same calls as the device
env; case 1's rows are literal numbers worked out by hand.  The expected side runs FIRST (a Plan: the flows and the rows after
every step), because a flow's cancellations and modifications name ids that rest on it.  Where a case says something only
under a condition - a trader beyond depth, an empty trader, a partially filled resting order, a resting trader without a
row, an idle book-step, pools filled beyond their first registers - the condition is counted on the expected side and
asserted before anything is compared."""

import ctypes

import numpy as np
import pytest

import accounts_model as AM
import open_orders_model as OM
import oracle_parity as P
from ingress_support import MOD, SEED, STEP, apply_oracle, ingress_env, members_env, submit
from members_ingress_cases import NOISE

pytestmark = pytest.mark.gpu
ORDER_LOG_FULL = 8
BK_INVALID_ARGUMENT = 5
NONE = (0xFFFFFFFF, 0, 0, 0)


@pytest.fixture(scope="module")
def bk():
    import bourse_amd

    return bourse_amd


def same_rows(got, want, tag):
    """(summary, entries) of some books against the model's, field by field"""
    (gs, ge), (ws, we) = got, want
    assert gs.dtype == ws.dtype == OM.OPEN_SUMMARY_DTYPE, (gs.dtype, ws.dtype)
    assert gs.shape == ws.shape, f"{tag}: summary rows {gs.shape} vs {ws.shape}"
    for f in ws.dtype.names:
        P.same_array(gs[f], ws[f], tag, f"summary field {f}")
    if we is None or we.shape[-1] == 0:
        assert ge is None, f"{tag}: entries without depth"
        return
    assert ge.dtype == we.dtype == OM.OPEN_ORDER_DTYPE and ge.shape == we.shape, f"{tag}: entries {ge.shape} vs {we.shape}"
    for f in we.dtype.names:
        P.same_array(ge[f], we[f], tag, f"entry field {f}")


def model_rows(views, n_traders, depth, max_orders=None):
    """the model over one oracle book view per book, stacked as env.open_orders() returns them"""
    rows = [OM.rows(v.orders_array(), n_traders, depth, max_orders) for v in views]
    return np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])


def pick(rows, books):
    return rows[0][books], (None if rows[1] is None else rows[1][books])


def instructions(per_book):
    """(offsets, arrays) in submit's / apply_oracle's format from per-book lists of (action, side, vol, trader, price, id)"""
    off = np.zeros(len(per_book) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(x) for x in per_book])
    flat = [r for rs in per_book for r in rs]
    col = lambda k, dt: np.array([r[k] for r in flat], dtype=dt)
    return off, (col(0, np.uint32), col(1, np.uint8), col(2, np.uint32), col(3, np.uint32), col(4, np.uint32), col(5, np.uint64))


def new(bid, vol, trader, price):
    return (1, int(bid), int(vol), int(trader), int(price), 0)


def flow(rng, refs, tick, n_new, traders, idle=(), p_cancel=0.3, n_mod=3, trader_of=None):
    """One step of a busy flow for every book: n_new[b] new limit orders (side uniform, a bid's price U{40..51} x tick and
    an ask's U{49..60} x tick - most rest, the overlap trades - volume U{1..5} or, with probability 0.2, U{50..199}, trader
    drawn from `traders`), then cancellations of about p_cancel of that many of the orders that rest on the expected side
    now, and n_mod modifications (price, volume or both) of others; the books in `idle` get nothing."""
    per_book = []
    for b, r in enumerate(refs):
        rows = []
        if b not in idle:
            n = int(n_new[b])
            for _ in range(n):
                vol = int(rng.integers(50, 200)) if rng.random() < 0.2 else int(rng.integers(1, 6))
                t = int(rng.choice(traders))
                bid = int(rng.integers(0, 2))
                rows.append(new(bid, vol, trader_of(b, t) if trader_of else t, int(rng.integers(40, 52) + 9 * (1 - bid)) * tick))
            o = r.book.orders_array()
            live = rng.permutation(o["order_id"][o["status"] == 1])
            n_c = min(len(live), int(round(p_cancel * n)))
            rows += [(2, 0, 0, 0, 0, int(i)) for i in live[:n_c]]
            for k, i in enumerate(live[n_c:n_c + n_mod]):
                has = (2, 4, 6)[k % 3]  # a new price, a new volume, both
                rows.append((MOD, has, int(rng.integers(1, 30)), 0, int(rng.integers(45, 56)) * tick, int(i)))
            rows = [rows[i] for i in rng.permutation(len(rows))]
        per_book.append(rows)
    return instructions(per_book)


class Plan:
    """The expected side of a run, made before the device sees anything: one oracle StepEnv per book, every step's
    instructions and the model's rows after it, and the conditions the rows were met under."""

    def __init__(self, oracle, B, tick, n_traders, depth, max_orders=None):
        self.B, self.tick, self.NT, self.depth, self.max_orders = B, tick, n_traders, depth, max_orders
        self.refs = [oracle.StepEnv(SEED + b, 0, tick, STEP) for b in range(B)]
        self.steps = []  # (offsets, arrays, rows after the step)
        self.beyond_depth = self.empty = self.partial = self.skipped = self.idle = self.most_live = 0

    def rows(self, books=None):
        views = [self.refs[b].book for b in (range(self.B) if books is None else books)]
        return model_rows(views, self.NT, self.depth, self.max_orders)

    def step(self, off, ins):
        for b, r in enumerate(self.refs):
            apply_oracle(r, int(off[b]), int(off[b + 1]), ins)
            r.step()
            self.idle += off[b] == off[b + 1]
        want = self.rows()
        self.steps.append((off, ins, want))
        n = want[0]["n_bid"].astype(np.int64) + want[0]["n_ask"]
        self.beyond_depth += int((n > self.depth).sum())
        self.empty += int((n == 0).sum())
        for r in self.refs:
            o, t = r.book.orders_array(), r.book.trades_array()
            active = o["status"] == 1
            hit = np.zeros(len(o), dtype=bool)
            hit[t["passive_id"].astype(np.int64)] = True
            self.partial += int((active & hit & (o["trader_id"] < self.NT)).sum())
            self.skipped += int((active & (o["trader_id"] >= self.NT)).sum())
            self.most_live = max(self.most_live, int(active.sum()))
        return want


def run_plan(torch, env, plan, tag, after=None):
    """the plan's steps on the device, its rows compared after every one"""
    for s, (off, ins, want) in enumerate(plan.steps):
        submit(torch, env, off, ins)
        env.step(sync=False)
        same_rows(env.open_orders(), want, f"{tag}: after step {s}")
        if after:
            after(s)


# ------------------------------------------------------------------------------------------------ 1. by hand
HAND_STAGES = [
    # s0  rests: trader 0 bids 10 @ 100 (id 0) and 5 @ 99 (id 2), trader 1 asks 8 @ 105 (id 1)
    ([new(1, 10, 0, 100), new(0, 8, 1, 105), new(1, 5, 0, 99)],
     [(15, 0, 2, 0, 100, 0xFFFFFFFF), (0, 8, 0, 1, 0, 105), (0, 0, 0, 0, 0, 0xFFFFFFFF)],
     [[(0, 100, 10, 1), (2, 99, 5, 1)], [(1, 105, 8, 0), NONE], [NONE, NONE]]),
    # s1  a partial fill: trader 2 sells 4 @ 100 (id 3) into id 0, which keeps 6
    ([new(0, 4, 2, 100)],
     [(11, 0, 2, 0, 100, 0xFFFFFFFF), (0, 8, 0, 1, 0, 105), (0, 0, 0, 0, 0, 0xFFFFFFFF)],
     [[(0, 100, 6, 1), (2, 99, 5, 1)], [(1, 105, 8, 0), NONE], [NONE, NONE]]),
    # s2  a full fill: trader 2 sells 6 @ 100 (id 4), id 0 is gone
    ([new(0, 6, 2, 100)],
     [(5, 0, 1, 0, 99, 0xFFFFFFFF), (0, 8, 0, 1, 0, 105), (0, 0, 0, 0, 0, 0xFFFFFFFF)],
     [[(2, 99, 5, 1), NONE], [(1, 105, 8, 0), NONE], [NONE, NONE]]),
    # s3  a cancel: id 1
    ([(2, 0, 0, 0, 0, 1)],
     [(5, 0, 1, 0, 99, 0xFFFFFFFF), (0, 0, 0, 0, 0, 0xFFFFFFFF), (0, 0, 0, 0, 0, 0xFFFFFFFF)],
     [[(2, 99, 5, 1), NONE], [NONE, NONE], [NONE, NONE]]),
    # s4  a modify of price: id 2 to 98
    ([(MOD, 2, 0, 0, 98, 2)],
     [(5, 0, 1, 0, 98, 0xFFFFFFFF), (0, 0, 0, 0, 0, 0xFFFFFFFF), (0, 0, 0, 0, 0, 0xFFFFFFFF)],
     [[(2, 98, 5, 1), NONE], [NONE, NONE], [NONE, NONE]]),
    # s5  a modify of volume: id 2 to 3
    ([(MOD, 4, 3, 0, 0, 2)],
     [(3, 0, 1, 0, 98, 0xFFFFFFFF), (0, 0, 0, 0, 0, 0xFFFFFFFF), (0, 0, 0, 0, 0, 0xFFFFFFFF)],
     [[(2, 98, 3, 1), NONE], [NONE, NONE], [NONE, NONE]]),
    # s6  a trader on both sides: trader 0 asks 7 @ 110 (id 5)
    ([new(0, 7, 0, 110)],
     [(3, 7, 1, 1, 98, 110), (0, 0, 0, 0, 0, 0xFFFFFFFF), (0, 0, 0, 0, 0, 0xFFFFFFFF)],
     [[(2, 98, 3, 1), (5, 110, 7, 0)], [NONE, NONE], [NONE, NONE]]),
    # s7  depth = 2 and trader 0 rests three: bid 1 @ 97 (id 6) is counted and summed, the oldest two are listed
    ([new(1, 1, 0, 97)],
     [(4, 7, 2, 1, 98, 110), (0, 0, 0, 0, 0, 0xFFFFFFFF), (0, 0, 0, 0, 0, 0xFFFFFFFF)],
     [[(2, 98, 3, 1), (5, 110, 7, 0)], [NONE, NONE], [NONE, NONE]]),
]


def hand_rows(summary, entries):
    """the literal rows of book 0 and the empty rows of book 1 as (summary[2, 3], entries[2, 3, 2])"""
    s = np.array([summary, [OM.EMPTY_SUMMARY] * 3], dtype=OM.OPEN_SUMMARY_DTYPE)
    e = np.zeros((2, 3, 2), dtype=OM.OPEN_ORDER_DTYPE)
    for t in range(3):
        for k in range(2):
            e[0, t, k], e[1, t, k] = entries[t][k], NONE
    return s, e


def test_rows_worked_out_by_hand(bk, oracle):
    """Two books with tick 1, n_traders = 3, depth = 2.  Book 1 is never touched: its rows stay empty.  Book 0 goes through
    HAND_STAGES, one step each (a step shuffles its events, so no stage depends on the order inside one); rows and entries
    are literal numbers, compared after every stage - and the model over the oracle's book gives the same."""
    import torch

    env = ingress_env(bk, torch, 2, len(HAND_STAGES), 64, 0, 8, tick=1, n_orders=32)
    env.enable_open_orders(3, 2)
    same_rows(env.open_orders(), hand_rows([OM.EMPTY_SUMMARY] * 3, [[NONE, NONE]] * 3), "at enable")
    plan = Plan(oracle, 2, 1, 3, 2)
    for s, (rows, summary, entries) in enumerate(HAND_STAGES):
        off, ins = instructions([rows, []])
        same_rows(plan.step(off, ins), hand_rows(summary, entries), f"the model over the oracle's book, stage {s}")
        submit(torch, env, off, ins)
        env.step(sync=False)
        same_rows(env.open_orders(), hand_rows(summary, entries), f"stage {s}")
    P.no_flags(env)
    want = hand_rows(*HAND_STAGES[-1][1:])
    same_rows(env.open_orders(1, 1), pick(want, slice(1, 2)), "open_orders(first_book, n_books)")
    env.refresh_open_orders()  # (nothing changed a pool: the same rows)
    same_rows(env.open_orders(), want, "after refresh_open_orders")
    env.close()


# ------------------------------------------------------------------------------------------------ 2. after every step
def busy_plan(oracle, pool, B=5, T=4, NT=7, depth=4, seed=7):
    """B = 5 books (the last block of 4 waves partly empty) of `pool` slots: every step about 2/7 of the pool in new orders per book
    of traders 0..8 (7 and 8 have no row; trader 6 never trades in books 3 and 4), 30 % cancels and three modifies; book 4
    idles in the odd steps."""
    tick = 2
    plan = Plan(oracle, B, tick, NT, depth)
    rng = np.random.default_rng(seed + pool)
    for s in range(T):
        n_new = rng.integers(2 * pool // 7 - 3, 2 * pool // 7 + 4, size=B)
        plan.step(*flow(rng, plan.refs, tick, n_new, np.arange(9), idle=(4,) if s % 2 else (),
                        trader_of=lambda b, t: 5 if (t == 6 and b >= 3) else t))
    return plan


@pytest.mark.parametrize("pool", [64, 128, 256, 512])
def test_rows_equal_the_model_after_every_step_of_a_busy_flow(bk, oracle, pool):
    import torch

    plan = busy_plan(oracle, pool)
    assert plan.beyond_depth > 0 and plan.empty > 0 and plan.partial > 0 and plan.skipped > 0 and plan.idle > 0, vars(plan)
    # the pool is used beyond its first half (every register of a 128 / 256-slot pool, five of eight at 512) and never full
    assert pool // 2 < plan.most_live < pool, (plan.most_live, pool)
    qcap = max(len(ins[0]) for _, ins, _ in plan.steps)
    env = ingress_env(bk, torch, plan.B, len(plan.steps), pool, 0, qcap, tick=plan.tick, n_ext=qcap)
    env.enable_open_orders(plan.NT, plan.depth)
    run_plan(torch, env, plan, f"pool {pool}")
    P.no_flags(env)
    for b in range(plan.B):
        P.same_live(env, b, plan.refs[b].book)
    env.close()


# ------------------------------------------------------------------------------------------------ 3. more than 64 traders
def wide_plan(oracle, NT=70, depth=2):
    plan = Plan(oracle, 3, 2, NT, depth)
    rng = np.random.default_rng(31)
    for s in range(3):
        plan.step(*flow(rng, plan.refs, 2, [40, 36, 30], np.arange(76), n_mod=2))
    return plan


def test_more_traders_than_a_wave_has_lanes(bk, oracle):
    """n_traders = 70 at a 128-slot pool: the kernel takes the traders 64 at a time, and the second chunk holds six rows."""
    import torch

    plan = wide_plan(oracle)
    s, _ = plan.steps[-1][2]
    resting = (s["n_bid"] + s["n_ask"]) > 0
    assert resting[:, :64].any() and resting[:, 64:].any() and (~resting[:, 64:]).any(), "both chunks, used and empty"
    assert resting.sum(axis=1).max() > 40 and plan.skipped > 0 and 64 < plan.most_live < 128, vars(plan)
    qcap = max(len(ins[0]) for _, ins, _ in plan.steps)
    env = ingress_env(bk, torch, plan.B, len(plan.steps), 128, 0, qcap, tick=plan.tick, n_ext=qcap)
    env.enable_open_orders(plan.NT, plan.depth)
    run_plan(torch, env, plan, "70 traders")
    P.no_flags(env)
    env.close()


# ------------------------------------------------------------------------------------------------ 4. depth = 0
def test_depth_zero_keeps_the_summaries_only(bk, oracle):
    import torch

    plan = busy_plan(oracle, 128, T=2, depth=0)
    assert plan.beyond_depth > 0 and plan.empty > 0
    qcap = max(len(ins[0]) for _, ins, _ in plan.steps)
    env = ingress_env(bk, torch, plan.B, len(plan.steps), 128, 0, qcap, tick=plan.tick, n_ext=qcap)
    env.enable_open_orders(plan.NT, 0)
    summary_ptr, entries_ptr = env.open_orders_device_ptrs()
    assert summary_ptr and entries_ptr is None
    views = env.open_orders_views()
    assert views[1] is None and views[0].__cuda_array_interface__["shape"] == (plan.B, plan.NT, 4)
    run_plan(torch, env, plan, "depth 0")
    got = env.open_orders()
    assert got[1] is None and got[0]["n_bid"].any()
    P.no_flags(env)
    env.close()


# ------------------------------------------------------------------------------------------------ 5. members in the loop
def external(rng, B, n_max, traders):
    """a few limit orders of the strategy's traders around the members' prices"""
    per_book = []
    for _ in range(B):
        per_book.append([new(rng.integers(0, 2), rng.integers(20, 200), rng.choice(traders), rng.integers(40, 60))
                         for _ in range(int(rng.integers(1, n_max + 1)))])
    return instructions(per_book)


@pytest.mark.parametrize("kind", ["members", "random"])
def test_members_and_agents_in_the_loop(bk, oracle, kind):
    """members: Noise members with agent_id_start = 1000 >= n_traders through update_members - the strategy's rows
    (traders 40..47) equal the model and the members' resting orders appear nowhere.  random: RandomAgents through
    update_agents, whose trader ids are the agents' indices 0..29 - below n_traders, so they DO appear, in rows 0..29, and
    the model, which reads the oracle's trader ids, says the same."""
    import torch

    B, T, NT, NX, depth = 3, 6, 64, 6, 3
    if kind == "members":
        members = [("noise", 1000, 30, dict(NOISE, p_limit=0.5, p_market=0.3))]
        env = members_env(bk, torch, B, T, 128, members, 1, n_ext=NX)
        env.set_agents(members)
        sets = [oracle.AgentSet(members) for _ in range(B)]
        update = env.update_members
    else:
        groups = [(30, (40, 60), (10, 40), 1, 0.8)]
        env = ingress_env(bk, torch, B, T, 128, 30, 30 + NX, tick=1, n_ext=NX)
        env.set_random_agents(groups)
        sets = [oracle.RandomAgentSet(groups) for _ in range(B)]
        update = env.update_agents
    env.enable_open_orders(NT, depth)
    refs = [oracle.StepEnv(SEED + b, 0, 1, STEP) for b in range(B)]
    rng = np.random.default_rng(3)
    got, want = [], []
    for _ in range(T):
        update(sync=False)
        off, ins = external(rng, B, NX, np.arange(40, 48))
        submit(torch, env, off, ins)
        env.step(sync=False)
        for b in range(B):
            sets[b].update(refs[b])
            apply_oracle(refs[b], int(off[b]), int(off[b + 1]), ins)
            refs[b].step()
        got.append(env.open_orders())
        want.append(model_rows([r.book for r in refs], NT, depth))
    s = want[-1][0]
    n = s["n_bid"].astype(np.int64) + s["n_ask"]
    assert n[:, 40:48].any(), "no resting order of the strategy's traders"
    active = [r.book.orders_array() for r in refs]
    active = [o[o["status"] == 1] for o in active]
    if kind == "members":
        assert all((o["trader_id"] >= 1000).any() for o in active), "no resting order of a member"
        assert not n[:, :40].any() and not n[:, 48:].any()
        assert [int(x) for x in n.sum(axis=1)] == [int((o["trader_id"] < NT).sum()) for o in active]
    else:
        assert n[:, :30].any(), "no resting order of an agent"
    P.no_flags(env)
    for s, (g, w) in enumerate(zip(got, want)):
        same_rows(g, w, f"{kind}: after step {s}")
    env.close()


# ------------------------------------------------------------------------------------------------ 6. beyond max_orders
def test_a_resting_order_beyond_max_orders_is_left_out_and_flagged(bk, oracle):
    """max_orders = 8.  Book 0 gets 12 bids that all come to rest (ids 0..11): ids 8..11 have no record to look the trader up
    in, are left out of the rows, and the event kernel has set ORDER_LOG_FULL on book 0 - on that book only; book 1 (6 orders)
    is exact."""
    import torch

    B, NT, depth, MAXO = 2, 4, 8, 8
    plan = Plan(oracle, B, 1, NT, depth, max_orders=MAXO)
    plan.step(*instructions([[new(1, 3 + i, i % 3, 90 + i) for i in range(12)], [new(i % 2, 2 + i, i % 4, 100 + 10 * (i % 2)) for i in range(6)]]))
    o0 = plan.refs[0].book.orders_array()
    assert ((o0["status"] == 1) & (o0["order_id"] >= MAXO)).sum() == 4 and (o0["status"] == 1).sum() == 12
    full = OM.rows(o0, NT, depth)
    assert full[0].tolist() != plan.steps[0][2][0][0].tolist(), "the ids beyond max_orders change no row"
    env = bk.ManyBookEnv(B, SEED, 0, 1, STEP, levels=10, max_live_orders=64, max_orders=MAXO, trade_capacity=64,
                         history_capacity=2, strict=False, stream=torch.cuda.current_stream().cuda_stream)
    env.enable_device_ingress(queue_capacity=16)
    env.enable_open_orders(NT, depth)
    run_plan(torch, env, plan, "beyond max_orders")
    flags = env.flags()
    assert flags[0] == ORDER_LOG_FULL and flags[1] == 0, flags
    env.close()


# ------------------------------------------------------------------------------------------------ 7. reset
def only_new(rng, B, tick, n_lo, n_hi):
    n_b = rng.integers(n_lo, n_hi + 1, size=B)
    return instructions([[new(rng.integers(0, 2), rng.integers(1, 30), rng.integers(0, 7), int(rng.integers(45, 56)) * tick)
                          for _ in range(int(n))] for n in n_b])


def test_reset_books_show_the_snapshots_orders_at_once(bk, oracle):
    """3 steps, save, 3 steps, reset books 0 and 2 from a device mask with no step in between: the masked books show the
    model's rows AT THE SNAPSHOT, the others their current rows.  Then 2 more steps: the oracle cannot be rewound, so a reset
    book's expected side is a REPLAY - a fresh oracle env given steps 0..2 and then the two steps after the reset."""
    import torch

    B, tick, NT, depth = 4, 2, 5, 3
    flows = [only_new(np.random.default_rng(60 + s), B, tick, 12, 20) for s in range(8)]
    plan = Plan(oracle, B, tick, NT, depth)
    for f in flows[:3]:
        plan.step(*f)
    at_snapshot = plan.steps[-1][2]
    for f in flows[3:6]:
        plan.step(*f)
    current = plan.steps[-1][2]
    replay = Plan(oracle, B, tick, NT, depth)
    for f in flows[:3] + flows[6:]:
        replay.step(*f)
    for f in flows[6:]:
        plan.step(*f)
    mask = np.array([1, 0, 1, 0], dtype=bool)
    for b in np.flatnonzero(mask):
        assert at_snapshot[0][b].tolist() != current[0][b].tolist() and plan.skipped > 0

    env = ingress_env(bk, torch, B, 8, 256, 0, 32, tick=tick, n_ext=20)
    env.enable_open_orders(NT, depth)
    for s, (off, ins, want) in enumerate(plan.steps[:6]):
        submit(torch, env, off, ins)
        env.step(sync=False)
        if s == 2:
            env.save_ingress_snapshot()
    same_rows(env.open_orders(), current, "before the reset")
    env.reset_ingress_books(torch.tensor(mask, device="cuda"), sync=False)
    now = env.open_orders()
    same_rows(pick(now, mask), pick(at_snapshot, mask), "masked books: the snapshot's resting orders")
    same_rows(pick(now, ~mask), pick(current, ~mask), "unmasked books: their current rows")
    for s in (6, 7):
        off, ins, want = plan.steps[s]
        submit(torch, env, off, ins)
        env.step(sync=False)
        got = env.open_orders()
        same_rows(pick(got, ~mask), pick(want, ~mask), f"never reset, step {s}")
        same_rows(pick(got, mask), pick(replay.steps[s - 3][2], mask), f"reset: the replayed book, step {s}")
    P.no_flags(env)
    for b in range(B):
        P.same_live(env, b, (replay if mask[b] else plan).refs[b].book)
    env.close()


# ------------------------------------------------------------------------------------------------ 8. enable mid-run
def test_enabled_mid_run_the_table_is_right_at_once(bk, oracle):
    """Enabled after three steps and while an ingress snapshot slot is held: right before the next step, and after it."""
    import torch

    plan = busy_plan(oracle, 128, B=3, T=4, seed=11)
    qcap = max(len(ins[0]) for _, ins, _ in plan.steps)
    env = ingress_env(bk, torch, plan.B, 4, 128, 0, qcap, tick=plan.tick, n_ext=qcap)
    for off, ins, _ in plan.steps[:3]:
        submit(torch, env, off, ins)
        env.step(sync=False)
    env.save_ingress_snapshot()
    env.enable_open_orders(plan.NT, plan.depth)
    assert plan.steps[2][2][0]["n_bid"].any()
    same_rows(env.open_orders(), plan.steps[2][2], "right after enable")
    off, ins, want = plan.steps[3]
    submit(torch, env, off, ins)
    env.step(sync=False)
    same_rows(env.open_orders(), want, "after the next step")
    P.no_flags(env)
    env.close()


# ------------------------------------------------------------------------------------------------ 9. with accounts
def test_accounts_and_open_orders_on_one_env(bk, oracle):
    import torch

    plan = busy_plan(oracle, 128, B=3, T=3, seed=13)
    qcap = max(len(ins[0]) for _, ins, _ in plan.steps)
    env = ingress_env(bk, torch, plan.B, 3, 128, 0, qcap, tick=plan.tick, n_ext=qcap)
    env.enable_open_orders(plan.NT, plan.depth)
    env.enable_accounts(plan.NT)
    run_plan(torch, env, plan, "with accounts")
    P.no_flags(env)
    want = np.stack([AM.fold(r.book.trades_array(), r.book.orders_array(), plan.NT) for r in plan.refs])
    assert want["fills"].any()
    got = env.accounts()
    for f in want.dtype.names:
        P.same_array(got[f], want[f], "accounts beside open orders", f)
    env.close()


# ------------------------------------------------------------------------------------------------ 10. markets
def test_markets_keep_rows_per_book(bk, oracle):
    import torch

    NM, A, T, NT, depth, TICKS = 2, 2, 4, 4, 3, [1, 2]
    env = bk.ManyMarketEnv(NM, SEED, 0, TICKS, STEP, levels=10, max_live_orders=128, max_orders=256, trade_capacity=512,
                           history_capacity=T, stream=torch.cuda.current_stream().cuda_stream)
    env.enable_device_ingress(64)
    env.enable_open_orders(NT, depth)
    refs = [oracle.ManyMarkets(1, SEED + m, 0, TICKS, STEP, True, 10) for m in range(NM)]
    rng = np.random.default_rng(17)
    views = [refs[b // A].book(0, b % A) for b in range(NM * A)]
    for s in range(T):
        n_b = rng.integers(8, 16, size=NM * A)
        off, ins = instructions([[new(rng.integers(0, 2), rng.integers(1, 30), rng.integers(0, 6), int(rng.integers(48, 53)) * 2)
                                  for _ in range(int(n))] for n in n_b])
        submit(torch, env, off, ins)
        for b in range(NM * A):
            for i in range(int(off[b]), int(off[b + 1])):
                refs[b // A].place_order(0, b % A, bool(ins[1][i]), int(ins[2][i]), int(ins[3][i]), price=int(ins[4][i]))
        env.step(sync=False)
        for r in refs:
            r.step()
        want = model_rows(views, NT, depth)
        assert ((want[0]["n_bid"] + want[0]["n_ask"]) > 0).any(axis=1).all(), "a book without a resting order"
        same_rows(env.open_orders(), want, f"markets: after step {s}")
    P.no_flags(env)
    assert env.open_orders()[0].shape == (NM * A, NT)
    env.close()


# ------------------------------------------------------------------------------------------------ 11. the device views
def split_summary(a):
    """the summary view's int64 [.., 4] as the six fields"""
    u = a.astype(np.int64).view(np.uint64)
    return {"bid_vol": u[..., 0], "ask_vol": u[..., 1], "n_bid": u[..., 2] & 0xFFFFFFFF, "n_ask": u[..., 2] >> 32,
            "best_bid": u[..., 3] & 0xFFFFFFFF, "best_ask": u[..., 3] >> 32}


def test_the_device_views_are_the_tables_in_place(bk, oracle):
    import torch

    plan = busy_plan(oracle, 128, B=3, T=2, seed=19)
    B, NT, depth = plan.B, plan.NT, plan.depth
    qcap = max(len(ins[0]) for _, ins, _ in plan.steps)
    env = ingress_env(bk, torch, B, 2, 128, 0, qcap, tick=plan.tick, n_ext=qcap)
    env.enable_open_orders(NT, depth)
    sv, ev = env.open_orders_views()
    stream = torch.cuda.current_stream().cuda_stream
    for view, shape, typestr in ((sv, (B, NT, 4), "<i8"), (ev, (B, NT, depth, 4), "<i4")):
        cai = view.__cuda_array_interface__
        assert cai["shape"] == shape and cai["typestr"] == typestr and cai["version"] == 3 and cai["strides"] is None
        assert cai["stream"] == (stream if stream else 1)
    ts, te = torch.as_tensor(sv, device="cuda"), torch.as_tensor(ev, device="cuda")
    assert ts.dtype == torch.int64 and te.dtype == torch.int32 and ts.is_contiguous() and te.is_contiguous()
    assert env.open_orders_device_ptrs() == (ts.data_ptr(), te.data_ptr())

    def check_views(tag):
        env.sync()
        summary, entries = env.open_orders()
        fields = split_summary(ts.cpu().numpy())
        for f in summary.dtype.names:
            P.same_array(fields[f], summary[f].astype(np.uint64), tag, f"summary view, {f}")
        e = te.cpu().numpy().view(np.uint32)
        for k, f in enumerate(entries.dtype.names):
            P.same_array(e[..., k], entries[f], tag, f"entries view, {f}")
        return summary, entries

    off, ins, want = plan.steps[0]
    submit(torch, env, off, ins)
    env.step(sync=False)
    first = ts.clone()  # queued on the same stream, behind the refresh
    same_rows(check_views("after step 0"), want, "views, step 0")
    off, ins, want = plan.steps[1]
    submit(torch, env, off, ins)
    env.step(sync=False)
    same_rows(check_views("after step 1"), want, "views, step 1")  # the same tensors, no new call
    assert not torch.equal(first, ts), "the view did not change with the step"
    env.close()


# ------------------------------------------------------------------------------------------------ 12. refusals
def _refused(bk, call, match):
    with pytest.raises(bk.BourseError, match=match) as e:
        call()
    assert e.value.code == BK_INVALID_ARGUMENT


def _one_order_and_a_step(torch, env, B):
    submit(torch, env, *instructions([[new(1, 2, 0, 100)]] * B))
    env.step()


def test_refusals_leave_the_env_working(bk, oracle):
    import torch

    B = 2
    stream = torch.cuda.current_stream().cuda_stream
    # without the device ingress (a host-driven env)
    env = bk.ManyBookEnv(B, SEED, 0, 1, STEP, max_live_orders=64, max_orders=64, stream=stream)
    _refused(bk, lambda: env.enable_open_orders(4), "device ingress")
    env.place_order(0, True, 5, 1, price=100)
    env.step()
    assert env.order_count(0) == 1
    env.close()
    # max_orders = 0
    env = bk.ManyBookEnv(B, SEED, 0, 1, STEP, max_live_orders=64, max_orders=0, strict=False, stream=stream)
    env.enable_device_ingress(16)
    _refused(bk, lambda: env.enable_open_orders(4), "max_orders")
    _one_order_and_a_step(torch, env, B)
    env.close()
    # n_traders and depth out of range, the other entries without the view, a second call, a book range out of bounds
    env = ingress_env(bk, torch, B, 4, 64, 0, 16, tick=1, n_orders=64)
    _refused(bk, lambda: env.enable_open_orders(0), "n_traders")
    _refused(bk, lambda: env.enable_open_orders(65537), "n_traders")
    _refused(bk, lambda: env.enable_open_orders(4, depth=65), "depth")
    _refused(bk, env.open_orders, "no open-order view")
    _refused(bk, env.refresh_open_orders, "no open-order view")
    _refused(bk, env.open_orders_device_ptrs, "no open-order view")
    _refused(bk, env.open_orders_views, "no open-order view")
    a, b = ctypes.c_void_p(), ctypes.c_void_p()
    for rc in (env._L.bk_open_orders_refresh(env._h), env._L.bk_open_orders_device_ptrs(env._h, ctypes.byref(a), ctypes.byref(b)),
               env._L.bk_get_open_orders(env._h, 0, 1, None, None)):
        assert rc == BK_INVALID_ARGUMENT and b"no open-order view" in env._L.bk_last_error()
    _one_order_and_a_step(torch, env, B)
    env.enable_open_orders(65536, depth=64)  # the largest of both, after a step
    _refused(bk, lambda: env.enable_open_orders(4), "already enabled")
    _refused(bk, lambda: env.open_orders(1, 2), "out of bounds")
    _refused(bk, lambda: env.open_orders(3, 0), "out of bounds")
    summary, entries = env.open_orders(1, 1)
    assert summary.shape == (1, 65536) and entries.shape == (1, 65536, 64)
    assert summary[0, 0].tolist() == (2, 0, 1, 0, 100, 0xFFFFFFFF) and entries[0, 0, 0].tolist() == (0, 100, 2, 1)
    assert not summary["n_bid"][0, 1:].any() and (entries["order_id"][0, 1:] == 0xFFFFFFFF).all()
    _one_order_and_a_step(torch, env, B)
    assert env.open_orders(0, 1)[0][0, 0].tolist() == (4, 0, 2, 0, 100, 0xFFFFFFFF)
    env.close()
