"""The queue view of a device-ingress env (bk_open_queue_enable; bourse_amd/csrc/open_queue.hpp): beside every entry of the
open-order view a row {ahead_vol, level_ahead_vol, level_vol, ahead_orders, level_ahead_orders}, recomputed on the device from
the pool right behind the open-order rows - behind every step and every reset.

The expected side never shares code with the kernel: tests/open_queue_model.py::rows (plain Python) over the orders and the
key times of one oracle.StepEnv(SEED + b) per book (one oracle.ManyMarkets(1, SEED + m) per market) that is given the same
calls as the device env, and over tests/open_orders_model.py's entry lists; case 1's rows are literal numbers worked out by
hand.  The expected side runs FIRST (a QueuePlan: the flows and the rows after every step), because a flow's cancellations
and modifications name ids that rest on it.  Where a case says something only under a condition - a level queue of two or
more, a younger id ahead (an order re-stamped by a modification), the front of the book, a partially filled order ahead, more
than 64 orders ahead, used entries beyond the first 64, live orders without a row - the condition is counted on the expected
side and asserted before anything is compared."""
import ctypes

import numpy as np
import pytest

import open_orders_model as OM
import open_queue_model as QM
import oracle_parity as P
import test_gpu_open_orders as OO
from ingress_support import MOD, SEED, STEP, apply_oracle, ingress_env, members_env, submit
from members_ingress_cases import NOISE
from test_gpu_open_orders import flow, instructions, new

pytestmark = pytest.mark.gpu
BK_INVALID_ARGUMENT = 5
ORDER_LOG_FULL = 8
Z = (0, 0, 0, 0, 0)


@pytest.fixture(scope="module")
def bk():
    import bourse_amd

    return bourse_amd


def same_queue(got, want, tag):
    assert got.dtype == want.dtype == QM.OPEN_QUEUE_DTYPE, (got.dtype, want.dtype)
    assert got.shape == want.shape, f"{tag}: queue rows {got.shape} vs {want.shape}"
    for f in want.dtype.names:
        P.same_array(got[f], want[f], tag, f"queue field {f}")


class Counts:
    """the conditions of a comparison, counted on the expected side"""

    def __init__(self):
        self.listed = self.level2 = self.younger = self.front = self.partial_ahead = self.far = self.second_pass = 0
        self.no_row_ahead = self.most_ahead = self.most_live = self.idle = 0

    def note(self, view, entries, rows, n_traders, max_orders=None):
        o = view.orders_array()
        queues = QM.sides(o, view.keys()[2])
        hit = set(int(i) for i in view.trades_array()["passive_id"])
        at = {i: (s, k) for s, q in queues.items() for k, (i, _, _) in enumerate(q)}
        self.most_live = max(self.most_live, len(at))
        flat = 0
        for t, listed in enumerate(entries):
            for k, e in enumerate(listed):
                flat += 1
                if e[0] == QM.NO_ORDER:
                    continue
                s, place = at[e[0]]
                before = queues[s][:place]
                row = rows[t][k]
                self.listed += 1
                self.second_pass += flat > 64
                self.level2 += row[4] >= 2
                self.front += row[3] == 0
                self.far += row[3] > 64
                self.most_ahead = max(self.most_ahead, row[3])
                self.younger += any(p == e[1] and i > e[0] for i, p, _ in before)
                self.partial_ahead += any(i in hit for i, _, _ in before)
                self.no_row_ahead += any(int(o["trader_id"][i]) >= n_traders or (max_orders is not None and i >= max_orders)
                                         for i, _, _ in before)


def model(views, n_traders, depth, counts=None, max_orders=None):
    """the queue model over one oracle book view per book, stacked as env.open_queue() returns it"""
    out = []
    for v in views:
        o = v.orders_array()
        entries = OM.rows_ints(o, n_traders, depth, max_orders)[1]
        rows = QM.rows_ints(o, v.keys()[2], entries)
        if counts is not None:
            counts.note(v, entries, rows, n_traders, max_orders)
        q = np.zeros((n_traders, depth), dtype=QM.OPEN_QUEUE_DTYPE)
        for t in range(n_traders):
            for k in range(depth):
                q[t, k] = rows[t][k]
        out.append(q)
    return np.stack(out)


class QueuePlan:
    """The expected side of a run, made before the device sees anything: one oracle StepEnv per book, every step's
    instructions, the open-order model's and the queue model's rows after it, and the conditions they were met under."""

    def __init__(self, oracle, B, tick, n_traders, depth, max_orders=None):
        self.B, self.tick, self.NT, self.depth, self.max_orders = B, tick, n_traders, depth, max_orders
        self.refs = [oracle.StepEnv(SEED + b, 0, tick, STEP) for b in range(B)]
        self.steps = []  # (offsets, arrays, open-order rows, queue rows)
        self.c = Counts()

    def rows(self, count=True):
        views = [r.book for r in self.refs]
        return (OO.model_rows(views, self.NT, self.depth, self.max_orders),
                model(views, self.NT, self.depth, self.c if count else None, self.max_orders))

    def step(self, off, ins):
        for b, r in enumerate(self.refs):
            apply_oracle(r, int(off[b]), int(off[b + 1]), ins)
            r.step()
            self.c.idle += off[b] == off[b + 1]
        open_rows, queue = self.rows()
        self.steps.append((off, ins, open_rows, queue))
        return queue

    @property
    def qcap(self):
        return max(len(ins[0]) for _, ins, _, _ in self.steps)


def run_plan(torch, env, plan, tag, first=0):
    """the plan's steps on the device, both tables compared after every one"""
    for s, (off, ins, open_rows, queue) in enumerate(plan.steps[first:], first):
        submit(torch, env, off, ins)
        env.step(sync=False)
        OO.same_rows(env.open_orders(), open_rows, f"{tag}: open orders after step {s}")
        same_queue(env.open_queue(), queue, f"{tag}: after step {s}")


# ------------------------------------------------------------------------------------------------ 1. by hand
# Book 0 of six, tick 1, n_traders = 2, depth = 4; trader 9 has no row.  One stage per step (a step shuffles its events, so
# no stage depends on the order inside one: the two orders of stage 3 rest on different sides).  Rows are (ahead_vol,
# level_ahead_vol, level_vol, ahead_orders, level_ahead_orders); trader 0's entries are ids 0, 1, 4, trader 1's id 2.
HAND_STAGES = [
    # s0  bid 10 @ 100 (id 0): alone
    ([new(1, 10, 0, 100)], [[(0, 0, 10, 0, 0), Z, Z, Z], [Z, Z, Z, Z]]),
    # s1  bid 20 @ 100 (id 1) behind it
    ([new(1, 20, 0, 100)], [[(0, 0, 30, 0, 0), (10, 10, 30, 1, 1), Z, Z], [Z, Z, Z, Z]]),
    # s2  bid 30 @ 100 of trader 1 (id 2): three bids at one price
    ([new(1, 30, 1, 100)], [[(0, 0, 60, 0, 0), (10, 10, 60, 1, 1), Z, Z], [(30, 30, 60, 2, 2), Z, Z, Z]]),
    # s3  a better bid 5 @ 101 of trader 9, who has no row (id 3), and trader 0's ask 8 @ 105 (id 4)
    ([new(1, 5, 9, 101), new(0, 8, 0, 105)],
     [[(5, 0, 60, 1, 0), (15, 10, 60, 2, 1), (0, 0, 8, 0, 0), Z], [(35, 30, 60, 3, 2), Z, Z, Z]]),
    # s4  id 0 modified to a LARGER volume, 15: replaced, behind ids 1 and 2 - the level is 20, 30, 15
    ([(MOD, 4, 15, 0, 0, 0)],
     [[(55, 50, 65, 3, 2), (5, 0, 65, 1, 0), (0, 0, 8, 0, 0), Z], [(25, 20, 65, 2, 1), Z, Z, Z]]),
    # s5  id 1 modified to a SMALLER volume, 12: keeps its place - the level is 12, 30, 15
    ([(MOD, 4, 12, 0, 0, 1)],
     [[(47, 42, 57, 3, 2), (5, 0, 57, 1, 0), (0, 0, 8, 0, 0), Z], [(17, 12, 57, 2, 1), Z, Z, Z]]),
    # s6  trader 9 sells 9 @ 100: id 3 fills (5), then a partial fill at the front of the level, id 1 keeps 8 - 8, 30, 15
    ([new(0, 9, 9, 100)],
     [[(38, 38, 53, 2, 2), (0, 0, 53, 0, 0), (0, 0, 8, 0, 0), Z], [(8, 8, 53, 1, 1), Z, Z, Z]]),
]


def hand_rows(rows, B=6):
    q = np.zeros((B, 2, 4), dtype=QM.OPEN_QUEUE_DTYPE)
    for t in range(2):
        for k in range(4):
            q[0, t, k] = rows[t][k]
    return q


def test_rows_worked_out_by_hand(bk, oracle):
    import torch

    B = 6
    plan = QueuePlan(oracle, B, 1, 2, 4)
    for s, (rows, want) in enumerate(HAND_STAGES):
        got = plan.step(*instructions([rows] + [[]] * (B - 1)))
        same_queue(got, hand_rows(want), f"the model over the oracle's book, stage {s}")
    c = plan.c
    assert c.younger > 0 and c.partial_ahead > 0 and c.no_row_ahead > 0 and c.level2 > 0 and c.front > 0, vars(c)
    env = ingress_env(bk, torch, B, len(HAND_STAGES), 64, 0, 8, tick=1, n_orders=32)
    env.enable_open_orders(2, 4)
    env.enable_open_queue()
    same_queue(env.open_queue(), hand_rows([[Z] * 4] * 2), "at enable")
    for s, (off, ins, _, _) in enumerate(plan.steps):
        submit(torch, env, off, ins)
        env.step(sync=False)
        same_queue(env.open_queue(), hand_rows(HAND_STAGES[s][1]), f"stage {s}")
    P.no_flags(env)
    same_queue(env.open_queue(0, 1), hand_rows(HAND_STAGES[-1][1])[:1], "open_queue(first_book, n_books)")
    env.refresh_open_orders()  # (nothing changed a pool: the same rows)
    same_queue(env.open_queue(), hand_rows(HAND_STAGES[-1][1]), "after refresh_open_orders")
    env.close()


# ------------------------------------------------------------------------------------------------ 2. after every step
N_NEW = {64: (5, 12), 128: (10, 30), 256: (30, 56), 512: (60, 120)}  # n_new U{lo .. hi - 1} per book-step, by pool size


def busy_plan(oracle, pool, B=6, T=8, NT=4, depth=8, traders=6, seed=5):
    """B books with tick 2, T steps of test_gpu_open_orders.flow with traders 0 .. traders - 1 (those >= NT have no row);
    book 2 idles every third step"""
    plan = QueuePlan(oracle, B, 2, NT, depth)
    rng = np.random.default_rng(seed)
    lo, hi = N_NEW[pool]
    for s in range(T):
        plan.step(*flow(rng, plan.refs, 2, rng.integers(lo, hi, size=B), np.arange(traders), idle=(2,) if s % 3 == 2 else ()))
    return plan


@pytest.mark.parametrize("pool", [64, 128, 256, 512])
def test_rows_equal_the_model_after_every_step_of_a_busy_flow(bk, oracle, pool):
    import torch

    plan = busy_plan(oracle, pool)
    c = plan.c
    assert c.listed > 0 and c.level2 > 0 and c.younger > 0 and c.front > 0 and c.partial_ahead > 0, vars(c)
    assert c.no_row_ahead > 0 and c.idle > 0, vars(c)
    if pool >= 256:
        assert c.far > 0, vars(c)
    assert pool // 2 < c.most_live <= pool, (c.most_live, pool)  # beyond the pool's first half, and within it
    env = ingress_env(bk, torch, plan.B, len(plan.steps), pool, 0, plan.qcap, tick=plan.tick, n_ext=plan.qcap)
    env.enable_open_orders(plan.NT, plan.depth)
    env.enable_open_queue()
    run_plan(torch, env, plan, f"pool {pool}")
    P.no_flags(env)
    for b in range(plan.B):
        P.same_live(env, b, plan.refs[b].book)
    env.close()


# ------------------------------------------------------------------------------------------------ 3. more than 64 entries
@pytest.mark.parametrize("NT,depth,traders", [(12, 8, 14), (70, 2, 76), (4, 1, 6), (1, 64, 1)])
def test_more_entries_than_a_wave_has_lanes(bk, oracle, NT, depth, traders):
    """12 x 8 and 70 x 2: the entries of a book are taken 64 at a time, and the second pass (the third of 70 x 2) holds used
    ones; depth 1; depth 64 with one trader who rests more than 64 orders - a whole pass of used entries and a partly used one."""
    import torch

    plan = busy_plan(oracle, 128, B=6, T=6, NT=NT, depth=depth, traders=traders, seed=23)
    c = plan.c
    assert c.listed > 0 and c.level2 > 0 and c.front > 0 and 64 < c.most_live <= 128, vars(c)
    if NT * depth > 64:
        assert c.second_pass > 0, vars(c)
    if NT == 1:
        s = plan.steps[-1][2][0]
        assert (s["n_bid"].astype(np.int64) + s["n_ask"]).max() > 64, "no trader rests more than 64 orders"
    else:
        assert c.no_row_ahead > 0, vars(c)
    env = ingress_env(bk, torch, plan.B, len(plan.steps), 128, 0, plan.qcap, tick=plan.tick, n_ext=plan.qcap)
    env.enable_open_orders(NT, depth)
    env.enable_open_queue()
    run_plan(torch, env, plan, f"{NT} traders x depth {depth}")
    P.no_flags(env)
    env.close()


# ------------------------------------------------------------------------------------------------ 4. counted, without a row
@pytest.mark.parametrize("kind", ["members", "random"])
def test_members_and_agents_in_the_loop(bk, oracle, kind):
    """members: Noise members with agent_id_start = 1000 >= n_traders through update_members - their resting orders have no
    row and stand in the strategy's (traders 40..47) queues.  random: RandomAgents through update_agents, whose trader ids are
    the agents' indices 0..29: they have rows of their own and stand in everybody's queues."""
    import torch

    B, T, NT, NX, depth = 6, 6, 64, 6, 3
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
    env.enable_open_queue()
    refs = [oracle.StepEnv(SEED + b, 0, 1, STEP) for b in range(B)]
    rng = np.random.default_rng(3)
    got, want, c = [], [], Counts()
    for _ in range(T):
        update(sync=False)
        off, ins = OO.external(rng, B, NX, np.arange(40, 48))
        submit(torch, env, off, ins)
        env.step(sync=False)
        for b in range(B):
            sets[b].update(refs[b])
            apply_oracle(refs[b], int(off[b]), int(off[b + 1]), ins)
            refs[b].step()
        got.append(env.open_queue())
        want.append(model([r.book for r in refs], NT, depth, c))
    assert c.listed > 0 and c.front > 0 and c.most_ahead > 0, vars(c)
    if kind == "members":
        assert c.no_row_ahead > 0, vars(c)  # a member's order ahead of a strategy's
    P.no_flags(env)
    for s, (g, w) in enumerate(zip(got, want)):
        same_queue(g, w, f"{kind}: after step {s}")
    env.close()


def test_a_resting_order_beyond_max_orders_counts(bk, oracle):
    """max_orders = 8.  Book 0 gets 12 bids at rising prices that all come to rest (ids 0..11): ids 8..11 have no record and
    no entry, but they are the four best bids and stand ahead of every listed one - the kernel reads the pool alone."""
    import torch

    B, NT, depth, MAXO = 6, 4, 8, 8
    plan = QueuePlan(oracle, B, 1, NT, depth, max_orders=MAXO)
    plan.step(*instructions([[new(1, 3 + i, i % 3, 90 + i) for i in range(12)]] +
                            [[new(i % 2, 2 + i, i % 4, 100 + 10 * (i % 2)) for i in range(6)]] * (B - 1)))
    q = plan.steps[0][3]
    assert plan.c.no_row_ahead >= 8 and q["ahead_orders"][0].max() == 11 and q["ahead_orders"][0, 0, 0] == 11, vars(plan.c)
    assert q["ahead_vol"][0, 2, 1] == sum(3 + i for i in range(6, 12))  # id 5, trader 2's second: ids 6..11 are ahead
    env = bk.ManyBookEnv(B, SEED, 0, 1, STEP, levels=10, max_live_orders=64, max_orders=MAXO, trade_capacity=64,
                         history_capacity=2, strict=False, stream=torch.cuda.current_stream().cuda_stream)
    env.enable_device_ingress(queue_capacity=16)
    env.enable_open_orders(NT, depth)
    env.enable_open_queue()
    run_plan(torch, env, plan, "beyond max_orders")
    flags = env.flags()
    assert flags[0] == ORDER_LOG_FULL and not flags[1:].any(), flags
    env.close()


# ------------------------------------------------------------------------------------------------ 5. reset, enabling mid-run
def test_reset_books_show_the_snapshots_queue_at_once(bk, oracle):
    """3 steps, save, ENABLE (mid-run, a snapshot slot held: right at once), 3 steps, reset books 0, 2 and 5 from a device
    mask with no step in between: the masked books show the model's rows AT THE SNAPSHOT, the others their current rows.  Then
    2 more steps: a reset book's expected side is a REPLAY - a fresh oracle env given steps 0..2 and then the two steps after
    the reset."""
    import torch

    B, tick, NT, depth = 6, 2, 5, 3
    flows = [OO.only_new(np.random.default_rng(60 + s), B, tick, 12, 20) for s in range(8)]
    plan, replay = QueuePlan(oracle, B, tick, NT, depth), QueuePlan(oracle, B, tick, NT, depth)
    for f in flows[:6]:
        plan.step(*f)
    for f in flows[:3] + flows[6:]:
        replay.step(*f)
    for f in flows[6:]:
        plan.step(*f)
    at_snapshot, current = plan.steps[2], plan.steps[5]
    mask = np.array([1, 0, 1, 0, 0, 1], dtype=bool)
    for b in np.flatnonzero(mask):
        assert at_snapshot[3][b].tolist() != current[3][b].tolist()
    assert plan.c.level2 > 0 and plan.c.no_row_ahead > 0 and replay.c.level2 > 0, vars(plan.c)

    env = ingress_env(bk, torch, B, 8, 256, 0, 32, tick=tick, n_ext=20)
    for s, (off, ins, open_rows, queue) in enumerate(plan.steps[:6]):
        submit(torch, env, off, ins)
        env.step(sync=False)
        if s == 2:
            env.save_ingress_snapshot()
            env.enable_open_orders(NT, depth)
            env.enable_open_queue()
            same_queue(env.open_queue(), queue, "right after enable, a snapshot slot held")
        elif s > 2:
            same_queue(env.open_queue(), queue, f"after step {s}")
    env.reset_ingress_books(torch.tensor(mask, device="cuda"), sync=False)
    now = env.open_queue()
    same_queue(now[mask], at_snapshot[3][mask], "masked books: the snapshot's queue")
    same_queue(now[~mask], current[3][~mask], "unmasked books: their current rows")
    OO.same_rows(OO.pick(env.open_orders(), mask), OO.pick(at_snapshot[2], mask), "masked books: the snapshot's entries")
    for s in (6, 7):
        off, ins, _, want = plan.steps[s]
        submit(torch, env, off, ins)
        env.step(sync=False)
        got = env.open_queue()
        same_queue(got[~mask], want[~mask], f"never reset, step {s}")
        same_queue(got[mask], replay.steps[s - 3][3][mask], f"reset: the replayed book, step {s}")
    P.no_flags(env)
    env.close()


# ------------------------------------------------------------------------------------------------ 6. markets
def market_flow(rng, n_books):
    n_b = rng.integers(8, 16, size=n_books)
    return instructions([[new(rng.integers(0, 2), rng.integers(1, 30), rng.integers(0, 6), int(rng.integers(48, 53)) * 2)
                          for _ in range(int(n))] for n in n_b])


class MarketPlan:
    """the expected side of a run of markets: one oracle.ManyMarkets(1, SEED + m) per market, the queue rows after every step"""

    def __init__(self, oracle, NM, ticks, NT, depth):
        self.A, self.NT, self.depth, self.c = len(ticks), NT, depth, Counts()
        self.refs = [oracle.ManyMarkets(1, SEED + m, 0, ticks, STEP, True, 10) for m in range(NM)]
        self.views = [self.refs[b // self.A].book(0, b % self.A) for b in range(NM * self.A)]
        self.rows = []

    def step(self, off, ins):
        for b in range(len(self.views)):
            for i in range(int(off[b]), int(off[b + 1])):
                self.refs[b // self.A].place_order(0, b % self.A, bool(ins[1][i]), int(ins[2][i]), int(ins[3][i]), price=int(ins[4][i]))
        for r in self.refs:
            r.step()
        self.rows.append(model(self.views, self.NT, self.depth, self.c))
        return self.rows[-1]


def test_markets_keep_rows_per_book(bk, oracle):
    """Three markets of three assets: nine books, so the last block of four waves holds one.  Two steps, save, two steps, then
    markets 0 and 2 are reset from a device mask of one byte per MARKET (the refresh behind the reset takes the mask three
    books to a byte): their six books show the snapshot's rows at once, market 1's three their current rows.  One more step:
    a reset market's expected side is a replay - fresh markets given steps 0, 1 and 4."""
    import torch

    NM, A, T, NT, depth, TICKS = 3, 3, 5, 4, 3, [1, 2, 2]
    rng = np.random.default_rng(17)
    flows = [market_flow(rng, NM * A) for _ in range(T)]
    plan, replay = MarketPlan(oracle, NM, TICKS, NT, depth), MarketPlan(oracle, NM, TICKS, NT, depth)
    for f in flows:
        want = plan.step(*f)
        assert (want["level_vol"] > 0).any(axis=(1, 2)).all(), "a book without a listed order"
    for f in flows[:2] + flows[4:]:
        replay.step(*f)
    c = plan.c
    assert c.level2 > 0 and c.front > 0 and c.no_row_ahead > 0 and c.partial_ahead > 0 and replay.c.level2 > 0, vars(c)
    markets = np.array([1, 0, 1], dtype=bool)
    mask = np.repeat(markets, A)  # per book
    for b in np.flatnonzero(mask):
        assert plan.rows[1][b].tolist() != plan.rows[3][b].tolist(), "a reset that changes nothing"

    env = bk.ManyMarketEnv(NM, SEED, 0, TICKS, STEP, levels=10, max_live_orders=128, max_orders=256, trade_capacity=512,
                           history_capacity=T, stream=torch.cuda.current_stream().cuda_stream)
    env.enable_device_ingress(64)
    env.enable_open_orders(NT, depth)
    env.enable_open_queue()
    for s in range(4):
        submit(torch, env, *flows[s])
        env.step(sync=False)
        same_queue(env.open_queue(), plan.rows[s], f"markets: after step {s}")
        if s == 1:
            env.save_ingress_snapshot()
    env.reset_ingress_books(torch.tensor(markets, device="cuda"), sync=False)
    now = env.open_queue()
    same_queue(now[mask], plan.rows[1][mask], "reset markets: the snapshot's queue in every book of them")
    same_queue(now[~mask], plan.rows[3][~mask], "the other market: its current rows")
    submit(torch, env, *flows[4])
    env.step(sync=False)
    got = env.open_queue()
    same_queue(got[~mask], plan.rows[4][~mask], "never reset, step 4")
    same_queue(got[mask], replay.rows[2][mask], "reset: the replayed markets, step 4")
    P.no_flags(env)
    assert got.shape == (NM * A, NT, depth)
    env.close()


# ------------------------------------------------------------------------------------------------ 7. the device view
def test_the_device_view_is_the_table_in_place(bk, oracle):
    import torch

    plan = busy_plan(oracle, 128, T=2, seed=19)
    B, NT, depth = plan.B, plan.NT, plan.depth
    env = ingress_env(bk, torch, B, 2, 128, 0, plan.qcap, tick=plan.tick, n_ext=plan.qcap)
    env.enable_open_orders(NT, depth)
    env.enable_open_queue()
    view = env.open_queue_view()
    stream = torch.cuda.current_stream().cuda_stream
    cai = view.__cuda_array_interface__
    assert cai["shape"] == (B, NT, depth, 4) and cai["typestr"] == "<i8" and cai["version"] == 3 and cai["strides"] is None
    assert cai["stream"] == (stream if stream else 1)
    t = torch.as_tensor(view, device="cuda")
    assert t.dtype == torch.int64 and t.is_contiguous() and env.open_queue_device_ptr() == t.data_ptr()

    def check_view(tag):
        env.sync()
        rows = env.open_queue()
        u = t.cpu().numpy().view(np.uint64)
        fields = {"ahead_vol": u[..., 0], "level_ahead_vol": u[..., 1], "level_vol": u[..., 2],
                  "ahead_orders": u[..., 3] & 0xFFFFFFFF, "level_ahead_orders": u[..., 3] >> 32}
        for f in rows.dtype.names:
            P.same_array(fields[f], rows[f].astype(np.uint64), tag, f"queue view, {f}")
        return rows

    off, ins, _, want = plan.steps[0]
    submit(torch, env, off, ins)
    env.step(sync=False)
    first = t.clone()  # queued on the same stream, behind the refresh
    same_queue(check_view("after step 0"), want, "view, step 0")
    off, ins, _, want = plan.steps[1]
    submit(torch, env, off, ins)
    env.step(sync=False)
    same_queue(check_view("after step 1"), want, "view, step 1")  # the same tensor, no new call
    assert not torch.equal(first, t), "the view did not change with the step"
    env.close()


# ------------------------------------------------------------------------------------------------ 8. refusals
def _refused(bk, call, match):
    with pytest.raises(bk.BourseError, match=match) as e:
        call()
    assert e.value.code == BK_INVALID_ARGUMENT


def test_refusals_leave_the_env_working(bk, oracle):
    import torch

    B = 6
    step = lambda env: (submit(torch, env, *instructions([[new(1, 2, 0, 100)]] * B)), env.step())
    # before enable_open_orders; the readers without the view
    env = ingress_env(bk, torch, B, 4, 64, 0, 16, tick=1, n_orders=64)
    _refused(bk, env.enable_open_queue, "bk_open_orders_enable")
    a = ctypes.c_void_p()
    for rc in (env._L.bk_open_queue_device_ptr(env._h, ctypes.byref(a)), env._L.bk_get_open_queue(env._h, 0, 1, None)):
        assert rc == BK_INVALID_ARGUMENT and b"no queue view" in env._L.bk_last_error()
    env.enable_open_orders(2, 2)
    for reader in (env.open_queue, env.open_queue_device_ptr, env.open_queue_view):
        _refused(bk, reader, "no queue view")
    assert env._L.bk_get_open_queue(env._h, 0, 1, None) == BK_INVALID_ARGUMENT and b"no queue view" in env._L.bk_last_error()
    step(env)
    env.enable_open_queue()  # after a step
    _refused(bk, env.enable_open_queue, "already enabled")
    _refused(bk, lambda: env.open_queue(1, B), "out of bounds")
    _refused(bk, lambda: env.open_queue(B + 1, 0), "out of bounds")
    rows = env.open_queue(1, 2)
    assert rows.shape == (2, 2, 2) and rows[0, 0].tolist() == [(0, 0, 2, 0, 0), Z] and rows[0, 1].tolist() == [Z, Z]
    step(env)
    assert env.open_queue(B - 1, 1)[0, 0].tolist() == [(0, 0, 4, 0, 0), (2, 2, 4, 1, 1)]
    env.close()
    # depth = 0: no entries, nothing to describe
    env = ingress_env(bk, torch, B, 4, 64, 0, 16, tick=1, n_orders=64)
    env.enable_open_orders(2, 0)
    _refused(bk, env.enable_open_queue, "depth")
    step(env)
    assert env.open_orders()[0]["n_bid"][:, 0].tolist() == [1] * B
    env.close()


def test_an_env_that_never_enables_it_is_unchanged(bk, oracle):
    """the open-order tests' busy flow on an env with the open-order view alone: the same rows as ever"""
    import torch

    plan = OO.busy_plan(oracle, 128, T=3)
    qcap = max(len(ins[0]) for _, ins, _ in plan.steps)
    env = ingress_env(bk, torch, plan.B, len(plan.steps), 128, 0, qcap, tick=plan.tick, n_ext=qcap)
    env.enable_open_orders(plan.NT, plan.depth)
    OO.run_plan(torch, env, plan, "no queue view")
    _refused(bk, env.open_queue, "no queue view")
    P.no_flags(env)
    for b in range(plan.B):
        P.same_live(env, b, plan.refs[b].book)
    env.close()
