"""Trader accounts of a device-ingress env (bk_accounts_enable; bourse_amd/csrc/accounts.hpp): per-book rows
{position, cash, volume, fills} per trader, folded on the device from every step's new trade records.

The expected side never shares code with the kernel: tests/accounts_model.py::fold (plain Python ints) over the trades and
orders of one oracle.StepEnv(SEED + b) per book (one oracle.ManyMarkets(1, SEED + m) per market - the oracle's MarketEnv)
that is given the same calls as the device env; case 1's rows are literal numbers worked out by hand.  Where a case says
something only under a condition - a step with more trades than two chunks, many parties of one chunk on one trader,
self-trades, traders without a row, idle book-steps - the condition is counted on the expected side and asserted before
anything is compared."""

import numpy as np
import pytest

import accounts_model as AM
import oracle_parity as P
from ingress_support import SEED, STEP, apply_oracle, ingress_env, members_env, submit
from members_ingress_cases import NOISE

pytestmark = pytest.mark.gpu
TRADE_OVERFLOW, ORDER_LOG_FULL, INEXACT = 2, 8, 512
BK_INVALID_ARGUMENT = 5


@pytest.fixture(scope="module")
def bk():
    import bourse_amd

    return bourse_amd


def same_rows(got, want, tag):
    assert got.dtype == want.dtype == AM.ACCOUNT_DTYPE, (got.dtype, want.dtype)
    assert got.shape == want.shape, f"{tag}: rows {got.shape} vs {want.shape}"
    for f in want.dtype.names:
        P.same_array(got[f], want[f], tag, f"account field {f}")


def new_orders(n_b, side, vol, trader, price):
    """(offsets, arrays) of new limit orders, n_b[b] for book b, in submit's / apply_oracle's format"""
    off = np.zeros(len(n_b) + 1, dtype=np.int64)
    off[1:] = np.cumsum(n_b)
    n = int(off[-1])
    return off, (np.ones(n, np.uint32), np.asarray(side, np.uint8), np.asarray(vol, np.uint32), np.asarray(trader, np.uint32),
                 np.asarray(price, np.uint32), np.zeros(n, np.uint64))


def busy_flow(rng, B, tick, idle=(), n_lo=80, n_hi=160, n_ids=7):
    """One step of case 2's recipe: per book 80..160 new limit orders, side uniform, price U{45..55} x tick, volume U{1..5}
    or, with probability 0.2, U{50..199}, trader U{0..6}; the books in `idle` get none."""
    n_b = np.array([0 if b in idle else int(rng.integers(n_lo, n_hi + 1)) for b in range(B)])
    n = int(n_b.sum())
    side = rng.integers(0, 2, size=n)
    price = rng.integers(45, 56, size=n) * tick
    small, large = rng.integers(1, 6, size=n), rng.integers(50, 200, size=n)
    vol = np.where(rng.random(n) < 0.2, large, small)
    return new_orders(n_b, side, vol, rng.integers(0, n_ids, size=n), price)


class Books:
    """One oracle StepEnv per book and (env given) the device env driven by the same calls."""

    def __init__(self, oracle, B, tick, env=None, torch=None):
        self.env, self.torch, self.B = env, torch, B
        self.refs = [oracle.StepEnv(SEED + b, 0, tick, STEP) for b in range(B)]
        self.last_trades = [0] * B  # each book's trade count before its latest step

    def submit(self, off, ins):
        if self.env is not None:
            submit(self.torch, self.env, off, ins)
        for b, r in enumerate(self.refs):
            apply_oracle(r, int(off[b]), int(off[b + 1]), ins)

    def step(self):
        if self.env is not None:
            self.env.step(sync=False)
        self.last_trades = [r.book.n_trades() for r in self.refs]
        for r in self.refs:
            r.step()

    def want(self, n_traders, first=None, books=None):
        books = range(self.B) if books is None else books
        return np.stack([AM.fold(self.refs[b].book.trades_array(), self.refs[b].book.orders_array(), n_traders,
                                 0 if first is None else first[b]) for b in books])


class Seen:
    """What the fold met, counted on the expected side: the most trades of one book-step, the most parties of one 64-record
    chunk (counted from the book's trade count before the step, as the device's cursor counts) on one trader, self-trades,
    parties without a row, book-steps without a trade."""

    def __init__(self, n_traders):
        self.n_traders, self.most_trades, self.most_parties, self.self_trades, self.skipped, self.idle = n_traders, 0, 0, 0, 0, 0

    def note(self, books):
        for b, r in enumerate(books.refs):
            t, o, first = r.book.trades_array(), r.book.orders_array(), books.last_trades[b]
            self.most_trades = max(self.most_trades, len(t) - first)
            self.idle += len(t) == first
            self.most_parties = max(self.most_parties, AM.parties_per_chunk(t, o, first, self.n_traders))
            ta = o["trader_id"][t["active_id"][first:].astype(np.int64)]
            tp = o["trader_id"][t["passive_id"][first:].astype(np.int64)]
            self.self_trades += int(((ta == tp) & (ta < self.n_traders)).sum())
            self.skipped += int((ta >= self.n_traders).sum() + (tp >= self.n_traders).sum())


# ------------------------------------------------------------------------------------------------ 1. by hand
def test_rows_worked_out_by_hand(bk, oracle):
    """Book 0, tick 1, one stage per step (a step shuffles its events, so nothing here depends on the order inside one):
      s0  trader 0 rests ask 10 @ 100 (id 0)
      s1  trader 1 bids 4 @ 100 (id 1): a PARTIAL fill of id 0 - 4 @ 100, 1 buys from 0
      s2  trader 2 rests ask 3 @ 101 (id 2), trader 0 rests ask 2 @ 102 (id 3)
      s3  trader 3 bids 11 @ 102 (id 4): ONE AGGRESSOR SWEEPS three resting orders of two traders - 6 @ 100 from 0, 3 @ 101
          from 2, 2 @ 102 from 0
      s4  trader 1 rests bid 5 @ 90 (id 5)
      s5  trader 2 sells 3 at the market (price 0, id 6): 3 @ 90, 1 buys from 2
      s6  trader 1 asks 2 @ 90 (id 7): a SELF-TRADE with its own bid id 5 - 2 @ 90, position and cash unchanged, volume + 4,
          fills + 2
      s7  trader 0 rests ask 4 000 000 000 @ 4 000 000 000 (id 8)
      s8  trader 3 bids the same (id 9): 4e9 @ 4e9 = 16e18 > 2^63, the cash words wrap
    trader 0: position -4 -8 -4e9, cash 400 + 804 + 16e18 (mod 2^64), volume 4 + 8 + 4e9, fills 1 + 2 + 1
    trader 1: position +4 +3 (+2 -2), cash -400 -270 (-180 +180), volume 4 + 3 + 2 + 2, fills 1 + 1 + 2
    trader 2: position -3 -3, cash 303 + 270, volume 6, fills 2
    trader 3: position +11 +4e9, cash -(600 + 303 + 204) - 16e18 (mod 2^64), volume 11 + 4e9, fills 3 + 1
    Book 1 is never touched: its rows stay zero."""
    import torch

    BIG = 4_000_000_000
    stages = [[(0, 10, 0, 100)], [(1, 4, 1, 100)], [(0, 3, 2, 101), (0, 2, 0, 102)], [(1, 11, 3, 102)], [(1, 5, 1, 90)],
              [(0, 3, 2, 0)], [(0, 2, 1, 90)], [(0, BIG, 0, BIG)], [(1, BIG, 3, BIG)]]  # (bid, vol, trader, price)
    env = ingress_env(bk, torch, 2, len(stages), 64, 0, 8, tick=1, n_orders=32)
    env.enable_accounts(4)
    books = Books(oracle, 2, 1, env, torch)
    for rows in stages:
        books.submit(*new_orders([len(rows), 0], *zip(*rows)))
        books.step()
    env.sync()
    P.no_flags(env)
    want = np.zeros((2, 4), dtype=AM.ACCOUNT_DTYPE)
    want[0] = [(-4_000_000_012, -2_446_744_073_709_550_412, 4_000_000_012, 4),
               (7, -670, 11, 4),
               (-6, 573, 6, 2),
               (4_000_000_011, 2_446_744_073_709_550_509, 4_000_000_011, 4)]
    got = env.accounts()
    assert got.shape == (2, 4) and got.dtype == bk.ACCOUNT_DTYPE
    same_rows(got, want, "by hand")
    assert not got[1].view(np.uint64).any()
    # the oracle's book made exactly these trades, and the model folds them to the same rows
    assert books.refs[0].book.n_trades() == 7 and books.refs[1].book.n_trades() == 0
    same_rows(books.want(4), want, "the model over the oracle's trades")
    same_rows(env.accounts(1, 1), want[1:], "accounts(first_book, n_books)")
    env.close()


# ------------------------------------------------------------------------------------------------ 2. after every step
def test_rows_equal_the_oracle_fold_after_every_step(bk, oracle):
    import torch

    B, T, tick, NT = 5, 6, 2, 5
    env = ingress_env(bk, torch, B, T, 256, 0, 256, tick=tick, n_ext=160)
    env.enable_accounts(NT)
    books, seen = Books(oracle, B, tick, env, torch), Seen(NT)
    rng = np.random.default_rng(7)
    got = []
    for s in range(T):
        books.submit(*busy_flow(rng, B, tick, idle=(4,) if s % 2 else ()))
        books.step()
        seen.note(books)
        got.append((env.accounts(), books.want(NT)))
    assert seen.most_trades > 128, seen.most_trades       # three chunks in one launch of one wave
    assert seen.most_parties >= 8, seen.most_parties      # conflicts inside a chunk
    assert seen.self_trades > 0 and seen.skipped > 0 and seen.idle > 0, vars(seen)
    P.no_flags(env)
    for s, (g, w) in enumerate(got):
        same_rows(g, w, f"after step {s}")
    for b in range(B):  # (consume_trades = 0: the host's readers see every record)
        assert env.trade_count(b) == (books.refs[b].book.n_trades(), 0), b
        P.same_trades(env, b, books.refs[b].book)
    env.close()


def test_traders_that_share_a_lane_take_further_passes(bk, oracle):
    """The fold gives trader x to lane x % 64, and two traders of one chunk on one lane cost a further pass over the
    chunk.  Here the rows are 3, 67, 131, 195 (all lane 3) and 4, 68 (lane 4) of n_traders = 200, with 250 left out: every
    chunk of a busy step holds four traders on one lane and two on another."""
    import torch

    B, T, tick, NT = 2, 3, 2, 200
    ids = np.array([3, 67, 131, 195, 4, 68, 250], dtype=np.uint32)
    env = ingress_env(bk, torch, B, T, 256, 0, 256, tick=tick, n_ext=160)
    env.enable_accounts(NT)
    books = Books(oracle, B, tick, env, torch)
    rng = np.random.default_rng(23)
    shared = 0  # the most distinct traders (with a row) of one chunk on one lane
    for s in range(T):
        off, ins = busy_flow(rng, B, tick)
        books.submit(off, ins[:3] + (ids[ins[3]],) + ins[4:])
        books.step()
        for b, r in enumerate(books.refs):
            t, o = r.book.trades_array(), r.book.orders_array()["trader_id"]
            for lo in range(books.last_trades[b], len(t), 64):
                who = np.unique(np.concatenate([o[t["active_id"][lo:lo + 64].astype(np.int64)],
                                                o[t["passive_id"][lo:lo + 64].astype(np.int64)]]))
                shared = max(shared, int(np.bincount(who[who < NT] % 64).max()))
    assert shared == 4, shared
    P.no_flags(env)
    want = books.want(NT)
    assert (want["fills"] > 0).sum(axis=1).tolist() == [6] * B  # exactly the six rows, in both books
    same_rows(env.accounts(), want, "traders on shared lanes")
    env.close()


# ------------------------------------------------------------------------------------------------ 3. members in the loop
def external(rng, B, n_max):
    """a few limit orders of traders 40..47 around the members' prices, and now and then a market order"""
    n_b = rng.integers(1, n_max + 1, size=B)
    n = int(n_b.sum())
    bid = rng.integers(0, 2, size=n)
    price = rng.integers(40, 60, size=n)
    market = rng.random(n) < 0.2
    price[market] = np.where(bid[market] == 1, 0xFFFFFFFF, 0)
    return new_orders(n_b, bid, rng.integers(20, 200, size=n), rng.integers(40, 48, size=n), price)


@pytest.mark.parametrize("kind", ["members", "random"])
def test_members_and_agents_in_the_loop(bk, oracle, kind):
    import torch

    B, T, NT, NX = 3, 8, 64, 6
    if kind == "members":
        members = [("noise", 0, 30, dict(NOISE, p_limit=0.5, p_market=0.5))]
        env = members_env(bk, torch, B, T, 128, members, 1, n_ext=NX)
        env.set_agents(members)
        sets = [oracle.AgentSet(members) for _ in range(B)]
        update = env.update_members
    else:
        groups = [(30, (40, 60), (10, 40), 1, 0.8)]  # trader id = the agent's index: 0..29
        env = ingress_env(bk, torch, B, T, 128, 30, 30 + NX, tick=1, n_ext=NX)
        env.set_random_agents(groups)
        sets = [oracle.RandomAgentSet(groups) for _ in range(B)]
        update = env.update_agents
    env.enable_accounts(NT)
    books = Books(oracle, B, 1, env, torch)
    rng = np.random.default_rng(3)
    for _ in range(T):
        update(sync=False)
        for b in range(B):
            sets[b].update(books.refs[b])
        books.submit(*external(rng, B, NX))
        books.step()
    want = books.want(NT)
    assert want["fills"][:, :30].any() and want["fills"][:, 40:48].any(), "no fills of the members / of the external traders"
    assert not want["fills"][:, 30:40].any() and not want["fills"][:, 48:].any()
    P.no_flags(env)
    same_rows(env.accounts(), want, kind)
    for b in range(B):
        P.same_trades(env, b, books.refs[b].book)
    env.close()


# ------------------------------------------------------------------------------------------------ 4. consume_trades
def test_consumed_trades_need_room_for_one_step_only(bk, oracle):
    import torch

    B, T, tick, NT = 3, 10, 2, 5
    flows = [busy_flow(np.random.default_rng(40 + s), B, tick, n_lo=150, n_hi=160) for s in range(T)]
    plan = Books(oracle, B, tick)  # the expected side first: it sizes trade_capacity
    per_step = []
    for f in flows:
        plan.submit(*f)
        plan.step()
        per_step.append([r.book.n_trades() - n0 for r, n0 in zip(plan.refs, plan.last_trades)])
    cap = 2 * max(max(x) for x in per_step)
    totals = [r.book.n_trades() for r in plan.refs]
    assert min(totals) > 3 * cap, (totals, cap)
    n_orders = 160 * T + 16
    env = bk.ManyBookEnv(B, SEED, 0, tick, STEP, levels=10, max_live_orders=512, max_orders=n_orders, trade_capacity=cap,
                         history_capacity=T, stream=torch.cuda.current_stream().cuda_stream)
    env.enable_device_ingress(queue_capacity=256)
    env.enable_accounts(NT, consume_trades=True)
    books = Books(oracle, B, tick, env, torch)
    for f in flows:
        books.submit(*f)
        books.step()
        for b in range(B):
            n = books.refs[b].book.n_trades()
            assert env.trade_count(b) == (n, n), (b, env.trade_count(b), n)
    P.no_flags(env)
    same_rows(env.accounts(), books.want(NT), "consume_trades")
    env.close()


# ------------------------------------------------------------------------------------------------ 5. inexact is flagged
def test_dropped_trade_records_flag_their_book_only(bk, oracle):
    import torch

    B, T, tick, NT = 3, 4, 2, 5
    rng = np.random.default_rng(11)
    flows = []
    for s in range(T):  # book 0 trades a lot, the others a little
        n_b = [120, 8, 8]
        n = sum(n_b)
        flows.append(new_orders(n_b, rng.integers(0, 2, size=n), rng.integers(1, 6, size=n), rng.integers(0, 7, size=n),
                                rng.integers(48, 53, size=n) * tick))
    plan = Books(oracle, B, tick)
    for f in flows:
        plan.submit(*f)
        plan.step()
    totals = [r.book.n_trades() for r in plan.refs]
    cap = 64
    assert totals[0] > cap + 64 and 0 < max(totals[1:]) < cap, totals
    env = bk.ManyBookEnv(B, SEED, 0, tick, STEP, levels=10, max_live_orders=256, max_orders=120 * T + 16, trade_capacity=cap,
                         history_capacity=T, strict=False, stream=torch.cuda.current_stream().cuda_stream)
    env.enable_device_ingress(queue_capacity=128)
    env.enable_accounts(NT)
    books = Books(oracle, B, tick, env, torch)
    for f in flows:
        books.submit(*f)
        books.step()
    env.sync()
    flags = env.flags()
    assert flags[0] == TRADE_OVERFLOW | INEXACT and not flags[1:].any(), flags
    want = books.want(NT)
    got = env.accounts()
    same_rows(got[1:], want[1:], "the books that kept every record")
    # book 0 holds exactly the records that were kept: the first trade_capacity of them
    t0 = books.refs[0].book
    same_rows(got[:1], AM.fold(t0.trades_array()[:cap], t0.orders_array(), NT)[None], "the records that were kept")
    with pytest.raises(bk.CapacityError, match="ACCOUNTS_INEXACT"):
        env.raise_on_flags()
    env.close()


def test_an_order_beyond_max_orders_flags_its_book_only(bk, oracle):
    import torch

    B, tick, NT, MAXO = 2, 1, 4, 24
    # book 0: 20 resting asks, then 20 bids that cross them (ids 20..39: 24.. are beyond max_orders); book 1: 6 + 6
    rest = new_orders([20, 6], np.zeros(26), np.full(26, 3), np.arange(26) % 3, np.full(26, 100))
    cross = new_orders([20, 6], np.ones(26), np.full(26, 3), 1 + np.arange(26) % 3, np.full(26, 100))
    env = bk.ManyBookEnv(B, SEED, 0, tick, STEP, levels=10, max_live_orders=64, max_orders=MAXO, trade_capacity=256,
                         history_capacity=2, strict=False, stream=torch.cuda.current_stream().cuda_stream)
    env.enable_device_ingress(queue_capacity=32)
    env.enable_accounts(NT)
    books = Books(oracle, B, tick, env, torch)
    for f in (rest, cross):
        books.submit(*f)
        books.step()
    env.sync()
    t0, o0 = books.refs[0].book.trades_array(), books.refs[0].book.orders_array()
    beyond = (t0["active_id"] >= MAXO) | (t0["passive_id"] >= MAXO)
    assert beyond.any() and not beyond.all() and len(t0) == 20
    flags = env.flags()
    f0 = int(flags[0])
    assert f0 & INEXACT and not f0 & ~(ORDER_LOG_FULL | INEXACT) and flags[1] == 0, flags
    got = env.accounts()
    same_rows(got[1:], books.want(NT, books=[1]), "the book inside max_orders")
    same_rows(got[:1], AM.fold(t0[~beyond], o0, NT)[None], "the records whose orders have a record")
    env.close()


# ------------------------------------------------------------------------------------------------ 6. reset and clear
def test_a_reset_book_counts_from_its_reset(bk, oracle):
    """3 steps, save, 3 steps, reset books 0 and 2 (a torch CUDA mask), 2 steps.  The oracle cannot be rewound, so a reset
    book's expected side is a REPLAY (tests/test_gpu_ingress_reset.py): a fresh oracle env given steps 0..2 again and then
    the two steps after the reset; its rows are the fold of that env's trades from the snapshot's trade count on."""
    import torch

    B, tick, NT = 4, 2, 5
    env = ingress_env(bk, torch, B, 8, 256, 0, 64, tick=tick, n_ext=40)
    env.enable_accounts(NT)
    books = Books(oracle, B, tick, env, torch)
    flows = [busy_flow(np.random.default_rng(60 + s), B, tick, n_lo=30, n_hi=40) for s in range(8)]

    def run(lo, hi, bs=books):
        for f in flows[lo:hi]:
            bs.submit(*f)
            bs.step()

    run(0, 3)
    env.save_ingress_snapshot()
    snap_trades = [r.book.n_trades() for r in books.refs]
    run(3, 6)
    before = env.accounts()
    same_rows(before, books.want(NT), "before the reset")
    mask = np.array([1, 0, 1, 0], dtype=bool)
    env.reset_ingress_books(torch.tensor(mask, device="cuda"), sync=False)
    now = env.accounts()
    assert not now[mask].view(np.uint64).any(), "the masked rows read zero at once"
    same_rows(now[~mask], before[~mask], "the unmasked rows are unchanged")
    run(6, 8)
    replay = Books(oracle, B, tick)
    run(0, 3, replay)
    assert [r.book.n_trades() for r in replay.refs] == snap_trades
    run(6, 8, replay)
    got = env.accounts()
    P.no_flags(env)
    kept, reset = np.flatnonzero(~mask), np.flatnonzero(mask)
    assert all(replay.refs[b].book.n_trades() > snap_trades[b] > 0 for b in reset)
    same_rows(got[kept], books.want(NT, books=kept), "never reset: every trade")
    same_rows(got[reset], replay.want(NT, first=snap_trades, books=reset), "reset: the replayed trades since the snapshot")
    env.close()


@pytest.mark.parametrize("kind", ["host", "device", "all"])
def test_cleared_rows_count_the_next_steps_only(bk, oracle, kind):
    import torch

    B, tick, NT = 4, 2, 5
    env = ingress_env(bk, torch, B, 4, 256, 0, 64, tick=tick, n_ext=40)
    env.enable_accounts(NT)
    books = Books(oracle, B, tick, env, torch)
    flows = [busy_flow(np.random.default_rng(80 + s), B, tick, n_lo=30, n_hi=40) for s in range(4)]
    for f in flows[:3]:
        books.submit(*f)
        books.step()
    before = env.accounts()
    assert before["fills"].any(axis=1).all()
    mask = np.ones(B, dtype=bool) if kind == "all" else np.array([0, 1, 1, 0], dtype=bool)
    first = [r.book.n_trades() if mask[b] else 0 for b, r in enumerate(books.refs)]
    if kind == "all":
        env.clear_accounts()
    elif kind == "host":
        env.clear_accounts(mask)
    else:
        env.clear_accounts(torch.tensor(mask, device="cuda"), sync=False)
    now = env.accounts()
    assert not now[mask].view(np.uint64).any()
    same_rows(now[~mask], before[~mask], "the unmasked rows are unchanged")
    books.submit(*flows[3])
    books.step()
    assert all(r.book.n_trades() > n for r, n in zip(books.refs, books.last_trades))
    same_rows(env.accounts(), books.want(NT, first=first), f"after clear_accounts ({kind})")
    P.no_flags(env)
    env.close()


# ------------------------------------------------------------------------------------------------ 7. markets
def test_markets_keep_rows_per_book(bk, oracle):
    import torch

    NM, A, T, NT, TICKS = 2, 2, 5, 4, [1, 2]
    env = bk.ManyMarketEnv(NM, SEED, 0, TICKS, STEP, levels=10, max_live_orders=256, max_orders=512, trade_capacity=1024,
                           history_capacity=T, stream=torch.cuda.current_stream().cuda_stream)
    env.enable_device_ingress(128)
    env.enable_accounts(NT)
    refs = [oracle.ManyMarkets(1, SEED + m, 0, TICKS, STEP, True, 10) for m in range(NM)]
    rng = np.random.default_rng(17)
    for _ in range(T):
        n_b = rng.integers(20, 40, size=NM * A)
        n = int(n_b.sum())
        off, ins = new_orders(n_b, rng.integers(0, 2, size=n), rng.integers(1, 30, size=n), rng.integers(0, 6, size=n),
                              rng.integers(48, 53, size=n) * 2)
        submit(torch, env, off, ins)
        for b in range(NM * A):
            for i in range(int(off[b]), int(off[b + 1])):
                refs[b // A].place_order(0, b % A, bool(ins[1][i]), int(ins[2][i]), int(ins[3][i]), price=int(ins[4][i]))
        env.step(sync=False)
        for r in refs:
            r.step()
    got = env.accounts()
    P.no_flags(env)
    assert got.shape == (NM * A, NT)
    for m in range(NM):
        active = []
        for a in range(A):
            view = refs[m].book(0, a)
            want = AM.fold(view.trades_array(), view.orders_array(), NT)
            assert want["fills"].all(), "a trader without a fill in this book"
            same_rows(got[env.book(m, a)], want, (m, a))
            P.same_trades(env, env.book(m, a), view)
            active.append(want["fills"] > 0)
        assert (active[0] & active[1]).any()  # the same trader in both assets of the market, one row per book
    env.close()


# ------------------------------------------------------------------------------------------------ 8. the device view
def test_the_device_view_is_the_table_in_place(bk, oracle):
    import torch

    B, tick, NT = 3, 2, 5
    env = ingress_env(bk, torch, B, 2, 256, 0, 64, tick=tick, n_ext=40)
    env.enable_accounts(NT)
    view = env.accounts_view()
    cai = view.__cuda_array_interface__
    assert cai["shape"] == (B, NT, 4) and cai["typestr"] == "<i8" and cai["version"] == 3 and cai["strides"] is None
    stream = torch.cuda.current_stream().cuda_stream
    assert cai["stream"] == (stream if stream else 1)  # (the interface spells the legacy default stream 1, never 0)
    t = torch.as_tensor(view, device="cuda")
    assert t.dtype == torch.int64 and tuple(t.shape) == (B, NT, 4) and t.is_contiguous()
    assert env.accounts_device_ptr() == t.data_ptr() == cai["data"][0]
    books = Books(oracle, B, tick, env, torch)
    for s in range(2):
        books.submit(*busy_flow(np.random.default_rng(90 + s), B, tick, n_lo=30, n_hi=40))
        books.step()  # step(sync=False) on the env's stream, which is torch's current one
    on_device = t.clone()  # queued on the same stream, behind the fold
    torch.cuda.current_stream().synchronize()
    rows = env.accounts()
    assert rows["fills"].any()
    for tensor in (on_device, t):
        a = tensor.cpu().numpy()
        for k, f in enumerate(("position", "cash", "volume", "fills")):
            P.same_array(a[:, :, k].view(rows[f].dtype), rows[f], "device view", f)
    same_rows(rows, books.want(NT), "device view")
    env.close()


# ------------------------------------------------------------------------------------------------ 9. refusals
def _refused(bk, call, match):
    with pytest.raises(bk.BourseError, match=match) as e:
        call()
    assert e.value.code == BK_INVALID_ARGUMENT


def _one_order_and_a_step(torch, env, B):
    submit(torch, env, *new_orders([1] * B, np.ones(B), np.full(B, 2), np.zeros(B), np.full(B, 100)))
    env.step()


def test_refusals_leave_the_env_working(bk, oracle):
    import torch

    B = 2
    stream = torch.cuda.current_stream().cuda_stream
    # without the device ingress
    env = bk.ManyBookEnv(B, SEED, 0, 1, STEP, max_live_orders=64, max_orders=64, stream=stream)
    _refused(bk, lambda: env.enable_accounts(4), "device ingress")
    env.place_order(0, True, 5, 1, price=100)
    env.step()
    assert env.order_count(0) == 1
    env.close()
    # max_orders = 0
    env = bk.ManyBookEnv(B, SEED, 0, 1, STEP, max_live_orders=64, max_orders=0, strict=False, stream=stream)
    env.enable_device_ingress(16)
    _refused(bk, lambda: env.enable_accounts(4), "max_orders")
    _one_order_and_a_step(torch, env, B)
    env.close()
    # n_traders out of range, an ingress slot held, twice, load_book
    env = ingress_env(bk, torch, B, 4, 64, 0, 16, tick=1, n_orders=64)
    _refused(bk, lambda: env.enable_accounts(0), "n_traders")
    _refused(bk, lambda: env.enable_accounts(65537), "n_traders")
    _refused(bk, env.accounts, "no trader accounts")
    _refused(bk, env.accounts_device_ptr, "no trader accounts")
    _refused(bk, env.clear_accounts, "no trader accounts")
    env.save_ingress_snapshot()
    _refused(bk, lambda: env.enable_accounts(4), "snapshot slot")
    env.drop_ingress_snapshot()
    env.enable_accounts(65536)
    _refused(bk, lambda: env.enable_accounts(4), "already enabled")
    assert env.accounts().shape == (B, 65536)
    rc = env._L.bk_load_book(env._h, 0, 0, 0, 0, None, None, None, 0, None)
    assert rc == BK_INVALID_ARGUMENT and b"trader accounts" in env._L.bk_last_error()
    _one_order_and_a_step(torch, env, B)
    env.save_ingress_snapshot()  # (a slot may be saved once the accounts exist)
    env.close()
    # after a step
    env = ingress_env(bk, torch, B, 4, 64, 0, 16, tick=1, n_orders=64)
    _one_order_and_a_step(torch, env, B)
    _refused(bk, lambda: env.enable_accounts(4), "before the first")
    _one_order_and_a_step(torch, env, B)
    assert env.order_count(0) == 2
    env.close()
