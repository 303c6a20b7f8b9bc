"""Per-step trade bars of a device-ingress env (bk_trade_bars_enable; bourse_amd/csrc/trade_bars.hpp): a ring of
{open, high, low, close, buy_vol, sell_vol, notional, n_buy, n_sell} per book, folded on the device from every step's new
trade records.

The expected side never shares code with the kernel: tests/trade_bars_model.py::fold (plain Python ints) over the trades
of one oracle.StepEnv(SEED + b) per book (one oracle.ManyMarkets(1, SEED + m) per market) that is given the same calls as
the device env, with the number of records each step made counted on that side; case 1's rows are literal numbers worked
out by hand.  Where a case says something only under a condition - a book-step of three chunks, a high or low outside the
first chunk, idle book-steps, members' trades - the condition is counted on the expected side and asserted before anything
is compared."""

import numpy as np
import pytest

import oracle_parity as P
import trade_bars_model as TM
from ingress_support import SEED, STEP, ingress_env, members_env, submit
from members_ingress_cases import NOISE
from test_gpu_accounts import Books, busy_flow, external, new_orders
from test_gpu_accounts import same_rows as same_accounts

pytestmark = pytest.mark.gpu
TRADE_OVERFLOW = 2
BK_INVALID_ARGUMENT = 5
FIELDS = TM.TRADE_BAR_DTYPE.names


@pytest.fixture(scope="module")
def bk():
    import bourse_amd

    return bourse_amd


def same_bars(got, want, tag):
    assert got.dtype == want.dtype == TM.TRADE_BAR_DTYPE, (got.dtype, want.dtype)
    assert got.shape == want.shape, f"{tag}: rows {got.shape} vs {want.shape}"
    for f in FIELDS:
        P.same_array(got[f], want[f], tag, f"bar field {f}")


def idle(p):
    return (p, p, p, p, 0, 0, 0, 0, 0)


class Tape(Books):
    """Books that also keep, per book, the number of trade records each step made - what the model folds by."""

    def __init__(self, oracle, B, tick, env=None, torch=None):
        super().__init__(oracle, B, tick, env, torch)
        self.counts = [[] for _ in range(B)]

    def step(self):
        super().step()
        for b, r in enumerate(self.refs):
            self.counts[b].append(r.book.n_trades() - self.last_trades[b])

    def bars(self, window, books=None, since=0, first=None):
        """the rings after the steps so far: steps `since`.. folded from record first[b] on, the steps before left out"""
        books = range(self.B) if books is None else books
        return np.stack([TM.fold(self.refs[b].book.trades_array(), self.counts[b][since:], window, since,
                                 0 if first is None else first[b]) for b in books])


# ------------------------------------------------------------------------------------------------ 1. by hand
def test_bars_worked_out_by_hand(bk, oracle):
    """Book 0, tick 1, one stage per step (a step shuffles its events, so nothing here depends on the order inside one),
    window 4 - step k goes to slot k % 4:
      s0  trader 0 rests ask 10 @ 100                                   no trade before the first: all zero
      s1  trader 1 bids 4 @ 100: a PARTIAL fill, 4 @ 100, bought        {100 100 100 100, 4 0, 400, 1 0}
      s2  trader 2 rests ask 3 @ 105, trader 0 rests ask 2 @ 102        idle: carries 100
      s3  trader 3 bids 11 @ 105: a SWEEP of three levels - 6 @ 100, 2 @ 102, 3 @ 105 - open 100 != close 105; one
          aggressor walks the levels in price order, so a sweep's high is its close: {100 105 100 105, 11 0, 1119, 3 0}
      s4  nothing at all                                                idle: carries 105 (slot 0 again)
      s5  trader 1 rests bid 5 @ 90                                     idle: carries 105
      s6  trader 2 sells 3 at the market (price 0): 3 @ 90, sold        {90 90 90 90, 0 3, 270, 0 1}
      s7  traders 0 and 2 rest asks 4 000 000 000 @ 4 000 000 000       idle: carries 90
      s8  traders 3 and 1 bid the same: two records of 4e9 @ 4e9 - buy_vol 8e9 passes 2^32 and the notional 32e18 wraps:
          32e18 - 2^64 = 13 553 255 926 290 448 384                     (slot 0 a third time)
    Book 1 is never touched: its rows stay zero."""
    import torch

    BIG = 4_000_000_000
    stages = [[(0, 10, 0, 100)], [(1, 4, 1, 100)], [(0, 3, 2, 105), (0, 2, 0, 102)], [(1, 11, 3, 105)], [], [(1, 5, 1, 90)],
              [(0, 3, 2, 0)], [(0, BIG, 0, BIG), (0, BIG, 2, BIG)], [(1, BIG, 3, BIG), (1, BIG, 1, BIG)]]  # (bid, vol, trader, price)
    env = ingress_env(bk, torch, 2, len(stages), 64, 0, 8, tick=1, n_orders=32)
    env.enable_trade_bars(4)
    assert env.trade_bars_slot() == 3  # (before the first step: (0 - 1) % 4)
    tape = Tape(oracle, 2, 1, env, torch)
    after_s3 = None
    for s, rows in enumerate(stages):
        tape.submit(*new_orders([len(rows), 0], *(zip(*rows) if rows else ([], [], [], []))))
        tape.step()
        assert env.trade_bars_slot() == s % 4
        if s == 3:
            after_s3 = env.trade_bars()
    env.sync()
    P.no_flags(env)
    want = np.zeros((2, 4), dtype=TM.TRADE_BAR_DTYPE)
    want[0] = [idle(0), (100, 100, 100, 100, 4, 0, 400, 1, 0), idle(100), (100, 105, 100, 105, 11, 0, 600 + 204 + 315, 3, 0)]
    same_bars(after_s3, want, "by hand, after step 3")
    want[0] = [(BIG, BIG, BIG, BIG, 2 * BIG, 0, 13_553_255_926_290_448_384, 2, 0), idle(105), (90, 90, 90, 90, 0, 3, 270, 0, 1), idle(90)]
    assert 2 * BIG * BIG - (1 << 64) == 13_553_255_926_290_448_384 and 2 * BIG > 1 << 32
    got = env.trade_bars()
    assert got.shape == (2, 4) and got.dtype == bk.TRADE_BAR_DTYPE
    same_bars(got, want, "by hand")
    assert not got[1].view(np.uint32).any()
    # the oracle's book made exactly these trades, and the model folds them to the same rows
    assert tape.counts[0] == [0, 1, 0, 3, 0, 0, 1, 0, 2] and tape.refs[1].book.n_trades() == 0
    same_bars(tape.bars(4), want, "the model over the oracle's trades")
    same_bars(env.trade_bars(1, 1), want[1:], "trade_bars(first_book, n_books)")
    env.close()


# ------------------------------------------------------------------------------------------------ 2. after every step
@pytest.mark.parametrize("window", [3, 1])
def test_bars_equal_the_model_after_every_step(bk, oracle, window):
    import torch

    B, T, tick = 5, 7, 2  # (5 books: the last block of four waves holds one; 7 steps: a ring of 3 wraps twice)
    env = ingress_env(bk, torch, B, T, 256, 0, 256, tick=tick, n_ext=160)
    env.enable_trade_bars(window)
    tape = Tape(oracle, B, tick, env, torch)
    rng = np.random.default_rng(7)
    got = []
    for s in range(T):
        tape.submit(*busy_flow(rng, B, tick, idle=(4,) if s % 2 else ()))
        tape.step()
        got.append((env.trade_bars(), tape.bars(window)))
    most = outside = idle_steps = 0  # counted from each book's trade count before the step, as the device's cursor counts
    for b, r in enumerate(tape.refs):
        price, lo = r.book.trades_array()["price"], 0
        for n in tape.counts[b]:
            p = price[lo:lo + n]
            most, idle_steps, lo = max(most, n), idle_steps + (n == 0), lo + n
            outside += n > 64 and (p[:64].max() < p.max() or p[:64].min() > p.min())
    assert most > 128, most            # three chunks in one launch of one wave
    assert outside > 0 and idle_steps > 0, (outside, idle_steps)
    P.no_flags(env)
    for s, (g, w) in enumerate(got):
        same_bars(g, w, f"window {window}, after step {s}")
    for b in range(B):  # (consume_trades = 0: the host's readers see every record)
        assert env.trade_count(b) == (tape.refs[b].book.n_trades(), 0), b
        P.same_trades(env, b, tape.refs[b].book)
    env.close()


# ------------------------------------------------------------------------------------------------ 3. beside the accounts
@pytest.mark.parametrize("consume", ["none", "bars", "accounts"])
def test_bars_and_accounts_on_one_env(bk, oracle, consume):
    """Both folds read the same records: the bars' first, and with consumption - asked for by ONE of the two - the last fold
    of the step consumes for both, so trade_capacity holds one step's trades and neither hides a record from the other."""
    import torch

    B, T, tick, NT, W = 3, 6, 2, 5, 2
    flows = [busy_flow(np.random.default_rng(40 + s), B, tick, n_lo=150, n_hi=160) for s in range(T)]
    plan = Tape(oracle, B, tick)  # the expected side first: it sizes trade_capacity
    for f in flows:
        plan.submit(*f)
        plan.step()
    totals = [r.book.n_trades() for r in plan.refs]
    cap = max(max(c) for c in plan.counts)  # exactly the busiest book-step
    assert min(totals) > 3 * cap, (totals, cap)
    n_orders = 160 * T + 16
    env = bk.ManyBookEnv(B, SEED, 0, tick, STEP, levels=10, max_live_orders=512, max_orders=n_orders,
                         trade_capacity=2 * n_orders if consume == "none" else cap, history_capacity=T,
                         stream=torch.cuda.current_stream().cuda_stream)
    env.enable_device_ingress(queue_capacity=256)
    env.enable_accounts(NT, consume_trades=consume == "accounts")
    env.enable_trade_bars(W, consume_trades=consume == "bars")
    tape = Tape(oracle, B, tick, env, torch)
    for f in flows:
        tape.submit(*f)
        tape.step()
        for b in range(B):
            n = tape.refs[b].book.n_trades()
            assert env.trade_count(b) == (n, 0 if consume == "none" else n), (b, env.trade_count(b), n)
        same_bars(env.trade_bars(), tape.bars(W), f"consume = {consume}")
    P.no_flags(env)
    same_accounts(env.accounts(), tape.want(NT), f"accounts, consume = {consume}")
    env.close()


def test_bars_alone_consume_their_records(bk, oracle):
    import torch

    B, T, tick = 2, 4, 2
    flows = [busy_flow(np.random.default_rng(50 + s), B, tick, n_lo=150, n_hi=160) for s in range(T)]
    plan = Tape(oracle, B, tick)
    for f in flows:
        plan.submit(*f)
        plan.step()
    cap = max(max(c) for c in plan.counts)
    assert min(r.book.n_trades() for r in plan.refs) > 2 * cap
    env = bk.ManyBookEnv(B, SEED, 0, tick, STEP, levels=10, max_live_orders=512, max_orders=160 * T + 16, trade_capacity=cap,
                         history_capacity=T, stream=torch.cuda.current_stream().cuda_stream)
    env.enable_device_ingress(queue_capacity=256)
    env.enable_trade_bars(1, consume_trades=True)
    tape = Tape(oracle, B, tick, env, torch)
    for f in flows:
        tape.submit(*f)
        tape.step()
        for b in range(B):
            n = tape.refs[b].book.n_trades()
            assert env.trade_count(b) == (n, n), (b, env.trade_count(b), n)
    P.no_flags(env)
    same_bars(env.trade_bars(), tape.bars(1), "consume_trades")
    env.close()


# ------------------------------------------------------------------------------------------------ 4. dropped records
def test_dropped_trade_records_flag_their_book_only(bk, oracle):
    import torch

    B, T, tick, W, cap = 3, 4, 2, 2, 64
    rng = np.random.default_rng(11)
    flows = []
    for s in range(T):  # book 0 trades a lot, the others a little
        n_b = [120, 8, 8]
        n = sum(n_b)
        flows.append(new_orders(n_b, rng.integers(0, 2, size=n), rng.integers(1, 6, size=n), rng.integers(0, 7, size=n),
                                rng.integers(48, 53, size=n) * tick))
    plan = Tape(oracle, B, tick)
    for f in flows:
        plan.submit(*f)
        plan.step()
    totals = [r.book.n_trades() for r in plan.refs]
    assert totals[0] > cap + 64 and 0 < max(totals[1:]) < cap, totals
    env = bk.ManyBookEnv(B, SEED, 0, tick, STEP, levels=10, max_live_orders=256, max_orders=120 * T + 16, trade_capacity=cap,
                         history_capacity=T, strict=False, stream=torch.cuda.current_stream().cuda_stream)
    env.enable_device_ingress(queue_capacity=128)
    env.enable_trade_bars(W)
    tape = Tape(oracle, B, tick, env, torch)
    for f in flows:
        tape.submit(*f)
        tape.step()
    env.sync()
    flags = env.flags()
    # (the bars have no flag bit of their own: the book whose bars miss records is the one that carries TRADE_OVERFLOW)
    assert flags[0] == TRADE_OVERFLOW and not flags[1:].any(), flags
    got = env.trade_bars()
    same_bars(got[1:], tape.bars(W, books=[1, 2]), "the books that kept every record")
    # book 0's bars are those of the records that were kept - the first trade_capacity of them, step by step
    ends = np.minimum(np.cumsum(tape.counts[0]), cap)
    kept = np.diff(np.concatenate([[0], ends])).tolist()
    assert kept != tape.counts[0] and kept[-1] == 0 and kept[0] > 0, kept  # a step that lost every record, one that kept some
    same_bars(got[:1], TM.fold(tape.refs[0].book.trades_array()[:cap], kept, W)[None], "the records that were kept")
    with pytest.raises(bk.CapacityError, match="TRADE_OVERFLOW"):
        env.raise_on_flags()
    env.close()


# ------------------------------------------------------------------------------------------------ 5. members in the loop
def test_members_in_the_loop(bk, oracle):
    import torch

    B, T, NX, W = 3, 8, 6, 3
    members = [("noise", 0, 30, dict(NOISE, p_limit=0.5, p_market=0.5))]
    env = members_env(bk, torch, B, T, 128, members, 1, n_ext=NX)
    env.set_agents(members)
    sets = [oracle.AgentSet(members) for _ in range(B)]
    env.enable_trade_bars(W)
    tape = Tape(oracle, B, 1, env, torch)
    rng = np.random.default_rng(3)
    for _ in range(T):
        env.update_members(sync=False)
        for b in range(B):
            sets[b].update(tape.refs[b])
        tape.submit(*external(rng, B, NX))
        tape.step()
        same_bars(env.trade_bars(), tape.bars(W), "members")
    among, outside = 0, 0  # trades between two members, and trades with an external trader (ids 40..47)
    for r in tape.refs:
        t, who = r.book.trades_array(), r.book.orders_array()["trader_id"]
        a, p = who[t["active_id"].astype(np.int64)], who[t["passive_id"].astype(np.int64)]
        among, outside = among + int(((a < 30) & (p < 30)).sum()), outside + int(((a >= 40) | (p >= 40)).sum())
    assert among > 0 and outside > 0, (among, outside)
    P.no_flags(env)
    for b in range(B):
        P.same_trades(env, b, tape.refs[b].book)
    env.close()


# ------------------------------------------------------------------------------------------------ 6. reset and clear
def test_a_reset_book_counts_from_its_reset(bk, oracle):
    """3 steps, save, 3 steps, reset books 0 and 2 (a torch CUDA mask), 2 steps.  The oracle cannot be rewound, so a reset
    book's expected side is a REPLAY: a fresh oracle env given steps 0..2 again and then the two steps after the reset; its
    ring is the fold of that env's trades from the snapshot's trade count on, into a zero ring, at the env's step counter
    (which a reset does not rewind): steps 6 and 7, slots 0 and 1 of 3, slot 2 still zero."""
    import torch

    B, tick, W = 4, 2, 3
    env = ingress_env(bk, torch, B, 8, 256, 0, 64, tick=tick, n_ext=40)
    env.enable_trade_bars(W)
    tape = Tape(oracle, B, tick, env, torch)
    flows = [busy_flow(np.random.default_rng(60 + s), B, tick, n_lo=30, n_hi=40) for s in range(8)]

    def run(lo, hi, bs=tape):
        for f in flows[lo:hi]:
            bs.submit(*f)
            bs.step()

    run(0, 3)
    env.save_ingress_snapshot()
    snap_trades = [r.book.n_trades() for r in tape.refs]
    run(3, 6)
    before = env.trade_bars()
    same_bars(before, tape.bars(W), "before the reset")
    assert before["close"].all(), "a row that is zero already"
    mask = np.array([1, 0, 1, 0], dtype=bool)
    env.reset_ingress_books(torch.tensor(mask, device="cuda"), sync=False)
    now = env.trade_bars()
    assert not now[mask].view(np.uint32).any(), "the masked rows read zero at once"
    same_bars(now[~mask], before[~mask], "the unmasked rows are unchanged")
    run(6, 8)
    replay = Tape(oracle, B, tick)
    run(0, 3, replay)
    assert [r.book.n_trades() for r in replay.refs] == snap_trades
    run(6, 8, replay)
    got = env.trade_bars()
    P.no_flags(env)
    kept, reset = np.flatnonzero(~mask), np.flatnonzero(mask)
    assert all(min(replay.counts[b][3:]) > 0 and snap_trades[b] > 0 for b in reset)
    same_bars(got[kept], tape.bars(W, books=kept), "never reset: every step")
    # (the replay's steps 3 and 4 are the env's steps 6 and 7)
    want = np.stack([TM.fold(replay.refs[b].book.trades_array(), replay.counts[b][3:], W, 6, snap_trades[b]) for b in reset])
    assert not np.ascontiguousarray(want[:, 2]).view(np.uint32).any() and want["close"][:, :2].all()
    same_bars(got[reset], want, "reset: the replayed steps since the snapshot, into a zero ring")
    env.close()


def test_a_reset_book_carries_price_zero(bk, oracle):
    """After a reset, a step without a trade carries 0 - not the close the book had - while an unmasked book carries on."""
    import torch

    B, tick, W = 2, 2, 2
    env = ingress_env(bk, torch, B, 4, 256, 0, 64, tick=tick, n_ext=40)
    env.enable_trade_bars(W)
    tape = Tape(oracle, B, tick, env, torch)
    env.save_ingress_snapshot()
    for s in range(2):
        tape.submit(*busy_flow(np.random.default_rng(70 + s), B, tick, n_lo=30, n_hi=40))
        tape.step()
    before = env.trade_bars()
    assert before["close"].all()
    env.reset_ingress_books(np.array([1, 0], dtype=bool))
    env.step()  # nothing submitted: step 2, slot 0
    got = env.trade_bars()
    assert env.trade_bars_slot() == 0
    assert not got[0].view(np.uint32).any()
    assert tuple(got[1, 0]) == idle(int(before[1, 1]["close"])) and got[1, 1] == before[1, 1]
    P.no_flags(env)
    env.close()


@pytest.mark.parametrize("kind", ["host", "device", "all"])
def test_cleared_rows_count_the_next_steps_only(bk, oracle, kind):
    import torch

    B, tick, W = 4, 2, 2
    env = ingress_env(bk, torch, B, 4, 256, 0, 64, tick=tick, n_ext=40)
    env.enable_trade_bars(W)
    tape = Tape(oracle, B, tick, env, torch)
    flows = [busy_flow(np.random.default_rng(80 + s), B, tick, n_lo=30, n_hi=40) for s in range(4)]
    for f in flows[:3]:
        tape.submit(*f)
        tape.step()
    before = env.trade_bars()
    assert before["close"].all()
    mask = np.ones(B, dtype=bool) if kind == "all" else np.array([0, 1, 1, 0], dtype=bool)
    first = [r.book.n_trades() for r in tape.refs]
    if kind == "all":
        env.clear_trade_bars()
    elif kind == "host":
        env.clear_trade_bars(mask)
    else:
        env.clear_trade_bars(torch.tensor(mask, device="cuda"), sync=False)
    now = env.trade_bars()
    assert not now[mask].view(np.uint32).any()
    same_bars(now[~mask], before[~mask], "the unmasked rows are unchanged")
    tape.submit(*flows[3])
    tape.step()
    assert all(c[3] > 0 for c in tape.counts)
    got = env.trade_bars()
    for b in range(B):  # a cleared book: step 3 alone, into a zero ring
        want = tape.bars(W, books=[b], since=3, first=first) if mask[b] else tape.bars(W, books=[b])
        same_bars(got[b:b + 1], want, f"after clear_trade_bars ({kind}), book {b}")
    P.no_flags(env)
    env.close()


# ------------------------------------------------------------------------------------------------ 7. markets
def test_markets_keep_rows_per_book(bk, oracle):
    import torch

    NM, A, T, W, TICKS = 2, 2, 5, 2, [1, 2]
    env = bk.ManyMarketEnv(NM, SEED, 0, TICKS, STEP, levels=10, max_live_orders=256, max_orders=512, trade_capacity=1024,
                           history_capacity=T + 1, stream=torch.cuda.current_stream().cuda_stream)
    env.enable_device_ingress(128)
    env.enable_trade_bars(W)
    env.save_ingress_snapshot()
    refs = [oracle.ManyMarkets(1, SEED + m, 0, TICKS, STEP, True, 10) for m in range(NM)]
    counts = [[] for _ in range(NM * A)]
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
        before = [len(refs[b // A].book(0, b % A).trades_array()) for b in range(NM * A)]
        for r in refs:
            r.step()
        for b in range(NM * A):
            counts[b].append(len(refs[b // A].book(0, b % A).trades_array()) - before[b])
    got = env.trade_bars()
    P.no_flags(env)
    assert got.shape == (NM * A, W)
    for m in range(NM):
        for a in range(A):
            view, b = refs[m].book(0, a), env.book(m, a)
            assert b == m * A + a and min(counts[b][-W:]) > 0, "a book without a trade in the last steps"
            same_bars(got[b], TM.fold(view.trades_array(), counts[b], W), (m, a))
            P.same_trades(env, b, view)
    # a reset market: both of its books read zero and carry 0 through a step without a trade; the other market carries on
    env.reset_ingress_markets(np.array([0, 1], dtype=bool))
    env.step()  # step 5, slot 1
    now = env.trade_bars()
    assert not now[A:].view(np.uint32).any()
    for b in range(A):
        assert now[b, 0] == got[b, 0] and tuple(now[b, 1]) == idle(int(got[b, 0]["close"])), b
    env.close()


# ------------------------------------------------------------------------------------------------ 8. the device view
def test_the_device_view_is_the_table_in_place(bk, oracle):
    import torch

    B, tick, W = 3, 2, 2
    env = ingress_env(bk, torch, B, 3, 256, 0, 64, tick=tick, n_ext=40)
    env.enable_trade_bars(W)
    view = env.trade_bars_view()
    cai = view.__cuda_array_interface__
    assert cai["shape"] == (B, W, 6) and cai["typestr"] == "<i8" and cai["version"] == 3 and cai["strides"] is None
    stream = torch.cuda.current_stream().cuda_stream
    assert cai["stream"] == (stream if stream else 1)  # (the interface spells the legacy default stream 1, never 0)
    t = torch.as_tensor(view, device="cuda")
    assert t.dtype == torch.int64 and tuple(t.shape) == (B, W, 6) and t.is_contiguous()
    assert env.trade_bars_device_ptr() == t.data_ptr() == cai["data"][0]
    tape = Tape(oracle, B, tick, env, torch)
    for s in range(3):
        tape.submit(*busy_flow(np.random.default_rng(90 + s), B, tick, n_lo=30, n_hi=40))
        tape.step()  # step(sync=False) on the env's stream, which is torch's current one
    on_device = t.clone()  # queued on the same stream, behind the fold
    newest = on_device[:, env.trade_bars_slot()].cpu().numpy().view(np.uint64)
    torch.cuda.current_stream().synchronize()
    rows = env.trade_bars()
    assert (rows["n_buy"] + rows["n_sell"]).all()
    for tensor in (on_device, t):
        a = tensor.cpu().numpy().view(np.uint64)
        lo, hi = a & np.uint64(0xFFFFFFFF), a >> np.uint64(32)
        for k, f in ((0, "open"), (1, "low"), (5, "n_buy")):
            P.same_array(lo[:, :, k], rows[f], "device view", f)
        for k, f in ((0, "high"), (1, "close"), (5, "n_sell")):
            P.same_array(hi[:, :, k], rows[f], "device view", f)
        for k, f in ((2, "buy_vol"), (3, "sell_vol"), (4, "notional")):
            P.same_array(a[:, :, k], rows[f], "device view", f)
    want = tape.bars(W)
    same_bars(rows, want, "device view")
    # trade_bars_slot() names the newest row: step 2 of 3 went to slot 0
    assert env.trade_bars_slot() == 0
    P.same_array(newest[:, 1] >> np.uint64(32), want["close"][:, 0], "device view", "close of the newest row")
    P.same_array(newest[:, 4], want["notional"][:, 0], "device view", "notional of the newest row")
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
    _refused(bk, lambda: env.enable_trade_bars(4), "device ingress")
    env.place_order(0, True, 5, 1, price=100)
    env.step()
    assert env.order_count(0) == 1
    env.close()
    # a reader before enable, window out of range, twice, load_book - mid-run, with an ingress slot held
    env = ingress_env(bk, torch, B, 8, 64, 0, 16, tick=1, n_orders=64)
    _one_order_and_a_step(torch, env, B)
    env.save_ingress_snapshot()
    for reader in (env.trade_bars, env.trade_bars_device_ptr, env.trade_bars_view, env.trade_bars_slot, env.clear_trade_bars):
        _refused(bk, reader, "no trade bars")
    for call in (env._L.bk_get_trade_bars, env._L.bk_trade_bars_clear, env._L.bk_trade_bars_clear_device):
        assert call(env._h, *([0, 0, None] if call is env._L.bk_get_trade_bars else [None])) == BK_INVALID_ARGUMENT
        assert b"no trade bars" in env._L.bk_last_error()
    _refused(bk, lambda: env.enable_trade_bars(0), "window")
    _refused(bk, lambda: env.enable_trade_bars(1025), "window")
    _one_order_and_a_step(torch, env, B)
    env.enable_trade_bars(1024)
    _refused(bk, lambda: env.enable_trade_bars(4), "already enabled")
    assert env.trade_bars().shape == (B, 1024) and not env.trade_bars().view(np.uint32).any()  # steps before the enable: zero rows
    rc = env._L.bk_load_book(env._h, 0, 0, 0, 0, None, None, None, 0, None)
    assert rc == BK_INVALID_ARGUMENT and b"trade bars" in env._L.bk_last_error()
    _one_order_and_a_step(torch, env, B)
    assert env.order_count(0) == 3 and env.trade_bars_slot() == 2
    env.close()
