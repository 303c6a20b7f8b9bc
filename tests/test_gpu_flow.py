"""The per-book flow table of the trade records (bk_flow_enable; bourse_amd/csrc/flow.hpp): eight base words and K lag rows
per book, folded on the device from each book's trade records in record order, the carry that makes every split of a fold
equal, and the count of the records it could not read.

The expected side never shares code with the kernel: tests/flow_model.py (plain Python ints) over the ORACLE's trades -
oracle.ManyBooks / ManyMarkets for bk_run, one oracle.StepEnv per book (one oracle.ManyMarkets per market) for the device
ingress - given the same calls; case 1's rows are literal numbers worked out by hand.  Before anything is compared the
expected side is asserted not to be trivial (`busy`): every compared book has more than K trades of both signs, some sum_ss
is negative and some positive, and n_lost is 0 where the case says nothing is lost.  All comparisons are bit for bit."""
import numpy as np
import pytest

import counter_shift as CS
import flow_model as FM
import oracle_parity as P
import trade_bars_model as TM
from ingress_support import SEED, STEP, ingress_env, members_env, submit
from members_ingress_cases import NOISE
from test_gpu_accounts import Books, external, new_orders
from test_gpu_accounts import same_rows as same_accounts
from test_gpu_reset_books import C2, MEMBERS, PIPELINES, as_kind, do_reset, make_env, make_mask, ref_books
from test_gpu_trade_bars import Tape, same_bars

pytestmark = pytest.mark.gpu
TRADE_OVERFLOW = 2
BK_INVALID_ARGUMENT = 5
M64 = (1 << 64) - 1
BIG = 1 << 62


@pytest.fixture(scope="module")
def bk():
    import bourse_amd

    return bourse_amd


def tape_of(view):
    """an oracle book's trades as the model's tape: (price, vol, side_is_bid) in record order"""
    t = view.trades_array()
    return list(zip(t["price"].tolist(), t["vol"].tolist(), t["side"].tolist()))


def whole(tape, K, start=0):
    return FM.fold_tape(tape, K, [(len(tape), 0, BIG)], start=start)


def same_flow(got, want, tag):
    assert got.dtype == want.dtype and got.shape == want.shape, f"{tag}: {got.dtype} {got.shape} vs {want.dtype} {want.shape}"
    for f in want.dtype.names:
        P.same_array(got[f], want[f], tag, f"flow field {f}")


def busy(want, K, lost=False):
    """the expected rows say something"""
    assert (want["n_trades"] > K).all(), want["n_trades"]
    assert ((want["n_buy"] > 0) & (want["n_buy"] < want["n_trades"])).all(), (want["n_buy"], want["n_trades"])
    ss = want["lags"][..., FM.LAG.index("sum_ss")]
    assert (ss < 0).any() and (ss > 0).any(), ss
    assert (want["lags"][:, K - 1, 0] > 0).all(), "no pair at the deepest lag"
    if not lost:
        assert not want["n_lost"].any(), want["n_lost"]


def same_state(env, models, tag):
    carry, seen = env.flow_state()
    P.same_array(carry, np.array([m.carry() for m in models], dtype=np.uint64), tag, "carry")
    P.same_array(seen, np.array([m.seen for m in models], dtype=np.uint64), tag, "cursor")


def per_book_flow(rng, n_b, tick, n_ids=7, unit=()):
    """test_gpu_accounts.busy_flow's recipe - side uniform, price U{45..55} x tick, volume U{1..5} or, with probability 0.2,
    U{50..199}, trader U{0..6} - with the number of new orders given per book; the orders of the books in `unit` all have
    volume 1.  Why not busy_flow itself: it gives every book 80..160 orders, so no fold of one to four records ever occurs,
    and its large orders sweep runs of small ones, so that the trade signs cluster and sum_ss at lag 1 came out positive in
    every one of the five books (+172 .. +307 over the seven steps) - `busy` (some sum_ss negative) would then refuse the case at K = 1.  A book whose orders
    all have volume 1 trades one record per crossing order: its signs do not cluster and its sum_ss takes both signs."""
    n = int(np.sum(n_b))
    vol = np.where(rng.random(n) < 0.2, rng.integers(50, 200, size=n), rng.integers(1, 6, size=n))
    for b in unit:
        vol[int(np.sum(n_b[:b])):int(np.sum(n_b[:b + 1]))] = 1
    return new_orders(list(n_b), rng.integers(0, 2, size=n), vol, rng.integers(0, n_ids, size=n), rng.integers(45, 56, size=n) * tick)


# ------------------------------------------------------------------------------------------------ 1. by hand
HAND_STAGES = [[(0, 10, 0, 100)], [(1, 4, 1, 100)], [(0, 3, 2, 105), (0, 2, 0, 102)], [(1, 11, 3, 105)], [], [(1, 5, 1, 90)],
               [(0, 3, 2, 0)], [(1, 2, 0, 95)], [(0, 2, 3, 95)]]  # (bid, vol, trader, price)


def test_rows_worked_out_by_hand(bk, oracle):
    """Book 0, tick 1, one stage per step (a step shuffles its events, so nothing here depends on the order inside one), K = 3:
      s0  trader 0 rests ask 10 @ 100
      s1  trader 1 bids 4 @ 100: a partial fill                         record 0: 4 @ 100, bought
      s2  trader 2 rests ask 3 @ 105, trader 0 rests ask 2 @ 102
      s3  trader 3 bids 11 @ 105: a SWEEP of three levels               records 1 - 3: 6 @ 100, 2 @ 102, 3 @ 105, bought
      s4  nothing at all
      s5  trader 1 rests bid 5 @ 90
      s6  trader 2 sells 3 at the market (price 0)                      record 4: 3 @ 90, sold
      s7  trader 0 rests bid 2 @ 95
      s8  trader 3 sells 2 @ 95                                         record 5: 2 @ 95, sold
    the tape of tests/test_flow_cpu.py::HAND, whose sums are worked out there pair by pair.  Book 1 is never touched."""
    import torch

    from test_flow_cpu import HAND, HAND_BASE, HAND_LAGS

    K = 3
    env = ingress_env(bk, torch, 2, len(HAND_STAGES), 64, 0, 8, tick=1, n_orders=32)
    env.enable_flow(K)
    books = Books(oracle, 2, 1, env, torch)
    after_s3 = None
    for s, rows in enumerate(HAND_STAGES):
        books.submit(*new_orders([len(rows), 0], *(zip(*rows) if rows else ([], [], [], []))))
        books.step()
        if s == 3:
            after_s3 = env.flow()
    env.sync()
    P.no_flags(env)
    assert tape_of(books.refs[0].book) == HAND and books.refs[1].book.n_trades() == 0
    want = FM.rows_of([[6, 4, 20, 15, 78, 1979, 6, 0, 5, 3, -15 & M64, 15, 25, 263, 4, 0, -15 & M64, 29, 29, 273,
                        3, -1 & M64, -12 & M64, 22, 22, 174], [0] * 26], K)
    assert want[0].tolist()[:8] == tuple(HAND_BASE) and want[0]["lags"].tolist() == HAND_LAGS
    busy(want[:1], K)
    got = env.flow()
    assert got.dtype == bk.flow_dtype(K) == env.flow_dtype() and got.shape == (2,)
    same_flow(got, want, "by hand")
    assert not got[1:].view(np.uint64).any()
    same_flow(FM.rows_of([whole(tape_of(r.book), K)[0] for r in books.refs], K), want, "the model over the oracle's trades")
    # after the sweep: four buys - lag 1 (0, 2, 3), lag 2 (2, 5), lag 3 (5)
    same_flow(after_s3, FM.rows_of([[4, 4, 15, 15, 65, 1519, 6, 0, 3, 3, 5, 5, 5, 13, 2, 2, 7, 7, 7, 29, 1, 1, 5, 5, 5, 25], [0] * 26], K),
              "by hand, after step 3")
    same_flow(env.flow(1, 1), want[1:], "flow(first_book, n_books)")
    carry, seen = env.flow_state()
    assert carry.tolist() == [[(1 << 63) | 95, (1 << 63) | 90, (3 << 62) | 105], [0, 0, 0]] and seen.tolist() == [6, 0]
    m = bk.flow_moments(got)
    assert m["buy_share"][0] == 4 / 6 and m["response"][0].tolist() == [-3.0, -3.75, -4.0] and np.isnan(m["buy_share"][1])
    env.fold_flow(sync=True)  # nothing new: nothing changes
    same_flow(env.flow(), want, "a fold without a new record")
    env.close()


# ------------------------------------------------------------------------------------------------ 2. after every step
@pytest.mark.parametrize("K", [1, 5, 64])
def test_rows_equal_the_model_after_every_step(bk, oracle, K):
    import torch

    B, T, tick = 5, 7, 2  # (5 books: the last block of four waves holds one)
    env = ingress_env(bk, torch, B, T, 256, 0, 256, tick=tick, n_ext=160)
    env.enable_flow(K)
    books = Books(oracle, B, tick, env, torch)
    rng = np.random.default_rng(7)
    models = [FM.FlowModel(K) for _ in range(B)]
    got, counts = [], []
    for s in range(T):
        n_b = rng.integers(80, 161, size=B)
        if s % 2:
            n_b[4] = 0   # an idle book-step
        if s == 3:
            n_b[1] = 3   # a fold of a few records
        if s == 5:
            n_b[2] = 30  # ... of fewer than 64
        books.submit(*per_book_flow(rng, n_b, tick, unit=(3,)))
        books.step()
        counts.append([r.book.n_trades() - n0 for r, n0 in zip(books.refs, books.last_trades)])
        for b, r in enumerate(books.refs):
            models[b].fold(tape_of(r.book), r.book.n_trades())
        got.append((env.flow(), FM.rows_of([m.words() for m in models], K)))
    flat = [n for step in counts for n in step]
    assert max(flat) > 128, max(flat)  # three chunks in one launch of one wave
    assert 0 in flat and any(0 < n < 5 for n in flat) and any(5 <= n < 64 for n in flat), counts
    busy(got[-1][1], K)
    P.no_flags(env)
    for s, (g, w) in enumerate(got):
        same_flow(g, w, f"K = {K}, after step {s}")
    same_state(env, models, f"K = {K}")
    for b in range(B):  # (consume_trades = 0: the host's readers see every record)
        assert env.trade_count(b) == (books.refs[b].book.n_trades(), 0), b
        P.same_trades(env, b, books.refs[b].book)
    env.close()


# ------------------------------------------------------------------------------------------------ 3. bk_run, every pipeline
@pytest.mark.parametrize("pipeline", PIPELINES)
def test_run_folded_after_every_step_in_sevens_and_once(bk, oracle, pipeline):
    B, T, K = 5, 18, 16
    ref = ref_books(oracle, B, 16, T, groups=C2)
    models = [FM.FlowModel(K) for _ in range(B)]
    for b, m in enumerate(models):
        m.fold(tape_of(ref.book(b)), ref.book(b).n_trades())
    want = FM.rows_of([m.words() for m in models], K)
    busy(want, K)
    seen = []
    for chunk in (1, 7, T):
        env = make_env(bk, B, groups=C2, levels=16, pool=64, steps=T)
        env.set_pipeline(pipeline)
        env.enable_flow(K)
        left = T
        while left:
            n = min(chunk, left)
            env.run(n, sync=False)
            env.fold_flow()
            left -= n
        env.sync()
        P.no_flags(env)
        seen.append((env.flow(),) + env.flow_state())
        same_flow(seen[-1][0], want, f"{pipeline}, folded every {chunk} steps")
        same_state(env, models, f"{pipeline}, folded every {chunk} steps")
        P.same_trades(env, B - 1, ref.book(B - 1))
        env.close()
    for rows, carry, cursor in seen[1:]:
        assert rows.tobytes() == seen[0][0].tobytes() and carry.tobytes() == seen[0][1].tobytes() and cursor.tobytes() == seen[0][2].tobytes()


# ------------------------------------------------------------------------------------------------ 4. members and markets
def test_noise_and_momentum_members_folded_in_sevens(bk, oracle):
    B, T, K = 5, 20, 6
    ref = ref_books(oracle, B, 10, T, members=MEMBERS, tick=1)
    want = FM.rows_of([whole(tape_of(ref.book(b)), K)[0] for b in range(B)], K)
    busy(want, K)
    env = make_env(bk, B, members=MEMBERS, levels=10, pool=256, steps=T, tick=1)
    env.enable_flow(K)
    for n in (7, 7, 6):
        env.run(n, sync=False)
        env.fold_flow()
    env.sync()
    P.no_flags(env)
    same_flow(env.flow(), want, "members")
    env.close()


MKT3_TICKS = [1, 2, 1]
MKT3_GROUPS = [(0, 40, (40, 56), (10, 20), 1, 0.8), (1, 30, (40, 56), (50, 70), 2, 0.5), (2, 30, (40, 56), (10, 30), 1, 0.7),
               (0, 20, (30, 70), (5, 9), 2, 0.3)]


def test_markets_keep_rows_per_book(bk, oracle):
    NM, A, T, K = 2, 3, 14, 8
    ref = oracle.ManyMarkets(NM, SEED, 0, MKT3_TICKS, STEP, True, 10, MKT3_GROUPS)
    ref.run(T)
    want = FM.rows_of([whole(tape_of(ref.book(m, a)), K)[0] for m in range(NM) for a in range(A)], K)
    busy(want, K)
    env = bk.ManyMarketEnv(NM, SEED, 0, MKT3_TICKS, STEP, True, levels=10, max_live_orders=128, trade_capacity=4096, history_capacity=T)
    env.set_random_market_agents(MKT3_GROUPS)
    env.enable_flow(K)
    env.run(9, sync=False)
    env.fold_flow()
    env.run(T - 9, sync=False)
    env.fold_flow(sync=True)
    P.no_flags(env)
    got = env.flow()
    assert got.shape == (NM * A,)
    same_flow(got, want, "markets")
    for m in range(NM):
        for a in range(A):
            assert env.book(m, a) == m * A + a
            P.same_trades(env, env.book(m, a), ref.book(m, a))
    env.close()


def test_members_beside_submitted_instructions(bk, oracle):
    import torch

    B, T, NX, K = 3, 8, 6, 4
    members = [("noise", 0, 30, dict(NOISE, p_limit=0.5, p_market=0.5))]
    env = members_env(bk, torch, B, T, 128, members, 1, n_ext=NX)
    env.set_agents(members)
    sets = [oracle.AgentSet(members) for _ in range(B)]
    env.enable_flow(K)
    books = Books(oracle, B, 1, env, torch)
    rng = np.random.default_rng(3)
    for _ in range(T):
        env.update_members(sync=False)
        for b in range(B):
            sets[b].update(books.refs[b])
        books.submit(*external(rng, B, NX))
        books.step()
    want = FM.rows_of([whole(tape_of(r.book), K)[0] for r in books.refs], K)
    busy(want, K)
    P.no_flags(env)
    same_flow(env.flow(), want, "members beside instructions")
    for b in range(B):
        P.same_trades(env, b, books.refs[b].book)
    env.close()


# ------------------------------------------------------------------------------------------------ 5. lost records
def test_dropped_records_are_counted_flagged_and_shift_no_lag(bk, oracle):
    """trade_capacity = 16 and a consuming table: a book-step of more than 16 records drops its tail - counted in n_lost,
    flagged TRADE_OVERFLOW on that book alone - and the next step's records are read again, so a pair across a short gap
    counts at its true lag."""
    import torch

    B, T, tick, K, cap = 3, 8, 2, 8, 16
    rng = np.random.default_rng(19)
    flows = [per_book_flow(rng, [int(rng.integers(18, 60)), 6, 5], tick) for _ in range(T)]  # book 0 trades a lot, the others a little
    plan = Tape(oracle, B, tick)
    for f in flows:
        plan.submit(*f)
        plan.step()
    over = [[max(0, n - cap) for n in c] for c in plan.counts]
    assert any(0 < g < K and n_next > 0 for g, n_next in zip(over[0], plan.counts[0][1:])), over[0]  # a short gap with records behind it
    assert any(g >= K for g in over[0]) and not any(over[1]) and not any(over[2]) and sum(plan.counts[1]) > K, (over, plan.counts)
    models = [FM.FlowModel(K) for _ in range(B)]
    uncut = []
    for b, r in enumerate(plan.refs):
        tp, total = tape_of(r.book), 0
        for n in plan.counts[b]:
            models[b].fold(tp, total + n, total, cap)  # (the fold before consumed up to `total`)
            total += n
        uncut.append(whole(tp, K)[0])
    want = FM.rows_of([m.words() for m in models], K)
    assert want["n_lost"].tolist() == [sum(over[0]), 0, 0] and want["n_lost"][0] > 0
    assert models[0].words() != uncut[0] and models[1].words() == uncut[1]
    env = bk.ManyBookEnv(B, SEED, 0, tick, STEP, levels=10, max_live_orders=256, max_orders=64 * T + 16, trade_capacity=cap,
                         history_capacity=T, strict=False, stream=torch.cuda.current_stream().cuda_stream)
    env.enable_device_ingress(queue_capacity=128)
    env.enable_flow(K, consume_trades=True)
    tape = Tape(oracle, B, tick, env, torch)
    for f in flows:
        tape.submit(*f)
        tape.step()
    env.sync()
    flags = env.flags()
    assert flags[0] == TRADE_OVERFLOW and not flags[1:].any(), flags
    same_flow(env.flow(), want, "dropped records")
    same_state(env, models, "dropped records")
    for b in range(B):
        n = tape.refs[b].book.n_trades()
        assert env.trade_count(b) == (n, n), b
    env.close()


def test_records_cleared_before_the_fold_are_counted_as_lost(bk, oracle):
    """run(4), fold, run(1), clear_trades(), run(3), fold: the records of step 4 were consumed before the table saw them - a
    gap below K in one book and of at least K in another."""
    B, K = 5, 15
    at4, at5, at8 = (ref_books(oracle, B, 16, L, groups=C2) for L in (4, 5, 8))
    c4, c5, c8 = ([int(x) for x in r.trade_counts()] for r in (at4, at5, at8))
    gaps = [b - a for a, b in zip(c4, c5)]
    assert any(0 < g < K for g in gaps) and any(g >= K for g in gaps), gaps
    models = [FM.FlowModel(K) for _ in range(B)]
    for b, m in enumerate(models):
        tp = tape_of(at8.book(b))
        m.fold(tp, c4[b])
        m.fold(tp, c8[b], c5[b])
    want = FM.rows_of([m.words() for m in models], K)
    assert want["n_lost"].tolist() == gaps
    busy(want, K, lost=True)
    env = make_env(bk, B, groups=C2, levels=16, pool=64, steps=8)
    env.enable_flow(K)
    env.run(4, sync=False)
    env.fold_flow()
    env.run(1, sync=False)
    env.clear_trades()
    env.run(3, sync=False)
    env.fold_flow(sync=True)
    P.no_flags(env)
    same_flow(env.flow(), want, "cleared before the fold")
    same_state(env, models, "cleared before the fold")
    env.close()


# ------------------------------------------------------------------------------------------------ 6. consume
def test_a_consuming_table_needs_room_for_one_chunk(bk, oracle):
    B, K, c, chunks = 5, 16, 2, 10
    counts = [[int(x) for x in ref_books(oracle, B, 16, L, groups=C2).trade_counts()] for L in range(0, c * chunks + 1, c)]
    cap = max(b - a for lo, hi in zip(counts, counts[1:]) for a, b in zip(lo, hi))
    ref = ref_books(oracle, B, 16, c * chunks, groups=C2)
    assert min(counts[-1]) > 3 * cap, (counts[-1], cap)
    want = FM.rows_of([whole(tape_of(ref.book(b)), K)[0] for b in range(B)], K)
    busy(want, K)
    env = make_env(bk, B, groups=C2, levels=16, pool=64, steps=c, trade_capacity=cap)
    env.enable_flow(K, consume_trades=True)
    env.run_series(c * chunks, chunk=c)
    env.sync()
    P.no_flags(env)
    same_flow(env.flow(), want, "run_series, consuming")
    for b in range(B):
        assert env.trade_count(b) == (counts[-1][b], counts[-1][b]), b
    env.close()


def test_flow_bars_and_accounts_on_one_env_consume_once(bk, oracle):
    """All three folds read the same records - the flow's first, then the bars', then the accounts' - and with consumption
    asked for by the FLOW alone the last fold of the step consumes for all, so trade_capacity holds one step's trades."""
    import torch

    B, T, tick, NT, K = 3, 6, 2, 5, 12
    rng = np.random.default_rng(40)
    flows = [per_book_flow(rng, rng.integers(150, 161, size=B), tick, unit=(1,)) for s in range(T)]
    plan = Tape(oracle, B, tick)
    for f in flows:
        plan.submit(*f)
        plan.step()
    cap = max(max(c) for c in plan.counts)  # exactly the busiest book-step
    assert min(r.book.n_trades() for r in plan.refs) > 2 * cap
    n_orders = 160 * T + 16
    env = bk.ManyBookEnv(B, SEED, 0, tick, STEP, levels=10, max_live_orders=512, max_orders=n_orders, trade_capacity=cap,
                         history_capacity=T, stream=torch.cuda.current_stream().cuda_stream)
    env.enable_device_ingress(queue_capacity=256)
    env.enable_accounts(NT)
    env.enable_trade_bars(T)
    env.enable_flow(K, consume_trades=True)
    tape = Tape(oracle, B, tick, env, torch)
    for f in flows:
        tape.submit(*f)
        tape.step()
        for b in range(B):
            n = tape.refs[b].book.n_trades()
            assert env.trade_count(b) == (n, n), (b, env.trade_count(b), n)
    P.no_flags(env)
    want = FM.rows_of([whole(tape_of(r.book), K)[0] for r in tape.refs], K)
    busy(want, K)
    got, bars = env.flow(), env.trade_bars()
    same_flow(got, want, "flow beside bars and accounts")
    same_bars(bars, tape.bars(T), "bars beside the flow")
    same_accounts(env.accounts(), tape.want(NT), "accounts beside the flow")
    # the siblings agree: the bars of all steps sum to the flow's buy words
    P.same_array(bars["n_buy"].sum(axis=1, dtype=np.uint64), got["n_buy"], "bars against flow", "n_buy")
    P.same_array(bars["buy_vol"].sum(axis=1, dtype=np.uint64), got["buy_vol"], "bars against flow", "buy_vol")
    P.same_array((bars["n_buy"] + bars["n_sell"]).sum(axis=1, dtype=np.uint64), got["n_trades"], "bars against flow", "n_trades")
    env.close()


# ------------------------------------------------------------------------------------------------ 7. resets and clears
@pytest.mark.parametrize("kind", ["host", "device"])
def test_reset_books_cuts_the_books_it_resets(bk, oracle, kind):
    B, K, (n, m, k) = 5, 8, (6, 5, 7)
    long_, before, after = (ref_books(oracle, B, 16, L, groups=C2) for L in (n + m + k, n + m, n + k))
    c_n = [int(x) for x in ref_books(oracle, B, 16, n, groups=C2).trade_counts()]
    for name in ("alternate", "all", "none"):
        mask = make_mask(name, B)
        models = []
        for b in range(B):
            md = FM.FlowModel(K)
            if mask[b]:  # the old episode up to the reset, the cut at the snapshot's count, the new episode from there
                md.fold(tape_of(before.book(b)), before.book(b).n_trades())
                md.cut(c_n[b])
                md.fold(tape_of(after.book(b)), after.book(b).n_trades())
                joined = whole(tape_of(before.book(b)) + tape_of(after.book(b))[c_n[b]:], K)[0]
                assert md.words() != joined, f"a cut would not show in book {b}"
            else:
                md.fold(tape_of(long_.book(b)), long_.book(b).n_trades())
            models.append(md)
        want = FM.rows_of([md.words() for md in models], K)
        busy(want, K)
        env = make_env(bk, B, groups=C2, levels=16, pool=64, steps=n + m + k, kind=kind)
        env.enable_flow(K)
        env.run(n)
        env.save_snapshot()
        env.run(m)  # (not folded: the reset folds what is outstanding)
        do_reset(env, mask, kind)
        env.run(k)
        env.fold_flow(sync=True)
        P.no_flags(env)
        same_flow(env.flow(), want, f"reset_books ({kind}, {name})")
        same_state(env, models, f"reset_books ({kind}, {name})")
        env.close()


def test_reset_ingress_books_cuts_and_the_sums_go_on(bk, oracle):
    """3 steps, save, 3 steps, reset books 0 and 2 (a torch CUDA mask), 2 steps.  The oracle cannot be rewound, so a reset
    book's new episode is a REPLAY: a fresh oracle env given steps 0..2 again and then the two steps after the reset."""
    import torch

    B, tick, K = 4, 2, 6
    env = ingress_env(bk, torch, B, 8, 256, 0, 64, tick=tick, n_ext=40)
    env.enable_flow(K)
    books = Books(oracle, B, tick, env, torch)
    rng = np.random.default_rng(60)
    flows = [per_book_flow(rng, rng.integers(30, 41, size=B), tick, unit=(2, 3)) for s in range(8)]

    def run(lo, hi, bs=books):
        for f in flows[lo:hi]:
            bs.submit(*f)
            bs.step()

    run(0, 3)
    env.save_ingress_snapshot()
    snap = [r.book.n_trades() for r in books.refs]
    run(3, 6)
    at_reset = [r.book.n_trades() for r in books.refs]
    before = env.flow()
    mask = np.array([1, 0, 1, 0], dtype=bool)
    env.reset_ingress_books(torch.tensor(mask, device="cuda"), sync=False)
    same_flow(env.flow(), before, "a reset changes no sum")
    carry, seen = env.flow_state()
    assert not carry[mask].any() and carry[~mask].all() and seen.tolist() == [snap[b] if mask[b] else at_reset[b] for b in range(B)]
    run(6, 8)
    replay = Books(oracle, B, tick)
    run(0, 3, replay)
    assert [r.book.n_trades() for r in replay.refs] == snap
    run(6, 8, replay)
    models = []
    for b in range(B):
        md = FM.FlowModel(K)
        if mask[b]:
            md.fold(tape_of(books.refs[b].book), at_reset[b])
            md.cut(snap[b])
            md.fold(tape_of(replay.refs[b].book), replay.refs[b].book.n_trades())
            assert replay.refs[b].book.n_trades() > snap[b] + K
        else:
            md.fold(tape_of(books.refs[b].book), books.refs[b].book.n_trades())
        models.append(md)
    want = FM.rows_of([md.words() for md in models], K)
    busy(want, K)
    P.no_flags(env)
    same_flow(env.flow(), want, "reset_ingress_books")
    same_state(env, models, "reset_ingress_books")
    env.close()


def test_restore_clears_and_rebases_and_warm_changes_nothing(bk, oracle):
    B, K = 5, 8
    at5, at9 = (ref_books(oracle, B, 16, L, groups=C2) for L in (5, 9))
    c5 = [int(x) for x in at5.trade_counts()]
    env = make_env(bk, B, groups=C2, levels=16, pool=64, steps=9)
    env.enable_flow(K)
    env.run(5)
    img = env.checkpoint()
    env.fold_flow(sync=True)
    rows, (carry, seen) = env.flow(), env.flow_state()
    same_flow(rows, FM.rows_of([whole(tape_of(at5.book(b)), K)[0] for b in range(B)], K), "before warm")
    env.warm(6)
    env.sync()
    assert env.flow().tobytes() == rows.tobytes() and env.flow_state()[0].tobytes() == carry.tobytes()
    assert env.flow_state()[1].tolist() == seen.tolist() == c5
    env.fold_flow(sync=True)  # (and the scratch steps left no record behind)
    assert env.flow().tobytes() == rows.tobytes()
    env.run(4)
    env.fold_flow(sync=True)
    full = FM.rows_of([whole(tape_of(at9.book(b)), K)[0] for b in range(B)], K)
    busy(full, K)
    same_flow(env.flow(), full, "after warm")
    # back to step 5: zero rows, an invalid carry, the cursors at the restored counts; then steps 5 .. 8 alone
    env.restore(img)
    carry, seen = env.flow_state()
    assert not env.flow().view(np.uint64).any() and not carry.any() and seen.tolist() == c5
    env.run(4)
    env.fold_flow(sync=True)
    models = [FM.FlowModel(K, c5[b]) for b in range(B)]
    for b, md in enumerate(models):
        md.fold(tape_of(at9.book(b)), at9.book(b).n_trades())
    want = FM.rows_of([md.words() for md in models], K)
    busy(want, K)
    assert (want["n_trades"] < full["n_trades"]).all()
    P.no_flags(env)
    same_flow(env.flow(), want, "after restore")
    same_state(env, models, "after restore")
    env.close()


@pytest.mark.parametrize("kind", ["host", "device", "all"])
def test_a_masked_clear_folds_first_and_counts_the_next_records_only(bk, oracle, kind):
    B, K = 5, 8
    at6, at12 = (ref_books(oracle, B, 16, L, groups=C2) for L in (6, 12))
    c6 = [int(x) for x in at6.trade_counts()]
    mask = np.ones(B, dtype=bool) if kind == "all" else np.array([0, 1, 1, 0, 1], dtype=bool)
    env = make_env(bk, B, groups=C2, levels=16, pool=64, steps=12, kind="device" if kind == "device" else "host")
    env.enable_flow(K)
    env.run(6)
    if kind == "all":
        env.clear_flow()
    else:
        env.clear_flow(as_kind(mask, kind)[0], sync=(kind == "host"))
    now = env.flow()
    assert not now[mask].view(np.uint64).any()
    if kind != "all":  # the masked clear folded first: the other books hold steps 0 .. 5
        same_flow(now[~mask], FM.rows_of([whole(tape_of(at6.book(b)), K)[0] for b in np.flatnonzero(~mask)], K), "the unmasked rows")
    env.run(6)
    env.fold_flow(sync=True)
    models = [FM.FlowModel(K, c6[b] if mask[b] else 0) for b in range(B)]
    for b, md in enumerate(models):
        md.fold(tape_of(at12.book(b)), at12.book(b).n_trades())
    want = FM.rows_of([md.words() for md in models], K)
    busy(want, K)
    P.no_flags(env)
    same_flow(env.flow(), want, f"clear_flow ({kind})")
    same_state(env, models, f"clear_flow ({kind})")
    env.close()


# ------------------------------------------------------------------------------------------------ 8. refusals
def _refused(bk, call, match):
    with pytest.raises(bk.BourseError, match=match) as e:
        call()
    assert e.value.code == BK_INVALID_ARGUMENT


def test_refusals_leave_the_env_working(bk, oracle):
    B, K = 5, 4
    ref = ref_books(oracle, B, 16, 6, groups=C2)
    c3 = [int(x) for x in ref_books(oracle, B, 16, 3, groups=C2).trade_counts()]
    # without trade records
    env = make_env(bk, B, groups=C2, levels=16, pool=64, steps=6, trade_capacity=0, strict=False)  # (every trade is dropped)
    _refused(bk, lambda: env.enable_flow(K), "trade_capacity")
    env.run(2)
    assert env.steps_done() == 2
    env.close()
    env = make_env(bk, B, groups=C2, levels=16, pool=64, steps=6)
    for call in (env.flow, env.fold_flow, env.flow_device_ptr, env.flow_view, env.clear_flow, env.flow_state):
        _refused(bk, call, "no flow table")
    n = np.zeros(1, dtype=np.uint32)
    for call, args in ((env._L.bk_get_flow, [0, 0, None]), (env._L.bk_flow_clear, [None]), (env._L.bk_flow_clear_device, [None]),
                       (env._L.bk_flow_fold, []), (env._L.bk_flow_lags, [n.ctypes.data_as(env._L.bk_flow_lags.argtypes[1])])):
        assert call(env._h, *args) == BK_INVALID_ARGUMENT and b"no flow table" in env._L.bk_last_error()
    _refused(bk, lambda: env.enable_flow(0), "n_lags")
    _refused(bk, lambda: env.enable_flow(65), "n_lags")
    env.run(3)
    env.enable_flow(K)  # mid-run: the records so far are not counted
    assert env._L.bk_flow_lags(env._h, n.ctypes.data_as(env._L.bk_flow_lags.argtypes[1])) == 0 and n[0] == K
    _refused(bk, lambda: env.enable_flow(K), "already enabled")
    assert not env.flow().view(np.uint64).any() and env.flow_state()[1].tolist() == c3
    rc = env._L.bk_load_book(env._h, 0, 0, 0, 0, None, None, None, 0, None)
    assert rc == BK_INVALID_ARGUMENT and b"flow table" in env._L.bk_last_error()
    env.run(3)
    env.fold_flow(sync=True)
    want = FM.rows_of([whole(tape_of(ref.book(b)), K, start=c3[b])[0] for b in range(B)], K)
    busy(want, K)
    P.no_flags(env)
    same_flow(env.flow(), want, "after the refusals")
    env.close()


# ------------------------------------------------------------------------------------------------ 9. the device view
def test_the_device_view_is_the_table_in_place(bk, oracle):
    import torch

    B, K = 5, 4
    env = make_env(bk, B, groups=C2, levels=16, pool=64, steps=8, kind="device")
    env.enable_flow(K)
    view = env.flow_view()
    cai = view.__cuda_array_interface__
    assert cai["shape"] == (B, 8 + 6 * K) and cai["typestr"] == "<i8" and cai["version"] == 3 and cai["strides"] is None
    t = torch.as_tensor(view, device="cuda")
    assert t.dtype == torch.int64 and tuple(t.shape) == (B, 8 + 6 * K) and t.is_contiguous()
    assert env.flow_device_ptr() == t.data_ptr() == cai["data"][0]
    assert not t.any().item()
    env.run(4, sync=False)
    env.fold_flow()
    first = t.clone()  # queued on the same stream, behind the fold
    env.run(4, sync=False)
    env.fold_flow()
    torch.cuda.current_stream().synchronize()
    rows = env.flow()
    at4, at8 = (ref_books(oracle, B, 16, L, groups=C2) for L in (4, 8))
    for tensor, ref, tag in ((first, at4, "the clone after the first fold"), (t, at8, "the view after the second")):
        want = FM.rows_of([whole(tape_of(ref.book(b)), K)[0] for b in range(B)], K)
        P.same_array(tensor.cpu().numpy().view(np.uint64), want.view(np.uint64).reshape(B, -1), "device view", tag)
    same_flow(rows, want, "flow() beside the view")
    env.close()


# ------------------------------------------------------------------------------------------------ 10. range
def test_volumes_and_prices_of_four_billion_wrap_as_the_model_does(bk, oracle):
    import torch

    V = 4_000_000_000
    stages = [[(0, V, 0, V), (0, V, 2, V)], [(1, V, 3, V), (1, V, 1, V)], [(1, 5, 1, 1)], [(0, 5, 2, 0)], [(0, V, 0, V)], [(1, V, 3, V)]]
    K = 2
    env = ingress_env(bk, torch, 2, len(stages), 64, 0, 8, tick=1, n_orders=32)
    env.enable_flow(K)
    books = Books(oracle, 2, 1, env, torch)
    for rows in stages:
        n = len(rows)
        books.submit(*new_orders([n, n], *zip(*(rows + rows))))
        books.step()
    tp = tape_of(books.refs[0].book)
    assert tp == [(V, V, 0), (V, V, 0), (1, 5, 1), (V, V, 0)] == tape_of(books.refs[1].book)
    want = FM.rows_of([whole(tp, K)[0]] * 2, K)
    d = V - 1
    assert 3 * V * V > M64 and 2 * d * d > M64 and 3 * V > 1 << 32
    assert want[0].tolist()[:8] == (4, 3, 3 * V + 5, 3 * V, (3 * V * V + 25) & M64, (3 * V * V + 5) & M64, V, 0)
    # lag 1: (1, 0) dp 0; (2, 1) dp -d at a sell behind a buy; (3, 2) dp +d at a buy behind a sell.  lag 2: (2, 0) -d; (3, 1) 0
    assert want[0]["lags"].view(np.uint64).tolist() == [[3, -1 & M64, -2 * d & M64, 2 * d, 2 * d, (2 * d * d) & M64],
                                                        [2, 0, -d & M64, d, d, d * d]]
    P.no_flags(env)
    same_flow(env.flow(), want, "four billion")
    env.close()


def test_the_cursor_and_the_table_continue_past_2_to_the_32(bk, oracle):
    """5 steps, a checkpoint whose trade counters are moved (tests/counter_shift.py) so that every book's H_TRADES carries
    into its high word within the next steps, a restore - which rebases the cursors - and 6 steps more, folded twice."""
    B, K, pool = 5, 8, 64
    at5, at8, at11 = (ref_books(oracle, B, 16, L, groups=C2) for L in (5, 8, 11))
    c5, c8, c11 = ([int(x) for x in r.trade_counts()] for r in (at5, at8, at11))
    off = [(1 << 32) - (a + b) // 2 for a, b in zip(c5, c11)]  # the carry falls in the middle of the six steps
    assert all((c5[b] + off[b]) >> 32 == 0 and (c11[b] + off[b]) >> 32 == 1 for b in range(B))
    env = make_env(bk, B, groups=C2, levels=16, pool=pool, steps=11)
    env.enable_flow(K)
    env.run(5)
    env.restore(CS.shift(env.checkpoint(), B, pool, trades=off))
    assert env.flow_state()[1].tolist() == [c5[b] + off[b] for b in range(B)]
    env.run(3, sync=False)
    env.fold_flow()
    env.run(3, sync=False)
    env.fold_flow(sync=True)
    models = [FM.FlowModel(K, c5[b]) for b in range(B)]
    for b, md in enumerate(models):
        md.fold(tape_of(at11.book(b)), c8[b])
        md.fold(tape_of(at11.book(b)), c11[b])
    want = FM.rows_of([md.words() for md in models], K)
    busy(want, K)
    P.no_flags(env)
    same_flow(env.flow(), want, "past 2^32")
    carry, seen = env.flow_state()
    P.same_array(carry, np.array([md.carry() for md in models], dtype=np.uint64), "past 2^32", "carry")
    assert seen.tolist() == [c11[b] + off[b] for b in range(B)] and min(seen.tolist()) > 1 << 32
    for b in range(B):
        assert env.trade_count(b) == (c11[b] + off[b], c5[b] + off[b]), b
    env.close()
