"""Books whose counters pass 2^32: the u32 arrival stamps (H_SEQ, pool field 3) and the 64-bit counters kept as two header
words (H_TRADES / H_TRADE_BASE, H_EVENTS, H_STEPS and the env's steps_done).

STAMPS.  Time priority inside a price level is "smaller stamp first", compared raw by the event-by-event loop
(book_device.hpp match_side and its assembly twin), the queue view (open_queue_rows.hpp place) and bk_live_orders; the keyed
loops work with wrapping differences.  A level that holds one order stamped just below 2^32 and one stamped just above 0
would trade youngest first on one loop and oldest first on the other.  The library keeps that from happening off the hot
path: live stamps never straddle a wrap, because the host queues the stamp compaction (stamp_rows.hpp: every live stamp
becomes its rank) in front of a launch that could take H_SEQ past 2^32 - 1.  BOURSE_AMD_SEQ_START starts every fresh book's
counter next to the wrap, BOURSE_AMD_STAMP_ROOM shrinks the room so that the compaction runs every few steps; every case is
bit for bit the oracle's, whose priority is the (price, time) key and knows no stamp.

Each case says something only under conditions that are counted on the expected side (the oracle's order log, replayed)
and asserted before anything is compared: which loop a step took (a), how many books' counters wrapped (b), the rows of the
straddling levels (c), the share of wide-span steps and the number of straddling ties (d), the carries crossed (e).

COUNTERS.  tests/counter_shift.py moves a checkpoint image's counters next to the carry into their high words; the
restored env must go on exactly as the oracle's later steps, in every reader."""
import numpy as np
import pytest

import counter_shift as CS
import open_orders_model as OM
import oracle_parity as P
import test_gpu_keyed_events as KE
import test_gpu_reset_books as RB

pytestmark = pytest.mark.gpu

M32 = 1 << 32
KEY_PSPAN = 32_762  # book_device.hpp: the price span a key window holds
STEP = 100_000


@pytest.fixture(scope="module")
def bk():
    import bourse_amd

    return bourse_amd


# ============================================================================================== the oracle's order log
def rests_of(view):
    """The orders of an oracle book that rested, in the order they did: (ids, key time, end time, price, side).  An order
    that never rested (filled on arrival, a market order) keeps the provisional key time 0 (orderbook.rs:388-391); RandomAgents
    and the hand-made flows here never modify, so an order rests at most once.  Needs start_time > 0."""
    o = view.orders_array()
    kt = view.keys()[2]
    ids = np.flatnonzero(kt != 0)
    ids = ids[np.argsort(kt[ids], kind="stable")]
    return ids, kt[ids].astype(np.uint64), o["end_time"][ids], o["price"][ids], o["side"][ids]


def straddling_ties(view, seq_start, wide_steps=None, start_time=0):
    """(trades whose passive order's level, when the aggressor arrived, also held an order from the other side of the
    book's wrap; how many of them on a step in ``wide_steps``; the step the counter wrapped at, or None).  The k-th order to
    rest carries stamp seq_start + k."""
    ids, kt, end, price, side = rests_of(view)
    past = (seq_start + np.arange(len(ids), dtype=np.int64)) >= M32
    if not past.any():
        return 0, 0, None
    wrap_step = int((int(kt[np.argmax(past)]) - start_time) // STEP)
    at = {int(i): k for k, i in enumerate(ids)}
    ties = wide = 0
    for t, pas in zip(view.trades_array()["t"], view.trades_array()["passive_id"]):
        k = at[int(pas)]
        level = (price == price[k]) & (side == side[k]) & (kt < t) & (end >= t)
        if (past[level] != past[k]).any():
            ties += 1
            wide += wide_steps is not None and int((int(t) - start_time) // STEP) in wide_steps
    return ties, wide, wrap_step


def wide_span_steps(view, n_steps, start_time=0):
    """the steps at whose start the book's resting prices span more than a key window"""
    _, kt, end, price, _ = rests_of(view)
    out = set()
    for s in range(n_steps):
        t0 = start_time + s * STEP
        live = (kt < t0) & (end >= t0)
        if live.any() and int(price[live].max()) - int(price[live].min()) > KEY_PSPAN:
            out.add(s)
    return out


# ============================================================================================== a. host-driven, by hand
# One real order per step (a step shuffles its events): ids 0 .. 7 rest with stamps 2^32 - 5 .. 2, so ids 0 - 4 lie below the
# wrap and ids 5 - 7 above it.  Bids at 100 hold ids 0 and 5, bids at 99 ids 1 and 6, asks at 102 ids 2 and 7 - three
# straddling levels - and asks at 103 ids 3 and 4 (stamps 2^32 - 2 and 2^32 - 1).  Then one aggressor per step eats a level
# in full, oldest first; the last one fills id 3 in part, and id 3 is cancelled.
HAND_RESTS = [(True, 100), (True, 99), (False, 102), (False, 103), (False, 103), (True, 100), (True, 99), (False, 102)]
HAND_VOLS = [3, 4, 5, 6, 7, 8, 9, 10]
# (aggressor: bid, price, volume), then the passive ids it trades with, in order
HAND_AGGRESSORS = [((False, 100, 3 + 8), [0, 5]), ((False, 99, 4 + 9), [1, 6]), ((True, 102, 5 + 10), [2, 7]), ((True, 103, 2), [3])]
HAND_PASSIVE_IDS = [0, 5, 1, 6, 2, 7, 3]
SEQ_START_HAND = M32 - 5


def _hand_calls(book):
    """the real calls of one book, one list per step: its volumes are the table's times book + 1"""
    m = book + 1
    steps = [[("place_order", bid, HAND_VOLS[i] * m, 10 + i, price)] for i, (bid, price) in enumerate(HAND_RESTS)]
    steps += [[("place_order", bid, vol * m, 20, price)] for (bid, price, vol), _ in HAND_AGGRESSORS]
    steps += [[("cancel_order", 3)]]
    return steps


@pytest.mark.parametrize("pool", [64, 128, 256, 512])
def test_a_level_across_the_wrap_trades_oldest_first_on_both_loops(bk, oracle, monkeypatch, pool):
    monkeypatch.setenv("BOURSE_AMD_SEQ_START", str(SEQ_START_HAND))
    B, T = 3, len(_hand_calls(0))
    for zero in (True, False):  # with one zero-volume market order per step: event by event; without: keyed
        env = bk.ManyBookEnv(B, 41, 0, 1, STEP, levels=10, max_live_orders=pool, max_orders=64, trade_capacity=64, history_capacity=T)
        refs = [oracle.StepEnv(41 + b, 0, 1, STEP) for b in range(B)]
        real = [[] for _ in range(B)]  # the ids of the real orders, in the order of the table
        for s in range(T):
            before = env.event_steps_keyed().copy()
            for b in range(B):
                for f, *args in _hand_calls(b)[s]:
                    if f == "cancel_order":
                        args = [real[b][args[0]]]
                    got = getattr(env, f)(b, *args)
                    want = getattr(refs[b], f)(*args)
                    if f == "place_order":
                        assert got == want
                        real[b].append(got)
                if zero:
                    assert env.place_order(b, bool(s & 1), 0, 30, None) == refs[b].place_order(bool(s & 1), 0, 30, None)
            env.step()
            for r in refs:
                r.step()
            moved = env.event_steps_keyed() - before
            assert moved.tolist() == [0 if zero else 1] * B, (s, zero, moved)
            for b in range(B):
                P.same_live(env, b, refs[b].book, tag=(b, f"live orders after step {s}", zero))
        P.no_flags(env)
        hist = env.history()
        for b in range(B):
            P.same_history(hist[:, b], refs[b].history(), f"L2 history of book {b}")
            P.same_book(env, b, refs[b].book, orders=True, keys=True)
            want_passive = [real[b][i] for i in HAND_PASSIVE_IDS]
            assert real[b][:8] == ([0, 2, 4, 6, 8, 10, 12, 14] if zero else list(range(8)))
            got = env.trades(b, first=0)
            assert got["passive_id"].tolist() == want_passive, (b, zero, got["passive_id"].tolist())
            assert got["vol"].tolist() == [v * (b + 1) for v in (3, 8, 4, 9, 5, 10, 2)]
            # what is left: id 4 alone at 103 (id 3 was cancelled after its partial fill)
            live = env.live_orders(b)
            assert live["order_id"].tolist() == [real[b][4]] and live["vol"].tolist() == [7 * (b + 1)]
        env.close()


def test_the_hand_made_levels_straddle_the_wrap():
    """the stamps the table implies, without a device: ids 0 - 4 below 2^32, ids 5 - 7 past it, three levels hold both"""
    stamps = [(SEQ_START_HAND + k) % M32 for k in range(8)]
    assert stamps == [M32 - 5, M32 - 4, M32 - 3, M32 - 2, M32 - 1, 0, 1, 2]
    levels = {}
    for k, key in enumerate(HAND_RESTS):
        levels.setdefault(key, []).append(stamps[k])
    straddle = [key for key, s in levels.items() if max(s) - min(s) > M32 // 2]
    assert sorted(straddle) == [(False, 102), (True, 99), (True, 100)] and len(levels) == 4
    # raw stamp order would put the younger order first on each of them
    for key in straddle:
        assert levels[key] != sorted(levels[key])
    assert [i for _, ids in HAND_AGGRESSORS for i in ids] == HAND_PASSIVE_IDS


# ============================================================================================== b. host-driven, random
ROOMS = {"shipped room": None, "room 300": "300"}
DRIVE = {64: (12, 0.004), 256: (44, 0.04)}  # pool: (n_max, p_market) as test_gpu_keyed_events drives these pools


def _set_room(monkeypatch, room):
    if ROOMS[room]:
        monkeypatch.setenv("BOURSE_AMD_STAMP_ROOM", ROOMS[room])


@pytest.mark.parametrize("room", list(ROOMS))
@pytest.mark.parametrize("pool", list(DRIVE))
def test_random_host_streams_wrap_mid_run_on_alternating_loops(bk, oracle, monkeypatch, pool, room):
    """test_gpu_keyed_events._drive's stream with volumes of 0 (those steps run event by event), every book's counter
    starting 2 n_max + 1 below 2^32: a step hands out at most one stamp per event and has at most 2 n_max events, so no book
    wraps in step 0; every book has rested more orders than that by the end (counted in the oracle's log: an order that
    rested at all took at least one stamp), so every book wraps mid-run."""
    n_max, p_market = DRIVE[pool]
    B, T, w = 16, 25, 2 * n_max + 1
    monkeypatch.setenv("BOURSE_AMD_SEQ_START", str(M32 - w))
    _set_room(monkeypatch, room)
    env, refs, busy, clean = KE._drive(bk, oracle, pool, n_max, B, T, 900 + pool, p_market, p_mod=0.05, p_zero=0.03)
    rested = [int((r.book.keys()[2] != 0).sum()) for r in refs]
    assert min(rested) > w, (min(rested), w)
    keyed = env.event_steps_keyed()
    assert np.all(keyed <= clean.sum(axis=0)), "a step with a volume of 0 ran keyed"
    assert 0.25 * busy.sum() < clean.sum() < busy.sum(), "the stream should mix both kinds of step"
    assert 0 < keyed.sum() < busy.sum()
    KE._same_as_oracle(env, refs)
    for b, r in enumerate(refs):
        P.same_keys(env, b, r.book)
    if ROOMS[room]:
        assert env.stamp_compactions() >= 2, env.stamp_compactions()
    env.close()


# ============================================================================================== c. device ingress, queue view
@pytest.mark.parametrize("room", list(ROOMS))
@pytest.mark.parametrize("pool", [64, 256])
def test_the_queue_view_of_levels_across_the_wrap(bk, oracle, monkeypatch, pool, room):
    """The scenario of (a) through submit_instructions_device, traders 0 and 1 listed: after every step the open-order rows
    and the queue rows are the models' over the oracle's book - tests/open_queue_model.py ranks a level by the oracle's key
    times, the arrival order, and never sees a stamp."""
    import torch

    import test_gpu_open_queue as OQ
    from ingress_support import ingress_env
    from test_gpu_open_orders import instructions, new

    monkeypatch.setenv("BOURSE_AMD_SEQ_START", str(SEQ_START_HAND))
    _set_room(monkeypatch, room)
    B, NT, depth = 3, 2, 8
    plan = OQ.QueuePlan(oracle, B, 1, NT, depth)
    calls = [_hand_calls(b) for b in range(B)]
    T = len(calls[0])
    after_rests = None
    for s in range(T):
        per_book = []
        for b in range(B):
            rows = []
            for f, *args in calls[b][s]:
                if f == "place_order":
                    bid, vol, trader, price = args
                    rows.append(new(bid, vol, trader % 2 if trader < 20 else 9, price))  # (the aggressors' trader has no row)
                else:
                    rows.append((2, 0, 0, 0, 0, args[0]))
            per_book.append(rows)
        queue = plan.step(*instructions(per_book))
        if s == 7:
            after_rests = queue
            entries = [OM.rows_ints(r.book.orders_array(), NT, depth)[1] for r in plan.refs]
    # the condition, on the expected side: with all eight orders resting, the younger order of every straddling level has
    # exactly its elder ahead of it at its price, the elder nobody (trader 0 lists ids 0, 2, 4, 6, trader 1 ids 1, 3, 5, 7)
    def row(q, b, i):
        k = [e[0] for e in entries[b][i % 2]].index(i)
        return q[b, i % 2, k]

    for b in range(B):
        for elder, younger in ((0, 5), (1, 6), (2, 7), (3, 4)):
            assert int(row(after_rests, b, elder)["level_ahead_orders"]) == 0, (b, elder)
            assert int(row(after_rests, b, younger)["level_ahead_orders"]) == 1, (b, younger)
            assert int(row(after_rests, b, younger)["level_ahead_vol"]) == HAND_VOLS[elder] * (b + 1), (b, younger)
        assert int(row(after_rests, b, 6)["ahead_orders"]) == 3 and int(row(after_rests, b, 1)["ahead_orders"]) == 2  # bids at 99 behind both at 100
        assert int(row(after_rests, b, 4)["ahead_orders"]) == 3  # asks at 103: both asks at 102, then id 3
    c = plan.c
    assert c.front > 0 and c.partial_ahead > 0, vars(c)
    env = ingress_env(bk, torch, B, T, pool, 0, plan.qcap, tick=1, n_orders=32)
    env.enable_open_orders(NT, depth)
    env.enable_open_queue()
    OQ.run_plan(torch, env, plan, f"pool {pool}")
    P.no_flags(env)
    hist = env.history()
    for b, r in enumerate(plan.refs):
        P.same_history(hist[:, b], r.history(), f"L2 history of book {b}")
        P.same_book(env, b, r.book, orders=True, keys=True)
        assert env.trades(b, first=0)["passive_id"].tolist() == HAND_PASSIVE_IDS, b
    if ROOMS[room]:
        assert env.stamp_compactions() >= 1
    env.close()


# ============================================================================================== d. bk_run
# RandomAgents at tick 1: a busy narrow group, 16 ticks wide, next to the top of the range of a slow wide group (4 agents,
# ticks (2, 70 000), rate 0.05, volume 1).  A wide bid rests wherever it lands below the narrow group, so the resting prices
# of a book span more than a key window (KEY_PSPAN) as soon as one landed in the lower half: keys_begin refuses those steps
# and they run event by event, on raw stamps.  About a third of the (step, book) pairs behind the wrap are such steps - the
# wide group acts once in five steps per book - which is what the conditions below ask for at least a quarter of.
D_BOOKS, D_STEPS, D_START = 70, 24, 1  # (a partial wave; start_time 1: rests_of tells a rested order by its key time)
WIDE = (4, (2, 70_000), (1, 2), 1, 0.05)
NOISE_P = dict(tick_size=1, p_limit=0.3, p_market=0.3, p_cancel=0.2, trade_vol=2, price_dist_mu=0.0, price_dist_sigma=1.0)
MOM_P = dict(tick_size=1, p_cancel=0.2, trade_vol=2, decay=1.0, demand=5.0, scale=0.5, order_ratio=1.0, price_dist_mu=0.0,
             price_dist_sigma=3.0)


def _narrow(n, lo=68_000):
    return (n, (lo, lo + 16), (1, 4), 1, 0.8)


D_FLOWS = {
    # name: (kind, pool, seed, agents)
    "random 64": ("books", 64, 265, [_narrow(40), WIDE]),
    "random 128": ("books", 128, 329, [_narrow(60), WIDE]),
    "random 256": ("books", 256, 457, [_narrow(60), WIDE]),
    "random 512": ("books", 512, 713, [_narrow(60), WIDE]),
    "members 256": ("members", 256, 301, [("random",) + _narrow(40), ("random",) + WIDE, ("noise", 100, 10, NOISE_P),
                                          ("momentum", 200, 6, MOM_P)]),
    "market 128": ("market", 128, 401, [(0,) + _narrow(40), (0,) + WIDE, (1, 40, (34_000, 34_008), (1, 4), 2, 0.8),
                                        (1, 4, (1, 35_000), (1, 2), 2, 0.05)]),
}
_d_refs = {}


def d_ref(oracle, flow):
    """The oracle's run of a flow, made once and never stepped again, with what the conditions need: (ref, views, w, counts).
    w: the books start w below 2^32, one less than the fewest orders a book has rested by the end of the first third."""
    if flow not in _d_refs:
        kind, pool, seed, agents = D_FLOWS[flow]
        if kind == "market":
            ref = oracle.ManyMarkets(D_BOOKS // 2, seed, D_START, [1, 2], STEP, True, 10, agents)
            ref.run(D_STEPS, 2)
            views = [ref.book(m, a) for m in range(D_BOOKS // 2) for a in range(2)]
        else:
            ref = oracle.ManyBooks(D_BOOKS, seed, D_START, 1, STEP, True, 10, **{"groups" if kind == "books" else "members": agents})
            ref.run(D_STEPS, 2)
            views = [ref.book(b) for b in range(D_BOOKS)]
        third = D_START + (D_STEPS // 3) * STEP
        w = min(int((rests_of(v)[1] < third).sum()) for v in views) - 1
        ties = on_wide = behind = wide_behind = 0
        wraps = []
        for v in views:
            wide = wide_span_steps(v, D_STEPS, D_START)
            t, tw, wrap = straddling_ties(v, M32 - w, wide, D_START)
            ties, on_wide = ties + t, on_wide + tw
            wraps.append(wrap)
            if wrap is not None:
                behind += D_STEPS - wrap
                wide_behind += sum(1 for s in wide if s >= wrap)
        _d_refs[flow] = (ref, views, w, dict(ties=ties, ties_on_wide_steps=on_wide, wraps=wraps, wide_share=wide_behind / max(behind, 1)))
    return _d_refs[flow]


def d_env(bk, flow, pipeline):
    kind, pool, seed, agents = D_FLOWS[flow]
    kw = dict(levels=10, max_live_orders=pool, trade_capacity=4096, history_capacity=D_STEPS)
    if kind == "market":
        env = bk.ManyMarketEnv(D_BOOKS // 2, seed, D_START, [1, 2], STEP, True, **kw)
        env.set_random_market_agents(agents)
    else:
        env = bk.ManyBookEnv(D_BOOKS, seed, D_START, 1, STEP, True, **kw)
        env.set_agents(agents) if kind == "members" else env.set_random_agents(agents)
    if pipeline:
        env.set_pipeline(pipeline)
    return env


D_CASES = [(f, p) for f in D_FLOWS for p in (("split", "wave_split") if D_FLOWS[f][0] != "market" else (None,))]


@pytest.mark.parametrize("room", list(ROOMS))
@pytest.mark.parametrize("flow,pipeline", D_CASES)
def test_bk_run_across_the_wrap_on_wide_books(bk, oracle, monkeypatch, flow, pipeline, room):
    """Every book wraps within the first third of the run; levels that hold orders from both sides of the wrap trade, some of
    them on steps whose prices no key window holds.  Counted by replaying the oracle's order log (the k-th order to rest
    carries stamp start + k), over the 70 books and 24 steps of each flow:

        flow          w    straddling ties   of them on wide-span steps   wide-span share behind the wrap
        random 64     114        103                  20                            0.37
        random 128    171        177                  37                            0.32
        random 256    179        192                  45                            0.37
        random 512    180        193                  54                            0.37
        members 256   153        197                 108                            0.62
        market 128    118        130                  33                            0.39
    """
    ref, views, w, c = d_ref(oracle, flow)
    assert w > 0 and all(x is not None and x < D_STEPS // 3 for x in c["wraps"]), c["wraps"]
    assert c["wide_share"] >= 0.25, c
    assert c["ties"] >= 50 and c["ties_on_wide_steps"] >= 10, c
    monkeypatch.setenv("BOURSE_AMD_SEQ_START", str(M32 - w))
    _set_room(monkeypatch, room)
    env = d_env(bk, flow, pipeline)
    env.run(D_STEPS)
    P.no_flags(env)
    P.same_history(env.history(), ref.history())
    for b, v in enumerate(views):
        P.same_book(env, b, v)
    if ROOMS[room]:
        assert env.stamp_compactions() >= 3, env.stamp_compactions()
    else:
        assert env.stamp_compactions() == 1  # the one in front of the launch that would have wrapped
    env.close()


# ============================================================================================== the compaction beside resets
def test_reset_books_under_a_small_room(bk, oracle, monkeypatch):
    """test_gpu_reset_books' first case with a compaction every few steps: a snapshot remembers its own bound, a reset takes
    the larger one, and the books are the oracle's all the same."""
    monkeypatch.setenv("BOURSE_AMD_STAMP_ROOM", "300")
    for mask_name in RB.MASKS:
        RB.same_seed_case(bk, oracle, 97, RB.C2, 16, 64, 6, 5, 7, mask_name, "host", (RB.PIPELINES[0], RB.PIPELINES[1]))


# ============================================================================================== e. the 64-bit counters
# n steps, a checkpoint, and the image's counters moved (tests/counter_shift.py) so that - per book - H_TRADES and H_EVENTS
# carry into their high words in the middle of what the book does in the next T1 steps, and H_STEPS / steps_done stand at
# 2^32 - 3.  The restored env runs T1 + T2 + T3 steps; everything it reports is the oracle's steps n .. n + T1 + T2 + T3, the
# counts plus their offsets.  The events a book has processed are no fact of the oracle's: they are read from the images of
# the unshifted env, which runs the same steps first.
E_N, E_T1, E_T2, E_T3, E_CAP = 5, 5, 3, 3, 12  # (a ring of 12 slots: a step count cut to 32 bits lands in another slot)
E_FLOWS = {p: ("books", dict(groups=RB.C2, levels=16, pool=64, tick=RB.TICK), p) for p in RB.PIPELINES}
E_FLOWS["members"] = ("books", dict(members=RB.MEMBERS, levels=10, pool=256, tick=1), "wave_split")
E_FLOWS["market"] = ("market", None, None)
E_BOOKS = 6


class _EFlow:
    def __init__(self, bk, oracle, name):
        self.bk, self.oracle, self.name = bk, oracle, name
        self.kind, self.kw, self.pipeline = E_FLOWS[name]
        self.pool = 128 if self.kind == "market" else self.kw["pool"]

    def env(self):
        if self.kind == "market":
            return RB.market_env(self.bk, E_BOOKS // 2, RB.MKT_TICKS, E_CAP, RB.MKT_GROUPS)
        kw = dict(self.kw)
        env = RB.make_env(self.bk, E_BOOKS, steps=E_CAP, **kw)
        env.set_pipeline(self.pipeline)
        return env

    def ref(self, L):
        """(history [L, B, W], per-book views) of the oracle after L steps"""
        if self.kind == "market":
            r = RB.ref_markets(self.oracle, E_BOOKS // 2, ((L, True),))
            return r.history(), [r.book(m, a) for m in range(E_BOOKS // 2) for a in range(2)]
        kw = {k: v for k, v in self.kw.items() if k in ("groups", "members", "tick")}
        r = RB.ref_books(self.oracle, E_BOOKS, self.kw["levels"], L, **kw)
        return RB.facts(r)["history"], [r.book(b) for b in range(E_BOOKS)]

    def counts(self, L):
        return [v.n_trades() for v in self.ref(L)[1]]


def _hdr64(env, word, pool):
    return CS.read64(CS.books_view(env.checkpoint(), env.n_books, pool), word)


@pytest.mark.parametrize("name", list(E_FLOWS))
def test_counters_carry_into_their_high_words(bk, oracle, name):
    import series_model as SM
    from test_gpu_series import same_rows

    F = _EFlow(bk, oracle, name)
    B, n = E_BOOKS, E_N
    L1, L2, L3 = n + E_T1, n + E_T1 + E_T2, n + E_T1 + E_T2 + E_T3
    # ---- the unshifted env: the image at n, and the books' event counts at n, L1 and L3
    env = F.env()
    env.run(n)
    img = env.checkpoint()
    ev = {n: _hdr64(env, CS.H_EVENTS, F.pool)}
    assert _hdr64(env, CS.H_TRADES, F.pool) == F.counts(n) and _hdr64(env, CS.H_STEPS, F.pool) == [n] * B
    env.run(L1 - n)
    ev[L1] = _hdr64(env, CS.H_EVENTS, F.pool)
    env.run(L3 - L1)
    ev[L3] = _hdr64(env, CS.H_EVENTS, F.pool)
    env.close()
    # ---- the offsets; the conditions: every book's trade and event counts cross 2^32 inside the first T1 steps, the steps too
    tc = {L: F.counts(L) for L in (n, L1, L2, L3)}
    assert all(tc[L1][b] - tc[n][b] >= 2 and ev[L1][b] - ev[n][b] >= 2 for b in range(B)), (tc, ev)
    off_t = [M32 - 1 - tc[n][b] - (tc[L1][b] - tc[n][b]) // 2 for b in range(B)]
    off_e = [M32 - 1 - ev[n][b] - (ev[L1][b] - ev[n][b]) // 2 for b in range(B)]
    off_s = M32 - 3 - n
    for b in range(B):
        assert (tc[n][b] + off_t[b]) >> 32 == 0 and (tc[L1][b] + off_t[b]) >> 32 == 1, b
        assert (ev[n][b] + off_e[b]) >> 32 == 0 and (ev[L1][b] + off_e[b]) >> 32 == 1, b
    assert n + off_s < M32 <= L1 + off_s and (n + off_s) % E_CAP != n % E_CAP
    moved = CS.shift(img, B, F.pool, trades=off_t, events=off_e, steps=off_s)

    def held(env, L, base_L, tag, since=n):
        """the env, restored at step `since`, is the oracle after L steps, its retained trades those from step base_L on, every
        count plus its offset"""
        hist, views = F.ref(L)
        P.no_flags(env)
        assert env.steps_done() == L + off_s, tag
        tail = min(L - since, E_CAP)
        P.same_history(env.history(), hist[L - tail:L], tag=f"{tag}: L2 history")
        assert env.trade_counts().tolist() == [tc[L][b] + off_t[b] for b in range(B)], tag
        for b, v in enumerate(views):
            assert env.trade_count(b) == (tc[L][b] + off_t[b], tc[base_L][b] + off_t[b]), (tag, b)
            P.same_records(env.trades(b), v.trades_array()[tc[base_L][b]:], (tag, b), "retained trade")
            P.same_live(env, b, v, (tag, b))
        assert _hdr64(env, CS.H_TRADES, F.pool) == [tc[L][b] + off_t[b] for b in range(B)], tag
        assert _hdr64(env, CS.H_TRADE_BASE, F.pool) == [tc[base_L][b] + off_t[b] for b in range(B)], tag
        assert _hdr64(env, CS.H_STEPS, F.pool) == [L + off_s] * B, tag
        if L in ev:
            assert _hdr64(env, CS.H_EVENTS, F.pool) == [ev[L][b] + off_e[b] for b in range(B)], tag
            st = env.stats()
            assert st["sum_trades"] == sum(tc[L][b] + off_t[b] for b in range(B)) & CS.M64, (tag, st)
            assert st["sum_events"] == sum(ev[L][b] + off_e[b] for b in range(B)) & CS.M64, (tag, st)

    # ---- the restored env: T1 steps through run_series in chunks of 2, then every reader
    env = F.env()
    env.enable_series()
    env.restore(moved)
    assert env.steps_done() == M32 - 3
    env.run_series(E_T1, chunk=2)
    env.sync()
    held(env, L1, n, "after the carry")
    same_rows(env.series(), SM.rows(F.ref(L1)[0][n:L1], first_step=n + off_s), "series rows over the carry")
    assert env.flags_summary() == (0, max(tc[L1][b] - tc[n][b] for b in range(B)))
    env.save_snapshot()
    second = env.checkpoint()
    off, rec = env.drain_trades()
    views = F.ref(L1)[1]
    assert off.tolist() == np.concatenate([[0], np.cumsum([tc[L1][b] - tc[n][b] for b in range(B)])]).tolist()
    for b, v in enumerate(views):
        P.same_records(rec[int(off[b]):int(off[b + 1])], v.trades_array()[tc[n][b]:], (b, "drained"), "trade")
    held(env, L1, L1, "after drain_trades")
    # ---- T2 more steps, then the books (markets) of a mask go back to the snapshot: their trade base is the snapshot's count
    env.run(E_T2)
    held(env, L2, L1, "T2 steps on")
    units = B // 2 if F.kind == "market" else B
    mask = RB.make_mask("alternate", units)
    (env.reset_markets if F.kind == "market" else env.reset_books)(mask)
    env.run(E_T3)
    env.sync()
    per_book = np.repeat(mask, B // units)
    P.no_flags(env)
    assert env.steps_done() == L3 + off_s
    kept_h, kept_v = F.ref(L3)
    back_h, back_v = F.ref(L1 + E_T3)
    got_h = env.history()
    tcb = F.counts(L1 + E_T3)
    for b in range(B):
        h, v, c = (back_h, back_v, tcb) if per_book[b] else (kept_h, kept_v, tc[L3])
        L = L1 + E_T3 if per_book[b] else L3
        P.same_history(got_h[len(got_h) - E_T3:, b], h[L - E_T3:L, b], tag=f"book {b} after the reset: L2 history tail")
        assert env.trade_count(b) == (c[b] + off_t[b], tc[L1][b] + off_t[b]), b
        P.same_records(env.trades(b), v[b].trades_array()[tc[L1][b]:], (b, "after the reset"), "retained trade")
        P.same_live(env, b, v[b], (b, "after the reset"))
    env.close()
    # ---- a third env from the checkpoint taken behind the carry continues identically
    env = F.env()
    env.restore(second)
    assert env.steps_done() == L1 + off_s
    env.run(E_T2)
    held(env, L2, L1, "third env, restored behind the carry", since=L1)
    env.run(E_T3)
    held(env, L3, L1, "third env at the end", since=L1)
    env.close()
