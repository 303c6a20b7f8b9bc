"""bk_submit_quotes_device / bk_submit_quotes (bourse_amd/csrc/quotes_ingress.hpp): a dense table of target quotes per book and
trader, joined with the open-order view's entries on the device and queued as cancellations, in-place reductions and new orders.

The expected side never shares code with the kernel: tests/quotes_model.py::expand (plain Python) makes the dense grid from
open_orders_model.rows_ints over the oracle's orders, the grid goes to one oracle.StepEnv(SEED + b) per book through
ingress_support.apply_oracle, and the device env is compared with ingress_support.check - level-2 history, trades, live orders
in priority order, the order log, the keys and the RNG state.  The expected side runs FIRST (tests/quotes_cases.py::QuotePlan),
because a step's quotes name ids that rest on it; where a case says something only under a condition, the condition is counted
on the expected side and asserted before anything is compared."""

import ctypes

import numpy as np
import pytest

import accounts_model as AM
import open_orders_model as OM
import oracle_parity as P
import quotes_cases as QC
import quotes_model as QM
from ingress_support import SEED, STEP, apply_oracle, check, ingress_env, members_env, submit, thin_flow
from members_ingress_cases import NOISE
from quotes_cases import O, UNTOUCHED, cancel, failing_step, grid_rows, new, outputs, quotes_dev, reduce, twin_step

pytestmark = pytest.mark.gpu
BK_INVALID_ARGUMENT = 5
KEEP = QM.KEEP
U64MAX = 0xFFFFFFFFFFFFFFFF
NONE = (0xFFFFFFFF, 0, 0, 0)


@pytest.fixture(scope="module")
def bk():
    import bourse_amd

    return bourse_amd


def plan_env(bk, torch, plan, pool, extra_orders=0):
    """a device env that takes the plan: the queue holds a step's background and its whole grid, the log every order"""
    n_bg = max([0] + [int(np.diff(bg[0]).max()) for bg, _, _, _ in plan.steps if bg is not None])
    n_orders = sum(int((g[1][0] == 1).sum()) + (len(bg[1][0]) if bg is not None else 0) for bg, _, g, _ in plan.steps)
    env = ingress_env(bk, torch, plan.B, max(len(plan.steps), 1), pool, 0, n_bg + plan.NT * plan.G,
                      tick=plan.tick, n_orders=n_orders + extra_orders + 16)
    env.enable_open_orders(plan.NT, plan.depth)
    return env


def same_rows(got, want, tag):
    for k, part in enumerate(("summary", "entries")):
        for f in want[k].dtype.names:
            P.same_array(got[k][f], want[k][f], tag, f"{part} field {f}")


def device_step(torch, env, plan, s, tag, host=False):
    """step s of the plan on the device: background, quotes, step; the ids and the status the call reports, and the open-order
    rows after the step, against the expected side's"""
    bg, quotes, _, want_ids = plan.steps[s]
    if bg is not None:
        submit(torch, env, *bg)
    ids, status = outputs(torch, plan)
    env.submit_quotes(quotes if host else quotes_dev(torch, quotes), ids, status, check_status=True)
    env.step(sync=False)
    P.same_array(ids.cpu().numpy().view(np.uint64), want_ids, f"{tag}, step {s}", "out_ids")
    st = status.cpu().numpy()
    assert (st[:, 0] == 0).all() and (st[:, 1] == plan.NT * plan.G).all(), (tag, s, st.tolist())
    same_rows(env.open_orders(), plan.rows_after[s], f"{tag}: rows after step {s}")


def run_plan(torch, env, plan, tag, host=False):
    for s in range(len(plan.steps)):
        device_step(torch, env, plan, s, tag, host)
    P.no_flags(env)
    check(env, plan.refs)


# ------------------------------------------------------------------------------------------------ 1. by hand
# One trader (row 0; row 1 never quotes) at depth 3 on a book with tick 1, a third party (trader 5000) beside it.  Per stage:
# the third party's orders, trader 0's quote row, the five grid positions of trader 0 the model must make, trader 0's entries
# after the step, and the passive ids of the trades the step must add, in order.
K = (0, KEEP, 0, KEEP)
HAND_STAGES = [
    # fresh quotes: ids 0 (bid) and 1 (ask)
    ([], (100, 10, 104, 10), [O, O, O, new(0, 1, 100, 10), new(0, 0, 104, 10)], [(0, 100, 10, 1), (1, 104, 10, 0), NONE], []),
    # the same quotes again: nothing.  The third party bids 5 @ 100 behind id 0 (id 2)
    ([(1, 1, 5, 5000, 100, 0)], (100, 10, 104, 10), [O] * 5, [(0, 100, 10, 1), (1, 104, 10, 0), NONE], []),
    # a smaller bid volume: id 0 is reduced to 6 in place ...
    ([], (100, 6, 104, 10), [reduce(0, 0, 6), O, O, O, O], [(0, 100, 6, 1), (1, 104, 10, 0), NONE], []),
    # ... and keeps its place: the third party sells 8 @ 100 (id 3) - 6 from id 0, THEN 2 from id 2
    ([(1, 0, 8, 5000, 100, 0)], K, [O] * 5, [(1, 104, 10, 0), NONE, NONE], [0, 2]),
    # a larger ask volume: id 1 keeps, the top-up of 15 (id 4) queues behind it
    ([], (0, KEEP, 104, 25), [O, O, O, O, new(0, 0, 104, 15)], [(1, 104, 10, 0), (4, 104, 15, 0), NONE], []),
    # the third party buys 12 @ 104 (id 5): 10 from the keeper, then 2 from the top-up
    ([(1, 1, 12, 5000, 104, 0)], K, [O] * 5, [(4, 104, 13, 0), NONE, NONE], [1, 4]),
    # a moved price: the ask at 104 is cancelled and a new one placed at 105; a fresh bid at 99 (ids 6, 7: the bid comes first)
    ([], (99, 4, 105, 13), [cancel(0, 4), O, O, new(0, 1, 99, 4), new(0, 0, 105, 13)], [(6, 99, 4, 1), (7, 105, 13, 0), NONE], []),
    # vol 0 pulls the bid, KEEP leaves the ask
    ([], (99, 0, 0, KEEP), [cancel(0, 6), O, O, O, O], [(7, 105, 13, 0), NONE, NONE], []),
    # KEEP on both sides: nothing
    ([], K, [O] * 5, [(7, 105, 13, 0), NONE, NONE], []),
]


def test_a_book_worked_out_by_hand_stage_by_stage(bk, oracle):
    """Two books, tick 1, n_traders = 2, depth = 3; book 1 is never touched.  Everything is compared after every stage."""
    import torch

    plan = QC.QuotePlan(oracle, 2, 1, 2, 3)
    env = ingress_env(bk, torch, 2, len(HAND_STAGES), 64, 0, 16, tick=1, n_orders=32)
    env.enable_open_orders(2, 3)
    n_trades = 0
    for s, (third, quote, grid, entries, passive) in enumerate(HAND_STAGES):
        off = np.array([0, len(third), len(third)], dtype=np.int64)
        col = lambda k, dt: np.array([r[k] for r in third], dtype=dt)
        bg = (off, (col(0, np.uint32), col(1, np.uint8), col(2, np.uint32), col(3, np.uint32), col(4, np.uint32), col(5, np.uint64)))
        quotes = np.array([[quote, K], [K, K]], dtype=np.uint32)
        assert grid_rows(plan.entries()[0], quotes[0].tolist(), 3) == grid + [O] * 5, f"the model's grid, stage {s}"
        plan.step(quotes, background=bg if third else None)
        view = plan.refs[0].book
        assert OM.rows_ints(view.orders_array(), 2, 3)[1][0] == entries, f"the model over the oracle's book, stage {s}"
        t = view.trades_array()
        assert [int(x) for x in t["passive_id"][n_trades:]] == passive, f"the oracle's trades, stage {s}"
        n_trades = len(t)
        device_step(torch, env, plan, s, "by hand")
        assert [tuple(int(x) for x in e) for e in env.open_orders()[1][0, 0]] == entries, f"the device's entries, stage {s}"
        check(env, plan.refs)
    P.no_flags(env)
    assert plan.count["reduce"] == 1 and plan.count["topup"] == 1 and plan.count["fresh"] == 4 and plan.count["cancel"] == 2
    env.close()


# ------------------------------------------------------------------------------------------------ 2. the busy flow
@pytest.mark.parametrize("pool", [64, 512])
def test_the_busy_flow_equals_the_oracle(bk, oracle, pool):
    """6 books x 10 steps, 5 traders at depth 3 (tests/quotes_cases.py::busy_plan; tests/test_quotes_cpu.py asserts the same
    conditions without a GPU).  At 512 slots the event kernel is chosen by k_ingest's hint word, which the quotes'
    modifications set; at 64 slots the full kernel always runs: both must equal the oracle."""
    import torch

    plan = QC.busy_plan(oracle, pool)
    QC.assert_busy(plan, pool)
    assert plan.count["reduce"] > 0  # (a modification: the hint path at 512 slots)
    env = plan_env(bk, torch, plan, pool)
    run_plan(torch, env, plan, f"busy, pool {pool}")
    env.close()


# ------------------------------------------------------------------------------------------------ 3. shapes
def deep_plan(oracle):
    """depth 64, G = 66: one trader spans two passes.  Trader 0 of every book first rests 70 bids (more than 64, more than a
    pass) placed through the ingress, then quotes: the 64 listed ones are cancelled but the keeper, the six unlisted stay."""
    plan = QC.QuotePlan(oracle, 2, 2, 2, 64)
    n = 70
    off = np.array([0, n, 2 * n], dtype=np.int64)
    price = np.tile((30 + np.arange(n) % 10) * 2, 2).astype(np.uint32)
    bg = (off, (np.ones(2 * n, np.uint32), np.ones(2 * n, np.uint8), np.full(2 * n, 3, np.uint32), np.zeros(2 * n, np.uint32), price,
                np.zeros(2 * n, np.uint64)))
    plan.step(np.full((2, 2, 4), [0, KEEP, 0, KEEP], dtype=np.uint32), background=bg)
    plan.step(np.array([[(70, 9, 110, 5), (60, 1, 112, 2)], [(62, 2, 0, KEEP), (0, KEEP, 0, KEEP)]], dtype=np.uint32))
    plan.step(np.array([[(70, 4, 110, 8), (0, KEEP, 112, 0)], [(62, 0, 120, 1), (64, 3, 0, KEEP)]], dtype=np.uint32))
    return plan


@pytest.mark.parametrize("shape", ["12 x 8", "70 x 3", "depth 1", "depth 64"])
def test_shapes(bk, oracle, shape):
    import torch

    if shape == "12 x 8":    # 120 grid positions: two passes
        plan, pool = QC.shape_plan(oracle, 3, 12, 8, 5, 223), 256
        assert plan.NT * plan.G == 120 and plan.most_live_positions > 0
    elif shape == "70 x 3":  # 350 positions, six passes; G = 5 and 64 = 12 * 5 + 4: trader 12 straddles the first boundary
        plan, pool = QC.wide_plan(oracle), 256
        assert plan.most_live_positions > 64, "no book with more than 64 live grid positions in one call"
        live = np.stack([step[2][1][0].reshape(3, 70, 5) != 0 for step in plan.steps])
        assert (live[:, :, 12, 3] & live[:, :, 12, 4]).any(), "the trader across the first pass boundary never places both orders"
    elif shape == "depth 1":
        plan, pool = QC.shape_plan(oracle, 3, 6, 1, 6, 227), 128
        assert plan.beyond_depth > 0
    else:
        plan, pool = deep_plan(oracle), 256
        assert plan.most_resting > 64 and plan.beyond_depth > 0 and plan.unlisted_stay >= 6 and plan.count["cancel"] > 64
        assert plan.most_live_positions > 64
    for w in ("cancel", "fresh"):
        assert plan.count[w] > 0, (w, plan.count)
    if shape != "depth 64":
        assert plan.count["reduce"] > 0 and plan.count["topup"] > 0 and plan.count["untouched"] > 0, plan.count
    assert plan.most_live < pool, (plan.most_live, pool)
    env = plan_env(bk, torch, plan, pool)
    run_plan(torch, env, plan, shape)
    env.close()


# ------------------------------------------------------------------------------------------------ 4. failures, against a twin
def test_an_off_tick_bid_stops_its_book_there_and_the_neighbours_are_whole(bk, oracle):
    import torch

    B, NT, depth, tick = 3, 4, 2, 2
    plan = QC.QuotePlan(oracle, B, tick, NT, depth)
    q0 = np.zeros((B, NT, 4), dtype=np.uint32)
    q0[:] = (96, 10, 104, 10)
    plan.step(q0)
    env, twin = plan_env(bk, torch, plan, 64, extra_orders=64), plan_env(bk, torch, plan, 64, extra_orders=64)
    device_step(torch, env, plan, 0, "before the bad price")
    twin_step(torch, twin, plan, 0)
    # every trader moves both sides; trader 2 of book 1 bids at 95, which the tick 2 does not divide
    q1 = np.zeros((B, NT, 4), dtype=np.uint32)
    q1[:] = (94, 5, 106, 5)
    q1[1, 2, 0] = 95
    ids = failing_step(torch, env, twin, plan, q1, (1, 2 * (depth + 2) + depth), 1, (ValueError, "book 1: a quoted price"))
    # the two new ids of a whole trader, u64::MAX where nothing was created, untouched from the failing element on
    assert ids[0].tolist() == [[8 + 2 * t, 9 + 2 * t] for t in range(NT)]
    assert ids[1].tolist() == [[8, 9], [10, 11], [UNTOUCHED, UNTOUCHED], [UNTOUCHED, UNTOUCHED]]
    for e in (env, twin):
        e.sync()
        for b in range(B):
            P.same_book(e, b, plan.refs[b].book, orders=False)
    env.close()
    twin.close()


def test_a_queue_too_small_for_the_grid_gives_capacity_with_the_applied_count(bk, oracle):
    import torch

    B, NT, depth, tick = 2, 4, 2, 2
    plan = QC.QuotePlan(oracle, B, tick, NT, depth)
    envs = []
    for _ in range(2):
        e = ingress_env(bk, torch, B, 4, 64, 0, 5, tick=tick, n_orders=64, strict=False)  # room for five events a step
        e.enable_open_orders(NT, depth)
        envs.append(e)
    env, twin = envs
    # book 0: traders 0 and 1 quote (4 events); book 1: all four traders do (8 events): the sixth, trader 2's ask at grid
    # position 2 * 4 + 3 = 11, does not fit
    q = np.full((B, NT, 4), [0, KEEP, 0, KEEP], dtype=np.uint32)
    q[0, :2] = (96, 10, 104, 10)
    q[1, :] = (96, 10, 104, 10)
    ids = failing_step(torch, env, twin, plan, q, (1, 11), 3, (bk.CapacityError, "book 1"))
    assert ids[1].tolist() == [[0, 1], [2, 3], [4, UNTOUCHED], [UNTOUCHED, UNTOUCHED]]
    assert ids[0].tolist() == [[0, 1], [2, 3], [U64MAX, U64MAX], [U64MAX, U64MAX]]
    for e in (env, twin):
        e.sync()
        for b in range(B):
            P.same_book(e, b, plan.refs[b].book, orders=False)
    env.close()
    twin.close()


# ------------------------------------------------------------------------------------------------ 5. composition in one step
@pytest.mark.parametrize("order", ["quotes first", "quotes last"])
def test_quotes_beside_instructions_and_members_in_one_step(bk, oracle, order):
    """One step holds three calls on one queue: the quotes, a submit_instructions_device of a third party and update_members of
    Noise members with agent_id_start = 1000 >= n_traders - in that order and in the reverse.  The accounts run beside it."""
    import torch

    B, T, NT, depth, tick, NX = 3, 6, 4, 3, 1, 4
    members = [("noise", 1000, 20, dict(NOISE, p_limit=0.5, p_market=0.3))]
    sets = [oracle.AgentSet(members) for _ in range(B)]
    plan = QC.QuotePlan(oracle, B, tick, NT, depth)
    rng = np.random.default_rng(5)
    last, flows = None, []
    update = lambda b, r: sets[b].update(r)
    for _ in range(T):
        last = QC.draw_quotes(rng, plan, last)
        bg = thin_flow(rng, B, NX, tick)
        flows.append(bg)
        third = lambda b, r, bg=bg: apply_oracle(r, int(bg[0][b]), int(bg[0][b + 1]), bg[1])
        if order == "quotes first":
            plan.step(last, after=lambda b, r, third=third: (third(b, r), update(b, r)))
        else:
            plan.step(last, before=lambda b, r, third=third: (update(b, r), third(b, r)))
    assert plan.count["fresh"] > 0 and plan.count["cancel"] > 0 and plan.count["untouched"] + plan.count["topup"] + plan.count["reduce"] > 0
    active = [r.book.orders_array() for r in plan.refs]
    assert all(((o["status"] == 1) & (o["trader_id"] >= 1000)).any() for o in active), "no resting order of a member"
    env = members_env(bk, torch, B, T, 256, members, tick, n_ext=NX + NT * plan.G)
    env.set_agents(members)
    env.enable_open_orders(NT, depth)
    env.enable_accounts(NT)
    for s, (_, quotes, _, want_ids) in enumerate(plan.steps):
        ids, status = outputs(torch, plan)
        if order == "quotes first":
            env.submit_quotes(quotes_dev(torch, quotes), ids, status)
            submit(torch, env, *flows[s])
            env.update_members(sync=False)
        else:
            env.update_members(sync=False)
            submit(torch, env, *flows[s])
            env.submit_quotes(quotes_dev(torch, quotes), ids, status)
        env.step(sync=False)
        P.same_array(ids.cpu().numpy().view(np.uint64), want_ids, f"{order}, step {s}", "out_ids")
        same_rows(env.open_orders(), plan.rows_after[s], f"{order}: rows after step {s}")
    P.no_flags(env)
    check(env, plan.refs)
    want = np.stack([AM.fold(r.book.trades_array(), r.book.orders_array(), NT) for r in plan.refs])
    assert want["fills"].any()
    got = env.accounts()
    for f in want.dtype.names:
        P.same_array(got[f], want[f], "accounts beside the quotes", f)
    env.close()


def test_after_a_partial_reset_the_masked_books_requote_from_the_snapshots_entries(bk, oracle):
    """3 steps, save, 2 steps, reset books 0 and 2, 2 steps.  The oracle cannot be rewound: a reset book's expected side is a
    replay - a fresh plan given steps 0..2 and then the two steps after the reset, whose grids come from the snapshot's
    entries."""
    import torch

    B, NT, depth, tick = 3, 4, 3, 2
    rng = np.random.default_rng(41)
    plan, replay = QC.QuotePlan(oracle, B, tick, NT, depth), QC.QuotePlan(oracle, B, tick, NT, depth)
    last, calls = None, []
    for _ in range(7):
        last = QC.draw_quotes(rng, plan, last)
        calls.append((last, thin_flow(rng, B, 3, tick)))
    for q, bg in calls:
        plan.step(q, background=bg)
    for q, bg in calls[:3] + calls[5:]:
        replay.step(q, background=bg)
    mask = np.array([1, 0, 1], dtype=bool)
    for b in np.flatnonzero(mask):  # the masked books requote from other entries than they would have
        assert not np.array_equal(plan.rows_after[4][1][b], plan.rows_after[2][1][b])
        assert [x[b * NT * plan.G:(b + 1) * NT * plan.G].tolist() for x in plan.steps[5][2][1]] != \
               [x[b * NT * plan.G:(b + 1) * NT * plan.G].tolist() for x in replay.steps[3][2][1]]
    env = plan_env(bk, torch, plan, 128)
    for s in range(5):
        device_step(torch, env, plan, s, "before the reset")
        if s == 2:
            env.save_ingress_snapshot()
    env.reset_ingress_books(torch.tensor(mask, device="cuda"), sync=False)
    for s in (5, 6):
        bg, quotes, _, _ = plan.steps[s]
        submit(torch, env, *bg)
        ids, status = outputs(torch, plan)
        env.submit_quotes(quotes_dev(torch, quotes), ids, status, check_status=True)
        env.step(sync=False)
        got, got_ids = env.open_orders(), ids.cpu().numpy().view(np.uint64)
        for b in range(B):
            src, at = (replay, s - 2) if mask[b] else (plan, s)
            P.same_array(got_ids[b], src.steps[at][3][b], f"book {b}, step {s}", "out_ids")
            same_rows((got[0][b], got[1][b]), (src.rows_after[at][0][b], src.rows_after[at][1][b]), f"book {b}: rows after step {s}")
    P.no_flags(env)
    for b in range(B):
        P.same_live(env, b, (replay if mask[b] else plan).refs[b].book)
    env.close()


# ------------------------------------------------------------------------------------------------ 6. markets
def test_three_asset_markets_requote_per_book(bk, oracle):
    """3 markets x 3 assets = 9 books with ticks 1, 2 and 5: the rows are per book (market * assets + asset), one wave walks
    its market's assets in order into the market's one queue."""
    import torch

    NM, A, T, NT, depth, TICKS = 3, 3, 6, 4, 3, [1, 2, 5]
    G = depth + 2
    env = bk.ManyMarketEnv(NM, SEED, 0, TICKS, STEP, levels=10, max_live_orders=128, max_orders=512, trade_capacity=1024,
                           history_capacity=T, stream=torch.cuda.current_stream().cuda_stream)
    env.enable_device_ingress(A * (NT * G + 4))
    env.enable_open_orders(NT, depth)
    refs = [oracle.ManyMarkets(1, SEED + m, 0, TICKS, STEP, True, 10) for m in range(NM)]
    views = [refs[b // A].book(0, b % A) for b in range(NM * A)]
    rng = np.random.default_rng(43)
    count = {}
    for s in range(T):
        # a third party around 100 on every book; every price is a multiple of 10, which all three ticks divide
        n_b = rng.integers(1, 5, size=NM * A)
        off = np.zeros(NM * A + 1, dtype=np.int64)
        off[1:] = np.cumsum(n_b)
        n = int(off[-1])
        bid = rng.integers(0, 2, size=n).astype(np.uint8)
        bg = (off, (np.ones(n, np.uint32), bid, rng.integers(20, 200, size=n).astype(np.uint32), np.full(n, 5000, np.uint32),
                    (rng.integers(8, 13, size=n) * 10).astype(np.uint32), np.zeros(n, np.uint64)))
        quotes = np.zeros((NM * A, NT, 4), dtype=np.uint32)
        for b in range(NM * A):
            for t in range(NT):
                for k, base in ((0, 90), (2, 110)):
                    u = rng.random()
                    quotes[b, t, k:k + 2] = (0, KEEP) if u < 0.15 else (base, 0) if u < 0.25 else \
                        (base + 10 * int(rng.random() < 0.3), int(rng.choice([50, 100, 200])))
        want_ids = np.full((NM * A, NT, 2), U64MAX, dtype=np.uint64)
        # the market's queue takes each call's events asset by asset: the third party's of every book, then the quotes'
        for b in range(NM * A):
            for i in range(int(off[b]), int(off[b + 1])):
                refs[b // A].place_order(0, b % A, bool(bg[1][1][i]), int(bg[1][2][i]), int(bg[1][3][i]), price=int(bg[1][4][i]))
        for b, view in enumerate(views):
            m, a = divmod(b, A)
            g = QM.expand(OM.rows_ints(view.orders_array(), NT, depth)[1], quotes[b].tolist(), depth, count)
            next_id = view.n_orders()
            for i in range(len(g[0])):
                act = int(g[0][i])
                if act == 1:
                    refs[m].place_order(0, a, bool(g[1][i]), int(g[2][i]), int(g[3][i]), price=int(g[4][i]))
                    want_ids[b, i // G, i % G - depth] = next_id
                    next_id += 1
                elif act == 2:
                    refs[m].cancel_order(0, a, int(g[5][i]))
                elif act == QM.MOD:
                    refs[m].modify_order(0, a, int(g[5][i]), new_vol=int(g[2][i]))
        submit(torch, env, *bg)
        ids = torch.full((NM * A, NT, 2), UNTOUCHED, dtype=torch.int64, device="cuda")
        status = torch.full((NM * A, 2), UNTOUCHED, dtype=torch.int32, device="cuda")
        env.submit_quotes(quotes_dev(torch, quotes), ids, status, check_status=True)
        env.step(sync=False)
        for r in refs:
            r.step()
        P.same_array(ids.cpu().numpy().view(np.uint64), want_ids, f"markets, step {s}", "out_ids")
        assert status.cpu().numpy().tolist() == [[0, NT * G]] * (NM * A)
        rows = [OM.rows(v.orders_array(), NT, depth) for v in views]
        same_rows(env.open_orders(), (np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])), f"markets: rows after step {s}")
    for w in ("cancel", "reduce", "topup", "fresh", "untouched"):
        assert count.get(w, 0) > 0, (w, count)
    P.no_flags(env)
    env.sync()
    for b, view in enumerate(views):
        P.same_book(env, b, view, orders=True)
    env.close()


# ------------------------------------------------------------------------------------------------ 7. the host-array entry
@pytest.mark.parametrize("form", ["uint32 array", "QUOTE_DTYPE rows", "int64 array"])
def test_the_host_array_entry_gives_what_the_device_entry_gives(bk, oracle, form):
    import torch

    plan = QC.shape_plan(oracle, 3, 5, 3, 4, 229)
    assert plan.count["reduce"] + plan.count["topup"] > 0 and plan.count["cancel"] > 0
    env = plan_env(bk, torch, plan, 128)
    for s, (bg, quotes, _, _) in enumerate(plan.steps):
        if form == "QUOTE_DTYPE rows":
            plan.steps[s] = (bg, quotes.view(bk.QUOTE_DTYPE).reshape(plan.B, plan.NT)) + plan.steps[s][2:]
        elif form == "int64 array":
            plan.steps[s] = (bg, quotes.astype(np.int64)) + plan.steps[s][2:]
    run_plan(torch, env, plan, f"host entry, {form}", host=True)
    env.close()


# ------------------------------------------------------------------------------------------------ 8. refusals
def _refused(bk, call, match):
    with pytest.raises(bk.BourseError, match=match) as e:
        call()
    assert e.value.code == BK_INVALID_ARGUMENT


def test_refusals_leave_the_env_working(bk, oracle):
    import torch

    B, NT = 2, 3
    stream = torch.cuda.current_stream().cuda_stream
    q = torch.zeros((B, NT, 4), dtype=torch.int32, device="cuda")
    host = np.zeros((B, NT, 4), dtype=np.uint32)
    # without the device ingress (a host-driven env)
    env = bk.ManyBookEnv(B, SEED, 0, 1, STEP, max_live_orders=64, max_orders=64, stream=stream)
    _refused(bk, lambda: env.submit_quotes(q), "bk_device_ingress_enable")
    _refused(bk, lambda: env.submit_quotes(host), "bk_device_ingress_enable")
    env.place_order(0, True, 5, 1, price=100)
    env.step()
    assert env.order_count(0) == 1
    env.close()
    # without the open-order view, then with depth == 0
    env = ingress_env(bk, torch, B, 4, 64, 0, 16, tick=1, n_orders=64)
    _refused(bk, lambda: env.submit_quotes(q), "bk_open_orders_enable")
    _refused(bk, lambda: env.submit_quotes(host), "bk_open_orders_enable")
    env.enable_open_orders(NT, 0)
    _refused(bk, lambda: env.submit_quotes(q), "depth > 0")
    _refused(bk, lambda: env.submit_quotes(host), "depth > 0")
    env.step()
    assert env.order_count(0) == 0, "a refused call queued something"
    env.close()
    # null quotes, a table of the wrong shape, a tensor of the wrong width or not on the device
    env = ingress_env(bk, torch, B, 4, 64, 0, 16, tick=1, n_orders=64)
    env.enable_open_orders(NT, 2)
    for rc in (env._L.bk_submit_quotes_device(env._h, None, None, None), env._L.bk_submit_quotes(env._h, None, None, None)):
        assert rc == BK_INVALID_ARGUMENT and b"null quotes" in env._L.bk_last_error()
    assert env._L.bk_submit_quotes_device(env._h, ctypes.c_void_p(q.data_ptr() + 4), None, None) == BK_INVALID_ARGUMENT
    assert b"16-byte aligned" in env._L.bk_last_error()
    with pytest.raises(ValueError, match="shape"):
        env.submit_quotes(q[:, :2].contiguous())
    with pytest.raises(ValueError, match="shape"):
        env.submit_quotes(host[:1])
    with pytest.raises(ValueError, match="4-byte"):
        env.submit_quotes(q.to(torch.int64))
    with pytest.raises(ValueError, match="32-bit"):
        env.submit_quotes(host.astype(np.int64) - 1)
    with pytest.raises(ValueError, match="status"):
        env.submit_quotes(q, check_status=True)
    # ... and the env works
    host[:] = (100, 5, 104, 5)
    env.submit_quotes(host)
    env.step()
    assert [env.order_count(b) for b in range(B)] == [2 * NT] * B and len(env.live_orders(1)) == 2 * NT
    P.no_flags(env)
    env.close()


# ------------------------------------------------------------------------------------------------ 9. an env that never calls it
def test_an_env_that_never_calls_it_is_unchanged(bk, oracle):
    """The same instruction flow on an env with the open-order view and on one without: neither ever submits a quote, and
    both equal the oracle - the feature adds nothing to a step that does not use it."""
    import torch

    B, T, tick = 4, 5, 2
    refs = [oracle.StepEnv(SEED + b, 0, tick, STEP) for b in range(B)]
    rng = np.random.default_rng(47)
    flows = [thin_flow(rng, B, 8, tick) for _ in range(T)]
    envs = [ingress_env(bk, torch, B, T, 128, 0, 8, tick=tick, n_orders=8 * T + 16) for _ in range(2)]
    envs[0].enable_open_orders(4, 3)
    for off, ins in flows:
        for b, r in enumerate(refs):
            apply_oracle(r, int(off[b]), int(off[b + 1]), ins)
            r.step()
        for e in envs:
            submit(torch, e, off, ins)
            e.step(sync=False)
    assert sum(len(r.book.trades_array()) for r in refs) > 0
    for e in envs:
        P.no_flags(e)
        check(e, refs)
        e.close()
