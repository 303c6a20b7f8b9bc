"""Per-book series moments of the level-2 history (bk_series_enable; bourse_amd/csrc/series.hpp): one row of 24 integer
words per book, folded on the device from the history ring.

The expected side never shares code with the kernel: tests/series_model.py::fold (plain Python ints) over the ORACLE's
history() of the same run - oracle.ManyBooks / ManyMarkets for bk_run, one oracle.StepEnv per book for the host-driven and
the device-ingress flows - and the device's own history is held against the oracle's through tests/oracle_parity.py where
the ring still retains it; case 1's rows are literal numbers worked out by hand.  Where a case says something only under a
condition - one-sided steps, pairs, returns of both signs, a word that wraps - the condition is asserted on the expected
side before anything is compared."""
import numpy as np
import pytest

import oracle_parity as P
import series_model as SM
from ingress_support import ingress_env
from test_gpu_reset_books import C2, MEMBERS, PIPELINES, STEP, make_env, ref_books

pytestmark = pytest.mark.gpu
M64 = (1 << 64) - 1
MAXU = 0xFFFFFFFF
SEED = 101


@pytest.fixture(scope="module")
def bk():
    import bourse_amd

    return bourse_amd


def same_rows(got, want, tag):
    assert got.dtype == want.dtype == SM.SERIES_DTYPE, (got.dtype, want.dtype)
    assert got.shape == want.shape, f"{tag}: rows {got.shape} vs {want.shape}"
    for f in SM.FIELDS:
        P.same_array(got[f], want[f], tag, f"series word {f}")


def cleared_rows(n):
    return np.array([SM.row(SM.cleared())] * n, dtype=SM.SERIES_DTYPE)


def lost(bk, call, n):
    with pytest.raises(bk.BourseError, match=rf"\b{n} step\(s\) of the series were lost") as e:
        call()
    assert e.value.code == 5


def refused(bk, call, match):
    with pytest.raises(bk.BourseError, match=match) as e:
        call()
    assert e.value.code == 5


def run_env(bk, B, cap, groups=C2, members=None, **kw):
    """an env of test_gpu_reset_books' shape (levels 16, pool 64) with the table on"""
    env = make_env(bk, B, groups=None if members else groups, members=members, steps=cap, **kw)
    env.enable_series()
    return env


# ------------------------------------------------------------------------------------------------ 1. by hand
def test_rows_worked_out_by_hand(bk, oracle):
    """Two books, tick 1, a ring of 8, six host-driven steps (one call per step, so nothing depends on a step's shuffle).
    Book 0:                                                  bid  ask   m    d   bid_vol ask_vol tv
      s0  nothing: empty                                       -    -                0      0
      s1  bid 5 @ 100 (id 0): one-sided                      100    -                5      0
      s2  ask 3 @ 104 (id 1): two-sided                      100  104  204           5      3
      s3  bid 2 @ 102 (id 2): a move up                      102  104  206  +2       7      3
      s4  cancel id 2: a move down                           100  104  204  -2       5      3
      s5  ask 1 @ 100 (id 3): fills 1 of id 0, no move       100  104  204   0       4      3     1
    Book 1 gets bid 9 @ 50 in s1 and nothing else: never two-sided."""
    env = bk.ManyBookEnv(2, SEED, 0, 1, STEP, levels=5, max_live_orders=16, max_orders=16, trade_capacity=16, history_capacity=8)
    refs = [oracle.StepEnv(SEED + b, 0, 1, STEP, True, 5) for b in range(2)]
    env.enable_series()
    calls = [[], [("place_order", 0, (True, 5, 1, 100)), ("place_order", 1, (True, 9, 1, 50))], [("place_order", 0, (False, 3, 2, 104))],
             [("place_order", 0, (True, 2, 3, 102))], [("cancel_order", 0, (2,))], [("place_order", 0, (False, 1, 4, 100))]]
    for step in calls:
        for f, b, args in step:
            got, want = getattr(env, f)(b, *args), getattr(refs[b], f)(*args)
            assert f != "place_order" or got == want
        env.step()
        for r in refs:
            r.step()
    same_rows(env.series(), cleared_rows(2), "nothing is folded before fold_series()")
    env.fold_series(sync=True)
    P.no_flags(env)
    want = cleared_rows(2)
    for n, x in dict(n_steps=6, n_two_sided=4, sum_m=204 + 206 + 204 + 204, sum_spread=4 + 2 + 4 + 4, sum_spread_sq=16 + 4 + 16 + 16,
                     sum_bid_vol=0 + 5 + 5 + 7 + 5 + 4, sum_ask_vol=4 * 3, sum_trade_vol=1, sum_trade_vol_sq=1, n_trade_steps=1,
                     n_ret=3, sum_d=0, sum_abs_d=4, sum_d2=8, sum_d4_lo=32, sum_d4_hi=0, max_abs_d=2, n_pairs=2, sum_dd=-4,
                     sum_abs_dd=4, min_m=204, max_m=206, carry_m=(3 << 62) | 204, carry_d=0).items():
        want[0][n] = x
    want[1]["n_steps"], want[1]["sum_bid_vol"] = 6, 5 * 9
    got = env.series()
    assert got.dtype == bk.SERIES_DTYPE and got.shape == (2,)
    same_rows(got, want, "by hand")
    # the oracle's books went through exactly these quotes, and the model folds them to the same rows
    hist = env.history()
    for b, r in enumerate(refs):
        P.same_history(hist[:, b], r.history(), f"L2 history of book {b}")
    same_rows(SM.rows(hist), want, "the model over the oracle's history")
    same_rows(env.series(1, 1), want[1:], "series(first_book, n_books)")
    env.fold_series(sync=True)  # no new step: no launch, nothing changes
    same_rows(env.series(), want, "a second fold_series() without a step")
    env.close()


# ------------------------------------------------------------------------------------------------ 2. / 3. bk_run
@pytest.mark.parametrize("pipeline", [None] + list(PIPELINES))
def test_run_folded_in_three_parts_equals_the_model_and_one_pass(bk, oracle, pipeline):
    """5 books (the last block of four waves holds one), a ring of 96: run(70) and fold - a lane's second step for six
    lanes - run(26) and fold - the ring at its last slots - run(40) and fold - the ring wrapped.  The same under every
    pipeline: the fold does not depend on who wrote the ring."""
    B, cap, parts = 5, 96, (70, 26, 40)
    hist = ref_books(oracle, B, 16, sum(parts), groups=C2).history()
    final = SM.rows(hist)
    assert (final["n_two_sided"] < final["n_steps"]).any() and (final["n_pairs"] > 0).all(), final[["n_steps", "n_two_sided", "n_pairs"]]
    d = np.diff(hist[:, :, 1].astype(np.int64) + hist[:, :, 2].astype(np.int64), axis=0)
    both = (hist[1:, :, 1] != 0) & (hist[:-1, :, 1] != 0) & (hist[1:, :, 2] != MAXU) & (hist[:-1, :, 2] != MAXU)
    assert (d[both] > 0).any() and (d[both] < 0).any()
    env = run_env(bk, B, cap)
    if pipeline:
        env.set_pipeline(pipeline)
    done = 0
    for n in parts:
        env.run(n, sync=False)
        env.fold_series()
        done += n
        same_rows(env.series(), SM.rows(hist[:done]), f"after {done} steps ({pipeline})")
    P.no_flags(env)
    same_rows(env.series(), final, "three folds against one pass of the model")
    P.same_history(env.history(), hist[done - cap:])
    env.close()


# ------------------------------------------------------------------------------------------------ 4. members, markets
def test_noise_and_momentum_members_folded_in_chunks_of_seven(bk, oracle):
    B, T = 3, 40
    hist = ref_books(oracle, B, 16, T, members=MEMBERS).history()
    env = run_env(bk, B, T, members=MEMBERS)
    for lo in range(0, T, 7):
        env.run(min(7, T - lo), sync=False)
        env.fold_series()
    P.no_flags(env)
    want = SM.rows(hist)
    assert (want["n_ret"] > 0).all()
    same_rows(env.series(), want, "Noise + Momentum")
    P.same_history(env.history(), hist)
    env.close()


def test_markets_keep_rows_per_book(bk, oracle):
    NM, ticks, T = 3, [2, 2], 30
    groups = [(0, 24, (40, 56), (10, 20), 2, 0.8), (1, 24, (40, 56), (10, 20), 2, 0.6), (1, 8, (40, 56), (50, 70), 2, 0.3)]
    env = bk.ManyMarketEnv(NM, SEED, 0, ticks, STEP, True, levels=10, max_live_orders=64, trade_capacity=4096, history_capacity=T)
    env.set_random_market_agents(groups)
    env.enable_series()
    ref = oracle.ManyMarkets(NM, SEED, 0, ticks, STEP, True, 10, groups)
    ref.run(T)
    hist = ref.history()
    for n in (11, 19):
        env.run(n, sync=False)
        env.fold_series()
    P.no_flags(env)
    want = SM.rows(hist)
    assert want.shape == (6,) and (want["n_two_sided"] > 0).all() and len({tuple(r.tolist()) for r in want}) == 6
    same_rows(env.series(), want, "markets, rows per book")
    P.same_history(env.history(), hist)
    env.close()


# ------------------------------------------------------------------------------------------------ 5. device ingress
def test_ingress_folded_after_every_step_equals_one_fold_at_the_end(bk, oracle):
    """fold_series() behind EVERY step takes the carry path every time (each lane-0 step reads the row's carry words); a twin
    env folds once at the end.  Bars and accounts run beside the table on the first env and still equal their own models."""
    import torch

    from test_gpu_accounts import busy_flow
    from test_gpu_accounts import same_rows as same_accounts
    from test_gpu_trade_bars import Tape, same_bars

    B, T, tick, NT, W = 4, 9, 2, 5, 3
    flows = [busy_flow(np.random.default_rng(20 + s), B, tick, idle=(1,) if s in (3, 4) else (), n_lo=30, n_hi=40) for s in range(T)]
    env = ingress_env(bk, torch, B, T, 256, 0, 64, tick=tick, n_ext=40)
    twin = ingress_env(bk, torch, B, T, 256, 0, 64, tick=tick, n_ext=40)
    env.enable_accounts(NT)
    env.enable_trade_bars(W)
    env.enable_series()
    twin.enable_series()
    tape, other = Tape(oracle, B, tick, env, torch), Tape(oracle, B, tick, twin, torch)
    for s, f in enumerate(flows):
        for t in (tape, other):
            t.submit(*f)
            t.step()
        env.fold_series()
        if s == 4:
            mid = env.series()
    twin.fold_series()
    hist = np.stack([r.history() for r in tape.refs], axis=1)
    want = SM.rows(hist)
    assert (want["n_pairs"] > 0).all() and (want["n_trade_steps"] > 0).all()
    same_rows(mid, SM.rows(hist[:5]), "after step 4")
    same_rows(env.series(), want, "folded after every step")
    same_rows(twin.series(), want, "folded once")
    for e in (env, twin):
        P.no_flags(e)
        P.same_history(e.history(), hist)
    same_bars(env.trade_bars(), tape.bars(W), "the bars beside the series")
    same_accounts(env.accounts(), tape.want(NT), "the accounts beside the series")
    env.close()
    twin.close()


# ------------------------------------------------------------------------------------------------ 6. lost steps
def test_lost_steps_refuse_the_fold_and_a_full_clear_recovers(bk, oracle):
    B = 3
    hist = ref_books(oracle, B, 16, 16, groups=C2).history()
    env = run_env(bk, B, 8)
    env.run(3)
    env.fold_series()
    before = env.series()
    same_rows(before, SM.rows(hist[:3]), "three steps")
    env.run(9)  # steps 3 .. 11 into a ring of 8: step 3 is gone
    lost(bk, env.fold_series, 1)
    same_rows(env.series(), before, "a refused fold leaves the rows")
    lost(bk, env.fold_series, 1)  # ... and the cursor
    lost(bk, lambda: env.clear_series(np.array([1, 0, 0], dtype=bool)), 1)
    same_rows(env.series(), before, "a refused clear leaves the rows")
    env.clear_series()
    same_rows(env.series(), cleared_rows(B), "clear_series() clears every row")
    env.run(2)
    env.fold_series()
    same_rows(env.series(), SM.rows(hist[12:14], first_step=12), "counted from the clear on")
    # the same through clear_history(): the two steps run since the last fold are no longer retained
    env.run(2)
    env.clear_history()
    lost(bk, env.fold_series, 2)
    env.clear_series()
    env.close()


# ------------------------------------------------------------------------------------------------ 7. resets
@pytest.mark.parametrize("kind", ["host", "device"])
def test_reset_books_cuts_the_carry_of_the_books_it_resets(bk, oracle, kind):
    """6 steps, save, fold; 5 steps NOT folded; reset books 0, 2, 4 - which folds the five first - then 7 steps.  A reset
    book replays steps 6 .. 12 of the same seed: its series is the oracle's steps 0 .. 10, a cut, steps 6 .. 12.  The sums
    go on; no return spans the reset."""
    B, n, m, k = 5, 6, 5, 7
    hist = ref_books(oracle, B, 16, n + m + k, groups=C2).history()
    env = run_env(bk, B, n + m + k, kind=kind)
    env.run(n)
    env.save_snapshot()
    env.fold_series()
    env.run(m)
    mask = np.array([1, 0, 1, 0, 1], dtype=bool)
    if kind == "device":
        import torch

        env.reset_books(torch.tensor(mask, device="cuda"), sync=False)
    else:
        env.reset_books(mask)
    at_reset = env.series()
    want = []
    for b in range(B):
        s = SM.fold(hist[:n + m, b])
        want.append(SM.row(SM.cut(s) if mask[b] else s))
    same_rows(at_reset, np.array(want, dtype=SM.SERIES_DTYPE), "the reset folded the five steps and cut the masked carries")
    assert not at_reset["carry_m"][mask].any() and not at_reset["carry_d"][mask].any() and at_reset["carry_m"][~mask].any()
    env.run(k)
    env.fold_series()
    want = []
    for b in range(B):
        if mask[b]:
            s = SM.fold(hist[n:n + k, b], cuts=[n + m], first_step=n + m, into=SM.fold(hist[:n + m, b]))
        else:
            s = SM.fold(hist[:, b])
        want.append(SM.row(s))
    want = np.array(want, dtype=SM.SERIES_DTYPE)
    assert (want["n_steps"] == n + m + k).all() and (want["n_ret"][mask] > 0).all()
    same_rows(env.series(), want, f"reset_books ({kind})")
    P.no_flags(env)
    env.close()


def test_a_reset_is_refused_when_steps_were_lost(bk, oracle):
    env = run_env(bk, 3, 8)
    env.run(2)
    env.save_snapshot()
    env.run(9)
    lost(bk, lambda: env.reset_books(np.array([1, 0, 0], dtype=bool)), 3)
    assert env.steps_done() == 11
    env.clear_series()
    env.reset_books(np.array([1, 0, 0], dtype=bool))
    env.close()


def test_reset_ingress_books_cuts_the_carry_too(bk, oracle):
    """3 steps, save, 3 steps, reset books 0 and 2 (a torch CUDA mask; the three steps are folded by the reset), 2 steps.
    The oracle cannot be rewound: a reset book's quotes after the reset are those of a REPLAY, a fresh oracle env given
    steps 0 .. 2 again and then the two steps after the reset (tests/test_gpu_accounts.py)."""
    import torch

    from test_gpu_accounts import Books, busy_flow

    B, tick = 4, 2
    env = ingress_env(bk, torch, B, 8, 256, 0, 64, tick=tick, n_ext=40)
    env.enable_series()
    books = Books(oracle, B, tick, env, torch)
    flows = [busy_flow(np.random.default_rng(60 + s), B, tick, n_lo=30, n_hi=40) for s in range(8)]

    def run(lo, hi, bs=books):
        for f in flows[lo:hi]:
            bs.submit(*f)
            bs.step()

    run(0, 3)
    env.save_ingress_snapshot()
    env.fold_series()
    run(3, 6)
    mask = np.array([1, 0, 1, 0], dtype=bool)
    env.reset_ingress_books(torch.tensor(mask, device="cuda"), sync=False)
    run(6, 8)
    env.fold_series()
    replay = Books(oracle, B, tick)
    run(0, 3, replay)
    run(6, 8, replay)
    want = []
    for b in range(B):
        h = books.refs[b].history()
        if mask[b]:
            s = SM.fold(replay.refs[b].history()[3:5], cuts=[6], first_step=6, into=SM.fold(h[:6]))
        else:
            s = SM.fold(h)
        want.append(SM.row(s))
    want = np.array(want, dtype=SM.SERIES_DTYPE)
    assert (want["n_steps"] == 8).all() and (want["n_two_sided"] > 4).all()
    same_rows(env.series(), want, "reset_ingress_books")
    P.no_flags(env)
    env.close()


# ------------------------------------------------------------------------------------------------ 8. clears and views
@pytest.mark.parametrize("kind", ["host", "device"])
def test_a_masked_clear_folds_first_and_the_view_is_the_table_in_place(bk, oracle, kind):
    import torch

    B = 5
    hist = ref_books(oracle, B, 16, 16, groups=C2).history()
    env = run_env(bk, B, 16, kind="device")
    view = torch.as_tensor(env.series_view(), device="cuda")
    assert tuple(view.shape) == (B, 24) and view.dtype == torch.int64 and view.data_ptr() == env.series_device_ptr()
    env.run(10, sync=False)  # (not folded: the masked clear folds the ten steps first)
    mask = np.array([1, 0, 1, 0, 0], dtype=bool)
    if kind == "host":
        env.clear_series(mask)
    else:
        env.clear_series(torch.tensor(mask, device="cuda"), sync=False)
    now = env.series()
    same_rows(now[mask], cleared_rows(2), "the masked rows are cleared, carry included")
    same_rows(now[~mask], SM.rows(hist[:10])[~mask], "the others hold the ten steps")
    env.run(6, sync=False)
    env.fold_series(sync=True)
    want = SM.rows(hist)
    want[mask] = SM.rows(hist[10:], first_step=10)[mask]
    same_rows(env.series(), want, f"after clear_series ({kind})")
    # the tensor made before any step sees the latest fold without a new call
    seen = np.ascontiguousarray(view.cpu().numpy()).view(SM.SERIES_DTYPE).reshape(B)
    same_rows(seen, want, "series_view() as a zero-copy tensor")
    P.no_flags(env)
    env.close()


# ------------------------------------------------------------------------------------------------ 9. checkpoints
def test_restore_clears_the_rows_and_rebases_the_cursor(bk, oracle):
    B = 3
    hist = ref_books(oracle, B, 16, 16, groups=C2).history()
    env = run_env(bk, B, 16)
    env.run(6)
    env.fold_series()
    ck = env.checkpoint()
    env.run(4)  # (outstanding when the checkpoint comes back: forgotten, not folded)
    env.restore(ck)
    assert env.steps_done() == 6
    same_rows(env.series(), cleared_rows(B), "restore clears every row")
    env.run(5)
    env.fold_series()
    same_rows(env.series(), SM.rows(hist[6:11], first_step=6), "counted from the restored step on")
    P.no_flags(env)
    env.close()


# ------------------------------------------------------------------------------------------------ 10. extremes
def test_extreme_prices_and_volumes(bk, oracle):
    """Host-driven, tick 1.  A bid of u32::MAX volume at 1 and an ask of u32::MAX volume at 0xFFFFFFFE rest; a small bid at
    0xFFFFFFFD comes and goes, so twice the mid jumps by 0xFFFFFFFC up and down, twice each - four fourth powers of just
    under 2^128; then an ask of u32::MAX volume at 1 takes the whole bid (trade_vol = u32::MAX, the book one-sided), the bid
    is placed again and taken again: sum_trade_vol_sq = 2 (2^32 - 1)^2 wraps.  The expected words are the model's over the
    oracle's history."""
    B, T = 2, 8
    env = bk.ManyBookEnv(B, SEED, 0, 1, 1000, levels=5, max_live_orders=16, max_orders=32, trade_capacity=16, history_capacity=T)
    refs = [oracle.StepEnv(SEED + b, 0, 1, 1000, True, 5) for b in range(B)]
    env.enable_series()
    steps = [[("place_order", (True, MAXU, 1, 1)), ("place_order", (False, MAXU, 2, 0xFFFFFFFE))],
             [("place_order", (True, 7, 3, 0xFFFFFFFD))], [("cancel_order", (2,))],
             [("place_order", (True, 7, 3, 0xFFFFFFFD))], [("cancel_order", (3,))],
             [("place_order", (False, MAXU, 4, 1))], [("place_order", (True, MAXU, 1, 1))], [("place_order", (False, MAXU, 4, 1))]]
    for ops in steps:
        for b in range(B):
            for f, args in ops:
                got, want = getattr(env, f)(b, *args), getattr(refs[b], f)(*args)
                assert f != "place_order" or got == want
        env.step()
        for r in refs:
            r.step()
    env.fold_series(sync=True)
    hist = env.history()
    for b, r in enumerate(refs):
        P.same_history(hist[:, b], r.history(), f"L2 history of book {b}")
    want = SM.rows(np.stack([r.history() for r in refs], axis=1))
    a = 0xFFFFFFFC
    for w in want:
        assert int(w["max_abs_d"]) == a and int(w["n_ret"]) == 4 and int(w["n_pairs"]) == 3 and int(w["sum_d"]) == 0
        assert 4 * a ** 4 > 1 << 128 and int(w["sum_d4_hi"]) == ((4 * a ** 4) >> 64) & M64 != 0
        assert int(w["sum_d4_lo"]) == (4 * a ** 4) & M64 and int(w["sum_d2"]) == (4 * a * a) & M64 != 4 * a * a
        assert int(w["sum_trade_vol"]) == 2 * MAXU and int(w["sum_trade_vol_sq"]) == (2 * MAXU * MAXU) & M64 == 0xFFFFFFFC00000002
        assert int(w["n_two_sided"]) == 6 and int(w["max_m"]) == (1 << 33) - 5 and int(w["min_m"]) == MAXU
        assert int(w["sum_dd"]) & M64 == (-3 * a * a) & M64 and int(w["sum_abs_dd"]) == (3 * a * a) & M64
    same_rows(env.series(), want, "extremes")
    env.close()


# ------------------------------------------------------------------------------------------------ 11. refusals
def test_refusals_leave_the_env_working(bk, oracle):
    env = make_env(bk, 2, groups=C2, steps=8)
    for call in (env.fold_series, env.series, env.series_device_ptr, env.series_view, env.clear_series,
                 lambda: env.clear_series(np.ones(2, dtype=bool))):
        refused(bk, call, "no series moments: call bk_series_enable first")
    env.run(2)
    env.enable_series()
    refused(bk, env.enable_series, "already enabled")
    with pytest.raises(ValueError):
        env.clear_series(np.ones(3, dtype=bool))
    with pytest.raises(ValueError):
        env.run_series(4, chunk=9)
    env.run(3)
    env.fold_series()
    hist = ref_books(oracle, 2, 16, 16, groups=C2).history()
    same_rows(env.series(), SM.rows(hist[2:5], first_step=2), "steps before enable_series() are not counted")
    env.close()
    none = make_env(bk, 2, groups=C2, steps=0)
    refused(bk, none.enable_series, "history_capacity must be > 0")
    none.run(2)
    none.close()
    # a host-driven env: a book cannot be loaded into an env with the table
    host = bk.ManyBookEnv(2, SEED, 0, 1, STEP, levels=5, max_live_orders=16, max_orders=16, trade_capacity=16, history_capacity=4)
    host.place_order(0, True, 5, 1, 100)
    host.step()
    state = host.book_state(0)
    host.load_book_state(1, state)
    host.enable_series()
    refused(bk, lambda: host.load_book_state(1, state), "series moments")
    host.step()
    host.fold_series(sync=True)
    assert host.series()["n_steps"].tolist() == [1, 1] and host.series()["sum_bid_vol"].tolist() == [5, 5]
    host.close()


# ------------------------------------------------------------------------------------------------ 12. run_series, moments
def test_run_series_runs_more_steps_than_the_ring_holds(bk, oracle):
    B, T = 5, 50
    hist = ref_books(oracle, B, 16, T, groups=C2).history()
    env = run_env(bk, B, 16)
    env.run_series(T, chunk=16)
    assert env.steps_done() == T
    env.sync()
    P.no_flags(env)
    rows = env.series()
    same_rows(rows, SM.rows(hist), "run_series(50, chunk=16) on a ring of 16")
    P.same_history(env.history(), hist[T - 16:])
    got = bk.series_moments(rows)
    for b in range(B):
        h = hist[:, b].astype(np.float64)
        tv, bid, ask, av, bv = (h[:, i] for i in range(5))
        two = (hist[:, b, 1] != 0) & (hist[:, b, 2] != MAXU)
        m = bid + ask
        ret = two[1:] & two[:-1]
        d = (m[1:] - m[:-1])[ret]
        pair = ret[1:] & ret[:-1]
        dd = ((m[2:] - m[1:-1]) * (m[1:-1] - m[:-2]))[pair]
        want = dict(
            mean_mid=np.mean(m[two]) / 2, mean_spread=np.mean((ask - bid)[two]), var_spread=np.var((ask - bid)[two]),
            mean_return=np.mean(d) / 2, var_return=np.var(d / 2), kurtosis_return=len(d) * np.sum(d ** 4) / np.sum(d ** 2) ** 2 - 3,
            acf1_return=(np.mean(dd) - np.mean(d) ** 2) / np.var(d),
            acf1_abs_return=(np.mean(np.abs(dd)) - np.mean(np.abs(d)) ** 2) / np.var(np.abs(d)),
            mean_trade_vol=np.mean(tv), mean_bid_vol=np.mean(bv), mean_ask_vol=np.mean(av))
        assert len(dd) > 10
        for k, v in want.items():
            assert abs(got[b][k] - v) <= 1e-12 * abs(v), (b, k, got[b][k], v)
    env.clear_series()
    none = bk.series_moments(env.series())
    assert all(np.isnan(none[k]).all() for k in none.dtype.names)
    env.close()
