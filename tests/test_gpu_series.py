"""Per-book series moments of the level-2 history (bk_series_enable; bourse_amd/csrc/series.hpp): one row of 24 integer
words per book, folded on the device from the history ring.

The expected side never shares code with the kernel: tests/series_model.py::fold (plain Python ints) over the ORACLE's
history() of the same run - oracle.ManyBooks / ManyMarkets for bk_run, one oracle.StepEnv per book for the host-driven and
the device-ingress flows - and the device's own history is held against the oracle's through tests/oracle_parity.py where
the ring still retains it; case 1's rows are literal numbers worked out by hand.  Where a case says something only under a
condition - one-sided steps, pairs, returns of both signs, a word that wraps - the condition is asserted on the expected
side before anything is compared.

Here: the series' own cases. What it shares with the other two tables is written once: the three scenarios at the end of
this file in tests/hist_tables.py, the rest - the other flows, lost steps, the ingress reset, a restore, the refusals - in
tests/test_gpu_hist_tables.py[series]."""
import numpy as np
import pytest

pytest.register_assert_rewrite("hist_tables")  # (a support module: its asserts report their values too)

import oracle_parity as P  # noqa: E402
import series_model as SM  # noqa: E402
from hist_tables import SERIES as TABLE  # noqa: E402
from hist_tables import bk, lost, masked_clear_folds_first, reset_books_cuts_the_carry, run_env, run_folded_in_three_parts  # noqa: E402,F401 (bk is a fixture)
from test_gpu_reset_books import C2, PIPELINES, STEP, ref_books  # noqa: E402

pytestmark = pytest.mark.gpu
same_rows, cleared_rows = TABLE.same, TABLE.cleared
M64 = (1 << 64) - 1
MAXU = 0xFFFFFFFF
SEED = 101


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


# ------------------------------------------------------------------------------------------------ 7. resets
def test_a_reset_is_refused_when_steps_were_lost(bk, oracle):
    env = run_env(bk, TABLE, 3, 8)
    env.run(2)
    env.save_snapshot()
    env.run(9)
    lost(bk, TABLE, lambda: env.reset_books(np.array([1, 0, 0], dtype=bool)), 3)
    assert env.steps_done() == 11
    env.clear_series()
    env.reset_books(np.array([1, 0, 0], dtype=bool))
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


# ------------------------------------------------------------------------------------------------ 12. run_series, moments
def test_run_series_runs_more_steps_than_the_ring_holds(bk, oracle):
    B, T = 5, 50
    hist = ref_books(oracle, B, 16, T, groups=C2).history()
    env = run_env(bk, TABLE, B, 16)
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


# ------------------------------------------------------------------------------------------------ 13. the shared scenarios
# (written once in tests/hist_tables.py for the three tables; the rest of what they share is tests/test_gpu_hist_tables.py)
@pytest.mark.parametrize("pipeline", [None] + list(PIPELINES))
def test_run_folded_in_three_parts_equals_the_model_and_one_pass(bk, oracle, pipeline):
    run_folded_in_three_parts(bk, oracle, TABLE, None, pipeline)


@pytest.mark.parametrize("kind", ["host", "device"])
def test_reset_books_cuts_the_carry_of_the_books_it_resets(bk, oracle, kind):
    reset_books_cuts_the_carry(bk, oracle, TABLE, kind)


@pytest.mark.parametrize("kind", ["host", "device"])
def test_a_masked_clear_folds_first_and_the_view_is_the_table_in_place(bk, oracle, kind):
    masked_clear_folds_first(bk, oracle, TABLE, kind)
