"""The per-book lag table of the level-2 history (bk_lags_enable; bourse_amd/csrc/lags.hpp): K rows of ten integer words
per book, one per lag, folded on the device from the history ring, and the carry that makes every split of a fold equal.

The expected side never shares code with the kernel: tests/lags_model.py::fold (plain Python ints) over the ORACLE's
history() of the same run - oracle.ManyBooks / ManyMarkets for bk_run, one oracle.StepEnv per book for the host-driven and
the device-ingress flows - and the device's own history is held against the oracle's through tests/oracle_parity.py where
the ring still retains it; case 1's rows are literal numbers worked out by hand.  Where a case says something only under a
condition - one-sided steps, pairs at the deepest lag, products of both signs, a word that wraps - the condition is asserted
on the expected side before anything is compared.  All comparisons are exact.

Here: the lag table's own cases. What it shares with the other two tables is written once: the three scenarios at the end
of this file in tests/hist_tables.py, the rest - the other flows, lost steps, the ingress reset, a restore, the refusals -
in tests/test_gpu_hist_tables.py[lags]."""
import numpy as np
import pytest

pytest.register_assert_rewrite("hist_tables")  # (a support module: its asserts report their values too)

import lags_model as LM  # noqa: E402
import oracle_parity as P  # noqa: E402
import series_model as SM  # noqa: E402
from hist_tables import LAGS as TABLE  # noqa: E402
from hist_tables import (bk, host_driven, lost, masked_clear_folds_first, refused, reset_books_cuts_the_carry, run_env,  # noqa: E402,F401
                         run_folded_in_three_parts, same_as_series)
from test_gpu_reset_books import C2, PIPELINES, ref_books  # noqa: E402

pytestmark = pytest.mark.gpu
M64 = (1 << 64) - 1
M128 = (1 << 128) - 1
same_rows, zeros, model = TABLE.same, TABLE.cleared, TABLE.model


# ------------------------------------------------------------------------------------------------ 1. by hand
def test_rows_worked_out_by_hand(bk, oracle):
    """tests/test_gpu_series.py's hand case: two books, tick 1, a ring of 8, six host-driven steps, one call per step.
    Book 0 is empty at s0, one-sided at s1, and two-sided from s2 on with m = 204, 206, 204, 204: d = +2, -2, 0.
      lag 1: pairs (-2)(+2), (0)(-2); spans +2, -2, 0      lag 2: pair (0)(+2); spans 204 - 204, 204 - 206
      lag 3: no pair (r_2 is false); span 204 - 204
    Book 1 gets one bid and is never two-sided."""
    K = 3
    steps = [[], [("place_order", (0,), (True, 5, 1, 100)), ("place_order", (1,), (True, 9, 1, 50))],
             [("place_order", (0,), (False, 3, 2, 104))], [("place_order", (0,), (True, 2, 3, 102))], [("cancel_order", (0,), (2,))],
             [("place_order", (0,), (False, 1, 4, 100))]]
    (env,), refs = host_driven(bk, oracle, 2, 8, [lambda e: e.enable_lags(K)], steps, max_orders=16)
    same_rows(env.lags(), zeros(2, K), "nothing is folded before fold_lags()")
    env.fold_lags(sync=True)
    P.no_flags(env)
    want = zeros(2, K)
    for k, words in enumerate([(2, -4, 4, 3, 0, 4, 8, 32, 0, 2), (1, 0, 0, 2, -2, 2, 4, 16, 0, 2), (0, 0, 0, 1, 0, 0, 0, 0, 0, 0)]):
        for n, x in zip(LM.FIELDS, words):
            want[0, k][n] = x
    got = env.lags()
    assert got.dtype == bk.LAG_DTYPE and got.shape == (2, K)
    same_rows(got, want, "by hand")
    hist = env.history()
    for b, r in enumerate(refs):
        P.same_history(hist[:, b], r.history(), f"L2 history of book {b}")
    same_rows(LM.rows(np.stack([r.history() for r in refs], axis=1), K), want, "the model over the oracle's history")
    same_rows(env.lags(1, 1), want[1:], "lags(first_book, n_books)")
    env.fold_lags(sync=True)  # no new step: no launch, nothing changes
    same_rows(env.lags(), want, "a second fold_lags() without a step")
    env.close()


# ------------------------------------------------------------------------------------------------ 3. single steps
@pytest.mark.parametrize("K", [64, 5])
def test_single_step_folds_with_a_carry_deeper_than_the_ring(bk, oracle, K):
    """A ring of 8 and 24 folds of one step each: from step 8 on every word the fold reads beyond its own step comes from
    the carry, which at K = 64 reaches 65 steps back - eight times the ring."""
    B, T = 3, 24
    hist = ref_books(oracle, B, 16, T, groups=C2).history()
    env = run_env(bk, TABLE, B, 8, K)
    sums = [LM.cleared(K) for _ in range(B)]
    for t in range(T):
        env.run(1, sync=False)
        env.fold_lags()
        for b in range(B):
            LM.fold(hist[t:t + 1, b], first_step=t, into=sums[b])
        want = np.array([LM.table(s) for s in sums], dtype=LM.LAG_DTYPE)
        same_rows(env.lags(), want, f"after step {t} (K = {K})")
    assert (want[:, min(K, 16) - 1]["n_h"] > 0).all() and (want[:, 0]["n_pairs"] > 0).all()
    same_rows(want, LM.rows(hist, K), "the model is split-invariant")
    P.no_flags(env)
    P.same_history(env.history(), hist[T - 8:])
    env.close()


# ------------------------------------------------------------------------------------------------ 6. resets, clears
@pytest.mark.parametrize("kind", ["host", "device"])
def test_reset_markets_cuts_the_carry_of_every_book_of_a_masked_market(bk, oracle, kind):
    """3 markets x 2 assets: the mask has one byte per MARKET and the cut must reach both books of markets 0 and 2 and
    neither book of market 1.  6 steps, save, 5 steps not folded, reset, 7 steps: as the books' case (tests/hist_tables.py)."""
    from test_gpu_reset_books import MKT_GROUPS, MKT_TICKS, as_kind, market_env, ref_markets

    NM, A, n, m, k, K = 3, 2, 6, 5, 7, 4
    hist = ref_markets(oracle, NM, ((n + m + k, True),)).history()
    assert hist.shape[:2] == (n + m + k, NM * A)
    env = market_env(bk, NM, MKT_TICKS, n + m + k, MKT_GROUPS, kind)
    env.enable_lags(K)
    env.run(n)
    env.save_snapshot()
    env.run(m)
    mask = np.array([1, 0, 1], dtype=bool)
    mm, _ = as_kind(mask, kind)
    env.reset_markets(mm, sync=(kind == "host"))
    env.run(k)
    env.fold_lags()
    want = []
    for b in range(NM * A):
        # what the book went through: a reset one replays steps n .. n + k - 1 behind a cut, a kept one has no cut
        went = np.concatenate([hist[:n + m, b], hist[n:n + k, b]]) if mask[b // A] else hist[:, b]
        cut, uncut = (LM.table(LM.fold(went, K, cuts=c)) for c in ([n + m], []))
        assert (cut != uncut).any(), f"a cut would show in book {b}"
        want.append(cut if mask[b // A] else uncut)
    same_rows(env.lags(), np.array(want, dtype=LM.LAG_DTYPE), f"reset_markets ({kind})")
    P.no_flags(env)
    env.close()


def test_a_reset_is_refused_when_steps_were_lost_and_changes_neither_table(bk, oracle):
    """Both tables on: the series is folded up to step 7, the lag table never; at step 11 a ring of 8 has lost three of the
    lag table's steps and none of the series'.  The reset is refused before the series folds its four outstanding steps."""
    B, K = 3, 4
    env = run_env(bk, TABLE, B, 8, K)
    env.enable_series()
    env.run(2)
    env.save_snapshot()
    env.run(5)
    env.fold_series()
    series_at_7 = env.series()
    env.run(4)
    lost(bk, TABLE, lambda: env.reset_books(np.array([1, 0, 0], dtype=bool)), 3)
    assert env.steps_done() == 11
    got = env.series()
    assert all((got[f] == series_at_7[f]).all() for f in SM.FIELDS) and (got["n_steps"] == 7).all()
    same_rows(env.lags(), zeros(B, K), "the lag table is untouched")
    env.clear_lags()
    env.reset_books(np.array([1, 0, 0], dtype=bool))
    assert (env.series()["n_steps"] == 11).all()  # (now the reset went through: the series folded its four steps)
    env.close()


# ------------------------------------------------------------------------------------------------ 7. extremes, run_series
def test_jumps_between_the_ends_of_the_price_range(bk, oracle):
    """Host-driven, tick 1: the second hand case on the device.  A bid at 1 and an ask at 0xFFFFFFFE rest for good, an ask
    of volume 1 at 2 makes m = 3.  Two equal bids of volume 1 at 0xFFFFFFFD in ONE step - the first takes the ask at 2, the
    second rests, whichever comes first in the step's shuffle - make m = 2^33 - 5: d = +(2^33 - 8).  Two equal asks of
    volume 1 at 2 take it back: d = -(2^33 - 8).  Twice each: a * a wraps 2^64 in every term, a^4 is reduced modulo 2^128,
    the lag-1 products are negative and the lag-2 products positive."""
    B, K = 2, 3
    up = [("place_order", range(B), (True, 1, 3, 0xFFFFFFFD))] * 2
    down = [("place_order", range(B), (False, 1, 4, 2))] * 2
    steps = [[("place_order", range(B), (True, 50, 1, 1)), ("place_order", range(B), (False, 50, 2, 0xFFFFFFFE)),
              ("place_order", range(B), (False, 1, 2, 2))], up, down, up, down]
    (env,), refs = host_driven(bk, oracle, B, 8, [lambda e: e.enable_lags(K)], steps, step_size=1000)
    env.fold_lags(sync=True)
    hist = env.history()
    for b, r in enumerate(refs):
        P.same_history(hist[:, b], r.history(), f"L2 history of book {b}")
    want = LM.rows(np.stack([r.history() for r in refs], axis=1), K)
    a = (1 << 33) - 8
    assert a * a > M64 and a ** 4 > M128

    def i64(x):  # a sum modulo 2^64 read as two's complement
        x &= M64
        return x - (1 << 64) if x >> 63 else x

    for w in want:
        assert [int(x) for x in w[0].tolist()] == [3, i64(-3 * a * a), (3 * a * a) & M64, 4, 0, 4 * a, (4 * a * a) & M64,
                                                   (4 * a ** 4) & M64, ((4 * a ** 4) & M128) >> 64, a]
        assert [int(x) for x in w[1].tolist()] == [2, i64(2 * a * a), (2 * a * a) & M64, 3, 0, 0, 0, 0, 0, 0]
        assert [int(x) for x in w[2].tolist()] == [1, i64(-a * a), (a * a) & M64, 2, 0, 2 * a, (2 * a * a) & M64,
                                                   (2 * a ** 4) & M64, ((2 * a ** 4) & M128) >> 64, a]
        assert int(w[0]["sum_h4_hi"]) != 0 and i64(-3 * a * a) != -3 * a * a
    same_rows(env.lags(), want, "extremes")
    env.close()


@pytest.mark.parametrize("series", [False, True])
def test_run_series_runs_more_steps_than_the_ring_holds(bk, oracle, series):
    B, T, K = 5, 50, 20
    hist = ref_books(oracle, B, 16, T, groups=C2).history()
    env = run_env(bk, TABLE, B, 16, K)
    if series:
        env.enable_series()
    env.run_series(T, chunk=16)
    assert env.steps_done() == T
    env.sync()
    P.no_flags(env)
    rows = env.lags()
    want = model(hist, K, ("run_series", K, T))
    assert (want[:, K - 1]["n_pairs"] > 0).all()
    same_rows(rows, want, "run_series(50, chunk=16) on a ring of 16")
    P.same_history(env.history(), hist[T - 16:])
    if series:
        got = env.series()
        assert (got["n_steps"] == T).all()
        same_as_series(rows, got, "run_series with both tables")
        # at lag 1 the moments are the series' bit for bit
        lm, sm = bk.lag_moments(rows), bk.series_moments(got)
        assert lm.shape == (B, K)
        for a, b in (("acf_return", "acf1_return"), ("acf_abs_return", "acf1_abs_return"), ("var_h", "var_return")):
            assert (lm[:, 0][a] == sm[b]).all() and not np.isnan(sm[b]).any(), (a, lm[:, 0][a], sm[b])
    else:
        refused(bk, env.fold_series, "no series moments")
    env.close()


# ------------------------------------------------------------------------------------------------ 8. refusals


# ------------------------------------------------------------------------------------------------ 9. the shared scenarios
# (written once in tests/hist_tables.py for the three tables; the rest of what they share is tests/test_gpu_hist_tables.py)
@pytest.mark.parametrize("K,pipeline", [(64, None)] + [(64, p) for p in PIPELINES] + [(1, None), (5, None)])
def test_run_folded_in_three_parts_equals_the_model_and_one_pass(bk, oracle, K, pipeline):
    run_folded_in_three_parts(bk, oracle, TABLE, K, pipeline)


@pytest.mark.parametrize("kind", ["host", "device"])
def test_reset_books_cuts_the_carry_of_the_books_it_resets(bk, oracle, kind):
    reset_books_cuts_the_carry(bk, oracle, TABLE, kind)


@pytest.mark.parametrize("kind", ["host", "device"])
def test_a_masked_clear_folds_first_and_the_view_is_the_table_in_place(bk, oracle, kind):
    masked_clear_folds_first(bk, oracle, TABLE, kind)
