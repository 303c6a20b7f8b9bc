"""The per-book bin table of the level-2 history (bk_bins_enable; bourse_amd/csrc/bins.hpp): per book S + 2 rows of B u64
counts - the change of twice the mid over S spans, the spread, the traded volume - folded on the device from the history
ring, and the carry that makes every split of a fold equal.

The expected side never shares code with the kernel: tests/bins_model.py::fold (plain Python ints) over the ORACLE's
history() of the same run - oracle.ManyBooks / ManyMarkets for bk_run, one oracle.StepEnv per book for the host-driven and
the device-ingress flows - and the device's own history is held against the oracle's through tests/oracle_parity.py where
the ring still retains it; case 1's counts are literal numbers worked out by hand.  Where a case says something only under a
condition - one-sided steps, counts at the deepest span, clamped values, traded steps - the condition is asserted on the
expected side before anything is compared.  All comparisons are exact.

Here: the bin table's own cases, and the reset that all three tables refuse. What it shares with the other two tables is
written once: the three scenarios at the end of this file in tests/hist_tables.py, the rest - the other flows, lost steps,
the ingress reset, a restore, the refusals - in tests/test_gpu_hist_tables.py[bins]."""
import numpy as np
import pytest

pytest.register_assert_rewrite("hist_tables")  # (a support module: its asserts report their values too)

import bins_model as BM  # noqa: E402
import lags_model as LM  # noqa: E402
import oracle_parity as P  # noqa: E402
import series_model as SM  # noqa: E402
from hist_tables import BINS as TABLE  # noqa: E402
from hist_tables import (LAGS, SERIES, bk, host_driven, lost, masked_clear_folds_first, refused, reset_books_cuts_the_carry,  # noqa: E402,F401
                         run_env, run_folded_in_three_parts)
from test_gpu_reset_books import C2, PIPELINES, ref_books  # noqa: E402

pytestmark = pytest.mark.gpu
MAXU = 0xFFFFFFFF
same_bins, zeros, model, enable = TABLE.same, TABLE.cleared, TABLE.model, TABLE.enable


def at(B, **bins):
    r = np.zeros(B, dtype=np.uint64)
    for i, c in bins.items():
        r[int(i[1:])] = c
    return r


# ------------------------------------------------------------------------------------------------ 1. by hand
def test_counts_worked_out_by_hand(bk, oracle):
    """tests/test_gpu_series.py's hand case: two books, tick 1, a ring of 8, six host-driven steps, one call per step.
    Book 0 is empty at s0, one-sided at s1, and two-sided from s2 on with m = 204, 206, 204, 204 and spreads 4, 2, 4, 4; the
    ask of volume 1 at 100 in s5 trades.  Spans (1, 3), 8 bins of width 1:
      span 1: +2, -2, 0 -> bins 6, 2, 4      span 3: 204 - 204 at s5 -> bin 4
      spread: bins 4, 2, 4, 4                volume: five steps in bin 0, s5 in bin 1
    Book 1 gets one bid and is never two-sided: its six steps count in the volume channel only."""
    cfg = BM.config((1, 3), 8)
    steps = [[], [("place_order", (0,), (True, 5, 1, 100)), ("place_order", (1,), (True, 9, 1, 50))],
             [("place_order", (0,), (False, 3, 2, 104))], [("place_order", (0,), (True, 2, 3, 102))], [("cancel_order", (0,), (2,))],
             [("place_order", (0,), (False, 1, 4, 100))]]
    (env,), refs = host_driven(bk, oracle, 2, 8, [lambda e: enable(e, cfg)], steps, max_orders=16)
    same_bins(env.bins(), zeros(2, cfg), "nothing is folded before fold_bins()")
    env.fold_bins(sync=True)
    P.no_flags(env)
    want = zeros(2, cfg)
    want[0] = [at(8, b2=1, b4=1, b6=1), at(8, b4=1), at(8, b2=1, b4=3), at(8, b0=5, b1=1)]
    want[1, 3] = at(8, b0=6)
    got = env.bins()
    assert got.dtype == np.uint64 and got.shape == (2, 4, 8)
    same_bins(got, want, "by hand")
    hist = env.history()
    for b, r in enumerate(refs):
        P.same_history(hist[:, b], r.history(), f"L2 history of book {b}")
    same_bins(BM.rows(np.stack([r.history() for r in refs], axis=1), cfg), want, "the model over the oracle's history")
    same_bins(env.bins(1, 1), want[1:], "bins(first_book, n_books)")
    env.fold_bins(sync=True)  # no new step: no launch, nothing changes
    same_bins(env.bins(), want, "a second fold_bins() without a step")
    back = env.bins_config()
    assert back.dtype == bk.BINS_CONFIG_DTYPE and back["spans"].tolist() == [1, 3, 0, 0]
    assert [int(back[n]) for n in ("n_bins", "n_spans", "ret_width", "spread_width", "vol_width")] == [8, 2, 1, 1, 1]
    assert (bk.bin_edges(back) == bk.bin_edges(cfg)).all()
    env.close()


# ------------------------------------------------------------------------------------------------ 2. bk_run
@pytest.mark.parametrize("cfg", [BM.config((1, 5, 64), 2), BM.config((1, 5, 20, 64), 256), BM.config((64, 1, 5), 64, 3, 2, 7),
                                 BM.config((5, 5), 16, 2, 1, 40)], ids=["B2", "B256x4", "widths327", "twice5"])
def test_bin_counts_widths_and_span_orders(bk, oracle, cfg):
    """The smallest and the largest table (2 and 256 bins; six channels of 256 are the 24 KB of LDS a block may ask for),
    widths (3, 2, 7) with the spans out of order, and one span twice: 70 + 26 + 40 steps on a ring of 96."""
    B, cap, parts = 5, 96, (70, 26, 40)
    hist = ref_books(oracle, B, 16, sum(parts), groups=C2).history()
    want = model(hist, cfg, ("run", sum(parts)))
    if cfg["n_bins"] == 2:
        assert (want[:, 0] > 0).all(), "both halves of the return axis are hit"
    if cfg["ret_width"] == 3:
        m = hist[:, :, 1].astype(np.int64) + hist[:, :, 2].astype(np.int64)
        two = (hist[:, :, 1] != 0) & (hist[:, :, 2] != MAXU)
        d = (m[1:] - m[:-1])[two[1:] & two[:-1]]
        assert ((d < 0) & (d % 3 != 0)).any(), "a negative return that a truncating division would put one bin too high"
    if cfg["spans"] == (5, 5):
        assert (want[:, 0] == want[:, 1]).all() and want[:, 0].any()
    env = run_env(bk, TABLE, B, cap, cfg)
    for n in parts:
        env.run(n, sync=False)
        env.fold_bins()
    P.no_flags(env)
    same_bins(env.bins(), want, f"{cfg}")
    env.close()


# ------------------------------------------------------------------------------------------------ 3. single steps
def test_single_step_folds_with_a_carry_deeper_than_the_ring(bk, oracle):
    """A ring of 8 and 24 folds of one step each at spans (64, 3, 12): from step 8 on every partner comes from the carry,
    which reaches 64 steps back - eight times the ring."""
    B, T = 3, 24
    cfg = BM.config((64, 3, 12), 64)
    hist = ref_books(oracle, B, 16, T, groups=C2).history()
    env = run_env(bk, TABLE, B, 8, cfg)
    sums = [BM.cleared(cfg) for _ in range(B)]
    for t in range(T):
        env.run(1, sync=False)
        env.fold_bins()
        for b in range(B):
            BM.fold(hist[t:t + 1, b], first_step=t, into=sums[b])
        want = np.array([BM.table(s) for s in sums], dtype=np.uint64)
        same_bins(env.bins(), want, f"after step {t}")
    assert (want[:, 2].sum(axis=1) > 0).all() and (want[:, 1].sum(axis=1) > 0).all() and not want[:, 0].any()
    same_bins(want, BM.rows(hist, cfg), "the model is split-invariant")
    P.no_flags(env)
    P.same_history(env.history(), hist[T - 8:])
    env.close()


# ------------------------------------------------------------------------------------------------ 6. resets, clears
@pytest.mark.parametrize("kind", ["host", "device"])
def test_reset_markets_cuts_the_carry_of_every_book_of_a_masked_market(bk, oracle, kind):
    """3 markets x 2 assets: the mask has one byte per MARKET and the cut must reach both books of markets 0 and 2 and
    neither book of market 1.  6 steps, save, 5 steps not folded, reset, 7 steps: as the books' case (tests/hist_tables.py)."""
    from test_gpu_reset_books import MKT_GROUPS, MKT_TICKS, as_kind, market_env, ref_markets

    NM, A, n, m, k = 3, 2, 6, 5, 7
    cfg = BM.config((1, 4), 64)
    hist = ref_markets(oracle, NM, ((n + m + k, True),)).history()
    assert hist.shape[:2] == (n + m + k, NM * A)
    env = market_env(bk, NM, MKT_TICKS, n + m + k, MKT_GROUPS, kind)
    enable(env, cfg)
    env.run(n)
    env.save_snapshot()
    env.run(m)
    mask = np.array([1, 0, 1], dtype=bool)
    mm, _ = as_kind(mask, kind)
    env.reset_markets(mm, sync=(kind == "host"))
    env.run(k)
    env.fold_bins()
    want = []
    for b in range(NM * A):
        # what the book went through: a reset one replays steps n .. n + k - 1 behind a cut, a kept one has no cut
        went = np.concatenate([hist[:n + m, b], hist[n:n + k, b]]) if mask[b // A] else hist[:, b]
        cut, uncut = (BM.table(BM.fold(went, cfg, cuts=c)) for c in ([n + m], []))
        assert (cut != uncut).any(), f"a cut would show in book {b}"
        want.append(cut if mask[b // A] else uncut)
    same_bins(env.bins(), np.array(want, dtype=np.uint64), f"reset_markets ({kind})")
    P.no_flags(env)
    env.close()


def test_a_reset_is_refused_when_steps_were_lost_and_changes_none_of_the_three_tables(bk, oracle):
    """All three tables on: the series and the lag table are folded up to step 7, the bin table never; at step 11 a ring
    of 8 has lost three of the bin table's steps and none of the siblings'.  The reset is refused before either sibling folds
    its four outstanding steps.  Then the other way round: the bin table is up to date and the lag table has lost steps.
    Then the series has lost a step while the lag and the bin table each have four outstanding: the three checks stand in
    one loop in front of the loop that folds, and the message is that of the last check."""
    B = 3
    cfg = BM.config((1, 4), 64)
    env = run_env(bk, TABLE, B, 8, cfg)
    env.enable_series()
    env.enable_lags(4)
    env.run(2)
    env.save_snapshot()
    env.run(5)
    env.fold_series()
    env.fold_lags()
    series_at_7, lags_at_7 = env.series(), env.lags()
    env.run(4)
    mask = np.array([1, 0, 0], dtype=bool)
    lost(bk, TABLE, lambda: env.reset_books(mask), 3)
    assert env.steps_done() == 11
    got = env.series()
    assert all((got[f] == series_at_7[f]).all() for f in SM.FIELDS) and (got["n_steps"] == 7).all()
    assert all((env.lags()[f] == lags_at_7[f]).all() for f in LM.FIELDS)
    same_bins(env.bins(), zeros(B, cfg), "the bin table is untouched")
    env.clear_bins()
    env.reset_books(mask)
    assert (env.series()["n_steps"] == 11).all()  # (now the reset went through: the siblings folded their four steps)
    assert (env.lags()[:, 0]["n_h"] > lags_at_7[:, 0]["n_h"]).any()
    same_bins(env.bins(), zeros(B, cfg), "cleared at step 11 and nothing run since")
    # the lag table falls out of the ring, the bin table does not: refused by the lag table, the bin table not folded
    env.run(5)
    env.fold_bins()
    env.fold_series()
    at_16 = env.bins()
    assert (at_16[:, 3].sum(axis=1) == 5).all()
    env.run(4)
    with pytest.raises(bk.BourseError, match=r"\b1 step\(s\) of the lag table were lost"):
        env.reset_books(mask)
    same_bins(env.bins(), at_16, "a reset the lag table refused leaves the bin table")
    assert (env.series()["n_steps"] == 16).all()
    # the series falls out of the ring - the LAST check in the order - with four steps of both siblings outstanding: refused
    # with the series' message, and neither sibling folded
    env.clear_lags()
    env.fold_bins()
    env.fold_series()
    env.run(5)
    env.fold_bins()
    env.fold_lags()
    bins_at_25, lags_at_25, series_at_20 = env.bins(), env.lags(), env.series()
    assert (bins_at_25[:, 3].sum(axis=1) == 14).all() and (series_at_20["n_steps"] == 20).all() and lags_at_25[:, 0]["n_h"].any()
    env.run(4)
    lost(bk, SERIES, lambda: env.reset_books(mask), 1)
    assert env.steps_done() == 29
    same_bins(env.bins(), bins_at_25, "a reset the series refused leaves the bin table")
    LAGS.same(env.lags(), lags_at_25, "a reset the series refused leaves the lag table")
    SERIES.same(env.series(), series_at_20, "... and the series")
    env.clear_series()
    env.reset_books(mask)
    assert (env.bins()[:, 3].sum(axis=1) == 18).all()  # (now the reset went through: the siblings folded their four steps)
    env.close()


# ------------------------------------------------------------------------------------------------ 7. extremes, run_series
def test_jumps_between_the_ends_of_the_price_range(bk, oracle):
    """Host-driven, tick 1 (tests/test_gpu_lags.py's extremes): a bid at 1 and an ask at 0xFFFFFFFE rest for good, an ask of
    volume 1 at 2 makes m = 3; two equal bids at 0xFFFFFFFD in one step make m = 2^33 - 5, two equal asks at 2 take it
    back.  h = +-(2^33 - 8) twice each: at ret_width 1 and 256 bins it is clamped into the two end bins; at ret_width
    0xFFFFFFFF and 8 bins floor(h / w) is +1 and -2.  The spread is 1 at both ends - bin 1, or bin 0 at spread_width
    0xFFFFFFFF - and every jump step trades volume 1."""
    B = 2
    cfgs = [BM.config((1, 2), 256, 1, 1, 1), BM.config((1, 2), 8, MAXU, MAXU, MAXU)]
    up = [("place_order", range(B), (True, 1, 3, 0xFFFFFFFD))] * 2
    down = [("place_order", range(B), (False, 1, 4, 2))] * 2
    steps = [[("place_order", range(B), (True, 50, 1, 1)), ("place_order", range(B), (False, 50, 2, 0xFFFFFFFE)),
              ("place_order", range(B), (False, 1, 2, 2))], up, down, up, down]
    envs, refs = host_driven(bk, oracle, B, 8, [lambda e, c=c: enable(e, c) for c in cfgs], steps, step_size=1000)
    ref_hist = np.stack([r.history() for r in refs], axis=1)
    assert ref_hist[:, 0, 1].tolist() == [1, 0xFFFFFFFD, 1, 0xFFFFFFFD, 1] and ref_hist[:, 0, 2].tolist() == [2, 0xFFFFFFFE] * 2 + [2]
    assert ref_hist[:, 0, 0].tolist() == [0, 1, 1, 1, 1]
    for env, cfg in zip(envs, cfgs):
        env.fold_bins(sync=True)
        hist = env.history()
        for b, r in enumerate(refs):
            P.same_history(hist[:, b], r.history(), f"L2 history of book {b}")
        want = BM.rows(ref_hist, cfg)
        nb = cfg["n_bins"]
        for w in want:
            if nb == 256:
                assert (w[0] == at(256, b0=2, b255=2)).all() and (w[1] == at(256, b128=3)).all()
                assert (w[2] == at(256, b1=5)).all() and (w[3] == at(256, b0=1, b1=4)).all()
            else:
                assert (w[0] == at(8, b2=2, b5=2)).all() and (w[1] == at(8, b4=3)).all()
                assert (w[2] == at(8, b0=5)).all() and (w[3] == at(8, b0=5)).all()
        same_bins(env.bins(), want, f"extremes at ret_width {cfg['ret_width']}")
        env.close()


def test_run_series_runs_more_steps_than_the_ring_holds_with_all_three_tables(bk, oracle):
    B, T, K = 5, 50, 20
    cfg = BM.config((1, 20), 64)
    hist = ref_books(oracle, B, 16, T, groups=C2).history()
    env = run_env(bk, TABLE, B, 16, cfg)
    env.enable_series()
    env.enable_lags(K)
    env.run_series(T, chunk=16)
    assert env.steps_done() == T
    env.sync()
    P.no_flags(env)
    got = env.bins()
    want = model(hist, cfg, ("run_series", T))
    assert (want[:, 1].sum(axis=1) > 0).all()
    same_bins(got, want, "run_series(50, chunk=16) on a ring of 16")
    P.same_history(env.history(), hist[T - 16:])
    ser, lag = env.series(), env.lags()
    assert (ser["n_steps"] == T).all()
    P.same_array(got[:, 3].sum(axis=1), ser["n_steps"], "run_series", "the volume channel's total")
    P.same_array(got[:, 2].sum(axis=1), ser["n_two_sided"], "run_series", "the spread channel's total")
    P.same_array(got[:, 1].sum(axis=1), lag[:, K - 1]["n_h"], "run_series", "span 20 against the lag table")
    env.close()
    # the bin table alone: run_series folds it and nothing else
    alone = run_env(bk, TABLE, B, 16, cfg)
    alone.run_series(T, chunk=16)
    same_bins(alone.bins(), want, "run_series with the bin table alone")
    refused(bk, alone.fold_series, "no series moments")
    alone.close()


# ------------------------------------------------------------------------------------------------ 8. refusals


# ------------------------------------------------------------------------------------------------ 9. the shared scenarios
# (written once in tests/hist_tables.py for the three tables; the rest of what they share is tests/test_gpu_hist_tables.py)
@pytest.mark.parametrize("pipeline", [None] + list(PIPELINES))
def test_run_folded_in_three_parts_equals_the_model_and_one_pass(bk, oracle, pipeline):
    run_folded_in_three_parts(bk, oracle, TABLE, TABLE.deepest, pipeline)


@pytest.mark.parametrize("kind", ["host", "device"])
def test_reset_books_cuts_the_carry_of_the_books_it_resets(bk, oracle, kind):
    reset_books_cuts_the_carry(bk, oracle, TABLE, kind)


@pytest.mark.parametrize("kind", ["host", "device"])
def test_a_masked_clear_folds_first_and_the_view_is_the_table_in_place(bk, oracle, kind):
    masked_clear_folds_first(bk, oracle, TABLE, kind)
