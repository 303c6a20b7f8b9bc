"""The per-book lag table of the level-2 history (bk_lags_enable; bourse_amd/csrc/lags.hpp): K rows of ten integer words
per book, one per lag, folded on the device from the history ring, and the carry that makes every split of a fold equal.

The expected side never shares code with the kernel: tests/lags_model.py::fold (plain Python ints) over the ORACLE's
history() of the same run - oracle.ManyBooks / ManyMarkets for bk_run, one oracle.StepEnv per book for the host-driven and
the device-ingress flows - and the device's own history is held against the oracle's through tests/oracle_parity.py where
the ring still retains it; case 1's rows are literal numbers worked out by hand.  Where a case says something only under a
condition - one-sided steps, pairs at the deepest lag, products of both signs, a word that wraps - the condition is asserted
on the expected side before anything is compared.  All comparisons are exact."""
import numpy as np
import pytest

import lags_model as LM
import oracle_parity as P
import series_model as SM
from ingress_support import ingress_env
from test_gpu_reset_books import C2, MEMBERS, PIPELINES, STEP, make_env, ref_books

pytestmark = pytest.mark.gpu
M64 = (1 << 64) - 1
M128 = (1 << 128) - 1
MAXU = 0xFFFFFFFF
SEED = 101
# a lag row's words and the series row's over the same steps and cuts
SERIES_WORDS = (("n_pairs", "n_pairs"), ("sum_dd", "sum_dd"), ("sum_abs_dd", "sum_abs_dd"), ("n_h", "n_ret"), ("sum_h", "sum_d"),
                ("sum_abs_h", "sum_abs_d"), ("sum_h2", "sum_d2"), ("sum_h4_lo", "sum_d4_lo"), ("sum_h4_hi", "sum_d4_hi"),
                ("max_abs_h", "max_abs_d"))


@pytest.fixture(scope="module")
def bk():
    import bourse_amd

    return bourse_amd


def same_rows(got, want, tag):
    assert got.dtype == want.dtype == LM.LAG_DTYPE, (got.dtype, want.dtype)
    assert got.shape == want.shape, f"{tag}: rows {got.shape} vs {want.shape}"
    for f in LM.FIELDS:
        P.same_array(got[f], want[f], tag, f"lag word {f}")


def same_as_series(lag_rows, series_rows, tag):
    for a, b in SERIES_WORDS:
        P.same_array(lag_rows[:, 0][a], series_rows[b].astype(lag_rows[a].dtype), tag, f"row 0's {a} against the series' {b}")


def zeros(B, K):
    return np.zeros((B, K), dtype=LM.LAG_DTYPE)


_want = {}


def model(hist, K, key, **kw):
    """LM.rows over the oracle's history, computed once per (run, K, range) and shared"""
    if key not in _want:
        _want[key] = LM.rows(hist, K, **kw)
    return _want[key].copy()


def lost(bk, call, n):
    with pytest.raises(bk.BourseError, match=rf"\b{n} step\(s\) of the lag table were lost") as e:
        call()
    assert e.value.code == 5


def refused(bk, call, match):
    with pytest.raises(bk.BourseError, match=match) as e:
        call()
    assert e.value.code == 5


def run_env(bk, B, cap, K, groups=C2, members=None, **kw):
    """an env of test_gpu_reset_books' shape (levels 16, pool 64) with the table on"""
    env = make_env(bk, B, groups=None if members else groups, members=members, steps=cap, **kw)
    env.enable_lags(K)
    return env


def host_driven(bk, oracle, B, cap, K, steps, tick=1, step_size=STEP, max_orders=32):
    """B books driven by place / cancel calls, the same for every book unless an op names its book, beside one oracle env
    per book; returns (env, refs) with nothing folded"""
    env = bk.ManyBookEnv(B, SEED, 0, tick, step_size, levels=5, max_live_orders=16, max_orders=max_orders, trade_capacity=16,
                         history_capacity=cap)
    refs = [oracle.StepEnv(SEED + b, 0, tick, step_size, True, 5) for b in range(B)]
    env.enable_lags(K)
    for ops in steps:
        for f, books, args in ops:
            for b in books:
                got, want = getattr(env, f)(b, *args), getattr(refs[b], f)(*args)
                assert f != "place_order" or got == want
        env.step()
        for r in refs:
            r.step()
    return env, refs


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
    env, refs = host_driven(bk, oracle, 2, 8, K, steps, max_orders=16)
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


# ------------------------------------------------------------------------------------------------ 2. bk_run
@pytest.mark.parametrize("K,pipeline", [(64, None)] + [(64, p) for p in PIPELINES] + [(1, None), (5, None)])
def test_run_folded_in_three_parts_equals_the_model_and_one_pass(bk, oracle, K, pipeline):
    """5 books (the last block of four waves holds one), a ring of 96: run(70) and fold - two chunks of the window - run(26)
    and fold - the ring at its last slots - run(40) and fold - the ring wrapped.  A twin with a ring of 136 folds once, in
    three chunks.  With the series on the same env, row 0 is the series row.  The same under every pipeline."""
    B, cap, parts = 5, 96, (70, 26, 40)
    T = sum(parts)
    hist = ref_books(oracle, B, 16, T, groups=C2).history()
    deep = model(hist, 64, ("run", 64, T))
    two = (hist[:, :, 1] != 0) & (hist[:, :, 2] != MAXU)
    assert ((~two).sum(axis=0) >= 1).all(), "every book has a one-sided step"
    assert (deep[:, 63]["n_pairs"] > 0).all(), deep[:, 63]["n_pairs"]
    m = hist[:, :, 1].astype(np.int64) + hist[:, :, 2].astype(np.int64)
    d = np.diff(m, axis=0)
    r = two[1:] & two[:-1]
    for k in (1, 64):
        assert ((d[k:] * d[:-k])[r[k:] & r[:-k]] < 0).any(), f"a negative product at lag {k}"
    env = run_env(bk, B, cap, K)
    env.enable_series()
    twin = run_env(bk, B, T, K)
    if pipeline:
        env.set_pipeline(pipeline)
        twin.set_pipeline(pipeline)
    done = 0
    for n in parts:
        env.run(n, sync=False)
        twin.run(n, sync=False)
        env.fold_lags()
        env.fold_series()  # (a cursor of its own: the series must not fall out of the ring either)
        done += n
        same_rows(env.lags(), model(hist[:done], K, ("run", K, done)), f"after {done} steps ({pipeline}, K = {K})")
    twin.fold_lags()
    final = model(hist, K, ("run", K, T))
    if K == 64:
        same_rows(final, deep, "the model is the model")
    same_rows(twin.lags(), final, "one fold of 136 steps")
    same_rows(env.lags(), final, "three folds against one pass of the model")
    same_as_series(env.lags(), env.series(), "three folds")
    same_as_series(final, SM.rows(hist), "the models")
    for e in (env, twin):
        P.no_flags(e)
    P.same_history(env.history(), hist[done - cap:])
    P.same_history(twin.history(), hist)
    env.close()
    twin.close()


# ------------------------------------------------------------------------------------------------ 3. single steps
@pytest.mark.parametrize("K", [64, 5])
def test_single_step_folds_with_a_carry_deeper_than_the_ring(bk, oracle, K):
    """A ring of 8 and 24 folds of one step each: from step 8 on every word the fold reads beyond its own step comes from
    the carry, which at K = 64 reaches 65 steps back - eight times the ring."""
    B, T = 3, 24
    hist = ref_books(oracle, B, 16, T, groups=C2).history()
    env = run_env(bk, B, 8, K)
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


# ------------------------------------------------------------------------------------------------ 4. the other flows
def test_noise_and_momentum_members_folded_in_chunks_of_seven(bk, oracle):
    B, T, K = 3, 40, 16
    hist = ref_books(oracle, B, 16, T, members=MEMBERS).history()
    env = run_env(bk, B, T, K, members=MEMBERS)
    for lo in range(0, T, 7):
        env.run(min(7, T - lo), sync=False)
        env.fold_lags()
    P.no_flags(env)
    want = LM.rows(hist, K)
    assert (want[:, K - 1]["n_h"] > 0).all() and (want[:, 0]["n_pairs"] > 0).all()
    same_rows(env.lags(), want, "Noise + Momentum")
    P.same_history(env.history(), hist)
    env.close()


def test_markets_keep_rows_per_book(bk, oracle):
    NM, ticks, T, K = 3, [2, 2], 30, 8
    groups = [(0, 24, (40, 56), (10, 20), 2, 0.8), (1, 24, (40, 56), (10, 20), 2, 0.6), (1, 8, (40, 56), (50, 70), 2, 0.3)]
    env = bk.ManyMarketEnv(NM, SEED, 0, ticks, STEP, True, levels=10, max_live_orders=64, trade_capacity=4096, history_capacity=T)
    env.set_random_market_agents(groups)
    env.enable_lags(K)
    ref = oracle.ManyMarkets(NM, SEED, 0, ticks, STEP, True, 10, groups)
    ref.run(T)
    hist = ref.history()
    for n in (11, 19):
        env.run(n, sync=False)
        env.fold_lags()
    P.no_flags(env)
    want = LM.rows(hist, K)
    assert want.shape == (6, K) and (want[:, 0]["n_h"] > 0).all() and len({tuple(r.tolist()) for r in want[:, 0]}) == 6
    same_rows(env.lags(), want, "markets, rows per book")
    P.same_history(env.history(), hist)
    env.close()


def test_ingress_folded_after_every_step_equals_one_fold_at_the_end(bk, oracle):
    """fold_lags() behind EVERY step takes the carry path every time; a twin env folds once at the end."""
    import torch

    from test_gpu_accounts import Books, busy_flow

    B, T, tick, K = 4, 9, 2, 6
    flows = [busy_flow(np.random.default_rng(20 + s), B, tick, idle=(1,) if s in (3, 4) else (), n_lo=30, n_hi=40) for s in range(T)]
    env = ingress_env(bk, torch, B, T, 256, 0, 64, tick=tick, n_ext=40)
    twin = ingress_env(bk, torch, B, T, 256, 0, 64, tick=tick, n_ext=40)
    env.enable_lags(K)
    twin.enable_lags(K)
    books, other = Books(oracle, B, tick, env, torch), Books(oracle, B, tick, twin, torch)
    for s, f in enumerate(flows):
        for t in (books, other):
            t.submit(*f)
            t.step()
        env.fold_lags()
        if s == 4:
            mid = env.lags()
    twin.fold_lags()
    hist = np.stack([r.history() for r in books.refs], axis=1)
    want = LM.rows(hist, K)
    assert (want[:, 0]["n_pairs"] > 0).all() and (want[:, K - 1]["n_h"] > 0).all()
    same_rows(mid, LM.rows(hist[:5], K), "after step 4")
    same_rows(env.lags(), want, "folded after every step")
    same_rows(twin.lags(), want, "folded once")
    for e in (env, twin):
        P.no_flags(e)
        P.same_history(e.history(), hist)
    env.close()
    twin.close()


# ------------------------------------------------------------------------------------------------ 5. lost steps
def test_lost_steps_refuse_the_fold_and_a_full_clear_recovers(bk, oracle):
    B, K = 3, 4
    hist = ref_books(oracle, B, 16, 16, groups=C2).history()
    env = run_env(bk, B, 8, K)
    env.run(3)
    env.fold_lags()
    before = env.lags()
    same_rows(before, LM.rows(hist[:3], K), "three steps")
    env.run(9)  # steps 3 .. 11 into a ring of 8: step 3 is gone
    lost(bk, env.fold_lags, 1)
    same_rows(env.lags(), before, "a refused fold leaves the rows")
    lost(bk, env.fold_lags, 1)  # ... and the cursor
    lost(bk, lambda: env.clear_lags(np.array([1, 0, 0], dtype=bool)), 1)
    same_rows(env.lags(), before, "a refused clear leaves the rows")
    env.clear_lags()
    same_rows(env.lags(), zeros(B, K), "clear_lags() clears every row")
    env.run(2)
    env.fold_lags()
    want = LM.rows(hist[12:14], K, first_step=12)  # (the carry was cleared too: step 12 has no past)
    assert (want[:, 0]["n_h"] <= 1).all() and not want[:, 1:]["n_h"].any()
    same_rows(env.lags(), want, "counted from the clear on")
    # the same through clear_history(): the two steps run since the last fold are no longer retained
    env.run(2)
    env.clear_history()
    lost(bk, env.fold_lags, 2)
    env.clear_lags()
    env.close()


# ------------------------------------------------------------------------------------------------ 6. resets, clears
@pytest.mark.parametrize("kind", ["host", "device"])
def test_reset_books_cuts_the_carry_of_the_books_it_resets(bk, oracle, kind):
    """6 steps, save, fold; 5 steps NOT folded; reset books 0, 2, 4 - which folds the five first - then 7 steps.  A reset
    book replays steps 6 .. 12 of the same seed: its table is the oracle's steps 0 .. 10, a cut, steps 6 .. 12.  The sums
    go on; no span or pair reaches over the reset."""
    B, n, m, k, K = 5, 6, 5, 7, 4
    hist = ref_books(oracle, B, 16, n + m + k, groups=C2).history()
    env = run_env(bk, B, n + m + k, K, kind=kind)
    env.run(n)
    env.save_snapshot()
    env.fold_lags()
    env.run(m)
    mask = np.array([1, 0, 1, 0, 1], dtype=bool)
    if kind == "device":
        import torch

        env.reset_books(torch.tensor(mask, device="cuda"), sync=False)
    else:
        env.reset_books(mask)
    same_rows(env.lags(), LM.rows(hist[:n + m], K), "the reset folded the five steps (a cut leaves the rows)")
    env.run(k)
    env.fold_lags()
    want, uncut = [], []
    for b in range(B):
        if mask[b]:
            s = LM.fold(hist[n:n + k, b], cuts=[n + m], first_step=n + m, into=LM.fold(hist[:n + m, b], K))
            uncut.append(LM.table(LM.fold(hist[n:n + k, b], first_step=n + m, into=LM.fold(hist[:n + m, b], K))))
        else:
            s = LM.fold(hist[:, b], K)
        want.append(LM.table(s))
    want = np.array(want, dtype=LM.LAG_DTYPE)
    assert any((u != w).any() for u, w in zip(uncut, want[mask])), "the cut shows in the masked books' rows"
    assert (want[mask][:, 0]["n_h"] > 0).all()
    same_rows(env.lags(), want, f"reset_books ({kind})")
    P.no_flags(env)
    env.close()


def test_reset_ingress_books_cuts_the_carry_too(bk, oracle):
    """3 steps, save, 3 steps, reset books 0 and 2 (a torch CUDA mask; the three steps are folded by the reset), 2 steps.
    A reset book's quotes after the reset are those of a REPLAY (tests/test_gpu_series.py)."""
    import torch

    from test_gpu_accounts import Books, busy_flow

    B, tick, K = 4, 2, 3
    env = ingress_env(bk, torch, B, 8, 256, 0, 64, tick=tick, n_ext=40)
    env.enable_lags(K)
    books = Books(oracle, B, tick, env, torch)
    flows = [busy_flow(np.random.default_rng(60 + s), B, tick, n_lo=30, n_hi=40) for s in range(8)]

    def run(lo, hi, bs=books):
        for f in flows[lo:hi]:
            bs.submit(*f)
            bs.step()

    run(0, 3)
    env.save_ingress_snapshot()
    env.fold_lags()
    run(3, 6)
    mask = np.array([1, 0, 1, 0], dtype=bool)
    env.reset_ingress_books(torch.tensor(mask, device="cuda"), sync=False)
    run(6, 8)
    env.fold_lags()
    replay = Books(oracle, B, tick)
    run(0, 3, replay)
    run(6, 8, replay)
    want = []
    for b in range(B):
        h = books.refs[b].history()
        if mask[b]:
            s = LM.fold(replay.refs[b].history()[3:5], cuts=[6], first_step=6, into=LM.fold(h[:6], K))
        else:
            s = LM.fold(h, K)
        want.append(LM.table(s))
    want = np.array(want, dtype=LM.LAG_DTYPE)
    assert (want[:, 0]["n_h"] > 3).all()
    same_rows(env.lags(), want, "reset_ingress_books")
    P.no_flags(env)
    env.close()


@pytest.mark.parametrize("kind", ["host", "device"])
def test_reset_markets_cuts_the_carry_of_every_book_of_a_masked_market(bk, oracle, kind):
    """3 markets x 2 assets: the mask has one byte per MARKET and the cut must reach both books of markets 0 and 2 and
    neither book of market 1.  6 steps, save, 5 steps not folded, reset, 7 steps: as the books' case above."""
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
    env = run_env(bk, B, 8, K)
    env.enable_series()
    env.run(2)
    env.save_snapshot()
    env.run(5)
    env.fold_series()
    series_at_7 = env.series()
    env.run(4)
    lost(bk, lambda: env.reset_books(np.array([1, 0, 0], dtype=bool)), 3)
    assert env.steps_done() == 11
    got = env.series()
    assert all((got[f] == series_at_7[f]).all() for f in SM.FIELDS) and (got["n_steps"] == 7).all()
    same_rows(env.lags(), zeros(B, K), "the lag table is untouched")
    env.clear_lags()
    env.reset_books(np.array([1, 0, 0], dtype=bool))
    assert (env.series()["n_steps"] == 11).all()  # (now the reset went through: the series folded its four steps)
    env.close()


@pytest.mark.parametrize("kind", ["host", "device"])
def test_a_masked_clear_folds_first_and_the_view_is_the_table_in_place(bk, oracle, kind):
    import torch

    B, K = 5, 4
    hist = ref_books(oracle, B, 16, 16, groups=C2).history()
    env = run_env(bk, B, 16, K, kind="device")
    view = torch.as_tensor(env.lags_view(), device="cuda")
    assert tuple(view.shape) == (B, K, 10) and view.dtype == torch.int64 and view.data_ptr() == env.lags_device_ptr()
    env.run(10, sync=False)  # (not folded: the masked clear folds the ten steps first)
    mask = np.array([1, 0, 1, 0, 0], dtype=bool)
    if kind == "host":
        env.clear_lags(mask)
    else:
        env.clear_lags(torch.tensor(mask, device="cuda"), sync=False)
    now = env.lags()
    same_rows(now[mask], zeros(2, K), "the masked rows are cleared")
    same_rows(now[~mask], LM.rows(hist[:10], K)[~mask], "the others hold the ten steps")
    env.run(6, sync=False)
    env.fold_lags(sync=True)
    want = LM.rows(hist, K)
    want[mask] = LM.rows(hist[10:], K, first_step=10)[mask]  # (their carry was cleared too: step 10 has no past)
    same_rows(env.lags(), want, f"after clear_lags ({kind})")
    # the tensor made before any step sees the latest fold without a new call
    seen = np.ascontiguousarray(view.cpu().numpy()).view(LM.LAG_DTYPE).reshape(B, K)
    same_rows(seen, want, "lags_view() as a zero-copy tensor")
    P.no_flags(env)
    env.close()


def test_restore_clears_rows_and_carry_and_rebases_the_cursor(bk, oracle):
    B, K = 3, 4
    hist = ref_books(oracle, B, 16, 16, groups=C2).history()
    env = run_env(bk, B, 16, K)
    env.run(6)
    env.fold_lags()
    ck = env.checkpoint()
    env.run(4)  # (outstanding when the checkpoint comes back: forgotten, not folded)
    env.restore(ck)
    assert env.steps_done() == 6
    same_rows(env.lags(), zeros(B, K), "restore clears every row")
    env.run(5)
    env.fold_lags()
    same_rows(env.lags(), LM.rows(hist[6:11], K, first_step=6), "counted from the restored step on, with no past")
    P.no_flags(env)
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
    env, refs = host_driven(bk, oracle, B, 8, K, steps, step_size=1000)
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
    env = run_env(bk, B, 16, K)
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
def test_refusals_leave_the_env_working(bk, oracle):
    K = 2
    env = make_env(bk, 2, groups=C2, steps=8)
    for call in (env.fold_lags, env.lags, env.lags_device_ptr, env.lags_view, env.clear_lags,
                 lambda: env.clear_lags(np.ones(2, dtype=bool))):
        refused(bk, call, "no lag table: call .*bk_lags_enable.* first")
    env.run(2)
    for n in (0, 65, 1 << 20):
        refused(bk, lambda: env.enable_lags(n), r"n_lags must be in 1\.\.64")
    refused(bk, env.fold_lags, "no lag table")  # (a refused enable left the env without the table)
    env.enable_lags(K)
    refused(bk, lambda: env.enable_lags(K), "already enabled")
    refused(bk, lambda: env.enable_lags(3), "already enabled")
    assert env.lags().shape == (2, K)
    # a null out-pointer and a book range past the end: refused, the table as it was
    for rc in (env._L.bk_lags_device_ptr(env._h, None), env._L.bk_get_lags(env._h, 0, 2, None)):
        assert rc == 5 and b"null argument" in env._L.bk_last_error()
    for first, n in ((1, 2), (3, 0), (0, 3)):
        refused(bk, lambda: env.lags(first, n), "book range out of bounds")
    assert env.lags(2, 0).shape == (0, K) and env.lags(1).shape == (1, K)
    with pytest.raises(ValueError):
        env.lags(-1, 1)
    same_rows(env.lags(), zeros(2, K), "refusals leave the rows")
    with pytest.raises(ValueError):
        env.clear_lags(np.ones(3, dtype=bool))
    with pytest.raises(ValueError):
        env.run_series(4, chunk=9)
    env.run(3)
    env.fold_lags()
    hist = ref_books(oracle, 2, 16, 16, groups=C2).history()
    same_rows(env.lags(), LM.rows(hist[2:5], K, first_step=2), "steps before enable_lags() are not counted")
    env.close()
    none = make_env(bk, 2, groups=C2, steps=0)
    refused(bk, lambda: none.enable_lags(K), "history_capacity must be > 0")
    none.run(2)
    none.close()
    # a host-driven env: a book cannot be loaded into an env with the table
    host = bk.ManyBookEnv(2, SEED, 0, 1, STEP, levels=5, max_live_orders=16, max_orders=16, trade_capacity=16, history_capacity=4)
    host.place_order(0, True, 5, 1, 100)
    host.step()
    state = host.book_state(0)
    host.load_book_state(1, state)
    host.enable_lags(K)
    refused(bk, lambda: host.load_book_state(1, state), "lag table")
    host.step()
    host.fold_lags(sync=True)
    same_rows(host.lags(), zeros(2, K), "one-sided books add nothing")
    host.close()
