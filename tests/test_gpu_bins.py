"""The per-book bin table of the level-2 history (bk_bins_enable; bourse_amd/csrc/bins.hpp): per book S + 2 rows of B u64
counts - the change of twice the mid over S spans, the spread, the traded volume - folded on the device from the history
ring, and the carry that makes every split of a fold equal.

The expected side never shares code with the kernel: tests/bins_model.py::fold (plain Python ints) over the ORACLE's
history() of the same run - oracle.ManyBooks / ManyMarkets for bk_run, one oracle.StepEnv per book for the host-driven and
the device-ingress flows - and the device's own history is held against the oracle's through tests/oracle_parity.py where
the ring still retains it; case 1's counts are literal numbers worked out by hand.  Where a case says something only under a
condition - one-sided steps, counts at the deepest span, clamped values, traded steps - the condition is asserted on the
expected side before anything is compared.  All comparisons are exact."""
import numpy as np
import pytest

import bins_model as BM
import lags_model as LM
import oracle_parity as P
import series_model as SM
from ingress_support import ingress_env
from test_gpu_reset_books import C2, MEMBERS, PIPELINES, STEP, make_env, ref_books

pytestmark = pytest.mark.gpu
MAXU = 0xFFFFFFFF
SEED = 101
CFG = BM.config((1, 5, 64), 64)


@pytest.fixture(scope="module")
def bk():
    import bourse_amd

    return bourse_amd


def same_bins(got, want, tag):
    assert got.dtype == want.dtype == np.uint64, (got.dtype, want.dtype)
    assert got.shape == want.shape, f"{tag}: table {got.shape} vs {want.shape}"
    for c in range(want.shape[1]):
        P.same_array(got[:, c], want[:, c], tag, f"bin counts of channel {c}")


def zeros(B, cfg):
    return np.zeros((B, len(cfg["spans"]) + 2, cfg["n_bins"]), dtype=np.uint64)


_want = {}


def model(hist, cfg, key, **kw):
    """BM.rows over the oracle's history, computed once per (run, configuration, range) and shared"""
    key = key + (repr(cfg),)
    if key not in _want:
        _want[key] = BM.rows(hist, cfg, **kw)
    return _want[key].copy()


def lost(bk, call, n):
    with pytest.raises(bk.BourseError, match=rf"\b{n} step\(s\) of the bin table were lost") as e:
        call()
    assert e.value.code == 5


def refused(bk, call, match):
    with pytest.raises(bk.BourseError, match=match) as e:
        call()
    assert e.value.code == 5


def enable(env, cfg):
    env.enable_bins(cfg["spans"], cfg["n_bins"], cfg["ret_width"], cfg["spread_width"], cfg["vol_width"])
    return env


def run_env(bk, B, cap, cfg, groups=C2, members=None, **kw):
    """an env of test_gpu_reset_books' shape (levels 16, pool 64) with the table on"""
    return enable(make_env(bk, B, groups=None if members else groups, members=members, steps=cap, **kw), cfg)


def host_driven(bk, oracle, B, cap, cfgs, steps, tick=1, step_size=STEP, max_orders=32):
    """B books driven by place / cancel calls, the same for every book unless an op names its book, beside one oracle env
    per book - one device env per configuration of ``cfgs``; returns (envs, refs) with nothing folded"""
    envs = [enable(bk.ManyBookEnv(B, SEED, 0, tick, step_size, levels=5, max_live_orders=16, max_orders=max_orders, trade_capacity=16,
                                  history_capacity=cap), c) for c in cfgs]
    refs = [oracle.StepEnv(SEED + b, 0, tick, step_size, True, 5) for b in range(B)]
    for ops in steps:
        for f, books, args in ops:
            for b in books:
                want = getattr(refs[b], f)(*args)
                for env in envs:
                    got = getattr(env, f)(b, *args)
                    assert f != "place_order" or got == want
        for env in envs:
            env.step()
        for r in refs:
            r.step()
    return envs, refs


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
    (env,), refs = host_driven(bk, oracle, 2, 8, [cfg], steps, max_orders=16)
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
@pytest.mark.parametrize("pipeline", [None] + list(PIPELINES))
def test_run_folded_in_three_parts_equals_the_model_and_one_pass(bk, oracle, pipeline):
    """5 books (the last block of four waves holds one), a ring of 96: run(70) and fold - lanes with two steps each -
    run(26) and fold - the ring at its last slots - run(40) and fold - the ring wrapped.  A twin with a ring of 136 folds
    once, three steps a lane.  With the lag table at K = 64 and the series on the same env, the channels' totals are their
    counts.  The same under every pipeline."""
    B, cap, parts = 5, 96, (70, 26, 40)
    T = sum(parts)
    hist = ref_books(oracle, B, 16, T, groups=C2).history()
    final = model(hist, CFG, ("run", T))
    two = (hist[:, :, 1] != 0) & (hist[:, :, 2] != MAXU)
    assert ((~two).sum(axis=0) >= 1).all(), "every book has a one-sided step"
    assert (final[:, 2].sum(axis=1) > 0).all() and (final[:, 4, 1:].sum(axis=1) > 0).all(), "span 64 counts, steps trade"
    env = run_env(bk, B, cap, CFG)
    env.enable_series()
    env.enable_lags(64)
    twin = run_env(bk, B, T, CFG)
    if pipeline:
        env.set_pipeline(pipeline)
        twin.set_pipeline(pipeline)
    done = 0
    for n in parts:
        env.run(n, sync=False)
        twin.run(n, sync=False)
        env.fold_bins()
        env.fold_series()  # (cursors of their own: the siblings must not fall out of the ring either)
        env.fold_lags()
        done += n
        same_bins(env.bins(), model(hist[:done], CFG, ("run", done)), f"after {done} steps ({pipeline})")
    twin.fold_bins()
    same_bins(twin.bins(), final, "one fold of 136 steps")
    same_bins(env.bins(), final, "three folds against one pass of the model")
    # the identities: the totals are the lag table's n_h at each span, the series' n_two_sided and n_steps
    got, lag, ser = env.bins(), env.lags(), env.series()
    for j, k in enumerate(CFG["spans"]):
        P.same_array(got[:, j].sum(axis=1), lag[:, k - 1]["n_h"], "totals", f"channel {j} against the lag table's n_h at span {k}")
        for b in range(B):
            if not got[b, j, 0] and not got[b, j, -1]:  # nothing clamped at ret_width 1: the first moment is sum_h
                first = sum((i - 32) * int(c) for i, c in enumerate(got[b, j]))
                assert first == int(lag[b, k - 1]["sum_h"]), (b, k)
    P.same_array(got[:, 3].sum(axis=1), ser["n_two_sided"], "totals", "the spread channel against the series' n_two_sided")
    P.same_array(got[:, 4].sum(axis=1), ser["n_steps"], "totals", "the volume channel against the series' n_steps")
    assert (ser["n_steps"] == T).all()
    for e in (env, twin):
        P.no_flags(e)
    P.same_history(env.history(), hist[done - cap:])
    P.same_history(twin.history(), hist)
    env.close()
    twin.close()


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
    env = run_env(bk, B, cap, cfg)
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
    env = run_env(bk, B, 8, cfg)
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


# ------------------------------------------------------------------------------------------------ 4. the other flows
def test_noise_and_momentum_members_folded_in_chunks_of_seven(bk, oracle):
    B, T = 3, 40
    cfg = BM.config((1, 16), 64, 2, 2, 50)
    hist = ref_books(oracle, B, 16, T, members=MEMBERS).history()
    env = run_env(bk, B, T, cfg, members=MEMBERS)
    for lo in range(0, T, 7):
        env.run(min(7, T - lo), sync=False)
        env.fold_bins()
    P.no_flags(env)
    want = BM.rows(hist, cfg)
    assert (want[:, 1].sum(axis=1) > 0).all() and (want[:, 3, 1:].sum(axis=1) > 0).all()
    same_bins(env.bins(), want, "Noise + Momentum")
    P.same_history(env.history(), hist)
    env.close()


def test_markets_keep_counts_per_book(bk, oracle):
    NM, ticks, T = 3, [2, 2], 30
    cfg = BM.config((1, 8), 32, 2, 2, 10)
    groups = [(0, 24, (40, 56), (10, 20), 2, 0.8), (1, 24, (40, 56), (10, 20), 2, 0.6), (1, 8, (40, 56), (50, 70), 2, 0.3)]
    env = bk.ManyMarketEnv(NM, SEED, 0, ticks, STEP, True, levels=10, max_live_orders=64, trade_capacity=4096, history_capacity=T)
    env.set_random_market_agents(groups)
    enable(env, cfg)
    ref = oracle.ManyMarkets(NM, SEED, 0, ticks, STEP, True, 10, groups)
    ref.run(T)
    hist = ref.history()
    for n in (11, 19):
        env.run(n, sync=False)
        env.fold_bins()
    P.no_flags(env)
    want = BM.rows(hist, cfg)
    assert want.shape == (6, 4, 32) and (want[:, 0].sum(axis=1) > 0).all() and len({w.tobytes() for w in want}) == 6
    same_bins(env.bins(), want, "markets, counts per book")
    P.same_history(env.history(), hist)
    env.close()


def test_ingress_folded_after_every_step_equals_one_fold_at_the_end(bk, oracle):
    """fold_bins() behind EVERY step takes the carry path every time; a twin env folds once at the end."""
    import torch

    from test_gpu_accounts import Books, busy_flow

    B, T, tick = 4, 9, 2
    cfg = BM.config((1, 6, 2), 32, 2, 2, 5)
    flows = [busy_flow(np.random.default_rng(20 + s), B, tick, idle=(1,) if s in (3, 4) else (), n_lo=30, n_hi=40) for s in range(T)]
    env = ingress_env(bk, torch, B, T, 256, 0, 64, tick=tick, n_ext=40)
    twin = ingress_env(bk, torch, B, T, 256, 0, 64, tick=tick, n_ext=40)
    enable(env, cfg)
    enable(twin, cfg)
    books, other = Books(oracle, B, tick, env, torch), Books(oracle, B, tick, twin, torch)
    for s, f in enumerate(flows):
        for t in (books, other):
            t.submit(*f)
            t.step()
        env.fold_bins()
        if s == 4:
            mid = env.bins()
    twin.fold_bins()
    hist = np.stack([r.history() for r in books.refs], axis=1)
    want = BM.rows(hist, cfg)
    assert (want[:, 1].sum(axis=1) > 0).all() and (want[:, 4, 1:].sum(axis=1) > 0).all()
    same_bins(mid, BM.rows(hist[:5], cfg), "after step 4")
    same_bins(env.bins(), want, "folded after every step")
    same_bins(twin.bins(), want, "folded once")
    for e in (env, twin):
        P.no_flags(e)
        P.same_history(e.history(), hist)
    env.close()
    twin.close()


# ------------------------------------------------------------------------------------------------ 5. lost steps
def test_lost_steps_refuse_the_fold_and_a_full_clear_recovers(bk, oracle):
    B = 3
    cfg = BM.config((1, 4), 64)
    hist = ref_books(oracle, B, 16, 16, groups=C2).history()
    env = run_env(bk, B, 8, cfg)
    env.run(3)
    env.fold_bins()
    before = env.bins()
    same_bins(before, BM.rows(hist[:3], cfg), "three steps")
    env.run(9)  # steps 3 .. 11 into a ring of 8: step 3 is gone
    lost(bk, env.fold_bins, 1)
    same_bins(env.bins(), before, "a refused fold leaves the table")
    lost(bk, env.fold_bins, 1)  # ... and the cursor
    lost(bk, lambda: env.clear_bins(np.array([1, 0, 0], dtype=bool)), 1)
    same_bins(env.bins(), before, "a refused clear leaves the table")
    env.clear_bins()
    same_bins(env.bins(), zeros(B, cfg), "clear_bins() clears every count")
    env.run(2)
    env.fold_bins()
    want = BM.rows(hist[12:14], cfg, first_step=12)  # (the carry was cleared too: step 12 has no past)
    assert (want[:, 0].sum(axis=1) <= 1).all() and not want[:, 1].any() and (want[:, 3].sum(axis=1) == 2).all()
    same_bins(env.bins(), want, "counted from the clear on")
    # the same through clear_history(): the two steps run since the last fold are no longer retained
    env.run(2)
    env.clear_history()
    lost(bk, env.fold_bins, 2)
    same_bins(env.bins(), want, "a refused fold leaves the table (clear_history)")
    env.clear_bins()
    env.close()


# ------------------------------------------------------------------------------------------------ 6. resets, clears
@pytest.mark.parametrize("kind", ["host", "device"])
def test_reset_books_cuts_the_carry_of_the_books_it_resets(bk, oracle, kind):
    """6 steps, save, fold; 5 steps NOT folded; reset books 0, 2, 4 - which folds the five first - then 7 steps.  A reset
    book replays steps 6 .. 12 of the same seed: its table is the oracle's steps 0 .. 10, a cut, steps 6 .. 12.  The counts
    go on; no span reaches over the reset."""
    B, n, m, k = 5, 6, 5, 7
    cfg = BM.config((1, 4), 64)
    hist = ref_books(oracle, B, 16, n + m + k, groups=C2).history()
    env = run_env(bk, B, n + m + k, cfg, kind=kind)
    env.run(n)
    env.save_snapshot()
    env.fold_bins()
    env.run(m)
    mask = np.array([1, 0, 1, 0, 1], dtype=bool)
    if kind == "device":
        import torch

        env.reset_books(torch.tensor(mask, device="cuda"), sync=False)
    else:
        env.reset_books(mask)
    same_bins(env.bins(), BM.rows(hist[:n + m], cfg), "the reset folded the five steps (a cut leaves the counts)")
    env.run(k)
    env.fold_bins()
    want, uncut = [], []
    for b in range(B):
        if mask[b]:
            s = BM.fold(hist[n:n + k, b], cuts=[n + m], first_step=n + m, into=BM.fold(hist[:n + m, b], cfg))
            uncut.append(BM.table(BM.fold(hist[n:n + k, b], first_step=n + m, into=BM.fold(hist[:n + m, b], cfg))))
        else:
            s = BM.fold(hist[:, b], cfg)
        want.append(BM.table(s))
    want = np.array(want, dtype=np.uint64)
    assert any((u != w).any() for u, w in zip(uncut, want[mask])), "the cut shows in the masked books' counts"
    assert (want[mask][:, 0].sum(axis=1) > 0).all()
    same_bins(env.bins(), want, f"reset_books ({kind})")
    P.no_flags(env)
    env.close()


def test_reset_ingress_books_cuts_the_carry_too(bk, oracle):
    """3 steps, save, 3 steps, reset books 0 and 2 (a torch CUDA mask; the three steps are folded by the reset), 2 steps.
    A reset book's quotes after the reset are those of a REPLAY (tests/test_gpu_series.py)."""
    import torch

    from test_gpu_accounts import Books, busy_flow

    B, tick = 4, 2
    cfg = BM.config((1, 3), 32, 2, 2, 5)
    env = ingress_env(bk, torch, B, 8, 256, 0, 64, tick=tick, n_ext=40)
    enable(env, cfg)
    books = Books(oracle, B, tick, env, torch)
    flows = [busy_flow(np.random.default_rng(60 + s), B, tick, n_lo=30, n_hi=40) for s in range(8)]

    def run(lo, hi, bs=books):
        for f in flows[lo:hi]:
            bs.submit(*f)
            bs.step()

    run(0, 3)
    env.save_ingress_snapshot()
    env.fold_bins()
    run(3, 6)
    mask = np.array([1, 0, 1, 0], dtype=bool)
    env.reset_ingress_books(torch.tensor(mask, device="cuda"), sync=False)
    run(6, 8)
    env.fold_bins()
    replay = Books(oracle, B, tick)
    run(0, 3, replay)
    run(6, 8, replay)
    want = []
    for b in range(B):
        h = books.refs[b].history()
        if mask[b]:
            s = BM.fold(replay.refs[b].history()[3:5], cuts=[6], first_step=6, into=BM.fold(h[:6], cfg))
        else:
            s = BM.fold(h, cfg)
        want.append(BM.table(s))
    want = np.array(want, dtype=np.uint64)
    assert (want[:, 0].sum(axis=1) > 3).all() and (want[:, 3].sum(axis=1) == 8).all()
    same_bins(env.bins(), want, "reset_ingress_books")
    P.no_flags(env)
    env.close()


@pytest.mark.parametrize("kind", ["host", "device"])
def test_reset_markets_cuts_the_carry_of_every_book_of_a_masked_market(bk, oracle, kind):
    """3 markets x 2 assets: the mask has one byte per MARKET and the cut must reach both books of markets 0 and 2 and
    neither book of market 1.  6 steps, save, 5 steps not folded, reset, 7 steps: as the books' case above."""
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
    its four outstanding steps.  Then the other way round: the bin table is up to date and the lag table has lost steps."""
    B = 3
    cfg = BM.config((1, 4), 64)
    env = run_env(bk, B, 8, cfg)
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
    lost(bk, lambda: env.reset_books(mask), 3)
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
    env.close()


@pytest.mark.parametrize("kind", ["host", "device"])
def test_a_masked_clear_folds_first_and_the_view_is_the_table_in_place(bk, oracle, kind):
    import torch

    B = 5
    cfg = BM.config((1, 4), 64)
    hist = ref_books(oracle, B, 16, 16, groups=C2).history()
    env = run_env(bk, B, 16, cfg, kind="device")
    view = torch.as_tensor(env.bins_view(), device="cuda")
    assert tuple(view.shape) == (B, 4, 64) and view.dtype == torch.int64 and view.data_ptr() == env.bins_device_ptr()
    env.run(10, sync=False)  # (not folded: the masked clear folds the ten steps first)
    mask = np.array([1, 0, 1, 0, 0], dtype=bool)
    if kind == "host":
        env.clear_bins(mask)
    else:
        env.clear_bins(torch.tensor(mask, device="cuda"), sync=False)
    now = env.bins()
    same_bins(now[mask], zeros(2, cfg), "the masked books are cleared")
    same_bins(now[~mask], BM.rows(hist[:10], cfg)[~mask], "the others hold the ten steps")
    env.run(6, sync=False)
    env.fold_bins(sync=True)
    want = BM.rows(hist, cfg)
    want[mask] = BM.rows(hist[10:], cfg, first_step=10)[mask]  # (their carry was cleared too: step 10 has no past)
    assert (want[mask][:, 1].sum(axis=1) < want[~mask][:, 1].sum(axis=1).min()).all()
    same_bins(env.bins(), want, f"after clear_bins ({kind})")
    # the tensor made before any step sees the latest fold without a new call
    seen = np.ascontiguousarray(view.cpu().numpy()).view(np.uint64).reshape(B, 4, 64)
    same_bins(seen, want, "bins_view() as a zero-copy tensor")
    P.no_flags(env)
    env.close()


def test_restore_clears_counts_and_carry_and_rebases_the_cursor(bk, oracle):
    B = 3
    cfg = BM.config((1, 4), 64)
    hist = ref_books(oracle, B, 16, 16, groups=C2).history()
    env = run_env(bk, B, 16, cfg)
    env.run(6)
    env.fold_bins()
    ck = env.checkpoint()
    env.run(4)  # (outstanding when the checkpoint comes back: forgotten, not folded)
    env.restore(ck)
    assert env.steps_done() == 6
    same_bins(env.bins(), zeros(B, cfg), "restore clears every count")
    env.run(5)
    env.fold_bins()
    same_bins(env.bins(), BM.rows(hist[6:11], cfg, first_step=6), "counted from the restored step on, with no past")
    P.no_flags(env)
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
    envs, refs = host_driven(bk, oracle, B, 8, cfgs, steps, step_size=1000)
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
    env = run_env(bk, B, 16, cfg)
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
    alone = run_env(bk, B, 16, cfg)
    alone.run_series(T, chunk=16)
    same_bins(alone.bins(), want, "run_series with the bin table alone")
    refused(bk, alone.fold_series, "no series moments")
    alone.close()


# ------------------------------------------------------------------------------------------------ 8. refusals
def test_refusals_leave_the_env_working(bk, oracle):
    cfg = BM.config((1, 2), 8)
    env = make_env(bk, 2, groups=C2, steps=8)
    for call in (env.fold_bins, env.bins, env.bins_config, env.bins_device_ptr, env.bins_view, env.clear_bins,
                 lambda: env.clear_bins(np.ones(2, dtype=bool))):
        refused(bk, call, "no bin table: call .*bk_bins_enable.* first")
    env.run(2)
    for kw, why in ((dict(n_bins=0), "n_bins must be even"), (dict(n_bins=7), "n_bins must be even"), (dict(n_bins=258), "n_bins must be even"),
                    (dict(n_bins=1 << 20), "n_bins must be even"), (dict(spans=()), r"n_spans must be in 1\.\.4"),
                    (dict(spans=(1, 2, 3, 4, 5)), r"n_spans must be in 1\.\.4"), (dict(spans=(0,)), r"span must be in 1\.\.64"),
                    (dict(spans=(1, 65)), r"span must be in 1\.\.64"), (dict(spans=(3, 1, 1 << 20)), r"span must be in 1\.\.64"),
                    (dict(ret_width=0), "must be >= 1"), (dict(spread_width=0), "must be >= 1"), (dict(vol_width=0), "must be >= 1")):
        refused(bk, lambda: env.enable_bins(**kw), why)
        refused(bk, env.fold_bins, "no bin table")  # (a refused enable left the env without the table)
    with pytest.raises(ValueError):
        env.enable_bins(ret_width=1 << 32)
    assert env._L.bk_bins_enable(env._h, None) == 5 and b"null argument" in env._L.bk_last_error()
    enable(env, cfg)
    refused(bk, lambda: enable(env, cfg), "already enabled")
    refused(bk, lambda: env.enable_bins((3,), 16), "already enabled")
    assert env.bins().shape == (2, 4, 8) and env.bins_config()["spans"].tolist() == [1, 2, 0, 0]
    # a null out-pointer and a book range past the end: refused, the table as it was
    for rc in (env._L.bk_bins_device_ptr(env._h, None), env._L.bk_get_bins(env._h, 0, 2, None), env._L.bk_bins_config_get(env._h, None)):
        assert rc == 5 and b"null argument" in env._L.bk_last_error()
    for first, n in ((1, 2), (3, 0), (0, 3)):
        refused(bk, lambda: env.bins(first, n), "book range out of bounds")
    assert env.bins(2, 0).shape == (0, 4, 8) and env.bins(1).shape == (1, 4, 8)
    with pytest.raises(ValueError):
        env.bins(-1, 1)
    same_bins(env.bins(), zeros(2, cfg), "refusals leave the table")
    with pytest.raises(ValueError):
        env.clear_bins(np.ones(3, dtype=bool))
    env.run(3)
    env.fold_bins()
    hist = ref_books(oracle, 2, 16, 16, groups=C2).history()
    same_bins(env.bins(), BM.rows(hist[2:5], cfg, first_step=2), "steps before enable_bins() are not counted")
    env.close()
    none = make_env(bk, 2, groups=C2, steps=0)
    refused(bk, lambda: enable(none, cfg), "history_capacity must be > 0")
    none.run(2)
    none.close()
    # a host-driven env: a book cannot be loaded into an env with the table
    host = bk.ManyBookEnv(2, SEED, 0, 1, STEP, levels=5, max_live_orders=16, max_orders=16, trade_capacity=16, history_capacity=4)
    host.place_order(0, True, 5, 1, 100)
    host.step()
    state = host.book_state(0)
    host.load_book_state(1, state)
    enable(host, cfg)
    refused(bk, lambda: host.load_book_state(1, state), "bin table")
    host.step()
    host.fold_bins(sync=True)
    want = zeros(2, cfg)
    want[:, 3, 0] = 1
    same_bins(host.bins(), want, "one-sided books count in the volume channel only")
    host.close()
