"""The per-level depth table (bk_depth_enable; bourse_amd/csrc/depth.hpp): per book levels + 1 rows of sixteen u64 words -
the sums of the resting volume and order count per level, of the cumulative imbalance and of the mid's next move against
it, and the header - folded on the device from the ladder of the level-2 history ring beside the series moments, whose
cursor, fold, clears and cuts it shares.

The expected side never shares code with the kernel: tests/depth_model.py::fold (plain Python ints) over the ORACLE's
history() of the same run - oracle.ManyBooks / ManyMarkets for bk_run, one oracle.StepEnv per book for the host-driven and
the device-ingress flows - and the device's own history is held against the oracle's through tests/oracle_parity.py where
the ring still retains it.  Where a case says something only under a condition - occupied levels, one-sided steps, moves
with and against the imbalance, a sum that wraps - the condition is asserted on the expected side before anything is
compared.  All comparisons are exact.  The scenarios the three ring tables share (tests/hist_tables.py,
tests/test_gpu_hist_tables.py) run here through an adapter whose fold and clear are the series'."""
import numpy as np
import pytest

pytest.register_assert_rewrite("hist_tables")  # (a support module: its asserts report their values too)

import depth_model as DM  # noqa: E402
import oracle_parity as P  # noqa: E402
import series_model as SM  # noqa: E402
import test_gpu_hist_tables as HT  # noqa: E402
from hist_tables import (SEED, SERIES, Table, bk, host_driven, lost, masked_clear_folds_first, refused,  # noqa: E402,F401
                         reset_books_cuts_the_carry)
from test_gpu_reset_books import PIPELINES, STEP, as_kind, make_env, ref_books  # noqa: E402

pytestmark = pytest.mark.gpu
MAXU = 0xFFFFFFFF
M64 = (1 << 64) - 1
# the usual C2 groups leave every level from 16 on empty: prices 10 .. 150 around the mid fill 64 levels of tick 2
WIDE = [(32, (10, 150), (10, 20), 2, 0.8), (32, (10, 150), (50, 70), 2, 0.2)]
F, H = {n: i for i, n in enumerate(DM.FIELDS)}, {n: i for i, n in enumerate(DM.HEADER_FIELDS)}
NO_TABLE = "this env has no depth table: call bk_depth_enable first"


class Depth(Table):
    """the depth table as tests/hist_tables.py sees a table: its configuration is the env's level count, and its fold and
    clear are the series'"""
    name, noun, dtype = "depth", "series", np.uint64
    cfg = dict(reset=16, clear=16, restore=16, ingress_reset=10, markets=10)

    def enable(self, env, L=None):
        assert L is None or L == env.levels
        env.enable_series()
        env.enable_depth()
        return env

    def fold(self, env, **kw):
        return env.fold_series(**kw)

    def clear(self, env, *a, **kw):
        return env.clear_series(*a, **kw)

    def rows(self, hist, L=None, **kw):
        return DM.rows(hist, **kw)

    def fold_model(self, h, L=None, **kw):
        return DM.fold(h, **kw)

    def table(self, s):
        return DM.table(s)

    def cleared(self, B, L):
        return np.zeros((B, L + 1, 16), dtype=np.uint64)

    def same(self, got, want, tag):
        assert got.dtype == want.dtype == np.uint64, (got.dtype, want.dtype)
        assert got.shape == want.shape, f"{tag}: table {got.shape} vs {want.shape}"
        for i, n in enumerate(DM.FIELDS):
            P.same_array(got[:, :-1, i], want[:, :-1, i], tag, f"depth word {n} of every level")
        P.same_array(got[:, -1], want[:, -1], tag, "the header row")

    def view_shape(self, B, L):
        return (B, L + 1, 16)

    def at_reset(self, hist, mask, L):
        return DM.rows(hist)  # (a cut leaves the rows)

    def busy(self, case, want, L=None, mask=None, uncut=None, total=None, hist=None, got=None):
        if case == "reset":
            assert any((u != w).any() for u, w in zip(uncut, want[mask])), "the cut shows in the masked books' rows"
            assert (want[:, -1, H["n_steps"]] == total).all() and (want[mask][:, -1, H["n_pairs"]] > 0).all()
        elif case == "ingress_reset":
            assert (want[:, -1, H["n_steps"]] == 8).all() and (want[:, -1, H["n_pairs"]] > 0).all()
            assert (want[:, 0, F["n_signed"]] > 0).all()
        elif case == "clear":  # the masked books start again at step 10
            assert (want[mask][:, -1, H["n_steps"]] == 6).all() and (want[~mask][:, -1, H["n_steps"]] == 16).all()


DEPTH = Depth()
same_depth = DEPTH.same


def header_is_the_series(rows, series, tag):
    """the header's identities against the series row over the same steps and cuts"""
    for a, b in (("n_steps", "n_steps"), ("n_two_sided", "n_two_sided"), ("n_pairs", "n_ret"), ("sum_d", "sum_d"), ("sum_abs_d", "sum_abs_d")):
        P.same_array(rows[:, -1, H[a]], series[b].astype(np.uint64), tag, f"the header's {a} against the series' {b}")
    assert not rows[:, -1, len(H):].any(), f"{tag}: words 9 .. 15 of the header are zero"


def busy_ladder(want, hist):
    """what the issue found on the CPU oracle at every level count, asserted before anything is compared"""
    lv, hd = want[:, :-1], want[:, -1]
    assert (lv[:, :, F["n_bid_steps"]] >= 3).all() and (lv[:, :, F["n_ask_steps"]] >= 3).all(), "every level is occupied on both sides"
    assert (hd[:, H["n_two_sided"]] < hd[:, H["n_steps"]]).sum() >= 4, "four of the five books have a one-sided step"
    for q in (0, -1):
        agree = int(lv[:, q, F["n_agree"]].sum())
        against = int(lv[:, q, F["n_move"]].sum()) - agree
        assert agree > 40 and against > 40, (q, agree, against)
    up, down = int(hd[:, H["n_up"]].sum()), int(hd[:, H["n_down"]].sum())
    assert min(up, down) > 0.8 * max(up, down), (up, down)
    assert (hd[:, H["n_steps"]] == hist.shape[0]).all()


_models = {}


def model_at(oracle, L, B, total, ends):
    """the model's tables after every prefix in ``ends`` of the oracle's run, folded once and shared"""
    key = (L, B, total, tuple(ends))
    if key not in _models:
        hist = ref_books(oracle, B, L, total, groups=WIDE).history()
        states, lo, out = [DM.cleared(L) for _ in range(B)], 0, {}
        for y in ends:
            for b in range(B):
                DM.fold(hist[lo:y, b], first_step=lo, into=states[b])
            out[y], lo = np.array([DM.table(s) for s in states], dtype=np.uint64), y
        _models[key] = (hist, out)
    return _models[key]


def wide_env(bk, B, L, cap, **kw):
    return DEPTH.enable(make_env(bk, B, groups=WIDE, levels=L, pool=64, steps=cap, **kw))


# ------------------------------------------------------------------------------------------------ 1. levels and fold lengths
def folded_in_three_parts(bk, oracle, L, pipeline=None):
    """5 books (the last block of four waves holds one), a ring of 96: run(70) and fold, run(26) and fold - the ring at its
    last slots - run(40) and fold - the ring wrapped; a twin with a ring of 136 folds once.  At 64 / Lp steps a pass every
    fold ends in a pass that is not full for some L, and starts from the carry."""
    B, cap, parts = 5, 96, (70, 26, 40)
    total = sum(parts)
    ends = tuple(int(x) for x in np.cumsum(parts))
    hist, want = model_at(oracle, L, B, total, ends)
    busy_ladder(want[total], hist)
    env, twin = wide_env(bk, B, L, cap), wide_env(bk, B, L, total)
    if pipeline:
        env.set_pipeline(pipeline)
        twin.set_pipeline(pipeline)
    same_depth(env.depth(), DEPTH.cleared(B, L), "nothing is folded before fold_series()")
    done = 0
    for n in parts:
        env.run(n, sync=False)
        twin.run(n, sync=False)
        env.fold_series()
        done += n
        same_depth(env.depth(), want[done], f"after {done} steps (L = {L}, {pipeline})")
        header_is_the_series(env.depth(), env.series(), f"after {done} steps")
    twin.fold_series()
    same_depth(twin.depth(), want[total], "one fold of 136 steps")
    same_depth(want[total], DM.rows(hist), "three folds of the model against one pass")
    header_is_the_series(twin.depth(), twin.series(), "one fold")
    header_is_the_series(want[total], SM.rows(hist), "the models")
    same_depth(env.depth(1, 3), want[total][1:4], "depth(first_book, n_books)")
    env.fold_series(sync=True)  # no new step: no launch, nothing changes
    same_depth(env.depth(), want[total], "a second fold without a step")
    for e in (env, twin):
        P.no_flags(e)
    P.same_history(env.history(), hist[done - cap:])
    P.same_history(twin.history(), hist)
    env.close()
    twin.close()


@pytest.mark.parametrize("L", [1, 5, 16, 33, 64])
def test_levels_and_fold_lengths_equal_the_model_and_one_pass(bk, oracle, L):
    folded_in_three_parts(bk, oracle, L)


@pytest.mark.parametrize("pipeline", PIPELINES)
def test_the_fold_does_not_depend_on_who_wrote_the_ring(bk, oracle, pipeline):
    folded_in_three_parts(bk, oracle, 16, pipeline)


# ------------------------------------------------------------------------------------------------ 2. single steps
def test_single_step_folds_across_a_one_sided_step(bk, oracle):
    """A ring of 8 and 30 folds of one step each at L = 5 (twelve lanes of a pass hold no step, eight steps a pass): every
    pair takes its first half from the carry, and the one-sided steps in the middle break the chain."""
    B, T, L = 5, 30, 5
    hist = ref_books(oracle, B, L, T, groups=WIDE).history()
    two = (hist[:, :, 1] != 0) & (hist[:, :, 2] != MAXU)
    assert (~two[2:T - 2]).any() and two[:2].all() and two[T - 2:].all(), "a one-sided step in the middle of the run"
    env = wide_env(bk, B, L, 8)
    states = [DM.cleared(L) for _ in range(B)]
    for t in range(T):
        env.run(1, sync=False)
        env.fold_series()
        for b in range(B):
            DM.fold(hist[t:t + 1, b], first_step=t, into=states[b])
        want = np.array([DM.table(s) for s in states], dtype=np.uint64)
        same_depth(env.depth(), want, f"after step {t}")
    assert (want[:, -1, H["n_pairs"]] > 10).all() and (want[:, :-1, F["n_signed"]] > 0).all()
    assert (want[:, -1, H["n_pairs"]] < T - 1).any()
    same_depth(want, DM.rows(hist), "the model is split-invariant")
    header_is_the_series(env.depth(), env.series(), "single steps")
    P.no_flags(env)
    P.same_history(env.history(), hist[T - 8:])
    env.close()


# ------------------------------------------------------------------------------------------------ 3. enable order
def test_enable_order(bk, oracle):
    B, L = 3, 16
    hist = ref_books(oracle, B, L, 16, groups=WIDE).history()
    env = make_env(bk, B, groups=WIDE, levels=L, pool=64, steps=8)
    refused(bk, env.enable_depth, "bk_series_enable")  # depth without the series
    for call in (env.depth, env.depth_device_ptr, env.depth_view):
        refused(bk, call, NO_TABLE)
    env.enable_series()
    for call in (env.depth, env.depth_device_ptr, env.depth_view):
        refused(bk, call, NO_TABLE)
    # lost steps: the series' fold refuses, so does the enable, and the env stays without the table
    env.run(9)
    lost(bk, SERIES, env.enable_depth, 1)
    refused(bk, env.depth, NO_TABLE)
    lost(bk, SERIES, env.fold_series, 1)
    assert (env.series()["n_steps"] == 0).all()
    env.close()
    # 7 folded and 3 unfolded steps: the enable folds the three into the series, the depth rows count from step 10
    env = make_env(bk, B, groups=WIDE, levels=L, pool=64, steps=16)
    env.enable_series()
    env.run(7)
    env.fold_series()
    env.run(3)
    env.enable_depth()
    assert (env.series()["n_steps"] == 10).all()
    same_depth(env.depth(), DEPTH.cleared(B, L), "cleared at the enable")
    refused(bk, env.enable_depth, "already enabled")  # a second enable
    assert env._L.bk_depth_device_ptr(env._h, None) == 5 and b"null argument" in env._L.bk_last_error()
    assert env._L.bk_get_depth(env._h, 0, B, None) == 5 and b"null argument" in env._L.bk_last_error()
    for first, n in ((1, 3), (4, 0), (0, 4)):
        refused(bk, lambda: env.depth(first, n), "book range out of bounds")
    assert env.depth(3, 0).shape == (0, L + 1, 16) and env.depth(1).shape == (2, L + 1, 16)
    env.run(6)
    env.fold_series(sync=True)
    want = DM.rows(hist[10:], first_step=10)  # (step 10 has no past: no pair reaches in front of the enable)
    assert (want[:, -1, H["n_steps"]] == 6).all() and (want[:, -1, H["n_pairs"]] > 0).all()
    same_depth(env.depth(), want, "counted from the enable on")
    SERIES.same(env.series(), SM.rows(hist), "the series row holds all sixteen steps")
    P.no_flags(env)
    env.close()


# ------------------------------------------------------------------------------------------------ 4. cuts, clears, restore
@pytest.mark.parametrize("kind", ["host", "device"])
def test_reset_books_cuts_the_carry_of_the_books_it_resets(bk, oracle, kind):
    reset_books_cuts_the_carry(bk, oracle, DEPTH, kind)


@pytest.mark.parametrize("kind", ["host", "device"])
def test_a_masked_clear_folds_first_clears_both_tables_and_the_view_is_the_table_in_place(bk, oracle, kind):
    """clear_series(mask) folds first and then clears both tables of the masked books; the view, made before any step,
    shows the latest fold"""
    masked_clear_folds_first(bk, oracle, DEPTH, kind)


def test_a_full_clear_starts_both_tables_again(bk, oracle):
    B, L = 3, 16
    hist = ref_books(oracle, B, L, 16, groups=WIDE).history()
    env = wide_env(bk, B, L, 16)
    env.run(6)
    env.fold_series()
    same_depth(env.depth(), DM.rows(hist[:6]), "six steps")
    env.run(4)  # (outstanding: a full clear folds nothing)
    env.clear_series()
    same_depth(env.depth(), DEPTH.cleared(B, L), "clear_series() clears the depth rows")
    assert (env.series()["n_steps"] == 0).all()
    env.run(6)
    env.fold_series()
    want = DM.rows(hist[10:], first_step=10)
    assert (want[:, -1, H["n_pairs"]] > 0).all()
    same_depth(env.depth(), want, "both count from step 10 on, with no past")
    header_is_the_series(env.depth(), env.series(), "after the full clear")
    P.no_flags(env)
    env.close()


def test_restore_clears_both_tables(bk, oracle):
    HT.test_restore_clears_the_table_and_rebases_the_cursor(bk, oracle, DEPTH)


def test_a_reset_refused_for_lost_steps_changes_neither_table(bk, oracle):
    B, L = 3, 16
    hist = ref_books(oracle, B, L, 16, groups=WIDE).history()
    env = wide_env(bk, B, L, 8)
    env.run(2)
    env.save_snapshot()
    env.run(3)
    env.fold_series()
    depth_at_5, series_at_5 = env.depth(), env.series()
    same_depth(depth_at_5, DM.rows(hist[:5]), "five steps")
    env.run(9)  # steps 5 .. 13 into a ring of 8: step 5 is gone
    mask = np.array([1, 0, 1], dtype=bool)
    lost(bk, SERIES, lambda: env.reset_books(mask), 1)
    assert env.steps_done() == 14
    same_depth(env.depth(), depth_at_5, "a refused reset leaves the depth rows")
    SERIES.same(env.series(), series_at_5, "... and the series")
    lost(bk, SERIES, lambda: env.clear_series(mask), 1)
    same_depth(env.depth(), depth_at_5, "a refused clear leaves the depth rows")
    env.clear_series()
    env.reset_books(mask)
    same_depth(env.depth(), DEPTH.cleared(B, L), "cleared at step 14 and nothing folded since")
    env.close()


# ------------------------------------------------------------------------------------------------ 5. host-driven volumes
def test_host_driven_volumes_pass_two_to_the_32_and_the_sums_wrap(bk, oracle):
    """Host-driven, L = 5, tick 1: three bids of volume 2^32 - 1 at 100, 99, 98 against an ask of 3 at 104 and one far out
    at 0xFFFFFFFE.  A bid at 104 takes the near ask: the mid jumps by almost 2^31 with J_2 = 3 (2^32 - 1) - 3 in front of it,
    so sum_imb_d passes 2^64 and I_q^2 wraps at every level from 1 on.  Then a bid at 101 and its cancellation: one move
    with and one against the imbalance of the deeper levels."""
    B, BIG = 2, MAXU
    steps = [[("place_order", range(B), (True, BIG, 1, 100)), ("place_order", range(B), (True, BIG, 1, 99)),
              ("place_order", range(B), (True, BIG, 1, 98)), ("place_order", range(B), (False, 3, 2, 104)),
              ("place_order", range(B), (False, 50, 2, 0xFFFFFFFE))],
             [("place_order", range(B), (True, 3, 3, 104))], [("place_order", range(B), (True, 7, 3, 101))],
             [("cancel_order", range(B), (6,))], [("place_order", (1,), (False, 2, 4, 100))]]
    (env,), refs = host_driven(bk, oracle, B, 8, [lambda e: DEPTH.enable(e)], steps, step_size=1000)
    ref_hist = np.stack([r.history() for r in refs], axis=1)
    assert ref_hist[:, 0, 1].tolist() == [100, 100, 101, 100, 100] and ref_hist[:, 0, 2].tolist() == [104] + [0xFFFFFFFE] * 4
    assert ref_hist[0, 0, 5:17].tolist() == [BIG, 1, 3, 1, BIG, 1, 0, 0, BIG, 1, 0, 0]
    exact = [DM.fold(ref_hist[:, b]) for b in range(B)]
    for s in exact:
        assert s["rows"][2]["sum_imb_d"] >> 64 and s["rows"][2]["sum_imb_sq"] >> 64, "the exact sums pass 2^64"
        assert s["rows"][2]["sum_abs_imb"] // 5 > 1 << 32, "the cumulative imbalance passes 2^32"
        # the cancellation's move down: with the imbalance at the touch (7 against 50), against it from level 1 on
        assert s["rows"][0]["n_agree"] == 3 and s["rows"][2]["n_agree"] == 2 and s["rows"][2]["n_move"] == 3 and s["header"]["n_down"] == 1
    env.fold_series(sync=True)
    P.no_flags(env)
    hist = env.history()
    for b, r in enumerate(refs):
        P.same_history(hist[:, b], r.history(), f"L2 history of book {b}")
    want = DM.rows(ref_hist)
    assert (want[0] != want[1]).any()
    same_depth(env.depth(), want, "volumes of 2^32 - 1")
    header_is_the_series(env.depth(), env.series(), "host-driven")
    m = bk.depth_moments(env.depth())
    assert m.shape == (B, 5) and (m["hit_rate"][:, 0] == 1.0).all() and (m["hit_rate"][:, 2] == 2 / 3).all() and (m["bid_occupancy"][:, :3] == 1.0).all()
    env.close()


# ------------------------------------------------------------------------------------------------ 6. device ingress
def test_reset_ingress_books_cuts_the_carry_too(bk, oracle):
    HT.test_reset_ingress_books_cuts_the_carry_too(bk, oracle, DEPTH)


# ------------------------------------------------------------------------------------------------ 7. markets
@pytest.mark.parametrize("kind", ["host", "device"])
def test_markets_keep_rows_per_book_and_reset_markets_cuts_per_market(bk, oracle, kind):
    """2 markets x 3 assets, rows per book; the reset's mask has one byte per MARKET and the cut must reach the three books
    of market 0 and none of market 1.  6 steps, save, 5 steps not folded, reset, 7 steps."""
    NM, A, n, m, k, L = 2, 3, 6, 5, 7, 10
    ticks = [1, 2, 2]
    groups = [(0, 40, (40, 56), (10, 20), 1, 0.8), (1, 30, (40, 56), (50, 70), 2, 0.5), (2, 30, (40, 56), (10, 30), 2, 0.6),
              (0, 20, (30, 70), (5, 9), 2, 0.3)]
    ref = oracle.ManyMarkets(NM, SEED, 0, ticks, STEP, True, L, groups)
    ref.run(n + m + k)
    hist = ref.history()
    assert hist.shape == (n + m + k, NM * A, 5 + 4 * L)
    kw = {}
    if kind == "device":
        import torch

        kw["stream"] = torch.cuda.current_stream().cuda_stream
    env = bk.ManyMarketEnv(NM, SEED, 0, ticks, STEP, True, levels=L, max_live_orders=128, trade_capacity=4096,
                           history_capacity=n + m + k, **kw)
    env.set_random_market_agents(groups)
    DEPTH.enable(env)
    env.run(n)
    env.save_snapshot()
    env.fold_series()
    rows = DM.rows(hist[:n])
    assert rows.shape == (6, L + 1, 16) and len({w.tobytes() for w in rows}) == 6 and (rows[:, 0, F["n_bid_steps"]] > 0).all()
    same_depth(env.depth(), rows, "markets, rows per book")
    env.run(m)
    mask = np.array([1, 0], dtype=bool)
    mm, _ = as_kind(mask, kind)
    env.reset_markets(mm, sync=(kind == "host"))
    env.run(k)
    env.fold_series()
    want = []
    for b in range(NM * A):
        # what the book went through: a reset one replays steps n .. n + k - 1 behind a cut, a kept one has no cut
        went = np.concatenate([hist[:n + m, b], hist[n:n + k, b]]) if mask[b // A] else hist[:, b]
        cut, uncut = (DM.table(DM.fold(went, cuts=c)) for c in ([n + m], []))
        assert (cut != uncut).any(), f"a cut would show in book {b}"
        want.append(cut if mask[b // A] else uncut)
    same_depth(env.depth(), np.array(want, dtype=np.uint64), f"reset_markets ({kind})")
    P.no_flags(env)
    env.close()
