"""Every table folded on the device, on ONE env, across the carry of the absolute step number into its high word.

tests/test_gpu_counter_wrap.py::test_counters_carry_into_their_high_words takes an env over steps_done = 2^32 with the series
alone, whose kernel never sees a step number.  Here the restored env has the whole family on - the series with its depth
and candle companions (bars of W = 3 steps on N = 4 slots: candles::k_fold gets seen / W, seen % W, (seen / W) % N and the
last bar from the host and writes the absolute first_step into every row), the lag table, the bin table, and the flow table
(the book flows) or the per-market cross table (the market flow) - four cursors of their own, eight fold launches and as
many clears on one stream, on a ring of 12 slots (2^32 % 12 = 4, 2^32 % 3 = 1: a step cut to 32 bits anywhere between
steps_done and a kernel's arguments lands in another slot, bar and phase).  One scenario per flow: restore at 2^32 - 3,
run over the carry, save, reset the alternate units behind unfolded steps, lose a step to the ring, and continue a third
env from the image taken behind the carry.

The expected side is tests/tables_step_carry.py: the tables' plain-Python models over the ORACLE's run of the same flow,
with the conditions that keep the comparison from being trivial asserted before anything is compared (and again, without
a device, in tests/test_tables_step_carry_cpu.py).  All comparisons are exact, word for word."""
import numpy as np
import pytest

pytest.register_assert_rewrite("hist_tables", "tables_step_carry")  # (support modules: their asserts report their values too)

import counter_shift as CS  # noqa: E402
import oracle_parity as P  # noqa: E402
import tables_step_carry as SC  # noqa: E402
import test_gpu_counter_wrap as CW  # noqa: E402
from hist_tables import SERIES, bk, refused  # noqa: E402,F401 (bk is a fixture)
from tables_step_carry import CANDLE_N, CANDLE_W, CFG, FLOW_K, LOST, M32, START, T1, T2, T3  # noqa: E402

pytestmark = pytest.mark.gpu


def all_tables_on(F, p):
    """a fresh env of the flow with every folded table it can hold"""
    env = F.env()
    env.enable_series()
    env.enable_depth()
    env.enable_candles(CANDLE_W, CANDLE_N)
    env.enable_lags(CFG["lags"])
    b = CFG["bins"]
    env.enable_bins(b["spans"], b["n_bins"], b["ret_width"], b["spread_width"], b["vol_width"])
    if p.flow:
        env.enable_flow(FLOW_K)  # (not consuming: the host's readers keep every record)
    else:
        env.enable_cross(CFG["cross"])
    return env


def fold_all(env, p):
    for name in SC.FOLDS:
        if name in p.want:
            getattr(env, f"fold_{name}")()
    if p.flow:
        env.fold_flow()
    env.sync()


def read_all(env, p):
    got = {t: getattr(env, t)() for t in p.want}
    if p.flow:
        got["flow"] = (env.flow(),) + env.flow_state()
    return got


def same_flow(got, want, tag):
    assert got.dtype == want.dtype and got.shape == want.shape, f"{tag}: {got.dtype} {got.shape} vs {want.dtype} {want.shape}"
    for f in want.dtype.names:
        P.same_array(got[f], want[f], tag, f"flow field {f}")


def same_tables(env, p, stage, tag):
    """every table of the env, word for word, is the plan's table of the stage"""
    for t, w in p.want.items():
        SC.RING_TABLES[t].same(getattr(env, t)(), w[stage], f"{p.name}, {tag}: {t}")
    if p.flow:
        same_flow(env.flow(), p.flow_rows(stage), f"{p.name}, {tag}: flow")
        carry, seen = env.flow_state()
        want_carry, want_seen = p.flow_state(stage)
        P.same_array(carry, want_carry, tag, "the flow table's carry")
        P.same_array(seen, want_seen, tag, "the flow table's cursors")


def cleared_at(env, p, L, tag):
    """right behind a restore at the oracle's step L: every table reads as its cleared table, the flow's cursors stand at the
    restored trade counts, and no bar is folded"""
    for t, w in p.want.items():
        SC.RING_TABLES[t].same(getattr(env, t)(), w["cleared"], f"{p.name}, {tag}: {t}")
    if p.flow:
        carry, seen = env.flow_state()
        assert not env.flow().view(np.uint64).any() and not carry.any() and seen.tolist() == p.flow["counts"][L], tag
    assert env.candles_latest() is None and env.candles_config() == (CANDLE_W, CANDLE_N), tag


def newest_bar(rows):
    """(bar, slot) of the newest bar of the model's rows, in plain integers: the same for every book"""
    found = {(int(r["first_step"][k]) // CANDLE_W, k) for r in rows for k in [int(np.argmax(r["first_step"]))]}
    assert len(found) == 1, found
    return found.pop()


def candle_readers(bk, env, p, stage, done, tag):
    """candles_latest() and candle_series() against the model's rows of the stage, whose first_step words pass 2^32"""
    want = p.want["candles"][stage]
    bar, slot = newest_bar(want)
    assert (bar, slot) == ((done - 1) // CANDLE_W, (done - 1) // CANDLE_W % CANDLE_N) and bar > M32 // CANDLE_W - 2, (tag, bar, slot)
    assert env.candles_latest() == (bar, slot), (tag, env.candles_latest(), bar, slot)
    got, model = bk.candle_series(env.candles(), CANDLE_W), bk.candle_series(want, CANDLE_W)
    assert got.shape == model.shape == (SC.BOOKS, CANDLE_N)
    for f in model.dtype.names:  # (bit patterns: a NaN equals itself)
        a, b = (np.ascontiguousarray(x[f]) for x in (got, model))
        P.same_array(a.view(np.uint64) if a.dtype == np.float64 else a, b.view(np.uint64) if b.dtype == np.float64 else b, tag, f"candle_series {f}")
    for b in range(SC.BOOKS):  # ... and against the model's words themselves, oldest to newest
        held = sorted((int(r["first_step"]), r) for r in want[b] if r["n_steps"] > 0)
        empty = CANDLE_N - len(held)
        assert got["bar"][b].tolist() == [-1] * empty + [fs // CANDLE_W for fs, _ in held], (tag, b, got["bar"][b])
        assert got["complete"][b].tolist() == [False] * empty + [int(r["n_steps"]) == CANDLE_W for _, r in held], (tag, b)
        for k, (_, r) in enumerate(held, start=empty):
            if r["n_two_sided"] > 0:
                assert got["close"][b, k] == int(r["close_m"]) / 2.0 and got["open"][b, k] == int(r["open_m"]) / 2.0, (tag, b, k)
            else:
                assert np.isnan(got["close"][b, k]), (tag, b, k)


@pytest.mark.parametrize("name", SC.FLOWS)
def test_every_folded_table_crosses_the_step_carry_on_one_env(bk, oracle, name):
    """6 books, at most 50 steps, three envs a case: 0.02 - 0.03 s a case on an MI355X inside the whole suite (0.26 s for a
    case that is the first to touch the device)."""
    p = SC.plan(oracle, name)
    p.conditions()
    F = CW._EFlow(bk, oracle, name)
    B, n, L1, L2, L3, off, hist = SC.BOOKS, p.n, p.L1, p.L2, p.L3, p.off, p.hist
    # ---- 1. the unshifted env: the image at n, its step counters moved next to the carry
    env = F.env()
    env.run(n)
    moved = CS.shift(env.checkpoint(), B, F.pool, steps=off)
    env.close()
    # ---- 2. a fresh env with every table on, restored at 2^32 - 3
    env = all_tables_on(F, p)
    env.restore(moved)
    assert env.steps_done() == START == n + off
    cleared_at(env, p, n, "restored at 2^32 - 3")
    # ---- 3. T1 steps over the carry, folded every two steps
    env.run_series(T1, chunk=2)
    if p.flow:
        env.fold_flow()
    env.sync()
    assert env.steps_done() == L1 + off > M32
    same_tables(env, p, "T1", "over the carry")
    candle_readers(bk, env, p, "T1", L1 + off, "over the carry")
    P.same_history(env.history(), hist[n:L1], tag=f"{name}: L2 history over the carry")
    P.no_flags(env)
    # ---- 4. a snapshot and an image behind the carry; T2 steps NOT folded; the reset folds them and cuts the masked carries
    env.save_snapshot()
    image = env.checkpoint()
    env.run(T2)
    (env.reset_markets if p.market else env.reset_books)(p.mask)
    same_tables(env, p, "at_reset", "right behind the reset: the counts have gone on")
    SERIES.busy("at_reset", None, mask=p.per_book, got=env.series())
    if p.flow:
        carry = env.flow_state()[0]
        assert not carry[p.per_book].any() and carry[~p.per_book].any()
    assert env.candles_latest() == newest_bar(p.want["candles"]["at_reset"]) == ((L2 + off - 1) // CANDLE_W, (L2 + off - 1) // CANDLE_W % CANDLE_N)
    # ---- 5. T3 steps: a kept unit holds [n, L3), a reset one [n, L2), the cut, and the oracle's steps L1 .. L1 + T3 replayed
    env.run(T3)
    fold_all(env, p)
    assert env.steps_done() == L3 + off
    same_tables(env, p, "T3", "behind the reset")
    candle_readers(bk, env, p, "T3", L3 + off, "behind the reset")
    tail = env.history()[-T3:]
    for b in range(B):
        L = L1 + T3 if p.per_book[b] else L3
        P.same_history(tail[:, b], hist[L - T3:L, b], tag=f"{name}: L2 history tail of book {b} behind the reset")
    P.no_flags(env)
    # ---- 6. LOST = 13 steps into a ring of 12 without a fold: every fold refuses, naming the lost step by its 64-bit number
    before = read_all(env, p)
    env.run(LOST)
    done = L3 + off
    assert env.steps_done() == done + LOST and done > M32
    for _ in range(2):  # (twice: a refusal leaves the cursor too)
        for fold, noun in SC.FOLDS.items():
            if fold in p.want:
                refused(bk, getattr(env, f"fold_{fold}"), rf"\b1 step\(s\) of the {noun} were lost: steps \[{done}, {done + 1}\) are no longer retained")
    after = read_all(env, p)
    for t in p.want:
        SC.RING_TABLES[t].same(after[t], before[t], f"{name}: {t} is unchanged by the refusals")
    if p.flow:
        assert all(a.tobytes() == b.tobytes() for a, b in zip(after["flow"], before["flow"])), "the flow table is unchanged"
    env.close()
    # ---- 7. a third env from the image taken behind the carry: cleared, rebased at n + T1 + off > 2^32, and on from there
    env = all_tables_on(F, p)
    env.restore(image)
    assert env.steps_done() == L1 + off > M32
    cleared_at(env, p, L1, "the third env, restored behind the carry")
    env.run(T2)
    fold_all(env, p)
    assert env.steps_done() == L2 + off
    same_tables(env, p, "third", "the third env")
    candle_readers(bk, env, p, "third", L2 + off, "the third env")
    P.same_history(env.history(), hist[L1:L2], tag=f"{name}: L2 history of the third env")
    P.no_flags(env)
    env.close()
