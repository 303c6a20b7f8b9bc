"""The per-market cross table (bk_cross_enable; bourse_amd/csrc/cross.hpp): per market, span and ORDERED pair of assets eight
u64 words - the moments behind the covariance of the two assets' changes of the mid over the span, and the product of one
asset's change with the other's previous one - folded on the device from the level-2 history ring.

The expected side never shares code with the kernel: tests/cross_model.py::fold (plain Python ints) over the ORACLE's
history() of the same run - oracle.ManyMarkets for bk_run, for the device ingress and for the host-driven market - and the
device's own history is held against the oracle's through tests/oracle_parity.py where the ring still retains it.  Where a
case says something only under a condition - pairs that are thinner than their diagonals, both signs, a cut that shows, a
product that wraps - the condition is asserted on the expected side before anything is compared.  All comparisons are
exact."""
import numpy as np
import pytest

import cross_model as XM
import lags_model as LM
import oracle_parity as P
import series_model as SM

pytestmark = pytest.mark.gpu
SEED, STEP, LEVELS = 101, 100, 10
MAXU = 0xFFFFFFFF
M64 = (1 << 64) - 1
FOLD_WAVES = 4  # cross::FOLD_WAVES: markets per block of k_fold
PIPELINES = ("fused", "split", "wave_split", "wave")  # (a market env takes every request: pipeline_plan.hpp falls back)
NO_TABLE = "no cross table: call .*bk_cross_enable.* first"


@pytest.fixture(scope="module")
def bk():
    import bourse_amd

    return bourse_amd


def refused(bk, call, match):
    with pytest.raises(bk.BourseError, match=match) as e:
        call()
    assert e.value.code == 5


def lost(bk, call, n):
    refused(bk, call, rf"\b{n} step\(s\) of the cross table were lost")


def groups_of(A):
    """two groups per asset; at A = 8 only the first of each (an env takes at most 8 groups)"""
    g = []
    for a in range(A):
        g.append((a, 24, (40, 56), (10, 20), 2, 0.8 - 0.05 * a))
        if A != 8:
            g.append((a, 8, (40, 56), (50, 70), 2, 0.3))
    return g


def pool_of(A):
    """max_live_orders: 64 where the market's agents fit - an env refuses fewer slots than agents (one pool slot per agent),
    and a market of A assets has 32 A of them (24 A at A = 8) - else the next pool size that holds them"""
    agents = sum(g[1] for g in groups_of(A))
    return next(p for p in (64, 128, 256, 512) if p >= agents)


def market_env(bk, NM, A, cap, spans=None, kind="host", step=STEP, **kw):
    if kind == "device":
        import torch

        kw["stream"] = torch.cuda.current_stream().cuda_stream
    env = bk.ManyMarketEnv(NM, SEED, 0, [2] * A, step, True, levels=LEVELS, max_live_orders=pool_of(A), trade_capacity=4096, history_capacity=cap,
                           **kw)
    env.set_random_market_agents(groups_of(A))
    if spans is not None:
        env.enable_cross(spans)
    return env


_hists, _want = {}, {}


def ref_hist(oracle, NM, A, steps, step=STEP):
    """the history of oracle.ManyMarkets of this shape after `steps` steps: computed once, shared, never changed"""
    key = (NM, A, steps, step)
    if key not in _hists:
        ref = oracle.ManyMarkets(NM, SEED, 0, [2] * A, step, True, LEVELS, groups_of(A))
        ref.run(steps)
        _hists[key] = ref.history()
        assert _hists[key].shape == (steps, NM * A, 5 + 4 * LEVELS)
        _hists[key].flags.writeable = False
    return _hists[key]


def model(hist, spans, A, key, **kw):
    """cross_model.rows over the oracle's history, computed once per (run, spans, range) and shared"""
    key = (tuple(spans), A) + key
    if key not in _want:
        _want[key] = XM.rows(hist, spans, A, **kw)
    return _want[key].copy()


def same(got, want, tag):
    assert got.dtype == want.dtype == XM.CROSS_DTYPE, (got.dtype, want.dtype)
    assert got.shape == want.shape, f"{tag}: rows {got.shape} vs {want.shape}"
    for f in XM.FIELDS:
        P.same_array(got[f], want[f], tag, f"cross word {f}")


def cleared(NM, spans, A):
    return np.zeros((NM, len(spans), A, A), dtype=XM.CROSS_DTYPE)


def busy(want, hist, A, lead=True):
    """what the oracle's run must hold for the comparison to say anything (asserted over the EXPECTED table): every ordered
    pair counts, the off-diagonal pairs are thinner than their diagonals in nearly all cases, the off-diagonal products
    take both signs, and every book has a one-sided step"""
    assert (want["n"] > 0).all(), want["n"]
    if lead:
        assert (want["n_lead"] > 0).all(), want["n_lead"]
    off = ~np.eye(A, dtype=bool)
    diag = want["n"][..., np.arange(A), np.arange(A)]  # [NM, S, A]
    thinner = (want["n"] < diag[..., :, None]) & (want["n"] < diag[..., None, :])
    assert thinner[..., off].mean() > 0.9, thinner[..., off].mean()
    for f in ("sum_xy", "sum_lead"):
        assert (want[f][..., off] > 0).any() and (want[f][..., off] < 0).any(), f
    two = (hist[:, :, 1] != 0) & (hist[:, :, 2] != MAXU)
    assert ((~two).sum(axis=0) >= 1).all(), "every book has a one-sided step"


# ------------------------------------------------------------------------------------------------ 1. three parts, one pass
@pytest.mark.parametrize("pipeline", [None] + list(PIPELINES))
def test_run_folded_in_three_parts_equals_the_model_and_one_pass(bk, oracle, pipeline):
    """5 markets of 3 assets (the last block of four waves holds one), spans (1, 5, 64), a ring of 96: run(70) and fold - two
    chunks of the windows - run(26) and fold - the ring at its last slots - run(40) and fold - the ring wrapped.  A twin
    with a ring of 136 folds once.  The same under every pipeline: the fold does not depend on who wrote the ring."""
    NM, A, spans, cap, parts = FOLD_WAVES + 1, 3, (1, 5, 64), 96, (70, 26, 40)
    total = sum(parts)
    hist = ref_hist(oracle, NM, A, total)
    final = model(hist, spans, A, ("run", NM, total))
    busy(final, hist, A)
    at64 = final[:, 2]
    assert (at64["n"] >= 38).all() and (at64["n_lead"] >= 2).all() and (at64["n_lead"] <= 8).all(), (at64["n"].min(), at64["n_lead"])
    env, twin = market_env(bk, NM, A, cap, spans), market_env(bk, NM, A, total, spans)
    if pipeline:
        env.set_pipeline(pipeline)
        twin.set_pipeline(pipeline)
    done = 0
    for n in parts:
        env.run(n, sync=False)
        twin.run(n, sync=False)
        env.fold_cross()
        done += n
        same(env.cross(), model(hist[:done], spans, A, ("run", NM, done)), f"after {done} steps ({pipeline})")
    twin.fold_cross()
    same(twin.cross(), final, "one fold of 136 steps")
    same(env.cross(), final, "three folds against one pass of the model")
    same(env.cross(1, 2), final[1:3], "cross(first_market, n_markets)")
    for e in (env, twin):
        P.no_flags(e)
    P.same_history(env.history(), hist[done - cap:])
    P.same_history(twin.history(), hist)
    env.close()
    twin.close()


# ------------------------------------------------------------------------------------------------ 2. rounds
@pytest.mark.parametrize("A,NM,spans,parts", [(8, 2, (1, 2, 3, 8), (11, 29)), (4, 2, (1, 2, 3, 8), (11, 29)), (2, 5, (1, 5, 20, 64), (70, 66))],
                         ids=["256_units", "64_units", "16_units"])
def test_four_rounds_one_full_round_and_a_quarter_of_one(bk, oracle, A, NM, spans, parts):
    """A = 8 with four spans: 256 units, every lane owns four; A = 4: 64 units, one full round and no second; A = 2: 16 units
    on 16 lanes, at spans up to 64 over 136 steps.  At A = 8 a market's 192 agents queue more than 100 events a step, and a
    step of 100 time units raises FLAG_STEP_SIZE in market 0 (seen on the device): that case runs at a step size of 200, the
    nearest shape that raises no flag."""
    total = sum(parts)
    assert len(spans) * A * A == {8: 256, 4: 64, 2: 16}[A]
    step = 200 if A == 8 else STEP
    hist = ref_hist(oracle, NM, A, total, step)
    final = model(hist, spans, A, ("run", NM, total))
    busy(final, hist, A)
    env = market_env(bk, NM, A, total, spans, step=step)
    done = 0
    for n in parts:
        env.run(n, sync=False)
        env.fold_cross()
        done += n
        got = env.cross()
        P.no_flags(env)  # (a book that dropped an order has left the oracle's path: say that, not a difference of sums)
        P.same_history(env.history(), hist[:done])
        same(got, model(hist[:done], spans, A, ("run", NM, done)), f"after {done} steps")
    assert env.cross_config()["n_spans"] == 4 and env.cross_config()["spans"].tolist() == list(spans)
    P.no_flags(env)
    P.same_history(env.history(), hist)
    env.close()


# ------------------------------------------------------------------------------------------------ 3. single steps, a short ring
def test_single_step_folds_on_a_ring_shorter_than_the_carry(bk, oracle):
    """spans (1, 3): the carry holds 6 steps of every asset, the ring 4; a fold behind every one of 13 steps takes every
    word in front of the step from the carry"""
    NM, A, spans, cap, T = 3, 2, (1, 3), 4, 13
    hist = ref_hist(oracle, NM, A, T)
    final = model(hist, spans, A, ("run", NM, T))
    assert (final["n"] > 0).all(), final["n"]
    env = market_env(bk, NM, A, cap, spans)
    states = [XM.cleared(spans, A) for _ in range(NM)]
    for t in range(T):
        env.run(1, sync=False)
        env.fold_cross()
        for m in range(NM):
            XM.fold(hist[t:t + 1, m * A:(m + 1) * A], first_step=t, into=states[m])
        same(env.cross(), np.array([XM.table(s) for s in states], dtype=XM.CROSS_DTYPE), f"after step {t}")
    same(env.cross(), final, "thirteen folds against one pass of the model")
    P.no_flags(env)
    P.same_history(env.history(), hist[T - cap:])
    env.close()


# ------------------------------------------------------------------------------------------------ 4. the lag table pins the diagonal
def test_identities_with_the_lag_table_on_the_same_env(bk, oracle):
    NM, A, spans, T = 2, 3, (1, 5, 64), 136
    hist = ref_hist(oracle, NM, A, T)
    want = model(hist, spans, A, ("run", NM, T))
    busy(want, hist, A)
    env = market_env(bk, NM, A, T, spans)
    env.enable_lags(64)
    env.run(70, sync=False)
    env.fold_cross()
    env.fold_lags()
    env.run(66, sync=False)
    env.fold_lags()
    env.fold_cross(sync=True)
    got, lag = env.cross(), env.lags()
    same(got, want, "the cross table")
    want_lag = LM.rows(hist, 64)
    for f in LM.FIELDS:
        P.same_array(lag[f], want_lag[f], "the lag table beside it", f"lag word {f}")
    for rows, lags, tag in ((got, lag, "device"), (want, want_lag, "models")):
        for m in range(NM):
            for a in range(A):
                for j, h in enumerate(spans):
                    d, l = rows[m, j, a, a], lags[m * A + a, h - 1]
                    assert d["n"] == l["n_h"] and d["sum_x"] == d["sum_y"] == l["sum_h"], (tag, m, a, h)
                    assert d["sum_xx"] == d["sum_yy"] == l["sum_h2"] and np.uint64(d["sum_xy"]) == l["sum_h2"], (tag, m, a, h)
                d, l = rows[m, 0, a, a], lags[m * A + a, 0]
                assert d["n_lead"] == l["n_pairs"] and d["sum_lead"] == l["sum_dd"], (tag, m, a)
        t = np.swapaxes(rows, 2, 3)
        for f, g in (("n", "n"), ("sum_xy", "sum_xy"), ("sum_x", "sum_y"), ("sum_xx", "sum_yy")):
            P.same_array(rows[f], t[g], tag, f"{f} of (a, b) against {g} of (b, a)")
    P.no_flags(env)
    P.same_history(env.history(), hist)
    env.close()


# ------------------------------------------------------------------------------------------------ 5. resets
@pytest.mark.parametrize("kind", ["host", "device"])
def test_reset_markets_cuts_every_asset_of_a_masked_market(bk, oracle, kind):
    """3 markets x 2 assets; 6 steps, save, fold; 5 steps NOT folded; reset markets 0 and 2 - which folds the five first and
    cuts the carry of both assets - then 7 steps.  A reset market replays steps 6 .. 12 of the same seed behind the cut; no
    span or lead reaches over it, and the sums go on."""
    NM, A, n, m, k, spans = 3, 2, 6, 5, 7, (1, 3)
    hist = ref_hist(oracle, NM, A, n + m + k)
    env = market_env(bk, NM, A, n + m + k, spans, kind=kind)
    env.run(n)
    env.save_snapshot()
    env.fold_cross()
    same(env.cross(), model(hist[:n], spans, A, ("run", NM, n)), "six steps")
    env.run(m)
    mask = np.array([1, 0, 1], dtype=bool)
    if kind == "device":
        import torch

        env.reset_markets(torch.tensor(mask, device="cuda"), sync=False)
    else:
        env.reset_markets(mask)
    same(env.cross(), model(hist[:n + m], spans, A, ("run", NM, n + m)), "the reset folded the five steps (a cut leaves the rows)")
    env.run(k)
    env.fold_cross()
    want = []
    for mk in range(NM):
        h = hist[:, mk * A:(mk + 1) * A]
        went = np.concatenate([h[:n + m], h[n:n + k]]) if mask[mk] else h
        cut, uncut = (XM.table(XM.fold(went, spans, A, cuts=c)) for c in ([n + m], []))
        assert not mask[mk] or (cut != uncut).any(), f"the cut shows in market {mk}"
        assert (cut["n"] > 0).all(), cut["n"]
        want.append(cut if mask[mk] else uncut)
    same(env.cross(), np.array(want, dtype=XM.CROSS_DTYPE), f"reset_markets ({kind})")
    P.no_flags(env)
    env.close()


# ------------------------------------------------------------------------------------------------ 6. clears, the view
@pytest.mark.parametrize("kind", ["host", "device"])
def test_a_masked_clear_per_market_folds_first_and_the_view_is_the_table_in_place(bk, oracle, kind):
    import torch

    NM, A, spans, T = 3, 2, (1, 4), 16
    hist = ref_hist(oracle, NM, A, T)
    env = market_env(bk, NM, A, T, spans, kind="device")
    view = torch.as_tensor(env.cross_view(), device="cuda")
    assert tuple(view.shape) == (NM, 2, A, A, 8) and view.dtype == torch.int64 and view.data_ptr() == env.cross_device_ptr()
    env.run(10, sync=False)  # (not folded: the masked clear folds the ten steps first)
    mask = np.array([1, 0, 1], dtype=bool)
    if kind == "device":
        env.clear_cross(torch.tensor(mask, device="cuda"), sync=False)
    else:
        env.clear_cross(mask)
    now = env.cross()
    same(now[mask], cleared(2, spans, A), "the masked markets are cleared")
    same(now[~mask], model(hist[:10], spans, A, ("run", NM, 10))[~mask], "the others hold the ten steps")
    env.run(6, sync=False)
    env.fold_cross(sync=True)
    want = model(hist, spans, A, ("run", NM, T))
    restarted = XM.rows(hist[10:], spans, A, first_step=10)  # (their carry was cleared too: step 10 has no past)
    kept_n = want["n"] - model(hist[:10], spans, A, ("run", NM, 10))["n"]  # what cleared rows behind a KEPT carry would count
    assert (restarted["n"][mask] < kept_n[mask]).any(), "an empty carry shows in the masked markets' rows"
    assert (restarted[mask]["n"][:, 0] > 0).all()
    want[mask] = restarted[mask]
    same(env.cross(), want, f"after the masked clear ({kind})")
    # the tensor made before any step sees the latest fold without a new call
    seen = np.ascontiguousarray(view.cpu().numpy()).view(XM.CROSS_DTYPE).reshape(want.shape)
    same(seen, want, "the view as a zero-copy tensor")
    with pytest.raises(ValueError):
        env.clear_cross(np.ones(NM * A, dtype=bool))  # (one entry per MARKET, not per book)
    with pytest.raises(ValueError):
        env.clear_cross(torch.ones(NM * A, dtype=torch.bool, device="cuda"))
    P.no_flags(env)
    P.same_history(env.history(), hist)
    env.close()


# ------------------------------------------------------------------------------------------------ 7. lost steps
def test_lost_steps_refuse_fold_clear_and_reset_and_a_full_clear_recovers(bk, oracle):
    NM, A, spans = 3, 2, (1, 2)
    hist = ref_hist(oracle, NM, A, 16)
    env = market_env(bk, NM, A, 8, spans)
    env.enable_lags(4)
    env.enable_series()
    env.run(3)
    env.save_snapshot()
    for fold in (env.fold_cross, env.fold_lags, env.fold_series):
        fold()
    before = env.cross()
    same(before, model(hist[:3], spans, A, ("run", NM, 3)), "three steps")
    assert (before["n"][:, 0] > 0).any()
    # steps 3 .. 11 into a ring of 8: step 3 is gone for the cross table; the siblings fold at step 8 and lose nothing, so
    # that a reset is refused for the cross table's lost step alone - with four steps of theirs outstanding
    env.run(5)
    env.fold_lags()
    env.fold_series()
    lags_before, series_before = env.lags(), env.series()
    assert (series_before["n_steps"] == 8).all()
    env.run(4)
    mask = np.array([1, 0, 0], dtype=bool)
    for _ in range(2):  # (twice: a refusal leaves the cursor too)
        lost(bk, env.fold_cross, 1)
        lost(bk, lambda: env.clear_cross(mask), 1)
        lost(bk, lambda: env.reset_markets(mask), 1)
        same(env.cross(), before, "a refusal leaves the table")
    # ... and a refused reset has folded nothing into the other tables - every table is checked before any launches - nor
    # touched the books
    assert (env.lags() == lags_before).all() and (env.series() == series_before).all()
    assert env.steps_done() == 12
    P.same_history(env.history(), hist[4:12])
    env.clear_cross()
    same(env.cross(), cleared(NM, spans, A), "a full clear clears every market")
    env.run(2)
    env.fold_cross()
    want = XM.rows(hist[12:14], spans, A, first_step=12)  # (the carry was cleared too: step 12 has no past)
    assert not want["n"][:, 1].any() and not want["n_lead"].any() and (want["n"][:, 0] <= 1).all()
    same(env.cross(), want, "counted from the clear on")
    # the same through clear_history(): the two steps run since the last fold are no longer retained
    env.run(2)
    env.clear_history()
    lost(bk, env.fold_cross, 2)
    same(env.cross(), want, "a refused fold leaves the table (clear_history)")
    env.clear_cross()
    env.run(1)
    env.fold_cross(sync=True)
    P.no_flags(env)
    env.close()


# ------------------------------------------------------------------------------------------------ 8. the device ingress
def test_ingress_folded_after_every_step_equals_one_fold_at_the_end(bk, oracle):
    """a two-asset market env with the device ingress, its RandomMarketAgents queued by update_market_agents(): a fold
    behind EVERY step takes the carry path every time; a twin folds once at the end"""
    import torch

    NM, A, spans, T = 5, 2, (1, 3), 20
    groups = groups_of(A)
    na = sum(g[1] for g in groups)
    envs = []
    for _ in range(2):
        e = bk.ManyMarketEnv(NM, SEED, 0, [2] * A, STEP, levels=LEVELS, max_live_orders=pool_of(A), max_orders=na * T + 16, trade_capacity=2 * (na * T + 16),
                             history_capacity=T, stream=torch.cuda.current_stream().cuda_stream)
        e.enable_device_ingress(queue_capacity=na)
        e.set_random_market_agents(groups)
        e.enable_cross(spans)
        envs.append(e)
    env, twin = envs
    hist = ref_hist(oracle, NM, A, T)  # (ManyMarkets.run is update + step, T times)
    for s in range(T):
        for e in envs:
            e.update_market_agents(sync=False)
            e.step(sync=False)
        env.fold_cross()
        if s == 5:
            mid = env.cross()
    twin.fold_cross()
    want = XM.rows(hist, spans, A)
    assert (want["n"] > 0).all() and (want["n_lead"] > 0).all(), (want["n"], want["n_lead"])
    same(mid, XM.rows(hist[:6], spans, A), "after step 5")
    same(env.cross(), want, "folded after every step")
    same(twin.cross(), want, "folded once")
    for e in envs:
        P.no_flags(e)
        P.same_history(e.history(), hist)
        e.close()


# ------------------------------------------------------------------------------------------------ 9. restore, run_series
def test_restore_clears_rows_and_carry_and_the_step_count_goes_on(bk, oracle):
    NM, A, spans = 3, 2, (1, 3)
    hist = ref_hist(oracle, NM, A, 16)
    env = market_env(bk, NM, A, 16, spans)
    env.run(6)
    env.fold_cross()
    ck = env.checkpoint()
    env.run(4)  # (outstanding when the checkpoint comes back: forgotten, not folded)
    env.restore(ck)
    assert env.steps_done() == 6
    same(env.cross(), cleared(NM, spans, A), "restore clears every market")
    env.run(10)
    env.fold_cross()
    want = XM.rows(hist[6:16], spans, A, first_step=6)
    assert (want["n"] < model(hist, spans, A, ("run", NM, 16))["n"]).all() and (want["n"][:, 0] > 0).all(), "step 6 has no past"
    same(env.cross(), want, "counted from the restored step on, with no past")
    P.no_flags(env)
    env.close()


@pytest.mark.parametrize("alone", [False, True], ids=["beside_the_series", "the_only_table"])
def test_run_series_folds_the_table_in_chunks_of_seven(bk, oracle, alone):
    NM, A, spans, T = 3, 2, (1, 5), 40
    hist = ref_hist(oracle, NM, A, T)
    env = market_env(bk, NM, A, 16, spans)
    if not alone:
        env.enable_series()
    env.run_series(T, chunk=7)
    assert env.steps_done() == T
    env.sync()
    P.no_flags(env)
    want = model(hist, spans, A, ("run", NM, T))
    assert (want["n"] > 0).all() and (want["n_lead"] > 0).all()
    same(env.cross(), want, "run_series(40, chunk=7) on a ring of 16")
    if not alone:
        got, ser = env.series(), SM.rows(hist)
        for f in SM.FIELDS:
            P.same_array(got[f], ser[f], "the series beside it", f"series word {f}")
    P.same_history(env.history(), hist[T - 16:])
    env.close()


# ------------------------------------------------------------------------------------------------ 10. refusals
def test_refusals_leave_the_env_working(bk, oracle):
    NM, A, spans = 2, 2, (1, 2)
    env = market_env(bk, NM, A, 8)
    calls = (env.fold_cross, env.cross, lambda: env.cross(0, 1), env.cross_device_ptr, env.cross_view, env.cross_config, env.clear_cross,
             lambda: env.clear_cross(np.ones(NM, dtype=bool)))
    for call in calls:
        refused(bk, call, NO_TABLE)
    for rc in (env._L.bk_cross_fold(env._h), env._L.bk_cross_clear_device(env._h, None), env._L.bk_get_cross(env._h, 0, 1, None),
               env._L.bk_cross_device_ptr(env._h, None), env._L.bk_cross_config_get(env._h, None)):
        assert rc == 5 and b"no cross table" in env._L.bk_last_error()
    env.run(2)
    for bad, why in (((), r"n_spans must be in 1\.\.4"), ((1, 2, 3, 4, 5), r"n_spans must be in 1\.\.4"), ((0,), r"span must be in 1\.\.64"),
                     ((1, 65), r"span must be in 1\.\.64"), ((3, 1, 1 << 20), r"span must be in 1\.\.64")):
        refused(bk, lambda: env.enable_cross(bad), why)
        refused(bk, env.fold_cross, NO_TABLE)  # (a refused enable left the env without the table)
    with pytest.raises(ValueError):
        env.enable_cross((1 << 32,))
    assert env._L.bk_cross_enable(env._h, None) == 5 and b"null argument" in env._L.bk_last_error()
    env.enable_cross(spans)
    refused(bk, lambda: env.enable_cross(spans), "already enabled")
    refused(bk, lambda: env.enable_cross((3,)), "already enabled")
    assert env.cross().shape == (NM, 2, A, A) and env.cross_config()["spans"].tolist() == [1, 2, 0, 0]
    # a null out-pointer and a market range past the end: refused, the table as it was
    for rc in (env._L.bk_cross_device_ptr(env._h, None), env._L.bk_get_cross(env._h, 0, 2, None), env._L.bk_cross_config_get(env._h, None)):
        assert rc == 5 and b"null argument" in env._L.bk_last_error()
    for first, n in ((1, 2), (3, 0), (0, 3)):
        refused(bk, lambda: env.cross(first, n), "market range out of bounds")
    assert env.cross(2, 0).shape == (0, 2, A, A) and env.cross(1).shape == (1, 2, A, A)
    with pytest.raises(ValueError):
        env.cross(-1, 1)
    with pytest.raises(ValueError):
        env.clear_cross(np.ones(NM + 1, dtype=bool))
    same(env.cross(), cleared(NM, spans, A), "refusals leave the rows")
    env.run(3)
    env.fold_cross()
    hist = ref_hist(oracle, NM, A, 16)
    same(env.cross(), XM.rows(hist[2:5], spans, A, first_step=2), "steps before the enable are not counted")
    P.no_flags(env)
    env.close()
    cfg = np.array([1, 1, 0, 0, 0], dtype=np.uint32)
    # an env of independent books, a market env of one asset, an env without a ring: refused, and they go on running
    books = bk.ManyBookEnv(4, SEED, 0, 2, STEP, True, levels=LEVELS, max_live_orders=64, trade_capacity=4096, history_capacity=8)
    books.set_random_agents([(24, (40, 56), (10, 20), 2, 0.8)])
    one = bk.ManyMarketEnv(2, SEED, 0, [2], STEP, True, levels=LEVELS, max_live_orders=64, trade_capacity=4096, history_capacity=8)
    one.set_random_market_agents([(0, 24, (40, 56), (10, 20), 2, 0.8)])
    for e in (books, one):
        assert e._L.bk_cross_enable(e._h, cfg.ctypes.data) == 5
        msg = e._L.bk_last_error()
        assert b"assets >= 2" in msg and b"independent books" in msg, msg
        assert e._L.bk_cross_fold(e._h) == 5 and b"no cross table" in e._L.bk_last_error()
        e.run(2)
        P.no_flags(e)
    refused(bk, lambda: one.enable_cross((1,)), "assets >= 2")
    books.close()
    one.close()
    none = market_env(bk, NM, A, 0)
    refused(bk, lambda: none.enable_cross(spans), "history_capacity must be > 0")
    none.run(2)
    none.close()


# ------------------------------------------------------------------------------------------------ 11. extremes
def test_jumps_between_the_ends_of_the_price_range_in_both_assets(bk, oracle):
    """a host-driven market of two assets, tick 1: twice the mid jumps between 3 and 2^33 - 5 - asset 0 up, down, up, down,
    asset 1 up, stays, down, up - so x = +-(2^33 - 8) or 0, and x * x, x * y pass 2^64 with both signs"""
    A, spans = 2, (1, 2)
    ups = {0: (1, 3), 1: (1, 4)}  # the steps at which the asset jumps up ...
    downs = {0: (2, 4), 1: (3,)}  # ... and down
    env = bk.ManyMarketEnv(1, SEED, 0, [1, 1], 1000, True, levels=5, max_live_orders=16, max_orders=32, trade_capacity=16, history_capacity=8)
    env.enable_cross(spans)
    ref = oracle.ManyMarkets(1, SEED, 0, [1, 1], 1000, True, 5)

    def place(a, bid, vol, trader, price):
        ref.place_order(0, a, bid, vol, trader, price=price)
        env.place_order(0, a, bid, vol, trader, price)

    for s in range(5):
        for a in range(A):
            if s == 0:
                place(a, True, 50, 1, 1)
                place(a, False, 50, 2, 0xFFFFFFFE)
                place(a, False, 1, 2, 2)
            elif s in ups[a]:
                place(a, True, 1, 3, 0xFFFFFFFD)
                place(a, True, 1, 3, 0xFFFFFFFD)
            elif s in downs[a]:
                place(a, False, 1, 4, 2)
                place(a, False, 1, 4, 2)
        env.step()
        ref.step()
    ref_hist_ = ref.history()
    big, a_ = (1 << 33) - 5, (1 << 33) - 8
    assert (ref_hist_[:, 0, 1].astype(np.int64) + ref_hist_[:, 0, 2].astype(np.int64)).tolist() == [3, big, 3, big, 3]
    assert (ref_hist_[:, 1, 1].astype(np.int64) + ref_hist_[:, 1, 2].astype(np.int64)).tolist() == [3, big, big, 3, big]
    exact = XM.fold(ref_hist_, spans, A)["rows"]
    # span 1: x_0 = +a, -a, +a, -a; x_1 = +a, 0, -a, +a
    assert exact[0][0][0]["sum_xx"] == 4 * a_ * a_ and exact[0][0][0]["sum_xx"] >> 64 and exact[0][0][1]["sum_xy"] == -a_ * a_
    assert exact[0][0][1]["sum_xy"] < -(1 << 64) and exact[0][0][1]["sum_lead"] == 0 and exact[0][1][0]["sum_lead"] == 2 * a_ * a_
    u = lambda x: x & M64  # noqa: E731
    sq = u(4 * a_ * a_)
    assert XM.words(XM.fold(ref_hist_, spans, A))[0][0][0] == [4, 0, 0, sq, sq, sq, 3, u(-3 * a_ * a_)], "row (span 1, 0, 0) by hand"
    want = XM.rows(ref_hist_, spans, A)
    env.fold_cross(sync=True)
    P.no_flags(env)
    P.same_history(env.history(), ref_hist_)
    same(env.cross(), want, "jumps of 2^33 - 8 in both assets")
    env.close()
