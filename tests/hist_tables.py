"""What the GPU tests of the three tables folded from the level-2 history ring share (tests/test_gpu_hist_tables.py and
tests/test_gpu_{series,lags,bins}.py): the helpers each of them used to type for itself, and one adapter per table - how
to enable it with a configuration, fold, read, clear and view it, its plain-Python model, its all-clear table, its exact
comparison, the noun its lost steps are reported under, and per scenario the shape it is enabled with today and what must
hold of the EXPECTED table before anything is compared (a table that is trivially empty proves nothing)."""
import numpy as np
import pytest

import bins_model as BM
import lags_model as LM
import oracle_parity as P
import series_model as SM
from test_gpu_reset_books import C2, STEP, make_env, ref_books

MAXU = 0xFFFFFFFF
SEED = 101


@pytest.fixture(scope="module")
def bk():
    import bourse_amd

    return bourse_amd


def refused(bk, call, match):
    with pytest.raises(bk.BourseError, match=match) as e:
        call()
    assert e.value.code == 5


def lost(bk, T, call, n):
    refused(bk, call, rf"\b{n} step\(s\) of the {T.noun} were lost")


def run_env(bk, T, B, cap, cfg=None, groups=C2, members=None, **kw):
    """an env of test_gpu_reset_books' shape (levels 16, pool 64) with table T on"""
    return T.enable(make_env(bk, B, groups=None if members else groups, members=members, steps=cap, **kw), cfg)


def host_driven(bk, oracle, B, cap, enables, steps, tick=1, step_size=STEP, max_orders=32):
    """B books driven by place / cancel calls, the same for every book unless an op names its book, beside one oracle env
    per book - one device env per callable of ``enables``, which turns that env's table on; returns (envs, refs) with
    nothing folded"""
    envs = [bk.ManyBookEnv(B, SEED, 0, tick, step_size, levels=5, max_live_orders=16, max_orders=max_orders, trade_capacity=16,
                           history_capacity=cap) for _ in enables]
    for env, on in zip(envs, enables):
        on(env)
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


def reset_by(env, mask, kind):
    """reset_books through a host mask, or through a torch CUDA mask without a synchronisation"""
    if kind == "device":
        import torch

        env.reset_books(torch.tensor(mask, device="cuda"), sync=False)
    else:
        env.reset_books(mask)


def clear_by(T, env, mask, kind):
    if kind == "device":
        import torch

        T.clear(env, torch.tensor(mask, device="cuda"), sync=False)
    else:
        T.clear(env, mask)


def same_as_series(lag_rows, series_rows, tag):
    """a lag table's row 0 and the series row over the same steps and cuts"""
    for a, b in (("n_pairs", "n_pairs"), ("sum_dd", "sum_dd"), ("sum_abs_dd", "sum_abs_dd"), ("n_h", "n_ret"), ("sum_h", "sum_d"),
                 ("sum_abs_h", "sum_abs_d"), ("sum_h2", "sum_d2"), ("sum_h4_lo", "sum_d4_lo"), ("sum_h4_hi", "sum_d4_hi"),
                 ("max_abs_h", "max_abs_d")):
        P.same_array(lag_rows[:, 0][a], series_rows[b].astype(lag_rows[a].dtype), tag, f"row 0's {a} against the series' {b}")


class Table:
    """the calls every adapter answers the same way, by the table's name"""
    _want = {}

    def fold(self, env, **kw):
        return getattr(env, f"fold_{self.name}")(**kw)

    def read(self, env, *a):
        return getattr(env, self.name)(*a)

    def clear(self, env, *a, **kw):
        return getattr(env, f"clear_{self.name}")(*a, **kw)

    def view(self, env):
        return getattr(env, f"{self.name}_view")()

    def device_ptr(self, env):
        return getattr(env, f"{self.name}_device_ptr")()

    def calls(self, env):
        """every call that needs the table"""
        return (lambda: self.fold(env), lambda: self.read(env), lambda: self.device_ptr(env), lambda: self.view(env),
                lambda: self.clear(env), lambda: self.clear(env, np.ones(2, dtype=bool)))

    def model(self, hist, cfg, key, **kw):
        """rows() over the oracle's history, computed once per (run, configuration, range) and shared"""
        key = (self.name, repr(cfg)) + key
        if key not in Table._want:
            Table._want[key] = self.rows(hist, cfg, **kw)
        return Table._want[key].copy()

    def stack(self, tables):
        return np.array(tables, dtype=self.dtype)

    def beside(self, env):  # the siblings the three-part run keeps on the same env, and what must hold between them
        pass

    def fold_beside(self, env):
        pass

    def identities(self, env, final, hist, cfg):
        pass

    def __repr__(self):
        return self.name


class Series(Table):
    name, noun, dtype = "series", "series", SM.SERIES_DTYPE
    no_table, loading = "no series moments: call bk_series_enable first", "series moments"
    # the shape each shared scenario enables the table with (the series has none)
    cfg = dict(lost=None, reset=None, ingress_reset=None, clear=None, restore=None, refusals=None, members=None, markets=None,
               ingress=None)
    deepest = None  # the configuration the three-part run's expected table is judged at

    def enable(self, env, cfg=None):
        env.enable_series()
        return env

    def rows(self, hist, cfg=None, **kw):
        return SM.rows(hist, **kw)

    def fold_model(self, h, cfg=None, **kw):
        return SM.fold(h, **kw)

    def table(self, s):
        return SM.row(s)

    def cleared(self, B, cfg=None):
        return np.array([SM.row(SM.cleared())] * B, dtype=SM.SERIES_DTYPE)

    def same(self, got, want, tag):
        assert got.dtype == want.dtype == SM.SERIES_DTYPE, (got.dtype, want.dtype)
        assert got.shape == want.shape, f"{tag}: rows {got.shape} vs {want.shape}"
        for f in SM.FIELDS:
            P.same_array(got[f], want[f], tag, f"series word {f}")

    def view_shape(self, B, cfg):
        return (B, 24)

    def at_reset(self, hist, mask, cfg):
        """the table right behind a reset that folded hist: the sums go on, the masked books' carry is cut"""
        states = [SM.fold(hist[:, b]) for b in range(hist.shape[1])]
        return self.stack([SM.row(SM.cut(s) if mask[b] else s) for b, s in enumerate(states)])

    def busy(self, case, want, cfg=None, mask=None, uncut=None, total=None, hist=None, got=None):
        if case == "three_parts":
            assert (want["n_two_sided"] < want["n_steps"]).any() and (want["n_pairs"] > 0).all(), want[["n_steps", "n_two_sided", "n_pairs"]]
            d = np.diff(hist[:, :, 1].astype(np.int64) + hist[:, :, 2].astype(np.int64), axis=0)
            both = (hist[1:, :, 1] != 0) & (hist[:-1, :, 1] != 0) & (hist[1:, :, 2] != MAXU) & (hist[:-1, :, 2] != MAXU)
            assert (d[both] > 0).any() and (d[both] < 0).any()
        elif case == "members":
            assert (want["n_ret"] > 0).all()
        elif case == "markets":
            assert want.shape == (6,) and (want["n_two_sided"] > 0).all() and len({tuple(r.tolist()) for r in want}) == 6
        elif case == "ingress":
            assert (want["n_pairs"] > 0).all() and (want["n_trade_steps"] > 0).all()
        elif case == "at_reset":  # the device's rows: the two carry words of the masked books are zero
            assert not got["carry_m"][mask].any() and not got["carry_d"][mask].any() and got["carry_m"][~mask].any()
        elif case == "reset":
            assert (want["n_steps"] == total).all() and (want["n_ret"][mask] > 0).all()
        elif case == "ingress_reset":
            assert (want["n_steps"] == 8).all() and (want["n_two_sided"] > 4).all()

    def bad_enables(self, bk, env):
        pass

    def enabled(self, bk, env, cfg):
        refused(bk, lambda: self.enable(env), "already enabled")

    def one_sided(self, host, cfg):
        assert host.series()["n_steps"].tolist() == [1, 1] and host.series()["sum_bid_vol"].tolist() == [5, 5]


class Lags(Table):
    name, noun, dtype = "lags", "lag table", LM.LAG_DTYPE
    no_table, loading = "no lag table: call .*bk_lags_enable.* first", "lag table"
    cfg = dict(lost=4, reset=4, ingress_reset=3, clear=4, restore=4, refusals=2, members=16, markets=8, ingress=6)
    deepest = 64

    def enable(self, env, K):
        env.enable_lags(K)
        return env

    def rows(self, hist, K, **kw):
        return LM.rows(hist, K, **kw)

    def fold_model(self, h, K=None, **kw):
        return LM.fold(h, **kw) if "into" in kw else LM.fold(h, K, **kw)

    def table(self, s):
        return LM.table(s)

    def cleared(self, B, K):
        return np.zeros((B, K), dtype=LM.LAG_DTYPE)

    def same(self, got, want, tag):
        assert got.dtype == want.dtype == LM.LAG_DTYPE, (got.dtype, want.dtype)
        assert got.shape == want.shape, f"{tag}: rows {got.shape} vs {want.shape}"
        for f in LM.FIELDS:
            P.same_array(got[f], want[f], tag, f"lag word {f}")

    def view_shape(self, B, K):
        return (B, K, 10)

    def at_reset(self, hist, mask, K):
        return LM.rows(hist, K)  # (a cut leaves the rows)

    def busy(self, case, want, K=None, mask=None, uncut=None, total=None, hist=None, got=None):
        if case == "three_parts":  # (want: the model at K = 64)
            two = (hist[:, :, 1] != 0) & (hist[:, :, 2] != MAXU)
            assert ((~two).sum(axis=0) >= 1).all(), "every book has a one-sided step"
            assert (want[:, 63]["n_pairs"] > 0).all(), want[:, 63]["n_pairs"]
            d = np.diff(hist[:, :, 1].astype(np.int64) + hist[:, :, 2].astype(np.int64), axis=0)
            r = two[1:] & two[:-1]
            for k in (1, 64):
                assert ((d[k:] * d[:-k])[r[k:] & r[:-k]] < 0).any(), f"a negative product at lag {k}"
        elif case in ("members", "ingress"):
            assert (want[:, K - 1]["n_h"] > 0).all() and (want[:, 0]["n_pairs"] > 0).all()
        elif case == "markets":
            assert want.shape == (6, K) and (want[:, 0]["n_h"] > 0).all() and len({tuple(r.tolist()) for r in want[:, 0]}) == 6
        elif case == "lost":  # two steps behind a full clear: step 12 has no past
            assert (want[:, 0]["n_h"] <= 1).all() and not want[:, 1:]["n_h"].any()
        elif case == "reset":
            assert any((u != w).any() for u, w in zip(uncut, want[mask])), "the cut shows in the masked books' rows"
            assert (want[mask][:, 0]["n_h"] > 0).all()
        elif case == "ingress_reset":
            assert (want[:, 0]["n_h"] > 3).all()

    def beside(self, env):
        env.enable_series()

    def fold_beside(self, env):
        env.fold_series()  # (a cursor of its own: the series must not fall out of the ring either)

    def identities(self, env, final, hist, K):
        same_as_series(env.lags(), env.series(), "three folds")
        same_as_series(final, SM.rows(hist), "the models")

    def bad_enables(self, bk, env):
        for n in (0, 65, 1 << 20):
            refused(bk, lambda: env.enable_lags(n), r"n_lags must be in 1\.\.64")
        refused(bk, env.fold_lags, "no lag table")  # (a refused enable left the env without the table)

    def enabled(self, bk, env, K):
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
        self.same(env.lags(), self.cleared(2, K), "refusals leave the rows")

    def one_sided(self, host, K):
        self.same(host.lags(), self.cleared(2, K), "one-sided books add nothing")


class Bins(Table):
    name, noun, dtype = "bins", "bin table", np.uint64
    no_table, loading = "no bin table: call .*bk_bins_enable.* first", "bin table"
    cfg = dict(lost=BM.config((1, 4), 64), reset=BM.config((1, 4), 64), ingress_reset=BM.config((1, 3), 32, 2, 2, 5),
               clear=BM.config((1, 4), 64), restore=BM.config((1, 4), 64), refusals=BM.config((1, 2), 8),
               members=BM.config((1, 16), 64, 2, 2, 50), markets=BM.config((1, 8), 32, 2, 2, 10), ingress=BM.config((1, 6, 2), 32, 2, 2, 5))
    deepest = BM.config((1, 5, 64), 64)

    def enable(self, env, cfg):
        env.enable_bins(cfg["spans"], cfg["n_bins"], cfg["ret_width"], cfg["spread_width"], cfg["vol_width"])
        return env

    def rows(self, hist, cfg, **kw):
        return BM.rows(hist, cfg, **kw)

    def fold_model(self, h, cfg=None, **kw):
        return BM.fold(h, **kw) if "into" in kw else BM.fold(h, cfg, **kw)

    def table(self, s):
        return BM.table(s)

    def cleared(self, B, cfg):
        return np.zeros((B, len(cfg["spans"]) + 2, cfg["n_bins"]), dtype=np.uint64)

    def same(self, got, want, tag):
        assert got.dtype == want.dtype == np.uint64, (got.dtype, want.dtype)
        assert got.shape == want.shape, f"{tag}: table {got.shape} vs {want.shape}"
        for c in range(want.shape[1]):
            P.same_array(got[:, c], want[:, c], tag, f"bin counts of channel {c}")

    def view_shape(self, B, cfg):
        return (B, len(cfg["spans"]) + 2, cfg["n_bins"])

    def at_reset(self, hist, mask, cfg):
        return BM.rows(hist, cfg)  # (a cut leaves the counts)

    def busy(self, case, want, cfg=None, mask=None, uncut=None, total=None, hist=None, got=None):
        if case == "three_parts":
            two = (hist[:, :, 1] != 0) & (hist[:, :, 2] != MAXU)
            assert ((~two).sum(axis=0) >= 1).all(), "every book has a one-sided step"
            assert (want[:, 2].sum(axis=1) > 0).all() and (want[:, 4, 1:].sum(axis=1) > 0).all(), "span 64 counts, steps trade"
        elif case == "members":
            assert (want[:, 1].sum(axis=1) > 0).all() and (want[:, 3, 1:].sum(axis=1) > 0).all()
        elif case == "markets":
            assert want.shape == (6, 4, 32) and (want[:, 0].sum(axis=1) > 0).all() and len({w.tobytes() for w in want}) == 6
        elif case == "ingress":
            assert (want[:, 1].sum(axis=1) > 0).all() and (want[:, 4, 1:].sum(axis=1) > 0).all()
        elif case == "lost":  # two steps behind a full clear: step 12 has no past
            assert (want[:, 0].sum(axis=1) <= 1).all() and not want[:, 1].any() and (want[:, 3].sum(axis=1) == 2).all()
        elif case == "reset":
            assert any((u != w).any() for u, w in zip(uncut, want[mask])), "the cut shows in the masked books' counts"
            assert (want[mask][:, 0].sum(axis=1) > 0).all()
        elif case == "ingress_reset":
            assert (want[:, 0].sum(axis=1) > 3).all() and (want[:, 3].sum(axis=1) == 8).all()
        elif case == "clear":  # the masked books start again at step 10: fewer returns over span 4 than any other book
            assert (want[mask][:, 1].sum(axis=1) < want[~mask][:, 1].sum(axis=1).min()).all()

    def beside(self, env):
        env.enable_series()
        env.enable_lags(64)

    def fold_beside(self, env):
        env.fold_series()  # (cursors of their own: the siblings must not fall out of the ring either)
        env.fold_lags()

    def identities(self, env, final, hist, cfg):
        """the totals are the lag table's n_h at each span, the series' n_two_sided and n_steps"""
        got, lag, ser = env.bins(), env.lags(), env.series()
        for j, k in enumerate(cfg["spans"]):
            P.same_array(got[:, j].sum(axis=1), lag[:, k - 1]["n_h"], "totals", f"channel {j} against the lag table's n_h at span {k}")
            for b in range(got.shape[0]):
                if not got[b, j, 0] and not got[b, j, -1]:  # nothing clamped at ret_width 1: the first moment is sum_h
                    first = sum((i - 32) * int(c) for i, c in enumerate(got[b, j]))
                    assert first == int(lag[b, k - 1]["sum_h"]), (b, k)
        P.same_array(got[:, 3].sum(axis=1), ser["n_two_sided"], "totals", "the spread channel against the series' n_two_sided")
        P.same_array(got[:, 4].sum(axis=1), ser["n_steps"], "totals", "the volume channel against the series' n_steps")
        assert (ser["n_steps"] == hist.shape[0]).all()

    def calls(self, env):
        return super().calls(env) + (env.bins_config,)

    def bad_enables(self, bk, env):
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

    def enabled(self, bk, env, cfg):
        refused(bk, lambda: self.enable(env, cfg), "already enabled")
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
        self.same(env.bins(), self.cleared(2, cfg), "refusals leave the table")

    def one_sided(self, host, cfg):
        want = self.cleared(2, cfg)
        want[:, 3, 0] = 1
        self.same(host.bins(), want, "one-sided books count in the volume channel only")


SERIES, LAGS, BINS = Series(), Lags(), Bins()
TABLES = (SERIES, LAGS, BINS)


# ------------------------------------------------------------------------------------------------ scenarios run from the tables' files
# (under the ids they always had there: tests/test_gpu_{series,lags,bins}.py parametrise them)
def run_folded_in_three_parts(bk, oracle, T, cfg, pipeline):
    """5 books (the last block of four waves holds one), a ring of 96: run(70) and fold - more than one step a lane, two
    chunks of the lag window - run(26) and fold - the ring at its last slots - run(40) and fold - the ring wrapped.  A twin
    with a ring of 136 folds once.  The bin table runs with the lag table at K = 64 and the series on the same env, the lag
    table with the series: cursors of their own, and identities between the tables.  The same under every pipeline: the
    fold does not depend on who wrote the ring."""
    B, cap, parts = 5, 96, (70, 26, 40)
    total = sum(parts)
    hist = ref_books(oracle, B, 16, total, groups=C2).history()
    deepest = T.deepest
    T.busy("three_parts", T.model(hist, deepest, ("run", total)), deepest, hist=hist)
    env, twin = run_env(bk, T, B, cap, cfg), run_env(bk, T, B, total, cfg)
    T.beside(env)
    if pipeline:
        env.set_pipeline(pipeline)
        twin.set_pipeline(pipeline)
    done = 0
    for n in parts:
        env.run(n, sync=False)
        twin.run(n, sync=False)
        T.fold(env)
        T.fold_beside(env)
        done += n
        T.same(T.read(env), T.model(hist[:done], cfg, ("run", done)), f"after {done} steps ({pipeline}, {cfg})")
    T.fold(twin)
    final = T.model(hist, cfg, ("run", total))
    T.same(T.read(twin), final, "one fold of 136 steps")
    T.same(T.read(env), final, "three folds against one pass of the model")
    T.identities(env, final, hist, cfg)
    for e in (env, twin):
        P.no_flags(e)
    P.same_history(env.history(), hist[done - cap:])
    P.same_history(twin.history(), hist)
    env.close()
    twin.close()


def reset_books_cuts_the_carry(bk, oracle, T, kind):
    """6 steps, save, fold; 5 steps NOT folded; reset books 0, 2, 4 - which folds the five first - then 7 steps.  A reset
    book replays steps 6 .. 12 of the same seed: its table is the oracle's steps 0 .. 10, a cut, steps 6 .. 12.  The sums
    and counts go on; no return, span or pair reaches over the reset."""
    B, n, m, k, cfg = 5, 6, 5, 7, T.cfg["reset"]
    hist = ref_books(oracle, B, 16, n + m + k, groups=C2).history()
    env = run_env(bk, T, B, n + m + k, cfg, kind=kind)
    env.run(n)
    env.save_snapshot()
    T.fold(env)
    env.run(m)
    mask = np.array([1, 0, 1, 0, 1], dtype=bool)
    reset_by(env, mask, kind)
    at_reset = T.read(env)
    T.same(at_reset, T.at_reset(hist[:n + m], mask, cfg), "the reset folded the five steps and cut the masked carries")
    T.busy("at_reset", None, cfg, mask=mask, got=at_reset)
    env.run(k)
    T.fold(env)
    want, uncut = [], []
    for b in range(B):
        if mask[b]:
            s = T.fold_model(hist[n:n + k, b], cuts=[n + m], first_step=n + m, into=T.fold_model(hist[:n + m, b], cfg))
            uncut.append(T.table(T.fold_model(hist[n:n + k, b], first_step=n + m, into=T.fold_model(hist[:n + m, b], cfg))))
        else:
            s = T.fold_model(hist[:, b], cfg)
        want.append(T.table(s))
    want = T.stack(want)
    T.busy("reset", want, cfg, mask=mask, uncut=uncut, total=n + m + k)
    T.same(T.read(env), want, f"reset_books ({kind})")
    P.no_flags(env)
    env.close()


def masked_clear_folds_first(bk, oracle, T, kind):
    import torch

    B, cfg = 5, T.cfg["clear"]
    hist = ref_books(oracle, B, 16, 16, groups=C2).history()
    env = run_env(bk, T, B, 16, cfg, kind="device")
    view = torch.as_tensor(T.view(env), device="cuda")
    assert tuple(view.shape) == T.view_shape(B, cfg) and view.dtype == torch.int64 and view.data_ptr() == T.device_ptr(env)
    env.run(10, sync=False)  # (not folded: the masked clear folds the ten steps first)
    mask = np.array([1, 0, 1, 0, 0], dtype=bool)
    clear_by(T, env, mask, kind)
    now = T.read(env)
    T.same(now[mask], T.cleared(2, cfg), "the masked books are cleared, carry included")
    T.same(now[~mask], T.rows(hist[:10], cfg)[~mask], "the others hold the ten steps")
    env.run(6, sync=False)
    T.fold(env, sync=True)
    want = T.rows(hist, cfg)
    want[mask] = T.rows(hist[10:], cfg, first_step=10)[mask]  # (their carry was cleared too: step 10 has no past)
    T.busy("clear", want, cfg, mask=mask)
    T.same(T.read(env), want, f"after the masked clear ({kind})")
    # the tensor made before any step sees the latest fold without a new call
    seen = np.ascontiguousarray(view.cpu().numpy()).view(T.dtype).reshape(want.shape)
    T.same(seen, want, "the view as a zero-copy tensor")
    P.no_flags(env)
    env.close()
