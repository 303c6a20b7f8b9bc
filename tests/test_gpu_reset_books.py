"""Per-book reset to a device-resident snapshot (bk_snapshot_save / bk_reset_books* through ManyBookEnv.save_snapshot /
reset_books and ManyMarketEnv.reset_markets), bit for bit against the CPU oracle.

The scheme: the device env runs n steps, saves a snapshot, runs m steps, resets the masked books and runs k steps.  A book
that was never reset equals the oracle's book after n + m + k steps; a reset book equals the oracle's book after n + k steps
(the same constructor run shorter) in its last k history rows, trade count, RNG state, clock, live orders in priority
order, and its retained trades are the oracle's from the snapshot's count on.  Every book of every env is compared."""
import numpy as np
import pytest

import oracle_parity as P

pytestmark = pytest.mark.gpu

SEED, STEP, TICK = 101, 100_000, 2
C2 = [(32, (40, 56), (10, 20), 2, 0.8), (32, (40, 56), (50, 70), 2, 0.2)]
C3 = [(64, (32, 64), (10, 20), 2, 0.8), (64, (32, 64), (50, 70), 2, 0.2)]
C5 = [(256, (100, 164), (10, 20), 2, 0.8), (256, (100, 164), (50, 70), 2, 0.2)]
# (tests/test_gpu_parity.py's members, restated)
NOISE_P = dict(tick_size=2, p_limit=0.2, p_market=0.2, p_cancel=0.1, trade_vol=100, price_dist_mu=0.0, price_dist_sigma=1.0)
MOM_P = dict(tick_size=2, p_cancel=0.1, trade_vol=100, decay=1.0, demand=5.0, scale=0.5, order_ratio=1.0,
             price_dist_mu=0.0, price_dist_sigma=10.0)
MEMBERS = [("momentum", 0, 10, MOM_P), ("noise", 10, 20, NOISE_P)]
PIPELINES = ("fused", "split", "wave_split", "wave")
MASKS = ("none", "all", "first", "last", "alternate", "third")
FLAG_TRADE_OVERFLOW = 2


@pytest.fixture(scope="module")
def bk():
    import bourse_amd

    return bourse_amd


def make_mask(name, B):
    m = np.zeros(B, dtype=bool)
    if name == "all":
        m[:] = True
    elif name == "first":
        m[0] = True
    elif name == "last":
        m[B - 1] = True
    elif name == "alternate":
        m[::2] = True
    elif name == "third":
        m[np.random.default_rng(5).choice(B, B // 3, replace=False)] = True
    return m


def as_kind(mask, kind, seeds=None):
    """The mask (and seeds) as the host arrays they are, or as torch CUDA tensors written on the current stream."""
    if kind == "host":
        return mask, seeds
    import torch

    # (uint64 seeds travel as their int64 bit patterns: 8-byte elements are what the entry takes)
    return (torch.tensor(mask, device="cuda"),
            None if seeds is None else torch.tensor(np.asarray(seeds, dtype=np.uint64).view(np.int64), device="cuda"))


def make_env(bk, B, groups=None, members=None, levels=16, pool=64, steps=18, seed=SEED, kind="host", tick=TICK, **kw):
    if kind == "device":
        import torch

        kw["stream"] = torch.cuda.current_stream().cuda_stream
    kw.setdefault("trade_capacity", 4096)
    env = bk.ManyBookEnv(B, seed, 0, tick, STEP, True, levels=levels, max_live_orders=pool, history_capacity=steps, **kw)
    if members is not None:
        env.set_agents(members)
    elif groups is not None:
        env.set_random_agents(groups)
    return env


def do_reset(env, mask, kind, seeds=None, slot=0):
    m, s = as_kind(mask, kind, seeds)
    env.reset_books(m, seeds=s, slot=slot, sync=(kind == "host"))


_refs = {}


def ref_books(oracle, B, levels, steps, groups=None, members=None, seed=SEED, tick=TICK):
    """oracle.ManyBooks of this shape after `steps` steps: computed once, shared, never stepped again."""
    key = (B, levels, steps, repr(groups), repr(members), seed, tick)
    if key not in _refs:
        ref = oracle.ManyBooks(B, seed, 0, tick, STEP, True, levels, groups=groups, members=members)
        if steps:
            ref.run(steps, 2)
        _refs[key] = ref
    return _refs[key]


def facts(ref):
    """The oracle's arrays, read once per oracle."""
    if not hasattr(ref, "_facts"):
        ref._facts = {"history": ref.history(), "trade_counts": ref.trade_counts(), "rng": ref.rng_states()}
    return ref._facts


def verify(env, ref_of, lens, tail, snap_len=None, allow_flags=0):
    """Every book b of the env is the oracle's book after lens[b] steps: the last `tail` history rows, trade count, RNG
    state, clock, live orders in priority order and trades.  ref_of(b, L) = (the oracle after L steps, b's index in it).
    snap_len[b] (None / -1: never reset) is the length of the snapshot b was last reset to: b then retains the oracle's
    trades from the count at that length on, and reports that count as its first retained record."""
    P.no_flags(env, allow=allow_flags)
    hist, tc = env.history(), env.trade_counts()
    for b in range(env.n_books):
        L = int(lens[b])
        ref, rb = ref_of(b, L)
        f, view = facts(ref), ref.book(rb)
        was_reset = snap_len is not None and snap_len[b] >= 0
        tag = (b, "reset" if was_reset else "kept")
        P.same_history(hist[len(hist) - tail:, b], f["history"][L - tail:L, rb], tag=f"{tag}: L2 history tail")
        assert int(tc[b]) == int(f["trade_counts"][rb]), tag
        assert env.rng_state(b) == tuple(int(x) for x in f["rng"][rb]), tag
        assert env.time(b) == L * STEP == view.get_time(), tag
        if not was_reset:
            P.same_book(env, b, view, tag=tag)
        else:
            snap_ref, sb = ref_of(b, int(snap_len[b]))
            base = int(facts(snap_ref)["trade_counts"][sb])
            assert env.trade_count(b) == (int(f["trade_counts"][rb]), base), tag
            P.same_records(env.trades(b), view.trades_array()[base:], tag, "retained trade")
            P.same_live(env, b, view, tag)


def same_seed_case(bk, oracle, B, groups, levels, pool, n, m, k, mask_name, kind, pipes=(None, None), members=None):
    mask = make_mask(mask_name, B)
    env = make_env(bk, B, groups=groups, members=members, levels=levels, pool=pool, steps=n + m + k, kind=kind)
    if pipes[0]:
        env.set_pipeline(pipes[0])
    env.run(n)
    env.save_snapshot()
    env.run(m)
    do_reset(env, mask, kind)
    if pipes[1]:
        env.set_pipeline(pipes[1])
    env.run(k)
    assert env.steps_done() == n + m + k
    lens = np.where(mask, n + k, n + m + k)
    verify(env, lambda b, L: (ref_books(oracle, B, levels, L, groups=groups, members=members), b), lens, k,
           snap_len=np.where(mask, n, -1))
    env.close()


# ------------------------------------------------------------------ 1. every mask, both kinds, across the pipelines
@pytest.mark.parametrize("kind", ["host", "device"])
@pytest.mark.parametrize("pipe", range(4))
def test_masked_books_rewind_and_the_others_carry_on(bk, oracle, pipe, kind):
    # the pipeline is switched between the run before and the run after the reset
    pipes = (PIPELINES[pipe], PIPELINES[(pipe + 1) % 4])
    for mask_name in MASKS:
        same_seed_case(bk, oracle, 97, C2, 16, 64, 6, 5, 7, mask_name, kind, pipes)


# ------------------------------------------------------------------ 2. the other pool sizes
@pytest.mark.parametrize("kind", ["host", "device"])
@pytest.mark.parametrize("shape", [(70, "C3", 32, 128, 6, 5, 7), (6, "C5", 64, 512, 4, 3, 4), (21, "C3x2", 10, 256, 5, 4, 5)])
def test_pool_sizes(bk, oracle, shape, kind):
    # R = 2 (3 vectors per lane, W = 133), R = 8 (11 per lane, W = 261) and R = 4 (6 per lane, W = 45)
    B, name, levels, pool, n, m, k = shape
    groups = {"C3": C3, "C5": C5, "C3x2": C3 + C3}[name]
    for mask_name in ("alternate", "all", "last"):
        same_seed_case(bk, oracle, B, groups, levels, pool, n, m, k, mask_name, kind)


# ------------------------------------------------------------------ 3. reseed from the empty book
@pytest.mark.parametrize("kind", ["host", "device"])
def test_reseed_from_the_empty_book(bk, oracle, kind):
    B, S, levels = 97, 9_000_000_019, 16
    mask = make_mask("third", B)
    mask[[0, B - 1]] = True
    seeds = (S + np.arange(B)).astype(np.uint64)
    env = make_env(bk, B, groups=C2, levels=levels, steps=13, kind=kind)
    env.save_snapshot()
    assert env.steps_done() == 0
    env.run(5)
    do_reset(env, mask, kind, seeds=seeds)
    env.sync()
    fresh = make_env(bk, B, groups=C2, levels=levels, steps=13, seed=S)
    for b in range(B):
        want = fresh.rng_state(b) if mask[b] else tuple(int(x) for x in ref_books(oracle, B, levels, 5, groups=C2).rng_states()[b])
        assert env.rng_state(b) == want, b
    fresh.close()
    env.run(8)

    def ref_of(b, L):  # a reseeded book has lived 8 steps of seed S + b (0 at its snapshot), the others 13 of the original
        return ref_books(oracle, B, levels, L, groups=C2, seed=S if mask[b] else SEED), b

    verify(env, ref_of, np.where(mask, 8, 13), 8, snap_len=np.where(mask, 0, -1))
    env.close()


# ------------------------------------------------------------------ 4. Noise + Momentum members, two resets from one slot
@pytest.mark.parametrize("pipe", ["split", "wave_split"])
def test_members_lists_are_rebuilt_after_each_reset(bk, oracle, pipe):
    B, levels, pool, (n, m, k, k2) = 12, 10, 256, (6, 5, 7, 4)
    env = make_env(bk, B, members=MEMBERS, levels=levels, pool=pool, steps=n + m + k + k2, tick=1)
    env.set_pipeline(pipe)
    ref_of = lambda b, L: (ref_books(oracle, B, levels, L, members=MEMBERS, tick=1), b)  # noqa: E731
    env.run(n)
    env.save_snapshot()
    env.run(m)
    m1 = make_mask("alternate", B)
    env.reset_books(m1)
    env.run(k)
    verify(env, ref_of, np.where(m1, n + k, n + m + k), k, snap_len=np.where(m1, n, -1))
    m2 = np.zeros(B, dtype=bool)
    m2[[1, 2, 3, B - 1]] = True  # kept and reset books of the first round alike
    env.reset_books(m2.astype(np.uint8))
    env.run(k2)
    lens = np.where(m2, n + k2, np.where(m1, n + k + k2, n + m + k + k2))
    verify(env, ref_of, lens, k2, snap_len=np.where(m1 | m2, n, -1))
    assert int(env.trade_counts().sum()) > 0
    env.close()


# ------------------------------------------------------------------ 5. a market env
def market_env(bk, NM, ticks, steps, groups, kind="host", seed=SEED, **kw):
    if kind == "device":
        import torch

        kw["stream"] = torch.cuda.current_stream().cuda_stream
    env = bk.ManyMarketEnv(NM, seed, 0, ticks, STEP, True, levels=10, max_live_orders=128, trade_capacity=4096,
                           history_capacity=steps, **kw)
    env.set_random_market_agents(groups)
    return env


MKT_TICKS = [1, 2]
MKT_GROUPS = [(0, 40, (40, 56), (10, 20), 1, 0.8), (1, 30, (40, 56), (50, 70), 2, 0.5), (0, 20, (30, 70), (5, 9), 2, 0.3)]
_mkt_refs = {}


def ref_markets(oracle, NM, plan, seed=SEED):
    """oracle.ManyMarkets after the plan's runs: plan = ((steps, trading on), ...)."""
    key = (NM, plan, seed)
    if key not in _mkt_refs:
        ref = oracle.ManyMarkets(NM, seed, 0, MKT_TICKS, STEP, True, 10, MKT_GROUPS)
        for steps, on in plan:
            ref.set_trading(on)
            if steps:
                ref.run(steps)
        _mkt_refs[key] = ref
    return _mkt_refs[key]


def verify_markets(env, NM, A, mask, ref_kept, ref_reset, ref_snap, tail, len_kept, len_reset):
    P.no_flags(env)
    hist, tc = env.history(), env.trade_counts()
    for mk in range(NM):
        ref, L = (ref_reset, len_reset) if mask[mk] else (ref_kept, len_kept)
        for a in range(A):
            b, view = mk * A + a, ref.book(mk, a)
            tag = (mk, a, "reset" if mask[mk] else "kept")
            P.same_history(hist[len(hist) - tail:, b], ref.history()[L - tail:L, b], tag=f"{tag}: L2 history tail")
            assert env.rng_state(b) == tuple(int(x) for x in ref.rng_states()[mk]), tag
            assert env.time(b) == L * STEP, tag
            assert int(tc[b]) == view.n_trades(), tag
            if mask[mk]:
                base = ref_snap.book(mk, a).n_trades()
                assert env.trade_count(b) == (view.n_trades(), base), tag
                P.same_records(env.trades(b), view.trades_array()[base:], tag, "retained trade")
                P.same_live(env, b, view, tag)
            else:
                P.same_book(env, b, view, tag=tag)


@pytest.mark.parametrize("kind", ["host", "device"])
def test_markets_rewind_both_books(bk, oracle, kind):
    NM, A, (n, m, k) = 9, 2, (6, 5, 7)
    mask = make_mask("alternate", NM)
    env = market_env(bk, NM, MKT_TICKS, n + m + k, MKT_GROUPS, kind)
    env.run(n)
    env.save_snapshot()
    env.run(m)
    mm, _ = as_kind(mask, kind)
    env.reset_markets(mm, sync=(kind == "host"))
    env.run(k)
    verify_markets(env, NM, A, mask, ref_markets(oracle, NM, ((n + m + k, True),)), ref_markets(oracle, NM, ((n + k, True),)),
                   ref_markets(oracle, NM, ((n, True),)), k, n + m + k, n + k)
    env.close()


def test_markets_reseed_puts_both_books_on_the_new_stream(bk, oracle):
    NM, A, S = 9, 2, 77_000
    mask = make_mask("third", NM)
    env = market_env(bk, NM, MKT_TICKS, 13, MKT_GROUPS)
    env.save_snapshot()
    env.run(5)
    env.reset_markets(mask, seeds=(S + np.arange(NM)).astype(np.uint64))
    fresh = market_env(bk, NM, MKT_TICKS, 1, MKT_GROUPS, seed=S)
    for mk in np.flatnonzero(mask):
        assert env.rng_state(mk * A) == env.rng_state(mk * A + 1) == fresh.rng_state(mk * A), mk
    fresh.close()
    env.run(8)
    verify_markets(env, NM, A, mask, ref_markets(oracle, NM, ((13, True),)), ref_markets(oracle, NM, ((8, True),), seed=S),
                   ref_markets(oracle, NM, ((0, True),), seed=S), 8, 13, 8)
    env.close()


# ------------------------------------------------------------------ 6. per-book tables
def test_per_book_rows_keep_stepping_their_own_books(bk, oracle):
    B, levels, (n, m, k) = 16, 10, (6, 5, 7)
    r = np.random.default_rng(3)
    base = []
    for _ in range(8):
        row = []
        for g in range(2):
            tlo, vlo = int(r.integers(20, 60)), int(r.integers(1, 40))
            row.append((32, (tlo, tlo + int(r.integers(1, 30))), (vlo, vlo + int(r.integers(1, 30))), 2 * int(r.integers(1, 4)),
                        float(r.choice([1.0, float(r.random())]))))
        base.append(row)
    rows = [base[b % 8] for b in range(B)]
    env = make_env(bk, B, levels=levels, steps=n + m + k)
    env.set_random_agents_per_book(rows)
    mask = make_mask("alternate", B)
    mask[:8] = ~mask[:8]  # half the books, and each of the 8 rows on a reset and on a kept book
    env.run(n)
    env.save_snapshot()
    env.run(m)
    env.reset_books(mask)
    env.run(k)

    # the oracle is built per row: ManyBooks(1, seed + b, .., row b)
    verify(env, lambda b, L: (ref_books(oracle, 1, levels, L, groups=rows[b], seed=SEED + b), 0),
           np.where(mask, n + k, n + m + k), k, snap_len=np.where(mask, n, -1))
    env.close()


# ------------------------------------------------------------------ 7. two slots
def test_two_slots_resave_and_drop(bk, oracle):
    B, levels = 24, 16
    env = make_env(bk, B, groups=C2, levels=levels, steps=30)
    ref_of = lambda b, L: (ref_books(oracle, B, levels, L, groups=C2), b)  # noqa: E731
    env.run(4)
    env.save_snapshot(0)
    env.run(5)
    env.save_snapshot(1)
    env.run(3)  # 12 steps
    m0, m1 = np.zeros(B, dtype=bool), np.zeros(B, dtype=bool)
    m0[:8], m1[8:16] = True, True
    env.reset_books(m0, slot=0)
    env.reset_books(m1, slot=1)
    env.run(6)  # kept 18, slot 0's 4 + 6, slot 1's 9 + 6
    lens = np.where(m0, 10, np.where(m1, 15, 18))
    snaps = np.where(m0, 4, np.where(m1, 9, -1))
    verify(env, ref_of, lens, 6, snap_len=snaps)
    # a later save of slot 0 changes what a reset from it restores
    env.save_snapshot(0)
    env.run(2)
    m2 = np.zeros(B, dtype=bool)
    m2[[0, 9, 20]] = True
    env.reset_books(m2, slot=0)
    env.run(3)
    lens2 = np.where(m2, lens + 3, lens + 5)
    # (a reset book's retained trades start at the count of ITS OWN line at the save: length lens[b])
    hist, tc = env.history(), env.trade_counts()
    for b in range(B):
        L = int(lens2[b])
        ref = ref_of(b, L)[0]
        P.same_history(hist[-3:, b], facts(ref)["history"][L - 3:L, b], tag=f"book {b} after the re-save")
        assert int(tc[b]) == int(facts(ref)["trade_counts"][b]) and env.time(b) == L * STEP, b
        assert env.rng_state(b) == tuple(int(x) for x in facts(ref)["rng"][b]), b
        P.same_live(env, b, ref.book(b))
        if m2[b]:
            base = int(facts(ref_of(b, int(lens[b]))[0])["trade_counts"][b])
            assert env.trade_count(b) == (int(tc[b]), base), b
            P.same_records(env.trades(b), ref.book(b).trades_array()[base:], b, "retained trade")
    assert env.snapshot_bytes() == B * (env.state_bytes_per_book() + 4 * env.width)
    env.drop_snapshot(0)
    before = P.snapshot(env, books=[17])  # (a book that was never reset: all its trades are retained)
    with pytest.raises(bk.BourseError, match="empty"):
        env.reset_books(m2, slot=0)
    P.assert_same(before, P.snapshot(env, books=[17]))
    env.drop_snapshot(0)  # (dropping an empty slot is not an error)
    env.reset_books(m1, slot=1)  # the other slot is still there
    env.close()


# ------------------------------------------------------------------ 8. the header fix-ups
def test_a_sticky_flag_survives_the_reset(bk, oracle):
    B = 20
    env = make_env(bk, B, groups=C2, steps=20, trade_capacity=8, strict=False)
    env.save_snapshot()  # (of the empty books: no flag in the snapshot)
    assert not env.flags().any()
    env.run(8)
    flagged = env.flags()
    assert (flagged & FLAG_TRADE_OVERFLOW).any(), "8 records per book were meant to overflow"
    env.reset_books(np.ones(B, dtype=bool))
    assert np.array_equal(env.flags(), flagged)
    env.clear_trades()
    env.run(1)
    assert np.array_equal(env.flags() & flagged, flagged)
    env.clear_flags()
    assert not env.flags().any()
    env.close()


def test_reset_books_take_the_envs_current_trading_flag(bk, oracle):
    # (the market oracle is the one with a trading switch)
    NM, A, (n, m, k) = 9, 2, (6, 5, 7)
    mask = make_mask("alternate", NM)
    env = market_env(bk, NM, MKT_TICKS, n + m + k, MKT_GROUPS)
    env.run(n)
    env.save_snapshot()  # the snapshot's books trade
    env.run(m)
    env.disable_trading()
    env.reset_markets(mask)
    env.run(k)
    short = ref_markets(oracle, NM, ((n, True), (k, False)))
    verify_markets(env, NM, A, mask, ref_markets(oracle, NM, ((n + m, True), (k, False))), short,
                   ref_markets(oracle, NM, ((n, True),)), k, n + m + k, n + k)
    for mk in np.flatnonzero(mask):  # no trade after the reset
        for a in range(A):
            assert env.trade_count(mk * A + a)[0] == ref_markets(oracle, NM, ((n, True),)).book(mk, a).n_trades()
    env.close()


def test_trade_count_after_a_reset_is_the_snapshots(bk, oracle):
    B, levels = 10, 16
    env = make_env(bk, B, groups=C2, levels=levels, steps=11)
    env.run(6)
    env.save_snapshot()
    at_save = [env.trade_count(b) for b in range(B)]
    assert all(t == int(w) and first == 0 for (t, first), w in zip(at_save, ref_books(oracle, B, levels, 6, groups=C2).trade_counts()))
    assert sum(t for t, _ in at_save) > 0
    env.run(5)
    mask = make_mask("alternate", B)
    env.reset_books(mask)
    for b in range(B):
        total, first = env.trade_count(b)
        if mask[b]:
            assert (total, first) == (at_save[b][0], at_save[b][0]), b
            assert len(env.trades(b)) == 0
        else:
            assert first == 0 and total == int(ref_books(oracle, B, levels, 11, groups=C2).trade_counts()[b]), b
    env.close()


# ------------------------------------------------------------------ 9. neighbours: checkpoint / restore and warm
def _state(env):
    return {"level2": env.level2(), "trade_counts": env.trade_counts(), "order_counts": env.order_counts(), "flags": env.flags(),
            "retained": [env.trades(b) for b in range(env.n_books)], "first": [env.trade_count(b)[1] for b in range(env.n_books)],
            "live": [env.live_orders(b) for b in range(env.n_books)], "rng": [env.rng_state(b) for b in range(env.n_books)],
            "time": [env.time(b) for b in range(env.n_books)]}


def test_checkpoint_restore_and_warm_after_a_reset(bk, oracle):
    B, levels = 14, 16
    env = make_env(bk, B, groups=C2, levels=levels, steps=40)
    env.run(6)
    env.save_snapshot()
    env.run(5)
    mask = make_mask("alternate", B)
    env.reset_books(mask)
    env.run(2)
    image = env.checkpoint()
    other = make_env(bk, B, groups=C2, levels=levels, steps=40)
    other.restore(image)
    before = _state(env)
    env.warm(5)
    env.sync()
    P.assert_same(before, _state(env))  # warm() after a reset changes nothing
    env.run(7)
    other.run(7)
    mine, theirs = _state(env), _state(other)
    # (a restore retains no earlier trade record: the records of the 7 steps are compared)
    for b in range(B):
        n7 = int(theirs["trade_counts"][b]) - theirs["first"][b]
        mine["retained"][b] = mine["retained"][b][len(mine["retained"][b]) - n7:]
    mine.pop("first"), theirs.pop("first")
    P.assert_same(mine, theirs)
    P.same_history(env.history()[-7:], other.history()[-7:])
    lens = np.where(mask, 6 + 2 + 7, 6 + 5 + 2 + 7)
    verify(env, lambda b, L: (ref_books(oracle, B, levels, L, groups=C2), b), lens, 9, snap_len=np.where(mask, 6, -1))
    env.close()
    other.close()


# ------------------------------------------------------------------ 10. refusals leave the env as it was
def test_refusals_leave_the_env_unchanged(bk, oracle):
    B = 12
    env = make_env(bk, B, groups=C2, steps=20)
    env.run(5)
    env.save_snapshot(1)
    env.run(3)
    before = P.snapshot(env)
    mask = make_mask("alternate", B)
    with pytest.raises(bk.BourseError, match="empty"):
        env.reset_books(mask, slot=0)
    with pytest.raises(bk.BourseError, match="slot"):
        env.reset_books(mask, slot=4)
    with pytest.raises(bk.BourseError, match="slot"):
        env.save_snapshot(4)
    with pytest.raises(ValueError):
        env.reset_books(mask[:-1], slot=1)
    with pytest.raises(ValueError):
        env.reset_books(np.zeros(B + 1, dtype=np.uint8), slot=1)
    with pytest.raises(ValueError):
        env.reset_books(mask, seeds=np.arange(B - 1, dtype=np.uint64), slot=1)
    import torch

    with pytest.raises(ValueError):
        env.reset_books(mask, seeds=torch.zeros(B, dtype=torch.int64, device="cuda"), slot=1)
    with pytest.raises(ValueError):
        env.reset_books(torch.zeros(B, dtype=torch.uint8, device="cuda"), seeds=np.arange(B, dtype=np.uint64), slot=1)
    with pytest.raises(ValueError):
        env.reset_books(torch.zeros(B - 1, dtype=torch.uint8, device="cuda"), slot=1)
    P.assert_same(before, P.snapshot(env))
    # agents installed again with other parameters since the snapshot
    env.set_random_agents([(32, (40, 56), (10, 20), 2, 0.7), (32, (40, 56), (50, 70), 2, 0.2)])
    with pytest.raises(bk.BourseError, match="install the same agents first"):
        env.reset_books(mask, slot=1)
    P.assert_same(before, P.snapshot(env))
    env.set_random_agents(C2)  # the same agents again: the slot is good again
    env.reset_books(mask, slot=1)
    env.close()

    dev = make_env(bk, B, steps=4)
    dev.enable_device_ingress()
    with pytest.raises(bk.BourseError, match="checkpoints"):
        dev.save_snapshot()
    with pytest.raises(bk.BourseError, match="checkpoints"):
        dev.reset_books(mask)
    dev.close()

    log = make_env(bk, B, groups=C2, steps=4, max_orders=512)
    log.enable_agent_order_log()
    log.run(2)
    before = P.snapshot(log)
    with pytest.raises(bk.BourseError, match="order log"):
        log.save_snapshot()
    with pytest.raises(bk.BourseError, match="order log"):
        log.reset_books(mask)
    P.assert_same(before, P.snapshot(log))
    log.close()

    host = make_env(bk, B, steps=4, max_orders=16)
    host.place_order(3, True, 10, 1, 100)
    host.step()
    before = P.snapshot(host)
    with pytest.raises(bk.BourseError, match="host-placed"):
        host.save_snapshot()
    with pytest.raises(bk.BourseError, match="host-placed"):
        host.reset_books(mask)
    P.assert_same(before, P.snapshot(host))
    host.close()
