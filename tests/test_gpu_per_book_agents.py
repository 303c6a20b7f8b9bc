"""RandomAgents parameters per book (bk_set_random_agents_per_book / ManyBookEnv.set_random_agents_per_book): book b of an
env stepped with a per-unit table steps as book b of an env given set_random_agents(row b) does - bit for bit against the
CPU oracle (ManyBooks(1, seed + b, ..., row b)) under every pipeline and pool size, at scale with parts, on markets, on a
shard, with the order log, bk_warm and checkpoints, and the refusals leave the installed agents in place."""
import numpy as np
import pytest

import oracle_parity as P

pytestmark = pytest.mark.gpu

SEED, STEP, LEVELS, T = 101, 100_000, 10, 30
MODES = ("auto", "fused", "split", "wave_split", "wave")
POOLS = (64, 128, 256, 512)
# unequal group sizes that do not align to 64 slots
SIZES = {64: (23, 30), 128: (50, 41, 30), 256: (100, 77, 70), 512: (200, 150, 130)}


@pytest.fixture(scope="module")
def bk():
    import bourse_amd

    return bourse_amd


def het_rows(n_units, pool, seed=7):
    """Seeded random rows: widths 1 and wide, activity 0.0 / 1.0 / random, tick sizes multiples of the env's 2."""
    r = np.random.default_rng(seed + pool)
    rows = []
    for _ in range(n_units):
        row = []
        for n in SIZES[pool]:
            tlo = int(r.integers(1, 300))
            tw = int(r.choice([1, int(r.integers(2, 40)), int(r.integers(500, 4000))]))
            vlo = int(r.integers(1, 60))
            vw = int(r.choice([1, int(r.integers(2, 30)), int(r.integers(200, 2000))]))
            rate = float(r.choice([0.0, 1.0, float(r.random())]))
            row.append((n, (tlo, tlo + tw), (vlo, vlo + vw), 2 * int(r.integers(1, 5)), rate))
        rows.append(row)
    return rows


def same_rows(n_units, pool):
    n = SIZES[pool]
    return [[(n[0], (32, 64), (10, 20), 2, 0.8)] + [(k, (30 + 5 * i, 70), (40, 60 + i), 4, 0.3) for i, k in enumerate(n[1:])]
            for _ in range(n_units)]


def make_env(bk, B, pool, steps=T, **kw):
    return bk.ManyBookEnv(B, SEED, 0, 2, STEP, True, levels=LEVELS, max_live_orders=pool, trade_capacity=3 * pool * steps,
                          history_capacity=steps, **kw)


def run_split(env, mode):
    env.set_pipeline(mode)
    env.run(13)
    env.run(T - 13)


_oracle = {}


def oracle_book(oracle, b, row, steps=T, seed=SEED):
    key = (seed + b, repr(row), steps)
    if key not in _oracle:
        ref = oracle.ManyBooks(1, seed + b, 0, 2, STEP, True, LEVELS, row)
        ref.run(steps)
        _oracle[key] = (ref.history()[:, 0], int(ref.trade_counts()[0]), tuple(int(x) for x in ref.rng_states()[0]),
                        ref.book(0).get_time(), ref)
    return _oracle[key]


def check_against_oracle(oracle, env, rows, sample):
    hist, tc = env.history(), env.trade_counts()
    P.no_flags(env)
    for b, row in enumerate(rows):
        h, n, rng, t, ref = oracle_book(oracle, b, row)
        assert np.array_equal(hist[:, b], h), b
        assert int(tc[b]) == n, b
        assert env.rng_state(b) == rng, b
        assert env.time(b) == t, b
        if b in sample:
            P.same_book(env, b, ref.book(0))


# ------------------------------------------------------------------ 1. identity with the uniform call
@pytest.mark.parametrize("pool", POOLS)
@pytest.mark.parametrize("mode", MODES)
def test_identical_rows_equal_the_uniform_agents(bk, pool, mode):
    B = 512
    rows = same_rows(B, pool)
    outs = []
    for per_book in (False, True):
        env = make_env(bk, B, pool)
        if per_book:
            # (the structured-array form of the table; the list form is covered below)
            tab = np.zeros((B, len(rows[0])), dtype=bk.RANDOM_AGENTS_DTYPE)
            for g, (n, tr, vr, ts, rate) in enumerate(rows[0]):
                tab[:, g] = (n, tr[0], tr[1], vr[0], vr[1], ts, np.float32(rate))
            env.set_random_agents_per_book(tab)
        else:
            env.set_random_agents(rows[0])
        run_split(env, mode)
        outs.append(P.snapshot(env))
        if per_book and mode == "fused":
            assert env.pipeline()[0] == "split"  # (k_run_random has no per-book form)
        env.close()
    P.assert_same(outs[0], outs[1])


# ------------------------------------------------------------------ 2. heterogeneous rows against the oracle
@pytest.mark.parametrize("pool", POOLS)
@pytest.mark.parametrize("mode", MODES)
def test_heterogeneous_rows_match_the_oracle(bk, oracle, pool, mode):
    B = 320
    rows = het_rows(B, pool)
    env = make_env(bk, B, pool)
    env.set_random_agents_per_book(rows)
    run_split(env, mode)
    check_against_oracle(oracle, env, rows, sample={0, 1, 77, 191, B - 1})
    # live orders in priority order: those of a uniform env given the book's row (book_offset = b: the same RNG stream)
    for b in (3, 150, B - 2):
        one = make_env(bk, 1, pool, book_offset=b)
        one.set_random_agents(rows[b])
        one.run(T)
        assert np.array_equal(env.live_orders(b), one.live_orders(0)), b
        one.close()
    env.close()


# ------------------------------------------------------------------ 3. at scale, with parts
def blocks_env(bk, B, pool, n_blocks):
    base = het_rows(n_blocks, pool, seed=11)
    per = B // n_blocks
    rows = [base[b // per] for b in range(B)]
    env = bk.ManyBookEnv(B, SEED, 0, 2, STEP, True, levels=LEVELS, max_live_orders=pool, trade_capacity=2048, history_capacity=20)
    env.set_random_agents_per_book(rows)
    return env, base, per


def check_blocks(oracle, env, base, per, steps):
    hist, tc = env.history(), env.trade_counts()
    P.no_flags(env)
    for k, row in enumerate(base):
        b0 = k * per
        ref = oracle.ManyBooks(per, SEED + b0, 0, 2, STEP, True, LEVELS, row)
        ref.run(steps, n_threads=8)
        assert np.array_equal(hist[:, b0:b0 + per], ref.history()), k
        assert np.array_equal(tc[b0:b0 + per], ref.trade_counts()), k
        assert [env.rng_state(b) for b in range(b0, b0 + per, 97)] == [tuple(int(x) for x in r) for r in ref.rng_states()[::97]]


def test_wave_split_at_8192_books_with_four_parts(bk, oracle):
    env, base, per = blocks_env(bk, 8192, 128, 8)
    env.set_pipeline("wave_split")
    env.set_wave_options(parts=4)
    env.run(20)
    assert env.pipeline() == ("wave_split", 4)
    check_blocks(oracle, env, base, per, 20)
    env.close()


def test_lane_split_at_scale_with_four_parts(bk, oracle):
    env, base, per = blocks_env(bk, 27648, 128, 8)
    env.set_split_parts(4)
    env.run(20)
    assert env.pipeline() == ("split", 4)  # (auto at R = 2 from 27 648 books)
    check_blocks(oracle, env, base, per, 20)
    env.close()


# ------------------------------------------------------------------ 4. markets
@pytest.mark.parametrize("ticks", [[1, 2], [2, 1, 4]])
def test_markets_with_rows_per_market(bk, oracle, ticks):
    NM, r = 96, np.random.default_rng(len(ticks))
    A = len(ticks)
    sizes = (40, 33, 20)[:A]
    rows = []
    for m in range(NM):
        row = []
        for i, n in enumerate(sizes):
            a = i % A
            tlo = int(r.integers(5, 60))
            row.append((a, n, (tlo, tlo + int(r.choice([1, int(r.integers(2, 300))]))), (1 + i, 9 + int(r.integers(0, 50))),
                        ticks[a] * int(r.integers(1, 4)), float(r.choice([0.0, 1.0, float(r.random())]))))
        rows.append(row)
    env = bk.ManyMarketEnv(NM, SEED, 0, ticks, STEP, True, levels=LEVELS, max_live_orders=128, trade_capacity=4000,
                           history_capacity=T)
    env.set_random_market_agents_per_market(rows)
    env.run(11)
    env.run(T - 11)
    hist = env.history()
    P.no_flags(env)
    for m in range(NM):
        ref = oracle.ManyMarkets(1, SEED + m, 0, ticks, STEP, True, LEVELS, rows[m])
        ref.run(T)
        assert np.array_equal(hist[:, m * A:(m + 1) * A], ref.history()), m
        assert env.rng_state(m * A) == tuple(int(x) for x in ref.rng_states()[0]), m
    env.close()


# ------------------------------------------------------------------ 5. sharding
def test_a_shard_with_its_local_rows_equals_the_slice_of_the_full_env(bk):
    B, pool, k, n = 1024, 128, 384, 256
    rows = het_rows(B, pool, seed=3)
    full = make_env(bk, B, pool)
    full.set_random_agents_per_book(rows)
    full.run(T)
    shard = make_env(bk, n, pool, book_offset=k)
    shard.set_random_agents_per_book(rows[k:k + n])
    shard.run(T)
    assert np.array_equal(full.history()[:, k:k + n], shard.history())
    assert np.array_equal(full.trade_counts()[k:k + n], shard.trade_counts())
    assert [full.rng_state(k + b) for b in range(n)] == [shard.rng_state(b) for b in range(n)]
    full.close()
    shard.close()


# ------------------------------------------------------------------ 6. composition
@pytest.mark.parametrize("mode", ["auto", "fused", "wave_split"])
def test_order_log_with_a_table(bk, oracle, mode):
    B, pool = 256, 128
    rows = het_rows(B, pool, seed=5)
    env = bk.ManyBookEnv(B, SEED, 0, 2, STEP, True, levels=LEVELS, max_live_orders=pool, max_orders=pool * T,
                         trade_capacity=3 * pool * T, history_capacity=T)
    env.set_random_agents_per_book(rows)
    env.enable_agent_order_log()
    run_split(env, mode)
    for b in (0, 9, 130, B - 1):
        P.same_orders(env, b, oracle_book(oracle, b, rows[b])[-1].book(0))
    env.close()


@pytest.mark.parametrize("pool,mode", [(64, "auto"), (128, "split"), (256, "wave_split"), (512, "wave")])
def test_warm_changes_nothing(bk, pool, mode):
    B = 512
    rows = het_rows(B, pool, seed=9)
    outs = []
    for warm in (False, True):
        env = make_env(bk, B, pool)
        env.set_random_agents_per_book(rows)
        env.set_pipeline(mode)
        if warm:
            env.warm(7)
        env.run(T)
        outs.append(P.snapshot(env, books=range(0, B, 17)))
        env.close()
    P.assert_same(outs[0], outs[1])


def test_checkpoint_continues_and_refuses_another_table(bk):
    B, pool = 512, 128
    rows = het_rows(B, pool, seed=13)
    a = make_env(bk, B, pool)
    a.set_random_agents_per_book(rows)
    a.run(12)
    img = a.checkpoint()
    a.run(T - 12)
    b = make_env(bk, B, pool)
    b.set_random_agents_per_book(rows)
    b.restore(img)
    b.run(T - 12)
    assert np.array_equal(a.history(12, T - 12), b.history(12, T - 12))
    assert np.array_equal(a.trade_counts(), b.trade_counts())
    assert [a.rng_state(i) for i in range(B)] == [b.rng_state(i) for i in range(B)]
    other = [list(r) for r in rows]
    n, tr, vr, ts, rate = other[200][0]
    other[200][0] = (n, (tr[0], tr[1] + 1), vr, ts, rate)
    c = make_env(bk, B, pool)
    c.set_random_agents_per_book(other)
    with pytest.raises(bk.BourseError, match="different agent set"):
        c.restore(img)
    u = make_env(bk, B, pool)
    u.set_random_agents(rows[0])  # (the uniform set of row 0 is not the table either)
    with pytest.raises(bk.BourseError, match="different agent set"):
        u.restore(img)
    for e in (a, b, c, u):
        e.close()


# ------------------------------------------------------------------ 7. refusals and replacement
def test_refusals_keep_the_installed_agents_and_a_uniform_call_replaces_the_table(bk):
    from bourse_amd import _lib

    B, pool = 256, 128
    rows = het_rows(B, pool, seed=17)

    def bad(u, g, **kw):
        t = [list(r) for r in rows]
        n, tr, vr, ts, rate = t[u][g]
        d = dict(n=n, tr=tr, vr=vr, ts=ts, rate=rate)
        d.update(kw)
        t[u][g] = (d["n"], d["tr"], d["vr"], d["ts"], d["rate"])
        return t

    cases = [(bad(40, 1, tr=(50, 50)), _lib.BK_INVALID, "unit 40, group 1"),
             (bad(41, 2, vr=(9, 3)), _lib.BK_INVALID, "unit 41, group 2"),
             (bad(42, 0, tr=(0, 5)), _lib.BK_INVALID, "unit 42, group 0"),
             (bad(43, 0, ts=3), _lib.BK_PRICE, "unit 43, group 0"),
             (bad(44, 1, n=SIZES[pool][1] + 1), _lib.BK_INVALID, "n_agents differs"),
             ([[(pool, (1, 5), (1, 5), 2, 0.5)] * 2 for _ in range(B)], _lib.BK_CAPACITY, "max_live_orders")]
    ref = make_env(bk, B, pool)
    ref.set_random_agents_per_book(rows)
    ref.run(T)
    want = P.snapshot(ref, books=range(0, B, 11))
    ref.close()
    env = make_env(bk, B, pool, strict=False)
    env.set_random_agents_per_book(rows)
    for table, code, msg in cases:
        with pytest.raises((bk.BourseError, ValueError)) as ei:  # (BK_PRICE_NOT_TICK_MULTIPLE is a ValueError, as in the reference)
            env.set_random_agents_per_book(table)
        assert getattr(ei.value, "code", _lib.BK_PRICE) == code and isinstance(ei.value, bk.BourseError) == (code != _lib.BK_PRICE), msg
        assert msg in str(ei.value), str(ei.value)
    env.run(T)
    P.assert_same(want, P.snapshot(env, books=range(0, B, 11)))
    env.close()
    # a later set_random_agents replaces the table: the env is uniform again
    outs = []
    for first_table in (False, True):
        e = make_env(bk, B, pool)
        if first_table:
            e.set_random_agents_per_book(rows)
        e.set_random_agents(rows[5])
        e.set_pipeline("fused")
        e.run(T)
        assert e.pipeline()[0] == "fused"
        outs.append(P.snapshot(e, books=range(0, B, 13)))
        e.close()
    P.assert_same(outs[0], outs[1])
