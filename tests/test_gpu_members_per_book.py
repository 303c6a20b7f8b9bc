"""AgentSet members (NoiseAgent / MomentumAgent, with RandomAgents) whose parameters differ per book or market
(bk_set_agents_per_book / ManyBookEnv.set_agents_per_book / ManyMarketEnv.set_market_agents_per_market): book b of an env
stepped with a per-unit table steps as book b of an env given set_agents(row b) does - identical rows give exactly the
uniform call's outputs, heterogeneous rows match the CPU oracle (ManyBooks(1, seed + b, ..., members=row b)) under every
pipeline (k_run_mixed, the lane kernel with its per-lane price queue, the wave-per-book kernel, the wave decode), at scale
with parts, on markets, on a shard, with bk_warm and checkpoints, and refusals leave the installed agents in place."""
import numpy as np
import pytest

import oracle_parity as P

pytestmark = pytest.mark.gpu

SEED, STEP, LEVELS, T, TICK = 101, 1_000_000, 10, 30, 2
# fused = k_run_mixed; split = k_agents_mixed_lanes; split_wave = k_agents_mixed; wave_split = k_agents_mixed_wave;
# "mixed" cycles through the four between launches (they share the device state)
MODES = ("fused", "split", "split_wave", "wave_split", "mixed")
NOISE_P = dict(tick_size=2, p_limit=0.2, p_market=0.2, p_cancel=0.3, trade_vol=100, price_dist_mu=0.0, price_dist_sigma=1.0)
MOM_P = dict(tick_size=2, p_cancel=0.3, trade_vol=100, decay=1.0, demand=5.0, scale=0.5, order_ratio=1.0, price_dist_mu=0.0,
             price_dist_sigma=3.0)
SETS = {  # member kinds and sizes of the heterogeneous tables, and the pool they run on
    "noise": ((("noise", 0, 16),), 128),
    "doc": ((("momentum", 0, 10), ("noise", 10, 20)), 256),  # the reference's doc example (crates/step_sim/src/lib.rs:37-88)
    "four": ((("random", 40), ("noise", 0, 30), ("momentum", 100, 25), ("noise", 200, 10)), 512),
}
CLAMP_BOOK = 5  # the noise table's row whose sigma 10 reaches the u32::MAX clamp: FLAG_PRICE_TICK on that book only


@pytest.fixture(scope="module")
def bk():
    import bourse_amd

    return bourse_amd


def _noise(r, clamp=False):
    p_limit = 1.0 if clamp else float(r.choice([0.0, 1.0, 0.5 * float(r.random())]))
    return dict(tick_size=TICK * int(r.integers(1, 5)), p_limit=p_limit, p_market=float(r.choice([0.0, 1.0, 0.3 * float(r.random())])),
                p_cancel=1.0 if p_limit == 1.0 else float(0.4 + 0.6 * r.random()), trade_vol=int(r.integers(1, 200)),
                price_dist_mu=5.0 if clamp else float(r.normal() * 0.5),
                price_dist_sigma=10.0 if clamp else float(r.choice([0.0, 0.3 + 2.0 * float(r.random())])))


def _momentum(r):
    return dict(tick_size=TICK * int(r.integers(1, 5)), p_cancel=float(r.choice([1.0, 0.5 + 0.5 * float(r.random())])),
                trade_vol=int(r.integers(1, 200)), decay=float(r.choice([0.0, 1.0, float(r.random())])),
                demand=float(r.choice([0.0, 20.0 * float(r.random())])), scale=float(r.random()), order_ratio=float(2.0 * r.random()),
                price_dist_mu=float(r.normal() * 0.5), price_dist_sigma=float(r.choice([0.0, 0.3 + 3.0 * float(r.random())])))


def het_row(kind, r, clamp=False):
    row = []
    for m in SETS[kind][0]:
        if m[0] == "random":
            lo = 1073741800 + int(r.integers(0, 20))
            row.append(("random", m[1], (lo, lo + int(r.integers(1, 40))), (1 + int(r.integers(0, 10)), 30 + int(r.integers(0, 50))),
                        TICK, float(r.choice([0.0, 1.0, float(r.random())]))))
        elif m[0] == "noise":
            row.append(("noise", m[1], m[2], _noise(r, clamp)))
        else:
            row.append(("momentum", m[1], m[2], _momentum(r)))
    return row


def het_rows(kind, n, seed=7):
    r = np.random.default_rng(seed + len(kind))
    return [het_row(kind, r, clamp=(kind == "noise" and b == CLAMP_BOOK)) for b in range(n)]


def make_env(bk, B, pool, steps=T, **kw):
    kw.setdefault("strict", False)  # (flags are compared as outputs, or checked against the expected ones)
    return bk.ManyBookEnv(B, SEED, 0, TICK, STEP, True, levels=LEVELS, max_live_orders=pool, trade_capacity=8 * pool * steps,
                          history_capacity=steps, **kw)


def run_chunks(env, mode, chunks=(7, 1, 13, 9)):
    for i, c in enumerate(chunks):
        env.set_pipeline(("fused", "wave_split", "split", "split_wave")[i % 4] if mode == "mixed" else mode)
        env.run(c)


_oracle = {}


def oracle_book(oracle, b, row, steps=T, seed=SEED):
    key = (seed + b, repr(row), steps)
    if key not in _oracle:
        ref = oracle.ManyBooks(1, seed + b, 0, TICK, STEP, True, LEVELS, members=row)
        ref.run(steps)
        _oracle[key] = (ref.history()[:, 0], int(ref.trade_counts()[0]), tuple(int(x) for x in ref.rng_states()[0]),
                        ref.book(0).get_time(), ref)
    return _oracle[key]


def check_against_oracle(bk, oracle, env, rows, sample, clamp_book=None):
    hist, tc, flags = env.history(), env.trade_counts(), env.flags()
    want_flags = np.zeros_like(flags)
    if clamp_book is not None:
        want_flags[clamp_book] = bk._lib.FLAG_PRICE_TICK
    assert np.array_equal(flags, want_flags), np.flatnonzero(flags)[:8]
    for b, row in enumerate(rows):
        h, n, rng, t, ref = oracle_book(oracle, b, row)
        assert np.array_equal(hist[:, b], h), b
        assert int(tc[b]) == n, b
        assert env.rng_state(b) == rng, b
        assert env.time(b) == t, b
        if b in sample:
            P.same_book(env, b, ref.book(0))


# ------------------------------------------------------------------ 1. identity with the uniform call
@pytest.mark.parametrize("pool", (64, 128, 256, 512))
@pytest.mark.parametrize("mode", MODES)
def test_identical_rows_equal_the_uniform_agents(bk, pool, mode):
    B = 320
    members = [("momentum", 0, 8, MOM_P), ("noise", 8, 12, NOISE_P)]
    if pool == 512:
        members = [("random", 40, (1073741800, 1073741840), (10, 20), 2, 0.5)] + members
    outs = []
    for per_book in (False, True):
        env = make_env(bk, B, pool)
        if per_book:
            env.set_agents_per_book([members] * B)
        else:
            env.set_agents(members)
        run_chunks(env, mode)
        outs.append(P.snapshot(env))
        env.close()
    assert int(outs[0]["trade_counts"].sum()) > 0
    P.assert_same(outs[0], outs[1])


# ------------------------------------------------------------------ 2. heterogeneous rows against the oracle
@pytest.mark.parametrize("kind", sorted(SETS))
@pytest.mark.parametrize("mode", MODES)
def test_heterogeneous_rows_match_the_oracle(bk, oracle, kind, mode):
    B = 96  # (the lane kernel: one full wave and a partial one)
    rows = het_rows(kind, B)
    env = make_env(bk, B, SETS[kind][1])
    env.set_agents_per_book(rows)
    run_chunks(env, mode)
    check_against_oracle(bk, oracle, env, rows, sample={0, 1, CLAMP_BOOK, 63, 64, B - 1},
                         clamp_book=CLAMP_BOOK if kind == "noise" else None)
    assert int(env.trade_counts().sum()) > 0
    env.close()


# ------------------------------------------------------------------ 3. at scale, with parts
def blocks_env(bk, B, n_blocks, pool=128):
    base = het_rows("doc", n_blocks, seed=11)
    per = B // n_blocks
    env = bk.ManyBookEnv(B, SEED, 0, TICK, STEP, True, levels=LEVELS, max_live_orders=pool, trade_capacity=4096,
                         history_capacity=20)
    env.set_agents_per_book([base[b // per] for b in range(B)])
    return env, base, per


def check_blocks(oracle, env, base, per, steps, blocks):
    hist, tc = env.history(), env.trade_counts()
    P.no_flags(env)
    for k in blocks:
        b0 = k * per
        n = 256  # (the first 256 books of the block)
        ref = oracle.ManyBooks(n, SEED + b0, 0, TICK, STEP, True, LEVELS, members=base[k])
        ref.run(steps, 8)
        assert np.array_equal(hist[:, b0:b0 + n], ref.history()), k
        assert np.array_equal(tc[b0:b0 + n], ref.trade_counts()), k
        assert [env.rng_state(b) for b in range(b0, b0 + n, 37)] == [tuple(int(x) for x in r) for r in ref.rng_states()[::37]]


def test_wave_split_at_8192_books_with_four_parts(bk, oracle):
    env, base, per = blocks_env(bk, 8192, 8)
    env.set_pipeline("wave_split")
    env.set_wave_options(parts=4)
    env.run(20)
    assert env.pipeline() == ("wave_split", 4)
    check_blocks(oracle, env, base, per, 20, blocks=(0, 3, 7))
    env.close()


def test_lane_split_at_scale_in_parts(bk, oracle):
    env, base, per = blocks_env(bk, 12300, 12)
    env.set_pipeline("split")
    env.run(20)
    assert env.pipeline() == ("split", 3)
    check_blocks(oracle, env, base, per, 20, blocks=(0, 5, 11))
    env.close()


# ------------------------------------------------------------------ 4. markets (the lane kernel's per-lane parameters)
@pytest.mark.parametrize("ticks", [[2, 2], [2, 4, 2]])
def test_markets_with_rows_per_market(bk, oracle, ticks):
    NM, A = 80, len(ticks)
    r = np.random.default_rng(A)
    rows = []
    for m in range(NM):
        row = [(0, ("noise", 0, 12, dict(_noise(r), tick_size=4 * int(r.integers(1, 3))))),
               (1, ("momentum", 12, 8, dict(_momentum(r), tick_size=4 * int(r.integers(1, 3)))))]
        if A > 2:
            lo = int(r.integers(5, 60))
            row.append((2, ("random", 10, (lo, lo + int(r.integers(1, 300))), (1, 9 + int(r.integers(0, 50))), 2,
                            float(r.choice([0.0, 1.0, float(r.random())])))))
        rows.append(row)
    env = bk.ManyMarketEnv(NM, SEED, 0, ticks, STEP, True, levels=LEVELS, max_live_orders=128, trade_capacity=8000,
                           history_capacity=T)
    env.set_market_agents_per_market(rows)
    env.run(11)
    env.run(T - 11)
    hist = env.history()
    P.no_flags(env)
    for m in range(NM):
        ref = oracle.ManyMarkets(1, SEED + m, 0, ticks, STEP, True, LEVELS, members=rows[m])
        ref.run(T)
        assert np.array_equal(hist[:, m * A:(m + 1) * A], ref.history()), m
        assert env.rng_state(m * A) == tuple(int(x) for x in ref.rng_states()[0]), m
    assert int(env.trade_counts().sum()) > 0
    env.close()


# ------------------------------------------------------------------ 5. shard, warm, checkpoints
def test_a_shard_with_its_local_rows_equals_the_slice_of_the_full_env(bk):
    B, k, n = 1024, 384, 256
    rows = het_rows("doc", B, seed=3)
    full = make_env(bk, B, 256)
    full.set_agents_per_book(rows)
    full.run(T)
    shard = make_env(bk, n, 256, book_offset=k)
    shard.set_agents_per_book(rows[k:k + n])
    shard.run(T)
    assert np.array_equal(full.flags()[k:k + n], shard.flags())
    assert np.array_equal(full.history()[:, k:k + n], shard.history())
    assert np.array_equal(full.trade_counts()[k:k + n], shard.trade_counts())
    assert [full.rng_state(k + b) for b in range(n)] == [shard.rng_state(b) for b in range(n)]
    full.close()
    shard.close()


@pytest.mark.parametrize("mode", ["fused", "split", "split_wave", "wave_split"])
def test_warm_changes_nothing(bk, mode):
    B = 320
    rows = het_rows("four", B, seed=9)
    outs = []
    for warm in (False, True):
        env = make_env(bk, B, 512)
        env.set_agents_per_book(rows)
        env.set_pipeline(mode)
        if warm:
            env.warm(7)
        env.run(T)
        outs.append(P.snapshot(env, books=range(0, B, 17)))
        env.close()
    P.assert_same(outs[0], outs[1])


def test_checkpoint_continues_and_refuses_another_table(bk):
    B = 512
    rows = het_rows("doc", B, seed=13)
    a = make_env(bk, B, 256)
    a.set_agents_per_book(rows)
    a.run(12)
    img = a.checkpoint()
    a.run(T - 12)
    b = make_env(bk, B, 256)
    b.set_agents_per_book(rows)
    b.restore(img)
    b.run(T - 12)
    assert np.array_equal(a.history(12, T - 12), b.history(12, T - 12))
    assert np.array_equal(a.trade_counts(), b.trade_counts())
    assert [a.rng_state(i) for i in range(B)] == [b.rng_state(i) for i in range(B)]
    other = [list(r) for r in rows]
    kind, start, n, p = other[200][1]
    other[200][1] = (kind, start, n, dict(p, trade_vol=p["trade_vol"] + 1))
    c = make_env(bk, B, 256)
    c.set_agents_per_book(other)
    with pytest.raises(bk.BourseError, match="different agent set"):
        c.restore(img)
    u = make_env(bk, B, 256)
    u.set_agents(rows[0])  # (the uniform set of row 0 is not the table either)
    with pytest.raises(bk.BourseError, match="different agent set"):
        u.restore(img)
    for e in (a, b, c, u):
        e.close()


# ------------------------------------------------------------------ 6. refusals and replacement
def test_refusals_keep_the_installed_agents_and_a_uniform_call_replaces_the_table(bk):
    from bourse_amd import _lib

    B = 256
    rows = het_rows("doc", B, seed=17)

    def bad(u, i, **kw):
        t = [list(r) for r in rows]
        kind, start, n, p = t[u][i]
        t[u][i] = (kw.pop("kind", kind), start, kw.pop("n", n), dict(p, **kw))
        return t

    cases = [(bad(40, 1, price_dist_sigma=-1.0), _lib.BK_INVALID, "unit 40, member 1: LogNormal"),
             (bad(41, 0, tick_size=3), _lib.BK_PRICE, "unit 41, member 0"),
             (bad(42, 1, n=21), _lib.BK_INVALID, "unit 42, member 1: n_agents differs"),
             (bad(43, 0, kind="noise", p_limit=0.1, p_market=0.1), _lib.BK_INVALID, "unit 43, member 0: type differs"),
             ([rows[0] * 3 for _ in range(B)], _lib.BK_INVALID, "at most 4 members")]
    ref = make_env(bk, B, 256)
    ref.set_agents_per_book(rows)
    ref.run(T)
    want = P.snapshot(ref, books=range(0, B, 11))
    ref.close()
    env = make_env(bk, B, 256)
    env.set_agents_per_book(rows)
    for table, code, msg in cases:
        with pytest.raises((bk.BourseError, ValueError)) as ei:  # (BK_PRICE_NOT_TICK_MULTIPLE is a ValueError)
            env.set_agents_per_book(table)
        assert getattr(ei.value, "code", _lib.BK_PRICE) == code and isinstance(ei.value, bk.BourseError) == (code != _lib.BK_PRICE), msg
        assert msg in str(ei.value), str(ei.value)
    env.run(T)
    P.assert_same(want, P.snapshot(env, books=range(0, B, 11)))
    env.close()
    # a logging env refuses the table as set_agents refuses such members
    lg = bk.ManyBookEnv(B, SEED, 0, TICK, STEP, True, levels=LEVELS, max_live_orders=256, max_orders=256 * T,
                        trade_capacity=8 * 256 * T, history_capacity=T)
    lg.set_random_agents([(64, (32, 64), (10, 20), 2, 0.8)])
    lg.enable_agent_order_log()
    with pytest.raises(bk.BourseError, match="cannot be installed on a logging env"):
        lg.set_agents_per_book(rows)
    lg.close()
    # a later set_agents replaces the table: the env is uniform again
    outs = []
    for first_table in (False, True):
        e = make_env(bk, B, 256)
        if first_table:
            e.set_agents_per_book(rows)
        e.set_agents(rows[5])
        e.run(T)
        outs.append(P.snapshot(e, books=range(0, B, 13)))
        e.close()
    P.assert_same(outs[0], outs[1])


def test_an_all_random_table_is_the_random_table(bk):
    B, pool = 256, 128
    r = np.random.default_rng(5)
    rows = [[("random", 50, (lo, lo + int(r.integers(2, 300))), (1, 30), 2, float(r.random()))] for lo in r.integers(5, 90, B)]
    outs = []
    for members in (True, False):
        env = make_env(bk, B, pool)
        if members:
            env.set_agents_per_book(rows)
        else:
            env.set_random_agents_per_book([[m[1:] for m in row] for row in rows])
        env.run(T)
        outs.append(P.snapshot(env, books=range(0, B, 7)))
        env.close()
    P.assert_same(outs[0], outs[1])
