"""GPU parity tests: the HIP path (through the C ABI) against the CPU oracle, bit-exact.

Everything here needs a real MI355X (``-m gpu``).  Inputs are seeded identically on both
sides: book b's RNG is ``seed_from_u64(seed + b)``; outputs compared: level-2 history
(every step, every book), trade records (order, times, prices, vols, fill ids), RNG state,
order/trade counts and the resting orders in priority order.
"""
import os

import numpy as np
import pytest

import oracle_parity as P

pytestmark = pytest.mark.gpu

C2_GROUPS = [(32, (40, 56), (10, 20), 2, 0.8), (32, (40, 56), (50, 70), 2, 0.2)]
C3_GROUPS = [(64, (32, 64), (10, 20), 2, 0.8), (64, (32, 64), (50, 70), 2, 0.2)]
C5_GROUPS = [(256, (100, 164), (10, 20), 2, 0.8), (256, (100, 164), (50, 70), 2, 0.2)]  # §8d C5 stand-in


@pytest.fixture(scope="module")
def bk():
    import bourse_amd

    return bourse_amd


def test_dpp_reductions(bk):
    import ctypes as C

    L = bk._lib.load()
    rng = np.random.default_rng(5)
    n = 64
    x = rng.integers(0, 2**32, size=(n, 64), dtype=np.uint32)
    x[0] = 7
    x[1] = np.arange(64)
    x[2] = np.arange(64)[::-1]
    x[3, 17] = 0
    x[4, 63] = 2**32 - 1
    out = np.zeros((n, 4), dtype=np.uint32)
    bk._lib.check(L.bk_selftest_reduce(bk._lib.p32(x), n, bk._lib.p32(out)))
    assert np.array_equal(out[:, 0], x.min(axis=1))
    assert np.array_equal(out[:, 1], x.max(axis=1))
    assert np.array_equal(out[:, 2], x.sum(axis=1, dtype=np.uint64).astype(np.uint32))
    assert np.all(out[:, 3] == 32 * 1 + 32 * 2)


def _compare_random(bk, oracle, n_books, groups, levels, n_steps, seed=101, tick=2, step_size=100_000, chunks=None,
                    max_live=None, trade_cap=None, pipeline="fused", lookahead=None, wave_parts=0):
    n_agents = sum(g[0] for g in groups)
    if chunks:
        n_steps = sum(chunks)
    env = bk.ManyBookEnv(n_books, seed, 0, tick, step_size, True, levels=levels,
                         max_live_orders=max_live or n_agents, trade_capacity=trade_cap or 2 * n_agents * n_steps,
                         history_capacity=n_steps)
    env.set_random_agents(groups)
    if lookahead is not None:
        env.set_wave_options(lookahead, wave_parts)
    for i, c in enumerate(chunks or [n_steps]):
        # "mixed": alternate the kernel pipelines between launches — they share the device state
        env.set_pipeline(("fused", "wave", "split", "wave_split")[i % 4] if pipeline == "mixed" else pipeline)
        env.run(c)
    ref = oracle.ManyBooks(n_books, seed, 0, tick, step_size, True, levels, groups)
    ref.run(n_steps, n_threads=4)

    P.no_flags(env)
    hist = env.history()
    P.same_history(hist, ref.history())
    assert np.array_equal(env.level2(), hist[-1])
    assert np.array_equal(env.trade_counts(), ref.trade_counts())
    want_rng = ref.rng_states()
    for b in range(n_books):
        assert env.rng_state(b) == (int(want_rng[b, 0]), int(want_rng[b, 1])), f"rng state book {b}"
        assert env.time(b) == n_steps * step_size
    for b in sorted(set(x for x in (0, 1, n_books // 2, n_books - 1) if x < n_books)):
        P.same_book(env, b, ref.book(b))  # (trades; resting orders in price-time priority per side)
    env.close()
    return hist


# one wave per book for everything / RNG phases one lane per book + event kernel / RNG phases one wave per book with the
# wave-parallel stream decode (k_agents_wave) + event kernel
PIPELINES = ["fused", "split", "wave_split", "wave"]


@pytest.mark.parametrize("pipeline", PIPELINES)
def test_random_agents_c2_shape(bk, oracle, pipeline):
    _compare_random(bk, oracle, n_books=96, groups=C2_GROUPS, levels=16, n_steps=40, pipeline=pipeline)


@pytest.mark.parametrize("pipeline", PIPELINES)
def test_random_agents_c3_shape(bk, oracle, pipeline):
    _compare_random(bk, oracle, n_books=200, groups=C3_GROUPS, levels=32, n_steps=40, pipeline=pipeline)


@pytest.mark.parametrize("pipeline", PIPELINES)
def test_random_agents_c5_shape_deep_book(bk, oracle, pipeline):
    _compare_random(bk, oracle, n_books=8, groups=C5_GROUPS, levels=64, n_steps=12, pipeline=pipeline)


@pytest.mark.parametrize("pipeline", PIPELINES)
def test_random_agents_reference_bench_workload(bk, oracle, pipeline):
    # the reference's own divan bench parameters scaled down (crates/step_sim/benches/benchmarks.rs:14-23):
    # env tick 1, agents tick 2, two groups with different windows; 10 L2 levels
    groups = [(100, (40, 60), (10, 20), 2, 0.8), (100, (10, 90), (50, 70), 2, 0.2)]
    _compare_random(bk, oracle, n_books=5, groups=groups, levels=10, n_steps=60, tick=1, step_size=1_000_000,
                    pipeline=pipeline)


@pytest.mark.parametrize("pipeline", PIPELINES)
def test_random_agents_edge_shapes(bk, oracle, pipeline):
    # single agent, odd counts, rate 0 and rate 1 groups, empty group, books not a multiple of 4 or 64
    _compare_random(bk, oracle, n_books=3, groups=[(1, (10, 20), (20, 30), 1, 1.0)], levels=10, n_steps=25, tick=1,
                    step_size=1000, pipeline=pipeline)
    _compare_random(bk, oracle, n_books=7, groups=[(5, (10, 14), (1, 3), 3, 0.0), (37, (10, 14), (1, 3), 3, 1.0),
                                                   (23, (9, 13), (1, 2), 6, 0.5)], levels=4, n_steps=50, tick=3,
                    pipeline=pipeline)
    _compare_random(bk, oracle, n_books=67, groups=[(0, (10, 14), (1, 3), 1, 0.5), (2, (10, 12), (1, 2), 1, 0.9),
                                                    (0, (10, 14), (1, 3), 1, 0.5)], levels=3, n_steps=40, tick=1,
                    step_size=10, pipeline=pipeline)


@pytest.mark.parametrize("pipeline", PIPELINES)
def test_zero_volume_orders_rest_without_trading(bk, oracle, pipeline):
    """Volume ranges that start at 0: a new order of volume 0 matches nothing and rests (place_order's `while order.vol > 0`,
    orderbook.rs:429 / :462), a resting one is "filled" by the first aggressor with a zero-volume trade.  The keyed event loop
    only tests for it in steps that hold such an order (event_asm.hpp EK_VCHK): both of its variants run here, on 64-, 128-
    and 256-slot pools."""
    _compare_random(bk, oracle, n_books=9, groups=[(40, (10, 16), (0, 3), 1, 0.9), (24, (12, 18), (0, 2), 1, 0.7)], levels=8,
                    n_steps=60, tick=1, pipeline=pipeline)
    _compare_random(bk, oracle, n_books=5, groups=[(70, (10, 16), (0, 2), 1, 0.9), (50, (12, 18), (3, 9), 1, 0.7)], levels=8,
                    n_steps=50, tick=1, pipeline=pipeline)
    _compare_random(bk, oracle, n_books=3, groups=[(200, (10, 30), (0, 4), 2, 0.8)], levels=16, n_steps=30, tick=2,
                    pipeline=pipeline)


@pytest.mark.parametrize("pipeline", PIPELINES + ["mixed"])
def test_chunked_launches_equal_one_launch(bk, oracle, pipeline):
    a = _compare_random(bk, oracle, n_books=16, groups=C2_GROUPS, levels=16, n_steps=30, chunks=[1, 2, 3, 24],
                        pipeline=pipeline)
    b = _compare_random(bk, oracle, n_books=16, groups=C2_GROUPS, levels=16, n_steps=30)
    assert np.array_equal(a, b)


@pytest.mark.parametrize("pipeline", ["wave_split", "wave"])
@pytest.mark.parametrize("lookahead", [1, 2, 7, 33])
def test_wave_decode_slow_path_small_lookahead(bk, oracle, lookahead, pipeline):
    """k_agents_wave resolves a placement on its vector path only if its side / tick / vol draws end inside the
    look-ahead; otherwise draw by draw on the scalar path.  A tiny look-ahead sends most placements there: the
    results must not change (nor across launch chunkings, which restart from the cached lane states)."""
    _compare_random(bk, oracle, n_books=70, groups=C3_GROUPS, levels=32, n_steps=30, pipeline=pipeline, lookahead=lookahead,
                    chunks=[1, 4, 25])
    _compare_random(bk, oracle, n_books=9, groups=[(5, (10, 14), (1, 3), 3, 0.0), (37, (10, 14), (1, 3), 3, 1.0),
                                                    (23, (9, 13), (1, 2), 6, 0.5)], levels=4, n_steps=40, tick=3,
                    pipeline=pipeline, lookahead=lookahead)


def test_wave_decode_many_parts_and_odd_batches(bk, oracle):
    # more parts than the default, book counts that are not multiples of 4 (the workgroup holds four books)
    for nb, parts in ((5, 2), (130, 3), (257, 8)):
        _compare_random(bk, oracle, n_books=nb, groups=C2_GROUPS, levels=16, n_steps=16, pipeline="wave_split", lookahead=64,
                        wave_parts=parts)
        _compare_random(bk, oracle, n_books=nb, groups=C2_GROUPS, levels=16, n_steps=16, pipeline="wave")
    # every agent acts every step (rate 1): the longest streams, group boundaries in every window
    for pipe in ("wave_split", "wave"):
        _compare_random(bk, oracle, n_books=33, groups=[(100, (10, 100), (1, 2), 1, 1.0), (28, (50, 51), (5, 6), 1, 1.0)],
                        levels=10, n_steps=25, tick=1, pipeline=pipe)


def test_book_offset_sharding_is_seed_transparent(bk):
    # books [4, 12) of a 16-book run equal an 8-book env created with book_offset=4 (multi-GPU sharding rule)
    full = bk.ManyBookEnv(16, 101, 0, 2, 100_000, levels=16, max_live_orders=64, trade_capacity=4096, history_capacity=20)
    full.set_random_agents(C2_GROUPS)
    full.run(20)
    part = bk.ManyBookEnv(8, 101, 0, 2, 100_000, levels=16, max_live_orders=64, trade_capacity=4096, history_capacity=20,
                          book_offset=4)
    part.set_random_agents(C2_GROUPS)
    part.run(20)
    assert np.array_equal(full.history()[:, 4:12], part.history())
    s_full, s_part = full.stats(), part.stats()
    assert s_part["n_books"] == 8 and s_full["n_books"] == 16
    assert s_part["sum_trades"] == int(part.trade_counts().sum())


def test_trade_capacity_overflow_is_flagged_not_silent(bk, oracle):
    env = bk.ManyBookEnv(4, 101, 0, 2, 100_000, levels=16, max_live_orders=64, trade_capacity=8, history_capacity=30)
    env.set_random_agents(C2_GROUPS)
    with pytest.raises(bk.CapacityError, match="TRADE_OVERFLOW"):  # strict (default): a synchronous run() raises
        env.run(30)
    assert (env.flags() & 2).all()
    total, base = env.trade_count(0)
    assert total > 8 and base == 0
    with pytest.raises(bk.CapacityError):
        env.trades(0, first=0)
    assert len(env.trades(0, first=0, n=8)) == 8
    # only RECORDS are lost: the books, the counts and the retained records are still the oracle's
    ref = oracle.ManyBooks(4, 101, 0, 2, 100_000, True, 16, C2_GROUPS)
    ref.run(30, 2)
    assert np.array_equal(env.history(), ref.history())
    assert np.array_equal(env.trade_counts(), ref.trade_counts())
    for b in range(4):
        P.same_records(env.trades(b, first=0, n=8), ref.book(b).trades_array()[:8], (b,), "trade")
    # a reported bit moves to the host-side record (flags() still shows it; the device summary reads 0 again) and a book
    # that overflows AGAIN is reported AGAIN - a caller that caught the first error is not left with silent losses
    assert env.flags_summary()[0] == 0
    with pytest.raises(bk.CapacityError, match="TRADE_OVERFLOW"):
        env.run(5)  # (the L2 history is a ring of the last 30 steps: stepping on is fine; the trade buffer is still full)
    assert (env.flags() & 2).all()
    env.clear_trades()
    env.clear_flags(2)  # handled: cleared on the device and in the host-side record
    P.no_flags(env)
    with pytest.raises(bk.CapacityError, match="TRADE_OVERFLOW"):
        env.run(10)
    first, n = env.history_len()
    assert (first, n) == (15, 30)
    with pytest.raises(bk.BourseError):
        env.history(first_step=0, n_steps=3)  # ... reading a step that was overwritten is an error, never stale data


# ------------------------------------------------------------------- host-driven path (C ABI Env methods)
def test_kat_env_three_steps_on_gpu(bk):  # SURVEY C.11, ref crates/step_sim/src/env.rs:312-368
    env = bk.core.StepEnv(101, 0, 1, 1000)
    env.place_order(True, 10, 101, 10)
    env.place_order(False, 20, 101, 20)
    env.step()
    assert env.bid_ask == (10, 20) and [env.order_status(i) for i in range(2)] == [1, 1] and env.time == 1000
    env.place_order(True, 10, 101, 11)
    env.place_order(False, 20, 101, 21)
    env.step()
    assert env.bid_ask == (11, 20) and env.time == 2000
    env.place_order(True, 30, 101, None)
    env.step()
    assert env.bid_ask == (11, 21) and env.ask_vol == 10 and env.time == 3000
    assert env.order_status(1) == 2 and env.order_status(4) == 2 and len(env.get_trades()) == 2
    bids, asks = env.get_prices()
    assert bids.tolist() == [10, 11, 11] and asks.tolist() == [20, 20, 21]
    bv, av = env.get_volumes()
    assert bv.tolist() == [10, 20, 20] and av.tolist() == [20, 40, 10]
    tb, ta = env.get_touch_volumes()
    assert tb.tolist() == [10, 10, 10] and ta.tolist() == [20, 20, 10]
    cb, ca = env.get_touch_order_counts()
    assert cb.tolist() == [1, 1, 1] and ca.tolist() == [1, 1, 1]
    assert env.get_trade_volumes().tolist() == [0, 0, 30]


def test_kat_python_step_env_on_gpu(bk):  # SURVEY C.12, ref tests/test_step_sim/test_env.py:7-115
    env = bk.core.StepEnv(101, 0, 1, 100_000)
    env.place_order(True, 100, 101, price=50)
    env.place_order(False, 100, 101, price=60)
    env.step()
    assert env.bid_ask == (50, 60) and (env.ask_vol, env.bid_vol, env.time) == (100, 100, 100_000)
    env.place_order(True, 100, 101, price=55)
    env.place_order(False, 100, 101, price=65)
    env.step()
    assert env.bid_ask == (55, 60) and (env.ask_vol, env.bid_vol, env.time) == (200, 200, 200_000)
    env.place_order(True, 150, 101)
    env.step()
    assert env.bid_ask == (55, 65) and (env.ask_vol, env.bid_vol, env.time) == (50, 200, 300_000)
    env.step()
    d = env.get_market_data()
    assert len(d) == 45
    assert d["bid_price"].tolist() == [50, 55, 55, 55] and d["ask_price"].tolist() == [60, 60, 65, 65]
    assert d["bid_vol"].tolist() == [100, 200, 200, 200] and d["ask_vol"].tolist() == [100, 200, 50, 50]
    assert d["bid_vol_0"].tolist() == [100] * 4 and d["ask_vol_0"].tolist() == [100, 100, 50, 50]
    assert d["n_bid_0"].tolist() == [1] * 4 and d["n_ask_0"].tolist() == [1] * 4
    assert d["trade_vol"].tolist() == [0, 0, 150, 0]
    bad = bk.core.StepEnv(101, 0, 2, 100_000)
    with pytest.raises(ValueError, match="Price 21 was not a multiple of tick-size 2"):
        bad.place_order(True, 100, 101, price=21)


def test_kat_numpy_api_on_gpu(bk):  # SURVEY C.13, ref tests/test_step_sim/test_numpy_api.py:7-71
    env = bk.core.StepEnvNumpy(101, 0, 1, 100_000)
    sides = np.array([True, True, True, False, False, False])
    vols = np.array([10, 11, 12, 10, 11, 12], dtype=np.uint32)
    tr = np.array([1, 1, 1, 2, 2, 2], dtype=np.uint32)
    prices = np.array([20, 20, 19, 22, 22, 23], dtype=np.uint32)
    ids = env.submit_limit_orders((sides, vols, tr, prices))
    env.step()
    assert ids.tolist() == list(range(6))
    assert env.level_1_data().tolist() == [0, 20, 22, 33, 33, 21, 2, 21, 2]
    l2 = env.level_2_data()
    assert l2.shape == (45,) and l2[:13].tolist() == [0, 20, 22, 33, 33, 21, 2, 21, 2, 12, 1, 12, 1] and not l2[13:].any()
    env.submit_cancellations(np.array([0, 1, 3, 4], dtype=np.uint64))
    env.step()
    l1 = env.level_1_data()
    assert (l1[1], l1[2]) == (19, 23) and (l1[5], l1[6]) == (12, 1) and (l1[7], l1[8]) == (12, 1)
    bad = bk.core.StepEnvNumpy(101, 0, 2, 100_000)
    with pytest.raises(ValueError):
        bad.submit_limit_orders((sides[:2], vols[:2], tr[:2], np.array([20, 21], dtype=np.uint32)))


def test_runner_with_deterministic_agents_on_gpu(bk):  # ref tests/test_step_sim/test_env.py:118-145, test_numpy_api.py:85-120
    class A(bk.step_sim.agents.BaseAgent):
        def __init__(self, side, start):
            self.side, self.start, self.k = side, start, 0

        def update(self, _rng, env):
            env.place_order(self.side, 10, 101, price=self.start + self.k if self.side else self.start - self.k)
            self.k += 1

    data = bk.step_sim.run(bk.core.StepEnv(101, 0, 1, 100_000), [A(True, 10), A(False, 50)], 10, 101, show_progress=False)
    assert data["bid_price"].tolist() == list(range(10, 20)) and data["ask_price"].tolist() == list(range(50, 40, -1))
    assert data["bid_vol"].tolist() == [10 * k for k in range(1, 11)] and data["ask_vol"].tolist() == [10 * k for k in range(1, 11)]
    assert data["bid_vol_0"].tolist() == [10] * 10 and data["trade_vol"].tolist() == [0] * 10

    class N(bk.step_sim.agents.BaseNumpyAgent):
        def __init__(self, side, start):
            self.side, self.start, self.k = side, start, 0

        def update(self, _rng, _l2):
            p = self.start + self.k if self.side else self.start - self.k
            self.k += 1
            return (np.array([1], dtype=np.uint32), np.array([self.side]), np.array([10], dtype=np.uint32),
                    np.array([101], dtype=np.uint32), np.array([p], dtype=np.uint32), np.array([0], dtype=np.uint64))

    data = bk.step_sim.run(bk.core.StepEnvNumpy(101, 0, 1, 100_000), [N(True, 10), N(False, 50)], 10, 101,
                           show_progress=False, use_numpy=True)
    assert data["bid_price"].tolist() == list(range(10, 20)) and data["ask_price"].tolist() == list(range(50, 40, -1))


def _random_host_stream(env_gpu, env_ref, seed, n_steps, n_traders=24, tick=2, with_modify=True):
    """Drive both envs with the same pseudo-random mix of limit/market/cancel/modify instructions."""
    rng = np.random.default_rng(seed)
    ids = []
    for _ in range(n_steps):
        for _k in range(int(rng.integers(0, n_traders))):
            u = rng.random()
            if u < 0.55 or not ids:
                side = bool(rng.integers(0, 2))
                vol = int(rng.integers(0, 40))  # includes zero-volume orders (App. A quirk)
                price = None if rng.random() < 0.1 else int(rng.integers(40, 60)) * tick
                a = env_gpu.place_order(side, vol, 7, price)
                b = env_ref.place_order(side, vol, 7, price)
                assert a == b
                ids.append(a)
            elif u < 0.8:
                i = int(rng.choice(ids))
                env_gpu.cancel_order(i)
                env_ref.cancel_order(i)
            elif with_modify:
                i = int(rng.choice(ids))
                np_ = None if rng.random() < 0.4 else int(rng.integers(40, 60)) * tick
                nv = None if rng.random() < 0.3 else int(rng.integers(0, 50))
                env_gpu.modify_order(i, np_, nv)
                env_ref.modify_order(i, np_, nv)
        if rng.random() < 0.05:
            env_gpu.disable_trading()
            env_ref.disable_trading()
        elif rng.random() < 0.3:
            env_gpu.enable_trading()
            env_ref.enable_trading()
        env_gpu.step()
        env_ref.step()
        assert np.array_equal(env_gpu.level_2_data_array(), env_ref.level_2_data_array())
    return ids


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_host_driven_random_stream_matches_oracle(bk, oracle, seed):
    g = bk.core.StepEnv(seed, 0, 2, 100_000)
    r = oracle.StepEnv(seed, 0, 2, 100_000)
    _random_host_stream(g, r, seed, n_steps=60)
    assert g.get_trades() == r.get_trades()
    assert g.get_orders() == r.get_orders()
    dg, dr = g.get_market_data(), r.get_market_data()
    assert set(dg) == set(dr)
    for k in dr:
        assert np.array_equal(dg[k], dr[k]), k
    assert g._env.rng_state(0) == tuple(int(x) for x in r.rng_state())


def test_c1_random_trades_plumbing_on_gpu(bk, oracle):
    # BASELINE config 1: examples/random_trades.py run(101, 200, 50) — Python RandomAgents over StepEnv
    def agents(mod):
        return [mod.RandomAgent(i, 0.5, (10, 100), (20, 50), 2) for i in range(50)]

    g = bk.core.StepEnv(101, 0, 2, 100_000)
    dg = bk.step_sim.run(g, agents(bk.step_sim.agents), 200, 101, show_progress=False)
    # same agents over the oracle env (duck-typed: the agent only calls order_status/cancel/place)
    r = oracle.StepEnv(101, 0, 2, 100_000)
    rng = np.random.default_rng(101)
    ags = agents(bk.step_sim.agents)
    for _ in range(200):
        for a in ags:
            a.update(rng, r)
        r.step()
    dr = r.get_market_data()
    for k in dr:
        assert np.array_equal(dg[k], dr[k]), k
    assert g.get_trades() == r.get_trades()
    assert g.get_orders() == r.get_orders()


# ------------------------------------------------------------------- committed golden fixtures (no oracle needed)
def _golden(name):
    import os

    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name))


def test_golden_c1_instruction_stream_on_gpu(bk):
    """Replay the instruction stream the REFERENCE's Python RandomAgents emitted (examples/random_trades.py,
    run(101, 200, 50)) through the GPU StepEnv; outputs must equal the committed fixture."""
    fx = _golden("c1_random_trades.npz")
    env = bk.core.StepEnv(101, 0, 2, 100_000)
    ins = fx["instructions"]
    k = 0
    for s in range(200):
        while k < len(ins) and ins[k, 0] == s:
            _, action, bid, vol, trader, price, oid = (int(x) for x in ins[k])
            if action == 1:
                assert env.place_order(bool(bid), vol, trader, price=price) == oid
            else:
                env.cancel_order(oid)
            k += 1
        env.step()
    assert k == len(ins)
    md = env.get_market_data()
    for key, v in md.items():
        assert np.array_equal(v, fx[f"md_{key}"]), key
    assert np.array_equal(np.array(env.get_trades(), dtype=np.uint64), fx["trades"])
    assert np.array_equal(np.array(env.get_orders(), dtype=np.uint64), fx["orders"])


def test_golden_numpy_agents_on_gpu(bk):
    fx = _golden("numpy_random_agents.npz")
    env = bk.core.StepEnvNumpy(101, 0, 2, 100_000)
    for s in range(40):
        i = fx["instructions"][s]
        ids = env.submit_instructions((i[0].astype(np.uint32), i[1].astype(bool), i[2].astype(np.uint32),
                                       i[3].astype(np.uint32), i[4].astype(np.uint32), i[5]))
        assert ids.tolist() == list(range(30 * s, 30 * s + 30))
        env.step()
    for key, v in env.get_market_data().items():
        assert np.array_equal(v, fx[f"md_{key}"]), key
    assert np.array_equal(np.array(env.get_trades(), dtype=np.uint64), fx["trades"])


def test_golden_on_device_random_agents(bk):
    fx = _golden("oracle_random_agents_c2x4.npz")
    env = bk.ManyBookEnv(4, 101, 0, 2, 100_000, levels=16, max_live_orders=64, trade_capacity=4096, history_capacity=25)
    env.set_random_agents(C2_GROUPS)
    env.run(25)
    assert np.array_equal(env.history(), fx["history"])
    assert np.array_equal(env.trade_counts(), fx["trade_counts"])
    assert [env.rng_state(b) for b in range(4)] == [tuple(int(x) for x in r) for r in fx["rng"]]
    P.same_records(env.trades(0, first=0), fx["trades0"], (0,), "trade")


# ------------------------------------------------------------------- full-size structural properties (headline shape)
def test_full_size_invariants_c3(bk):
    """65 536 books x 128 agents x 32 levels: properties that need no oracle at this size."""
    B, T = 65536, 12
    env = bk.ManyBookEnv(B, 101, 0, 2, 100_000, levels=32, max_live_orders=128, trade_capacity=128 * T, history_capacity=T)
    env.set_random_agents(C3_GROUPS)
    env.run(T)
    P.no_flags(env)
    h = env.history()                                  # [T, B, 133]
    lv = h[:, :, 5:].reshape(T, B, 32, 4)
    # touch level is never empty on a non-empty side; level sums never exceed the side total
    assert np.all((h[:, :, 4] == 0) == (lv[:, :, 0, 1] == 0))
    assert np.all((h[:, :, 3] == 0) == (lv[:, :, 0, 3] == 0))
    assert np.all(lv[:, :, :, 0].sum(axis=2) <= h[:, :, 4]) and np.all(lv[:, :, :, 2].sum(axis=2) <= h[:, :, 3])
    # with a 32-tick price window and 32 levels/side the ladder is exact: level sums EQUAL the side totals
    assert np.array_equal(lv[:, :, :, 0].sum(axis=2), h[:, :, 4]) and np.array_equal(lv[:, :, :, 2].sum(axis=2), h[:, :, 3])
    # an uncrossed book after every step; prices inside the agents' window
    both = (h[:, :, 4] > 0) & (h[:, :, 3] > 0)
    assert np.all(h[:, :, 1][both] < h[:, :, 2][both])
    assert np.all(h[:, :, 1][h[:, :, 4] > 0] >= 64) and np.all(h[:, :, 2][h[:, :, 3] > 0] < 128)
    # per-step trade volume equals the sum of that step's trade records (checksum of checksums), sampled books
    tc = env.trade_counts()
    for b in (0, 1, 4097, 32768, 65535):
        tr = env.trades(b, first=0)
        assert len(tr) == tc[b]
        step = (tr["t"] // 100_000).astype(np.int64)
        vol_by_step = np.bincount(step, weights=tr["vol"].astype(np.float64), minlength=T)[:T]
        assert np.array_equal(vol_by_step.astype(np.uint32), h[:, b, 0])
        assert np.all(np.diff(tr["t"].astype(np.int64)) >= 0)          # records in processing order
        assert np.all(tr["active_id"] != tr["passive_id"])
    # books 0..63 equal a small run (independence of the batch size)
    small = bk.ManyBookEnv(64, 101, 0, 2, 100_000, levels=32, max_live_orders=128, trade_capacity=128 * T, history_capacity=T)
    small.set_random_agents(C3_GROUPS)
    small.run(T)
    assert np.array_equal(small.history(), h[:, :64])
    st = env.stats()
    assert st["n_books"] == B and st["sum_trades"] == int(tc.sum()) and st["sum_trade_vol"] == int(h[-1, :, 0].sum())


# ------------------------------------------------------------------- immediate-mode OrderBook on the GPU
def test_order_book_python_suite_on_gpu(bk):
    """The reference's tests/test_order_book.py vectors on bourse_amd.core.OrderBook."""
    MAXP = bk.MAX_PRICE
    ob = bk.core.OrderBook(0, 1)                                          # test_order_book_init :6-15
    assert ob.bid_ask() == (0, MAXP) and (ob.bid_vol(), ob.ask_vol()) == (0, 0)
    assert ob.best_bid_vol_and_orders() == (0, 0) and ob.best_ask_vol_and_orders() == (0, 0)
    ob.place_order(True, 10, 11, price=50)                                # test_place_order :18-42
    ob.place_order(False, 20, 12, price=60)
    assert ob.bid_ask() == (50, 60) and (ob.bid_vol(), ob.ask_vol()) == (10, 20)
    assert ob.best_bid_vol_and_orders() == (10, 1) and ob.best_ask_vol_and_orders() == (20, 1)
    ob.place_order(True, 10, 11, price=55)
    ob.place_order(False, 20, 12, price=65)
    assert ob.bid_ask() == (55, 60) and (ob.bid_vol(), ob.ask_vol()) == (20, 40)
    assert (ob.best_bid_vol(), ob.best_ask_vol()) == (10, 20)
    bad = bk.core.OrderBook(0, 2)                                         # test_incorrect_order_price :45-52
    with pytest.raises(ValueError):
        bad.place_order(True, 10, 101, price=11)

    ob = bk.core.OrderBook(0, 1)                                          # test_cancel_order :54-88
    ids = [ob.place_order(True, 10, 11, price=50), ob.place_order(False, 20, 12, price=60),
           ob.place_order(True, 10, 11, price=55), ob.place_order(False, 20, 12, price=65)]
    ob.cancel_order(ids[2])
    ob.cancel_order(ids[3])
    assert ob.order_status(ids[2]) == 3 and ob.order_status(ids[3]) == 3
    assert ob.bid_ask() == (50, 60) and (ob.bid_vol(), ob.ask_vol()) == (10, 20)
    ob.cancel_order(ids[0])
    ob.cancel_order(ids[1])
    assert ob.bid_ask() == (0, MAXP) and ob.best_bid_vol_and_orders() == (0, 0) and ob.best_ask_vol_and_orders() == (0, 0)

    ob = bk.core.OrderBook(0, 1)                                          # test_trades :91-135 (C.14)
    ob.place_order(True, 10, 11, price=50)
    id1 = ob.place_order(False, 20, 12, price=60)
    id2 = ob.place_order(True, 10, 11, price=55)
    id3 = ob.place_order(False, 20, 12, price=65)
    ob.set_time(10)
    id4 = ob.place_order(True, 30, 11)
    assert ob.order_status(id4) == 2 and ob.order_status(id1) == 2
    assert ob.bid_ask() == (55, 65) and (ob.bid_vol(), ob.ask_vol()) == (20, 10)
    ob.set_time(20)
    id5 = ob.place_order(False, 20, 12, price=55)
    assert ob.order_status(id5) == 1 and ob.order_status(id2) == 2
    assert ob.bid_ask() == (50, 55) and (ob.bid_vol(), ob.ask_vol()) == (10, 20)
    tr = ob.get_trades()
    assert [t[0] for t in tr] == [10, 10, 20] and [t[2] for t in tr] == [60, 65, 55] and [t[3] for t in tr] == [20, 10, 10]
    assert [t[4] for t in tr] == [id4, id4, id5] and [t[5] for t in tr] == [id1, id3, id2]

    ob = bk.core.OrderBook(0, 1)                                          # test_mod_order_volume :138-154
    ob.place_order(True, 10, 11, price=50)
    i1 = ob.place_order(True, 10, 11, price=55)
    i2 = ob.place_order(False, 20, 12, price=65)
    ob.place_order(False, 20, 12, price=60)
    ob.modify_order(i1, new_vol=5)
    ob.modify_order(i2, new_vol=10)
    assert ob.bid_ask() == (55, 60) and (ob.bid_vol(), ob.ask_vol()) == (15, 30) and (ob.best_bid_vol(), ob.best_ask_vol()) == (5, 20)
    ob = bk.core.OrderBook(0, 1)                                          # test_modify_order :157-169
    a = ob.place_order(True, 10, 11, price=50)
    ob.place_order(False, 30, 11, price=60)
    ob.modify_order(a, new_price=45, new_vol=20)
    assert ob.bid_ask() == (45, 60) and (ob.bid_vol(), ob.ask_vol()) == (20, 30) and ob.order_status(a) == 1
    o = ob.get_orders()                                                   # test_get_orders :172-187 (tuple layout)
    assert [x[0] for x in o] == [True, False] and [x[8] for x in o] == [0, 1] and [x[6] for x in o] == [45, 60]


def test_order_book_rust_kats_on_gpu(bk):
    """orderbook.rs unit vectors needing immediate mode: C.7 crossing modify, C.8 sweep, C.9 market edge cases."""
    MAXP = bk.MAX_PRICE
    b = bk.core.OrderBook(0, 1)                                           # C.7 orderbook.rs:1145-1168
    b.place_order(False, 10, 0, 100)
    b.place_order(True, 10, 0, 50)
    b.modify_order(1, 100, 20)
    assert (b.ask_vol(), b.best_ask_vol_and_orders()) == (0, (0, 0)) and (b.bid_vol(), b.best_bid_vol_and_orders()) == (10, (10, 1))
    assert b.bid_ask() == (100, MAXP)
    t = b.get_trades()
    assert len(t) == 1 and (t[0][2], t[0][3]) == (100, 10)
    b = bk.core.OrderBook(0, 1)                                           # C.8 orderbook.rs:1171-1214
    for t_, (bid, vol, price) in enumerate([(False, 101, 20), (False, 101, 18), (True, 202, 12), (True, 202, 14)]):
        b.set_time(t_)
        b.place_order(bid, vol, 101, price)
    b.set_time(4)
    b.place_order(True, 102, 101, None)
    assert b.ask_vol() == 100 and b.bid_ask() == (14, 20)
    tr = b.get_trades()
    assert [(x[2], x[3]) for x in tr] == [(18, 101), (20, 1)]
    b.place_order(False, 204, 101, 14)
    assert (b.bid_vol(), b.ask_vol()) == (202, 102) and b.best_bid_vol_and_orders() == (202, 1) and b.best_ask_vol_and_orders() == (2, 1)
    assert b.bid_ask() == (12, 14)
    tr = b.get_trades()
    assert (tr[2][2], tr[2][3]) == (14, 202) and [x[4] for x in tr] == [4, 4, 5] and [x[5] for x in tr] == [1, 0, 3]
    b = bk.core.OrderBook(0, 1, False)                                    # C.9 orderbook.rs:1217-1227
    b.place_order(True, 101, 101, None)
    assert b.bid_ask() == (0, MAXP) and b.order_status(0) == 4
    b = bk.core.OrderBook(0, 1)                                           # C.9 orderbook.rs:1230-1242
    b.place_order(False, 10, 101, 50)
    b.place_order(True, 20, 101, None)
    assert b.bid_ask() == (0, MAXP) and (b.bid_vol(), b.ask_vol()) == (0, 0) and b.order_status(1) == 3


def test_host_driven_many_books_match_oracle(bk, oracle):
    """B > 1 on the host-driven path: every book gets its own instruction stream and its own shuffle RNG."""
    B, T = 5, 25
    env = bk.ManyBookEnv(B, 77, 0, 1, 1000, levels=10, max_live_orders=256, max_orders=4096, trade_capacity=4096,
                         history_capacity=T)
    refs = [oracle.StepEnv(77 + b, 0, 1, 1000) for b in range(B)]
    rng = np.random.default_rng(9)
    for _ in range(T):
        for b in range(B):
            for _k in range(int(rng.integers(0, 12))):
                bid, vol, price = bool(rng.integers(0, 2)), int(rng.integers(1, 30)), int(rng.integers(90, 110))
                assert env.place_order(b, bid, vol, b, price) == refs[b].place_order(bid, vol, b, price)
            n = refs[b].book.n_orders()
            if n and rng.random() < 0.5:
                i = int(rng.integers(0, n))
                env.cancel_order(b, i)
                refs[b].cancel_order(i)
        env.step()
        for r in refs:
            r.step()
    h = env.history()
    for b in range(B):
        assert np.array_equal(h[:, b], refs[b].history()), b
        P.same_book(env, b, refs[b].book, orders=True)


def test_checkpoint_restore_continues_bit_identically(bk):
    def mk():
        e = bk.ManyBookEnv(48, 5, 0, 2, 100_000, levels=16, max_live_orders=64, trade_capacity=8192, history_capacity=40)
        e.set_random_agents(C2_GROUPS)
        return e

    a = mk()
    a.run(15)
    ck = a.checkpoint()
    a.run(25)
    b = mk()
    b.restore(ck)
    assert b.steps_done() == 15
    b.set_pipeline("split")
    b.run(25)
    assert np.array_equal(a.history()[15:], b.history())
    assert np.array_equal(a.trade_counts(), b.trade_counts())
    assert [a.rng_state(i) for i in range(48)] == [b.rng_state(i) for i in range(48)]
    ta, tb = a.trades(3, first=0), b.trades(3)
    assert np.array_equal(ta[len(ta) - len(tb):], tb)
    with pytest.raises(bk.BourseError):
        bk.ManyBookEnv(4, 5, 0, 2, 100_000, levels=16, max_live_orders=64).restore(ck)


# ------------------------------------------------------------------- NoiseAgent / MomentumAgent on the device (§8f rank 1)
NOISE_P = dict(tick_size=2, p_limit=0.2, p_market=0.2, p_cancel=0.1, trade_vol=100, price_dist_mu=0.0, price_dist_sigma=1.0)
MOM_P = dict(tick_size=2, p_cancel=0.1, trade_vol=100, decay=1.0, demand=5.0, scale=0.5, order_ratio=1.0,
             price_dist_mu=0.0, price_dist_sigma=10.0)  # the reference's doc example, crates/step_sim/src/lib.rs:53-73


def _compare_members(bk, oracle, n_books, members, levels, n_steps, tick=1, step_size=1_000_000, seed=101, pool=256,
                     chunks=None, pipeline="fused"):
    env = bk.ManyBookEnv(n_books, seed, 0, tick, step_size, True, levels=levels, max_live_orders=pool,
                         trade_capacity=64 * n_steps * 8, history_capacity=n_steps)
    env.set_agents(members)
    for i, c in enumerate(chunks or [n_steps]):
        # fused = k_run_mixed; split = k_agents_mixed_lanes + k_step_batch per step; split_wave = k_agents_mixed + k_step_batch;
    # "mixed" cycles through the three between launches (they share the device state; the lane kernel's lists are rebuilt)
        # wave_split = k_agents_mixed_wave (wave-parallel decode of the members' streams) + k_step_batch
        env.set_pipeline(("fused", "wave_split", "split", "split_wave")[i % 4] if pipeline == "mixed" else pipeline)
        env.run(c)
    ref = oracle.ManyBooks(n_books, seed, 0, tick, step_size, True, levels, members=members)
    ref.run(n_steps, 2)
    P.no_flags(env)
    hist = env.history()
    P.same_history(hist, ref.history())
    assert np.array_equal(env.trade_counts(), ref.trade_counts())
    want_rng = ref.rng_states()
    for b in range(n_books):
        assert env.rng_state(b) == (int(want_rng[b, 0]), int(want_rng[b, 1])), b
    for b in (0, n_books - 1):
        P.same_book(env, b, ref.book(b))
    assert int(ref.trade_counts().sum()) > 0
    env.close()
    return hist


@pytest.mark.parametrize("pipeline", ["fused", "split", "split_wave", "wave_split"])
def test_noise_agents_on_device(bk, oracle, pipeline):
    _compare_members(bk, oracle, 24, [("noise", 0, 20, NOISE_P)], levels=10, n_steps=80, pipeline=pipeline)
    _compare_members(bk, oracle, 5, [("noise", 3, 50, dict(NOISE_P, p_limit=0.6, p_market=0.1, p_cancel=0.3, price_dist_sigma=2.5,
                                                           price_dist_mu=1.0, tick_size=4))], levels=16, n_steps=60, tick=2,
                     pipeline=pipeline)


def test_momentum_and_noise_doc_example_on_device(bk, oracle):
    # crates/step_sim/src/lib.rs:37-88: MomentumAgent(0, 10) + NoiseAgent(10, 20), Env::new(0, 1, 1_000_000, true), seed 101
    members = [("momentum", 0, 10, MOM_P), ("noise", 10, 20, NOISE_P)]
    a = _compare_members(bk, oracle, 16, members, levels=10, n_steps=50)
    b = _compare_members(bk, oracle, 16, members, levels=10, n_steps=50, chunks=[7, 1, 42])
    c = _compare_members(bk, oracle, 16, members, levels=10, n_steps=50, pipeline="split")
    d = _compare_members(bk, oracle, 16, members, levels=10, n_steps=50, chunks=[7, 1, 20, 3, 9, 10], pipeline="mixed")
    e = _compare_members(bk, oracle, 16, members, levels=10, n_steps=50, pipeline="split_wave")
    f = _compare_members(bk, oracle, 16, members, levels=10, n_steps=50, pipeline="wave_split")
    g = _compare_members(bk, oracle, 16, members, levels=10, n_steps=50, chunks=[7, 1, 42], pipeline="wave_split")
    assert np.array_equal(a, b) and np.array_equal(a, c) and np.array_equal(a, d) and np.array_equal(a, e)
    assert np.array_equal(a, f) and np.array_equal(a, g)


def test_mixed_random_noise_momentum_set_on_device(bk, oracle):
    members = [("random", 40, (1073741800, 1073741840), (10, 20), 2, 0.5), ("noise", 0, 30, dict(NOISE_P, p_limit=0.4)),
               ("momentum", 100, 25, dict(MOM_P, demand=8.0, scale=0.01, decay=0.5)), ("noise", 200, 10, dict(NOISE_P, price_dist_sigma=3.0))]
    _compare_members(bk, oracle, 12, members, levels=32, n_steps=60, tick=2, pool=512)
    _compare_members(bk, oracle, 12, members, levels=32, n_steps=60, tick=2, pool=512, chunks=[11, 20, 10, 4, 15], pipeline="mixed")
    _compare_members(bk, oracle, 70, members, levels=32, n_steps=60, tick=2, pool=512, pipeline="split")
    _compare_members(bk, oracle, 70, members, levels=32, n_steps=60, tick=2, pool=512, pipeline="wave_split")


def test_mixed_members_split_pipeline_in_parts(bk, oracle):
    # enough books for the multi-part staggered launch of k_agents_mixed + k_step_batch
    members = [("momentum", 0, 10, MOM_P), ("noise", 10, 20, NOISE_P)]
    _compare_members(bk, oracle, 12300, members, levels=10, n_steps=8, pool=128, pipeline="split")


def test_c5_as_written_momentum_plus_noise_512_agents(bk, oracle):
    # BASELINE configs[4]: 512 momentum + "market-maker" (= NoiseAgent, the reference has no market maker) agents, 64 levels
    members = [("momentum", 0, 256, dict(MOM_P, demand=20.0)), ("noise", 256, 256, dict(NOISE_P, p_limit=0.3, p_cancel=0.2))]
    _compare_members(bk, oracle, 6, members, levels=64, n_steps=40, pool=512)
    _compare_members(bk, oracle, 6, members, levels=64, n_steps=40, pool=512, pipeline="split")
    _compare_members(bk, oracle, 6, members, levels=64, n_steps=40, pool=512, pipeline="split_wave")
    _compare_members(bk, oracle, 6, members, levels=64, n_steps=40, pool=512, pipeline="wave_split")
    _compare_members(bk, oracle, 37, members, levels=64, n_steps=40, pool=512, chunks=[9, 1, 10, 5, 15], pipeline="mixed")


@pytest.mark.parametrize("seed", range(10))
def test_fuzz_random_agent_configs_vs_oracle(bk, oracle, seed):
    """Randomly drawn RandomAgents sets (group counts/sizes, windows, volumes incl. tiny ranges, rates incl. 0/1, ticks,
    level depth, batch size) on a randomly chosen pipeline, against the oracle."""
    rng = np.random.default_rng(1000 + seed)
    tick = int(rng.choice([1, 2, 5]))
    n_groups = int(rng.integers(1, 5))
    groups, total = [], 0
    for _ in range(n_groups):
        n = int(rng.integers(0, 90))
        lo = int(rng.integers(1, 200))
        w = int(rng.integers(1, 40))
        vlo = int(rng.integers(1, 100))
        vw = int(rng.integers(1, 60))
        rate = float(rng.choice([0.0, 1.0, rng.random()]))
        tsz = tick * int(rng.integers(1, 4))
        if os.environ.get("BOURSE_FUZZ_PRICE_TOP"):  # scripts/fuzz_parts.py: price windows ending at the top of u32
            lo = (2**32 - 2) // tsz - w - (lo % 3)
        if seed % 11 == 3 and not groups:  # (no extra draw: the seeds keep their configurations) volumes from 0: orders that
            vlo = 0                          # match nothing and rest - the event loop's checked variant (event_asm.hpp EK_VCHK)
        groups.append((n, (lo, lo + w), (vlo, vlo + vw), tsz, rate))
        total += n
    if total == 0:
        groups[0] = (7,) + groups[0][1:]
        total = 7
    n_books = int(rng.integers(1, 150)) * int(os.environ.get("BOURSE_FUZZ_BOOKS_SCALE", "1"))
    levels = int(rng.integers(1, 65))
    n_steps = int(rng.integers(5, 40))
    step_size = max(int(rng.choice([300, 100_000])), total + 1)  # events per step < step_size (App. A.9)
    book_seed = int(rng.integers(0, 2**40))
    rng.choice(["fused", "split", "mixed"])  # (round 1 drew the pipeline here; kept so that the seeds keep their configurations)
    chunks = None if rng.random() < 0.5 else [3, 1, 1]
    # the pipeline and the wave decode's look-ahead rotate with the seed: every configuration family meets every pipeline
    pipeline = ("fused", "split", "mixed", "wave_split", "wave")[seed % 5]
    _compare_random(bk, oracle, n_books=n_books, groups=groups, levels=levels, n_steps=n_steps, tick=tick, step_size=step_size,
                    seed=book_seed, pipeline=pipeline, chunks=chunks, max_live=max(64, total),
                    lookahead=(64, 64, 3, 64, 17, 64, 1)[seed % 7])


def test_two_envs_interleaved_on_the_shared_part_streams(bk, oracle):
    """The parts' streams are process-wide (one set per device): two envs launching multi-part pipelines alternately,
    without synchronising in between, queue behind each other on them and still get their own results."""
    T, chunks = 12, [5, 4, 3]
    a = bk.ManyBookEnv(4096, 11, 0, 2, 100_000, True, levels=32, max_live_orders=128, trade_capacity=128 * T, history_capacity=T)
    b = bk.ManyBookEnv(6144, 12, 0, 2, 100_000, True, levels=32, max_live_orders=128, trade_capacity=128 * T, history_capacity=T)
    a.set_random_agents(C3_GROUPS); b.set_random_agents(C3_GROUPS)
    a.set_pipeline("wave_split"); a.set_wave_options(64, 2)
    b.set_pipeline("split"); b.set_split_parts(3, 2048)
    for c in chunks:
        a.run(c, sync=False)
        b.run(c, sync=False)
    for env, seed, n in ((a, 11, 4096), (b, 12, 6144)):
        ref = oracle.ManyBooks(n, seed, 0, 2, 100_000, True, 32, C3_GROUPS)
        ref.run(T, n_threads=8)
        P.no_flags(env)
        assert np.array_equal(env.history(), ref.history())
        assert np.array_equal(env.trade_counts(), ref.trade_counts())


# The keyed event loop (event_asm.hpp) packs price-time priority into one 32-bit key per order and falls back to the
# two-reduction loop whenever a step's prices or arrival stamps do not fit the key's fields.  Steps on either side of
# that test, and runs that cross it back and forth:
KEYED_CASES = {
    # two price windows farther apart than the 15-bit price field: every step with orders from both takes the fallback
    "wide": dict(groups=[(40, (1, 30), (1, 20), 1, 0.6), (40, (70000, 70030), (1, 20), 1, 0.6)], n_steps=40, n_books=9),
    # the span sits right at the field's limit (32 762 since the signed keys): steps flip between the two loops as orders
    # come and go
    "edge": dict(groups=[(30, (2, 5), (1, 20), 1, 0.5), (30, (32761, 32768), (1, 20), 1, 0.5),
                         (20, (15000, 15010), (5, 9), 1, 0.9)], n_steps=60, n_books=9),
    # prices 1 and 2 at the bottom: the price field starts at 2 (1 is the market ask's), so a step with an order at
    # price 1 takes the fallback and the others the keyed loop
    "low": dict(groups=[(30, (1, 3), (1, 20), 1, 0.3), (40, (2, 6), (1, 20), 1, 0.7)], n_steps=60, n_books=9),
    # prices at the top of u32 (the window test must not wrap)
    "top": dict(groups=[(40, (2**32 - 40, 2**32 - 1), (1, 20), 1, 0.7), (30, (2**32 - 30, 2**32 - 2), (1, 9), 1, 0.9)],
                n_steps=40, n_books=9),
    # arrival stamps: ten sleepers (one action per ~2 000 steps) hold their deep bids while 124 busy agents rest ~25 orders
    # per step, so the span of the live stamps passes the 16-bit field after ~2 600 steps and comes back when they cancel
    "age": dict(groups=[(10, (1, 3), (1, 5), 1, 0.0005), (62, (40, 60), (1, 30), 1, 1.0), (62, (50, 70), (1, 30), 1, 1.0)],
                n_steps=8000, n_books=3),
}


@pytest.mark.parametrize("pipeline", ["split", "wave"])
@pytest.mark.parametrize("case", sorted(KEYED_CASES))
def test_keyed_event_loop_window_and_fallback(bk, oracle, case, pipeline):
    c = KEYED_CASES[case]
    n_agents = sum(g[0] for g in c["groups"])
    _compare_random(bk, oracle, n_books=c["n_books"], groups=c["groups"], levels=16, n_steps=c["n_steps"], tick=1,
                    seed=4242, pipeline=pipeline, max_live=max(64, n_agents), trade_cap=n_agents * c["n_steps"])


def test_history_ring_and_streaming_egress(bk, oracle):
    """History ring: the last N steps are retained across launches and pipelines; streamed chunks equal the oracle."""
    B, T, chunk = 40, 36, 6
    env = bk.ManyBookEnv(B, 9, 0, 2, 100_000, levels=16, max_live_orders=64, trade_capacity=64 * T, history_capacity=2 * chunk)
    env.set_random_agents(C2_GROUPS)
    ref = oracle.ManyBooks(B, 9, 0, 2, 100_000, True, 16, C2_GROUPS)
    ref.run(T, 2)
    want = ref.history()
    got = {}
    env.set_pipeline("split")
    stats = env.stream_history(T, chunk, on_chunk=lambda first, arr: got.__setitem__(first, arr.copy()))
    assert sorted(got) == list(range(0, T, chunk)) and stats["bytes"] == T * B * env.width * 4
    for first, arr in got.items():
        assert np.array_equal(arr, want[first:first + chunk]), first
    first, n = env.history_len()
    assert (first, n) == (T - 2 * chunk, 2 * chunk)
    assert np.array_equal(env.history(), want[T - 2 * chunk:])  # wrapped read of the ring
    env.set_pipeline("fused")
    env.run(5)
    ref.run(5, 1)
    assert np.array_equal(env.history(), ref.history()[T + 5 - 2 * chunk:])


# ------------------------------------------------------------------ MarketEnv mode
def test_kat_market_env_on_gpu(bk):  # ref crates/step_sim/src/market_env.rs:342-407
    MAXP = 2**32 - 1
    env = bk.ManyMarketEnv(1, 101, 0, [1, 1], 1000, levels=10, max_live_orders=64, max_orders=64, trade_capacity=64,
                           history_capacity=8)
    env.place_order(0, 0, True, 10, 101, 10)
    env.place_order(0, 0, False, 20, 101, 20)
    env.step()
    l2 = env.level2()
    assert (l2[0, 1], l2[0, 2]) == (10, 20) and (l2[1, 1], l2[1, 2]) == (0, MAXP)
    o = env.orders(0)
    assert len(o) == 2 and list(o["status"]) == [1, 1]
    assert env.time(0) == env.time(1) == 1000
    env.place_order(0, 0, True, 10, 101, 11)
    env.place_order(0, 0, False, 20, 101, 21)
    env.step()
    l2 = env.level2()
    assert (l2[0, 1], l2[0, 2]) == (11, 20) and (l2[1, 1], l2[1, 2]) == (0, MAXP)
    assert len(env.orders(0)) == 4 and env.time(1) == 2000
    env.place_order(0, 0, True, 30, 101, None)
    env.step()
    l2 = env.level2()
    assert (l2[0, 1], l2[0, 2]) == (11, 21) and (l2[0, 3], l2[1, 3]) == (10, 0)
    o = env.orders(0)
    assert len(o) == 5 and o["status"][1] == 2 and o["status"][4] == 2
    assert len(env.trades(0, first=0)) == 2 and len(env.trades(1, first=0)) == 0
    h = env.history()[:, 0]
    assert list(h[:, 1]) == [10, 11, 11] and list(h[:, 2]) == [20, 20, 21]   # prices
    assert list(h[:, 4]) == [10, 20, 20] and list(h[:, 3]) == [20, 40, 10]   # volumes
    assert list(h[:, 5]) == [10, 10, 10] and list(h[:, 7]) == [20, 20, 10]   # touch volumes
    assert list(h[:, 6]) == [1, 1, 1] and list(h[:, 8]) == [1, 1, 1]         # touch order counts
    assert list(h[:, 0]) == [0, 0, 30]                                       # trade vols
    with pytest.raises(ValueError):
        bk.ManyMarketEnv(1, 1, 0, [1, 3], 1000, max_orders=8).place_order(0, 1, True, 1, 0, 10)  # tick of asset 1


def _compare_markets(bk, oracle, n_markets, ticks, groups, levels, n_steps, seed=101, step_size=100_000, chunks=None):
    A = len(ticks)
    n_agents = sum(g[1] for g in groups)
    env = bk.ManyMarketEnv(n_markets, seed, 0, ticks, step_size, True, levels=levels, max_live_orders=n_agents,
                           trade_capacity=2 * n_agents * n_steps, history_capacity=n_steps)
    env.set_random_market_agents(groups)
    for c in (chunks or [n_steps]):
        env.run(c)
    ref = oracle.ManyMarkets(n_markets, seed, 0, ticks, step_size, True, levels, groups)
    ref.run(n_steps, n_threads=4)
    P.no_flags(env)
    hist = env.history()
    P.same_history(hist, ref.history())
    assert np.array_equal(env.level2(), hist[-1])
    want_rng = ref.rng_states()
    for m in sorted(set([0, 1, n_markets // 2, n_markets - 1])):
        for a in range(A):
            b = env.book(m, a)
            assert env.rng_state(b) == (int(want_rng[m, 0]), int(want_rng[m, 1])), (m, a)
            assert env.time(b) == n_steps * step_size
            P.same_book(env, b, ref.book(m, a), tag=(m, a))
    env.close()


def test_random_market_agents_doc_example(bk, oracle):  # ref agents/random_agent.rs:146-162 (two assets, tick 1 / agents' 2)
    groups = [(0, 10, (40, 60), (10, 20), 2, 0.8), (1, 10, (40, 60), (10, 20), 2, 0.8)]
    _compare_markets(bk, oracle, 64, [1, 1], groups, 10, 40, step_size=1_000_000)


def test_random_market_agents_three_assets_mixed_ticks(bk, oracle):
    # several groups per asset, an asset nobody trades, per-asset tick sizes, launches in chunks
    groups = [(0, 40, (30, 50), (10, 20), 4, 0.7), (2, 33, (20, 40), (5, 9), 3, 0.9), (0, 20, (30, 50), (50, 70), 2, 0.3),
              (2, 35, (22, 38), (1, 4), 6, 0.5)]
    _compare_markets(bk, oracle, 70, [2, 5, 3], groups, 16, 30, chunks=[1, 12, 17])


def test_random_market_agents_large_batch_parts(bk, oracle):
    # enough books for a staggered launch in at least three parts (>= 12 288 books)
    groups = [(0, 24, (40, 56), (10, 20), 2, 0.8), (1, 24, (40, 56), (10, 20), 2, 0.8), (1, 16, (40, 56), (50, 70), 2, 0.2)]
    _compare_markets(bk, oracle, 6200, [2, 2], groups, 16, 12)


@pytest.mark.parametrize("seed", [4, 5])
def test_market_host_driven_random_stream(bk, oracle, seed):
    """MarketEnv::place/cancel/modify across assets: ONE shuffled queue per market, events stamped t0 + global index."""
    NM, A, T = 3, 3, 20
    ticks = [1, 2, 5]
    env = bk.ManyMarketEnv(NM, 50 + seed, 0, ticks, 1000, levels=10, max_live_orders=256, max_orders=4096,
                           trade_capacity=4096, history_capacity=T)
    ref = oracle.ManyMarkets(NM, 50 + seed, 0, ticks, 1000, True, 10)
    rng = np.random.default_rng(seed)
    for _ in range(T):
        for m in range(NM):
            for _k in range(int(rng.integers(0, 25))):
                a = int(rng.integers(0, A))
                kind = rng.random()
                n = ref.book(m, a).n_orders()
                if kind < 0.65 or n == 0:
                    bid, vol = bool(rng.integers(0, 2)), int(rng.integers(1, 30))
                    price = None if rng.random() < 0.1 else int(rng.integers(18, 24)) * 5 * ticks[a]
                    assert env.place_order(m, a, bid, vol, 7, price) == ref.place_order(m, a, bid, vol, 7, price)
                elif kind < 0.85:
                    i = int(rng.integers(0, n))
                    env.cancel_order(m, a, i)
                    ref.cancel_order(m, a, i)
                else:
                    i = int(rng.integers(0, n))
                    np_ = None if rng.random() < 0.5 else int(rng.integers(18, 24)) * 5 * ticks[a]
                    nv = None if rng.random() < 0.4 else int(rng.integers(1, 30))
                    env.modify_order(m, a, i, np_, nv)
                    ref.modify_order(m, a, i, np_, nv)
        env.step()
        ref.step()
    h, want = env.history(), ref.history()
    P.same_history(h, want)
    for m in range(NM):
        for a in range(A):
            P.same_book(env, env.book(m, a), ref.book(m, a), orders=True, tag=(m, a))
    want_rng = ref.rng_states()
    for m in range(NM):
        for a in range(A):
            assert env.rng_state(env.book(m, a)) == (int(want_rng[m, 0]), int(want_rng[m, 1]))
    # Market::save_json layout (market.rs:367-377): {"order_books": [...]}; load into another market and carry on
    st = env.market_state(1)
    for a in range(A):
        v = ref.book(1, a)
        v._trading = True
        assert st["order_books"][a] == oracle.OrderBook.state(v), a
    env.load_market_state(0, st)
    assert env.market_state(0) == st
    assert np.array_equal(env.level2()[0:A], env.level2()[A:2 * A])


# ------------------------------------------------------------------ JSON snapshots (serde layout of the reference)
def _random_book_ops(rng, books, t0, n_ops):
    """The same random immediate-mode operations on every book in ``books`` (distinct times: SURVEY App. A.9)."""
    t = t0
    for _ in range(n_ops):
        t += int(rng.integers(1, 5))
        for b in books:
            b.set_time(t)
        n = len(books[0].get_orders())
        kind = rng.random()
        if kind < 0.6 or n == 0:
            args = (bool(rng.integers(0, 2)), int(rng.integers(1, 40)), int(rng.integers(0, 9)),
                    None if rng.random() < 0.1 else int(rng.integers(45, 56)) * 2)
            ids = {b.place_order(*args) for b in books}
            assert len(ids) == 1
        elif kind < 0.8:
            i = int(rng.integers(0, n))
            for b in books:
                b.cancel_order(i)
        else:
            i = int(rng.integers(0, n))
            np_ = None if rng.random() < 0.4 else int(rng.integers(45, 56)) * 2
            nv = None if rng.random() < 0.4 else int(rng.integers(1, 40))
            for b in books:
                b.modify_order(i, np_, nv)
    return t


@pytest.mark.parametrize("seed", [12, 13])
def test_json_snapshot_matches_oracle_and_round_trips(bk, oracle, tmp_path, seed):
    import json
    rng = np.random.default_rng(seed)
    g, o = bk.core.OrderBook(0, 2), oracle.OrderBook(0, 2)
    t = _random_book_ops(rng, [g, o], 0, 150)
    # the device's serde state (orders WITH their priority keys, trades, clock, trade_vol) equals the oracle's
    gp, op = tmp_path / "gpu.json", tmp_path / "orc.json"
    g.save_json_snapshot(str(gp))
    o.save_json_snapshot(str(op))
    assert json.loads(gp.read_text()) == json.loads(op.read_text())
    assert gp.read_text() == op.read_text()
    g.save_json_snapshot(str(tmp_path / "pretty.json"), pretty=True)
    assert json.loads((tmp_path / "pretty.json").read_text()) == json.loads(op.read_text())
    # cross-load: a snapshot written by either side continues identically on both
    g2 = bk.core.order_book_from_json(str(op))
    o2 = oracle.order_book_from_json(str(gp))
    for x in (g2, o2):
        assert x.bid_ask() == o.bid_ask() and x.get_orders() == o.get_orders() and x.get_trades() == o.get_trades()
        assert x.best_bid_vol_and_orders() == o.best_bid_vol_and_orders()
        assert x.best_ask_vol_and_orders() == o.best_ask_vol_and_orders()
        assert (x.bid_vol(), x.ask_vol()) == (o.bid_vol(), o.ask_vol())
    _random_book_ops(rng, [g, o, g2, o2], t, 120)
    want = o.state()
    assert o2.state() == want
    for x in (g, g2):
        x.save_json_snapshot(str(gp))
        assert json.loads(gp.read_text()) == want


def test_json_snapshot_python_reference_test(bk, tmp_path):  # ref tests/test_order_book.py:189-210
    ob = bk.core.OrderBook(0, 1)
    ob.place_order(True, 100, 101, price=50)
    ob.place_order(False, 100, 101, price=60)
    ob.place_order(True, 10, 11, price=55)
    ob.place_order(False, 20, 12, price=65)
    path = str(tmp_path / "foo.json")
    ob.save_json_snapshot(path)
    loaded_ob = bk.core.order_book_from_json(path)
    assert ob.bid_ask() == loaded_ob.bid_ask()
    assert ob.best_ask_vol_and_orders() == loaded_ob.best_ask_vol_and_orders()
    assert ob.best_bid_vol_and_orders() == loaded_ob.best_bid_vol_and_orders()
    assert ob.get_orders() == loaded_ob.get_orders()
    assert ob.get_trades() == loaded_ob.get_trades()


def test_json_golden_snapshot_loads_on_gpu(bk):
    """tests/golden/orderbook_snapshot.json: written by the oracle in the build container (make_golden.py)."""
    import json
    path = os.path.join(os.path.dirname(__file__), "golden", "orderbook_snapshot.json")
    s = json.load(open(path))
    ob = bk.core.order_book_from_json(path)
    assert ob._env.book_state(0, trading=s["trading"], trade_vol=ob.trade_vol()) == s
    act = [e["order"] for e in s["orders"] if e["order"]["status"] == "Active"]
    bids = [x["price"] for x in act if x["side"] == "Bid"]
    asks = [x["price"] for x in act if x["side"] == "Ask"]
    assert ob.bid_ask() == (max(bids, default=0), min(asks, default=2**32 - 1))


def test_trade_stream_compaction_matches_oracle(bk, oracle):
    """bk_trades_compact: every book's records as one dense CSR stream, chunk after chunk, equals the oracle's trades."""
    B, chunks = 300, [7, 1, 12, 5]
    env = bk.ManyBookEnv(B, 21, 0, 2, 100_000, levels=16, max_live_orders=64, trade_capacity=64 * max(chunks))
    env.set_random_agents(C2_GROUPS)
    ref = oracle.ManyBooks(B, 21, 0, 2, 100_000, True, 16, C2_GROUPS)
    done = np.zeros(B, dtype=np.int64)
    for i, c in enumerate(chunks):
        env.set_pipeline(("fused", "split")[i % 2])
        env.run(c)
        ref.run(c, 4)
        off, rec = env.drain_trades()
        assert off[0] == 0 and off[-1] == len(rec) and np.all(np.diff(off.astype(np.int64)) >= 0)
        want_counts = ref.trade_counts().astype(np.int64) - done
        assert np.array_equal(np.diff(off.astype(np.int64)), want_counts)
        for b in (0, 1, B // 2, B - 1):
            P.same_records(rec[int(off[b]):int(off[b + 1])], ref.book(b).trades_array()[done[b]:], (i, b), "trade")
        done += want_counts
        total, base = env.trade_count(0)
        assert total == base == done[0]  # consumed
    off, rec = env.drain_trades()
    assert len(rec) == 0 and not off.any()
    P.no_flags(env)


@pytest.mark.parametrize("shape", [(50, 24, 4, "auto"), (130, 21, 7, "split"), (3, 9, 1, "fused")])
def test_streaming_l2_and_trades_together(bk, oracle, shape):
    B, T, chunk, pipeline = shape  # T need not be a multiple of chunk: the last chunk is short
    env = bk.ManyBookEnv(B, 5, 0, 2, 100_000, levels=16, max_live_orders=64, trade_capacity=64 * chunk,
                         history_capacity=2 * chunk)
    env.set_random_agents(C2_GROUPS)
    env.set_pipeline(pipeline)
    ref = oracle.ManyBooks(B, 5, 0, 2, 100_000, True, 16, C2_GROUPS)
    ref.run(T, 2)
    want = ref.history()
    got_l2, got_tr = {}, {b: [] for b in range(B)}

    def on_chunk(first, l2, tr):
        got_l2[first] = l2.copy()
        off, rec = tr
        for b in range(B):
            got_tr[b].append(rec[int(off[b]):int(off[b + 1])].copy())

    env.stream_history(T, chunk, on_chunk=on_chunk, trades=True)
    for first, arr in got_l2.items():
        assert np.array_equal(arr, want[first:first + chunk])
    for b in range(B):
        P.same_records(np.concatenate(got_tr[b]), ref.book(b).trades_array(), (b,), "trade")
    P.no_flags(env)


def test_checkpoint_restore_with_noise_and_momentum_members(bk):
    """The checkpoint carries the books AND their latest level-2 records (the lane-per-book members' update takes the
    mid price from there); the members' lists are rebuilt from the pool after a restore."""
    members = [("momentum", 0, 10, MOM_P), ("noise", 10, 20, NOISE_P)]

    def mk(pipeline):
        e = bk.ManyBookEnv(40, 9, 0, 1, 1_000_000, levels=10, max_live_orders=128, trade_capacity=4096, history_capacity=64)
        e.set_agents(members)
        e.set_pipeline(pipeline)
        return e

    a = mk("split")
    a.run(17)
    ck = a.checkpoint()
    a.run(23)
    for pipeline in ("split", "fused", "split_wave"):
        b = mk(pipeline)
        b.restore(ck)
        b.run(23)
        assert np.array_equal(a.history()[17:], b.history()), pipeline
        assert [a.rng_state(i) for i in range(40)] == [b.rng_state(i) for i in range(40)]
        assert np.array_equal(a.trade_counts(), b.trade_counts())


def _compare_market_members(bk, oracle, n_markets, ticks, members, levels, n_steps, seed=101, step_size=1_000_000, pool=256,
                            chunks=None, allow_flags=0):
    A = len(ticks)
    env = bk.ManyMarketEnv(n_markets, seed, 0, ticks, step_size, True, levels=levels, max_live_orders=pool,
                           trade_capacity=64 * n_steps * 8, history_capacity=n_steps, strict=not allow_flags)
    env.set_market_agents(members)
    for c in (chunks or [n_steps]):
        env.run(c)
    ref = oracle.ManyMarkets(n_markets, seed, 0, ticks, step_size, True, levels, members=members)
    ref.run(n_steps, 4)
    P.no_flags(env, allow=allow_flags)
    hist = env.history()
    P.same_history(hist, ref.history())
    want_rng = ref.rng_states()
    n_tr = 0
    for m in sorted(set([0, 1, n_markets // 2, n_markets - 1])):
        for a in range(A):
            b = env.book(m, a)
            assert env.rng_state(b) == (int(want_rng[m, 0]), int(want_rng[m, 1])), (m, a)
            P.same_book(env, b, ref.book(m, a), tag=(m, a))
            n_tr += ref.book(m, a).n_trades()
    assert n_tr > 0
    env.close()
    return hist


def test_noise_and_momentum_market_agents_doc_examples(bk, oracle):
    # ref noise_agent.rs:196-222 (NoiseMarketAgent::new(0, 5, 0, params) on MarketEnv<1>) and momentum_agent.rs:251-279
    a = _compare_market_members(bk, oracle, 40, [1, 1], [(0, ("noise", 0, 5, NOISE_P)), (1, ("noise", 5, 5, NOISE_P))],
                                levels=10, n_steps=60)
    b = _compare_market_members(bk, oracle, 40, [1, 1], [(0, ("noise", 0, 5, NOISE_P)), (1, ("noise", 5, 5, NOISE_P))],
                                levels=10, n_steps=60, chunks=[9, 1, 50])
    assert np.array_equal(a, b)
    m3 = [(1, ("momentum", 0, 10, MOM_P)), (1, ("noise", 10, 20, NOISE_P)), (0, ("noise", 30, 20, dict(NOISE_P, tick_size=1)))]
    _compare_market_members(bk, oracle, 33, [1, 1], m3, levels=10, n_steps=50)


def test_agent_price_clamped_off_tick_is_flagged(bk, oracle):
    """A log-normal offset (sigma 10) can push a limit price to the u32::MAX clamp, which a tick-2 book rejects: the
    reference `.unwrap()`s that Err (common.rs:107,140) and panics.  Here the order is not created (as the Err implies,
    and as the oracle does) and the book is flagged BK_FLAG_PRICE_TICK — never silent."""
    m3 = [(1, ("momentum", 0, 10, MOM_P)), (1, ("noise", 10, 20, NOISE_P)), (0, ("noise", 30, 20, dict(NOISE_P, tick_size=1)))]
    env = bk.ManyMarketEnv(33, 101, 0, [1, 2], 1_000_000, True, levels=10, max_live_orders=256, trade_capacity=64 * 50 * 8,
                           history_capacity=50)
    env.set_market_agents(m3)
    with pytest.raises(bk.BourseError, match="PRICE_TICK"):  # the reference panics here; strict envs raise after the run
        env.run(50)
    ref = oracle.ManyMarkets(33, 101, 0, [1, 2], 1_000_000, True, 10, members=m3)
    ref.run(50, 2)
    f = env.flags()
    assert (f & 64).any() and not (f & ~np.uint32(64)).any() and not (f[0::2] != 0).any()  # only tick-2 books (asset 1)
    assert np.array_equal(env.history(), ref.history())


def test_market_agent_set_all_member_kinds_three_assets(bk, oracle):
    members = [(2, ("random", 30, (1073741800, 1073741840), (10, 20), 2, 0.5)), (0, ("noise", 0, 30, dict(NOISE_P, p_limit=0.4))),
               (2, ("momentum", 100, 25, dict(MOM_P, demand=8.0, scale=0.01, decay=0.5))),
               (2, ("noise", 200, 10, dict(NOISE_P, price_dist_sigma=3.0)))]
    _compare_market_members(bk, oracle, 70, [2, 1, 1], members, levels=16, n_steps=40, pool=256, chunks=[13, 27])


# 5072: a sell limit clamped to u32::MAX off the tick grid is dropped while the book's order 0 is still Active (the oracle
# once left a bogus id 0 in the member's list for such a drop and then drew a cancel decision for order 0)
@pytest.mark.parametrize("seed", list(range(6)) + [5072])
def test_fuzz_agent_sets_and_markets_vs_oracle(bk, oracle, seed, checkpoint_at=3):
    """Randomly drawn AgentSets / MarketAgentSets (1-4 members of every kind, 1-3 assets, random parameters and tick
    sizes, random launch chunking) against the oracle.  Off-tick clamped prices may be flagged (both sides drop them)."""
    rng = np.random.default_rng(7000 + seed)
    A = int(rng.integers(1, 4))
    # scripts/fuzz_wave_members.py: only sets k_agents_mixed_wave takes (independent books, Noise / Momentum members)
    wave_members = bool(os.environ.get("BOURSE_FUZZ_WAVE_MEMBERS"))
    if wave_members:
        A = 1
    ticks = [int(rng.choice([1, 1, 2, 5])) for _ in range(A)]
    members, fixed = [], [0] * A
    for j in range(int(rng.integers(1, 5))):
        a = int(rng.integers(0, A))
        kind = rng.choice(["random", "noise", "momentum"])
        if wave_members and kind == "random":
            kind = ("noise", "momentum")[j % 2]
        tsz = ticks[a] * int(rng.integers(1, 3))
        if kind == "random":
            n = int(rng.integers(1, 40))
            lo = int(rng.integers(10_000, 20_000))
            m = ("random", n, (lo, lo + int(rng.integers(1, 30))), (1, int(rng.integers(2, 50))), tsz, float(rng.random()))
            fixed[a] += n
        elif kind == "noise":
            m = ("noise", 100 * j, int(rng.integers(1, 60)), dict(
                tick_size=tsz, p_limit=float(rng.random() * 0.6), p_market=float(rng.random() * 0.3),
                p_cancel=float(rng.random() * 0.5), trade_vol=int(rng.integers(1, 200)),
                price_dist_mu=float(rng.normal()), price_dist_sigma=float(rng.random() * 3)))
        else:
            m = ("momentum", 100 * j, int(rng.integers(1, 60)), dict(
                tick_size=tsz, p_cancel=float(rng.random() * 0.5), trade_vol=int(rng.integers(1, 200)),
                decay=float(rng.random()), demand=float(rng.random() * 20), scale=float(rng.random()),
                order_ratio=float(rng.random() * 2), price_dist_mu=float(rng.normal()), price_dist_sigma=float(rng.random() * 4)))
        members.append((a, m))
    NM, T, levels = int(rng.integers(1, 90)), int(rng.integers(5, 50)), int(rng.integers(1, 33))
    NM *= int(os.environ.get("BOURSE_FUZZ_BOOKS_SCALE", "1"))  # scripts/fuzz_parts.py: batches large enough for several parts
    chunks, left = [], T
    while left:
        c = int(rng.integers(1, left + 1))
        chunks.append(c)
        left -= c
    # pool size (registers per pool field R = pool / 64) from its own stream: seeds keep their configuration
    pool = int(np.random.default_rng(99 + seed).choice([128, 256, 512, 512]))
    def mk():
        try:
            if A == 1:
                e = bk.ManyBookEnv(NM, seed, 0, ticks[0], 1_000_000, True, levels=levels, max_live_orders=pool,
                                   trade_capacity=64 * T * 8, history_capacity=T, strict=False)
                e.set_agents([m for _, m in members])
            else:
                e = bk.ManyMarketEnv(NM, seed, 0, ticks, 1_000_000, True, levels=levels, max_live_orders=pool,
                                     trade_capacity=64 * T * 8, history_capacity=T, strict=False)
                e.set_market_agents(members)
        except bk.CapacityError:
            pytest.skip("the drawn RandomAgents members do not fit the drawn pool")
        return e

    env = mk()
    if A == 1:
        ref = oracle.ManyBooks(NM, seed, 0, ticks[0], 1_000_000, True, levels, members=[m for _, m in members])
    else:
        ref = oracle.ManyMarkets(NM, seed, 0, ticks, 1_000_000, True, levels, members=members)
    for i, c in enumerate(chunks):
        if A == 1:
            env.set_pipeline(("split", "fused", "split_wave", "wave_split")[(i + seed) % 4])
        env.run(c)
    ref.run(T, 4)
    if (env.flags() & (1 | 128)).any():  # the drawn set needs more pool slots / queue entries than drawn: reported, not comparable
        pytest.skip("capacity flagged (BK_FLAG_POOL_OVERFLOW / BK_FLAG_EVENT_OVERFLOW): configuration exceeds max_live_orders")
    P.no_flags(env, allow=64)
    want = ref.history()
    P.same_history(env.history(), want, tag=f"A={A} ticks={ticks} members={members} chunks={chunks}: L2 history")
    want_rng = ref.rng_states()
    for u in range(NM):
        assert env.rng_state(u * A) == (int(want_rng[u, 0]), int(want_rng[u, 1])), u
    if checkpoint_at is not None and len(chunks) > 1:
        # the same run interrupted by a checkpoint at a chunk boundary and continued in a FRESH env on another pipeline
        j = 1 + checkpoint_at % (len(chunks) - 1)
        a = mk()
        for i, c in enumerate(chunks[:j]):
            if A == 1:
                a.set_pipeline(("split", "fused", "split_wave", "wave_split")[(i + seed) % 4])
            a.run(c)
        ck = a.checkpoint()
        b = mk()
        b.restore(ck)
        for i, c in enumerate(chunks[j:]):
            if A == 1:
                b.set_pipeline(("fused", "wave_split", "split", "split_wave")[(i + seed) % 4])
            b.run(c)
        done = sum(chunks[:j])
        if ((a.flags() | b.flags()) & (1 | 128)).any():
            # the lane-per-book members' update keeps a filled order's slot reserved until its member's next update, so
            # it can run out of pool slots where the other pipelines just fit: flagged, not comparable
            pytest.skip("capacity flagged on the checkpoint leg's pipelines")
        assert np.array_equal(b.history(), want[done:]), f"after restore at step {done}"
        for u in range(NM):
            assert b.rng_state(u * A) == (int(want_rng[u, 0]), int(want_rng[u, 1])), u


def test_batched_submit_for_all_books_matches_per_book_calls(bk, oracle):
    """bk_submit_instructions_csr: one call queues every book's instructions (SURVEY §8b batched SoA ops)."""
    B, T = 64, 6
    a = bk.ManyBookEnv(B, 3, 0, 1, 1000, levels=10, max_live_orders=128, max_orders=4096, trade_capacity=4096, history_capacity=T)
    refs = [oracle.StepEnvNumpy(3 + b, 0, 1, 1000) for b in range(B)]
    rng = np.random.default_rng(4)
    for _ in range(T):
        counts = rng.integers(0, 20, size=B)
        off = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
        n = int(off[-1])
        action = rng.choice([0, 1, 1, 1, 2], size=n).astype(np.uint32)
        sides = rng.integers(0, 2, size=n).astype(bool)
        vols = rng.integers(1, 30, size=n).astype(np.uint32)
        traders = rng.integers(0, 9, size=n).astype(np.uint32)
        prices = rng.integers(95, 106, size=n).astype(np.uint32)
        ids = np.zeros(n, dtype=np.uint64)
        for b in range(B):  # cancels refer to ids that exist in that book
            lo, hi = int(off[b]), int(off[b + 1])
            n_orders = refs[b].book.n_orders()
            for i in range(lo, hi):
                if action[i] == 2:
                    if n_orders:
                        ids[i] = rng.integers(0, n_orders)
                    else:
                        action[i] = 0
        got = a.submit_instructions_all(off, (action, sides, vols, traders, prices, ids))
        for b in range(B):
            lo, hi = int(off[b]), int(off[b + 1])
            want = refs[b].submit_instructions((action[lo:hi], sides[lo:hi], vols[lo:hi], traders[lo:hi], prices[lo:hi], ids[lo:hi]))
            assert np.array_equal(got[lo:hi], np.asarray(want, dtype=np.uint64)), b
        a.step()
        for r in refs:
            r.step()
    h = a.history()
    for b in range(B):
        assert np.array_equal(h[:, b], refs[b].history()), b


def _same_dense_trades(env, ref, B):
    """EVERY book's trade records (t, side, price, vol, both ids): the device compacts the books' buffers into one dense
    CSR stream (bk_trades_compact, which consumes them), the oracle's per-book vectors are concatenated.  Returns their number."""
    off, rec = env.drain_trades()
    assert np.array_equal(np.diff(off), ref.trade_counts().astype(np.uint64))
    want_rec = np.concatenate([ref.book(b).trades_array() for b in range(B)])
    assert len(rec) == len(want_rec)
    for f in rec.dtype.names:
        if not np.array_equal(rec[f], want_rec[f]):
            i = int(np.argmax(rec[f] != want_rec[f]))
            raise AssertionError(f"trade field {f} differs first at record {i} (book {int(np.searchsorted(off, i, 'right')) - 1})")
    return len(rec)


def test_full_size_c3_exact_parity_vs_oracle(bk, oracle):
    """The headline configuration itself (65 536 books x 128 agents x 32 levels, the shipped split pipeline in four
    parts): every book's level-2 history, trade count and RNG state against the oracle run on all host threads."""
    B, T = 65536, 12
    env = bk.ManyBookEnv(B, 101, 0, 2, 100_000, levels=32, max_live_orders=128, trade_capacity=64 * T, history_capacity=T)
    env.set_random_agents(C3_GROUPS)
    assert env.pipeline() == ("split", 4)
    env.run(T)
    ref = oracle.ManyBooks(B, 101, 0, 2, 100_000, True, 32, C3_GROUPS)
    ref.run(T, os.cpu_count() or 8)
    P.no_flags(env)
    P.same_history(env.history(), ref.history())
    assert np.array_equal(env.trade_counts(), ref.trade_counts())
    want = ref.rng_states()
    got = np.array([env.rng_state(b) for b in range(0, B, 97)], dtype=np.uint64)
    assert np.array_equal(got, want[::97])
    for b in (0, 21845, 43690, B - 1):  # first / last book of every part
        P.same_book(env, b, ref.book(b))
    # ... and EVERY book's trade RECORDS, all 5 M of them (was scripts/c3_fullsize_parity.py, outside the suite: VERDICT r3)
    assert _same_dense_trades(env, ref, B) == int(ref.trade_counts().sum()) > 4_000_000


def test_c_abi_argument_validation(bk):
    """Bad arguments are refused with a status code and a message (never a crash, never silently accepted)."""
    E = bk.BourseError
    for kw in (dict(n_books=0), dict(levels=0), dict(levels=65), dict(tick_size=0), dict(max_live_orders=1024), dict(device=99)):
        args = dict(n_books=4, seed=1, start_time=0, tick_size=1, step_size=1000, levels=10)
        args.update(kw)
        with pytest.raises((E, ValueError)):
            bk.ManyBookEnv(**args)
    with pytest.raises((E, ValueError)):
        bk.ManyBookEnv(10, 1, 0, 1, 1000, assets=3)        # assets must divide n_books
    with pytest.raises((E, ValueError)):
        bk.ManyBookEnv(18, 1, 0, 1, 1000, assets=9)        # at most 8 assets
    env = bk.ManyBookEnv(4, 1, 0, 2, 1000, levels=10, max_live_orders=64, max_orders=8, trade_capacity=16, history_capacity=4)
    with pytest.raises((E, IndexError, ValueError)):
        env.place_order(4, True, 1, 0, 10)                 # book out of range
    with pytest.raises(ValueError):
        env.place_order(0, True, 1, 0, 11)                 # not a tick multiple
    with pytest.raises((E, ValueError)):
        env.set_random_agents([(10, (5, 5), (1, 2), 2, 0.5)])          # empty tick range (gen_range asserts low < high)
    with pytest.raises((E, ValueError)):
        env.set_random_agents([(10, (1, 5), (1, 2), 3, 0.5)])          # agent tick not a multiple of the env tick
    with pytest.raises((E, ValueError)):
        env.set_random_agents([(40, (1, 5), (1, 2), 2, 0.5)] * 2)      # more agents than pool slots
    with pytest.raises((E, ValueError)):
        env.set_random_agents([(1, (1, 5), (1, 2), 2, 0.5)] * 9)       # more than 8 groups
    with pytest.raises((E, ValueError)):
        env.set_agents([("noise", 0, 5, dict(tick_size=2, p_limit=0.1, p_market=0.1, p_cancel=0.1, trade_vol=1,
                                             price_dist_mu=0.0, price_dist_sigma=-1.0))])  # LogNormal::new(.., sigma < 0)
    with pytest.raises((E, ValueError)):
        env.history(first_step=0, n_steps=1)               # nothing retained yet
    env.cancel_order(0, 123)                               # unknown id: reported when the event is processed
    with pytest.raises((E, IndexError, ValueError)):
        env.step()
    env2 = bk.ManyBookEnv(2, 1, 0, 1, 1000, levels=10, max_live_orders=64, max_orders=8, trade_capacity=16)
    env2.place_order(0, True, 5, 0, 10)
    with pytest.raises((E, ValueError)):
        env2.set_random_agents([(4, (1, 5), (1, 2), 1, 0.5)]) or env2.run(1)  # on-device agents cannot mix with host-driven orders
    off, rec = env2.drain_trades()                         # compaction with nothing to compact
    assert len(rec) == 0 and not off.any()
    with pytest.raises((E, ValueError)):
        env2.set_pipeline("nonsense") if False else env2._L and bk._lib.check(env2._L.bk_set_pipeline(env2._h, 7))
    # raw ABI: null arrays and ranges that wrap are refused, not dereferenced
    import ctypes as C
    L, h = env2._L, env2._h
    nd = C.c_size_t(0)
    assert L.bk_submit_instructions(h, 0, 3, None, None, None, None, None, None, None, C.byref(nd)) == bk._lib.BK_INVALID
    assert L.bk_get_orders(h, 0, 0, 1, None) == bk._lib.BK_INVALID
    assert L.bk_get_orders(h, 0, 2**64 - 1, 2, None) == bk._lib.BK_INVALID      # first + n wraps
    assert L.bk_get_trades(h, 0, 2**64 - 1, 2, None) == bk._lib.BK_INVALID
    assert L.bk_get_order_keys(h, 0, 2**64 - 1, 2, None, None) == bk._lib.BK_INVALID
    assert L.bk_rng_state(h, 0, None) == bk._lib.BK_INVALID
    assert L.bk_trade_vol(h, 0, None) == bk._lib.BK_INVALID
    assert L.bk_live_orders(h, 0, 4, None, None) == bk._lib.BK_INVALID
    assert L.bk_history(h, 2**64 - 1, 2, 0, 1, (C.c_uint32 * 64)()) == bk._lib.BK_INVALID
    assert b"null" in L.bk_last_error() or b"range" in L.bk_last_error() or b"retained" in L.bk_last_error()


@pytest.mark.parametrize("parts", [2, 3, 5, 8])
def test_split_pipeline_any_number_of_parts(bk, oracle, parts, monkeypatch):
    """The split pipeline cuts the batch into min(parts, units / min_part) contiguous parts on separate streams: the
    partition must not show in the results (RandomAgents, AgentSet members one lane per book, markets)."""
    monkeypatch.setenv("BOURSE_AMD_SPLIT_PARTS", str(parts))
    monkeypatch.setenv("BOURSE_AMD_MIN_PART", "64")
    groups = [(40, (40, 56), (10, 20), 2, 0.8), (24, (40, 56), (50, 70), 2, 0.3)]
    env = bk.ManyBookEnv(64 * parts + 37, 1, 0, 2, 100_000, levels=8, max_live_orders=64)
    env.set_random_agents(groups)
    env.set_pipeline("split")
    assert env.pipeline() == ("split", parts)
    env.close()
    _compare_random(bk, oracle, 64 * parts + 37, groups, 16, 12, pipeline="split", chunks=[5, 7])
    members = [("momentum", 0, 10, MOM_P), ("noise", 10, 20, NOISE_P)]
    _compare_members(bk, oracle, 64 * parts + 5, members, levels=10, n_steps=14, pipeline="split", chunks=[6, 8])
    mgroups = [(0, 24, (40, 56), (10, 20), 2, 0.8), (1, 24, (40, 56), (10, 20), 2, 0.8), (1, 16, (40, 56), (50, 70), 2, 0.2)]
    _compare_markets(bk, oracle, 64 * parts + 9, [2, 2], mgroups, 16, 8)


def _bulk_instructions(rng, B, N, step, n_prev):
    n = B * N
    action = np.ones(n, dtype=np.uint32)
    ids = np.zeros(n, dtype=np.uint64)
    if step:
        canc = rng.random(n) < 0.3
        action[canc] = 2
        ids[canc] = rng.integers(0, max(n_prev, 1), size=int(canc.sum()))  # ids every book has created by now
    return (action, rng.integers(0, 2, size=n).astype(bool), rng.integers(1, 30, size=n).astype(np.uint32),
            np.zeros(n, dtype=np.uint32), rng.integers(90, 111, size=n).astype(np.uint32), ids)


def test_host_threads_do_not_change_the_host_driven_path(bk, oracle, monkeypatch):
    """Large host-driven batches are spread over the env's host threads (bk_submit_instructions_csr: tick check, id
    assignment, queueing; bk_step: validation + flattening into the upload buffer).  Same ids, same books as one thread,
    and as the oracle; errors name the first offender in book order."""
    B, N, T = 2048, 40, 3
    off = np.arange(B + 1, dtype=np.uint64) * N
    envs = {}
    for nt in (1, 7):
        monkeypatch.setenv("BOURSE_AMD_HOST_THREADS", str(nt))
        env = bk.ManyBookEnv(B, 9, 0, 1, 100_000, levels=10, max_live_orders=256, max_orders=N * (T + 1),
                             trade_capacity=N * (T + 1), history_capacity=T)
        rng = np.random.default_rng(11)
        got_ids = []
        for s in range(T):
            ins = _bulk_instructions(rng, B, N, s, int(0.6 * N * s))
            got_ids.append(env.submit_instructions_all(off, ins))
            env.step()
            if nt == 1 and s == T - 1:
                last = ins
        envs[nt] = (env, got_ids)
    (e1, ids1), (e7, ids7) = envs[1], envs[7]
    for a, b in zip(ids1, ids7):
        assert np.array_equal(a, b)
    assert np.array_equal(e1.history(), e7.history())
    assert np.array_equal(e1.trade_counts(), e7.trade_counts()) and int(e1.trade_counts().sum()) > 0
    for b in (0, 1, B // 2, B - 1):
        P.same_records(e1.trades(b, first=0), e7.trades(b, first=0), (b,), "trade")
    # against the oracle: replay book b's slice of the same instruction stream
    rng = np.random.default_rng(11)
    streams = [_bulk_instructions(rng, B, N, s, int(0.6 * N * s)) for s in range(T)]
    for b in (0, 777, B - 1):
        ref = oracle.StepEnvNumpy(9 + b, 0, 1, 100_000)  # 10 levels, as bourse.core.StepEnvNumpy
        for s in range(T):
            lo, hi = b * N, (b + 1) * N
            want = ref.submit_instructions(tuple(x[lo:hi] for x in streams[s]))
            assert np.array_equal(ids7[s][lo:hi], np.asarray(want, dtype=np.uint64))
            ref.step()
        assert np.array_equal(e7.history()[:, b], ref.history()), b
    # errors: a price off the tick grid in the middle of a threaded batch stops that book's range at the offender
    e7.close()
    e1.close()
    env = bk.ManyBookEnv(B, 9, 0, 2, 100_000, levels=12, max_live_orders=256, max_orders=4 * N, trade_capacity=4 * N)
    ins = list(_bulk_instructions(np.random.default_rng(1), B, N, 0, 0))
    ins[4] = (ins[4] // 2 * 2).astype(np.uint32)
    bad = 1234 * N + 7
    ins[4][bad] = 101
    with pytest.raises(ValueError, match="101"):
        env.submit_instructions_all(off, tuple(ins))
    assert env.order_count(1234) == 7 and env.order_count(0) == N
    # ... and an unknown id in a threaded bk_step is refused before anything is uploaded or cleared
    env2 = bk.ManyBookEnv(B, 9, 0, 1, 100_000, levels=12, max_live_orders=256, max_orders=4 * N, trade_capacity=4 * N)
    ins = list(_bulk_instructions(np.random.default_rng(2), B, N, 0, 0))
    ins[0][5 * N + 3] = 2
    ins[5][5 * N + 3] = 10_000
    env2.submit_instructions_all(off, tuple(ins))
    with pytest.raises((bk.BourseError, IndexError, ValueError), match="10000"):
        env2.step()
    assert env2.steps_done() == 0


def test_host_driven_step_at_the_event_capacity_boundary(bk, oracle):
    """One step may carry up to 8192 events per book (the device-side shuffle permutation lives in LDS, sized by the
    step's longest queue): exactly 8192 is processed and matches the oracle, 8193 is refused without side effects."""
    N = 8192
    env = bk.ManyBookEnv(3, 21, 0, 1, 100_000, levels=10, max_live_orders=512, max_orders=N + 8, trade_capacity=N,
                         history_capacity=2)
    ref = oracle.StepEnvNumpy(21 + 1, 0, 1, 100_000)  # book 1 carries the big step
    rng = np.random.default_rng(5)
    # crossing flow so that the 512-slot pool never fills: alternating sides around one price, small volumes
    sides = (np.arange(N) % 2).astype(bool)
    vols = rng.integers(1, 4, size=N).astype(np.uint32)
    prices = np.where(sides, 101, 100).astype(np.uint32)   # bids at 101, asks at 100: every order finds a counterparty
    ins = (np.ones(N, dtype=np.uint32), sides, vols, np.zeros(N, dtype=np.uint32), prices, np.zeros(N, dtype=np.uint64))
    off = np.array([0, 0, N, N], dtype=np.uint64)
    got = env.submit_instructions_all(off, ins)
    want = ref.submit_instructions(ins)
    assert np.array_equal(got, np.asarray(want, dtype=np.uint64))
    env.place_order(0, True, 5, 0, 99)       # a quiet neighbour: 1 event
    env.step()
    ref.step()
    P.no_flags(env)
    assert np.array_equal(env.history()[:, 1], ref.history())
    g, e = env.trades(1, first=0), ref.get_trades()
    assert len(g) == len(e) > 1000
    assert env.rng_state(1) == tuple(int(x) for x in ref.rng_state())
    # one more than the capacity: refused, queues intact, nothing stepped
    more = tuple(np.concatenate([x, x[:1]]) for x in ins)
    env.submit_instructions_all(np.array([0, 0, N + 1, N + 1], dtype=np.uint64), more)
    with pytest.raises(bk.CapacityError):
        env.step()
    assert env.steps_done() == 1


def test_readers_on_book_and_step_windows(bk):
    """bk_history / bk_level2 on sub-ranges of books and of retained steps (strided device-to-host copies, across the
    ring's wrap point) return exactly the corresponding slices of the full reads."""
    B, cap = 37, 10
    env = bk.ManyBookEnv(B, 3, 0, 2, 100_000, levels=7, max_live_orders=64, trade_capacity=4096, history_capacity=cap)
    env.set_random_agents(C2_GROUPS)
    env.run(6)
    env.run(7)   # 13 steps done: the ring holds steps 3..12 and its wrap point lies inside the window
    first, n = env.history_len()
    assert (first, n) == (3, 10)
    full = env.history()
    assert full.shape == (10, B, env.width)
    l2 = env.level2()
    assert np.array_equal(full[-1], l2)
    rng = np.random.default_rng(0)
    for _ in range(25):
        fb = int(rng.integers(0, B)); nb = int(rng.integers(1, B - fb + 1))
        fs = int(rng.integers(first, first + n)); ns = int(rng.integers(1, first + n - fs + 1))
        got = env.history(first_step=fs, n_steps=ns, first_book=fb, n_books=nb)
        assert np.array_equal(got, full[fs - first:fs - first + ns, fb:fb + nb]), (fs, ns, fb, nb)
        assert np.array_equal(env.level2(fb, nb), l2[fb:fb + nb])
    with pytest.raises((bk.BourseError, ValueError)):
        env.history(first_step=first, n_steps=1, first_book=B - 1, n_books=2)   # book window past the end
    with pytest.raises((bk.BourseError, ValueError)):
        env.level2(B, 1)


@pytest.mark.parametrize("pipeline", ["fused", "split"])
def test_trading_disabled_with_on_device_agents(bk, oracle, pipeline):
    """With trading off nothing matches: limit orders rest (crossed books are legal), market orders are Rejected
    (orderbook.rs:526-529); toggling between launches takes effect from the next step."""
    B, T = 40, 20
    env = bk.ManyBookEnv(B, 7, 0, 2, 100_000, False, levels=16, max_live_orders=64, trade_capacity=4096, history_capacity=T)
    env.set_random_agents(C2_GROUPS)
    env.set_pipeline(pipeline)
    env.run(T)
    ref = oracle.ManyBooks(B, 7, 0, 2, 100_000, False, 16, C2_GROUPS)
    ref.run(T, 2)
    assert np.array_equal(env.history(), ref.history())
    assert int(env.trade_counts().sum()) == 0 == int(ref.trade_counts().sum())
    assert [env.rng_state(b) for b in range(B)] == [tuple(int(x) for x in r) for r in ref.rng_states()]
    # AgentSet with market orders (Rejected while trading is off), then markets toggled between launches
    members = [("momentum", 0, 10, MOM_P), ("noise", 10, 20, NOISE_P)]
    env2 = bk.ManyBookEnv(12, 7, 0, 1, 1_000_000, False, levels=10, max_live_orders=256, trade_capacity=4096, history_capacity=30)
    env2.set_agents(members)
    env2.set_pipeline(pipeline)
    env2.run(30)
    ref2 = oracle.ManyBooks(12, 7, 0, 1, 1_000_000, False, 10, members=members)
    ref2.run(30, 2)
    assert np.array_equal(env2.history(), ref2.history())
    assert [env2.rng_state(b) for b in range(12)] == [tuple(int(x) for x in r) for r in ref2.rng_states()]
    groups = [(0, 24, (40, 56), (10, 20), 2, 0.8), (1, 24, (40, 56), (10, 20), 2, 0.8)]
    m = bk.ManyMarketEnv(9, 5, 0, [2, 2], 100_000, True, levels=8, max_live_orders=64, trade_capacity=4096, history_capacity=24)
    m.set_random_market_agents(groups)
    r = oracle.ManyMarkets(9, 5, 0, [2, 2], 100_000, True, 8, groups)
    for on, steps in ((True, 6), (False, 7), (True, 5), (False, 2), (True, 4)):
        (m.enable_trading if on else m.disable_trading)()
        r.set_trading(on)
        m.run(steps)
        r.run(steps, 2)
    assert np.array_equal(m.history(), r.history())
    want_counts = np.array([len(r.book(k, a).get_trades()) for k in range(9) for a in range(2)], dtype=np.uint64)
    assert np.array_equal(m.trade_counts(), want_counts) and int(want_counts.sum()) > 0



def test_market_event_queue_overflow_is_flagged_not_silent(bk):
    """A market's books share ONE event queue of max_live_orders entries per step.  Members that queue more than that in
    a step (here ~2 x 60 noise traders on 2 assets against 64 entries) get the excess dropped and the book flagged
    BK_FLAG_EVENT_OVERFLOW; nothing is written out of bounds and the run goes on."""
    noisy = dict(NOISE_P, p_limit=0.9, p_market=0.5, tick_size=1)
    members = [(0, ("noise", 0, 60, noisy)), (1, ("noise", 100, 60, noisy))]
    env = bk.ManyMarketEnv(70, 3, 0, [1, 1], 1_000_000, True, levels=8, max_live_orders=64, trade_capacity=4096, history_capacity=4)
    env.set_market_agents(members)
    with pytest.raises(bk.CapacityError, match="EVENT_OVERFLOW"):
        env.run(6)
    f = env.flags()
    assert (f & 128).any() and not (f & ~np.uint32(1 | 64 | 128)).any(), np.unique(f)
    first, n = env.history_len()
    assert n == 4 and env.history().shape[0] == 4


# ------------------------------------------------------------------- every BASELINE config at its stated size
def _full_size_vs_oracle(bk, oracle, B, levels, T, groups=None, members=None, pool=None, trade_cap=None, pipelines=("auto",),
                         allow_flags=0, rng_stride=61, sample_books=None, book_offset=0):
    """One BASELINE configuration at its FULL size: every book's level-2 record of every step, every book's trade count,
    sampled RNG states and sampled trade streams against the oracle (all host threads).  The steps are cut into one
    launch per entry of `pipelines` (the pipelines share the device state)."""
    n_agents = sum(g[0] for g in groups) if groups else sum(m[2] for m in members)
    env = bk.ManyBookEnv(B, 101, 0, 2, 100_000, levels=levels, max_live_orders=pool or min(n_agents, 512),
                         trade_capacity=trade_cap or n_agents * T, history_capacity=T, strict=False, book_offset=book_offset)
    # (a shard's book b is the job's book book_offset + b: seeded 101 + book_offset + b, runner.rs:53)
    if groups:
        env.set_random_agents(groups)
        ref = oracle.ManyBooks(B, 101 + book_offset, 0, 2, 100_000, True, levels, groups)
    else:
        env.set_agents(members)
        ref = oracle.ManyBooks(B, 101 + book_offset, 0, 2, 100_000, True, levels, members=members)
    cuts = [T // len(pipelines)] * len(pipelines)
    cuts[-1] += T - sum(cuts)
    used = []
    for c, p in zip(cuts, pipelines):
        env.set_pipeline(p)
        used.append(env.pipeline())
        env.run(c)
    ref.run(T, os.cpu_count() or 8)
    P.no_flags(env, allow=allow_flags)
    P.same_history(env.history(), ref.history())
    assert np.array_equal(env.trade_counts(), ref.trade_counts())
    wr = ref.rng_states()
    got = np.array([env.rng_state(b) for b in range(0, B, rng_stride)], dtype=np.uint64)
    assert np.array_equal(got, wr[::rng_stride])
    for b in sample_books or (0, B // 3, B // 2, B - 1):
        P.same_book(env, b, ref.book(b))
    assert _same_dense_trades(env, ref, B) > 0
    env.close()
    return used


def test_full_size_c2_exact_parity_vs_oracle(bk, oracle):
    """BASELINE configs[1]: 4 096 books x 64 RandomAgents x 16 levels, at its size, on the pipeline bk_run
    picks by itself and on the other ones."""
    _full_size_vs_oracle(bk, oracle, 4096, 16, 18, groups=C2_GROUPS, pipelines=("auto", "split", "fused"))


@pytest.mark.parametrize("n_gpus,T", [(8, 12), (4, 2), (2, 2)])
def test_full_size_c4_shard_as_written_exact_parity_vs_oracle(bk, oracle, n_gpus, T):
    """BASELINE configs[3] as ONE RANK runs it: the LAST shard of 65 536 books x 128 agents x 32 levels cut
    over 8 / 4 / 2 GPUs (a non-zero book_offset), on the pipeline bk_run picks by itself at that shard size - every
    book's level-2 history and trade count, strided RNG states and four trade streams against the oracle seeded by
    GLOBAL book index (independent books: ref crates/step_sim/src/runner.rs:46-69)."""
    B = 65536 // n_gpus
    used = _full_size_vs_oracle(bk, oracle, B, 32, T, groups=C3_GROUPS, pipelines=("auto",), book_offset=(n_gpus - 1) * B,
                                rng_stride=53)
    assert used[0] == C4_AUTO_PIPELINE[B], used


# the auto rule at the C4 shard sizes (bourse_amd.hip bk_get_pipeline); the test above pins it so that a change of the
# thresholds is a visible decision
C4_AUTO_PIPELINE = {8192: ("wave_split", 4), 16384: ("wave_split", 4), 32768: ("split", 4)}


def test_full_size_c5_standin_exact_parity_vs_oracle(bk, oracle):
    """BASELINE configs[4] as the RandomAgents deep-book stress: 8 192 books x 512 agents x 64 levels."""
    _full_size_vs_oracle(bk, oracle, 8192, 64, 8, groups=C5_GROUPS, pipelines=("auto", "fused"), trade_cap=512 * 8)


def test_full_size_c5_as_written_exact_parity_vs_oracle(bk, oracle):
    """BASELINE configs[4] as written: 8 192 books x (256 MomentumAgent + 256 NoiseAgent) x 64 levels, the bench's
    parameters (bench.py C5M).  BK_FLAG_PRICE_TICK (a log-normal offset clamped to u32::MAX off the tick grid: the
    reference panics, the order is not created - here and in the oracle) is the one flag allowed."""
    mom = dict(tick_size=2, p_cancel=0.1, trade_vol=100, decay=1.0, demand=20.0, scale=0.5, order_ratio=1.0,
               price_dist_mu=0.0, price_dist_sigma=10.0)
    noise = dict(tick_size=2, p_limit=0.3, p_market=0.2, p_cancel=0.2, trade_vol=100, price_dist_mu=0.0, price_dist_sigma=1.0)
    _full_size_vs_oracle(bk, oracle, 8192, 64, 12, members=[("momentum", 0, 256, mom), ("noise", 256, 256, noise)],
                         pool=512, trade_cap=96 * 12, pipelines=("auto", "split_wave"), allow_flags=64, rng_stride=7)


# ------------------------------------------------------------------- capacity / mode errors are raised, never silent
def test_strict_env_raises_on_pool_overflow_in_step(bk):
    """The reference's book is unbounded; a 65th resting order in a 64-slot pool must not vanish silently: step() raises."""
    env = bk.ManyBookEnv(2, 1, 0, 1, 1000, levels=10, max_live_orders=64, max_orders=256, trade_capacity=64, history_capacity=4)
    for i in range(64):
        env.place_order(0, True, 1, 0, 10 + i)
    env.step()                                   # exactly full: fine
    env.place_order(0, True, 1, 0, 5)
    with pytest.raises(bk.CapacityError, match="POOL_OVERFLOW"):
        env.step()
    lax = bk.ManyBookEnv(1, 1, 0, 1, 1000, levels=10, max_live_orders=64, max_orders=256, trade_capacity=64, strict=False)
    for i in range(65):
        lax.place_order(0, True, 1, 0, 10 + i)
    lax.step()                                   # strict=False: the sticky flag is the report
    assert lax.flags()[0] & 1


def test_strict_env_reports_a_flag_once_and_step_size_only_warns(bk):
    """sticky flags must not make every later step() raise, and the reference's Env::step (env.rs:116-134)
    never checks the event count against step_size - BK_FLAG_STEP_SIZE is a warning."""
    env = bk.ManyBookEnv(2, 1, 0, 1, 1000, levels=10, max_live_orders=64, max_orders=256, trade_capacity=64, history_capacity=4)
    for i in range(64):
        env.place_order(0, True, 1, 0, 10 + i)
    env.step()
    env.place_order(0, True, 1, 0, 5)
    with pytest.raises(bk.CapacityError, match="POOL_OVERFLOW"):
        env.step()
    env.place_order(1, True, 1, 0, 7)
    env.step()                                   # book 0's bit was reported: stepping goes on
    assert env.flags()[0] & 1 and not env.flags()[1]
    assert env.flags_summary()[0] == 0           # reported bits live in the host-side record: the cheap poll stays cheap
    env.place_order(0, True, 1, 0, 3)            # ... and the SAME book overflowing again is reported again
    with pytest.raises(bk.CapacityError, match="POOL_OVERFLOW"):
        env.step()
    env.clear_flags()
    P.no_flags(env)
    tiny = bk.ManyBookEnv(1, 1, 0, 1, 2, levels=10, max_live_orders=64, max_orders=64, trade_capacity=64)
    for i in range(3):
        tiny.place_order(0, True, 1, 0, 10 + i)
    with pytest.warns(RuntimeWarning, match="STEP_SIZE"):
        tiny.step()                              # 3 events >= step_size 2: flagged, warned, not raised
    assert tiny.flags()[0] == 4
    assert int(tiny.level2()[0][4]) == 3
    # a workload that queues >= step_size events EVERY step (which the reference tolerates) is warned about once;
    # the warning-only bit stays on the device and is no longer polled, clear_flags() re-arms it
    import warnings

    for i in range(3):
        tiny.place_order(0, True, 1, 0, 20 + i)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        tiny.step()
    assert tiny.flags()[0] == 4 and tiny.flags_summary()[0] == 4
    tiny.clear_flags()
    for i in range(3):
        tiny.place_order(0, True, 1, 0, 30 + i)
    with pytest.warns(RuntimeWarning, match="STEP_SIZE"):
        tiny.step()


def test_reported_flag_bits_travel_with_the_python_checkpoint(bk):
    """raise_on_flags moves reported ERROR bits off the device into a host-side record; ManyBookEnv.checkpoint()
    carries that record as a trailer, so flags() reads the same after a restore into a fresh env."""
    kw = dict(levels=32, max_live_orders=128, trade_capacity=8, history_capacity=4)
    env = bk.ManyBookEnv(64, 101, 0, 2, 100_000, **kw)
    env.set_random_agents(C3_GROUPS)
    with pytest.raises(bk.CapacityError, match="TRADE_OVERFLOW"):
        env.run(4)  # ~35 trades per book-step against 8 retained records
    f = env.flags()
    assert (f & 2).any() and env.flags_summary()[0] == 0  # reported: moved to the host-side record
    img = env.checkpoint()
    assert img.nbytes == int(env._L.bk_checkpoint_bytes(env._h)) + 16 + 4 * 64
    fresh = bk.ManyBookEnv(64, 101, 0, 2, 100_000, **kw)
    fresh.set_random_agents(C3_GROUPS)
    fresh.restore(img)
    assert np.array_equal(fresh.flags(), f)
    plain = bk.ManyBookEnv(64, 101, 0, 2, 100_000, strict=False, **kw)  # an env that never reported anything: no trailer
    plain.set_random_agents(C3_GROUPS)
    plain.run(4)
    img2 = plain.checkpoint()
    assert img2.nbytes == int(plain._L.bk_checkpoint_bytes(plain._h))
    fresh.restore(img2)
    assert np.array_equal(fresh.flags(), plain.flags()) and (plain.flags() & 2).any()


def test_step_env_trades_outlive_the_device_trade_buffer(bk, oracle):
    """core.StepEnv drains the trade records into a host archive (like the level-2 history) before the
    device buffer fills: a long run returns EVERY trade, as the reference's unbounded Vec<Trade> does."""
    env = bk.core.StepEnv(7, 0, 1, 1000, trade_capacity=64, history_capacity=8)
    ref = oracle.StepEnv(7, 0, 1, 1000)
    n = 0
    for s in range(40):
        for e in (env, ref):
            e.place_order(True, 5, 1, price=100)
            e.place_order(False, 5, 2, price=100)
            e.place_order(True, 3, 3, price=101)
            e.place_order(False, 3, 4, price=99)
        env.step()
        ref.step()
    got, want = env.get_trades(), ref.get_trades()
    assert len(want) > 64 and got == want
    assert not (env._env.flags() & 2).any()


def test_bk_warm_leaves_no_trace(bk, oracle):
    """bk_warm: scratch steps of the env's own kernels; state, level-2 records, history, trades and the step counter are
    as if it had never run - before the first step and between launches, on every RandomAgents pipeline and an AgentSet."""
    for pipeline in ("auto", "split", "wave_split", "fused"):
        env = bk.ManyBookEnv(192, 101, 0, 2, 100_000, levels=32, max_live_orders=128, trade_capacity=128 * 12, history_capacity=12)
        env.set_random_agents(C3_GROUPS)
        env.set_pipeline(pipeline)
        env.warm(7)
        env.run(5)
        env.warm(3)
        env.run(7)
        ref = oracle.ManyBooks(192, 101, 0, 2, 100_000, True, 32, C3_GROUPS)
        ref.run(12, 4)
        assert env.history_len() == (0, 12)
        P.same_history(env.history(), ref.history(), tag=f"{pipeline}: L2 history")
        assert np.array_equal(env.trade_counts(), ref.trade_counts())
        P.no_flags(env)
        for b in (0, 191):
            P.same_book(env, b, ref.book(b), tag=(pipeline, b))
            assert env.rng_state(b) == tuple(int(x) for x in ref.rng_states()[b])
        env.close()


def test_bk_warm_leaves_no_trace_on_agent_sets_and_multi_part_launches(bk, oracle):
    """bk_warm on the paths bench.py relies on - an AgentSet of Noise + Momentum members on the wave-parallel
    members' decode (its lists are rebuilt from the owner tags after the roll-back, the Momentum header state is part of
    the restored block) and multi-part launches (the fork / join of the parts' streams around the snapshot and restore
    copies) - between two run() chunks, against the oracle."""
    members = [("momentum", 0, 10, MOM_P), ("noise", 10, 20, NOISE_P)]
    for pipeline, B, parts in (("auto", 4096, 2), ("wave_split", 600, 1), ("split", 4096, 1)):  # (4 096 / 2 048 = 2 parts)
        env = bk.ManyBookEnv(B, 101, 0, 1, 1_000_000, True, levels=10, max_live_orders=128, trade_capacity=64 * 14,
                             history_capacity=14)
        env.set_agents(members)
        env.set_pipeline(pipeline)
        if pipeline == "auto":
            assert env.pipeline() == ("wave_split", parts)
        env.warm(4)
        env.run(6)
        env.warm(5)
        env.run(8)
        ref = oracle.ManyBooks(B, 101, 0, 1, 1_000_000, True, 10, members=members)
        ref.run(14, 8)
        assert env.history_len() == (0, 14)
        P.no_flags(env)
        assert np.array_equal(env.history(), ref.history()), pipeline
        assert np.array_equal(env.trade_counts(), ref.trade_counts()), pipeline
        want = ref.rng_states()
        for b in (0, B // 2, B - 1):
            assert env.rng_state(b) == (int(want[b, 0]), int(want[b, 1])), (pipeline, b)
            P.same_book(env, b, ref.book(b), tag=(pipeline, b))
        env.close()
    # RandomAgents, the parts forced: 4 parts of the lane split and 3 of the wave split on 4 096 books
    for pipeline, setup in (("split", lambda e: e.set_split_parts(4, 64)), ("wave_split", lambda e: e.set_wave_options(64, 3))):
        B = 4096
        env = bk.ManyBookEnv(B, 101, 0, 2, 100_000, levels=32, max_live_orders=128, trade_capacity=128 * 10, history_capacity=10)
        env.set_random_agents(C3_GROUPS)
        env.set_pipeline(pipeline)
        setup(env)
        assert env.pipeline()[1] >= 3, env.pipeline()
        env.run(4)
        env.warm(6)
        env.run(6)
        ref = oracle.ManyBooks(B, 101, 0, 2, 100_000, True, 32, C3_GROUPS)
        ref.run(10, 8)
        assert np.array_equal(env.history(), ref.history()), pipeline
        assert np.array_equal(env.trade_counts(), ref.trade_counts()), pipeline
        P.no_flags(env)
        want = ref.rng_states()
        for b in (0, 1365, B - 1):
            assert env.rng_state(b) == (int(want[b, 0]), int(want[b, 1])), (pipeline, b)
        env.close()


def test_checkpoint_restore_marks_the_env_as_on_device_flow(bk):
    """a fresh env restored from an agents' checkpoint must refuse host-driven orders (their ids would restart
    at 0 and collide with the agents')."""
    a = bk.ManyBookEnv(4, 1, 0, 2, 1000, levels=8, max_live_orders=64, max_orders=64, trade_capacity=1024, history_capacity=4)
    a.set_random_agents(C2_GROUPS)
    a.run(3)
    img = a.checkpoint()
    b = bk.ManyBookEnv(4, 1, 0, 2, 1000, levels=8, max_live_orders=64, max_orders=64, trade_capacity=1024, history_capacity=4)
    b.set_random_agents(C2_GROUPS)
    b.restore(img)
    with pytest.raises(bk.BourseError, match="on-device agents"):
        b.place_order(0, True, 1, 0, 10)
    b.run(2)
    a.run(2)
    assert np.array_equal(a.level2(), b.level2())


def test_immediate_mode_order_book_flags_stay_clear(bk):
    """step_size 0 (immediate mode) used to raise BK_FLAG_STEP_SIZE on every call; the flags must be pollable."""
    from bourse_amd.core import OrderBook

    ob = OrderBook(0, 1)
    a = ob.place_order(True, 10, 0, price=50)
    ob.place_order(False, 10, 1, price=60)
    ob.cancel_order(a)
    assert not ob._env.flags().any()


def test_host_orders_refused_after_on_device_agents_ran(bk):
    env = bk.ManyBookEnv(4, 1, 0, 2, 1000, levels=8, max_live_orders=64, max_orders=64, trade_capacity=1024, history_capacity=4)
    env.set_random_agents(C2_GROUPS)
    env.run(3)
    for call in (lambda: env.place_order(0, True, 1, 0, 10), lambda: env.cancel_order(0, 0),
                 lambda: env.modify_order(0, 0, new_vol=1), env.step):
        with pytest.raises(bk.BourseError, match="on-device agents"):
            call()


def test_checkpoint_refuses_a_differently_configured_env(bk):
    def mk(levels=16, groups=C2_GROUPS, books=8):
        e = bk.ManyBookEnv(books, 101, 0, 2, 100_000, levels=levels, max_live_orders=64, trade_capacity=4096, history_capacity=8)
        e.set_random_agents(groups)
        return e
    a = mk()
    a.disable_trading()
    a.run(5)
    ck = a.checkpoint()
    for other in (mk(levels=8), mk(books=4), mk(groups=[(32, (40, 56), (10, 20), 2, 0.7), C2_GROUPS[1]])):
        with pytest.raises(bk.BourseError):
            other.restore(ck)
    bad = ck.copy()
    bad[0] ^= 0xFF                                # magic
    with pytest.raises(bk.BourseError, match="magic"):
        mk().restore(bad)
    b = mk()
    b.restore(ck)                                 # same shape and agents: accepted, trading flag restored with the books
    a.run(4)
    b.run(4)
    assert np.array_equal(a.level2(), b.level2()) and np.array_equal(a.trade_counts(), b.trade_counts())
    b.enable_trading()
    a.enable_trading()
    a.run(3)
    b.run(3)
    assert np.array_equal(a.level2(), b.level2()) and int(a.trade_counts().sum()) > 0


def test_step_env_history_outlives_the_device_ring(bk, oracle):
    """StepEnv keeps every step's record like the reference (data.rs:26-56): the device ring is drained before it wraps."""
    from bourse_amd.core import StepEnv

    env = StepEnv(7, 0, 1, 1000, history_capacity=4)
    ref = oracle.StepEnv(7, 0, 1, 1000)
    for k in range(11):
        for e in (env, ref):
            e.place_order(True, 5 + k, 0, price=10 + k)
            e.place_order(False, 3, 1, price=90 - k)
            e.step()
    for name in ("get_prices", "get_volumes", "get_touch_volumes", "get_trade_volumes"):
        g, w = getattr(env, name)(), getattr(ref, name)()
        g, w = (g if isinstance(g, tuple) else (g,)), (w if isinstance(w, tuple) else (w,))
        for x, y in zip(g, w):
            assert len(x) == 11 and np.array_equal(x, y), name
    assert all(np.array_equal(v, ref.get_market_data()[k]) for k, v in env.get_market_data().items())


def test_auto_pipeline_does_not_change_results_at_the_pool_capacity_edge(bk):
    """The lane-per-book members' update keeps a filled order's pool slot until its member's next update, so it overflows
    a nearly full pool where the wave-per-book kernels still fit (1 of 60 000 fuzz draws in round 1).  A pipeline chosen
    BY THE LIBRARY must not change results.  Rounds 1-2 guarded the auto-selected lane pipeline with a snapshot and a
    roll-back; since round 3 the auto choice for every AgentSet on independent books is the wave-parallel decode
    (k_agents_mixed_wave), which frees slots exactly like the fused kernel: identical results AND flags, nothing to roll
    back - with and without a RandomAgents member in the set.  Configurations found with scripts/find_capacity_edge.py."""
    B, T = 4096, 30
    worse = 0
    for n, pl, pm_, pc in ((125, 0.3, 0.2, 0.7), (120, 0.4, 0.3, 0.6)):
        P = dict(tick_size=1, p_limit=pl, p_market=pm_, p_cancel=pc, trade_vol=10, price_dist_mu=0.0, price_dist_sigma=1.0)
        for with_random in (False, True):
            # (the RandomAgents member never acts - rate 0 - but owns pool slot 0 and draws once per step)
            members = ([("random", 1, (50, 51), (1, 2), 1, 0.0)] if with_random else []) + [("noise", 0, n, P)]
            res = {}
            for pipe in ("split", "fused", "auto"):
                e = bk.ManyBookEnv(B, 11, 0, 1, 1_000_000, True, levels=8, max_live_orders=128, trade_capacity=128 * T,
                                   history_capacity=T, strict=False)
                e.set_agents(members)
                e.set_pipeline(pipe)
                if pipe == "auto":
                    assert e.pipeline()[0] == "wave_split"
                for c in (T // 3, T - T // 3):
                    e.run(c)
                res[pipe] = (e.flags() & 1, e.pipeline_fallbacks(), e.history(), e.trade_counts(), [e.rng_state(b) for b in (0, 77, B - 1)])
                e.close()
            assert res["split"][1] == 0 and res["fused"][1] == 0 and res["auto"][1] == 0
            for k in (0, 2, 3):
                assert np.array_equal(res["auto"][k], res["fused"][k]), (n, with_random, k)
            assert res["auto"][4] == res["fused"][4]
            worse += int(res["split"][0].sum()) > int(res["fused"][0].sum())
    assert worse >= 1  # the edge exists: the (explicitly requested) lane pipeline flags books the other kernels do not


def test_env_lifecycle_returns_its_device_memory(bk):
    """bk_env_destroy frees everything bk_env_create and the first launches allocated: 40 envs of every flow created, run and
    destroyed leave the device's free memory where it was (the parts' streams are process-wide and stay)."""
    import ctypes

    hip = ctypes.CDLL("libamdhip64.so")

    def free_bytes():
        assert hip.hipDeviceSynchronize() == 0
        free, total = ctypes.c_size_t(0), ctypes.c_size_t(0)
        assert hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0
        return free.value

    def cycle(i):
        env = bk.ManyBookEnv(2048 + 64 * (i % 3), 5 + i, 0, 2, 100_000, levels=16, max_live_orders=128 if i % 2 else 512,
                             trade_capacity=4096, history_capacity=4, strict=False)
        if i % 4 == 3:
            env.set_agents([("momentum", 0, 32, dict(tick_size=2, p_cancel=0.1, trade_vol=100, decay=1.0, demand=8.0, scale=0.5,
                                                      order_ratio=1.0, price_dist_mu=0.0, price_dist_sigma=3.0)),
                            ("noise", 32, 32, dict(tick_size=2, p_limit=0.3, p_market=0.2, p_cancel=0.2, trade_vol=100,
                                                   price_dist_mu=0.0, price_dist_sigma=1.0))])
        else:
            env.set_random_agents(C3_GROUPS if i % 2 else C5_GROUPS)
        env.set_pipeline(("split", "wave_split", "fused", "wave_split")[i % 4])
        env.run(3)
        env.trade_counts(), env.level2(), env.stats(), env.checkpoint()
        env.warm(2)
        env.close()

    for i in range(4):  # first use of every pipeline: streams, event pools, lazily created staging buffers
        cycle(i)
    free0 = free_bytes()
    for i in range(40):
        cycle(i)
    free1 = free_bytes()
    assert free0 - free1 < 32 << 20, f"device memory shrank by {(free0 - free1) >> 20} MiB over 40 env lifecycles"


def test_envs_driven_from_concurrent_host_threads(bk, oracle):
    """Distinct envs may be driven from distinct host threads at the same time (include/bourse_amd.h "Threads"): four threads,
    each with its own env and pipeline, run chunked launches, read results and poll flags concurrently (ctypes releases the
    GIL inside every call) - every env must still match its oracle run."""
    import threading

    T, chunks = 15, [4, 6, 5]
    jobs = [(3072, 31, "split", C3_GROUPS, 128), (2048, 32, "wave_split", C3_GROUPS, 128), (1024, 33, "fused", C2_GROUPS, 64),
            (1536, 34, "wave_split", C5_GROUPS, 512)]
    out, errs = {}, []

    def work(n, seed, pipe, groups, pool):
        try:
            env = bk.ManyBookEnv(n, seed, 0, 2, 100_000, True, levels=32, max_live_orders=pool, trade_capacity=512 * T,
                                 history_capacity=T, strict=False)
            env.set_random_agents(groups)
            env.set_pipeline(pipe)
            if pipe == "split":
                env.set_split_parts(3, 512)
            for c in chunks:
                env.run(c)
                env.flags_summary(); env.trade_counts()
            out[seed] = (env.flags().copy(), env.history().copy(), env.trade_counts().copy(), env.rng_state(n - 1))
            env.close()
        except Exception as e:  # noqa: BLE001
            errs.append((seed, repr(e)))

    th = [threading.Thread(target=work, args=j) for j in jobs]
    [t.start() for t in th]
    [t.join() for t in th]
    assert not errs, errs
    for n, seed, pipe, groups, pool in jobs:
        ref = oracle.ManyBooks(n, seed, 0, 2, 100_000, True, 32, groups)
        ref.run(T, n_threads=8)
        flags, hist, tc, rs = out[seed]
        assert not flags.any(), (seed, np.unique(flags))
        assert np.array_equal(hist, ref.history()), (seed, pipe)
        assert np.array_equal(tc, ref.trade_counts()), (seed, pipe)
        want = ref.rng_states()[n - 1]
        assert rs == (int(want[0]), int(want[1])), (seed, pipe)
