"""The hand-written shuffle and publish loops of k_agents_fsm (bourse_amd/csrc/fsm_asm.hpp: fsm_shuffle_asm,
fsm_publish_asm) against the CPU oracle, bit for bit.

Both statements serve k_agents_fsm<1|2|4|8>; every case runs on the `split` pipeline (forced: small batches would
otherwise take the fused kernel) and compares the level-2 history of every step, the trade counts, the RNG state of every
book, and the first / middle / last book in full.  A group of rate 1.0 queues one event per agent on every step, so its
agent count IS the list length n_ev: the shuffle draws the ranges n_ev .. 2 on every step (powers of two never reject,
ranges just above one reject nearly half the time) and the publish loop stores n_ev / 8 full groups of eight events and
one partial group of n_ev % 8.  Lengths: no shuffle (1), one draw of range 2 (2), the odd tail (3), the publish group
boundary (7, 8, 9), the boundary between k_step_batch's two list registers (63, 64, 65), the full list of 64 R entries
(127, 128).  One env's books share their groups, so the lanes of a wave differ in length by their draws only: a short
list (lengths 0 .. 5 side by side) and a long one (about 30 +- 4) make lanes leave both loops at different times.
"""
import numpy as np
import pytest

import oracle_parity as P

pytestmark = pytest.mark.gpu

C2_GROUPS = [(32, (40, 56), (10, 20), 2, 0.8), (32, (40, 56), (50, 70), 2, 0.2)]
C3_GROUPS = [(64, (32, 64), (10, 20), 2, 0.8), (64, (32, 64), (50, 70), 2, 0.2)]
R4_GROUPS = [(128, (60, 124), (10, 20), 2, 0.8), (128, (60, 124), (50, 70), 2, 0.2)]
C5_GROUPS = [(256, (100, 164), (10, 20), 2, 0.8), (256, (100, 164), (50, 70), 2, 0.2)]
# 130 books (two full waves and a wave with two live lanes); list lengths 0 .. 5, and about 30 +- 4
SHORT_GROUPS = [(3, (10, 14), (1, 4), 3, 0.5), (60, (9, 13), (50, 70), 6, 0.02)]
LONG_GROUPS = [(60, (10, 14), (1, 4), 3, 0.5), (60, (9, 13), (50, 70), 6, 0.02)]


@pytest.fixture(scope="module")
def bk():
    import bourse_amd

    return bourse_amd


def _compare_split(bk, oracle, n_books, groups, levels, n_steps, seed=211, tick=1, step_size=100_000, chunks=None,
                   max_live=None):
    n_agents = sum(g[0] for g in groups)
    if chunks:
        n_steps = sum(chunks)
    env = bk.ManyBookEnv(n_books, seed, 0, tick, step_size, True, levels=levels, max_live_orders=max_live or n_agents,
                         trade_capacity=2 * n_agents * n_steps, history_capacity=n_steps)
    env.set_random_agents(groups)
    env.set_pipeline("split")
    for c in chunks or [n_steps]:
        env.run(c)
    ref = oracle.ManyBooks(n_books, seed, 0, tick, step_size, True, levels, groups)
    ref.run(n_steps, n_threads=4)

    P.no_flags(env)
    hist = env.history()
    P.same_history(hist, ref.history())
    assert np.array_equal(env.trade_counts(), ref.trade_counts())
    want_rng = ref.rng_states()
    for b in range(n_books):
        assert env.rng_state(b) == (int(want_rng[b, 0]), int(want_rng[b, 1])), f"rng state book {b}"
    for b in sorted({0, n_books // 2, n_books - 1}):
        P.same_book(env, b, ref.book(b))
    env.close()
    return hist


@pytest.mark.parametrize("n_ev", [1, 2, 3, 7, 8, 9, 63, 64, 65, 127, 128])
def test_exact_list_length_in_a_pool_of_128(bk, oracle, n_ev):
    # R = 2 whatever the agent count; every step's list holds exactly n_ev events
    _compare_split(bk, oracle, n_books=3, groups=[(n_ev, (20, 36), (10, 20), 2, 1.0)], levels=16, n_steps=25, max_live=128)


@pytest.mark.parametrize("groups", [SHORT_GROUPS, LONG_GROUPS], ids=["lengths_0_to_5", "lengths_about_30"])
def test_lanes_leave_the_loops_at_different_times(bk, oracle, groups):
    _compare_split(bk, oracle, n_books=130, groups=groups, levels=8, n_steps=25, max_live=128)


def test_last_lane_of_a_wave_and_one_lane_wave(bk, oracle):
    _compare_split(bk, oracle, n_books=65, groups=C3_GROUPS, levels=32, n_steps=25, tick=2)


@pytest.mark.parametrize("groups,n_books,pool,n_steps", [(C2_GROUPS, 96, 64, 30), (R4_GROUPS, 8, 256, 16), (C5_GROUPS, 8, 512, 12)],
                         ids=["R1", "R4", "R8"])
def test_other_pool_sizes_run_the_same_statements(bk, oracle, groups, n_books, pool, n_steps):
    _compare_split(bk, oracle, n_books=n_books, groups=groups, levels=32, n_steps=n_steps, tick=2, max_live=pool)


def test_market_of_two_assets(bk, oracle):
    # the lane owns a MARKET: one list, one batch (the market's), and both books carry a copy of the RNG state
    ticks = [1, 2]
    groups = [(0, 37, (40, 60), (10, 20), 2, 0.8), (1, 30, (40, 60), (10, 20), 2, 0.7)]
    NM, T = 5, 20
    env = bk.ManyMarketEnv(NM, 212, 0, ticks, 100_000, True, levels=10, max_live_orders=128, trade_capacity=4096,
                           history_capacity=T)
    env.set_random_market_agents(groups)
    env.set_pipeline("split")
    env.run(T)
    ref = oracle.ManyMarkets(NM, 212, 0, ticks, 100_000, True, 10, groups)
    ref.run(T, n_threads=4)
    P.no_flags(env)
    P.same_history(env.history(), ref.history())
    want_rng = ref.rng_states()
    for m in range(NM):
        for a in range(2):
            b = env.book(m, a)
            assert env.rng_state(b) == (int(want_rng[m, 0]), int(want_rng[m, 1])), f"rng state market {m} asset {a}"
            P.same_book(env, b, ref.book(m, a), tag=(m, a))
    env.close()


def test_chunked_launches_equal_one_launch(bk, oracle):
    a = _compare_split(bk, oracle, n_books=130, groups=LONG_GROUPS, levels=8, n_steps=9, chunks=[3, 1, 5], max_live=128)
    b = _compare_split(bk, oracle, n_books=130, groups=LONG_GROUPS, levels=8, n_steps=9, max_live=128)
    assert np.array_equal(a, b)


def test_compiled_loops_of_the_same_library_agree(bk, oracle, monkeypatch):
    # the kernel's second copy of its body (C++ draw loop, C++ shuffle, C++ publish): same oracle, same history
    a = _compare_split(bk, oracle, n_books=130, groups=LONG_GROUPS, levels=8, n_steps=12, max_live=128)
    monkeypatch.setenv("BOURSE_AMD_FSM_LOOP", "compiled")
    b = _compare_split(bk, oracle, n_books=130, groups=LONG_GROUPS, levels=8, n_steps=12, max_live=128)
    assert np.array_equal(a, b)
