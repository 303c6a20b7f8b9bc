"""The hand-written draw loop of k_agents_fsm (bourse_amd/csrc/fsm_asm.hpp) against the CPU oracle, bit for bit.

One statement serves k_agents_fsm<1|2|4|8>, so every pool size runs it here, on the `split` pipeline (forced: small
batches would otherwise take the fused kernel), at the smallest shapes at which the loop can still go wrong: a group that
crosses a 64-slot segment, rate 0 and rate 1 groups, a volume range of 1 (zone all ones), ranges that are no power of
two, a wave with two live lanes, a wave's 64th lane and a one-lane wave, a list of at most one event (no shuffle).
Compared: level-2 history of every step, trade counts, the RNG state of every book, and the first / middle / last book
in full (trades, resting orders in priority order).  The kernel also carries the compiled C++ loop, the statement's
specification (BOURSE_AMD_FSM_LOOP=compiled, read when an env is created): one case runs it beside the statement.
"""
import numpy as np
import pytest

import oracle_parity as P

pytestmark = pytest.mark.gpu

C2_GROUPS = [(32, (40, 56), (10, 20), 2, 0.8), (32, (40, 56), (50, 70), 2, 0.2)]
C3_GROUPS = [(64, (32, 64), (10, 20), 2, 0.8), (64, (32, 64), (50, 70), 2, 0.2)]
C5_GROUPS = [(256, (100, 164), (10, 20), 2, 0.8), (256, (100, 164), (50, 70), 2, 0.2)]
# 128 agents (R = 2): the second group crosses the segment boundary at slot 64; rate 1 and rate 0; vol range 1
SEGMENT_GROUPS = [(40, (10, 14), (1, 4), 3, 0.5), (50, (9, 13), (50, 70), 6, 1.0), (38, (10, 14), (1, 2), 3, 0.0)]


@pytest.fixture(scope="module")
def bk():
    import bourse_amd

    return bourse_amd


def _compare_split(bk, oracle, n_books, groups, levels, n_steps, seed=101, tick=1, step_size=100_000, chunks=None,
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


def test_segment_boundary_rate_extremes_and_unit_volume_range(bk, oracle):
    # 130 books: two full waves and a wave with two live lanes
    _compare_split(bk, oracle, n_books=130, groups=SEGMENT_GROUPS, levels=8, n_steps=30)


def test_c3_shape_last_lane_and_one_lane_wave(bk, oracle):
    # the benchmark's R = 2 shape; book 63 is a wave's 64th lane, book 64 a wave of its own
    _compare_split(bk, oracle, n_books=65, groups=C3_GROUPS, levels=32, n_steps=25, tick=2)


def test_single_agent_list_never_shuffled(bk, oracle):
    _compare_split(bk, oracle, n_books=3, groups=[(1, (10, 20), (20, 30), 1, 1.0)], levels=10, n_steps=25, step_size=1000)


def test_c5_shape_pool_of_512(bk, oracle):
    # R = 8 through the same statement
    _compare_split(bk, oracle, n_books=8, groups=C5_GROUPS, levels=64, n_steps=12, tick=2, max_live=512)


def test_c2_shape_pool_of_64(bk, oracle):
    # R = 1
    _compare_split(bk, oracle, n_books=96, groups=C2_GROUPS, levels=16, n_steps=40, tick=2)


def test_chunked_launches_equal_one_launch(bk, oracle):
    a = _compare_split(bk, oracle, n_books=130, groups=SEGMENT_GROUPS, levels=8, n_steps=9, chunks=[3, 1, 5])
    b = _compare_split(bk, oracle, n_books=130, groups=SEGMENT_GROUPS, levels=8, n_steps=9)
    assert np.array_equal(a, b)


def test_compiled_loop_of_the_same_library_agrees(bk, oracle, monkeypatch):
    # the kernel's second copy of its body, with the C++ draw loop: same oracle, same history as the statement's
    a = _compare_split(bk, oracle, n_books=130, groups=SEGMENT_GROUPS, levels=8, n_steps=12)
    monkeypatch.setenv("BOURSE_AMD_FSM_LOOP", "compiled")
    b = _compare_split(bk, oracle, n_books=130, groups=SEGMENT_GROUPS, levels=8, n_steps=12)
    assert np.array_equal(a, b)
