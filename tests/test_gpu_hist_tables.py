"""The contract the three tables folded from the level-2 history ring share - the series moments, the lag table and the bin
table (bk_series_*, bk_lags_*, bk_bins_*) - each scenario written once and run for every table through its
adapter in tests/hist_tables.py: folds in parts on every flow, lost steps, the ingress reset's cut of the carry, a restore,
and the refusals.  Three more scenarios are written once as functions of tests/hist_tables.py and run from the tables' own
files under the ids they always had: the run folded in three parts on every pipeline, reset_books' cut, the masked clear.

The expected side never shares code with the kernels: the tables' plain-Python models (tests/series_model.py,
lags_model.py, bins_model.py) over the ORACLE's history() of the same run - oracle.ManyBooks / ManyMarkets for bk_run, one
oracle.StepEnv per book for the device-ingress flows - and the device's own history is held against the oracle's through
tests/oracle_parity.py where the ring still retains it.  Where a case says something only under a condition, the adapter's
busy() asserts it on the expected side before anything is compared.  All comparisons are exact.  The tables' own cases -
rows by hand, extreme values, widths, carries deeper than the ring, markets' resets, run_series - are in their files."""
import numpy as np
import pytest

pytest.register_assert_rewrite("hist_tables")  # (a support module: its asserts report their values too)

import oracle_parity as P  # noqa: E402
from hist_tables import SEED, TABLES, bk, lost, refused, run_env  # noqa: E402,F401 (bk is a fixture)
from ingress_support import ingress_env  # noqa: E402
from test_gpu_reset_books import C2, MEMBERS, STEP, make_env, ref_books  # noqa: E402

pytestmark = pytest.mark.gpu
each_table = pytest.mark.parametrize("T", TABLES, ids=repr)


# ------------------------------------------------------------------------------------------------ bk_run and the other flows
@each_table
def test_noise_and_momentum_members_folded_in_chunks_of_seven(bk, oracle, T):
    B, steps, cfg = 3, 40, T.cfg["members"]
    hist = ref_books(oracle, B, 16, steps, members=MEMBERS).history()
    env = run_env(bk, T, B, steps, cfg, members=MEMBERS)
    for lo in range(0, steps, 7):
        env.run(min(7, steps - lo), sync=False)
        T.fold(env)
    P.no_flags(env)
    want = T.rows(hist, cfg)
    T.busy("members", want, cfg)
    T.same(T.read(env), want, "Noise + Momentum")
    P.same_history(env.history(), hist)
    env.close()


@each_table
def test_markets_keep_rows_per_book(bk, oracle, T):
    NM, ticks, steps, cfg = 3, [2, 2], 30, T.cfg["markets"]
    groups = [(0, 24, (40, 56), (10, 20), 2, 0.8), (1, 24, (40, 56), (10, 20), 2, 0.6), (1, 8, (40, 56), (50, 70), 2, 0.3)]
    env = bk.ManyMarketEnv(NM, SEED, 0, ticks, STEP, True, levels=10, max_live_orders=64, trade_capacity=4096, history_capacity=steps)
    env.set_random_market_agents(groups)
    T.enable(env, cfg)
    ref = oracle.ManyMarkets(NM, SEED, 0, ticks, STEP, True, 10, groups)
    ref.run(steps)
    hist = ref.history()
    for n in (11, 19):
        env.run(n, sync=False)
        T.fold(env)
    P.no_flags(env)
    want = T.rows(hist, cfg)
    T.busy("markets", want, cfg)
    T.same(T.read(env), want, "markets, a table per book")
    P.same_history(env.history(), hist)
    env.close()


@each_table
def test_ingress_folded_after_every_step_equals_one_fold_at_the_end(bk, oracle, T):
    """A fold behind EVERY step takes the carry path every time; a twin env folds once at the end.  Beside the series, bars
    and accounts run on the first env and still equal their own models."""
    import torch

    from test_gpu_accounts import busy_flow
    from test_gpu_accounts import same_rows as same_accounts
    from test_gpu_trade_bars import Tape, same_bars

    B, steps, tick, NT, W, cfg = 4, 9, 2, 5, 3, T.cfg["ingress"]
    flows = [busy_flow(np.random.default_rng(20 + s), B, tick, idle=(1,) if s in (3, 4) else (), n_lo=30, n_hi=40) for s in range(steps)]
    env = ingress_env(bk, torch, B, steps, 256, 0, 64, tick=tick, n_ext=40)
    twin = ingress_env(bk, torch, B, steps, 256, 0, 64, tick=tick, n_ext=40)
    if T.name == "series":
        env.enable_accounts(NT)
        env.enable_trade_bars(W)
    T.enable(env, cfg)
    T.enable(twin, cfg)
    tape, other = Tape(oracle, B, tick, env, torch), Tape(oracle, B, tick, twin, torch)
    for s, f in enumerate(flows):
        for t in (tape, other):
            t.submit(*f)
            t.step()
        T.fold(env)
        if s == 4:
            mid = T.read(env)
    T.fold(twin)
    hist = np.stack([r.history() for r in tape.refs], axis=1)
    want = T.rows(hist, cfg)
    T.busy("ingress", want, cfg)
    T.same(mid, T.rows(hist[:5], cfg), "after step 4")
    T.same(T.read(env), want, "folded after every step")
    T.same(T.read(twin), want, "folded once")
    for e in (env, twin):
        P.no_flags(e)
        P.same_history(e.history(), hist)
    if T.name == "series":
        same_bars(env.trade_bars(), tape.bars(W), "the bars beside the series")
        same_accounts(env.accounts(), tape.want(NT), "the accounts beside the series")
    env.close()
    twin.close()


# ------------------------------------------------------------------------------------------------ lost steps
@each_table
def test_lost_steps_refuse_the_fold_and_a_full_clear_recovers(bk, oracle, T):
    B, cfg = 3, T.cfg["lost"]
    hist = ref_books(oracle, B, 16, 16, groups=C2).history()
    env = run_env(bk, T, B, 8, cfg)
    env.run(3)
    T.fold(env)
    before = T.read(env)
    T.same(before, T.rows(hist[:3], cfg), "three steps")
    env.run(9)  # steps 3 .. 11 into a ring of 8: step 3 is gone
    lost(bk, T, lambda: T.fold(env), 1)
    T.same(T.read(env), before, "a refused fold leaves the table")
    lost(bk, T, lambda: T.fold(env), 1)  # ... and the cursor
    lost(bk, T, lambda: T.clear(env, np.array([1, 0, 0], dtype=bool)), 1)
    T.same(T.read(env), before, "a refused clear leaves the table")
    T.clear(env)
    T.same(T.read(env), T.cleared(B, cfg), "a full clear clears every book")
    env.run(2)
    T.fold(env)
    want = T.rows(hist[12:14], cfg, first_step=12)  # (the carry was cleared too: step 12 has no past)
    T.busy("lost", want, cfg)
    T.same(T.read(env), want, "counted from the clear on")
    # the same through clear_history(): the two steps run since the last fold are no longer retained
    env.run(2)
    env.clear_history()
    lost(bk, T, lambda: T.fold(env), 2)
    T.same(T.read(env), want, "a refused fold leaves the table (clear_history)")
    T.clear(env)
    env.close()


# ------------------------------------------------------------------------------------------------ resets, clears, restore
@each_table
def test_reset_ingress_books_cuts_the_carry_too(bk, oracle, T):
    """3 steps, save, 3 steps, reset books 0 and 2 (a torch CUDA mask; the three steps are folded by the reset), 2 steps.
    The oracle cannot be rewound: a reset book's quotes after the reset are those of a REPLAY, a fresh oracle env given
    steps 0 .. 2 again and then the two steps after the reset (tests/test_gpu_accounts.py)."""
    import torch

    from test_gpu_accounts import Books, busy_flow

    B, tick, cfg = 4, 2, T.cfg["ingress_reset"]
    env = ingress_env(bk, torch, B, 8, 256, 0, 64, tick=tick, n_ext=40)
    T.enable(env, cfg)
    books = Books(oracle, B, tick, env, torch)
    flows = [busy_flow(np.random.default_rng(60 + s), B, tick, n_lo=30, n_hi=40) for s in range(8)]

    def run(lo, hi, bs=books):
        for f in flows[lo:hi]:
            bs.submit(*f)
            bs.step()

    run(0, 3)
    env.save_ingress_snapshot()
    T.fold(env)
    run(3, 6)
    mask = np.array([1, 0, 1, 0], dtype=bool)
    env.reset_ingress_books(torch.tensor(mask, device="cuda"), sync=False)
    run(6, 8)
    T.fold(env)
    replay = Books(oracle, B, tick)
    run(0, 3, replay)
    run(6, 8, replay)
    want = []
    for b in range(B):
        h = books.refs[b].history()
        if mask[b]:
            s = T.fold_model(replay.refs[b].history()[3:5], cuts=[6], first_step=6, into=T.fold_model(h[:6], cfg))
        else:
            s = T.fold_model(h, cfg)
        want.append(T.table(s))
    want = T.stack(want)
    T.busy("ingress_reset", want, cfg)
    T.same(T.read(env), want, "reset_ingress_books")
    P.no_flags(env)
    env.close()


@each_table
def test_restore_clears_the_table_and_rebases_the_cursor(bk, oracle, T):
    B, cfg = 3, T.cfg["restore"]
    hist = ref_books(oracle, B, 16, 16, groups=C2).history()
    env = run_env(bk, T, B, 16, cfg)
    env.run(6)
    T.fold(env)
    ck = env.checkpoint()
    env.run(4)  # (outstanding when the checkpoint comes back: forgotten, not folded)
    env.restore(ck)
    assert env.steps_done() == 6
    T.same(T.read(env), T.cleared(B, cfg), "restore clears every book")
    env.run(5)
    T.fold(env)
    T.same(T.read(env), T.rows(hist[6:11], cfg, first_step=6), "counted from the restored step on, with no past")
    P.no_flags(env)
    env.close()


# ------------------------------------------------------------------------------------------------ refusals
@each_table
def test_refusals_leave_the_env_working(bk, oracle, T):
    cfg = T.cfg["refusals"]
    env = make_env(bk, 2, groups=C2, steps=8)
    for call in T.calls(env):
        refused(bk, call, T.no_table)
    env.run(2)
    T.bad_enables(bk, env)  # (the table's own argument checks: each leaves the env without the table)
    T.enable(env, cfg)
    T.enabled(bk, env, cfg)  # (enabled twice, null out-pointers, book ranges past the end: the table as it was)
    with pytest.raises(ValueError):
        T.clear(env, np.ones(3, dtype=bool))
    with pytest.raises(ValueError):
        env.run_series(4, chunk=9)
    env.run(3)
    T.fold(env)
    hist = ref_books(oracle, 2, 16, 16, groups=C2).history()
    T.same(T.read(env), T.rows(hist[2:5], cfg, first_step=2), "steps before the enable are not counted")
    env.close()
    none = make_env(bk, 2, groups=C2, steps=0)
    refused(bk, lambda: T.enable(none, cfg), "history_capacity must be > 0")
    none.run(2)
    none.close()
    # a host-driven env: a book cannot be loaded into an env with the table
    host = bk.ManyBookEnv(2, SEED, 0, 1, STEP, levels=5, max_live_orders=16, max_orders=16, trade_capacity=16, history_capacity=4)
    host.place_order(0, True, 5, 1, 100)
    host.step()
    state = host.book_state(0)
    host.load_book_state(1, state)
    T.enable(host, cfg)
    refused(bk, lambda: host.load_book_state(1, state), T.loading)
    host.step()
    T.fold(host, sync=True)
    T.one_sided(host, cfg)
    host.close()
