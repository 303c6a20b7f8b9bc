"""GPU parity at the value ranges where 32-bit kernels go wrong: 64-bit clocks, volumes and sums that wrap u32, huge and
odd tick sizes, the widest sampling ranges, and the statistics record.

Every case compares the device with the CPU oracle bit for bit (level-2 history of every step and book, trade records,
live orders in priority order, RNG states, clocks; the order log where the env keeps one).  Where the level ladder's
u32 multiply wraps ((levels - 1) * tick >= 2^32) the level-2 record is also checked against a few lines of Python that
apply the reference's rule (orderbook.rs:229-264).
"""
import numpy as np
import pytest

import oracle_parity as P

pytestmark = pytest.mark.gpu

U32 = 2**32
MAXP = U32 - 1
SEED = 101
# (start_time, step_size): a carry inside a step (event k of step 0 is stamped start + k: from the 5th on the high word is 1;
# the step is wider than any step's queue here - a queue of step_size events or more overlaps the next step's times, which
# the library flags as STEP_SIZE), a carry between steps, epoch nanoseconds, a step size with a high word
TIMES = [(U32 - 5, 128), (U32 - 5 * 100_000, 100_000), (1_700_000_000_000_000_000, 1_000_000), (2**63 + 12_345, U32 + 3)]
TIME_IDS = ["carry-in-step", "carry-between-steps", "epoch-ns", "step-hi-word"]
GROUPS = [(24, (40, 56), (10, 20), 2, 0.8), (16, (40, 56), (50, 70), 2, 0.3)]
AGENT_PIPELINES = ["fused", "split", "wave_split", "wave"]
MEMBER_PIPELINES = ["fused", "split", "split_wave", "wave_split"]
NOISE_P = dict(tick_size=2, p_limit=0.3, p_market=0.2, p_cancel=0.1, trade_vol=100, price_dist_mu=0.0, price_dist_sigma=2.0)
MOM_P = dict(tick_size=2, p_cancel=0.1, trade_vol=100, decay=1.0, demand=5.0, scale=0.5, order_ratio=1.0,
             price_dist_mu=0.0, price_dist_sigma=10.0)
HUGE_TICKS = [3, 2**16 + 1, 2**31 - 1, 2**30, 2**31, MAXP]
# RandomAgents at the env tick (half-open tick ranges; the top price (hi - 1) * tick stays below u32::MAX); none for MAXP
AGENT_TICK_RANGE = {3: (1000, 1040), 2**16 + 1: (1000, 65535), 2**31 - 1: (1, 3), 2**30: (1, 4), 2**31: (1, 2)}


@pytest.fixture(scope="module")
def bk():
    import bourse_amd

    return bourse_amd


# ------------------------------------------------------------------------------------------------ reference rules
def _l2_rule(orders, levels, tick):
    """Words 1.. of the level-2 record of a book whose resting orders are ``orders`` (an order array; status 1 = Active),
    straight from the reference: touch prices, side volumes (u32 sums) and level i = price touch -/+ i * tick, all in
    wrapping u32 arithmetic (several levels may name one price)."""
    act = orders[orders["status"] == 1]
    out = np.zeros(4 + 4 * levels, dtype=np.uint64)
    bids = [(int(o["price"]), int(o["vol"])) for o in act if o["side"] == 1]
    asks = [(int(o["price"]), int(o["vol"])) for o in act if o["side"] == 0]
    bb = max((p for p, _ in bids), default=0)
    ba = min((p for p, _ in asks), default=MAXP)
    out[:4] = (bb, ba, sum(v for _, v in asks) % U32, sum(v for _, v in bids) % U32)
    for i in range(levels):
        for side, touch, sgn, col in ((bids, bb, -1, 0), (asks, ba, 1, 2)):
            target = (touch + sgn * i * tick) % U32
            at = [v for p, v in side if p == target]
            out[4 + 4 * i + col] = sum(at) % U32
            out[4 + 4 * i + col + 1] = len(at)
    return out.astype(np.uint32)


def _carried_in_step0(views, start, step):
    """When the first step straddles 2^32: some order or trade of these books was stamped in step 0 at or above 2^32."""
    if not start < U32 < start + step:
        return
    hits = 0
    for v in views:
        o, t = v.orders_array(), v.trades_array()
        hits += int(((o["arr_time"] >= U32) & (o["arr_time"] < start + step)).sum())
        hits += int(((t["t"] >= U32) & (t["t"] < start + step)).sum())
    assert hits > 0, "no event of step 0 was stamped past 2^32"


# ------------------------------------------------------------------------------------- on-device agents (bk_run)
def _run_agents(bk, oracle, B, T, *, start=0, step=100_000, tick=2, levels=10, groups=None, members=None,
                pipeline="fused", lookahead=None, pool=None, log=False, chunks=None, check_rule=False):
    n_agents = sum(g[0] for g in groups) if groups else sum(m[2] for m in members)
    pool = pool or max(64, n_agents)
    env = bk.ManyBookEnv(B, SEED, start, tick, step, True, levels=levels, max_live_orders=pool,
                         max_orders=(4 * n_agents * T + 64) if log else 0, trade_capacity=4 * n_agents * T + 64,
                         history_capacity=T)
    if groups:
        env.set_random_agents(groups)
    else:
        env.set_agents(members)
    if log:
        env.enable_agent_order_log()
    if lookahead is not None:
        env.set_wave_options(lookahead, 0)
    env.set_pipeline(pipeline)
    for c in (chunks or [T]):
        env.run(c)
    ref = oracle.ManyBooks(B, SEED, start, tick, step, True, levels, groups, members=members)
    ref.run(T, n_threads=4)
    P.no_flags(env)
    hist = env.history()
    P.same_history(hist, ref.history())
    assert np.array_equal(env.level2(), hist[-1])
    assert np.array_equal(env.trade_counts(), ref.trade_counts())
    want_rng = ref.rng_states()
    for b in range(B):
        assert env.rng_state(b) == (int(want_rng[b, 0]), int(want_rng[b, 1])), b
        assert env.time(b) == start + T * step, b
        P.same_book(env, b, ref.book(b), orders=log)
        if check_rule:
            assert np.array_equal(hist[-1, b, 1:], _l2_rule(ref.book(b).orders_array(), levels, tick)), b
    assert int(ref.trade_counts().sum()) > 0
    _carried_in_step0([ref.book(b) for b in range(B)], start, step)
    env.close()
    return hist


@pytest.mark.parametrize("pipeline", AGENT_PIPELINES)
@pytest.mark.parametrize("times", TIMES, ids=TIME_IDS)
def test_random_agents_at_64_bit_times(bk, oracle, times, pipeline):
    _run_agents(bk, oracle, 6, 12, start=times[0], step=times[1], groups=GROUPS, pipeline=pipeline)


@pytest.mark.parametrize("times", TIMES, ids=TIME_IDS)
def test_noise_momentum_at_64_bit_times(bk, oracle, times):
    members = [("momentum", 0, 10, MOM_P), ("noise", 10, 20, NOISE_P)]
    _run_agents(bk, oracle, 6, 16, start=times[0], step=times[1], tick=1, members=members, pool=256)
    _run_agents(bk, oracle, 6, 16, start=times[0], step=times[1], tick=1, members=members, pool=256, pipeline="wave_split")


@pytest.mark.parametrize("times", TIMES, ids=TIME_IDS)
def test_agent_order_log_at_64_bit_times(bk, oracle, times):
    for pipeline in ("split", "wave_split"):
        _run_agents(bk, oracle, 5, 12, start=times[0], step=times[1], groups=GROUPS, pipeline=pipeline, log=True)


@pytest.mark.parametrize("times", TIMES[:2] + TIMES[3:], ids=[TIME_IDS[0], TIME_IDS[1], TIME_IDS[3]])
def test_checkpoint_restore_across_the_carry(bk, times):
    start, step = times

    def mk():
        e = bk.ManyBookEnv(8, 5, start, 2, step, levels=10, max_live_orders=64, trade_capacity=4096, history_capacity=12)
        e.set_random_agents(GROUPS)
        return e

    a = mk()
    a.run(6)  # (every pair above has crossed 2^32 by step 6)
    assert a.time(0) == start + 6 * step and (a.time(0) >> 32) != (start >> 32)
    ck = a.checkpoint()
    a.run(6)
    b = mk()
    b.restore(ck)
    assert b.time(3) == start + 6 * step
    b.set_pipeline("split")
    b.run(6)
    assert np.array_equal(a.history()[6:], b.history())
    assert [a.rng_state(i) for i in range(8)] == [b.rng_state(i) for i in range(8)]
    assert all(a.time(i) == b.time(i) == start + 12 * step for i in range(8))
    ta, tb = a.trades(2, first=0), b.trades(2)
    assert len(tb) and np.array_equal(ta[len(ta) - len(tb):], tb)
    a.close()
    b.close()


@pytest.mark.parametrize("times", TIMES, ids=TIME_IDS)
def test_random_market_agents_at_64_bit_times(bk, oracle, times):
    start, step = times
    ticks = [1, 2]
    groups = [(0, 16, (40, 60), (10, 20), 2, 0.8), (1, 16, (40, 60), (10, 20), 2, 0.7)]
    NM, T = 5, 12
    env = bk.ManyMarketEnv(NM, SEED, start, ticks, step, True, levels=10, max_live_orders=64, trade_capacity=2048,
                           history_capacity=T)
    env.set_random_market_agents(groups)
    env.run(T)
    ref = oracle.ManyMarkets(NM, SEED, start, ticks, step, True, 10, groups)
    ref.run(T, n_threads=4)
    P.no_flags(env)
    P.same_history(env.history(), ref.history())
    want_rng = ref.rng_states()
    for m in range(NM):
        for a in range(2):
            b = env.book(m, a)
            assert env.rng_state(b) == (int(want_rng[m, 0]), int(want_rng[m, 1]))
            assert env.time(b) == start + T * step
            P.same_book(env, b, ref.book(m, a), tag=(m, a))
    _carried_in_step0([ref.book(m, a) for m in range(NM) for a in range(2)], start, step)
    env.close()


# ----------------------------------------------------------------------------------------- host-driven steps
def _random_ops(rng, made, prices, vols, n, p_market=0.1, p_cancel=0.2, p_mod=0.1, zero_vol=False):
    """n random host calls: (method, args) with limit / market placements, cancellations and modifications."""
    ops = []
    for _ in range(n):
        u = rng.random()
        if u < p_cancel and made:
            ops.append(("cancel_order", (int(rng.integers(0, made)),)))
        elif u < p_cancel + p_mod and made:
            np_ = None if rng.random() < 0.5 else int(rng.choice(prices))
            nv = None if rng.random() < 0.3 else int(rng.choice(vols))
            ops.append(("modify_order", (int(rng.integers(0, made)), np_, nv)))
        else:
            price = None if rng.random() < p_market else int(rng.choice(prices))
            ops.append(("place_order", (bool(rng.integers(0, 2)), int(rng.choice(vols)), int(rng.integers(0, 9)), price)))
            made += 1
    if zero_vol:  # a resting order of volume 0: the keyed form does not take the step
        ops.append(("place_order", (True, 0, 1, int(min(prices)))))
        made += 1
    return ops, made


def _host_env(bk, oracle, B, T, start, step, tick, levels, pool=128, strict=True):
    env = bk.ManyBookEnv(B, SEED, start, tick, step, levels=levels, max_live_orders=pool, max_orders=4096,
                         trade_capacity=8192, history_capacity=T, strict=strict)
    refs = [oracle.StepEnv(SEED + b, start, tick, step, True, levels) for b in range(B)]
    return env, refs


def _apply(env, refs, b, ops):
    for f, args in ops:
        if f == "place_order":
            assert getattr(env, f)(b, *args) == getattr(refs[b], f)(*args)
        else:
            getattr(env, f)(b, *args)
            getattr(refs[b], f)(*args)


def _check_host(env, refs, start=None, step=None, T=None, rule=None):
    P.no_flags(env)
    h = env.history()
    for b, r in enumerate(refs):
        P.same_history(h[:, b], r.history(), f"L2 history of book {b}")
        P.same_book(env, b, r.book, orders=True)
        if start is not None:
            assert env.time(b) == start + T * step, b
        if rule is not None:
            assert np.array_equal(h[-1, b, 1:], _l2_rule(r.book.orders_array(), *rule)), b
    if start is not None:
        _carried_in_step0([r.book for r in refs], start, step)
    return h


@pytest.mark.parametrize("loop", ["keyed", "event-by-event"])
@pytest.mark.parametrize("times", TIMES, ids=TIME_IDS)
def test_host_driven_steps_at_64_bit_times(bk, oracle, times, loop):
    start, step = times
    B, T = 6, 10
    env, refs = _host_env(bk, oracle, B, T, start, step, 1, 10)
    rng = np.random.default_rng(3)
    made = [0] * B
    for _ in range(T):
        for b in range(B):
            ops, made[b] = _random_ops(rng, made[b], list(range(95, 106)), list(range(1, 30)), int(rng.integers(4, 16)),
                                       p_mod=0.1, zero_vol=loop != "keyed")
            _apply(env, refs, b, ops)
        env.step()
        for r in refs:
            r.step()
    _check_host(env, refs, start, step, T)
    keyed = env.event_steps_keyed()
    assert (keyed.sum() > 0) if loop == "keyed" else (keyed.sum() == 0), keyed
    env.close()


@pytest.mark.parametrize("times", TIMES, ids=TIME_IDS)
def test_submit_instructions_all_at_64_bit_times(bk, oracle, times):
    start, step = times
    B, T = 5, 8
    env, refs = _host_env(bk, oracle, B, T, start, step, 2, 10)
    rng = np.random.default_rng(4)
    made = [0] * B
    for _ in range(T):
        rows = []
        off = [0]
        for b in range(B):
            for _k in range(int(rng.integers(0, 12))):
                if made[b] and rng.random() < 0.25:
                    rows.append((2, 0, 0, 0, 0, int(rng.integers(0, made[b]))))
                else:
                    rows.append((1, int(rng.integers(0, 2)), int(rng.integers(1, 30)), 3, 2 * int(rng.integers(45, 56)), 0))
                    made[b] += 1
            off.append(len(rows))
        cols = list(zip(*rows)) if rows else [()] * 6
        ins = [np.array(c, dtype=t) for c, t in zip(cols, (np.uint32, np.uint8, np.uint32, np.uint32, np.uint32, np.uint64))]
        ids = env.submit_instructions_all(np.array(off, dtype=np.uint64), ins)
        for b in range(B):
            sl = slice(off[b], off[b + 1])
            want = oracle.StepEnvNumpy.submit_instructions(refs[b], [x[sl] for x in ins])
            assert np.array_equal(ids[sl], want), b
        env.step()
        for r in refs:
            r.step()
    _check_host(env, refs, start, step, T)
    env.close()


def _torch_or_skip():
    import torch

    assert torch.cuda.is_available()
    return torch


@pytest.mark.parametrize("times", TIMES, ids=TIME_IDS)
def test_device_ingress_and_agents_at_64_bit_times(bk, oracle, times):
    """submit_instructions_device (k_ingest) and update_agents (agents_ingress.hpp) beside it: the time stamps they copy
    from the header."""
    torch = _torch_or_skip()
    start, step = times
    B, T = 6, 8
    groups = [(16, (40, 56), (10, 20), 2, 0.8), (8, (40, 56), (50, 70), 2, 0.3)]
    env = bk.ManyBookEnv(B, SEED, start, 2, step, levels=10, max_live_orders=128, max_orders=2048, trade_capacity=4096,
                         history_capacity=T, stream=torch.cuda.current_stream().cuda_stream)
    env.enable_device_ingress(queue_capacity=64)
    env.set_random_agents(groups)
    refs = [oracle.StepEnv(SEED + b, start, 2, step) for b in range(B)]
    agents = [oracle.RandomAgentSet(groups) for _ in range(B)]
    rng = np.random.default_rng(5)
    for s in range(T):
        rows, off = [], [0]
        for b in range(B):
            n0 = refs[b].book.n_orders()
            for _k in range(int(rng.integers(0, 6))):
                if n0 and rng.random() < 0.3:
                    rows.append((2, 0, 0, 0, 0, int(rng.integers(0, n0))))
                else:
                    rows.append((1, int(rng.integers(0, 2)), int(rng.integers(1, 30)), 3, 2 * int(rng.integers(44, 57)), 0))
            off.append(len(rows))
        cols = list(zip(*rows))
        dt = (np.int32, np.uint8, np.int32, np.int32, np.int64, np.int64)
        host = [np.array(c).astype(t) for c, t in zip(cols, dt)]
        host[4] = host[4].astype(np.uint32).view(np.int32)
        dev = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in host]
        offs = torch.from_numpy(np.array(off, dtype=np.int64)).cuda()
        out = torch.zeros(len(rows), dtype=torch.int64, device="cuda")
        st = torch.zeros(2 * B, dtype=torch.int32, device="cuda")
        env.submit_instructions_device(offs, *dev, out_ids=out, status=st, check_status=True)
        for b in range(B):
            for a, sd, v, tr, p, oid in rows[off[b]:off[b + 1]]:
                if a == 1:
                    refs[b].place_order(bool(sd), v, tr, p)
                else:
                    refs[b].cancel_order(oid)
        if s % 2 == 0:
            env.update_agents(sync=False)
            for r, ag in zip(refs, agents):
                ag.update(r)
        env.step()
        for r in refs:
            r.step()
    env.sync()
    _check_host(env, refs, start, step, T)
    for b in range(B):
        assert env.rng_state(b) == tuple(int(x) for x in refs[b].rng_state()), b
    env.close()


def test_immediate_order_book_set_time_across_2_pow_32(bk, oracle):
    g, o = bk.core.OrderBook(U32 - 20, 2), oracle.OrderBook(U32 - 20, 2)
    rng = np.random.default_rng(6)
    t = U32 - 20
    for k in range(60):
        t += int(rng.integers(1, 4)) if k != 30 else 2**40  # both sides of 2^32, then a jump far above
        for x in (g, o):
            x.set_time(t)
        n = len(o.get_orders())
        if n and rng.random() < 0.2:
            i = int(rng.integers(0, n))
            g.cancel_order(i)
            o.cancel_order(i)
        elif n and rng.random() < 0.2:
            i, p, v = int(rng.integers(0, n)), 2 * int(rng.integers(45, 56)), int(rng.integers(1, 20))
            g.modify_order(i, p, v)
            o.modify_order(i, p, v)
        else:
            args = (bool(rng.integers(0, 2)), int(rng.integers(1, 30)), 1,
                    None if rng.random() < 0.1 else 2 * int(rng.integers(45, 56)))
            assert g.place_order(*args) == o.place_order(*args)
    assert g.get_trades() == o.get_trades()
    assert g.get_orders() == o.get_orders()
    assert g.bid_ask() == o.bid_ask()


# --------------------------------------------------------------------------------------------------- volumes
BIG_VOL_GROUPS = [(8, (40, 56), (0, MAXP), 2, 0.8), (8, (40, 56), (2**31 - 5, 2**31 + 5), 2, 0.6),
                  (8, (40, 56), (U32 - 9, MAXP), 2, 0.5), (16, (40, 56), (1, 20), 2, 0.9)]


@pytest.mark.parametrize("pipeline", AGENT_PIPELINES)
def test_random_agents_with_volumes_near_2_pow_32(bk, oracle, pipeline):
    """Big and small orders in one book match each other; side volumes, level volumes and the step's trade volume wrap."""
    hist = _run_agents(bk, oracle, 8, 16, groups=BIG_VOL_GROUPS, pipeline=pipeline)
    assert (hist[:, :, 4].astype(np.uint64) < hist[:, :, 5].astype(np.uint64)).any()  # a side's u32 sum has wrapped


def test_noise_momentum_trade_vol_u32_max(bk, oracle):
    members = [("momentum", 0, 10, dict(MOM_P, trade_vol=MAXP)), ("noise", 10, 20, dict(NOISE_P, trade_vol=MAXP)),
               ("noise", 30, 10, NOISE_P)]
    for pipeline in MEMBER_PIPELINES:
        _run_agents(bk, oracle, 6, 16, tick=1, members=members, pool=256, pipeline=pipeline)


def test_host_driven_volumes_beyond_2_pow_32(bk, oracle):
    """Resting bid volume, one level's volume and one step's traded volume each above 2^32; a market order of volume
    u32::MAX sweeps the book; modifications to volume u32::MAX.  Every step fits the narrow key window (the 2^22 volume
    bound is the wide windows' only), so all of them run on the keyed loop."""
    B, T = 4, 6
    env, refs = _host_env(bk, oracle, B, T, 0, 1000, 1, 10)
    big = [3_000_000_000, 2_500_000_000, MAXP, 2**31, 7]
    for s in range(T):
        for b in range(B):
            ops = []
            if s == 0:
                ops += [("place_order", (True, big[(b + k) % 5], 1, 100 - (k % 3))) for k in range(6)]
                ops += [("place_order", (False, big[(b + k + 2) % 5], 2, 103 + (k % 3))) for k in range(6)]
            elif s == 1:
                ops += [("place_order", (False, MAXP, 3, 99)), ("place_order", (False, MAXP, 3, None))]
            elif s == 2:
                ops += [("modify_order", (6 + b % 4, None, MAXP)), ("modify_order", (b % 3, 104, MAXP)),
                        ("place_order", (True, MAXP, 4, None)), ("place_order", (True, 5, 4, 98))]
            elif s == 3:
                ops += [("place_order", (True, MAXP, 5, 200)), ("place_order", (False, MAXP, 5, 50)),
                        ("place_order", (True, 2**31 + b, 6, 101)), ("place_order", (True, 2**31 + 3, 6, 101))]
            else:
                ops += [("place_order", (s % 2 == 0, 1_000_000_000 * (1 + b), 7, 100 + s)), ("cancel_order", (s + b,))]
            _apply(env, refs, b, ops)
        env.step()
        for r in refs:
            r.step()
    h = _check_host(env, refs, rule=(10, 1))
    # what step 0 rests (nothing crosses) reaches past 2^32: every book's bid volume, and the touch level (k = 0, 3) of some
    assert all(sum(big[(b + k) % 5] for k in range(6)) > U32 for b in range(B))
    assert any(big[b % 5] + big[(b + 3) % 5] > U32 for b in range(B))
    per_step = [np.bincount((t["t"] // 1000).astype(np.int64), weights=t["vol"].astype(np.float64)).max()
                for t in (r.book.trades_array() for r in refs) if len(t)]
    assert max(per_step) > U32  # one step's traded volume in one book above 2^32
    assert env.event_steps_keyed().tolist() == [T] * B
    env.close()


def _far_stream(vol, high):
    if high:
        far = [("place_order", False, (3 + i) if i else vol, 9, 3_000_000 + 7 * i) for i in range(5)]
    else:
        far = [("place_order", True, (3 + i) if i else vol, 9, 1 + i) for i in range(5)]
    near = [("place_order", i % 2 == 0, 2 + i % 5, i, 50_000 + (i % 6) - (3 if i % 2 == 0 else 0)) for i in range(14)]

    def busy(s):
        return [("place_order", (i + s) % 2 == 0, 1 + (i + s) % 4, i, 50_000 + ((i + s) % 5) - (2 if (i + s) % 2 == 0 else 0))
                for i in range(10)] + [("cancel_order", 6 + s)]
    return [far + near, busy(1), busy(2) + [("place_order", high, 2, 3, None)], busy(3)]


@pytest.mark.parametrize("high", [False, True], ids=["far-low-bids", "far-high-asks"])
@pytest.mark.parametrize("pool", [64, 256])
def test_keyed_wide_windows_at_the_volume_bound(bk, oracle, pool, high):
    """keys_begin_wide / keys_begin_wide_high keep a step keyed while every live or new order's volume is below 2^22."""
    vols = [2**22 - 1, 2**22]
    B, T = len(vols), 4
    env = bk.ManyBookEnv(B, 77, 0, 1, 100_000, levels=10, max_live_orders=pool, max_orders=400, trade_capacity=800,
                         history_capacity=T)
    refs = [oracle.StepEnv(77 + b, 0, 1, 100_000) for b in range(B)]
    streams = [_far_stream(v, high) for v in vols]
    for s in range(T):
        for b in range(B):
            for f, *args in streams[b][s]:
                _apply(env, refs, b, [(f, tuple(args))])
        env.step()
        for r in refs:
            r.step()
    _check_host(env, refs)
    assert env.event_steps_keyed().tolist() == [3, 0]
    env.close()


# ---------------------------------------------------------------------------------------------- prices, ticks
def test_extreme_limit_prices(bk, oracle):
    """Limit prices 1, 2, 3 and u32::MAX - 1; a limit bid at u32::MAX and a limit ask at 0 that cannot fill completely
    are market orders (orderbook.rs:595-603): their remainder never rests.  (A book spanning 1 .. u32::MAX - 1 fits no key
    window: these steps run event by event.)"""
    B, T = 4, 6
    env, refs = _host_env(bk, oracle, B, T, 0, 1000, 1, 5)
    for s in range(T):
        for b in range(B):
            ops = [("place_order", (k % 2 == 0, 3 + k + b, 1, p)) for k, p in enumerate([1, 2, 3, MAXP - 1, 2, MAXP - 1])]
            if s % 2 == 1:
                ops += [("place_order", (True, 40 + b, 2, MAXP)), ("place_order", (False, 50 + b, 2, 0))]
            if s == 4:
                ops += [("modify_order", (b, 1, None)), ("cancel_order", (b + 1,))]
            _apply(env, refs, b, ops)
        env.step()
        for r in refs:
            r.step()
    _check_host(env, refs, rule=(5, 1))
    for r in refs:
        o = r.book.orders_array()
        assert not ((o["status"] == 1) & ((o["price"] == MAXP) & (o["side"] == 1) | (o["price"] == 0) & (o["side"] == 0))).any()
    env.close()


@pytest.mark.parametrize("ingress", [False, True], ids=["host-csr", "device-ingress"])
def test_extreme_prices_through_submit_instructions(bk, oracle, ingress):
    B, T = 4, 5
    env, refs = _host_env(bk, oracle, B, T, U32 - 3, 1000, 1, 5)
    if ingress:
        env.enable_device_ingress(queue_capacity=64)
    for s in range(T):
        rows, off = [], [0]
        for b in range(B):
            for k, p in enumerate([1, 2, 3, MAXP - 1, MAXP, 0, 2, MAXP - 1]):
                side = 1 if p == MAXP else 0 if p == 0 else (k + s + b) % 2
                rows.append((1, side, 5 + k + 9 * s, 1, p, 0))
            if s:
                rows.append((2, 0, 0, 0, 0, b + s))
            off.append(len(rows))
        ins = [np.array(c, dtype=t) for c, t in zip(zip(*rows), (np.uint32, np.uint8, np.uint32, np.uint32, np.uint32, np.uint64))]
        ids = env.submit_instructions_all(np.array(off, dtype=np.uint64), ins)
        for b in range(B):
            sl = slice(off[b], off[b + 1])
            assert np.array_equal(ids[sl], oracle.StepEnvNumpy.submit_instructions(refs[b], [x[sl] for x in ins])), b
        env.step()
        for r in refs:
            r.step()
    _check_host(env, refs, U32 - 3, 1000, T, rule=(5, 1))
    env.close()


@pytest.mark.parametrize("pipeline", AGENT_PIPELINES)
def test_random_agents_top_price_u32_max_minus_1(bk, oracle, pipeline):
    groups = [(16, (2**31 - 20, 2**31), (1, 30), 2, 0.8), (16, (2**31 - 12, 2**31), (1, 30), 2, 0.5)]
    hist = _run_agents(bk, oracle, 6, 14, groups=groups, pipeline=pipeline)
    assert (hist[:, :, 2] == MAXP - 1).any() or (hist[:, :, 1] == MAXP - 1).any()


@pytest.mark.parametrize("levels", [1, 5, 64])
@pytest.mark.parametrize("tick", [t for t in HUGE_TICKS if t in AGENT_TICK_RANGE], ids=str)
def test_random_agents_at_huge_env_ticks(bk, oracle, tick, levels):
    lo, hi = AGENT_TICK_RANGE[tick]
    groups = [(16, (lo, hi), (1, 40), tick, 0.8), (12, (lo, hi), (1, 40), tick, 0.4)]
    for pipeline in AGENT_PIPELINES:
        _run_agents(bk, oracle, 4, 10, tick=tick, levels=levels, groups=groups, pipeline=pipeline, check_rule=True)


def _tick_prices(tick):
    """Legal limit prices at a tick (multiples below u32::MAX, as many as there are up to 8) and the two extremes."""
    ks = [k for k in range(1, 9) if k * tick < MAXP] or [0]
    return [k * tick for k in ks]


@pytest.mark.parametrize("levels", [1, 5, 64])
@pytest.mark.parametrize("tick", HUGE_TICKS, ids=str)
def test_host_driven_steps_at_huge_ticks(bk, oracle, tick, levels):
    B, T = 4, 6
    env, refs = _host_env(bk, oracle, B, T, 0, 1000, tick, levels)
    prices = _tick_prices(tick)
    rng = np.random.default_rng(tick % 1000 + levels)
    made = [0] * B
    for _ in range(T):
        for b in range(B):
            ops, made[b] = _random_ops(rng, made[b], prices, list(range(1, 20)), int(rng.integers(3, 12)), p_market=0.05)
            if tick == MAXP:  # no legal limit price: the extremes 0 / u32::MAX are multiples (market orders)
                ops = [("place_order", (bool(k % 2), 3 + k, 1, MAXP if k % 2 else 0)) for k in range(4)]
            _apply(env, refs, b, ops)
        env.step()
        for r in refs:
            r.step()
    _check_host(env, refs, rule=(levels, tick))
    env.close()


@pytest.mark.parametrize("tick", [2**30, 2**31, 2**31 - 1, 2**16 + 1], ids=str)
def test_immediate_order_book_and_load_book_state_at_huge_ticks(bk, oracle, tick):
    """core.OrderBook (one event per call) and bk_load_book's host-side level 2 at a huge tick: both follow the rule."""
    prices = _tick_prices(tick)
    g, o = bk.core.OrderBook(0, tick), oracle.OrderBook(0, tick)
    L = bk.core.LEVELS
    rng = np.random.default_rng(8)
    for t in range(1, 40):
        for x in (g, o):
            x.set_time(t)
        n = len(o.get_orders())
        if n and rng.random() < 0.2:
            i = int(rng.integers(0, n))
            g.cancel_order(i)
            o.cancel_order(i)
        else:
            args = (bool(rng.integers(0, 2)), int(rng.integers(1, 20)), 1, int(rng.choice(prices)))
            assert g.place_order(*args) == o.place_order(*args)
        assert np.array_equal(g._l2()[1:], _l2_rule(o.orders_array(), L, tick)), t
    assert g.get_trades() == o.get_trades() and g.get_orders() == o.get_orders()
    st = o.state()
    env = bk.ManyBookEnv(2, 1, 0, tick, 1000, levels=5, max_live_orders=128, max_orders=256, trade_capacity=256)
    env.load_book_state(1, st)
    assert np.array_equal(env.level2()[1, 1:], _l2_rule(o.orders_array(), 5, tick))
    assert env.book_state(1) == st
    env.close()


def test_json_snapshot_with_a_53_bit_plus_time_round_trips(bk, oracle, tmp_path):
    import json

    t0 = 2**53 + 12_345
    g, o = bk.core.OrderBook(t0, 2), oracle.OrderBook(t0, 2)
    for k in range(30):
        for x in (g, o):
            x.set_time(t0 + 3 * k)
        args = (k % 2 == 0, 5 + k, 1, 2 * (48 + (k % 7)))
        assert g.place_order(*args) == o.place_order(*args)
    p = tmp_path / "s.json"
    g.save_json_snapshot(str(p))
    st = json.loads(p.read_text())
    assert st == o.state() and st["t"] > 2**53
    env = bk.ManyBookEnv(1, 1, 0, 2, 1000, levels=10, max_live_orders=128, max_orders=256, trade_capacity=256)
    env.load_book_state(0, st)
    assert env.time(0) == t0 + 87 and env.book_state(0) == st
    env.close()


@pytest.mark.parametrize("huge", [2**30, 2**31, 2**31 - 1])
def test_market_with_a_huge_tick_asset_beside_a_tick_1_asset(bk, oracle, huge):
    lo, hi = AGENT_TICK_RANGE[huge]
    groups = [(0, 16, (lo, hi), (1, 30), huge, 0.8), (1, 16, (40, 60), (1, 30), 1, 0.8)]
    NM, T, L = 4, 10, 5
    env = bk.ManyMarketEnv(NM, SEED, 0, [huge, 1], 1000, True, levels=L, max_live_orders=64, trade_capacity=2048,
                           history_capacity=T)
    env.set_random_market_agents(groups)
    env.run(T)
    ref = oracle.ManyMarkets(NM, SEED, 0, [huge, 1], 1000, True, L, groups)
    ref.run(T, n_threads=4)
    P.no_flags(env)
    h = env.history()
    P.same_history(h, ref.history())
    for m in range(NM):
        for a, tick in enumerate((huge, 1)):
            P.same_book(env, env.book(m, a), ref.book(m, a), tag=(m, a))
            assert np.array_equal(h[-1, env.book(m, a), 1:], _l2_rule(ref.book(m, a).orders_array(), L, tick)), (m, a)
    env.close()


# ------------------------------------------------------------------------------------------ sampling ranges
SAMPLING = {
    "width-1": [(16, (40, 41), (10, 11), 2, 0.8), (16, (41, 42), (7, 8), 2, 0.7)],
    "width-2": [(16, (40, 42), (10, 12), 2, 0.8), (16, (41, 43), (1, 3), 2, 0.7)],
    "width-2^k+1": [(16, (40, 57), (0, 2**31 + 1), 2, 0.8), (16, (40, 57), (5, 22), 2, 0.7)],
    "vol-width-2^32-1": [(16, (40, 56), (0, MAXP), 2, 0.8), (16, (40, 56), (1, MAXP), 2, 0.6)],
}


@pytest.mark.parametrize("pipeline", AGENT_PIPELINES)
@pytest.mark.parametrize("case", list(SAMPLING))
def test_sampling_range_edges(bk, oracle, case, pipeline):
    _run_agents(bk, oracle, 6, 12, groups=SAMPLING[case], pipeline=pipeline)


@pytest.mark.parametrize("lookahead", [1, 2])
@pytest.mark.parametrize("pipeline", ["wave_split", "wave"])
@pytest.mark.parametrize("case", list(SAMPLING))
def test_sampling_range_edges_small_lookahead(bk, oracle, case, pipeline, lookahead):
    _run_agents(bk, oracle, 6, 12, groups=SAMPLING[case], pipeline=pipeline, lookahead=lookahead)


# ------------------------------------------------------------------------------------------------ statistics
def _stats_from(env, books=None):
    l2 = env.level2().astype(np.uint64)
    tc = env.trade_counts().astype(np.uint64)
    want = dict(n_books=env.n_books, sum_trade_vol=int(l2[:, 0].sum()), sum_trades=int(tc.sum()),
                sum_bid_vol=int(l2[:, 4].sum()), sum_ask_vol=int(l2[:, 3].sum()))
    bids, asks = [], []
    for b in (range(env.n_books) if books is None else books):
        live = env.live_orders(b)
        if (live["side"] == 1).any():
            bids.append(int(live["price"][live["side"] == 1].max()))
        if (live["side"] == 0).any():
            asks.append(int(live["price"][live["side"] == 0].min()))
    return want, bids, asks


def test_stats_of_host_driven_books_with_wrapping_totals(bk, oracle):
    B, T = 12, 4
    env, refs = _host_env(bk, oracle, B, T, 0, 1000, 1, 5)
    n_ev = 0
    for s in range(T):
        for b in range(B):
            if b % 4 == 1:  # asks only
                ops = [("place_order", (False, MAXP - b - k, 1, 500 + 10 * b + k)) for k in range(2)]
            elif b % 4 == 2:  # bids only
                ops = [("place_order", (True, MAXP - k, 1, 100 + b + k + s)) for k in range(2)]
            elif b % 4 == 3:  # nothing rests
                ops = [] if s else [("place_order", (True, 5, 1, 10)), ("cancel_order", (0,))]
            else:
                ops = [("place_order", (True, 2**31 + k, 1, 100 + b + k)) for k in range(2)]
                ops += [("place_order", (False, 2**31 + 3, 2, 100 + b + 1)), ("place_order", (False, 7, 2, 300 + s))]
                if s:
                    ops.append(("modify_order", (1, None, 3)))
            n_ev += len(ops)
            _apply(env, refs, b, ops)
        env.step()
        for r in refs:
            r.step()
    _check_host(env, refs)
    st = env.stats()
    want, bids, asks = _stats_from(env)
    for k, v in want.items():
        assert st[k] == v, (k, st[k], v)
    assert st["sum_events"] == n_ev
    assert (st["min_bid"], st["max_bid"]) == (min(bids), max(bids))
    assert (st["min_ask"], st["max_ask"]) == (min(asks), max(asks))
    assert st["sum_bid_vol"] > U32 and st["sum_ask_vol"] > U32
    env.close()


def test_stats_grid_stride_over_300_000_books(bk):
    """More books than k_stats' grid covers in one pass (1 024 blocks x 256 threads)."""
    B, T = 300_000, 3
    env = bk.ManyBookEnv(B, 7, 0, 2, 1000, levels=1, max_live_orders=64, trade_capacity=16, history_capacity=0)
    env.set_random_agents([(1, (40, 60), (U32 - 9, MAXP), 2, 0.9)])
    env.run(T)
    P.no_flags(env)
    st = env.stats()
    l2 = env.level2().astype(np.uint64)
    assert st["n_books"] == B
    assert st["sum_trade_vol"] == int(l2[:, 0].sum()) and st["sum_trades"] == int(env.trade_counts().sum())
    assert st["sum_bid_vol"] == int(l2[:, 4].sum()) and st["sum_ask_vol"] == int(l2[:, 3].sum())
    bid_ok = (l2[:, 4] != 0) | (l2[:, 6] != 0)
    ask_ok = (l2[:, 3] != 0) | (l2[:, 8] != 0)
    assert bid_ok.any() and ask_ok.any()
    assert (st["min_bid"], st["max_bid"]) == (int(l2[bid_ok, 1].min()), int(l2[bid_ok, 1].max()))
    assert (st["min_ask"], st["max_ask"]) == (int(l2[ask_ok, 2].min()), int(l2[ask_ok, 2].max()))
    # books past the first pass of the grid hold orders too
    assert bid_ok[262_144:].any() and ask_ok[262_144:].any()
    env.close()
