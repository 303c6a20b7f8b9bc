"""What the GPU tests of bk_update_market_agents / bk_update_market_members share: the market env they build, how one
step's instructions reach the device and oracle.ManyMarkets, and the comparison of every book (m, a) with
ManyMarkets.book(m, a) through tests/oracle_parity.py - level-2 history, trades, live orders in priority order, the order
log, the keys - and of the RNG words of every book of a market with rng_states()[m]."""
import numpy as np

import oracle_parity as P
from ingress_support import MOD, SEED, STEP, submit

LEVELS = 10


def market_env(bk, torch, NM, ticks, T, pool, qcap, n_orders, strict=True, seed=SEED):
    env = bk.ManyMarketEnv(NM, seed, 0, ticks, STEP, levels=LEVELS, max_live_orders=pool, max_orders=n_orders,
                           trade_capacity=2 * n_orders, history_capacity=T, strict=strict,
                           stream=torch.cuda.current_stream().cuda_stream)
    env.enable_device_ingress(queue_capacity=qcap)
    return env


def many_markets(oracle, NM, ticks, seed=SEED, **kw):
    return oracle.ManyMarkets(NM, seed, 0, ticks, STEP, True, LEVELS, **kw)


def check_markets(env, ref_of, markets=None):
    """market m of the env against market `i` of `ref`, (ref, i) = ref_of(m)"""
    env.sync()
    hist, A = env.history(), env.assets
    hists = {}
    for m in (range(env.n_markets) if markets is None else markets):
        ref, i = ref_of(m)
        want_hist = hists.setdefault(id(ref), ref.history())
        want_rng = tuple(int(x) for x in ref.rng_states()[i])
        for a in range(A):
            b, tag = m * A + a, (m, a)
            P.same_history(hist[:, b], want_hist[:, i * A + a], f"L2 history of market {m}, asset {a}")
            P.same_book(env, b, ref.book(i, a), orders=True, keys=True, tag=tag)
            assert env.rng_state(b) == want_rng, f"{tag}: rng state {env.rng_state(b)} vs {want_rng}"


def apply_market(ref, i, a, lo, hi, ins):
    """elements [lo, hi) of one book's batch on market i, asset a of a ManyMarkets"""
    action, side, vol, trader, price, order_id = ins
    for k in range(lo, hi):
        act = int(action[k])
        if act == 1:
            ref.place_order(i, a, bool(side[k] & 1), int(vol[k]), int(trader[k]), price=int(price[k]))
        elif act == 2:
            ref.cancel_order(i, a, int(order_id[k]))
        elif act == MOD:
            ref.modify_order(i, a, int(order_id[k]), new_price=int(price[k]) if side[k] & 2 else None,
                             new_vol=int(vol[k]) if side[k] & 4 else None)


def submit_markets(torch, env, ref_of, off, ins):
    """one step's instructions (offsets over the flat books) to the device and, book by book in the device's order - a
    market's assets in turn - to the oracle"""
    submit(torch, env, off, ins)
    A = env.assets
    for b in range(env.n_books):
        ref, i = ref_of(b // A)
        apply_market(ref, i, b % A, int(off[b]), int(off[b + 1]), ins)


def external(rng, n0, ticks, n_max, new_only=False, band=(30, 68)):
    """up to n_max instructions per book: limit orders on the book's tick grid and (unless new_only) cancellations and
    modifications of ids the book had before this step (n0[b]).  Returns (offsets, arrays, cancel / modify targets)."""
    B, A = len(n0), len(ticks)
    n_b = rng.integers(0, n_max + 1, size=B)
    off = np.zeros(B + 1, dtype=np.int64)
    off[1:] = np.cumsum(n_b)
    n = int(off[-1])
    book = np.repeat(np.arange(B), n_b)
    tick = np.asarray(ticks, dtype=np.int64)[book % A]
    action = (np.ones(n) if new_only else rng.choice([1, 2, MOD], size=n, p=[0.5, 0.25, 0.25])).astype(np.uint32)
    bid = rng.integers(0, 2, size=n).astype(np.uint8)
    has_p, has_v = rng.integers(0, 2, size=n).astype(np.uint8), rng.integers(0, 2, size=n).astype(np.uint8)
    side = np.where(action == MOD, (has_p << 1) | (has_v << 2), bid).astype(np.uint8)
    vol = rng.integers(1, 40, size=n).astype(np.uint32)
    trader = rng.integers(5000, 6000, size=n).astype(np.uint32)
    price = (rng.integers(band[0], band[1], size=n) * 2 * tick).astype(np.uint32)
    order_id = np.zeros(n, dtype=np.uint64)
    targets = 0
    for k in range(n):
        if action[k] == 1:
            continue
        if n0[book[k]] == 0:
            action[k] = 0  # nothing to target yet: a no-op
            continue
        order_id[k] = rng.integers(0, n0[book[k]])
        targets += 1
    return off, (action, side, vol, trader, price, order_id), targets
