"""Cost of per-book AgentSet member parameters (bk_set_agents_per_book): book-steps/s of bk_run with the uniform members,
with a table whose rows are all the uniform members, and with a heterogeneous table (every book's probabilities, price
distribution, momentum parameters and tick size drawn around the uniform ones; same kinds and sizes), set up as bench.py
sets up C5M (momentum 256 + noise 256 agents, 64 levels, the pool min(512, agents)):
  C5M     8 192 books (wave_split: k_agents_mixed_wave)
  C5M256  256 books (fused: k_run_mixed)
  MKT2    2 048 two-asset markets of the same members, one per asset (the lane kernel k_agents_mixed_lanes<R, true>)
bench.py's trade and history capacities, 50 steps per launch with the records drained in between.  The three arms are three
envs of the same seed, timed ALTERNATELY region by region; before every region the env's own bk_warm steps (state restored)
keep the clocks up, as bench.py's pre-heat does.  Also prints the agents kernel's time per launch (HIP events).

usage: python scripts/mixed_per_book_rate.py [C5M|C5M256|MKT2 ...] [--regions N]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import bourse_amd  # noqa: E402

MOM_P = dict(tick_size=2, p_cancel=0.1, trade_vol=100, decay=1.0, demand=20.0, scale=0.5, order_ratio=1.0,
             price_dist_mu=0.0, price_dist_sigma=10.0)
NOISE_P = dict(tick_size=2, p_limit=0.3, p_market=0.2, p_cancel=0.2, trade_vol=100, price_dist_mu=0.0, price_dist_sigma=1.0)
MEMBERS = [("momentum", 0, 256, MOM_P), ("noise", 256, 256, NOISE_P)]  # bench.py WORKLOADS["C5M"]
WORKLOADS = {"C5M": (8192, 1, 64), "C5M256": (256, 1, 64), "MKT2": (2048, 2, 64)}  # units, assets, levels
ARMS = ("uniform", "same_rows", "heterogeneous")
SPL, WARMUP, TICK = 50, 10, 2


def het_member(m, r):
    kind, start, n, p = m
    q = dict(p, tick_size=TICK * int(r.integers(1, 3)), p_cancel=float(np.clip(p["p_cancel"] + r.uniform(-0.05, 0.05), 0, 1)),
             price_dist_sigma=p["price_dist_sigma"] * float(r.uniform(0.8, 1.2)))
    if kind == "noise":
        q.update(p_limit=float(np.clip(p["p_limit"] + r.uniform(-0.1, 0.1), 0, 1)),
                 p_market=float(np.clip(p["p_market"] + r.uniform(-0.1, 0.1), 0, 1)))
    else:
        q.update(decay=float(r.uniform(0.5, 1.0)), demand=p["demand"] * float(r.uniform(0.8, 1.2)),
                 scale=p["scale"] * float(r.uniform(0.8, 1.2)), order_ratio=float(r.uniform(0.5, 1.5)))
    return (kind, start, n, q)


def make(name, arm):
    U, A, levels = WORKLOADS[name]
    n = sum(m[2] for m in MEMBERS)
    kw = dict(levels=levels, max_live_orders=min(n, 512), trade_capacity=max(64, n // 2 * 3 // 2) * SPL, history_capacity=SPL,
              strict=False)
    if A > 1:
        env = bourse_amd.ManyMarketEnv(U, 101, 0, [TICK] * A, 100_000, True, **kw)
        members = [(i % A, m) for i, m in enumerate(MEMBERS)]
    else:
        env = bourse_amd.ManyBookEnv(U, 101, 0, TICK, 100_000, True, **kw)
        members = MEMBERS
    r = np.random.default_rng(5)
    rows = [[(a, het_member(m, r)) for a, m in members] if A > 1 else [het_member(m, r) for m in members] for _ in range(U)]
    if arm == "uniform":
        env.set_market_agents(members) if A > 1 else env.set_agents(members)
    else:
        rows = rows if arm == "heterogeneous" else [members] * U
        env.set_market_agents_per_market(rows) if A > 1 else env.set_agents_per_book(rows)
    env.run(WARMUP)
    return env


def preheat(env, ms=200.0):
    t0 = time.perf_counter()
    while (time.perf_counter() - t0) * 1e3 < ms:
        env.warm(20)
        env.sync()


def region(env):
    env.clear_history()
    env.clear_trades()
    preheat(env)
    t = time.perf_counter()
    env.run(SPL)
    return env.n_books * SPL / (time.perf_counter() - t) / 1e6


def kernel_us(env, kind):
    env.clear_history()
    env.clear_trades()
    preheat(env)
    env.profile(1)
    env.run(SPL)
    ms, n = env.profile_read_kind(kind)
    env.profile(0)
    return ms / n * 1e3 if n else float("nan")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("configs", nargs="*", default=["C5M", "C5M256", "MKT2"])
    ap.add_argument("--regions", type=int, default=4)
    args = ap.parse_args()
    for name in args.configs:
        envs = {arm: make(name, arm) for arm in ARMS}
        rates = {arm: [] for arm in ARMS}
        for _ in range(args.regions):
            for arm in ARMS:
                rates[arm].append(region(envs[arm]))
        for arm in ARMS:
            env = envs[arm]
            pipe = env.pipeline()
            kind = 0 if pipe[0] == "fused" else 1  # (the fused kernel, or the split forms' agents kernel)
            us = kernel_us(env, kind)
            r = rates[arm]
            print(f"{name} {arm:13s} {pipe[0]}x{pipe[1]}: {np.median(r):7.2f} M book-steps/s (regions "
                  f"{' '.join(f'{x:.2f}' for x in r)}); {'k_run_mixed' if kind == 0 else 'agents kernel'} {us:8.1f} us/launch",
                  flush=True)
        for env in envs.values():
            env.close()


if __name__ == "__main__":
    main()
