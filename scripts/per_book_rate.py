"""Cost of per-book RandomAgents parameters (bk_set_random_agents_per_book): book-steps/s of bk_run with the uniform groups,
with a table whose rows are all the uniform groups, and with a heterogeneous table (every book's ranges, tick size and
activity drawn at random around the uniform ones; same group sizes), set up as bench.py sets up its workloads:
  C2     4 096 books x 64 agents, 16 levels (k_run_wave)
  SHARD  8 192 books x 128 agents, 32 levels (wave_split, the C3 groups on an 8 192-book shard)
  C3     65 536 books x 128 agents, 32 levels (split)
  C5     8 192 books x 512 agents, 64 levels (wave_split; the C5 stand-in)
bench.py's trade and history capacities, 50 steps per launch with the records drained in between.  The three arms are
three envs of the same seed, timed ALTERNATELY region by region; before every region the env's own bk_warm steps (state
restored) keep the clocks up, as bench.py's pre-heat does.  Also prints the agents kernel's time per launch (HIP events).

usage: python scripts/per_book_rate.py [C2|SHARD|C3|C5 ...] [--regions N]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import bourse_amd  # noqa: E402

C3G = [(64, (32, 64), (10, 20), 2, 0.8), (64, (32, 64), (50, 70), 2, 0.2)]
WORKLOADS = {  # books, levels, groups: bench.py WORKLOADS
    "C2": (4096, 16, [(32, (40, 56), (10, 20), 2, 0.8), (32, (40, 56), (50, 70), 2, 0.2)]),
    "SHARD": (8192, 32, C3G),
    "C3": (65536, 32, C3G),
    "C5": (8192, 64, [(256, (100, 164), (10, 20), 2, 0.8), (256, (100, 164), (50, 70), 2, 0.2)]),
}
ARMS = ("uniform", "same_rows", "heterogeneous")
SPL, WARMUP = 50, 10


def table(B, groups, arm):
    rows = np.zeros((B, len(groups)), dtype=bourse_amd.RANDOM_AGENTS_DTYPE)
    r = np.random.default_rng(5)
    for g, (n, tr, vr, ts, rate) in enumerate(groups):
        rows[:, g] = (n, tr[0], tr[1], vr[0], vr[1], ts, np.float32(rate))
        if arm == "heterogeneous":  # ranges shifted / widened per book, tick size 2 or 4, activity +-0.1
            lo = tr[0] + r.integers(-8, 9, B)
            rows["tick_lo"][:, g] = lo
            rows["tick_hi"][:, g] = lo + (tr[1] - tr[0]) + r.integers(-8, 9, B)
            rows["vol_hi"][:, g] = vr[1] + r.integers(0, 10, B)
            rows["tick_size"][:, g] = 2 * r.integers(1, 3, B)
            rows["activity_rate"][:, g] = np.clip(rate + r.uniform(-0.1, 0.1, B), 0, 1).astype(np.float32)
    return rows


def make(name, arm):
    B, levels, groups = WORKLOADS[name]
    n = sum(g[0] for g in groups)
    env = bourse_amd.ManyBookEnv(B, 101, 0, 2, 100_000, True, levels=levels, max_live_orders=n,
                                 trade_capacity=max(64, n // 2 * 3 // 2) * SPL, history_capacity=SPL, strict=False)
    if arm == "uniform":
        env.set_random_agents(groups)
    else:
        env.set_random_agents_per_book(table(B, groups, arm))
    env.run(WARMUP)
    return env


def preheat(env, ms=200.0):
    t0 = time.perf_counter()
    while (time.perf_counter() - t0) * 1e3 < ms:
        env.warm(50)
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
    ap.add_argument("configs", nargs="*", default=["C2", "SHARD", "C3", "C5"])
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
            kind = 0 if pipe[0] == "wave" else 1  # (the fused kernel, or the split forms' agents kernel)
            us = kernel_us(env, kind)
            r = rates[arm]
            print(f"{name} {arm:13s} {pipe[0]}x{pipe[1]}: {np.median(r):7.2f} M book-steps/s (regions "
                  f"{' '.join(f'{x:.2f}' for x in r)}); {'k_run_wave' if kind == 0 else 'agents kernel'} {us:8.1f} us/launch",
                  flush=True)
        for env in envs.values():
            env.close()


if __name__ == "__main__":
    main()
