"""Cost of the agents' order log (bk_set_agent_order_log): book-steps/s of bk_run with and without it, set up as bench.py
sets up its workloads (C2: 4 096 books x 64 agents, 16 levels - k_run_wave without the log, wave_split with it; C3: 65 536
books x 128 agents, 32 levels - the lane split either way; bench.py's trade and history capacities, 50 steps per launch
with the records drained in between), and the event kernel's time per launch (HIP events: k_step_batch without the log,
k_step_batch_log with it).

The two arms are two envs of the same seed, timed ALTERNATELY, region by region; before every region the env's own
bk_warm steps (state restored) keep the clocks up, as bench.py's pre-heat does.  A region is one 50-step launch after 10
warm-up steps.  The log's capacity is sized for every order of the run (~0.4 new orders per agent and step, measured).

usage: python scripts/agent_order_log_rate.py [C2|C3 ...] [--regions N]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import bourse_amd  # noqa: E402

WORKLOADS = {  # books, levels, groups: bench.py WORKLOADS
    "C2": (4096, 16, [(32, (40, 56), (10, 20), 2, 0.8), (32, (40, 56), (50, 70), 2, 0.2)]),
    "C3": (65536, 32, [(64, (32, 64), (10, 20), 2, 0.8), (64, (32, 64), (50, 70), 2, 0.2)]),
}
SPL, WARMUP = 50, 10


def make(name, log, regions):
    B, levels, groups = WORKLOADS[name]
    n = sum(g[0] for g in groups)
    steps = WARMUP + SPL * (regions + 1)  # (+1: the profiled region)
    env = bourse_amd.ManyBookEnv(B, 101, 0, 2, 100_000, True, levels=levels, max_live_orders=n,
                                 max_orders=int(0.45 * n * steps) if log else 0,
                                 trade_capacity=max(64, n // 2 * 3 // 2) * SPL, history_capacity=SPL, strict=False)
    env.set_random_agents(groups)
    if log:
        env.enable_agent_order_log()
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


def kernel_us(env):
    env.clear_history()
    env.clear_trades()
    preheat(env)
    env.profile(1)
    env.run(SPL)
    ms, n = env.profile_read_kind(2)
    env.profile(0)
    return ms / n * 1e3 if n else float("nan")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("configs", nargs="*", default=["C2", "C3"])
    ap.add_argument("--regions", type=int, default=4)
    args = ap.parse_args()
    for name in args.configs:
        envs = {log: make(name, log, args.regions) for log in (False, True)}
        rates = {False: [], True: []}
        for _ in range(args.regions):
            for log in (False, True):
                rates[log].append(region(envs[log]))
        for log in (False, True):
            env = envs[log]
            us = kernel_us(env)
            full = int(np.bitwise_or.reduce(env.flags())) & bourse_amd._lib.FLAG_ORDER_LOG_FULL
            pipe = env.pipeline()
            r = rates[log]
            print(f"{name} log={int(log)} {pipe[0]}x{pipe[1]}: {np.median(r):7.2f} M book-steps/s (regions {' '.join(f'{x:.2f}' for x in r)}); "
                  f"{'k_step_batch_log' if log else 'k_step_batch'} {us:7.1f} us/launch{' (LOG FULL)' if full else ''}", flush=True)
            env.close()


if __name__ == "__main__":
    main()
