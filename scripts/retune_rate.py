"""Cost of a retune (bk_retune_random_agents_device / bk_retune_agents_device) in front of a one-step run, set up as bench.py
sets up its workloads:
  C3     65 536 books x 128 agents, 32 levels: its two RandomAgents groups as a per-book table of identical rows
  C5M    8 192 books x 512 agents, 64 levels: its two members (256 momentum + 256 noise) the same way
One env per workload, and the arms timed ALTERNATELY region by region - before every region the env's own bk_warm steps
keep the clocks up, as bench.py's pre-heat does.  A region is ITERS iterations queued back to back on the env's stream and
one synchronise at the end (host clock):
  run           bk_run(1) alone: the same library without the call
  retune_none   device retune with an all-zero mask + bk_run(1): the cost of asking
  retune_1pct   the same with 1 % of the books masked
  retune_all    the same with every book masked
  retune_host   the host entry (every book: host checks, pinned + device staging, the same kernel) + bk_run(1)
  install       the only way before the retune: set_random_agents_per_book / set_agents_per_book of the full table from
                host memory + bk_run(1) (it also makes the agents forget what they hold)
  retune_only   the device retune alone, every book masked, no run in between: the kernel by itself, whose bytes
                (28 or 104 B in, 48 or 128 B out per entry, 1 B of mask, 8 B of status per book) are printed beside it

usage: python scripts/retune_rate.py [C3|C5M ...] [--regions N] [--iters N] [--books N]
"""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bourse_amd  # noqa: E402
from bourse_amd import _lib, env as E  # noqa: E402

MOM_P = dict(tick_size=2, p_cancel=0.1, trade_vol=100, decay=1.0, demand=20.0, scale=0.5, order_ratio=1.0,
             price_dist_mu=0.0, price_dist_sigma=10.0)
NOISE_P = dict(tick_size=2, p_limit=0.3, p_market=0.2, p_cancel=0.2, trade_vol=100, price_dist_mu=0.0, price_dist_sigma=1.0)
WORKLOADS = {  # books, levels, agents: bench.py WORKLOADS
    "C3": (65536, 32, [(64, (32, 64), (10, 20), 2, 0.8), (64, (32, 64), (50, 70), 2, 0.2)]),
    "C5M": (8192, 64, [("momentum", 0, 256, MOM_P), ("noise", 256, 256, NOISE_P)]),
}
ARMS = ("run", "retune_none", "retune_1pct", "retune_all", "retune_host", "install")
WARMUP = 10


def make(name, iters, books=None):
    B, levels, groups = WORKLOADS[name]
    B = books or B
    mixed = isinstance(groups[0][0], str)
    n = sum(g[2] if mixed else g[0] for g in groups)
    env = bourse_amd.ManyBookEnv(B, 101, 0, 2, 100_000, True, levels=levels, max_live_orders=min(n, 512),
                                 trade_capacity=max(64, n // 2 * 3 // 2) * iters, history_capacity=iters, strict=False,
                                 stream=torch.cuda.current_stream().cuda_stream)
    if mixed:
        host = E._members_rows([groups] * B, B)
        rows = C.cast(host.ctypes.data, C.POINTER(_lib.AgentDesc))
        install = lambda: env._L.bk_set_agents_per_book(env._h, host.shape[1], rows, None)  # noqa: E731
        retune = env.retune_agents
    else:
        host = E._agents_table([groups] * B, B, lambda g: g)
        install = lambda: env._L.bk_set_random_agents_per_book(env._h, host.shape[1], host.ctypes.data, None)  # noqa: E731
        retune = env.retune_random_agents
    assert install() == 0
    env.run(WARMUP)
    dev = torch.from_numpy(host.view(np.int32).reshape(B, host.shape[1], -1).copy()).cuda()
    return env, host, dev, install, retune


def preheat(env, ms=200.0):
    t0 = time.perf_counter()
    while (time.perf_counter() - t0) * 1e3 < ms:
        env.warm(50)
        env.sync()


def region(env, iters, before, run=True):
    """Microseconds per iteration of [`before`()] [+ bk_run(1)]."""
    env.clear_history()
    env.clear_trades()
    preheat(env)
    t = time.perf_counter()
    for _ in range(iters):
        if before is not None:
            before()
        if run:
            env.run(1, sync=False)
    env.sync()
    return (time.perf_counter() - t) / iters * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("configs", nargs="*", default=["C3", "C5M"])
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--books", type=int, default=0, help="override the workload's book count (a rehearsal)")
    args = ap.parse_args()
    for name in args.configs:
        env, host, dev, install, retune = make(name, args.iters, args.books)
        B, width = env.n_books, host.shape[1]
        r = np.random.default_rng(5)
        one = np.zeros(B, dtype=np.uint8)
        one[r.choice(B, max(1, B // 100), replace=False)] = 1
        masks = {"retune_none": torch.zeros(B, dtype=torch.uint8, device="cuda"), "retune_1pct": torch.tensor(one, device="cuda"),
                 "retune_all": torch.ones(B, dtype=torch.uint8, device="cuda")}
        status = torch.zeros((B, 2), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        before = {"run": None, "retune_host": lambda: retune(host, sync=False), "install": install}
        for arm, m in masks.items():
            before[arm] = lambda m=m: retune(dev, m, status, sync=False)
        us = {arm: [] for arm in ARMS}
        only = []
        for _ in range(args.regions):
            for arm in ARMS:
                us[arm].append(region(env, args.iters, before[arm]))
            only.append(region(env, args.iters, before["retune_all"], run=False))
        med = {arm: float(np.median(v)) for arm, v in us.items()}
        pipe = env.pipeline()
        print(f"{name} {B} books x {width} entries, {pipe[0]}x{pipe[1]}: table {host.nbytes / 1e6:.1f} MB of rows in, "
              f"{B * width * (128 if host.dtype.itemsize == 104 else 48) / 1e6:.1f} MB of records out", flush=True)
        for arm in ARMS:
            print(f"{name} {arm:12s} {med[arm]:9.1f} us/iteration (regions {' '.join(f'{x:.1f}' for x in us[arm])}); "
                  f"over run alone {med[arm] - med['run']:+9.1f} us", flush=True)
        k = float(np.median(only))
        moved = B * width * (host.dtype.itemsize + (128 if host.dtype.itemsize == 104 else 48) + 32) + B * 9
        print(f"{name} retune_only  every book {k:8.1f} us/launch, {moved / 1e6:.1f} MB read + written = {moved / k / 1e3:7.1f} GB/s "
              f"(regions {' '.join(f'{x:.1f}' for x in only)})", flush=True)
        assert env.retune_rejected() == 0
        env.close()


if __name__ == "__main__":
    main()
