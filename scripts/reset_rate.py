"""Cost of the per-book reset (bk_snapshot_save / bk_reset_books_device), set up as bench.py sets up its workloads:
  C3     65 536 books x 128 agents, 32 levels (RandomAgents)
  C5M    8 192 books x 512 agents, 64 levels (256 momentum + 256 noise members: the members' lists are rebuilt by the run
         after every reset)
One env per workload, a snapshot saved after the warm-up steps, and the arms timed ALTERNATELY region by region - before
every region the env's own bk_warm steps keep the clocks up, as bench.py's pre-heat does.  A region is ITERS iterations
queued back to back on the env's stream and one synchronise at the end (host clock):
  run          bk_run(1) alone
  ask          bk_run(1) + bk_reset_books_device with an all-zero mask: the cost of asking
  reset_1pct   the same with 1 % of the books masked
  reset_all    the same with every book masked
  reset_only   bk_reset_books_device alone, every book masked (no run in between: the copy kernel by itself, whose bytes
               2 * n_books * (stride + W) * 4 over its time is compared with the 8 TB/s HBM peak)
and, for scale, the way through the host: ManyBookEnv.checkpoint() and restore() of the same env, each timed whole.
On C5M "ask - run - reset_only(no mask)" is what the members' list rebuild costs the next run.

usage: python scripts/reset_rate.py [C3|C5M ...] [--regions N] [--iters N]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bourse_amd  # noqa: E402

HBM_PEAK_GBPS = 8000.0  # bench.py's
MOM_P = dict(tick_size=2, p_cancel=0.1, trade_vol=100, decay=1.0, demand=20.0, scale=0.5, order_ratio=1.0,
             price_dist_mu=0.0, price_dist_sigma=10.0)
NOISE_P = dict(tick_size=2, p_limit=0.3, p_market=0.2, p_cancel=0.2, trade_vol=100, price_dist_mu=0.0, price_dist_sigma=1.0)
WORKLOADS = {  # books, levels, agents: bench.py WORKLOADS
    "C3": (65536, 32, [(64, (32, 64), (10, 20), 2, 0.8), (64, (32, 64), (50, 70), 2, 0.2)]),
    "C5M": (8192, 64, [("momentum", 0, 256, MOM_P), ("noise", 256, 256, NOISE_P)]),
}
ARMS = ("run", "ask", "reset_1pct", "reset_all")
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
        env.set_agents(groups)
    else:
        env.set_random_agents(groups)
    env.run(WARMUP)
    return env


def preheat(env, ms=200.0):
    t0 = time.perf_counter()
    while (time.perf_counter() - t0) * 1e3 < ms:
        env.warm(50)
        env.sync()


def region(env, iters, mask, run=True):
    """Microseconds per iteration of [bk_run(1)] [+ reset with `mask`]."""
    env.clear_history()
    env.clear_trades()
    preheat(env)
    t = time.perf_counter()
    for _ in range(iters):
        if run:
            env.run(1, sync=False)
        if mask is not None:
            env.reset_books(mask, sync=False)
    env.sync()
    return (time.perf_counter() - t) / iters * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("configs", nargs="*", default=["C3", "C5M"])
    ap.add_argument("--regions", type=int, default=4)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--books", type=int, default=0, help="override the workload's book count (a rehearsal)")
    args = ap.parse_args()
    for name in args.configs:
        env = make(name, args.iters, args.books)
        B = env.n_books
        env.save_snapshot()
        r = np.random.default_rng(5)
        one = np.zeros(B, dtype=np.uint8)
        one[r.choice(B, max(1, B // 100), replace=False)] = 1
        masks = {"run": None, "ask": torch.zeros(B, dtype=torch.uint8, device="cuda"),
                 "reset_1pct": torch.tensor(one, device="cuda"), "reset_all": torch.ones(B, dtype=torch.uint8, device="cuda")}
        us = {arm: [] for arm in ARMS}
        only = {"ask": [], "reset_all": []}
        for _ in range(args.regions):
            for arm in ARMS:
                us[arm].append(region(env, args.iters, masks[arm]))
            for arm in only:
                only[arm].append(region(env, args.iters, masks[arm], run=False))
        med = {arm: float(np.median(v)) for arm, v in us.items()}
        pipe = env.pipeline()
        print(f"{name} {B} books {pipe[0]}x{pipe[1]}: snapshot {env.snapshot_bytes() / 1e6:.1f} MB per slot", flush=True)
        for arm in ARMS:
            print(f"{name} {arm:11s} {med[arm]:9.1f} us/iteration ({B / med[arm]:7.2f} M book-steps/s; regions "
                  f"{' '.join(f'{x:.1f}' for x in us[arm])}); over run alone {med[arm] - med['run']:+8.1f} us", flush=True)
        k_ask, k_all = float(np.median(only["ask"])), float(np.median(only["reset_all"]))
        moved = 2 * env.snapshot_bytes()
        print(f"{name} reset_only  no mask {k_ask:8.1f} us/launch; every book {k_all:8.1f} us/launch = "
              f"{moved / k_all / 1e3:7.1f} GB/s read + written = {100 * moved / k_all / 1e3 / HBM_PEAK_GBPS:5.1f} % of "
              f"{HBM_PEAK_GBPS / 1e3:.0f} TB/s (regions {' '.join(f'{x:.1f}' for x in only['reset_all'])})", flush=True)
        print(f"{name} list rebuild + launch gap the run after a reset pays: ask - run - reset_only(no mask) = "
              f"{med['ask'] - med['run'] - k_ask:+8.1f} us", flush=True)
        # the way through the host, for scale
        env.sync()
        host = []
        for _ in range(2):
            t = time.perf_counter()
            image = env.checkpoint()
            t1 = time.perf_counter()
            env.restore(image)
            env.sync()
            host.append(((t1 - t) * 1e3, (time.perf_counter() - t1) * 1e3))
        print(f"{name} through the host: checkpoint {min(h[0] for h in host):8.1f} ms, restore {min(h[1] for h in host):8.1f} ms "
              f"({len(image) / 1e6:.1f} MB)", flush=True)
        env.close()


if __name__ == "__main__":
    main()
