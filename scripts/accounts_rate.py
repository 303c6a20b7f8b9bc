"""Cost of the trader accounts (bk_accounts_enable: accounts::k_fold behind every step's event kernel), priced against the
same library with accounts off.  Two envs of one shape take the IDENTICAL flow, one with accounts and one without; the two
are timed ALTERNATELY region by region after one untimed warm-up region each (both see the same clocks).  A region is
`iters` steps queued back to back on the env's stream and one synchronise at the end (host clock); after it every book goes
back to an ingress snapshot of the fresh env (untimed), so that every region runs the same steps.  Arms:
  a  bench.py --workload INGRESS's flow (48 instructions per book-step: 30 % cancellations of earlier ids, the rest new
     limit orders at 90..110; bench.ingress_batch) at 65 536 books, 512-slot pools
  b  the same flow at 8 192 books, 256-slot pools
  c  a flow that never trades (the same stream with every new order a bid) at 65 536 books: every wave of the fold takes
     the early-out - four header words and the cursor per book
  d  update_members + step with bench.py's C5M set (256 momentum + 256 noise traders, 512-slot pools, 64 levels) at 8 192
     books, n_traders = 512 (scripts/ingress_reset_rate.py's c5m shape)
The benchmark's flow gives every order trader 0; here the trader ids are uniform in 0 .. --traders - 1 (default 16, which
is also n_traders), the same array for both envs - `--traders 1` is the benchmark's array, every party of a chunk on one row.
Reported per arm, one JSON line: the medians of the regions in microseconds per step, off and on, and their difference -
what the fold adds to a step; trades per book-step; `must_bytes_per_step`, what the fold has to move: 16 B of header words
and 8 B of cursor per book, 32 B per new record plus two 16 B order look-ups, and 64 B (read + write) per touched row, the
rows counted as min(n_traders, 2 x records) per book-step - an upper estimate.  The kernel's own time per launch:
  rocprofv3 --kernel-trace --stats -- python scripts/accounts_rate.py --arms a --regions 2
and `must_bytes_per_step` over that time is the rate to set against the memory system's.

usage: python scripts/accounts_rate.py [--arms a,b,c,d] [--regions N] [--iters N] [--traders N] [--books N]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import bourse_amd as bk  # noqa: E402

MOM_P = dict(tick_size=2, p_cancel=0.1, trade_vol=100, decay=1.0, demand=20.0, scale=0.5, order_ratio=1.0,
             price_dist_mu=0.0, price_dist_sigma=10.0)
NOISE_P = dict(tick_size=2, p_limit=0.3, p_market=0.2, p_cancel=0.2, trade_vol=100, price_dist_mu=0.0, price_dist_sigma=1.0)
C5M = [("momentum", 0, 256, MOM_P), ("noise", 256, 256, NOISE_P)]
ARMS = {"a": ("ingress", 65536), "b": ("ingress", 8192), "c": ("idle", 65536), "d": ("members", 8192)}
N, STEP = bench.INGRESS_N, 100_000


class IngressArm:
    """bench.py's INGRESS stream (or, `idle`, the same with every new order a bid) through submit + step"""

    def __init__(self, B, iters, n_traders, idle):
        self.B, self.iters, self.n_traders = B, iters, n_traders
        g = torch.Generator(device="cuda").manual_seed(0)
        self.off = torch.arange(B + 1, dtype=torch.int64, device="cuda") * N
        self.batches = []
        for s in range(iters):
            action, side, vol, trader, price, ids = bench.ingress_batch(torch, g, B * N, N, s)
            if idle:
                side = torch.ones_like(side)
            trader = torch.randint(0, n_traders, (B * N,), device="cuda", generator=g, dtype=torch.int32)
            self.batches.append((action, side, vol, trader, price, ids))

    def env(self, accounts):
        pool = 512 if self.B > 8192 else 256
        e = bk.ManyBookEnv(self.B, 1, 0, 1, STEP, levels=16, max_live_orders=pool, max_orders=N * (self.iters + 8),
                           trade_capacity=64 * (self.iters + 8), strict=False, history_capacity=0,
                           stream=torch.cuda.current_stream().cuda_stream)
        e.enable_device_ingress(N)
        if accounts:
            e.enable_accounts(self.n_traders)
        return e

    def run(self, e):
        for b in self.batches:
            e.submit_instructions_device(self.off, *b)
            e.step(sync=False)


class MembersArm:
    def __init__(self, B, iters, n_traders):
        self.B, self.iters, self.n_traders = B, iters, 512

    def env(self, accounts):
        per_update = sum(2 * m[2] for m in C5M)
        e = bk.ManyBookEnv(self.B, 101, 0, 2, STEP, levels=64, max_live_orders=512, max_orders=per_update // 2 * (self.iters + 2),
                           trade_capacity=per_update * (self.iters + 1), strict=False, history_capacity=0,
                           stream=torch.cuda.current_stream().cuda_stream)
        e.enable_device_ingress(per_update + 512)
        e.set_agents(C5M)
        if accounts:
            e.enable_accounts(self.n_traders)
        return e

    def run(self, e):
        for _ in range(self.iters):
            e.update_members(sync=False)
            e.step(sync=False)


def region(arm, e, every):
    """microseconds per step of one region; every book back to the fresh env after (untimed)"""
    e.sync()
    t = time.perf_counter()
    arm.run(e)
    e.sync()
    us = (time.perf_counter() - t) / arm.iters * 1e6
    trades = int(e.trade_counts().sum())
    e.reset_ingress_books(every, sync=True)
    return us, trades


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arms", default="a,b,c,d")
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--iters", type=int, default=24, help="steps per region (the INGRESS stream fills the pools: <= 33)")
    ap.add_argument("--traders", type=int, default=16)
    ap.add_argument("--books", type=int, default=0, help="override the arm's book count (a rehearsal)")
    args = ap.parse_args()
    for name in (a for a in args.arms.split(",") if a):
        kind, B = ARMS[name]
        B = args.books or B
        arm = MembersArm(B, args.iters, args.traders) if kind == "members" else IngressArm(B, args.iters, args.traders, kind == "idle")
        envs = {"off": arm.env(False), "on": arm.env(True)}
        every = torch.ones(B, dtype=torch.uint8, device="cuda")
        for e in envs.values():
            e.save_ingress_snapshot()
            region(arm, e, every)  # the warm-up
        us, trades = {"off": [], "on": []}, {}
        for _ in range(args.regions):
            for k, e in envs.items():
                t, trades[k] = region(arm, e, every)
                us[k].append(t)
        assert trades["off"] == trades["on"], trades  # the identical flow
        med = {k: float(np.median(v)) for k, v in us.items()}
        tr = trades["on"] / (B * arm.iters)  # per book-step
        must = B * 24 + B * tr * 64 + B * min(arm.n_traders, 2 * tr) * 64
        # one more region on the env with accounts, kept: the rows against the flags (an inexact row would be flagged)
        arm.run(envs["on"])
        rows = envs["on"].accounts()
        out = dict(arm=name, flow=kind, books=B, n_traders=arm.n_traders, iters=arm.iters, trades_per_book_step=round(tr, 3),
                   us_per_step={k: round(v, 1) for k, v in med.items()}, fold_adds_us=round(med["on"] - med["off"], 1),
                   regions={k: [round(x, 1) for x in v] for k, v in us.items()}, must_bytes_per_step=int(must),
                   fills=int(rows["fills"].sum()), flags=int(np.bitwise_or.reduce(envs["on"].flags())))
        print(json.dumps(out), flush=True)
        for e in envs.values():
            e.close()


if __name__ == "__main__":
    main()
