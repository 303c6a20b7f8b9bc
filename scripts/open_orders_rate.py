"""Cost of the open-order view (bk_open_orders_enable: open_orders::k_refresh behind every step's event kernel), priced
against the same library with the view off, on the pattern of scripts/accounts_rate.py.  Two envs of one shape take the
IDENTICAL flow, one with the view and one without; the two are timed ALTERNATELY region by region after one untimed warm-up
region each (both see the same clocks).  A region is `iters` steps queued back to back on the env's stream and one
synchronise at the end (host clock); after it every book goes back to an ingress snapshot of the fresh env (untimed), so that
every region runs the same steps.  Arms:
  a   bench.py --workload INGRESS's flow (48 instructions per book-step; bench.ingress_batch) with trader ids uniform in
      0..15 at 65 536 books, 512-slot pools, n_traders = 16, depth = 8
  a0  the same with depth = 0 (summary rows only)
  b   the same flow at 8 192 books, 256-slot pools, depth = 8
  b0  the same with depth = 0
  d   update_members + step with bench.py's C5M set (256 momentum + 256 noise traders, 512-slot pools, 64 levels; their ids
      start at 1000) at 8 192 books beside the strategy's n_traders = 16, depth = 8: full pools, empty rows
  r   reset_ingress_books with an ALL-ZERO device mask on arm b's shape, `iters` calls per region: what the masked refresh
      adds to a reset that resets nothing
Reported per arm, one JSON line: the medians of the regions in microseconds per step (per call for r), off and on, and
their difference - what the view adds; the resting orders per book after a region (the rows' own counts); and
`must_bytes_per_step`, what the refresh has to move: four pool fields of every slot (16 B a slot), one 32-byte sector of
an order record per resting order, and the book's rows written once (n_traders x (32 + 16 x depth) B).  The kernel's own
time per launch:
  rocprofv3 --kernel-trace --stats -- python scripts/open_orders_rate.py --arms a --regions 2
and `must_bytes_per_step` over that time is the rate to set against the memory system's.

usage: python scripts/open_orders_rate.py [--arms a,a0,b,b0,d,r] [--regions N] [--iters N] [--traders N] [--books N]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import accounts_rate as AR  # noqa: E402  (the INGRESS stream and C5M's parameters)
import bourse_amd as bk  # noqa: E402

C5M = [("momentum", 1000, 256, AR.MOM_P), ("noise", 1256, 256, AR.NOISE_P)]
ARMS = {"a": ("ingress", 65536, 8), "a0": ("ingress", 65536, 0), "b": ("ingress", 8192, 8), "b0": ("ingress", 8192, 0),
        "d": ("members", 8192, 8), "r": ("reset", 8192, 8)}


class IngressArm(AR.IngressArm):
    def __init__(self, B, iters, n_traders, depth):
        super().__init__(B, iters, n_traders, False)
        self.depth, self.pool = depth, 512 if B > 8192 else 256

    def env(self, view):
        e = super().env(False)
        if view:
            e.enable_open_orders(self.n_traders, self.depth)
        return e


class MembersArm(AR.MembersArm):
    def __init__(self, B, iters, n_traders, depth):
        self.B, self.iters, self.n_traders, self.depth, self.pool = B, iters, n_traders, depth, 512

    def env(self, view):
        per_update = sum(2 * m[2] for m in C5M)
        e = bk.ManyBookEnv(self.B, 101, 0, 2, AR.STEP, levels=64, max_live_orders=512, max_orders=per_update // 2 * (self.iters + 2),
                           trade_capacity=per_update * (self.iters + 1), strict=False, history_capacity=0,
                           stream=torch.cuda.current_stream().cuda_stream)
        e.enable_device_ingress(per_update + 512)
        e.set_agents(C5M)
        if view:
            e.enable_open_orders(self.n_traders, self.depth)
        return e


class ResetArm(IngressArm):
    """`iters` resets that reset nothing, behind one region of the flow (so that the pools are not empty)"""

    def run(self, e):
        if not hasattr(self, "zero"):
            self.zero = torch.zeros(self.B, dtype=torch.uint8, device="cuda")
        for _ in range(self.iters):
            e.reset_ingress_books(self.zero, sync=False)


def region(arm, e, every):
    """microseconds per step (call) of one region; every book back to the fresh env after (untimed)"""
    if isinstance(arm, ResetArm):
        IngressArm.run(arm, e)
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
    ap.add_argument("--arms", default="a,a0,b,b0,d,r")
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--iters", type=int, default=24, help="steps per region (the INGRESS stream fills the pools: <= 33)")
    ap.add_argument("--traders", type=int, default=16)
    ap.add_argument("--books", type=int, default=0, help="override the arm's book count (a rehearsal)")
    args = ap.parse_args()
    for name in (a for a in args.arms.split(",") if a):
        kind, B, depth = ARMS[name]
        B = args.books or B
        arm = {"ingress": IngressArm, "members": MembersArm, "reset": ResetArm}[kind](B, args.iters, args.traders, depth)
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
        # one more region on the env with the view, kept: the rows it ends with
        (IngressArm.run if kind == "reset" else type(arm).run)(arm, envs["on"])
        summary, _ = envs["on"].open_orders()
        listed = float((summary["n_bid"].astype(np.int64) + summary["n_ask"]).sum()) / B
        must = B * (arm.pool * 16 + listed * 32 + arm.n_traders * (32 + 16 * depth))
        out = dict(arm=name, flow=kind, books=B, pool=arm.pool, n_traders=arm.n_traders, depth=depth, iters=arm.iters,
                   us={k: round(v, 1) for k, v in med.items()}, view_adds_us=round(med["on"] - med["off"], 1),
                   regions={k: [round(x, 1) for x in v] for k, v in us.items()}, resting_in_rows_per_book=round(listed, 2),
                   must_bytes_per_step=int(must), flags=int(np.bitwise_or.reduce(envs["on"].flags())))
        print(json.dumps(out), flush=True)
        for e in envs.values():
            e.close()


if __name__ == "__main__":
    main()
