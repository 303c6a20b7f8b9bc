"""Cost of the queue view (bk_open_queue_enable: open_queue::k_refresh behind open_orders::k_refresh behind every step's event
kernel), priced against the same library with the queue view off, on the pattern of scripts/open_orders_rate.py.  Two envs of
one shape take the IDENTICAL flow, BOTH with the open-order view, one with the queue view and one without; the two are timed
ALTERNATELY region by region after one untimed warm-up region each (both see the same clocks).  A region is `iters` steps
queued back to back on the env's stream and one synchronise at the end (host clock); after it every book goes back to an
ingress snapshot of the fresh env (untimed), so that every region runs the same steps.  Arms:
  a   bench.py --workload INGRESS's flow (48 instructions per book-step; bench.ingress_batch) with trader ids uniform in
      0..15 at 65 536 books, 512-slot pools, n_traders = 16, depth = 8
  b   the same flow at 8 192 books, 256-slot pools, depth = 8
  b1  the same with depth = 1 (16 entries a book: one pass, a quarter of a wave)
  d   update_members + step with bench.py's C5M set (256 momentum + 256 noise traders, 512-slot pools, 64 levels; their ids
      start at 1000) at 8 192 books beside the strategy's n_traders = 16, depth = 8: full pools, unused entries - the one
      ballot per pass is all the kernel does behind its loads
Reported per arm, one JSON line: the medians of the regions in microseconds per step, off and on, and their difference - what
the queue view adds; the listed entries and the resting orders of the traders with a row per book after a region; and `must_bytes_per_step`, what the
refresh has to move: five pool fields of every slot (20 B a slot), the book's entries read once (16 B each) and its rows
written once (32 B each).  The kernel's own time per launch, beside open_orders::k_refresh's in the same trace:
  rocprofv3 --kernel-trace --stats -- python scripts/open_queue_rate.py --arms a --regions 2

usage: python scripts/open_queue_rate.py [--arms a,b,b1,d] [--regions N] [--iters N] [--traders N] [--books N]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import open_orders_rate as OR  # noqa: E402  (the arms' envs and the timed region)

ARMS = {"a": ("ingress", 65536, 8), "b": ("ingress", 8192, 8), "b1": ("ingress", 8192, 1), "d": ("members", 8192, 8)}


def make_env(arm, queue):
    e = arm.env(True)  # the open-order view in both
    if queue:
        e.enable_open_queue()
    return e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arms", default="a,b,b1,d")
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--iters", type=int, default=24, help="steps per region (the INGRESS stream fills the pools: <= 33)")
    ap.add_argument("--traders", type=int, default=16)
    ap.add_argument("--books", type=int, default=0, help="override the arm's book count (a rehearsal)")
    args = ap.parse_args()
    for name in (a for a in args.arms.split(",") if a):
        kind, B, depth = ARMS[name]
        B = args.books or B
        arm = {"ingress": OR.IngressArm, "members": OR.MembersArm}[kind](B, args.iters, args.traders, depth)
        envs = {"off": make_env(arm, False), "on": make_env(arm, True)}
        every = torch.ones(B, dtype=torch.uint8, device="cuda")
        for e in envs.values():
            e.save_ingress_snapshot()
            OR.region(arm, e, every)  # the warm-up
        us, trades = {"off": [], "on": []}, {}
        for _ in range(args.regions):
            for k, e in envs.items():
                t, trades[k] = OR.region(arm, e, every)
                us[k].append(t)
        assert trades["off"] == trades["on"], trades  # the identical flow
        med = {k: float(np.median(v)) for k, v in us.items()}
        # one more region on the env with the view, kept: the rows it ends with
        arm.run(envs["on"])
        summary, entries = envs["on"].open_orders()
        queue = envs["on"].open_queue()
        listed = float((entries["order_id"] != 0xFFFFFFFF).sum()) / B
        assert not queue["level_vol"][entries["order_id"] == 0xFFFFFFFF].any()
        resting = float((summary["n_bid"].astype(np.int64) + summary["n_ask"]).sum()) / B
        must = B * (arm.pool * 20 + arm.n_traders * depth * (16 + 32))
        out = dict(arm=name, flow=kind, books=B, pool=arm.pool, n_traders=arm.n_traders, depth=depth, iters=arm.iters,
                   us={k: round(v, 1) for k, v in med.items()}, queue_adds_us=round(med["on"] - med["off"], 1),
                   regions={k: [round(x, 1) for x in v] for k, v in us.items()}, listed_per_book=round(listed, 2),
                   resting_in_rows_per_book=round(resting, 2), mean_ahead_orders=round(float(queue["ahead_orders"][entries["order_id"] != 0xFFFFFFFF].mean()), 1)
                   if listed else None, must_bytes_per_step=int(must), flags=int(np.bitwise_or.reduce(envs["on"].flags())))
        print(json.dumps(out), flush=True)
        for e in envs.values():
            e.close()


if __name__ == "__main__":
    main()
