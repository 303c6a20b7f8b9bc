"""Cost of the per-step trade bars (bk_trade_bars_enable: trade_bars::k_fold behind every step's event kernel), priced
against the same library with bars off, with the trader accounts' fold measured in the same run as the yardstick.  Three
envs of one shape take the IDENTICAL flow - nothing enabled, bars, accounts - and are timed ALTERNATELY region by region
after one untimed warm-up region each (all see the same clocks), exactly as scripts/accounts_rate.py times its two: a
region is `iters` steps queued back to back on the env's stream and one synchronise at the end (host clock); after it every
book goes back to an ingress snapshot of the fresh env (untimed), so that every region runs the same steps.  Arms:
  a  bench.py --workload INGRESS's flow (48 instructions per book-step; accounts_rate.py's arm a) at 65 536 books
  b  the same flow at 8 192 books
  c  a flow that never trades (every new order a bid) at 65 536 books: every wave of the bars' fold takes the idle path -
     the header words, the cursor, the previous close, and the 48-byte row it still has to write
Reported per arm, one JSON line: the medians of the regions in microseconds per step for each env, what the bars' fold and
the accounts' fold each add to a step; trades per book-step; `must_bytes_per_step`, what the bars' fold has to move: 16 B
of header words, 8 B of cursor, 16 B of previous close and 48 B of row per book, and 32 B per new record.  The kernel's own
time per launch:
  rocprofv3 --kernel-trace --stats -- python scripts/trade_bars_rate.py --arms a --regions 2

usage: python scripts/trade_bars_rate.py [--arms a,b,c] [--regions N] [--iters N] [--window N] [--books N]
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

import accounts_rate as AR  # noqa: E402

ARMS = {"a": ("ingress", 65536), "b": ("ingress", 8192), "c": ("idle", 65536)}
KINDS = ("off", "bars", "accounts")


class Arm(AR.IngressArm):
    def __init__(self, B, iters, n_traders, idle, window):
        super().__init__(B, iters, n_traders, idle)
        self.window = window

    def env(self, kind):
        e = super().env(kind == "accounts")
        if kind == "bars":
            e.enable_trade_bars(self.window)
        return e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arms", default="a,b,c")
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--iters", type=int, default=24, help="steps per region (the INGRESS stream fills the pools: <= 33)")
    ap.add_argument("--traders", type=int, default=16, help="n_traders of the accounts' env, the yardstick")
    ap.add_argument("--window", type=int, default=4)
    ap.add_argument("--books", type=int, default=0, help="override the arm's book count (a rehearsal)")
    args = ap.parse_args()
    for name in (a for a in args.arms.split(",") if a):
        kind, B = ARMS[name]
        B = args.books or B
        arm = Arm(B, args.iters, args.traders, kind == "idle", args.window)
        envs = {k: arm.env(k) for k in KINDS}
        every = torch.ones(B, dtype=torch.uint8, device="cuda")
        for e in envs.values():
            e.save_ingress_snapshot()
            AR.region(arm, e, every)  # the warm-up
        us, trades = {k: [] for k in KINDS}, {}
        for _ in range(args.regions):
            for k, e in envs.items():
                t, trades[k] = AR.region(arm, e, every)
                us[k].append(t)
        assert trades["off"] == trades["bars"] == trades["accounts"], trades  # the identical flow
        med = {k: float(np.median(v)) for k, v in us.items()}
        tr = trades["bars"] / (B * arm.iters)  # per book-step
        must = B * (16 + 8 + 16 + 48) + B * tr * 32
        # one more region on the env with bars, kept: the rows against the trade counts and the flags
        arm.run(envs["bars"])
        rows = envs["bars"].trade_bars()
        out = dict(arm=name, flow=kind, books=B, window=arm.window, n_traders=arm.n_traders, iters=arm.iters,
                   trades_per_book_step=round(tr, 3), us_per_step={k: round(v, 1) for k, v in med.items()},
                   bars_fold_adds_us=round(med["bars"] - med["off"], 1), accounts_fold_adds_us=round(med["accounts"] - med["off"], 1),
                   regions={k: [round(x, 1) for x in v] for k, v in us.items()}, must_bytes_per_step=int(must),
                   records_in_ring=int(rows["n_buy"].sum() + rows["n_sell"].sum()),
                   flags=int(np.bitwise_or.reduce(envs["bars"].flags())))
        print(json.dumps(out), flush=True)
        for e in envs.values():
            e.close()


if __name__ == "__main__":
    main()
