"""Cost of requoting from a dense table (bk_submit_quotes_device: quotes::k_submit in front of the step), priced against the
floor k_ingest sets for the same queue work, on the pattern of scripts/open_queue_rate.py.  Two envs of one shape, BOTH with
the open-order view (n_traders = 16, depth = 8) and both taking bench.py --workload INGRESS's flow (48 instructions per
book-step) as background; the two are timed ALTERNATELY region by region after one untimed warm-up region each.  A region is
`iters` steps queued back to back on the env's stream and one synchronise at the end (host clock); after it every book goes
back to an ingress snapshot of the fresh env (untimed), so that every region runs the same steps.  Arms:
  a  every step submits a quote table for the 16 traders (prebuilt on the device: a bid at 97..99 and an ask at 101..103 of
     volume 1..50, one side in ten KEEP, one in ten pulled) through submit_quotes
  b  every step submits, through submit_instructions_device, a prebuilt dense grid of the same shape (16 x 10 positions a
     book): the same new orders wherever arm a's table names a target, and in the trader's first two entry slots the
     cancellation of the orders the trader's previous row placed (their ids recorded in the warm-up region) - every requote
     a cancel and a new order, about what arm a queues
Shapes: 65 536 books x 512 slots and 8 192 books x 256 slots.  Reported per shape, one JSON line: the medians of the regions in
microseconds per step for both arms and their difference; the new orders per book-step either arm created and arm b's
cancellations.  The kernel's own time per launch, beside k_ingest's in the same trace:
  rocprofv3 --kernel-trace --stats -- python scripts/quotes_rate.py --shapes big --regions 2

usage: python scripts/quotes_rate.py [--shapes big,small] [--regions N] [--iters N] [--books N]
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

import accounts_rate as AR  # noqa: E402  (the INGRESS stream)
import bourse_amd as bk  # noqa: E402
import open_orders_rate as OR  # noqa: E402  (the timed region)

SHAPES = {"big": 65536, "small": 8192}
NT, DEPTH = 16, 8
G = DEPTH + 2
assert bk.QUOTE_KEEP == 0xFFFFFFFF


class QuoteArm(AR.IngressArm):
    def __init__(self, B, iters):
        super().__init__(B, iters, NT, False)
        self.pool = 512 if B > 8192 else 256
        g = torch.Generator(device="cuda").manual_seed(1)
        self.quotes = []
        for _ in range(iters):
            q = torch.empty((B, NT, 4), dtype=torch.int32, device="cuda")  # (KEEP is -1 here: the same bits)
            for k, base in ((0, 97), (2, 101)):
                u = torch.rand((B, NT), device="cuda", generator=g)
                q[..., k] = torch.randint(base, base + 3, (B, NT), device="cuda", generator=g, dtype=torch.int32)
                vol = torch.randint(1, 51, (B, NT), device="cuda", generator=g, dtype=torch.int32)
                q[..., k + 1] = torch.where(u < 0.1, torch.full_like(vol, -1), torch.where(u < 0.2, torch.zeros_like(vol), vol))
            self.quotes.append(q)
        self.ids = torch.empty((B, NT, 2), dtype=torch.int64, device="cuda")

    def env(self, view=True):
        e = bk.ManyBookEnv(self.B, 1, 0, 1, AR.STEP, levels=16, max_live_orders=self.pool, max_orders=(AR.N + 2 * NT) * (self.iters + 8),
                           trade_capacity=64 * (self.iters + 8), strict=False, history_capacity=0,
                           stream=torch.cuda.current_stream().cuda_stream)
        e.enable_device_ingress(AR.N + NT * G)
        e.enable_open_orders(NT, DEPTH)
        return e

    def run(self, e):
        for b, q in zip(self.batches, self.quotes):
            e.submit_instructions_device(self.off, *b)
            e.submit_quotes(q, self.ids)
            e.step(sync=False)


class GridArm(QuoteArm):
    """the same background, and per step a dense grid through k_ingest; `record` builds the grids while it runs"""

    def __init__(self, B, iters):
        super().__init__(B, iters)
        self.goff = torch.arange(B + 1, dtype=torch.int64, device="cuda") * (NT * G)
        self.grids, self.gids = None, torch.empty((B, NT, G), dtype=torch.int64, device="cuda")

    def grid(self, q, last_ids):
        B = self.B
        action = torch.zeros((B, NT, G), dtype=torch.int32, device="cuda")
        side = torch.zeros((B, NT, G), dtype=torch.uint8, device="cuda")
        vol, price = torch.zeros_like(action), torch.zeros_like(action)
        oid = torch.zeros((B, NT, G), dtype=torch.int64, device="cuda")
        for k, at in ((0, DEPTH), (2, DEPTH + 1)):
            target = (q[..., k + 1] != -1) & (q[..., k + 1] != 0)
            action[..., at] = target.to(torch.int32)
            side[..., at] = 1 if k == 0 else 0
            vol[..., at], price[..., at] = q[..., k + 1] * target, q[..., k] * target
            if last_ids is not None:  # the order this trader's previous row placed on this side goes
                had = (last_ids[..., at] >= 0) & (q[..., k + 1] != -1)
                action[..., k // 2] = 2 * had.to(torch.int32)
                oid[..., k // 2] = last_ids[..., at] * had
        return tuple(x.reshape(-1).contiguous() for x in (action, side, vol, torch.zeros_like(action), price, oid))

    def record(self, e):
        """one region that builds each step's grid from the ids the step before created (u64::MAX reads -1)"""
        self.grids, last = [], None
        for b, q in zip(self.batches, self.quotes):
            self.grids.append(self.grid(q, last))
            e.submit_instructions_device(self.off, *b)
            e.submit_instructions_device(self.goff, *self.grids[-1], out_ids=self.gids.reshape(-1))
            e.step(sync=False)
            last = self.gids.clone()
        e.sync()

    def run(self, e):
        for b, g in zip(self.batches, self.grids):
            e.submit_instructions_device(self.off, *b)
            e.submit_instructions_device(self.goff, *g, out_ids=self.gids.reshape(-1))
            e.step(sync=False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="big,small")
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--iters", type=int, default=24, help="steps per region (the INGRESS stream fills the pools: <= 33)")
    ap.add_argument("--books", type=int, default=0, help="override the shape's book count (a rehearsal)")
    args = ap.parse_args()
    for name in (s for s in args.shapes.split(",") if s):
        B = args.books or SHAPES[name]
        arms = {"quotes": QuoteArm(B, args.iters), "grid": GridArm(B, args.iters)}
        envs = {k: a.env() for k, a in arms.items()}
        every = torch.ones(B, dtype=torch.uint8, device="cuda")
        for e in envs.values():
            e.save_ingress_snapshot()
        arms["grid"].record(envs["grid"])
        envs["grid"].reset_ingress_books(every, sync=True)
        for k in arms:
            OR.region(arms[k], envs[k], every)  # the warm-up
        us = {k: [] for k in arms}
        for _ in range(args.regions):
            for k in arms:
                us[k].append(OR.region(arms[k], envs[k], every)[0])
        med = {k: float(np.median(v)) for k, v in us.items()}
        # one more region on each, kept: what the last step created
        new = {}
        for k in arms:
            arms[k].run(envs[k])
            envs[k].sync()
            ids = arms[k].ids if k == "quotes" else arms[k].gids[..., DEPTH:]
            new[k] = float((ids >= 0).sum().item()) / B
        cancels = float(np.mean([float((g[0] == 2).sum().item()) for g in arms["grid"].grids])) / B
        out = dict(shape=name, books=B, pool=arms["quotes"].pool, n_traders=NT, depth=DEPTH, iters=args.iters,
                   us={k: round(v, 1) for k, v in med.items()}, quotes_over_grid_us=round(med["quotes"] - med["grid"], 1),
                   regions={k: [round(x, 1) for x in v] for k, v in us.items()},
                   new_orders_last_step_per_book={k: round(v, 2) for k, v in new.items()}, grid_cancels_per_book_step=round(cancels, 2),
                   flags={k: int(np.bitwise_or.reduce(e.flags())) for k, e in envs.items()})
        print(json.dumps(out), flush=True)
        for e in envs.values():
            e.close()


if __name__ == "__main__":
    main()
