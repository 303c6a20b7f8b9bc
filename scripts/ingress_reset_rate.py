"""Cost of the per-book reset of a device-ingress env (bk_ingress_snapshot_save / bk_ingress_reset_books_device) beside
on-device Noise / Momentum members (bk_update_members), set up as scripts/members_ingress_rate.py sets up its shapes:
  small  10 momentum + 20 noise traders, 65 536 books, a 128-slot pool, 10 levels;
  c5m    bench.py's C5M member set (256 momentum + 256 noise traders), 8 192 books, a 512-slot pool, 64 levels.
One env per (shape, snapshot depth): `depth` steps of update_members + step, then the snapshot - the deeper, the more order
records per book the slot holds (n_keep).  The arms are timed ALTERNATELY region by region after a warm-up (every arm sees
the same clocks); a region is ITERS iterations queued back to back on the env's stream and one synchronise at the end
(host clock), after which every book is put back to the snapshot (untimed), so that every region starts at the same depth:
  step         update_members + step alone
  ask          the same + bk_ingress_reset_books_device with an all-zero mask: the cost of asking, which must not
               depend on n_keep (compare the depths)
  reset_1pct   the same with 1 % of the books masked
  reset_all    the same with every book masked
  reset_only   bk_ingress_reset_books_device alone, every book masked: k_reset_books + k_collect_units + k_reset_records
               back to back; bytes = 2 x what the three move (state blocks, level-2 rows, the order records of the ids
               below each book's own next id, the members' lists up to their lengths and their small rows)
The medians of the regions are reported, one JSON line per (shape, depth).  The record kernel's own time per launch:
  rocprofv3 --kernel-trace --stats -- python scripts/ingress_reset_rate.py --shapes small --depths 50 --arms reset_only
and `record_bytes` of the JSON line over that time is its rate.

usage: python scripts/ingress_reset_rate.py [--shapes small,c5m] [--depths 5,50] [--regions N] [--iters N] [--arms a,b]
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

import bourse_amd as bk  # noqa: E402

MOM_P = dict(tick_size=2, p_cancel=0.1, trade_vol=100, decay=1.0, demand=20.0, scale=0.5, order_ratio=1.0,
             price_dist_mu=0.0, price_dist_sigma=10.0)
NOISE_P = dict(tick_size=2, p_limit=0.3, p_market=0.2, p_cancel=0.2, trade_vol=100, price_dist_mu=0.0, price_dist_sigma=1.0)
SHAPES = {  # name: (books, pool, levels, members) - scripts/members_ingress_rate.py's
    "small": (65536, 128, 10, [("momentum", 0, 10, dict(MOM_P, demand=5.0)),
                               ("noise", 10, 20, dict(NOISE_P, p_limit=0.2, p_cancel=0.1))]),
    "c5m": (8192, 512, 64, [("momentum", 0, 256, MOM_P), ("noise", 256, 256, NOISE_P)]),
}
ARMS = ("step", "ask", "reset_1pct", "reset_all", "reset_only")
TICK, STEP = 2, 100_000


def make_env(shape, depth, iters):
    B, pool, levels, members = SHAPES[shape]
    per_update = sum(2 * m[2] for m in members)
    # the order log holds the warm-up's and one region's orders (a trader places well under one order a step on average)
    max_orders = per_update // 2 * (depth + iters + 2)
    e = bk.ManyBookEnv(B, 101, 0, TICK, STEP, levels=levels, max_live_orders=pool, max_orders=max_orders,
                       trade_capacity=per_update * (iters + 1), strict=False, history_capacity=0,
                       stream=torch.cuda.current_stream().cuda_stream)
    e.enable_device_ingress(per_update + pool)
    e.set_agents(members)
    for _ in range(depth):
        e.update_members(sync=False)
        e.step(sync=False)
    e.sync()
    return e, max_orders


def region(env, iters, mask, every, step=True):
    """Microseconds per iteration of [update_members + step] [+ reset with `mask`]; every book back to the snapshot after."""
    env.clear_trades()
    env.sync()
    t = time.perf_counter()
    for _ in range(iters):
        if step:
            env.update_members(sync=False)
            env.step(sync=False)
        if mask is not None:
            env.reset_ingress_books(mask, sync=False)
    env.sync()
    us = (time.perf_counter() - t) / iters * 1e6
    env.reset_ingress_books(every, sync=True)
    return us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="small,c5m")
    ap.add_argument("--depths", default="5,50")
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--arms", default=",".join(ARMS))
    ap.add_argument("--books", type=int, default=0, help="override the shape's book count (a rehearsal)")
    args = ap.parse_args()
    arms = [a for a in args.arms.split(",") if a]
    for shape in args.shapes.split(","):
        if args.books:
            SHAPES[shape] = (args.books,) + SHAPES[shape][1:]
        for depth in (int(d) for d in args.depths.split(",")):
            env, max_orders = make_env(shape, depth, args.iters)
            B, n_members = env.n_books, len(SHAPES[shape][3])
            env.save_ingress_snapshot()
            keep = np.minimum(env.order_counts(), max_orders)
            lens = sum(len(env.member_orders(b, j)) for b in range(0, B, max(1, B // 256)) for j in range(n_members))
            lens = lens * B // len(range(0, B, max(1, B // 256)))  # (the lists' entries, from a sample of 256 books)
            record_bytes = 2 * int(keep.sum()) * 80
            small_bytes = 2 * (B * (env.state_bytes_per_book() + 4 * env.width) + lens * 4 + B * (n_members * 20 + 8))
            r = np.random.default_rng(5)
            one = np.zeros(B, dtype=np.uint8)
            one[r.choice(B, max(1, B // 100), replace=False)] = 1
            every = torch.ones(B, dtype=torch.uint8, device="cuda")
            masks = {"step": None, "ask": torch.zeros(B, dtype=torch.uint8, device="cuda"),
                     "reset_1pct": torch.tensor(one, device="cuda"), "reset_all": every, "reset_only": every}
            for arm in arms:  # the warm-up: one untimed region per arm
                region(env, args.iters, masks[arm], every, step=arm != "reset_only")
            us = {arm: [] for arm in arms}
            for _ in range(args.regions):
                for arm in arms:
                    us[arm].append(region(env, args.iters, masks[arm], every, step=arm != "reset_only"))
            med = {arm: round(float(np.median(v)), 1) for arm, v in us.items()}
            out = dict(shape=shape, books=B, depth=depth, n_keep_max=int(keep.max()), keep_mean=round(float(keep.mean()), 1),
                       snapshot_mb=round(env.ingress_snapshot_bytes() / 1e6, 1), record_bytes=record_bytes,
                       other_bytes=small_bytes, us_per_iteration=med,
                       regions={arm: [round(x, 1) for x in v] for arm, v in us.items()}, flags=int(np.bitwise_or.reduce(env.flags())))
            if "step" in med:
                out["over_step_us"] = {arm: round(med[arm] - med["step"], 1) for arm in med if arm not in ("step", "reset_only")}
            if "reset_only" in med:
                out["reset_only_gbps"] = round((record_bytes + small_bytes) / med["reset_only"] / 1e3, 1)
            print(json.dumps(out), flush=True)
            env.close()


if __name__ == "__main__":
    main()
