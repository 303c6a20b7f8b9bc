"""Cost of the per-book candle table (bk_candles_enable: candles::k_fold over words 0..2 of the history ring's records),
priced against the same library with the series moments alone and with no table.  Per workload (bench.py's C3, C2 and C5
set-ups with history_capacity = 64) and per shape (W, N) three envs - no table / the series / the series and the candle
table - are warmed (bk_warm) and then timed ALTERNATELY region by region (all see the same clocks): a region is
clear_history, clear_trades, run(64) [+ fold_series()] queued on the env's stream and one synchronise at the end (host
clock).  Reported per workload and shape, one JSON line: the medians and the ranges of the regions, the microseconds the
candle fold adds per 64-step chunk over the series alone, whether the two arms' ranges overlap (then the cost is not
resolved), and the fold's necessary bytes: the 32-byte sectors that hold words 0..2 of every record it reads (a record is
4 W bytes and only 4-byte aligned: 12 bytes touch one or two sectors) and the 128 B read + written of every row it touches.
The kernel's own time per launch:
  rocprofv3 --kernel-trace --stats -- python scripts/candles_rate.py --workloads C3 --shapes 16x64 --regions 2

usage: python scripts/candles_rate.py [--workloads C3,C2,C5] [--shapes 1x64,16x64,256x16] [--regions N] [--books N]
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
import bourse_amd  # noqa: E402

CHUNK = 64
ARMS = ("off", "series", "candles")


def make_env(workload, B, arm, shape):
    _, levels, groups = bench.WORKLOADS[workload]
    n_agents = sum(g[0] for g in groups)
    env = bourse_amd.ManyBookEnv(B, bench.SEED, 0, bench.TICK, bench.STEP_SIZE, True, levels=levels, max_live_orders=min(n_agents, 512),
                                 trade_capacity=max(64, n_agents // 2 * 3 // 2) * CHUNK, history_capacity=CHUNK,
                                 stream=torch.cuda.current_stream().cuda_stream, strict=False)
    env.set_random_agents(groups)
    if arm != "off":
        env.enable_series()
    if arm == "candles":
        env.enable_candles(*shape)
    env.warm(100)
    return env


def region(env, fold):
    env.clear_history()
    env.clear_trades()
    t0 = time.perf_counter()
    env.run(CHUNK, sync=False)
    if fold:
        env.fold_series()
    env.sync()
    return (time.perf_counter() - t0) * 1e6


def sectors(l2_width, n_books, steps=CHUNK):
    """32-byte sectors that hold bytes [0, 12) of the records of `steps` slots of the ring (records of 4 * l2_width bytes,
    back to back)"""
    base = np.arange(steps * n_books, dtype=np.int64) * (4 * l2_width)
    return int(np.unique(np.concatenate([base // 32, (base + 11) // 32])).size)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="C3,C2,C5")
    ap.add_argument("--shapes", default="1x64,16x64,256x16", help="WxN, comma separated")
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--books", type=int, default=0, help="override the workload's book count (a rehearsal)")
    args = ap.parse_args()
    shapes = [tuple(int(x) for x in s.split("x")) for s in args.shapes.split(",") if s]
    for name in (w for w in args.workloads.split(",") if w):
        B = args.books or bench.WORKLOADS[name][0]
        for W, N in shapes:
            envs = {arm: make_env(name, B, arm, (W, N)) for arm in ARMS}
            for k, e in envs.items():
                region(e, k != "off")  # untimed: the first launches
            us = {k: [] for k in envs}
            for _ in range(args.regions):
                for k, e in envs.items():
                    us[k].append(region(e, k != "off"))
            med = {k: float(np.median(v)) for k, v in us.items()}
            adds = med["candles"] - med["series"]
            env = envs["candles"]
            bars_touched = min(N, -(-CHUNK // W) + 1)  # (a chunk of 64 steps may start inside a bar)
            must = sectors(env.width, B) * 32 + B * 2 * bars_touched * 128
            rows = env.candles(0, min(B, 64))
            s = bourse_amd.candle_series(rows, W)
            out = dict(workload=name, books=B, chunk=CHUNK, width=W, n_candles=N, l2_width=env.width,
                       us_per_chunk={k: round(v, 1) for k, v in med.items()},
                       range_us={k: [round(min(v), 1), round(max(v), 1)] for k, v in us.items()},
                       candles_adds_us_per_chunk=round(adds, 1), candles_adds_share_of_series_arm=round(adds / med["series"], 4),
                       ranges_overlap=bool(min(us["candles"]) <= max(us["series"])),
                       series_adds_us_per_chunk=round(med["series"] - med["off"], 1),
                       candles_adds_ns_per_book_step=round(adds * 1e3 / (B * CHUNK), 4), must_bytes_per_fold=must,
                       must_tb_per_s=round(must / (adds * 1e-6) / 1e12, 3) if adds > 0 else None,
                       m_book_steps_per_s={k: round(B * CHUNK / v, 1) for k, v in med.items()},
                       latest=env.candles_latest(), bars_held=int((rows["n_steps"][0] > 0).sum()),
                       mean_realized_var=round(float(np.nanmean(s["realized_var"])), 4),
                       flags=int(np.bitwise_or.reduce(env.flags())))
            print(json.dumps(out), flush=True)
            for e in envs.values():
                e.close()


if __name__ == "__main__":
    main()
