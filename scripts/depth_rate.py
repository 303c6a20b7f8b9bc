"""Cost of the per-level depth table (bk_depth_enable: depth::k_fold over the ladder of the history ring), priced against
the same library with the series moments alone and with no table.  Per workload (bench.py's C3, C2 and C5 set-ups with
history_capacity = 64) three envs of one shape - no table / the series / the series and the depth table - are warmed
(bk_warm) and then timed ALTERNATELY region by region (all see the same clocks): a region is clear_history, clear_trades,
run(64) [+ fold_series()] queued on the env's stream and one synchronise at the end (host clock).  Reported per workload,
one JSON line: the medians of the regions, the microseconds the depth fold adds per 64-step chunk over the series alone and
per book-step, and the fold's necessary bytes over that time - every record it reads whole (4 W bytes; the series reads the
first 20 of the same record) and (L + 1) * 128 B read + written per book per fold.  The kernel's own time per launch:
  rocprofv3 --kernel-trace --stats -- python scripts/depth_rate.py --workloads C3 --regions 2

usage: python scripts/depth_rate.py [--workloads C3,C2,C5] [--regions N] [--books N]
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
ARMS = ("off", "series", "depth")


def make_env(workload, B, arm):
    _, levels, groups = bench.WORKLOADS[workload]
    n_agents = sum(g[0] for g in groups)
    env = bourse_amd.ManyBookEnv(B, bench.SEED, 0, bench.TICK, bench.STEP_SIZE, True, levels=levels, max_live_orders=min(n_agents, 512),
                                 trade_capacity=max(64, n_agents // 2 * 3 // 2) * CHUNK, history_capacity=CHUNK,
                                 stream=torch.cuda.current_stream().cuda_stream, strict=False)
    env.set_random_agents(groups)
    if arm != "off":
        env.enable_series()
    if arm == "depth":
        env.enable_depth()
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="C3,C2,C5")
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--books", type=int, default=0, help="override the workload's book count (a rehearsal)")
    args = ap.parse_args()
    for name in (w for w in args.workloads.split(",") if w):
        B = args.books or bench.WORKLOADS[name][0]
        envs = {arm: make_env(name, B, arm) for arm in ARMS}
        for k, e in envs.items():
            region(e, k != "off")  # untimed: the first launches
        us = {k: [] for k in envs}
        for _ in range(args.regions):
            for k, e in envs.items():
                us[k].append(region(e, k != "off"))
        med = {k: float(np.median(v)) for k, v in us.items()}
        adds = med["depth"] - med["series"]
        L, W = envs["depth"].levels, envs["depth"].width
        must = B * CHUNK * W * 4 + B * 2 * (L + 1) * 128
        rows = envs["depth"].depth()
        moments = bourse_amd.depth_moments(rows[:64])
        out = dict(workload=name, books=B, chunk=CHUNK, levels=L, l2_width=W, us_per_chunk={k: round(v, 1) for k, v in med.items()},
                   regions={k: [round(x, 1) for x in v] for k, v in us.items()}, depth_adds_us_per_chunk=round(adds, 1),
                   depth_adds_share_of_series_arm=round(adds / med["series"], 4),
                   series_adds_us_per_chunk=round(med["series"] - med["off"], 1),
                   depth_adds_ns_per_book_step=round(adds * 1e3 / (B * CHUNK), 4), must_bytes_per_fold=must,
                   must_tb_per_s=round(must / (adds * 1e-6) / 1e12, 3) if adds > 0 else None,
                   m_book_steps_per_s={k: round(B * CHUNK / v, 1) for k, v in med.items()},
                   steps_folded=int(rows[0, -1, 0]), deepest_level_bid_occupancy=round(float(np.nanmean(moments["bid_occupancy"][:, -1])), 4),
                   hit_rate_level_0=round(float(np.nanmean(moments["hit_rate"][:, 0])), 4),
                   flags=int(np.bitwise_or.reduce(envs["depth"].flags())))
        print(json.dumps(out), flush=True)
        for e in envs.values():
            e.close()


if __name__ == "__main__":
    main()
