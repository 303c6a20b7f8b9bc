"""Cost of the per-market cross table (bk_cross_enable: cross::k_fold over the history ring), priced against the same library
with no table and against the lag fold at K = 64 beside it for scale.  Four envs of one shape - a three-asset
RandomMarketAgents env of scripts/market_agents_rate.py's set-up with history_capacity = 64: no table / the cross table at
spans (1,) / at spans (1, 5, 20, 64) / the lag table at K = 64 on the same books - are warmed (bk_warm) and then timed
ALTERNATELY region by region (all see the same clocks): a region is clear_history, clear_trades, run(64) [+ the arm's fold]
queued on the env's stream and one synchronise at the end (host clock).  Reported per market count, one JSON line: medians and
ranges of five regions, the microseconds each fold adds per 64-step chunk ("not resolved" where the arm's range overlaps
the range without a table), and the cross fold's "must move" bytes - one 128-byte line of every record it reads (the lane
reads 8 B of it), 64 B read + 64 B written per row, 8 * 2 Hmax B of carry read and written per book - over that time.  The
kernel's own time per launch:
  rocprofv3 --kernel-trace --stats -f csv -- python scripts/cross_rate.py --regions 2

usage: python scripts/cross_rate.py [--markets 8192] [--regions N]
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

CHUNK = 64
TICKS, POOL, LEVELS, STEP = [2, 2, 2], 512, 10, 100_000
RND = (32, 64), (10, 20), 2
GROUPS = [(0, 70, *RND, 0.8), (1, 5, (30, 66), (50, 70), 2, 0.5), (2, 0, *RND, 0.8), (0, 20, (30, 66), (50, 70), 2, 0.3),
          (2, 64, *RND, 0.8), (1, 40, *RND, 0.7)]
ARMS = {"off": None, "cross1": (1,), "cross4": (1, 5, 20, 64), "lags64": 64}


def make_env(NM, arm):
    env = bk.ManyMarketEnv(NM, 101, 0, TICKS, STEP, levels=LEVELS, max_live_orders=POOL, trade_capacity=64 * CHUNK, strict=False,
                           history_capacity=CHUNK, stream=torch.cuda.current_stream().cuda_stream)
    env.set_random_market_agents(GROUPS)
    if arm.startswith("cross"):
        env.enable_cross(ARMS[arm])
    elif arm.startswith("lags"):
        env.enable_lags(ARMS[arm])
    env.warm(100)
    return env


def region(env, arm):
    env.clear_history()
    env.clear_trades()
    t0 = time.perf_counter()
    env.run(CHUNK, sync=False)
    if arm.startswith("cross"):
        env.fold_cross()
    elif arm.startswith("lags"):
        env.fold_lags()
    env.sync()
    return (time.perf_counter() - t0) * 1e6


def must_bytes(NM, A, spans):
    return NM * (A * CHUNK * 128 + 2 * len(spans) * A * A * 64 + 2 * 8 * A * 2 * max(spans))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--markets", default="8192")
    ap.add_argument("--regions", type=int, default=5)
    args = ap.parse_args()
    A = len(TICKS)
    for NM in (int(x) for x in args.markets.split(",") if x):
        envs = {arm: make_env(NM, arm) for arm in ARMS}
        for arm, e in envs.items():
            region(e, arm)  # untimed: the first launches
        us = {arm: [] for arm in envs}
        for _ in range(args.regions):
            for arm, e in envs.items():
                us[arm].append(region(e, arm))
        med = {arm: float(np.median(v)) for arm, v in us.items()}
        out = dict(markets=NM, assets=A, books=NM * A, chunk=CHUNK, l2_width=envs["off"].width,
                   us_per_chunk={a: round(v, 1) for a, v in med.items()},
                   us_range={a: [round(min(v), 1), round(max(v), 1)] for a, v in us.items()},
                   regions={a: [round(x, 1) for x in v] for a, v in us.items()})
        for arm in list(ARMS)[1:]:
            adds = med[arm] - med["off"]
            resolved = min(us[arm]) > max(us["off"])
            out[arm] = dict(fold_adds_us_per_chunk=round(adds, 1) if resolved else "not resolved", median_difference_us=round(adds, 1),
                            share_of_chunk=round(adds / med["off"], 4))
            if arm.startswith("cross"):
                rows = envs[arm].cross()
                b = must_bytes(NM, A, ARMS[arm])
                out[arm].update(units_per_market=len(ARMS[arm]) * A * A, must_bytes_per_fold=b,
                                must_tb_per_s=round(b / (adds * 1e-6) / 1e12, 3) if resolved else None,
                                pairs_folded=int(rows["n"].sum()), leads_folded=int(rows["n_lead"].sum()))
        out["flags"] = int(np.bitwise_or.reduce(np.concatenate([e.flags() for e in envs.values()])))
        print(json.dumps(out), flush=True)
        for e in envs.values():
            e.close()


if __name__ == "__main__":
    main()
