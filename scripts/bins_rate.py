"""Cost of the per-book bin table (bk_bins_enable: bins::k_fold over the history ring), priced against the same library with
no table and against the lag table's fold beside it.  Per workload (bench.py's C3 and C2 set-ups with history_capacity = 64)
four envs of one shape - no table / the lag table at K = 64 / bins at spans (1,) and 64 bins / bins at spans (1, 5, 20, 64)
and 256 bins - are warmed (bk_warm) and then timed ALTERNATELY region by region (all see the same clocks): a region is
clear_history, clear_trades, run(64) [+ the arm's fold] queued on the env's stream and one synchronise at the end (host
clock).  Reported per workload, one JSON line: medians and ranges of the regions, the microseconds each fold adds per
64-step chunk and per book-step, and the bin fold's "must move" bytes - one 128-byte line of every record it reads (the lane
reads 12 B of it), at most 8 B read + 8 B written per count, 8 Kmax B of carry read and written per book - over that time.
The kernel's own time per launch, one configuration at a time (the stats do not separate them):
  rocprofv3 --kernel-trace --stats -f csv -- python scripts/bins_rate.py --workloads C3 --regions 2 --arms off,bins4x256

usage: python scripts/bins_rate.py [--workloads C3,C2] [--regions N] [--books N] [--arms off,lags64,bins1x64,bins4x256]
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
BINS = {"bins1x64": ((1,), 64), "bins4x256": ((1, 5, 20, 64), 256)}
ARMS = ("off", "lags64") + tuple(BINS)


def make_env(workload, B, arm):
    _, levels, groups = bench.WORKLOADS[workload]
    n_agents = sum(g[0] for g in groups)
    env = bourse_amd.ManyBookEnv(B, bench.SEED, 0, bench.TICK, bench.STEP_SIZE, True, levels=levels, max_live_orders=min(n_agents, 512),
                                 trade_capacity=max(64, n_agents // 2 * 3 // 2) * CHUNK, history_capacity=CHUNK,
                                 stream=torch.cuda.current_stream().cuda_stream, strict=False)
    env.set_random_agents(groups)
    if arm == "lags64":
        env.enable_lags(64)
    elif arm in BINS:
        env.enable_bins(*BINS[arm])
    env.warm(100)
    return env


def region(env, arm):
    env.clear_history()
    env.clear_trades()
    t0 = time.perf_counter()
    env.run(CHUNK, sync=False)
    if arm == "lags64":
        env.fold_lags()
    elif arm != "off":
        env.fold_bins()
    env.sync()
    return (time.perf_counter() - t0) * 1e6


def must_bytes(B, spans, n_bins):
    return B * (CHUNK * 128 + 2 * 8 * (len(spans) + 2) * n_bins + 2 * 8 * max(spans))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="C3,C2")
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--books", type=int, default=0, help="override the workload's book count (a rehearsal)")
    ap.add_argument("--arms", default=",".join(ARMS), help="the arms to build and time; 'off' is always among them")
    args = ap.parse_args()
    arms = tuple(a for a in ARMS if a == "off" or a in args.arms.split(","))
    for name in (w for w in args.workloads.split(",") if w):
        B = args.books or bench.WORKLOADS[name][0]
        envs = {arm: make_env(name, B, arm) for arm in arms}
        for arm, e in envs.items():
            region(e, arm)  # untimed: the first launches
        us = {arm: [] for arm in envs}
        for _ in range(args.regions):
            for arm, e in envs.items():
                us[arm].append(region(e, arm))
        med = {arm: float(np.median(v)) for arm, v in us.items()}
        out = dict(workload=name, books=B, chunk=CHUNK, l2_width=envs["off"].width, us_per_chunk={a: round(v, 1) for a, v in med.items()},
                   us_range={a: [round(min(v), 1), round(max(v), 1)] for a, v in us.items()},
                   regions={a: [round(x, 1) for x in v] for a, v in us.items()},
                   m_book_steps_per_s={a: round(B * CHUNK / v, 1) for a, v in med.items()})
        for arm in arms[1:]:
            adds = med[arm] - med["off"]
            out[arm] = dict(fold_adds_us_per_chunk=round(adds, 1), fold_adds_ns_per_book_step=round(adds * 1e3 / (B * CHUNK), 4),
                            share_of_chunk=round(adds / med["off"], 4))
            if arm in BINS:
                spans, n_bins = BINS[arm]
                counts = envs[arm].bins()
                nonzero = int((counts != 0).sum())
                out[arm].update(must_bytes_per_fold_at_most=must_bytes(B, spans, n_bins),
                                must_tb_per_s=round(must_bytes(B, spans, n_bins) / (adds * 1e-6) / 1e12, 3) if adds > 0 else None,
                                steps_counted=int(counts[:, -1].sum()), returns_counted_at_span_1=int(counts[:, 0].sum()),
                                share_in_the_fullest_return_bin=round(float(counts[:, 0].max(axis=1).sum() / max(1, counts[:, 0].sum())), 4),
                                counts_raised_per_book=round(nonzero / B, 1))
        out["flags"] = int(np.bitwise_or.reduce(np.concatenate([e.flags() for e in envs.values()])))
        print(json.dumps(out), flush=True)
        for e in envs.values():
            e.close()


if __name__ == "__main__":
    main()
