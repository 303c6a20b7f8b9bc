"""Cost of the per-book series moments (bk_series_enable: series::k_fold over the history ring), priced against the same
library with the table off, and against what a user does today for the same numbers.  Per workload (bench.py's C3 and C2
set-ups with history_capacity = 64) two envs of one shape - the table off / on - are warmed (bk_warm) and then timed
ALTERNATELY region by region (both see the same clocks): a region is clear_history, clear_trades, run(64) [+ fold_series()]
queued on the env's stream and one synchronise at the end (host clock).
  arm 1  run(64) against run(64) + fold_series(): medians of the regions, the microseconds the fold adds per 64-step chunk
         and per book-step, and the fold's "must move" bytes over that time - one 128-byte line of every record it reads
         (the lane reads 20 B of it) and 192 B read + 192 B written per book per fold
  arm 2  today's way: bk_history_copy_async of the same 64 steps to pinned memory (timed to the copy stream's end) and a
         vectorised numpy fold of the five words into the same sums (timed on its own)
Reported per workload, one JSON line.  The kernel's own time per launch:
  rocprofv3 --kernel-trace --stats -- python scripts/series_rate.py --workloads C3 --regions 2 --no-egress

usage: python scripts/series_rate.py [--workloads C3,C2] [--regions N] [--books N] [--no-egress]
"""
import argparse
import ctypes as C
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
from bourse_amd import _lib  # noqa: E402

CHUNK = 64


def make_env(workload, B, series):
    _, levels, groups = bench.WORKLOADS[workload]
    n_agents = sum(g[0] for g in groups)
    env = bourse_amd.ManyBookEnv(B, bench.SEED, 0, bench.TICK, bench.STEP_SIZE, True, levels=levels, max_live_orders=min(n_agents, 512),
                                 trade_capacity=max(64, n_agents // 2 * 3 // 2) * CHUNK, history_capacity=CHUNK,
                                 stream=torch.cuda.current_stream().cuda_stream, strict=False)
    env.set_random_agents(groups)
    if series:
        env.enable_series()
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


def numpy_fold(h):
    """the sums of bk_series_row from [steps, books, 5] records, vectorised over the books (one chunk, no carry in)"""
    h = h.astype(np.int64)
    tv, bid, ask, av, bv = (h[:, :, i] for i in range(5))
    two = (bid != 0) & (ask != 0xFFFFFFFF)
    m, sp = bid + ask, ask - bid
    ret = two[1:] & two[:-1]
    d = np.where(ret, m[1:] - m[:-1], 0)
    pair = ret[1:] & ret[:-1]
    dd = np.where(pair, d[1:] * d[:-1], 0)
    d2 = d * d
    return dict(n_two_sided=two.sum(0), sum_m=np.where(two, m, 0).sum(0), sum_spread=np.where(two, sp, 0).sum(0),
                sum_spread_sq=np.where(two, sp * sp, 0).sum(0), sum_bid_vol=bv.sum(0), sum_ask_vol=av.sum(0), sum_trade_vol=tv.sum(0),
                sum_trade_vol_sq=(tv * tv).sum(0), n_trade_steps=(tv > 0).sum(0), n_ret=ret.sum(0), sum_d=d.sum(0),
                sum_abs_d=np.abs(d).sum(0), sum_d2=d2.sum(0), sum_d4=(d2.astype(np.float64) ** 2).sum(0), n_pairs=pair.sum(0),
                sum_dd=dd.sum(0), sum_abs_dd=np.abs(dd).sum(0))


def egress(env, regions):
    """arm 2 on the env without the table: copy the chunk's history to pinned memory, then fold it in numpy"""
    L, B, W = env._L, env.n_books, env.width
    cs, p = C.c_void_p(), C.c_void_p()
    _lib.check(L.bk_stream_create(C.byref(cs)))
    _lib.check(L.bk_pinned_alloc(CHUNK * B * W * 4, C.byref(p)))
    buf = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint32)), shape=(CHUNK, B, W))
    copy_us, fold_us, sums = [], [], None
    for _ in range(regions):
        env.clear_history()
        env.clear_trades()
        env.run(CHUNK, sync=False)
        env.sync()
        first, n = env.history_len()
        t0 = time.perf_counter()
        _lib.check(L.bk_history_copy_async(env._h, first, n, 0, B, C.cast(p, C.POINTER(C.c_uint32)), cs))
        _lib.check(L.bk_stream_sync(cs))
        t1 = time.perf_counter()
        sums = numpy_fold(buf[:, :, :5])
        t2 = time.perf_counter()
        copy_us.append((t1 - t0) * 1e6)
        fold_us.append((t2 - t1) * 1e6)
    _lib.check(L.bk_stream_destroy(cs))
    _lib.check(L.bk_pinned_free(p))
    return float(np.median(copy_us)), float(np.median(fold_us)), CHUNK * B * W * 4, sums


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="C3,C2")
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--books", type=int, default=0, help="override the workload's book count (a rehearsal)")
    ap.add_argument("--no-egress", action="store_true", help="leave out arm 2")
    args = ap.parse_args()
    for name in (w for w in args.workloads.split(",") if w):
        B = args.books or bench.WORKLOADS[name][0]
        envs = {"off": make_env(name, B, False), "on": make_env(name, B, True)}
        for k, e in envs.items():
            region(e, k == "on")  # untimed: the first launches
        us = {k: [] for k in envs}
        for _ in range(args.regions):
            for k, e in envs.items():
                us[k].append(region(e, k == "on"))
        med = {k: float(np.median(v)) for k, v in us.items()}
        adds = med["on"] - med["off"]
        must = B * CHUNK * 128 + B * 2 * 192
        rows = envs["on"].series()
        out = dict(workload=name, books=B, chunk=CHUNK, l2_width=envs["on"].width, us_per_chunk={k: round(v, 1) for k, v in med.items()},
                   regions={k: [round(x, 1) for x in v] for k, v in us.items()}, fold_adds_us_per_chunk=round(adds, 1),
                   fold_adds_ns_per_book_step=round(adds * 1e3 / (B * CHUNK), 4), must_bytes_per_fold=must,
                   must_tb_per_s=round(must / (adds * 1e-6) / 1e12, 3) if adds > 0 else None,
                   m_book_steps_per_s={k: round(B * CHUNK / v, 1) for k, v in med.items()},
                   steps_folded=int(rows["n_steps"][0]), two_sided_share=round(float(rows["n_two_sided"].sum() / rows["n_steps"].sum()), 4),
                   flags=int(np.bitwise_or.reduce(envs["on"].flags())))
        if not args.no_egress:
            copy_us, fold_us, nbytes, _ = egress(envs["off"], max(2, args.regions // 2))
            out.update(egress_copy_us_per_chunk=round(copy_us, 1), egress_gb_per_s=round(nbytes / (copy_us * 1e-6) / 1e9, 2),
                       numpy_fold_us_per_chunk=round(fold_us, 1), egress_bytes_per_chunk=nbytes)
        print(json.dumps(out), flush=True)
        for e in envs.values():
            e.close()


if __name__ == "__main__":
    main()
