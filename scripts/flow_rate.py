"""Cost of the per-book flow table (bk_flow_enable: flow::k_fold over the books' trade records), priced against the same
library with no table, against its siblings in the same run, and against today's way to the same numbers.

  run      per workload (bench.py's C3 and C2 set-ups, chunks of 64 steps) three envs of one shape - no table / the flow
           table at K = 16 / at K = 64 - are warmed (bk_warm) and then timed ALTERNATELY region by region (all see the same
           clocks): a region is clear_history, clear_trades, run(64) [+ fold_flow] queued on the env's stream and one
           synchronise at the end (host clock).
  host     today's way to the same numbers, once, for one C3 chunk: run(64), drain_trades() through the host link, and the
           sums folded in numpy, lags 1 .. 16, vectorised per lag over all books' records at once; the drain and every lag
           are timed on their own, and the fold stops at the first lag that ends beyond --host-budget seconds.
  ingress  bench.py --workload INGRESS's flow (48 instructions per book-step) at 65 536 and 8 192 books: four envs take the
           IDENTICAL flow - nothing enabled, the flow table at K = 16, the trade bars, the accounts - timed as
           scripts/trade_bars_rate.py times its three; every region ends with an ingress reset (untimed).
One JSON line per workload / arm: medians and ranges of the regions, what each fold adds, trades per book-step, and the
fold's "must move" bytes - 32 B per record read, 16 B of header words and 8 B of cursor per book, and for a book with a new
record (8 + 6 K) 8 B of table and 8 K B of carry read and written.  The kernel's own time per launch:
  rocprofv3 --kernel-trace --stats -f csv -- python scripts/flow_rate.py --parts run --workloads C3 --regions 2

usage: python scripts/flow_rate.py [--parts run,ingress,host] [--workloads C3,C2] [--regions N] [--books N] [--iters N]
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

import accounts_rate as AR  # noqa: E402
import bench  # noqa: E402
import bourse_amd  # noqa: E402

CHUNK = 64
RUN_ARMS = ("off", "flow16", "flow64")
INGRESS_ARMS = {"a": 65536, "b": 8192}
KINDS = ("off", "flow", "bars", "accounts")


def make_env(workload, B, arm):
    _, levels, groups = bench.WORKLOADS[workload]
    n_agents = sum(g[0] for g in groups)
    env = bourse_amd.ManyBookEnv(B, bench.SEED, 0, bench.TICK, bench.STEP_SIZE, True, levels=levels, max_live_orders=min(n_agents, 512),
                                 trade_capacity=max(64, n_agents // 2 * 3 // 2) * CHUNK, history_capacity=CHUNK,
                                 stream=torch.cuda.current_stream().cuda_stream, strict=False)
    env.set_random_agents(groups)
    if arm.startswith("flow"):
        env.enable_flow(int(arm[4:]))
    env.warm(100)
    return env


def numpy_fold(off, rec, K, budget_s=1e9):
    """the flow table's sums from drained records, all books at once (float64 sums: a yardstick for the time, not for the
    bits): per lag one pass over the records, a pair counting where both ends lie in one book.  Returns the base sums, the
    lags' sums and the seconds each lag took; stops behind the first lag that ends beyond budget_s."""
    book = np.repeat(np.arange(len(off) - 1), np.diff(off).astype(np.int64))
    s = np.where(rec["side"] == 0, 1, -1).astype(np.int64)
    p, v = rec["price"].astype(np.int64), rec["vol"].astype(np.uint64)
    B = len(off) - 1
    base = [np.bincount(book, minlength=B), np.bincount(book, weights=s > 0, minlength=B), np.bincount(book, weights=v, minlength=B),
            np.bincount(book, weights=v * v, minlength=B), np.bincount(book, weights=v * rec["price"], minlength=B)]
    lags, secs, t_all = [], [], time.perf_counter()
    for k in range(1, K + 1):
        t_lag = time.perf_counter()
        same = book[k:] == book[:-k]
        dp = (p[k:] - p[:-k])[same]
        bk_, si, sk = book[k:][same], s[k:][same], s[:-k][same]
        lags.append([np.bincount(bk_, minlength=B), np.bincount(bk_, weights=si * sk, minlength=B), np.bincount(bk_, weights=sk * dp, minlength=B),
                     np.bincount(bk_, weights=si * dp, minlength=B), np.bincount(bk_, weights=np.abs(dp), minlength=B),
                     np.bincount(bk_, weights=dp * dp, minlength=B)])
        secs.append(time.perf_counter() - t_lag)
        if time.perf_counter() - t_all > budget_s:
            break
    return base, lags, secs


def region(env, arm):
    env.clear_history()
    env.clear_trades()
    t0 = time.perf_counter()
    env.run(CHUNK, sync=False)
    if arm.startswith("flow"):
        env.fold_flow()
    env.sync()
    return (time.perf_counter() - t0) * 1e6


def must_bytes(B, K, records):
    return records * 32 + B * (16 + 8) + B * 2 * ((8 + 6 * K) * 8 + 8 * K)


def part_run(args):
    for name in (w for w in args.workloads.split(",") if w):
        B = args.books or bench.WORKLOADS[name][0]
        arms = RUN_ARMS
        envs = {arm: make_env(name, B, arm) for arm in arms}
        for arm, e in envs.items():
            region(e, arm)  # untimed: the first launches
        us = {arm: [] for arm in envs}
        for _ in range(args.regions):
            for arm, e in envs.items():
                us[arm].append(region(e, arm))
        med = {arm: float(np.median(v)) for arm, v in us.items()}
        out = dict(part="run", workload=name, books=B, chunk=CHUNK, us_per_chunk={a: round(v, 1) for a, v in med.items()},
                   us_range={a: [round(min(v), 1), round(max(v), 1)] for a, v in us.items()},
                   regions={a: [round(x, 1) for x in v] for a, v in us.items()},
                   m_book_steps_per_s={a: round(B * CHUNK / v, 1) for a, v in med.items()})
        for arm in arms[1:]:
            adds = med[arm] - med["off"]
            out[arm] = dict(adds_us_per_chunk=round(adds, 1), adds_ns_per_book_step=round(adds * 1e3 / (B * CHUNK), 4),
                            share_of_chunk=round(adds / med["off"], 4))
            if arm.startswith("flow"):
                K = int(arm[4:])
                envs[arm].clear_flow()
                region(envs[arm], arm)  # one more chunk into a cleared table: what one fold reads
                rows = envs[arm].flow()
                n = int(rows["n_trades"].sum())
                out[arm].update(records_per_fold=n, trades_per_book_step=round(n / (B * CHUNK), 3), lost=int(rows["n_lost"].sum()),
                                pairs_at_lag_k=int(rows["lags"][:, K - 1, 0].sum()), must_bytes_per_fold=must_bytes(B, K, n),
                                must_tb_per_s=round(must_bytes(B, K, n) / (adds * 1e-6) / 1e12, 3) if adds > 0 else None)
        out["flags"] = int(np.bitwise_or.reduce(np.concatenate([e.flags() for e in envs.values()])))
        print(json.dumps(out), flush=True)
        for e in envs.values():
            e.close()


def part_host(args):
    B = args.books or bench.WORKLOADS["C3"][0]
    env = make_env("C3", B, "off")
    region(env, "off")  # untimed: the first launches
    us_run = region(env, "off")  # (leaves the chunk's records retained)
    t0 = time.perf_counter()
    off, rec = env.drain_trades()
    t1 = time.perf_counter()
    base_t0 = time.perf_counter()
    base, lags, secs = numpy_fold(off, rec, 16, args.host_budget)
    t2 = time.perf_counter()
    print(json.dumps(dict(part="host", workload="C3", books=B, chunk=CHUNK, records=int(len(rec)), record_bytes=int(rec.nbytes),
                          run_us=round(us_run, 1), drain_s=round(t1 - t0, 3), fold_s=round(t2 - base_t0, 3), lags_folded=len(lags),
                          base_s=round(t2 - base_t0 - sum(secs), 3), s_per_lag=[round(x, 3) for x in secs],
                          book_steps_per_s_of_drain_and_fold=round(B * CHUNK / (t2 - t0), 1), flags=int(np.bitwise_or.reduce(env.flags())))),
          flush=True)
    env.close()


class Arm(AR.IngressArm):
    def env(self, kind):
        e = super().env(kind == "accounts")
        if kind == "bars":
            e.enable_trade_bars(4)
        elif kind == "flow":
            e.enable_flow(16)
        return e


def part_ingress(args):
    for name, B in INGRESS_ARMS.items():
        B = args.books or B
        arm = Arm(B, args.iters, 16, False)
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
        assert len(set(trades.values())) == 1, trades  # the identical flow
        med = {k: float(np.median(v)) for k, v in us.items()}
        tr = trades["flow"] / (B * arm.iters)
        envs["flow"].clear_flow()
        arm.run(envs["flow"])  # one more region, kept: the table against the trade counts
        rows = envs["flow"].flow()
        out = dict(part="ingress", arm=name, books=B, iters=arm.iters, trades_per_book_step=round(tr, 3),
                   us_per_step={k: round(v, 1) for k, v in med.items()},
                   us_range={k: [round(min(v), 1), round(max(v), 1)] for k, v in us.items()},
                   adds_us_per_step={k: round(med[k] - med["off"], 1) for k in KINDS[1:]},
                   must_bytes_per_step=int(must_bytes(B, 16, B * tr)), records_in_table=int(rows["n_trades"].sum()),
                   records_made=int(envs["flow"].trade_counts().sum()), lost=int(rows["n_lost"].sum()),
                   flags=int(np.bitwise_or.reduce(envs["flow"].flags())))
        print(json.dumps(out), flush=True)
        for e in envs.values():
            e.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="run,ingress")
    ap.add_argument("--workloads", default="C3,C2")
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--iters", type=int, default=24, help="ingress: steps per region (the INGRESS stream fills the pools: <= 33)")
    ap.add_argument("--books", type=int, default=0, help="override the book count (a rehearsal)")
    ap.add_argument("--host-budget", type=float, default=90.0, help="host: seconds after which the numpy fold takes no further lag")
    args = ap.parse_args()
    parts = args.parts.split(",")
    if "run" in parts:
        part_run(args)
    if "ingress" in parts:
        part_ingress(args)
    if "host" in parts:
        part_host(args)


if __name__ == "__main__":
    main()
