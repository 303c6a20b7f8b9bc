"""On-device Noise / Momentum members beside submitted instructions (bk_update_members): the rate of one env's step when its
AgentSet goes through the device-resident ingress queues, next to bk_run on the same AgentSet.  Two shapes:
  c5m    bench.py's C5M member set (256 momentum + 256 noise traders), 8 192 books, a 512-slot pool, 64 levels;
  small  the small mixed set of the parity tests (10 momentum + 20 noise traders), 65 536 books, a 128-slot pool, 10 levels.
Three arms, each its own env, alternated round by round after a warm-up (bench.py's discipline: every arm sees the same
clocks), the median of the rounds reported:
  run      bk_run on the same AgentSet (the default pipeline of the shape);
  members  update_members + step, no external instruction;
  mixed    update_members + 16 external instructions per book-step from device arrays (bk_submit_instructions_device) + step.
One JSON line per shape.  GPU box:  python scripts/members_ingress_rate.py [--shapes c5m,small] [--steps K] [--rounds N]
Per-launch kernel times:  rocprofv3 --kernel-trace --stats -- python scripts/members_ingress_rate.py --shapes c5m --arm members"""
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
SHAPES = {
    # name: (books, pool, levels, members)
    "c5m": (8192, 512, 64, [("momentum", 0, 256, MOM_P), ("noise", 256, 256, NOISE_P)]),  # bench.py C5M
    "small": (65536, 128, 10, [("momentum", 0, 10, dict(MOM_P, demand=5.0)),
                               ("noise", 10, 20, dict(NOISE_P, p_limit=0.2, p_cancel=0.1))]),  # tests/test_gpu_parity.py
}
TICK, STEP, NX = 2, 100_000, 16


def make_env(shape, arm, spl):
    B, pool, levels, members = SHAPES[shape]
    stream = torch.cuda.current_stream().cuda_stream
    per_update = sum(2 * m[2] for m in members)
    e = bk.ManyBookEnv(B, 101, 0, TICK, STEP, levels=levels, max_live_orders=pool, trade_capacity=per_update * spl,
                       strict=False, history_capacity=0, stream=stream)
    if arm != "run":  # every trader's two orders and a cancellation for every order that can rest
        e.enable_device_ingress(per_update + pool + (NX if arm == "mixed" else 0))
    e.set_agents(members)
    return e


class External:
    """16 instructions per book-step made on the device ahead of the timed loop: 60 % limit orders in a band of prices
    (bids at its top, asks at its bottom: most of them trade at once), 25 % cancellations and 15 % modifications of ids the
    book created two steps or more before (the members' ids and external ones alike)."""

    def __init__(self, B, n_batches):
        g = torch.Generator(device="cuda").manual_seed(5)
        n = B * NX
        self.off = torch.arange(B + 1, dtype=torch.int64, device="cuda") * NX
        self.batches = []
        for s in range(n_batches):
            u = torch.rand(n, device="cuda", generator=g)
            action = torch.where(u < 0.6, 1, torch.where(u < 0.85, 2, 0x80000003)).to(torch.int32)
            if s < 2:
                action = torch.ones_like(action)
            side = torch.randint(0, 2, (n,), device="cuda", generator=g, dtype=torch.uint8)
            side = torch.where(action == 1, side, side * 6)  # modifications: price and volume, or neither
            vol = torch.randint(1, 30, (n,), device="cuda", generator=g, dtype=torch.int32)
            tick = torch.randint(0, 4, (n,), device="cuda", generator=g, dtype=torch.int32)
            price = torch.where(side == 1, 63 - tick, 32 + tick) * TICK
            trader = torch.full((n,), 100_000, dtype=torch.int32, device="cuda")
            ids = (torch.rand(n, device="cuda", generator=g) * max(1, 30 * (s - 1))).to(torch.int64) * (action != 1)
            self.batches.append((action, side, vol, trader, price, ids))


def steps(env, arm, k, ext, s0):
    if arm == "run":
        env.run(k, sync=False)
        return
    for s in range(s0, s0 + k):
        env.update_members(sync=False)
        if ext is not None:
            env.submit_instructions_device(ext.off, *ext.batches[s % len(ext.batches)])
        env.step(sync=False)


def measure(shape, k, rounds, warm):
    B, pool, levels, members = SHAPES[shape]
    arms = ("run", "members", "mixed")
    envs = {a: make_env(shape, a, k) for a in arms}
    ext = External(B, warm + k * rounds)
    done = {a: 0 for a in arms}
    rates = {a: [] for a in arms}
    torch.cuda.synchronize()
    for a in arms:
        steps(envs[a], a, warm, ext if a == "mixed" else None, 0)
        done[a] += warm
    torch.cuda.synchronize()
    for r in range(rounds):
        for a in (arms if r % 2 == 0 else arms[::-1]):
            envs[a].clear_trades()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            steps(envs[a], a, k, ext if a == "mixed" else None, done[a])
            torch.cuda.synchronize()
            rates[a].append(B * k / (time.perf_counter() - t0))
            done[a] += k
    out = {"shape": shape, "books": B, "pool": pool, "levels": levels, "traders": sum(m[2] for m in members),
           "external_per_book_step": NX, "steps_per_round": k, "rounds": rounds, "warmup": warm}
    for a in arms:
        f = envs[a].flags()
        out[a] = {"M_book_steps_per_s": float(np.median(rates[a])) / 1e6, "values_M": [v / 1e6 for v in rates[a]],
                  "flags": [int(x) for x in np.unique(f)]}
        envs[a].close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="c5m,small")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--arm", default=None, help="time one arm alone (members / mixed / run): for a kernel trace")
    args = ap.parse_args()
    for shape in args.shapes.split(","):
        if args.arm:
            env = make_env(shape, args.arm, args.warmup + args.steps)
            ext = External(SHAPES[shape][0], args.warmup + args.steps) if args.arm == "mixed" else None
            steps(env, args.arm, args.warmup + args.steps, ext, 0)
            torch.cuda.synchronize()
            print(json.dumps({"shape": shape, "arm": args.arm, "steps": args.warmup + args.steps,
                              "flags": [int(x) for x in np.unique(env.flags())]}))
            env.close()
            continue
        print(json.dumps(measure(shape, args.steps, args.rounds, args.warmup)), flush=True)


if __name__ == "__main__":
    main()
