"""On-device RandomAgents beside submitted instructions (bk_update_agents): the rate of one env's step when its agents go
through the device-resident ingress queues, next to bk_run's fused / split pipelines on the same agents.  C3's agents (two
groups, 128 agents), a 128-slot pool, 32 levels.  Three arms, each its own env, alternated round by round after a warm-up
(bench.py's discipline: every arm sees the same clocks):
  run      bk_run on the same agents (the default pipeline of the shape);
  agents   update_agents + step, no external instruction;
  mixed    update_agents + 16 external instructions per book-step from device arrays (bk_submit_instructions_device) + step.
One JSON line per book count.  GPU box:  python scripts/agents_ingress_rate.py [--books 8192,65536] [--steps K] [--rounds N]"""
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

GROUPS = [(64, (32, 64), (10, 20), 2, 0.8), (64, (32, 64), (50, 70), 2, 0.2)]  # bench.py C3
POOL, LEVELS, TICK, STEP, NX = 128, 32, 2, 100_000, 16


def make_env(B, arm, spl):
    stream = torch.cuda.current_stream().cuda_stream
    e = bk.ManyBookEnv(B, 101, 0, TICK, STEP, levels=LEVELS, max_live_orders=POOL, trade_capacity=64 * spl, strict=False,
                       history_capacity=0, stream=stream)
    if arm != "run":
        e.enable_device_ingress(128 + (NX if arm == "mixed" else 0))
    e.set_random_agents(GROUPS)
    return e


class External:
    """16 instructions per book-step made on the device ahead of the timed loop: 60 % limit orders at the far end of the
    agents' price range (bids at the top, asks at the bottom: most of them trade at once and the 128-slot pool keeps room),
    25 % cancellations and 15 % modifications of ids the book created two steps or more before (agents' ids and external
    ones alike)."""

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
            trader = torch.full((n,), 1000, dtype=torch.int32, device="cuda")
            ids = (torch.rand(n, device="cuda", generator=g) * max(1, 30 * (s - 1))).to(torch.int64) * (action != 1)
            self.batches.append((action, side, vol, trader, price, ids))


def steps(env, arm, k, ext, s0):
    if arm == "run":
        env.run(k, sync=False)
        return
    for s in range(s0, s0 + k):
        env.update_agents(sync=False)
        if ext is not None:
            env.submit_instructions_device(ext.off, *ext.batches[s % len(ext.batches)])
        env.step(sync=False)


def measure(B, k, rounds, warm):
    arms = ("run", "agents", "mixed")
    envs = {a: make_env(B, a, k) for a in arms}
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
    out = {"books": B, "pool": POOL, "levels": LEVELS, "agents": sum(g[0] for g in GROUPS), "external_per_book_step": NX,
           "steps_per_round": k, "rounds": rounds, "warmup": warm}
    for a in arms:
        f = envs[a].flags()
        out[a] = {"M_book_steps_per_s": float(np.median(rates[a])) / 1e6, "values_M": [v / 1e6 for v in rates[a]],
                  "flags": [int(x) for x in np.unique(f)]}
        envs[a].close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--books", default="8192,65536")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--arm", default=None, help="time one arm alone (agents / mixed / run): for a kernel trace")
    args = ap.parse_args()
    for B in (int(x) for x in args.books.split(",")):
        if args.arm:
            env = make_env(B, args.arm, args.warmup + args.steps)
            ext = External(B, args.warmup + args.steps) if args.arm == "mixed" else None
            steps(env, args.arm, args.warmup + args.steps, ext, 0)
            torch.cuda.synchronize()
            print(json.dumps({"books": B, "arm": args.arm, "steps": args.warmup + args.steps,
                              "flags": [int(x) for x in np.unique(env.flags())]}))
            env.close()
            continue
        print(json.dumps(measure(B, args.steps, args.rounds, args.warmup)), flush=True)


if __name__ == "__main__":
    main()
