"""On-device market agents beside submitted instructions (bk_update_market_agents / bk_update_market_members): the rate of
one market env's step when its agents go through the device-resident ingress queues, next to bk_run on the same agents.
Three assets of tick 2, a 512-slot pool, 10 levels.  Three arms, each its own env, alternated round by round after a
warm-up (bench.py's discipline: every arm sees the same clocks), medians reported:
  run      bk_run on the same agents (a set of more than four members has no bk_run: the arm is left out);
  agents   update_market_agents (or update_market_members) + step, no external instruction;
  mixed    the same + 16 external instructions per book-step from device arrays (bk_submit_instructions_device).
--set agents: six RandomMarketAgents groups in asset order 0, 1, 2, 0, 2, 1 (70 / 5 / 0 / 20 / 64 / 40 agents);
--set members: the seven members of tests/test_gpu_market_members_with_ingress.py.
One JSON line per market count.  GPU box:  python scripts/market_agents_rate.py [--set agents] [--markets 8192,21845]"""
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

TICKS, POOL, LEVELS, STEP, NX = [2, 2, 2], 512, 10, 100_000, 16
RND = (32, 64), (10, 20), 2
GROUPS = [(0, 70, *RND, 0.8), (1, 5, (30, 66), (50, 70), 2, 0.5), (2, 0, *RND, 0.8), (0, 20, (30, 66), (50, 70), 2, 0.3),
          (2, 64, *RND, 0.8), (1, 40, *RND, 0.7)]
NOISE = dict(tick_size=2, p_limit=0.2, p_market=0.2, p_cancel=0.1, trade_vol=100, price_dist_mu=0.0, price_dist_sigma=1.0)
MOM = dict(tick_size=2, p_cancel=0.1, trade_vol=100, decay=1.0, demand=5.0, scale=0.5, order_ratio=1.0, price_dist_mu=0.0,
           price_dist_sigma=10.0)
MEMBERS = [(0, ("random", 72, *RND, 0.8)), (1, ("noise", 1000, 20, NOISE)), (0, ("momentum", 2000, 10, MOM)),
           (2, ("random", 5, *RND, 0.8)), (1, ("momentum", 3000, 10, MOM)),
           (2, ("noise", 4000, 70, dict(NOISE, p_limit=0.6, p_market=0.3))), (0, ("noise", 5000, 12, NOISE))]


def events(which):
    if which == "agents":
        return sum(g[1] for g in GROUPS)
    return sum(m[1] if m[0] == "random" else 2 * m[2] for _, m in MEMBERS) + 3 * POOL


def make_env(NM, which, arm, spl):
    stream = torch.cuda.current_stream().cuda_stream
    e = bk.ManyMarketEnv(NM, 101, 0, TICKS, STEP, levels=LEVELS, max_live_orders=POOL, trade_capacity=64 * spl, strict=False,
                         history_capacity=0, stream=stream)
    if arm != "run":
        e.enable_device_ingress(events(which) + (len(TICKS) * NX if arm == "mixed" else 0))
    if which == "agents":
        e.set_random_market_agents(GROUPS)
    else:
        e.set_market_agents(MEMBERS)
    return e


class External:
    """16 instructions per book-step made on the device ahead of the timed loop: 60 % limit orders at the far ends of the
    agents' price range (most trade at once), 25 % cancellations and 15 % modifications of ids the book created earlier"""

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
            side = torch.where(action == 1, side, side * 6)
            vol = torch.randint(1, 30, (n,), device="cuda", generator=g, dtype=torch.int32)
            tick = torch.randint(0, 4, (n,), device="cuda", generator=g, dtype=torch.int32)
            price = torch.where(side == 1, 63 - tick, 32 + tick) * 2
            trader = torch.full((n,), 9000, dtype=torch.int32, device="cuda")
            ids = (torch.rand(n, device="cuda", generator=g) * max(1, 30 * (s - 1))).to(torch.int64) * (action != 1)
            self.batches.append((action, side, vol, trader, price, ids))


def steps(env, which, arm, k, ext, s0):
    if arm == "run":
        env.run(k, sync=False)
        return
    update = env.update_market_agents if which == "agents" else env.update_market_members
    for s in range(s0, s0 + k):
        update(sync=False)
        if ext is not None:
            env.submit_instructions_device(ext.off, *ext.batches[s % len(ext.batches)])
        env.step(sync=False)


def measure(NM, which, k, rounds, warm):
    arms = ("run", "agents", "mixed") if which == "agents" else ("agents", "mixed")
    envs = {a: make_env(NM, which, a, k) for a in arms}
    ext = External(NM * len(TICKS), warm + k * rounds)
    done = {a: 0 for a in arms}
    rates = {a: [] for a in arms}
    torch.cuda.synchronize()
    for a in arms:
        steps(envs[a], which, a, warm, ext if a == "mixed" else None, 0)
        done[a] += warm
    torch.cuda.synchronize()
    for r in range(rounds):
        for a in (arms if r % 2 == 0 else arms[::-1]):
            envs[a].clear_trades()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            steps(envs[a], which, a, k, ext if a == "mixed" else None, done[a])
            torch.cuda.synchronize()
            rates[a].append(NM * len(TICKS) * k / (time.perf_counter() - t0))
            done[a] += k
    out = {"set": which, "markets": NM, "assets": len(TICKS), "pool": POOL, "levels": LEVELS, "external_per_book_step": NX,
           "steps_per_round": k, "rounds": rounds, "warmup": warm}
    for a in arms:
        f = envs[a].flags()
        out[a] = {"M_book_steps_per_s": float(np.median(rates[a])) / 1e6, "values_M": [v / 1e6 for v in rates[a]],
                  "flags": [int(x) for x in np.unique(f)]}
        envs[a].close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--set", default="agents", choices=("agents", "members"))
    ap.add_argument("--markets", default="8192,21845")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--arm", default=None, help="run one arm alone (agents / mixed / run): for a kernel trace")
    args = ap.parse_args()
    for NM in (int(x) for x in args.markets.split(",")):
        if args.arm:
            env = make_env(NM, args.set, args.arm, args.warmup + args.steps)
            ext = External(NM * len(TICKS), args.warmup + args.steps) if args.arm == "mixed" else None
            steps(env, args.set, args.arm, args.warmup + args.steps, ext, 0)
            torch.cuda.synchronize()
            print(json.dumps({"set": args.set, "markets": NM, "arm": args.arm, "steps": args.warmup + args.steps,
                              "flags": [int(x) for x in np.unique(env.flags())]}))
            env.close()
            continue
        print(json.dumps(measure(NM, args.set, args.steps, args.rounds, args.warmup)), flush=True)


if __name__ == "__main__":
    main()
