"""One public-API configuration per instantiation of ingress::k_update_members<R> (bourse_amd/csrc/members_ingress.hpp), in
the style of tests/kernel_cases.py.  The kernel lives in a nested namespace, so tools/kernel_isa_counts.py::measure - which
takes the names that start with "k_" once "void bkd::" is stripped - does not list it, and profiles/kernel_isa_baseline.json
and tests/kernel_cases.py stay as they are; its instruction counts are in profiles/kernel_isa_members_ingress.json
(tests/test_members_ingress_isa.py) and its parity cases here (tests/test_members_ingress_cases.py keeps the two equal,
tests/test_gpu_members_with_ingress.py runs every entry, with every member set below, against the CPU oracle).

Which instantiation a configuration launches: bk_update_members picks R = max_live_orders / 64 (by_R, bourse_amd.hip).

Plain data: importing this module initialises nothing.
"""
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILE = os.path.join(ROOT, "profiles", "kernel_isa_members_ingress.json")
FAMILY = "ingress::k_update_members"
POOLS = {1: 64, 2: 128, 4: 256, 8: 512}
SETS = ("noise", "momentum", "mixed", "mixed_reversed")

# the parameters of the existing suites: NOISE of tests/test_gpu_agents_with_ingress.py (= NOISE_P of tests/test_gpu_parity.py)
# and MOM_P of tests/test_gpu_parity.py (the reference's doc example, crates/step_sim/src/lib.rs:53-73)
NOISE = dict(tick_size=2, p_limit=0.2, p_market=0.2, p_cancel=0.1, trade_vol=100, price_dist_mu=0.0, price_dist_sigma=1.0)
MOM = dict(tick_size=2, p_cancel=0.1, trade_vol=100, decay=1.0, demand=5.0, scale=0.5, order_ratio=1.0, price_dist_mu=0.0,
           price_dist_sigma=10.0)


def member_set(R, which):
    """The AgentSet of a case: a Noise member alone, a Momentum member alone, or RandomAgents + Noise + Momentum in that
    order / reversed.  The RandomAgents member grows with the pool: at rate 1 every agent places an order in the first
    update, and with trading off for that step (the GPU test does that) they all rest - more than 64 (R - 1) orders, the
    pool's last register in use.  A 64-slot pool takes shorter-lived orders (a higher p_cancel) and fewer agents."""
    small = R == 1
    noise = dict(NOISE, p_cancel=0.3) if small else NOISE
    mom = dict(MOM, p_cancel=0.7) if small else MOM
    n_rand = 64 * (R - 1) + 8 if R > 1 else 12
    rnd = ("random", n_rand, (32, 64), (10, 20), 2, 1.0)
    if which == "noise":
        return [("noise", 0, 20, noise)]
    if which == "momentum":
        return [("momentum", 0, 10, mom)]
    mixed = [rnd, ("noise", n_rand, 6 if small else 10, noise), ("momentum", n_rand + 10, 6 if small else 10, mom)]
    assert which in ("mixed", "mixed_reversed"), which
    return mixed if which == "mixed" else mixed[::-1]


CASES = {}
for _R in (1, 2, 4, 8):
    CASES[f"{FAMILY}<{_R}>"] = dict(name=f"{FAMILY}<{_R}>", R=_R, pool=POOLS[_R], books=64, steps=30, sets=SETS, unreachable=None)


def profile_kernels(path=PROFILE):
    with open(path) as f:
        return set(json.load(f)["kernels"])
