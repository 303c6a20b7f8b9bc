"""One public-API configuration per shipped kernel instantiation (the keys of "kernels" in profiles/kernel_isa_baseline.json).

tests/test_gpu_kernel_cases.py runs every entry against the CPU oracle; tests/test_kernel_case_table.py keeps the table's
names equal to the baseline's.  Which instantiation a configuration launches follows make_plan (pipeline_plan.hpp) and the
launch code of bourse_amd.hip (launch_fused, launch_split, launch_events, bk_update_agents):

  flow "run"     bk_run with on-device agents: the plan's fused kernel, or per step and part its agents kernel + k_step_batch
                 (k_step_batch_log with the agents' order log, k_step_decode under BOURSE_AMD_STEP_DECODE=1 on wave_split);
                 the first launch of the members' lane / wave split rebuilds their order lists (k_mixed_lists_rebuild /
                 k_wave_lists_rebuild)
  flow "host"    host calls + bk_step: k_step_events<R, MARKETS, CHUNKS, MODS>; CHUNKS when the longest queue of the step
                 exceeds 64 R events, MODS = false only at R = 8 until the env has seen a modification
  flow "update"  device ingress + bk_update_agents (k_update_agents<R>) + bk_step

Plain data: importing this module initialises nothing.
"""
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASELINE = os.path.join(ROOT, "profiles", "kernel_isa_baseline.json")

POOLS = {1: 64, 2: 128, 4: 256, 8: 512}
FLOWS = ("run", "host", "update")
AGENTS = (None, "random", "random_table", "members", "members_table")
REQUESTS = ("auto", "fused", "split", "split_wave", "wave_split", "wave")
# what pipeline() reports (kind, parts) for the run flow
KINDS = ("fused", "split", "wave_split", "wave")
# books (or markets) per workgroup of each kernel family; one book per workgroup where absent
PER_BLOCK = {"k_run_random": 4, "k_run_mixed": 4, "k_agents_wave": 4, "k_agents_mixed": 4, "k_step_decode": 4,
             "k_mixed_lists_rebuild": 4, "k_wave_lists_rebuild": 4, "k_run_wave": 8, "k_agents_mixed_wave": 8,
             "k_agents_fsm": 64, "k_agents_mixed_lanes": 64}
TICKS = (1, 2)  # the markets' books

# ---------------------------------------------------------------------------------------------------- the agents
# RandomAgents (n, tick_range, vol_range, tick_size, rate): a filler group of 64 (R - 1) + 8 agents at rate 1 places an
# order each odd step and cancels it each even one, so a run's first launch - an odd number of steps with trading off -
# ends with more than 64 (R - 1) orders resting (the pool's last register in use); the next launches trade.  A second,
# slower group keeps trading.
# Variant 1 is another row of a per-book (per-market) table: same sizes, other ranges and rates.


def random_groups(R, variant=0):
    n_fill = 64 * (R - 1) + 8 if R > 1 else 40
    if variant == 0:
        return [(n_fill, (20, 200), (10, 20), 2, 1.0), (8, (40, 160), (1, 40), 2, 0.5)]
    return [(n_fill, (30, 150), (5, 30), 2, 1.0), (8, (60, 120), (20, 60), 2, 0.7)]


def random_market_groups(R, variant=0):
    """(asset, n, tick_range, vol_range, tick_size, rate): the filler on asset 0 (the market's queue holds every asset's
    events: 64 (R - 1) + 8 + 8 <= 64 R)"""
    (nf, tf, vf, sf, rf), (na, ta, va, sa, ra) = random_groups(R, variant)
    return [(0, nf, tf, vf, sf, rf), (1, na, ta, va, sa, ra)]


def noise_params(variant=0):
    # limit orders below / above the mid (they rest), a few market orders; 1 / p_cancel steps of life
    if variant == 0:
        return dict(tick_size=1, p_limit=1.0, p_market=0.1, p_cancel=0.25, trade_vol=20, price_dist_mu=0.0,
                    price_dist_sigma=3.0)
    return dict(tick_size=1, p_limit=0.9, p_market=0.15, p_cancel=0.2, trade_vol=15, price_dist_mu=0.5,
                price_dist_sigma=4.0)


def momentum_params(variant=0):
    return dict(tick_size=1, p_cancel=0.1 if variant == 0 else 0.2, trade_vol=20, decay=1.0 if variant == 0 else 0.6,
                demand=5.0, scale=0.5, order_ratio=1.0, price_dist_mu=0.0, price_dist_sigma=3.0)


def members(R, variant=0):
    """An AgentSet: the RandomAgents filler as its first member (one order per agent at most, so a step's queue never
    takes the pool past n_fill + the others' few dozen), then Noise and Momentum traders"""
    n_fill = 64 * (R - 1) + 8 if R > 1 else 16
    tr, rate = ((90, 110), 1.0) if variant == 0 else ((85, 115), 1.0)
    return [("random", n_fill, tr, (10, 20), 1, rate), ("noise", n_fill, 4, noise_params(variant)),
            ("momentum", n_fill + 4, 3, momentum_params(variant))]


def market_members(R, variant=0):
    """[(asset, member)]: the set of members() on asset 0 and a few noise traders on asset 1 (tick 2)"""
    rnd, noi, mom = members(R, variant)
    return [(0, rnd), (0, noi), (0, mom), (1, ("noise", mom[1] + mom[2], 4, dict(noise_params(1 - variant), tick_size=2)))]


# ---------------------------------------------------------------------------------------------------- the table
CASES = {}


def _add(name, **cfg):
    assert name not in CASES, name
    R = int(name.split("<")[1].split(",")[0].rstrip(">"))
    case = dict(name=name, R=R, pool=POOLS[R], flow="run", units=6, markets=False, agents=None, pipeline=None,
                split_parts=None, wave_options=None, log=False, knobs={}, launches=(3, 4), kind=None, parts=1,
                chunks=False, mods_from=None, unreachable=None)
    case.update(cfg)
    CASES[name] = case


def _b(v):
    return "true" if v else "false"


for R in (1, 2, 4, 8):
    la = 5 if R in (2, 8) else 64  # a small look-ahead (the decode's scalar slow path) on some wave-decode cases
    # RandomAgents on independent books
    _add(f"k_run_random<{R}>", agents="random", pipeline="fused", kind="fused")
    _add(f"k_run_wave<{R}>", agents="random", pipeline="wave", units=10, kind="wave", wave_options=(la, 0))
    _add(f"k_run_wave<{R}, true>", agents="random_table", pipeline="wave", units=10, kind="wave")
    _add(f"k_agents_fsm<{R}>", agents="random", pipeline="split", units=198, split_parts=(3, 64), kind="split", parts=3)
    _add(f"k_agents_fsm<{R}, true>", agents="random_table", pipeline="split", units=198, split_parts=(3, 64), kind="split",
         parts=3)
    _add(f"k_agents_wave<{R}>", agents="random", pipeline="wave_split", units=198, wave_options=(la, 3), kind="wave_split",
         parts=3)
    _add(f"k_agents_wave<{R}, true>", agents="random_table", pipeline="wave_split", units=198, wave_options=(64, 3),
         kind="wave_split", parts=3)
    _add(f"k_step_batch<{R}, false, false>", agents="random", pipeline="split", kind="split")
    _add(f"k_step_batch_log<{R}, false>", agents="random", pipeline="split", units=198, split_parts=(3, 64), log=True,
         kind="split", parts=3)
    _add(f"k_step_decode<{R}>", agents="random", pipeline="wave_split", units=198, wave_options=(la if R == 2 else 64, 3),
         knobs={"BOURSE_AMD_STEP_DECODE": "1"}, kind="wave_split", parts=3)
    # RandomMarketAgents (the lane split is the markets' only split form)
    _add(f"k_step_batch<{R}, true, false>", agents="random", markets=True, units=5, kind="split")
    _add(f"k_step_batch_log<{R}, true>", agents="random", markets=True, units=5, log=True, kind="split")
    # AgentSets with Noise / Momentum members on independent books
    _add(f"k_run_mixed<{R}>", agents="members", pipeline="fused", kind="fused")
    _add(f"k_run_mixed<{R}, true>", agents="members_table", pipeline="fused", kind="fused")
    _add(f"k_agents_mixed<{R}>", agents="members", pipeline="split_wave", units=198, split_parts=(3, 64), kind="split", parts=3)
    _add(f"k_agents_mixed<{R}, true>", agents="members_table", pipeline="split_wave", units=198, split_parts=(3, 64),
         kind="split", parts=3)
    _add(f"k_agents_mixed_lanes<{R}, false>", agents="members", pipeline="split", units=198, split_parts=(3, 64), kind="split",
         parts=3)
    _add(f"k_agents_mixed_lanes<{R}, false, true>", agents="members_table", pipeline="split", units=198, split_parts=(3, 64),
         kind="split", parts=3)
    _add(f"k_agents_mixed_wave<{R}>", agents="members", pipeline="wave_split", units=198, wave_options=(la, 3),
         kind="wave_split", parts=3)
    _add(f"k_agents_mixed_wave<{R}, true>", agents="members_table", pipeline="wave_split", units=198, wave_options=(64, 3),
         kind="wave_split", parts=3)
    _add(f"k_step_batch<{R}, false, true>", agents="members", pipeline="split", kind="split")
    _add(f"k_mixed_lists_rebuild<{R}>", agents="members", pipeline="split", kind="split")
    _add(f"k_wave_lists_rebuild<{R}>", agents="members", pipeline="wave_split", kind="wave_split")
    # ... on markets
    _add(f"k_agents_mixed_lanes<{R}, true>", agents="members", markets=True, units=198, split_parts=(3, 64), kind="split",
         parts=3)
    _add(f"k_agents_mixed_lanes<{R}, true, true>", agents="members_table", markets=True, units=198, split_parts=(3, 64),
         kind="split", parts=3)
    _add(f"k_step_batch<{R}, true, true>", agents="members", markets=True, units=5, kind="split")
    # RandomAgents into the device-resident queues
    _add(f"k_update_agents<{R}>", flow="update", agents="random")
    # host-driven steps
    for mkt in (False, True):
        units = 5 if mkt else 6
        _add(f"k_step_events<{R}, {_b(mkt)}, true, true>", flow="host", markets=mkt, units=units, chunks=True, mods_from=1,
             launches=(1, 4))
        if R < 8:
            _add(f"k_step_events<{R}, {_b(mkt)}, false, true>", flow="host", markets=mkt, units=units, mods_from=1,
                 launches=(1, 4))
        else:  # the same steps before and after the env's first modification
            for mods in (False, True):
                _add(f"k_step_events<8, {_b(mkt)}, false, {_b(mods)}>", flow="host", markets=mkt, units=units, mods_from=3,
                     launches=(1, 4))


def part_sizes(units, parts):
    """The units of each part of a split launch (launch_split: boundaries rounded down to multiples of 4)."""
    cut = [(units * i // parts) & ~3 for i in range(parts)] + [units]
    return [cut[i + 1] - cut[i] for i in range(parts)]


def family(name):
    return name.split("<")[0]


def baseline_kernels(path=BASELINE):
    with open(path) as f:
        return set(json.load(f)["kernels"])


def compare_with_baseline(names, kernels):
    """(baseline instantiations without a case, cases without a baseline instantiation), both sorted"""
    names, kernels = set(names), set(kernels)
    return sorted(kernels - names), sorted(names - kernels)
