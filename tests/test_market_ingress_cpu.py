"""The market update entries (bk_update_market_agents / bk_update_market_members) without a GPU: the pass schedule of
bourse_amd/csrc/market_walk.hpp, compiled with g++, against a plain-Python schedule over random group lists and a case
worked out by hand; the C ABI - both entries are exported, bound, declared and refuse a null env; the kernels sit in the
nested namespace and share the walk with the book kernels."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BK_INVALID_ARGUMENT = 5
ENTRIES = ("bk_update_market_agents", "bk_update_market_members")


def schedule(groups):
    """[(first, len, asset, trader0, group)] of a list of (n, asset): every agent gets (asset of its group, index in its
    group); a pass is a maximal run of at most 64 consecutive agents of one asset"""
    agents = [(asset, t, g) for g, (n, asset) in enumerate(groups) for t in range(n)]
    passes, i = [], 0
    while i < len(agents):
        k = i + 1
        while k < len(agents) and k - i < 64 and agents[k][0] == agents[i][0]:
            k += 1
        passes.append((i, k - i, agents[i][0], agents[i][1], agents[i][2]))
        i = k
    return passes


def test_the_plain_schedule_on_the_hand_worked_case():
    # groups of 70 / 5 / 0 / 20 / 64 / 40 agents on assets 0, 1, 2, 0, 2, 1: the first takes two passes, the empty group
    # ends nothing, the walk returns to assets 0, 2 and 1
    groups = [(70, 0), (5, 1), (0, 2), (20, 0), (64, 2), (40, 1)]
    assert schedule(groups) == [(0, 64, 0, 0, 0), (64, 6, 0, 64, 0), (70, 5, 1, 0, 1), (75, 20, 0, 0, 3), (95, 64, 2, 0, 4),
                                (159, 40, 1, 0, 5)]
    # two groups of one asset share a pass; an empty group between them does not cut it; a pass is cut at 64 inside the second
    groups = [(5, 1), (0, 0), (65, 1), (130, 1), (1, 0)]
    assert schedule(groups) == [(0, 64, 1, 0, 0), (64, 64, 1, 59, 2), (128, 64, 1, 58, 3), (192, 8, 1, 122, 3), (200, 1, 0, 0, 4)]


def _random_lists(rng, n_lists):
    sizes = [0, 5, 64, 65, 130, 1, 63, 70, 128]
    lists = []
    for _ in range(n_lists):
        assets = int(rng.integers(1, 9))
        n_groups = int(rng.integers(0, 9))
        lists.append([(int(rng.choice(sizes)) if rng.random() < 0.7 else int(rng.integers(0, 200)), int(rng.integers(0, assets)))
                      for _ in range(n_groups)])
    return lists


def test_market_walk_hpp_equals_the_plain_schedule(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path / "market_walk_test")
    res = subprocess.run([gxx, "-std=c++17", "-O2", os.path.join(ROOT, "tests", "cpp", "market_walk_test.cpp"), "-o", exe],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    rng = np.random.default_rng(18)
    lists = [[(70, 0), (5, 1), (0, 2), (20, 0), (64, 2), (40, 1)], [(5, 1), (0, 0), (65, 1), (130, 1), (1, 0)], [], [(0, 0)],
             [(0, 3), (0, 1)]] + _random_lists(rng, 2000)
    returns = sum(1 for l in lists if any(a == l[i][1] and l[i + 1][1] != a for i, (_, a) in enumerate(l[:-2])
                                           for _, a2 in l[i + 2:] if a2 == a))
    shared = sum(1 for l in lists for p in schedule(l) if p[3] + p[1] > l[p[4]][0])  # a pass that holds more than one group
    assert returns > 300 and shared > 300, (returns, shared)
    for size in (0, 5, 64, 65, 130):
        assert sum(1 for l in lists for n, _ in l if n == size) > 100, size
    assert {max((a for _, a in l), default=0) for l in lists} >= set(range(8))
    with open(tmp_path / "lists.txt", "w") as f:
        f.write(f"{len(lists)}\n")
        for l in lists:
            f.write(f"{len(l)}" + "".join(f" {n} {a}" for n, a in l) + "\n")
    run = subprocess.run([exe, str(tmp_path / "lists.txt"), str(tmp_path / "passes.txt")], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip().endswith(f"market_walk ok {len(lists)} lists")
    got, cur = [], []
    for line in open(tmp_path / "passes.txt"):
        if line.strip() == "-":
            got.append(cur)
            cur = []
        else:
            cur.append(tuple(int(x) for x in line.split()))
    assert len(got) == len(lists)
    for i, (l, g) in enumerate(zip(lists, got)):
        assert g == schedule(l), f"list {i} {l}: {g} vs {schedule(l)}"


def test_the_entries_are_exported_bound_and_declared():
    import bourse_amd
    from bourse_amd import _lib

    L = _lib.load()
    header = open(os.path.join(ROOT, "include", "bourse_amd.h")).read()
    hpp = open(os.path.join(ROOT, "include", "bourse_amd.hpp")).read()
    rust = open(os.path.join(ROOT, "integration", "rust", "bourse_amd_sys.rs")).read()
    for name in ENTRIES:
        assert hasattr(L, name), name
        assert name in _lib.SIGNATURES, name
        assert re.search(rf"\bint {name}\(bk_env\* env\);", header), name
        assert f"{name}(h_)" in hpp, name
        assert f"pub fn {name}(env: *mut BkEnv) -> c_int;" in rust, name
    for method in ("update_market_agents", "update_market_members"):
        assert callable(getattr(bourse_amd.ManyBookEnv, method)), method
        assert getattr(bourse_amd.ManyMarketEnv, method) is getattr(bourse_amd.ManyBookEnv, method), method
    # the header cites the reference's traits
    for cite in ("random_agent.rs:204-245", "noise_agent.rs:226-340", "momentum_agent.rs:282-397", "runner.rs:108-131"):
        assert cite in header, cite


def test_a_null_env_is_refused():
    from bourse_amd import _lib

    L = _lib.load()
    for name in ENTRIES:
        L.bk_device_count(ctypes.byref(ctypes.c_int(0)))  # (anything that may leave another message behind)
        assert getattr(L, name)(None) == BK_INVALID_ARGUMENT, name
        assert b"null env" in L.bk_last_error(), name


def test_the_kernels_sit_in_the_nested_namespace_and_share_the_walk():
    """bkd::ingress::k_update_market_* are not among the names the ISA baselines list (profiles/*.json stay as they are),
    take their passes from market_walk.hpp, and run the book kernels' own pass and member code - no copy of it, no LDS,
    no atomic."""
    import json

    src = open(os.path.join(ROOT, "bourse_amd", "csrc", "market_ingress.hpp")).read()
    assert re.search(r"namespace bkd \{\s*namespace ingress \{", src)
    for k in ("k_update_market_agents", "k_update_market_members"):
        assert re.search(rf"__global__[^;{{]*\b{k}\(", src), k
    code = re.sub(r"//.*", "", src)
    assert "asm" not in code and "atomic" not in code and "__shared__" not in code
    assert '#include "market_walk.hpp"' in src and '#include "members_ingress.hpp"' in src
    for f in ("next_pass(", "random_agent<R>(", "random_pass_end(", '#include "members_update_body.inc"'):
        assert f in code, f
    book = open(os.path.join(ROOT, "bourse_amd", "csrc", "members_ingress.hpp")).read()
    assert '#include "members_update_body.inc"' in book  # ONE text of a member's update for both kernels
    walk = open(os.path.join(ROOT, "bourse_amd", "csrc", "market_walk.hpp")).read()
    assert "hip_runtime" not in walk and "asm" not in re.sub(r"//.*", "", walk)
    for prof in ("kernel_isa_baseline.json", "kernel_isa_members_ingress.json"):
        base = json.load(open(os.path.join(ROOT, "profiles", prof)))["kernels"]
        assert not [k for k in base if "market_agents" in k or "market_members" in k], prof
    # the book entries keep their refusal of markets
    host = open(os.path.join(ROOT, "bourse_amd", "csrc", "bourse_amd.hip")).read()
    assert "bk_update_agents runs RandomAgents on independent books (assets == 1)" in host
    assert "bk_update_members runs an AgentSet on independent books (assets == 1)" in host
