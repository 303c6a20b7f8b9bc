"""The stamp compaction without a GPU: the rank rule of bourse_amd/csrc/stamp_rows.hpp, compiled with g++,
against arrival numbers that never wrapped and against the plain sort of tests/stamp_model.py - over pools of every pool
size whose stamps straddle 2^32, ties impossible, dead slots untouched, a fixed point - and the layout of the kernel's
source."""
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import stamp_model as SM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M32 = 1 << 32


def _pool(rng, n_slots):
    """A pool made from the truth: the k-th order to rest since the book's start carries stamp (start + k) mod 2^32.  Returns
    (counter, live, stamps, arrival numbers of the live slots or None)."""
    start = int(rng.choice([0, 1, M32 - 1, M32 - 5, M32 - n_slots // 2, int(rng.integers(0, M32))]))
    n_live = int(rng.integers(0, n_slots + 1))
    # the live orders arrived within a window of fewer than 2^32 rests that ends at the counter
    span = int(rng.choice([n_live + 1, 3 * n_slots, 1 << 16, M32 - 1]))
    span = max(span, n_live + 1)
    total = int(rng.integers(span, span + 1000))          # rests so far
    offs = set(int(x) for x in rng.integers(0, span, size=n_live))
    while len(offs) < n_live:
        offs.add(int(rng.integers(0, span)))
    ks = [total - 1 - x for x in rng.permutation(sorted(offs)).tolist()]
    live = np.zeros(n_slots, dtype=bool)
    live[rng.choice(n_slots, size=n_live, replace=False)] = True
    seq = rng.integers(0, M32, size=n_slots).astype(object)    # dead slots: stale words
    arrival = {}
    for slot, k in zip(np.flatnonzero(live), ks):
        seq[slot] = (start + int(k)) % M32
        arrival[int(slot)] = int(k)
    return (start + total) % M32, live, [int(x) for x in seq], arrival


def test_stamp_rows_hpp_ranks_by_arrival(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path / "stamp_rows_test")
    res = subprocess.run([gxx, "-std=c++17", "-O2", os.path.join(ROOT, "tests", "cpp", "stamp_rows_test.cpp"), "-o", exe],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    rng = np.random.default_rng(23)
    pools = [_pool(rng, n) for n in (64, 128, 256, 512) for _ in range(150)]
    # hand-made: the level of the issue (stamps 2^32 - 5 .. 2), an empty pool, a full one right at the wrap
    pools.append((3, np.ones(8, dtype=bool), [M32 - 5, M32 - 4, M32 - 3, M32 - 2, M32 - 1, 0, 1, 2], {i: i for i in range(8)}))
    pools.append((M32 - 1, np.zeros(64, dtype=bool), list(range(64)), {}))
    pools.append((0, np.ones(64, dtype=bool), [(M32 - 64 + (i * 37) % 64) for i in range(64)], {i: (i * 37) % 64 for i in range(64)}))
    straddling = 0
    with open(tmp_path / "pools.txt", "w") as f:
        f.write(f"{len(pools)}\n")
        for ctr, live, seq, arrival in pools:
            f.write(f"{ctr} {len(seq)}\n" + "".join(f"{int(live[i])} {seq[i]}\n" for i in range(len(seq))))
            s = [seq[i] for i in arrival]
            straddling += bool(s) and max(s) - min(s) > M32 // 2
    assert straddling > 100, straddling
    run = subprocess.run([exe, str(tmp_path / "pools.txt"), str(tmp_path / "out.txt")], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip().endswith(f"stamp_rows ok {len(pools)} pools")
    got = [[int(x) for x in line.split()] for line in open(tmp_path / "out.txt")]
    assert len(got) == len(pools)
    for p, ((ctr, live, seq, arrival), g) in enumerate(zip(pools, got)):
        new_ctr, new = g[0], g[1:]
        assert new_ctr == len(arrival), p
        by_arrival = sorted(arrival, key=lambda i: arrival[i])
        assert [new[i] for i in by_arrival] == list(range(len(arrival))), f"pool {p}: ranks are not the arrival order"
        assert len({new[i] for i in arrival}) == len(arrival), f"pool {p}: a tie"
        assert all(new[i] == seq[i] for i in range(len(seq)) if not live[i]), f"pool {p}: a dead slot changed"
        assert (new_ctr, new) == SM.compact(ctr, live, seq), f"pool {p}: the plain sort differs"
        assert SM.compact(new_ctr, live, new) == (new_ctr, new), f"pool {p}: not a fixed point"


def test_the_plain_sort_on_a_level_worked_out_by_hand():
    # stamps 2^32 - 2, 2^32 - 1, 0, 1 handed out in that order, counter 2; slot 2 is dead and keeps its word
    ctr, out = SM.compact(2, [1, 1, 0, 1, 1, 1], [0, M32 - 1, 77, 1, M32 - 2, M32 - 7])
    assert ctr == 5 and out == [3, 2, 77, 4, 1, 0]
    assert SM.compact(0, [0, 0], [5, 6]) == (0, [5, 6])


def test_the_kernel_stays_out_of_the_baselined_namespace_and_is_plain_hip():
    """bkd::stamps::k_compact is not among the names the ISA baseline lists, so profiles/kernel_isa_baseline.json stays as it
    is; the kernel is plain C++ - no inline assembly, no atomic, no LDS, no shuffle - and shares its rule with the CPU test
    through stamp_rows.hpp; the stepping kernels' sources do not mention it."""
    src = open(os.path.join(ROOT, "bourse_amd", "csrc", "stamp_compact.hpp")).read()
    assert re.search(r"namespace bkd \{\s*namespace stamps \{", src)
    assert re.search(r"__global__[^;{]*\bk_compact\(", src)
    code = re.sub(r"//.*", "", src)
    assert "asm" not in code and "atomic" not in code and "__shared__" not in code and "__shfl" not in code
    assert '#include "stamp_rows.hpp"' in src and "older(" in code
    rows = open(os.path.join(ROOT, "bourse_amd", "csrc", "stamp_rows.hpp")).read()
    assert "hip_runtime" not in rows and "asm" not in re.sub(r"//.*", "", rows)
    base = json.load(open(os.path.join(ROOT, "profiles", "kernel_isa_baseline.json")))["kernels"]
    assert not [k for k in base if "stamps" in k or "k_compact" in k]
    for name in ("book_device.hpp", "step_events.hpp", "event_asm.hpp", "wave_agents.hpp", "mixed_agents.hpp"):
        assert "stamps::" not in open(os.path.join(ROOT, "bourse_amd", "csrc", name)).read(), name


def test_the_entry_and_the_knobs_are_declared():
    import bourse_amd
    from bourse_amd import _lib

    L = _lib.load()
    assert hasattr(L, "bk_stamp_compactions") and "bk_stamp_compactions" in _lib.SIGNATURES
    header = open(os.path.join(ROOT, "include", "bourse_amd.h")).read()
    assert re.search(r"\bbk_stamp_compactions\s*\([^;]*;", header)
    assert callable(bourse_amd.ManyBookEnv.stamp_compactions)
    assert re.search(r"pub fn bk_stamp_compactions\(", open(os.path.join(ROOT, "integration", "rust", "bourse_amd_sys.rs")).read())
    assert "bk_stamp_compactions" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "BOURSE_AMD_SEQ_START" in readme and "BOURSE_AMD_STAMP_ROOM" in readme
    import ctypes

    out = ctypes.c_uint64(0)
    assert L.bk_stamp_compactions(None, ctypes.byref(out)) == 5 and b"null env" in L.bk_last_error()
