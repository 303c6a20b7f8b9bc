"""The compile-time switch of k_agents_fsm's hand-written shuffle and publish loops (BOURSE_AMD_FSM_TAIL, fsm_asm.hpp) on
the instruction-count yardstick of tools/kernel_isa_counts.py.

Switch off: fsm_unit.hip compiled with -DBOURSE_AMD_FSM_TAIL=0 (bourse_amd/_build.py's own flag list, device code only: two
seconds) gives k_agents_fsm<1|2|4|8> the parent commit's counts and loop spans exactly - the entries the committed baseline
held before these statements existed, kept in profiles/fsm_tail/kernel_isa_parent.json.  Switch on (the library the suite has
built): the kernel's largest loop of at most 80 instructions is still the 66-instruction compiled draw loop of its C++ copy
(tests/test_per_book_isa.py finds the draw loop that way), and the two new loops are the 30- and 19-instruction ones."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
PARENT = os.path.join(ROOT, "profiles", "fsm_tail", "kernel_isa_parent.json")
UNIFORM = [f"k_agents_fsm<{R}>" for R in (1, 2, 4, 8)]


@pytest.fixture(scope="module")
def K():
    import kernel_isa_counts as K

    if not all(K._tool(t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-objdump")):
        pytest.skip("no llvm-objdump / clang-offload-bundler")
    return K


def _fsm_unit_counts(K, tmp_path, defines):
    """k_agents_fsm's kernels of fsm_unit.hip compiled as bourse_amd/_build.py compiles it, plus `defines`."""
    from bourse_amd import _build

    obj = str(tmp_path / "fsm_unit.co")
    cmd = [_build.hipcc_path()] + _build.fsm_unit_flags(defines) + ["--cuda-device-only", "--no-gpu-bundle-output", "-c", "-o", obj,
                                                                     os.path.join(_build.CSRC, "fsm_unit.hip")]
    res = subprocess.run(cmd, cwd=_build.CSRC, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    ks = K.kernels_of(obj)
    names = K.demangle(sorted(ks))
    return {names[n]: v for n, v in ks.items()}


def test_switch_off_reproduces_the_parents_kernels(K, tmp_path):
    want = json.load(open(PARENT))["kernels"]
    got = _fsm_unit_counts(K, tmp_path, ["BOURSE_AMD_FSM_TAIL=0"])
    assert sorted(want) == UNIFORM
    for k in UNIFORM:
        assert got[k] == want[k], (k, got[k], want[k])


def test_switch_on_keeps_the_draw_loop_the_largest_small_loop(K):
    from bourse_amd import _build

    now = K.measure(_build.build())
    for k in UNIFORM:
        loops = now[k]["loops"]
        assert max(l for l in loops if l <= 80) == 66, (k, loops)  # the C++ copy's draw loop
        assert not [l for l in loops if 67 <= l <= 80], (k, loops)
        assert 30 in loops and 19 in loops, (k, loops)  # the hand-written shuffle, the publish loop's full groups
    parent = json.load(open(PARENT))["kernels"]
    for k in UNIFORM:  # the statements are shorter than what they replace
        assert now[k]["counts"]["total"] < parent[k]["counts"]["total"], k
