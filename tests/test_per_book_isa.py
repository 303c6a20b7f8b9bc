"""The per-unit parameter table's kernels (bk_set_random_agents_per_book) on the instruction-count yardstick of
tools/kernel_isa_counts.py, measured on the library the suite has just built: the lane-per-book draw loop of
k_agents_fsm<2, true> stays within three instructions of the uniform kernel's 66 (the parameters moved from scalar to
vector operands, no per-draw copies), and the wave-parallel decode's loops of k_agents_wave<R, true> match the uniform
kernel's within +-2 instructions each (the twelve largest) (the book's record is a scalar load, as DevArgs::groups is)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def counts():
    import kernel_isa_counts as K
    from bourse_amd import _build

    if not all(K._tool(t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-objdump")):
        pytest.skip("no llvm-objdump / clang-offload-bundler")
    return K.measure(_build.build())


def draw_loop(k):  # (the largest loop of at most 80 instructions: 66 in the uniform kernel)
    return max(l for l in k["loops"] if l <= 80)


def test_fsm_draw_loop_of_the_per_book_form(counts):
    assert draw_loop(counts["k_agents_fsm<2>"]) == 66, counts["k_agents_fsm<2>"]["loops"]
    for R in (1, 2, 4, 8):
        pb = counts[f"k_agents_fsm<{R}, true>"]
        assert draw_loop(pb) <= 69, (R, pb["loops"])
        assert pb["counts"]["smem"] <= counts[f"k_agents_fsm<{R}>"]["counts"]["smem"]  # (no scalar parameter loads added)


def test_wave_decode_loops_of_the_per_book_form(counts):
    for R in (1, 2, 4, 8):
        u, pb = counts[f"k_agents_wave<{R}>"], counts[f"k_agents_wave<{R}, true>"]
        assert len(u["loops"]) == len(pb["loops"]), R
        # the twelve largest loops, the decode's window / walk / chase loops (further down the sorted lists the small loops
        # of the shuffle resolution trade places, which a by-position comparison cannot follow)
        assert all(abs(x - y) <= 2 for x, y in zip(u["loops"][:12], pb["loops"][:12])), (R, u["loops"], pb["loops"])
        assert abs(u["counts"]["valu"] - pb["counts"]["valu"]) <= 2, R  # (the ballots keep scalar operands)


def test_fused_per_book_kernels_exist(counts):
    for R in (1, 2, 4, 8):
        u, pb = counts[f"k_run_wave<{R}>"], counts[f"k_run_wave<{R}, true>"]
        assert abs(u["counts"]["total"] - pb["counts"]["total"]) <= 0.03 * u["counts"]["total"], R
