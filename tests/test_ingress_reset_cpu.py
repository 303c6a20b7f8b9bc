"""The device-ingress reset's C ABI without a GPU: the five entries are exported, bound and declared, refuse a null env
instead of crashing, the Python methods exist, and the Rust declarations carry them."""
import ctypes
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("bk_ingress_snapshot_save", "bk_ingress_snapshot_drop", "bk_ingress_snapshot_bytes", "bk_ingress_reset_books_device",
           "bk_ingress_reset_books")
BK_INVALID_ARGUMENT = 5


def test_the_five_entries_are_exported_bound_and_declared():
    import bourse_amd

    L = bourse_amd._lib.load()
    header = open(os.path.join(ROOT, "include", "bourse_amd.h")).read()
    for name in ENTRIES:
        assert hasattr(L, name) and name in bourse_amd._lib.SIGNATURES, name
        m = re.search(r"\b" + name + r"\s*\([^;]*;", header)
        assert m, name
        # "(No counterpart in the reference.)" closes the comment in front of the declaration
        assert re.search(r"\(No counterpart\s+(\*\s+)?in the reference\.\)\s*\*/\s*(int|uint64_t)\s+$", header[:m.start()]), name
    for method in ("save_ingress_snapshot", "drop_ingress_snapshot", "ingress_snapshot_bytes", "reset_ingress_books"):
        assert callable(getattr(bourse_amd.ManyBookEnv, method)), method
    assert callable(bourse_amd.ManyMarketEnv.reset_ingress_markets)
    hpp = open(os.path.join(ROOT, "include", "bourse_amd.hpp")).read()
    for method in ("save_ingress_snapshot", "drop_ingress_snapshot", "reset_ingress_books"):
        assert re.search(r"\bvoid " + method + r"\(", hpp), method


def test_a_null_env_is_refused_not_dereferenced():
    import bourse_amd

    L = bourse_amd._lib.load()
    mask = (ctypes.c_uint8 * 4)(1, 0, 1, 0)
    assert L.bk_ingress_snapshot_save(None, 0) == BK_INVALID_ARGUMENT
    assert L.bk_ingress_snapshot_drop(None, 0) == BK_INVALID_ARGUMENT
    assert L.bk_ingress_reset_books(None, 0, ctypes.cast(mask, ctypes.c_void_p), None) == BK_INVALID_ARGUMENT
    assert L.bk_ingress_reset_books_device(None, 0, ctypes.cast(mask, ctypes.c_void_p), None) == BK_INVALID_ARGUMENT
    assert b"null env" in L.bk_last_error()
    assert L.bk_ingress_snapshot_bytes(None, 0) == 0


def test_the_rust_declarations_are_current():
    path = os.path.join(ROOT, "integration", "rust", "bourse_amd_sys.rs")
    before = open(path).read()
    for name in ENTRIES:
        assert re.search(r"pub fn " + name + r"\(", before), name
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_rust_sys.py")], check=True, capture_output=True)
    assert open(path).read() == before, "regenerate integration/rust/bourse_amd_sys.rs (tools/gen_rust_sys.py)"


def test_the_new_kernels_stay_out_of_the_baselined_namespace():
    """bkd::reset kernels are not among the names tools/kernel_isa_counts.py::measure lists (those start with k_ once
    "void bkd::" is stripped), so profiles/kernel_isa_baseline.json stays as it is."""
    src = open(os.path.join(ROOT, "bourse_amd", "csrc", "ingress_reset.hpp")).read()
    body = src[src.index("namespace bkd {"):]
    assert re.search(r"namespace bkd \{\s*namespace reset \{", body)
    for k in ("k_collect_units", "k_reset_records", "k_max_keep"):
        assert re.search(r"__global__[^;{]*\b" + k + r"\(", body), k
    assert "asm" not in re.sub(r"//.*", "", src)  # plain C++: no inline assembly
