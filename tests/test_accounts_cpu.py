"""Trader accounts (bk_accounts_enable) without a GPU: the plain-Python model against numbers worked out by hand, the
kernel's per-record arithmetic (bourse_amd/csrc/account_fold.hpp, compiled with g++) against the model, the C ABI - the
entries are exported, bound and declared, refuse a null env, and bk_account is 32 bytes laid out as ACCOUNT_DTYPE - and the
layout of the kernel's source."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import accounts_model as AM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("bk_accounts_enable", "bk_accounts_device_ptr", "bk_get_accounts", "bk_accounts_clear", "bk_accounts_clear_device")
BK_INVALID_ARGUMENT = 5
M64 = (1 << 64) - 1

TRADE = np.dtype([("side", "<u4"), ("price", "<u4"), ("vol", "<u4"), ("active_id", "<u8"), ("passive_id", "<u8")])
ORDER = np.dtype([("trader_id", "<u4")])


def _book(records, traders):
    """records (side_is_bid, price, vol, active id, passive id) and the orders' traders as the model's two arrays"""
    return np.array(records, dtype=TRADE), np.array([(t,) for t in traders], dtype=ORDER)


def test_the_model_against_rows_worked_out_by_hand():
    # orders 0..4 of traders 0, 1, 1, 2, 9 (9 has no row at n_traders = 3)
    trades, orders = _book([
        (0, 10, 5, 1, 0),   # passive ask of trader 0, active order of trader 1: 1 buys 5 at 10 from 0
        (1, 7, 2, 3, 2),    # passive bid of trader 1, active order of trader 2: 1 buys 2 at 7 from 2
        (1, 4, 3, 2, 1),    # passive bid of trader 1 hit by trader 1's own order: a self-trade of 3 at 4
        (0, 6, 1, 4, 0),    # trader 9 buys 1 at 6 from trader 0: only the seller has a row
    ], [0, 1, 1, 2, 9])
    rows = AM.fold(trades, orders, 3)
    assert rows.dtype == AM.ACCOUNT_DTYPE and rows.shape == (3,)
    assert rows[0].tolist() == (-6, 56, 6, 2)
    assert rows[1].tolist() == (7, -64, 13, 4)  # +5 +2 +3 -3; -50 -14 -12 +12; 5 + 2 + 3 + 3; the self-trade counts twice
    assert rows[2].tolist() == (-2, 14, 2, 1)
    assert AM.fold(trades, orders, 3, first=2)[1].tolist() == (0, 0, 6, 2)
    assert AM.parties_per_chunk(trades, orders, 0, 3) == 4
    # the words wrap modulo 2**64: two sales at the largest price and volume
    big, who = _book([(1, 0xFFFFFFFF, 0xFFFFFFFF, 1, 0)] * 3, [0, 1])
    r = AM.fold(big, who, 2)
    assert int(r[1]["cash"]) == AM._signed(3 * 0xFFFFFFFE00000001) and int(r[0]["cash"]) == AM._signed(-3 * 0xFFFFFFFE00000001)
    assert int(r[0]["position"]) == 3 * 0xFFFFFFFF and int(r[1]["position"]) == -3 * 0xFFFFFFFF


def _edge_records():
    out = []
    for side in (0, 1):
        out += [(side, 0xFFFFFFFF, 0xFFFFFFFF, 0, 1), (side, 0xFFFFFFFF, 0xFFFFFFFF, 1, 0), (side, 123, 0, 2, 3), (side, 0, 77, 3, 2),
                (side, 0, 0, 4, 4), (side, 0xFFFFFFFF, 1, 5, 5), (side, 1, 0xFFFFFFFF, 6, 0), (side, 2_000_000_000, 3_000_000_000, 0, 7)]
    return out


def test_account_fold_hpp_equals_the_model(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path / "account_fold_test")
    res = subprocess.run([gxx, "-std=c++17", "-O2", os.path.join(ROOT, "tests", "cpp", "account_fold_test.cpp"), "-o", exe],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    rng = np.random.default_rng(5)
    n, n_orders, n_traders = 4000, 600, 8
    traders = rng.integers(0, 11, size=n_orders)  # ids 8, 9, 10 have no row
    recs = [(int(rng.integers(0, 2)), int(rng.integers(0, 1 << 32)), int(rng.integers(0, 1 << 32)), int(rng.integers(0, n_orders)),
             int(rng.integers(0, n_orders))) for _ in range(n)]
    traders[:8] = np.arange(8)
    recs += _edge_records()  # (their order ids 0..7 are traders 0..7)
    # the wrap-around of a row: the largest product many times over on one pair of traders
    recs += [(1, 0xFFFFFFFF, 0xFFFFFFFF, 0, 1)] * 9
    trades, orders = _book(recs, traders)
    want = AM.fold_ints(trades, orders, n_traders)
    assert any(abs(r[1]) >> 64 for r in want), "no row's cash wraps: the case checks less than it says"
    with open(tmp_path / "records.txt", "w") as f:
        f.write(f"{n_traders} {len(recs)}\n")
        for side, price, vol, a, p in recs:
            f.write(f"{side} {price} {vol} {int(traders[a])} {int(traders[p])}\n")
    with open(tmp_path / "expected.txt", "w") as f:
        for row in want:
            f.write(" ".join(str(x & M64) for x in row) + "\n")
    run = subprocess.run([exe, str(tmp_path / "records.txt"), str(tmp_path / "expected.txt")], capture_output=True, text=True,
                         timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip().endswith(f"account_fold ok {len(recs)} records {n_traders} traders")
    # a wrong expectation is really caught: one word off by one
    want[3][1] += 1
    with open(tmp_path / "expected.txt", "w") as f:
        for row in want:
            f.write(" ".join(str(x & M64) for x in row) + "\n")
    run = subprocess.run([exe, str(tmp_path / "records.txt"), str(tmp_path / "expected.txt")], capture_output=True, text=True,
                         timeout=120)
    assert run.returncode == 1 and "trader 3" in run.stdout


def test_the_entries_are_exported_bound_and_declared():
    import bourse_amd
    from bourse_amd import _lib

    L = _lib.load()
    header = open(os.path.join(ROOT, "include", "bourse_amd.h")).read()
    for name in ENTRIES:
        assert hasattr(L, name) and name in _lib.SIGNATURES, name
        m = re.search(r"\b" + name + r"\s*\([^;]*;", header)
        assert m, name
        assert re.search(r"\(No counterpart\s+(\*\s+)?in\s+(\*\s+)?the reference\.\)\s*\*/\s*int\s+$", header[:m.start()]), name
    assert re.search(r"#define BK_FLAG_ACCOUNTS_INEXACT 512u", header) and _lib.FLAG_ACCOUNTS_INEXACT == 512
    taken = [int(v) for v in re.findall(r"#define BK_FLAG_\w+ (\d+)u", header)]
    assert len(taken) == len(set(taken)), taken  # the bit was free
    assert 512 in _lib.FLAG_NAMES and "ACCOUNTS_INEXACT" in _lib.FLAG_NAMES[512]
    for method in ("enable_accounts", "accounts", "accounts_device_ptr", "accounts_view", "clear_accounts"):
        assert callable(getattr(bourse_amd.ManyBookEnv, method)), method
        assert getattr(bourse_amd.ManyMarketEnv, method) is getattr(bourse_amd.ManyBookEnv, method), method
    assert bourse_amd.ManyBookEnv.ACCOUNT_DTYPE is _lib.ACCOUNT_DTYPE
    hpp = open(os.path.join(ROOT, "include", "bourse_amd.hpp")).read()
    for method in ("enable_accounts", "accounts", "accounts_device_ptr", "clear_accounts"):
        assert re.search(r"\b" + method + r"\(", hpp), method
    rs = open(os.path.join(ROOT, "integration", "rust", "bourse_amd_sys.rs")).read()
    for name in ENTRIES:
        assert re.search(r"pub fn " + name + r"\(", rs), name
    assert "pub struct BkAccount" in rs and "pub position: i64" in rs and "pub fills: u64" in rs
    assert "pub const BK_FLAG_ACCOUNTS_INEXACT: u32 = 512;" in rs


def test_bk_account_is_32_bytes_laid_out_as_the_dtype(tmp_path):
    from bourse_amd import _lib

    dt = _lib.ACCOUNT_DTYPE
    assert dt.itemsize == 32 and dt.names == ("position", "cash", "volume", "fills")
    assert [dt.fields[n][1] for n in dt.names] == [0, 8, 16, 24]
    assert [dt.fields[n][0].str for n in dt.names] == ["<i8", "<i8", "<u8", "<u8"]
    assert dt == AM.ACCOUNT_DTYPE
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    src = tmp_path / "layout.cpp"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "bourse_amd.h"\n'
                   'int main() { std::printf("%zu %zu %zu %zu %zu\\n", sizeof(bk_account), offsetof(bk_account, position), '
                   'offsetof(bk_account, cash), offsetof(bk_account, volume), offsetof(bk_account, fills)); return 0; }\n')
    exe = str(tmp_path / "layout")
    res = subprocess.run([gxx, "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60).stdout.split()
    assert [int(x) for x in out] == [32, 0, 8, 16, 24]


def test_a_null_env_is_refused_not_dereferenced():
    from bourse_amd import _lib

    L = _lib.load()
    mask = (ctypes.c_uint8 * 4)(1, 0, 1, 0)
    out = ctypes.c_void_p()
    rows = np.zeros(4, dtype=_lib.ACCOUNT_DTYPE)
    calls = {
        "bk_accounts_enable": lambda: L.bk_accounts_enable(None, 4, 0),
        "bk_accounts_device_ptr": lambda: L.bk_accounts_device_ptr(None, ctypes.byref(out)),
        "bk_get_accounts": lambda: L.bk_get_accounts(None, 0, 1, rows.ctypes.data_as(ctypes.c_void_p)),
        "bk_accounts_clear": lambda: L.bk_accounts_clear(None, ctypes.cast(mask, ctypes.c_void_p)),
        "bk_accounts_clear_device": lambda: L.bk_accounts_clear_device(None, ctypes.cast(mask, ctypes.c_void_p)),
    }
    assert set(calls) == set(ENTRIES)
    for name, call in calls.items():
        L.bk_device_count(ctypes.byref(ctypes.c_int(0)))  # (anything that may leave another message behind)
        assert call() == BK_INVALID_ARGUMENT, name
        assert b"null env" in L.bk_last_error(), name


def test_the_kernels_stay_out_of_the_baselined_namespace_and_hold_no_assembly():
    """bkd::accounts kernels are not among the names tools/kernel_isa_counts.py::measure lists (those start with k_ once
    "void bkd::" is stripped), so profiles/kernel_isa_baseline.json stays as it is; the fold is plain C++ and shares its
    per-record arithmetic with the CPU test through account_fold.hpp."""
    src = open(os.path.join(ROOT, "bourse_amd", "csrc", "accounts.hpp")).read()
    body = src[src.index("namespace bkd {"):]
    assert re.search(r"namespace bkd \{\s*namespace accounts \{", body)
    for k in ("k_fold", "k_clear"):
        assert re.search(r"__global__[^;{]*\b" + k + r"\(", body), k
    code = re.sub(r"//.*", "", src)
    assert "asm" not in code and "atomic" not in code and "__shared__" not in code
    assert '#include "account_fold.hpp"' in src
    for f in ("parties(", "buyer_delta(", "seller_delta("):
        assert f in code, f
    fold = open(os.path.join(ROOT, "bourse_amd", "csrc", "account_fold.hpp")).read()
    assert re.search(r"namespace bkd \{\s*namespace accounts \{", fold)
    assert "hip_runtime" not in fold and "asm" not in re.sub(r"//.*", "", fold)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_isa_counts as K
    import json

    base = json.load(open(K.BASELINE))["kernels"]
    assert not [k for k in base if "accounts" in k or "k_fold" in k]
