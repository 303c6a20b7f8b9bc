"""The open-order view (bk_open_orders_enable) without a GPU: the plain-Python model against rows worked out by hand, the
kernel's row arithmetic (bourse_amd/csrc/open_order_rows.hpp, compiled with g++) against the model over random pools of every
pool size, the C ABI - the entries are exported, bound and declared, refuse a null env, bk_open_summary and bk_open_order are
laid out as the dtypes, no flag bit was added - and the layout of the kernel's source."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import open_orders_model as OM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("bk_open_orders_enable", "bk_open_orders_refresh", "bk_open_orders_device_ptrs", "bk_get_open_orders")
BK_INVALID_ARGUMENT = 5
ORDER = np.dtype([("order_id", "<u8"), ("trader_id", "<u4"), ("side", "u1"), ("status", "u1"), ("price", "<u4"), ("vol", "<u4")])


def _orders(rows):
    """rows (order id, trader, side_is_bid, status, price, remaining volume) as the model's array"""
    return np.array(rows, dtype=ORDER)


def test_the_model_against_rows_worked_out_by_hand():
    book = _orders([
        (0, 0, 1, 1, 100, 5),    # trader 0 rests on both sides
        (1, 0, 0, 1, 110, 7),
        (2, 1, 1, 1, 99, 4),     # a bid of 10 of which 4 are left: the remaining volume counts
        (3, 1, 1, 1, 101, 3),
        (4, 1, 0, 1, 120, 2),    # trader 1's third resting order: beyond depth = 2
        (5, 2, 1, 2, 90, 9),     # Filled: trader 2 rests nothing
        (6, 7, 0, 1, 130, 1),    # trader 7 has no row at n_traders = 3
        (7, 0, 0, 3, 105, 1),    # Cancelled
    ])
    summary, entries = OM.rows(book, 3, 2)
    assert summary.dtype == OM.OPEN_SUMMARY_DTYPE and summary.shape == (3,)
    assert entries.dtype == OM.OPEN_ORDER_DTYPE and entries.shape == (3, 2)
    assert summary.tolist() == [(5, 7, 1, 1, 100, 110), (7, 2, 2, 1, 101, 120), (0, 0, 0, 0, 0, 0xFFFFFFFF)]
    assert entries[0].tolist() == [(0, 100, 5, 1), (1, 110, 7, 0)]
    assert entries[1].tolist() == [(2, 99, 4, 1), (3, 101, 3, 1)]  # the oldest two; n_bid + n_ask = 3 > depth says so
    assert entries[2].tolist() == [(0xFFFFFFFF, 0, 0, 0)] * 2
    # a deeper list is padded with the empty entry, depth 0 has no entries at all
    assert OM.rows(book, 3, 4)[1][1].tolist() == [(2, 99, 4, 1), (3, 101, 3, 1), (4, 120, 2, 0), (0xFFFFFFFF, 0, 0, 0)]
    s0, e0 = OM.rows(book, 3, 0)
    assert s0.tolist() == summary.tolist() and e0.shape == (3, 0)
    # ids at or beyond max_orders have no record on the device: left out
    s4, e4 = OM.rows(book, 3, 2, max_orders=4)
    assert s4[1].tolist() == (7, 0, 2, 0, 101, 0xFFFFFFFF) and e4[1].tolist() == entries[1].tolist()
    # the volume sums are 64-bit
    big = _orders([(i, 0, 1, 1, 10 + i, 0xFFFFFFFF) for i in range(3)])
    assert OM.rows(big, 1, 1)[0][0].tolist() == (3 * 0xFFFFFFFF, 0, 3, 0, 12, 0xFFFFFFFF)


def _random_pool(rng, n_slots):
    n_traders, depth = int(rng.integers(1, 12)), int(rng.integers(0, 9))
    live = rng.random(n_slots) < rng.random()
    ids = rng.choice(1 << 20, size=n_slots, replace=False).astype(np.uint64)
    if rng.random() < 0.3:
        ids += np.uint64(0xFFF00000)  # ids near the top of the u32 range compare as unsigned
    vol = rng.integers(0, 1 << 32, size=n_slots)
    if rng.random() < 0.3:
        vol[:] = 0xFFFFFFFF
    price = rng.integers(0, 1 << 32, size=n_slots)
    if rng.random() < 0.3:
        price = rng.integers(0, 4, size=n_slots) * 0x55555555  # ties, 0 and 0xFFFFFFFF among the prices
    side = rng.integers(0, 2, size=n_slots)
    trader = rng.integers(0, n_traders + 3, size=n_slots)  # the last three ids have no row
    return n_traders, depth, live, ids, price, vol, side, trader


def test_open_order_rows_hpp_equals_the_model(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path / "open_order_rows_test")
    res = subprocess.run([gxx, "-std=c++17", "-O2", os.path.join(ROOT, "tests", "cpp", "open_order_rows_test.cpp"), "-o", exe],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    rng = np.random.default_rng(9)
    pools = [_random_pool(rng, n) for n in (64, 128, 256, 512) for _ in range(600)]
    want, wide, deep, skipped = [], 0, 0, 0
    with open(tmp_path / "pools.txt", "w") as f:
        f.write(f"{len(pools)}\n")
        for n_traders, depth, live, ids, price, vol, side, trader in pools:
            f.write(f"{len(ids)} {n_traders} {depth}\n")
            f.write("".join(f"{int(live[i])} {ids[i]} {price[i]} {vol[i]} {side[i]} {trader[i]}\n" for i in range(len(ids))))
            book = np.zeros(len(ids), dtype=ORDER)
            book["order_id"], book["trader_id"], book["side"], book["price"], book["vol"] = ids, trader, side, price, vol
            book["status"] = np.where(live, 1, 2)
            summary, entries = OM.rows_ints(book, n_traders, depth)
            for s, e in zip(summary, entries):
                want.append([s[0] & 0xFFFFFFFF, s[0] >> 32, s[1] & 0xFFFFFFFF, s[1] >> 32, *s[2:]] + [x for ent in e for x in ent])
                wide += s[0] >> 32 != 0 or s[1] >> 32 != 0
                deep += s[2] + s[3] > depth
            skipped += int((live & (trader >= n_traders)).sum())
    assert wide > 100 and deep > 100 and skipped > 100, (wide, deep, skipped)
    run = subprocess.run([exe, str(tmp_path / "pools.txt"), str(tmp_path / "rows.txt")], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip().endswith(f"open_order_rows ok {len(pools)} pools")
    got = [[int(x) for x in line.split()] for line in open(tmp_path / "rows.txt")]
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"row {i}: {g} vs {w}"


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
    for method in ("enable_open_orders", "refresh_open_orders", "open_orders", "open_orders_device_ptrs", "open_orders_views"):
        assert callable(getattr(bourse_amd.ManyBookEnv, method)), method
        assert getattr(bourse_amd.ManyMarketEnv, method) is getattr(bourse_amd.ManyBookEnv, method), method
    assert bourse_amd.OPEN_SUMMARY_DTYPE is _lib.OPEN_SUMMARY_DTYPE and bourse_amd.OPEN_ORDER_DTYPE is _lib.OPEN_ORDER_DTYPE
    hpp = open(os.path.join(ROOT, "include", "bourse_amd.hpp")).read()
    for method in ("enable_open_orders", "refresh_open_orders", "open_orders", "open_orders_device_ptrs"):
        assert re.search(r"\b" + method + r"\(", hpp), method
    rs = open(os.path.join(ROOT, "integration", "rust", "bourse_amd_sys.rs")).read()
    for name in ENTRIES:
        assert re.search(r"pub fn " + name + r"\(", rs), name
    assert "pub struct BkOpenSummary" in rs and "pub bid_vol: u64" in rs and "pub best_ask: u32" in rs
    assert "pub struct BkOpenOrder" in rs and "pub side_is_bid: u32" in rs
    md = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ENTRIES:
        assert name in md, name


def test_no_flag_bit_was_added():
    from bourse_amd import _lib

    header = open(os.path.join(ROOT, "include", "bourse_amd.h")).read()
    taken = sorted(int(v) for v in re.findall(r"#define BK_FLAG_\w+ (\d+)u", header))
    assert taken == [1, 2, 4, 8, 16, 32, 64, 128, 256, 512], taken
    assert sorted(_lib.FLAG_NAMES) == [1, 2, 4, 8, 16, 32, 64, 128, 256, 512]


def test_the_structs_are_laid_out_as_the_dtypes(tmp_path):
    from bourse_amd import _lib

    s, e = _lib.OPEN_SUMMARY_DTYPE, _lib.OPEN_ORDER_DTYPE
    assert s.itemsize == 32 and s.names == ("bid_vol", "ask_vol", "n_bid", "n_ask", "best_bid", "best_ask")
    assert [s.fields[n][1] for n in s.names] == [0, 8, 16, 20, 24, 28]
    assert [s.fields[n][0].str for n in s.names] == ["<u8", "<u8", "<u4", "<u4", "<u4", "<u4"]
    assert e.itemsize == 16 and e.names == ("order_id", "price", "vol", "side_is_bid")
    assert [e.fields[n][1] for n in e.names] == [0, 4, 8, 12] and all(e.fields[n][0].str == "<u4" for n in e.names)
    assert s == OM.OPEN_SUMMARY_DTYPE and e == OM.OPEN_ORDER_DTYPE
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    src = tmp_path / "layout.cpp"
    fields = [("bk_open_summary", n) for n in s.names] + [("bk_open_order", n) for n in e.names]
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "bourse_amd.h"\n'
                   'int main() { std::printf("%zu %zu", sizeof(bk_open_summary), sizeof(bk_open_order));\n' +
                   "".join(f'std::printf(" %zu", offsetof({t}, {n}));\n' for t, n in fields) + "return 0; }\n")
    exe = str(tmp_path / "layout")
    res = subprocess.run([gxx, "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60).stdout.split()
    assert [int(x) for x in out] == [32, 16, 0, 8, 16, 20, 24, 28, 0, 4, 8, 12]


def test_a_null_env_is_refused_not_dereferenced():
    from bourse_amd import _lib

    L = _lib.load()
    a, b = ctypes.c_void_p(), ctypes.c_void_p()
    summary = np.zeros(4, dtype=_lib.OPEN_SUMMARY_DTYPE)
    entries = np.zeros(8, dtype=_lib.OPEN_ORDER_DTYPE)
    calls = {
        "bk_open_orders_enable": lambda: L.bk_open_orders_enable(None, 4, 2),
        "bk_open_orders_refresh": lambda: L.bk_open_orders_refresh(None),
        "bk_open_orders_device_ptrs": lambda: L.bk_open_orders_device_ptrs(None, ctypes.byref(a), ctypes.byref(b)),
        "bk_get_open_orders": lambda: L.bk_get_open_orders(None, 0, 1, summary.ctypes.data_as(ctypes.c_void_p),
                                                           entries.ctypes.data_as(ctypes.c_void_p)),
    }
    assert set(calls) == set(ENTRIES)
    for name, call in calls.items():
        L.bk_device_count(ctypes.byref(ctypes.c_int(0)))  # (anything that may leave another message behind)
        assert call() == BK_INVALID_ARGUMENT, name
        assert b"null env" in L.bk_last_error(), name


def test_the_kernel_stays_out_of_the_baselined_namespace_and_is_plain_hip():
    """bkd::open_orders::k_refresh is not among the names the ISA baseline lists (those start with k_ once "void bkd::" is
    stripped), so profiles/kernel_isa_baseline.json stays as it is; the kernel is plain C++ - no inline assembly, no atomic,
    no LDS - and shares its row arithmetic with the CPU test through open_order_rows.hpp."""
    import json

    src = open(os.path.join(ROOT, "bourse_amd", "csrc", "open_orders.hpp")).read()
    body = src[src.index("namespace bkd {"):]
    assert re.search(r"namespace bkd \{\s*namespace open_orders \{", body)
    assert re.search(r"__global__[^;{]*\bk_refresh\(", body)
    code = re.sub(r"//.*", "", src)
    assert "asm" not in code and "atomic" not in code and "__shared__" not in code and "__shfl" not in code
    assert '#include "open_order_rows.hpp"' in src
    for f in ("add_order(", "empty_summary(", "empty_entry(", "pack_entry(", "summary_words("):
        assert f in code, f
    rows = open(os.path.join(ROOT, "bourse_amd", "csrc", "open_order_rows.hpp")).read()
    assert re.search(r"namespace bkd \{\s*namespace open_orders \{", rows)
    assert "hip_runtime" not in rows and "asm" not in re.sub(r"//.*", "", rows)
    base = json.load(open(os.path.join(ROOT, "profiles", "kernel_isa_baseline.json")))["kernels"]
    assert not [k for k in base if "open_orders" in k or "k_refresh" in k]
