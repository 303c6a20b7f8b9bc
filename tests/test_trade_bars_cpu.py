"""Per-step trade bars (bk_trade_bars_enable) without a GPU: the plain-Python model against bars worked out by hand, the
kernel's per-record arithmetic and its combination of partial bars (bourse_amd/csrc/trade_bar_fold.hpp, compiled with g++)
against the model, the C ABI - the entries are exported, bound and declared, refuse a null env, and bk_trade_bar is 48 bytes
laid out as TRADE_BAR_DTYPE - and the layout of the kernel's source."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import trade_bars_model as TM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("bk_trade_bars_enable", "bk_trade_bars_device_ptr", "bk_trade_bars_slot", "bk_get_trade_bars", "bk_trade_bars_clear",
           "bk_trade_bars_clear_device")
BK_INVALID_ARGUMENT = 5
M64 = (1 << 64) - 1
MAXU = 0xFFFFFFFF

TRADE = np.dtype([("side", "<u4"), ("price", "<u4"), ("vol", "<u4")])


def _trades(records):
    """records (side_is_bid, price, vol) as the model's array"""
    return np.array(records, dtype=TRADE)


def _rows(ring):
    return [tuple(int(x) for x in r) for r in ring]


def test_the_model_against_bars_worked_out_by_hand():
    trades = _trades([
        (0, 100, 4),                               # step 0: the aggressor buys 4 at 100
        (0, 100, 6), (1, 105, 3), (0, 101, 2),     # step 1: open 100, high 105, close 101; 8 bought, 3 sold
                                                   # step 2: nothing - the close of step 1 is carried
        (1, 90, 3),                                # step 3: 3 sold at 90
    ])                                             # step 4: nothing
    counts = [1, 3, 0, 1, 0]
    idle = lambda p: (p, p, p, p, 0, 0, 0, 0, 0)
    ring = TM.fold(trades, counts[:3], 3)
    assert ring.dtype == TM.TRADE_BAR_DTYPE and ring.shape == (3,)
    assert _rows(ring) == [(100, 100, 100, 100, 4, 0, 400, 1, 0), (100, 105, 100, 101, 8, 3, 600 + 315 + 202, 2, 1), idle(101)]
    # a window of 3 wraps: step 3 takes slot 0, step 4 slot 1 with step 3's close; slot 2 still holds step 2
    assert _rows(TM.fold(trades, counts, 3)) == [(90, 90, 90, 90, 0, 3, 270, 0, 1), idle(90), idle(101)]
    # a window of 1: the carried close is the slot's own, read before the write
    assert _rows(TM.fold(trades, counts[:3], 1)) == [idle(101)]
    assert _rows(TM.fold(trades, counts[:4], 1)) == [(90, 90, 90, 90, 0, 3, 270, 0, 1)]
    assert _rows(TM.fold(trades, counts, 1)) == [idle(90)]
    # before the first trade the carried price is 0; first / first_step start later in the records and in the ring
    assert _rows(TM.fold(trades, [0, 0], 2)) == [idle(0), idle(0)]
    assert _rows(TM.fold(trades, [1, 0], 2, first_step=3, first=4)) == [idle(90), (90, 90, 90, 90, 0, 3, 270, 0, 1)]
    # the notional wraps modulo 2**64 and a volume sum passes 2**32: three records of the largest price and volume
    big = _trades([(0, MAXU, MAXU)] * 3 + [(1, MAXU, MAXU)] * 2)
    (r,) = TM.fold(big, [5], 1)
    assert 5 * MAXU * MAXU > M64 and 3 * MAXU > MAXU
    assert int(r["notional"]) == (5 * 0xFFFFFFFE00000001) & M64
    assert int(r["buy_vol"]) == 3 * MAXU and int(r["sell_vol"]) == 2 * MAXU and (int(r["n_buy"]), int(r["n_sell"])) == (3, 2)
    assert (int(r["open"]), int(r["high"]), int(r["low"]), int(r["close"])) == (MAXU,) * 4


def _edge_records():
    out = []
    for side in (0, 1):
        out += [(side, MAXU, MAXU), (side, 123, 0), (side, 0, 77), (side, 0, 0), (side, MAXU, 1), (side, 1, MAXU),
                (side, 2_000_000_000, 3_000_000_000)]
    return out


def _write_case(tmp_path, steps, cuts, want):
    with open(tmp_path / "records.txt", "w") as f:
        f.write(f"{len(steps)}\n")
        for recs, c in zip(steps, cuts):
            f.write(" ".join(str(x) for x in [len(recs), len(c)] + list(c)) + "\n")
            for side, price, vol in recs:
                f.write(f"{side} {price} {vol}\n")
    with open(tmp_path / "expected.txt", "w") as f:
        for row in want:
            f.write(" ".join(str(int(x)) for x in row) + "\n")


def test_trade_bar_fold_hpp_equals_the_model(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path / "trade_bar_fold_test")
    res = subprocess.run([gxx, "-std=c++17", "-O2", os.path.join(ROOT, "tests", "cpp", "trade_bar_fold_test.cpp"), "-o", exe],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    rng = np.random.default_rng(5)
    steps = []
    for s in range(60):  # a few thousand random records in steps of 0..200, every third step idle
        n = 0 if s % 3 == 2 else int(rng.integers(1, 201))
        wide = s % 2 == 0  # full-range words, or a narrow band where high / low / open / close differ by little
        steps.append([(int(rng.integers(0, 2)), int(rng.integers(0, 1 << 32)) if wide else int(rng.integers(990, 1010)),
                       int(rng.integers(0, 1 << 32)) if wide else int(rng.integers(1, 50))) for _ in range(n)])
    steps += [_edge_records(), [], [(1, MAXU, MAXU)] * 9, [(0, MAXU, MAXU)] * 70_000]
    cuts = [sorted(set(int(c) for c in rng.integers(1, len(r), size=int(rng.integers(0, 9))))) if len(r) > 1 else [] for r in steps]
    cuts[-1] = [64, 128, 65_536]
    flat = _trades([r for recs in steps for r in recs])
    want = TM.fold(flat, [len(r) for r in steps], len(steps))  # (the window holds every step: one row per step)
    assert len(flat) > 4000 and sum(len(c) for c in cuts) > 100
    assert int(want[-1]["buy_vol"]) == 70_000 * MAXU > 1 << 48 and 9 * MAXU * MAXU > M64, "no word wraps: the case checks less than it says"
    assert any(len(r) == 0 and int(w["close"]) != 0 for r, w in zip(steps, want)), "no idle step carries a close"
    _write_case(tmp_path, steps, cuts, want)
    run = subprocess.run([exe, str(tmp_path / "records.txt"), str(tmp_path / "expected.txt")], capture_output=True, text=True,
                         timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    n_partials = sum(len(c) + 1 for r, c in zip(steps, cuts) if r)
    assert run.stdout.strip().endswith(f"trade_bar_fold ok {len(steps)} steps {len(flat)} records {n_partials} partial bars")
    # a wrong expectation is really caught: one word off by one
    want[7]["notional"] += 1
    _write_case(tmp_path, steps, cuts, want)
    run = subprocess.run([exe, str(tmp_path / "records.txt"), str(tmp_path / "expected.txt")], capture_output=True, text=True,
                         timeout=120)
    assert run.returncode == 1 and "step 7 " in run.stdout


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
    # the bars add no flag bit of their own (the set of bits is pinned by the open-order, queue and quote tests): a record
    # dropped beyond trade_capacity is left out of its bar, and its book carries TRADE_OVERFLOW, a capacity flag, already
    taken = [int(v) for v in re.findall(r"#define BK_FLAG_\w+ (\d+)u", header)]
    assert len(taken) == len(set(taken)) and sorted(taken) == sorted(_lib.FLAG_NAMES), taken
    assert "BARS" not in " ".join(re.findall(r"#define (BK_FLAG_\w+)", header))
    assert _lib.CAPACITY_FLAGS & _lib.FLAG_TRADE_OVERFLOW and "TRADE_OVERFLOW" in _lib.FLAG_NAMES[_lib.FLAG_TRADE_OVERFLOW]
    methods = ("enable_trade_bars", "trade_bars", "trade_bars_device_ptr", "trade_bars_view", "trade_bars_slot", "clear_trade_bars")
    for method in methods:
        assert callable(getattr(bourse_amd.ManyBookEnv, method)), method
        assert getattr(bourse_amd.ManyMarketEnv, method) is getattr(bourse_amd.ManyBookEnv, method), method
    assert bourse_amd.ManyBookEnv.TRADE_BAR_DTYPE is _lib.TRADE_BAR_DTYPE is bourse_amd.TRADE_BAR_DTYPE
    hpp = open(os.path.join(ROOT, "include", "bourse_amd.hpp")).read()
    for method in ("enable_trade_bars", "trade_bars", "trade_bars_device_ptr", "trade_bars_slot", "clear_trade_bars"):
        assert re.search(r"\b" + method + r"\(", hpp), method
    rs = open(os.path.join(ROOT, "integration", "rust", "bourse_amd_sys.rs")).read()
    for name in ENTRIES:
        assert re.search(r"pub fn " + name + r"\(", rs), name
    assert "pub struct BkTradeBar" in rs and "pub open: u32" in rs and "pub notional: u64" in rs and "pub n_sell: u32" in rs


def test_bk_trade_bar_is_48_bytes_laid_out_as_the_dtype(tmp_path):
    from bourse_amd import _lib

    dt = _lib.TRADE_BAR_DTYPE
    names = ("open", "high", "low", "close", "buy_vol", "sell_vol", "notional", "n_buy", "n_sell")
    assert dt.itemsize == 48 and dt.names == names
    assert [dt.fields[n][1] for n in names] == [0, 4, 8, 12, 16, 24, 32, 40, 44]
    assert [dt.fields[n][0].str for n in names] == ["<u4"] * 4 + ["<u8"] * 3 + ["<u4"] * 2
    assert dt == TM.TRADE_BAR_DTYPE
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    src = tmp_path / "layout.cpp"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "bourse_amd.h"\n'
                   'int main() { std::printf("%zu", sizeof(bk_trade_bar));\n' +
                   "".join(f'std::printf(" %zu", offsetof(bk_trade_bar, {n}));\n' for n in names) + 'return 0; }\n')
    exe = str(tmp_path / "layout")
    res = subprocess.run([gxx, "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60).stdout.split()
    assert [int(x) for x in out] == [48, 0, 4, 8, 12, 16, 24, 32, 40, 44]


def test_a_null_env_is_refused_not_dereferenced():
    from bourse_amd import _lib

    L = _lib.load()
    mask = (ctypes.c_uint8 * 4)(1, 0, 1, 0)
    out = ctypes.c_void_p()
    slot = ctypes.c_uint32()
    rows = np.zeros(4, dtype=_lib.TRADE_BAR_DTYPE)
    calls = {
        "bk_trade_bars_enable": lambda: L.bk_trade_bars_enable(None, 4, 0),
        "bk_trade_bars_device_ptr": lambda: L.bk_trade_bars_device_ptr(None, ctypes.byref(out)),
        "bk_trade_bars_slot": lambda: L.bk_trade_bars_slot(None, ctypes.byref(slot)),
        "bk_get_trade_bars": lambda: L.bk_get_trade_bars(None, 0, 1, rows.ctypes.data_as(ctypes.c_void_p)),
        "bk_trade_bars_clear": lambda: L.bk_trade_bars_clear(None, ctypes.cast(mask, ctypes.c_void_p)),
        "bk_trade_bars_clear_device": lambda: L.bk_trade_bars_clear_device(None, ctypes.cast(mask, ctypes.c_void_p)),
    }
    assert set(calls) == set(ENTRIES)
    for name, call in calls.items():
        L.bk_device_count(ctypes.byref(ctypes.c_int(0)))  # (anything that may leave another message behind)
        assert call() == BK_INVALID_ARGUMENT, name
        assert b"null env" in L.bk_last_error(), name


def test_the_kernels_stay_out_of_the_baselined_namespace_and_hold_no_assembly():
    """bkd::trade_bars kernels are not among the names tools/kernel_isa_counts.py::measure lists (those start with k_ once
    "void bkd::" is stripped), so profiles/kernel_isa_baseline.json stays as it is; the fold is plain C++ and shares its
    per-record arithmetic and its combination of partial bars with the CPU test through trade_bar_fold.hpp."""
    src = open(os.path.join(ROOT, "bourse_amd", "csrc", "trade_bars.hpp")).read()
    body = src[src.index("namespace bkd {"):]
    assert re.search(r"namespace bkd \{\s*namespace trade_bars \{", body)
    for k in ("k_fold", "k_clear"):
        assert re.search(r"__global__[^;{]*\b" + k + r"\(", body), k
    code = re.sub(r"//.*", "", src)
    assert "asm" not in code and "atomic" not in code and "__shared__" not in code
    assert '#include "trade_bar_fold.hpp"' in src
    for f in ("is_buy(", "notional(", "extend(", "idle(", "words("):
        assert f in code, f
    fold = open(os.path.join(ROOT, "bourse_amd", "csrc", "trade_bar_fold.hpp")).read()
    assert re.search(r"namespace bkd \{\s*namespace trade_bars \{", fold)
    assert "hip_runtime" not in fold and "asm" not in re.sub(r"//.*", "", fold)
    # one guard in front of every new launch of the step and of the reset
    hip = open(os.path.join(ROOT, "bourse_amd", "csrc", "bourse_amd.hip")).read()
    for launch in ("launch_bars_fold(env);", "launch_bars_clear(env, mask_dev, env->M);"):
        at = hip.index(launch)
        assert re.search(r"if \(env->bars_window\) \{[^\n]*\n\s*$", hip[:at]), launch
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_isa_counts as K
    import json

    base = json.load(open(K.BASELINE))["kernels"]
    assert not [k for k in base if "trade_bars" in k or "k_fold" in k]
