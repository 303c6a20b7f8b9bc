"""Per-book series moments (bk_series_enable) without a GPU: the plain-Python model against rows worked out by hand, the
kernel's per-record arithmetic, carry and combination of partial rows (bourse_amd/csrc/series_fold.hpp, compiled with g++)
against the model over every split, the C ABI - the entries are exported, bound and declared, refuse a null env, and
bk_series_row is 192 bytes laid out as SERIES_DTYPE - the layout of the kernel's source, and series_moments against numpy."""
import ctypes
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import series_model as SM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("bk_series_enable", "bk_series_fold", "bk_series_clear", "bk_series_clear_device", "bk_series_device_ptr", "bk_get_series")
BK_INVALID_ARGUMENT = 5
M64 = (1 << 64) - 1
MAXU = 0xFFFFFFFF


def _hist(records):
    """records (trade_vol, bid, ask, ask_vol, bid_vol) as an [n_steps, 5] history"""
    return np.array(records, dtype=np.uint64).reshape(-1, 5)


def _named(s):
    return dict(zip(SM.FIELDS, SM.words(s)))


def test_the_model_against_rows_worked_out_by_hand():
    # a one-sided step in the middle breaks the chain: returns on both sides of it, no pair across it
    h = _hist([(0, 100, 104, 5, 7),    # m 204, spread 4
               (3, 101, 105, 5, 7),    # m 206: d +2
               (0, 0, 105, 5, 0),      # no bid: the chain breaks
               (2, 99, 103, 1, 1),     # m 202: two-sided again, no return
               (0, 98, 102, 1, 1),     # m 200: d -2, but no d before it: no pair
               (0, 100, 102, 1, 1)])   # m 202: d +2, pair (+2)(-2)
    w = _named(SM.fold(h))
    assert w == dict(
        n_steps=6, n_two_sided=5, sum_m=204 + 206 + 202 + 200 + 202, sum_spread=18, sum_spread_sq=4 * 16 + 4, sum_bid_vol=17,
        sum_ask_vol=18, sum_trade_vol=5, sum_trade_vol_sq=13, n_trade_steps=2, n_ret=3, sum_d=2, sum_abs_d=6, sum_d2=12,
        sum_d4_lo=48, sum_d4_hi=0, max_abs_d=2, n_pairs=1, sum_dd=(-4) & M64, sum_abs_dd=4, min_m=200, max_m=206,
        carry_m=(3 << 62) | 202, carry_d=2)
    r = SM.row(SM.fold(h))
    assert r.dtype == SM.SERIES_DTYPE and int(r["sum_dd"]) == -4 and int(r["sum_d"]) == 2
    # the same in two folds, split anywhere - also right behind the one-sided step - is the same row
    for y in range(1, 6):
        s = SM.fold(h[:y])
        assert SM.words(SM.fold(h[y:], first_step=y, into=s)) == SM.words(SM.fold(h)), y
    # a cut in front of step 5 (a reset there): step 5 has no return, so n_ret 2, no pair, and the carry holds m only
    w = _named(SM.fold(h, cuts=[5]))
    assert (w["n_ret"], w["n_pairs"], w["sum_d"], w["sum_dd"], w["carry_m"], w["carry_d"]) == (2, 0, 0, 0, (1 << 63) | 202, 0)
    assert w["n_two_sided"] == 5 and w["sum_m"] == 1014  # (the sums go on)
    # a single two-sided step: no return; a cleared row; a series that ends one-sided carries nothing
    w = _named(SM.fold(_hist([(0, 5, 9, 1, 1)])))
    assert (w["n_two_sided"], w["n_ret"], w["min_m"], w["max_m"], w["carry_m"], w["carry_d"]) == (1, 0, 14, 14, (1 << 63) | 14, 0)
    assert SM.words(SM.cleared()) == [M64 if n == "min_m" else 0 for n in SM.FIELDS]
    w = _named(SM.fold(_hist([(0, 5, 9, 1, 1), (0, 6, 9, 1, 1), (0, 6, MAXU, 0, 1)])))
    assert (w["n_ret"], w["sum_d"], w["carry_m"], w["carry_d"], w["min_m"]) == (1, 1, 0, 0, 14)
    # d of both signs, three in a row: two pairs
    w = _named(SM.fold(_hist([(0, 10, 20, 1, 1), (0, 13, 20, 1, 1), (0, 9, 20, 1, 1), (0, 9, 22, 1, 1)])))
    assert (w["n_ret"], w["sum_d"], w["sum_abs_d"], w["sum_d2"], w["sum_d4_lo"]) == (3, 1, 9, 9 + 16 + 4, 81 + 256 + 16)
    assert (w["n_pairs"], w["sum_dd"], w["sum_abs_dd"], w["max_abs_d"], w["carry_d"]) == (2, (-12 - 8) & M64, 12 + 8, 4, 2)
    # tv * tv and sum_d2 wrap 2**64; the jump from (1, 2) to (0xFFFFFFFD, 0xFFFFFFFE) has a = 2**33 - 8, whose a * a needs 66
    # bits and whose fourth power the modulo-2**128 rule
    h = _hist([(MAXU, 1, 2, MAXU, MAXU), (MAXU, 0xFFFFFFFD, 0xFFFFFFFE, MAXU, MAXU), (1, 1, 2, 0, 0)])
    w = _named(SM.fold(h))
    a = (1 << 33) - 8
    assert a * a > M64 and a ** 4 > (1 << 128) and 2 * MAXU * MAXU > M64
    assert w["sum_trade_vol_sq"] == (2 * MAXU * MAXU + 1) & M64 == 0xFFFFFFFC00000003
    assert (w["n_ret"], w["sum_d"], w["sum_abs_d"], w["max_abs_d"]) == (2, 0, 2 * a, a)
    assert w["sum_d2"] == (2 * a * a) & M64 == 0xFFFFFFC000000080
    assert (w["sum_d4_lo"], w["sum_d4_hi"]) == ((2 * a ** 4) & M64, ((2 * a ** 4) >> 64) & M64) and w["sum_d4_hi"] != 0
    assert (w["n_pairs"], w["sum_dd"], w["sum_abs_dd"]) == (1, (-a * a) & M64, (a * a) & M64)
    assert (w["min_m"], w["max_m"], w["carry_m"], w["carry_d"]) == (3, (1 << 33) - 5, (3 << 62) | 3, (-a) & M64)
    assert w["sum_spread"] == 3 and w["sum_bid_vol"] == 2 * MAXU


def _edge_series(rng):
    """extremes of every word: the largest prices and volumes, the widest spread, the largest jumps, empty sides"""
    out = [(MAXU, 1, 2, MAXU, MAXU), (MAXU, 0xFFFFFFFD, 0xFFFFFFFE, MAXU, MAXU), (MAXU, 1, 2, MAXU, MAXU),
           (0, 1, 0xFFFFFFFE, 0, 0), (0, 0xFFFFFFFE, 0xFFFFFFFE, 1, 1), (0, 0, MAXU, 0, 0), (5, 0, 7, 3, 0), (5, 7, MAXU, 0, 3),
           (0, MAXU, 0, 1, 1), (0, 1, 2, 1, 1), (0, 0xFFFFFFFD, 0xFFFFFFFE, 1, 1), (0, 1, 2, 1, 1), (0, 0xFFFFFFFD, 0xFFFFFFFE, 1, 1)]
    for _ in range(400):  # jumps between the two ends of the price range, so that the 128-bit sum carries many times
        lo = rng.integers(0, 2)
        out.append((int(rng.integers(0, 1 << 32)), 1 if lo else 0xFFFFFFFD, int(rng.integers(2, 9)) if lo else 0xFFFFFFFE,
                    int(rng.integers(0, 1 << 32)), int(rng.integers(0, 1 << 32))))
    return out


def _random_series(rng, n, wide):
    out = []
    for _ in range(n):
        one_sided = rng.random() < 0.1
        if wide:
            bid, ask = int(rng.integers(1, 1 << 32)), int(rng.integers(0, MAXU))
        else:
            bid = int(rng.integers(990, 1010))
            ask = bid + int(rng.integers(1, 6))
        if one_sided:
            if rng.random() < 0.5:
                bid = 0
            else:
                ask = MAXU
        vol = (lambda: int(rng.integers(0, 1 << 32))) if wide else (lambda: int(rng.integers(0, 50)))
        out.append((vol() if rng.random() < 0.5 else 0, bid, ask, vol(), vol()))
    return out


def _write_case(tmp_path, series, ends, want):
    with open(tmp_path / "records.txt", "w") as f:
        f.write(f"{len(series)}\n")
        for recs, e in zip(series, ends):
            f.write(" ".join(str(x) for x in [len(recs), len(e)] + list(e)) + "\n")
            for r in recs:
                f.write(" ".join(str(x) for x in r) + "\n")
    with open(tmp_path / "expected.txt", "w") as f:
        for per_series in want:
            for w in per_series:
                f.write(" ".join(str(x) for x in w) + "\n")


def test_series_fold_hpp_equals_the_model_over_every_split(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path / "series_fold_test")
    res = subprocess.run([gxx, "-std=c++17", "-O2", os.path.join(ROOT, "tests", "cpp", "series_fold_test.cpp"), "-o", exe],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    rng = np.random.default_rng(11)
    series = [_edge_series(rng), [(0, 5, 9, 1, 1)], [(1, 0, MAXU, 0, 0)]]
    series += [_random_series(rng, int(rng.integers(2, 1500)), wide=k % 2 == 0) for k in range(40)]
    ends = []
    for k, recs in enumerate(series):
        n = len(recs)
        if k == 0:
            e = list(range(1, n + 1))  # every fold a single step
        elif k % 3 == 0:
            e = [n]                    # one fold
        else:
            e = sorted(set(int(x) for x in rng.integers(1, n + 1, size=int(rng.integers(1, 12)))) | {n})
            if n > 4:
                e = sorted(set(e) | {1, 2})  # single-step folds at the front too
        ends.append(e)
    want = []
    n_one_sided = n_steps = 0
    for recs, e in zip(series, ends):
        h = _hist(recs)
        n_steps += len(h)
        n_one_sided += int(np.sum((h[:, 1] == 0) | (h[:, 2] == MAXU)))
        s, lo, per = SM.cleared(), 0, []
        for y in e:
            s = SM.fold(h[lo:y], first_step=lo, into=s)
            per.append(SM.words(s))
            lo = y
        assert per[-1] == SM.words(SM.fold(h))  # (the model itself is split-invariant)
        want.append(per)
    assert n_steps > 20_000 and 0.05 < n_one_sided / n_steps < 0.2
    last = dict(zip(SM.FIELDS, want[0][-1]))
    assert last["sum_d4_hi"] != 0 and last["max_abs_d"] == (1 << 33) - 8, "no word wraps: the case checks less than it says"
    assert any(len(e) > 2 and e[0] == 1 for e in ends) and any(len(r) > 64 * 3 and len(e) == 1 for r, e in zip(series, ends))
    _write_case(tmp_path, series, ends, want)
    run = subprocess.run([exe, str(tmp_path / "records.txt"), str(tmp_path / "expected.txt")], capture_output=True, text=True,
                         timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip().endswith(f"series_fold ok {len(series)} series {n_steps} steps {sum(len(e) for e in ends)} folds")
    # a wrong expectation is really caught: one word off by one
    want[7][0][SM.FIELDS.index("sum_abs_dd")] += 1
    _write_case(tmp_path, series, ends, want)
    run = subprocess.run([exe, str(tmp_path / "records.txt"), str(tmp_path / "expected.txt")], capture_output=True, text=True,
                         timeout=120)
    assert run.returncode == 1 and "series 7 fold 0 " in run.stdout and f"word {SM.FIELDS.index('sum_abs_dd')} " in run.stdout


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
    # a lost step refuses the fold: no flag bit is added (the set of bits is pinned by the open-order, queue and quote tests)
    taken = [int(v) for v in re.findall(r"#define BK_FLAG_\w+ (\d+)u", header)]
    assert len(taken) == len(set(taken)) and sorted(taken) == sorted(_lib.FLAG_NAMES) == [1 << i for i in range(10)], taken
    assert "SERIES" not in " ".join(re.findall(r"#define (BK_FLAG_\w+)", header))
    methods = ("enable_series", "fold_series", "series", "series_device_ptr", "series_view", "clear_series", "run_series")
    for method in methods:
        assert callable(getattr(bourse_amd.ManyBookEnv, method)), method
        assert getattr(bourse_amd.ManyMarketEnv, method) is getattr(bourse_amd.ManyBookEnv, method), method
    assert bourse_amd.ManyBookEnv.SERIES_DTYPE is _lib.SERIES_DTYPE is bourse_amd.SERIES_DTYPE
    assert bourse_amd.series_moments is _lib.series_moments
    hpp = open(os.path.join(ROOT, "include", "bourse_amd.hpp")).read()
    for method in ("enable_series", "fold_series", "series", "series_device_ptr", "clear_series"):
        assert re.search(r"\b" + method + r"\(", hpp), method
    # the Rust FFI file is the generator's output for this header: every entry, and the row field by field
    rs = open(os.path.join(ROOT, "integration", "rust", "bourse_amd_sys.rs")).read()
    for name in ENTRIES:
        assert re.search(r"pub fn " + name + r"\(", rs), name
    body = re.search(r"pub struct BkSeriesRow \{(.*?)\}", rs, flags=re.S).group(1)
    assert re.findall(r"pub (\w+): (\w+),", body) == [(n, "i64" if n in SM.SIGNED else "u64") for n in SM.FIELDS]


def test_bk_series_row_is_192_bytes_laid_out_as_the_dtype(tmp_path):
    from bourse_amd import _lib

    dt = _lib.SERIES_DTYPE
    assert dt.itemsize == 192 and dt.names == SM.FIELDS == _lib.SERIES_FIELDS
    assert [dt.fields[n][1] for n in dt.names] == [8 * i for i in range(24)]
    assert [dt.fields[n][0].str for n in dt.names] == ["<i8" if n in ("sum_d", "sum_dd", "carry_d") else "<u8" for n in dt.names]
    assert dt == SM.SERIES_DTYPE
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    src = tmp_path / "layout.cpp"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "bourse_amd.h"\n'
                   'int main() { std::printf("%zu", sizeof(bk_series_row));\n' +
                   "".join(f'std::printf(" %zu", offsetof(bk_series_row, {n}));\n' for n in dt.names) + 'return 0; }\n')
    exe = str(tmp_path / "layout")
    res = subprocess.run([gxx, "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60).stdout.split()
    assert [int(x) for x in out] == [192] + [8 * i for i in range(24)]


def test_a_null_env_is_refused_not_dereferenced():
    from bourse_amd import _lib

    L = _lib.load()
    mask = (ctypes.c_uint8 * 4)(1, 0, 1, 0)
    out = ctypes.c_void_p()
    rows = np.zeros(4, dtype=_lib.SERIES_DTYPE)
    calls = {
        "bk_series_enable": lambda: L.bk_series_enable(None),
        "bk_series_fold": lambda: L.bk_series_fold(None),
        "bk_series_clear": lambda: L.bk_series_clear(None, ctypes.cast(mask, ctypes.c_void_p)),
        "bk_series_clear_device": lambda: L.bk_series_clear_device(None, ctypes.cast(mask, ctypes.c_void_p)),
        "bk_series_device_ptr": lambda: L.bk_series_device_ptr(None, ctypes.byref(out)),
        "bk_get_series": lambda: L.bk_get_series(None, 0, 1, rows.ctypes.data_as(ctypes.c_void_p)),
    }
    assert set(calls) == set(ENTRIES)
    for name, call in calls.items():
        L.bk_device_count(ctypes.byref(ctypes.c_int(0)))  # (anything that may leave another message behind)
        assert call() == BK_INVALID_ARGUMENT, name
        assert b"null env" in L.bk_last_error(), name


def test_the_kernels_stay_out_of_the_baselined_namespace_and_every_launch_sits_behind_the_guard():
    """bkd::series kernels are not among the names tools/kernel_isa_counts.py::measure lists (those start with k_ once
    "void bkd::" is stripped), so profiles/kernel_isa_baseline.json stays as it is; the fold is plain C++ and shares its
    per-record arithmetic, its carry and its row with the CPU test through series_fold.hpp."""
    src = open(os.path.join(ROOT, "bourse_amd", "csrc", "series.hpp")).read()
    body = src[src.index("namespace bkd {"):]
    assert re.search(r"namespace bkd \{\s*namespace series \{", body)
    for k in ("k_fold", "k_clear"):
        assert re.search(r"__global__[^;{]*\b" + k + r"\(", body), k
    code = re.sub(r"//.*", "", src)
    assert "asm" not in code and "atomic" not in code and "__shared__" not in code
    assert '#include "series_fold.hpp"' in src
    for f in ("term(", "next(", "prev_of(", "quotes_only(", "add(", "merge(", "pack(", "unpack(", "cleared("):
        assert f in code, f
    fold = open(os.path.join(ROOT, "bourse_amd", "csrc", "series_fold.hpp")).read()
    assert re.search(r"namespace bkd \{\s*namespace series \{", fold)
    assert "hip_runtime" not in fold and "asm" not in re.sub(r"//.*", "", fold)
    # (where bourse_amd.hip launches them, and behind which guard: tests/test_hist_tables_cpu.py)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_isa_counts as K

    base = json.load(open(K.BASELINE))["kernels"]
    assert not [k for k in base if "series" in k or "k_fold" in k]


def test_series_moments_against_numpy_on_the_raw_history():
    from bourse_amd import _lib, series_moments

    rng = np.random.default_rng(3)
    recs = np.array(_random_series(rng, 500, wide=False), dtype=np.uint64)
    r = np.array([SM.row(SM.fold(recs))], dtype=_lib.SERIES_DTYPE)
    got = series_moments(r)[0]
    tv, bid, ask, av, bv = (recs[:, i].astype(np.float64) for i in range(5))
    two = (recs[:, 1] != 0) & (recs[:, 2] != MAXU)
    m = bid + ask
    ret = two[1:] & two[:-1]
    d = (m[1:] - m[:-1])[ret]
    pair = ret[1:] & ret[:-1]
    dd = ((m[2:] - m[1:-1]) * (m[1:-1] - m[:-2]))[pair]
    add = np.abs(dd)
    want = dict(
        mean_mid=np.mean(m[two]) / 2, mean_spread=np.mean((ask - bid)[two]), var_spread=np.var((ask - bid)[two]),
        mean_return=np.mean(d) / 2, var_return=np.var(d / 2), kurtosis_return=len(d) * np.sum(d ** 4) / np.sum(d ** 2) ** 2 - 3,
        acf1_return=(np.mean(dd) - np.mean(d) ** 2) / np.var(d),
        acf1_abs_return=(np.mean(add) - np.mean(np.abs(d)) ** 2) / np.var(np.abs(d)),
        mean_trade_vol=np.mean(tv), mean_bid_vol=np.mean(bv), mean_ask_vol=np.mean(av))
    assert len(d) > 300 and len(dd) > 200 and not two.all()
    for k, v in want.items():
        assert abs(got[k] - v) <= 1e-12 * abs(v), (k, got[k], v)
    # a zero count gives NaN, not an error: a cleared row, and a row of one two-sided step
    none = series_moments(np.array([SM.row(SM.cleared())], dtype=_lib.SERIES_DTYPE))[0]
    assert all(np.isnan(none[k]) for k in none.dtype.names)
    one = series_moments(np.array([SM.row(SM.fold(_hist([(4, 5, 9, 1, 2)])))], dtype=_lib.SERIES_DTYPE))[0]
    assert (one["mean_mid"], one["mean_spread"], one["var_spread"], one["mean_trade_vol"]) == (7.0, 4.0, 0.0, 4.0)
    assert all(np.isnan(one[k]) for k in ("mean_return", "var_return", "kurtosis_return", "acf1_return", "acf1_abs_return"))
    with pytest.raises(ValueError):
        series_moments(np.zeros(2, dtype=np.uint64))
