"""The per-book lag table (bk_lags_enable) without a GPU: the plain-Python model against rows worked out by hand, the
kernel's per-term arithmetic, window and carry (bourse_amd/csrc/lag_fold.hpp, compiled with g++ into a program of its own)
against the model over random splits, row 0 against the series' model, the C ABI - the entries are exported, bound and
declared, refuse a null env, and bk_lag_row is 80 bytes laid out as LAG_DTYPE - the layout of the kernel's source, and
lag_moments against numpy."""
import ctypes
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import lags_model as LM
import series_model as SM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("bk_lags_enable", "bk_lags_fold", "bk_lags_clear", "bk_lags_clear_device", "bk_lags_device_ptr", "bk_get_lags")
BK_INVALID_ARGUMENT = 5
M64 = (1 << 64) - 1
M128 = (1 << 128) - 1
MAXU = 0xFFFFFFFF
TWO = 1 << 63


def _cxx():
    """a host C++ compiler: g++, else any other on the path, else hipcc's (a .cpp file is plain C++ to it).  The header's
    word-for-word check must not drop out where a tool is missing, so having none is a failure, not a skip."""
    for name in ("g++", "c++", "clang++"):
        if shutil.which(name):
            return shutil.which(name)
    from bourse_amd import _build

    try:
        return _build.hipcc_path()
    except RuntimeError:
        pytest.fail("no host C++ compiler (g++, c++, clang++ or hipcc): lag_fold.hpp cannot be checked")


def _hist(quotes):
    """(bid, ask) per step as an [n_steps, 5] history: only words 1 and 2 are read"""
    h = np.zeros((len(quotes), 5), dtype=np.uint64)
    h[:, 1:3] = np.array(quotes, dtype=np.uint64).reshape(-1, 2)
    return h


def _row(n_pairs, sum_dd, sum_abs_dd, n_h, sum_h, sum_abs_h, sum_h2, sum_h4, max_abs_h):
    return [n_pairs, sum_dd & M64, sum_abs_dd & M64, n_h, sum_h & M64, sum_abs_h & M64, sum_h2 & M64, sum_h4 & M64,
            (sum_h4 & M128) >> 64, max_abs_h]


HAND = [(0, MAXU), (100, MAXU), (100, 104), (102, 104), (100, 104), (100, 104)]  # steps 2..5: m = 204, 206, 204, 204


def test_the_model_against_rows_worked_out_by_hand():
    # d = +2, -2, 0 at steps 3, 4, 5.  lag 1: (-2)(+2), (0)(-2).  span 2: 204 - 204, 204 - 206; lag 2: (0)(+2).  span 3: 204 - 204
    s = LM.fold(_hist(HAND), 3)
    assert LM.words(s) == [_row(2, -4, 4, 3, 0, 4, 8, 32, 2), _row(1, 0, 0, 2, -2, 2, 4, 16, 2), _row(0, 0, 0, 1, 0, 0, 0, 0, 0)]
    assert LM.carry(s) == [TWO | 204, TWO | 204, TWO | 206, TWO | 204]
    t = LM.table(s)
    assert t.dtype == LM.LAG_DTYPE and t.shape == (3,) and int(t[0]["sum_dd"]) == -4 and int(t[1]["sum_h"]) == -2
    # the same in two folds, split anywhere, is the same rows and carry
    for y in range(1, 6):
        part = LM.fold(_hist(HAND)[y:], first_step=y, into=LM.fold(_hist(HAND)[:y], 3))
        assert (LM.words(part), LM.carry(part)) == (LM.words(s), LM.carry(s)), y
    # a cut in front of step 4 (a reset there): step 4 has no past, step 5 a return of 0 and nothing to pair it with
    c = LM.fold(_hist(HAND), 3, cuts=[4])
    assert LM.words(c) == [_row(0, 0, 0, 2, 2, 2, 4, 16, 2), _row(0, 0, 0, 0, 0, 0, 0, 0, 0), _row(0, 0, 0, 0, 0, 0, 0, 0, 0)]
    assert LM.carry(c) == [TWO | 204, TWO | 204, 0, 0]
    # a one-sided step in the middle: span 2 reaches over it (only the end points count), no return touches it
    g = LM.fold(_hist([(10, 20), (0, 20), (12, 22)]), 2)
    assert LM.words(g) == [_row(0, 0, 0, 0, 0, 0, 0, 0, 0), _row(0, 0, 0, 1, 4, 4, 16, 256, 4)]
    assert LM.carry(g) == [TWO | 34, 0, TWO | 30]
    assert LM.words(LM.cleared(2)) == [[0] * 10, [0] * 10] and LM.carry(LM.cleared(2)) == [0, 0, 0]
    # the jump from (1, 2) to (0xFFFFFFFD, 0xFFFFFFFE) and back: a = 2**33 - 8, a * a needs 66 bits, a**4 the modulo-2**128
    # rule, and the one product of returns is negative
    a = (1 << 33) - 8
    assert a * a > M64 and 2 * a ** 4 > M128
    j = LM.fold(_hist([(1, 2), (0xFFFFFFFD, 0xFFFFFFFE), (1, 2)]), 2)
    assert LM.words(j) == [_row(1, -a * a, a * a, 2, 0, 2 * a, 2 * a * a, 2 * a ** 4, a), _row(0, 0, 0, 1, 0, 0, 0, 0, 0)]
    assert LM.words(j)[0][1] == (-a * a) & M64 == 0x1FFFFFFFC0 and LM.words(j)[0][8] != 0
    assert int(LM.table(j)[0]["sum_dd"]) == ((-a * a) & M64) != -a * a
    assert LM.carry(j) == [TWO | 3, TWO | ((1 << 33) - 5), TWO | 3]


def _edge_series(rng, n):
    """jumps between the two ends of the price range, so that the 128-bit sum carries many times, and empty sides"""
    out = [(1, 2), (0xFFFFFFFD, 0xFFFFFFFE), (1, 2), (1, 0xFFFFFFFE), (0xFFFFFFFE, 0xFFFFFFFE), (0, MAXU), (0, 7), (7, MAXU), (MAXU, 0)]
    while len(out) < n:
        out.append((1, int(rng.integers(2, 9))) if rng.integers(0, 2) else (0xFFFFFFFD, 0xFFFFFFFE))
    return out


def _random_series(rng, n, wide):
    out = []
    for _ in range(n):
        if wide:
            bid, ask = int(rng.integers(1, 1 << 32)), int(rng.integers(0, MAXU))
        else:
            bid = int(rng.integers(990, 1010))
            ask = bid + int(rng.integers(1, 6))
        if rng.random() < 0.1:
            if rng.random() < 0.5:
                bid = 0
            else:
                ask = MAXU
        out.append((bid, ask))
    return out


def _write_case(tmp_path, series, lags, ends, want):
    with open(tmp_path / "records.txt", "w") as f:
        f.write(f"{len(series)}\n")
        for recs, K, e in zip(series, lags, ends):
            f.write(" ".join(str(x) for x in [len(recs), K, len(e)] + list(e)) + "\n")
            for r in recs:
                f.write(f"{r[0]} {r[1]}\n")
    with open(tmp_path / "expected.txt", "w") as f:
        for per_series in want:
            for rows, carry in per_series:
                for w in rows:
                    f.write(" ".join(str(x) for x in w) + "\n")
                f.write(" ".join(str(x) for x in carry) + "\n")


def test_lag_fold_hpp_equals_the_model_over_random_splits(tmp_path):
    gxx = _cxx()
    exe = str(tmp_path / "lag_fold_test")
    res = subprocess.run([gxx, "-std=c++17", "-O2", os.path.join(ROOT, "tests", "cpp", "lag_fold_test.cpp"), "-o", exe],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    rng = np.random.default_rng(17)
    KS = (1, 2, 5, 63, 64)
    series, lags, ends = [], [], []
    # per K: an edge series folded step by step, and one cut at the lengths the kernel's paths turn on
    for K in KS:
        series.append(_edge_series(rng, 90))
        lags.append(K)
        ends.append(list(range(1, 91)))  # every fold a single step
        n = 1 + 64 + 65 + 3 + 130 + 2 + 200
        series.append(_random_series(rng, n, wide=K % 2 == 0))
        lags.append(K)
        ends.append(list(np.cumsum([1, 64, 65, 3, 130, 2, 200])))  # below K, exactly 64, 65, above 128
    series += [[(5, 9)], [(0, MAXU)], [(5, 9), (6, 9)]]
    lags += [64, 5, 1]
    ends += [[1], [1], [2]]
    for q in range(26):
        n = int(rng.integers(2, 420))
        series.append(_random_series(rng, n, wide=q % 2 == 0))
        lags.append(KS[q % len(KS)])
        e = [n] if q % 4 == 0 else sorted(set(int(x) for x in rng.integers(1, n + 1, size=int(rng.integers(1, 9)))) | {n})
        ends.append(e)
    want, n_one_sided, n_steps = [], 0, 0
    for recs, K, e in zip(series, lags, ends):
        h = _hist(recs)
        n_steps += len(h)
        n_one_sided += int(np.sum((h[:, 1] == 0) | (h[:, 2] == MAXU)))
        s, lo, per = LM.cleared(K), 0, []
        for y in e:
            s = LM.fold(h[lo:y], first_step=lo, into=s)
            per.append((LM.words(s), LM.carry(s)))
            lo = y
        one = LM.fold(h, K)
        assert per[-1] == (LM.words(one), LM.carry(one))  # (the model itself is split-invariant)
        want.append(per)
    assert len(series) > 30 and 0.05 < n_one_sided / n_steps < 0.2
    lens = [b - a for e in ends for a, b in zip([0] + e[:-1], e)]
    assert 1 in lens and 64 in lens and 65 in lens and max(lens) > 128 and any(x < 5 for x in lens)
    first = dict(zip(LM.FIELDS, want[0][-1][0][0]))  # the edge series at K = 1: the words really wrap
    assert first["sum_h4_hi"] != 0 and first["max_abs_h"] == (1 << 33) - 8 and first["n_pairs"] > 20, "no word wraps"
    deep = want[9][-1][0][63]  # K = 64, lag 64: pairs exist
    assert lags[9] == 64 and deep[0] > 100 and deep[3] > 100
    _write_case(tmp_path, series, lags, ends, want)
    run = subprocess.run([exe, str(tmp_path / "records.txt"), str(tmp_path / "expected.txt")], capture_output=True, text=True,
                         timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip().endswith(f"lag_fold ok {len(series)} series {n_steps} steps {sum(len(e) for e in ends)} folds")
    # a wrong expectation is really caught: one word of one row off by one, and one carry word
    want[9][2][0][63][LM.FIELDS.index("sum_abs_dd")] += 1
    _write_case(tmp_path, series, lags, ends, want)
    run = subprocess.run([exe, str(tmp_path / "records.txt"), str(tmp_path / "expected.txt")], capture_output=True, text=True,
                         timeout=120)
    assert run.returncode == 1 and "series 9 fold 2 (lanes): lag 64 word 2 " in run.stdout and "(serial): lag 64 word 2 " in run.stdout
    want[9][2][0][63][LM.FIELDS.index("sum_abs_dd")] -= 1
    want[9][3][1][64] ^= 1
    _write_case(tmp_path, series, lags, ends, want)
    run = subprocess.run([exe, str(tmp_path / "records.txt"), str(tmp_path / "expected.txt")], capture_output=True, text=True,
                         timeout=120)
    assert run.returncode == 1 and "series 9 fold 3 (lanes): carry 64 " in run.stdout


def test_row_0_is_the_series_row_over_the_same_steps_and_cuts():
    rng = np.random.default_rng(5)
    pairs = (("n_pairs", "n_pairs"), ("sum_dd", "sum_dd"), ("sum_abs_dd", "sum_abs_dd"), ("n_h", "n_ret"), ("sum_h", "sum_d"),
             ("sum_abs_h", "sum_abs_d"), ("sum_h2", "sum_d2"), ("sum_h4_lo", "sum_d4_lo"), ("sum_h4_hi", "sum_d4_hi"),
             ("max_abs_h", "max_abs_d"))
    assert tuple(p[0] for p in pairs) == LM.FIELDS
    for q, (recs, cuts) in enumerate([(_random_series(rng, 300, False), ()), (_random_series(rng, 300, True), (40, 41, 200)),
                                      (_edge_series(rng, 120), (3, 77)), (HAND, ()), (HAND, (4,))]):
        h = _hist(recs)
        ser = dict(zip(SM.FIELDS, SM.words(SM.fold(h, cuts=cuts))))
        for K in (1, 7):
            lag0 = dict(zip(LM.FIELDS, LM.words(LM.fold(h, K, cuts=cuts))[0]))
            assert lag0 == {a: ser[b] for a, b in pairs}, (q, K)
        assert ser["n_pairs"] > 0 or len(recs) < 10


def test_the_entries_are_exported_bound_and_declared():
    import bourse_amd
    from bourse_amd import _lib

    L = _lib.load()
    header = open(os.path.join(ROOT, "include", "bourse_amd.h")).read()
    for name in ENTRIES:
        assert hasattr(L, name) and name in _lib.SIGNATURES, name
        m = re.search(r"\b" + name + r"\s*\([^;]*;", header)
        assert m, name
        assert re.search(r"\(No counterpart\s+(\*\s+)?in\s+(\*\s+)?the\s+(\*\s+)?reference\.\)\s*\*/\s*int\s+$", header[:m.start()]), name
    # a lost step refuses the fold: the set of flag bits is unchanged
    taken = [int(v) for v in re.findall(r"#define BK_FLAG_\w+ (\d+)u", header)]
    assert len(taken) == len(set(taken)) and sorted(taken) == sorted(_lib.FLAG_NAMES) == [1 << i for i in range(10)], taken
    assert "LAG" not in " ".join(re.findall(r"#define BK_FLAG_(\w+)", header))
    for method in ("enable_lags", "fold_lags", "lags", "lags_device_ptr", "lags_view", "clear_lags", "run_series"):
        assert callable(getattr(bourse_amd.ManyBookEnv, method)), method
        assert getattr(bourse_amd.ManyMarketEnv, method) is getattr(bourse_amd.ManyBookEnv, method), method
    assert bourse_amd.ManyBookEnv.LAG_DTYPE is _lib.LAG_DTYPE is bourse_amd.LAG_DTYPE
    assert bourse_amd.lag_moments is _lib.lag_moments
    hpp = open(os.path.join(ROOT, "include", "bourse_amd.hpp")).read()
    for method in ("enable_lags", "fold_lags", "lags", "lags_device_ptr", "clear_lags"):
        assert re.search(r"\b" + method + r"\(", hpp), method
    # the Rust FFI file is the generator's output for this header: the six entries, and the row field by field
    rs = open(os.path.join(ROOT, "integration", "rust", "bourse_amd_sys.rs")).read()
    for name in ENTRIES:
        assert re.search(r"pub fn " + name + r"\(", rs), name
    assert re.search(r"pub fn bk_lags_enable\(env: \*mut BkEnv, n_lags: u32\) -> c_int;", rs)
    body = re.search(r"pub struct BkLagRow \{(.*?)\}", rs, flags=re.S).group(1)
    assert re.findall(r"pub (\w+): (\w+),", body) == [(n, "i64" if n in LM.SIGNED else "u64") for n in LM.FIELDS]


def test_bk_lag_row_is_80_bytes_laid_out_as_the_dtype(tmp_path):
    from bourse_amd import _lib

    dt = _lib.LAG_DTYPE
    assert dt.itemsize == 80 and dt.names == LM.FIELDS == _lib.LAG_FIELDS
    assert [dt.fields[n][1] for n in dt.names] == [8 * i for i in range(10)]
    assert [dt.fields[n][0].str for n in dt.names] == ["<i8" if n in ("sum_dd", "sum_h") else "<u8" for n in dt.names]
    assert dt == LM.LAG_DTYPE
    gxx = _cxx()
    src = tmp_path / "layout.cpp"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "bourse_amd.h"\n'
                   'int main() { std::printf("%zu", sizeof(bk_lag_row));\n' +
                   "".join(f'std::printf(" %zu", offsetof(bk_lag_row, {n}));\n' for n in dt.names) + 'return 0; }\n')
    exe = str(tmp_path / "layout")
    res = subprocess.run([gxx, "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60).stdout.split()
    assert [int(x) for x in out] == [80] + [8 * i for i in range(10)]


def test_a_null_env_is_refused_not_dereferenced():
    from bourse_amd import _lib

    L = _lib.load()
    mask = (ctypes.c_uint8 * 4)(1, 0, 1, 0)
    out = ctypes.c_void_p()
    rows = np.zeros((4, 3), dtype=_lib.LAG_DTYPE)
    calls = {
        "bk_lags_enable": lambda: L.bk_lags_enable(None, 3),
        "bk_lags_fold": lambda: L.bk_lags_fold(None),
        "bk_lags_clear": lambda: L.bk_lags_clear(None, ctypes.cast(mask, ctypes.c_void_p)),
        "bk_lags_clear_device": lambda: L.bk_lags_clear_device(None, ctypes.cast(mask, ctypes.c_void_p)),
        "bk_lags_device_ptr": lambda: L.bk_lags_device_ptr(None, ctypes.byref(out)),
        "bk_get_lags": lambda: L.bk_get_lags(None, 0, 1, rows.ctypes.data_as(ctypes.c_void_p)),
    }
    assert set(calls) == set(ENTRIES)
    for name, call in calls.items():
        L.bk_device_count(ctypes.byref(ctypes.c_int(0)))  # (anything that may leave another message behind)
        assert call() == BK_INVALID_ARGUMENT, name
        assert b"null env" in L.bk_last_error(), name


def test_the_kernels_stay_out_of_the_baselined_namespace_and_every_launch_sits_behind_the_guard():
    """bkd::lags kernels are not among the names tools/kernel_isa_counts.py::measure lists (those start with k_ once
    "void bkd::" is stripped), so profiles/kernel_isa_baseline.json stays as it is; the fold is plain C++ and shares its
    per-term arithmetic and its window with the CPU test through lag_fold.hpp."""
    src = open(os.path.join(ROOT, "bourse_amd", "csrc", "lags.hpp")).read()
    body = src[src.index("namespace bkd {"):]
    assert re.search(r"namespace bkd \{\s*namespace lags \{", body)
    for k in ("k_fold", "k_clear"):
        assert re.search(r"__global__[^;{]*\b" + k + r"\(", body), k
    code = re.sub(r"//.*", "", src)
    assert "asm" not in code and "atomic" not in code.replace("__ATOMIC_ACQ_REL", "") and "series::" not in code
    assert '#include "lag_fold.hpp"' in src
    for f in ("add(", "merge(", "word_of(", "carry_at(", "step_at(", "WINDOW_WORDS"):
        assert f in code, f
    fold = open(os.path.join(ROOT, "bourse_amd", "csrc", "lag_fold.hpp")).read()
    assert re.search(r"namespace bkd \{\s*namespace lags \{", fold)
    assert "hip_runtime" not in fold and "asm" not in re.sub(r"//.*", "", fold)
    # (where bourse_amd.hip launches them, and behind which guard: tests/test_hist_tables_cpu.py)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_isa_counts as K

    base = json.load(open(K.BASELINE))["kernels"]
    assert not [k for k in base if "lags" in k or "k_fold" in k]


def test_lag_moments_against_numpy_on_the_raw_history():
    from bourse_amd import _lib, lag_moments, series_moments

    rng = np.random.default_rng(3)
    K = 12
    recs = _random_series(rng, 600, wide=False)
    h = _hist(recs)
    rows = np.array([LM.table(LM.fold(h, K))], dtype=_lib.LAG_DTYPE)
    got = lag_moments(rows)
    assert got.shape == (1, K) and got.dtype == _lib.LAG_MOMENTS_DTYPE
    got = got[0]
    bid, ask = h[:, 1].astype(np.float64), h[:, 2].astype(np.float64)
    two = (h[:, 1] != 0) & (h[:, 2] != MAXU)
    m = bid + ask
    ret = np.concatenate([[False], two[1:] & two[:-1]])
    d = np.concatenate([[0.0], m[1:] - m[:-1]])
    mu, var = np.mean(d[ret]), np.var(d[ret])
    mua, vara = np.mean(np.abs(d[ret])), np.var(np.abs(d[ret]))
    var1 = None
    assert not two.all()
    for k in range(1, K + 1):
        pair = ret[k:] & ret[:-k]
        dd = (d[k:] * d[:-k])[pair]
        span = two[k:] & two[:-k]
        hk = (m[k:] - m[:-k])[span]
        assert len(dd) > 300 and len(hk) > 400
        var_h = np.var(hk) / 4
        var1 = var_h if k == 1 else var1
        want = dict(acf_return=(np.mean(dd) - mu ** 2) / var, acf_abs_return=(np.mean(np.abs(dd)) - mua ** 2) / vara, var_h=var_h,
                    kurtosis_h=len(hk) * np.sum(hk ** 4) / np.sum(hk ** 2) ** 2 - 3, variance_ratio=var_h / (k * var1))
        for name, v in want.items():
            assert abs(got[k - 1][name] - v) <= 1e-12 * abs(v), (k, name, got[k - 1][name], v)
    assert got[0]["variance_ratio"] == 1.0
    # at lag 1 the two autocorrelations are series_moments' bit for bit
    ser = series_moments(np.array([SM.row(SM.fold(h))], dtype=_lib.SERIES_DTYPE))[0]
    assert got[0]["acf_return"] == ser["acf1_return"] and got[0]["acf_abs_return"] == ser["acf1_abs_return"]
    assert got[0]["var_h"] == ser["var_return"] and got[0]["kurtosis_h"] == ser["kurtosis_return"]
    # a zero count or a zero variance gives NaN, not an error: a cleared table, and a book that never moved
    none = lag_moments(np.array([LM.table(LM.cleared(3))], dtype=_lib.LAG_DTYPE))
    assert none.shape == (1, 3) and all(np.isnan(none[n]).all() for n in none.dtype.names)
    flat = lag_moments(LM.table(LM.fold(_hist([(5, 9)] * 6), 2)))
    assert flat.shape == (2,) and flat["var_h"].tolist() == [0.0, 0.0]
    assert all(np.isnan(flat[n]).all() for n in ("acf_return", "acf_abs_return", "kurtosis_h", "variance_ratio"))
    with pytest.raises(ValueError):
        lag_moments(np.zeros(2, dtype=np.uint64))
