"""The per-market cross table (bk_cross_enable) without a GPU: the plain-Python model against rows worked out by hand, the
kernel's rules, window placement and unit mapping (bourse_amd/csrc/cross_fold.hpp, compiled with a host compiler into a
program of its own, plain and under the sanitizers) against the model over edge series, random series and every split of a
fold into two, the C ABI - the entries are exported, bound and declared and refuse a null env and a null config - the built
kernels' resources, and cross_moments against numpy."""
import copy
import ctypes
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import cross_model as XM
from test_candles_cpu import _cxx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bourse_amd", "csrc")
ENTRIES = ("bk_cross_enable", "bk_cross_config_get", "bk_cross_fold", "bk_cross_clear", "bk_cross_clear_device", "bk_cross_device_ptr",
           "bk_get_cross")
BK_INVALID_ARGUMENT = 5
MAXU = 0xFFFFFFFF
TWO = 1 << 63
M64 = (1 << 64) - 1
F = {n: i for i, n in enumerate(XM.FIELDS)}


def _u(x):
    return x & M64


def _hist(assets):
    """[[(bid, ask), ..] per asset] -> an [n_steps, A, 5] history: only words 1 and 2 are read"""
    h = np.zeros((len(assets[0]), len(assets), 5), dtype=np.uint64)
    for a, steps in enumerate(assets):
        for i, (bid, ask) in enumerate(steps):
            h[i, a, 1], h[i, a, 2] = bid, ask
    return h


# two assets, six steps, spans (1, 2).  Twice the mid:
#   asset 0: 204, 206,  - , 206, 207, 205      (one-sided at step 2)
#   asset 1: 102, 104, 105, 106,  - , 108      (one-sided at step 4)
HAND = [[(100, 104), (102, 104), (0, 104), (100, 106), (101, 106), (99, 106)],
        [(50, 52), (50, 54), (51, 54), (51, 55), (51, MAXU), (52, 56)]]
# span 1: x_0 = 2 at s = 1, 1 at s = 4, -2 at s = 5; x_1 = 2, 1, 1 at s = 1, 2, 3.  Both at s = 1 only.
#   lead (0, 0): s = 5: -2 * (207 - 206);  lead (1, 1): s = 2: 1 * 2, s = 3: 1 * 1
#   lead (0, 1): s = 4: 1 * (106 - 105), and asset 1 is one-sided AT step 4;  lead (1, 0): s = 2: 1 * (206 - 204), asset 0 one-sided at 2
# span 2: X_0 = 0 at s = 3, -1 at s = 5; X_1 = 3, 2, 2 at s = 2, 3, 5.  Both at s = 3 and 5.
#   leads at s = 5 only: z_0 = 206 - 206 = 0, z_1 = 106 - 104 = 2
#            n  sum_x   sum_y  xx  yy  xy   n_lead sum_lead
HAND_ROWS = [[[[3, 1, 1, 9, 9, 9, 1, _u(-2)], [1, 2, 2, 4, 4, 4, 1, 1]],
              [[1, 2, 2, 4, 4, 4, 1, 2], [3, 4, 4, 6, 6, 6, 2, 3]]],
             [[[2, _u(-1), _u(-1), 1, 1, 1, 1, 0], [2, _u(-1), 4, 1, 8, _u(-2), 1, _u(-2)]],
              [[2, 4, _u(-1), 8, 1, _u(-2), 1, 0], [3, 7, 7, 17, 17, 17, 1, 4]]]]
HAND_CARRY = [[0, TWO | 206, TWO | 207, TWO | 205], [TWO | 105, TWO | 106, 0, TWO | 108]]


def _state(s):
    return XM.words(s), XM.carry(s)


def test_the_model_against_rows_worked_out_by_hand():
    h = _hist(HAND)
    s = XM.fold(h, (1, 2))
    assert XM.words(s) == HAND_ROWS
    assert XM.carry(s) == HAND_CARRY
    w = XM.words(s)
    assert w[0][0][1][F["n"]] < w[0][0][0][F["n"]] and w[0][0][1][F["n"]] < w[0][1][1][F["n"]], "pairwise complete: n(0, 1) is below both diagonals"
    # every split into two folds gives the same table and carry
    for y in range(1, 6):
        part = XM.fold(h[y:], first_step=y, into=XM.fold(h[:y], (1, 2)))
        assert _state(part) == _state(s), y
    # a cut in front of step 5 removes every term of step 5 (both spans reach over it) and leaves the carry with step 5 alone
    c = XM.fold(h, (1, 2), cuts=[5])
    assert _state(c) == (XM.words(XM.fold(h[:5], (1, 2))), [[0, 0, 0, TWO | 205], [0, 0, 0, TWO | 108]])
    assert XM.carry(XM.cut(s)) == [[0] * 4] * 2 and XM.carry(XM.cleared((1, 2), 2)) == [[0] * 4] * 2
    # spans in another order and twice: the rows follow their span
    r = XM.words(XM.fold(h, (2, 1, 2)))
    assert r == [HAND_ROWS[1], HAND_ROWS[0], HAND_ROWS[1]]
    t = XM.table(s)
    assert t.dtype == XM.CROSS_DTYPE and t.shape == (2, 2, 2) and int(t["sum_lead"][0, 0, 0]) == -2 and int(t["sum_xy"][1, 0, 1]) == -2
    both = XM.rows(np.concatenate([h, h[:, ::-1]], axis=1), (1, 2), 2)
    assert both.shape == (2, 2, 2, 2) and (both[0] == t).all() and (both[1] == t[:, ::-1, ::-1]).all()
    # (a, b) and (b, a) share n and sum_xy and swap the rest
    for j in range(2):
        assert t[j, 0, 1]["n"] == t[j, 1, 0]["n"] and t[j, 0, 1]["sum_xy"] == t[j, 1, 0]["sum_xy"]
        assert t[j, 0, 1]["sum_x"] == t[j, 1, 0]["sum_y"] and t[j, 0, 1]["sum_xx"] == t[j, 1, 0]["sum_yy"]


def _random_hist(rng, n, A, wide=False, p_one_sided=0.1):
    """a random market: narrow quotes (or jumps between the two ends of the price range: bid 1 / ask 0xFFFFFFFE against the
    other end, so that products of two changes pass 2^64), one-sided steps at different steps in every asset"""
    h = np.zeros((n, A, 5), dtype=np.uint64)
    for i in range(n):
        for a in range(A):
            if wide:
                bid, ask = ((1, 2), (0xFFFFFFFD, 0xFFFFFFFE), (1, 0xFFFFFFFE))[int(rng.integers(0, 3))]
            else:
                bid = int(rng.integers(990, 1010)) + 10 * a
                ask = bid + int(rng.integers(1, 6))
            if rng.random() < p_one_sided:
                if rng.random() < 0.5:
                    bid = 0
                else:
                    ask = MAXU
            h[i, a, 1], h[i, a, 2] = bid, ask
    return h


def _prefix_states(h, spans, A):
    """(words, carry) of the model after every prefix h[:y], y = 1 .. n, in one pass"""
    s, out = XM.cleared(spans, A), []
    for y in range(len(h)):
        s = XM.fold(h[y:y + 1], first_step=y, into=s)
        out.append(copy.deepcopy(_state(s)))
    return out


def _cases(rng, short=False):
    """[(hist, A, spans, ends), ..] and what the model leaves after every fold"""
    cases, want = [], []

    def put(h, A, spans, splits):
        pre = _prefix_states(h, spans, A)
        assert pre[-1] == _state(XM.fold(h, spans, A))  # (the model itself is split-invariant)
        for ends in splits:
            cases.append((h, A, spans, ends))
            want.append([copy.deepcopy(pre[e - 1]) for e in ends])

    for A in (2, 3, 8):
        for spans in ((1,), (64, 1, 5, 64)) if not short else ((64, 3),):
            n = 10 if A == 8 else 24
            if short:
                n = 7
            # every split of one fold into two, on a series with the ends of the price range
            h = _random_hist(rng, n, A, wide=True, p_one_sided=0.15)
            put(h, A, spans, [[n]] + [[y, n] for y in range(1, n)])
            # single-step folds
            put(h, A, spans, [list(range(1, n + 1))])
            # more than one chunk, the windows moved, folds of 1, 64, 65 and 130 steps
            if not short:
                m = 1 + 64 + 65 + 130 + 3
                h = _random_hist(rng, m, A, wide=A == 3, p_one_sided=0.1)
                put(h, A, spans, [[1, 65, 130, 260, m], [m]])
    return cases, want


def _write_case(tmp_path, cases, want):
    with open(tmp_path / "records.txt", "w") as f:
        f.write(f"{len(cases)}\n")
        for h, A, spans, ends in cases:
            f.write(" ".join(str(x) for x in [len(h), A, len(spans), *spans, len(ends), *ends]) + "\n")
            for recs in h:
                f.write(" ".join(f"{int(r[1])} {int(r[2])}" for r in recs) + "\n")
    with open(tmp_path / "expected.txt", "w") as f:
        for per_fold in want:
            for words, carry in per_fold:
                for of_j in words:
                    for of_a in of_j:
                        for w in of_a:
                            f.write(" ".join(str(x) for x in w) + "\n")
                for c in carry:
                    f.write(" ".join(str(x) for x in c) + "\n")


def _build_exe(tmp_path, extra=()):
    exe = str(tmp_path / "cross_fold_test")
    res = subprocess.run([_cxx(), "-std=c++17", "-O2", *extra, os.path.join(ROOT, "tests", "cpp", "cross_fold_test.cpp"), "-o", exe],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return exe


def test_cross_fold_hpp_equals_the_model_over_edge_series_random_series_and_every_split(tmp_path):
    exe = _build_exe(tmp_path)
    cases, want = _cases(np.random.default_rng(53))
    # what the cases must hold to say anything: a product that passes 2^64, one-sided steps, both signs, leads without m_b(s)
    exact = XM.fold(cases[0][0], (1,))["rows"][0]
    assert max(abs(r["sum_xy"]) for of_a in exact for r in of_a) >> 64 or max(r["sum_xx"] for of_a in exact for r in of_a) >> 64
    last = [per[-1][0] for per in want]
    assert any(w[0][0][1][F["sum_xy"]] >> 63 for w in last) and any(0 < w[0][0][1][F["sum_xy"]] < TWO for w in last)
    assert any(w[0][0][1][F["n"]] < min(w[0][0][0][F["n"]], w[0][1][1][F["n"]]) for w in last)
    assert any(w[0][0][1][F["n_lead"]] > w[0][0][1][F["n"]] for w in last), "a lead term whose step lacks m_b(s)"
    assert {c[1] for c in cases} == {2, 3, 8} and {max(c[2]) for c in cases} == {1, 64}
    _write_case(tmp_path, cases, want)
    args = [exe, str(tmp_path / "records.txt"), str(tmp_path / "expected.txt")]
    run = subprocess.run(args, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout + run.stderr
    n_steps, n_folds = sum(len(c[0]) for c in cases), sum(len(c[3]) for c in cases)
    assert run.stdout.strip().endswith(f"cross_fold ok {len(cases)} markets {n_steps} steps {n_folds} folds")
    # a wrong expectation is really caught, by name: one word of a row, one carry bit
    q = next(i for i, c in enumerate(cases) if c[1] == 3 and len(c[3]) == 2 and c[3][0] == 5)
    want[q][1][0][0][2][1][F["sum_lead"]] ^= 1  # span 0, a = 2, b = 1: unit 7
    _write_case(tmp_path, cases, want)
    run = subprocess.run(args, capture_output=True, text=True, timeout=600)
    assert run.returncode == 1 and f"market {q} fold 1 (lanes): unit 7 word 7 " in run.stdout, run.stdout
    assert f"market {q} fold 1 (serial): unit 7 word 7 " in run.stdout
    want[q][1][0][0][2][1][F["sum_lead"]] ^= 1
    want[q][0][1][1][-1] ^= 1  # asset 1's last carry word
    _write_case(tmp_path, cases, want)
    run = subprocess.run(args, capture_output=True, text=True, timeout=600)
    C = 2 * max(cases[q][2])
    assert run.returncode == 1 and f"market {q} fold 0 (lanes): carry {2 * C - 1} is " in run.stdout, run.stdout
    assert f"market {q} fold 0 (serial): carry {2 * C - 1} is " in run.stdout


def test_cross_fold_hpp_under_the_address_and_undefined_behaviour_sanitizers(tmp_path):
    """the same program built once with -fsanitize=address,undefined, run on its own over a short case"""
    exe = _build_exe(tmp_path, ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    cases, want = _cases(np.random.default_rng(59), short=True)
    _write_case(tmp_path, cases, want)
    run = subprocess.run([exe, str(tmp_path / "records.txt"), str(tmp_path / "expected.txt")], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and f"cross_fold ok {len(cases)} markets" in run.stdout, run.stdout + run.stderr
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr


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
    assert sorted(set(re.findall(r"\bbk_\w*cross\w*(?=\()", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))) == sorted(ENTRIES)
    # no flag bit
    taken = [int(v) for v in re.findall(r"#define BK_FLAG_\w+ (\d+)u", header)]
    assert sorted(taken) == sorted(_lib.FLAG_NAMES) == [1 << i for i in range(10)], taken
    for method in ("enable_cross", "fold_cross", "cross", "cross_view", "cross_device_ptr", "cross_config", "clear_cross", "run_series"):
        assert callable(getattr(bourse_amd.ManyMarketEnv, method)), method
    assert bourse_amd.CROSS_FIELDS is _lib.CROSS_FIELDS and bourse_amd.CROSS_DTYPE is _lib.CROSS_DTYPE
    assert bourse_amd.CROSS_FIELDS == XM.FIELDS and bourse_amd.CROSS_DTYPE == XM.CROSS_DTYPE and bourse_amd.CROSS_DTYPE.itemsize == 64
    assert bourse_amd.cross_moments is _lib.cross_moments and _lib.CROSS_CONFIG_DTYPE.itemsize == 20
    # the header's struct names the words in their order
    struct = re.search(r"typedef struct bk_cross_row \{(.*?)\} bk_cross_row;", header, flags=re.S).group(1)
    assert re.findall(r"\b(n|sum_\w+|n_lead)\b(?=[,;])", re.sub(r"/\*.*?\*/", "", struct)) == list(XM.FIELDS)
    hpp = open(os.path.join(ROOT, "include", "bourse_amd.hpp")).read()
    for method in ("enable_cross", "cross_config", "fold_cross", "cross", "cross_device_ptr", "clear_cross"):
        assert re.search(r"\b" + method + r"\(", hpp), method
    rs = open(os.path.join(ROOT, "integration", "rust", "bourse_amd_sys.rs")).read()
    assert re.search(r"pub fn bk_cross_enable\(env: \*mut BkEnv, cfg: \*const BkCrossConfig\) -> c_int;", rs)
    assert re.search(r"pub fn bk_cross_config_get\(env: \*mut BkEnv, out: \*mut BkCrossConfig\) -> c_int;", rs)
    assert re.search(r"pub fn bk_cross_fold\(env: \*mut BkEnv\) -> c_int;", rs)
    assert re.search(r"pub fn bk_cross_clear\(env: \*mut BkEnv, mask_host: \*const u8\) -> c_int;", rs)
    assert re.search(r"pub fn bk_cross_clear_device\(env: \*mut BkEnv, mask_dev: \*const u8\) -> c_int;", rs)
    assert re.search(r"pub fn bk_cross_device_ptr\(env: \*mut BkEnv, out: \*mut \*mut c_void\) -> c_int;", rs)
    assert re.search(r"pub fn bk_get_cross\(env: \*mut BkEnv, first_market: u32, n_markets: u32, out: \*mut BkCrossRow\) -> c_int;", rs)
    assert "pub struct BkCrossRow" in rs and "pub struct BkCrossConfig" in rs and "pub spans: [u32; 4]," in rs
    # the enum of cross_fold.hpp is the same order, and the header reuses the lag table's window word
    fold = open(os.path.join(CSRC, "cross_fold.hpp")).read()
    words = re.search(r"enum Word : uint32_t \{[^\n]*\n(.*?)\};", fold, flags=re.S).group(1)
    assert [w.strip().split(" ")[0].lower() for w in words.replace("\n", " ").split(",")] == list(XM.FIELDS) + ["row_words"]
    code = re.sub(r"//.*", "", fold)
    assert "hip_runtime" not in fold and "asm" not in code and '#include "lag_fold.hpp"' in fold
    assert "using lags::word_of;" in code and not re.search(r"\bword_of\([^;{]*\)\s*\{", code) and "two_sided(" not in code


def test_a_null_env_and_a_null_config_are_refused_not_dereferenced():
    from bourse_amd import _lib

    L = _lib.load()
    out = ctypes.c_void_p()
    cfg = np.array([1, 1, 0, 0, 0], dtype=np.uint32)
    rows = np.zeros((1, 1, 2, 2), dtype=XM.CROSS_DTYPE)
    mask = np.ones(1, dtype=np.uint8)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    calls = {
        "bk_cross_enable": lambda: L.bk_cross_enable(None, P(cfg)),
        "bk_cross_config_get": lambda: L.bk_cross_config_get(None, P(cfg)),
        "bk_cross_fold": lambda: L.bk_cross_fold(None),
        "bk_cross_clear": lambda: L.bk_cross_clear(None, P(mask)),
        "bk_cross_clear_device": lambda: L.bk_cross_clear_device(None, None),
        "bk_cross_device_ptr": lambda: L.bk_cross_device_ptr(None, ctypes.byref(out)),
        "bk_get_cross": lambda: L.bk_get_cross(None, 0, 1, P(rows)),
    }
    assert set(calls) == set(ENTRIES)
    for name, call in calls.items():
        L.bk_device_count(ctypes.byref(ctypes.c_int(0)))  # (anything that may leave another message behind)
        assert call() == BK_INVALID_ARGUMENT, name
        assert b"null env" in L.bk_last_error(), name
    # the config is looked at only behind the env's check, and a null one is refused there in front of everything else
    src = re.sub(r"//.*", "", open(os.path.join(CSRC, "bourse_amd.hip")).read())
    enable = src[src.index("int bk_cross_enable("):src.index("int bk_cross_config_get(")]
    order = [enable.index(x) for x in ('"null env"', 'if (!cfg) return fail(BK_INVALID_ARGUMENT, "null argument")', "history_capacity", "env->M < 2u",
                                       "cross_config_fault(*cfg)", "already enabled", ".alloc(", "table_commit_enable(env, env->cross_table)")]
    assert order == sorted(order), order


def test_the_built_cross_kernels_use_no_scratch():
    """the built library's metadata, read with llvm-readelf: no scratch (the four rounds' accumulators stay in registers);
    the fold's LDS is dynamic, so none is fixed"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_isa_counts as K
    from bourse_amd import _build

    lib = _build.build()
    meta = {}
    with tempfile.TemporaryDirectory(prefix="bourse_cross_isa_") as tmp:
        for co in K.code_objects(lib, tmp):
            txt = subprocess.run([K._tool("llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
            for blk in re.split(r"\n\s+- \.agpr_count:", txt):
                name = re.search(r"\.name:\s+(\S+)", blk)
                if name and "5cross" in name.group(1):
                    meta[name.group(1)] = {k: int(v) for k, v in re.findall(
                        r"\.(private_segment_fixed_size|group_segment_fixed_size|vgpr_count|sgpr_count):\s+(\d+)", blk)}
    assert len(meta) == 2 and any("k_fold" in n for n in meta) and any("k_clear" in n for n in meta), meta
    for name, m in meta.items():
        assert m["private_segment_fixed_size"] == 0, (name, m)


def test_cross_moments_against_numpy_on_the_models_rows():
    from bourse_amd import cross_moments

    rng = np.random.default_rng(61)
    A, spans, n = 3, (1, 4), 200
    h = _random_hist(rng, n, A, p_one_sided=0.15)
    h[:, 2, 1], h[:, 2, 2] = 500, 504  # asset 2 never moves: its variance is 0
    rows = XM.rows(h, spans, A)
    got = cross_moments(rows)
    assert got.shape == (1, 2, A, A) and got.dtype.names == ("n", "cov", "corr", "beta", "lead_corr")
    m = (h[:, :, 1] + h[:, :, 2]).astype(np.float64) / 2.0
    two = (h[:, :, 1] != 0) & (h[:, :, 2] != MAXU)
    for j, k in enumerate(spans):
        for a in range(A):
            for b in range(A):
                s = np.arange(k, n)
                ok = two[s, a] & two[s - k, a] & two[s, b] & two[s - k, b]
                x, y = (m[s, a] - m[s - k, a])[ok], (m[s, b] - m[s - k, b])[ok]
                g = got[0, j, a, b]
                assert g["n"] == ok.sum() > 0
                cov = (x * y).mean() - x.mean() * y.mean()
                assert np.isclose(g["cov"], cov, rtol=1e-9, atol=1e-12), (j, a, b)
                if a == 2 or b == 2:
                    assert np.isnan(g["corr"]) and np.isnan(g["lead_corr"]) and (np.isnan(g["beta"]) if b == 2 else g["beta"] == 0.0), (j, a, b)
                    continue
                sd = np.sqrt(((x * x).mean() - x.mean() ** 2) * ((y * y).mean() - y.mean() ** 2))
                assert np.isclose(g["corr"], cov / sd, rtol=1e-9) and np.isclose(g["beta"], cov / ((y * y).mean() - y.mean() ** 2), rtol=1e-9)
                s2 = np.arange(2 * k, n)
                okl = two[s2, a] & two[s2 - k, a] & two[s2 - k, b] & two[s2 - 2 * k, b]
                xl, zl = (m[s2, a] - m[s2 - k, a])[okl], (m[s2 - k, b] - m[s2 - 2 * k, b])[okl]
                assert np.isclose(g["lead_corr"], ((xl * zl).mean() - x.mean() * y.mean()) / sd, rtol=1e-9, atol=1e-12), (j, a, b)
                if a == b:
                    assert np.isclose(g["corr"], 1.0) and np.isclose(g["beta"], 1.0)
    # the NaN cases: no step at all, one step (no variance), and no lead
    empty = cross_moments(np.zeros((2, 1, 2, 2), dtype=XM.CROSS_DTYPE))
    assert (empty["n"] == 0).all() and all(np.isnan(empty[f]).all() for f in ("cov", "corr", "beta", "lead_corr"))
    one = XM.rows(_hist(HAND)[:2], (1,), 2)
    g = cross_moments(one)[0, 0, 0, 1]
    assert g["n"] == 1 and g["cov"] == 0.0 and np.isnan(g["corr"]) and np.isnan(g["beta"]) and np.isnan(g["lead_corr"])
    few = XM.rows(_hist([[(10, 12), (11, 12), (12, 14)], [(20, 22), (20, 24), (21, 24)]]), (2,), 2)
    assert few["n"][0, 0, 0, 1] == 1 and few["n_lead"][0, 0, 0, 1] == 0
    with pytest.raises(ValueError):
        cross_moments(np.zeros((2, 8), dtype=np.uint64))
