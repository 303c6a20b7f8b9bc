"""The per-book candle table (bk_candles_enable) without a GPU: the plain-Python model against bars worked out by hand, the
kernel's rules and lane mapping (bourse_amd/csrc/candle_fold.hpp, compiled with a host compiler into a program of its own)
against the model over edge series, random series and splits, the bars' sums against the series' model, the C ABI - the
entries are exported, bound and declared and refuse a null env - the layout of the kernel's source, the built kernels'
resources, and candle_series against numpy."""
import ctypes
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import candles_model as CM
import series_model as SM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bourse_amd", "csrc")
ENTRIES = ("bk_candles_enable", "bk_candles_config_get", "bk_candles_device_ptr", "bk_get_candles")
BK_INVALID_ARGUMENT = 5
MAXU = 0xFFFFFFFF
TWO = 1 << 63
M64 = (1 << 64) - 1
F = {n: i for i, n in enumerate(CM.FIELDS)}
CONFIGS = ((1, 256), (3, 4), (5, 64), (64, 4), (100, 2), (7, 1), (1 << 20, 1))
FOLD_LENGTHS = (1, 64, 65, 3, 130, 2, 200)
SUMMED = ("n_steps", "n_two_sided", "sum_m", "sum_spread", "sum_trade_vol", "n_trade_steps", "n_ret", "sum_d", "sum_abs_d", "sum_d2")


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
        pytest.fail("no host C++ compiler (g++, c++, clang++ or hipcc): candle_fold.hpp cannot be checked")


def _hist(steps):
    """[(bid, ask) or (bid, ask, trade_vol), ..] -> an [n_steps, 5] history: words 3 and 4 are not read"""
    h = np.zeros((len(steps), 5), dtype=np.uint64)
    for i, s in enumerate(steps):
        h[i, 1], h[i, 2] = s[0], s[1]
        h[i, 0] = s[2] if len(s) > 2 else 0
    return h


def _state(s):
    return CM.words(s), CM.carry(s)


def _u(x):
    return x & M64


# the series' six-step case: m = -, -, 204, 206, 204, 204; one unit trades at step 5
HAND = [(0, MAXU), (100, MAXU), (100, 104), (102, 104), (100, 104), (100, 104, 1)]
#       first n  two open high low close sum_m spread vol n_tr n_ret sum_d |d| d2 max
BAR_1 = [2, 2, 2, 204, 206, 204, 206, 410, 6, 0, 0, 1, 2, 2, 4, 2]
BAR_2 = [4, 2, 2, 204, 204, 204, 204, 408, 8, 1, 1, 2, _u(-2), 2, 4, 2]
BAR_2_CUT = [4, 2, 2, 204, 204, 204, 204, 408, 8, 1, 1, 1, 0, 0, 0, 0]
BAR_0 = [0, 2] + [0] * 14


def test_the_model_against_bars_worked_out_by_hand():
    cfg = CM.config(2, 2)
    s = CM.fold(_hist(HAND), cfg)
    # bar 0 (steps 0, 1) is pushed out: 0 + 2 <= 2; slot 1 holds bar 1, slot 0 bar 2
    assert CM.words(s) == [BAR_2, BAR_1]
    assert CM.carry(s) == TWO | 204
    # every split into two folds gives the same table and carry
    for y in range(1, 6):
        part = CM.fold(_hist(HAND)[y:], first_step=y, into=CM.fold(_hist(HAND)[:y], cfg))
        assert _state(part) == _state(s), y
    # a cut in front of step 4 removes the return -2 from bar 2
    c = CM.fold(_hist(HAND), cfg, cuts=[4])
    assert CM.words(c) == [BAR_2_CUT, BAR_1] and CM.carry(c) == TWO | 204
    # at N = 4 bar 0 is present with its two steps and everything else 0
    w = CM.words(CM.fold(_hist(HAND), CM.config(2, 4)))
    assert w == [BAR_0, BAR_1, BAR_2, [0] * 16]
    # the last step one-sided: the carry is 0; behind a cut or a clear too
    assert CM.carry(CM.fold(_hist(HAND[:2]), cfg)) == 0 and CM.carry(CM.cut(s)) == 0 and CM.carry(CM.cleared(cfg)) == 0
    # an unaligned start: the first bar is partial and keeps the step it started at
    p = CM.words(CM.fold(_hist(HAND)[3:], CM.config(2, 4), first_step=3))
    assert p[1][:7] == [3, 1, 1, 206, 206, 206, 206] and p[1][11] == 0 and p[2] == BAR_2 and p[0] == [0] * 16
    t = CM.table(s)
    assert t.dtype == CM.CANDLE_DTYPE and t.shape == (2,) and int(t["sum_d"][0]) == -2 and int(t["first_step"][1]) == 2


def _random_hist(rng, n, wide=False, p_one_sided=0.1):
    """a random history: narrow quotes (or jumps between the two ends of the price range), one-sided steps, traded volume
    on some steps - small, or up to 2^32 - 1"""
    h = np.zeros((n, 5), dtype=np.uint64)
    for i in range(n):
        if wide:
            bid, ask = ((1, 2), (0xFFFFFFFD, 0xFFFFFFFE))[int(rng.integers(0, 2))]  # |d| = 2^33 - 8
        else:
            bid = int(rng.integers(990, 1010))
            ask = bid + int(rng.integers(1, 6))
        if rng.random() < p_one_sided:
            if rng.random() < 0.5:
                bid = 0
            else:
                ask = MAXU
        h[i, 1], h[i, 2] = bid, ask
        if rng.random() < 0.4:
            h[i, 0] = MAXU - int(rng.integers(0, 3)) if wide and rng.random() < 0.5 else int(rng.integers(1, 400))
    return h


def _edge_hist():
    """jumps between (1, 2) and (0xFFFFFFFD, 0xFFFFFFFE), empty sides, both sides empty, crossed quotes (the spread wraps),
    trade_vol up to 2^32 - 1"""
    lo, hi = (1, 2), (0xFFFFFFFD, 0xFFFFFFFE)
    steps = [lo, hi, lo + (MAXU,), hi, hi, (0, 2), lo, (1, MAXU), (0, MAXU), hi + (MAXU,), lo, (104, 100, 7), (104, 100), lo, hi, (0, 2, MAXU),
             (0, 5), hi, lo, lo, hi, (7, 3, 1), hi]
    return _hist(steps * 3)


def _write_case(tmp_path, cases, want):
    """cases: [(hist, cfg, first_step, [(end, cut), ..]), ..]"""
    with open(tmp_path / "records.txt", "w") as f:
        f.write(f"{len(cases)}\n")
        for h, cfg, first, folds in cases:
            f.write(" ".join(str(x) for x in [len(h), cfg["width"], cfg["n"], first, len(folds)] + [v for e in folds for v in e]) + "\n")
            for rec in h:
                f.write(f"{int(rec[0])} {int(rec[1])} {int(rec[2])}\n")
    with open(tmp_path / "expected.txt", "w") as f:
        for per_series in want:
            for words, carry in per_series:
                for w in words:
                    f.write(" ".join(str(x) for x in w) + "\n")
                f.write(f"{carry}\n")


def _expect(cases):
    want = []
    for h, cfg, first, folds in cases:
        s, lo, per = CM.cleared(cfg), 0, []
        for y, cut in folds:
            s = CM.fold(h[lo:y], cuts=[first + lo] if cut else (), first_step=first + lo, into=s)
            per.append(_state(s))
            lo = y
        cuts = [first + a for a, (_, cut) in zip([0] + [e for e, _ in folds[:-1]], folds) if cut]
        assert per[-1] == _state(CM.fold(h, cfg, cuts=cuts, first_step=first))  # (the model itself is split-invariant)
        want.append(per)
    return want


def _build_exe(tmp_path, extra=()):
    exe = str(tmp_path / "candle_fold_test")
    res = subprocess.run([_cxx(), "-std=c++17", "-O2", *extra, os.path.join(ROOT, "tests", "cpp", "candle_fold_test.cpp"), "-o", exe],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return exe


def test_candle_fold_hpp_equals_the_model_over_edge_series_random_series_and_splits(tmp_path):
    exe = _build_exe(tmp_path)
    rng = np.random.default_rng(31)
    cases = []
    for q, (W, N) in enumerate(CONFIGS):
        cfg = CM.config(W, N)
        first = 3 * W + W // 2 + (1 if W > 1 else 0) if W < 1000 else (1 << 33) + 11  # not a multiple of W (W > 1)
        assert W == 1 or first % W
        # the edge series, every fold a single step
        h = _edge_hist()
        cases.append((h, cfg, first, [(i + 1, 0) for i in range(len(h))]))
        # a random series at the fold lengths the issue names, one after the other, with two cuts
        h = _random_hist(rng, sum(FOLD_LENGTHS), wide=q % 2 == 1)
        cases.append((h, cfg, first + 1, [(int(e), 1 if i in (2, 5) else 0) for i, e in enumerate(np.cumsum(FOLD_LENGTHS))]))
        # random splits
        n = int(rng.integers(2, 300))
        h = _random_hist(rng, n, wide=q % 2 == 0, p_one_sided=0.2)
        ends = sorted(set(int(x) for x in rng.integers(1, n + 1, size=int(rng.integers(1, 9)))) | {n})
        cases.append((h, cfg, first + 2, [(e, int(rng.integers(0, 4) == 0)) for e in ends]))
    want = _expect(cases)
    n_steps = sum(len(c[0]) for c in cases)
    one_sided = sum(int(np.sum((c[0][:, 1] == 0) | (c[0][:, 2] == MAXU))) for c in cases)
    assert 0.05 < one_sided / n_steps < 0.3
    # what the cases must hold to say anything: bars skipped, bars continued over folds, a wrapped sum, both signs
    w34 = want[3 * CONFIGS.index((3, 4)) + 1][-1][0]
    assert all(r[F["n_steps"]] for r in w34) and min(r[F["first_step"]] for r in w34) > sum(FOLD_LENGTHS) - 4 * 3, "(3, 4): early bars left"
    w100 = want[3 * CONFIGS.index((100, 2)) + 1]
    assert any(r[F["n_steps"]] == 100 for words, _ in w100 for r in words), "(100, 2): a bar completed over several folds"
    exact = CM.fold(cases[3 * CONFIGS.index((1 << 20, 1))][0], CM.config(1 << 20, 1))
    assert max(b["sum_d2"] for b in exact["bars"].values()) >> 64, "a sum that wraps modulo 2^64 is among the cases"
    for q, per in enumerate(want[1::3]):
        assert [r for r in per[-1][0] if r[F["n_steps"]]]
        if CONFIGS[q][1] > 1:  # (a single slot shows seven bars in all)
            assert any(r[F["sum_d"]] >> 63 for words, _ in per for r in words) and any(0 < r[F["sum_d"]] < TWO for words, _ in per for r in words), q
    _write_case(tmp_path, cases, want)
    args = [exe, str(tmp_path / "records.txt"), str(tmp_path / "expected.txt")]
    run = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip().endswith(f"candle_fold ok {len(cases)} series {n_steps} steps {sum(len(c[3]) for c in cases)} folds")
    # a wrong expectation is really caught, by name: one word of a bar, one carry bit
    s5 = 3 * CONFIGS.index((5, 64)) + 1
    slot = next(i for i, r in enumerate(want[s5][2][0]) if r[F["n_steps"]])
    want[s5][2][0][slot][F["sum_abs_d"]] += 1
    _write_case(tmp_path, cases, want)
    run = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert run.returncode == 1 and f"series {s5} fold 2 (lanes): slot {slot} word 13 " in run.stdout, run.stdout
    assert f"series {s5} fold 2 (serial): slot {slot} word 13 " in run.stdout
    want[s5][2][0][slot][F["sum_abs_d"]] -= 1
    want[s5][4] = (want[s5][4][0], want[s5][4][1] ^ 1)
    _write_case(tmp_path, cases, want)
    run = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert run.returncode == 1 and f"series {s5} fold 4 (lanes): carry is " in run.stdout and f"series {s5} fold 4 (serial): carry is " in run.stdout


def test_candle_fold_hpp_under_the_address_and_undefined_behaviour_sanitizers(tmp_path):
    """the same program built once with -fsanitize=address,undefined, run on its own over a short case"""
    exe = _build_exe(tmp_path, ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    rng = np.random.default_rng(37)
    cases = [(_random_hist(rng, 70, wide=True), CM.config(3, 4), 7, [(i + 1, 0) for i in range(70)]),
             (_random_hist(rng, 150), CM.config(64, 4), 65, [(1, 0), (66, 0), (150, 1)]),
             (_edge_hist(), CM.config(1, 256), 5, [(3, 0), (4, 0), (69, 0)]),
             (_random_hist(rng, 130, wide=True), CM.config(1 << 20, 1), (1 << 33) + 11, [(63, 0), (64, 0), (130, 0)])]
    _write_case(tmp_path, cases, _expect(cases))
    run = subprocess.run([exe, str(tmp_path / "records.txt"), str(tmp_path / "expected.txt")], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "candle_fold ok 4 series" in run.stdout, run.stdout + run.stderr
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr


def series_identities(rows, series, tag=""):
    """rows: CANDLE_DTYPE [n_books, N] whose bars cover the whole run; series: the series rows over the same steps and cuts"""
    for n in SUMMED:
        got = rows[n].astype(np.uint64).sum(axis=1, dtype=np.uint64)  # (modulo 2^64, as the series' own word)
        assert (got == series[n].astype(np.uint64)).all(), (tag, n, got, series[n])
    assert (rows["high_m"].max(axis=1) == series["max_m"]).all(), tag
    low = np.where(rows["n_two_sided"] > 0, rows["low_m"], np.uint64(M64))
    assert (low.min(axis=1) == series["min_m"]).all(), tag
    assert (rows["max_abs_d"].max(axis=1) == series["max_abs_d"]).all(), tag


def test_the_bars_sum_to_the_series_models_row():
    rng = np.random.default_rng(41)
    for q, (h, cuts, (W, N), first) in enumerate([(_random_hist(rng, 300), (), (7, 64), 0), (_random_hist(rng, 300, wide=True), (40, 41, 200), (1, 512), 0),
                                                  (_random_hist(rng, 120, p_one_sided=0.4), (13, 77), (64, 4), 10), (_hist(HAND), (4,), (2, 4), 0)]):
        assert N * W >= len(h) + first % W
        two = (h[:, 1] != 0) & (h[:, 2] != MAXU)
        d = np.diff(h[:, 1].astype(np.int64) + h[:, 2].astype(np.int64))[two[1:] & two[:-1]]
        assert not two.all() and (d > 0).any() and (d < 0).any(), q  # one-sided steps, returns of both signs
        rows = CM.table(CM.fold(h, CM.config(W, N), cuts=cuts, first_step=first))[None]
        ser = np.array([SM.row(SM.fold(h, cuts=cuts, first_step=first))], dtype=SM.SERIES_DTYPE)
        assert int(ser["n_ret"][0]) > 0 and (rows["n_steps"] > 0).sum() >= min(2, len(h) // W)
        series_identities(rows, ser, q)


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
    # the table has no fold or clear entry of its own and no flag bit
    assert sorted(re.findall(r"\bbk_\w*candles\w*(?=\()", header)) == sorted(ENTRIES)
    taken = [int(v) for v in re.findall(r"#define BK_FLAG_\w+ (\d+)u", header)]
    assert len(taken) == len(set(taken)) and sorted(taken) == sorted(_lib.FLAG_NAMES) == [1 << i for i in range(10)], taken
    assert "CANDLE" not in " ".join(re.findall(r"#define BK_FLAG_(\w+)", header))
    for method in ("enable_candles", "candles", "candles_view", "candles_device_ptr", "candles_config", "candles_latest", "fold_series",
                   "clear_series", "run_series"):
        assert callable(getattr(bourse_amd.ManyBookEnv, method)), method
        assert getattr(bourse_amd.ManyMarketEnv, method) is getattr(bourse_amd.ManyBookEnv, method), method
    assert bourse_amd.CANDLE_FIELDS is _lib.CANDLE_FIELDS and bourse_amd.CANDLE_DTYPE is _lib.CANDLE_DTYPE
    assert bourse_amd.CANDLE_FIELDS == CM.FIELDS and bourse_amd.CANDLE_DTYPE == CM.CANDLE_DTYPE and bourse_amd.CANDLE_DTYPE.itemsize == 128
    assert bourse_amd.candle_series is _lib.candle_series
    # the header names the words in their order
    doc = header[header.index("per-book candle table"):header.index("int bk_candles_enable(")]
    at = [re.search(r"\b" + str(i) + r"  " + n + r"\b", doc) for i, n in enumerate(CM.FIELDS)]
    assert all(at) and [m.start() for m in at] == sorted(m.start() for m in at)
    hpp = open(os.path.join(ROOT, "include", "bourse_amd.hpp")).read()
    for method in ("enable_candles", "candles", "candles_config", "candles_device_ptr"):
        assert re.search(r"\b" + method + r"\(", hpp), method
    rs = open(os.path.join(ROOT, "integration", "rust", "bourse_amd_sys.rs")).read()
    assert re.search(r"pub fn bk_candles_enable\(env: \*mut BkEnv, width: u32, n_candles: u32\) -> c_int;", rs)
    assert re.search(r"pub fn bk_candles_config_get\(env: \*mut BkEnv, out: \*mut u32\) -> c_int;", rs)
    assert re.search(r"pub fn bk_candles_device_ptr\(env: \*mut BkEnv, out: \*mut \*mut c_void\) -> c_int;", rs)
    assert re.search(r"pub fn bk_get_candles\(env: \*mut BkEnv, first_book: u32, n_books: u32, out: \*mut u64\) -> c_int;", rs)
    # the enum of candle_fold.hpp is the same order
    fold = open(os.path.join(CSRC, "candle_fold.hpp")).read()
    words = re.search(r"enum Word : uint32_t \{[^\n]*\n(.*?)\};", fold, flags=re.S).group(1)
    assert [w.strip().split(" ")[0].lower() for w in words.replace("\n", " ").split(",")] == list(CM.FIELDS) + ["row_words"]


def test_a_null_env_is_refused_not_dereferenced():
    from bourse_amd import _lib

    L = _lib.load()
    out = ctypes.c_void_p()
    cfg = (ctypes.c_uint32 * 2)()
    rows = np.zeros((1, 4, 16), dtype=np.uint64)
    calls = {
        "bk_candles_enable": lambda: L.bk_candles_enable(None, 5, 4),
        "bk_candles_config_get": lambda: L.bk_candles_config_get(None, cfg),
        "bk_candles_device_ptr": lambda: L.bk_candles_device_ptr(None, ctypes.byref(out)),
        "bk_get_candles": lambda: L.bk_get_candles(None, 0, 1, rows.ctypes.data_as(ctypes.c_void_p)),
    }
    assert set(calls) == set(ENTRIES)
    for name, call in calls.items():
        L.bk_device_count(ctypes.byref(ctypes.c_int(0)))  # (anything that may leave another message behind)
        assert call() == BK_INVALID_ARGUMENT, name
        assert b"null env" in L.bk_last_error(), name


def _functions(hip):
    return {m.group(1): fn for fn in re.split(r"\n(?=(?:static )?[\w:]+ \w+\([^;]*\) \{)", hip)
            for m in [re.match(r"(?:static )?[\w:]+ (\w+)\(", fn)] if m}


def test_the_kernels_are_plain_namespaced_and_launched_only_beside_the_series():
    """bkd::candles kernels are not among the names profiles/kernel_isa_baseline.json lists, so it stays as it is; the fold
    is plain C++ and builtins and shares its rules and lane mapping with the CPU test through candle_fold.hpp;
    bourse_amd.hip launches it only from the series' two launchers and the enable's clear, each behind the test of the
    table's rows and behind the depth table's block; the HistTable registry is as it was."""
    src = open(os.path.join(CSRC, "candles.hpp")).read()
    code = re.sub(r"//.*", "", src)
    assert re.search(r"namespace bkd \{\s*namespace candles \{", code)
    for k in ("k_fold", "k_clear"):
        assert re.search(r"__global__[^;{]*\b" + k + r"\(", code), k
    assert "asm" not in code and "tomic" not in code and "__shared__" not in code
    assert "series::" not in code and "depth::" not in code and "reinterpret_cast" not in code
    assert '#include "candle_fold.hpp"' in src and '#include "hist_ring.hpp"' in src
    assert "__builtin_amdgcn_fence" not in code and "g.mask" not in code and code.count("ring::masked_book(") == 1
    for f in ("seg_of(", "tail_of(", "scan_round(", "merged_row(", "skipped(", "next_pass(", "term(", "word_of(", "slot_of(", "ring::record(",
              "ring::masked_book(", "wave_sync()"):
        assert f in code, f
    fold = open(os.path.join(CSRC, "candle_fold.hpp")).read()
    assert re.search(r"namespace bkd \{\s*namespace candles \{", fold)
    assert "hip_runtime" not in fold and "asm" not in re.sub(r"//.*", "", fold)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_isa_counts as K
    import json

    base = json.load(open(K.BASELINE))["kernels"]
    assert not [k for k in base if "candles" in k or "k_fold" in k]
    hip = re.sub(r"//.*", "", open(os.path.join(CSRC, "bourse_amd.hip")).read())
    fns = _functions(hip)
    assert [n for n, fn in fns.items() if "candles::k_fold," in fn] == ["launch_series_fold"] and hip.count("candles::k_fold,") == 1
    assert sorted(n for n, fn in fns.items() if "candles::k_clear," in fn) == ["bk_candles_enable", "launch_series_clear"]
    for name, kernel in (("launch_series_fold", "k_fold,"), ("launch_series_clear", "k_clear,")):
        fn = fns[name]
        assert fn.index("series::" + kernel) < fn.index("depth::" + kernel) < fn.index("if (env->candle_rows.p) {") < fn.index("candles::" + kernel), name
    assert "tables[T_SERIES].seen" in fns["launch_series_fold"]
    assert "enum { T_SERIES, T_LAGS, T_BINS, N_HIST_TABLES };" in hip
    enable = fns["bk_candles_enable"]
    order = [enable.index(x) for x in ("tables[T_SERIES].on", "bk_series_enable", "already enabled", "width must be", "n_candles must be",
                                       "table_fold(env, T_SERIES)", ".alloc(", "candles::k_clear,", "candle_rows.swap(")]
    assert order == sorted(order), order
    for name in ("bk_candles_config_get", "bk_candles_device_ptr", "bk_get_candles"):
        assert fns[name][fns[name].index("{"):].lstrip("{\n ").startswith("if (int rc = candles_ok(env)) return rc;"), name
    assert '"this env has no candle table: call bk_candles_enable first"' in fns["candles_ok"]


def test_the_built_candle_kernels_use_no_scratch_and_no_lds():
    """the built library's metadata, read with llvm-readelf: no scratch (the parts stay in registers), no LDS allocation
    (the shuffles are ds_bpermute, which needs none)"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_isa_counts as K
    from bourse_amd import _build

    lib = _build.build()
    meta = {}
    with tempfile.TemporaryDirectory(prefix="bourse_candles_isa_") as tmp:
        for co in K.code_objects(lib, tmp):
            txt = subprocess.run([K._tool("llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
            for blk in re.split(r"\n\s+- \.agpr_count:", txt):
                name = re.search(r"\.name:\s+(\S+)", blk)
                if name and "7candles" in name.group(1):
                    meta[name.group(1)] = {k: int(v) for k, v in re.findall(
                        r"\.(private_segment_fixed_size|group_segment_fixed_size|vgpr_count|sgpr_count):\s+(\d+)", blk)}
    assert len(meta) == 2 and any("k_fold" in n for n in meta) and any("k_clear" in n for n in meta), meta
    for name, m in meta.items():
        assert m["private_segment_fixed_size"] == 0 and m["group_segment_fixed_size"] == 0, (name, m)
        assert m["vgpr_count"] <= 128, (name, m)


def test_candle_series_against_numpy_on_the_models_rows():
    from bourse_amd import candle_series

    rng = np.random.default_rng(43)
    W, N, n, first = 7, 8, 45, 19  # bars 2 .. 9: bar 2 partial (steps 19, 20), bar 9 partial (step 63), bars 0, 1 never seen
    hists = [_random_hist(rng, n, p_one_sided=0.0), _random_hist(rng, n, p_one_sided=0.5)]
    hists[1][[0, 1, 44], 1] = 0  # bars 2 and 9 of the second book have no two-sided step
    rows = np.array([CM.table(CM.fold(h, CM.config(W, N), first_step=first)) for h in hists], dtype=CM.CANDLE_DTYPE)
    assert rows["first_step"][0].tolist() == [56, 63, 19, 21, 28, 35, 42, 49] and rows["n_steps"][0].tolist() == [7, 1, 2, 7, 7, 7, 7, 7]
    got = candle_series(rows, W)
    assert got.shape == (2, N) and got.dtype.names == ("open", "high", "low", "close", "twap", "mean_spread", "volume", "trade_share",
                                                       "realized_var", "bar", "complete")
    assert got["bar"][0].tolist() == list(range(2, 10)) and got["complete"][0].tolist() == [False] + [True] * 6 + [False]
    for b, h in enumerate(hists):
        h = h.astype(np.float64)
        two = (h[:, 1] != 0) & (h[:, 2] != MAXU)
        mid = (h[:, 1] + h[:, 2]) / 2.0
        d = np.diff(mid)
        ret = two[1:] & two[:-1]
        for k, bar in enumerate(range(2, 10)):
            lo, hi = max(bar * W, first) - first, min((bar + 1) * W, first + n) - first
            t = two[lo:hi]
            want = {"volume": h[lo:hi, 0].sum(), "trade_share": (h[lo:hi, 0] > 0).mean()}
            if t.any():
                m = mid[lo:hi][t]
                want.update(open=m[0], high=m.max(), low=m.min(), close=m[-1], twap=m.mean(), mean_spread=(h[lo:hi, 2] - h[lo:hi, 1])[t].mean())
            r = np.array([ret[s - 1] if s >= 1 else False for s in range(lo, hi)])
            if r.any():
                want["realized_var"] = (np.array([d[s - 1] for s in range(lo, hi) if s >= 1 and ret[s - 1]]) ** 2).sum()
            for name in got.dtype.names[:9]:
                if name in want:
                    assert np.isclose(got[name][b, k], want[name], rtol=1e-12, atol=0), (b, bar, name, got[name][b, k], want[name])
                else:
                    assert np.isnan(got[name][b, k]), (b, bar, name)
    assert np.isnan(got["open"][1]).any() and not np.isnan(got["open"][0]).any(), "a bar without a two-sided step is among the cases"
    # an empty slot: bar -1, first in the order, every value NaN, not complete
    few = candle_series(CM.table(CM.fold(hists[0][:10], CM.config(W, N), first_step=first)), W)
    assert few.shape == (1, N) and few["bar"][0].tolist() == [-1] * 5 + [2, 3, 4] and not few["complete"][0, :5].any()
    assert all(np.isnan(few[name][0, :5]).all() for name in few.dtype.names[:9]) and few["complete"][0].tolist()[5:] == [False, True, False]
    empty = candle_series(np.zeros((3, 4), dtype=CM.CANDLE_DTYPE), 5)
    assert (empty["bar"] == -1).all() and all(np.isnan(empty[name]).all() for name in empty.dtype.names[:9])
    with pytest.raises(ValueError):
        candle_series(np.zeros((2, 4, 16), dtype=np.uint64), 5)
    with pytest.raises(ValueError):
        candle_series(rows, 0)
