"""The per-book bin table (bk_bins_enable) without a GPU: the plain-Python model against tables worked out by hand, the
kernel's bin rules, span partners and carry (bourse_amd/csrc/bin_fold.hpp, compiled with g++ into a program of its own)
against the model over random splits, the totals against the lag table's and the series' models, the C ABI - the entries
are exported, bound and declared, refuse a null env, and bk_bins_config is nine u32 - the layout of the kernel's source and
of its launches, and bin_edges / bin_quantiles against numpy."""
import ctypes
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import bins_model as BM
import lags_model as LM
import series_model as SM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("bk_bins_enable", "bk_bins_config_get", "bk_bins_fold", "bk_bins_clear", "bk_bins_clear_device", "bk_bins_device_ptr",
           "bk_get_bins")
BK_INVALID_ARGUMENT = 5
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
        pytest.fail("no host C++ compiler (g++, c++, clang++ or hipcc): bin_fold.hpp cannot be checked")


def _hist(quotes, tv=None):
    """(bid, ask) per step, and trade_vol, as an [n_steps, 5] history: only words 0 .. 2 are read"""
    h = np.zeros((len(quotes), 5), dtype=np.uint64)
    h[:, 1:3] = np.array(quotes, dtype=np.uint64).reshape(-1, 2)
    if tv is not None:
        h[:, 0] = tv
    return h


def _row(B, **at):
    r = [0] * B
    for i, c in at.items():
        r[int(i[1:])] = c
    return r


HAND = [(0, MAXU), (100, MAXU), (100, 104), (102, 104), (100, 104), (100, 104)]  # steps 2..5: m = 204, 206, 204, 204
HAND_TV = [0, 0, 3, 0, 9, 1]


def test_the_model_against_tables_worked_out_by_hand():
    # spans (1, 3), B = 8, widths (1, 1, 2).  span 1: +2, -2, 0 at steps 3, 4, 5 -> bins 6, 2, 4.  span 3: 204 - 204 at step
    # 5 -> bin 4.  spread: 4, 2, 4, 4.  volume / 2: 0, 0, 1, 0, 4, 0
    cfg = BM.config((1, 3), 8, 1, 1, 2)
    s = BM.fold(_hist(HAND, HAND_TV), cfg)
    want = [_row(8, b2=1, b4=1, b6=1), _row(8, b4=1), _row(8, b2=1, b4=3), _row(8, b0=4, b1=1, b4=1)]
    assert BM.counts(s) == want
    assert BM.carry(s) == [TWO | 204, TWO | 204, TWO | 206]
    t = BM.table(s)
    assert t.dtype == np.uint64 and t.shape == (4, 8)
    # the same in two folds, split anywhere, is the same table and carry
    for y in range(1, 6):
        part = BM.fold(_hist(HAND, HAND_TV)[y:], first_step=y, into=BM.fold(_hist(HAND, HAND_TV)[:y], cfg))
        assert (BM.counts(part), BM.carry(part)) == (BM.counts(s), BM.carry(s)), y
    # a cut in front of step 4 (a reset there): step 4 has no past, step 5 a return of 0 and nothing three steps back
    c = BM.fold(_hist(HAND, HAND_TV), cfg, cuts=[4])
    assert BM.counts(c) == [_row(8, b4=1, b6=1), _row(8), want[2], want[3]]
    assert BM.carry(c) == [TWO | 204, TWO | 204, 0]
    # a one-sided step in the middle: span 2 reaches over it (only the end points count), span 1 never has both ends
    g = BM.fold(_hist([(10, 20), (0, 20), (12, 22)]), BM.config((2, 1), 4))
    assert BM.counts(g) == [_row(4, b3=1), _row(4), _row(4, b3=2), _row(4, b0=3)]  # h = +4 clamps into the end bin; spread 10
    assert BM.carry(g) == [TWO | 34, 0]
    assert BM.counts(BM.cleared(cfg)) == [[0] * 8] * 4 and BM.carry(BM.cleared(cfg)) == [0, 0, 0]
    # h = -1, -3, -4 at width 3: a true floor, bins B/2 - 1, B/2 - 1, B/2 - 2 (truncation would give B/2, B/2 - 1, B/2 - 1)
    for h, b in ((-1, 3), (-3, 3), (-4, 2), (0, 4), (2, 4), (3, 5)):
        f = BM.fold(_hist([(50, 54), (50, 54 + h)]), BM.config((1,), 8, 3))
        assert BM.counts(f)[0] == _row(8, **{f"b{b}": 1}), (h, b)
    # the jump from (1, 2) to (0xFFFFFFFD, 0xFFFFFFFE) and back: |h| = 2^33 - 8 is clamped into the end bins, at width 1 and
    # at the widest width, where floor(h / w) is +1 and -2
    for w, B in ((1, 256), (MAXU, 2), (MAXU, 8)):
        j = BM.fold(_hist([(1, 2), (0xFFFFFFFD, 0xFFFFFFFE), (1, 2)]), BM.config((1, 2), B, w, MAXU, 1))
        up = B - 1 if w == 1 or B == 2 else B // 2 + 1
        down = 0 if w == 1 or B == 2 else B // 2 - 2
        assert BM.counts(j)[0] == _row(B, **{f"b{up}": 1, f"b{down}": 1}), (w, B)
        assert BM.counts(j)[1] == _row(B, **{f"b{B // 2}": 1}) and BM.counts(j)[2] == _row(B, b0=3)
        assert BM.carry(j) == [TWO | 3, TWO | ((1 << 33) - 5)]


def _edge_series(rng, n):
    """jumps between the two ends of the price range, empty sides, crossed quotes (a wrapping spread) and huge volumes"""
    out = [(1, 2), (0xFFFFFFFD, 0xFFFFFFFE), (1, 2), (1, 0xFFFFFFFE), (0xFFFFFFFE, 0xFFFFFFFE), (0, MAXU), (0, 7), (7, MAXU), (MAXU, 0),
           (9, 3)]
    while len(out) < n:
        out.append((1, int(rng.integers(2, 9))) if rng.integers(0, 2) else (0xFFFFFFFD, 0xFFFFFFFE))
    return [(int(rng.integers(0, 1 << 32)) if rng.integers(0, 2) else int(rng.integers(0, 3)), b, a) for b, a in out]


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
        out.append((int(rng.integers(0, 40)) if rng.random() < 0.6 else 0, bid, ask))
    return out


def _rec_hist(recs):
    h = np.zeros((len(recs), 5), dtype=np.uint64)
    h[:, :3] = np.array(recs, dtype=np.uint64).reshape(-1, 3)
    return h


def _write_case(tmp_path, series, cfgs, ends, want):
    with open(tmp_path / "records.txt", "w") as f:
        f.write(f"{len(series)}\n")
        for recs, c, e in zip(series, cfgs, ends):
            head = [len(recs), c["n_bins"], len(c["spans"])] + list(c["spans"]) + [c["ret_width"], c["spread_width"], c["vol_width"]]
            f.write(" ".join(str(x) for x in head + [len(e)] + list(e)) + "\n")
            for r in recs:
                f.write(f"{r[0]} {r[1]} {r[2]}\n")
    with open(tmp_path / "expected.txt", "w") as f:
        for per_series in want:
            for counts, carry in per_series:
                for w in counts:
                    f.write(" ".join(str(x) for x in w) + "\n")
                f.write(" ".join(str(x) for x in carry) + "\n")


CFGS = [BM.config((1,), 64), BM.config((1, 5, 20, 64), 256), BM.config((64, 1, 5), 64, 3, 2, 7), BM.config((3, 3), 2),
        BM.config((2, 63), 16, MAXU, MAXU, MAXU), BM.config((7,), 10, 2, 1, 1)]


def _build_exe(tmp_path, extra=()):
    exe = str(tmp_path / "bin_fold_test")
    res = subprocess.run([_cxx(), "-std=c++17", "-O2", *extra, os.path.join(ROOT, "tests", "cpp", "bin_fold_test.cpp"), "-o", exe],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return exe


def test_bin_fold_hpp_equals_the_model_over_random_splits(tmp_path):
    exe = _build_exe(tmp_path)
    rng = np.random.default_rng(23)
    series, cfgs, ends = [], [], []
    # per configuration: an edge series folded step by step, and one cut at the lengths the kernel's paths turn on
    for c in CFGS:
        series.append(_edge_series(rng, 90))
        cfgs.append(c)
        ends.append(list(range(1, 91)))  # every fold a single step
        n = 1 + 64 + 65 + 3 + 130 + 2 + 200
        series.append(_random_series(rng, n, wide=c["ret_width"] > 100))
        cfgs.append(c)
        ends.append([int(x) for x in np.cumsum([1, 64, 65, 3, 130, 2, 200])])  # below Kmax, exactly 64, 65, above 128
    series += [[(4, 5, 9)], [(0, 0, MAXU)], [(1, 5, 9), (0, 6, 9)]]
    cfgs += [CFGS[1], CFGS[2], CFGS[0]]
    ends += [[1], [1], [2]]
    for q in range(26):
        n = int(rng.integers(2, 420))
        series.append(_random_series(rng, n, wide=q % 5 == 0))
        cfgs.append(CFGS[q % len(CFGS)])
        e = [n] if q % 4 == 0 else sorted(set(int(x) for x in rng.integers(1, n + 1, size=int(rng.integers(1, 9)))) | {n})
        ends.append(e)
    want, n_one_sided, n_steps = [], 0, 0
    for recs, c, e in zip(series, cfgs, ends):
        h = _rec_hist(recs)
        n_steps += len(h)
        n_one_sided += int(np.sum((h[:, 1] == 0) | (h[:, 2] == MAXU)))
        s, lo, per = BM.cleared(c), 0, []
        for y in e:
            s = BM.fold(h[lo:y], first_step=lo, into=s)
            per.append((BM.counts(s), BM.carry(s)))
            lo = y
        one = BM.fold(h, c)
        assert per[-1] == (BM.counts(one), BM.carry(one))  # (the model itself is split-invariant)
        want.append(per)
    assert len(series) > 30 and 0.05 < n_one_sided / n_steps < 0.2
    lens = [b - a for e in ends for a, b in zip([0] + e[:-1], e)]
    assert 1 in lens and 64 in lens and 65 in lens and 130 in lens and 200 in lens and any(x < 5 for x in lens)
    deep = want[3][-1][0]  # the four-span configuration over 465 steps: span 64 has counts, inner and end bins are hit
    assert cfgs[3]["spans"] == (1, 5, 20, 64) and sum(deep[3]) > 200 and sum(deep[0][1:-1]) > 200
    assert want[0][-1][0][0][0] > 0 and want[0][-1][0][0][63] > 0, "the edge series clamps into both end bins"
    _write_case(tmp_path, series, cfgs, ends, want)
    args = [exe, str(tmp_path / "records.txt"), str(tmp_path / "expected.txt")]
    run = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip().endswith(f"bin_fold ok {len(series)} series {n_steps} steps {sum(len(e) for e in ends)} folds")
    # a wrong expectation is really caught: one count off by one, and one carry word
    want[3][2][0][3][128] += 1
    _write_case(tmp_path, series, cfgs, ends, want)
    run = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert run.returncode == 1 and "series 3 fold 2 (lanes): channel 3 bin 128 " in run.stdout and "(serial): channel 3 bin 128 " in run.stdout
    want[3][2][0][3][128] -= 1
    want[3][3][1][63] ^= 1
    _write_case(tmp_path, series, cfgs, ends, want)
    run = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert run.returncode == 1 and "series 3 fold 3 (lanes): carry 63 " in run.stdout and "(serial): carry 63 " in run.stdout


def test_bin_fold_hpp_under_the_address_and_undefined_behaviour_sanitizers(tmp_path):
    """the same program built once with -fsanitize=address,undefined, run on its own over a short case"""
    exe = _build_exe(tmp_path, ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    rng = np.random.default_rng(29)
    series = [_edge_series(rng, 70), _random_series(rng, 150, False)]
    cfgs = [CFGS[1], CFGS[4]]
    ends = [list(range(1, 71)), [1, 66, 150]]
    want = []
    for recs, c, e in zip(series, cfgs, ends):
        s, lo, per = BM.cleared(c), 0, []
        for y in e:
            s = BM.fold(_rec_hist(recs)[lo:y], first_step=lo, into=s)
            per.append((BM.counts(s), BM.carry(s)))
            lo = y
        want.append(per)
    _write_case(tmp_path, series, cfgs, ends, want)
    run = subprocess.run([exe, str(tmp_path / "records.txt"), str(tmp_path / "expected.txt")], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "bin_fold ok 2 series" in run.stdout, run.stdout + run.stderr
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr


def test_the_totals_are_the_lag_tables_and_the_series_counts():
    rng = np.random.default_rng(5)
    for q, (recs, cuts) in enumerate([(_random_series(rng, 300, False), ()), (_random_series(rng, 300, True), (40, 41, 200)),
                                      (_edge_series(rng, 120), (3, 77)),
                                      ([(t, b, a) for t, (b, a) in zip(HAND_TV, HAND)], (4,))]):
        h = _rec_hist(recs)
        ser = dict(zip(SM.FIELDS, SM.words(SM.fold(h, cuts=cuts))))
        lag = LM.words(LM.fold(h, 64, cuts=cuts))
        for spans, B, w in (((1, 5, 20, 64), 256, 1), ((64, 2), 2, 9), ((3, 3, 7), 128, 1)):
            c = BM.counts(BM.fold(h, BM.config(spans, B, w, 3, 5), cuts=cuts))
            for j, k in enumerate(spans):
                assert sum(c[j]) == lag[k - 1][LM.FIELDS.index("n_h")], (q, spans, k)
            assert sum(c[len(spans)]) == ser["n_two_sided"] and sum(c[len(spans) + 1]) == ser["n_steps"] == len(recs), (q, spans)
            if w == 1 and q in (0, 3):  # narrow quotes: nothing is clamped, so the first moment is the lag table's sum_h
                for j, k in enumerate(spans):
                    assert c[j][0] == 0 and c[j][B - 1] == 0, (q, spans, k)
                    first = sum((i - B // 2) * n for i, n in enumerate(c[j]))
                    assert first & ((1 << 64) - 1) == lag[k - 1][LM.FIELDS.index("sum_h")], (q, spans, k)
        assert ser["n_two_sided"] > 0


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
    assert "BIN" not in " ".join(re.findall(r"#define BK_FLAG_(\w+)", header))
    for method in ("enable_bins", "fold_bins", "bins", "bins_config", "bins_device_ptr", "bins_view", "clear_bins", "run_series"):
        assert callable(getattr(bourse_amd.ManyBookEnv, method)), method
        assert getattr(bourse_amd.ManyMarketEnv, method) is getattr(bourse_amd.ManyBookEnv, method), method
    assert bourse_amd.ManyBookEnv.BINS_CONFIG_DTYPE is _lib.BINS_CONFIG_DTYPE is bourse_amd.BINS_CONFIG_DTYPE
    assert bourse_amd.bin_edges is _lib.bin_edges and bourse_amd.bin_quantiles is _lib.bin_quantiles
    hpp = open(os.path.join(ROOT, "include", "bourse_amd.hpp")).read()
    for method in ("enable_bins", "fold_bins", "bins", "bins_config", "bins_device_ptr", "clear_bins"):
        assert re.search(r"\b" + method + r"\(", hpp), method
    # the Rust FFI file is the generator's output for this header: the seven entries, and the config field by field
    rs = open(os.path.join(ROOT, "integration", "rust", "bourse_amd_sys.rs")).read()
    for name in ENTRIES:
        assert re.search(r"pub fn " + name + r"\(", rs), name
    assert re.search(r"pub fn bk_bins_enable\(env: \*mut BkEnv, cfg: \*const BkBinsConfig\) -> c_int;", rs)
    assert re.search(r"pub fn bk_get_bins\(env: \*mut BkEnv, first_book: u32, n_books: u32, out: \*mut u64\) -> c_int;", rs)
    body = re.search(r"pub struct BkBinsConfig \{(.*?)\}", rs, flags=re.S).group(1)
    assert re.findall(r"pub (\w+): ([\w\[\]; ]+),", body) == [("n_bins", "u32"), ("n_spans", "u32"), ("spans", "[u32; 4]"),
                                                             ("ret_width", "u32"), ("spread_width", "u32"), ("vol_width", "u32")]


def test_bk_bins_config_is_nine_u32_laid_out_as_the_dtype(tmp_path):
    from bourse_amd import _lib

    dt = _lib.BINS_CONFIG_DTYPE
    names = ("n_bins", "n_spans", "spans", "ret_width", "spread_width", "vol_width")
    assert dt.itemsize == 36 and dt.names == names
    assert [dt.fields[n][1] for n in names] == [0, 4, 8, 24, 28, 32] and dt.fields["spans"][0].shape == (4,)
    src = tmp_path / "layout.cpp"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "bourse_amd.h"\n'
                   'int main() { std::printf("%zu", sizeof(bk_bins_config));\n' +
                   "".join(f'std::printf(" %zu", offsetof(bk_bins_config, {n}));\n' for n in names) +
                   'std::printf(" %zu", sizeof(static_cast<bk_bins_config*>(nullptr)->spans));\nreturn 0; }\n')
    exe = str(tmp_path / "layout")
    res = subprocess.run([_cxx(), "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60).stdout.split()
    assert [int(x) for x in out] == [36, 0, 4, 8, 24, 28, 32, 16]


def test_a_null_env_is_refused_not_dereferenced():
    from bourse_amd import _lib

    L = _lib.load()
    mask = (ctypes.c_uint8 * 4)(1, 0, 1, 0)
    out = ctypes.c_void_p()
    cfg = np.array([64, 1, 1, 0, 0, 0, 1, 1, 1], dtype=np.uint32)
    rows = np.zeros((4, 3, 64), dtype=np.uint64)
    calls = {
        "bk_bins_enable": lambda: L.bk_bins_enable(None, cfg.ctypes.data_as(ctypes.c_void_p)),
        "bk_bins_config_get": lambda: L.bk_bins_config_get(None, cfg.ctypes.data_as(ctypes.c_void_p)),
        "bk_bins_fold": lambda: L.bk_bins_fold(None),
        "bk_bins_clear": lambda: L.bk_bins_clear(None, ctypes.cast(mask, ctypes.c_void_p)),
        "bk_bins_clear_device": lambda: L.bk_bins_clear_device(None, ctypes.cast(mask, ctypes.c_void_p)),
        "bk_bins_device_ptr": lambda: L.bk_bins_device_ptr(None, ctypes.byref(out)),
        "bk_get_bins": lambda: L.bk_get_bins(None, 0, 1, rows.ctypes.data_as(ctypes.c_void_p)),
    }
    assert set(calls) == set(ENTRIES)
    for name, call in calls.items():
        L.bk_device_count(ctypes.byref(ctypes.c_int(0)))  # (anything that may leave another message behind)
        assert call() == BK_INVALID_ARGUMENT, name
        assert b"null env" in L.bk_last_error(), name


def test_the_kernels_stay_out_of_the_baselined_namespace_and_every_launch_sits_behind_the_guard():
    """bkd::bins kernels are not among the names tools/kernel_isa_counts.py::measure lists (those start with k_ once
    "void bkd::" is stripped), so profiles/kernel_isa_baseline.json stays as it is; the fold is plain C++ - its only atomics
    are atomicAdd on its LDS counters - and shares its bin rules, partners and carry with the CPU test through bin_fold.hpp."""
    src = open(os.path.join(ROOT, "bourse_amd", "csrc", "bins.hpp")).read()
    body = src[src.index("namespace bkd {"):]
    assert re.search(r"namespace bkd \{\s*namespace bins \{", body)
    for k in ("k_fold", "k_clear"):
        assert re.search(r"__global__[^;{]*\b" + k + r"\(", body), k
    code = re.sub(r"//.*", "", src)
    assert "asm" not in code and "series::" not in code and "lags::" not in code
    atomics = re.findall(r"\w*[aA]tomic\w*", code.replace("__ATOMIC_ACQ_REL", ""))
    assert atomics and set(atomics) == {"atomicAdd"}, atomics
    assert all(a.startswith("&cnt[") for a in re.findall(r"atomicAdd\(([^,]*),", code)), "only the LDS counters are raised atomically"
    assert re.search(r"extern __shared__ uint32_t \w+\[\];", code) and code.count("__shared__") == 1
    assert '#include "bin_fold.hpp"' in src
    for f in ("ret_bin(", "spread_bin(", "vol_bin(", "partner(", "next_carry(", "slot_of(", "word_of("):
        assert f in code, f
    fold = open(os.path.join(ROOT, "bourse_amd", "csrc", "bin_fold.hpp")).read()
    assert re.search(r"namespace bkd \{\s*namespace bins \{", fold)
    assert "hip_runtime" not in fold and "asm" not in re.sub(r"//.*", "", fold)
    # (where bourse_amd.hip launches them, and behind which guard: tests/test_hist_tables_cpu.py)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_isa_counts as K

    base = json.load(open(K.BASELINE))["kernels"]
    assert not [k for k in base if "bins" in k or "k_fold" in k]


def test_bin_edges_against_numpy_histogram_of_clipped_values():
    from bourse_amd import _lib, bin_edges

    rng = np.random.default_rng(11)
    recs = _random_series(rng, 500, wide=False)
    h = _rec_hist(recs)
    cfg = BM.config((1, 4), 16, 3, 2, 7)
    edges = bin_edges(cfg)
    assert edges.dtype == np.float64 and edges.shape == (4, 16)
    assert edges[0].tolist() == edges[1].tolist() == [(i - 8) * 1.5 for i in range(16)]
    assert edges[2].tolist() == [2.0 * i for i in range(16)] and edges[3].tolist() == [7.0 * i for i in range(16)]
    rec = np.zeros((), dtype=_lib.BINS_CONFIG_DTYPE)
    rec["n_bins"], rec["n_spans"], rec["spans"], rec["ret_width"], rec["spread_width"], rec["vol_width"] = 16, 2, (1, 4, 0, 0), 3, 2, 7
    assert (bin_edges(rec) == edges).all()  # (the record bins_config() returns gives the same edges)
    got = BM.table(BM.fold(h, cfg))
    two = (h[:, 1] != 0) & (h[:, 2] != MAXU)
    mid = (h[:, 1].astype(np.float64) + h[:, 2].astype(np.float64)) / 2
    assert not two.all()
    for j, k in enumerate((1, 4)):
        ok = two[k:] & two[:-k]
        x = (mid[k:] - mid[:-k])[ok]  # the change of the MID: the edges are in its units
        top = edges[j][-1] + 1.5
        want, _ = np.histogram(np.clip(x, edges[j][0], top - 0.25), bins=np.append(edges[j], top))
        assert want.sum() > 300 and (got[j] == want.astype(np.uint64)).all(), (k, got[j], want)
    spread = (h[:, 2] - h[:, 1])[two].astype(np.float64)
    want, _ = np.histogram(np.clip(spread, 0, edges[2][-1]), bins=np.append(edges[2], edges[2][-1] + 2))
    assert (got[2] == want.astype(np.uint64)).all()
    vol = h[:, 0].astype(np.float64)
    want, _ = np.histogram(np.clip(vol, 0, edges[3][-1]), bins=np.append(edges[3], edges[3][-1] + 7))
    assert (got[3] == want.astype(np.uint64)).all() and want[0] > 0 and want[1:].sum() > 0


def test_bin_quantiles_name_the_bin_that_holds_numpys_quantile():
    from bourse_amd import bin_edges, bin_quantiles

    rng = np.random.default_rng(13)
    qs = (0.01, 0.1, 0.25, 0.5, 0.9, 0.99, 1.0)
    for n, width in ((1000, 3), (37, 1), (5000, 7)):
        x = rng.integers(0, 60 * width, size=n)  # values as the volume channel sees them: nothing reaches the end bin's overflow
        edges = bin_edges(BM.config((1,), 64, 1, 1, width))[2]
        counts = np.bincount(x // width, minlength=64).astype(np.uint64)
        got = bin_quantiles(counts, edges, float(width), qs)
        assert got.shape == (len(qs),)
        for q, e in zip(qs, got):
            v = np.quantile(x, q, method="inverted_cdf")
            assert e - width <= v < e, (n, width, q, v, e)
        assert bin_quantiles(counts, edges, float(width), 0.5) == got[3]
    # signed values through a return channel's edges (mid-price units: the bins are ret_width / 2 wide)
    h2 = rng.integers(-40, 40, size=800)  # changes of twice the mid
    edges = bin_edges(BM.config((1,), 64, 4))[0]
    counts = np.bincount(h2 // 4 + 32, minlength=64)
    for q in qs:
        e = bin_quantiles(counts, edges, 2.0, q)
        v = np.quantile(h2 / 2.0, q, method="inverted_cdf")
        assert e - 2.0 <= v < e, (q, v, e)
    # rows of a table at once, a zero total gives NaN
    table = np.stack([counts, np.zeros(64, dtype=np.int64)])
    both = bin_quantiles(table, edges, 2.0, (0.5, 0.9))
    assert both.shape == (2, 2) and not np.isnan(both[0]).any() and np.isnan(both[1]).all()
    with pytest.raises(ValueError):
        bin_quantiles(counts, edges[:-1], 2.0, 0.5)
    with pytest.raises(ValueError):
        bin_quantiles(counts, edges, 2.0, 0.0)
