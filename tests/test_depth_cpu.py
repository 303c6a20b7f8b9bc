"""The per-level depth table (bk_depth_enable) without a GPU: the plain-Python model against a table worked out by hand,
its split-invariance and its header against the series' model, the kernel's rules and lane mapping
(bourse_amd/csrc/depth_fold.hpp, compiled with g++ into a program of its own) against the model over random histories and
splits, the C ABI - the entries are exported, bound and declared and refuse a null env - the layout of the kernel's source,
its instruction profile and resources, and depth_moments against numpy."""
import ctypes
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import depth_model as DM
import series_model as SM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bourse_amd", "csrc")
ENTRIES = ("bk_depth_enable", "bk_depth_device_ptr", "bk_get_depth")
BK_INVALID_ARGUMENT = 5
MAXU = 0xFFFFFFFF
TWO = 1 << 63
M64 = (1 << 64) - 1
LEVELS = (1, 2, 5, 16, 31, 32, 33, 64)


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
        pytest.fail("no host C++ compiler (g++, c++, clang++ or hipcc): depth_fold.hpp cannot be checked")


def _hist(steps):
    """[(bid, ask, [(bv, bn, av, an), ..]), ..] -> an [n_steps, 5 + 4 L] history: words 0, 3 and 4 are not read"""
    L = len(steps[0][2])
    h = np.zeros((len(steps), 5 + 4 * L), dtype=np.uint64)
    for i, (bid, ask, lv) in enumerate(steps):
        h[i, 1], h[i, 2] = bid, ask
        h[i, 5:] = np.array(lv, dtype=np.uint64).reshape(-1)
    return h


def _state(s):
    return DM.words(s), DM.carry(s)


def _u(x):
    return x & M64


# two levels, six steps: m = 204, 206, -, 204, 208, 208; I_0 = 3, -2, 1, 0, 5, 5; I_1 = 4, -2, 1, 2, 3, 8
HAND = [(100, 104, [(5, 1, 2, 1), (1, 1, 0, 0)]),
        (102, 104, [(1, 1, 3, 2), (0, 0, 0, 0)]),
        (0, 104, [(4, 2, 3, 1), (0, 0, 0, 0)]),      # one-sided, in the middle
        (100, 104, [(2, 1, 2, 1), (2, 1, 0, 0)]),    # J = 0 at level 0 for the pair (3, 4)
        (104, 104, [(7, 1, 2, 1), (0, 0, 2, 1)]),
        (104, 104, [(7, 1, 2, 1), (3, 1, 0, 0)])]


def test_the_model_against_a_table_worked_out_by_hand():
    s = DM.fold(_hist(HAND))
    w = DM.words(s)
    # pairs: (0, 1) d = +2, (3, 4) d = +4, (4, 5) d = 0
    assert w[2] == [6, 5, 3, 6, 6, 2, 0, 5, 6, 0, 0, 0, 0, 0, 0, 0]
    # level 0.  volumes: bid 5 1 4 2 7 7, ask 2 3 3 2 2 2; I over two-sided steps: 3, -2, 0, 5, 5
    #   pairs: J = 3, d = 2: signed, agree, move, J d = 6;  J = 0, d = 4: nothing but n_pairs;  J = 5, d = 0: signed only
    assert w[0] == [26, 14, 25 + 1 + 16 + 4 + 49 + 49, 4 + 9 + 9 + 4 + 4 + 4, 7, 7, 6, 6,
                    11, 9 + 4 + 0 + 25 + 25, 2, 2, 1, 6, 1, 15]
    # level 1.  volumes: bid 1 0 0 2 0 3, ask 0 0 0 0 2 0; I over two-sided steps: 4, -2, 2, 3, 8
    #   pairs: J = 4, d = 2: agree, J d = 8;  J = 2, d = 4: agree, J d = 8;  J = 3, d = 0: signed only
    assert w[1] == [6, 2, 1 + 4 + 9, 4, 3, 1, 3, 1, 15, 16 + 4 + 4 + 9 + 64, 3, 6, 2, 16, 2, 19]
    assert DM.carry(s) == [5, 8, TWO | 208]
    # a cut in front of step 4: the pair (3, 4) is gone, the sums of every step stay
    c = DM.fold(_hist(HAND), cuts=[4])
    wc = DM.words(c)
    assert wc[2] == [6, 5, 2, 2, 2, 1, 0, 5, 6, 0, 0, 0, 0, 0, 0, 0]
    assert wc[0][:10] == w[0][:10] and wc[0][10:] == [2, 2, 1, 6, 1, 15]  # (that pair had J = 0 at level 0)
    assert wc[1][:10] == w[1][:10] and wc[1][10:] == [2, 2, 1, 8, 1, 19]
    assert DM.carry(c) == DM.carry(s)
    # a move against the imbalance: sgn(J) d < 0, J d < 0 - two's complement words
    n = DM.words(DM.fold(_hist([(100, 104, [(1, 1, 4, 1)]), (101, 104, [(1, 1, 4, 1)])])))
    assert n[0][10:15] == [1, _u(-1), 0, _u(-3), 1] and n[0][8] == _u(-6) and n[0][15] == 6 and n[1][3:7] == [1, 1, 1, 0]
    # the last step one-sided: its imbalance is carried, its word is 0; behind a cut or a clear the whole carry is 0
    o = DM.fold(_hist(HAND[:3]))
    assert DM.carry(o) == [1, 1, 0] and DM.carry(DM.cut(o)) == [0, 0, 0] and DM.carry(DM.cleared(2)) == [0, 0, 0]
    assert DM.table(s).dtype == np.uint64 and DM.table(s).shape == (3, 16)


def _random_hist(rng, n, L, wide=False, p_one_sided=0.1):
    """a random history: narrow quotes (or jumps between the two ends of the price range), one-sided steps, and per level
    small volumes with empty levels, or volumes up to 2^32 - 1"""
    h = np.zeros((n, 5 + 4 * L), dtype=np.uint64)
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
        for q in range(L):
            for side in (0, 2):
                if rng.random() < 0.25:
                    continue
                vol = MAXU - int(rng.integers(0, 3)) if wide and rng.random() < 0.5 else int(rng.integers(1, 400))
                h[i, 5 + 4 * q + side] = vol
                h[i, 6 + 4 * q + side] = int(rng.integers(1, 9))
    return h


def test_the_model_is_split_invariant_at_every_split_point():
    rng = np.random.default_rng(3)
    for L, wide in ((1, False), (5, True), (16, False)):
        h = _random_hist(rng, 40, L, wide)
        cuts = (7, 8, 30)
        one = _state(DM.fold(h, cuts=cuts))
        for y in range(1, len(h)):
            part = DM.fold(h[y:], cuts=cuts, first_step=y, into=DM.fold(h[:y], cuts=cuts))
            assert _state(part) == one, (L, y)
        assert _state(DM.fold(_hist(HAND)[2:], first_step=2, into=DM.fold(_hist(HAND)[:2]))) == _state(DM.fold(_hist(HAND)))


def test_the_header_is_the_series_models():
    rng = np.random.default_rng(5)
    for q, (h, cuts) in enumerate([(_random_hist(rng, 300, 5), ()), (_random_hist(rng, 300, 2, wide=True), (40, 41, 200)),
                                   (_random_hist(rng, 120, 33, p_one_sided=0.4), (3, 77)), (_hist(HAND), (4,))]):
        ser = dict(zip(SM.FIELDS, SM.words(SM.fold(h, cuts=cuts))))
        hdr = dict(zip(DM.HEADER_FIELDS, DM.words(DM.fold(h, cuts=cuts))[-1]))
        assert hdr["n_steps"] == ser["n_steps"] == len(h) and hdr["n_two_sided"] == ser["n_two_sided"], q
        assert hdr["n_pairs"] == ser["n_ret"] > 0 and hdr["sum_d"] == ser["sum_d"] and hdr["sum_abs_d"] == ser["sum_abs_d"], q
        assert hdr["n_up"] + hdr["n_down"] <= hdr["n_pairs"] and hdr["n_bid_side"] + hdr["n_ask_side"] - hdr["n_steps"] <= hdr["n_two_sided"]


def _write_case(tmp_path, hists, ends, want):
    with open(tmp_path / "records.txt", "w") as f:
        f.write(f"{len(hists)}\n")
        for h, e in zip(hists, ends):
            f.write(" ".join(str(x) for x in [len(h), DM.levels_of(h), len(e)] + list(e)) + "\n")
            for rec in h:
                f.write(" ".join(str(int(x)) for x in rec[[1, 2] + list(range(5, len(rec)))]) + "\n")
    with open(tmp_path / "expected.txt", "w") as f:
        for per_series in want:
            for words, carry in per_series:
                for w in words:
                    f.write(" ".join(str(x) for x in w) + "\n")
                f.write(" ".join(str(x) for x in carry) + "\n")


def _expect(hists, ends):
    want = []
    for h, e in zip(hists, ends):
        s, lo, per = DM.cleared(DM.levels_of(h)), 0, []
        for y in e:
            s = DM.fold(h[lo:y], first_step=lo, into=s)
            per.append(_state(s))
            lo = y
        assert per[-1] == _state(DM.fold(h))  # (the model itself is split-invariant)
        want.append(per)
    return want


def _build_exe(tmp_path, extra=()):
    exe = str(tmp_path / "depth_fold_test")
    res = subprocess.run([_cxx(), "-std=c++17", "-O2", *extra, os.path.join(ROOT, "tests", "cpp", "depth_fold_test.cpp"), "-o", exe],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return exe


def _fold_lengths(L):
    Lp = 1
    while Lp < L:
        Lp *= 2
    G = 64 // Lp
    return G, [x for x in (1, G - 1, G, G + 1, 64, 65, 130, 200) if x > 0]


def test_depth_fold_hpp_equals_the_model_over_random_histories_and_splits(tmp_path):
    exe = _build_exe(tmp_path)
    rng = np.random.default_rng(23)
    hists, ends = [], []
    for L in LEVELS:
        G, lens = _fold_lengths(L)
        # the fold lengths the lanes' paths turn on, one after the other; volumes up to 2^32 - 1 and jumps of 2^33 - 8
        hists.append(_random_hist(rng, sum(lens), L, wide=True))
        ends.append([int(x) for x in np.cumsum(lens)])
        # every fold a single step
        hists.append(_random_hist(rng, 70, L, wide=False, p_one_sided=0.2))
        ends.append(list(range(1, 71)))
        # random splits
        for q in range(2):
            n = int(rng.integers(2, 300))
            hists.append(_random_hist(rng, n, L, wide=q == 1))
            ends.append(sorted(set(int(x) for x in rng.integers(1, n + 1, size=int(rng.integers(1, 9)))) | {n}))
    want = _expect(hists, ends)
    n_steps = sum(len(h) for h in hists)
    one_sided = sum(int(np.sum((h[:, 1] == 0) | (h[:, 2] == MAXU))) for h in hists)
    assert 0.05 < one_sided / n_steps < 0.25
    lens = {(DM.levels_of(h), b - a) for h, e in zip(hists, ends) for a, b in zip([0] + e[:-1], e)}
    for L in LEVELS:
        assert all((L, x) in lens for x in _fold_lengths(L)[1]), L
    deep = want[4 * LEVELS.index(64)][-1]  # 64 levels of volumes near 2^32: the imbalance passes 2^32, sum_imb_d has wrapped
    assert max(min(x, M64 + 1 - x) for x in deep[1][:64]) > 1 << 32
    h64 = hists[4 * LEVELS.index(64)]
    exact = DM.fold(h64)["rows"][63]
    assert abs(exact["sum_imb_d"]) >> 64 or exact["sum_imb_sq"] >> 64, "a sum that wraps modulo 2^64 is among the cases"
    for per in want[::4]:
        words = per[-1][0]
        assert words[0][10] > 20 and words[0][12] > 5 and words[0][14] - words[0][12] > 5 and words[-1][2] > 40
    _write_case(tmp_path, hists, ends, want)
    args = [exe, str(tmp_path / "records.txt"), str(tmp_path / "expected.txt")]
    run = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip().endswith(f"depth_fold ok {len(hists)} series {n_steps} steps {sum(len(e) for e in ends)} folds")
    # a wrong expectation is really caught, by name: one word of a level's row, one of the header, one carry word
    s5 = 4 * LEVELS.index(5)
    want[s5][2][0][3][13] ^= 1
    _write_case(tmp_path, hists, ends, want)
    run = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert run.returncode == 1 and f"series {s5} fold 2 (lanes): row 3 word 13 " in run.stdout and "(serial): row 3 word 13 " in run.stdout
    want[s5][2][0][3][13] ^= 1
    want[s5][3][0][5][2] += 1
    want[s5][4][1][4] ^= 1
    _write_case(tmp_path, hists, ends, want)
    run = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert run.returncode == 1 and f"series {s5} fold 3 (lanes): row 5 word 2 " in run.stdout and f"series {s5} fold 4 (serial): carry 4 " in run.stdout


def test_depth_fold_hpp_under_the_address_and_undefined_behaviour_sanitizers(tmp_path):
    """the same program built once with -fsanitize=address,undefined, run on its own over a short case"""
    exe = _build_exe(tmp_path, ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    rng = np.random.default_rng(29)
    hists = [_random_hist(rng, 70, 5, wide=True), _random_hist(rng, 150, 33), _random_hist(rng, 100, 64, wide=True), _random_hist(rng, 130, 1)]
    ends = [list(range(1, 71)), [1, 66, 150], [3, 4, 100], [63, 64, 130]]
    _write_case(tmp_path, hists, ends, _expect(hists, ends))
    run = subprocess.run([exe, str(tmp_path / "records.txt"), str(tmp_path / "expected.txt")], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "depth_fold ok 4 series" in run.stdout, run.stdout + run.stderr
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
    # the table has no fold or clear entry of its own and no flag bit
    assert sorted(re.findall(r"\bbk_\w*depth\w*(?=\()", header)) == sorted(ENTRIES)
    taken = [int(v) for v in re.findall(r"#define BK_FLAG_\w+ (\d+)u", header)]
    assert len(taken) == len(set(taken)) and sorted(taken) == sorted(_lib.FLAG_NAMES) == [1 << i for i in range(10)], taken
    assert "DEPTH" not in " ".join(re.findall(r"#define BK_FLAG_(\w+)", header))
    for method in ("enable_depth", "depth", "depth_view", "depth_device_ptr", "fold_series", "clear_series", "run_series"):
        assert callable(getattr(bourse_amd.ManyBookEnv, method)), method
        assert getattr(bourse_amd.ManyMarketEnv, method) is getattr(bourse_amd.ManyBookEnv, method), method
    assert bourse_amd.DEPTH_FIELDS is _lib.DEPTH_FIELDS and bourse_amd.DEPTH_HEADER_FIELDS is _lib.DEPTH_HEADER_FIELDS
    assert bourse_amd.DEPTH_FIELDS == DM.FIELDS and bourse_amd.DEPTH_HEADER_FIELDS == DM.HEADER_FIELDS
    assert bourse_amd.depth_moments is _lib.depth_moments
    # the header names the words in their order, the levels' rows first, then the header row's
    doc = header[header.index("per-level depth table"):header.index("int bk_depth_enable(")]
    at = [re.search(r"\b" + n + r"\b", doc) for n in DM.FIELDS]
    assert all(at) and [m.start() for m in at] == sorted(m.start() for m in at)
    tail = doc[doc.index("Row L, the header"):]
    at = [re.search(r"\b" + str(i) + r" " + n + r"\b", tail) for i, n in enumerate(DM.HEADER_FIELDS)]
    assert all(at) and [m.start() for m in at] == sorted(m.start() for m in at)
    hpp = open(os.path.join(ROOT, "include", "bourse_amd.hpp")).read()
    for method in ("enable_depth", "depth", "depth_device_ptr"):
        assert re.search(r"\b" + method + r"\(", hpp), method
    rs = open(os.path.join(ROOT, "integration", "rust", "bourse_amd_sys.rs")).read()
    assert re.search(r"pub fn bk_depth_enable\(env: \*mut BkEnv\) -> c_int;", rs)
    assert re.search(r"pub fn bk_depth_device_ptr\(env: \*mut BkEnv, out: \*mut \*mut c_void\) -> c_int;", rs)
    assert re.search(r"pub fn bk_get_depth\(env: \*mut BkEnv, first_book: u32, n_books: u32, out: \*mut u64\) -> c_int;", rs)
    # the enum of depth_fold.hpp is the same order
    fold = open(os.path.join(CSRC, "depth_fold.hpp")).read()
    words = re.search(r"enum Word : uint32_t \{[^\n]*\n(.*?)\};", fold, flags=re.S).group(1)
    assert [w.strip().split(" ")[0].lower() for w in words.replace("\n", " ").split(",")] == list(DM.FIELDS) + ["row_words"]
    words = re.search(r"enum HeaderWord : uint32_t \{[^\n]*\n(.*?)\};", fold, flags=re.S).group(1)
    assert [w.strip().split(" ")[0].lower() for w in words.replace("\n", " ").split(",")] == list(DM.HEADER_FIELDS) + ["header_words"]


def test_a_null_env_is_refused_not_dereferenced():
    from bourse_amd import _lib

    L = _lib.load()
    out = ctypes.c_void_p()
    rows = np.zeros((1, 3, 16), dtype=np.uint64)
    calls = {
        "bk_depth_enable": lambda: L.bk_depth_enable(None),
        "bk_depth_device_ptr": lambda: L.bk_depth_device_ptr(None, ctypes.byref(out)),
        "bk_get_depth": lambda: L.bk_get_depth(None, 0, 1, rows.ctypes.data_as(ctypes.c_void_p)),
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
    """bkd::depth kernels are not among the names tools/kernel_isa_counts.py::measure lists, so
    profiles/kernel_isa_baseline.json stays as it is; the fold is plain C++ and builtins and shares its rules and lane
    mapping with the CPU test through depth_fold.hpp; bourse_amd.hip launches it only from the series' two launchers and
    the enable's clear, each behind the test of the table's rows."""
    src = open(os.path.join(CSRC, "depth.hpp")).read()
    code = re.sub(r"//.*", "", src)
    assert re.search(r"namespace bkd \{\s*namespace depth \{", code)
    for k in ("k_fold", "k_clear"):
        assert re.search(r"__global__[^;{]*\b" + k + r"\(", code), k
    assert "asm" not in code and "tomic" not in code.replace("__ATOMIC_ACQ_REL", "") and "__shared__" not in code
    assert "series::" not in code and "bk_u32x4*>" not in code and "reinterpret_cast" not in code
    assert '#include "depth_fold.hpp"' in src and '#include "hist_ring.hpp"' in src
    assert "__builtin_amdgcn_fence" not in code and "n_books + b" not in code and "g.mask" not in code
    for f in ("lanes_of(", "passes_of(", "step_of(", "level_of(", "group_of(", "last_lane(", "tail_lane(", "level_at(", "add_level(",
              "add_header(", "word_of(", "slot_of(", "ring::record(", "ring::masked_book(", "wave_sync()"):
        assert f in code, f
    fold = open(os.path.join(CSRC, "depth_fold.hpp")).read()
    assert re.search(r"namespace bkd \{\s*namespace depth \{", fold)
    assert "hip_runtime" not in fold and "asm" not in re.sub(r"//.*", "", fold)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_isa_counts as K

    base = json.load(open(K.BASELINE))["kernels"]
    assert not [k for k in base if "depth" in k or "k_fold" in k]
    hip = re.sub(r"//.*", "", open(os.path.join(CSRC, "bourse_amd.hip")).read())
    fns = _functions(hip)
    assert [n for n, fn in fns.items() if "depth::k_fold," in fn] == ["launch_series_fold"] and hip.count("depth::k_fold,") == 1
    assert sorted(n for n, fn in fns.items() if "depth::k_clear," in fn) == ["bk_depth_enable", "launch_series_clear"]
    for name, kernel in (("launch_series_fold", "depth::k_fold,"), ("launch_series_clear", "depth::k_clear,")):
        fn = fns[name]
        assert fn.index("series::k_" + kernel[9:]) < fn.index("if (env->depth_rows.p) {") < fn.index(kernel), name
    enable = fns["bk_depth_enable"]
    order = [enable.index(x) for x in ("tables[T_SERIES].on", "bk_series_enable", "already enabled", "table_fold(env, T_SERIES)", ".alloc(",
                                       "depth::k_clear,", "depth_rows.swap(")]
    assert order == sorted(order), order
    for name in ("bk_depth_device_ptr", "bk_get_depth"):
        assert fns[name][fns[name].index("{"):].lstrip("{\n ").startswith("if (int rc = depth_ok(env)) return rc;"), name
    assert '"this env has no depth table: call bk_depth_enable first"' in fns["depth_ok"]


def _built_kernels():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_isa_counts as K
    from bourse_amd import _build

    lib = _build.build()
    ks, meta = {}, {}
    with tempfile.TemporaryDirectory(prefix="bourse_depth_isa_") as tmp:
        for co in K.code_objects(lib, tmp):
            ks.update(K.kernels_of(co))
            txt = subprocess.run([K._tool("llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
            for blk in re.split(r"\n\s+- \.agpr_count:", txt):
                name = re.search(r"\.name:\s+(\S+)", blk)
                if name and "5depth" in name.group(1):
                    meta[name.group(1)] = {k: int(v) for k, v in re.findall(
                        r"\.(private_segment_fixed_size|group_segment_fixed_size|vgpr_count|sgpr_count):\s+(\d+)", blk)}
    names = K.demangle(sorted(ks))
    return K, {names[n].replace("bkd::", ""): v for n, v in ks.items() if "depth::k_" in names[n]}, meta


def test_the_depth_kernels_match_their_instruction_count_profile_and_use_no_scratch():
    """The two kernels' counts by issue class and their loop spans are pinned in profiles/kernel_isa_depth.json, within the
    baseline's 3 % (+-2 instructions always pass): the classes, not the total - the code object's padding stands behind
    whichever kernel comes last.  After an intended change of depth.hpp: write the new counts into the profile.  And the
    built library's metadata: no scratch, no LDS allocation (the shuffles are ds_bpermute, which needs none)."""
    K, now, meta = _built_kernels()
    base = json.load(open(os.path.join(ROOT, "profiles", "kernel_isa_depth.json")))["kernels"]
    assert sorted(now) == sorted(base) == ["depth::k_clear", "depth::k_fold"], (sorted(now), sorted(base))

    def off(a, b):
        return abs(a - b) > max(2, K.TOL * max(a, b))

    for k in base:
        for c in ("salu", "branch", "valu", "lds", "vmem", "smem"):
            assert not off(base[k]["counts"][c], now[k]["counts"][c]), (k, c, base[k]["counts"][c], now[k]["counts"][c])
        assert len(base[k]["loops"]) == len(now[k]["loops"]), (k, base[k]["loops"], now[k]["loops"])
        assert not [1 for x, y in zip(base[k]["loops"], now[k]["loops"]) if off(x, y)], (k, base[k]["loops"], now[k]["loops"])
    assert len(meta) == 2, meta
    for name, m in meta.items():
        assert m["private_segment_fixed_size"] == 0 and m["group_segment_fixed_size"] == 0, (name, m)
        assert m["vgpr_count"] <= 128, (name, m)


def test_depth_moments_against_numpy_on_a_synthetic_history():
    from bourse_amd import depth_moments

    rng = np.random.default_rng(11)
    L, n = 6, 400
    hists = [_random_hist(rng, n, L), _random_hist(rng, n, L, p_one_sided=0.3)]
    rows = np.array([DM.table(DM.fold(h)) for h in hists], dtype=np.uint64)
    got = depth_moments(rows)
    assert got.shape == (2, L) and got.dtype.names[:2] == ("mean_bid_vol", "mean_ask_vol")
    for b, h in enumerate(hists):
        h = h.astype(np.float64)
        lv = h[:, 5:].reshape(n, L, 4)
        bv, bn, av, an = (lv[:, :, i] for i in range(4))
        two = (h[:, 1] != 0) & (h[:, 2] != MAXU)
        imb = np.cumsum(bv - av, axis=1)
        pair = two[1:] & two[:-1]
        d = (h[1:, 1] + h[1:, 2] - h[:-1, 1] - h[:-1, 2])[pair]
        J = imb[:-1][pair]
        want = {"mean_bid_vol": bv.mean(0), "mean_ask_vol": av.mean(0), "var_bid_vol": bv.var(0), "var_ask_vol": av.var(0),
                "mean_bid_orders": bn.mean(0), "mean_ask_orders": an.mean(0), "bid_occupancy": (bn > 0).mean(0),
                "ask_occupancy": (an > 0).mean(0), "mean_imb": imb[two].mean(0), "var_imb": imb[two].var(0),
                "response": (np.sign(J) * d[:, None]).sum(0) / (J != 0).sum(0) / 2.0,
                "hit_rate": (np.sign(J) * d[:, None] > 0).sum(0) / ((J != 0) & (d[:, None] != 0)).sum(0),
                "slope": (J * d[:, None]).sum(0) / (imb[two] ** 2).sum(0)}
        assert pair.sum() > 100 and not two.all()
        for name, x in want.items():
            assert np.allclose(got[name][b], x, rtol=1e-9, atol=1e-9), (b, name, got[name][b], x)
    assert (depth_moments(rows[0])[0] == got[0]).all()  # one book's [L + 1, 16] too, and int64 bits read the same
    assert all((depth_moments(rows.view(np.int64))[n] == got[n]).all() for n in got.dtype.names)
    # zero counts and denominators give NaN: a cleared table, and a book whose imbalance was always 0
    empty = depth_moments(np.zeros((1, 3, 16), dtype=np.uint64))
    assert all(np.isnan(empty[n]).all() for n in empty.dtype.names)
    flat = _hist([(100, 104, [(3, 1, 3, 1)]), (101, 104, [(3, 1, 3, 1)]), (102, 104, [(3, 1, 3, 1)])])
    m = depth_moments(DM.table(DM.fold(flat)))
    assert np.isnan(m["response"]).all() and np.isnan(m["hit_rate"]).all() and np.isnan(m["slope"]).all()
    assert m["mean_bid_vol"][0, 0] == 3.0 and m["var_imb"][0, 0] == 0.0 and m["bid_occupancy"][0, 0] == 1.0
    with pytest.raises(ValueError):
        depth_moments(np.zeros((2, 3, 15), dtype=np.uint64))
    with pytest.raises(ValueError):
        depth_moments(np.zeros((2, 3, 16), dtype=np.float64))
