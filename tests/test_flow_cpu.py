"""The per-book flow table of the trade records (bk_flow_enable) without a GPU: the plain-Python model (tests/flow_model.py)
against a six-trade tape worked out by hand and against a double loop over all pairs; the kernel's rules
(bourse_amd/csrc/flow_fold.hpp, compiled with g++ into a program of its own, plain and under the sanitizers) against the
model on shared random tapes; flow_moments on hand-made rows; the C ABI; the shape of the host path in bourse_amd.hip; and
the kernels' metadata.

MODEL-ONLY (they run no code of the library and pass without it): the two test_the_model_*.  Every other test here calls,
reads or disassembles what the flow table added."""
import ctypes
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import flow_model as FM
from test_lags_cpu import _cxx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bourse_amd", "csrc")
ENTRIES = ("bk_flow_enable", "bk_flow_fold", "bk_flow_clear", "bk_flow_clear_device", "bk_flow_device_ptr", "bk_flow_lags",
           "bk_get_flow", "bk_get_flow_state")
BK_INVALID_ARGUMENT = 5
M64 = (1 << 64) - 1
V, BUY = 1 << 63, 1 << 62
BIG = 1 << 62

# (price, vol, side_is_bid): four buys - one of them a sweep of three levels - then two sells
HAND = [(100, 4, 0), (100, 6, 0), (102, 2, 0), (105, 3, 0), (90, 3, 1), (95, 2, 1)]
HAND_BASE = [6, 4, 20, 15, 78, 1979, 6, 0]
#            n_pairs sum_ss sum_resp sum_back sum_abs_dp sum_dp2
HAND_LAGS = [[5, 3, -15, 15, 25, 263],   # (0,+,+) (2,+,+) (3,+,+) (-15: s_i -, s_j +) (5,-,-)
             [4, 0, -15, 29, 29, 273],   # (2,+,+) (5,+,+) (-12: -,+) (-10: -,+)
             [3, -1, -12, 22, 22, 174]]  # (5,+,+) (-10: -,+) (-7: -,+)


def _words(base, lags):
    return [x & M64 for x in base] + [x & M64 for row in lags for x in row]


def test_the_model_against_a_six_trade_tape_worked_out_by_hand():
    words, carry, seen = FM.fold_tape(HAND, 3, [(6, 0, BIG)])
    assert words == _words(HAND_BASE, HAND_LAGS) and seen == 6
    assert carry == [V | 95, V | 90, V | BUY | 105]
    assert FM.brute_words(HAND, 3, [True] * 6) == words
    # every split into two folds, and one fold per record
    for y in range(7):
        assert FM.fold_tape(HAND, 3, [(y, 0, BIG), (6, 0, BIG)]) == (words, carry, 6), y
    assert FM.fold_tape(HAND, 3, [(y, 0, BIG) for y in range(1, 7)]) == (words, carry, 6)
    # a reset behind record 3 that restores the count 2: records 4, 5 pair with each other only; the cursor follows
    m = FM.FlowModel(3)
    m.fold(HAND, 4)
    m.cut(2)
    assert m.carry() == [0, 0, 0] and m.seen == 2
    m.fold(HAND[:2] + HAND[4:], 4)  # (the book's records 2, 3 after the reset are the tape's 4, 5)
    assert m.words() == _words([6, 4, 20, 15, 78, 1979, 6, 0], [[4, 4, 0, 0, 10, 38], [2, 2, 7, 7, 7, 29], [1, 1, 5, 5, 5, 25]])
    # record 2 lost (a capacity of 2 in the first fold, consumed before the second): n_lost 1, the pair (3, 1) stays at lag 2
    lost = FM.fold_tape(HAND, 3, [(3, 0, 2), (6, 3, BIG)])
    assert lost[0] == FM.brute_words(HAND, 3, [True, True, False, True, True, True])
    assert lost[0][:8] == [5, 3, 18, 13, 74, 1775, 6, 1] and lost[0][8 + 6] == 2  # lag 2: (3, 1) and (5, 3); (2, 0), (4, 2) are gone
    assert lost[0][8:14] == [3, 1, -20 & M64, 10, 20, 250]  # lag 1: (1, 0), (4, 3), (5, 4)
    # the whole table lost: a gap of a billion is counted, not walked
    gone = FM.fold_tape(HAND, 3, [(3, 0, BIG), (10 ** 9, 10 ** 9, BIG)])
    assert gone[0][7] == 10 ** 9 - 3 and gone[1] == [0, 0, 0] and gone[2] == 10 ** 9
    # words wrap as the device's do
    big = 4_000_000_000
    w = FM.fold_tape([(big, big, 0), (0, big, 1), (big, big, 0)], 1, [(3, 0, BIG)])[0]
    assert w[:8] == [3, 2, 3 * big, 2 * big, (3 * big * big) & M64, (2 * big * big) & M64, big, 0] and 3 * big * big > M64
    # (1, 0): dp = -big behind a buy, at a sell; (2, 1): dp = +big behind a sell, at a buy
    assert w[8:] == [2, -2 & M64, -2 * big & M64, 2 * big, 2 * big, (2 * big * big) & M64]


def _tape(rng, n, wide):
    if wide:
        return [(int(rng.integers(0, 1 << 32)), int(rng.integers(0, 1 << 32)), int(rng.integers(0, 3)) * int(rng.integers(1, 1 << 32)))
                for _ in range(n)]
    return [(int(rng.integers(990, 1010)), int(rng.integers(1, 200)), int(rng.random() < 0.4)) for _ in range(n)]


def test_the_model_against_a_double_loop_over_all_pairs():
    rng = np.random.default_rng(11)
    for q in range(12):
        K = (1, 2, 5, 16, 63, 64)[q % 6]
        tape = _tape(rng, int(rng.integers(1, 300)), q % 2 == 0)
        ends = sorted(set(int(x) for x in rng.integers(0, len(tape) + 1, size=5)) | {len(tape)})
        assert FM.fold_tape(tape, K, [(e, 0, BIG) for e in ends])[0] == FM.brute_words(tape, K, [True] * len(tape)), q


def _exe(tmp_path, extra=()):
    exe = str(tmp_path / "flow_fold_test")
    res = subprocess.run([_cxx(), "-std=c++17", "-O2", *extra, os.path.join(ROOT, "tests", "cpp", "flow_fold_test.cpp"), "-o", exe],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    return exe


def test_flow_fold_hpp_against_all_pairs_every_split_and_lost_indices(tmp_path):
    run = subprocess.run([_exe(tmp_path)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and re.search(r"flow_fold ok \d{3,} cases", run.stdout), run.stdout + run.stderr


def test_flow_fold_hpp_under_the_address_and_undefined_behaviour_sanitizers(tmp_path):
    """the same program built once with -fsanitize=address,undefined, run on its own"""
    exe = _exe(tmp_path, ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and "flow_fold ok" in run.stdout, run.stdout + run.stderr
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr


def _dump(exe, tape, K, start, folds):
    """flow_fold.hpp's answer for one case: folds = [(total, base, capacity, cut or -1)]"""
    text = f"{K} {len(tape)}\n" + "".join(f"{p} {v} {s}\n" for p, v, s in tape) + f"{start} {len(folds)}\n"
    text += "".join(f"{t} {b} {c} {cut}\n" for t, b, c, cut in folds)
    run = subprocess.run([exe, "dump"], input=text, capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
    words, carry, seen = run.stdout.strip().split("\n")
    return [int(x) for x in words.split()], [int(x) for x in carry.split()], int(seen)


def test_flow_fold_hpp_equals_the_model_on_shared_random_tapes(tmp_path):
    exe = _exe(tmp_path)
    rng = np.random.default_rng(23)
    n_lost = n_cut = n_short = 0
    for q in range(40):
        K = (1, 3, 16, 64)[q % 4]
        n = int(rng.integers(1, 400))
        tape = _tape(rng, n, q % 3 == 0)
        ends = sorted(set(int(x) for x in rng.integers(0, n + 1, size=int(rng.integers(1, 7)))) | {n})
        folds, base = [], 0
        for e in ends:  # what a run of folds can meet: a small capacity, records consumed between two folds, a reset
            cap = int(rng.choice([BIG, BIG, 16, 70]))
            cut = -1
            if rng.random() < 0.15:
                cut = int(rng.integers(0, e + 1))
            folds.append((e, base, cap, cut))
            if rng.random() < 0.5:
                base = e if rng.random() < 0.7 else min(n, e + int(rng.integers(0, K + 3)))
            if cut >= 0:
                base = min(base, cut)
        m = FM.FlowModel(K)
        for t, b, c, cut in folds:
            n_short += 0 < t - m.seen < K
            m.fold(tape, t, b, c)
            if cut >= 0:
                m.cut(cut)
                n_cut += 1
        n_lost += m.base["n_lost"] > 0
        assert _dump(exe, tape, K, 0, folds) == (m.words(), m.carry(), m.seen), (q, K, folds)
    assert n_lost > 10 and n_cut > 5 and n_short > 5, (n_lost, n_cut, n_short)
    # the hand tape through the header
    assert _dump(exe, HAND, 3, 0, [(6, 0, BIG, -1)]) == (_words(HAND_BASE, HAND_LAGS), [V | 95, V | 90, V | BUY | 105], 6)


def test_flow_moments_on_hand_made_rows():
    import bourse_amd
    from bourse_amd import _lib

    rows = FM.rows_of([_words(HAND_BASE, HAND_LAGS), [0] * 26, _words([2, 2, 8, 8, 32, 800, 4, 6], [[1, 1, 0, 0, 0, 0]] + [[0] * 6] * 2),
                       _words([0, 0, 0, 0, 0, 0, 0, 5], [[0] * 6] * 3)], 3)
    assert rows.dtype == _lib.flow_dtype(3) and rows.shape == (4,)
    got = bourse_amd.flow_moments(rows)
    assert got.shape == (4,) and got.dtype.names == _lib.FLOW_MOMENTS_BASE + _lib.FLOW_MOMENTS_LAG and got["sign_acf"].shape == (4, 3)
    h = got[0]
    from fractions import Fraction as F

    mean = F(1, 3)  # (4 buys - 2 sells) / 6
    assert h["buy_share"] == 4 / 6 and h["sign_mean"] == float(mean) and h["mean_vol"] == 20 / 6 and h["lost_share"] == 0.0
    assert h["var_vol"] == float(F(78, 6) - F(20, 6) ** 2) and h["vwap"] == 1979 / 20
    for k, (n, ss, resp, back, a, d2) in enumerate(HAND_LAGS):
        assert h["sign_acf"][k] == float((F(ss, n) - mean ** 2) / (1 - mean ** 2)), k
        assert h["response"][k] == resp / n and h["back_response"][k] == back / n and h["mean_abs_dp"][k] == a / n
        assert h["variogram"][k] == d2 / n
    # every NaN case: a cleared row - all of it; only buys - sign_acf (1 - mean^2 is 0), and the lags without a pair;
    # only lost records - everything but lost_share
    assert all(np.isnan(got[1][n]).all() for n in got.dtype.names)
    one = got[2]
    assert one["buy_share"] == 1.0 and one["sign_mean"] == 1.0 and one["lost_share"] == 0.75 and one["vwap"] == 100.0
    assert np.isnan(one["sign_acf"]).all() and one["response"][0] == 0.0 and np.isnan(one["response"][1:]).all()
    assert np.isnan(one["variogram"][1:]).all() and one["variogram"][0] == 0.0
    assert got[3]["lost_share"] == 1.0 and all(np.isnan(got[3][n]).all() for n in got.dtype.names if n != "lost_share")
    # unsigned words above 2^63 are read as unsigned, signed ones as signed
    wide = bourse_amd.flow_moments(FM.rows_of([_words([1, 1, 1, 1, 1, 1, 1, 0], [[2, -2, -6, 6, 6, (1 << 64) - 2]])], 1))[0]
    assert wide["response"][0] == -3.0 and wide["variogram"][0] == float(((1 << 64) - 2) / 2)
    with pytest.raises(ValueError):
        bourse_amd.flow_moments(np.zeros(2, dtype=np.uint64))


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
    # a lost record is counted in the table: the set of flag bits is unchanged
    taken = [int(v) for v in re.findall(r"#define BK_FLAG_\w+ (\d+)u", header)]
    assert sorted(taken) == sorted(_lib.FLAG_NAMES) == [1 << i for i in range(10)], taken
    for method in ("enable_flow", "fold_flow", "flow", "flow_view", "flow_device_ptr", "clear_flow", "flow_state", "run_series"):
        assert callable(getattr(bourse_amd.ManyBookEnv, method)), method
        assert getattr(bourse_amd.ManyMarketEnv, method) is getattr(bourse_amd.ManyBookEnv, method), method
    assert bourse_amd.ManyBookEnv.FLOW_DTYPE is _lib.FLOW_DTYPE is bourse_amd.FLOW_DTYPE
    assert bourse_amd.flow_moments is _lib.flow_moments and bourse_amd.flow_dtype is _lib.flow_dtype
    hpp = open(os.path.join(ROOT, "include", "bourse_amd.hpp")).read()
    for method in ("enable_flow", "fold_flow", "flow", "flow_device_ptr", "clear_flow"):
        assert re.search(r"\b" + method + r"\(", hpp), method
    rs = open(os.path.join(ROOT, "integration", "rust", "bourse_amd_sys.rs")).read()
    for name in ENTRIES:
        assert re.search(r"pub fn " + name + r"\(", rs), name
    assert re.search(r"pub fn bk_flow_enable\(env: \*mut BkEnv, n_lags: u32, consume_trades: c_int\) -> c_int;", rs)
    # ... and every word number the header names reaches Rust
    words = [("BK_FLOW_" + n.upper(), i) for i, n in enumerate(FM.BASE + ("base_words",))]
    words += [("BK_FLOW_" + n.upper(), i) for i, n in enumerate(FM.LAG + ("lag_words",))]
    for name, i in words:
        assert f"pub const {name}: c_int = {i};" in rs, name


def test_a_row_is_8_plus_6k_words_laid_out_as_the_header_numbers_them(tmp_path):
    from bourse_amd import _lib

    for K in (1, 16, 64):
        dt = _lib.flow_dtype(K)
        assert dt.itemsize == 8 * (8 + 6 * K) and dt.names == FM.BASE + ("lags",) == _lib.FLOW_BASE_FIELDS + ("lags",)
        assert [dt.fields[n][1] for n in dt.names] == [8 * i for i in range(9)]
        assert dt["lags"].shape == (K, 6) and dt["lags"].base == np.dtype("<i8")
    assert _lib.FLOW_DTYPE == _lib.flow_dtype(16) and _lib.FLOW_LAG_FIELDS == FM.LAG
    for bad in (0, 65):
        with pytest.raises(ValueError):
            _lib.flow_dtype(bad)
    src = tmp_path / "words.cpp"
    names = ["BK_FLOW_" + n.upper() for n in FM.BASE] + ["BK_FLOW_BASE_WORDS"] + ["BK_FLOW_" + n.upper() for n in FM.LAG] + ["BK_FLOW_LAG_WORDS"]
    src.write_text('#include <cstdio>\n#include "bourse_amd.h"\nint main() {\n' + "".join(f'std::printf("%d ", (int){n});\n' for n in names) +
                   "return 0; }\n")
    exe = str(tmp_path / "words")
    res = subprocess.run([_cxx(), "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60).stdout.split()
    assert [int(x) for x in out] == list(range(9)) + list(range(7))


def test_a_null_env_is_refused_not_dereferenced():
    from bourse_amd import _lib

    L = _lib.load()
    mask = (ctypes.c_uint8 * 4)(1, 0, 1, 0)
    out, n = ctypes.c_void_p(), ctypes.c_uint32()
    words = np.zeros(4 * 26, dtype=np.uint64)
    p = words.ctypes.data_as(ctypes.c_void_p)
    calls = {
        "bk_flow_enable": lambda: L.bk_flow_enable(None, 3, 0),
        "bk_flow_fold": lambda: L.bk_flow_fold(None),
        "bk_flow_clear": lambda: L.bk_flow_clear(None, ctypes.cast(mask, ctypes.c_void_p)),
        "bk_flow_clear_device": lambda: L.bk_flow_clear_device(None, ctypes.cast(mask, ctypes.c_void_p)),
        "bk_flow_device_ptr": lambda: L.bk_flow_device_ptr(None, ctypes.byref(out)),
        "bk_flow_lags": lambda: L.bk_flow_lags(None, ctypes.byref(n)),
        "bk_get_flow": lambda: L.bk_get_flow(None, 0, 1, p),
        "bk_get_flow_state": lambda: L.bk_get_flow_state(None, 0, 1, p, p),
    }
    assert set(calls) == set(ENTRIES)
    for name, call in calls.items():
        L.bk_device_count(ctypes.byref(ctypes.c_int(0)))  # (anything that may leave another message behind)
        assert call() == BK_INVALID_ARGUMENT, name
        assert b"null env" in L.bk_last_error(), name


def test_enable_flow_has_no_cpu_path():
    """Without a GPU the only way to enable_flow, the env's constructor, raises NoDeviceError; and the method itself goes
    straight to bk_flow_enable - an object without a handle gets the library's refusal of a null env, not a table folded
    somewhere else.  (The first half alone would pass without the feature: the second is what runs its code.)"""
    import bourse_amd
    from bourse_amd import _lib

    Env = bourse_amd.ManyBookEnv
    assert callable(Env.enable_flow) and callable(Env.fold_flow)
    bare = object.__new__(Env)  # no constructor: no handle, no table
    bare._L, bare._h, bare._flow_lags = _lib.load(), None, 0
    with pytest.raises(bourse_amd.BourseError, match="null env") as e:
        bare.enable_flow(4)
    assert e.value.code == BK_INVALID_ARGUMENT and bare._flow_lags == 0
    with pytest.raises(ValueError):
        bare.enable_flow(-1)
    for call in (bare.flow, bare.flow_dtype, bare.flow_state):  # refused before the library is asked
        with pytest.raises(bourse_amd.BourseError, match="no flow table"):
            call()
    n = ctypes.c_int(-1)
    _lib.load().bk_device_count(ctypes.byref(n))
    if n.value == 0:
        with pytest.raises(bourse_amd.NoDeviceError):
            Env(1, 101, 0, 1, 1000, trade_capacity=64).enable_flow(4)


def _functions(hip):
    return {m.group(1): fn for fn in re.split(r"\n(?=(?:static )?[\w:]+ \w+\([^;]*\) \{)", hip)
            for m in [re.match(r"(?:static )?[\w:]+ (\w+)\(", fn)] if m}


def test_every_launch_of_the_flow_kernels_sits_behind_the_on_test_and_the_step_consumes_once():
    code = re.sub(r"//.*", "", open(os.path.join(CSRC, "bourse_amd.hip")).read())
    fns = _functions(code)
    # each kernel is named at one launch site, inside its own launcher
    for k in ("fold", "clear"):
        sites = [name for name, fn in fns.items() if f"flow::k_{k}," in fn]
        assert sites == [f"launch_flow_{k}"] and code.count(f"flow::k_{k},") == 1, (k, sites)
    # every call of a launcher stands behind the table's on-test: `if (env->flow_lags) {` opens the block it is in, or the
    # function began with the guard flow_ok (the entries), or it is the enable, which has just set flow_lags
    guarded = {"bk_flow_fold", "bk_flow_clear_device"}
    users = {}
    for name, fn in fns.items():
        body = fn[fn.index("{"):]
        for m in re.finditer(r"\blaunch_flow_(fold|clear)\(env", body):
            if name == f"launch_flow_{m.group(1)}":
                continue
            users.setdefault(name, []).append(m.group(1))
            if name in guarded:
                assert body.lstrip("{\n ").startswith("if (int rc = flow_ok(env)) return rc;"), name
            elif name == "bk_flow_enable":
                assert "env->flow_lags = n_lags;" in body[:m.start()], name
            else:
                opened = body[:m.start()].rstrip()
                assert re.search(r"if \(env->flow_lags\) \{$", opened), (name, opened[-80:])
    assert users == {"bk_step_async": ["fold"], "bk_checkpoint_load": ["clear"], "reset_books_from": ["fold", "clear"],
                     "bk_ingress_reset_books_device": ["clear"], "bk_flow_enable": ["clear"], "bk_flow_fold": ["fold"],
                     "bk_flow_clear_device": ["fold", "clear"]}, users
    assert "if (!env->flow_lags) return fail(" in fns["flow_ok"]
    # bk_warm and bk_run launch nothing for it; bk_load_book refuses
    assert "flow" not in fns["bk_warm"].replace("device_flow", "").replace("flow0", "")
    assert "if (env->flow_lags)\n    return fail(" in fns["bk_load_book"]
    # the reset: fold in front of the books' reset, the cut behind it, and still two loops
    reset = fns["reset_books_from"]
    fold, go, cut = (reset.index(x) for x in ("launch_flow_fold(env", "launch_reset_books(", "launch_flow_clear(env, mask_dev, env->M, true)"))
    assert fold < go < cut and len(re.findall(r"\bfor \(", reset)) == 2
    assert "launch_flow_clear(env, mask_dev, env->M, true)" in fns["bk_ingress_reset_books_device"]
    assert "launch_flow_clear(env, nullptr, 1, false)" in fns["bk_checkpoint_load"]
    # the step: flow, bars, accounts in this order; the last fold consumes, once, if any of the three asked
    step = fns["bk_step_async"]
    order = [step.index(x) for x in ("launch_events<", "launch_flow_fold(env", "launch_bars_fold(env", "launch_accounts_fold(env")]
    assert order == sorted(order)
    assert "launch_flow_fold(env, env->flow_consume && !env->bars_window && !env->acct_traders);" in step
    assert "g.consume = !env->acct_traders && (env->bars_consume || env->flow_consume) ? 1u : 0u;" in fns["launch_bars_fold"]
    assert "g.consume = env->acct_consume || env->bars_consume || env->flow_consume ? 1u : 0u;" in fns["launch_accounts_fold"]
    # flow_consume is set by the enable alone (and taken back by its failure path): off, the expressions read as before
    assert re.findall(r"flow_consume = ([^;]+);", code) == ["false", "consume_trades != 0", "false"]


def test_the_flow_kernels_match_their_instruction_count_profile():
    """tools/kernel_isa_counts.py::measure lists only the kernels whose name starts with k_ once "void bkd::" is stripped, so
    profiles/kernel_isa_baseline.json holds no kernel of a namespace; the two flow kernels' counts by issue class and their
    loop spans are pinned in profiles/kernel_isa_flow.json instead, within the baseline's 3 % (+-2 instructions always pass).
    The classes, not the total: the code object's padding stands behind whichever kernel comes last.  After an intended
    change of flow.hpp: write the new counts into the profile."""
    import json

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_isa_counts as K
    from bourse_amd import _build

    lib = _build.build()
    ks = {}
    with tempfile.TemporaryDirectory(prefix="bourse_flow_isa_") as tmp:
        for co in K.code_objects(lib, tmp):
            ks.update(K.kernels_of(co))
    names = K.demangle(sorted(ks))
    now = {names[n].replace("bkd::", ""): v for n, v in ks.items() if "flow::k_" in names[n]}
    base = json.load(open(os.path.join(ROOT, "profiles", "kernel_isa_flow.json")))["kernels"]
    assert sorted(now) == sorted(base) == ["flow::k_clear", "flow::k_fold"], (sorted(now), sorted(base))

    def off(a, b):
        return abs(a - b) > max(2, K.TOL * max(a, b))

    for k in base:
        for c in ("salu", "branch", "valu", "lds", "vmem", "smem"):
            assert not off(base[k]["counts"][c], now[k]["counts"][c]), (k, c, base[k]["counts"][c], now[k]["counts"][c])
        assert len(base[k]["loops"]) == len(now[k]["loops"]), (k, base[k]["loops"], now[k]["loops"])
        assert not [1 for x, y in zip(base[k]["loops"], now[k]["loops"]) if off(x, y)], (k, base[k]["loops"], now[k]["loops"])
    assert 40 <= min(l for l in now["flow::k_fold"]["loops"] if l >= 40) <= 60  # the walk: about 52 instructions per record


def test_the_kernels_are_plain_share_their_rules_with_the_cpu_test_and_use_no_scratch():
    src = open(os.path.join(CSRC, "flow.hpp")).read()
    code = re.sub(r"//.*", "", src)
    assert re.search(r"namespace bkd \{\s*namespace flow \{", code)
    for k in ("k_fold", "k_clear"):
        assert re.search(r"__global__[^;{]*\b" + k + r"\(", code), k
    assert "asm" not in code and "atomic" not in code and "extern __shared__" not in code
    assert '#include "flow_fold.hpp"' in src
    for f in ("plan(", "carry_src(", "add_record(", "add_pair(", "merge(", "word_of(", "carry_at(", "rec_at(", "WINDOW_WORDS"):
        assert f in code, f
    fold = open(os.path.join(CSRC, "flow_fold.hpp")).read()
    assert re.search(r"namespace bkd \{\s*namespace flow \{", fold)
    assert "hip_runtime" not in fold and "asm" not in re.sub(r"//.*", "", fold)
    # wave_sum_u32 / wave_sum_u64 are written once, beside wave_add
    defs = {f: len(re.findall(r"uint64_t wave_sum_u(?:32|64)\(", re.sub(r"//.*", "", open(os.path.join(CSRC, f)).read())))
            for f in os.listdir(CSRC) if f.endswith((".hpp", ".hip", ".inc"))}
    assert {f: n for f, n in defs.items() if n} == {"book_device.hpp": 2}, defs
    # the metadata of the built library (what tools/kernel_resources.py reports as ScratchSize and LDS Size)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_isa_counts as K
    from bourse_amd import _build

    lib = _build.build()
    meta = {}
    with tempfile.TemporaryDirectory(prefix="bourse_flow_") as tmp:
        for co in K.code_objects(lib, tmp):
            txt = subprocess.run([K._tool("llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
            for blk in re.split(r"\n\s+- \.agpr_count:", txt):
                name = re.search(r"\.name:\s+(\S+)", blk)
                if name and "4flow" in name.group(1):
                    meta[name.group(1)] = {k: int(v) for k, v in re.findall(r"\.(private_segment_fixed_size|group_segment_fixed_size|vgpr_count|sgpr_count):\s+(\d+)", blk)}
    assert len(meta) == 2, meta
    for name, m in meta.items():
        assert m["private_segment_fixed_size"] == 0, (name, m)
        assert m["group_segment_fixed_size"] % 16 == 0 and m["vgpr_count"] <= 64, (name, m)
    fold_meta = [m for n, m in meta.items() if "k_fold" in n][0]
    assert fold_meta["group_segment_fixed_size"] == 4 * (64 + 64) * 8  # FOLD_WAVES windows of WINDOW_WORDS 8-byte words
