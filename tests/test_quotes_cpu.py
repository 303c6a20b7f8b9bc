"""bk_submit_quotes without a GPU: the plain-Python model (tests/quotes_model.py) against grids worked out by hand, the kernel's
per-position decision (bourse_amd/csrc/quote_rows.hpp, compiled with g++) against the model over random entry tables and quote
rows at depth 1, 3, 8 and 64, the C ABI - the entries are exported, bound and declared, refuse a null env and null quotes,
bk_quote is laid out as the dtype, no flag bit was added - the layout of the kernel's source, and the busy flow of
tests/test_gpu_quotes.py run on the expected side alone with its conditions asserted."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import quotes_cases as QC
import quotes_model as QM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("bk_submit_quotes_device", "bk_submit_quotes")
BK_INVALID_ARGUMENT = 5
F = 0xFFFFFFFF
KEEP = QM.KEEP
NONE = (F, 0, 0, 0)
O, cancel, grid_rows, new, reduce = QC.O, QC.cancel, QC.grid_rows, QC.new, QC.reduce


def test_the_model_against_grids_worked_out_by_hand():
    # depth 3, G = 5.  Entries are (order id, price, remaining volume, side_is_bid) in ascending id.
    # a keeper with equal volume: nothing at all
    assert grid_rows([[(4, 100, 10, 1), (5, 104, 7, 0), NONE]], [(100, 10, 104, 7)], 3) == [O, O, O, O, O]
    # a keeper with larger volume is reduced in place; the ask's keeper holds less: it stays and the top-up follows
    assert grid_rows([[(4, 100, 10, 1), (5, 104, 7, 0), NONE]], [(100, 6, 104, 9)], 3) == [
        reduce(0, 4, 6), O, O, O, new(0, 0, 104, 2)]
    # two listed orders at the target price: the older one keeps, the younger one goes; the bid at another price goes too
    assert grid_rows([[(2, 100, 3, 1), (6, 99, 1, 1), (9, 100, 8, 1)]], [(100, 5, 0, KEEP)], 3) == [
        O, cancel(0, 6), cancel(0, 9), new(0, 1, 100, 2), O]
    # a KEEP side beside a pulled side, and the reverse
    assert grid_rows([[(1, 100, 10, 1), (2, 104, 7, 0), (3, 105, 7, 0)]], [(0, KEEP, 104, 0)], 3) == [
        O, cancel(0, 2), cancel(0, 3), O, O]
    assert grid_rows([[(1, 100, 10, 1), (2, 104, 7, 0), (3, 105, 7, 0)]], [(100, 0, 0, KEEP)], 3) == [
        cancel(0, 1), O, O, O, O]
    # a moved price: a cancel and a new order
    assert grid_rows([[(1, 100, 10, 1), NONE, NONE]], [(98, 10, 0, KEEP)], 3) == [cancel(0, 1), O, O, new(0, 1, 98, 10), O]
    # an empty trader: two fresh orders; with KEEP and 0 nothing
    assert grid_rows([[NONE, NONE, NONE]], [(100, 5, 104, 6)], 3) == [O, O, O, new(0, 1, 100, 5), new(0, 0, 104, 6)]
    assert grid_rows([[NONE, NONE, NONE]], [(100, 0, 104, KEEP)], 3) == [O, O, O, O, O]
    # a trader whose entries are all of the other side: the asks are untouched by the bid's target, even at an equal price
    assert grid_rows([[(1, 100, 4, 0), (2, 100, 5, 0), (3, 101, 6, 0)]], [(100, 9, 0, KEEP)], 3) == [
        O, O, O, new(0, 1, 100, 9), O]
    # two traders: the second one's elements carry trader 1 and follow the first one's five positions
    assert grid_rows([[NONE, NONE, NONE], [(7, 50, F - 1, 1), NONE, NONE]], [(0, KEEP, 0, KEEP), (50, 1, 60, F - 1)], 3) == [
        O, O, O, O, O, reduce(1, 7, 1), O, O, O, new(1, 0, 60, F - 1)]
    # depth 1: the listed order is all the model sees
    assert grid_rows([[(3, 10, 2, 0)]], [(8, 1, 10, 5)], 1) == [O, new(0, 1, 8, 1), new(0, 0, 10, 3)]
    off, ins = QC.join([QM.expand([[NONE]], [(8, 1, 0, 0)], 1), QM.expand([[NONE]], [(0, KEEP, 0, KEEP)], 1)])
    assert off.tolist() == [0, 3, 6] and ins[0].tolist() == [0, 1, 0, 0, 0, 0] and ins[1].dtype == np.uint8 and ins[5].dtype == np.uint64


def _random_case(rng, depth):
    """a trader's packed list (ascending id, the used entries first) and a quote row; prices from a small set so keepers are
    common, now and then the same price on both sides, volumes up to 0xFFFFFFFE"""
    prices = [int(x) for x in rng.choice([0, 1, 100, 101, 102, F], size=3, replace=False)]
    n = int(rng.integers(0, depth + 1))
    ids = sorted(int(x) for x in rng.choice(1 << 16, size=n, replace=False))
    if rng.random() < 0.2:
        ids = [i + 0xFFFE0000 for i in ids]

    def volume():
        u = rng.random()
        return F - 1 if u < 0.15 else int(rng.integers(1, 6)) if u < 0.7 else int(rng.integers(1, 1 << 32) % (F - 1)) + 1

    entries = [(i, int(rng.choice(prices)), volume(), int(rng.integers(0, 2))) for i in ids] + [NONE] * (depth - n)

    def side():
        u = rng.random()
        return (int(rng.choice(prices)), KEEP if u < 0.15 else 0 if u < 0.3 else volume())

    bid, ask = side(), side()
    if rng.random() < 0.3:
        ask = (bid[0], ask[1])  # prices equal on both sides
    return entries, bid + ask


def test_quote_rows_hpp_equals_the_model(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path / "quote_rows_test")
    res = subprocess.run([gxx, "-std=c++17", "-O2", os.path.join(ROOT, "tests", "cpp", "quote_rows_test.cpp"), "-o", exe],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    rng = np.random.default_rng(23)
    cases = [(d,) + _random_case(rng, d) for d in (1, 3, 8, 64) for _ in range(900)]
    want, seen = [], {}
    with open(tmp_path / "cases.txt", "w") as f:
        f.write(f"{len(cases)}\n")
        for depth, entries, quote in cases:
            f.write(f"{depth}\n" + "".join("%d %d %d %d\n" % e for e in entries) + "%d %d %d %d\n" % quote)
            c = {}
            g = QM.expand([entries], [quote], depth, c)
            want += [[int(g[0][i]), int(g[1][i]), int(g[2][i]), int(g[4][i]), int(g[5][i])] for i in range(depth + 2)]
            for w in QC.WORDS:
                seen[w] = seen.get(w, 0) + c.get(w, 0)
            seen["huge"] = seen.get("huge", 0) + int((g[2] == F - 1).sum())
            seen["same price"] = seen.get("same price", 0) + (quote[0] == quote[2])
    assert min(seen.values()) > 100, seen
    run = subprocess.run([exe, str(tmp_path / "cases.txt"), str(tmp_path / "grid.txt")], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip().endswith(f"quote_rows ok {len(cases)} cases")
    got = [[int(x) for x in line.split()] for line in open(tmp_path / "grid.txt")]
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"grid position {i}: {g} vs {w}"


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
    assert callable(bourse_amd.ManyBookEnv.submit_quotes)
    assert bourse_amd.ManyMarketEnv.submit_quotes is bourse_amd.ManyBookEnv.submit_quotes
    assert bourse_amd.QUOTE_DTYPE is _lib.QUOTE_DTYPE and "QUOTE_DTYPE" in bourse_amd.__all__ and "QUOTE_KEEP" in bourse_amd.__all__
    assert bourse_amd.QUOTE_KEEP == bourse_amd.ManyBookEnv.QUOTE_KEEP == F
    assert re.search(r"#define BK_QUOTE_KEEP 0xFFFFFFFFu", header)
    hpp = open(os.path.join(ROOT, "include", "bourse_amd.hpp")).read()
    for method in ("submit_quotes_device", "submit_quotes"):
        assert re.search(r"\b" + method + r"\(", hpp), method
    rs = open(os.path.join(ROOT, "integration", "rust", "bourse_amd_sys.rs")).read()
    for name in ENTRIES:
        assert re.search(r"pub fn " + name + r"\(", rs), name
    assert "pub struct BkQuote" in rs and "pub ask_vol: u32" in rs and "pub const BK_QUOTE_KEEP: u32 = 0xFFFFFFFF;" in rs
    md = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ENTRIES:
        assert name in md, name


def test_no_flag_bit_was_added():
    from bourse_amd import _lib

    header = open(os.path.join(ROOT, "include", "bourse_amd.h")).read()
    taken = sorted(int(v) for v in re.findall(r"#define BK_FLAG_\w+ (\d+)u", header))
    assert taken == [1, 2, 4, 8, 16, 32, 64, 128, 256, 512], taken
    assert sorted(_lib.FLAG_NAMES) == [1, 2, 4, 8, 16, 32, 64, 128, 256, 512]


def test_the_struct_is_laid_out_as_the_dtype(tmp_path):
    from bourse_amd import _lib

    q = _lib.QUOTE_DTYPE
    assert q.itemsize == 16 and q.names == ("bid_price", "bid_vol", "ask_price", "ask_vol")
    assert [q.fields[n][1] for n in q.names] == [0, 4, 8, 12]
    assert [q.fields[n][0].str for n in q.names] == ["<u4"] * 4
    assert ctypes.sizeof(_lib.Quote) == 16
    assert [(n, getattr(_lib.Quote, n).offset) for n, _ in _lib.Quote._fields_] == [(n, q.fields[n][1]) for n in q.names]
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    src = tmp_path / "layout.cpp"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "bourse_amd.h"\n'
                   'int main() { std::printf("%zu", sizeof(bk_quote));\n' +
                   "".join(f'std::printf(" %zu", offsetof(bk_quote, {n}));\n' for n in q.names) +
                   'std::printf(" %u", BK_QUOTE_KEEP);\nreturn 0; }\n')
    exe = str(tmp_path / "layout")
    res = subprocess.run([gxx, "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60).stdout.split()
    assert [int(x) for x in out] == [16, 0, 4, 8, 12, F]


def test_a_null_env_and_null_quotes_are_refused_not_dereferenced():
    from bourse_amd import _lib

    L = _lib.load()
    rows = np.zeros(4, dtype=_lib.QUOTE_DTYPE)
    calls = {
        "bk_submit_quotes_device": lambda: L.bk_submit_quotes_device(None, rows.ctypes.data_as(ctypes.c_void_p), None, None),
        "bk_submit_quotes": lambda: L.bk_submit_quotes(None, rows.ctypes.data_as(ctypes.c_void_p), None, None),
    }
    assert set(calls) == set(ENTRIES)
    for name, call in calls.items():
        L.bk_device_count(ctypes.byref(ctypes.c_int(0)))  # (anything that may leave another message behind)
        assert call() == BK_INVALID_ARGUMENT, name
        assert b"null env" in L.bk_last_error(), name


def test_the_kernel_stays_out_of_the_baselined_namespace_and_is_plain_hip():
    """bkd::quotes::k_submit is not among the names the ISA baseline lists, so profiles/kernel_isa_baseline.json stays as it is;
    the kernel is plain C++ - no inline assembly, no atomic, no LDS, no shuffle - takes no pool-size template, and shares its
    per-position decision with the CPU test through quote_rows.hpp."""
    import json

    src = open(os.path.join(ROOT, "bourse_amd", "csrc", "quotes_ingress.hpp")).read()
    body = src[src.index("namespace bkd {"):]
    assert re.search(r"namespace bkd \{\s*namespace quotes \{", body)
    assert re.search(r"__global__[^;{]*\bk_submit\(", body) and "template" not in body
    code = re.sub(r"//.*", "", src)
    assert "asm" not in code and "atomic" not in code and "__shared__" not in code and "__shfl" not in code
    assert '#include "quote_rows.hpp"' in src
    for f in ("no_keepers(", "see_entry(", "entry_element(", "new_element(", "write_new_order(", "lane_rank("):
        assert f in code, f
    rows = open(os.path.join(ROOT, "bourse_amd", "csrc", "quote_rows.hpp")).read()
    assert re.search(r"namespace bkd \{\s*namespace quotes \{", rows)
    assert "hip_runtime" not in rows and "asm" not in re.sub(r"//.*", "", rows)
    base = json.load(open(os.path.join(ROOT, "profiles", "kernel_isa_baseline.json")))["kernels"]
    assert not [k for k in base if "quotes" in k or "k_submit" in k]


@pytest.mark.parametrize("pool", [64, 512])
def test_the_busy_flow_meets_its_conditions_on_the_expected_side(oracle, pool):
    """tests/test_gpu_quotes.py's busy flow, the expected side alone: cancellations, in-place reductions, top-ups, fresh
    orders, untouched keepers, KEEP sides, pulled sides, partially filled keepers, a trader resting more than `depth` orders
    whose unlisted orders stay, and pools that never fill - known to hold before anyone has a GPU."""
    plan = QC.busy_plan(oracle, pool)
    QC.assert_busy(plan, pool)
    assert len(plan.steps) == 10 and plan.B == 6 and plan.NT == 5 and plan.depth == 3
    # the 25 positions of a book's grid cannot hold more than 64 live ones: that condition is the wide shape's
    assert 0 < plan.most_live_positions <= 25
    wide = QC.wide_plan(oracle)
    assert wide.most_live_positions > 64, wide.most_live_positions
