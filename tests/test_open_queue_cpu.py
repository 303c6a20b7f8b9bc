"""The queue view (bk_open_queue_enable) without a GPU: the plain-Python model against rows worked out by hand, the kernel's row
arithmetic (bourse_amd/csrc/open_queue_rows.hpp, compiled with g++) against the model over random pools of every pool size, the
C ABI - the entries are exported, bound and declared, refuse a null env, bk_open_queue is laid out as the dtype, no flag bit
was added - and the layout of the kernel's source."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import open_orders_model as OM
import open_queue_model as QM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("bk_open_queue_enable", "bk_open_queue_device_ptr", "bk_get_open_queue")
BK_INVALID_ARGUMENT = 5
ORDER = np.dtype([("order_id", "<u8"), ("trader_id", "<u4"), ("side", "u1"), ("status", "u1"), ("price", "<u4"), ("vol", "<u4")])
F = 0xFFFFFFFF
NONE = (F, 0, 0, 0)


def test_the_model_against_rows_worked_out_by_hand():
    """Bids at 100: ids 0, 1, 2 of volume 0xFFFFFFFF each, created in that order; id 0 was modified to a larger volume later
    (key time 50) and stands behind the two younger ids.  Id 3, a better bid of trader 9 (no row), is ahead of all three.
    Asks at 105: id 4 then id 5.  Id 6 is filled, id 7 cancelled: neither counts."""
    book = np.array([
        (0, 0, 1, 1, 100, F),
        (1, 0, 1, 1, 100, F),
        (2, 1, 1, 1, 100, F),
        (3, 9, 1, 1, 101, 7),
        (4, 0, 0, 1, 105, 3),
        (5, 1, 0, 1, 105, 2),
        (6, 1, 1, 2, 100, 9),
        (7, 0, 0, 3, 104, 1),
        (8, 1, 0, 1, 106, 11),   # a worse ask: behind both asks at 105, in no row's sums but its own
    ], dtype=ORDER)
    key_time = [50, 20, 30, 40, 5, 6, 1, 2, 3]
    entries = OM.rows_ints(book, 2, 3)[1]
    assert entries == [[(0, 100, F, 1), (1, 100, F, 1), (4, 105, 3, 0)], [(2, 100, F, 1), (5, 105, 2, 0), (8, 106, 11, 0)]]
    q = QM.rows(book, key_time, entries)
    assert q.dtype == QM.OPEN_QUEUE_DTYPE and q.shape == (2, 3)
    assert q[0].tolist() == [(7 + 2 * F, 2 * F, 3 * F, 3, 2),   # id 0: behind the better bid and both younger ids
                             (7, 0, 3 * F, 1, 0),               # id 1: first of its level, behind the better bid
                             (0, 0, 5, 0, 0)]                   # id 4: the front of the asks
    assert q[1].tolist() == [(7 + F, F, 3 * F, 2, 1),           # id 2
                             (3, 3, 5, 1, 1),                   # id 5: behind id 4 at its own price
                             (5, 0, 11, 2, 0)]                  # id 8: two better asks, alone at its level
    assert 7 + 2 * F > F  # the sums are 64-bit
    # an unused entry and an entry whose order does not rest have the all-zero row; depth 0 has no rows
    assert QM.rows(book, key_time, [[NONE, (6, 100, 9, 1)]]).tolist() == [[(0, 0, 0, 0, 0)] * 2]
    assert QM.rows(book, key_time, [[], []]).shape == (2, 0)
    # equal key times fall back on the id
    tied = QM.rows_ints(book, [20, 20, 20, 40, 5, 5, 1, 2, 3], [[(0, 100, F, 1), (1, 100, F, 1), (2, 100, F, 1), (5, 105, 2, 0)]])
    assert [r[4] for r in tied[0]] == [0, 1, 2, 1]


def _random_pool(rng, n_slots):
    live = rng.random(n_slots) < rng.random()
    ids = rng.choice(1 << 20, size=n_slots, replace=False).astype(np.uint64)
    if rng.random() < 0.3:
        ids += np.uint64(0xFFF00000)  # ids near the top of the u32 range
    vol = rng.integers(0, 1 << 32, size=n_slots)
    if rng.random() < 0.3:
        vol[:] = F
    mode = rng.random()
    if mode < 0.5:
        price = rng.integers(1000, 1000 + int(rng.integers(1, 12)), size=n_slots)  # a few levels, long queues
    elif mode < 0.8:
        price = rng.integers(0, 4, size=n_slots) * 0x55555555  # ties, 0 and 0xFFFFFFFF among the prices
    else:
        price = rng.integers(0, 1 << 32, size=n_slots)
    side = rng.integers(0, 2, size=n_slots)
    seq = rng.choice(1 << 16, size=n_slots, replace=False).astype(np.uint64)  # unique per book, in no order of id or slot
    if rng.random() < 0.3:
        seq += np.uint64(0xFFFF0000)  # stamps compare as unsigned
    n_entries = int(rng.integers(1, 140))
    live_ids, dead_ids = ids[live], ids[~live]
    listed = []
    for _ in range(n_entries):
        u = rng.random()
        if u < 0.7 and len(live_ids):
            listed.append(int(rng.choice(live_ids)))
        elif u < 0.8 and len(dead_ids):
            listed.append(int(rng.choice(dead_ids)))  # listed, but not live in the pool
        else:
            listed.append(F)
    return live, ids, price, vol, side, seq, listed


def test_open_queue_rows_hpp_equals_the_model(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path / "open_queue_rows_test")
    res = subprocess.run([gxx, "-std=c++17", "-O2", os.path.join(ROOT, "tests", "cpp", "open_queue_rows_test.cpp"), "-o", exe],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    rng = np.random.default_rng(19)
    pools = [_random_pool(rng, n) for n in (64, 128, 256, 512) for _ in range(600)]
    want, wide, deep, level, dead, unused = [], 0, 0, 0, 0, 0
    with open(tmp_path / "pools.txt", "w") as f:
        f.write(f"{len(pools)}\n")
        for live, ids, price, vol, side, seq, listed in pools:
            f.write(f"{len(ids)} {len(listed)}\n")
            f.write("".join(f"{int(live[i])} {ids[i]} {price[i]} {vol[i]} {side[i]} {seq[i]}\n" for i in range(len(ids))))
            book = np.zeros(len(ids), dtype=ORDER)
            book["order_id"], book["side"], book["price"], book["vol"] = ids, side, price, vol
            book["status"] = np.where(live, 1, 2)
            at = {int(i): k for k, i in enumerate(ids)}
            key_time = {int(i): int(seq[k]) for i, k in at.items()}
            entries = [(i, int(price[at[i]]), int(vol[at[i]]), int(side[at[i]])) if i != F else NONE for i in listed]
            f.write("".join(f"{e[0]} {e[1]} {e[3]}\n" for e in entries))
            for e, r in zip(entries, QM.rows_ints(book, key_time, [entries])[0]):
                want.append([r[0] & F, r[0] >> 32, r[1] & F, r[1] >> 32, r[2] & F, r[2] >> 32, r[3], r[4]])
                wide += r[0] >> 32 != 0
                deep += r[3] > 64
                level += r[4] >= 2
                dead += e[0] != F and not live[at[e[0]]]
                unused += e[0] == F
    assert min(wide, deep, level, dead, unused) > 100, (wide, deep, level, dead, unused)
    run = subprocess.run([exe, str(tmp_path / "pools.txt"), str(tmp_path / "rows.txt")], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip().endswith(f"open_queue_rows ok {len(pools)} pools")
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
    for method in ("enable_open_queue", "open_queue", "open_queue_device_ptr", "open_queue_view"):
        assert callable(getattr(bourse_amd.ManyBookEnv, method)), method
        assert getattr(bourse_amd.ManyMarketEnv, method) is getattr(bourse_amd.ManyBookEnv, method), method
    assert bourse_amd.OPEN_QUEUE_DTYPE is _lib.OPEN_QUEUE_DTYPE and "OPEN_QUEUE_DTYPE" in bourse_amd.__all__
    hpp = open(os.path.join(ROOT, "include", "bourse_amd.hpp")).read()
    for method in ("enable_open_queue", "open_queue", "open_queue_device_ptr"):
        assert re.search(r"\b" + method + r"\(", hpp), method
    rs = open(os.path.join(ROOT, "integration", "rust", "bourse_amd_sys.rs")).read()
    for name in ENTRIES:
        assert re.search(r"pub fn " + name + r"\(", rs), name
    assert "pub struct BkOpenQueue" in rs and "pub level_ahead_vol: u64" in rs and "pub level_ahead_orders: u32" in rs
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

    q = _lib.OPEN_QUEUE_DTYPE
    assert q.itemsize == 32 and q.names == ("ahead_vol", "level_ahead_vol", "level_vol", "ahead_orders", "level_ahead_orders")
    assert [q.fields[n][1] for n in q.names] == [0, 8, 16, 24, 28]
    assert [q.fields[n][0].str for n in q.names] == ["<u8", "<u8", "<u8", "<u4", "<u4"]
    assert q == QM.OPEN_QUEUE_DTYPE
    assert ctypes.sizeof(_lib.OpenQueue) == 32
    assert [(n, getattr(_lib.OpenQueue, n).offset) for n, _ in _lib.OpenQueue._fields_] == [(n, q.fields[n][1]) for n in q.names]
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    src = tmp_path / "layout.cpp"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "bourse_amd.h"\n'
                   'int main() { std::printf("%zu", sizeof(bk_open_queue));\n' +
                   "".join(f'std::printf(" %zu", offsetof(bk_open_queue, {n}));\n' for n in q.names) + "return 0; }\n")
    exe = str(tmp_path / "layout")
    res = subprocess.run([gxx, "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60).stdout.split()
    assert [int(x) for x in out] == [32, 0, 8, 16, 24, 28]


def test_a_null_env_is_refused_not_dereferenced():
    from bourse_amd import _lib

    L = _lib.load()
    a = ctypes.c_void_p()
    rows = np.zeros(4, dtype=_lib.OPEN_QUEUE_DTYPE)
    calls = {
        "bk_open_queue_enable": lambda: L.bk_open_queue_enable(None),
        "bk_open_queue_device_ptr": lambda: L.bk_open_queue_device_ptr(None, ctypes.byref(a)),
        "bk_get_open_queue": lambda: L.bk_get_open_queue(None, 0, 1, rows.ctypes.data_as(ctypes.c_void_p)),
    }
    assert set(calls) == set(ENTRIES)
    for name, call in calls.items():
        L.bk_device_count(ctypes.byref(ctypes.c_int(0)))  # (anything that may leave another message behind)
        assert call() == BK_INVALID_ARGUMENT, name
        assert b"null env" in L.bk_last_error(), name


def test_the_kernel_stays_out_of_the_baselined_namespace_and_is_plain_hip():
    """bkd::open_queue::k_refresh is not among the names the ISA baseline lists, so profiles/kernel_isa_baseline.json stays as
    it is; the kernel is plain C++ - no inline assembly, no atomic, no LDS, no shuffle - reads pool facts only (never the
    order records) and shares its row arithmetic with the CPU test through open_queue_rows.hpp."""
    import json

    src = open(os.path.join(ROOT, "bourse_amd", "csrc", "open_queue.hpp")).read()
    body = src[src.index("namespace bkd {"):]
    assert re.search(r"namespace bkd \{\s*namespace open_queue \{", body)
    assert re.search(r"__global__[^;{]*\bk_refresh\(", body)
    code = re.sub(r"//.*", "", src)
    assert "asm" not in code and "atomic" not in code and "__shared__" not in code and "__shfl" not in code
    assert "dorders" not in code and "max_orders" not in code
    assert '#include "open_queue_rows.hpp"' in src
    for f in ("empty_row(", "place(", "add_order(", "row_words("):
        assert f in code, f
    rows = open(os.path.join(ROOT, "bourse_amd", "csrc", "open_queue_rows.hpp")).read()
    assert re.search(r"namespace bkd \{\s*namespace open_queue \{", rows)
    assert "hip_runtime" not in rows and "asm" not in re.sub(r"//.*", "", rows)
    base = json.load(open(os.path.join(ROOT, "profiles", "kernel_isa_baseline.json")))["kernels"]
    assert not [k for k in base if "open_queue" in k or "k_refresh" in k]
