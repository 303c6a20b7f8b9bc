"""CPU tests of the retune (bk_retune_*): the shared row text (bourse_amd/csrc/agent_rows.hpp, compiled with g++ against
the table builders and the floating-point definitions), the plain-Python model of "retune with a mask"
(tests/retune_model.py) against hand-written cases, and the ABI without a GPU."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import retune_model as RM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_shared_row_text_matches_the_table_builders(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path / "agent_rows_test")
    res = subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "agent_rows_test.cpp"),
                          "-o", exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    m = re.search(r"agent_rows ok: (\d+) rows", run.stdout)
    assert m and int(m.group(1)) > 8000, run.stdout


GOOD = (64, 10, 20, 1, 5, 2, 0.5)


def test_model_group_verdicts_by_hand():
    v = RM.group_verdict
    assert v(GOOD, 2, 64) == RM.OK
    assert v(GOOD, 1, 64) == RM.OK
    assert v((64, 10, 10, 1, 5, 2, 0.5), 2, 64) == RM.INVALID  # empty tick range
    assert v((64, 10, 20, 5, 5, 2, 0.5), 2, 64) == RM.INVALID  # empty vol range
    assert v((64, 10, 20, 1, 5, 3, 0.5), 2, 64) == RM.NOT_TICK_MULTIPLE
    assert v((64, 0, 20, 1, 5, 2, 0.5), 2, 64) == RM.INVALID  # tick_lo == 0
    assert v((64, 0, 20, 1, 5, 3, 0.5), 2, 64) == RM.NOT_TICK_MULTIPLE  # the tick check comes before the price bound
    assert v((64, 1, 0x55555556, 1, 5, 3, 0.5), 1, 64) == RM.INVALID  # 0x55555555 * 3 == u32::MAX: refused
    assert v((64, 1, 0x55555555, 1, 5, 3, 0.5), 1, 64) == RM.OK  # one tick below
    assert v((64, 1, 0xFFFFFFFF, 1, 5, 1, 0.5), 1, 64) == RM.OK  # top price u32::MAX - 1
    assert v(GOOD, 2, 65) == RM.INVALID  # n_agents is fixed
    assert v((64, 10, 20, 1, 5, 2, float("nan")), 2, 64) == RM.OK  # any rate is taken (NaN: never active)


def _noise(**kw):
    d = dict(type=RM.NOISE, n_agents=40, tick_lo=0, tick_hi=0, vol_lo=0, vol_hi=0, tick_size=2, activity_rate=0.0,
             agent_id_start=7, p_limit=0.3, p_market=0.1, p_cancel=0.2, trade_vol=10, reserved=0, price_dist_mu=1.5,
             price_dist_sigma=0.5, decay=0.0, demand=0.0, scale=0.0, order_ratio=0.0)
    d.update(kw)
    return d


def test_model_member_verdicts_by_hand():
    v = RM.member_verdict
    inst = _noise()
    assert v(_noise(p_limit=0.9, price_dist_mu=-2.0, trade_vol=99), 2, inst) == RM.OK
    assert v(_noise(tick_size=0), 2, inst) == RM.NOT_TICK_MULTIPLE
    assert v(_noise(tick_size=3), 2, inst) == RM.NOT_TICK_MULTIPLE
    for sigma in (-0.5, float("nan"), float("inf")):
        assert v(_noise(price_dist_sigma=sigma), 2, inst) == RM.INVALID
    assert v(_noise(price_dist_sigma=0.0), 2, inst) == RM.OK
    assert v(_noise(price_dist_mu=float("inf")), 2, inst) == RM.INVALID
    assert v(_noise(type=RM.MOMENTUM), 2, inst) == RM.INVALID  # the kind is fixed
    assert v(_noise(type=7), 2, inst) == RM.INVALID
    assert v(_noise(n_agents=41), 2, inst) == RM.INVALID
    assert v(_noise(agent_id_start=8), 2, inst) == RM.INVALID
    assert v(_noise(n_agents=65536), 2, _noise(n_agents=65536)) == RM.INVALID  # a u16 in the reference
    rnd = _noise(type=RM.RANDOM, tick_lo=10, tick_hi=20, vol_lo=1, vol_hi=5, activity_rate=0.5)
    assert v(rnd, 2, rnd) == RM.OK
    assert v(dict(rnd, tick_lo=0), 2, rnd) == RM.INVALID
    assert v(dict(rnd, vol_hi=1), 2, rnd) == RM.INVALID
    assert v(dict(rnd, tick_hi=0x80000001), 2, rnd) == RM.INVALID
    assert v(dict(rnd, tick_hi=0x80000000), 2, rnd) == RM.OK


def test_model_retune_is_all_or_nothing_per_unit():
    a, b, c = (64, 10, 20, 1, 5, 2, 0.5), (32, 30, 40, 2, 9, 4, 1.0), (8, 1, 2, 1, 2, 2, 0.0)
    table = [[a, b, c] for _ in range(5)]
    new = [[(64, 11, 21, 1, 5, 2, 0.25), (32, 31, 41, 2, 9, 4, 0.75), (8, 2, 3, 1, 2, 2, 1.0)] for _ in range(5)]
    new[1][2] = (8, 2, 3, 1, 2, 3, 1.0)  # unit 1: the last entry's tick is no multiple
    new[2][0] = (65, 11, 21, 1, 5, 2, 0.25)  # unit 2: n_agents changed in entry 0 ...
    new[2][1] = (32, 31, 31, 2, 9, 4, 0.75)  # ... and an empty range in entry 1: entry 0 is the one reported
    new[4][1] = (32, 0, 41, 2, 9, 4, 0.75)  # unit 4 is bad but unmasked: not read
    mask = [1, 1, 1, 0, 0]
    out, status, refused = RM.retune_groups(table, new, mask, [2])
    assert out[0] == new[0] and out[1] == table[1] and out[2] == table[2] and out[3] == table[3] and out[4] == table[4]
    assert status == [(0, 0), (RM.NOT_TICK_MULTIPLE, 2), (RM.INVALID, 0), (0, 0), (0, 0)]
    assert refused == 2
    out, status, refused = RM.retune_groups(table, new, None, [2])  # no mask: every unit
    assert refused == 3 and status[4] == (RM.INVALID, 1) and out[3] == new[3] and out[4] == table[4]
    # markets: entry j's tick is its installed asset's
    out, status, refused = RM.retune_groups(table[:1], [[a, (32, 30, 40, 2, 9, 6, 1.0), c]], None, [2, 4], assets=[0, 1, 0])
    assert status == [(RM.NOT_TICK_MULTIPLE, 1)] and refused == 1
    # members: the installed kind, size and first trader id come from the table
    mt = [[_noise(), _noise(type=RM.MOMENTUM, agent_id_start=100)] for _ in range(2)]
    mn = [[_noise(p_cancel=0.9), _noise(type=RM.MOMENTUM, agent_id_start=100, demand=5.0)],
          [_noise(p_cancel=0.9), _noise(type=RM.MOMENTUM, agent_id_start=101, demand=5.0)]]
    out, status, refused = RM.retune_members(mt, mn, None, [2])
    assert status == [(0, 0), (RM.INVALID, 1)] and refused == 1 and out[0] == mn[0] and out[1] == mt[1]


def test_abi_without_a_gpu():
    import bourse_amd
    from bourse_amd import _lib

    L = _lib.load()
    for name in ("bk_retune_random_agents_device", "bk_retune_random_agents", "bk_retune_agents_device", "bk_retune_agents",
                 "bk_retune_rejected"):
        assert hasattr(L, name) and name in _lib.SIGNATURES
    buf = (ctypes.c_uint8 * 256)()
    n = ctypes.c_uint64(5)
    assert L.bk_retune_random_agents_device(None, 1, buf, None, None) == RM.INVALID
    assert L.bk_retune_random_agents(None, 1, buf, None) == RM.INVALID
    assert L.bk_retune_agents_device(None, 1, buf, None, None) == RM.INVALID
    assert L.bk_retune_agents(None, 1, buf, None) == RM.INVALID
    assert L.bk_retune_rejected(None, ctypes.byref(n)) == RM.INVALID
    assert b"null" in L.bk_last_error()
    # the dtypes are the header's structs
    d = bourse_amd.AGENT_DESC_DTYPE
    assert d.itemsize == 104 == ctypes.sizeof(_lib.AgentDesc)
    for name, _ in _lib.AgentDesc._fields_:
        assert d.fields[name][1] == getattr(_lib.AgentDesc, name).offset, name
        assert d.fields[name][0].itemsize == getattr(_lib.AgentDesc, name).size, name
    assert list(d.names) == [n for n, _ in _lib.AgentDesc._fields_]
    r = bourse_amd.RANDOM_AGENTS_DTYPE
    assert r.itemsize == 28 == ctypes.sizeof(_lib.RandomAgentsCfg)
    for name, _ in _lib.RandomAgentsCfg._fields_:
        assert r.fields[name][1] == getattr(_lib.RandomAgentsCfg, name).offset, name
    # ... and the header's field order is the ctypes struct's
    hdr = open(os.path.join(ROOT, "include", "bourse_amd.h")).read()
    body = re.search(r"typedef struct bk_agent_desc \{(.*?)\} bk_agent_desc;", hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [f.strip() for decl in body.split(";") if decl.strip() for f in decl.strip().split(" ", 1)[1].split(",")]
    assert fields == list(d.names)


def test_python_rows_builders():
    from bourse_amd import AGENT_DESC_DTYPE, env as E

    rows = [[("noise", 7, 40, dict(tick_size=2, p_limit=0.3, p_market=0.1, p_cancel=0.2, trade_vol=10, price_dist_mu=1.5,
                                   price_dist_sigma=0.5)),
             ("random", 30, (10, 20), (1, 5), 2, 0.5)] for _ in range(3)]
    arr = E._members_rows(rows, 3)
    assert arr.shape == (3, 2) and arr.dtype == AGENT_DESC_DTYPE and arr.flags.c_contiguous
    assert arr[2, 0]["type"] == 1 and arr[2, 0]["agent_id_start"] == 7 and arr[2, 0]["price_dist_mu"] == 1.5
    assert arr[1, 1]["type"] == 0 and arr[1, 1]["tick_hi"] == 20 and arr[1, 1]["activity_rate"] == np.float32(0.5)
    assert E._members_rows(arr, 3) is not None
    with pytest.raises(ValueError):
        E._members_rows(rows[:2], 3)
    with pytest.raises(ValueError):
        E._members_rows(arr[:2], 3)
