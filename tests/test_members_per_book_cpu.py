"""CPU tests of bk_set_agents_per_book (AgentSet members with parameters per book or market): the host table builder
(bourse_amd/csrc/agent_table.hpp, compiled with g++ - records equal to the uniform call's per row, status codes with the
unit and member named, type / n_agents mismatch, hash), the pipeline plan's members_per_book over the plan grid, the
Python shape checks of ManyBookEnv.set_agents_per_book / ManyMarketEnv.set_market_agents_per_market, a C++ client of
ManyEnv::set_agents_per_book that compiles, links and fails loudly without a GPU, and the PB kernels on the
instruction-count yardstick of tools/kernel_isa_counts.py."""
import os
import re
import shutil
import subprocess
import sys
import tempfile
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

NOISE_P = dict(tick_size=2, p_limit=0.2, p_market=0.2, p_cancel=0.1, trade_vol=100, price_dist_mu=0.0, price_dist_sigma=1.0)
MOM_P = dict(tick_size=2, p_cancel=0.1, trade_vol=100, decay=1.0, demand=5.0, scale=0.5, order_ratio=1.0, price_dist_mu=0.0,
             price_dist_sigma=10.0)


def _compile_and_run(tmp_path, name, *args):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path / name)
    res = subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-o",
                          exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    run = subprocess.run([exe, *args], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    return run.stdout


def test_table_builder_records_codes_and_hash(tmp_path):
    out = _compile_and_run(tmp_path, "members_per_book_table_test")
    assert "members_per_book_table ok: 29 units x 4 members" in out


def test_plan_sets_members_per_book_and_changes_nothing_else(tmp_path):
    out = _compile_and_run(tmp_path, "members_per_book_plan_test", os.path.join(ROOT, "tests", "cpp", "pipeline_plan_expected.txt"))
    assert "members_per_book_plan ok: 3672 shapes, 235008 points" in out


class _Recorder:
    """Stands in for the library: records bk_set_agents_per_book's arguments."""

    def __init__(self):
        self.calls = []

    def bk_set_agents_per_book(self, h, n, arr, assets):
        self.calls.append((n, [(d.type, d.n_agents, d.tick_size, d.p_limit, d.price_dist_sigma, d.tick_hi) for d in arr],
                           None if assets is None else [assets[i] for i in range(n)]))
        return 0


def _stub(cls, **attrs):
    from bourse_amd import env as E

    s = types.SimpleNamespace(_h=None, _L=_Recorder(), **attrs)
    s._set_members_table = types.MethodType(E.ManyBookEnv._set_members_table, s)
    return s


def test_python_table_shapes_and_flattening():
    from bourse_amd import env as E

    rows = [[("noise", 0, 20, dict(NOISE_P, p_limit=0.25 * b)), ("momentum", 20, 10, dict(MOM_P, price_dist_sigma=float(b)))]
            for b in range(3)]
    s = _stub(E.ManyBookEnv, assets=1, n_books=3)
    E.ManyBookEnv.set_agents_per_book(s, rows)
    n, descs, assets = s._L.calls[-1]
    assert n == 2 and assets is None and len(descs) == 6
    assert [d[0] for d in descs] == [1, 2] * 3 and [d[1] for d in descs] == [20, 10] * 3
    assert [d[3] for d in descs[0::2]] == [0.0, 0.25, 0.5] and [d[4] for d in descs[1::2]] == [0.0, 1.0, 2.0]
    # the instance format and RandomAgents members
    inst = [[E.RandomAgents(8, (10, 20 + b), (1, 5), 2, 0.5), E.NoiseAgent(8, 5, E.NoiseAgentParams(**NOISE_P))] for b in range(3)]
    E.ManyBookEnv.set_agents_per_book(s, inst)
    n, descs, _ = s._L.calls[-1]
    assert n == 2 and [d[5] for d in descs[0::2]] == [20, 21, 22] and [d[0] for d in descs] == [0, 1] * 3
    with pytest.raises(ValueError):
        E.ManyBookEnv.set_agents_per_book(s, rows[:2])  # one row per book
    with pytest.raises(ValueError):
        E.ManyBookEnv.set_agents_per_book(s, rows[:2] + [rows[0][:1]])  # ragged
    with pytest.raises(ValueError):
        E.ManyBookEnv.set_agents_per_book(s, [[], [], []])
    with pytest.raises(ValueError):
        E.ManyBookEnv.set_agents_per_book(_stub(E.ManyBookEnv, assets=2, n_books=6), rows)  # markets: the per-market call
    m = _stub(E.ManyMarketEnv, assets=2, n_markets=3)
    mrows = [[(1, r[0]), (0, r[1])] for r in rows]
    E.ManyMarketEnv.set_market_agents_per_market(m, mrows)
    n, descs, assets = m._L.calls[-1]
    assert n == 2 and assets == [1, 0] and len(descs) == 6
    with pytest.raises(ValueError):
        E.ManyMarketEnv.set_market_agents_per_market(m, mrows[:2])
    with pytest.raises(ValueError):  # the assets must be the same in every market
        E.ManyMarketEnv.set_market_agents_per_market(m, mrows[:2] + [[(0, rows[2][0]), (1, rows[2][1])]])


def test_cpp_client_of_the_members_table_compiles_and_fails_loudly_without_gpu(tmp_path):
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present: the GPU suite runs the table (tests/test_gpu_members_per_book.py)")
    import bourse_amd._build as b

    b.build()
    src = tmp_path / "members_client.cpp"
    src.write_text(r'''
#include <cstdio>
#include <cstring>
#include "bourse_amd.hpp"
int main() {
  try {
    bourse_amd::ManyEnv env(4, 101, 0, 1, 1000);
    bk_agent_desc d;
    std::memset(&d, 0, sizeof(d));
    d.type = BK_AGENT_NOISE;
    d.n_agents = 20;
    d.tick_size = 1;
    d.p_limit = d.p_market = 0.2f;
    d.p_cancel = 0.1f;
    d.trade_vol = 100;
    d.price_dist_sigma = 1.0;
    std::vector<std::vector<bk_agent_desc>> table(4, std::vector<bk_agent_desc>{d});
    for (uint32_t b = 0; b < 4; ++b) table[b][0].price_dist_sigma = 0.5 * b;
    env.set_agents_per_book(table);
    env.run(5);
    std::printf("members_client: ran\n");
  } catch (const bourse_amd::Error& e) {
    std::printf("%s\n", e.what());
    return e.code == BK_NO_DEVICE ? 77 : 1;
  }
  return 0;
}
''')
    lib_dir = os.path.join(ROOT, "bourse_amd", "csrc")
    exe = str(tmp_path / "members_client")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-L",
                    lib_dir, "-lbourse_amd", f"-Wl,-rpath,{lib_dir}", "-o", exe], check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 77 and "no CPU execution path" in r.stdout, r.stdout + r.stderr


# ------------------------------------------------------------------ the PB kernels in the built library
@pytest.fixture(scope="module")
def built():
    import kernel_isa_counts as K
    from bourse_amd import _build

    if not all(K._tool(t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-objdump", "llvm-readelf")):
        pytest.skip("no llvm-objdump / clang-offload-bundler / llvm-readelf")
    return _build.build()


def test_wave_decode_loops_of_the_per_book_form(built):
    import kernel_isa_counts as K

    counts = K.measure(built)
    for R in (1, 2, 4, 8):
        u, pb = counts[f"k_agents_mixed_wave<{R}>"], counts[f"k_agents_mixed_wave<{R}, true>"]
        assert len(u["loops"]) == len(pb["loops"]), R
        if R >= 4:  # the decode's window / walk loops and the member loop around them, instruction for instruction +-2
            assert all(abs(x - y) <= 2 for x, y in zip(u["loops"][:12], pb["loops"][:12])), (R, u["loops"], pb["loops"])
        else:  # (R <= 2: the row's address is one more live scalar pair in a kernel at the SGPR limit - a few more spill
            # moves per pass)
            assert all(abs(x - y) <= max(2, 0.01 * x) for x, y in zip(u["loops"][:12], pb["loops"][:12])), (R, u["loops"], pb["loops"])
        assert abs(u["counts"]["total"] - pb["counts"]["total"]) <= 0.01 * u["counts"]["total"], R
    for R in (1, 2, 4, 8):
        for k in (f"k_run_mixed<{R}", f"k_agents_mixed<{R}", f"k_agents_mixed_lanes<{R}, false", f"k_agents_mixed_lanes<{R}, true"):
            u, pb = counts[k + ">"], counts[k + ", true>"]
            assert abs(u["counts"]["total"] - pb["counts"]["total"]) <= 0.03 * u["counts"]["total"], k


def _scratch(lib):
    """{demangled kernel: private (scratch) bytes per lane} from the code objects' metadata - what hipcc's
    kernel-resource-usage report (tools/kernel_resources.py) calls ScratchSize."""
    import kernel_isa_counts as K

    out = {}
    with tempfile.TemporaryDirectory(prefix="bourse_res_") as tmp:
        for co in K.code_objects(lib, tmp):
            txt = subprocess.run([K._tool("llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
            for m in re.finditer(r"\.name:\s+(\S+)\n\s+\.private_segment_fixed_size:\s+(\d+)", txt):
                out[m.group(1)] = int(m.group(2))
    names = K.demangle(sorted(out))
    return {names[n]: v for n, v in out.items()}


def test_no_per_book_kernel_uses_scratch_where_its_uniform_sibling_does_not(built):
    sc = _scratch(built)
    pairs = []
    for R in (1, 2, 4, 8):
        pairs += [(f"k_run_mixed<{R}>", f"k_run_mixed<{R}, true>"), (f"k_agents_mixed<{R}>", f"k_agents_mixed<{R}, true>"),
                  (f"k_agents_mixed_wave<{R}>", f"k_agents_mixed_wave<{R}, true>")]
        pairs += [(f"k_agents_mixed_lanes<{R}, {m}>", f"k_agents_mixed_lanes<{R}, {m}, true>") for m in ("false", "true")]
    for u, pb in pairs:
        assert u in sc and pb in sc, (u, pb)
        assert sc[pb] <= sc[u], (pb, sc[pb], u, sc[u])
