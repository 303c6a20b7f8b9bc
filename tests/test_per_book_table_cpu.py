"""CPU tests of bk_set_random_agents_per_book's host side: the table builder (bourse_amd/csrc/agent_table.hpp, compiled with
g++ - records, status codes with the unit named, n_agents mismatch, hash), the Python shape checks of
ManyBookEnv.set_random_agents_per_book, and a C++ client of ManyEnv::set_random_agents_per_book that compiles, links and
fails loudly without a GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_table_builder_records_codes_and_hash(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path / "per_book_table_test")
    res = subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "per_book_table_test.cpp"),
                          "-o", exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "per_book_table ok: 37 units x 3 groups" in run.stdout


def test_python_table_shapes_and_dtype():
    from bourse_amd import RANDOM_AGENTS_DTYPE, env as E

    assert RANDOM_AGENTS_DTYPE.itemsize == 28
    rows = [[(64, (10, 20), (1, 5), 2, 0.5), (32, (30, 40), (2, 9), 4, 1.0)] for _ in range(3)]
    arr = E._agents_table(rows, 3, lambda g: g)
    assert arr.shape == (3, 2) and arr.dtype == RANDOM_AGENTS_DTYPE and arr.flags.c_contiguous
    assert tuple(arr[1, 1]) == (32, 30, 40, 2, 9, 4, np.float32(1.0))
    assert E._agents_table(arr, 3, lambda g: g) is not None
    with pytest.raises(ValueError):
        E._agents_table(rows[:2], 3, lambda g: g)  # one row per unit
    with pytest.raises(ValueError):
        E._agents_table(rows[:2] + [rows[0][:1]], 3, lambda g: g)  # ragged
    with pytest.raises(ValueError):
        E._agents_table(arr[:2], 3, lambda g: g)
    with pytest.raises(ValueError):
        E._agents_table(arr.reshape(-1), 3, lambda g: g)


def test_cpp_client_of_the_per_book_table_compiles_and_fails_loudly_without_gpu(tmp_path):
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present: the GPU suite runs the table (tests/test_gpu_per_book_agents.py)")
    import bourse_amd._build as b

    b.build()
    src = tmp_path / "per_book_client.cpp"
    src.write_text(r'''
#include <cstdio>
#include "bourse_amd.hpp"
int main() {
  try {
    bourse_amd::ManyEnv env(4, 101, 0, 1, 1000);
    std::vector<std::vector<bk_random_agents>> table(4, std::vector<bk_random_agents>{{64, 10, 20, 1, 5, 1, 0.5f}});
    for (uint32_t b = 0; b < 4; ++b) table[b][0].tick_hi = 21 + b;
    env.set_random_agents_per_book(table);
    env.run(5);
    std::printf("per_book_client: ran\n");
  } catch (const bourse_amd::Error& e) {
    std::printf("%s\n", e.what());
    return e.code == BK_NO_DEVICE ? 77 : 1;
  }
  return 0;
}
''')
    lib_dir = os.path.join(ROOT, "bourse_amd", "csrc")
    exe = str(tmp_path / "per_book_client")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-L",
                    lib_dir, "-lbourse_amd", f"-Wl,-rpath,{lib_dir}", "-o", exe], check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 77 and "no CPU execution path" in r.stdout, r.stdout + r.stderr
