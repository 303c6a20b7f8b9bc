"""CPU test of the rule that picks bk_run's kernels (bourse_amd/csrc/pipeline_plan.hpp) against a table of expected plans."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pipeline_plan_matches_the_expected_table(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path / "pipeline_plan_test")
    res = subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "pipeline_plan_test.cpp"),
                          "-o", exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    run = subprocess.run([exe, os.path.join(ROOT, "tests", "cpp", "pipeline_plan_expected.txt")], capture_output=True, text=True,
                         timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "pipeline_plan ok: 3672 rows, 117504 points" in run.stdout
