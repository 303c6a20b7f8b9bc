"""CPU test of the per-unit parameter table's rule of bk_run's pipeline plan (bourse_amd/csrc/pipeline_plan.hpp
PlanInput::per_book / Plan::agents_per_book): the auto rule's choices stay, k_run_wave / wave_split / split run their PB
forms, the "fused" request's k_run_random takes the lane split, and k_step_decode stays off."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_per_book_plan_over_the_grid(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path / "per_book_plan_test")
    res = subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "per_book_plan_test.cpp"),
                          "-o", exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    run = subprocess.run([exe, os.path.join(ROOT, "tests", "cpp", "pipeline_plan_expected.txt")], capture_output=True,
                         text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "per_book_plan ok: 3672 shapes, 235008 points" in run.stdout
