"""CPU test of the order-log rule of bk_run's pipeline plan (bourse_amd/csrc/pipeline_plan.hpp PlanInput::order_log /
Plan::step_log): a logging RandomAgents env never runs a fused kernel, its event kernel is the logging one exactly on the
split kinds outside bk_warm, and every other choice is the plan of that split kind."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_order_log_plan_over_the_grid(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path / "agent_order_log_plan_test")
    res = subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-Werror",
                          os.path.join(ROOT, "tests", "cpp", "agent_order_log_plan_test.cpp"), "-o", exe],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    run = subprocess.run([exe, os.path.join(ROOT, "tests", "cpp", "pipeline_plan_expected.txt")], capture_output=True,
                         text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "agent_order_log_plan ok: 3672 shapes, 117504 points" in run.stdout
