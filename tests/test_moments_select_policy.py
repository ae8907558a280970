"""How accumulate_hydro_p_select is dispatched (plan_moments_select in old-vpic_amd/csrc/policy.h), without a GPU:
tests/moments_select_policy_check.cpp, built with the host compiler, drives one named case per rule -- a species whose
tile order is valid is summed by tile, any other per particle, and nothing is ever sorted, in both accumulation modes."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["tile_valid_is_tiled", "anything_else_is_per_particle", "never_a_sort"]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = os.path.join(str(tmp_path_factory.mktemp("moments_select_policy")), "moments_select_policy_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Werror",
                           "-I", os.path.join(ROOT, "old-vpic_amd", "csrc"),
                           os.path.join(ROOT, "tests", "moments_select_policy_check.cpp"), "-o", exe])
    return exe


def test_the_decision_stands_beside_plan_moments():
    src = open(os.path.join(ROOT, "old-vpic_amd", "csrc", "policy.h")).read()
    assert "#include <hip" not in src and '#include "hip' not in src
    assert src.index("inline MomentPlan plan_moments(") < src.index("inline MomentPlan plan_moments_select(")


def test_every_case_is_listed(driver):
    out = subprocess.run([driver, "--list"], capture_output=True, text=True, check=True).stdout.split()
    assert out == CASES


@pytest.mark.parametrize("case", CASES)
def test_moments_select_policy(driver, case):
    r = subprocess.run([driver, case], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok " + case, r.stdout + r.stderr
