"""How accumulate_hydro_p / accumulate_rho_p are dispatched (plan_moments) and how the 14 fixed-point scales of the
deterministic hydro sums are chosen (moment_scales), both in old-vpic_amd/csrc/policy.h, without a GPU:
tests/moments_policy_check.cpp, built with the host compiler, drives one named case per rule."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["tile_order_sums_by_tile", "tile_order_needs_partition_and_no_movers", "deterministic_sorts_by_tile_first",
         "deterministic_falls_back_to_per_particle", "float_untiled_is_the_old_path", "knob",
         "scales_convert", "scales_sum", "scales_resolve"]


def build_driver(directory):
    exe = os.path.join(str(directory), "moments_policy_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Werror",
                           "-I", os.path.join(ROOT, "old-vpic_amd", "csrc"),
                           os.path.join(ROOT, "tests", "moments_policy_check.cpp"), "-o", exe])
    return exe


def moment_scale_exponents(exe, q_max, q_m, r8V, c):
    """log2 of the 14 scales moment_scales chooses"""
    out = subprocess.run([exe, "--scales", repr(float(q_max)), repr(float(q_m)), repr(float(r8V)), repr(float(c))],
                         capture_output=True, text=True, check=True).stdout.split()
    assert len(out) == 14
    return [int(v) for v in out]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_driver(tmp_path_factory.mktemp("moments_policy"))


def test_policy_header_is_still_plain_cpp():
    src = open(os.path.join(ROOT, "old-vpic_amd", "csrc", "policy.h")).read()
    assert "#include <hip" not in src and '#include "hip' not in src
    assert "plan_moments" in src and "moment_scales" in src


def test_every_case_is_listed(driver):
    out = subprocess.run([driver, "--list"], capture_output=True, text=True, check=True).stdout.split()
    assert out == CASES


@pytest.mark.parametrize("case", CASES)
def test_moments_policy(driver, case):
    r = subprocess.run([driver, case], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok " + case, r.stdout + r.stderr


def test_scales_of_the_gpu_test_deck(driver):
    """unit cells, |q| <= 0.015, q_m = -1, c = 1: W = 0.015, every bound is W, frexp(0.015) = 0.96 x 2^-6: 2^(36 + 6); the
    off-diagonal stresses reach W / 2 only: one power of two more"""
    assert moment_scale_exponents(driver, 0.015, -1.0, 0.125, 1.0) == [42] * 11 + [43] * 3
