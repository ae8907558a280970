"""THE RULE of vpic_hip_species_load_profile as the library compiles it (old-vpic_amd/csrc/load_rule.h), without a GPU:
tests/load_rule_check.cpp, built with the host compiler at -O2 -ffp-contract=off, runs 4096 slots through the header and
every word it prints is held == to the numpy restatement tests/load_ref.py -- the global cell, the voxel, positions and U
of the generator mode, positions and momenta of the draws mode.  The slots include global cells beyond 2^32, j beyond 2^16,
cells at rest (D2 == 0), cold cells (uth == 0), the flip on and off, and draws that sit exactly on the flip's threshold."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import load_ref as R  # noqa: E402

N_SLOTS = 4096


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = os.path.join(str(tmp_path_factory.mktemp("load_rule")), "load_rule_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror",
                           "-I", os.path.join(ROOT, "old-vpic_amd", "csrc"),
                           os.path.join(ROOT, "tests", "load_rule_check.cpp"), "-o", exe])
    return exe


def slots():
    rng = np.random.default_rng(20)
    n = N_SLOTS
    s = dict()
    # global grids up to 5000 x 4000 x 3000 cells (6e10 of them): a third of the slots beyond cell 2^32
    s["G"] = np.stack([rng.integers(1, 5001, n), rng.integers(1, 4001, n), rng.integers(1, 3001, n)], axis=1)
    s["G"][: n // 3] = (5000, 4000, 3000)
    s["g"] = np.stack([rng.integers(0, s["G"][:, a]) for a in range(3)], axis=1)
    s["g"][: n // 3, 2] = rng.integers(500, 3000, n // 3)
    s["dims"] = np.stack([rng.integers(1, 9, n), rng.integers(1, 7, n), rng.integers(1, 6, n)], axis=1)
    s["c"] = np.stack([rng.integers(0, s["dims"][:, a]) for a in range(3)], axis=1)
    s["j"] = np.where(rng.random(n) < 0.3, rng.integers(1 << 16, 1 << 31, n), rng.integers(0, 1 << 16, n))
    s["seed"], s["stream"] = rng.integers(0, 1 << 32, n), rng.integers(0, 4, n)
    s["flip"] = rng.integers(0, 2, n)
    scale = 10.0 ** rng.uniform(-3, 1, (n, 1))
    s["uth"] = (scale * rng.uniform(0, 1, (n, 3))).astype(np.float32)
    s["ud"] = (10.0 ** rng.uniform(-3, 1, (n, 1)) * rng.standard_normal((n, 3))).astype(np.float32)
    s["uth"][rng.random(n) < 0.15] = 0                                 # cold cells
    s["ud"][rng.random(n) < 0.15] = 0                                  # cells at rest
    s["uth"][rng.random((n, 3)) < 0.05] = 0                            # ... and single components
    s["ud"][rng.random((n, 3)) < 0.05] = 0
    d = np.empty((n, 7), np.float32)
    d[:, :3] = R.unit_open(rng.integers(0, 1 << 32, (n, 3)).astype(np.uint32))
    d[:, 3:6] = rng.standard_normal((n, 3)).astype(np.float32)
    d[:, 6] = R.unit_open(rng.integers(0, 1 << 32, n).astype(np.uint32))
    d[: n // 2, 6] *= np.float32(1e-4)                                 # (half of them small: cold and slow cells flip too)
    d[:4, :3] = [[R.unit_open(0)] * 3, [R.UNIT_OPEN_MAX] * 3, [0.5] * 3, [0.25, 0.75, 0.5]]
    # on the flip's threshold: w = (-1, -1, 1), D = (1, 1, 1): gw = gd = 2, -wD = 1, the quotient 1/4 exactly (and 3/4 for
    # w = (-1, -1, -1)); U on it does not flip (the rule's > is strict), the float below does, the float above does not
    k = 8
    for nz_, thr in ((1.0, 0.25), (-1.0, 0.75)):
        for U in (np.float32(thr), np.nextafter(np.float32(thr), np.float32(0)), np.nextafter(np.float32(thr), np.float32(1))):
            for flip in (1, 0):
                s["uth"][k], s["ud"][k], d[k, 3:6], d[k, 6], s["flip"][k] = 1, 1, (-1, -1, nz_), U, flip
                k += 1
    s["threshold"] = (8, k)
    s["draws"] = d
    return s


@pytest.fixture(scope="module")
def run(driver):
    s = slots()
    f32 = lambda a: np.asarray(a, np.float32).view(np.uint32)
    lines = []
    for k in range(N_SLOTS):
        words = list(s["g"][k]) + list(s["G"][k][:2]) + list(s["c"][k]) + list(s["dims"][k][:2]) + [s["j"][k], s["seed"][k], s["stream"][k], s["flip"][k]]
        words += list(f32(s["uth"][k])) + list(f32(s["ud"][k])) + list(f32(s["draws"][k]))
        lines.append(" ".join(str(int(w)) for w in words))
    out = subprocess.run([driver], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout
    rows = [ln.replace("|", " ").split() for ln in out.splitlines()]
    assert len(rows) == N_SLOTS and all(len(r) == 12 for r in rows)
    return s, np.array([[int(v) for v in r] for r in rows], dtype=object)


def test_header_is_plain_cpp_and_the_kernel_includes_it():
    src = open(os.path.join(ROOT, "old-vpic_amd", "csrc", "load_rule.h")).read()
    assert "#include <hip" not in src and '#include "hip' not in src and "__global__" not in src
    hip = open(os.path.join(ROOT, "old-vpic_amd", "csrc", "load.hip")).read()
    assert '#include "load_rule.h"' in hip and "load_momentum(" in hip and "load_words(" in hip and "load_numbers(" in hip
    assert "-ffp-contract=off" in open(os.path.join(ROOT, "old-vpic_amd", "csrc", "Makefile")).read()


def test_the_slots_cover_what_they_should():
    s = slots()
    cell = s["g"][:, 0] + s["G"][:, 0] * (s["g"][:, 1] + s["G"][:, 1] * s["g"][:, 2])
    assert (cell > 1 << 32).sum() > 500 and (s["j"] > 1 << 16).sum() > 500
    rest, cold = ~s["ud"].any(axis=1), ~s["uth"].any(axis=1)
    assert rest.sum() > 100 and cold.sum() > 100 and (rest & cold).sum() > 5
    assert 1000 < s["flip"].sum() < 3000
    flipped = R.momentum(s["uth"], s["ud"], s["draws"][:, 3:6], s["draws"][:, 6], s["flip"].astype(bool), parts=True)[1]
    assert flipped.sum() > 100
    a, b = s["threshold"]
    assert list(flipped[a:b]) == [False, False, True, False, False, False] * 2      # (U on, below, above) x (flip on, off)


def test_global_cell_and_voxel(run):
    s, got = run
    G, g, c, dims = (s[k].astype(object) for k in ("G", "g", "c", "dims"))
    assert list(got[:, 0]) == list(g[:, 0] + G[:, 0] * (g[:, 1] + G[:, 1] * g[:, 2]))
    assert list(got[:, 1]) == list((c[:, 0] + 1) + (dims[:, 0] + 2) * ((c[:, 1] + 1) + (dims[:, 1] + 2) * (c[:, 2] + 1)))


def test_generator_mode_positions_and_u(run):
    s, got = run
    cell = np.array([int(v) for v in got[:, 0]], np.uint64)
    d = R.numbers(R.words(cell, s["j"], s["seed"], s["stream"]))
    want = np.stack([R.offsets(d[:, 0]), R.offsets(d[:, 1]), R.offsets(d[:, 2]), d[:, 6]], axis=1).view(np.uint32)
    assert np.array_equal(got[:, 2:6].astype(np.uint32), want)
    assert np.all(np.abs(want.view(np.float32)[:, :3]) < 1)


def test_draws_mode_everything(run):
    s, got = run
    d = s["draws"]
    u = R.momentum(s["uth"], s["ud"], d[:, 3:6], d[:, 6], s["flip"].astype(bool))
    want = np.concatenate([np.stack([R.offsets(d[:, a]) for a in range(3)], axis=1), u], axis=1).view(np.uint32)
    assert np.array_equal(got[:, 6:12].astype(np.uint32), want)
