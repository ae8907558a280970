"""The coordinates in the frame of the local magnetic field on the C++ deck host: tests/decks/fieldcoord_probe.cxx
(written for this test, deck API only) sets a magnetic and an electric field that vary in space with set_region_field,
runs four steps, and at the last one asks the host for a u_par-u_perp histogram of the particles inside a box given in
physical units (vpic_simulation::distribution) and for the particles with 0.9 <= pitch < 1, with the fields at them and
their indices (select_particles) -- then computes both with its own loop over sp->p and interpolator[p->i], the fields
in float as advance_p forms them and the rest in double as include/vpic_hip.h writes it down, and writes both.  The two
files must be identical, byte for byte, and the helpers must have answered BEFORE any particle came to the host: the
count of particle-mirror downloads is unchanged by them and non-zero after the deck's loop.

The deck's own loop must round every operation once, as the library does: old-vpic_amd/host/Makefile compiles a deck
with -ffp-contract=off (its `deck` rule), so `a + b*c` in the loop is a multiplication and an addition, never a fused
multiply-add; this test reads that flag in the rule before it trusts the comparison.  (The box's cells measure
2 x 1 x 0.5 from (-8, 0, 0), so the conversions between physical units and cells are exact on both sides.)"""
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_helpers_equal_the_deck_s_own_loop_without_a_download(tmp_path):
    host = os.path.join(ROOT, "old-vpic_amd", "host")
    deck = os.path.join(ROOT, "tests", "decks", "fieldcoord_probe.cxx")
    rule = re.search(r"^deck:\n\t(.*)$", open(os.path.join(host, "Makefile")).read(), re.M)
    assert rule and "-ffp-contract=off" in rule.group(1)           # the deck's loop is compiled unfused
    subprocess.check_call(["make", "-s", "-C", host, "deck", "DECK=" + deck, "OUT=" + str(tmp_path / "fieldcoord_probe")])
    r = subprocess.run([str(tmp_path / "fieldcoord_probe.hip.exe"), "-tpp=1"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    m = re.search(r"fieldcoord_probe: np (\d+), kept (\d+), mirror downloads before the helpers (\d+), after the helpers (\d+), "
                  r"after the loop (\d+)", r.stdout)
    assert m, r.stdout[-4000:]
    n_p, kept, before, after_helpers, after_loop = (int(v) for v in m.groups())
    print(m.group(0))
    assert n_p == 16 * 8 * 8 * 48
    assert after_helpers == before == 0
    assert after_loop > after_helpers
    helper = (tmp_path / "fieldcoord_helper.bin").read_bytes()
    loop = (tmp_path / "fieldcoord_loop.bin").read_bytes()
    # the probe is worth something: the histogram is populated and leaves particles out, the selection selects, the
    # fields vary from particle to particle
    bins = 64 * 48
    counts = np.frombuffer(loop, np.uint64, bins)
    print(f"histogram: {int(counts.sum())} counted, {np.count_nonzero(counts)} of {bins} bins non-empty")
    assert 0.1 * n_p < int(counts.sum()) < 0.3 * n_p and np.count_nonzero(counts) > bins // 2
    assert int(np.frombuffer(loop, np.int64, 1, 8 * bins)[0]) == kept and 0.01 * n_p < kept < 0.2 * n_p
    at = 8 * bins + 8
    fields = np.frombuffer(loop, np.float32, 6 * kept, at + 48 * kept).reshape(kept, 6)
    index = np.frombuffer(loop, np.int64, kept, at + 72 * kept)
    assert at + 80 * kept == len(loop)
    assert np.all(np.diff(index) > 0) and index[0] >= 0 and index[-1] < n_p
    assert np.all(fields != 0) and all(len(np.unique(fields[:, k])) > kept // 2 for k in range(6))
    assert len(helper) == len(loop)
    assert helper == loop
