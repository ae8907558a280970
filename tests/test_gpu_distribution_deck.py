"""vpic_simulation::distribution on the C++ deck host: tests/decks/distribution_probe.cxx (written for this test, deck
API only) asks the host for three histograms of its species in physical units at the last step -- one that fits in
LDS, one through the sliding window, one over momentum and log10 of energy inside a box and above an energy -- then
computes them with its own loop over sp->p in double, and writes both.  The two files must be identical, and the
helper must have answered BEFORE any particle came to the host: the host's count of particle-mirror downloads is
unchanged by the helper and non-zero after the deck's loop.

(The box's cells measure 2 x 1 x 0.5 from (-8, 0, 0), so the helper's conversion to cells and the loop's to physical
units are both exact.  The deck's log10 is the host's and the helper's the device's: with 98 304 particles against 50
log bins and one rounding of difference at the most, a particle on the wrong side would need a bin coordinate within
about 1e-14 of an integer.)"""
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_helper_equals_the_deck_s_own_loop_without_a_download(tmp_path):
    host = os.path.join(ROOT, "old-vpic_amd", "host")
    deck = os.path.join(ROOT, "tests", "decks", "distribution_probe.cxx")
    subprocess.check_call(["make", "-s", "-C", host, "deck", "DECK=" + deck, "OUT=" + str(tmp_path / "distribution_probe")])
    r = subprocess.run([str(tmp_path / "distribution_probe.hip.exe"), "-tpp=1"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    m = re.search(r"distribution_probe: np (\d+), mirror downloads before the helper (\d+), after the helper (\d+), after the loop (\d+)", r.stdout)
    assert m, r.stdout[-4000:]
    n_p, before, after_helper, after_loop = (int(v) for v in m.groups())
    print(m.group(0))
    assert n_p == 16 * 8 * 8 * 48
    assert after_helper == before == 0
    assert after_loop > after_helper
    helper = (tmp_path / "distribution_helper.bin").read_bytes()
    loop = (tmp_path / "distribution_loop.bin").read_bytes()
    shapes = [(64, 64), (320, 32), (50, 40)]
    assert len(helper) == len(loop) == 8 * sum(a * b for a, b in shapes)
    # the probe is worth something: the box holds every particle in x, all x bins are populated evenly, the selection selects
    counts = np.frombuffer(loop, np.uint64)
    first = 0
    parts = []
    for a, b in shapes:
        parts.append(counts[first:first + a * b].reshape(a, b))
        first += a * b
    for k in (0, 1):
        per_x = parts[k].sum(axis=0)
        assert 0.9 * n_p < per_x.sum() <= n_p and per_x.min() > 0.5 * per_x.mean()
        assert np.count_nonzero(parts[k]) > parts[k].size // 4
    assert 0.02 * n_p < parts[2].sum() < 0.3 * n_p and np.count_nonzero(parts[2]) > parts[2].size // 8
    print("counted:", [int(p.sum()) for p in parts], "non-empty bins:", [int(np.count_nonzero(p)) for p in parts])
    assert helper == loop
