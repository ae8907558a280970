"""vpic_simulation::energy_spectrum on the C++ deck host: tests/decks/spectrum_probe.cxx (written for this test, deck
API only) asks the host for the spectra of its species at the last step, then computes them with its own loop over
sp->p, and writes both.  The two files must be identical (every count is far below 2^24 here), and the helper must have
answered BEFORE any particle came to the host: the host's count of particle-mirror downloads is unchanged by the
helper and non-zero after the deck's loop."""
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_helper_equals_the_deck_s_own_loop_without_a_download(tmp_path):
    host = os.path.join(ROOT, "old-vpic_amd", "host")
    deck = os.path.join(ROOT, "tests", "decks", "spectrum_probe.cxx")
    subprocess.check_call(["make", "-s", "-C", host, "deck", "DECK=" + deck, "OUT=" + str(tmp_path / "spectrum_probe")])
    r = subprocess.run([str(tmp_path / "spectrum_probe.hip.exe"), "-tpp=1"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    m = re.search(r"spectrum_probe: np (\d+), mirror downloads before the helper (\d+), after the helper (\d+), after the loop (\d+)", r.stdout)
    assert m, r.stdout[-4000:]
    n_p, before, after_helper, after_loop = (int(v) for v in m.groups())
    print(m.group(0))
    assert n_p == 16 * 8 * 8 * 48
    assert after_helper == before == 0
    assert after_loop > after_helper
    helper = (tmp_path / "spectrum_helper.bin").read_bytes()
    loop = (tmp_path / "spectrum_loop.bin").read_bytes()
    nex, nbin, nv = 6, 800, 18 * 10 * 10
    assert len(helper) == len(loop) == 4 * (nex * nv + nbin)
    bands = np.frombuffer(loop, np.float32, nex * nv).reshape(nex, nv)
    spectrum = np.frombuffer(loop, np.float32, nbin, offset=4 * nex * nv)
    # the probe is worth something: every band is populated, the log spectrum holds (nearly) all particles in many bins
    assert (bands.max(axis=1) > 0).all() and abs(float(bands.sum(axis=0).min()) - 1.0) < 1e-6
    assert 0.98 * n_p <= spectrum.sum() <= n_p and (spectrum > 0).sum() > 100 and spectrum.max() < 2 ** 24
    assert helper == loop
