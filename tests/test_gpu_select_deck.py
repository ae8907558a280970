"""vpic_simulation::select_particles on the C++ deck host: tests/decks/select_probe.cxx (written for this test, deck API
only) gives every particle a tag of its own, runs four steps, and at the last one asks the host for two selections of
its species with particles, fields and indices -- the particles inside a box given in physical units and above an
energy, and every 16th tag -- then finds the same particles with its own loop over sp->p, interpolates the fields at
them from interpolator[p->i] in float, and writes both.  The two files must be identical, byte for byte, and the helper
must have answered BEFORE any particle came to the host: the host's count of particle-mirror downloads is unchanged by
the helper and non-zero after the deck's loop.

(The box's cells measure 2 x 1 x 0.5 from (-8, 0, 0), so the helper's conversion to cells and the loop's to physical
units are both exact; the deck is compiled without fused multiply-add, as the library is, so the six floats per
particle are rounded the same way on both sides.)"""
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_helper_equals_the_deck_s_own_loop_without_a_download(tmp_path):
    host = os.path.join(ROOT, "old-vpic_amd", "host")
    deck = os.path.join(ROOT, "tests", "decks", "select_probe.cxx")
    subprocess.check_call(["make", "-s", "-C", host, "deck", "DECK=" + deck, "OUT=" + str(tmp_path / "select_probe")])
    r = subprocess.run([str(tmp_path / "select_probe.hip.exe"), "-tpp=1"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    m = re.search(r"select_probe: np (\d+), kept (\d+) and (\d+), mirror downloads before the helper (\d+), after the helper (\d+), "
                  r"after the loop (\d+)", r.stdout)
    assert m, r.stdout[-4000:]
    n_p, kept_box, kept_tags, before, after_helper, after_loop = (int(v) for v in m.groups())
    print(m.group(0))
    assert n_p == 16 * 8 * 8 * 48
    assert after_helper == before == 0
    assert after_loop > after_helper
    helper = (tmp_path / "select_helper.bin").read_bytes()
    loop = (tmp_path / "select_loop.bin").read_bytes()
    # the probe is worth something: both selections select, the tags are every 16th, the fields are not all zero
    at = 0
    for kept in (kept_box, kept_tags):
        assert 0 < kept < n_p
        assert int(np.frombuffer(loop, np.int64, 1, at)[0]) == kept
        fields = np.frombuffer(loop, np.float32, 6 * kept, at + 8 + 48 * kept).reshape(kept, 6)
        index = np.frombuffer(loop, np.int64, kept, at + 8 + 72 * kept)
        assert np.all(np.diff(index) > 0) and index[0] >= 0 and index[-1] < n_p
        assert np.count_nonzero(fields) > fields.size // 2
        at += 8 + 80 * kept
    assert at == len(loop)
    assert kept_tags == n_p // 16 and 0.02 * n_p < kept_box < 0.3 * n_p
    assert len(helper) == len(loop)
    assert helper == loop
