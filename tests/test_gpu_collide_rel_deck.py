"""vpic_simulation::collide with collide_params_t::relativistic = 1 on the C++ deck host: tests/decks/collide_rel_probe.cxx
(written for this test, deck API only) holds electrons and ions of mass 100 at vth = 0.6 c, the electrons anisotropic
(u_th,z = 2 u_th,x), and collides the electrons among themselves and with the ions in begin_particle_collisions, every step
for four steps, with the relativistic pair.  The species have q/m = 0: only the collisions change a momentum.  Held: no
particle mirror comes to the host across the collisions; sum m u per component and sum m gamma of both species together
stay within the bounds of tests/test_gpu_collide_rel.py::test_conservation, once per call (equal weights; K = 4
WORST_P_REL and 4 WORST_E_REL of tests/test_collide_rel_ref.py's docstring, summed over the particles of each call); and
the electrons' anisotropy <uz^2> / <ux^2>, loaded at 4, has fallen towards 1."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from test_collide_rel_ref import WORST_E_REL, WORST_P_REL  # noqa: E402
from test_gpu_collide_deck import anisotropy, particles  # noqa: E402

STEPS, N, M_I = 4, 8 * 8 * 8 * 48, 100.0
ULP = 2.0 ** -24


def momenta(p):
    return np.stack([p["ux"], p["uy"], p["uz"]], 1).astype(np.float64)


def m_gamma_minus_one(u, m):
    uu = (u * u).sum(1)
    return m * uu / (np.sqrt(1.0 + uu) + 1.0)


def test_a_deck_collides_relativistically_on_the_device(tmp_path):
    host = os.path.join(ROOT, "old-vpic_amd", "host")
    deck = os.path.join(ROOT, "tests", "decks", "collide_rel_probe.cxx")
    subprocess.check_call(["make", "-s", "-C", host, "deck", "DECK=" + deck, "OUT=" + str(tmp_path / "collide_rel_probe")])
    r = subprocess.run([str(tmp_path / "collide_rel_probe.hip.exe"), "-tpp=1"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    calls = re.findall(r"collide_rel_probe: collisions of step (\d+), mirror downloads before (\d+), after (\d+)", r.stdout)
    print("\n".join(l for l in r.stdout.splitlines() if l.startswith("collide_rel_probe")))
    assert [int(s) for s, _, _ in calls] == list(range(STEPS))
    assert all(before == after for _, before, after in calls)       # no mirror came to the host for the collisions ...
    assert len({before for _, before, _ in calls}) == 1              # ... nor between them
    e0, i0 = particles(tmp_path / "electron.0.0", N), particles(tmp_path / "ion.0.0", N)
    e1, i1 = particles(tmp_path / ("electron.%d.0" % STEPS), N), particles(tmp_path / ("ion.%d.0" % STEPS), N)
    for a, b in ((e0, e1), (i0, i1)):
        assert np.array_equal(a["tag"], b["tag"]) and np.array_equal(a["q"], b["q"])
    ue0, ui0, ue1, ui1 = momenta(e0), momenta(i0), momenta(e1), momenta(i1)
    # two calls per step: the electrons in the first, electrons and ions in the second; the per-particle sums taken where
    # they are larger, before or after (the species exchange a little energy)
    sum_p = lambda u, m: m * np.sqrt((u * u).sum(1)).sum()           # noqa: E731
    sum_e = lambda u, m: m_gamma_minus_one(u, m).sum()               # noqa: E731
    bound_p = STEPS * 4 * WORST_P_REL * ULP * (2 * max(sum_p(ue0, 1.0), sum_p(ue1, 1.0)) + max(sum_p(ui0, M_I), sum_p(ui1, M_I)))
    bound_e = STEPS * 4 * WORST_E_REL * ULP * (2 * max(sum_e(ue0, 1.0), sum_e(ue1, 1.0)) + max(sum_e(ui0, M_I), sum_e(ui1, M_I)))
    dp = (ue1.sum(0) + M_I * ui1.sum(0)) - (ue0.sum(0) + M_I * ui0.sum(0))
    de = (sum_e(ue1, 1.0) + sum_e(ui1, M_I)) - (sum_e(ue0, 1.0) + sum_e(ui0, M_I))
    print("d(sum m u)", dp, "bound", bound_p, "; d(sum m gamma)", de, "bound", bound_e, "of", sum_e(ue0, 1.0) + sum_e(ui0, M_I))
    assert np.abs(dp).max() <= bound_p and abs(de) <= bound_e
    changed = (e1["ux"].view(np.uint32) != e0["ux"].view(np.uint32)).mean()
    rms = np.sqrt(((ue1 - ue0) ** 2).sum(1).mean())
    print("electrons changed", changed, "rms change of u", rms, "anisotropy", anisotropy(e0), "->", anisotropy(e1))
    assert changed > 0.99 and rms > 1e-2                             # far above rounding (vth = 0.6)
    assert not np.array_equal(i0["ux"], i1["ux"])
    assert abs(sum_e(ue0, 1.0) / N - 0.8) < 0.4                      # (relativistic electrons: gamma - 1 of order one)
    a0, a1 = anisotropy(e0), anisotropy(e1)
    assert 3.5 < a0 < 4.5 and abs(a1 - 1) < abs(a0 - 1) and a1 < 0.9 * a0
