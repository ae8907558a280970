"""vpic_simulation::hydro_dump( name, params, &sel ) on the C++ deck host: tests/decks/hydro_select_probe.cxx (written for
this test, deck API only) runs four steps and at the last one writes the hydro dump of a box-plus-energy selection of its
species -- the box in PHYSICAL units -- then field_dump and dump_particles.  The expectation is rebuilt from the two plain
dumps with the oracle: load_interpolator of the dumped fields (the interpolator the host has loaded when user_diagnostics
runs), the keep mask in physical units, accumulate_hydro_p of the kept particles, synchronize_hydro, and dumpfmt.gather for
the payload's layout; the payload is held to it within ACC_TOL = 2e-6 of each moment's largest entry.  The selected dump
must not have brought the particles to the host: the count of particle-mirror downloads is the same before and after it.

dump_particles writes the particles time-centred, as the reference does, so the test takes them back half a step with the
oracle's uncenter_p before it looks at their energies and sums their moments: the momenta the device holds, to a rounding
(one or two parts in 10^7, inside ACC_TOL).  The energy edge (0.06) lies between the cold and the hot population, where
particles are sparse; the test prints how near the nearest one is.  (The box's cells measure 2 x 1 x 0.5 from (-8, 0, 0):
the conversion between physical units and cells is exact on both sides.)"""
import importlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACC_TOL = 2e-6
NX, NY, NZ, PPC = 16, 8, 8, 48
X0, CELL = (-8.0, 0.0, 0.0), (2.0, 1.0, 0.5)
BOX_X, BOX_Z, KE_LO = (-2.0, 10.0), (1.0, 3.0), 0.06


def test_selected_hydro_dump_equals_the_oracle_on_the_plain_dumps(tmp_path):
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from oracle import dumpfmt as D, pyorc
    L = importlib.import_module("old-vpic_amd.layout")
    importlib.import_module("old-vpic_amd").lib()
    host = os.path.join(ROOT, "old-vpic_amd", "host")
    deck = os.path.join(ROOT, "tests", "decks", "hydro_select_probe.cxx")
    subprocess.check_call(["make", "-s", "-C", host, "deck", "DECK=" + deck, "OUT=" + str(tmp_path / "hydro_select_probe")])
    r = subprocess.run([str(tmp_path / "hydro_select_probe.hip.exe"), "-tpp=1"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    m = re.search(r"hydro_select_probe: np (\d+), mirror downloads before the selected dump (\d+), after it (\d+), after dump_particles (\d+)", r.stdout)
    assert m, r.stdout[-4000:]
    n_p, before, after, after_particles = (int(v) for v in m.groups())
    print(m.group(0))
    assert n_p == NX * NY * NZ * PPC
    assert after == before == 0 and after_particles > after

    nv = (NX + 2) * (NY + 2) * (NZ + 2)
    H = D.HEADER_V0 + 8 + 12
    raw = np.fromfile(tmp_path / "T.4" / "hsel.4.0", np.uint8)
    head = raw[:H].tobytes()                                                  # WRITE_HEADER_V0: nx, ny, nz at byte 35, dt at 47
    dt = float(np.frombuffer(head, np.float32, 1, 47)[0])
    assert tuple(np.frombuffer(head, np.int32, 3, 35)) == (NX, NY, NZ) and tuple(np.frombuffer(head, np.int32, 3, H - 12)) == (NX + 2, NY + 2, NZ + 2)
    got = raw[H:].view(np.float32).reshape(14, NZ + 2, NY + 2, NX + 2)
    fraw = np.fromfile(tmp_path / "T.4" / "fields.4.0", np.uint8)
    assert len(fraw) == H + nv * L.field_t.itemsize
    f = fraw[H:].view(L.field_t).copy()
    p = np.fromfile(tmp_path / "particles.4.0", L.particle_t, offset=D.HEADER_V0 + 8 + 4)
    assert len(p) == n_p

    g = pyorc.make_grid(NX, NY, NZ, NX * CELL[0], NY * CELL[1], NZ * CELL[2], np.float32(dt))
    fi = np.zeros(nv, L.interpolator_t)
    pyorc.load_interpolator(fi, f, g)
    pyorc.uncenter_p(p, len(p), -1.0, fi, g)                                  # the stored momenta, to a rounding
    i = p["i"].astype(np.int64)
    cx, cz = i % (NX + 2), i // ((NX + 2) * (NY + 2))
    x = X0[0] + CELL[0] * ((cx - 1) + (p["dx"].astype(np.float64) + 1.0) * 0.5)
    z = X0[2] + CELL[2] * ((cz - 1) + (p["dz"].astype(np.float64) + 1.0) * 0.5)
    ux, uy, uz = (p[c].astype(np.float64) for c in ("ux", "uy", "uz"))
    ke = np.sqrt(((1.0 + ux * ux) + uy * uy) + uz * uz) - 1.0
    keep = (x >= BOX_X[0]) & (x < BOX_X[1]) & (z >= BOX_Z[0]) & (z < BOX_Z[1]) & (ke >= KE_LO)
    print(f"kept {int(keep.sum())} of {n_p}; the nearest kinetic energy is {float(np.abs(ke / KE_LO - 1.0).min()):.2e} (relative) from the edge")
    assert 0.02 * n_p < keep.sum() < 0.1 * n_p

    def moments_of(rows):
        h = np.zeros(nv, L.hydro_t)
        pyorc.accumulate_hydro_p(h, np.ascontiguousarray(rows), len(rows), -1.0, fi, g)
        pyorc.synchronize_hydro_local(h, g)
        return D.gather(h, NX, NY, NZ, D.BAND, range(14), (1, 1, 1)).view(np.float32)

    want, whole = moments_of(p[keep]), moments_of(p)
    assert got.shape == want.shape
    for k, c in enumerate(L.hydro_t.names[:14]):
        err, top = float(np.abs(got[k].astype(np.float64) - want[k]).max()), float(np.abs(want[k]).max())
        far = float(np.abs(got[k].astype(np.float64) - whole[k]).max())
        print(f"{c}: max error {err:.3e}, largest entry {top:.3e}, ratio {err / top:.2e}; from the whole species' moments {far / top:.2e}")
        assert top > 0 and err <= ACC_TOL * top, c
        assert far > 0.1 * top, c                                            # the dump holds the selection, not the species
