"""The drop-in twins on a grid whose faces carry a custom particle boundary handler's code (<= -3).

The deck host writes particle dumps through the center_p twin (dump.cxx:313-320), also in a deck that has absorb_tally or
link_boundary walls.  center_p and energy_p never look at a face's particle code, so they serve such a grid and give, bit for
bit, what they give on the same grid with VPIC_ABSORB_PARTICLES in the code's place.  boundary_p is the one twin that would
have to CALL the handler: it still refuses such a grid, with the drop-in's ERROR convention (message, exit(1))."""
import ctypes as C
import importlib
import os
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

DIMS = (6, 5, 4)


def world(code):
    """(library, grid with `code` on both x faces, interpolator, particles)"""
    import det_exact as D
    drop = importlib.import_module("old-vpic_amd.dropin")
    L = importlib.import_module("old-vpic_amd.layout")
    nx, ny, nz = DIMS
    g = drop.reference_grid(nx, ny, nz, float(nx), float(ny), float(nz), np.float32(D.DT), pbc=[code, 0, 0, code, 0, 0])
    _, _, og = D.grids(DIMS, [L.ABSORB_PARTICLES, 0, 0, L.ABSORB_PARTICLES, 0, 0])
    fi = D.interpolator(og)
    p = D.particles(61, 3000, DIMS, 0.5)
    return drop.ref(), g, fi, p


def test_center_p_and_energy_p_do_not_look_at_the_code():
    L = importlib.import_module("old-vpic_amd.layout")
    out = {}
    for code in (L.ABSORB_PARTICLES, -3, -7):
        l, g, fi, p = world(code)
        en = l.vpic_hip_ref_energy_p(p.ctypes.data, len(p), -1.0, fi.ctypes.data, C.byref(g))
        l.vpic_hip_ref_center_p(p.ctypes.data, len(p), -1.0, fi.ctypes.data, C.byref(g))
        out[code] = (en, p.copy())
    en0, p0 = out[L.ABSORB_PARTICLES]
    assert en0 > 0 and not np.array_equal(p0["ux"], world(-3)[3]["ux"])              # center_p did something
    for code in (-3, -7):
        en, p = out[code]
        assert en == en0, (code, en, en0)
        assert p.tobytes() == p0.tobytes(), code


def test_boundary_p_still_refuses_the_code():
    child = ("import sys, ctypes as C, numpy as np\n"
             "sys.path[:0] = [%r, %r]\n"
             "import test_gpu_dropin_handler_codes as T, importlib\n"
             "L = importlib.import_module('old-vpic_amd.layout')\n"
             "l, g, fi, p = T.world(-3)\n"
             "f = np.zeros(L.nv(*T.DIMS), L.field_t)\n"
             "l.vpic_hip_ref_boundary_p(None, f.ctypes.data, None, C.byref(g), None)\n"
             "print('boundary_p returned')\n") % (ROOT, HERE)
    r = subprocess.run([sys.executable, "-c", child], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "boundary_p returned" not in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    assert "custom particle boundary handlers are not supported" in r.stderr, r.stderr[-2000:]
