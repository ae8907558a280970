"""What the GPU tests of the species diagnostics (test_gpu_spectrum.py, test_gpu_distribution.py, test_gpu_select.py,
test_gpu_moments.py) share: the package, the child process of the states that need a fresh engine, and the five array
states a species is checked in.

Array states: "unsorted" as uploaded; "voxel" after sort_p in the reference's order; "tile" in the engine's tile order;
"tile_only" (VPIC_HIP_TILE_COARSE=1, read when the engine is created: run in a fresh child process, which checks that
the species really is sorted by tile only); "tile_tail_holes": tile order, then N_TAIL appended particles, then one
step of the resident exchange with absorbing x walls, which removes N_DOOMED particles placed for it and leaves their
slots dead (i = -1)."""
import importlib
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from test_spectrum_ref import voxel  # noqa: E402

N_TAIL, N_DOOMED = 5000, 300
STATES = ["unsorted", "voxel", "tile", "tile_only", "tile_tail_holes"]


def package():
    v = importlib.import_module("old-vpic_amd")
    assert v.lib().vpic_hip_device_count() > 0, "no HIP device"
    return v


def run_child(script, args, timeout):
    """`script` (a test module, which prints "child OK" at the end of its __main__) with args in a fresh process"""
    env = dict(os.environ)
    if args[0] == "tile_only":
        env["VPIC_HIP_TILE_COARSE"] = "1"
    r = subprocess.run([sys.executable, os.path.abspath(script)] + [str(a) for a in args], env=env, capture_output=True,
                       text=True, timeout=timeout)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "child OK" in r.stdout


def build_state(V, state, p, grid, tail, dt, doomed_dx, coarse=False):
    """(engine, species) with particles p in the array state asked for.  tail: the N_TAIL particles appended in
    "tile_tail_holes" (not looked at otherwise); dt: the step of that state's one push; doomed_dx: the offset of the
    N_DOOMED particles on their way through the absorbing +x wall (ux = 3).  coarse: the caller has set
    VPIC_HIP_TILE_COARSE=1, so every tile sort is by tile only whatever the state (test_gpu_sort.py)."""
    L = V.layout
    nx, ny, nz = grid
    n = len(p)
    holes = state == "tile_tail_holes"
    kw = dict(pbc=[L.ABSORB_PARTICLES, 0, 0, L.ABSORB_PARTICLES, 0, 0]) if holes else {}
    e = V.Engine(V.make_grid(nx, ny, nz, float(nx), float(ny), float(nz), np.float32(dt), **kw))
    e.set_vacuum()
    e.load_interpolator()                                   # zero fields: the push leaves the momenta alone
    sp = e.new_species(-1.0, n + N_TAIL + N_DOOMED + 4096, 8192)
    if holes:
        rng = np.random.default_rng(5)
        d = np.zeros(N_DOOMED, L.particle_t)
        d["i"] = voxel(nx, rng.integers(1, ny + 1, N_DOOMED), rng.integers(1, nz + 1, N_DOOMED), grid)
        d["dx"], d["ux"], d["q"] = doomed_dx, 3.0, -0.01
        d["tag"] = np.arange(N_DOOMED) + 10 ** 7
        p = np.concatenate([p, d])
    e.set_particles(sp, p)
    if state == "voxel":
        e.sort_p(sp)
        assert e.species_order(sp) == "voxel"
    if state in ("tile", "tile_only", "tile_tail_holes"):
        e.set_sort_order("engine")
        e.sort_p(sp)
        assert e.species_order(sp) == "tile"
        assert e.species_stats(sp)["by_tile_only"] == (1 if state == "tile_only" or coarse else 0)
    if holes:
        assert len(tail) == N_TAIL
        e.append_particles(sp, tail)
        e.clear_accumulators()
        e.exchange_begin()
        e.advance_p_async(sp)
        e.exchange_pack([0] * 6, [0] * 6, 8192)
        e.exchange_finish([])
        assert e.exchange_flags == 0
        assert e.species_stats(sp)["dead_slots"] == N_DOOMED
        assert e.np(sp) == n + N_TAIL
    return e, sp
