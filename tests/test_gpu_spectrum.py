"""vpic_hip_energy_spectrum / vpic_hip_energy_bands on the GPU against the float64 restatement of test_spectrum_ref.py:
EXACT equality of every count (integer counters: no tolerance to choose), in every order a species' array can be in.

The inputs (test_spectrum_ref.spec_inputs, seed 20261016, 400 000 particles on a 12 x 10 x 9 grid whose tiles are
partial on every axis) keep every linear and log coordinate further than 1e-9 (relative) from an integer, asserted
below and without a GPU in test_spectrum_ref.py, so no particle is left out of the comparison.

Array states: "unsorted" as uploaded; "voxel" after sort_p in the reference's order; "tile" in the engine's tile order;
"tile_only" (VPIC_HIP_TILE_COARSE=1, read when the engine is created: run in a fresh child process, which checks that
the species really is sorted by tile only); "tile_tail_holes": tile order, then 5 000 appended particles, then one
step of the resident exchange with absorbing x walls, which removes 300 particles placed for it and leaves their slots
dead (i = -1).  In that last state every other particle sits at its cell's centre and the step is shorter than half a
cell, so no live particle changes cell.

The window misses (energy_spectrum_stats): 0 in voxel and tile order -- with 370 particles per voxel, any 64
consecutive particles of the ordered array lie in two neighbouring sort keys, or in two keys either side of the ghost
voxels between two rows or planes, which the two slides per pass cover (spectrum.hip); at most the appended
particles in the last state."""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import species_states  # noqa: E402
from species_states import N_TAIL, STATES, package  # noqa: E402
from test_spectrum_ref import bands_ref, coordinates, deck_params, edge_distance, spec_inputs, spectrum_ref, voxel  # noqa: E402

pytestmark = pytest.mark.gpu
SEED, N, GRID = 20261016, 400000, (12, 10, 9)


def particles(L, u, i, first_tag=1):
    p = np.zeros(len(i), L.particle_t)
    p["i"] = i
    p["ux"], p["uy"], p["uz"] = u[:, 0], u[:, 1], u[:, 2]
    p["q"] = -0.01
    p["tag"] = np.arange(len(i)) + first_tag
    return p


def build_state(V, L, state, vth):
    """(engine, species) with the test's particles in the array state asked for (species_states.build_state)"""
    u, i = spec_inputs(SEED, N, vth)
    tail = None
    if state == "tile_tail_holes":
        ut, it = spec_inputs(SEED + 1, N_TAIL, vth)
        tail = particles(L, ut, it, first_tag=2 * 10 ** 7)
    return species_states.build_state(V, state, particles(L, u, i), GRID, tail, dt=0.4, doomed_dx=0.9)


def check_state(state, vth):
    V = package()
    L = V.layout
    nx, ny, nz = GRID
    nv = L.nv(nx, ny, nz)
    prm = deck_params(vth)
    e, sp = build_state(V, L, state, vth)
    lin, log = e.energy_spectrum(sp, **prm)
    counted, misses = e.energy_spectrum_stats()
    lin2, log2 = e.energy_spectrum(sp, **prm)
    assert lin.tobytes() == lin2.tobytes() and log.tobytes() == log2.tobytes()          # two calls: identical bytes
    assert (counted, misses) == e.energy_spectrum_stats()
    # each part alone: the same part
    lin_only, none = e.energy_spectrum(sp, n_lin=prm["n_lin"], d_lin=prm["d_lin"])
    assert none is None and np.array_equal(lin_only, lin)
    none, log_only = e.energy_spectrum(sp, n_log=prm["n_log"], log_lo=prm["log_lo"], d_log=prm["d_log"])
    assert none is None and np.array_equal(log_only, log)
    got = e.get_particles(sp)                                # (after the calls: a download drops the dead slots)
    e.close()
    u = np.stack([got["ux"], got["uy"], got["uz"]], axis=1)
    q, x = coordinates(u, prm)
    print(f"{state} vth {vth}: {len(got)} live, counted {counted}, misses {misses}; closest edge lin "
          f"{edge_distance(q).min():.3g} log {edge_distance(x).min():.3g}; truncated {int(((x > -1) & (x < 0)).sum())} "
          f"below {int((x <= -1).sum())} clamped {int((q >= prm['n_lin'] - 1).sum())}")
    assert edge_distance(q).min() > 1e-9 and edge_distance(x).min() > 1e-9              # nobody is left out
    if vth == 0.05:                                          # every branch is exercised
        assert ((x > -1) & (x < 0)).sum() > 0 and (x <= -1).sum() > 0 and (q >= prm["n_lin"] - 1).sum() > 0
    want_lin, want_log = spectrum_ref(u, got["i"], nv, prm)
    assert lin.dtype == np.uint32 and lin.shape == (prm["n_lin"], nv) and log.dtype == np.uint64 and log.shape == (prm["n_log"],)
    assert np.array_equal(lin, want_lin)
    assert np.array_equal(log, want_log)
    live = N + N_TAIL if state == "tile_tail_holes" else N
    assert len(got) == live and counted == live and int(lin.sum()) == live and int(log.sum()) == int(want_log.sum())
    interior = np.zeros((nz + 2, ny + 2, nx + 2), bool)
    interior[1:-1, 1:-1, 1:-1] = True
    assert not lin[:, ~interior.ravel()].any()                # ghost voxels stay zero
    if state in ("voxel", "tile", "tile_only"):
        assert misses == 0
    if state == "tile_tail_holes":
        assert misses <= N_TAIL
    return misses


def run_child(args, timeout):
    species_states.run_child(__file__, args, timeout)


@pytest.mark.parametrize("vth", [0.05, 0.3])
@pytest.mark.parametrize("state", STATES)
def test_counts_equal_the_restatement_exactly(state, vth):
    if state == "tile_only":
        run_child([state, vth], timeout=600)                 # the knob is read when the engine is created: a fresh process
    else:
        check_state(state, vth)


def test_bands_bit_for_bit_with_ghost_fill():
    """energy_bands on a grid with one cell along z (both z ghost layers copy the one interior plane), with one interior
    voxel left empty; against bands_ref of the restated counts, bit for bit."""
    V = package()
    L = V.layout
    grid = (7, 5, 1)
    nx, ny, nz = grid
    nv = L.nv(nx, ny, nz)
    vth = 0.05
    prm = deck_params(vth)
    u, i = spec_inputs(SEED, 30000, vth, grid)
    keep = i != voxel(3, 3, 1, grid)
    u, i = u[keep], i[keep]
    e = V.Engine(V.make_grid(nx, ny, nz, float(nx), float(ny), float(nz), np.float32(0.4)))
    sp = e.new_species(-1.0, len(i) + 64, 64)
    e.set_particles(sp, particles(L, u, i))
    want = bands_ref(spectrum_ref(u, i, nv, prm)[0], grid)
    for order in ("unsorted", "sorted"):
        if order == "sorted":
            e.sort_p(sp)
        got = e.energy_bands(sp, prm["n_lin"], prm["d_lin"])
        assert got.dtype == np.float32 and got.shape == want.shape
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), order
    assert not got[:, voxel(3, 3, 1, grid)].any() and got[:, voxel(0, 0, 0, grid)].any()
    assert e.energy_spectrum_stats()[0] == len(i)
    e.close()


def test_the_pass_touches_no_particle_state():
    """advance_p, energy_spectrum, advance_p against advance_p, advance_p: the same particles bit for bit."""
    from conftest import bits_equal
    V = package()
    L = V.layout
    nx, ny, nz = GRID
    u, i = spec_inputs(SEED, 100000, 0.3)
    p = particles(L, u, i)
    rng = np.random.default_rng(2)
    for c in ("dx", "dy", "dz"):
        p[c] = rng.uniform(-1, 1, len(p)).astype(np.float32)
    fi = np.zeros(L.nv(nx, ny, nz), L.interpolator_t)
    for c in ("ex", "ey", "ez", "cbx", "cby", "cbz", "dexdy", "dcbxdx"):
        fi[c] = rng.uniform(-0.05, 0.05, len(fi)).astype(np.float32)
    prm = deck_params(0.3)
    out = []
    for with_spectrum in (False, True):
        e = V.Engine(V.make_grid(nx, ny, nz, float(nx), float(ny), float(nz), np.float32(0.4)))
        e.set_sort_order("engine")
        e.set_interpolator(fi)
        sp = e.new_species(-1.0, 2 * len(p), len(p))
        e.set_particles(sp, p)
        e.sort_p(sp)
        e.clear_accumulators()
        assert e.advance_p(sp) == 0
        if with_spectrum:
            e.energy_spectrum(sp, **prm)
            e.energy_bands(sp, prm["n_lin"], prm["d_lin"])
        assert e.advance_p(sp) == 0
        got = e.get_particles(sp)
        out.append(got[np.argsort(got["tag"], kind="stable")])
        e.close()
    assert bits_equal(out[0], out[1])


def test_argument_errors():
    V = package()
    eng = importlib.import_module("old-vpic_amd.engine")
    l = V.lib()
    e = V.Engine(V.make_grid(4, 4, 4, 4.0, 4.0, 4.0, np.float32(0.4)))
    sp = e.new_species(-1.0, 64, 8)
    nv = e.nv
    lin = np.zeros((6, nv), np.uint32)
    log = np.zeros(8192, np.uint64)
    bands = np.zeros((6, nv), np.float32)
    ok = eng.SpectrumParams(6, 800, 0.5, -4.0, 0.01)
    lp, gp, bp = (a.ctypes.data_as(C.c_void_p) for a in (lin, log, bands))

    def fails(rc, word):
        assert rc != 0
        msg = l.vpic_hip_last_error().decode()
        assert word in msg, msg

    assert l.vpic_hip_energy_spectrum(e._h, sp, C.byref(ok), lp, gp) == 0
    fails(l.vpic_hip_energy_spectrum(e._h, sp + 1, C.byref(ok), lp, gp), "species")
    fails(l.vpic_hip_energy_spectrum(e._h, -1, C.byref(ok), lp, gp), "species")
    fails(l.vpic_hip_energy_spectrum(e._h, sp, None, lp, gp), "parameters")
    fails(l.vpic_hip_energy_spectrum(e._h, sp, C.byref(eng.SpectrumParams(-1, 800, 0.5, -4.0, 0.01)), lp, gp), "negative")
    fails(l.vpic_hip_energy_spectrum(e._h, sp, C.byref(eng.SpectrumParams(6, -800, 0.5, -4.0, 0.01)), lp, gp), "negative")
    fails(l.vpic_hip_energy_spectrum(e._h, sp, C.byref(eng.SpectrumParams(6, 4097, 0.5, -4.0, 0.01)), lp, gp), "cap")
    assert l.vpic_hip_energy_spectrum(e._h, sp, C.byref(eng.SpectrumParams(6, 4096, 0.5, -4.0, 0.01)), lp, gp) == 0
    fails(l.vpic_hip_energy_bands(e._h, sp + 1, C.byref(ok), bp), "species")
    fails(l.vpic_hip_energy_bands(e._h, sp, None, bp), "parameters")
    fails(l.vpic_hip_energy_bands(e._h, sp, C.byref(eng.SpectrumParams(-6, 0, 0.5, 0.0, 0.0)), bp), "negative")
    fails(l.vpic_hip_energy_bands(e._h, sp, C.byref(ok), None), "bands")
    fails(l.vpic_hip_energy_spectrum_stats(e._h, None), "output")
    with pytest.raises(V.VpicHipError):
        e.energy_spectrum(sp, n_log=5000, d_log=0.01)
    # an empty species: all zero
    lin0, log0 = e.energy_spectrum(sp, 6, 0.5, 800, -4.0, 0.01)
    assert not lin0.any() and not log0.any() and e.energy_spectrum_stats() == (0, 0)
    e.close()


def check_fullsize():
    """2^28 particles in ONE species (128^3 cells x 128 per cell), a cold beam, so that nearly all of them fall into
    a few log bins: the fullest exceeds 2^24, where a float counter (the reference's edist[k]++) stops increasing.
    Log spectrum only; against the restatement over get_particles_range in chunks."""
    V = package()
    n_cells, ppc = 128, 128
    e = V.Engine(V.make_grid(n_cells, n_cells, n_cells, float(n_cells), float(n_cells), float(n_cells), np.float32(0.5)))
    n = n_cells ** 3 * ppc
    assert n >= 2 ** 28
    sp = e.new_species(-1.0, n, 4096)
    e.load_maxwellian(sp, ppc, 7, -1e-3, (0.2, 0.0, 0.0), 0.001)
    prm = dict(deck_params(0.05), n_lin=0)
    none, log = e.energy_spectrum(sp, n_log=prm["n_log"], log_lo=prm["log_lo"], d_log=prm["d_log"])
    assert none is None and e.energy_spectrum_stats() == (n, 0)
    want = np.zeros(prm["n_log"], np.uint64)
    chunk = 1 << 24
    closest = 1.0
    for first in range(0, n, chunk):
        p = e.get_particles_range(sp, first, min(chunk, n - first))
        u = np.stack([p["ux"], p["uy"], p["uz"]], axis=1)
        closest = min(closest, edge_distance(coordinates(u, prm)[1]).min())
        want += spectrum_ref(u, p["i"], 1, dict(prm))[1]
    e.close()
    print(f"fullsize: {n} particles, fullest bin {int(log.max())} (2^24 = {1 << 24}), closest log edge {closest:.3g}")
    assert int(log.max()) > 2 ** 24
    assert int(want.sum()) == n
    assert np.array_equal(log, want)


def test_fullsize_log_spectrum_counts_beyond_two_to_the_24():
    run_child(["fullsize"], timeout=1500)                    # its own, generous limit


if __name__ == "__main__":
    if sys.argv[1] == "fullsize":
        check_fullsize()
    else:
        check_state(sys.argv[1], float(sys.argv[2]))
    print("child OK")
