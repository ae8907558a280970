"""vpic_hip_species_distribution on the GPU against the float64 restatement of test_distribution_ref.py: EXACT equality
of every count and of the statistics (integer counters: no tolerance to choose), in every order a species' array can
be in, for the descriptors of test_distribution_ref.descriptors -- (a) 1-D ux in LDS, (b) x-ux through the sliding
window, (c) ux-uz under a z range and a KE threshold, (d) 1-D LOG10_KE with 800 bins, (e) ux-uy through global adds,
(f) the window with the position axis second and bins off the cells, (g) y-LOG10_KE under three ranges.

The inputs (test_distribution_ref.dist_inputs, seed 20261017: 560 000 particles on a 96 x 8 x 6 grid, at least 64 in
every voxel, offsets over all of (-1, 1)) keep every LOG10_KE coordinate further than 1e-9 (relative) from a bin edge
and from a range end -- asserted without a GPU in test_distribution_ref.py, and here again on the particles that
came back in the one state whose particles are not the inputs -- so no particle is left out of the comparison.

Array states, as in test_gpu_spectrum.py: "unsorted" as uploaded; "voxel"; "tile"; "tile_only" (VPIC_HIP_TILE_COARSE=1,
read when the engine is created: a fresh child process); "tile_tail_holes": tile order, then 5 000 appended particles,
then one step of the resident exchange with absorbing x walls, which removes 300 particles placed for it and leaves
their slots dead (i = -1).  In that last state the offsets span (-0.95, 0.95) and the step (dt = 0.02) moves nobody by
more than 0.04, so no live particle changes cell and the order of the sorted part is intact.

Misses (distribution_stats()[3]): 0 for every descriptor held in LDS, in every state; 0 for the window descriptors in
voxel and tile order, by tile only included, which is the rule include/vpic_hip.h states; at most the appended
particles in the last state; every counted particle for (e)."""
import ctypes as C
import functools
import importlib
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import species_states  # noqa: E402
from species_states import N_TAIL, STATES, package  # noqa: E402
from test_distribution_ref import GRID, N, SEED, VTH, descriptors, dist_inputs, distribution_ref, log_margin  # noqa: E402
from test_spectrum_ref import voxel  # noqa: E402

pytestmark = pytest.mark.gpu
IN_LDS, WINDOW, GLOBAL = "acdg", "bf", "e"


@functools.lru_cache(maxsize=None)
def reference_of_the_inputs():
    """{name: (counts, (seen, kept, counted))} of the inputs, computed once: the same in every state that holds them"""
    p = dist_inputs(SEED, N, VTH, GRID)
    return {name: distribution_ref(p, GRID, desc, stats=True) for name, desc in descriptors().items()}


def build_state(V, L, state):
    """(engine, species) with the test's particles in the array state asked for (species_states.build_state)"""
    holes = state == "tile_tail_holes"
    p = dist_inputs(SEED, N, VTH, GRID, spread=0.95 if holes else 1.0)
    p["tag"] = np.arange(N) + 1
    tail = None
    if holes:
        tail = dist_inputs(SEED + 1, N_TAIL, VTH, GRID, spread=0.95)
        tail["tag"] = np.arange(N_TAIL) + 2 * 10 ** 7
    # the doomed 300: 0.99 + 2 * 0.95 * 0.02 > 1, through the wall
    return species_states.build_state(V, state, p, GRID, tail, dt=0.02 if holes else 0.4, doomed_dx=0.99)


def check_state(state):
    V = package()
    L = V.layout
    eng = importlib.import_module("old-vpic_amd.engine")
    descs = descriptors(VTH, eng.DIST_LDS_BINS)
    e, sp = build_state(V, L, state)
    got = {}
    for name, desc in descs.items():
        counts = e.distribution(sp, desc["axes"], desc.get("select", ()))
        stats = e.distribution_stats()
        again = e.distribution(sp, desc["axes"], desc.get("select", ()))
        assert counts.tobytes() == again.tobytes() and stats == e.distribution_stats(), name      # two calls: identical bytes
        got[name] = (counts, stats)
    if state == "tile_tail_holes":
        back = e.get_particles(sp)                           # (after the calls: a download drops the dead slots)
        assert len(back) == N + N_TAIL
        want = {}
        for name, desc in descs.items():
            assert log_margin(back, GRID, desc) > 1e-9, name                                      # nobody is left out
            want[name] = distribution_ref(back, GRID, desc, stats=True)
    else:
        want = reference_of_the_inputs()
    e.close()
    for name, desc in descs.items():
        counts, stats = got[name]
        want_counts, want_stats = want[name]
        print(f"{state} ({name}): seen {stats[0]} kept {stats[1]} counted {stats[2]} through global memory {stats[3]}; "
              f"expected {want_stats}, differing bins {int((counts != want_counts).sum()) if counts.shape == want_counts.shape else 'shape'}")
        assert counts.dtype == np.uint64 and counts.shape == want_counts.shape
        assert np.array_equal(counts, want_counts), name
        assert stats[:3] == want_stats and int(counts.sum()) == stats[2], name
        if name in IN_LDS:
            assert stats[3] == 0, name
        if name in GLOBAL:
            assert stats[3] == stats[2], name
        if name in WINDOW and state in ("voxel", "tile", "tile_only"):
            assert stats[3] == 0, name
        if name in WINDOW and state == "tile_tail_holes":
            assert stats[3] <= N_TAIL, name


def run_child(args, timeout):
    species_states.run_child(__file__, args, timeout)


@pytest.mark.parametrize("state", STATES)
def test_counts_equal_the_restatement_exactly(state):
    if state == "tile_only":
        run_child([state], timeout=600)                      # the knob is read when the engine is created: a fresh process
    else:
        check_state(state)


@pytest.mark.parametrize("axis", ["y", "z"])
def test_window_along_y_and_z(axis):
    """The sliding window with Y or Z as the position axis (the grid of the other tests is too short for one there):
    the same particles on a grid that is long in that direction, in tile order and unsorted."""
    V = package()
    grid = {"y": (8, 96, 6), "z": (6, 8, 96)}[axis]
    nx, ny, nz = grid
    p = dist_inputs(SEED, N, VTH, grid)
    assert np.bincount(p["i"])[np.bincount(p["i"]) > 0].min() >= 64
    w = 3.0 * VTH
    descs = [dict(axes=[(axis, 0.0, 1.0, 96), ("ux", -w, 2 * w / 128, 128)]),
             dict(axes=[("uz", -w, 2 * w / 100, 100), (axis, 0.25, 0.75, 126)], select=[("x", 0.5, 5.5)])]
    want = [distribution_ref(p, grid, d, stats=True) for d in descs]
    for order in ("unsorted", "tile"):
        e = V.Engine(V.make_grid(nx, ny, nz, float(nx), float(ny), float(nz), np.float32(0.4)))
        sp = e.new_species(-1.0, N + 4096, 8192)
        e.set_particles(sp, p)
        if order == "tile":
            e.set_sort_order("engine")
            e.sort_p(sp)
            assert e.species_order(sp) == "tile"
        for d, (want_counts, want_stats) in zip(descs, want):
            counts = e.distribution(sp, d["axes"], d.get("select", ()))
            stats = e.distribution_stats()
            print(f"{axis} {order}: {stats}, expected {want_stats}, differing bins {int((counts != want_counts).sum())}")
            assert np.array_equal(counts, want_counts) and stats[:3] == want_stats
            if order == "tile":
                assert stats[3] == 0
        e.close()


def test_small_and_empty_species():
    """Fewer particles than one wavefront, on the edges of bins and ranges and with ke == 0 among them (the hand-made
    particles of the CPU test that an upload accepts: it refuses a dead slot and a ghost voxel), through all three
    paths; and an empty species."""
    from test_distribution_ref import HAND_GRID, handmade
    V = package()
    nx, ny, nz = HAND_GRID
    e = V.Engine(V.make_grid(nx, ny, nz, float(nx), float(ny), float(nz), np.float32(0.4)))
    sp = e.new_species(-1.0, 64, 8)
    assert not e.distribution(sp, [("x", 0.0, 0.75, 4)]).any() and e.distribution_stats() == (0, 0, 0, 0)
    p = handmade()[[0, 1, 2, 5, 6]]
    p["q"] = -0.01
    e.set_particles(sp, p)
    for desc in (dict(axes=[("x", 0.0, 0.75, 4)]), dict(axes=[("y", 0.0, 0.5, 4), ("z", 0.0, 0.25, 4)]),
                 dict(axes=[("uy", -1.0, 1.0, 2)], select=[("x", 0.0, 3.0), ("uz", -0.5, 0.5)]),
                 dict(axes=[("ke", 0.0, 0.25, 9)]), dict(axes=[("log10_ke", -5.0, 1.0, 6)]),
                 dict(axes=[("x", -1.0, 1.0, 5)], select=[("log10_ke", -4.5, np.inf)]),
                 dict(axes=[("x", -1.0, 0.125, 100), ("ke", 0.0, 0.025, 90)]),                # the window, 9 000 bins
                 dict(axes=[("ke", 0.0, 0.25, 20), ("x", -1.0, 0.001, 5000)]),                # bins too fine for a window: global adds
                 dict(axes=[("ux", -1.0, 0.01, 500), ("ke", 0.0, 0.25, 20)])):                # no position axis: global adds
        counts = e.distribution(sp, desc["axes"], desc.get("select", ()))
        want, want_stats = distribution_ref(p, HAND_GRID, desc, stats=True)
        assert np.array_equal(counts, want), desc
        assert e.distribution_stats()[:3] == want_stats, desc
    e.close()


def hash32(x):
    x = x ^ (x >> np.uint32(16))
    x = x * np.uint32(0x7feb352d)
    x = x ^ (x >> np.uint32(15))
    x = x * np.uint32(0x846ca68b)
    return x ^ (x >> np.uint32(16))


def loader_draw(seed, first, count):
    """the 24-bit integers h >> 8 behind the dx of particles [first, first + count) as load_maxwellian draws them
    (csrc/particles.hip: u01 of stream 0): integer hashing, exact in numpy"""
    idx = np.arange(first, first + count, dtype=np.uint32)
    with np.errstate(over="ignore"):
        salt = hash32(np.uint32(seed) * np.uint32(0x9e3779b9))
        return hash32(hash32(idx * np.uint32(9)) ^ salt) >> np.uint32(8)


def loader_dx(draw):
    """... and the dx made of them, dx = 2 * ((draw + 0.5f) / 2^24) - 1 in float: correctly rounded operations, exact in numpy"""
    u = (draw.astype(np.float32) + np.float32(0.5)) * np.float32(1.0 / 16777216.0)
    return np.float32(2.0) * u - np.float32(1.0)


def test_cold_beam_at_size():
    """2^28 particles in one species (256^3 cells x 16 per cell), a cold beam (vth = 0, drift 0.2 in x): x-ux at 256 x 256
    bins through the sliding window, every particle in the ONE momentum bin that holds the drift, a whole wavefront
    adding to a few words throughout.  No host pass over the particles: the expected counts follow from the loader.

    Every x bin of that row would hold exactly 16 * 256 * 256 = 2^20 if every particle were strictly inside its cell.  The
    loader draws dx = 2 * u01 - 1 in float with u01 = ((h >> 8) + 0.5f) / 2^24, and for h >> 8 = 2^24 - 1 the sum rounds up
    to 2^24: one draw in 2^24 -- 16 or so of these 2^28 -- gives dx = 1.0f exactly, a particle ON the upper face of its
    cell, X = cx, which the clean rule (bin = (int)t, t < n) puts in the NEXT bin, or in none behind the last cell.  The
    draws are integer hashes, so this test finds those particles exactly (loader_draw and loader_dx, a restatement checked below against
    the first 65 536 particles that the device drew) and demands, bin for bin, 2^20 less those that left plus those that
    came: still exact equality of every one of the 65 536 bins, and out[2] = 2^28 less the particles on the domain's face."""
    V = package()
    n_cells, ppc, seed = 256, 16, 11
    n = n_cells ** 3 * ppc
    assert n == 2 ** 28
    e = V.Engine(V.make_grid(n_cells, n_cells, n_cells, float(n_cells), float(n_cells), float(n_cells), np.float32(0.5)))
    sp = e.new_species(-1.0, n, 4096)
    e.load_maxwellian(sp, ppc, seed, -1e-3, (0.2, 0.0, 0.0), 0.0)
    counts = e.distribution(sp, [("x", 0.0, 1.0, 256), ("ux", -1.0, 2.0 / 256, 256)])
    stats = e.distribution_stats()
    head = e.get_particles_range(sp, 0, 1 << 16)
    e.close()
    assert np.array_equal(head["dx"].view(np.uint32), loader_dx(loader_draw(seed, 0, 1 << 16)).view(np.uint32))   # the restatement is the loader
    assert np.all(head["ux"] == np.float32(0.2))
    top = np.uint32((1 << 24) - 1)                           # the one draw that gives dx == 1, the next one down does not
    assert list(loader_dx(np.array([top, top - 1], np.uint32))) == [1.0, np.float32(1.0 - 2.0 ** -22)]
    on_face = np.zeros(n_cells + 1, np.int64)                # particles with dx == 1 by cell column cx = 1 .. 256
    chunk = 1 << 22
    with ThreadPoolExecutor(8) as pool:                      # (numpy's integer loops run outside the interpreter lock)
        for at in pool.map(lambda first: first + np.flatnonzero(loader_draw(seed, first, chunk) == top), range(0, n, chunk)):
            np.add.at(on_face, (at // ppc) % n_cells + 1, 1)
    row = int((np.float64(np.float32(0.2)) + 1.0) / (2.0 / 256))
    want = np.zeros((256, 256), np.uint64)
    want[row] = (ppc * n_cells * n_cells - on_face[1:] + on_face[:-1]).astype(np.uint64)
    print(f"cold beam: {n} particles, seen {stats[0]} kept {stats[1]} counted {stats[2]} through global memory {stats[3]}; "
          f"momentum row {row}, particles on an upper cell face {int(on_face.sum())}, of them on the domain's {int(on_face[-1])}; "
          f"differing bins {int((counts != want).sum())}")
    assert row == 153
    assert counts.shape == (256, 256) and np.array_equal(counts, want)
    assert stats[0] == stats[1] == n and stats[2] == n - int(on_face[-1]) == int(counts.sum())
    assert int(counts[row].sum()) > 2 ** 24 and int(counts[row].min()) >= 2 ** 20 - 4


def test_argument_errors():
    V = package()
    eng = importlib.import_module("old-vpic_amd.engine")
    l = V.lib()
    e = V.Engine(V.make_grid(4, 4, 4, 4.0, 4.0, 4.0, np.float32(0.4)))
    sp = e.new_species(-1.0, 64, 8)
    counts = np.zeros(1 << 16, np.uint64)
    cp = counts.ctypes.data_as(C.c_void_p)

    def call(axes, select=(), species=sp, counts_ptr=cp, patch=None):
        d = eng.dist_desc(axes, select)
        if patch:
            patch(d)
        return l.vpic_hip_species_distribution(e._h, species, C.byref(d), counts_ptr)

    def fails(rc, word):
        assert rc != 0
        msg = l.vpic_hip_last_error().decode()
        assert word in msg, msg

    ok = [("ux", -1.0, 0.5, 4)]
    assert call(ok) == 0
    fails(call(ok, species=sp + 1), "species")
    fails(call(ok, species=-1), "species")
    fails(l.vpic_hip_species_distribution(e._h, sp, None, cp), "descriptor")
    fails(call(ok, counts_ptr=None), "counts")
    fails(call(ok, patch=lambda d: setattr(d, "n_axes", 0)), "axes")
    fails(call(ok, patch=lambda d: setattr(d, "n_axes", 3)), "axes")
    fails(call(ok, patch=lambda d: setattr(d, "n_sel", -1)), "ranges")
    fails(call(ok, patch=lambda d: setattr(d, "n_sel", 5)), "ranges")
    fails(call(ok, patch=lambda d: setattr(d.axis[0], "coord", 8)), "coordinate")
    fails(call(ok, patch=lambda d: setattr(d.axis[0], "coord", -1)), "coordinate")
    fails(call(ok, [("ke", 0.0, 1.0)], patch=lambda d: setattr(d.sel[0], "coord", 8)), "coordinate")
    fails(call([("ux", -1.0, 0.5, 0)]), "bins")
    fails(call([("ux", -1.0, 0.5, 4), ("x", 0.0, 1.0, -2)]), "bins")
    for width in (0.0, -0.5, np.inf, np.nan):
        fails(call([("ux", -1.0, width, 4)]), "width")
    fails(call([("ux", -1.0, 0.5, 2048), ("uy", -1.0, 0.5, 2049)]), "cap")
    fails(call([("ux", -1.0, 0.5, 1 << 30), ("uy", -1.0, 0.5, 1 << 30)]), "cap")
    fails(l.vpic_hip_species_distribution_stats(e._h, None), "output")
    with pytest.raises(V.VpicHipError):
        e.distribution(sp, [("ux", -1.0, 0.0, 4)])
    with pytest.raises(KeyError):
        e.distribution(sp, [("pitch", -1.0, 0.5, 4)])
    # the engine is still usable, and the cap itself is accepted
    big = e.distribution(sp, [("ux", -1.0, 0.5, 2048), ("uy", -1.0, 0.5, 2048)])
    assert big.shape == (2048, 2048) and not big.any() and e.distribution_stats() == (0, 0, 0, 0)
    one = np.zeros(1, V.layout.particle_t)
    one["i"], one["ux"], one["q"] = voxel(1, 1, 1, (4, 4, 4)), 0.25, -0.01
    e.set_particles(sp, one)
    assert list(e.distribution(sp, ok)) == [0, 0, 1, 0] and e.distribution_stats() == (1, 1, 1, 0)
    e.close()


if __name__ == "__main__":
    check_state(sys.argv[1])
    print("child OK")
