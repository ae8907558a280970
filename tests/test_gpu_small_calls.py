"""The species calls beside the push on the GPU: center_p, uncenter_p, energy_p and load_maxwellian.

center_p / uncenter_p against the oracle's orc_center_p / orc_uncenter_p, EXACT: every word of every live particle as bytes,
in every array state (species_states.STATES), on grids 5x3x4 and 9x6x5, for q_m = -1 and 1 / 1836, with records that are
zero, weak, strong (the rotation far from its small-angle regime), E only, B only and subnormal, through uncenter_p, center_p,
center_p; the array order, the bookkeeping, the dead slots and the interpolator are what they were.

energy_p against the exact sum of the float chain's terms (small_calls_ref.energy_terms / energy_exact) within the bound of
the device's summation tree: HEIGHT additions at most on a term's way to the result.

load_maxwellian against its rule restated (small_calls_ref.loader_ref): cells, offsets and charge as bytes, the momenta
within the bound derived from the roundings of the float chain (small_calls_ref.loader_bound).  The loaded array is
cell-sorted by construction, but sort_p afterwards is NOT held to leave it byte for byte: the sort by voxel places the
particles of a cell in no fixed order (csrc/engine.hip: vpic_hip_debug_set_momenta says so), it promises no stability.

No tolerance here comes from what the device returned."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import small_calls_ref as R  # noqa: E402
import species_states  # noqa: E402
from oracle import pyorc  # noqa: E402
from species_states import N_DOOMED, N_TAIL, STATES, package  # noqa: E402
from test_cool_ref import GRIDS  # noqa: E402
from test_gpu_cool import bookkeeping, snapshot  # noqa: E402
from test_gpu_load import environment  # noqa: E402

pytestmark = pytest.mark.gpu
QMS = [-1.0, 1.0 / 1836.0]
# csrc/engine.hip: engine->dsum_count = 6 * 1024 partial sums, one per workgroup of energy_p_kernel (csrc/push.hip), 256 threads
# each; the header gives no way to read it
PARTIALS, BLOCK = 6144, 256
SPAN = PARTIALS * BLOCK                # particles per trip of the kernel's grid-stride loop


def height(extent):
    """additions on a term's way through energy_p: the trips of the stride loop over the array's extent, 6 shuffle steps,
    2 for the fold of the four wavefronts, the host's loop over the partials"""
    return max(1, -(-extent // SPAN)) + 6 + 2 + PARTIALS


class WithQm:
    """the package as species_states.build_state sees it, its engines creating their species at q_m (build_state's own is -1)"""

    def __init__(self, V, q_m):
        self._V, self._q_m = V, q_m

    def __getattr__(self, name):
        return getattr(self._V, name)

    def Engine(self, grid):
        e = self._V.Engine(grid)
        new = e.new_species
        e.new_species = lambda q_m, max_np, max_nm: new(self._q_m, max_np, max_nm)
        return e


def orc_grid(grid, dt):
    nx, ny, nz = grid
    return pyorc.make_grid(nx, ny, nz, float(nx), float(ny), float(nz), np.float32(dt))


def build(V, state, grid, seed, q_m):
    """(engine, species, the oracle's grid) with R.N generated particles in the array state asked for; the fields are zero
    while the state is built, so the one push of "tile_tail_holes" moves positions only.  There |v| < 1, cells of size 1
    and dt = 0.2: 0.5 + 2 * 0.2 < 1, nobody but the doomed leaves a cell; they do: 0.99 + 2 * 0.95 * 0.2 > 1"""
    holes = state == "tile_tail_holes"
    p = R.particles(seed, R.N, grid, spread=0.5 if holes else 1.0)
    tail = R.particles(seed + 1, N_TAIL, grid, spread=0.5, tag0=2 * 10 ** 7) if holes else None
    dt = 0.2 if holes else 0.4
    e, sp = species_states.build_state(WithQm(V, q_m), state, p, grid, tail, dt=dt, doomed_dx=0.99)
    return e, sp, orc_grid(grid, dt)


def check_energy(e, sp, p, fi, q_m, og, extent, what):
    """energy_p of the species whose live particles are p, within the bound of the device's tree; returns the value"""
    t = R.energy_terms(p, fi, q_m, og)
    exact, sabs = R.energy_exact(t, q_m, og)
    got = e.energy_p(sp)
    bound = R.energy_bound(height(extent), sabs, exact, q_m, og)
    err = float(abs(Fraction(got) - exact))
    sequential = pyorc.energy_p(p, len(p), q_m, fi, og) if len(p) else 0.0
    err_seq = float(abs(Fraction(sequential) - exact))
    print(f"energy_p {what}: np {len(p)} extent {extent} exact {float(exact):.17g} device {got:.17g} err {err:.3g} "
          f"sequential err {err_seq:.3g} bound {bound:.3g} sum|t| c^2/|q_m| {sabs * R.energy_scale(q_m, og):.6g}")
    assert err <= bound, what
    assert err_seq <= bound, what                                         # the bound is not vacuous: the oracle's own sum is inside
    if len(p):
        assert 0 < bound < 1e-11 * sabs * R.energy_scale(q_m, og), what   # ... and not loose
    else:
        assert got == 0.0
    return got


def check_state(state, g):
    V = package()
    grid = GRIDS[g]
    holes = state == "tile_tail_holes"
    for q_m in QMS:
        e, sp, og = build(V, state, grid, 70 + g, q_m)
        fi = R.interpolator(80 + g, grid)
        e.set_interpolator(fi)
        p0, idx0 = snapshot(e, sp)
        book = bookkeeping(e, sp)
        extent = e.capacity(sp)[0]
        assert len(p0) == R.N + (N_TAIL if holes else 0) and book[0]["dead_slots"] == (N_DOOMED if holes else 0)
        assert extent == len(p0) + (N_DOOMED if holes else 0) and idx0.max() < extent and (np.diff(idx0) > 0).all()
        prev = p0
        check_energy(e, sp, p0, fi, q_m, og, extent, (state, grid, q_m, "as built"))
        for call in ("uncenter_p", "center_p", "center_p"):
            ref = prev.copy()
            getattr(pyorc, call)(ref, len(ref), q_m, fi, og)
            getattr(e, call)(sp)
            got, idx = snapshot(e, sp)
            what = (state, grid, q_m, call)
            assert got.tobytes() == ref.tobytes(), what                       # every word of every live particle
            assert np.array_equal(idx, idx0) and bookkeeping(e, sp) == book, what
            assert e.species_stats(sp)["dead_slots"] == (N_DOOMED if holes else 0), what
            assert e.get_interpolator().tobytes() == fi.tobytes(), what
            changed = (got["ux"] != prev["ux"]) | (got["uy"] != prev["uy"]) | (got["uz"] != prev["uz"])
            assert changed.mean() > 0.3, what                                  # (the call did something: the zero and subnormal records and the fast particles under weak ones aside)
            check_energy(e, sp, got, fi, q_m, og, extent, what)
            after, idx = snapshot(e, sp)
            assert after.tobytes() == got.tobytes() and np.array_equal(idx, idx0) and bookkeeping(e, sp) == book, what   # energy_p touched nothing
            prev = got
        e.close()


@pytest.mark.parametrize("g", [0, 1])
@pytest.mark.parametrize("state", STATES)
def test_center_uncenter_energy_in_every_state(state, g):
    # a grid thinner than a tile on some axis (5x3x4) takes the tile order only when told to; the knobs are read when the
    # engine is created, and "tile_only" needs a fresh process for its own
    with environment(**(dict(VPIC_HIP_WINDOW="tile") if state.startswith("tile") else {})):
        if state == "tile_only":
            species_states.run_child(__file__, [state, g], timeout=300)
        else:
            check_state(state, g)


def plain_engine(V, grid, dt=0.4):
    nx, ny, nz = grid
    e = V.Engine(V.make_grid(nx, ny, nz, float(nx), float(ny), float(nz), np.float32(dt)))
    return e, orc_grid(grid, dt)


def test_center_p_particle_counts():
    """np = 1, around a workgroup, and 20 000, as uploaded: the ragged last block; np = 0 returns without an error"""
    V = package()
    grid = GRIDS[1]
    fi = R.interpolator(81, grid)
    everything = R.particles(71, R.N, grid)
    e, og = plain_engine(V, grid)
    e.set_interpolator(fi)
    sp = e.new_species(-1.0, R.N, 8)
    for call in ("center_p", "uncenter_p"):
        getattr(e, call)(sp)                                                   # np == 0
        assert e.np(sp) == 0
    assert e.energy_p(sp) == 0.0
    for n in (1, BLOCK - 1, BLOCK, BLOCK + 1, R.N):
        # (the tail of the array, so that the hand-made particles are in every size but the first)
        p = everything[R.N - n:] if n > 1 else everything[:1]
        for call in ("center_p", "uncenter_p"):
            e.set_particles(sp, p)
            ref = p.copy()
            getattr(pyorc, call)(ref, n, -1.0, fi, og)
            getattr(e, call)(sp)
            got, idx = snapshot(e, sp)
            assert got.tobytes() == ref.tobytes() and np.array_equal(idx, np.arange(n)), (n, call)
    e.close()


def test_energy_p_nearly_cancels():
    """the second half holds the first half's particles with -q, three particles have no twin: sum t is a few terms, sum |t|
    all of them -- the bound is stated on sum |t|, and holds"""
    V = package()
    grid = GRIDS[1]
    fi = R.interpolator(81, grid)
    half = R.particles(71, R.N, grid)[R.N // 2 + 3:]
    twin = half[3:].copy()
    twin["q"] = -twin["q"]
    twin["tag"] += 10 ** 6
    p = np.concatenate([half, twin])
    for q_m in QMS:
        e, og = plain_engine(V, grid)
        e.set_interpolator(fi)
        sp = e.new_species(q_m, len(p), 8)
        e.set_particles(sp, p)
        t = R.energy_terms(p, fi, q_m, og)
        exact, sabs = R.energy_exact(t, q_m, og)
        assert exact == R.energy_exact(t[:3], q_m, og)[0] != 0 and sabs > 1000 * abs(float(R.exact_sum(t)))
        check_energy(e, sp, p, fi, q_m, og, len(p), ("cancel", q_m))
        assert e.get_particles(sp).tobytes() == p.tobytes()
        e.close()


def test_energy_p_launch_shapes():
    """np = 1, around a workgroup (the fold of a partly filled last block), and around one and two trips of the grid-stride
    loop; the generated particles tiled, every copy with a weight factor of its own, one upload each"""
    V = package()
    grid = GRIDS[1]
    fi = R.interpolator(81, grid)
    q_m = -1.0
    base = R.particles(71, R.N, grid)
    n_max = 2 * SPAN + 77
    copies = -(-n_max // R.N)
    everything = np.tile(base, copies)[:n_max]
    factor = (1.0 + (np.arange(n_max) // R.N) / 64.0) * np.where((np.arange(n_max) // R.N) % 3 == 2, -1.0, 1.0)
    everything["q"] = (everything["q"].astype(np.float64) * factor).astype(np.float32)
    everything["tag"] = 0
    e, og = plain_engine(V, grid)
    e.set_interpolator(fi)
    sp = e.new_species(q_m, n_max, 8)
    t_all = R.energy_terms(everything, fi, q_m, og)                           # (computed once: a prefix's terms are the prefix of it)
    seen = set()
    for n in (1, BLOCK - 1, BLOCK, BLOCK + 1, SPAN - 1, SPAN, SPAN + 1, n_max):
        p = everything[:n]
        e.set_particles(sp, p)
        exact, sabs = R.energy_exact(t_all[:n], q_m, og)
        got = e.energy_p(sp)
        bound = R.energy_bound(height(n), sabs, exact, q_m, og)
        err = float(abs(Fraction(got) - exact))
        err_seq = float(abs(Fraction(pyorc.energy_p(p, n, q_m, fi, og)) - exact))
        print(f"energy_p np {n}: trips {-(-n // SPAN)} exact {float(exact):.17g} device {got:.17g} err {err:.3g} sequential err {err_seq:.3g} bound {bound:.3g}")
        assert err <= bound and err_seq <= bound and 0 < bound < 1e-11 * sabs * R.energy_scale(q_m, og), n
        assert e.np(sp) == n
        seen.add(got)
    assert len(seen) == 8                                                       # (the one particle behind a span's end counts)
    assert height(SPAN) == 1 + 8 + PARTIALS and height(SPAN + 1) == 2 + 8 + PARTIALS and height(n_max) == 3 + 8 + PARTIALS
    e.close()


# ---- load_maxwellian ----
DRIFTS = {0.0: (0.25, -0.125, 0.0625), 0.02: (0.03, -0.02, 0.01), 0.6: (0.3, -0.2, 0.1)}


@pytest.mark.parametrize("grid", [(5, 3, 4), (8, 8, 8)])
def test_load_maxwellian_equals_its_rule(grid):
    V = package()
    nx, ny, nz = grid
    e, _ = plain_engine(V, grid)
    sp = e.new_species(-1.0, nx * ny * nz * 64, 8)
    draws = {}
    for ppc in (1, 7, 64):
        for seed in (1, 2):
            for vth, drift in DRIFTS.items():
                q = -0.75 / ppc
                ref = R.loader_ref(grid, ppc, seed, q, drift, vth)
                e.load_maxwellian(sp, ppc, seed, q, u=drift, vth=vth)
                what = (grid, ppc, seed, vth)
                assert e.np(sp) == ref.np == nx * ny * nz * ppc and e.nm(sp) == 0, what
                p, idx = snapshot(e, sp)
                assert np.array_equal(idx, np.arange(ref.np)), what
                assert np.array_equal(p["i"], ref.i) and (np.diff(p["i"]) >= 0).all(), what
                for c in ("dx", "dy", "dz", "q"):
                    assert p[c].tobytes() == getattr(ref, c).tobytes(), (what, c)
                assert not p["tag"].any() and not p["tag2"].any(), what
                u = np.stack([p["ux"], p["uy"], p["uz"]], axis=1)
                if vth == 0.0:
                    assert u.tobytes() == np.tile(np.array(drift, np.float32), (ref.np, 1)).tobytes(), what
                else:
                    err = np.abs(u.astype(np.float64) - ref.u)
                    bound = R.loader_bound(ref)
                    print(what, "largest error / bound per component:", (err / bound).max(axis=0), "largest error / vth:", err.max() / vth)
                    assert (err <= bound).all(), what
                    assert (bound[ref.r <= 5.0] < 1e-5 * vth).all(), what
                draws[(ppc, seed)] = p["dx"].copy()
        assert not np.array_equal(draws[(ppc, 1)], draws[(ppc, 2)])             # the two seeds draw differently
        assert (draws[(ppc, 1)] != draws[(ppc, 2)]).mean() > 0.99
    assert 5 * 3 * 4 * 7 % BLOCK != 0                                           # (np = 420: a ragged last block)
    e.close()


def test_load_maxwellian_clears_the_tags():
    """include/vpic_hip.h: the loaded particles carry tag = tag2 = 0, whatever tags the species held before -- and tags
    switched on again afterwards start from zeros"""
    V = package()
    grid = (5, 3, 4)
    e, _ = plain_engine(V, grid)
    n = 5 * 3 * 4 * 7
    sp = e.new_species(-1.0, 2 * n, 8)
    old = R.particles(72, 2 * n, grid)
    old["tag"] = np.arange(2 * n) + 5
    old["tag2"] = -np.arange(2 * n) - 9
    e.set_particles(sp, old)
    assert e.get_particles(sp).tobytes() == old.tobytes()
    e.load_maxwellian(sp, 7, 1, -0.1, u=(0.0, 0.0, 0.0), vth=0.1)
    p, _ = snapshot(e, sp)
    ref = R.loader_ref(grid, 7, 1, -0.1, (0.0, 0.0, 0.0), 0.1)
    assert len(p) == n and np.array_equal(p["i"], ref.i) and p["dx"].tobytes() == ref.dx.tobytes()
    assert not p["tag"].any() and not p["tag2"].any()
    back = e.get_particles(sp)
    assert not back["tag"].any() and not back["tag2"].any()
    more = old[:10].copy()
    e.append_particles(sp, more)                                                 # tags on again: the loaded ones still read zero
    p, _ = snapshot(e, sp)
    assert len(p) == n + 10 and not p["tag"][:n].any() and not p["tag2"][:n].any()
    assert p[n:].tobytes() == more.tobytes()
    e.sort_p(sp)                                                                 # ... through a sort as well
    p = e.get_particles(sp)
    assert sorted(p["tag"].tolist()) == [0] * n + list(range(5, 15))
    assert sorted(p["tag2"].tolist()) == list(range(-18, -8)) + [0] * n
    e.close()


if __name__ == "__main__":
    check_state(sys.argv[1], int(sys.argv[2]))
    print("child OK")
