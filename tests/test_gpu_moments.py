"""accumulate_hydro_p / accumulate_rho_p summed by tile, and bit-reproducible in deterministic mode (csrc/moments.hip).

The deck: a 10 x 7 x 3 grid (partial tiles on every axis, one axis thinner than a tile, nv = 540) with reflecting z walls,
random non-zero E and B through the oracle's load_interpolator, 24 particles in every cell (5040: more than 4 nv, where the
float path of an unsorted species sorts by voxel), q uniform in +-50 %, u ~ 0.3 normal, tags 1..n.  Sums are held to the
oracle's accumulate_hydro_p / accumulate_rho_p within ACC_TOL = 2e-6 of each moment's largest entry (the file-wide tolerance
of test_gpu_kernels.py for summed quantities); deterministic sums are compared BIT FOR BIT with one another.

A grid with an axis thinner than a tile is not put into tile order by the engine's own choice (policy.h: wants_tile_order),
so the states in tile order are made under VPIC_HIP_WINDOW=tile, which the engine reads when it is created; the states
"unsorted" and "voxel" are made without it, and in deterministic mode take the per-particle pass (the engine would not push
them in tile order); "unsorted_wants_tile" is the unsorted array under the knob, which a deterministic call sorts by tile
first.  "tile_only" (VPIC_HIP_TILE_COARSE=1) and VPIC_HIP_MOMENTS_TILED=0 run in a fresh child process each.
"tile_tail_holes": tile order, 600 appended particles, then one step of the resident exchange with absorbing x walls which
removes 60 particles placed for it and leaves their slots dead; its particles are not the inputs any more (the step moved
them), so it is compared with the oracle on what get_particles returns afterwards, and bit for bit with itself.

This file proves reproducibility (GPU results against one another) and closeness to the largest entry; correctness node by
node -- every deterministic word against an exact reference, every float word within a derived bound, on more grids, q_m,
charges and momenta -- is tests/test_gpu_moments_exact.py."""
import contextlib
import functools
import importlib
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from species_states import package  # noqa: E402

pytestmark = pytest.mark.gpu
ACC_TOL = 2e-6
GRID = (10, 7, 3)
PPC = 24
N = GRID[0] * GRID[1] * GRID[2] * PPC
N_TAIL, N_DOOMED = 600, 60
SEED = 20261017
STATES = ["unsorted", "voxel", "unsorted_wants_tile", "tile", "tile_only", "tile_tail_holes"]
IN_TILE_ORDER = ("unsorted_wants_tile", "tile", "tile_only", "tile_tail_holes")


def oracle():
    from oracle import pyorc
    pyorc.lib()
    return pyorc


@contextlib.contextmanager
def environment(**values):
    old = {k: os.environ.get(k) for k in values}
    os.environ.update(values)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def walls(L, state="tile", periodic=False):
    if periodic:
        return {}
    kw = dict(fbc=[0, 0, L.PEC_FIELDS, 0, 0, L.PEC_FIELDS], pbc=[0, 0, L.REFLECT_PARTICLES, 0, 0, L.REFLECT_PARTICLES])
    if state == "tile_tail_holes":
        kw["pbc"] = [L.ABSORB_PARTICLES, 0, L.REFLECT_PARTICLES, L.ABSORB_PARTICLES, 0, L.REFLECT_PARTICLES]
    return kw


def grids(V, L, state="tile", dt=0.02, periodic=False):
    nx, ny, nz = GRID
    args = (nx, ny, nz, float(nx), float(ny), float(nz), np.float32(dt))
    return V.make_grid(*args, **walls(L, state, periodic)), oracle().make_grid(*args, **walls(L, state, periodic))


def new_engine(V, grid, tile_knob):
    if tile_knob:
        with environment(VPIC_HIP_WINDOW="tile"):
            return V.Engine(grid)
    return V.Engine(grid)


def all_cells(count):
    nx, ny, nz = GRID
    L = importlib.import_module("old-vpic_amd.layout")
    x, y, z = np.meshgrid(np.arange(1, nx + 1), np.arange(1, ny + 1), np.arange(1, nz + 1), indexing="ij")
    return np.repeat(L.voxel(x.ravel(), y.ravel(), z.ravel(), nx, ny, nz), count)


def make_particles(seed, n=N, spread=1.0, first_tag=1):
    """n particles: `PPC` in every cell when n == N, else in random cells"""
    L = importlib.import_module("old-vpic_amd.layout")
    rng = np.random.default_rng(seed)
    nx, ny, nz = GRID
    p = np.zeros(n, L.particle_t)
    for c in ("dx", "dy", "dz"):
        p[c] = rng.uniform(-spread, spread, n).astype(np.float32)
    p["i"] = all_cells(PPC) if n == N else L.voxel(rng.integers(1, nx + 1, n), rng.integers(1, ny + 1, n), rng.integers(1, nz + 1, n), nx, ny, nz)
    for c in ("ux", "uy", "uz"):
        p[c] = (rng.standard_normal(n) * 0.3).astype(np.float32)
    p["q"] = rng.uniform(0.5, 1.5, n).astype(np.float32) * np.float32(-0.01)
    p["tag"] = np.arange(n) + first_tag
    return p


@functools.lru_cache(maxsize=None)
def deck():
    """(fields, interpolator, particles, oracle hydro, oracle rhof) of the common deck, computed once and left unchanged"""
    V = package()
    L = V.layout
    orc = oracle()
    _, og = grids(V, L)
    rng = np.random.default_rng(SEED)
    f = np.zeros(og.nv, L.field_t)
    for c in ("ex", "ey", "ez", "cbx", "cby", "cbz"):
        f[c] = (rng.standard_normal(og.nv) * 0.2).astype(np.float32)
    fi = np.zeros(og.nv, L.interpolator_t)
    orc.load_interpolator(fi, f, og)
    p = make_particles(SEED + 1)
    ref_h, ref_rho = reference(p, -1.0, fi)
    for a in (f, fi, p, ref_h, ref_rho):
        a.setflags(write=False)
    return f, fi, p, ref_h, ref_rho


def reference(p, q_m, fi, periodic=False):
    V = package()
    L = V.layout
    orc = oracle()
    _, og = grids(V, L, periodic=periodic)
    p = np.array(p)
    h = np.zeros(og.nv, L.hydro_t)
    orc.accumulate_hydro_p(h, p, len(p), q_m, np.array(fi), og)
    f = np.zeros(og.nv, L.field_t)
    orc.accumulate_rho_p(f, p, len(p), og)
    return h, f["rhof"].copy()


def moments(h):
    return [c for c in h.dtype.names[:14]]


def hydro_bits(h):
    return np.stack([h[c].view(np.uint32) for c in moments(h)])


def assert_close(got, ref, what):
    for c in (moments(ref) if ref.dtype.names else [None]):
        g, r = (got[c], ref[c]) if c else (got, ref)
        err, top = float(np.abs(g.astype(np.float64) - r).max()), float(np.abs(r).max())
        print(f"{what} {c or 'rhof'}: max error {err:.3e}, largest entry {top:.3e}, ratio {err / top if top else 0.0:.2e}")
        assert err <= ACC_TOL * top, (what, c)


def build_state(state, perm_seed, mode):
    """(engine, species) holding the deck's particles, uploaded in the order of a permutation, in the array state asked for"""
    V = package()
    L = V.layout
    f, fi, p, _, _ = deck()
    holes = state == "tile_tail_holes"
    g, _ = grids(V, L, state)
    e = new_engine(V, g, state in IN_TILE_ORDER)
    e.set_fields(np.array(f)); e.set_interpolator(np.array(fi))
    e.set_accumulation(mode)
    sp = e.new_species(-1.0, N + N_TAIL + N_DOOMED + 4096, 4096)
    p = np.array(p)
    if holes:
        p = make_particles(SEED + 1, spread=0.95)
        rng = np.random.default_rng(5)
        d = make_particles(SEED + 2, N_DOOMED, first_tag=10 ** 7)
        d["i"] = L.voxel(GRID[0], rng.integers(1, GRID[1] + 1, N_DOOMED), rng.integers(1, GRID[2] + 1, N_DOOMED), *GRID)
        d["dx"], d["ux"] = 0.99, 3.0                     # on their way through the absorbing +x wall (0.99 + 2 * 0.95 * 0.02 > 1)
        p = np.concatenate([p, d])
    p = p[np.random.default_rng(perm_seed).permutation(len(p))]
    e.set_particles(sp, p)
    if state == "voxel":
        e.sort_p(sp)
        assert e.species_order(sp) == "voxel"
    if state in ("tile", "tile_only", "tile_tail_holes"):
        e.sort_p(sp)
        assert e.species_order(sp) == "tile"
        assert e.species_stats(sp)["by_tile_only"] == (1 if state == "tile_only" else 0)
    if holes:
        t = make_particles(SEED + 3, N_TAIL, spread=0.95, first_tag=2 * 10 ** 7)
        e.append_particles(sp, t[np.random.default_rng(perm_seed + 1).permutation(N_TAIL)])
        e.clear_accumulators()
        e.exchange_begin()
        e.advance_p_async(sp)
        e.exchange_pack([0] * 6, [0] * 6, 4096)
        e.exchange_finish([])
        assert e.exchange_flags == 0
        assert e.species_stats(sp)["dead_slots"] == N_DOOMED
        assert e.np(sp) == N + N_TAIL
    return e, sp


def hydro_of(e, sp):
    e.clear_hydro(); e.accumulate_hydro_p(sp)
    return e.get_hydro()


def rho_of(e, sp):
    e.clear_rhof(); e.accumulate_rho_p(sp)
    return e.get_fields()["rhof"]


def deterministic_hydro(state, perm_seed):
    """(hydro, statistics, oracle hydro of the particles the state holds)"""
    e, sp = build_state(state, perm_seed, "deterministic")
    h, stats = hydro_of(e, sp), e.moments_stats()
    if state == "tile_tail_holes":
        assert stats[0] == N + N_TAIL and stats[1] + stats[2] == stats[0] and stats[2] >= N_TAIL and stats[1] > 0
        back = e.get_particles(sp)                            # (after the call: a download drops the dead slots)
        assert len(back) == N + N_TAIL
        ref = reference(back, -1.0, deck()[1])[0]
    else:
        assert stats[0] == N and stats[3] == 0
        assert stats[1] == (N if state in IN_TILE_ORDER else 0) and stats[2] == N - stats[1]
        ref = deck()[3]
    e.close()
    return h, stats, ref


@functools.lru_cache(maxsize=None)
def baseline_bits():
    """the deterministic hydro bits of the deck's particles: state "tile", computed once"""
    return hydro_bits(deterministic_hydro("tile", 100)[0])


def run_child(job, env):
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "out.npz")
        r = subprocess.run([sys.executable, os.path.abspath(__file__), job, out], env=dict(os.environ, **env), capture_output=True,
                           text=True, timeout=300)
        print(r.stdout[-4000:])
        assert r.returncode == 0 and "child OK" in r.stdout, r.stdout[-4000:] + r.stderr[-4000:]
        with np.load(out) as z:
            return {k: z[k] for k in z.files}


def child(job, out):
    if job == "tile_only":
        a, _, ref = deterministic_hydro("tile_only", 1)
        b, _, _ = deterministic_hydro("tile_only", 2)
        assert_close(a, ref, "tile_only")
        np.savez(out, a=hydro_bits(a), b=hydro_bits(b))
    if job == "untiled":                                     # VPIC_HIP_MOMENTS_TILED=0 on a species in tile order
        e, sp = build_state("tile", 1, "deterministic")
        h, stats = hydro_of(e, sp), e.moments_stats()
        assert e.species_order(sp) == "tile" and stats == (N, 0, N, 0), stats     # per particle: nothing was sorted
        rho = rho_of(e, sp)
        assert e.moments_stats() == (N, 0, N, 0)
        e.close()
        np.savez(out, hydro=hydro_bits(h), rho=rho.view(np.uint32))


@pytest.mark.parametrize("state", STATES)
def test_deterministic_hydro_does_not_depend_on_the_order(state):
    """1. every state from two permutations of the same particles: all 14 moments equal as uint32 between the two and across
    all states that hold the same particles, and within ACC_TOL of the oracle."""
    if state == "tile_only":
        got = run_child("tile_only", dict(VPIC_HIP_TILE_COARSE="1", VPIC_HIP_WINDOW="tile"))
        a, b = got["a"], got["b"]
    else:
        ha, _, ref = deterministic_hydro(state, 1)
        hb, _, _ = deterministic_hydro(state, 2)
        assert_close(ha, ref, state)
        a, b = hydro_bits(ha), hydro_bits(hb)
    print(f"{state}: words that differ between the two permutations {int((a != b).sum())}")
    assert np.array_equal(a, b)
    if state != "tile_tail_holes":
        print(f"{state}: words that differ from state tile {int((a != baseline_bits()).sum())}")
        assert np.array_equal(a, baseline_bits())


@pytest.mark.parametrize("state", ["tile", "unsorted", "tile_tail_holes"])
def test_two_calls_in_a_row_give_identical_bytes(state):
    """2. clear_hydro, then the call, twice: the same bytes and the same statistics."""
    e, sp = build_state(state, 3, "deterministic")
    h1, s1 = hydro_of(e, sp), e.moments_stats()
    h2, s2 = hydro_of(e, sp), e.moments_stats()
    r1, t1 = rho_of(e, sp), e.moments_stats()
    r2, t2 = rho_of(e, sp), e.moments_stats()
    e.close()
    assert h1.tobytes() == h2.tobytes() and s1 == s2
    assert r1.tobytes() == r2.tobytes() and t1 == t2


def test_the_paths_give_the_same_bits():
    """3. VPIC_HIP_MOMENTS_TILED=0 (every deterministic call per particle: the path accumulate_rho_p had before there was a
    tile path) gives the hydro bits and the deterministic rhof bits of the tile path."""
    got = run_child("untiled", dict(VPIC_HIP_MOMENTS_TILED="0", VPIC_HIP_WINDOW="tile"))
    assert np.array_equal(got["hydro"], baseline_bits())
    e, sp = build_state("tile", 1, "deterministic")
    rho = rho_of(e, sp)
    assert e.moments_stats() == (N, N, 0, 0)
    e.close()
    assert_close(rho, deck()[4], "deterministic rho by tile")
    assert np.array_equal(got["rho"], rho.view(np.uint32))


@pytest.mark.parametrize("mode", ["float", "deterministic"])
def test_the_order_is_left_alone(mode):
    """4. a species in tile order keeps its order, its partition and its sort count through both calls, every particle
    goes through its tile's LDS window, and the sums are the oracle's."""
    _, _, _, ref_h, ref_rho = deck()
    e, sp = build_state("tile", 4, mode)
    tpart, sorts = e.get_tile_partition(sp), e.species_stats(sp)["sorts"]
    for what in ("hydro", "rho"):
        got = hydro_of(e, sp) if what == "hydro" else rho_of(e, sp)
        assert e.species_order(sp) == "tile", what
        assert np.array_equal(e.get_tile_partition(sp), tpart) and e.species_stats(sp)["sorts"] == sorts, what
        assert e.moments_stats() == (N, N, 0, 0), what
        assert_close(got, ref_h if what == "hydro" else ref_rho, f"{mode} {what} by tile")
    e.close()


def test_particles_outside_their_tiles_window():
    """5. a periodic box, zero fields, ux = 3 and half a cell per step: after six pushes without a sort the particles are
    three cells from where the sort left them; some are still inside their tile's window, the others add through global
    memory.  The deterministic bits equal those of the same particles uploaded afresh in another order."""
    V = package()
    L = V.layout
    dt = 0.5 / (3.0 / np.sqrt(10.0))                         # v dt = half a cell (unit cells, c = 1)
    g, og = grids(V, L, dt=dt, periodic=True)
    p = np.array(deck()[2])
    p["ux"] = 3.0
    e = new_engine(V, g, True)
    e.set_vacuum(); e.load_interpolator()
    e.set_accumulation("deterministic")
    sp = e.new_species(-1.0, N + 4096, 4096)
    e.set_particles(sp, p)
    e.sort_p(sp)
    assert e.species_order(sp) == "tile"
    e.clear_accumulators()
    for _ in range(6):
        e.advance_p(sp)
    assert e.species_order(sp) == "tile" and e.nm(sp) == 0
    det, stats = hydro_of(e, sp), e.moments_stats()
    print("statistics after six pushes:", stats)
    assert stats[1] > 0 and stats[2] > 0 and stats[1] + stats[2] == N and stats[0] == N and stats[3] == 0
    e.set_accumulation("float")
    flt = hydro_of(e, sp)
    assert e.moments_stats()[:3] == stats[:3] and e.species_order(sp) == "tile"
    now = e.get_particles(sp)
    e.close()
    assert len(now) == N
    ref = reference(now, -1.0, np.zeros(og.nv, L.interpolator_t), periodic=True)[0]
    assert_close(det, ref, "deterministic, drifted")
    assert_close(flt, ref, "float, drifted")
    e = new_engine(V, g, False)
    e.set_vacuum(); e.load_interpolator()
    e.set_accumulation("deterministic")
    sp = e.new_species(-1.0, N + 4096, 4096)
    e.set_particles(sp, now[np.random.default_rng(6).permutation(N)])
    again = hydro_of(e, sp)
    assert e.moments_stats() == (N, 0, N, 0)
    e.close()
    assert np.array_equal(hydro_bits(det), hydro_bits(again))


def test_range():
    """6. |u| = 2^12 converts; one particle at 2^40 makes the deterministic call fail with an error that names the range,
    leaves nothing behind in the fixed-point words, and is accepted in float mode as before."""
    V = package()
    L = V.layout
    f, fi, p, _, _ = deck()
    g, _ = grids(V, L)
    e = new_engine(V, g, True)
    e.set_fields(np.array(f)); e.set_interpolator(np.array(fi))
    e.set_accumulation("deterministic")
    fast, sane = e.new_species(-1.0, N + 4096, 4096), e.new_species(-1.0, N + 4096, 4096)
    q = np.array(p)
    q["ux"] = 4096.0
    e.set_particles(fast, q)
    e.set_particles(sane, np.array(p))
    e.sort_p(fast)
    assert_close(hydro_of(e, fast), reference(q, -1.0, fi)[0], "ux = 2^12")
    assert e.moments_stats() == (N, N, 0, 0)
    one = q[:1].copy()
    one["ux"], one["tag"] = 2.0 ** 40, 10 ** 8
    e.append_particles(fast, one)
    e.clear_hydro()
    rc = e._l.vpic_hip_accumulate_hydro_p(e._h, fast)
    assert rc != 0
    assert "range" in e._l.vpic_hip_last_error().decode()
    with pytest.raises(V.VpicHipError, match="range"):
        e.accumulate_hydro_p(fast)
    stats = e.moments_stats()
    print("statistics of the refused call:", stats)
    assert stats[3] >= 1 and stats[0] == N + 1
    assert np.array_equal(hydro_bits(hydro_of(e, sane)), baseline_bits())     # nothing of the refused calls is left
    e.set_accumulation("float")
    h = hydro_of(e, fast)                                     # float mode takes the particle, as it always did
    assert e.moments_stats()[3] == 0 and np.isfinite(h["rho"]).all()
    e.close()


@pytest.mark.parametrize("mode", ["float", "deterministic"])
def test_small_and_empty_species(mode):
    """7. no particle, one particle, and a chargeless species (rho adds nothing, hydro sums what the oracle sums)."""
    V = package()
    L = V.layout
    f, fi, p, _, _ = deck()
    g, og = grids(V, L)
    for tile_knob in (False, True):
        e = new_engine(V, g, tile_knob)
        e.set_fields(np.array(f)); e.set_interpolator(np.array(fi))
        e.set_accumulation(mode, 0.01)
        empty, single, ghost = (e.new_species(-1.0, 4096, 64) for _ in range(3))
        assert not hydro_bits(hydro_of(e, empty)).any() and e.moments_stats() == (0, 0, 0, 0)
        assert not rho_of(e, empty).any() and e.moments_stats() == (0, 0, 0, 0)
        one = np.array(p[1234:1235])
        e.set_particles(single, one)
        if tile_knob:
            e.sort_p(single)
        ref_h, ref_rho = reference(one, -1.0, fi)
        assert_close(hydro_of(e, single), ref_h, "one particle")
        assert e.moments_stats() == ((1, 1, 0, 0) if tile_knob else (1, 0, 1, 0))
        assert_close(rho_of(e, single), ref_rho, "one particle")
        z = np.array(p[:500])
        z["q"] = 0
        e.set_particles(ghost, z)
        if tile_knob:
            e.sort_p(ghost)
        assert_close(hydro_of(e, ghost), reference(z, -1.0, fi)[0], "chargeless")
        assert e.moments_stats()[0] == 500
        assert not rho_of(e, ghost).any()
        e.close()


def test_rounding_bound():
    """8. the distance of the deterministic sums from the exact ones, derived: a node collects from the particles of its 8
    cells (8 x 24 here), each contribution rounded to the fixed-point grid by half a quantum 2^-(e + 1) at the most (e: the
    base-2 logarithm of the moment's scale, printed by the CPU driver of policy.h).  That stays below a quarter of ACC_TOL
    of the moment's largest oracle entry."""
    from test_moments_policy import build_driver, moment_scale_exponents
    _, _, p, ref_h, _ = deck()
    assert np.bincount(p["i"]).max() == PPC
    with tempfile.TemporaryDirectory() as tmp:
        exps = moment_scale_exponents(build_driver(tmp), np.abs(p["q"]).max(), -1.0, 0.125, 1.0)
    for c, ex in zip(moments(ref_h), exps):
        worst, top = 8 * PPC * 2.0 ** -(ex + 1), float(np.abs(ref_h[c]).max())
        print(f"{c}: scale 2^{ex}, worst rounding per node {worst:.3e}, largest entry {top:.3e}, ratio {worst / top:.2e}")
        assert worst < 0.25 * ACC_TOL * top, c


if __name__ == "__main__":
    child(sys.argv[1], sys.argv[2])
    print("child OK")
