"""Radiative cooling of a species (include/vpic_hip.h: vpic_hip_species_cool): the numpy restatement of THE RULE
(tests/cool_ref.py) checked without a GPU -- on the cases whose answer is known beforehand (u along B, the E x B drift,
the photon bath alone, the rate of convergence against an RK4 solution), on the tally (its sign without E, its balance
against sum |q| (gamma - 1)), on hand-made particles that sit on every branch, and on the generated inputs of
tests/test_gpu_cool.py, which must populate what that test relies on; plus the C side of the new ABI (the header as C11,
the struct's size, the symbol list).  The GPU test compares the device with this restatement with ==, word for word."""
import ctypes as C
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

import cool_ref as R  # noqa: E402
from test_distribution_ref import HAND_GRID, particle_dtype  # noqa: E402
from test_select_ref import fields_ref, interpolator_dtype, random_interpolator  # noqa: E402
from test_spectrum_ref import voxel  # noqa: E402

# ---- the generated inputs of the GPU test ----
GRIDS = [(5, 3, 4), (9, 6, 5)]          # the second: larger than a tile (4 cells) in every axis and a multiple of none
N_GPU = 3000
SYNC, IC = 1e-2, 1e-3
# |q| = 0.01 and gamma - gamma' below gamma <= 31: |val| < 0.31 < 2^32 * 2^-33; a slow particle that E speeds up by
# sync * |A| ~ 0.05 changes its energy by ~1e-5, many quanta
QUANTUM = 2.0 ** -33
E_NAMES = ("ex", "dexdy", "dexdz", "d2exdydz", "ey", "deydz", "deydx", "d2eydzdx", "ez", "dezdx", "dezdy", "d2ezdxdy")


def n_voxels(grid):
    nx, ny, nz = grid
    return (nx + 2) * (ny + 2) * (nz + 2)


def cool_particles(seed, n, grid, spread=1.0):
    """particle_t[n]: |u| log-uniform in [1e-3, 30] in random directions, interior voxels and offsets uniform, q = -0.01,
    tags 1 .. n"""
    nx, ny, nz = grid
    rng = np.random.default_rng(seed)
    p = np.zeros(n, particle_dtype())
    mag = 10.0 ** rng.uniform(-3.0, np.log10(30.0), n)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    u = (mag[:, None] * d).astype(np.float32)
    p["ux"], p["uy"], p["uz"] = u[:, 0], u[:, 1], u[:, 2]
    p["i"] = voxel(rng.integers(1, nx + 1, n), rng.integers(1, ny + 1, n), rng.integers(1, nz + 1, n), grid)
    off = np.clip(rng.uniform(-1.0, 1.0, (n, 3)).astype(np.float32), np.float32(-0.9999999), np.float32(0.9999999)) * np.float32(spread)
    p["dx"], p["dy"], p["dz"] = off[:, 0], off[:, 1], off[:, 2]
    p["q"] = -0.01
    p["tag"] = np.arange(n) + 1
    return p


def cool_interpolator(seed, grid):
    """test_select_ref.random_interpolator with E about half of cB (halving a float32 is exact)"""
    fi = random_interpolator(seed, grid)
    for name in E_NAMES:
        fi[name] = fi[name] * np.float32(0.5)
    return fi


def guard_voxels(grid):
    """(the voxel that gets a NaN word, the voxel that gets an inf word): two interior voxels"""
    return int(voxel(2, 1, 1, grid)), int(voxel(1, 2, 1, grid))


def plant_guards(fi, grid):
    """a copy of fi with a NaN in one word of one voxel's record and an inf in one word of another's"""
    out = fi.copy()
    v_nan, v_inf = guard_voxels(grid)
    out["dezdy"][v_nan] = np.nan
    out["cby"][v_inf] = -np.inf
    return out


# ---- the C side ----
def test_header_compiles_as_c11_and_struct_size(tmp_path):
    src = ('#include "vpic_hip.h"\n_Static_assert(sizeof(vpic_hip_cool_t) == 32, "size");\n'
           '_Static_assert(VPIC_HIP_COOL_DRY == 1, "flag");\n'
           'int main(void){ vpic_hip_cool_t c = {1e-2, 1e-3, 0.5, VPIC_HIP_COOL_DRY, 0};\n'
           '  int (*f)(vpic_hip_engine_t *, int, const vpic_hip_cool_t *, int64_t *, int64_t *) = 0;\n'
           '  int (*t)(vpic_hip_engine_t *, int64_t *) = 0;\n'
           '  __typeof__(&vpic_hip_species_cool) f2 = f; __typeof__(&vpic_hip_species_cool_stats) t2 = t;\n'
           '  printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(c), offsetof(vpic_hip_cool_t, sync), offsetof(vpic_hip_cool_t, ic),\n'
           '         offsetof(vpic_hip_cool_t, quantum), offsetof(vpic_hip_cool_t, flags), offsetof(vpic_hip_cool_t, pad));\n'
           '  return !f2 && !t2 && c.quantum == 0.5 && c.flags == 1 ? 0 : 1; }\n')
    exe = str(tmp_path / "cool_hdr_test")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-x", "c", "-", "-o", exe],
                   input=("#include <stdio.h>\n#include <stddef.h>\n" + src).encode(), check=True)
    compiler = [int(w) for w in subprocess.check_output([exe]).split()]
    # the ctypes mirror (old-vpic_amd/cool.py) against the compiler: the size and every member's offset
    eng = importlib.import_module("old-vpic_amd.engine")
    D = eng.CoolDesc
    assert [name for name, _ in D._fields_] == ["sync", "ic", "quantum", "flags", "pad"]
    assert [C.sizeof(D), D.sync.offset, D.ic.offset, D.quantum.offset, D.flags.offset, D.pad.offset] == compiler == [32, 0, 8, 16, 24, 28]
    assert eng.COOL_DRY == 1


def test_symbols_are_listed():
    lib_mod = importlib.import_module("old-vpic_amd._lib")
    for name in ("vpic_hip_species_cool", "vpic_hip_species_cool_stats"):
        assert name in lib_mod.EXPORTS, name
    res, args = lib_mod.SIGNATURES["vpic_hip.h"]["vpic_hip_species_cool"]
    assert res is C.c_int and args == [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    eng = importlib.import_module("old-vpic_amd.engine")
    assert callable(eng.Engine.cool) and callable(eng.Engine.cool_stats)
    assert eng.CoolResult._fields == ("isum", "energy", "cell_isums", "stats")


# ---- cases whose answer is known beforehand ----
def one(u, e, b, sync, ic, quantum=2.0 ** -40, q=-0.01):
    """the rule on particles given by rows of u, with the same E and cB at every one"""
    u = np.atleast_2d(np.asarray(u, np.float32))
    f = np.tile(np.asarray(list(e) + list(b), np.float32), (len(u), 1))
    new, val, ok = R.cool_fields(f, u, np.full(len(u), q, np.float32), sync, ic, quantum)
    addend, refused = R.tally(val, ok, quantum)
    return new, val, ok, addend, refused


def test_u_along_b_is_untouched():
    for mag in (1e-3, 0.1, 1.0, 10.0, 30.0):
        for axis, b in ((2, (0.0, 0.0, 2.5)), (0, (-0.75, 0.0, 0.0))):
            u = np.zeros((1, 3), np.float32)
            u[0, axis] = mag
            new, val, ok, addend, refused = one(u, (0, 0, 0), b, sync=0.3, ic=0.0)
            assert ok.all() and not refused.any()
            assert new.view(np.uint32).tolist() == u.view(np.uint32).tolist(), mag      # every word
            assert addend.tolist() == [0] and val.tolist() == [0.0], mag


def test_exb_drift_is_untouched():
    """E = (0, .5, 0), cB = (0, 0, 1): the drift velocity is E x B / B^2 = (.5, 0, 0), u = gamma v.  E + v x cB vanishes up
    to the float rounding of u, 1e-8: sync * A is far below half an ulp of u."""
    v = 0.5
    u = np.array([[v / np.sqrt(1.0 - v * v), 0.0, 0.0]], np.float32)
    new, val, ok, addend, _ = one(u, (0.0, 0.5, 0.0), (0.0, 0.0, 1.0), sync=0.1, ic=0.0)
    assert ok.all() and new.view(np.uint32).tolist() == u.view(np.uint32).tolist()
    assert addend.tolist() == [0] and val.tolist() == [0.0]


def test_ic_alone():
    grid = GRIDS[0]
    p, fi = cool_particles(3, 2000, grid), cool_interpolator(4, grid)
    ic = 0.05
    ref = R.cool_ref(p, fi, 0.0, ic, QUANTUM)
    u = np.stack([p["ux"], p["uy"], p["uz"]], axis=1).astype(np.float64)
    g = np.sqrt(1.0 + ((u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1]) + u[:, 2] * u[:, 2]))
    want = (u / (1.0 + g * ic)[:, None]).astype(np.float32)
    assert ref.u.view(np.uint32).tolist() == want.view(np.uint32).tolist()
    assert ref.stats == dict(seen=2000, changed=int(ref.changed.sum()), refused=0, left_alone=0) and ref.changed.mean() > 0.99
    assert np.all(ref.val >= 0) and ref.isum > 0


def test_first_order_convergence():
    """u = (10, 0, 0) in cB = (0, 0, 1), E = 0, carried in double through 50, 100, 200, 400 calls that cover sync * calls =
    0.1, against an RK4 solution of du/dt = -k u sqrt(1 + u^2) (v x B is perpendicular to both: |u| alone changes)."""
    u0, total = 10.0, 0.1

    def f(u):
        return -u * np.sqrt(1.0 + u * u)
    u, n = u0, 20000
    h = total / n
    for _ in range(n):
        k1 = f(u); k2 = f(u + 0.5 * h * k1); k3 = f(u + 0.5 * h * k2); k4 = f(u + h * k3)
        u += h * (k1 + 2 * k2 + 2 * k3 + k4) / 6
    exact = u
    z, o = np.zeros(1), np.ones(1)
    errs = []
    for calls in (50, 100, 200, 400):
        x = (np.array([u0]), z.copy(), z.copy())
        for _ in range(calls):
            x, _, ok = R.cool_double(z, z, z, z, z, o, x[0], x[1], x[2], np.float64(total / calls), np.float64(0.0))
            assert ok.all()
        assert x[1][0] == 0.0 and x[2][0] == 0.0
        errs.append(float(x[0][0]) - exact)
    ratios = [errs[k] / errs[k + 1] for k in range(3)]
    print("errors", errs, "ratios", ratios)
    assert all(1.8 <= r <= 2.2 for r in ratios), ratios


# ---- the tally ----
def test_without_e_the_tally_is_never_below_float_rounding():
    """E = 0: the drag only takes.  Only the rounding of u' to float can make a val negative: val >= -2^-23 u2 / g per
    unit |q| (a relative 2^-24 per component on u2, over g + g1 >= g)."""
    n = 200000
    rng = np.random.default_rng(1)
    p = cool_particles(11, n, GRIDS[1])
    u = np.stack([p["ux"], p["uy"], p["uz"]], axis=1)
    f = np.zeros((n, 6), np.float32)
    f[:, 3:] = rng.normal(size=(n, 3)).astype(np.float32)
    q = np.ones(n, np.float32)
    new, val, ok = R.cool_fields(f, u, q, 1e-2, 0.0, 1.0)
    assert ok.all()
    u64 = u.astype(np.float64)
    u2 = (u64[:, 0] * u64[:, 0] + u64[:, 1] * u64[:, 1]) + u64[:, 2] * u64[:, 2]
    bound = -(2.0 ** -23) * u2 / np.sqrt(1.0 + u2)
    print("smallest val", val.min(), "smallest val - bound", (val - bound).min())
    assert np.all(val >= bound)


def test_tally_balances_the_kinetic_energy():
    """sum |q| (gamma - 1) before minus after == isum * quantum within half a quantum per particle plus the double
    rounding of the sums: each of the 3 n terms (two energies and a val per particle) is formed in at most 8 roundings
    and numpy's pairwise sums add log2(n) more, all relative to at most K_before + K_after."""
    for grid in GRIDS:
        p, fi = cool_particles(5, 20000, grid), cool_interpolator(6, grid)
        ref = R.cool_ref(p, fi, SYNC, IC, QUANTUM)
        before, after = R.kinetic(p), R.kinetic(R.apply_ref(p, ref))
        n = len(p)
        assert ref.stats["refused"] == 0 and ref.stats["left_alone"] == 0
        slack = n * QUANTUM / 2 + (8 + np.log2(n)) * 2.0 ** -53 * (before + after)
        print(grid, "before - after", before - after, "isum * quantum", ref.isum * QUANTUM, "slack", slack)
        assert abs((before - after) - ref.isum * QUANTUM) <= slack
        assert ref.cell_isums.sum() == ref.isum and ref.isum > 0


# ---- hand-made particles, one for each branch ----
def search_chi_negative():
    """(E float32[3], u float32[3]) with u = 2^30 E -- exactly along E, cB = 0, gamma ~ 1e9: chi = E^2 / gamma^2 is below
    the rounding of its two terms -- for which L2 - vE*vE < 0, the first of a million seeded candidates; None when there
    is none (the test asserts there is)"""
    rng = np.random.default_rng(7)
    for _ in range(10):
        e = rng.uniform(0.5, 2.0, (100000, 3)).astype(np.float32)
        u = e * np.float32(2.0 ** 30)                                          # (a power of two: exact)
        f = np.zeros((len(e), 6), np.float32)
        f[:, :3] = e
        hit = np.flatnonzero(R.chi_raw(f, u) < 0.0)
        if len(hit):
            return e[hit[0]], u[hit[0]]
    return None


V_PLAIN, V_NAN, V_INF, V_CHI = (voxel(1, 1, 1, HAND_GRID), voxel(2, 1, 1, HAND_GRID), voxel(3, 1, 1, HAND_GRID),
                                voxel(1, 2, 1, HAND_GRID))
V_GHOST = voxel(0, 1, 1, HAND_GRID)


def hand_interpolator():
    """all zero but for: V_PLAIN cB = (0, 0, 1), ey = 0.25; V_NAN the same with d2exdydz a NaN; V_INF the same with cbx
    +inf; V_CHI E = what search_chi_negative found; V_GHOST cby = 1 + 2 dy"""
    fi = np.zeros(n_voxels(HAND_GRID), interpolator_dtype())
    for v in (V_PLAIN, V_NAN, V_INF):
        fi["cbz"][v], fi["ey"][v] = 1.0, 0.25
    fi["d2exdydz"][V_NAN] = np.nan
    fi["cbx"][V_INF] = np.inf
    found = search_chi_negative()
    if found is not None:
        fi["ex"][V_CHI], fi["ey"][V_CHI], fi["ez"][V_CHI] = found[0]
    fi["cby"][V_GHOST], fi["dcbydy"][V_GHOST] = 1.0, 2.0
    return fi


def handmade_cool():
    """0: plain; 1: in the NaN voxel; 2: in the inf voxel; 3: a dead slot; 4: a ghost voxel, u across its B; 5: chi clamped;
    6: i == nv, not live"""
    rows = [(V_PLAIN, 0.0, 0.0, 0.0, 2.0, 0.0, 0.0), (V_NAN, 0.5, 0.5, 0.5, 2.0, 0.0, 0.0), (V_INF, 0.0, 0.0, 0.0, 2.0, 0.0, 0.0),
            (-1, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0), (V_GHOST, 0.0, 0.5, 0.0, 3.0, 0.0, 0.0), (V_CHI, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0),
            (n_voxels(HAND_GRID), 0.0, 0.0, 0.0, 1.0, 0.0, 0.0)]
    p = np.zeros(len(rows), particle_dtype())
    for k, (i, dx, dy, dz, ux, uy, uz) in enumerate(rows):
        p[k]["i"], p[k]["dx"], p[k]["dy"], p[k]["dz"], p[k]["ux"], p[k]["uy"], p[k]["uz"] = i, dx, dy, dz, ux, uy, uz
    found = search_chi_negative()
    if found is not None:
        p[5]["ux"], p[5]["uy"], p[5]["uz"] = found[1]
    p["q"] = -0.01
    p["tag"] = np.arange(len(p)) + 1
    return p


def test_a_clamped_chi_exists():
    found = search_chi_negative()
    assert found is not None
    f = np.zeros((1, 6), np.float32)
    f[0, :3] = found[0]
    raw = R.chi_raw(f, found[1][None, :])
    print("E", found[0], "u", found[1], "chi before the clamp", raw)
    assert raw[0] < 0.0


def test_handmade_particles_take_every_branch():
    p, fi = handmade_cool(), hand_interpolator()
    sync, ic, quantum = 0.05, 0.01, 2.0 ** -36
    live = p.copy()
    live["i"][[3, 6]] = V_PLAIN                                  # (fields_ref indexes the table: checked on stand-ins)
    assert np.isnan(fields_ref(live, fi)[1, 0]) and np.isinf(fields_ref(live, fi)[2, 3])
    ref = R.cool_ref(p, fi, sync, ic, quantum)
    assert ref.live.tolist() == [True, True, True, False, True, True, False]
    assert ref.alone.tolist() == [False, True, True, False, False, False, False]
    assert ref.stats == dict(seen=5, changed=3, refused=1, left_alone=2)
    # left alone, dead and not live: every word as it was, nothing tallied
    for k in (1, 2, 3, 6):
        assert ref.u[k].tobytes() == np.array([p[k]["ux"], p[k]["uy"], p[k]["uz"]], np.float32).tobytes() and ref.addend[k] == 0
    # 0, by hand: u = (2, 0, 0), g = sqrt 5, v = 2 / g; L = (0, .25 - v, 0); vE = 0; A = (Ly, 0, 0); chi = Ly^2
    g = np.sqrt(5.0)
    v = 2.0 * (1.0 / g)
    ly = 0.25 + (0.0 * 0.0 - v * 1.0)
    D = g * (sync * ((ly * ly + 0.0) + 0.0) + ic)
    want = np.float32((2.0 + sync * ((ly * 1.0 - 0.0 * 0.0) + 0.0 * 0.0)) / (1.0 + D))
    assert ref.u[0].tolist() == [float(want), 0.0, 0.0] and ref.addend[0] > 0
    # 4, the ghost voxel's own record: cB = (0, 2, 0) at dy = 0.5, E = 0: u = (3, 0, 0) across it loses, and keeps its direction
    assert ref.u[4, 0] < 3.0 and ref.u[4, 1] == 0.0 and ref.u[4, 2] == 0.0 and ref.addend[4] > 0
    assert ref.cell_isums[V_GHOST] == ref.addend[4]
    # 5, chi clamped to 0: D = g * ic exactly, and E along u pushes
    u5 = np.array([p[5]["ux"], p[5]["uy"], p[5]["uz"]], np.float64)
    g5 = np.sqrt(1.0 + ((u5[0] * u5[0] + u5[1] * u5[1]) + u5[2] * u5[2]))
    e5 = np.array([fi["ex"][V_CHI], fi["ey"][V_CHI], fi["ez"][V_CHI]], np.float64)
    rg = 1.0 / g5
    vE = ((u5[0] * rg) * e5[0] + (u5[1] * rg) * e5[1]) + (u5[2] * rg) * e5[2]
    want5 = ((u5 + sync * (vE * e5)) / (1.0 + g5 * (sync * 0.0 + ic))).astype(np.float32)
    assert ref.u[5].tobytes() == want5.tobytes()
    assert ref.refused[5] and ref.addend[5] == 0                 # (|q| gamma ~ 1e7: 1e18 quanta, far above 2^32)
    assert ref.isum == ref.addend[0] + ref.addend[4] == ref.cell_isums.sum()
    # a tiny quantum refuses every particle that loses anything, and still moves it
    tiny = R.cool_ref(p, fi, sync, ic, 1e-300)
    assert tiny.u.tobytes() == ref.u.tobytes() and tiny.isum == 0 and not tiny.cell_isums.any()
    assert tiny.stats == dict(seen=5, changed=3, refused=3, left_alone=2)


HAND_SYNC, HAND_QUANTUM = 0.05, 2.0 ** -36
HAND_ICS = (0.01, 0.0)           # without the photon bath the clamp decides particle 5's momentum (below)


def test_the_clamp_decides_a_float_word():
    """ic = 0: with chi clamped D is 0 and den is 1; without the clamp D = g sync chi ~ -3e-7 and u' moves by several float
    ulps.  The GPU test runs the hand-made particles with this ic, so a kernel without the clamp (or with another) fails it."""
    p, fi = handmade_cool(), hand_interpolator()
    ref = R.cool_ref(p, fi, HAND_SYNC, 0.0, HAND_QUANTUM)
    f = fields_ref(p[5:6], fi)
    u5 = np.array([[p[5]["ux"], p[5]["uy"], p[5]["uz"]]], np.float32)
    raw = R.chi_raw(f, u5)[0]
    assert raw < 0.0 and not ref.alone[5]
    u64 = u5.astype(np.float64)[0]
    g = np.sqrt(1.0 + ((u64[0] * u64[0] + u64[1] * u64[1]) + u64[2] * u64[2]))
    e = f[0, :3].astype(np.float64)
    rg = 1.0 / g
    vE = ((u64[0] * rg) * e[0] + (u64[1] * rg) * e[1]) + (u64[2] * rg) * e[2]
    top = u64 + HAND_SYNC * (vE * e)                                           # (cB = 0: A = vE E)
    clamped, unclamped = (top / (1.0 + g * (HAND_SYNC * 0.0 + 0.0))).astype(np.float32), (top / (1.0 + g * (HAND_SYNC * raw + 0.0))).astype(np.float32)
    assert ref.u[5].tobytes() == clamped.tobytes()
    assert np.all(clamped.view(np.uint32) != unclamped.view(np.uint32))
    print("particle 5: clamped", clamped, "unclamped", unclamped, "D without the clamp", g * HAND_SYNC * raw)


# ---- the generated inputs of the GPU test ----
def test_generated_inputs_populate_what_the_gpu_test_relies_on():
    for k, grid in enumerate(GRIDS):
        p, fi = cool_particles(20 + k, N_GPU, grid), cool_interpolator(30 + k, grid)
        assert set(np.unique(p["i"])) <= set(range(n_voxels(grid))) and len(np.unique(p["i"])) > 0.9 * grid[0] * grid[1] * grid[2]
        e = np.abs(np.stack([fi[n] for n in E_NAMES])).mean()
        b = np.abs(np.stack([fi[n] for n in ("cbx", "cby", "cbz", "dcbxdx", "dcbydy", "dcbzdz")])).mean()
        assert 0.45 < e / b < 0.55
        ref = R.cool_ref(p, fi, SYNC, IC, QUANTUM)
        print(grid, ref.stats, "isum", ref.isum, "negative addends", int((ref.addend < 0).sum()), "largest |t|",
              float(np.nanmax(np.abs(ref.val)) / QUANTUM))
        assert ref.stats["seen"] == N_GPU and ref.stats["changed"] >= 0.99 * N_GPU
        assert (ref.addend > 0).sum() > 100 and (ref.addend < 0).sum() > 100
        assert ref.stats["refused"] == 0 and ref.stats["left_alone"] == 0
        assert np.count_nonzero(ref.cell_isums) > 0.9 * grid[0] * grid[1] * grid[2]
        # ... and with the guards planted: both voxels hold particles, which are left alone, and only they
        v_nan, v_inf = guard_voxels(grid)
        planted = R.cool_ref(p, plant_guards(fi, grid), SYNC, IC, QUANTUM)
        in_guard = (p["i"] == v_nan) | (p["i"] == v_inf)
        assert (p["i"] == v_nan).sum() > 0 and (p["i"] == v_inf).sum() > 0
        assert planted.alone.tolist() == in_guard.tolist()
        assert planted.u[~in_guard].tobytes() == ref.u[~in_guard].tobytes()
        # a tiny quantum refuses all but the particles whose val is exactly 0
        tiny = R.cool_ref(p, fi, SYNC, IC, 1e-300)
        assert tiny.stats["refused"] >= 0.99 * N_GPU and tiny.u.tobytes() == ref.u.tobytes()
