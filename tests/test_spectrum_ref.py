"""The energy spectra of a species (include/vpic_hip.h: vpic_hip_energy_spectrum / vpic_hip_energy_bands), restated in
float64 numpy: what the GPU tests hold the kernels to.  Checked here, without a GPU, on a handful of hand-made
particles that sit on every branch of the binning; plus the C side of the new ABI (the header as C11, the struct's
size, the symbol list)."""
import importlib
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def kinetic_energy(u):
    """ke = sqrt(((1 + ux^2) + uy^2) + uz^2) - 1: the float32 momenta promoted, every operation in float64."""
    u = np.asarray(u, np.float32).astype(np.float64)
    return np.sqrt(((1.0 + u[:, 0] * u[:, 0]) + u[:, 1] * u[:, 1]) + u[:, 2] * u[:, 2]) - 1.0


def coordinates(u, params):
    """(ke / d_lin, (log10(ke) - log_lo) / d_log + 1): the two numbers whose truncation is the band and the bin."""
    ke = kinetic_energy(u)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = ke / params["d_lin"] if params.get("n_lin", 0) > 0 else np.zeros_like(ke)
        x = (np.log10(ke) - params["log_lo"]) / params["d_log"] + 1.0 if params.get("n_log", 0) > 0 else np.full_like(ke, -np.inf)
    return q, x


def spectrum_ref(u, i, nv, params):
    """(lin_counts[n_lin, nv] uint32, log_counts[n_log] uint64) of the particles with i >= 0."""
    u, i = np.asarray(u, np.float32), np.asarray(i, np.int64)
    live = i >= 0
    u, i = u[live], i[live]
    n_lin, n_log = params.get("n_lin", 0), params.get("n_log", 0)
    q, x = coordinates(u, params)
    lin = np.zeros((n_lin, nv), np.uint32)
    log = np.zeros(n_log, np.uint64)
    if n_lin > 0:
        band = np.minimum(np.trunc(q), n_lin - 1).astype(np.int64)        # everything beyond the last edge: the last band
        np.add.at(lin, (band, i), 1)
    if n_log > 0:
        ok = (x > -1.0) & (x < n_log)                                     # truncation toward zero: bin 0 takes (-1, 1)
        k = np.trunc(x[ok]).astype(np.int64)
        log += np.bincount(k, minlength=n_log).astype(np.uint64)
    return lin, log


def bands_ref(counts, grid):
    """float32[n_lin, nv]: every voxel's counts over their sum (0 where the sum is 0), one correctly rounded double
    division rounded once to float; then every ghost voxel takes the bands of the interior voxel that clamping each
    index into [1, n] gives."""
    nx, ny, nz = grid
    c = np.asarray(counts, np.uint32).astype(np.float64)
    tot = c.sum(axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        b = np.where(tot > 0, c / tot, 0.0).astype(np.float32)
    b = b.reshape(len(c), nz + 2, ny + 2, nx + 2)
    xs, ys, zs = (np.clip(np.arange(n + 2), 1, n) for n in (nx, ny, nz))
    return np.ascontiguousarray(b[:, zs][:, :, ys][:, :, :, xs]).reshape(len(c), -1)


def voxel(x, y, z, grid):
    nx, ny, nz = grid
    return x + (nx + 2) * (y + (ny + 2) * z)


def spec_inputs(seed, n, vth, grid=(12, 10, 9)):
    """Thermal momenta with a hot 2 % (sigma 2.0), voxels uniform over the interior of a grid whose tiles are partial
    on every axis: (u float32[n, 3], i int32[n])."""
    rng = np.random.default_rng(seed)
    u = (rng.standard_normal((n, 3)) * vth).astype(np.float32)
    hot = rng.random(n) < 0.02
    u[hot] = (rng.standard_normal((int(hot.sum()), 3)) * 2.0).astype(np.float32)
    nx, ny, nz = grid
    i = voxel(rng.integers(1, nx + 1, n), rng.integers(1, ny + 1, n), rng.integers(1, nz + 1, n), grid).astype(np.int32)
    return u, i


def deck_params(vth, nex=6, emax=300, nbin=800):
    """The production deck's binning constants, mixed float / double as the deck computes them."""
    return dict(n_lin=nex, d_lin=emax * (vth * vth / 2.0) / nex, n_log=nbin,
                log_lo=float(np.log10(np.float32(1e-4))), d_log=float(np.float32(8.0 / 800)))


def edge_distance(v):
    """relative distance of every coordinate to the nearest integer (where the device's log10 and the host's could
    legitimately round apart)"""
    v = v[np.isfinite(v)]
    return np.abs(v - np.round(v)) / np.maximum(np.abs(v), 1.0)


def test_handmade_particles_take_every_branch():
    grid = (3, 2, 1)
    nv = 5 * 4 * 3
    prm = dict(n_lin=4, d_lin=0.25, n_log=10, log_lo=-4.0, d_log=0.01)
    u = np.array([[1.0, 0.5, 0.0],          # 0: gam2 = 2.25 exactly, ke = 0.5: ke / d_lin == 2.0, band 2
                  [3.0, 0.0, 0.0],          # 1: ke = sqrt(10) - 1, far beyond the last edge: band 3
                  [0.0139, 0.0, 0.0],       # 2: log coordinate in (-1, 0): truncates to bin 0
                  [0.005, 0.0, 0.0],        # 3: log coordinate below -1: no bin
                  [0.0, 0.0, 0.0],          # 4: ke == 0: band 0, no bin
                  [1.0, 1.0, 1.0],          # 5: a dead slot
                  [0.01422, 0.0, 0.0]],     # 6: log coordinate in (1, 2): bin 1
                 np.float32)
    i = np.array([voxel(1, 1, 1, grid), voxel(3, 2, 1, grid), voxel(2, 1, 1, grid), voxel(2, 1, 1, grid),
                  voxel(1, 1, 1, grid), -1, voxel(2, 2, 1, grid)], np.int32)
    q, x = coordinates(u, prm)
    assert q[0] == 2.0 and q[1] > 4.0
    assert -1.0 < x[2] < 0.0 and x[3] < -1.0 and x[4] == -np.inf and 1.0 < x[6] < 2.0
    lin, log = spectrum_ref(u, i, nv, prm)
    assert lin.dtype == np.uint32 and lin.shape == (4, nv) and log.dtype == np.uint64 and log.shape == (10,)
    want = np.zeros((4, nv), np.uint32)
    want[2, i[0]] = 1
    want[3, i[1]] = 1
    want[0, i[2]] = 2                       # particles 2 and 3
    want[0, i[4]] = 1
    want[0, i[6]] = 1
    assert np.array_equal(lin, want)
    assert lin.sum() == 6                   # the dead slot is in no band
    assert log[0] == 1 and log[1] == 1 and log.sum() == 2
    # log-only and linear-only calls give the same parts
    assert np.array_equal(spectrum_ref(u, i, nv, dict(prm, n_lin=0))[1], log)
    assert np.array_equal(spectrum_ref(u, i, nv, dict(prm, n_log=0))[0], lin)


def test_bands_ref_normalises_and_fills_ghosts():
    grid = (3, 2, 1)
    nx, ny, nz = grid
    nv = 5 * 4 * 3
    counts = np.zeros((3, nv), np.uint32)
    counts[:, voxel(1, 1, 1, grid)] = (1, 2, 0)
    counts[:, voxel(3, 2, 1, grid)] = (0, 0, 7)
    counts[:, voxel(2, 1, 1, grid)] = (1, 1, 1)
    b = bands_ref(counts, grid)
    assert b.dtype == np.float32 and b.shape == (3, nv)
    third = np.float32(1.0 / 3.0)
    assert list(b[:, voxel(1, 1, 1, grid)]) == [third, np.float32(2.0 / 3.0), 0]
    assert list(b[:, voxel(2, 2, 1, grid)]) == [0, 0, 0]                    # an empty interior voxel stays 0
    # ghosts: the corner (0, 0, 0) and the face voxel (0, 1, 2) copy (1, 1, 1) (one cell along z: both z ghosts do);
    # the far corner copies (3, 2, 1)
    for g in (voxel(0, 0, 0, grid), voxel(0, 1, 2, grid), voxel(1, 0, 0, grid)):
        assert np.array_equal(b[:, g], b[:, voxel(1, 1, 1, grid)])
    assert list(b[:, voxel(nx + 1, ny + 1, nz + 1, grid)]) == [0, 0, 1]
    assert np.array_equal(b[:, voxel(2, 0, 2, grid)], np.full(3, third))


def test_generated_inputs_take_every_branch():
    """The populations the GPU test relies on (a change of the inputs must not quietly drop one), and how far the
    inputs stay from every edge."""
    for vth, want in ((0.05, (79, 2147, 7746)), (0.3, None)):
        u, i = spec_inputs(20261016, 400000, vth)
        prm = deck_params(vth)
        q, x = coordinates(u, prm)
        got = (int(((x > -1) & (x < 0)).sum()), int((x <= -1).sum()), int((q >= prm["n_lin"] - 1).sum()))
        if want:
            assert got == want
        assert edge_distance(q).min() > 1e-9 and edge_distance(x).min() > 1e-9
        assert i.min() > 0 and len(np.unique(i)) == 12 * 10 * 9


def test_header_compiles_as_c11_and_struct_size(tmp_path):
    src = ('#include "vpic_hip.h"\n_Static_assert(sizeof(vpic_hip_spectrum_t) == 32, "size");\n'
           'int main(void){ vpic_hip_spectrum_t s = {6, 800, 0.5, -4.0, 0.01}; return s.n_lin == 6 && sizeof(s) == 32 ? 0 : 1; }\n')
    exe = str(tmp_path / "spectrum_hdr_test")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-x", "c", "-", "-o", exe],
                   input=src.encode(), check=True)
    subprocess.check_call([exe])
    eng = importlib.import_module("old-vpic_amd.engine")
    import ctypes as C
    assert C.sizeof(eng.SpectrumParams) == 32


def test_symbols_are_listed():
    lib_mod = importlib.import_module("old-vpic_amd._lib")
    for name in ("vpic_hip_energy_spectrum", "vpic_hip_energy_bands", "vpic_hip_energy_spectrum_stats"):
        assert name in lib_mod.EXPORTS, name
