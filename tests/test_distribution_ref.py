"""The phase-space distributions of a species (include/vpic_hip.h: vpic_hip_species_distribution), restated in float64
numpy: what the GPU tests hold the kernel to.  Checked here, without a GPU, on hand-made particles that sit on every
branch of the rules, and on the generated inputs of tests/test_gpu_distribution.py (which must populate what that test
relies on, and stay away from every edge that a log10 is compared with); plus the C side of the new ABI (the header as
C11, the struct's size, the symbol list).

Every correctly rounded operation (+, -, x, /, sqrt) agrees bit for bit between numpy and the device; only log10 may
differ by an ulp.  So every descriptor with a LOG10_KE axis or range is held to a margin (log_margin): no particle's
bin coordinate within 1e-9 (relative) of an integer, no selected value within 1e-9 of a range end.  The first seed
tried (20261017) satisfies it.  The other coordinates need no margin and get none."""
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

from test_spectrum_ref import spec_inputs, voxel  # noqa: E402

COORDS = ("x", "y", "z", "ux", "uy", "uz", "ke", "log10_ke")

SEED, N, GRID, VTH = 20261017, 560000, (96, 8, 6), 0.05


def particle_dtype():
    return importlib.import_module("old-vpic_amd.layout").particle_t


def coordinate(p, grid, name):
    """float64 values of one coordinate for every particle of p (a particle_t array), as the header states them."""
    nx, ny, nz = grid
    if name in ("x", "y", "z"):
        i = p["i"].astype(np.int64)
        sy, sz = nx + 2, (nx + 2) * (ny + 2)
        cell = {"x": i % sy, "y": (i // sy) % (ny + 2), "z": i // sz}[name]
        return (cell - 1).astype(np.float64) + (p["d" + name].astype(np.float64) + 1.0) * 0.5
    if name in ("ux", "uy", "uz"):
        return p[name].astype(np.float64)
    ux, uy, uz = (p[c].astype(np.float64) for c in ("ux", "uy", "uz"))
    ke = np.sqrt(((1.0 + ux * ux) + uy * uy) + uz * uz) - 1.0
    if name == "ke":
        return ke
    assert name == "log10_ke"
    with np.errstate(divide="ignore"):
        return np.log10(ke)


def distribution_ref(p, grid, desc, stats=False):
    """uint64 counts, shape (n0,) or (n1, n0), of the particles of p under desc = dict(axes=[(coord, lo, d, n), ...],
    select=[(coord, lo, hi), ...]); with stats, also (live particles seen, kept by the selection, counted)."""
    nx, ny, nz = grid
    nv = (nx + 2) * (ny + 2) * (nz + 2)
    p = p[(p["i"] >= 0) & (p["i"] < nv)]                        # dead slots are skipped
    seen = len(p)
    keep = np.ones(len(p), bool)
    for coord, lo, hi in desc.get("select", ()):
        c = coordinate(p, grid, coord)
        keep &= (c >= lo) & (c < hi)
    p = p[keep]
    ok = np.ones(len(p), bool)
    ts = []
    for coord, lo, d, n in desc["axes"]:
        with np.errstate(invalid="ignore"):
            t = (coordinate(p, grid, coord) - lo) / d
            ok &= (t >= 0) & (t < n)                            # (a NaN is never counted)
        ts.append(t)
    bins = [np.trunc(t[ok]).astype(np.int64) for t in ts]
    n0 = desc["axes"][0][3]
    if len(bins) == 1:
        counts = np.bincount(bins[0], minlength=n0).astype(np.uint64)
    else:
        n1 = desc["axes"][1][3]
        counts = np.bincount(bins[1] * n0 + bins[0], minlength=n0 * n1).astype(np.uint64).reshape(n1, n0)
    return (counts, (seen, len(p), int(ok.sum()))) if stats else counts


def log_margin(p, grid, desc):
    """The smallest relative distance, over the live particles, of a LOG10_KE bin coordinate to an integer and of a
    LOG10_KE value to an end of a range on it (inf for a descriptor without LOG10_KE): where the device's log10 and
    numpy's could legitimately round a particle to different sides."""
    p = p[p["i"] >= 0]
    worst = np.inf
    for coord, lo, d, n in desc["axes"]:
        if coord == "log10_ke":
            t = (coordinate(p, grid, coord) - lo) / d
            t = t[np.isfinite(t)]
            worst = min(worst, float((np.abs(t - np.round(t)) / np.maximum(np.abs(t), 1.0)).min()))
    for coord, lo, hi in desc.get("select", ()):
        if coord == "log10_ke":
            c = coordinate(p, grid, coord)
            c = c[np.isfinite(c)]
            for end in (lo, hi):
                if np.isfinite(end):
                    worst = min(worst, float((np.abs(c - end) / max(abs(end), 1.0)).min()))
    return worst


def dist_inputs(seed, n, vth, grid, spread=1.0):
    """particle_t[n]: momenta and voxels of test_spectrum_ref.spec_inputs, offsets uniform in (-spread, spread)."""
    u, i = spec_inputs(seed, n, vth, grid)
    p = np.zeros(n, particle_dtype())
    p["i"] = i
    p["ux"], p["uy"], p["uz"] = u[:, 0], u[:, 1], u[:, 2]
    off = np.random.default_rng(seed + 1000).uniform(-1.0, 1.0, (n, 3)).astype(np.float32)
    off = np.clip(off, np.float32(-0.9999999), np.float32(0.9999999)) * np.float32(spread)     # (a float32 rounded up to 1 is not inside)
    p["dx"], p["dy"], p["dz"] = off[:, 0], off[:, 1], off[:, 2]
    p["q"] = -0.01
    return p


def descriptors(vth=VTH, lds_bins=8192):
    """The descriptors of the GPU test, by name; lds_bins: VPIC_HIP_DIST_LDS_BINS, which (b), (e) and (f) must exceed.
    On GRID = 96 x 8 x 6:
      a  1-D ux, 512 bins: the whole histogram in LDS
      b  x-ux, x bins one cell wide, 96 x 128 bins: the sliding window
      c  ux-uz, 64 x 48, of the particles with 1.5 <= Z < 4.25 and KE >= vth^2 / 2
      d  1-D LOG10_KE, 800 bins from 1e-4 to 10^0.8
      e  ux-uy, 128 x 128: no position axis, global adds
      f  ux-x with the position axis second and its bins 1.25 cells wide from -0.37: the window again, bins not on cells
      g  y-LOG10_KE (60 bins from -2.8 to -1.3) of the particles with -3 <= LOG10_KE < -1, 10 <= X < 50.5 and -1 <= uy < 1 (Y, and a log10 range)"""
    w = 3.0 * vth
    d = {
        "a": dict(axes=[("ux", -w, 2 * w / 512, 512)]),
        "b": dict(axes=[("x", 0.0, 1.0, 96), ("ux", -w, 2 * w / 128, 128)]),
        "c": dict(axes=[("ux", -w, 2 * w / 64, 64), ("uz", -w, 2 * w / 48, 48)],
                  select=[("z", 1.5, 4.25), ("ke", 0.5 * vth * vth, np.inf)]),
        "d": dict(axes=[("log10_ke", -4.0, 0.006, 800)]),
        "e": dict(axes=[("ux", -w, 2 * w / 128, 128), ("uy", -w, 2 * w / 128, 128)]),
        "f": dict(axes=[("ux", -w, 2 * w / 128, 128), ("x", -0.37, 1.25, 80)]),
        "g": dict(axes=[("y", 0.0, 0.5, 16), ("log10_ke", -2.8, 0.025, 60)],
                  select=[("log10_ke", -3.0, -1.0), ("x", 10.0, 50.5), ("uy", -1.0, 1.0)]),
    }
    for name in "bef":
        assert np.prod([a[3] for a in d[name]["axes"]]) > lds_bins
    for name in "acdg":
        assert np.prod([a[3] for a in d[name]["axes"]]) <= lds_bins
    return d


# ---- hand-made particles ----
HAND_GRID = (3, 2, 1)


def handmade():
    g = HAND_GRID
    rows = [  # voxel,           dx,   dy,   dz,    ux,     uy,  uz
        (voxel(1, 1, 1, g), -1.0, 0.0, 0.5, 1.0, 0.5, 0.0),        # 0: X = 0 exactly, Y = 0.5, Z = 0.75; ke = 0.5 exactly
        (voxel(3, 2, 1, g), 1.0, -0.5, 0.0, -0.25, 0.0, 0.25),     # 1: X = 3 = nx exactly, Y = 1.25, Z = 0.5; ke = sqrt(1.125) - 1
        (voxel(2, 1, 1, g), 0.0, 0.5, -1.0, 0.0, 0.0, 0.0),        # 2: X = 1.5, Y = 0.75, Z = 0; ke = 0, log10 = -inf
        (-1, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0),                        # 3: a dead slot
        (voxel(0, 1, 1, g), 0.5, 0.0, 0.0, 0.5, 0.0, 0.0),         # 4: a ghost voxel of the low x face: X = -0.25, Y = 0.5, Z = 0.5
        (voxel(2, 2, 1, g), 0.5, 0.0, 0.0, 3.0, 0.0, 0.75),        # 5: X = 1.75, Y = 1.5, Z = 0.5; gamma = 3.25, ke = 2.25 exactly
        (voxel(1, 2, 1, g), 0.0, 0.0, 0.0, 0.0139, 0.0, 0.0),      # 6: X = 0.5, Y = 1.5, Z = 0.5; ke = 9.66e-5, log10 = -4.015
    ]
    p = np.zeros(len(rows), particle_dtype())
    for k, (i, dx, dy, dz, ux, uy, uz) in enumerate(rows):
        p[k]["i"], p[k]["dx"], p[k]["dy"], p[k]["dz"], p[k]["ux"], p[k]["uy"], p[k]["uz"] = i, dx, dy, dz, ux, uy, uz
    return p


def test_handmade_coordinates():
    p, g = handmade(), HAND_GRID
    live = p["i"] >= 0
    x, y, z = (coordinate(p, g, c) for c in "xyz")
    assert list(x[live]) == [0.0, 3.0, 1.5, -0.25, 1.75, 0.5]
    assert list(y[live]) == [0.5, 1.25, 0.75, 0.5, 1.5, 1.5]
    assert list(z[live]) == [0.75, 0.5, 0.0, 0.5, 0.5, 0.5]
    ke, lg = coordinate(p, g, "ke"), coordinate(p, g, "log10_ke")
    assert ke[0] == 0.5 and ke[2] == 0.0 and ke[5] == 2.25 and lg[2] == -np.inf
    assert 9.6e-5 < ke[6] < 9.7e-5 and -4.02 < lg[6] < -4.01


def test_handmade_particles_take_every_branch():
    p, g = handmade(), HAND_GRID
    inf = np.inf

    def check(desc, want, want_stats):
        got, stats = distribution_ref(p, g, desc, stats=True)
        want = np.array(want, np.uint64)
        assert got.dtype == np.uint64 and got.shape == want.shape
        assert np.array_equal(got, want), (desc, got)
        assert stats == want_stats and int(got.sum()) == stats[2]

    # X: particle 0 sits exactly on lo (bin 0), particle 1 exactly on lo + n * d (not counted), the ghost's X is below
    check(dict(axes=[("x", 0.0, 0.75, 4)]), [2, 0, 2, 0], (6, 6, 4))
    # UX: particle 1 exactly on lo, particle 5 above the range
    check(dict(axes=[("ux", -0.25, 0.5, 3)]), [3, 1, 1], (6, 6, 5))
    # Y x Z, counts[bz][by]; the ghost of the x face has Y and Z inside and counts
    want = np.zeros((4, 4), np.uint64)
    want[3, 1] = 1          # particle 0: Y 0.5 -> 1, Z 0.75 -> 3
    want[2, 2] = 1          # particle 1: Y 1.25 -> 2, Z 0.5 -> 2
    want[0, 1] = 1          # particle 2: Y 0.75 -> 1, Z 0 -> 0 (on lo)
    want[2, 1] = 1          # particle 4
    want[2, 3] = 2          # particles 5 and 6
    check(dict(axes=[("y", 0.0, 0.5, 4), ("z", 0.0, 0.25, 4)]), want, (6, 6, 6))
    # UY under two selections: particles 1 (X == hi) and 4 (X < lo) fail the first only, particle 5 (uz = 0.75) the second only
    check(dict(axes=[("uy", -1.0, 1.0, 2)], select=[("x", 0.0, 3.0), ("uz", -0.5, 0.5)]), [0, 3], (6, 3, 3))
    # UZ
    check(dict(axes=[("uz", -1.0, 1.0, 2)]), [0, 6], (6, 6, 6))
    # KE: particle 2 (ke == 0) on lo, particle 5 (ke == 2.25) exactly on lo + n * d
    check(dict(axes=[("ke", 0.0, 0.25, 9)]), [4, 0, 1, 0, 0, 0, 0, 0, 0], (6, 6, 5))
    # LOG10_KE: ke == 0 gives -inf and no bin
    check(dict(axes=[("log10_ke", -5.0, 1.0, 6)]), [1, 0, 0, 1, 2, 1], (6, 6, 5))
    # a range on LOG10_KE with an infinite end, and one on KE: -inf is below every finite lo
    check(dict(axes=[("x", -1.0, 1.0, 5)], select=[("log10_ke", -4.5, inf)]), [1, 2, 1, 0, 1], (6, 5, 5))
    check(dict(axes=[("x", -1.0, 1.0, 5)], select=[("ke", 0.1, inf)]), [1, 1, 1, 0, 0], (6, 3, 3))


def test_generated_inputs_populate_what_the_gpu_test_relies_on():
    p = dist_inputs(SEED, N, VTH, GRID)
    nx, ny, nz = GRID
    for c in ("dx", "dy", "dz"):
        assert p[c].dtype == np.float32 and -1.0 < p[c].min() < -0.99 and 0.99 < p[c].max() < 1.0
    per_voxel = np.bincount(p["i"])
    per_voxel = per_voxel[per_voxel > 0]
    assert len(per_voxel) == nx * ny * nz and per_voxel.min() >= 64        # the header's rule for zero misses
    tail = dist_inputs(SEED + 1, 5000, VTH, GRID)
    for name, desc in descriptors().items():
        counts, (seen, kept, counted) = distribution_ref(p, GRID, desc, stats=True)
        margin = min(log_margin(p, GRID, desc), log_margin(tail, GRID, desc))
        below = above = 0
        kept_p = p
        for coord, lo, hi in desc.get("select", ()):
            c = coordinate(kept_p, GRID, coord)
            kept_p = kept_p[(c >= lo) & (c < hi)]
        for coord, lo, d, n in desc["axes"]:
            c = coordinate(kept_p, GRID, coord)
            below += int((c < lo).sum())
            above += int((c >= lo + n * d).sum())
        print(f"({name}) seen {seen} kept {kept} counted {counted}, below {below} above {above}, "
              f"non-empty {np.count_nonzero(counts)} of {counts.size}, log margin {margin:.3g}")
        assert seen == N and int(counts.sum()) == counted
        assert below > 0 and above > 0                                     # out of range on both sides
        assert np.count_nonzero(counts) > counts.size // 2
        if "select" in desc:
            assert 0.02 * N < kept < 0.6 * N                               # a selection that selects
        else:
            assert kept == N
        if any(c[0] == "log10_ke" for c in desc["axes"] + desc.get("select", [])):
            assert margin > 1e-9                                           # nobody is left out of the GPU comparison
        else:
            assert margin == np.inf


def test_header_compiles_as_c11_and_struct_size(tmp_path):
    src = ('#include "vpic_hip.h"\n_Static_assert(sizeof(vpic_hip_dist_t) == 152, "size");\n'
           '_Static_assert(VPIC_HIP_COORD_LOG10_KE == 7 && VPIC_HIP_DIST_MAX_BINS == 4194304 && VPIC_HIP_DIST_LDS_BINS > 0, "constants");\n'
           'int main(void){ vpic_hip_dist_t d = {1, 0, {{VPIC_HIP_COORD_UX, 8, -1.0, 0.25}}, {{0}}};\n'
           '  int64_t out[4]; (void)out; return d.axis[0].n == 8 && sizeof(d.axis[0]) == 24 && sizeof(d.sel[0]) == 24 ? 0 : 1; }\n')
    exe = str(tmp_path / "dist_hdr_test")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-x", "c", "-", "-o", exe],
                   input=src.encode(), check=True)
    subprocess.check_call([exe])
    eng = importlib.import_module("old-vpic_amd.engine")
    assert C.sizeof(eng.DistDesc) == 152 and C.sizeof(eng.DistAxis) == 24 and C.sizeof(eng.DistRange) == 24
    assert eng.DistDesc.axis.offset == 8 and eng.DistDesc.sel.offset == 56
    assert tuple(sorted(eng.DIST_COORDS, key=eng.DIST_COORDS.get)) == COORDS
    # the two constants of the Python side are the header's
    text = open(os.path.join(ROOT, "include", "vpic_hip.h")).read()
    assert f"#define VPIC_HIP_DIST_LDS_BINS {eng.DIST_LDS_BINS}\n" in text and eng.DIST_MAX_BINS == 1 << 22
    d = eng.dist_desc([("x", 0.0, 1.0, 96), ("ux", -1.0, 0.5, 4)], [("ke", 0.5, 2.0)])
    assert (d.n_axes, d.n_sel, d.axis[1].coord, d.axis[1].n, d.axis[1].d, d.sel[0].coord, d.sel[0].hi) == (2, 1, 3, 4, 0.5, 6, 2.0)


def test_symbols_are_listed():
    lib_mod = importlib.import_module("old-vpic_amd._lib")
    for name in ("vpic_hip_species_distribution", "vpic_hip_species_distribution_stats"):
        assert name in lib_mod.EXPORTS, name
    eng = importlib.import_module("old-vpic_amd.engine")
    assert callable(eng.Engine.distribution) and callable(eng.Engine.distribution_stats)
