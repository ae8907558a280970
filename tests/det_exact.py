"""What tests/test_det_ref.py (CPU) and tests/test_gpu_det_exact.py (GPU) share: the inputs of one push and the exact
reference of the engine's deterministic accumulation (include/vpic_hip.h: vpic_hip_set_accumulation) -- the oracle's push
with its fixed-point switch on (oracle/vpic_oracle.h: orc_set_fixed_accumulator; pyorc.fixed_accumulator, finalize)."""
import importlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from oracle import pyorc  # noqa: E402

L = importlib.import_module("old-vpic_amd.layout")

REFLECT, ABSORB = L.REFLECT_PARTICLES, L.ABSORB_PARTICLES
# particle walls, faces -x -y -z +x +y +z (0: this same domain, periodic)
WALLS = {
    "periodic": [0, 0, 0, 0, 0, 0],
    "reflect": [REFLECT] * 6,
    "absorb_x_reflect_z": [ABSORB, 0, REFLECT, ABSORB, 0, REFLECT],
    "reflect_y_absorb_z": [0, REFLECT, ABSORB, 0, REFLECT, ABSORB],
}
Q_M = -1.0
Q0 = 0.01            # the reference charge of the cases (q_ref); charges are Q0 * U(0.5, 1.5) unless a case says otherwise
DT = 0.95            # cells of size 1, c = 1: a particle at |v| -> c moves 0.95 of a cell per step, on every axis at once
COLD, HOT = 0.02, 1.0   # momentum spreads: hardly any particle leaves its cell / more than a third do


def grids(dims, walls, dt=DT):
    """(engine grid arguments, keywords, oracle grid) of a box of unit cells with the particle walls of WALLS[walls] (or
    walls itself, six codes)"""
    nx, ny, nz = dims
    kw = dict(pbc=list(WALLS[walls] if isinstance(walls, str) else walls))
    args = (nx, ny, nz, float(nx), float(ny), float(nz), np.float32(dt))
    return args, kw, pyorc.make_grid(*args, **kw)


def interpolator(og, seed=7):
    """A random interpolator of the size tests/golden/kernels.npz's K2 uses: E, cB ~ N(0, 1) on the mesh, loaded, times
    0.05.  Ghost voxels stay zero (no particle sits in one)."""
    rng = np.random.default_rng(seed)
    f = np.zeros(og.nv, L.field_t)
    for c in ("ex", "ey", "ez", "cbx", "cby", "cbz"):
        f[c] = rng.standard_normal(og.nv).astype(np.float32)
    fi = np.zeros(og.nv, L.interpolator_t)
    pyorc.load_interpolator(fi, f, og)
    for c in fi.dtype.names:
        if not c.startswith("_"):
            fi[c] *= np.float32(0.05)
    return fi


def particles(seed, n, dims, u_scale, q0=-Q0, first_tag=1, cells=None):
    """n particles uniform over the interior cells (or over `cells`, voxel indices), momenta N(0, u_scale) per axis,
    charges q0 * U(0.5, 1.5), tags first_tag .. first_tag + n - 1, in random array order"""
    nx, ny, nz = dims
    rng = np.random.default_rng(seed)
    p = np.zeros(n, L.particle_t)
    for c in ("dx", "dy", "dz"):
        p[c] = rng.uniform(-1, 1, n).astype(np.float32)
    if cells is None:
        p["i"] = L.voxel(rng.integers(1, nx + 1, n), rng.integers(1, ny + 1, n), rng.integers(1, nz + 1, n), nx, ny, nz)
    else:
        p["i"] = np.asarray(cells)[rng.integers(0, len(cells), n)]
    for c in ("ux", "uy", "uz"):
        p[c] = (u_scale * rng.standard_normal(n)).astype(np.float32)
    p["q"] = (q0 * rng.uniform(0.5, 1.5, n)).astype(np.float32)
    p["tag"] = np.arange(n) + first_tag
    return p


class Pushed:
    """One oracle push of a copy of p: p (in array order), pm[:nm], the float accumulator a, and the exact sums a64[nv, 12]
    with streaks[nv]"""

    def __init__(self, og, p, fi, scale, q_m=Q_M, a64=None, streaks=None):
        self.p = p.copy()
        self.pm = np.zeros(len(p) + 1, L.particle_mover_t)
        self.a = np.zeros(og.nv + 1, L.accumulator_t)
        with pyorc.fixed_accumulator(og, scale) as (self.a64, self.streaks):
            self.nm = pyorc.advance_p(self.p, len(p), q_m, self.pm, self.a, fi, og)
        self.pm = self.pm[:self.nm]
        if a64 is not None:                                  # a second species into the same sums
            self.a64 += a64
            self.streaks += streaks

    def movers_by_tag(self):
        """(tags, movers) sorted by the particle's tag"""
        tags = self.p["tag"][self.pm["i"]]
        order = np.argsort(tags, kind="stable")
        return tags[order], self.pm[order]


def by_tag(p):
    return p[np.argsort(p["tag"], kind="stable")]


def describe_bad_words(got, a64, streaks, scale, dims, limit=6):
    """None when the float accumulator `got` (accumulator_t[nv]) is, as uint32 words, finalize(a64, scale); else a
    message naming the first bad words: voxel, (x, y, z), component, streaks, the expected integer, the difference in
    quanta."""
    nx, ny, nz = dims
    want = pyorc.finalize(a64, scale)
    g32 = np.ascontiguousarray(got[:len(want)]).view(np.uint32).reshape(-1, 12)
    w32 = want.view(np.uint32).reshape(-1, 12)
    bad = np.argwhere(g32 != w32)
    if len(bad) == 0:
        return None
    gf = np.ascontiguousarray(got[:len(want)]).view(np.float32).reshape(-1, 12)
    lines = ["%d of %d accumulator words differ from the exact sums" % (len(bad), g32.size)]
    for v, k in bad[:limit]:
        x, y, z = v % (nx + 2), (v // (nx + 2)) % (ny + 2), v // ((nx + 2) * (ny + 2))
        lines.append("voxel %d (%d, %d, %d) %s[%d]: streaks %d, expected integer %d (float bits %08x, got %08x), off by %.3f quanta"
                     % (v, x, y, z, ("jx", "jy", "jz")[k // 4], k % 4, streaks[v], a64[v, k], w32[v, k], g32[v, k],
                        float(gf[v, k]) * scale - float(a64[v, k])))
    return "\n".join(lines)
