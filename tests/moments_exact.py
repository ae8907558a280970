"""What tests/test_moments_exact_ref.py (CPU) and tests/test_gpu_moments_exact.py (GPU) share: the decks and the exact
reference of accumulate_hydro_p / accumulate_rho_p, per node and moment -- the oracle's two functions with their
fixed-point switch on (oracle/vpic_oracle.h: orc_set_fixed_moments; pyorc.fixed_moments, finalize_moments).

Deterministic mode (include/vpic_hip.h: vpic_hip_set_accumulation): every contribution is rounded to a 64-bit integer at a
power-of-two scale and summed as an integer, and each sum is rounded once into the float array, so an order-free CPU
computation predicts every word: Reference.hydro_words / rho_words.

Float mode: the same floats are summed in some order, in some tree.  Against R = sum / scale of the integer reference
(n contributions at the node, A = sum of |integers| / scale, q = 1 / scale, u = 2^-24, gamma_n = n u / (1 - n u)):

    |got - R| <= gamma_n (A + n q / 2) + n q / 2 + ulp32(R) / 2

 - a float sum of n terms c_i in any order or tree is within gamma_(n-1) sum |c_i| of their exact sum (Higham, Accuracy and
   Stability of Numerical Algorithms, section 4.2); sum |c_i| <= A + n q / 2, since each integer is within half a quantum
   of c_i scale;
 - for the same reason the exact sum is within n q / 2 of R;
 - ulp32(R) / 2 for one more rounding of the result (a partial sum added to an array that is not empty).
Nothing in it is measured.  A node without contributions must hold exactly zero."""
import functools
import importlib
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import det_exact as D  # noqa: E402
from det_exact import L, pyorc  # noqa: E402
from test_moments_policy import build_driver, moment_scale_exponents  # noqa: E402

MOMENTS = L.hydro_t.names[:14]
assert MOMENTS == ("jx", "jy", "jz", "rho", "px", "py", "pz", "ke", "txx", "tyy", "tzz", "tyz", "tzx", "txy")
Q0 = D.Q0                      # the reference charge every case hands to set_accumulation; charges are +-Q0 U(0.5, 1.5) or 0
Q_MS = (-1.0, 1.0 / 25.0)      # q_m = 1/25: mc_q = 25 c shifts the scales of moments 4 to 13 (and is no float)
DT = 0.02
U_SCALES = (1e-6, 0.3, 30.0)
U = 2.0 ** -24

# name: (cells, lengths, cvac).  unit: cells of size 1, c = 1
GRIDS = {
    "10x9x7": ((10, 9, 7), None, 1.0),                        # partial tiles on every axis
    "4x4x4": ((4, 4, 4), None, 1.0),                          # exactly one tile
    "5x3x2": ((5, 3, 2), None, 1.0),                          # thinner than a tile
    "16x1x6": ((16, 1, 6), None, 1.0),                        # thinner than a tile
    "65x5x4": ((65, 5, 4), None, 1.0),                        # 17 tiles along x
    "10x9x7-stretched": ((10, 9, 7), (13.0, 4.5, 21.7), 2.0),  # r8V, c and every frexp off the powers of two
}
THIN = ("5x3x2", "16x1x6")
# particles per grid: above 4 nv (the float path "cells"), at most 16 000; SPARSE: below 4 nv (the per-particle float path)
N_PARTICLES = {"10x9x7": 8000, "4x4x4": 3000, "5x3x2": 2000, "16x1x6": 3000, "65x5x4": 16000, "10x9x7-stretched": 8000}
N_SPARSE = 900


def dims_of(grid):
    return GRIDS[grid][0]


def nv_of(grid):
    nx, ny, nz = dims_of(grid)
    return (nx + 2) * (ny + 2) * (nz + 2)


def grid_args(grid, dt=DT, fbc=None, pbc=None):
    """(arguments, keywords) of make_grid, the engine's and the oracle's alike"""
    (nx, ny, nz), lengths, cvac = GRIDS[grid]
    lx, ly, lz = lengths or (float(nx), float(ny), float(nz))
    kw = dict(cvac=cvac)
    if fbc is not None:
        kw["fbc"] = list(fbc)
    if pbc is not None:
        kw["pbc"] = list(pbc)
    return (nx, ny, nz, lx, ly, lz, np.float32(dt)), kw


def oracle_grid(grid, dt=DT, fbc=None, pbc=None):
    args, kw = grid_args(grid, dt, fbc, pbc)
    return pyorc.make_grid(*args, **kw)


@functools.lru_cache(maxsize=None)
def interpolator(grid, seed=7):
    """det_exact.interpolator of the grid (random E and cB through the oracle's load_interpolator), computed once"""
    fi = D.interpolator(oracle_grid(grid), seed)
    fi.setflags(write=False)
    return fi


def particles(seed, n, grid, first_tag=1, cells=None):
    """det_exact.particles, then: momenta from three scales (1e-6, 0.3, 30, a third of the particles each), charge signs
    mixed inside the species (node sums cancel), about 2 % with q = 0, and about 2 % each with dx, dy, dz exactly -1, 0 or
    +1 (zero weights: nothing may appear on the far node)"""
    p = D.particles(seed, n, dims_of(grid), 1.0, q0=Q0, first_tag=first_tag, cells=cells)
    rng = np.random.default_rng(seed + 1000)
    scale = np.array(U_SCALES, np.float32)[rng.integers(0, 3, n)]
    for c in ("ux", "uy", "uz"):
        p[c] *= scale
    p["q"] *= rng.choice(np.array([-1.0, 1.0], np.float32), n)
    p["q"][rng.random(n) < 0.02] = 0
    for c in ("dx", "dy", "dz"):
        edge = rng.random(n) < 0.02
        p[c][edge] = rng.choice(np.array([-1.0, 0.0, 1.0], np.float32), int(edge.sum()))
    return p


def one_per_odd_cell(seed, grid):
    """one particle of particles() in every cell whose three cell coordinates are all odd: no two share a node"""
    nx, ny, nz = dims_of(grid)
    x, y, z = np.meshgrid(np.arange(1, nx + 1, 2), np.arange(1, ny + 1, 2), np.arange(1, nz + 1, 2), indexing="ij")
    cells = L.voxel(x.ravel(), y.ravel(), z.ravel(), nx, ny, nz)
    p = particles(seed, len(cells), grid)
    p["i"] = cells
    return p


def q_max_of(p):
    """Species::q_max of a species the host has put exactly p into"""
    return float(np.abs(p["q"]).max()) if len(p) else 0.0


# ---- the scales ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _driver():
    """the CPU driver of policy.h (tests/moments_policy_check.cpp), built once per process"""
    _driver.tmp = tempfile.TemporaryDirectory()
    return build_driver(_driver.tmp.name)


def r8V_of(og):
    """r8V as the engine (and the reference) forms it: the product in double, stored as a float"""
    return float(np.float32(0.125 * float(og.rdx) * float(og.rdy) * float(og.rdz)))


@functools.lru_cache(maxsize=None)
def _hydro_scales(q_max, q_m, r8V, c):
    return tuple(2.0 ** ex for ex in moment_scale_exponents(_driver(), q_max, q_m, r8V, c))


def hydro_scales(q_max, q_m, og):
    """the 14 scales policy.h: moment_scales chooses for a species whose largest |q| ever uploaded is q_max (falling back
    on the reference charge when there is none), taken from the header itself through its CPU driver"""
    return np.array(_hydro_scales(float(np.float32(q_max)) if q_max > 0 else Q0, float(np.float32(q_m)), r8V_of(og), float(og.cvac)))


def rho_scale(og, q_ref=Q0):
    """the accumulator's scale moved to where a weight of 8 r8V |q| lands (moments.hip: k_accumulate_rho_p)"""
    import math
    return pyorc.fixed_scale(q_ref) * 2.0 ** -math.frexp(8.0 * r8V_of(og))[1]


# ---- the reference --------------------------------------------------------------------------------------------------------
class Reference:
    """The oracle's accumulate_hydro_p and accumulate_rho_p of the rows p with the switch on: m (pyorc.FixedMoments: h64,
    habs64, count, r64, rabs64, rcount, skipped, scales, rho_scale) and the oracle's own float results h, rhof.  q_max: the
    charge the hydro scales follow (default: the largest |q| of p)."""

    def __init__(self, og, p, q_m, fi, q_max=None, q_ref=Q0):
        p = np.array(p)
        self.og, self.n = og, len(p)
        self.h = np.zeros(og.nv, L.hydro_t)
        f = np.zeros(og.nv, L.field_t)
        scales = hydro_scales(q_max_of(p) if q_max is None else q_max, q_m, og)
        with pyorc.fixed_moments(og, scales, rho_scale(og, q_ref)) as self.m:
            pyorc.accumulate_hydro_p(self.h, p, len(p), q_m, np.array(fi), og)
            pyorc.accumulate_rho_p(f, p, len(p), og)
        self.rhof = f["rhof"].copy()
        assert not self.m.skipped.any(), "the deck leaves the fixed-point range"

    def hydro_words(self, prev=None):
        """hydro_t[nv] a deterministic call leaves in prev (default: a cleared array)"""
        return pyorc.finalize_moments(np.zeros(self.og.nv, L.hydro_t) if prev is None else prev, self.m.h64, self.m.scales)

    def rho_words(self, prev=None):
        return pyorc.finalize_moments(np.zeros(self.og.nv, np.float32) if prev is None else prev, self.m.r64, [self.m.rho_scale])


def float_view(a):
    """float32[nv, 14] of a hydro_t array, float32[nv, 1] of a rhof array"""
    a = np.ascontiguousarray(a)
    return a.view(np.float32).reshape(len(a), -1)[:, :14]


def _parts(refs, rho):
    for r in refs:
        m = r.m
        if rho:
            yield m.r64[:, None], m.rabs64[:, None], m.rcount, np.array([m.rho_scale])
        else:
            yield m.h64, m.habs64, m.count, m.scales


def float_bound(refs, rho=False):
    """(R, bound, n) per node and moment of the float sums of the contributions of refs (References added into one array
    without a clear in between): the module's docstring, with A, n q and n summed over the references."""
    R = A = nq = n = 0
    for s64, abs64, count, scales in _parts(refs, rho):
        inv = 1.0 / scales
        R = R + s64.astype(np.float64) * inv
        A = A + abs64.astype(np.float64) * inv
        nq = nq + count[:, None].astype(np.float64) * inv
        n = n + count.astype(np.int64)
    nn = n[:, None].astype(np.float64)
    gamma = nn * U / (1.0 - nn * U)
    ulp = np.spacing(np.abs(R).astype(np.float32)).astype(np.float64)
    return R, gamma * (A + 0.5 * nq) + 0.5 * nq + 0.5 * ulp, n


def float_errors(got, refs, rho=False):
    """(worst error / bound, words compared, message or None) of a float-mode result against float_bound(refs): every word
    of every node is compared; a node without contributions must hold zero bits"""
    g = float_view(got)
    R, bound, n = float_bound(refs, rho)
    assert g.shape == R.shape
    err = np.abs(g.astype(np.float64) - R)
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(n[:, None] > 0, err / bound, 0.0)
    empty_bad = (n[:, None] == 0) & (g.view(np.uint32) != 0)
    bad = np.argwhere((err > bound) | ~np.isfinite(g) | empty_bad)
    msg = None
    if len(bad):
        nx, ny, _ = (refs[0].og.nx, refs[0].og.ny, refs[0].og.nz)
        lines = ["%d of %d words are outside the float bound" % (len(bad), g.size)]
        for v, k in bad[:6]:
            lines.append("voxel %d (%d, %d, %d) %s: %d contributions, got %.9g, reference %.17g, error %.3e, bound %.3e"
                         % (v, v % (nx + 2), (v // (nx + 2)) % (ny + 2), v // ((nx + 2) * (ny + 2)),
                            "rhof" if rho else MOMENTS[k], n[v], g[v, k], R[v, k], err[v, k], bound[v, k]))
        msg = "\n".join(lines)
    return float(ratio.max()), int(g.size), msg


def describe_bad_words(got, want, refs, rho=False, limit=6):
    """None when `got` (hydro_t[nv], or float32[nv] of rhof) equals `want` (Reference.hydro_words / rho_words, chained
    over refs) in every uint32 word, ghosts included; else a message naming the first bad words: voxel, (x, y, z), moment,
    contributions at the node, the expected integer (of the last of refs), got / expected float bits, the difference in
    quanta of that reference's scale."""
    g, w = float_view(got), float_view(want)
    assert g.shape == w.shape
    g32, w32 = g.view(np.uint32), w.view(np.uint32)
    bad = np.argwhere(g32 != w32)
    if len(bad) == 0:
        return None
    og = refs[-1].og
    nx, ny = og.nx, og.ny
    s64, _, count, scales = list(_parts(refs, rho))[-1]
    n = sum(c for _, _, c, _ in _parts(refs, rho))
    lines = ["%d of %d words differ from the exact sums" % (len(bad), g32.size)]
    for v, k in bad[:limit]:
        lines.append("voxel %d (%d, %d, %d) %s: %d contributions, expected integer %d at scale 2^%d (float bits %08x, got %08x), off by %.3f quanta"
                     % (v, v % (nx + 2), (v // (nx + 2)) % (ny + 2), v // ((nx + 2) * (ny + 2)), "rhof" if rho else MOMENTS[k],
                        n[v], s64[v, k], int(np.log2(scales[k])), w32[v, k], g32[v, k],
                        (float(g[v, k]) - float(w[v, k])) * scales[k]))
    return "\n".join(lines)
