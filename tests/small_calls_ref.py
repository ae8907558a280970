"""What tests/test_gpu_small_calls.py holds center_p / uncenter_p / energy_p / load_maxwellian to, without a GPU: the
generated particles and interpolator records those tests share, the float chain of energy_p restated in numpy float32
with its exact sum, and the rule of the synthetic loader restated draw for draw.  tests/test_small_calls_ref.py pins all
of it against the oracle and against what a Maxwellian is.

energy_p (push.hip: energy_p_kernel; the oracle's orc_energy_p): per particle, in float32 with every operation rounded once,
    v_a = u_a + qdt_2mc * ((e + d1 * de1) + d2 * (de2 + d1 * dde))          a = x, y, z
    w   = (vx * vx + vy * vy) + vz * vz;   w = w / (sqrt(1 + w) + 1)
    t   = (double)w * (double)q             -- exact: 24 x 24 bits
and E = c^2 * sum(t) / q_m.  Only the ORDER of the double sum differs between implementations; exact_sum() has none.

load_maxwellian (particles.hip: load_maxwellian_kernel): particle idx lies in interior cell idx // ppc, x fastest; draw k
of particle idx is unit_top_closed(mix(mix(idx * 9 + k) ^ mix(seed * 0x9e3779b9 + k))), all in uint32 (csrc/unit_draw.h);
offsets 2 u_k - 1 (k = 0, 1, 2) in float32; r1 = sqrt(-2 log u_3), a1 = 6.2831853f * u_4, r2 = sqrt(-2 log u_5),
a2 = 6.2831853f * u_6; u = drift + vth * (r1 cos a1, r1 sin a1, r2 cos a2)."""
import importlib
import math
import os
import sys
from fractions import Fraction

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from collide_ref import mix32  # noqa: E402
from test_spectrum_ref import voxel  # noqa: E402

N = 20000
U = 2.0 ** -53                         # one rounding of a double, relative
KINDS = ("zero", "weak", "strong", "e_only", "b_only", "tiny")      # a voxel's kind: KINDS[voxel % 6]
STRONG = 40.0                          # with qdt_4mc = 0.1 (q_m = -1, dt = 0.4): v2 = (qdt_4mc / gamma)^2 |cB|^2 up to 16 / gamma^2 and more
TINY = 1e-39                           # a subnormal float (the smallest normal one is 1.18e-38)
N_HAND = 12
E_NAMES = ("ex", "dexdy", "dexdz", "d2exdydz", "ey", "deydz", "deydx", "d2eydzdx", "ez", "dezdx", "dezdy", "d2ezdxdy")
B_NAMES = ("cbx", "dcbxdx", "cby", "dcbydy", "cbz", "dcbzdz")


def layout():
    return importlib.import_module("old-vpic_amd.layout")


def n_voxels(grid):
    nx, ny, nz = grid
    return (nx + 2) * (ny + 2) * (nz + 2)


def interior_voxels(grid):
    nx, ny, nz = grid
    z, y, x = np.meshgrid(np.arange(1, nz + 1), np.arange(1, ny + 1), np.arange(1, nx + 1), indexing="ij")
    return voxel(x, y, z, grid).reshape(-1).astype(np.int32)


def interpolator(seed, grid):
    """interpolator_t[nv], ghosts included; the kind of voxel v is KINDS[v % 6]: all zero, weak (about 1e-3), strong (up to
    STRONG), E only, B only (both of order 1), and tiny (subnormal words: every product with them is subnormal or zero)"""
    nv = n_voxels(grid)
    rng = np.random.default_rng(seed)
    fi = np.zeros(nv, layout().interpolator_t)
    kind = np.arange(nv) % len(KINDS)
    scale = np.array([0.0, 1e-3, STRONG, 1.0, 1.0, TINY])[kind]
    for name in E_NAMES + B_NAMES:
        v = rng.uniform(0.25, 1.0, nv) * rng.choice([-1.0, 1.0], nv) * scale
        if name in E_NAMES:
            v[kind == KINDS.index("b_only")] = 0.0
        else:
            v[kind == KINDS.index("e_only")] = 0.0
        fi[name] = v.astype(np.float32)
    return fi


def voxel_of_kind(grid, kind, which=0):
    """an interior voxel of that kind"""
    v = interior_voxels(grid)
    return int(v[v % len(KINDS) == KINDS.index(kind)][which])


def handmade(grid):
    """particle_t[N_HAND]: u = 0 in every kind of voxel that matters; one momentum component only; and, in a tiny voxel,
    momenta so small that the half kick qdt_2mc * E, the squares u * u and the rotation's products are subnormal floats"""
    p = np.zeros(N_HAND, layout().particle_t)
    rows = [
        # (kind, dx, dy, dz, ux, uy, uz, q)
        ("zero", 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0),
        ("strong", 0.25, -0.5, 1.0, 0.0, 0.0, 0.0, 0.5),
        ("e_only", -1.0, 1.0, 0.0, 0.0, 0.0, 0.0, -0.25),
        ("b_only", 1.0, -1.0, -1.0, 0.0, 0.0, 0.0, 0.125),
        ("strong", 0.5, 0.5, 0.5, 2.0, 0.0, 0.0, 0.01),
        ("b_only", -0.5, 0.0, 0.25, 0.0, -0.75, 0.0, -0.01),
        ("weak", 0.0, 0.75, -0.25, 0.0, 0.0, 30.0, 0.02),
        ("tiny", 0.5, -0.25, 0.75, 1e-20, -2e-20, 3e-20, 1.0),          # u * u = 1e-40 ...: subnormal
        ("tiny", -0.75, 0.5, 0.0, 3e-39, 0.0, 0.0, 0.5),                 # u itself subnormal
        ("tiny", 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, -1.0),                    # nothing but the subnormal half kick
        ("tiny", 1.0, 1.0, 1.0, 1e-3, 1e-3, -1e-3, 0.25),                # a normal u times subnormal fields
        ("zero", -1.0, -1.0, -1.0, 1e-20, 0.0, -1e-19, 0.0),
    ]
    assert len(rows) == N_HAND
    for k, (kind, dx, dy, dz, ux, uy, uz, q) in enumerate(rows):
        p[k] = (dx, dy, dz, voxel_of_kind(grid, kind, k % 2), ux, uy, uz, q, 0, 0)
    return p


def particles(seed, n, grid, spread=1.0, tag0=1):
    """particle_t[n], tags tag0 .. tag0 + n - 1: |u| log-uniform over 1e-3 .. 30 in isotropic directions; interior voxels;
    offsets uniform in [-1, 1], a handful exactly at +-1 and 0; weights |q| log-uniform over two decades, a fifth of them
    negative and some exactly 0; the last N_HAND (n permitting) are handmade().  spread scales every offset (a state that
    is built with a push keeps its particles in their cells that way)."""
    nx, ny, nz = grid
    rng = np.random.default_rng(seed)
    p = np.zeros(n, layout().particle_t)
    mag = 10.0 ** rng.uniform(-3.0, np.log10(30.0), n)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    u = (mag[:, None] * d).astype(np.float32)
    p["ux"], p["uy"], p["uz"] = u[:, 0], u[:, 1], u[:, 2]
    p["i"] = voxel(rng.integers(1, nx + 1, n), rng.integers(1, ny + 1, n), rng.integers(1, nz + 1, n), grid)
    off = rng.uniform(-1.0, 1.0, (n, 3)).astype(np.float32)
    for k, value in enumerate((1.0, -1.0, 0.0, 1.0, -1.0, 0.0, 1.0, -1.0, 0.0)):     # slots 0 .. 8: one axis each, thrice
        if k < n:
            off[k, k % 3] = value
    q = 10.0 ** rng.uniform(-3.0, -1.0, n) * np.where(rng.random(n) < 0.2, -1.0, 1.0)
    q[rng.random(n) < 0.01] = 0.0
    p["q"] = q.astype(np.float32)
    if n >= 4 * N_HAND:
        hand = handmade(grid)
        p[n - N_HAND:] = hand
        off[n - N_HAND:] = np.stack([hand["dx"], hand["dy"], hand["dz"]], axis=1)
    off *= np.float32(spread)
    p["dx"], p["dy"], p["dz"] = off[:, 0], off[:, 1], off[:, 2]
    p["tag"] = np.arange(n) + tag0
    return p


# ---- energy_p ----
def qdt_2mc(q_m, g):
    """the host constant of center_p, uncenter_p, energy_p and the push: double arithmetic on float inputs, stored as float"""
    return np.float32(0.5 * float(np.float32(q_m)) * float(np.float32(g.dt)) / float(np.float32(g.cvac)))


def energy_terms(p, fi, q_m, g):
    """float64[len(p)]: t_k = (double)w_k * (double)q_k, each exact, with w_k from the float32 chain in the module's docstring"""
    f = fi[p["i"]]
    k, one = qdt_2mc(q_m, g), np.float32(1.0)
    dx, dy, dz = p["dx"], p["dy"], p["dz"]
    assert dx.dtype == np.float32 and f["ex"].dtype == np.float32 and p["ux"].dtype == np.float32
    with np.errstate(under="ignore"):
        v0 = p["ux"] + k * ((f["ex"] + dy * f["dexdy"]) + dz * (f["dexdz"] + dy * f["d2exdydz"]))
        v1 = p["uy"] + k * ((f["ey"] + dz * f["deydz"]) + dx * (f["deydx"] + dz * f["d2eydzdx"]))
        v2 = p["uz"] + k * ((f["ez"] + dx * f["dezdx"]) + dy * (f["dezdy"] + dx * f["d2ezdxdy"]))
        w = (v0 * v0 + v1 * v1) + v2 * v2
        w = w / (np.sqrt(one + w) + one)
        assert w.dtype == np.float32
        return w.astype(np.float64) * p["q"].astype(np.float64)


def exact_sum(t):
    """the sum of the doubles t as a Fraction, exact: the 53-bit integers of the mantissas are added per exponent in two
    26-bit halves (each half's sum stays below 2^53 for fewer than 2^26 terms), the exponents are combined as integers"""
    t = np.ascontiguousarray(t, np.float64)
    assert len(t) < 1 << 26 and np.isfinite(t).all()
    m, ex = np.frexp(t)
    mi = np.ldexp(m, 53).astype(np.int64)                  # |mi| < 2^53, an integer: exact
    sign, mag = np.sign(mi), np.abs(mi)
    hi, lo = sign * (mag >> 26), sign * (mag & ((1 << 26) - 1))
    lo_ex = int(ex.min()) if len(t) else 0
    width = (int(ex.max()) - lo_ex + 1) if len(t) else 1
    # (bincount adds in float64: integers below 2^27 each, fewer than 2^26 of them -- every partial sum is exact)
    sums = [np.bincount(ex - lo_ex, weights=half.astype(np.float64), minlength=width) for half in (hi, lo)]
    total = 0
    for k in range(width):
        total += ((int(sums[0][k]) << 26) + int(sums[1][k])) << k
    return Fraction(total) * Fraction(2) ** (lo_ex - 53)


def energy_exact(t, q_m, g):
    """(c^2 * sum(t) / q_m as a Fraction: no rounding at all; sum |t_k| as a float, rounded once)"""
    c = Fraction(float(np.float32(g.cvac)))
    return c * c * exact_sum(t) / Fraction(float(np.float32(q_m))), math.fsum(np.abs(t))


def energy_scale(q_m, g):
    """c^2 / |q_m|: what a sum of t is multiplied with"""
    return float(np.float32(g.cvac)) ** 2 / abs(float(np.float32(q_m)))


def energy_bound(height, sabs, energy, q_m, g):
    """|computed - exact| for a sum of the t_k by any tree of that height (each t_k passes through at most `height`
    additions, each of which rounds once: the error is at most height * 2^-53 * sum |t_k| to first order), times
    c^2 / |q_m|, plus the two roundings of `c^2 * sum / q_m`"""
    return height * U * sabs * energy_scale(q_m, g) + 2 * U * abs(float(energy))


# ---- load_maxwellian ----
TWO_PI_F = np.float32(6.2831853)
K_LOG, K_TRIG = 2, 2                   # ulp: see loader_bound


def unit_top_closed(r):
    """csrc/unit_draw.h: ((float)(r >> 8) + 0.5f) * 2^-24, in float32 (the sum rounds to even from 2^23 on)"""
    x = (np.asarray(r, np.uint32) >> np.uint32(8)).astype(np.float32)
    return (x + np.float32(0.5)) * np.float32(1.0 / 16777216.0)


def loader_draw(n, seed, k):
    """float32[n]: draw k of particles 0 .. n - 1"""
    idx = np.arange(n, dtype=np.uint64)
    a = mix32(idx * np.uint64(9) + np.uint64(k))                                    # (mix32 keeps the low 32 bits of what it is given)
    b = mix32(np.uint64((int(seed) * 0x9e3779b9 + k) & 0xffffffff))
    return unit_top_closed(mix32(a ^ b))


class Loaded:
    pass


def loader_ref(grid, ppc, seed, q, u, vth):
    """What load_maxwellian(ppc, seed, q, u, vth) writes on that grid.  Exact members: np, i, dx, dy, dz, q (float32, int32),
    and the float32 inputs of the transcendental functions l1, a1, l2, a2 (r1 = sqrt(-2 log l1), r2 = sqrt(-2 log l2)).
    From there in float64: r1, r2, normals float64[np, 3] = (r1 cos a1, r1 sin a1, r2 cos a2), and the momenta
    u = drift + vth * normals with drift and vth the float32 values the library is handed."""
    nx, ny, nz = grid
    n = nx * ny * nz * int(ppc)
    out = Loaded()
    out.np = n
    cell = np.arange(n, dtype=np.int64) // int(ppc)
    cz, r = cell // (nx * ny), cell % (nx * ny)
    out.i = voxel(r % nx + 1, r // nx + 1, cz + 1, grid).astype(np.int32)
    two, one = np.float32(2.0), np.float32(1.0)
    out.dx, out.dy, out.dz = (two * loader_draw(n, seed, k) - one for k in range(3))
    out.q = np.full(n, q, np.float32)
    out.l1, out.l2 = loader_draw(n, seed, 3), loader_draw(n, seed, 5)
    out.a1, out.a2 = TWO_PI_F * loader_draw(n, seed, 4), TWO_PI_F * loader_draw(n, seed, 6)
    assert out.a1.dtype == np.float32 and out.dx.dtype == np.float32
    out.r1 = np.sqrt(-2.0 * np.log(out.l1.astype(np.float64)))
    out.r2 = np.sqrt(-2.0 * np.log(out.l2.astype(np.float64)))
    a1, a2 = out.a1.astype(np.float64), out.a2.astype(np.float64)
    out.normals = np.stack([out.r1 * np.cos(a1), out.r1 * np.sin(a1), out.r2 * np.cos(a2)], axis=1)
    out.r = np.stack([out.r1, out.r1, out.r2], axis=1)
    drift = np.array([float(np.float32(c)) for c in u])
    out.vth = float(np.float32(vth))
    out.u = drift[None, :] + out.vth * out.normals
    return out


def loader_bound(ref):
    """float64[np, 3]: how far a float32 momentum of the device may lie from ref.u.  The device computes
    u = drift + (vth * r) * trig(a) in float32 with r = sqrtf(-2 logf(l)).  logf is K_LOG ulp off at most, the root halves
    a relative error and rounds once, and -2 * x is exact: r carries (K_LOG / 2 + 1) roundings -- stated as K_LOG / 2 + 2;
    vth * r rounds once; cosf / sinf are K_TRIG ulp of 1 off in absolute terms; the last product and the sum round once
    each: vth * r * (K_LOG / 2 + K_TRIG + 4) * 2^-24 + 2^-24 * |u_ref|.  K_LOG = K_TRIG = 2: the installed ROCm states no
    error bound for logf, sinf or cosf in its headers or documents, so the fallback of two ulp each stands; nothing here
    comes from a device run."""
    return ref.vth * ref.r * (K_LOG / 2 + K_TRIG + 4) * 2.0 ** -24 + 2.0 ** -24 * np.abs(ref.u)
