"""The deposit MOMENTS of the float push instances (push_device.h: streak12_moments, term_of, moments_to_terms), without a GPU.

The four terms of an axis group of a streak are a +-1 combination of four moments; for the x group, with S0 = q ux,
S1 = S0 dy, S2 = S0 dz, T3 = S1 dz + v5:

    a0 = S0 - S1 - S2 + T3    a1 = S0 + S1 - S2 - T3    a2 = S0 - S1 + S2 - T3    a3 = S0 + S1 + S2 + T3

and cyclically for y and z; the moments sit in the group's four accumulator slots as (T3, S1, S2, S0).  The float instances
sum the moments (scan, LDS atomics, window) and apply the map where a value leaves for the global accumulator.
Checked here:
  * the map reproduces streak12's formula (restated below operation by operation) in float64 on random streaks, with
    |d| = 1, u = 0 and q = 0 among them -- to a few float64 roundings;
  * the map is its own inverse up to the factor 4 (exactly: small integers);
  * a model of the kernel's rounding -- per-particle values in float32 with the kernel's contracted multiply-adds, float32
    sums over blocks of 16 lanes (TILE_MAIN_BLOCK), the blocks and the map in double (the tile window), one rounding to
    float32 -- against exact float64 sums: the moment route stays within ACC_TOL of the largest entry and within twice the
    term route's own worst error, for a cold beam and a vth = 0.6 c plasma at 16 and 64 particles per cell.
"""
import numpy as np
import pytest

ACC_TOL = 2e-6                      # the project's bound on float accumulator sums (tests/test_gpu_kernels.py)
f32, f64 = np.float32, np.float64

# rows: term j of a group; columns: the group's four slots, which hold (T3, S1, S2, S0)
MAP = np.array([[1, -1, -1, 1],
                [-1, 1, -1, 1],
                [-1, -1, 1, 1],
                [1, 1, 1, 1]], f64)
AXES = ((0, 1, 2), (1, 2, 0), (2, 0, 1))     # ACCUMULATE_J(x,y,z), (y,z,x), (z,x,y)


def streak12_ref(q, d, u, v5, t=f64):
    """push_device.h: streak12, operation by operation, in arithmetic t.  q, v5: [n]; d, u: [n, 3].  Returns [n, 12]."""
    one = t(1)
    out = []
    for X, Y, Z in AXES:
        v4 = q * u[:, X]
        v1 = v4 * d[:, Y]
        v0 = v4 - v1
        v1 = v1 + v4
        v4 = one + d[:, Z]
        v2 = v0 * v4
        v3 = v1 * v4
        v4 = one - d[:, Z]
        v0 = v0 * v4
        v1 = v1 * v4
        out += [v0 + v5, v1 - v5, v2 - v5, v3 + v5]
    return np.stack(out, axis=1).astype(t)


def moments_ref(q, d, u, v5):
    """the twelve moments in accumulator order, float64"""
    out = []
    for X, Y, Z in AXES:
        s0 = q * u[:, X]
        s1 = s0 * d[:, Y]
        out += [s1 * d[:, Z] + v5, s1, s0 * d[:, Z], s0]
    return np.stack(out, axis=1)


def expand(m):
    """the map, group by group: [n, 12] moments -> [n, 12] terms"""
    return np.concatenate([m[:, g:g + 4] @ MAP.T for g in (0, 4, 8)], axis=1)


def random_streaks(rng, n):
    d = rng.uniform(-1, 1, (n, 3))
    u = rng.standard_normal((n, 3)) * 0.3
    q = rng.uniform(-1.5, 1.5, n) * 0.01
    # the edge cases: a midpoint on a face or in a corner, a particle at rest, no charge
    d[0] = (1, -1, 1); d[1] = (-1, -1, -1); d[2] = (1, 0.25, -1); d[3:40, 0] = np.sign(d[3:40, 0])
    u[40:50] = 0; u[50:60, 1] = 0
    q[60:70] = 0
    return q, d, u, q * u[:, 0] * u[:, 1] * u[:, 2] / 3.0


def test_the_map_gives_streak12_s_terms():
    rng = np.random.default_rng(7)
    q, d, u, v5 = random_streaks(rng, 4096)
    terms = streak12_ref(q, d, u, v5)
    got = expand(moments_ref(q, d, u, v5))
    # a term is at most |q u| (1 + |dy|) (1 + |dz|) + |v5| <= 4 |q u| + |v5|, either way a handful of roundings of that
    scale = 4 * np.abs(q)[:, None] * np.abs(u).max(axis=1)[:, None] + np.abs(v5)[:, None]
    assert np.all(np.abs(got - terms) <= 8 * np.finfo(f64).eps * scale)
    assert np.all(got[40:50] == 0) and np.all(got[60:70] == 0)          # u = 0, q = 0: nothing to deposit, exactly
    # |d| = 1: the terms on the far side of the face vanish up to v5
    far = streak12_ref(q[:3], d[:3], u[:3], 0 * v5[:3])
    assert np.all(np.abs(expand(moments_ref(q[:3], d[:3], u[:3], 0 * v5[:3])) - far) <= 8 * np.finfo(f64).eps * scale[:3])
    assert np.count_nonzero(far[0]) < 12


def test_the_map_is_its_own_inverse_up_to_4():
    assert np.array_equal(MAP @ MAP, 4 * np.eye(4))
    assert np.array_equal(MAP, MAP.T)
    rng = np.random.default_rng(8)
    m = rng.integers(-1000, 1000, (64, 12)).astype(f64)
    assert np.array_equal(expand(expand(m)), 4 * m)


def fma32(a, b, c):
    """float32 fma of float32 operands: the product is exact in float64, the sum rounded there and once more to float32"""
    return (a.astype(f64) * b.astype(f64) + c.astype(f64)).astype(f32)


def per_particle_float32(q, d, u):
    """what a lane forms: the terms as the parent's contracted form had them, and the moments (streak12_moments)"""
    one = f32(1)
    qu = [q * u[:, k] for k in range(3)]
    v5 = (qu[0] * u[:, 1]) * (u[:, 2] * f32(1.0 / 3.0))
    terms, moments = [], []
    for X, Y, Z in AXES:
        s0 = qu[X]
        v0, v1 = fma32(-s0, d[:, Y], s0), fma32(s0, d[:, Y], s0)
        zp, zm = one + d[:, Z], one - d[:, Z]
        terms += [fma32(v0, zm, v5), fma32(v1, zm, -v5), fma32(v0, zp, -v5), fma32(v1, zp, v5)]
        s1 = s0 * d[:, Y]
        moments += [fma32(s1, d[:, Z], v5), s1, s0 * d[:, Z], s0]
    return np.stack(terms, axis=1), np.stack(moments, axis=1)


def block_sums(a, ncell, ppc):
    """float32 sums over blocks of 16 consecutive lanes (in lane order), the blocks then in double: [ncell, 12] float64"""
    a = a.reshape(ncell, ppc // 16, 16, 12)
    s = np.zeros((ncell, ppc // 16, 12), f32)
    for k in range(16):
        s = s + a[:, :, k, :]
    return s.astype(f64).sum(axis=1)


@pytest.mark.parametrize("ppc", [16, 64])
@pytest.mark.parametrize("plasma", ["cold beam", "hot"])
def test_rounding_model_moments_no_worse_than_terms(plasma, ppc):
    rng = np.random.default_rng(ppc + (1 if plasma == "hot" else 0))
    ncell = 8192 // ppc * 4
    n = ncell * ppc
    q = np.full(n, -1.0 / ppc, f32)
    d = rng.uniform(-1, 1, (n, 3)).astype(f32)                                   # streak midpoints
    vth, drift = (0.6, 0.0) if plasma == "hot" else (0.02, 0.2)
    u = (vth * rng.standard_normal((n, 3))).astype(f32)
    u[:, 0] += f32(drift)
    u *= f32(0.55)                                                               # half displacement in cells
    keep = np.abs(d + u).max(axis=1) <= 1                                        # the in-cell deposit: a crosser lane carries charge 0
    q = np.where(keep, q, f32(0))
    terms, moments = per_particle_float32(q, d, u)
    q64, d64, u64 = q.astype(f64), d.astype(f64), u.astype(f64)
    exact = streak12_ref(q64, d64, u64, q64 * u64[:, 0] * u64[:, 1] * u64[:, 2] / 3.0).reshape(ncell, ppc, 12).sum(axis=1)
    top = np.abs(exact).max()
    err_t = np.abs(block_sums(terms, ncell, ppc).astype(f32) - exact).max() / top
    err_m = np.abs(expand(block_sums(moments, ncell, ppc)).astype(f32) - exact).max() / top
    print("%s, %d ppc: worst error of the term route %.3e, of the moment route %.3e (of the largest entry; ACC_TOL %.0e)" % (plasma, ppc, err_t, err_m, ACC_TOL))
    assert err_m <= ACC_TOL
    assert err_m <= 2 * err_t
