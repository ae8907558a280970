"""tests/load_ref.py -- the numpy restatement of THE RULE of vpic_hip_species_load_profile (include/vpic_hip.h) -- held to
what can be known without a GPU: the published answers of Philox-4x32-10, the open interval of the positions, the boost
against the production deck's own formula, the Lorentz factor of the boosted momentum, and the share of particles that
Zenitani's flipping method turns around.

Agreement found here (10 000 draws at each |D| of 1e-3, 1e-2, 0.1, 1, 10; uth = 0.6), in units of 2^-53 relative:
    | u_rule - u_deck | / | u_deck |   (drift in the x-y plane, no flip; decks/trecon-part/turbulence.cxx:538-541)   : WORST_BOOST = 68.43
    | sqrt(1 + u.u) - gd (gw + (D.w) / gd) | / gamma                                                                  : WORST_GAMMA = 17.45
(The boost's worst case is at |D| = 1, where a thermal momentum against the drift nearly cancels it and |u_deck| is small;
at the other drifts it is 15 or less.  The tests here assert the constants as they stand, later tests take 4 x.)"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import load_ref as R  # noqa: E402

ULP = 2.0 ** -53
WORST_BOOST, WORST_GAMMA = 68.43, 17.45
DRIFTS = (1e-3, 1e-2, 0.1, 1.0, 10.0)


@pytest.mark.parametrize("counter, key, want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xffffffff,) * 4, (0xffffffff, 0xffffffff), "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(counter, key, want):
    got = R.philox(np.array(counter, np.uint32), key)
    assert " ".join("%08x" % int(v) for v in got) == want


def test_words_are_two_blocks_of_cell_and_number():
    """block b of (cell, j) is philox((lo32 c, hi32 c, j, b), (seed, stream)), also for a cell beyond 2^32"""
    cell, j = np.array([5, (7 << 32) + 3], np.uint64), np.array([0, 70000])
    w = R.words(cell, j, 11, 3)
    for k in range(2):
        for b in range(2):
            ctr = np.array([int(cell[k]) & 0xffffffff, int(cell[k]) >> 32, int(j[k]), b], np.uint32)
            assert np.array_equal(w[k, 4 * b:4 * b + 4], R.philox(ctr, (11, 3)))
    assert not np.array_equal(R.words(cell, j, 11, 4), w) and not np.array_equal(R.words(cell, j, 12, 3), w)


def test_positions_are_strictly_inside_at_the_extreme_words():
    r = np.array([0, 1, 0xff, 0x100, 0x7fffffff, 0x80000000, 0xfffffeff, 0xffffff00, 0xffffffff], np.uint32)
    x = R.unit_open(r)
    assert x.dtype == np.float32 and np.all(x > 0) and np.all(x < 1)
    assert x[0] == np.float32(2.0 ** -25) and x[-1] == np.nextafter(np.float32(1), np.float32(0))
    d = R.offsets(x)
    assert d.dtype == np.float32 and np.all(d > -1) and np.all(d < 1)
    n = R.numbers(np.tile(r[:, None], (1, 8)))
    assert np.all(np.isfinite(n))


def sample(n, seed):
    """n particles' numbers from the generator itself (cell 0 .. 9, j = 0 ..)"""
    m = np.arange(n)
    return R.numbers(R.words((m % 10).astype(np.uint64), m // 10, seed, 0))


def boost_case(drift, n=10000):
    d = sample(n, 1234)
    rng = np.random.default_rng(7)
    angle = rng.uniform(0, 2 * np.pi, n)
    ud = np.stack([drift * np.cos(angle), drift * np.sin(angle), np.zeros(n)], axis=1).astype(np.float32)
    uth = np.full((n, 3), 0.6, np.float32)
    return uth, ud, d


def test_boost_is_the_decks_formula():
    """no flip, drift in the x-y plane: ux = (GVD upa VDX / VD - upe VDY / VD) + GVD VDX gu, uy likewise, uz = uz1"""
    worst = 0.0
    for drift in DRIFTS:
        uth, ud, d = boost_case(drift)
        u, flipped, w, gw, gd, wD = R.momentum(uth, ud, d[:, 3:6], d[:, 6], False, parts=True)
        assert not flipped.any()
        D = ud.astype(np.float64)
        GVD = np.sqrt(1 + D[:, 0] ** 2 + D[:, 1] ** 2)
        VDX, VDY = D[:, 0] / GVD, D[:, 1] / GVD
        VD = np.sqrt(VDX ** 2 + VDY ** 2)
        upa1 = (w[:, 0] * VDX + w[:, 1] * VDY) / VD                    # the thermal draw along and across the drift
        upe1 = (-w[:, 0] * VDY + w[:, 1] * VDX) / VD
        uz1 = w[:, 2]
        gu1 = np.sqrt(1.0 + upa1 * upa1 + upe1 * upe1 + uz1 * uz1)
        ux = (GVD * upa1 * VDX / VD - upe1 * VDY / VD) + GVD * VDX * gu1
        uy = (GVD * upa1 * VDY / VD + upe1 * VDX / VD) + GVD * VDY * gu1
        deck = np.stack([ux, uy, uz1], axis=1)
        err = np.linalg.norm(u - deck, axis=1) / np.linalg.norm(deck, axis=1) / ULP
        print("boost |D| = %g: worst %.2f x 2^-53" % (drift, err.max()))
        worst = max(worst, float(err.max()))
    assert worst <= WORST_BOOST


def test_gamma_of_the_boosted_momentum():
    """gamma_lab = gd (gw + (D . w) / gd), with and without the flip (w and D . w after it)"""
    worst = 0.0
    for flip in (False, True):
        for drift in DRIFTS:
            uth, ud, d = boost_case(drift)
            ud[:, 2] = np.float32(0.3 * drift)                           # (any direction)
            u, flipped, w, gw, gd, wD = R.momentum(uth, ud, d[:, 3:6], d[:, 6], flip, parts=True)
            assert flipped.any() == flip
            gamma = np.sqrt(1 + (u * u).sum(axis=1))
            err = np.abs(gamma - gd * (gw + wD / gd)) / gamma / ULP
            print("gamma flip = %d |D| = %g: worst %.2f x 2^-53" % (flip, drift, err.max()))
            worst = max(worst, float(err.max()))
    assert worst <= WORST_GAMMA


def test_rest_frame_and_cold_cells():
    """D2 == 0: u = w exactly; uth == 0: u = D exactly, flipped or not"""
    d = sample(1000, 5)
    uth = np.full((1000, 3), 0.6, np.float32)
    zero = np.zeros((1000, 3), np.float32)
    u = R.momentum(uth, zero, d[:, 3:6], d[:, 6], True)
    assert np.array_equal(u, (uth.astype(np.float64) * d[:, 3:6].astype(np.float64)).astype(np.float32))
    ud = np.tile(np.array([0.3, -2.0, 0.01], np.float32), (1000, 1))
    for flip in (False, True):
        assert np.array_equal(R.momentum(zero, ud, d[:, 3:6], d[:, 6], flip), ud)


def test_flipped_share_is_the_analytic_one():
    """isotropic uth = 0.6 boosted by |D| = 1: a particle is flipped with probability max(0, -beta_d . v), v = w / gw; the
    share of the sample is held within 6 standard errors of the mean of that over the Gaussian (quadrature over the
    component along the drift and the radius across it).  The indicator is a Bernoulli variable of that mean."""
    n, sigma = 100000, 0.6
    d = sample(n, 99)
    uth = np.full((n, 3), sigma, np.float32)
    ud = np.tile((np.array([1.0, 2.0, -2.0]) / 3.0).astype(np.float32), (n, 1))
    D2 = float((ud[0].astype(np.float64) ** 2).sum())
    beta = np.sqrt(D2 / (1 + D2))
    flipped = R.momentum(uth, ud, d[:, 3:6], d[:, 6], True, parts=True)[1]
    wp = np.linspace(-10 * sigma, 0, 4001)[:, None]                    # along the drift (only w_par < 0 can flip)
    rho = np.linspace(0, 10 * sigma, 4001)[None, :]
    pdf = np.exp(-wp ** 2 / (2 * sigma ** 2)) / (sigma * np.sqrt(2 * np.pi)) * rho / sigma ** 2 * np.exp(-rho ** 2 / (2 * sigma ** 2))
    integrand = pdf * (-beta * wp / np.sqrt(1 + wp ** 2 + rho ** 2))
    def trapezoid(y, x):
        return ((y[..., 1:] + y[..., :-1]) * np.diff(x) / 2).sum(axis=-1)
    expect = float(trapezoid(trapezoid(integrand, rho[0]), wp[:, 0]))
    share = float(flipped.mean())
    se = np.sqrt(expect * (1 - expect) / n)
    print("flipped share %.5f, expected %.5f, standard error %.5f" % (share, expect, se))
    assert 0.05 < expect < 0.2
    assert abs(share - expect) <= 6 * se


def test_order_and_partition_of_a_call():
    """ascending voxel, ascending j within a cell; partition[] with ghost voxels as empty ranges"""
    dims = (3, 2, 2)
    count = np.arange(12).reshape(2, 2, 3) % 4
    p, part, cell, j = R.load(dims, count, -0.5, seed=3, global_dims=(10, 9, 8), offset=(2, 3, 4), tag0=100)
    n = int(count.sum())
    assert len(p) == n and part[-1] == n and len(part) == 5 * 4 * 4 + 1
    assert np.all(np.diff(p["i"]) >= 0) and np.array_equal(p["tag"], 100 + np.arange(n))
    for v in range(5 * 4 * 4):
        assert np.all(p["i"][part[v]:part[v + 1]] == v)
    same = np.diff(p["i"]) == 0
    assert np.all(np.diff(j)[same] == 1) and np.all(j[1:][~same] == 0)
    x, y, z = p["i"] % 5 - 1, p["i"] // 5 % 4 - 1, p["i"] // 20 - 1
    assert np.array_equal(cell, ((2 + x) + 10 * ((3 + y) + 9 * (4 + z))).astype(np.uint64))
