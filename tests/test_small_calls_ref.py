"""The references of tests/test_gpu_small_calls.py (tests/small_calls_ref.py) pinned without a GPU: the generated inputs
hold what the GPU tests rely on; energy_terms / energy_exact agree with the oracle's orc_energy_p, in total and term for
term, within the bound of a sequential double sum; the restated loader draws what a Maxwellian is (means, variances and
every correlation of its six draws inside five standard errors -- a draw index used twice would sit at 1 / sqrt(12)-ish,
hundreds of them); and both derived bounds discriminate."""
import os
import sys
from fractions import Fraction

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import small_calls_ref as R  # noqa: E402
from oracle import pyorc  # noqa: E402

GRIDS = [(5, 3, 4), (9, 6, 5)]
QMS = [-1.0, 1.0 / 1836.0]


def orc_grid(grid, dt=0.4):
    nx, ny, nz = grid
    return pyorc.make_grid(nx, ny, nz, float(nx), float(ny), float(nz), np.float32(dt))


def test_generated_inputs_hold_what_the_gpu_tests_rely_on():
    for grid in GRIDS:
        p = R.particles(3, R.N, grid)
        fi = R.interpolator(4, grid)
        inner = R.interior_voxels(grid)
        assert np.isin(p["i"], inner).all() and len(np.unique(p["tag"])) == R.N
        for kind in range(len(R.KINDS)):                                         # every kind of record under some particles
            assert (p["i"] % len(R.KINDS) == kind).sum() > 100, (grid, R.KINDS[kind])
        mag = np.sqrt(p["ux"].astype(np.float64) ** 2 + p["uy"].astype(np.float64) ** 2 + p["uz"].astype(np.float64) ** 2)
        body = mag[:-R.N_HAND]
        assert body.min() < 2e-3 and body.max() > 20.0 and 0.9e-3 < body.min() and body.max() < 30.1
        for c in ("dx", "dy", "dz"):
            assert (p[c] == 1.0).any() and (p[c] == -1.0).any() and (p[c] == 0.0).any() and np.abs(p[c]).max() <= 1.0
        q = p["q"].astype(np.float64)
        assert (q < 0).sum() > 0.1 * R.N and (q > 0).sum() > 0.5 * R.N and 50 < (q == 0).sum() < 0.03 * R.N
        nz = np.abs(q[:-R.N_HAND][q[:-R.N_HAND] != 0])
        assert nz.max() / nz.min() > 50.0
        # the hand-made block: u = 0, one component only, subnormal products
        hand = p[-R.N_HAND:]
        u = np.stack([hand["ux"], hand["uy"], hand["uz"]], axis=1)
        assert ((u == 0).all(axis=1)).sum() >= 4 and ((u != 0).sum(axis=1) == 1).sum() >= 3
        tiny = np.float32(np.finfo(np.float32).tiny)
        sq = (hand["ux"] * hand["ux"])[7]
        assert 0 < sq < tiny                                                      # u * u is a subnormal float, not zero
        assert 0 < abs(hand["ux"][8]) < tiny
        k = R.qdt_2mc(-1.0, orc_grid(grid))
        rec = fi[hand["i"][9]]
        assert all(0 < abs(rec[n]) < tiny for n in R.E_NAMES + R.B_NAMES) and 0 < abs(k * rec["ex"]) < tiny
        # the strong records: v2 = (qdt_4mc / gamma)^2 |cB|^2 reaches 1 and above for part of the particles
        f = fi[p["i"]]
        cb2 = f["cbx"].astype(np.float64) ** 2 + f["cby"].astype(np.float64) ** 2 + f["cbz"].astype(np.float64) ** 2
        v2 = (0.5 * float(k)) ** 2 / (1.0 + mag ** 2) * cb2
        assert 0.03 * R.N < (v2 >= 1.0).sum() < 0.2 * R.N and v2.max() > 10.0
        assert (v2 == 0).sum() > 0.2 * R.N                                        # "zero" and "e_only" voxels


def test_exact_sum_is_exact():
    rng = np.random.default_rng(0)
    t = rng.normal(size=3000) * 10.0 ** rng.uniform(-40, 3, 3000)
    t[::7] = 0.0
    assert R.exact_sum(t) == sum((Fraction(float(x)) for x in t), Fraction(0))
    assert R.exact_sum(np.array([1e300, 1.0, -1e300])) == 1 and R.exact_sum(np.zeros(0)) == 0
    assert R.exact_sum(np.array([5e-324, -2.0 ** -1074 * 3])) == Fraction(-2) * Fraction(2) ** -1074


def test_energy_exact_agrees_with_the_oracle():
    """within the bound of the oracle's sequential sum, np * 2^-53 * sum |t| * c^2 / |q_m|, plus the two roundings of its result"""
    for g, grid in enumerate(GRIDS):
        og = orc_grid(grid)
        p = R.particles(3 + g, R.N, grid)
        fi = R.interpolator(4 + g, grid)
        for q_m in QMS:
            t = R.energy_terms(p, fi, q_m, og)
            exact, sabs = R.energy_exact(t, q_m, og)
            got = pyorc.energy_p(p, len(p), q_m, fi, og)
            bound = R.energy_bound(len(p), sabs, exact, q_m, og)
            err = abs(Fraction(got) - exact)
            print(grid, q_m, float(exact), float(err), bound)
            assert err <= bound and bound < 1e-11 * sabs * R.energy_scale(q_m, og) and float(exact) != 0.0
            assert (t < 0).any() and (t > 0).any() and sabs > 1.2 * abs(float(R.exact_sum(t)))     # weights of both signs


def test_energy_terms_equal_the_oracle_term_for_term():
    """t_k c^2 / q_m against orc_energy_p over the first k + 1 particles minus over the first k: each of the two is off by
    its own sequential bound at most"""
    grid = GRIDS[0]
    og = orc_grid(grid)
    fi = R.interpolator(4, grid)
    head, hand = R.particles(3, R.N, grid)[:300], R.handmade(grid)
    for q_m in QMS:
        c2_qm = Fraction(float(np.float32(og.cvac))) ** 2 / Fraction(float(np.float32(q_m)))
        t = R.energy_terms(head, fi, q_m, og)
        prefix = [pyorc.energy_p(head, k, q_m, fi, og) for k in range(len(head) + 1)]
        worst = 0.0
        for k in range(len(head)):
            sabs = float(np.abs(t[:k + 1]).sum())
            bound = R.energy_bound(k + 1, sabs, prefix[k + 1], q_m, og) + R.energy_bound(k, sabs, prefix[k], q_m, og)
            err = abs(Fraction(prefix[k + 1]) - Fraction(prefix[k]) - Fraction(float(t[k])) * c2_qm)
            assert err <= bound, (q_m, k, float(err), bound)
            if t[k] != 0:
                worst = max(worst, bound / abs(float(t[k]) * float(c2_qm)))
        print(q_m, "largest bound relative to its term:", worst)
        assert worst < 1e-2
        # the hand-made particles one at a time (behind larger terms a subnormal one would be lost in the prefix sums):
        # the sum is the term itself, only the two roundings of the result remain
        t = R.energy_terms(hand, fi, q_m, og)
        for k in range(len(hand)):
            one = pyorc.energy_p(hand[k:k + 1].copy(), 1, q_m, fi, og)
            assert abs(Fraction(one) - Fraction(float(t[k])) * c2_qm) <= 2 * R.U * abs(one), (q_m, k)
    # the subnormal squares contribute (u = 1e-20: w is a subnormal float, not zero); a subnormal half kick alone squares to zero
    t = R.energy_terms(hand, fi, -1.0, og)
    assert t[7] != 0 and abs(t[7]) < 1e-38 and t[9] == 0 and t[0] == 0 and t[10] != 0


def test_loader_restatement_is_a_maxwellian():
    grid, ppc = (16, 16, 16), 64
    ref = R.loader_ref(grid, ppc, 1, -0.5, (0.0, 0.0, 0.0), 1.0)
    n = ref.np
    assert n == 16 ** 3 * 64 and ref.u.shape == (n, 3)
    six = np.concatenate([ref.normals, np.sqrt(3.0) * np.stack([ref.dx, ref.dy, ref.dz], axis=1).astype(np.float64)], axis=1)
    se = 1.0 / np.sqrt(n)
    mean = six.mean(axis=0)
    var = ref.normals.var(axis=0)
    corr = np.corrcoef(six.T)
    off = corr[~np.eye(6, dtype=bool)]
    print("means / se", mean / se, "variances", (var - 1) / np.sqrt(2.0 / n), "largest correlation / se", np.abs(off).max() / se)
    assert (np.abs(mean) <= 5 * se).all()
    assert (np.abs(var - 1.0) <= 5 * np.sqrt(2.0 / n)).all()
    assert (np.abs(off) <= 5 * se).all()
    # cells: x fastest, ppc each, non-decreasing
    assert (np.diff(ref.i) >= 0).all() and (np.bincount(ref.i)[R.interior_voxels(grid)] == ppc).all()
    assert ref.i[0] == R.voxel(1, 1, 1, grid) and ref.i[ppc] == R.voxel(2, 1, 1, grid) and ref.i[16 * ppc] == R.voxel(1, 2, 1, grid)
    for c in (ref.dx, ref.dy, ref.dz):
        assert c.dtype == np.float32 and -1.0 < c.min() and c.max() <= 1.0
    other = R.loader_ref(grid, 1, 2, -0.5, (0.0, 0.0, 0.0), 1.0)
    assert not np.array_equal(other.dx, ref.dx[::ppc][:other.np])


def test_loader_bound_discriminates():
    """below 1e-5 vth per component for all but the tail r > 5"""
    for vth, drift in ((0.02, (0.03, -0.02, 0.01)), (0.6, (0.3, -0.2, 0.1))):
        ref = R.loader_ref((8, 8, 8), 64, 1, -0.5, drift, vth)
        b = R.loader_bound(ref)
        body = ref.r <= 5.0
        assert body.mean() > 0.9999 and (b[body] < 1e-5 * ref.vth).all() and (b > 0).all()
        print(vth, "largest bound / vth in the body:", b[body].max() / ref.vth)
