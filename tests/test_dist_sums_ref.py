"""The per-bin sums of particle quantities (include/vpic_hip.h: vpic_hip_species_distribution_sums), restated in float64
numpy: what tests/test_gpu_dist_sums.py holds the kernels to.  Checked here, without a GPU, on hand-made particles that
sit on every branch of the rules -- a value exactly on half a quantum both ways, t just below 2^32 and at it, negative
values, a NaN through a zeroed interpolator record, q of two magnitudes, one, two and three factors; the expected sums
worked out by hand or by a scalar restatement in Python floats, asserted with == -- and on the generated inputs of the GPU
test, which must populate what that test relies on; plus the C side of the new ABI.

A factor is a coordinate (test_distribution_ref.coordinate, test_fieldcoord_ref.field_coordinate) or one of "one", "q",
"edotv", "epar_vpar".  Everything behind a value is +, -, x, / and sqrt in double on floats formed by single float
operations, which numpy and the device both round correctly; rint is exact.  So nothing here needs a margin: the GPU test
compares int64 sums with == and leaves no particle out.  (No factor is LOG10_KE: the library refuses it.)"""
import ctypes as C
import functools
import importlib
import math
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from test_distribution_ref import GRID, HAND_GRID, N, SEED, VTH, dist_inputs, particle_dtype  # noqa: E402
from test_fieldcoord_ref import (FIELD_NAMES, V_345, V_Z2, V_ZERO, field_coordinate, generated_interpolator,  # noqa: E402
                                 hand_interpolator, n_voxels)
from test_select_ref import INF, fields_ref  # noqa: E402

FACTORS = {"one": 32, "q": 33, "edotv": 34, "epar_vpar": 35}                  # VPIC_HIP_FACTOR_*
TWO32 = 4294967296.0
LDS_WORDS = 8192                                                              # VPIC_HIP_DIST_LDS_BINS: 32-bit words of the LDS path


def factor_value(p, grid, fi, name):
    """float64 values of one factor for every (live) particle of p"""
    if name == "one":
        return np.ones(len(p))
    if name == "q":
        return p["q"].astype(np.float64)
    if name in ("edotv", "epar_vpar"):
        ux, uy, uz = (p[c].astype(np.float64) for c in ("ux", "uy", "uz"))
        gamma = np.sqrt(((1.0 + ux * ux) + uy * uy) + uz * uz)
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            if name == "edotv":
                f = fields_ref(p, fi).astype(np.float64)
                return ((f[:, 0] * ux + f[:, 1] * uy) + f[:, 2] * uz) / gamma
            return (field_coordinate(p, grid, fi, "e_par") * field_coordinate(p, grid, fi, "u_par")) / gamma
    assert name != "log10_ke"
    return field_coordinate(p, grid, fi, name)


def distribution_sums_ref(p, grid, fi, desc, values):
    """(counts uint64, isums int64[n_val, ...], refused int64[n_val], (seen, kept, counted)) of the particles of p under
    desc = dict(axes=[(coord, lo, d, n), ...], select=[(coord, lo, hi), ...]) and values = [((factor, ...), quantum), ...]"""
    p = p[(p["i"] >= 0) & (p["i"] < n_voxels(grid))]
    seen = len(p)
    keep = np.ones(len(p), bool)
    for coord, lo, hi in desc.get("select", ()):
        c = field_coordinate(p, grid, fi, coord)
        with np.errstate(invalid="ignore"):
            keep &= (c >= lo) & (c < hi)
    p = p[keep]
    ok = np.ones(len(p), bool)
    ts = []
    for coord, lo, d, n in desc["axes"]:
        with np.errstate(invalid="ignore"):
            t = (field_coordinate(p, grid, fi, coord) - lo) / d
            ok &= (t >= 0) & (t < n)
        ts.append(t)
    kept = len(p)
    p = p[ok]
    bins = [np.trunc(t[ok]).astype(np.int64) for t in ts]
    shape = tuple(a[3] for a in reversed(desc["axes"]))
    n0 = desc["axes"][0][3]
    flat = bins[0] if len(bins) == 1 else bins[1] * n0 + bins[0]
    n_bins = int(np.prod(shape))
    counts = np.bincount(flat, minlength=n_bins).astype(np.uint64).reshape(shape)
    isums = np.zeros((len(values), n_bins), np.int64)
    refused = np.zeros(len(values), np.int64)
    for k, (factors, quantum) in enumerate(values):
        f = [factor_value(p, grid, fi, name) for name in tuple(factors) + ("one",) * (3 - len(factors))]
        with np.errstate(invalid="ignore", over="ignore"):
            t = ((f[0] * f[1]) * f[2]) / quantum
            taken = np.abs(t) < TWO32                                         # (a NaN is refused)
        refused[k] = int((~taken).sum())
        np.add.at(isums[k], flat[taken], np.rint(t[taken]).astype(np.int64))  # rint: to nearest, ties to even
    return counts, isums.reshape((len(values),) + shape), refused, (seen, kept, len(p))


def lds_words(desc, values):
    """32-bit LDS words the histogram and its sums take: a count and n_val 64-bit sums per bin"""
    return int(np.prod([a[3] for a in desc["axes"]])) * (1 + 2 * len(values))


# ---- generated inputs: the particles of the distribution tests with a seeded weight ----
def seeded_q(seed, n):
    """float32 macro-charges of two populations: a background around -0.01 and, one particle in eight, a beam 16 times heavier"""
    rng = np.random.default_rng(seed + 77)
    q = -0.01 * rng.uniform(0.5, 1.5, n)
    q[rng.integers(0, 8, n) == 0] *= 16.0
    return q.astype(np.float32)


def generated_inputs(seed=SEED, n=N, spread=1.0, first_tag=1):
    p = dist_inputs(seed, n, VTH, GRID, spread=spread)
    p["q"] = seeded_q(seed, n)
    p["tag"] = np.arange(n) + first_tag
    return p


def cases(vth=VTH):
    """The descriptors of the GPU test with their values, by name, on GRID = 96 x 8 x 6:
      lds4        1-D ke, 600 bins, four values (q; q ke; q edotv; mu one): LDS, the FIELDS instance
      global2d    ux-uz at 128 x 128 with q: above the LDS budget, global adds, no field
      par_perp    u_par-u_perp at 128 x 96 with q edotv: global adds, the FIELDS instance
      mixed       u_par-x at 40 x 24 of the particles under a ke threshold, a z range and a pitch range, three values
                  (q x; epar_vpar; q u_perp u_perp -- three factors): LDS
      refusing    1-D ke, 200 bins, q ke at a quantum that refuses a good share of the particles beside q, which refuses none
      edge_lds    1-D ux with q at 2730 bins: 8190 words, the last size in LDS (no field)
      edge_global 1-D ux with q at 2731 bins: 8193 words, the first size through global memory"""
    w = 3.0 * vth
    c = {
        "lds4": (dict(axes=[("ke", 0.0, 0.012 / 600, 600)]),
                 [(("q",), 1e-9), (("q", "ke"), 1e-11), (("q", "edotv"), 1e-9), (("mu", "one"), 1e-8)]),
        "global2d": (dict(axes=[("ux", -w, 2 * w / 128, 128), ("uz", -w, 2 * w / 128, 128)]), [(("q",), 1e-9)]),
        "par_perp": (dict(axes=[("u_par", -w, 2 * w / 128, 128), ("u_perp", 0.0, w / 96, 96)]), [(("q", "edotv"), 1e-9)]),
        "mixed": (dict(axes=[("u_par", -w, 2 * w / 40, 40), ("x", 0.0, 4.0, 24)],
                       select=[("ke", 0.5 * vth * vth, INF), ("z", 1.5, 4.25), ("cos_pitch", -0.5, 0.9)]),
                  [(("q", "x"), 1e-8), (("epar_vpar",), 1e-9), (("q", "u_perp", "u_perp"), 1e-8)]),
        "refusing": (dict(axes=[("ke", 0.0, 0.012 / 200, 200)]), [(("q", "ke"), 1e-14), (("q",), 1e-9)]),
        "edge_lds": (dict(axes=[("ux", -w, 2 * w / 2730, 2730)]), [(("q",), 1e-9)]),
        "edge_global": (dict(axes=[("ux", -w, 2 * w / 2731, 2731)]), [(("q",), 1e-9)]),
    }
    return c


IN_LDS, GLOBAL = ("lds4", "mixed", "refusing", "edge_lds"), ("global2d", "par_perp", "edge_global")
REFUSING = "refusing"


@functools.lru_cache(maxsize=None)
def reference_of_the_inputs():
    """{name: distribution_sums_ref(...)} of the generated inputs, computed once and left unchanged"""
    p, fi = generated_inputs(), generated_interpolator()
    out = {name: distribution_sums_ref(p, GRID, fi, desc, values) for name, (desc, values) in cases().items()}
    for r in out.values():
        for a in r[:3]:
            a.setflags(write=False)
    return out


# ---- hand-made particles ----
Q_SMALL, Q_LARGE = np.float32(-0.01), np.float32(-0.16)
U_AT, U_BELOW = 2.0 ** 30, 2.0 ** 30 - 64.0                                   # (float32 steps by 64 below 2^30)


def handmade_sums():
    """0: B == 0 in its voxel (a zeroed record), ux on half a quantum of 0.25 (t = 0.5); 1: t = 1.5; 2: t = -1.5; 3: t = -0.5;
    4: t = 2^32 exactly; 5: t = 2^32 - 256, the float32 below; 6: a dead slot; 7: u = (0.75, 0, 0) in B = (3, 0, 4),
    E = (1, 0, 0), the larger q: gamma = 1.25, EDOTV = 0.6; 8: i == nv"""
    rows = [  # voxel, dx,  dy,   dz,    ux,    uy,  uz,  q
        (V_ZERO, 0.25, -0.5, 0.0, 0.125, 0.0, 0.0, Q_SMALL),
        (V_Z2, 0.5, 0.25, -0.75, 0.375, 0.0, 0.0, Q_LARGE),
        (V_Z2, -0.5, 0.0, 0.5, -0.375, 0.0, 0.0, Q_SMALL),
        (V_Z2, 0.0, 0.0, 0.0, -0.125, 0.0, 0.0, Q_LARGE),
        (V_Z2, 0.0, 0.0, 0.0, U_AT, 0.0, 0.0, Q_SMALL),
        (V_Z2, 0.0, 0.0, 0.0, U_BELOW, 0.0, 0.0, Q_SMALL),
        (-1, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0, Q_SMALL),
        (V_345, 0.5, 0.0, 0.5, 0.75, 0.0, 0.0, Q_LARGE),
        (n_voxels(HAND_GRID), 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, Q_SMALL),
    ]
    p = np.zeros(len(rows), particle_dtype())
    for k, (i, dx, dy, dz, ux, uy, uz, q) in enumerate(rows):
        p[k]["i"], p[k]["dx"], p[k]["dy"], p[k]["dz"], p[k]["ux"], p[k]["uy"], p[k]["uz"], p[k]["q"] = i, dx, dy, dz, ux, uy, uz, q
    p["tag"] = np.arange(len(rows)) + 1
    assert float(p[5]["ux"]) == U_BELOW and float(p[4]["ux"]) == U_AT
    return p


HAND_UPLOADABLE = [0, 1, 2, 3, 4, 5, 7]          # an upload refuses a dead slot and i == nv
HAND_LIVE = HAND_UPLOADABLE
HAND_CASES = [
    (dict(axes=[("uy", -1.0, 2.0, 1)]),
     [(("ux",), 0.25), (("q", "ux"), 2.0 ** -20), (("q", "ux", "ux"), 2.0 ** -30), (("mu",), 0.5)]),
    (dict(axes=[("ux", -0.5, 0.5, 3)]), [(("edotv",), 2.0 ** -10), (("epar_vpar", "q"), 2.0 ** -24), (("one",), 1.0), (("b", "q"), 2.0 ** -16)]),
    (dict(axes=[("b", 0.0, 2.5, 2), ("ux", -1.0, 1.0, 2)], select=[("ke", 0.005, 1.0)]), [(("q", "ke", "b"), 2.0 ** -28), (("u_par", "one", "ux"), 2.0 ** -12)]),
]


def scalar_value(p, k, fi, name):
    """one factor of particle k, in Python floats, operation by operation as the header states it"""
    f32 = np.float32
    r, f = p[k], fi[p[k]["i"]]
    dx, dy, dz = f32(r["dx"]), f32(r["dy"]), f32(r["dz"])
    ux, uy, uz = float(r["ux"]), float(r["uy"]), float(r["uz"])
    ex = float((f["ex"] + dy * f["dexdy"]) + dz * (f["dexdz"] + dy * f["d2exdydz"]))
    ey = float((f["ey"] + dz * f["deydz"]) + dx * (f["deydx"] + dz * f["d2eydzdx"]))
    ez = float((f["ez"] + dx * f["dezdx"]) + dy * (f["dezdy"] + dx * f["d2ezdxdy"]))
    bx, by, bz = float(f["cbx"] + dx * f["dcbxdx"]), float(f["cby"] + dy * f["dcbydy"]), float(f["cbz"] + dz * f["dcbzdz"])
    gamma = math.sqrt(((1.0 + ux * ux) + uy * uy) + uz * uz)
    b = math.sqrt((bx * bx + by * by) + bz * bz)

    def over(a, d):
        return a / d if d != 0 else (math.nan if a == 0 or a != a else math.copysign(math.inf, a))

    u_par = over((ux * bx + uy * by) + uz * bz, b)
    e_par = over((ex * bx + ey * by) + ez * bz, b)
    u2 = (ux * ux + uy * uy) + uz * uz
    perp2 = u2 - u_par * u_par
    p2 = 0.0 if perp2 < 0 else perp2
    return {"one": 1.0, "q": float(r["q"]), "ux": ux, "uy": uy, "uz": uz, "ke": gamma - 1.0, "b": b, "u_par": u_par, "mu": over(p2, 2.0 * b),
            "edotv": ((ex * ux + ey * uy) + ez * uz) / gamma, "epar_vpar": (e_par * u_par) / gamma}[name]


def scalar_sums(p, fi, which, bins_of, n_bins, values):
    """the sums and refusals of particles `which` (bins_of[k]: the flat bin of particle k) by the scalar restatement;
    Python's round() is to nearest, ties to even"""
    isums = np.zeros((len(values), n_bins), np.int64)
    refused = np.zeros(len(values), np.int64)
    for k in which:
        for j, (factors, quantum) in enumerate(values):
            f = [scalar_value(p, k, fi, name) for name in tuple(factors) + ("one",) * (3 - len(factors))]
            t = ((f[0] * f[1]) * f[2]) / quantum
            if abs(t) < TWO32:
                isums[j, bins_of[k]] += round(t)
            else:
                refused[j] += 1
    return isums, refused


def test_handmade_particles_take_every_branch():
    p, g, fi = handmade_sums(), HAND_GRID, hand_interpolator()
    live = HAND_LIVE
    # the first case by hand: one bin holds all seven live particles
    desc, values = HAND_CASES[0]
    counts, isums, refused, stats = distribution_sums_ref(p, g, fi, desc, values)
    assert list(counts) == [7] and stats == (7, 7, 7) and isums.dtype == np.int64 and isums.shape == (4, 1)
    # ux in quanta of 0.25: 0.5 -> 0 and 1.5 -> 2 (ties to even, both ways), -1.5 -> -2, -0.5 -> -0, 2^32 refused, 2^32 - 256 taken, 3
    assert int(isums[0, 0]) == 0 + 2 - 2 - 0 + (2 ** 32 - 256) + 3 and refused[0] == 1
    t = factor_value(p[live], g, fi, "ux") / 0.25
    assert list(t) == [0.5, 1.5, -1.5, -0.5, TWO32, TWO32 - 256.0, 3.0]
    assert list(np.rint(t[:4])) == [0.0, 2.0, -2.0, -0.0]
    # q ux, two factors and two magnitudes of q, in quanta of 2^-20: the two huge momenta are refused
    qs, ql = float(Q_SMALL), float(Q_LARGE)
    want = sum(round(((q * u) * 1.0) / 2.0 ** -20) for q, u in ((qs, 0.125), (ql, 0.375), (qs, -0.375), (ql, -0.125), (ql, 0.75)))
    assert int(isums[1, 0]) == want and refused[1] == 2 and abs(qs) * 10 < abs(ql)
    # q ux ux, three factors
    want = sum(round(((q * u) * u) / 2.0 ** -30) for q, u in ((qs, 0.125), (ql, 0.375), (qs, -0.375), (ql, -0.125), (ql, 0.75)))
    assert int(isums[2, 0]) == want and refused[2] == 2
    # mu: NaN in the zeroed record (refused), ux^2 / 4 in B = (0, 0, 2) -- 2^58 and nearly that refused --, 0.5625 (1 - 0.36) / 10 in B = (3, 0, 4)
    mu = factor_value(p[live], g, fi, "mu")
    assert np.isnan(mu[0]) and list(mu[1:4]) == [0.03515625, 0.03515625, 0.00390625] and mu[4] == 2.0 ** 58
    assert int(isums[3, 0]) == 0 + 0 + 0 + round(scalar_value(p, 7, fi, "mu") / 0.5) and refused[3] == 3
    # particle 7: gamma = 1.25, E . u / gamma = 0.6, e_par = 0.6
    assert factor_value(p[[7]], g, fi, "edotv")[0] == 0.6 and scalar_value(p, 7, fi, "edotv") == 0.6
    assert factor_value(p[[7]], g, fi, "epar_vpar")[0] == (0.6 * scalar_value(p, 7, fi, "u_par")) / 1.25
    # the zeroed record: E == 0 gives EDOTV == 0 (taken), B == 0 gives NaN for EPAR_VPAR (refused)
    assert factor_value(p[[0]], g, fi, "edotv")[0] == 0.0 and np.isnan(factor_value(p[[0]], g, fi, "epar_vpar")[0])
    # every case against the scalar restatement, bin by bin
    for desc, values in HAND_CASES:
        counts, isums, refused, stats = distribution_sums_ref(p, g, fi, desc, values)
        bins_of, which = {}, []
        n0 = desc["axes"][0][3]
        for k in live:
            if not all(lo <= scalar_value(p, k, fi, c) < hi for c, lo, hi in desc.get("select", ())):
                continue
            t = [(scalar_value(p, k, fi, c) - lo) / d for c, lo, d, n in desc["axes"]]
            if all(0 <= tt < a[3] for tt, a in zip(t, desc["axes"])):
                which.append(k)
                bins_of[k] = int(t[0]) + (int(t[1]) * n0 if len(t) == 2 else 0)
        want_isums, want_refused = scalar_sums(p, fi, which, bins_of, counts.size, values)
        assert stats[0] == 7 and stats[2] == len(which) == int(counts.sum()), desc
        assert np.array_equal(isums.reshape(len(values), -1), want_isums), (desc, isums, want_isums)
        assert np.array_equal(refused, want_refused), (desc, refused, want_refused)
        assert np.array_equal(np.bincount(list(bins_of.values()), minlength=counts.size), counts.ravel())
    # the second case spreads over its bins and counts with ONE; the third leaves particles out by its range and its axes
    counts, isums, refused, stats = distribution_sums_ref(p, g, fi, *HAND_CASES[1])
    assert list(counts) == [2, 2, 1] and list(isums[2]) == [2, 2, 1] and refused[2] == 0 and refused[1] == 1
    counts, isums, refused, stats = distribution_sums_ref(p, g, fi, *HAND_CASES[2])
    assert stats == (7, 5, 4) and int(counts.sum()) == 4 and refused[1] == 1          # (B == 0: U_PAR is NaN)


def test_generated_inputs_populate_what_the_gpu_test_relies_on():
    p, fi = generated_inputs(), generated_interpolator()
    q = p["q"].astype(np.float64)
    assert len(np.unique(p["q"])) > N // 2 and q.max() < 0 and q.min() < -0.08 and np.median(q) > -0.015     # two populations
    ref = reference_of_the_inputs()
    paths = set()
    full = 0
    for name, (desc, values) in cases().items():
        counts, isums, refused, (seen, kept, counted) = ref[name]
        words = lds_words(desc, values)
        paths.add("lds" if words <= LDS_WORDS else "global")
        assert (words <= LDS_WORDS) == (name in IN_LDS) and (words > LDS_WORDS) == (name in GLOBAL), name
        print(f"({name}) seen {seen} kept {kept} counted {counted}, {words} words, non-empty {np.count_nonzero(counts)} of {counts.size}, "
              f"refused {list(refused)}, largest |sum| {[int(np.abs(s).max()) for s in isums]}")
        assert seen == N and int(counts.sum()) == counted and 0.02 * N < counted < N
        full += int(np.all(counts > 0))
        if name == REFUSING:
            assert 0.05 * counted < refused[0] < 0.95 * counted and refused[1] == 0      # refuses some, not all
        else:
            assert not refused.any(), name
        for k, (factors, quantum) in enumerate(values):
            assert np.count_nonzero(isums[k]) > 0.4 * np.count_nonzero(counts), (name, k)
            if factors == ("one",):
                assert np.array_equal(isums[k].astype(np.uint64), counts)
        if "select" in desc:
            assert 0.02 * N < kept < 0.6 * N
    assert paths == {"lds", "global"} and full >= 1
    assert lds_words(*cases()["edge_lds"]) == 8190 and lds_words(*cases()["edge_global"]) == 8193
    # the weight matters: the q-weighted histogram is not a multiple of the counts
    counts, isums = ref["lds4"][0], ref["lds4"][1]
    mean_q = isums[0][counts > 0] / counts[counts > 0]
    assert mean_q.max() - mean_q.min() > 0.05 * abs(mean_q.mean())
    # mixed signs: q edotv sums to far less than its absolute values do
    assert np.any(isums[2] > 0) and np.any(isums[2] < 0)
    # the field factors are finite for every generated particle
    for name in ("edotv", "epar_vpar") + FIELD_NAMES:
        assert np.all(np.isfinite(factor_value(p, GRID, fi, name))), name


def test_header_compiles_as_c11_and_struct_size(tmp_path):
    src = ('#include "vpic_hip.h"\n_Static_assert(sizeof(vpic_hip_dist_value_t) == 24, "size");\n'
           '_Static_assert(VPIC_HIP_FACTOR_ONE == 32 && VPIC_HIP_FACTOR_Q == 33 && VPIC_HIP_FACTOR_EDOTV == 34 && VPIC_HIP_FACTOR_EPAR_VPAR == 35\n'
           '               && VPIC_HIP_DIST_MAX_VALUES == 4, "constants");\n'
           'int main(void){ vpic_hip_dist_value_t v = {{VPIC_HIP_FACTOR_Q, VPIC_HIP_COORD_KE, VPIC_HIP_FACTOR_ONE}, 0, 1e-11};\n'
           '  int (*f)(vpic_hip_engine_t *, int, const vpic_hip_dist_t *, const vpic_hip_dist_value_t *, int, uint64_t *, int64_t *) = vpic_hip_species_distribution_sums;\n'
           '  int (*s)(vpic_hip_engine_t *, int64_t *) = vpic_hip_species_distribution_sums_stats; (void)f; (void)s;\n'
           '  return v.factor[1] == 6 && sizeof(v.quantum) == 8 && (char *)&v.quantum - (char *)&v == 16 ? 0 : 1; }\n')
    obj = str(tmp_path / "dist_sums_hdr_test.o")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-x", "c", "-", "-c", "-o", obj],
                   input=src.encode(), check=True)
    eng = importlib.import_module("old-vpic_amd.engine")
    assert C.sizeof(eng.DistValue) == 24 and eng.DistValue.quantum.offset == 16 and eng.VALUE_FACTORS == FACTORS
    assert eng.DIST_MAX_VALUES == 4 and eng.DIST_LDS_BINS == LDS_WORDS
    v = eng.dist_values([(("q",), 1e-9), (("q", "ke"), 1e-11), (("q", "edotv", "cos_pitch"), 1e-14)])
    assert [list(x.factor) for x in v] == [[33, 32, 32], [33, 6, 32], [33, 34, 18]] and v[2].quantum == 1e-14
    for bad in ([(("weight",), 1.0)], [(("pitch",), 1.0)]):
        try:
            eng.dist_values(bad)
        except KeyError:
            continue
        raise AssertionError("an unknown factor was accepted")
    for bad in ([], [(("q",), 1.0)] * 5, [((), 1.0)], [(("q",) * 4, 1.0)]):
        try:
            eng.dist_values(bad)
        except ValueError:
            continue
        raise AssertionError("a malformed value list was accepted")


def test_symbols_are_listed():
    lib_mod = importlib.import_module("old-vpic_amd._lib")
    for name in ("vpic_hip_species_distribution_sums", "vpic_hip_species_distribution_sums_stats"):
        assert name in lib_mod.EXPORTS, name
    eng = importlib.import_module("old-vpic_amd.engine")
    assert callable(eng.Engine.distribution_sums) and callable(eng.Engine.distribution_sums_stats)
