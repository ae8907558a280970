"""The coordinates of a particle in the frame of the local magnetic field (include/vpic_hip.h: VPIC_HIP_COORD_U_PAR ..
VPIC_HIP_COORD_E_PAR), restated in float64 numpy: what tests/test_gpu_fieldcoord.py holds the kernels to.  Checked here,
without a GPU, on hand-made particles that sit on every branch of the rules -- each expected value worked out by hand or
by a scalar restatement in Python floats, and asserted with == -- and on the generated inputs of the GPU test, which
must populate what that test relies on; plus the constants of the C and the Python side.

The fields at the particle are test_select_ref.fields_ref (float32, one numpy operation per rounding); everything after
the promotion to double is +, -, x, / and sqrt, which numpy and the device both round correctly.  So nothing here needs
a margin: the GPU test compares with == and leaves no particle out.  (No descriptor here uses LOG10_KE.)"""
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

from test_distribution_ref import COORDS, GRID, HAND_GRID, N, SEED, VTH, coordinate, dist_inputs, particle_dtype  # noqa: E402
from test_select_ref import INF, fields_ref, interpolator_dtype, random_interpolator  # noqa: E402
from test_spectrum_ref import voxel  # noqa: E402

FIELD_NAMES = ("u_par", "u_perp", "cos_pitch", "mu", "b", "e_par")            # codes 16 .. 21
NAME_OF_CODE = {**dict(enumerate(COORDS)), **{16 + k: name for k, name in enumerate(FIELD_NAMES)}}


def n_voxels(grid):
    nx, ny, nz = grid
    return (nx + 2) * (ny + 2) * (nz + 2)


def field_coordinate(p, grid, fi, name):
    """float64 values of one coordinate for every slot of p, the six of the local field's frame from the interpolator
    fi; a slot that holds no live particle (a dead slot, i >= nv) reads NaN for those six."""
    if name not in FIELD_NAMES:
        return coordinate(p, grid, name)
    live = (p["i"] >= 0) & (p["i"] < n_voxels(grid))
    q = p.copy()
    q["i"][~live] = 0
    f = fields_ref(q, fi).astype(np.float64)
    ex, ey, ez, bx, by, bz = (f[:, k] for k in range(6))
    ux, uy, uz = (p[c].astype(np.float64) for c in ("ux", "uy", "uz"))
    with np.errstate(invalid="ignore", divide="ignore"):
        b = np.sqrt((bx * bx + by * by) + bz * bz)
        u_par = ((ux * bx + uy * by) + uz * bz) / b
        u2 = (ux * ux + uy * uy) + uz * uz
        perp2 = u2 - u_par * u_par
        p2 = np.where(perp2 < 0, 0.0, perp2)                               # (a NaN stays a NaN)
        out = {"b": lambda: b, "u_par": lambda: u_par, "u_perp": lambda: np.sqrt(p2), "cos_pitch": lambda: u_par / np.sqrt(u2),
               "mu": lambda: p2 / (2.0 * b), "e_par": lambda: ((ex * bx + ey * by) + ez * bz) / b}[name]()
    return np.where(live, out, np.nan)


def perp2_of(p, grid, fi):
    """u2 - U_PAR^2 before the clamp, for the checks below"""
    f = fields_ref(p, fi).astype(np.float64)
    bx, by, bz = f[:, 3], f[:, 4], f[:, 5]
    ux, uy, uz = (p[c].astype(np.float64) for c in ("ux", "uy", "uz"))
    with np.errstate(invalid="ignore", divide="ignore"):
        u_par = ((ux * bx + uy * by) + uz * bz) / np.sqrt((bx * bx + by * by) + bz * bz)
        return ((ux * ux + uy * uy) + uz * uz) - u_par * u_par


def distribution_ref(p, grid, fi, desc, stats=False):
    """test_distribution_ref.distribution_ref with the interpolator: uint64 counts, shape (n0,) or (n1, n0), of the
    particles of p under desc = dict(axes=[(coord, lo, d, n), ...], select=[(coord, lo, hi), ...]); with stats, also
    (live particles seen, kept by the selection, counted)."""
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
            ok &= (t >= 0) & (t < n)                                       # (a NaN is never counted)
        ts.append(t)
    bins = [np.trunc(t[ok]).astype(np.int64) for t in ts]
    n0 = desc["axes"][0][3]
    if len(bins) == 1:
        counts = np.bincount(bins[0], minlength=n0).astype(np.uint64)
    else:
        n1 = desc["axes"][1][3]
        counts = np.bincount(bins[1] * n0 + bins[0], minlength=n0 * n1).astype(np.uint64).reshape(n1, n0)
    return (counts, (seen, len(p), int(ok.sum()))) if stats else counts


def keep_mask(p, grid, fi, desc):
    """test_select_ref.keep_mask with the interpolator: bool[len(p)], which slots hold a kept particle, by the numbers
    of the vpic_hip_select_t that engine.select_desc makes of desc"""
    eng = importlib.import_module("old-vpic_amd.engine")
    d = eng.select_desc(**desc)
    keep = (p["i"] >= 0) & (p["i"] < n_voxels(grid))
    for k in range(d.n_sel):
        c = field_coordinate(p, grid, fi, NAME_OF_CODE[d.sel[k].coord])
        with np.errstate(invalid="ignore"):
            keep &= (c >= d.sel[k].lo) & (c < d.sel[k].hi)                 # (a NaN is in no range)
    tag = p["tag"].astype(np.int64)
    if d.flags & 1:
        keep &= (tag >= d.tag_lo) & (tag < d.tag_hi)
    if d.flags & 2:
        keep &= tag % np.int64(d.tag_every) == d.tag_phase
    assert not d.flags & ~3
    return keep


def select_ref(p, grid, fi, desc):
    """(index int64[n], particles particle_t[n], fields float32[n, 6]) of the kept particles, in array order"""
    index = np.flatnonzero(keep_mask(p, grid, fi, desc)).astype(np.int64)
    kept = p[index]
    return index, kept, fields_ref(kept, fi)


def descriptors(vth=VTH, lds_bins=8192):
    """The histograms of the GPU test, by name, on GRID = 96 x 8 x 6:
      par_perp  u_par x u_perp, 128 x 96: no position axis and too many bins for LDS, global adds
      cos_pitch 1-D pitch, 200 bins over [-0.8, 0.8): LDS
      x_pitch   x x pitch, 96 x 128, x bins one cell wide: the sliding window
      ke_mu     ke x mu, 64 x 64, of the particles with 1.5 <= B < 3 and -1.5 <= E_PAR < 2
      b         1-D B, 512 bins, of the particles with -0.5 <= pitch < 0.9 and 1.5 <= Z < 4.25
      e_par     1-D E_PAR, 300 bins, of the particles with u_perp >= vth"""
    w = 3.0 * vth
    d = {
        "par_perp": dict(axes=[("u_par", -w, 2 * w / 128, 128), ("u_perp", 0.0, w / 96, 96)]),
        "cos_pitch": dict(axes=[("cos_pitch", -0.8, 0.008, 200)]),
        "x_pitch": dict(axes=[("x", 0.0, 1.0, 96), ("cos_pitch", -0.8, 0.0125, 128)]),
        "ke_mu": dict(axes=[("ke", 0.0, 0.01 / 64, 64), ("mu", 0.0, 0.004 / 64, 64)], select=[("b", 1.5, 3.0), ("e_par", -1.5, 2.0)]),
        "b": dict(axes=[("b", 0.5, 4.0 / 512, 512)], select=[("cos_pitch", -0.5, 0.9), ("z", 1.5, 4.25)]),
        "e_par": dict(axes=[("e_par", -3.0, 0.02, 300)], select=[("u_perp", vth, INF)]),
    }
    assert np.prod([a[3] for a in d["par_perp"]["axes"]]) > lds_bins and np.prod([a[3] for a in d["x_pitch"]["axes"]]) > lds_bins
    for name in ("cos_pitch", "ke_mu", "b", "e_par"):
        assert np.prod([a[3] for a in d[name]["axes"]]) <= lds_bins
    return d


IN_LDS, WINDOW, GLOBAL = ("cos_pitch", "ke_mu", "b", "e_par"), ("x_pitch",), ("par_perp",)


def selections():
    """the selections of the GPU test, by name, with the number each keeps of generated_inputs() under
    random_interpolator(4, GRID): computed on the CPU when the feature was specified, and asserted below"""
    return {
        "pitch_every": (dict(select=[("cos_pitch", 0.9, 1.0)], tag_every=(3, 1)), 9187),
        "mu": (dict(select=[("mu", 0.003, INF)]), 61505),
        "b": (dict(select=[("b", 2.0, 2.5)]), 136083),
        "par": (dict(select=[("u_par", -0.02, 0.03), ("ke", 0.004, INF)]), 44146),
    }


B_RANGE = (2.0, 2.5)                                                      # of selections()["b"]


def generated_inputs():
    p = dist_inputs(SEED, N, VTH, GRID)
    p["tag"] = np.arange(N) + 1
    return p


@functools.lru_cache(maxsize=None)
def generated_interpolator():
    return random_interpolator(4, GRID)


# ---- hand-made particles ----
def search_perp2_negative():
    """(cbx, cby, cbz) in float32 for which u = B / 2 -- exactly along B -- has u2 - U_PAR^2 < 0 by rounding alone, the
    first of a seeded sequence of candidates; None when there is none (the test asserts there is)"""
    rng = np.random.default_rng(7)
    for _ in range(1000):
        b = rng.uniform(0.5, 2.0, 3).astype(np.float32)
        bx, by, bz = (float(v) for v in b)
        ux, uy, uz = (float(np.float32(0.5) * v) for v in b)               # (halving a float32 is exact)
        u_par = ((ux * bx + uy * by) + uz * bz) / math.sqrt((bx * bx + by * by) + bz * bz)
        if ((ux * ux + uy * uy) + uz * uz) - u_par * u_par < 0.0:
            return b
    return None


V_ZERO, V_Z2, V_ALONG, V_345 = (voxel(1, 1, 1, HAND_GRID), voxel(2, 1, 1, HAND_GRID), voxel(3, 1, 1, HAND_GRID),
                                voxel(1, 2, 1, HAND_GRID))
V_GHOST = voxel(0, 1, 1, HAND_GRID)


def hand_interpolator():
    """all zero -- V_ZERO's record stays so: B == 0 there -- but for:
      V_Z2     B = (0, 0, 2) whatever the offsets, ez = 0.5
      V_ALONG  B = what search_perp2_negative found (no gradient)
      V_345    cbx = 1 + 4 dx, cbz = 5 - 2 dz: (3, 0, 4) at dx = dz = 0.5; ex = 1
      V_GHOST  cby = 1 + 2 dy: (0, 2, 0) at dy = 0.5"""
    fi = np.zeros(n_voxels(HAND_GRID), interpolator_dtype())
    fi[V_Z2]["cbz"], fi[V_Z2]["ez"] = 2.0, 0.5
    b = search_perp2_negative()
    fi[V_ALONG]["cbx"], fi[V_ALONG]["cby"], fi[V_ALONG]["cbz"] = b
    fi[V_345]["cbx"], fi[V_345]["dcbxdx"], fi[V_345]["cbz"], fi[V_345]["dcbzdz"], fi[V_345]["ex"] = 1.0, 4.0, 5.0, -2.0, 1.0
    fi[V_GHOST]["cby"], fi[V_GHOST]["dcbydy"] = 1.0, 2.0
    return fi


def handmade_field():
    """0: B == 0 in its voxel; 1: u == 0; 2: u exactly along B, perp2 < 0 before the clamp; 3: u exactly opposite to B;
    4: U_PERP == 0.75 (a bin edge) and U_PAR == 0.5 (a range's hi); 5: a dead slot; 6: a ghost voxel; 7: i == nv"""
    b = search_perp2_negative()
    half = np.float32(0.5) * b
    rows = [  # voxel,   dx,  dy,  dz,   ux,    uy,  uz
        (V_ZERO, 0.25, -0.5, 0.0, 1.0, 0.5, 0.0),
        (V_Z2, 0.5, 0.25, -0.75, 0.0, 0.0, 0.0),
        (V_ALONG, 0.0, 0.0, 0.0, half[0], half[1], half[2]),
        (V_345, 0.5, 0.0, 0.5, -0.75, 0.0, -1.0),
        (V_Z2, -0.5, 0.0, 0.5, 0.75, 0.0, 0.5),
        (-1, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0),
        (V_GHOST, 0.0, 0.5, 0.0, 0.0, 1.0, 0.0),
        (n_voxels(HAND_GRID), 0.0, 0.0, 0.0, 1.0, 0.0, 0.0),
    ]
    p = np.zeros(len(rows), particle_dtype())
    for k, (i, dx, dy, dz, ux, uy, uz) in enumerate(rows):
        p[k]["i"], p[k]["dx"], p[k]["dy"], p[k]["dz"], p[k]["ux"], p[k]["uy"], p[k]["uz"] = i, dx, dy, dz, ux, uy, uz
    p["tag"] = np.arange(len(rows)) + 1
    p["q"] = -0.01
    return p


UPLOADABLE = [0, 1, 2, 3, 4]          # an upload refuses a dead slot, a ghost voxel and i == nv


def test_handmade_coordinates():
    p, g, fi = handmade_field(), HAND_GRID, hand_interpolator()
    assert search_perp2_negative() is not None                            # the search found its particle
    c = {name: field_coordinate(p, g, fi, name) for name in FIELD_NAMES}
    nan = np.isnan
    # 0: B == 0: B is 0 and the other five are NaN
    assert c["b"][0] == 0.0 and all(nan(c[n][0]) for n in FIELD_NAMES if n != "b")
    # 1: u == 0 in B = (0, 0, 2), ez = 0.5
    assert (c["b"][1], c["u_par"][1], c["u_perp"][1], c["mu"][1], c["e_par"][1]) == (2.0, 0.0, 0.0, 0.0, 0.5) and nan(c["cos_pitch"][1])
    # 2: along B: perp2 < 0 before the clamp, so U_PERP and MU are exactly 0; the rest by a scalar restatement
    assert perp2_of(p[[2]], g, fi)[0] < 0.0
    bx, by, bz = (float(fi[V_ALONG][n]) for n in ("cbx", "cby", "cbz"))
    ux, uy, uz = (float(p[2][n]) for n in ("ux", "uy", "uz"))
    b = math.sqrt((bx * bx + by * by) + bz * bz)
    u_par = ((ux * bx + uy * by) + uz * bz) / b
    assert (c["b"][2], c["u_par"][2], c["u_perp"][2], c["mu"][2], c["e_par"][2]) == (b, u_par, 0.0, 0.0, 0.0)
    assert c["cos_pitch"][2] == u_par / math.sqrt((ux * ux + uy * uy) + uz * uz)
    # 3: opposite to B = (3, 0, 4), u = -B / 4, E = (1, 0, 0)
    assert (c["b"][3], c["u_par"][3], c["u_perp"][3], c["cos_pitch"][3], c["mu"][3], c["e_par"][3]) == (5.0, -1.25, 0.0, -1.0, 0.0, 0.6)
    # 4: u = (0.75, 0, 0.5) in B = (0, 0, 2): u2 = 0.8125, perp2 = 0.5625
    assert (c["b"][4], c["u_par"][4], c["u_perp"][4], c["mu"][4], c["e_par"][4]) == (2.0, 0.5, 0.75, 0.140625, 0.5)
    assert c["cos_pitch"][4] == 0.5 / math.sqrt(0.8125)
    # 6: the ghost voxel's own record: B = (0, 2, 0), u along it
    assert (c["b"][6], c["u_par"][6], c["u_perp"][6], c["cos_pitch"][6], c["mu"][6], c["e_par"][6]) == (2.0, 1.0, 0.0, 1.0, 0.0, 0.0)
    # 5, 7: not live
    assert all(nan(c[n][5]) and nan(c[n][7]) for n in FIELD_NAMES)


def test_handmade_particles_take_every_branch():
    p, g, fi = handmade_field(), HAND_GRID, hand_interpolator()

    def check(desc, want, want_stats):
        got, stats = distribution_ref(p, g, fi, desc, stats=True)
        want = np.array(want, np.uint64)
        assert got.dtype == np.uint64 and got.shape == want.shape
        assert np.array_equal(got, want), (desc, got)
        assert stats == want_stats and int(got.sum()) == stats[2]

    def kept(**desc):
        return list(select_ref(p, g, fi, desc)[0])

    live = [0, 1, 2, 3, 4, 6]
    assert kept() == live
    # B: particle 0 (B == 0) on lo of the first bin; 2.0 on an edge (bin 2; particle 2's 2.2096 too); 5.0 on lo + n d: not counted
    check(dict(axes=[("b", 0.0, 1.0, 5)]), [1, 0, 4, 0, 0], (6, 6, 5))
    # U_PERP: particle 0's NaN is in no bin; 0.75 exactly on the edge of bin 3
    check(dict(axes=[("u_perp", 0.0, 0.25, 4)]), [4, 0, 0, 1], (6, 6, 5))
    # PITCH: NaN for particles 0 (B == 0) and 1 (u == 0); -1 on lo; +1 on lo + n d: not counted, nor is particle 2, whose
    # quotient is 1 + 2^-52: nothing clamps it
    assert field_coordinate(p, g, fi, "cos_pitch")[2] == 1.0 + 2.0 ** -52
    check(dict(axes=[("cos_pitch", -1.0, 0.5, 4)]), [1, 0, 0, 1], (6, 6, 2))
    # a NaN is kept by no range, not even (-inf, inf): particle 0 for every coordinate but B, particle 1 for PITCH
    for name in FIELD_NAMES:
        want = live if name == "b" else [1, 2, 3, 4, 6] if name != "cos_pitch" else [2, 3, 4, 6]
        assert kept(select=[(name, -INF, INF)]) == want, name
    # U_PAR: 0.5 exactly on a range's hi is out, on its lo is in
    assert kept(select=[("u_par", 0.0, 0.5)]) == [1] and kept(select=[("u_par", 0.5, 1.0)]) == [4]
    # MU == 0 for u == 0, along, opposite, and the ghost
    assert kept(select=[("mu", 0.0, 0.140625)]) == [1, 2, 3, 6] and kept(select=[("mu", 0.140625, INF)]) == [4]
    # E_PAR with a box-frame range and a tag condition beside it
    assert kept(select=[("e_par", 0.5, 0.6)]) == [1, 4] and kept(select=[("e_par", 0.5, 0.7), ("ux", -1.0, 0.5)], tag_every=(2, 0)) == [1, 3]
    # two axes, counts[b1][b0]: U_PAR (4 bins of 0.75 from -1.5) x B (3 bins of 2 from 0.5)
    want = np.zeros((3, 4), np.uint64)
    want[2, 0] = 1          # particle 3: U_PAR -1.25 -> 0, B 5 -> 2
    want[0, 2] = 2          # particles 1 and 4: U_PAR 0 and 0.5 -> 2, B 2 -> 0
    want[0, 3] = 2          # particle 2 (U_PAR 1.1048, B 2.2096) and the ghost (U_PAR 1, B 2)
    check(dict(axes=[("u_par", -1.5, 0.75, 4), ("b", 0.5, 2.0, 3)]), want, (6, 6, 5))


def test_generated_inputs_populate_what_the_gpu_test_relies_on():
    p, fi = generated_inputs(), generated_interpolator()
    c = {name: field_coordinate(p, GRID, fi, name) for name in FIELD_NAMES}
    assert not np.any(perp2_of(p, GRID, fi) < 0) and not np.any(c["b"] == 0)
    assert all(np.all(np.isfinite(v)) for v in c.values())
    assert np.all(np.abs(c["cos_pitch"]) < 1.0)
    counts, (seen, kept, counted) = distribution_ref(p, GRID, fi, dict(axes=[("u_par", -0.15, 0.3 / 128, 128), ("u_perp", 0.0, 0.15 / 96, 96)]), stats=True)
    assert (seen, kept, counted, int(np.count_nonzero(counts)), counts.size) == (N, N, 541084, 11684, 12288)
    as_axis, as_range = set(), set()
    for name, desc in descriptors().items():
        counts, (seen, kept, counted) = distribution_ref(p, GRID, fi, desc, stats=True)
        print(f"({name}) seen {seen} kept {kept} counted {counted}, non-empty {np.count_nonzero(counts)} of {counts.size}")
        assert seen == N and int(counts.sum()) == counted
        assert 0.02 * N < counted < 0.98 * N, name                         # a non-trivial share in, a non-trivial share out
        assert np.count_nonzero(counts) > counts.size // 2, name
        if "select" in desc:
            assert 0.02 * N < kept < 0.9 * N, name
        else:
            assert kept == N
        assert not any("log10_ke" in (a[0],) for a in desc["axes"] + desc.get("select", []))
        as_axis |= {a[0] for a in desc["axes"]}
        as_range |= {r[0] for r in desc.get("select", [])}
    for name, (desc, want) in selections().items():
        index = select_ref(p, GRID, fi, desc)[0]
        print(f"{name}: {len(index)} kept of {N}")
        assert len(index) == want, name
        as_range |= {r[0] for r in desc["select"]}
    assert as_axis >= set(FIELD_NAMES) and as_range >= set(FIELD_NAMES)
    # what a histogram keeps under a range is what a selection by the same range keeps
    assert distribution_ref(p, GRID, fi, dict(axes=[("ux", -1.0, 2.0, 1)], select=selections()["b"][0]["select"]), stats=True)[1][1] == selections()["b"][1]
    # the b selection: the double norm of the float fields lies in the range
    index, _, f = select_ref(p, GRID, fi, selections()["b"][0])
    bx, by, bz = (f[:, k].astype(np.float64) for k in (3, 4, 5))
    norm = np.sqrt((bx * bx + by * by) + bz * bz)
    assert np.all((norm >= B_RANGE[0]) & (norm < B_RANGE[1]))


def test_header_compiles_as_c11_and_constants(tmp_path):
    src = ('#include "vpic_hip.h"\n'
           '_Static_assert(VPIC_HIP_COORD_U_PAR == 16 && VPIC_HIP_COORD_E_PAR == 21 && VPIC_HIP_COORD_LOG10_KE == 7, "codes");\n'
           '_Static_assert(VPIC_HIP_COORD_U_PERP == 17 && VPIC_HIP_COORD_PITCH == 18 && VPIC_HIP_COORD_MU == 19 && VPIC_HIP_COORD_B == 20, "codes");\n'
           '_Static_assert(sizeof(vpic_hip_dist_t) == 152 && sizeof(vpic_hip_select_t) == 136 && sizeof(vpic_hip_dist_axis_t) == 24\n'
           '               && sizeof(vpic_hip_dist_range_t) == 24, "sizes");\n'
           'int main(void){ vpic_hip_dist_t d = {1, 1, {{VPIC_HIP_COORD_PITCH, 8, -1.0, 0.25}}, {{VPIC_HIP_COORD_MU, 0, 0.0, 1.0}}};\n'
           '  return d.axis[0].coord == 18 && d.sel[0].coord == 19 ? 0 : 1; }\n')
    exe = str(tmp_path / "fieldcoord_hdr_test")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-x", "c", "-", "-o", exe],
                   input=src.encode(), check=True)
    subprocess.check_call([exe])


def test_python_names():
    eng = importlib.import_module("old-vpic_amd.engine")
    assert eng.FIELD_COORDS == {name: 16 + k for k, name in enumerate(FIELD_NAMES)}
    assert tuple(sorted(eng.DIST_COORDS, key=eng.DIST_COORDS.get)) == COORDS and len(eng.DIST_COORDS) == 8
    assert C.sizeof(eng.DistDesc) == 152 and C.sizeof(eng.SelectDesc) == 136
    d = eng.dist_desc([("u_par", -1.0, 0.02, 100), ("u_perp", 0.0, 0.01, 100)], [("z", 60, 68), ("e_par", -1.0, 1.0)])
    assert (d.axis[0].coord, d.axis[1].coord, d.sel[0].coord, d.sel[1].coord, d.sel[1].hi) == (16, 17, 2, 21, 1.0)
    s = eng.select_desc([("ke", 0.5, INF), ("cos_pitch", 0.9, 1.0), ("mu", 0.0, 1.0), ("b", 0.0, 1.0)])
    assert [s.sel[k].coord for k in range(4)] == [6, 18, 19, 20]
    for make in (lambda: eng.dist_desc([("gyrophase", 0.0, 1.0, 4)]), lambda: eng.select_desc([("gyrophase", 0.0, 1.0)]),
                 lambda: eng.dist_desc([("pitch", 0.0, 1.0, 4)]), lambda: eng.select_desc([("pitch", 0.0, 1.0)])):      # (the bare word stays unknown)
        try:
            make()
        except KeyError:
            continue
        raise AssertionError("an unknown name was accepted")
    text = open(os.path.join(ROOT, "include", "vpic_hip.h")).read()
    assert "VPIC_HIP_COORD_U_PAR = 16" in text
