"""Cell distributions (include/vpic_hip.h: vpic_hip_cell_distribution), restated in float32 / float64 numpy: what
tests/test_gpu_cell_dist.py holds the kernels to.  Checked here, without a GPU,
  - on a hand-made 2 x 2 x 2 grid whose cells sit on every branch of the rules -- a value exactly on half a quantum both
    ways, t just below 2^32 and at it, negative values, a cell whose cb words are all zero (E_PAR_C is NaN: counted,
    refused, in no range), a coordinate exactly on a bin edge and on hi -- the expected numbers worked out by hand and by a
    scalar restatement in Python floats, asserted with ==;
  - against the C oracle's load_interpolator: EX_C .. BZ_C of the restatement are its ex, ey, ez, cbx, cby, cbz at every
    interior cell, bit for bit;
  - on the generated inputs of the GPU test, which must populate what that test relies on;
  - plus the C side of the new ABI.

Every operation behind a value is +, -, x, / or sqrt in the stated precision (float for the fields at the cell's centre,
double after), which numpy and the device both round correctly; rint is exact.  So nothing here needs a margin: the GPU
test compares with == and leaves no cell out."""
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

from oracle import field_chain as FC  # noqa: E402

L = importlib.import_module("old-vpic_amd.layout")

F32 = np.float32
TWO32 = 4294967296.0
LDS_WORDS = 8192                                                              # VPIC_HIP_DIST_LDS_BINS: 32-bit words of the LDS path
FIELD_WORDS = ("ex", "ey", "ez", "div_e_err", "cbx", "cby", "cbz", "div_b_err", "tcax", "tcay", "tcaz", "rhob", "jfx", "jfy", "jfz", "rhof")
HYDRO_WORDS = ("jx", "jy", "jz", "rho", "px", "py", "pz", "ke", "txx", "tyy", "tzz", "tyz", "tzx", "txy")
CENTRED = ("ex_c", "ey_c", "ez_c", "bx_c", "by_c", "bz_c", "jx_c", "jy_c", "jz_c")
DERIVED = ("e_c", "b_c", "e_par_c", "j_par_c", "jdote_c")
CODES = {"x": 64, "y": 65, "z": 66, "one": 127}                               # VPIC_HIP_CELL_*
CODES.update({n: 72 + w for w, n in enumerate(FIELD_WORDS)})
CODES.update({"hydro." + n: 88 + w for w, n in enumerate(HYDRO_WORDS)})
CODES.update({n: 104 + k for k, n in enumerate(CENTRED)})
CODES.update({n: 113 + k for k, n in enumerate(DERIVED)})
GRIDS = [(1, 1, 6), (3, 1, 1), (6, 5, 4), (67, 3, 2), (33, 17, 9), (130, 9, 65)]
assert all(g in FC.GRIDS for g in GRIDS)


def interior(dims):
    """(cx, cy, cz, v) of the interior cells, x fastest: the order of the items"""
    nx, ny, nz = dims
    cz, cy, cx = np.meshgrid(np.arange(1, nz + 1), np.arange(1, ny + 1), np.arange(1, nx + 1), indexing="ij")
    cx, cy, cz = cx.ravel(), cy.ravel(), cz.ravel()
    return cx, cy, cz, L.voxel(cx, cy, cz, nx, ny, nz)


def _centre4(a, v, s1, s2):
    w0, w1, w2, w3 = a[v], a[v + s1], a[v + s2], a[v + s1 + s2]
    return F32(0.25) * ((w3 + w0) + (w1 + w2))


def centred(f, dims, name):
    """float32: a field at the cell's centre by load_interpolator's expressions, every operation rounded once"""
    nx, ny, nz = dims
    sy, sz = nx + 2, (nx + 2) * (ny + 2)
    v = interior(dims)[3]
    kind, axis = name[0], "xyz".index(name[1])
    if kind == "b":
        a = np.ascontiguousarray(f["cb" + name[1]])
        return F32(0.5) * (a[v + (1, sy, sz)[axis]] + a[v])
    a = np.ascontiguousarray(f[("e" if kind == "e" else "jf") + name[1]])
    s1, s2 = ((sy, sz), (sz, 1), (1, sy))[axis]
    return _centre4(a, v, s1, s2)


def cell_coordinate(f, hydro, dims, name):
    """float64 values of one coordinate or factor for every interior cell"""
    cx, cy, cz, v = interior(dims)
    if name == "one":
        return np.ones(len(v))
    if name in ("x", "y", "z"):
        return ({"x": cx, "y": cy, "z": cz}[name] - 1).astype(np.float64) + 0.5
    if name in FIELD_WORDS:
        return f[name][v].astype(np.float64)
    if name.startswith("hydro."):
        assert name[6:] in HYDRO_WORDS
        return hydro[name[6:]][v].astype(np.float64)
    if name in CENTRED:
        return centred(f, dims, name).astype(np.float64)
    e = [centred(f, dims, n).astype(np.float64) for n in ("ex_c", "ey_c", "ez_c")]
    b = [centred(f, dims, n).astype(np.float64) for n in ("bx_c", "by_c", "bz_c")]
    j = [centred(f, dims, n).astype(np.float64) for n in ("jx_c", "jy_c", "jz_c")]
    with np.errstate(invalid="ignore", divide="ignore"):
        if name == "e_c":
            return np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
        b_c = np.sqrt((b[0] * b[0] + b[1] * b[1]) + b[2] * b[2])
        if name == "b_c":
            return b_c
        if name == "e_par_c":
            return ((e[0] * b[0] + e[1] * b[1]) + e[2] * b[2]) / b_c
        if name == "j_par_c":
            return ((j[0] * b[0] + j[1] * b[1]) + j[2] * b[2]) / b_c
    assert name == "jdote_c", name
    return (j[0] * e[0] + j[1] * e[1]) + j[2] * e[2]


def cell_distribution_ref(f, hydro, dims, desc, values=()):
    """(counts uint64, isums int64[n_val, ...], refused int64[n_val], (seen, kept, counted)) of the interior cells under
    desc = dict(axes=[(coord, lo, d, n), ...], select=[(coord, lo, hi), ...]) and values = [((factor, ...), quantum), ...]"""
    seen = int(np.prod(dims))
    keep = np.ones(seen, bool)
    for coord, lo, hi in desc.get("select", ()):
        assert coord != "one"
        c = cell_coordinate(f, hydro, dims, coord)
        with np.errstate(invalid="ignore"):
            keep &= (c >= lo) & (c < hi)
    ok = keep.copy()
    ts = []
    for coord, lo, d, n in desc["axes"]:
        assert coord != "one"
        with np.errstate(invalid="ignore"):
            t = (cell_coordinate(f, hydro, dims, coord) - lo) / d
            ok &= (t >= 0) & (t < n)
        ts.append(t)
    bins = [np.trunc(t[ok]).astype(np.int64) for t in ts]
    shape = tuple(a[3] for a in reversed(desc["axes"]))
    n0 = desc["axes"][0][3]
    flat = bins[0] if len(bins) == 1 else bins[1] * n0 + bins[0]
    n_bins = int(np.prod(shape))
    counts = np.bincount(flat, minlength=n_bins).astype(np.uint64).reshape(shape)
    isums = np.zeros((len(values), n_bins), np.int64)
    refused = np.zeros(len(values), np.int64)
    for k, (factors, quantum) in enumerate(values):
        fac = [cell_coordinate(f, hydro, dims, name)[ok] for name in tuple(factors) + ("one",) * (3 - len(factors))]
        with np.errstate(invalid="ignore", over="ignore"):
            t = ((fac[0] * fac[1]) * fac[2]) / quantum
            taken = np.abs(t) < TWO32                                         # (a NaN is refused)
        refused[k] = int((~taken).sum())
        np.add.at(isums[k], flat[taken], np.rint(t[taken]).astype(np.int64))  # rint: to nearest, ties to even
    return counts, isums.reshape((len(values),) + shape), refused, (seen, int(keep.sum()), int(ok.sum()))


def lds_words(desc, values):
    """32-bit LDS words the histogram and its sums take: a count and n_val 64-bit sums per bin"""
    return int(np.prod([a[3] for a in desc["axes"]])) * (1 + 2 * len(values))


# ---- generated inputs: the field chain's fields (random in every component, ghosts included) and a seeded hydro array ----
def generated_fields(dims):
    return FC.inputs(dims)["f"]


def generated_hydro(dims):
    rng = np.random.default_rng([FC.SEED, 14] + list(dims))
    h = np.zeros(L.nv(*dims), L.hydro_t)
    for c in HYDRO_WORDS:
        h[c] = rng.standard_normal(len(h)).astype(np.float32)
    return h


Q = 2.0 ** -20


def cases(dims):
    """The descriptors of the GPU test with their values, by name, for one grid (every case on every grid but map2d):
      profile     1-D z, one bin per cell, four values (cbx; ex_c; jdote_c; one): LDS
      pdf         1-D jdote_c, 512 bins, no values: LDS
      map2d       (130, 9, 65) only: x-z, one bin per cell, 8450 bins, two values (ey_c; rhof b_c): global adds
      hydro       1-D hydro.rho, 64 bins, values of three factors (hydro.jx bx_c one; hydro.ke hydro.ke one): LDS
      selected    1-D e_c of the cells inside ranges over b_c, x and hydro.rho together, three values
      refusing    1-D y, rhof at a quantum that refuses a good share of the cells beside one, which refuses none
      edge_lds / edge_global      1-D rhof at 8192 and 8193 bins, no values: 8192 words, the last size in LDS, and the first beyond
      edge_lds1 / edge_global1    1-D rhof with tcax at 2730 and 2731 bins: 8190 and 8193 words
    The four edge axes span [-8, 8): every cell is counted by each (a float32 normal deviate does not reach 8), so the
    pair's totals are identical."""
    nx, ny, nz = dims
    c = {
        "profile": (dict(axes=[("z", 0.0, 1.0, nz)]), [(("cbx",), Q), (("ex_c",), Q), (("jdote_c",), Q), (("one",), 1.0)]),
        "pdf": (dict(axes=[("jdote_c", -1.5, 3.0 / 512, 512)]), []),
        "hydro": (dict(axes=[("hydro.rho", -3.0, 6.0 / 64, 64)]), [(("hydro.jx", "bx_c", "one"), Q), (("hydro.ke", "hydro.ke", "one"), Q)]),
        "selected": (dict(axes=[("e_c", 0.0, 0.06, 40)],
                          select=[("b_c", 0.4, 1.4), ("x", 0.0, nx / 2 + 0.5), ("hydro.rho", -0.5, 1.5)]),
                     [(("e_par_c",), Q), (("j_par_c", "b_c"), Q), (("x", "y", "z"), 0.125)]),
        "refusing": (dict(axes=[("y", 0.0, 1.0, ny)]), [(("rhof",), 2.0 ** -33), (("one",), 1.0)]),
        "edge_lds": (dict(axes=[("rhof", -8.0, 16.0 / 8192, 8192)]), []),
        "edge_global": (dict(axes=[("rhof", -8.0, 16.0 / 8193, 8193)]), []),
        "edge_lds1": (dict(axes=[("rhof", -8.0, 16.0 / 2730, 2730)]), [(("tcax",), Q)]),
        "edge_global1": (dict(axes=[("rhof", -8.0, 16.0 / 2731, 2731)]), [(("tcax",), Q)]),
    }
    if tuple(dims) == (130, 9, 65):
        c["map2d"] = (dict(axes=[("x", 0.0, 1.0, nx), ("z", 0.0, 1.0, nz)]), [(("ey_c",), Q), (("rhof", "b_c"), Q)])
    return c


GLOBAL = ("map2d", "edge_global", "edge_global1")
REFUSING = "refusing"


@functools.lru_cache(maxsize=None)
def reference_of_the_inputs(dims):
    """{name: cell_distribution_ref(...)} of the generated inputs of one grid, computed once and left unchanged"""
    f, h = generated_fields(dims), generated_hydro(dims)
    out = {name: cell_distribution_ref(f, h, dims, desc, values) for name, (desc, values) in cases(dims).items()}
    for r in out.values():
        for a in r[:3]:
            a.setflags(write=False)
    return out


# ---- the hand-made grid ----
HAND_DIMS = (2, 2, 2)
U_AT, U_BELOW = 2.0 ** 30, 2.0 ** 30 - 64.0                                   # (float32 steps by 64 below 2^30)
HAND_RHOF = [0.125, 0.375, -0.375, -0.125, U_AT, U_BELOW, 0.75, 1.0]          # by cell, x fastest


def hand_voxel(cx, cy, cz):
    return int(L.voxel(cx, cy, cz, *HAND_DIMS))


def handmade_grid():
    """(f, hydro) on 2 x 2 x 2.  Cell k = (cx - 1) + 2 (cy - 1) + 4 (cz - 1).
    rhof: 0.125, 0.375, -0.375, -0.125 -- in quanta of 0.25, t = 0.5, 1.5, -1.5, -0.5: ties both ways and both signs --
      2^30 (t = 2^32: refused), 2^30 - 64 (t = 2^32 - 256, the float32 below: taken), 0.75, 1.0.
    cb: cbx = cby = 0, cbz = 2 everywhere but at cell 0's voxel and the one above it (0: cell 0 has B_C = 0, cell 4 has
      BZ_C = 0.5 (2 + 0) = 1); cell 7 has cbx = 3 at its voxel and the next in x and cbz = 4 at its voxel and the one
      above: B_C = 5 (cell 6, whose +x neighbour is cell 7's voxel, has BX_C = 1.5, BZ_C = 2: B_C = 2.5; cell 3, below
      cell 7, has BZ_C = 0.5 (4 + 2) = 3).
    ex = 1 at the four words of cell 7's EX_C, jfx = 2 at the same four: EX_C = 1, JX_C = 2, E_PAR_C = 3 / 5 = 0.6,
      J_PAR_C = 1.2, JDOTE_C = 2.  ey = 0.5 at cell 0's voxel only: EY_C = 0.125 there, so E is not zero where B is.
    hydro rho = cell number / 4 at the cell's voxel, jx = -1.5 at cell 3's."""
    nv = L.nv(*HAND_DIMS)
    sy, sz = 4, 16
    f, h = np.zeros(nv, L.field_t), np.zeros(nv, L.hydro_t)
    f["cbz"] = 2.0
    v0, v7 = hand_voxel(1, 1, 1), hand_voxel(2, 2, 2)
    f["cbz"][[v0, v0 + sz]] = 0.0
    f["cbx"][[v7, v7 + 1]] = 3.0
    f["cbz"][[v7, v7 + sz]] = 4.0
    f["ex"][[v7, v7 + sy, v7 + sz, v7 + sy + sz]] = 1.0
    f["jfx"][[v7, v7 + sy, v7 + sz, v7 + sy + sz]] = 2.0
    f["ey"][v0] = 0.5
    v = interior(HAND_DIMS)[3]
    f["rhof"][v] = HAND_RHOF
    h["rho"][v] = np.arange(8) / 4.0
    h["jx"][v[3]] = -1.5
    assert float(f["rhof"][v[5]]) == U_BELOW and float(f["rhof"][v[4]]) == U_AT
    return f, h


HAND_CASES = [
    (dict(axes=[("rhob", -1.0, 2.0, 1)]), [(("rhof",), 0.25), (("e_par_c",), 0.125), (("jdote_c", "one", "b_c"), 0.5), (("hydro.rho", "hydro.jx"), 2.0 ** -10)]),
    (dict(axes=[("x", 0.5, 1.0, 2), ("z", 0.0, 1.0, 2)]), [(("one",), 1.0), (("y", "rhof"), 0.25)]),
    (dict(axes=[("x", 0.5, 0.5, 2)], select=[("z", 0.0, 1.5)]), [(("b_c",), 0.5)]),
    (dict(axes=[("b_c", 0.0, 2.5, 2)], select=[("e_par_c", -1.0, 1.0)]), []),
    (dict(axes=[("hydro.rho", 0.0, 0.25, 8)], select=[("j_par_c", -1e300, 1e300), ("y", 0.5, 1.5)]), [(("jdote_c", "hydro.rho"), 2.0 ** -5)]),
]


def scalar_cell(f, h, k, name):
    """one coordinate of hand cell k, in NumPy float32 scalars and Python floats, operation by operation as the header states it"""
    cx, cy, cz = 1 + k % 2, 1 + (k // 2) % 2, 1 + k // 4
    v, sy, sz = hand_voxel(cx, cy, cz), 4, 16

    def four(a, s1, s2):
        return float(F32(0.25) * ((a[v + s1 + s2] + a[v]) + (a[v + s1] + a[v + s2])))

    def two(a, s):
        return float(F32(0.5) * (a[v + s] + a[v]))

    def over(a, d):
        return a / d if d != 0 else (math.nan if a == 0 or a != a else math.copysign(math.inf, a))

    ex, ey, ez = four(f["ex"], sy, sz), four(f["ey"], sz, 1), four(f["ez"], 1, sy)
    jx, jy, jz = four(f["jfx"], sy, sz), four(f["jfy"], sz, 1), four(f["jfz"], 1, sy)
    bx, by, bz = two(f["cbx"], 1), two(f["cby"], sy), two(f["cbz"], sz)
    b = math.sqrt((bx * bx + by * by) + bz * bz)
    table = {"one": 1.0, "x": (cx - 1) + 0.5, "y": (cy - 1) + 0.5, "z": (cz - 1) + 0.5,
             "ex_c": ex, "ey_c": ey, "ez_c": ez, "bx_c": bx, "by_c": by, "bz_c": bz, "jx_c": jx, "jy_c": jy, "jz_c": jz,
             "e_c": math.sqrt((ex * ex + ey * ey) + ez * ez), "b_c": b, "e_par_c": over((ex * bx + ey * by) + ez * bz, b),
             "j_par_c": over((jx * bx + jy * by) + jz * bz, b), "jdote_c": (jx * ex + jy * ey) + jz * ez}
    if name in table:
        return table[name]
    return float(h[name[6:]][v]) if name.startswith("hydro.") else float(f[name][v])


def scalar_distribution(f, h, desc, values):
    """cell_distribution_ref of the hand grid by the scalar restatement; Python's round() is to nearest, ties to even"""
    shape = tuple(a[3] for a in reversed(desc["axes"]))
    n0, n_bins = desc["axes"][0][3], int(np.prod(shape))
    counts, isums, refused = np.zeros(n_bins, np.uint64), np.zeros((len(values), n_bins), np.int64), np.zeros(len(values), np.int64)
    kept = 0
    for k in range(8):
        if not all(lo <= scalar_cell(f, h, k, c) < hi for c, lo, hi in desc.get("select", ())):
            continue
        kept += 1
        t = [(scalar_cell(f, h, k, c) - lo) / d for c, lo, d, n in desc["axes"]]
        if not all(0 <= tt < a[3] for tt, a in zip(t, desc["axes"])):
            continue
        b = int(t[0]) + (int(t[1]) * n0 if len(t) == 2 else 0)
        counts[b] += 1
        for j, (factors, quantum) in enumerate(values):
            fac = [scalar_cell(f, h, k, name) for name in tuple(factors) + ("one",) * (3 - len(factors))]
            tq = ((fac[0] * fac[1]) * fac[2]) / quantum
            if abs(tq) < TWO32:
                isums[j, b] += round(tq)
            else:
                refused[j] += 1
    return counts.reshape(shape), isums.reshape((len(values),) + shape), refused, (8, kept, int(counts.sum()))


def test_handmade_cells_take_every_branch():
    f, h = handmade_grid()
    d = HAND_DIMS
    # the coordinates by hand
    assert list(cell_coordinate(f, h, d, "x")) == [0.5, 1.5] * 4 and list(cell_coordinate(f, h, d, "z")) == [0.5] * 4 + [1.5] * 4
    assert list(cell_coordinate(f, h, d, "b_c")) == [0.0, 2.0, 2.0, 3.0, 1.0, 2.0, 2.5, 5.0]
    e_par = cell_coordinate(f, h, d, "e_par_c")
    assert np.isnan(e_par[0]) and list(e_par[1:7]) == [0.0] * 6 and e_par[7] == 0.6
    assert cell_coordinate(f, h, d, "ex_c")[7] == 1.0 and cell_coordinate(f, h, d, "jx_c")[7] == 2.0
    assert cell_coordinate(f, h, d, "jdote_c")[7] == 2.0 and cell_coordinate(f, h, d, "j_par_c")[7] == 1.2
    assert cell_coordinate(f, h, d, "ey_c")[0] == 0.125 and cell_coordinate(f, h, d, "e_c")[0] == 0.125     # E is not zero where B is
    # cell 7's ex words are neighbours of three other cells: one of cell 1's four, two of cell 3's and of cell 5's
    assert list(cell_coordinate(f, h, d, "ex_c")) == [0.0, 0.25, 0.0, 0.5, 0.0, 0.5, 0.0, 1.0]
    # the first case by hand: one bin holds all eight cells
    counts, isums, refused, stats = cell_distribution_ref(f, h, d, *HAND_CASES[0])
    assert list(counts) == [8] and stats == (8, 8, 8) and isums.dtype == np.int64 and isums.shape == (4, 1)
    # rhof in quanta of 0.25: 0.5 -> 0 and 1.5 -> 2 (ties to even, both ways), -1.5 -> -2, -0.5 -> -0, 2^32 refused, 2^32 - 256 taken, 3, 4
    t = cell_coordinate(f, h, d, "rhof") / 0.25
    assert list(t) == [0.5, 1.5, -1.5, -0.5, TWO32, TWO32 - 256.0, 3.0, 4.0] and list(np.rint(t[:4])) == [0.0, 2.0, -2.0, -0.0]
    assert int(isums[0, 0]) == 0 + 2 - 2 - 0 + (2 ** 32 - 256) + 3 + 4 and refused[0] == 1
    # e_par_c: NaN in cell 0 (counted above, refused here), 0 in six cells, 0.6 / 0.125 = 4.8 -> 5 in cell 7
    assert int(isums[1, 0]) == 5 and refused[1] == 1
    # jdote_c b_c: 2 x 5 = 10 in cell 7, 20 quanta; cell 0 has B_C = 0, a value of 0 and no NaN: taken
    assert int(isums[2, 0]) == sum(round(((scalar_cell(f, h, k, "jdote_c") * 1.0) * scalar_cell(f, h, k, "b_c")) / 0.5) for k in range(8))
    # (cell 1: 0.125 x 2 / 0.5 = 0.5 -> 0, a tie again; cell 3: 0.5 x 3 -> 3; cell 5: 0.5 x 2 -> 2; cell 7: 2 x 5 -> 20)
    assert refused[2] == 0 and int(isums[2, 0]) == 0 + 3 + 2 + 20
    # hydro.rho hydro.jx: only cell 3 has a jx: 0.75 x -1.5 = -1.125, a negative value, -1152 quanta of 2^-10
    assert int(isums[3, 0]) == -1152 and refused[3] == 0
    # a coordinate exactly on a bin edge: X = 0.5 and 1.5 with lo = 0.5, d = 1 give t = 0 and 1; four bins of two cells
    counts, isums, refused, stats = cell_distribution_ref(f, h, d, *HAND_CASES[1])
    assert counts.tolist() == [[2, 2], [2, 2]] and isums[0].tolist() == [[2, 2], [2, 2]] and stats == (8, 8, 8)
    assert refused.tolist() == [0, 0] and int(isums[1, 1, 0]) == 2 ** 31 + 4  # (y rhof of cell 4: 0.5 x 2^30 / 0.25 = 2^31 is taken; cell 6: 1.5 x 0.75 / 0.25 = 4.5 -> 4)
    # t == n is outside: with d = 0.5, X = 1.5 gives t = 2 = n; and Z = 1.5 lies ON hi of the range: only cells 0 and 2 are counted
    counts, isums, refused, stats = cell_distribution_ref(f, h, d, *HAND_CASES[2])
    assert list(counts) == [2, 0] and stats == (8, 4, 2) and int(isums[0, 0]) == 0 + 4
    # a NaN lies in no range: cell 0 is not kept; B_C = 5.0 has t = 2 = n: kept and not counted
    counts, isums, refused, stats = cell_distribution_ref(f, h, d, *HAND_CASES[3])
    assert stats == (8, 7, 6) and list(counts) == [4, 2]                      # (B_C = 2.5 lies ON the edge between the bins: the upper one)
    # a range as wide as the doubles still leaves the NaN out
    counts, isums, refused, stats = cell_distribution_ref(f, h, d, *HAND_CASES[4])
    assert stats == (8, 3, 3) and list(counts) == [0, 1, 0, 0, 1, 1, 0, 0] and list(isums[0]) == [0, 1, 0, 0, 0, 20, 0, 0]
    # every case against the scalar restatement, bin by bin
    for desc, values in HAND_CASES:
        got, want = cell_distribution_ref(f, h, d, desc, values), scalar_distribution(f, h, desc, values)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]) and got[3] == want[3], desc
    # every coordinate of every cell
    for name in CODES:
        a, b = cell_coordinate(f, h, d, name), np.array([scalar_cell(f, h, k, name) for k in range(8)])
        assert np.array_equal(a, b, equal_nan=True), name


def test_centred_fields_equal_the_oracle_s_interpolator_bit_for_bit():
    import oracle_engine
    eng = importlib.import_module("old-vpic_amd.engine")
    for dims in GRIDS[:5]:
        f = generated_fields(dims)
        oe = oracle_engine.OracleEngine(eng.make_grid(*dims, *FC.box(dims), FC.DT))
        oe.set_fields(f)
        oe.load_interpolator()
        fi = oe.fi
        v = interior(dims)[3]
        for name, member in zip(CENTRED[:6], ("ex", "ey", "ez", "cbx", "cby", "cbz")):
            got = centred(f, dims, name)
            assert got.dtype == np.float32 and got.tobytes() == np.ascontiguousarray(fi[member][v]).tobytes(), (dims, name)
        # the current takes E's expressions: jf in E's place gives the same bits
        swapped = f.copy()
        for a in "xyz":
            swapped["e" + a] = f["jf" + a]
        for a in "xyz":
            assert centred(f, dims, "j%s_c" % a).tobytes() == centred(swapped, dims, "e%s_c" % a).tobytes()


def test_generated_inputs_populate_what_the_gpu_test_relies_on():
    paths = set()
    for dims in GRIDS:
        ref = reference_of_the_inputs(dims)
        cells = int(np.prod(dims))
        for name, (desc, values) in cases(dims).items():
            counts, isums, refused, (seen, kept, counted) = ref[name]
            words = lds_words(desc, values)
            paths.add("lds" if words <= LDS_WORDS else "global")
            assert (words > LDS_WORDS) == (name in GLOBAL), name
            assert seen == cells and int(counts.sum()) == counted and kept <= seen
            if name == REFUSING:
                assert refused[1] == 0 and refused[0] <= counted
                if cells > 100:
                    assert 0.3 * counted < refused[0] < 0.9 * counted        # refuses a good share, not all
            else:
                assert not refused.any(), (dims, name)
            if name in ("profile", "map2d", "refusing") or name.startswith("edge"):
                assert counted == cells, (dims, name)                         # every cell is counted
            if name == "profile":
                assert np.array_equal(isums[3].astype(np.uint64), counts) and np.all(counts == dims[0] * dims[1])
            if cells > 1000:
                assert counted > 0.02 * cells, (dims, name)
                if name == "selected":
                    assert 0.05 * cells < kept < 0.6 * cells
                if name == "pdf":
                    assert 0.9 * cells < counted < cells and np.count_nonzero(counts) > 256
                for k in range(len(values)):
                    assert np.count_nonzero(isums[k]) > 0.4 * np.count_nonzero(counts), (dims, name, k)
        for a, b in (("edge_lds", "edge_global"), ("edge_lds1", "edge_global1")):
            assert np.array_equal(ref[a][1].sum(axis=1), ref[b][1].sum(axis=1)) and ref[a][3] == ref[b][3]
        assert lds_words(*cases(dims)["edge_lds"]) == 8192 and lds_words(*cases(dims)["edge_global"]) == 8193
        assert lds_words(*cases(dims)["edge_lds1"]) == 8190 and lds_words(*cases(dims)["edge_global1"]) == 8193
    assert paths == {"lds", "global"} and lds_words(*cases((130, 9, 65))["map2d"]) == 8450 * 5
    # the fields differ in the ghosts too: a wrong neighbour offset changes a centred field
    f = generated_fields((6, 5, 4))
    assert np.count_nonzero(f["ex"]) == len(f) and np.count_nonzero(f["cbz"]) == len(f)


def test_header_compiles_as_c11_and_enum_values(tmp_path):
    checks = " && ".join(f"VPIC_HIP_CELL_{n} == {v}" for n, v in (
        ("X", 64), ("Y", 65), ("Z", 66), ("F0", 72), ("F_EX", 72), ("F_DIV_E_ERR", 75), ("F_CBX", 76), ("F_TCAX", 80), ("F_RHOB", 83),
        ("F_JFX", 84), ("F_RHOF", 87), ("H0", 88), ("H_JX", 88), ("H_RHO", 91), ("H_KE", 95), ("H_TXY", 101), ("EX_C", 104), ("BX_C", 107),
        ("JX_C", 110), ("JZ_C", 112), ("E_C", 113), ("B_C", 114), ("E_PAR_C", 115), ("J_PAR_C", 116), ("JDOTE_C", 117), ("ONE", 127)))
    src = ('#include "vpic_hip.h"\n_Static_assert(' + checks + ', "constants");\n'
           'int main(void){ vpic_hip_dist_value_t v = {{VPIC_HIP_CELL_JDOTE_C, VPIC_HIP_CELL_ONE, VPIC_HIP_CELL_ONE}, 0, 1e-11};\n'
           '  int (*f)(vpic_hip_engine_t *, const vpic_hip_dist_t *, const vpic_hip_dist_value_t *, int, uint64_t *, int64_t *) = vpic_hip_cell_distribution;\n'
           '  int (*s)(vpic_hip_engine_t *, int64_t *) = vpic_hip_cell_distribution_stats; (void)f; (void)s;\n'
           '  return v.factor[0] == 117 ? 0 : 1; }\n')
    obj = str(tmp_path / "cell_dist_hdr_test.o")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-x", "c", "-", "-c", "-o", obj],
                   input=src.encode(), check=True)
    eng = importlib.import_module("old-vpic_amd.engine")
    names = dict(eng.CELL_COORDS)
    names.update(eng.CELL_FACTORS)
    assert names == CODES and "one" not in eng.CELL_COORDS
    # no particle code is a cell code
    assert not set(CODES.values()) & (set(eng.DIST_COORDS.values()) | set(eng.FIELD_COORDS.values()) | set(eng.VALUE_FACTORS.values()))
    d = eng.cell_dist_desc([("x", 0.0, 1.0, 6), ("hydro.rho", -1.0, 0.5, 4)], [("b_c", 0.0, 1.0)])
    assert (d.n_axes, d.n_sel, d.axis[0].coord, d.axis[1].coord, d.axis[1].n, d.sel[0].coord) == (2, 1, 64, 91, 4, 114)
    v, n = eng.cell_dist_values([(("jdote_c",), 1e-9), (("hydro.jx", "bx_c", "one"), 1e-11)])
    assert n == 2 and [list(x.factor) for x in v] == [[117, 127, 127], [88, 107, 127]] and v[1].quantum == 1e-11
    assert eng.cell_dist_values([])[1] == 0
    for bad in ("ux", "ke", "b", "e_par", "q", "hydro.ex", "hydro", "jf", "ex_C"):
        for make in (lambda n: eng.cell_dist_desc([(n, 0.0, 1.0, 2)]), lambda n: eng.cell_dist_desc([("x", 0.0, 1.0, 2)], [(n, 0.0, 1.0)]),
                     lambda n: eng.cell_dist_values([((n,), 1.0)])):
            try:
                make(bad)
            except KeyError:
                continue
            raise AssertionError("an unknown name was accepted: " + bad)
    for make in (lambda: eng.cell_dist_desc([("one", 0.0, 1.0, 2)]), lambda: eng.cell_dist_desc([("x", 0.0, 1.0, 2)], [("one", 0.0, 2.0)])):
        try:
            make()
        except KeyError:
            continue
        raise AssertionError('"one" was accepted as a coordinate')
    for bad in ([(("one",), 1.0)] * 5, [((), 1.0)], [(("x",) * 4, 1.0)]):
        try:
            eng.cell_dist_values(bad)
        except ValueError:
            continue
        raise AssertionError("a malformed value list was accepted")


def test_symbols_are_listed():
    lib_mod = importlib.import_module("old-vpic_amd._lib")
    for name in ("vpic_hip_cell_distribution", "vpic_hip_cell_distribution_stats"):
        assert name in lib_mod.EXPORTS, name
    eng = importlib.import_module("old-vpic_amd.engine")
    assert callable(eng.Engine.cell_distribution) and callable(eng.Engine.cell_distribution_stats)
    # the library exports them (built by build(); cross-compiled where there is no GPU)
    so = lib_mod.SO
    if os.path.exists(so):
        exported = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
        for name in ("vpic_hip_cell_distribution", "vpic_hip_cell_distribution_stats"):
            assert (" T " + name + "\n") in exported, name
