"""The selected particles of a species (include/vpic_hip.h: vpic_hip_species_select), restated in numpy: what the GPU
tests hold the kernels to.  Checked here, without a GPU, on hand-made particles that sit on every branch of the rules,
and on the generated inputs of tests/test_gpu_select.py, whose selections must be neither empty nor everything -- the
counts below were computed on the CPU when the feature was specified and are asserted, so a change of the inputs cannot
quietly empty a selection; plus the C side of the new ABI (the header as C11, the struct's size, the symbol list).

Coordinates are test_distribution_ref.coordinate (float64, every operation correctly rounded: bit for bit the
device's, log10 apart -- and no selection here uses LOG10_KE).  Tags use % on int64, whose result has the sign of the
divisor: the header's non-negative remainder.  The fields at the particle are float32 arrays, one numpy operation per
rounding, in the order the header writes them."""
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

from test_distribution_ref import COORDS, GRID, HAND_GRID, N, SEED, VTH, coordinate, dist_inputs, handmade  # noqa: E402
from test_spectrum_ref import voxel  # noqa: E402

INF = float("inf")


def interpolator_dtype():
    return importlib.import_module("old-vpic_amd.layout").interpolator_t


def fields_ref(p, fi):
    """float32[n, 6]: ex, ey, ez, cbx, cby, cbz at every particle of p (all in voxels of fi)"""
    f = fi[p["i"]]
    dx, dy, dz = p["dx"], p["dy"], p["dz"]
    assert dx.dtype == np.float32 and f["ex"].dtype == np.float32
    out = np.zeros((len(p), 6), np.float32)
    out[:, 0] = (f["ex"] + dy * f["dexdy"]) + dz * (f["dexdz"] + dy * f["d2exdydz"])
    out[:, 1] = (f["ey"] + dz * f["deydz"]) + dx * (f["deydx"] + dz * f["d2eydzdx"])
    out[:, 2] = (f["ez"] + dx * f["dezdx"]) + dy * (f["dezdy"] + dx * f["d2ezdxdy"])
    out[:, 3] = f["cbx"] + dx * f["dcbxdx"]
    out[:, 4] = f["cby"] + dy * f["dcbydy"]
    out[:, 5] = f["cbz"] + dz * f["dcbzdz"]
    return out


def keep_mask(p, grid, desc):
    """bool[len(p)]: which slots of the array hold a kept particle; desc = dict(select=[(coord, lo, hi), ...],
    tag_range=(lo, hi), tag_every=(every, phase)), every key optional.  The rules are applied to the vpic_hip_select_t
    that engine.select_desc makes of desc -- the numbers the library is handed, not the words of the test."""
    eng = importlib.import_module("old-vpic_amd.engine")
    d = eng.select_desc(**desc)
    nx, ny, nz = grid
    nv = (nx + 2) * (ny + 2) * (nz + 2)
    keep = (p["i"] >= 0) & (p["i"] < nv)                          # live
    for k in range(d.n_sel):
        c = coordinate(p, grid, COORDS[d.sel[k].coord])
        with np.errstate(invalid="ignore"):
            keep &= (c >= d.sel[k].lo) & (c < d.sel[k].hi)        # (a NaN is in no range)
    tag = p["tag"].astype(np.int64)
    if d.flags & 1:                                               # VPIC_HIP_SELECT_TAG_RANGE
        keep &= (tag >= d.tag_lo) & (tag < d.tag_hi)
    if d.flags & 2:                                               # VPIC_HIP_SELECT_TAG_EVERY
        keep &= tag % np.int64(d.tag_every) == d.tag_phase
    assert not d.flags & ~3
    return keep


def select_ref(p, grid, fi, desc):
    """(index int64[n], particles particle_t[n], fields float32[n, 6]) of the kept particles, in array order"""
    index = np.flatnonzero(keep_mask(p, grid, desc)).astype(np.int64)
    kept = p[index]
    return index, kept, fields_ref(kept, fi)


def random_interpolator(seed, grid):
    """non-zero float32 values in every voxel and component, so that every term of the six formulas matters"""
    nx, ny, nz = grid
    nv = (nx + 2) * (ny + 2) * (nz + 2)
    rng = np.random.default_rng(seed)
    fi = np.zeros(nv, interpolator_dtype())
    for name in fi.dtype.names:
        if name != "_pad":
            v = rng.uniform(0.25, 2.0, nv) * rng.choice([-1.0, 1.0], nv)
            fi[name] = v.astype(np.float32)
    return fi


def selections(ke_max):
    """the selections of the GPU test, by name, with the number each keeps of the generated inputs"""
    return {
        "tail": (dict(select=[("ke", 0.012, INF)]), 23247),
        "box": (dict(select=[("x", 20.0, 52.0), ("z", 1.0, 4.0)]), 92945),
        "every": (dict(tag_every=(100, 7)), 5600),
        "tags": (dict(tag_range=(1000, 3000)), 2000),
        "mixed": (dict(select=[("x", 20.0, 52.0), ("ke", 0.004, INF)], tag_every=(7, 3)), 10088),
        "all": (dict(), N),
        "none": (dict(select=[("ke", 10.0 * ke_max, INF)]), 0),
    }


def generated_inputs():
    p = dist_inputs(SEED, N, VTH, GRID)
    p["tag"] = np.arange(N) + 1
    return p


# ---- hand-made particles ----
HAND_TAGS = [5, 10, -7, 99, 3, 20, -14, 1, 2]


def handmade_select():
    """the seven particles of test_distribution_ref.handmade (0: X == 0 exactly; 1: X == 3 exactly; 2: ke == 0; 3: a dead
    slot; 4: a ghost voxel; 5; 6), then 7: i == nv, not live; 8: a NaN momentum.  Tags HAND_TAGS."""
    nx, ny, nz = HAND_GRID
    p = np.concatenate([handmade(), np.zeros(2, handmade().dtype)])
    p[7]["i"], p[7]["ux"] = (nx + 2) * (ny + 2) * (nz + 2), 1.0
    p[8]["i"], p[8]["ux"], p[8]["dx"] = voxel(1, 1, 1, HAND_GRID), np.nan, 0.5
    p["tag"] = HAND_TAGS
    p["tag2"] = 1000 + np.arange(len(p))
    p["q"] = -0.01
    return p


def test_handmade_particles_take_every_branch():
    p, g = handmade_select(), HAND_GRID
    fi = random_interpolator(3, g)

    def kept(**desc):
        index, particles, fields = select_ref(p, g, fi, desc)
        assert particles.tobytes() == p[index].tobytes() and fields.shape == (len(index), 6)
        return list(index)

    # no condition: the live particles -- not the dead slot (3), not i == nv (7); the ghost voxel (4) and the NaN (8) are live
    assert kept() == [0, 1, 2, 4, 5, 6, 8]
    # X: particle 0 exactly on lo (kept), particle 1 exactly on hi (not kept), the ghost's X = -0.25 below
    assert kept(select=[("x", 0.0, 3.0)]) == [0, 2, 5, 6, 8]
    assert kept(select=[("x", -1.0, 0.0)]) == [4]
    # a NaN is in no range, however wide
    assert kept(select=[("ux", -INF, INF)]) == [0, 1, 2, 4, 5, 6]
    assert kept(select=[("ke", 0.0, INF)]) == [0, 1, 2, 4, 5, 6]
    # KE: particle 0 (ke == 0.5) on lo, particle 5 (ke == 2.25) on hi
    assert kept(select=[("ke", 0.5, 2.25)]) == [0]
    # tags: 5 at tag_lo (kept), 20 at tag_hi (not kept); the dead slot's 99 never
    assert kept(tag_range=(5, 20)) == [0, 1]
    assert kept(tag_range=(0, 100)) == [0, 1, 4, 5, 8]
    # a negative tag under tag_every: -7 % 7 == 0, -14 % 7 == 0, -7 % 5 == 3
    assert kept(tag_every=(7, 0)) == [2, 6]
    assert kept(tag_every=(5, 3)) == [2, 4]
    assert kept(tag_every=(1, 0)) == [0, 1, 2, 4, 5, 6, 8]
    # every condition must hold
    assert kept(select=[("x", 0.0, 3.0)], tag_range=(-10, 6), tag_every=(5, 0)) == [0]
    assert kept(select=[("x", 0.0, 3.0), ("uy", 0.25, 1.0)], tag_every=(5, 0)) == [0]
    check_fields_ref_is_the_header_s_arithmetic()


def check_fields_ref_is_the_header_s_arithmetic():
    """one particle by hand, in float32 scalars, one operation per line of the header"""
    g = HAND_GRID
    fi = random_interpolator(3, g)
    p = handmade_select()[[5]]
    p["dy"], p["dz"] = -0.375, 0.8125
    f = fi[p["i"][0]]
    dx, dy, dz = (np.float32(p[c][0]) for c in ("dx", "dy", "dz"))
    F = np.float32
    want = [F(F(f["ex"] + F(dy * f["dexdy"])) + F(dz * F(f["dexdz"] + F(dy * f["d2exdydz"])))),
            F(F(f["ey"] + F(dz * f["deydz"])) + F(dx * F(f["deydx"] + F(dz * f["d2eydzdx"])))),
            F(F(f["ez"] + F(dx * f["dezdx"])) + F(dy * F(f["dezdy"] + F(dx * f["d2ezdxdy"])))),
            F(f["cbx"] + F(dx * f["dcbxdx"])), F(f["cby"] + F(dy * f["dcbydy"])), F(f["cbz"] + F(dz * f["dcbzdz"]))]
    got = fields_ref(p, fi)
    assert got.dtype == np.float32 and got.shape == (1, 6)
    assert got[0].tobytes() == np.array(want, np.float32).tobytes()
    assert np.all(got != 0) and np.all(np.isfinite(got))
    # every one of the 18 components matters
    for name in fi.dtype.names:
        if name != "_pad":
            other = fi.copy()
            other[name] += np.float32(1.0)
            assert (fields_ref(p, other) != got).sum() == 1, name


def test_generated_inputs_keep_the_counts_the_gpu_test_relies_on():
    p = generated_inputs()
    ke = coordinate(p, GRID, "ke")
    fi = random_interpolator(4, GRID)
    for name, (desc, want) in selections(float(ke.max())).items():
        index, particles, fields = select_ref(p, GRID, fi, desc)
        print(f"{name}: {len(index)} kept of {N}")
        assert len(index) == want, name
        assert np.all(np.diff(index) > 0)
    # no ke within 1e-6 (relative) of an edge that a selection uses: nothing hangs on the last bit of a double
    for edge in (0.012, 0.004):
        margin = float(np.abs(ke / edge - 1.0).min())
        print(f"ke edge {edge}: nearest particle {margin:.3g} away (relative)")
        assert margin > 1e-6
    assert np.all(fields_ref(p[:1000], fi) != 0)


def test_header_compiles_as_c11_and_struct_size(tmp_path):
    src = ('#include "vpic_hip.h"\n_Static_assert(sizeof(vpic_hip_select_t) == 136, "size");\n'
           '_Static_assert(VPIC_HIP_SELECT_TAG_RANGE == 1 && VPIC_HIP_SELECT_TAG_EVERY == 2, "flags");\n'
           'int main(void){ vpic_hip_select_t s = {1, VPIC_HIP_SELECT_TAG_EVERY, {{VPIC_HIP_COORD_KE, 0, 0.5, 2.0}}, 0, 0, 100, 7};\n'
           '  /* the three declarations, with the argument lists the issue states (nothing is linked) */\n'
           '  int (*f)(vpic_hip_engine_t *, int, const vpic_hip_select_t *, int64_t, vpic_particle_t *, float *, int64_t *, int64_t *) = 0;\n'
           '  int (*c)(vpic_hip_engine_t *, int, const vpic_hip_select_t *, int64_t *) = 0;\n'
           '  int (*t)(vpic_hip_engine_t *, int64_t *) = 0;\n'
           '  __typeof__(&vpic_hip_species_select) f2 = f; __typeof__(&vpic_hip_species_select_count) c2 = c;\n'
           '  __typeof__(&vpic_hip_species_select_stats) t2 = t;\n'
           '  return !f2 && !c2 && !t2 && s.tag_every == 100 && s.tag_phase == 7 && sizeof(s.sel) == 96 ? 0 : 1; }\n')
    exe = str(tmp_path / "select_hdr_test")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-x", "c", "-", "-o", exe],
                   input=src.encode(), check=True)
    subprocess.check_call([exe])
    eng = importlib.import_module("old-vpic_amd.engine")
    assert C.sizeof(eng.SelectDesc) == 136
    assert (eng.SelectDesc.sel.offset, eng.SelectDesc.tag_lo.offset, eng.SelectDesc.tag_phase.offset) == (8, 104, 128)
    assert (eng.SELECT_TAG_RANGE, eng.SELECT_TAG_EVERY) == (1, 2)
    d = eng.select_desc([("ke", 0.5, INF), ("z", 60, 68)], tag_range=(3, 9), tag_every=(100, 7))
    assert (d.n_sel, d.flags, d.sel[0].coord, d.sel[0].lo, d.sel[1].coord, d.sel[1].hi) == (2, 3, 6, 0.5, 2, 68.0)
    assert (d.tag_lo, d.tag_hi, d.tag_every, d.tag_phase) == (3, 9, 100, 7)
    d = eng.select_desc()
    assert (d.n_sel, d.flags) == (0, 0)


def test_symbols_are_listed():
    lib_mod = importlib.import_module("old-vpic_amd._lib")
    for name in ("vpic_hip_species_select_count", "vpic_hip_species_select", "vpic_hip_species_select_stats"):
        assert name in lib_mod.EXPORTS, name
    eng = importlib.import_module("old-vpic_amd.engine")
    assert callable(eng.Engine.select) and callable(eng.Engine.select_count) and callable(eng.Engine.select_stats)
    assert eng.SelectResult._fields == ("count", "particles", "fields", "index")
