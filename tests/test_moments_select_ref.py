"""The hydro moments of a selection of a species (include/vpic_hip.h: vpic_hip_accumulate_hydro_p_select), restated as the
composition of two things the project already pins: which particles a descriptor keeps (test_fieldcoord_ref.keep_mask; the
tag rules are those of test_select_ref.keep_mask) and the oracle's accumulate_hydro_p (oracle.pyorc) on the kept rows.
tests/test_gpu_moments_select.py holds the kernels to it.

The deck is that of tests/test_gpu_moments.py -- a 10 x 7 x 3 grid, 24 particles in every cell (5040), random non-zero E
and B through the oracle's load_interpolator, tags 1..n -- with one change: q is drawn from the four values
{0.5, 0.75, 1.0, 1.5} x -0.01 instead of a continuum, so that every kept subset can hold a particle of the species' largest
|q| (0.015) and a species made of the kept particles alone has the fixed-point scale of the whole one: that is what lets
the GPU test compare deterministic sums bit for bit.

Checked here, without a GPU: that the parts add up (hydro(A) + hydro(not A) = hydro(all) within ACC_TOL); what the GPU
test rests on -- every selection that is neither "all" nor "empty" keeps at least 100 particles and leaves at least 100
out, contains a particle of |q| = 0.015, and the box takes particles from more than one tile with its edges inside tiles
and inside cells -- so that the GPU test cannot pass vacuously; and the C and the Python side of the new interface."""
import functools
import importlib
import inspect
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import test_gpu_moments as M  # noqa: E402  (the deck's constants and its particle generator; nothing here touches a GPU)
from test_fieldcoord_ref import field_coordinate, keep_mask  # noqa: E402
from test_select_ref import INF  # noqa: E402

ACC_TOL = M.ACC_TOL
GRID, N, SEED = M.GRID, M.N, M.SEED
Q_VALUES = (0.5, 0.75, 1.0, 1.5)
Q_TOP = np.float32(1.5) * np.float32(-0.01)                 # the species' largest |q|, as the particles hold it
TILE = 4                                                    # cells per edge of a tile (policy.h: TILE_EDGE)
BOX_X, BOX_Z = (2.5, 6.25), (0.5, 2.25)


def layout():
    return importlib.import_module("old-vpic_amd.layout")


def oracle_grid():
    L = layout()
    nx, ny, nz = GRID
    return M.oracle().make_grid(nx, ny, nz, float(nx), float(ny), float(nz), np.float32(0.02), **M.walls(L))


def discrete_charges(p, seed):
    """p with q drawn from Q_VALUES x -0.01"""
    rng = np.random.default_rng(seed)
    p["q"] = rng.choice(np.array(Q_VALUES, np.float32), len(p)) * np.float32(-0.01)
    return p


@functools.lru_cache(maxsize=None)
def inputs():
    """(fields, interpolator, particles) of the deck, computed once and left unchanged: the fields and the interpolator
    are those of test_gpu_moments.deck()"""
    L = layout()
    orc = M.oracle()
    og = oracle_grid()
    rng = np.random.default_rng(SEED)
    f = np.zeros(og.nv, L.field_t)
    for c in ("ex", "ey", "ez", "cbx", "cby", "cbz"):
        f[c] = (rng.standard_normal(og.nv) * 0.2).astype(np.float32)
    fi = np.zeros(og.nv, L.interpolator_t)
    orc.load_interpolator(fi, f, og)
    p = discrete_charges(M.make_particles(SEED + 1), SEED + 7)
    for a in (f, fi, p):
        a.setflags(write=False)
    return f, fi, p


def ke_of(p):
    ux, uy, uz = (p[c].astype(np.float64) for c in ("ux", "uy", "uz"))
    return np.sqrt(((1.0 + ux * ux) + uy * uy) + uz * uz) - 1.0


@functools.lru_cache(maxsize=None)
def ke_edge():
    """the 90th percentile of the inputs' kinetic energies"""
    return float(np.percentile(ke_of(inputs()[2]), 90.0))


def selections():
    """the selections of the CPU and the GPU test, by name (the arguments of Engine.select / Engine.accumulate_hydro_p)"""
    return {
        "all": dict(),
        "empty": dict(select=[("ke", 0.01, 0.01)]),                                       # lo == hi
        "box": dict(select=[("x", *BOX_X), ("z", *BOX_Z)]),
        "tail": dict(select=[("ke", ke_edge(), INF)]),
        "ke_pitch": dict(select=[("ke", 0.03, INF), ("cos_pitch", 0.2, 1.0)]),
        "mu_epar": dict(select=[("mu", 0.05, INF), ("e_par", -0.05, 0.3)]),
        "every": dict(tag_every=(16, 3)),
        "tags": dict(select=[("uz", 0.0, INF)], tag_range=(1000, 3000)),
    }


TRIVIAL = ("all", "empty")
USES_FIELDS = ("ke_pitch", "mu_epar")


def hydro_ref(p, fi, q_m=-1.0):
    """the oracle's accumulate_hydro_p of the rows p"""
    og = oracle_grid()
    h = np.zeros(og.nv, layout().hydro_t)
    p = np.array(p)
    if len(p):
        M.oracle().accumulate_hydro_p(h, p, len(p), q_m, np.array(fi), og)
    return h


def selected_hydro_ref(p, fi, desc):
    """(oracle hydro of the kept rows of p, the keep mask)"""
    keep = keep_mask(p, GRID, fi, desc)
    return hydro_ref(p[keep], fi), keep


def tile_of(p):
    """the tile index of every particle's cell"""
    L = layout()
    nx, ny, nz = GRID
    i = p["i"].astype(np.int64)
    sy, sz = nx + 2, (nx + 2) * (ny + 2)
    cz, cy, cx = i // sz, (i % sz) // sy, i % sy
    assert np.array_equal(L.voxel(cx, cy, cz, nx, ny, nz), i)
    ntx, nty = -(-nx // TILE), -(-ny // TILE)
    return (((cz - 1) // TILE) * nty + (cy - 1) // TILE) * ntx + (cx - 1) // TILE


def check_selection_is_usable(name, p, keep):
    """what the bit-for-bit comparison of the GPU test rests on, for one selection that is neither "all" nor "empty\""""
    kept = int(keep.sum())
    assert 100 <= kept <= len(p) - 100, (name, kept)
    assert np.any(p["q"][keep] == Q_TOP), name
    assert np.abs(p["q"]).max() == np.abs(Q_TOP)


def test_inputs_are_what_the_gpu_test_rests_on():
    _, fi, p = inputs()
    assert len(p) == N == 5040 and np.array_equal(p["tag"], np.arange(N) + 1)
    assert sorted(set(np.abs(p["q"]).tolist())) == [float(np.float32(v) * np.float32(0.01)) for v in Q_VALUES]
    top = GRID[0] + 2 + (GRID[0] + 2) * (GRID[1] + 2) + 1
    assert p["i"].max() < oracle_grid().nv - top                       # no particle in the skipped ghost voxels at the top
    sel = selections()
    assert set(sel) == {"all", "empty", "box", "tail", "ke_pitch", "mu_epar", "every", "tags"}
    for name, desc in sel.items():
        keep = keep_mask(p, GRID, fi, desc)
        print(f"{name}: {int(keep.sum())} kept of {N}")
        if name == "all":
            assert keep.all()
        elif name == "empty":
            assert not keep.any() and desc["select"][0][1] == desc["select"][0][2]
        else:
            check_selection_is_usable(name, p, keep)
    # the tail is the energetic tenth
    assert abs(int(keep_mask(p, GRID, fi, sel["tail"]).sum()) - N // 10) <= 1
    # the box: edges inside tiles (no multiple of 4) and inside cells (no integer), particles of more than one tile,
    # and cells that it cuts: particles of one cell on both sides
    for edge in BOX_X + BOX_Z:
        assert edge != int(edge) and 0 < edge
    keep = keep_mask(p, GRID, fi, sel["box"])
    assert len(set(tile_of(p[keep]).tolist())) >= 2
    cut = set(p["i"][keep].tolist()) & set(p["i"][~keep].tolist())
    assert len(cut) >= 10
    # the ranges in the frame of the local field see finite coordinates, and no edge has a particle within 1e-9 of it
    for name in USES_FIELDS + ("tail", "box", "tags"):
        for coord, lo, hi in sel[name]["select"]:
            c = field_coordinate(p, GRID, fi, coord)
            assert np.all(np.isfinite(c)), (name, coord)
            for edge in (lo, hi):
                if np.isfinite(edge) and name != "tail":
                    assert np.abs(c - edge).min() > 1e-9, (name, coord, edge)
    assert (keep_mask(p, GRID, fi, sel["every"]) == ((p["tag"] % 16) == 3)).all()


def test_the_parts_add_up():
    """hydro(A) + hydro(not A) = hydro(all), within ACC_TOL of each moment's largest entry, for every selection; the empty
    selection's moments are all zero and the full one's are the whole species'."""
    _, fi, p = inputs()
    whole = hydro_ref(p, fi)
    for name, desc in selections().items():
        inside, keep = selected_hydro_ref(p, fi, desc)
        outside = hydro_ref(p[~keep], fi)
        for c in M.moments(whole):
            total = inside[c].astype(np.float64) + outside[c]
            err, top = float(np.abs(total - whole[c]).max()), float(np.abs(whole[c]).max())
            print(f"{name} {c}: max error {err:.3e}, largest entry {top:.3e}, ratio {err / top:.2e}")
            assert top > 0 and err <= ACC_TOL * top, (name, c)
        if name == "empty":
            assert not M.hydro_bits(inside).any()
        elif name == "all":
            assert np.array_equal(M.hydro_bits(inside), M.hydro_bits(whole))
        else:
            assert np.abs(inside["rho"]).max() > 0 and np.abs(outside["rho"]).max() > 0


def test_header_compiles_as_c11_and_declares_the_call(tmp_path):
    src = ('#include "vpic_hip.h"\n'
           'int main(void){ vpic_hip_select_t s = {1, VPIC_HIP_SELECT_TAG_EVERY, {{VPIC_HIP_COORD_PITCH, 0, 0.9, 1.0}}, 0, 0, 100, 0};\n'
           '  int (*f)(vpic_hip_engine_t *, int, const vpic_hip_select_t *) = 0;\n'
           '  __typeof__(&vpic_hip_accumulate_hydro_p_select) f2 = f;   /* (nothing is linked) */\n'
           '  return !f2 && s.sel[0].coord == 18 ? 0 : 1; }\n')
    exe = str(tmp_path / "moments_select_hdr_test")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-x", "c", "-", "-o", exe],
                   input=src.encode(), check=True)
    subprocess.check_call([exe])


def test_symbol_is_declared_and_exported():
    lib_mod = importlib.import_module("old-vpic_amd._lib")
    assert "vpic_hip_accumulate_hydro_p_select" in lib_mod.EXPORTS
    text = open(os.path.join(ROOT, "include", "vpic_hip.h")).read()
    assert "int vpic_hip_accumulate_hydro_p_select(vpic_hip_engine_t *e, int sp, const vpic_hip_select_t *s);" in text
    assert hasattr(importlib.import_module("old-vpic_amd").lib(), "vpic_hip_accumulate_hydro_p_select")


def test_python_method_accepts_the_keywords():
    eng = importlib.import_module("old-vpic_amd.engine")
    prm = inspect.signature(eng.Engine.accumulate_hydro_p).parameters
    assert list(prm) == ["self", "sp", "select", "tag_range", "tag_every"]
    assert (prm["select"].default, prm["tag_range"].default, prm["tag_every"].default) == ((), None, None)
    assert list(inspect.signature(eng.Engine.select_count).parameters)[:5] == list(prm)     # the arguments of `select`

    class Recorder:
        """stands in for the library: records which entry point a call reaches"""
        def __init__(self):
            self.calls = []

        def __getattr__(self, name):
            def call(*args):
                self.calls.append((name, args))
                return 0
            return call

    e = eng.Engine.__new__(eng.Engine)
    e._l, e._h = Recorder(), None
    e.accumulate_hydro_p(2)
    assert [c[0] for c in e._l.calls] == ["vpic_hip_accumulate_hydro_p"] and e._l.calls[0][1] == (None, 2)
    e.accumulate_hydro_p(2, select=[("cos_pitch", 0.9, 1.0)], tag_every=(100, 7))
    name, args = e._l.calls[1]
    assert name == "vpic_hip_accumulate_hydro_p_select" and args[1] == 2
    d = args[2]._obj
    assert (d.n_sel, d.flags, d.sel[0].coord, d.sel[0].lo, d.tag_every, d.tag_phase) == (1, 2, 18, 0.9, 100, 7)
    e.accumulate_hydro_p(0, tag_range=(5, 9))
    assert e._l.calls[2][0] == "vpic_hip_accumulate_hydro_p_select" and e._l.calls[2][1][2]._obj.flags == 1
    try:
        e.accumulate_hydro_p(0, select=[("pitch", 0.0, 1.0)])          # (the bare word stays unknown)
    except KeyError:
        pass
    else:
        raise AssertionError("an unknown name was accepted")
    assert len(e._l.calls) == 3
