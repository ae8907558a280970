"""The HIP field solver (fields.hip through the C ABI) against the CPU oracle on the chain of oracle/field_chain.py: every
kind of field wall (PEC, symmetric, PMC, absorbing) on every face -- one axis at a time, a different kind at each end of
every axis, all six faces -- on grids with axes one cell thick in every position, an x extent across a wavefront and the
64-wide tile, a face of three blocks, and boxes one past a tile and longer than one 32-plane z sweep.  The oracle runs
live beside the engine (tests/test_oracle_field_walls.py pins it on the reference for exactly these runs, bit for bit).
GPU box only.

Every stage starts from the oracle's previous stage, so one difference cannot mask the next.  Criteria (the rules in the
header of test_gpu_kernels.py):
  per-voxel stages                         every component np.array_equal to the oracle's, ghosts included (equal as
                                           numbers: the sign of a zero ghost may differ, as K5 notes)
  rhof after accumulate_rho_p, the 14      within ACC_TOL = 2e-6 of the largest reference entry of the component (float sums
  moments after accumulate_hydro_p         in another order); every other component exact
  energy_f, the two rms, tang-E/norm-B     rel 1e-12 (double sums in another order)

Per case: damp 0 and 0.01; VPIC_HIP_FIELD_TILES 0 and 2 for advance_b / advance_e and VPIC_HIP_UNLOAD_TILED 0 and 2 for
clear_jf + unload (the only kernels that read either knob; the stages after them run once per damp); advance_e in one call
and as advance_e_part(1) + advance_e_part(2); clear_jf + unload_accumulator as two calls and fused.  Three materials on
(6,5,4) and (5,3,1) (the tiled advance_e is for one material by design and leaves those to the per-voxel kernel).
The nine small grids take all 19 wall layouts, the three largest the mixed and the all-six ones (every kind on every face)."""
import functools
import importlib

import numpy as np
import pytest

from oracle import field_chain as FC

pytestmark = pytest.mark.gpu
ACC_TOL = 2e-6      # |a_hip - a_ref| <= ACC_TOL * max|a_ref|  (single accumulation pass; test_gpu_kernels.py)

CASES = [(d, w) for d in FC.GRIDS if d not in FC.LARGE_GRIDS for w in FC.WALLS] + \
        [(d, w) for d in FC.LARGE_GRIDS for w in FC.MIXED_WALLS + FC.ALL_SIX_WALLS]


@pytest.fixture(scope="module")
def V():
    v = importlib.import_module("old-vpic_amd")
    assert v.lib().vpic_hip_device_count() > 0, "no HIP device"
    return v


@functools.lru_cache(maxsize=2)
def inputs(dims, materials):
    return FC.inputs(dims, materials=materials)


class Run:
    """One (grid, walls, damp, materials): the oracle's arrays after every stage, and engines to run single stages from them."""

    def __init__(self, V, L, api, dims, fbc, damp, materials):
        self.V, self.L, self.dims, self.fbc, self.damp = V, L, dims, fbc, damp
        self.key = FC.run_key(dims, fbc, damp, materials)
        self.inp = inputs(dims, materials)
        og = api.grid(dims, fbc, damp)
        self.m = api.coefficients(og, FC.PROPS if materials else None)
        _, self.scalars, finite, self.ref = FC.record(api, dims, fbc, damp, materials, self.inp, keep=True)
        assert finite, self.key + ": an oracle output is not finite"

    def engine(self, monkeypatch, tiles):
        monkeypatch.setenv("VPIC_HIP_FIELD_TILES", tiles)
        monkeypatch.setenv("VPIC_HIP_UNLOAD_TILED", tiles)
        self.tiles = tiles
        g = self.V.make_grid(*self.dims, *FC.box(self.dims), FC.DT, damp=self.damp, fbc=[int(b) for b in self.fbc], pbc=FC.pbc_for(self.fbc))
        e = self.V.Engine(g)
        e.set_material_coefficients(self.m)
        return e

    def same(self, got, stage, what="", skip=()):
        ref = self.ref[stage]
        for n in got.dtype.names:
            if n not in skip and not n.startswith("_"):
                if not np.array_equal(got[n], ref[n]):
                    bad = np.flatnonzero(got[n] != ref[n])
                    raise AssertionError(f"{self.key} tiles={self.tiles}: stage {stage}{what}, component {n}: {len(bad)} entries differ, "
                                         f"first at voxel {bad[0]}: {got[n][bad[0]]!r} against {ref[n][bad[0]]!r}")

    def close_sum(self, got, stage, n):
        ref = self.ref[stage][n]
        err, scale = np.abs(got[n].astype(np.float64) - ref).max(), np.abs(ref).max()
        assert err <= ACC_TOL * scale, f"{self.key}: stage {stage}, component {n}: error {err:.3e} against scale {scale:.3e}"

    def scalar(self, got, k, stage):
        want = self.scalars[k:k + np.size(got)]
        assert np.all(np.abs(np.atleast_1d(got) - want) <= 1e-12 * np.abs(want)), f"{self.key}: stage {stage}: {got!r} against {want!r}"

    def field_advance(self, e):
        """Stages 2-5a: the kernels that have an LDS-tiled twin."""
        inp, ref = self.inp, self.ref
        e.set_fields(inp["f"]); e.advance_b(0.5); self.same(e.get_fields(), "advance_b_1")
        e.set_fields(ref["advance_b_1"]); e.advance_e(); self.same(e.get_fields(), "advance_e")
        e.set_fields(ref["advance_b_1"]); e.advance_e_part(1); e.advance_e_part(2)
        self.same(e.get_fields(), "advance_e", " (as part 1 + part 2)")
        e.set_fields(ref["advance_e"]); e.advance_b(0.5); self.same(e.get_fields(), "advance_b_2")
        e.set_accumulator(inp["a"])
        e.set_fields(ref["advance_b_2"]); e.clear_jf(); e.unload_accumulator(); self.same(e.get_fields(), "unload")
        e.set_fields(ref["advance_b_2"]); e.clear_jf_unload_accumulator(); self.same(e.get_fields(), "unload", " (fused)")

    def rest(self, e):
        """Stages 1 and 5b-17."""
        inp, ref, L = self.inp, self.ref, self.L
        e.set_fields(inp["f"]); e.load_interpolator(); self.same(e.get_interpolator(), "load_interpolator")
        e.set_fields(ref["unload"]); e.synchronize_jf(); self.same(e.get_fields(), "sync_jf")
        sp = e.new_species(FC.Q_M, len(inp["p"]), 64)
        e.set_particles(sp, inp["p"])
        e.set_fields(ref["sync_jf"]); e.clear_rhof(); e.accumulate_rho_p(sp)
        f = e.get_fields(); self.same(f, "rho_p", skip=("rhof",)); self.close_sum(f, "rho_p", "rhof")
        e.set_fields(ref["rho_p"]); e.synchronize_rho(); self.same(e.get_fields(), "sync_rho")
        e.set_fields(ref["sync_rho"]); e.compute_rhob(); self.same(e.get_fields(), "rhob")
        f = ref["rhob"].copy(); f["rhob"] *= np.float32(0.9)
        e.set_fields(f); e.compute_div_e_err(); self.same(e.get_fields(), "div_e")
        self.scalar(e.compute_rms_div_e_err(), 0, "div_e (rms)")
        e.set_fields(ref["div_e"]); e.clean_div_e(); self.same(e.get_fields(), "clean_e")
        e.set_fields(ref["clean_e"]); e.compute_div_b_err(); self.same(e.get_fields(), "div_b")
        self.scalar(e.compute_rms_div_b_err(), 1, "div_b (rms)")
        e.set_fields(ref["div_b"]); e.clean_div_b(); self.same(e.get_fields(), "clean_b")
        e.set_fields(ref["clean_b"]); e.compute_curl_b(); self.same(e.get_fields(), "curl_b")
        e.set_fields(ref["curl_b"]); err = e.synchronize_tang_e_norm_b(); self.same(e.get_fields(), "sync_te")
        self.scalar(err, 2, "sync_te (error)")
        e.set_fields(ref["sync_te"]); self.scalar(e.energy_f(), 3, "energy_f")
        e.set_interpolator(inp["fi"])
        junk = np.zeros(e.nv, L.hydro_t); junk["ke"] = 3.0
        e.set_hydro(junk); e.clear_hydro(); e.accumulate_hydro_p(sp)
        h = e.get_hydro()
        for n in h.dtype.names[:-1]:
            self.close_sum(h, "hydro_p", n)
        e.set_hydro(ref["hydro_p"]); e.synchronize_hydro(); self.same(e.get_hydro(), "sync_hydro")


@pytest.mark.parametrize("dims,fbc", CASES, ids=[FC.grid_name(d) + "-" + FC.wall_name(w) for d, w in CASES])
def test_field_chain_against_the_oracle(V, L, orc, dims, fbc, monkeypatch):
    api = FC.orc_api()
    for materials in ((False, True) if dims in FC.MATERIAL_GRIDS else (False,)):
        for damp in FC.DAMPS:
            run = Run(V, L, api, dims, fbc, damp, materials)
            for tiles in ("0", "2"):
                e = run.engine(monkeypatch, tiles)
                run.field_advance(e)
                if tiles == "0":
                    run.rest(e)
                e.close()


def test_the_matrix_covers_every_kind_on_every_face():
    """Every (kind, face) pair on every grid with more than one cell along that face's axis -- and on the others as well."""
    assert len(CASES) == 9 * 19 + 3 * 7
    for dims in FC.GRIDS:
        walls = [w for d, w in CASES if d == dims]
        for kind in (FC.P, FC.S, FC.M, FC.A):
            for face in range(6):
                assert any(w[face] == kind for w in walls), (dims, kind, face)
        assert any(w[a] != w[a + 3] for w in walls for a in range(3))
