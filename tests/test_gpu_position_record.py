"""Position and cell of a particle live in one 16-byte record {dx, dy, dz, i} on the device (engine.h: ParticlesK).  The
layout is the engine's own business: what goes in through the C ABI comes back byte for byte, and one step of every
advance_p instance leaves every particle bit for bit the oracle's -- cell-crossers (one late 16-byte store each), reflected
ones (momenta negated in place), the appended share of a tile (a second base per workgroup) included.  GPU box only."""
import importlib

import numpy as np
import pytest

from conftest import bits_equal
from sort_ref import _records
from test_gpu_tiles import acc_close, hot_particles, random_interpolator, tile_key

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def V():
    v = importlib.import_module("old-vpic_amd")
    assert v.lib().vpic_hip_device_count() > 0, "no HIP device"
    return v


# ---- round trips through the C ABI ------------------------------------------------------------------------------------
RT_DIMS = (5, 6, 7)                                             # partial tiles on every axis


def _species(V, L, n, seed):
    nx, ny, nz = RT_DIMS
    rng = np.random.default_rng(seed)
    p = hot_particles(L, rng, nx, ny, nz, (n + nx * ny * nz - 1) // (nx * ny * nz))[:n].copy()
    p["tag"] = np.arange(n) + 1
    p["tag2"] = -(np.arange(n) + 7)
    e = V.Engine(V.make_grid(nx, ny, nz, float(nx), float(ny), float(nz), np.float32(0.3)))
    return e, e.new_species(-1.0, n + 100, 64), p


@pytest.mark.parametrize("n", [1, 63, 64, 65, 2049])
def test_set_get_round_trip(V, L, n):
    e, sp, p = _species(V, L, n, 1)
    e.set_particles(sp, p)
    assert e.np(sp) == n
    assert e.get_particles(sp).tobytes() == p.tobytes()
    e.close()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 2049])
def test_append_round_trip(V, L, n):
    """appended records land behind the ones that are there, whatever the alignment of the seam"""
    e, sp, p = _species(V, L, n + 66, 2)
    e.set_particles(sp, p[:n])
    e.append_particles(sp, p[n:n + 1])
    e.append_particles(sp, p[n + 1:])
    assert e.np(sp) == n + 66
    assert e.get_particles(sp).tobytes() == p.tobytes()
    e.close()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 2049])
def test_get_range_round_trip(V, L, n):
    """the four ends of a range: first or last record of a 64-record span, first or last of the array"""
    e, sp, p = _species(V, L, n, 3)
    e.set_particles(sp, p)
    firsts = sorted({0, n - 1, min(63, n - 1), min(64, n - 1), n // 2, max(n - 64, 0), max(n - 65, 0)})
    for first in firsts:
        for count in sorted({1, n - first, min(64, n - first), min(65, n - first), max((n - first) // 2, 1)}):
            got = e.get_particles_range(sp, first, count)
            assert got.tobytes() == p[first:first + count].tobytes(), (first, count)
    assert e.get_particles_range(sp, 0, n).tobytes() == p.tobytes()
    e.close()


# ---- one step of every advance_p instance against the oracle ----------------------------------------------------------
DIMS = (7, 9, 6)
INSTANCES = {
    #                  environment,                                                        q = 0, deterministic
    "tile":            ({"VPIC_HIP_WINDOW": "tile", "VPIC_HIP_TILE_COARSE": "0"}, False, False),
    "tile_only_stage": ({"VPIC_HIP_WINDOW": "tile", "VPIC_HIP_TILE_COARSE": "1", "VPIC_HIP_STAGE": "1"}, False, False),
    "chargeless":      ({"VPIC_HIP_WINDOW": "tile", "VPIC_HIP_TILE_COARSE": "0", "VPIC_HIP_STAGE": "1"}, True, False),
    "det_tile":        ({"VPIC_HIP_WINDOW": "tile", "VPIC_HIP_TILE_COARSE": "0"}, False, True),
    "row_narrow":      ({"VPIC_HIP_WINDOW": "narrow"}, False, False),
    "row_wide":        ({"VPIC_HIP_WINDOW": "wide"}, False, False),
}


def _setup(V, orc, L, monkeypatch, env, seed, ppc=20, chargeless=False):
    """reflecting walls in z (reflected crossers negate momenta in place), thermal spread 0.3 c: every pass, and every
    wavefront's last, partial pass, has cell-crossers"""
    for k in ("VPIC_HIP_WINDOW", "VPIC_HIP_TILE_COARSE", "VPIC_HIP_STAGE", "VPIC_HIP_SORT_IN_PUSH"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("VPIC_HIP_TAIL_SORT_MIN", "1")       # the appended particles are regrouped by tile: the first2 segment runs
    nx, ny, nz = DIMS
    kw = dict(pbc=[0, 0, L.REFLECT_PARTICLES, 0, 0, L.REFLECT_PARTICLES])
    rng = np.random.default_rng(seed)
    g = V.make_grid(nx, ny, nz, float(nx), float(ny), float(nz), np.float32(0.5), **kw)
    og = orc.make_grid(nx, ny, nz, float(nx), float(ny), float(nz), np.float32(0.5), **kw)
    fi = random_interpolator(orc, L, og, rng)
    p = hot_particles(L, rng, nx, ny, nz, ppc, vth=0.3)
    extra = hot_particles(L, rng, nx, ny, nz, 1, vth=0.3)[:37].copy()
    extra["tag"] = len(p) + 1 + np.arange(len(extra))
    if chargeless:
        p["q"] = 0
        extra["q"] = 0
    e = V.Engine(g)
    e.set_interpolator(fi)
    return e, og, fi, p, extra


def _check_state(got, ref, dims):
    nx, ny, nz = dims
    assert np.array_equal(got["i"], ref["i"])               # every live record's cell word is the oracle's cell
    for c in ("dx", "dy", "dz"):
        assert np.all(np.abs(got[c]) <= 1.0), c
    sy, sz = nx + 2, (nx + 2) * (ny + 2)
    z, r = np.divmod(got["i"], sz)
    y, x = np.divmod(r, sy)
    assert np.all((x >= 1) & (x <= nx) & (y >= 1) & (y <= ny) & (z >= 1) & (z <= nz))
    assert bits_equal(got, ref)


@pytest.mark.parametrize("name", list(INSTANCES))
def test_one_step_bit_for_bit(V, orc, L, monkeypatch, name):
    env, chargeless, det = INSTANCES[name]
    e, og, fi, p, extra = _setup(V, orc, L, monkeypatch, env, 17, chargeless=chargeless)
    if det:
        e.set_accumulation("deterministic")
    sp = e.new_species(-1.0, len(p) + 256, 4096)
    e.set_particles(sp, p)
    e.sort_p(sp)
    assert e.species_order(sp) == ("voxel" if name.startswith("row") else "tile")
    e.append_particles(sp, extra)                           # a few particles behind the sorted ones
    by_tag = lambda a: a[np.argsort(a["tag"], kind="stable")]
    ref = e.get_particles(sp)
    n = len(ref)
    assert n == len(p) + len(extra)
    pm = np.zeros(64, L.particle_mover_t)
    ref_a = np.zeros(og.nv, L.accumulator_t)
    assert orc.advance_p(ref, n, -1.0, pm, ref_a, fi, og) == 0
    crossed = np.count_nonzero(by_tag(ref)["i"] != by_tag(e.get_particles(sp))["i"])
    assert crossed > n // 20                                # (the case is about cell-crossers)
    e.clear_accumulators()
    assert e.advance_p(sp) == 0
    got = e.get_particles(sp)
    assert bits_equal(got[:len(p)], ref[:len(p)])           # the sorted part stays where it is, record for record
    _check_state(by_tag(got), by_tag(ref), DIMS)            # (the appended ones may have been regrouped among themselves)
    acc_close(e.get_accumulator(), ref_a)
    e.close()


def test_counting_push_then_sort_inside_the_push(V, orc, L, monkeypatch):
    """HIST followed by SORT: the counting push against the oracle, then the launch that writes every particle to its sorted
    place in the second buffer -- order and content of the new buffer, range by range."""
    env = {"VPIC_HIP_SORT_IN_PUSH": "1"}
    e, og, fi, p, _ = _setup(V, orc, L, monkeypatch, env, 19)
    nx, ny, nz = DIMS
    p["tag"] = 0                                            # (a tagged species sorts the ordinary way)
    e.set_sort_order("engine")
    sp = e.new_species(-1.0, 2 * len(p), 4096)
    e.set_particles(sp, p)
    e.sort_p(sp)
    assert e.species_order(sp) == "tile"
    pm = np.zeros(64, L.particle_mover_t)
    ref = e.get_particles(sp)
    ref_a = np.zeros(og.nv, L.accumulator_t)
    assert orc.advance_p(ref, len(ref), -1.0, pm, ref_a, fi, og) == 0
    V.lib().vpic_hip_species_sort_hint(e._h, sp)
    e.clear_accumulators()
    assert e.advance_p(sp) == 0                             # HIST: this push counts for the sort
    before = e.get_particles(sp)
    _check_state(before, ref, DIMS)
    acc_close(e.get_accumulator(), ref_a)
    e.profile_enable(True)
    e.clear_accumulators()
    assert e.sort_advance_p(sp) == 0                        # SORT
    assert e.profile_read_sorting()[1] == 1                 # ... inside the push
    got = e.get_particles(sp)
    kb = tile_key(before["i"].astype(np.int64), nx, ny, nz)
    counts = np.bincount(kb, minlength=kb.max() + 1)
    starts = np.concatenate([[0], np.cumsum(counts)])
    ref2 = before[np.argsort(kb, kind="stable")].copy()     # range k: the particles that were in key k before this push
    ref2_a = np.zeros(og.nv, L.accumulator_t)
    assert orc.advance_p(ref2, len(ref2), -1.0, pm, ref2_a, fi, og) == 0
    assert len(got) == len(ref2)
    for k in np.flatnonzero(counts):                        # (the order inside a cell is the atomics' order)
        lo, hi = starts[k], starts[k + 1]
        assert np.array_equal(_records(got[lo:hi]), _records(ref2[lo:hi])), k
    assert np.all(np.abs(np.stack([got["dx"], got["dy"], got["dz"]])) <= 1.0)
    acc_close(e.get_accumulator(), ref2_a)
    e.close()
