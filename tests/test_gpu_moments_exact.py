"""accumulate_hydro_p, accumulate_hydro_p_select and accumulate_rho_p against an exact reference, node by node (GPU box only).

The reference is tests/moments_exact.py: the oracle's two functions with their fixed-point switch on (pinned on the CPU by
tests/test_moments_exact_ref.py).  DETERMINISTIC mode: every word of all 14 moments over all nv voxels, ghosts included,
and every word of rhof, equals the finalized integer sums as uint32 -- no node, moment or case is left out.  FLOAT mode:
every word lies within the per-node bound derived in moments_exact.py's docstring (the error of a float sum of the node's
n contributions in any order or tree, the reference's own quantisation, one rounding); a node without contributions holds
zero.  The worst observed error / bound of each case is printed ("RATIO ..." lines) and is no threshold.

Decks (moments_exact.GRIDS): 10 x 9 x 7 (partial tiles on every axis), 4 x 4 x 4 (one tile), 5 x 3 x 2 and 16 x 1 x 6
(thinner than a tile: tile order only under VPIC_HIP_WINDOW=tile, as test_gpu_moments.py makes it), 65 x 5 x 4 (17 tiles
along x), and 10 x 9 x 7 with lengths (13, 4.5, 21.7) and c = 2; q_m = -1 and +1/25; charges of both signs and zero in one
species, offsets exactly -1, 0, +1, momenta of 1e-6, 0.3 and 30 (moments_exact.particles).

Array states and paths: "unsorted", "voxel", "tile" and "tile_only" (VPIC_HIP_TILE_COARSE=1, a fresh child process) as
tests/species_states.py builds them where it can (unit cells, q_m = -1); "untiled" (VPIC_HIP_MOMENTS_TILED=0, child) and
"per_particle" (VPIC_HIP_HYDRO_PER_PARTICLE / VPIC_HIP_RHO_PER_PARTICLE, child: the float paths) ; "sparse" (fewer than 4 nv
particles: the per-particle float path by the engine's own choice); "sort_first" (unsorted on an engine that wants tile
order: a deterministic call sorts by tile first); "tail_holes" (tile order, an appended tail, dead slots) and "stale" (six
pushes without a sort: particles outside their tile's window add through global memory).  Where a push has moved the
particles the reference is taken of what get_particles returns afterwards.

Further: two species and a repeated call into arrays cleared once (the += of the finalize step); the fixed-point scale
following the largest |q| that ever went into the species, host-made or emitted on the device; the moments of a selection
at the whole species' scale; synchronize_hydro on the finalized reference with ==."""
import functools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import moments_exact as X  # noqa: E402
import species_states as S  # noqa: E402
import test_gpu_moments as M  # noqa: E402
from moments_exact import L, pyorc  # noqa: E402
from species_states import package, run_child  # noqa: E402
from test_fieldcoord_ref import keep_mask  # noqa: E402

pytestmark = pytest.mark.gpu

CHILD_ENV = {"tile_only": dict(VPIC_HIP_TILE_COARSE="1"), "untiled": dict(VPIC_HIP_MOMENTS_TILED="0"),
             "per_particle": dict(VPIC_HIP_HYDRO_PER_PARTICLE="1", VPIC_HIP_RHO_PER_PARTICLE="1")}
IN_TILE_ORDER = ("tile", "tile_only", "untiled", "tail_holes", "stale")
WANTS_TILE = IN_TILE_ORDER + ("sort_first",)
STATES = ("unsorted", "voxel", "tile", "tile_only", "untiled", "per_particle", "sparse", "sort_first", "tail_holes", "stale")
HEAVY = 4.0                                              # the absorbed particle of "tail_holes": 4 x the largest |q| of the rest

# (grid, q_m, array state)
CASES = [("10x9x7", -1.0, s) for s in STATES] + [
    ("10x9x7", X.Q_MS[1], "tile"), ("10x9x7", X.Q_MS[1], "unsorted"), ("10x9x7", X.Q_MS[1], "sort_first"), ("10x9x7", X.Q_MS[1], "sparse"),
    ("4x4x4", -1.0, "tile"), ("4x4x4", -1.0, "unsorted"), ("4x4x4", X.Q_MS[1], "voxel"), ("4x4x4", X.Q_MS[1], "tile"),
    ("5x3x2", -1.0, "tile"), ("5x3x2", -1.0, "voxel"), ("5x3x2", X.Q_MS[1], "unsorted"), ("5x3x2", X.Q_MS[1], "sort_first"),
    ("16x1x6", -1.0, "tile"), ("16x1x6", -1.0, "unsorted"), ("16x1x6", X.Q_MS[1], "tile"), ("16x1x6", -1.0, "tile_only"),
    ("16x1x6", X.Q_MS[1], "voxel"),
    ("65x5x4", -1.0, "tile"), ("65x5x4", -1.0, "sort_first"), ("65x5x4", X.Q_MS[1], "unsorted"), ("65x5x4", X.Q_MS[1], "tile"),
    ("10x9x7-stretched", -1.0, "tile"), ("10x9x7-stretched", -1.0, "unsorted"), ("10x9x7-stretched", -1.0, "sort_first"),
    ("10x9x7-stretched", X.Q_MS[1], "tile"), ("10x9x7-stretched", X.Q_MS[1], "voxel"), ("10x9x7-stretched", X.Q_MS[1], "stale"),
    ("10x9x7-stretched", -1.0, "untiled"),
]


def case_id(c):
    return "%s-q_m%+.2f-%s" % c


@pytest.fixture(scope="module")
def V():
    return package()


def engine_for(V, grid, tile_knob, dt=X.DT, **walls):
    args, kw = X.grid_args(grid, dt, **walls)
    e = M.new_engine(V, V.make_grid(*args, **kw), tile_knob)
    e.set_vacuum()
    return e


def exchange_step(e, sp):
    """one push of the resident exchange: what reaches an absorbing wall leaves a dead slot"""
    e.clear_accumulators()
    e.exchange_begin()
    e.advance_p_async(sp)
    e.exchange_pack([0] * 6, [0] * 6, 8192)
    e.exchange_finish([])
    assert e.exchange_flags == 0 and e.nm(sp) == 0


def away_from_the_x_walls(p, grid):
    """p with |dx| <= 0.9 in the cells next to the x walls: none of them reaches an absorbing wall within two steps"""
    nx = X.dims_of(grid)[0]
    x = p["i"] % (nx + 2)
    p["dx"] = np.where((x == 1) | (x == nx), p["dx"] * np.float32(0.9), p["dx"])
    return p


def build(V, grid, q_m, state):
    """(engine, species, the largest |q| the host has put into the species, the grid's time step) in the array state asked
    for, the grid's random interpolator loaded.  species_states.build_state makes the states it can (unit cells, q_m = -1)."""
    dims, thin = X.dims_of(grid), grid in X.THIN
    fi = np.array(X.interpolator(grid))
    n = X.N_SPARSE if state == "sparse" else X.N_PARTICLES[grid]
    p = X.particles(41, n, grid)
    coarse = os.environ.get("VPIC_HIP_TILE_COARSE") == "1"
    shared = {"unsorted": "unsorted", "per_particle": "unsorted", "sparse": "unsorted", "voxel": "voxel", "tile": "tile",
              "untiled": "tile", "tile_only": "tile_only", "tail_holes": "tile_tail_holes"}
    if state in shared and X.GRIDS[grid][1] is None and q_m == -1.0:
        assert state != "tail_holes" or not thin
        tail = None
        if state == "tail_holes":
            p = away_from_the_x_walls(p, grid)
            tail = away_from_the_x_walls(X.particles(42, S.N_TAIL, grid, first_tag=2 * 10 ** 7), grid)
        with M.environment(**(dict(VPIC_HIP_WINDOW="tile") if thin and state in WANTS_TILE else {})):
            e, sp = S.build_state(V, shared[state], p, dims, tail, X.DT, 0.99, coarse=coarse)
        q_max = max(X.q_max_of(p), 0.01)                  # (the doomed particles of build_state carry -0.01)
        if state == "tail_holes":
            # one more absorbed particle, HEAVY times the largest |q| of all the others: Species::q_max keeps it
            q_max = max(q_max, X.q_max_of(tail))
            heavy = np.zeros(1, L.particle_t)
            heavy["i"], heavy["dx"], heavy["ux"] = L.voxel(dims[0], 1, 1, *dims), 0.99, 3.0
            heavy["q"], heavy["tag"] = np.float32(HEAVY * q_max), 3 * 10 ** 7
            e.append_particles(sp, heavy)
            exchange_step(e, sp)
            assert e.species_stats(sp)["dead_slots"] == S.N_DOOMED + 1 and e.np(sp) == n + S.N_TAIL
            q_max = float(heavy["q"][0])
        e.set_interpolator(fi)
        return e, sp, q_max, X.DT
    dt = X.DT
    if state == "stale":                                  # c dt = half the smallest cell: a fast particle crosses it in two pushes
        _, lengths, cvac = X.GRIDS[grid]
        dt = 0.5 * min(l / m for l, m in zip(lengths or dims, dims)) / cvac
    e = engine_for(V, grid, thin and state in WANTS_TILE, dt)
    e.set_interpolator(fi)
    sp = e.new_species(q_m, n + 4096, 4096)
    e.set_particles(sp, p)
    if state in WANTS_TILE:
        e.set_sort_order("engine")
    if state == "voxel":
        e.sort_p(sp)
        assert e.species_order(sp) == "voxel"
    if state in IN_TILE_ORDER:
        e.sort_p(sp)
        assert e.species_order(sp) == "tile" and e.species_stats(sp)["by_tile_only"] == (1 if coarse else 0)
    if state == "stale":
        e.clear_accumulators()
        for _ in range(6):
            e.advance_p(sp)
        assert e.species_order(sp) == "tile" and e.nm(sp) == 0 and e.species_stats(sp)["sorts"] == 1
    return e, sp, X.q_max_of(p), dt


def measure(e, sp, modes):
    """per mode: (hydro, its statistics, rhof, its statistics), each after a clear"""
    out = {}
    for mode in modes:
        e.set_accumulation(mode, X.Q0)
        h, hs = M.hydro_of(e, sp), e.moments_stats()
        r, rs = M.rho_of(e, sp), e.moments_stats()
        out[mode] = (h, hs, np.array(r), rs)
    return out


def check_words(what, mode, hydro, rhof, refs, prev_h=None, prev_r=None):
    """deterministic: every uint32 word of both arrays is the finalized reference (chained over refs onto prev);
    float: every word within the bound; prints the worst error / bound"""
    if mode == "deterministic":
        want_h, want_r = prev_h, prev_r
        for r in refs:
            want_h, want_r = r.hydro_words(want_h), r.rho_words(want_r)
        for got, want, rho in ((hydro, want_h, False), (rhof, want_r, True)):
            if got is not None:
                bad = X.describe_bad_words(got, want, refs, rho)
                assert bad is None, "%s deterministic %s\n%s" % (what, "rhof" if rho else "hydro", bad)
        return
    for got, rho in ((hydro, False), (rhof, True)):
        if got is not None:
            worst, words, bad = X.float_errors(got, refs, rho)
            print("RATIO %s float %s: worst error / bound %.4f over %d words" % (what, "rhof" if rho else "hydro", worst, words))
            assert bad is None, "%s float %s\n%s" % (what, "rhof" if rho else "hydro", bad)
            assert words == refs[0].og.nv * (1 if rho else 14)


def check_stats(what, state, mode, stats, n):
    """the path that was meant to run did (include/vpic_hip.h: vpic_hip_moments_stats)"""
    print("%s %s: statistics %s" % (what, mode, stats))
    assert stats[0] == n and stats[1] + stats[2] == n and stats[3] == 0, (what, mode, stats)
    tiled = state in ("tile", "tile_only") or (state == "sort_first" and mode == "deterministic")
    if tiled:
        assert stats[1] == n, (what, mode, stats)
    elif state == "tail_holes":
        assert stats[1] > 0 and stats[2] >= S.N_TAIL, (what, mode, stats)
    elif state == "stale":                                # both routes in use
        assert stats[1] > 0 and stats[2] > 0, (what, mode, stats)
    else:
        assert stats[2] == n, (what, mode, stats)


def run_case(V, case):
    grid, q_m, state = case
    what = case_id(case)
    e, sp, q_max, dt = build(V, grid, q_m, state)
    og = X.oracle_grid(grid, dt)
    # float first where the deterministic call sorts (by tile), deterministic first where the float call does (by voxel)
    modes = ("float", "deterministic") if state == "sort_first" else ("deterministic", "float")
    got = measure(e, sp, modes)
    if state == "sort_first":
        assert e.species_order(sp) == "tile", what
    if state in ("per_particle", "sparse"):
        assert e.species_order(sp) == "none", what         # nothing was sorted: not the path "cells"
    elif state in ("unsorted", "untiled"):
        assert e.species_order(sp) == "voxel", what        # the float path "cells" sorted by voxel
    back = e.get_particles(sp)                             # (last: a download drops the dead slots)
    e.close()
    n = len(back)
    assert n == (X.N_SPARSE if state == "sparse" else X.N_PARTICLES[grid]) + (S.N_TAIL if state == "tail_holes" else 0)
    assert (n < 4 * og.nv) == (state == "sparse")
    if state == "tail_holes":
        assert X.q_max_of(back) * HEAVY == q_max
    ref = X.Reference(og, back, q_m, X.interpolator(grid), q_max=q_max)
    for mode in modes:
        h, hs, r, rs = got[mode]
        check_stats(what + " hydro", state, mode, hs, n)
        check_stats(what + " rho", state, mode, rs, n)
        check_words(what, mode, h, r, [ref])
    if state == "tail_holes":
        # a second engine loaded with the survivors alone takes the finer scale, and equals ITS reference
        fine = X.Reference(og, back, q_m, X.interpolator(grid))
        assert np.array_equal(fine.m.scales, ref.m.scales * HEAVY)
        e = engine_for(V, grid, False, pbc=[L.ABSORB_PARTICLES, 0, 0, L.ABSORB_PARTICLES, 0, 0])
        e.set_interpolator(np.array(X.interpolator(grid)))
        e.set_sort_order("engine")
        sp = e.new_species(q_m, n + 64, 64)
        e.set_particles(sp, back)
        e.sort_p(sp)
        (h, hs, r, rs), = measure(e, sp, ("deterministic",)).values()
        e.close()
        assert hs == (n, n, 0, 0)
        check_words(what + " survivors alone", "deterministic", h, r, [fine])
        assert h.tobytes() != got["deterministic"][0].tobytes()
        assert r.tobytes() == got["deterministic"][2].tobytes()      # (rho's scale follows q_ref, not q_max)


def test_the_cases_cover_every_grid_species_and_state():
    assert len(set(CASES)) == len(CASES)
    assert {c[0] for c in CASES} == set(X.GRIDS) and {c[1] for c in CASES} == set(X.Q_MS) and {c[2] for c in CASES} == set(STATES)
    for grid in X.GRIDS:
        assert {c[1] for c in CASES if c[0] == grid} == set(X.Q_MS), grid
        assert {"tile", "unsorted"} <= {c[2] for c in CASES if c[0] == grid}, grid
        assert {"voxel", "sort_first"} & {c[2] for c in CASES if c[0] == grid}, grid
    for grid, _, state in CASES:
        assert X.N_PARTICLES[grid] + (S.N_TAIL + S.N_DOOMED + 1 if state == "tail_holes" else 0) <= 16000
        assert state not in ("tail_holes", "tile_only") or X.GRIDS[grid][1] is None     # species_states builds these


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_every_word_of_hydro_and_rho(V, case):
    """A species in one array state: deterministic hydro and rhof word for word, float hydro and rhof within the bound.
    "tail_holes" is also the rule of csrc/engine.h (Species::q_max) and include/vpic_hip.h: the fixed-point scale of the
    hydro moments follows the largest |q| the host has EVER put into the species, also after that particle has left --
    here an absorbed particle of 4 x the charge of the rest -- while a second engine that is handed the survivors alone
    takes the scale of their own largest charge, four times finer; each equals its own reference."""
    if case[2] in CHILD_ENV:
        env = dict(CHILD_ENV[case[2]])
        if case[0] in X.THIN:
            env["VPIC_HIP_WINDOW"] = "tile"
        with M.environment(**env):
            run_child(__file__, [case[2], CASES.index(case)], 120)
    else:
        run_case(V, case)


# ---- the += of the finalize step ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["engine", "reference"])
def test_two_species_and_the_same_call_twice_without_a_clear(V, order):
    """species a (q_m = -1), then b (q_m = 1/25: other scales), then b again, into arrays that are cleared once: each
    deterministic call rounds its own sums once onto what the array holds (moments_finalize_kernel's +=); in float mode
    the array holds one float sum of all the contributions"""
    grid = "10x9x7"
    og = X.oracle_grid(grid)
    fi = X.interpolator(grid)
    e = engine_for(V, grid, False)
    e.set_interpolator(np.array(fi))
    e.set_sort_order(order)
    pa, pb = X.particles(51, 6000, grid), X.particles(52, 5000, grid, first_tag=10 ** 6)
    sa, sb = e.new_species(X.Q_MS[0], 6064, 64), e.new_species(X.Q_MS[1], 6064, 64)
    for sp, p in ((sa, pa), (sb, pb)):
        e.set_particles(sp, p)
        e.sort_p(sp)
        assert e.species_order(sp) == ("tile" if order == "engine" else "voxel")
    ra, rb = X.Reference(og, pa, X.Q_MS[0], fi), X.Reference(og, pb, X.Q_MS[1], fi)
    assert not np.array_equal(ra.m.scales, rb.m.scales)
    for mode in ("deterministic", "float"):
        e.set_accumulation(mode, X.Q0)
        e.clear_hydro(); e.clear_rhof()
        for sp in (sa, sb, sb):
            e.accumulate_hydro_p(sp)
            e.accumulate_rho_p(sp)
        check_words("two species, %s order" % order, mode, e.get_hydro(), np.array(e.get_fields()["rhof"]), [ra, rb, rb])
    # ... and onto an array that was uploaded, not cleared
    prev = ra.hydro_words()
    e.set_accumulation("deterministic", X.Q0)
    e.set_hydro(prev)
    e.accumulate_hydro_p(sb)
    check_words("onto an uploaded array", "deterministic", e.get_hydro(), None, [rb], prev_h=prev)
    e.close()


# ---- charges the device makes itself --------------------------------------------------------------------------------------------
def test_emitted_charges_count(V):
    """A species that holds nothing but emitted particles (vpic_hip_emit on the faces of tests/golden/reflux.npz): their
    charges are computed on the device, and Species::q_max has to learn the largest of them, or the deterministic hydro
    moments of such a species are taken at scale 1 (all of them zero) and accumulate_rho_p, with q_ref = 0, finds no charge
    to scale by.  Both against the reference of what get_particles returns, at the scales of its largest |q|."""
    g = np.load(os.path.join(HERE, "golden", "reflux.npz"))
    nx, ny, nz = [int(v) for v in g["dims"]]
    lx, ly, lz, dt = [float(v) for v in g["box"]]
    n_emit, ut_perp, ut_para, q_m = [float(v) for v in g["emit_par"]]
    comp, fi = g["emit_component"], g["emit_fi"]
    og = pyorc.make_grid(nx, ny, nz, lx, ly, lz, np.float32(dt))
    e = V.Engine(V.make_grid(nx, ny, nz, lx, ly, lz, np.float32(dt)))
    e.set_vacuum()
    e.set_interpolator(fi)
    cap = 4 * len(comp) * int(n_emit)
    sp = e.new_species(q_m, cap, cap)
    e.clear_accumulators()
    e.emit(sp, comp, int(n_emit), ut_perp, ut_para)
    assert e.np(sp) > 100 and e.nm(sp) == 0
    got = {}
    for mode in ("deterministic", "float"):
        e.set_accumulation(mode, 0.0)                      # no reference charge: the scales come from the species
        got[mode] = (M.hydro_of(e, sp), np.array(M.rho_of(e, sp)))
        assert e.moments_stats() == (e.np(sp), 0, e.np(sp), 0)
    back = e.get_particles(sp)
    e.close()
    q_max = X.q_max_of(back)
    assert q_max > 0 and len(np.unique(back["q"])) > 10
    ref = X.Reference(og, back, q_m, fi, q_max=q_max, q_ref=q_max)
    for mode in ("deterministic", "float"):
        check_words("emitted", mode, got[mode][0], got[mode][1], [ref])


# ---- accumulate_hydro_p_select ---------------------------------------------------------------------------------------------
SELECTIONS = {
    "box": dict(select=[("ke", 0.01, 100.0), ("z", 2.0, 6.0)]),             # box frame
    "pitch": dict(select=[("cos_pitch", -0.3, 0.8)]),                       # the frame of the local field
    "every": dict(tag_every=(7, 3)),
}


@functools.lru_cache(maxsize=None)
def selected(state):
    """{(mode, selection): (hydro, statistics)} of one engine, and the particles it held; every call once"""
    V = package()
    e, sp, q_max, _ = build(V, "10x9x7", -1.0, state)
    order = e.species_order(sp)
    out = {}
    for mode in ("deterministic", "float"):
        e.set_accumulation(mode, X.Q0)
        for name, desc in SELECTIONS.items():
            e.clear_hydro()
            e.accumulate_hydro_p(sp, **desc)
            out[mode, name] = (e.get_hydro(), e.moments_stats())
            assert e.species_order(sp) == order
    back = e.get_particles(sp)
    e.close()
    return out, back, q_max


@pytest.mark.parametrize("name", list(SELECTIONS))
@pytest.mark.parametrize("state", ["unsorted", "tile", "tail_holes"])
def test_the_moments_of_a_selection(state, name):
    """against the reference over the rows test_fieldcoord_ref.keep_mask keeps, at the WHOLE species' scale (in
    "tail_holes": that of the absorbed heavy particle)"""
    grid = "10x9x7"
    out, back, q_max = selected(state)
    fi = X.interpolator(grid)
    keep = keep_mask(back, X.dims_of(grid), np.array(fi), SELECTIONS[name])
    assert 200 < keep.sum() < len(back) - 200
    ref = X.Reference(X.oracle_grid(grid), back[keep], -1.0, fi, q_max=q_max)
    for mode in ("deterministic", "float"):
        h, stats = out[mode, name]
        what = "select %s %s" % (state, name)
        print("%s %s: statistics %s, the reference keeps %d" % (what, mode, stats, keep.sum()))
        assert stats[0] == keep.sum() and stats[1] + stats[2] == stats[0] and stats[3] == 0
        assert (stats[1] > 0) == (state != "unsorted")
        check_words(what, mode, h, None, [ref])


# ---- synchronize_hydro ---------------------------------------------------------------------------------------------------------
P, Sy, Pm, A = L.PEC_FIELDS, L.SYMMETRIC_FIELDS, L.PMC_FIELDS, L.ABSORB_FIELDS
FIELD_WALLS = {"periodic": [0] * 6, "pec_z": [0, 0, P, 0, 0, P], "mixed_xz": [P, 0, Pm, Sy, 0, A], "mixed_xy": [A, Sy, 0, Pm, P, 0]}


@functools.lru_cache(maxsize=None)
def finalized_hydro(grid):
    p = X.particles(61, X.N_PARTICLES[grid], grid)
    return X.Reference(X.oracle_grid(grid), p, -1.0, X.interpolator(grid)).hydro_words()


@pytest.mark.parametrize("walls", list(FIELD_WALLS))
@pytest.mark.parametrize("grid", list(X.GRIDS))
def test_synchronize_hydro(V, grid, walls):
    """The finalized reference, uploaded with set_hydro: synchronize_hydro == pyorc.synchronize_hydro_local, word values
    compared with == (per-voxel arithmetic, nothing is reordered).  orc_local_adjust_hydro knows two kinds of face: a wall
    of any kind (doubled) and a face shared with the domain itself (folded); the mixed layouts put all four wall kinds
    and a periodic axis on the faces.  Only the periodic and the PEC layouts are pinned on the compiled reference today
    (tests/golden's k10): for the other wall kinds this is the engine against the oracle's restatement."""
    fbc = FIELD_WALLS[walls]
    pbc = [L.REFLECT_PARTICLES if b < 0 else 0 for b in fbc]
    og = X.oracle_grid(grid, fbc=fbc, pbc=pbc)
    h = finalized_hydro(grid)
    want = np.array(h)
    pyorc.synchronize_hydro_local(want, og)
    assert want.tobytes() != h.tobytes()
    e = engine_for(V, grid, False, fbc=fbc, pbc=pbc)
    e.set_hydro(np.array(h))
    e.synchronize_hydro()
    got = e.get_hydro()
    e.close()
    for c in X.MOMENTS:
        assert np.array_equal(got[c], want[c]), "%s %s: %s differs in %d voxels" % (grid, walls, c, (got[c] != want[c]).sum())


if __name__ == "__main__":                                          # the fresh child of the cases that set a knob (run_child)
    assert sys.argv[1] in CHILD_ENV and all(os.environ.get(k) == v for k, v in CHILD_ENV[sys.argv[1]].items())
    run_case(package(), CASES[int(sys.argv[2])])
    print("child OK")
