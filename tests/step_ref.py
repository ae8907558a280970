"""vpic_hip_step held to the oracle step by step (tests/test_step_ref.py on the CPU, tests/test_gpu_step.py on the GPU).

Float sums depend on their order, so an oracle that runs freely beside the engine drifts away from it and only loose
bounds hold.  SteppedRun restarts the oracle from the engine's OWN state before every step instead: it downloads fields,
interpolator and every species' particles (in array order), lets the engine step, runs pyorc._push on the downloaded
state with the fixed-point switch on, and holds what the engine has afterwards to three criteria:

  1  particles, per species: the same count, the oracle's records bit for bit (by tag for a tagged species, as a multiset
     of records for a tag-less one), every cell an interior voxel, every offset within [-1, 1];
  2  accumulator (still the step's own: it is cleared at the head of the NEXT step): deterministic mode -- every word,
     ghosts included, equal as uint32 to pyorc.finalize of the exact integer sums; float mode -- max |a - finalize(a64)| <=
     ACC_TOL max |finalize(a64)| over jx, jy, jz.  The reference is the exact sums, so the whole budget is the engine's;
  3  fields and interpolator: pyorc._fields on the pre-step fields with the ENGINE's downloaded accumulator gives the
     engine's post-step fields and interpolator, every component equal as a number (the sign of a zero is free), ghosts
     included.  Everything behind the accumulator is arithmetic per voxel, which the project holds bit for bit: no
     tolerance, no drift, in float mode too.  One word is not behind the accumulator: rhob, to which the particles an
     absorbing wall takes add their charge with float atomics, in the order of the launch.  It is unchanged bit for bit on
     every node that no absorbed particle touches, and elsewhere within the bound of a float sum of that node's terms of
     the step taken in two orders (rhob_bound; the terms are counted per node from the oracle's movers).

Plain numpy and oracle.pyorc; no GPU import.  `engine` is anything with get_fields, get_interpolator, get_accumulator,
get_particles(sp), np(sp), step(k, interval) and species_stats(sp)."""
import importlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from oracle import pyorc  # noqa: E402
import det_exact as D  # noqa: E402
from sort_ref import _records, words  # noqa: E402
from test_gpu_tiles import hot_particles  # noqa: E402

L = importlib.import_module("old-vpic_amd.layout")

ACC_TOL = 2e-6                       # the project's bound on a float accumulator against its reference
DT = 0.95 / np.sqrt(3.0)             # unit cells, c = 1: 0.95 of the Courant limit
Q0 = 0.004                           # reference charge of the decks: 2 x 20 ppc of it put omega_p dt near 0.2
FIELD_WORDS = [n for n in L.field_t.names if L.field_t[n].kind == "f" and n != "rhob"]
INTERPOLATOR_WORDS = [n for n in L.interpolator_t.names if not n.startswith("_")]


class StepMismatch(AssertionError):
    """what SteppedRun.advance raises: .step, .criterion (1, 2 or 3), .species (index or None)"""

    def __init__(self, step, criterion, species, text):
        self.step, self.criterion, self.species = step, criterion, species
        where = "" if species is None else " species %d" % species
        AssertionError.__init__(self, "step %d, criterion %d%s: %s" % (step, criterion, where, text))


def _xyz(v, dims):
    nx, ny, _ = dims
    return int(v % (nx + 2)), int(v // (nx + 2) % (ny + 2)), int(v // ((nx + 2) * (ny + 2)))


def _show(rec):
    return "(" + ", ".join("%s=%r" % (n, rec[n].item()) for n in ("i", "dx", "dy", "dz", "ux", "uy", "uz", "q")) + ")"


def exact_float(a64, scale):
    """float64[3, nv, 4] of pyorc.finalize(a64, scale): jx, jy, jz"""
    a = pyorc.finalize(a64, scale)
    return np.stack([a["jx"], a["jy"], a["jz"]]).astype(np.float64)


def acc_float(a, nv):
    return np.stack([a["jx"][:nv], a["jy"][:nv], a["jz"][:nv]]).astype(np.float64)


def acc_ratio(a, a64, scale):
    """max |a - finalize(a64)| / max |finalize(a64)| over jx, jy, jz: what criterion 2 bounds by ACC_TOL in float mode"""
    want = exact_float(a64, scale)
    return float(np.abs(acc_float(a, want.shape[1]) - want).max() / np.abs(want).max())


def rhob_bound(ref_abs, n_terms):
    """per node: two float sums of the same n_terms + 1 terms of one sign (what the node held, then one per absorbed particle
    that touches the node), whose absolute values sum to ref_abs, differ by at most 2 n_terms 2^-24 ref_abs (each running
    sum rounds n_terms times by half an ulp of at most ref_abs, to first order; the factor 2 for the two orders).
    n_terms: int array per node, or a number"""
    return 2.0 * n_terms * 2.0 ** -24 * ref_abs


def rhob_terms(og, voxels):
    """int64[nv]: per node, how many of the particles absorbed in `voxels` (the cell each one stopped in) add to it -- the
    eight nodes of the cell (boundary_p.c:9-71)"""
    sy, sz = og.nx + 2, (og.nx + 2) * (og.ny + 2)
    n = np.zeros(og.nv + sz + sy + 2, np.int64)
    v = np.asarray(voxels, np.int64)
    for off in (0, 1, sy, sy + 1, sz, sz + 1, sz + sy, sz + sy + 1):
        np.add.at(n, v + off, 1)
    return n[:og.nv]


class SteppedRun:
    """species_meta: per species of the engine, in the order the engine pushes them, dict(sp=<the engine's id>, q_m=...,
    tagged=bool).  det_scale: the fixed-point scale of an engine in deterministic accumulation (pyorc.fixed_scale(q_ref)),
    None for float accumulation."""

    def __init__(self, engine, og, m, species_meta, det_scale=None):
        self.e, self.og, self.m, self.meta, self.det_scale = engine, og, m, list(species_meta), det_scale
        self.dims = (og.nx, og.ny, og.nz)
        self.scale = det_scale
        interior = np.zeros(og.nv, bool)
        nx, ny, nz = self.dims
        z, y, x = np.meshgrid(np.arange(1, nz + 1), np.arange(1, ny + 1), np.arange(1, nx + 1), indexing="ij")
        interior[L.voxel(x, y, z, nx, ny, nz).ravel()] = True
        self.interior = interior
        self.log = []

    # ---- criterion 1 ----
    def _particles(self, k, s, got, ref, tagged):
        if len(got) != len(ref):
            raise StepMismatch(k, 1, s, "%d particles, the oracle has %d" % (len(got), len(ref)))
        if tagged:
            g, r = D.by_tag(got), D.by_tag(ref)
            if not np.array_equal(g["tag"], r["tag"]):
                j = int(np.flatnonzero(g["tag"] != r["tag"])[0])
                raise StepMismatch(k, 1, s, "the tags differ from the oracle's: tag %d where the oracle has tag %d" % (g["tag"][j], r["tag"][j]))
            bad = np.flatnonzero((words(g) != words(r)).any(axis=1))
            if len(bad):
                j = int(bad[0])
                raise StepMismatch(k, 1, s, "%d records differ from the oracle's; tag %d is %s, the oracle has %s"
                                   % (len(bad), g["tag"][j], _show(g[j]), _show(r[j])))
        else:
            g, r = _records(got), _records(ref)
            bad = np.flatnonzero((g != r).any(axis=1))
            if len(bad):
                j = int(bad[0])
                as_rec = lambda w: _show(np.ascontiguousarray(w).view(np.dtype([(n, "i4" if n == "i" else "f4") for n in ("dx", "dy", "dz", "i", "ux", "uy", "uz", "q")]))[0])
                raise StepMismatch(k, 1, s, "%d records of the sorted multiset differ from the oracle's; the first is %s, the oracle has %s"
                                   % (len(bad), as_rec(g[j]), as_rec(r[j])))
        i = got["i"].astype(np.int64)
        out = (i < 0) | (i >= self.og.nv)
        out[~out] = ~self.interior[i[~out]]
        if out.any():
            j = int(np.flatnonzero(out)[0])
            raise StepMismatch(k, 1, s, "array slot %d sits in voxel %d, which is no interior voxel: %s" % (j, i[j], _show(got[j])))
        for c in ("dx", "dy", "dz"):
            far = ~(np.abs(got[c]) <= 1)
            if far.any():
                j = int(np.flatnonzero(far)[0])
                raise StepMismatch(k, 1, s, "array slot %d has %s = %r outside its cell: %s" % (j, c, got[c][j].item(), _show(got[j])))

    # ---- criterion 2 ----
    def _accumulator(self, k, a, a64, streaks):
        if self.det_scale is not None:
            bad = D.describe_bad_words(a, a64, streaks, self.scale, self.dims)
            if bad is not None:
                raise StepMismatch(k, 2, None, bad)
            return 0.0
        want = exact_float(a64, self.scale)
        got = acc_float(a, self.og.nv)
        top = np.abs(want).max()
        err = np.abs(got - want)
        ratio = float(err.max() / top) if top > 0 else float(err.max() > 0) * np.inf
        if not ratio <= ACC_TOL:
            c, v, w = np.unravel_index(int(np.argmax(err)), err.shape)
            raise StepMismatch(k, 2, None, "accumulator %s[%d] of voxel %d %s is %r, the exact sum is %r: off by %.3g of the largest sum %.6g, the bound is %.3g (%d words over it)"
                               % (("jx", "jy", "jz")[c], w, v, _xyz(v, self.dims), float(got[c, v, w]), float(want[c, v, w]), ratio, top, ACC_TOL,
                                  int((err > ACC_TOL * top).sum())))
        return ratio

    # ---- criterion 3 ----
    def _same(self, k, what, names, got, want):
        for c in names:
            if not np.array_equal(got[c], want[c]):
                bad = np.flatnonzero(got[c] != want[c])
                v = int(bad[0])
                raise StepMismatch(k, 3, None, "%s.%s differs in %d voxels from the oracle's field chain on the engine's accumulator; voxel %d %s%s is %r, expected %r"
                                   % (what, c, len(bad), v, _xyz(v, self.dims), "" if self.interior[v] else " (ghost)", got[c][v].item(), want[c][v].item()))

    def _rhob(self, k, f0, f1, f_orc, terms):
        """terms: rhob_terms of the step's absorbed particles.  A node none of them touches keeps its word (the oracle's is
        then the pre-step word itself: tolerance 0)."""
        got, want = f1["rhob"].astype(np.float64), f_orc["rhob"].astype(np.float64)
        assert np.array_equal(f_orc["rhob"][terms == 0], f0["rhob"][terms == 0])
        tol = rhob_bound(np.abs(want) * (1 + 2.0 ** -20), terms)
        bad = np.flatnonzero(~(np.abs(got - want) <= tol))
        if len(bad):
            v = int(bad[0])
            raise StepMismatch(k, 3, None, "fields.rhob differs in %d voxels; voxel %d %s is %r, expected %r within %.3g (%d absorbed particles add to this node in this step)"
                               % (len(bad), v, _xyz(v, self.dims), float(got[v]), float(want[v]), float(tol[v]), int(terms[v])))

    def advance(self, k, interval):
        """One engine step held to the oracle; raises StepMismatch, returns the step's facts."""
        e, og = self.e, self.og
        f0, fi0 = e.get_fields(), e.get_interpolator()
        p0 = [e.get_particles(meta["sp"]) for meta in self.meta]
        if self.scale is None:                                   # float mode: the exact sums need a scale of their own
            qmax = max([float(np.abs(p["q"]).max()) for p in p0 if len(p)] + [0.0])
            self.scale = pyorc.fixed_scale(qmax if qmax > 0 else 1.0)
        e.step(k, interval)
        p1 = [e.get_particles(meta["sp"]) for meta in self.meta]
        a1, f1, fi1 = e.get_accumulator(), e.get_fields(), e.get_interpolator()
        # the oracle on the downloaded state
        f, fi = f0.copy(), fi0.copy()
        a = np.zeros(og.nv + 1, L.accumulator_t)
        species = [dict(p=np.concatenate([p, np.zeros(1, L.particle_t)]), np=len(p), q_m=meta["q_m"], pm=np.zeros(len(p) + 1, L.particle_mover_t))
                   for p, meta in zip(p0, self.meta)]
        crossed, movers, stopped = [], [], []
        for sp, p in zip(species, p0):                           # (facts only: a push of a copy, outside the switch)
            q = sp["p"].copy()
            nm = pyorc.advance_p(q, sp["np"], sp["q_m"], sp["pm"], np.zeros(og.nv + 1, L.accumulator_t), fi, og)
            crossed.append(int((q["i"][:len(p)] != p["i"]).sum()) + nm)
            movers.append(int(nm))
            stopped.append(q["i"][sp["pm"]["i"][:nm]].astype(np.int64))   # the cells the movers stopped in: on a wall
        with pyorc.fixed_accumulator(og, self.scale) as (a64, streaks):
            pyorc._push(f, fi, a, species, og, False)
        absorbed = [len(p) - sp["np"] for p, sp in zip(p0, species)]
        for s, (got, sp, meta) in enumerate(zip(p1, species, self.meta)):
            self._particles(k, s, got, sp["p"][:sp["np"]], meta["tagged"])
        ratio = self._accumulator(k, a1, a64, streaks)
        fr, fir = f0.copy(), fi0.copy()
        ar = np.zeros(og.nv + 1, L.accumulator_t)
        ar[:og.nv] = a1[:og.nv]
        pyorc._fields(fr, fir, ar, self.m, species, og, False, False, False)
        self._same(k, "fields", FIELD_WORDS, f1, fr)
        if sum(absorbed):
            # (on one domain every mover the push leaves is taken by an absorbing wall; the bound is that of terms of one sign)
            signs = {np.sign(v) for p in p0 for v in (p["q"].min(), p["q"].max()) if len(p)} - {0.0}
            if len(signs) > 1 or movers != absorbed:
                raise ValueError("SteppedRun bounds rhob for charges of one sign and movers that are all absorbed")
        self._rhob(k, f0, f1, f, rhob_terms(og, np.concatenate(stopped)))
        self._same(k, "interpolator", INTERPOLATOR_WORDS, fi1, fir)
        facts = dict(step=k, crossed=crossed, movers=movers, absorbed=absorbed, np=[len(p) for p in p1], acc_ratio=ratio,
                     species_stats=[e.species_stats(meta["sp"]) for meta in self.meta])
        self.log.append(facts)
        return facts


# ---- decks of the matrix: (dims, walls, species) with species a list of dict(p, q_m, tagged) --------------------------------
def _untag(p):
    p["tag"] = 0
    p["tag2"] = 0
    return p


def _beams(dims, ppc, tagged, vth=0.02, drift=0.2, seed=40):
    n = dims[0] * dims[1] * dims[2] * ppc
    out = []
    for k, d in enumerate((drift, -drift)):                      # two species of the same sign of charge
        p = D.particles(seed + k, n, dims, vth, q0=-Q0, first_tag=1 + k * n)
        p["ux"] += np.float32(d)
        out.append(dict(p=p if tagged else _untag(p), q_m=-1.0, tagged=tagged))
    return out


def _hot(dims, ppc, tagged, vth=0.5, seed=50, q_m=-1.0):
    nx, ny, nz = dims
    p = hot_particles(L, np.random.default_rng(seed), nx, ny, nz, ppc, vth=vth, q=-Q0)
    return [dict(p=p if tagged else _untag(p), q_m=q_m, tagged=tagged)]


def _chargeless(dims, ppc):
    sp = _hot(dims, ppc, True)[0]
    copy = dict(p=sp["p"].copy(), q_m=sp["q_m"], tagged=True)
    copy["p"]["q"] = 0
    copy["p"]["tag"] += 10 ** 7
    return [sp, copy]


def _clumped(n=80000, seed=21):
    """every particle in tile (1, 1, 1) of a 16^3 grid, as test_a_clumped_species_leaves_the_tile_order places them"""
    dims = (16, 16, 16)
    cells = L.voxel(*np.meshgrid(np.arange(5, 9), np.arange(5, 9), np.arange(5, 9), indexing="ij"), 16, 16, 16).ravel()
    p = D.particles(seed, n, dims, 0.3, q0=-Q0, cells=cells)
    return [dict(p=_untag(p), q_m=-1.0, tagged=False)]


def _clumped_spread(n_light=68000, n_heavy=40, seed=21):
    """the clumped deck for float sums.  Over 65536 particles in one tile are a thousand per cell, and the oracle's OWN
    float sums of so many equal terms are 1.2e-6 to 1.8e-6 from the exact ones (tests/test_step_ref.py wants at most
    ACC_TOL / 2).  So the charge is spread: 68000 particles of charge Q0 / 1000 in 63 cells of the tile and 40 of charge Q0,
    cold and drifting, in the 64th.  The tile is as full, and the sums of the 64th cell and of the cells its particles
    drift into set the scale of criterion 2 -- about 30 times the light cells' sums, which it therefore holds 30 times
    less tightly than the deterministic run of the equal-charge deck does (exactly)."""
    dims = (16, 16, 16)
    cells = L.voxel(*np.meshgrid(np.arange(5, 9), np.arange(5, 9), np.arange(5, 9), indexing="ij"), 16, 16, 16).ravel()
    light = D.particles(seed, n_light, dims, 0.3, q0=-Q0 / 1000, cells=cells[:63])
    heavy = D.particles(seed + 1, n_heavy, dims, 0.05, q0=-Q0, cells=cells[63:])
    for c in ("ux", "uy", "uz"):
        heavy[c] += np.float32(0.3)
    return [dict(p=_untag(np.concatenate([light, heavy])), q_m=-1.0, tagged=False)]


MAIN, RAGGED, THIN, LONG = (16, 12, 8), (10, 9, 7), (12, 1, 12), (65, 5, 4)
DECKS = {
    # name: (dims, particle walls, builder of the species)
    "beams": (MAIN, "periodic", lambda: _beams(MAIN, 20, False)),
    "beams_tagged": (MAIN, "periodic", lambda: _beams(MAIN, 20, True)),
    "hot_tagged": (MAIN, "periodic", lambda: _hot(MAIN, 20, True)),
    "hot": (MAIN, "periodic", lambda: _hot(MAIN, 20, False)),
    "hot_reflect": (RAGGED, "reflect", lambda: _hot(RAGGED, 16, True, seed=51)),
    "thin": (THIN, "periodic", lambda: _hot(THIN, 40, False, seed=52)),
    "walls_ragged_ax": (RAGGED, "absorb_x_reflect_z", lambda: _hot(RAGGED, 24, False, seed=53)),
    "walls_ragged_az": (RAGGED, "reflect_y_absorb_z", lambda: _hot(RAGGED, 24, False, seed=54)),
    "walls_long_ax": (LONG, "absorb_x_reflect_z", lambda: _hot(LONG, 16, False, seed=55)),
    "walls_long_az": (LONG, "reflect_y_absorb_z", lambda: _hot(LONG, 16, False, seed=56)),
    "chargeless": (RAGGED, "periodic", lambda: _chargeless(RAGGED, 16)),
    "clumped": ((16, 16, 16), "periodic", _clumped),
    "clumped_spread": ((16, 16, 16), "periodic", _clumped_spread),
}


FLOAT_DECKS = [d for d in DECKS if d != "clumped"]        # (clumped: deterministic mode; clumped_spread is its float deck)


def deck(name):
    """(dims, walls, engine grid arguments, keywords, oracle grid, species) of a deck of the matrix"""
    dims, walls, build = DECKS[name]
    args, kw, og = D.grids(dims, walls, DT)
    return dims, walls, args, kw, og, build()


def arrivals(dims, n, seed, first_tag=10 ** 8, tagged=False, vth=0.5):
    """n particles to append between steps"""
    p = D.particles(seed, n, dims, vth, q0=-Q0, first_tag=first_tag)
    return p if tagged else _untag(p)
