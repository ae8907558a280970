"""What tests/test_source_ref.py (CPU), tests/test_gpu_reflux.py and tests/test_gpu_emit.py (GPU) share: the reference world of
the particle sources at walls -- Maxwellian reflux handlers (the `code <= -3` branch of boundary_p) on one domain, and, at
the end of the file, the surface emitter's test-mode arithmetic restated in numpy (emit_restatement).

It offers the inputs of a case (grid, particle walls, handlers, species, seeded particles whose charge is a distinct float
each, q0 * (1 + k * 2^-14), so that the charge identifies a particle after it has lost its tag), the draw tables, and
predict_round(): one round of boundary_p predicted from a given state -- particles in array order plus movers, as read from
the device before the round -- by the oracle's orc_boundary_p_reflux_round (oracle/vpic_oracle.h), which
tests/test_oracle_golden.py pins on the reference's own boundary_p bit for bit.  The array order is the state's, so the
back-fill order of a round does not matter: survivors are compared as a multiset.

The device's logf is not the host's.  predict_round therefore takes, per refluxed particle, the magnitude of the new normal
momentum the device produced (read from the particle, found by its charge), checks it against
ut_para * sqrt(2) * sqrt(-log(d)) taken in float64 within NORMAL_ULPS float ulps, and hands it to the oracle in place of
maxwellian_reflux.c:120: everything downstream of that one number is + - * / sqrtf, exact on both sides, so every other
comparison is `==`.

NORMAL_ULPS = 4: two float products, one correctly rounded sqrtf and the float constant sqrt(2) give 2 ulps; the other 2 are
half of an allowed 4 ulp error of logf (sqrt halves a relative error) -- looser than any bound a math library claims."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import det_exact as D  # noqa: E402
from det_exact import L, pyorc  # noqa: E402

F = np.float32
REFLECT, ABSORB = L.REFLECT_PARTICLES, L.ABSORB_PARTICLES
NORMAL_ULPS = 4
MAX_ROUNDS = 5
SCALE = pyorc.fixed_scale(D.Q0)

# particle walls, faces -x -y -z +x +y +z (0: this same domain); codes <= -3 name handlers
WALLS = {
    "reflux6": [-3] * 6,
    "reflux_absorb_reflect": [-3, ABSORB, REFLECT, -3, ABSORB, REFLECT],
    "two_handlers": [-3, -4, 0, -4, -3, 0],
    "unregistered": [-3, -5, 0, -3, -5, 0],              # -5 is registered nowhere: absorbed into rhob
    "reflux_x": [-3, 0, 0, -3, 0, 0],
}
# handler code -> (ut_para, ut_perp) per species (up to two species per case)
HANDLERS = {
    "one": {-3: [(0.11, 0.04), (0.3, 0.2)]},
    "two": {-3: [(0.11, 0.04), (0.3, 0.2)], -4: [(0.5, 0.25), (0.4, 0.15)]},
    "hot_x": {-3: [(2.0, 0.3), (2.0, 0.3)]},              # refluxed particles cross a one-cell grid: second and third rounds
    "zero_second": {-3: [(0.11, 0.04), (0.0, 0.0)]},      # the second species: momentum and displacement exactly zero
}
# species of a case: (q_m, charge factor); a factor of 0 is a copy of species 0 without charge (the chargeless instance of the
# push, injectors that deposit nothing): its particles are found by their tags, its refluxed ones by their tangential momenta
SPECIES = {
    "one": [(-1.0, -1.0)],
    "two": [(-1.0, -1.0), (0.25, 1.0)],
    "with_chargeless_copy": [(-1.0, -1.0), (-1.0, 0.0)],
}
N_PARTICLES = {(10, 9, 7): 8000, (5, 3, 2): 2000, (65, 5, 4): 16000, (1, 6, 5): 3000}


def handlers_of(case, s):
    """[(code, ut_para, ut_perp)] as species s of the case sees them"""
    return [(code, F(ut[s][0]), F(ut[s][1])) for code, ut in sorted(HANDLERS[case["handlers"]].items(), reverse=True)]


def grids(case):
    """(engine grid arguments, keywords, oracle grid): unit cells, except that the one-cell grid is a slab a quarter of a
    cell thick -- a refluxed particle with most of its step left then reaches the opposite face (at c dt = 0.95 it could
    not cross a whole unit cell)"""
    args, kw, og = D.grids(case["dims"], WALLS[case["walls"]])
    if case["dims"][0] == 1:
        args = args[:3] + (0.25,) + args[4:]
        og = pyorc.make_grid(*args, **kw)
    return args, kw, og


def species_particles(case, s, n=None):
    """the seeded hot particles of species s: det_exact.particles with charges q0 * (1 + k * 2^-14), distinct floats"""
    n = N_PARTICLES[case["dims"]] if n is None else n
    p = D.particles(31 + 7 * s, n, case["dims"], D.HOT, first_tag=1 + s * 10 ** 6)
    factor = SPECIES[case["species"]][s][1]
    if factor == 0:
        p = species_particles(dict(case, species="one"), 0, n)
        p["q"] = 0
        p["tag"] += s * 10 ** 6
        return p
    p["q"] =(F(D.Q0 * factor) * (1 + np.arange(n) * 2.0 ** -14)).astype(F)
    assert len(np.unique(p["q"])) == n
    return p


def draw_table(n, seed=5):
    """float32[n, 3]: (uniform strictly inside (0, 1), normal, normal) per array slot -- vpic_hip_set_reflux_draws"""
    rng = np.random.default_rng(seed)
    d = np.empty((n, 3), F)
    d[:, 0] = np.clip(rng.uniform(0, 1, n), 2.0 ** -24, 1 - 2.0 ** -24).astype(F)
    d[:, 1:] = rng.standard_normal((n, 2)).astype(F)
    assert np.all((d[:, 0] > 0) & (d[:, 0] < 1))
    return d


# ---- rhob: the weights of accumulate_rhob (boundary_p.c:9-71) in numpy, and the bound of a node's sum ----------------------
def rhob_terms(p, og):
    """(nodes int64[n, 8], weights float32[n, 8]) that accumulate_rhob adds for the particles p: the first product in double,
    rounded once, everything after it in float, operation by operation"""
    dims = (og.nx, og.ny, og.nz)
    sy, sz = og.nx + 2, (og.nx + 2) * (og.ny + 2)
    w0 = (0.125 * p["q"].astype(np.float64) * np.float64(F(og.rdx)) * np.float64(F(og.rdy)) * np.float64(F(og.rdz))).astype(F)
    one = F(1)
    t = p["dx"] * w0
    w1 = w0 + t
    w0 = w0 - t
    t = p["dy"]
    w3 = one + t
    w2 = w0 * w3
    w3 = w3 * w1
    t = one - t
    w0 = w0 * t
    w1 = w1 * t
    t = p["dz"]
    w7 = one + t
    w4, w5, w6 = w0 * w7, w1 * w7, w2 * w7
    w7 = w7 * w3
    t = one - t
    w0, w1, w2, w3 = w0 * t, w1 * t, w2 * t, w3 * t
    w = np.stack([w0, w1, w2, w3, w4, w5, w6, w7], axis=1).astype(F)
    v = p["i"].astype(np.int64)
    c = [v % sy, v // sy % (og.ny + 2), v // sz]
    for axis, (lo, hi) in enumerate((((0, 2, 4, 6), (1, 3, 5, 7)), ((0, 1, 4, 5), (2, 3, 6, 7)), ((0, 1, 2, 3), (4, 5, 6, 7)))):
        for cols, at in ((lo, 1), (hi, dims[axis])):
            rows = np.flatnonzero(c[axis] == at)
            for k in cols:
                w[rows, k] += w[rows, k]
    nodes = v[:, None] + np.array([0, 1, sy, sy + 1, sz, sz + 1, sz + sy, sz + sy + 1])[None, :]
    return nodes, w


def rhob_bound(prior, p_absorbed, og):
    """Per node of the field array: (the sum of its terms in float64, the bound on a float sum of them taken in any order,
    the float sum where order cannot matter, the number of terms).  The terms are the node's prior value (when not zero) and
    the weights absorbed particles add; n terms summed in float in any order are within
    (n - 1) 2^-24 / (1 - (n - 1) 2^-24) * sum|c_k| of the true sum, and two terms or fewer give the correctly rounded sum
    whatever the order."""
    nodes, w = rhob_terms(p_absorbed, og)
    nv = len(prior)
    n = (prior != 0).astype(np.int64)
    s, sabs, s32 = prior.astype(np.float64), np.abs(prior).astype(np.float64), prior.astype(F).copy()
    np.add.at(n, nodes.ravel(), 1)
    np.add.at(s, nodes.ravel(), w.ravel().astype(np.float64))
    np.add.at(sabs, nodes.ravel(), np.abs(w.ravel()).astype(np.float64))
    np.add.at(s32, nodes.ravel(), w.ravel())
    m = np.maximum(n - 1, 0) * 2.0 ** -24
    assert nv == len(s)
    return s, m / (1 - m) * sabs, s32, n


def describe_rhob(got, prior, p_absorbed, og):
    """None when got is within the node bound of rhob_bound everywhere and bit-equal where a node has at most two terms;
    else a message naming the first bad nodes"""
    s, bound, s32, n = rhob_bound(prior, p_absorbed, og)
    bad = np.abs(got.astype(np.float64) - s) > bound
    bad |= (n <= 2) & (got.view(np.uint32) != s32.view(np.uint32))
    if not bad.any():
        return None
    return "rhob differs at %d nodes; first: " % bad.sum() + "; ".join(
        "node %d: got %.9g, sum of %d terms %.17g, bound %.3g" % (v, got[v], n[v], s[v], bound[v]) for v in np.flatnonzero(bad)[:4])


# ---- one round -------------------------------------------------------------------------------------------------------------
def expected_normal(draw0, ut_para):
    """|ut_para * sqrt(2) * sqrt(-log(d))| in float64 from the float inputs"""
    return np.abs(np.asarray(ut_para, F).astype(np.float64) * np.sqrt(2.0) * np.sqrt(-np.log(np.asarray(draw0, F).astype(np.float64))))


class Round:
    """what predict_round returns for one species: p (survivors, then the refluxed particles in the oracle's order), pm
    (the movers left), n_keep, inj / who / face (the injectors, the index in the old mover list of the mover behind each,
    the face whose handler made it), absorbed (the particle records that went into rhob), ulps (the error of each new
    normal momentum taken from the device, in float ulps of the expected value; empty without device momenta)"""


def predict_round(og, p, pm, sp_id, handlers, draws, f, a, after=None, fixed=None):
    """One round of boundary_p for one species from the state (p in array order, pm): rhob is added to f and the deposits
    to a, in place (and to the fixed-point sums, inside pyorc.fixed_accumulator).  after: None -- the oracle's own logf
    decides the new normal momenta (tests/test_source_ref.py); or the species' particles as the device left them after the
    round -- the magnitude of each refluxed particle's new normal momentum is read from the particle it became, found by
    its charge among after[n_keep:], and replaces maxwellian_reflux.c:120 (its sign is the face's).  A refluxed particle
    that cannot be found there is an AssertionError that names it.  fixed: the (a64, streaks) of the fixed_accumulator
    block this runs in, if any -- the pass that only tells who refluxes where must leave no deposits in them."""
    r = Round()
    u_normal, r.ulps = None, np.zeros(0)
    if after is not None:
        f0, a0 = f.copy(), np.zeros_like(a)                             # a first pass tells who refluxes at which face
        keep = None if fixed is None else [x.copy() for x in fixed]
        _, _, inj, who, face = pyorc.boundary_p_reflux_round(p, pm, sp_id, f0, a0, og, handlers, draws)
        if fixed is not None:
            fixed[0][...], fixed[1][...] = keep
        n_keep = len(p) - len(pm)
        tail = after[n_keep:]
        at = match_refluxed(inj, face, tail, by_charge=bool(np.any(p["q"] != 0)))
        missing = np.flatnonzero(at < 0)
        assert len(missing) == 0, "species %d: %d refluxed particles are not among the %d the device appended; first: %s" % (
            sp_id, len(missing), len(tail), "; ".join(describe_mover(p, pm, who[k], face[k], og) for k in missing[:4]))
        assert len(np.unique(at)) == len(at), "species %d: two refluxed particles were matched with one particle of the device" % sp_id
        r.match = at
        got = tail[at]
        axis = face % 3
        mag = np.abs(np.choose(axis, [got["ux"], got["uy"], got["uz"]]))
        u_normal = np.zeros(len(pm), F)
        u_normal[who] = np.where(face >= 3, -mag, mag)
        para = np.array([dict((h[0], h[1]) for h in handlers)[og.pbc[fc]] for fc in face], F) if len(face) else np.zeros(0, F)
        want = expected_normal(draws[pm["i"][who], 0], para)
        ulp = np.spacing(np.maximum(want, np.finfo(F).tiny).astype(F)).astype(np.float64)
        r.ulps = np.abs(mag.astype(np.float64) - want) / ulp
    r.p, r.pm, r.inj, r.who, r.face = pyorc.boundary_p_reflux_round(p, pm, sp_id, f, a, og, handlers, draws, u_normal)
    r.n_keep = len(p) - len(pm)
    gone = np.ones(len(pm), bool)
    gone[r.who] = False
    r.absorbed = p[pm["i"][gone]]
    return r


def describe_mover(p, pm, k, face, og):
    s = int(pm["i"][k])
    q = p[s]
    v = int(q["i"])
    x, y, z = v % (og.nx + 2), v // (og.nx + 2) % (og.ny + 2), v // ((og.nx + 2) * (og.ny + 2))
    on = [f for f in range(6) if q[("dx", "dy", "dz")[f % 3]] == (1 if f >= 3 else -1) and (q[("ux", "uy", "uz")[f % 3]] > 0) == (f >= 3)]
    return "mover %d (slot %d, q %.9g, tag %d, cell (%d, %d, %d), on faces %s with codes %s, refluxed at face %d)" % (
        k, s, q["q"], q["tag"], x, y, z, on, [og.pbc[f] for f in on], face)


def _sorted_search(keys, wanted):
    """index into keys of each of wanted, -1 where it is not there"""
    if len(keys) == 0:
        return np.full(len(wanted), -1, np.int64)
    o = np.argsort(keys, kind="stable")
    at = np.minimum(np.searchsorted(keys[o], wanted), len(keys) - 1)
    return np.where(keys[o][at] == wanted, o[at], -1)


def match_refluxed(inj, face, tail, by_charge):
    """For each injector the handlers made (inj, face), the index in `tail` (the particles the device appended) of the
    particle it became, -1 where there is none.  By charge, where the species has charges (distinct floats).  A chargeless
    copy of a species is matched by the two tangential momenta instead: ut_perp * draw, one float product each, the same
    bits on both sides, which a move changes at most in sign and which two slots of a table of random normals do not
    share (they must not be zero: a chargeless species needs ut_perp != 0)."""
    if by_charge:
        return _sorted_search(tail["q"], inj["q"])
    at = np.full(len(inj), -1, np.int64)

    def key(rec, axis):
        u = [np.ascontiguousarray(rec[c]) for c in ("ux", "uy", "uz")]
        t1 = np.abs(u[(axis + 1) % 3]).view(np.uint32).astype(np.uint64)
        t2 = np.abs(u[(axis + 2) % 3]).view(np.uint32).astype(np.uint64)
        return (t1 << np.uint64(32)) | t2
    for axis in range(3):
        m = np.flatnonzero(face % 3 == axis)
        k = key(inj[m], axis)
        assert np.all(k != 0), "a chargeless species cannot be matched at ut_perp == 0"
        at[m] = _sorted_search(key(tail, axis), k)
    return at


def ordered(p):
    """p in an order that depends on its content alone: by charge (a distinct float per particle of a charged species), then
    by tag (distinct among the particles of a chargeless copy that never refluxed), then by the rest of the record"""
    cols = [np.ascontiguousarray(p[c]).view(np.uint32) for c in ("uz", "uy", "ux", "dz", "dy", "dx")] + [p["i"], p["tag"], p["q"]]
    return p[np.lexsort(cols)]


def movers_keyed(p, pm):
    """(the movers' particle records, the movers), both in the order of ordered()"""
    rec = p[pm["i"]]
    cols = [np.ascontiguousarray(rec[c]).view(np.uint32) for c in ("uz", "uy", "ux", "dz", "dy", "dx")] + [rec["i"], rec["tag"], rec["q"]]
    o = np.lexsort(cols)
    return rec[o], pm[o]


# ---- parked movers: what a push produces only by coincidence --------------------------------------------------------------------
# wall kinds of the pairings: a registered handler, a code registered nowhere, absorb, reflect, this same domain
KINDS = {"handler": -3, "unregistered": -5, "absorb": ABSORB, "reflect": REFLECT, "self": 0}
PARKED_DIMS = (6, 5, 4)


def parked_pairings():
    """[(kind of the first face, kind of the second, walls)]: every ordered pairing of the five kinds on the faces -x
    (first in the reference's face order) and -y (second); the other faces reflect (opposite a face of this same domain
    lies this same domain: an axis is periodic on both sides or on none)"""
    self_or_reflect = lambda kind: 0 if kind == "self" else REFLECT
    return [(a, b, [KINDS[a], KINDS[b], REFLECT, self_or_reflect(a), self_or_reflect(b), REFLECT]) for a in KINDS for b in KINDS]


def parked_on(faces, n, dims, seed, q0=-D.Q0, first=0, n_rest=0):
    """(p, pm): n particles parked on all of `faces` at once (different axes), leaving through each, with something of the
    step left, among n_rest bystanders; the movers' list ascends.  Charges q0 * (1 + (first + k) * 2^-14)."""
    rng = np.random.default_rng(seed)
    nx, ny, nz = dims
    total = n + n_rest
    p = D.particles(seed, total, dims, 0.8)
    p["q"] = (F(q0) * (1 + (first + np.arange(total)) * 2.0 ** -14)).astype(F)
    slots = np.sort(rng.choice(total, n, replace=False))
    c = [rng.integers(1, m + 1, n) for m in dims]
    for f in faces:
        axis, hi = f % 3, f >= 3
        p[("dx", "dy", "dz")[axis]][slots] = 1.0 if hi else -1.0
        u = np.abs(p[("ux", "uy", "uz")[axis]][slots]) + F(0.05)
        p[("ux", "uy", "uz")[axis]][slots] = u if hi else -u
        c[axis][:] = dims[axis] if hi else 1
    p["i"][slots] = L.voxel(c[0], c[1], c[2], nx, ny, nz)
    pm = np.zeros(n, L.particle_mover_t)
    for k in ("dispx", "dispy", "dispz"):
        pm[k] = (0.3 * rng.uniform(-1, 1, n)).astype(F)
    pm["i"] = slots
    return p, pm


# ---- the pushed cases: one advance_p of seeded hot particles, then rounds until no species has movers -----------------------------
# array states: as uploaded; the reference's order; tile order; tile only (a fresh child); tile order with particles appended
# after the sort, VPIC_HIP_TAIL_SORT_MIN below / above the tail's length; "thin": a grid thinner than a tile keeps the
# reference's order whatever is asked
STATES = ("unsorted", "voxel", "tile", "tile_only", "tail_below", "tail_above", "thin")
N_TAIL = 1500
TAIL_SORT_MIN = {"tail_below": 100, "tail_above": 1 << 20}
THIN = ((5, 3, 2), (1, 6, 5))
A, B, C_, X = (10, 9, 7), (5, 3, 2), (65, 5, 4), (1, 6, 5)
# (grid, particle walls, handlers, species, array state, accumulation).  The long grid has two species in every case: its x
# faces are 20 cells of 1300, and one species of 16000 sends only some 40 particles through each.
CASES = [
    (A, "reflux6", "one", "one", "tile", "deterministic"),
    (A, "reflux6", "one", "one", "tile", "float"),
    (A, "reflux_absorb_reflect", "one", "two", "tile", "deterministic"),
    (A, "two_handlers", "two", "two", "tile", "deterministic"),
    (A, "unregistered", "one", "one", "tile", "deterministic"),
    (A, "two_handlers", "two", "two", "voxel", "float"),
    (A, "reflux_absorb_reflect", "one", "one", "voxel", "deterministic"),
    (A, "reflux_absorb_reflect", "one", "one", "unsorted", "deterministic"),
    (A, "unregistered", "one", "two", "unsorted", "float"),
    (A, "reflux6", "one", "one", "tile_only", "deterministic"),
    (A, "reflux_absorb_reflect", "one", "one", "tile_only", "float"),
    (A, "unregistered", "one", "one", "tail_below", "deterministic"),
    (A, "two_handlers", "two", "one", "tail_above", "deterministic"),
    (A, "reflux6", "zero_second", "two", "tile", "deterministic"),
    (A, "reflux_absorb_reflect", "one", "with_chargeless_copy", "tile", "deterministic"),
    (A, "unregistered", "one", "with_chargeless_copy", "voxel", "float"),
    (B, "reflux6", "one", "one", "thin", "deterministic"),
    (B, "reflux_absorb_reflect", "one", "two", "thin", "float"),
    (B, "two_handlers", "two", "one", "thin", "deterministic"),
    (B, "unregistered", "one", "one", "thin", "deterministic"),
    (C_, "reflux6", "one", "two", "tile", "deterministic"),
    (C_, "reflux_absorb_reflect", "one", "two", "tile", "float"),
    (C_, "two_handlers", "two", "two", "voxel", "deterministic"),
    (C_, "unregistered", "one", "two", "tile", "deterministic"),
    (X, "reflux_x", "hot_x", "one", "thin", "deterministic"),
    (X, "reflux_x", "hot_x", "two", "thin", "float"),
]


def case_of(c):
    return dict(zip(("dims", "walls", "handlers", "species", "state", "mode"), c))


def case_id(c):
    return "%dx%dx%d-%s-%s-%s-%s-%s" % (c[0] + c[1:])


def oracle_world(c):
    """The case on the oracle alone: orc_advance_p, then rounds with the oracle's own logf.  Returns the rounds as a list
    of lists (one Round per species, None for a species without movers) and the movers each species had before each."""
    case = case_of(c)
    _, _, og = grids(case)
    fi = D.interpolator(og)
    n_sp = len(SPECIES[case["species"]])
    n = N_PARTICLES[case["dims"]]
    draws = draw_table(n + 64)
    state = []
    for s in range(n_sp):
        r = D.Pushed(og, species_particles(case, s), fi, SCALE, SPECIES[case["species"]][s][0])
        state.append((r.p, r.pm))
    f, a = np.zeros(og.nv, L.field_t), np.zeros(og.nv + 1, L.accumulator_t)
    rounds, movers = [], []
    while any(len(pm) for _, pm in state) and len(rounds) <= MAX_ROUNDS:
        movers.append([len(pm) for _, pm in state])
        this = []
        for s, (p, pm) in enumerate(state):
            r = predict_round(og, p, pm, s, handlers_of(case, s), draws, f, a) if len(pm) else None
            this.append(r)
            if r is not None:
                state[s] = (r.p, r.pm)
        rounds.append(this)
    return og, rounds, movers


# ---- the surface emitter (vpic_hip_emit) in test mode: the arithmetic include/vpic_hip.h states, one operation per line -----
EMIT_FACES = {12: (0, 1), 10: (1, 1), 4: (2, 1), 14: (0, -1), 16: (1, -1), 22: (2, -1)}    # BOUNDARY code -> (axis, dir)
COEF = {"child_langmuir": 32.0 / 81.0, "ccube": 1.0, "ivory": 1.0 / 6.0}


def _emit_common(og, fi, comps, n_emit, q_m, thresh):
    """per slot t = component index * n_emit + k: (emits, cell, axis, dir, normal field)"""
    comps = np.asarray(comps, np.int64)
    c = np.repeat(np.arange(len(comps)), n_emit)
    cell, typ = comps[c] >> 5, comps[c] & 31
    axis = np.array([EMIT_FACES.get(int(t), (-1, 0))[0] for t in typ])
    dirn = np.array([EMIT_FACES.get(int(t), (-1, 0))[1] for t in typ]).astype(F)
    sy, sz = og.nx + 2, (og.nx + 2) * (og.ny + 2)
    real = (axis >= 0) & (cell > 0) & (cell < og.nv - sz - sy - 1)
    at = np.where(real, cell, 0)
    en = np.choose(np.maximum(axis, 0), [fi["ex"][at], fi["ey"][at], fi["ez"][at]]).astype(F)
    emits = real & (F(q_m) * (dirn * en) > 0) & (np.abs(en) >= F(thresh))
    return emits, cell, axis, dirn, en


def _emit_records(emits, cell, pos, u, qp, disp, sp_id):
    inj = np.zeros(int(emits.sum()), L.particle_injector_t)
    for k, name in enumerate(("dx", "dy", "dz")):
        inj[name] = pos[k][emits]
    for k, name in enumerate(("ux", "uy", "uz")):
        inj[name] = u[k][emits]
    for k, name in enumerate(("dispx", "dispy", "dispz")):
        inj[name] = disp[k][emits]
    inj["i"], inj["q"], inj["sp_id"] = cell[emits], qp[emits], sp_id
    return inj


def _emit_draw_side(axis, dirn, ut_perp, ut_para, d):
    """position on the face and momenta from the double draws, one rounding each -- the same expressions on the device and
    in the reference: pos = (float)(2 d - 1), u normal = (float)(dir |ut_para d2|), u tangential = (float)(ut_perp d)"""
    n = len(axis)
    pos, u = [np.zeros(n, F) for _ in range(3)], [np.zeros(n, F) for _ in range(3)]
    para, perp = np.float64(F(ut_para)), np.float64(F(ut_perp))
    for a in range(3):
        m = axis == a
        ay, az = (a + 1) % 3, (a + 2) % 3
        pos[a][m] = -dirn[m]
        pos[ay][m] = (2 * d[m, 0] - 1).astype(F)
        pos[az][m] = (2 * d[m, 1] - 1).astype(F)
        u[a][m] = (dirn[m].astype(np.float64) * np.abs(para * d[m, 2])).astype(F)
        u[ay][m] = (perp * d[m, 3]).astype(F)
        u[az][m] = (perp * d[m, 4]).astype(F)
    return pos, u


def emit_restatement(og, fi, comps, n_emit, ut_perp, ut_para, q_m, coef, thresh, slot_draws, sp_id=0):
    """vpic_hip_emit in test mode, operation by operation in float32 (include/vpic_hip.h).  slot_draws: float64[n, 6] indexed
    by slot.  Returns (the injector records of the emitting slots, in slot order; the particle records whose accumulate_rhob
    the emitter adds: the position on the face with the charge negated)."""
    emits, cell, axis, dirn, en = _emit_common(og, fi, comps, n_emit, q_m, thresh)
    d = np.asarray(slot_draws, np.float64).reshape(-1, 6)[:len(emits)]
    size, rsize = [F(og.dx), F(og.dy), F(og.dz)], [F(og.rdx), F(og.rdy), F(og.rdz)]
    ax = np.maximum(axis, 0)
    dX, dY, dZ = [np.array([size[(a + j) % 3] for a in ax], F) for j in range(3)]
    pos, u = _emit_draw_side(axis, dirn, ut_perp, ut_para, d)
    with np.errstate(invalid="ignore", divide="ignore"):
        e3 = F(q_m) * en
        e3 = e3 * en
        e3 = e3 * en
        s = F(coef) * np.abs(e3)
        s = s / dX
        s = np.sqrt(s)
        qp = F(og.eps0) * dY
        qp = qp * dZ
        qp = qp * F(og.dt)
        qp = qp * s
        qp = qp / F(n_emit)
        if q_m < 0:
            qp = -qp
        g = u[0] * u[0] + u[1] * u[1]
        g = g + u[2] * u[2]
        g = g + F(1)
        age = d[:, 5].astype(F) * ((F(og.cvac) * F(og.dt)) / np.sqrt(g))
        disp = [(u[k] * age) * rsize[k] for k in range(3)]
    inj = _emit_records(emits, cell, pos, u, qp.astype(F), disp, sp_id)
    left = np.zeros(len(inj), L.particle_t)
    for name in ("dx", "dy", "dz", "i"):
        left[name] = inj[name]
    left["q"] = -inj["q"]
    return inj, left


def emit_reference(og, fi, comps, n_emit, ut_perp, ut_para, q_m, slot_draws, sp_id=0):
    """child-langmuir.c:43-97 as the oracle's orc_child_langmuir computes it, up to the injector: the charge with the
    square root in double and one rounding, the age in double, the displacements divided by the cell size
    (tests/test_source_ref.py holds it to orc_child_langmuir through orc_boundary_p_inject, particle for particle)"""
    emits, cell, axis, dirn, en = _emit_common(og, fi, comps, n_emit, q_m, 0.0)
    d = np.asarray(slot_draws, np.float64).reshape(-1, 6)[:len(emits)]
    size = [F(og.dx), F(og.dy), F(og.dz)]
    ax = np.maximum(axis, 0)
    dX, dY, dZ = [np.array([size[(a + j) % 3] for a in ax], F) for j in range(3)]
    pos, u = _emit_draw_side(axis, dirn, ut_perp, ut_para, d)
    e3 = ((F(q_m) * en) * en) * en
    pre = ((F(og.eps0) * dY) * dZ) * F(og.dt)                           # float products, as in the C expression
    qp = (pre.astype(np.float64) * np.sqrt((32. / 81.) * np.abs(e3).astype(np.float64) / dX.astype(np.float64)) / np.float64(F(n_emit))).astype(F)
    if q_m < 0:
        qp = -qp
    uc = [np.choose((ax + j) % 3, u) for j in range(3)]                 # the macro's X, Y, Z: the face's axis first, cyclically
    g = ((uc[0] * uc[0] + uc[1] * uc[1]) + uc[2] * uc[2]) + F(1)        # float, converted for sqrt
    age = (d[:, 5].astype(F).astype(np.float64) * (np.float64(F(og.cvac) * F(og.dt)) / np.sqrt(g.astype(np.float64)))).astype(F)
    disp = [(u[k] * age) / size[k] for k in range(3)]
    return _emit_records(emits, cell, pos, u, qp, disp, sp_id)


def slot_table(emits_per_slot, draws_in_emission_order):
    """float64[n_slots, 6]: the draws the reference consumed, in emission order, placed at the slots that emit"""
    t = np.zeros((len(emits_per_slot), 6))
    t[emits_per_slot] = draws_in_emission_order
    return t
