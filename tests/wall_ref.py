"""What tests/test_wall_ref.py (CPU) and tests/test_gpu_wall.py (GPU) share: absorbing walls that tally and record what
they take (include/vpic_hip.h: vpic_hip_wall_*), restated in numpy.

Three things: the TAKER rule (which mover is absorbed at which face, absorbed_faces), the TALLY rule (tally: the table
[7][n_species] with Python integers as the exact check of the quantisation) and the RECORD prediction (records).

The oracle (source_ref.predict_round: orc_boundary_p_reflux_round, pinned on the reference's own boundary_p) sees a wall
code as VPIC_ABSORB_PARTICLES on that face (oracle_grid): both absorb at the first met face, with the same rhob.  So
predict_round on such a grid is the reference for survivors, refluxed particles, movers and rhob, and its Round.absorbed
is what the taker rule must call absorbed.

Nothing here touches a GPU."""
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import source_ref as S  # noqa: E402
from source_ref import D, L, pyorc, F  # noqa: E402

REFLECT, ABSORB = S.REFLECT, S.ABSORB
TALLY, RECORD = L.WALL_TALLY, L.WALL_RECORD
ROWS = L.WALL_ROWS
P_WORDS = ("dx", "dy", "dz", "i", "ux", "uy", "uz", "q")
R_WORDS = P_WORDS + ("tag", "tag2", "face", "sp")

# Quanta of the sums of q and of q * ke that refuse nothing here: |q| < 2 Q0 and ke < 2^8 (momenta ~ N(0, 1) per axis) give
# |t| < 2^33 Q0 / quantum, so a quantum of Q0 2^-20 keeps |t| below 2^13 ... 2^29.
QUANTA = (D.Q0 * 2.0 ** -20, D.Q0 * 2.0 ** -20)
# Quanta that refuse SOME: |q| / quantum < 2^32 only for |q| < 1.2 Q0 (the charges run from Q0 up to Q0 (1 + n 2^-14), n in
# the thousands), and |q| ke / quantum < 2^32 only for |q| ke < Q0 (ke of a hot particle is of order 1)
REFUSING_QUANTA = (1.2 * D.Q0 * 2.0 ** -32, D.Q0 * 2.0 ** -32)

# wall layouts, faces -x -y -z +x +y +z: the particle codes, {wall code: its flags}, the name of the reflux handlers
LAYOUTS = {
    "wall6": dict(walls=[-3, -4, ABSORB, -3, -4, ABSORB], walled={-3: TALLY, -4: TALLY | RECORD, ABSORB: TALLY}, handlers=None),
    "mixed": dict(walls=[-3, -4, REFLECT, -4, ABSORB, REFLECT], walled={-4: TALLY | RECORD}, handlers="one"),      # ABSORB not registered: row 6
    "nowhere": dict(walls=[-4, -5, 0, -4, -5, 0], walled={-4: TALLY}, handlers=None),                              # -5 registered nowhere: row 6
}
A, B, C_, X = (10, 9, 7), (5, 3, 2), (65, 5, 4), (1, 6, 5)
# (grid, layout, species, array state, accumulation): every layout on the four grids of source_ref.N_PARTICLES, every layout
# in both accumulation modes, every state of source_ref.STATES; the long grid has two species in every case (its x faces
# take only some 30 particles of one)
CASES = [
    (A, "wall6", "two", "tile", "deterministic"),
    (A, "wall6", "one", "tile", "float"),
    (A, "wall6", "with_chargeless_copy", "voxel", "deterministic"),
    (A, "wall6", "one", "unsorted", "float"),
    (A, "wall6", "one", "tile_only", "deterministic"),
    (A, "mixed", "two", "tile", "deterministic"),
    (A, "mixed", "one", "voxel", "float"),
    (A, "mixed", "with_chargeless_copy", "tile", "deterministic"),
    (A, "mixed", "one", "tail_below", "deterministic"),
    (A, "nowhere", "two", "tile", "float"),
    (A, "nowhere", "one", "tail_above", "deterministic"),
    (A, "nowhere", "with_chargeless_copy", "unsorted", "float"),
    (B, "wall6", "two", "thin", "deterministic"),
    (B, "mixed", "one", "thin", "float"),
    (B, "nowhere", "two", "thin", "deterministic"),
    (C_, "wall6", "two", "tile", "float"),
    (C_, "mixed", "two", "voxel", "deterministic"),
    (C_, "nowhere", "two", "tile", "deterministic"),
    (X, "wall6", "two", "thin", "float"),
    (X, "mixed", "two", "thin", "deterministic"),
    (X, "nowhere", "one", "thin", "deterministic"),
]


def case_of(c):
    """the case as a dict that source_ref's helpers take (species_particles, handlers_of)"""
    lay = LAYOUTS[c[1]]
    return dict(dims=c[0], layout=c[1], walls=lay["walls"], walled=lay["walled"], handlers=lay["handlers"], species=c[2],
                state=c[3], mode=c[4])


def case_id(c):
    return "%dx%dx%d-%s-%s-%s-%s" % (c[0] + c[1:])


def handlers_of(case, s):
    return S.handlers_of(case, s) if case["handlers"] else []


def reflux_codes(case):
    return sorted(S.HANDLERS[case["handlers"]]) if case["handlers"] else []


def grids(case):
    """(engine grid arguments, keywords, the oracle's grid): source_ref.grids for a list of codes.  The engine's grid has the
    wall codes; the oracle's has VPIC_ABSORB_PARTICLES in their place (oracle_codes)."""
    args, kw, _ = D.grids(case["dims"], case["walls"])
    if case["dims"][0] == 1:                                           # (the one-cell grid is a slab: source_ref.grids)
        args = args[:3] + (0.25,) + args[4:]
    og = pyorc.make_grid(*args, pbc=oracle_codes(case["walls"], case["walled"]))
    return args, kw, og


def oracle_codes(codes, walled):
    return [ABSORB if c in walled else c for c in codes]


# ---- the taker rule ------------------------------------------------------------------------------------------------------------
def met(rec, f):
    """face f is met: the stored position component on its axis is exactly -1 / +1 and the momentum points out"""
    c, hi = "xyz"[f % 3], f >= 3
    return (rec["d" + c] == 1) & (rec["u" + c] > 0) if hi else (rec["d" + c] == -1) & (rec["u" + c] < 0)


def absorbed_faces(p, pm, codes, walled, reflux=(), rank=0):
    """int[len(pm)]: the face 0..5 at which each mover is absorbed, 6 for "none", -1 for a mover that is not absorbed (sent
    to another domain or refluxed).  The faces are walked in order; at the first met face whose code is a wall or
    VPIC_ABSORB_PARTICLES the mover is absorbed there; a shared face sends, a registered reflux code refluxes; anything
    else passes the mover on."""
    rec = p[pm["i"]]
    out = np.full(len(pm), -1)
    open_ = np.ones(len(pm), bool)
    for f in range(6):
        m = open_ & met(rec, f)
        code = codes[f]
        if code in walled or code == ABSORB:
            out[m] = f
            open_ &= ~m
        elif (code >= 0 and code != rank) or (code <= -3 and code in reflux):
            open_ &= ~m
    out[open_] = 6
    return out


# ---- the tally rule -------------------------------------------------------------------------------------------------------------
def kinetic(rec):
    """VPIC_HIP_COORD_KE of each record in IEEE double, every operation rounded once: sqrt(((1 + ux ux) + uy uy) + uz uz) - 1"""
    ux, uy, uz = (rec[c].astype(np.float64) for c in ("ux", "uy", "uz"))
    return np.sqrt(((1.0 + ux * ux) + uy * uy) + uz * uz) - 1.0


def quantised(rec, quanta):
    """(taken bool[n, 2], addends: a list of n pairs of Python integers) of the values q and q * ke"""
    q = rec["q"].astype(np.float64)
    val = np.stack([q, q * kinetic(rec)], 1)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        t = val / np.asarray(quanta, np.float64)[None, :]
        taken = np.abs(t) < 4294967296.0                                # (a NaN is refused)
    add = [[int(np.rint(t[k, j])) if taken[k, j] else 0 for j in range(2)] for k in range(len(rec))]   # rint: to nearest, ties to even, as llrint
    for k in range(len(rec)):                                          # the exact check: Python's own rounding of the same quotient
        for j in range(2):
            if taken[k, j]:
                assert add[k][j] == round(float(t[k, j])) and math.isfinite(t[k, j])
    return taken, add


def tally(rec, faces, sp, codes, walled, quanta, table=None, n_species=1):
    """Adds the absorbed particles rec (absorbed at `faces`, 0..6) of species sp to the table (L.wall_tally_t[7, n_species], made
    when None) and returns it.  The sums are formed as Python integers and must fit 64 bits."""
    if table is None:
        table = np.zeros((ROWS, n_species), L.wall_tally_t)
    taken, add = quantised(rec, quanta)
    count = [0] * ROWS
    isum = [[0, 0] for _ in range(ROWS)]
    refused = [[0, 0] for _ in range(ROWS)]
    for k in range(len(rec)):
        f = int(faces[k])
        assert 0 <= f <= 6
        row = f if f < 6 and codes[f] in walled else 6
        count[row] += 1
        for j in range(2):
            if taken[k, j]:
                isum[row][j] += add[k][j]
            else:
                refused[row][j] += 1
    for row in range(ROWS):
        table["count"][row, sp] += count[row]
        for j in range(2):
            total = int(table["isum"][row, sp, j]) + isum[row][j]
            assert -2 ** 63 <= total < 2 ** 63
            table["isum"][row, sp, j] = total
            table["refused"][row, sp, j] += refused[row][j]
    return table


# ---- the records ---------------------------------------------------------------------------------------------------------------
def records(rec, faces, sp, codes, walled, tagged=True):
    """L.wall_record_t of the absorbed particles whose face is a wall registered with RECORD: the particle as stored, its two
    tags (0 for a species without tags), the face and the species"""
    keep = np.array([f < 6 and (walled.get(codes[f], 0) & RECORD) != 0 for f in faces], bool)
    src = rec[keep]
    out = np.zeros(len(src), L.wall_record_t)
    for c in P_WORDS:
        out[c] = src[c]
    if tagged:
        out["tag"], out["tag2"] = src["tag"], src["tag2"]
    out["face"], out["sp"] = np.asarray(faces)[keep], sp
    return out


def same_records(a, b):
    """a and b are the same multiset of records, byte for byte"""
    ra = np.sort(np.ascontiguousarray(a).view(np.dtype((np.void, L.wall_record_t.itemsize))).ravel())
    rb = np.sort(np.ascontiguousarray(b).view(np.dtype((np.void, L.wall_record_t.itemsize))).ravel())
    return len(ra) == len(rb) and bool(np.all(ra == rb))


def same_table(a, b):
    return all(np.array_equal(a[n], b[n]) for n in ("count", "isum", "refused"))


def describe_table(got, want):
    bad = [(row, sp, n) for n in ("count", "isum", "refused") for row in range(ROWS) for sp in range(want.shape[1])
           if not np.array_equal(got[n][row, sp], want[n][row, sp])]
    return "; ".join("row %d species %d %s: got %s, want %s" % (r, s, n, got[n][r, s], want[n][r, s]) for r, s, n in bad[:6])


# ---- a pushed case on the oracle alone -------------------------------------------------------------------------------------------
_WORLDS = {}


def oracle_world(c):
    """The case on the oracle alone (cached by grid, layout and species): one advance_p of source_ref.species_particles, then
    rounds with the oracle's own logf.  Returns (oracle grid, rounds): per round and species None (no movers) or
    (p, pm, Round) -- the state before the round and what predict_round made of it."""
    key = (c[0], c[1], c[2])
    if key in _WORLDS:
        return _WORLDS[key]
    case = case_of(c)
    _, _, og = grids(case)
    fi = D.interpolator(og)
    species = S.SPECIES[case["species"]]
    n = S.N_PARTICLES[case["dims"]]
    draws = S.draw_table(n + 64)
    state = []
    for s in range(len(species)):
        r = D.Pushed(og, S.species_particles(case, s), fi, S.SCALE, species[s][0])
        state.append((r.p, r.pm))
    f, a = np.zeros(og.nv, L.field_t), np.zeros(og.nv + 1, L.accumulator_t)
    rounds = []
    while any(len(pm) for _, pm in state):
        assert len(rounds) <= S.MAX_ROUNDS
        this = []
        for s, (p, pm) in enumerate(state):
            if len(pm) == 0:
                this.append(None)
                continue
            r = S.predict_round(og, p, pm, s, handlers_of(case, s), draws, f, a)
            this.append((p, pm, r))
            state[s] = (r.p, r.pm)
        rounds.append(this)
    _WORLDS[key] = (og, rounds)
    return _WORLDS[key]


# ---- parked movers: every ordered pairing of the wall kinds on the faces -x and -y ----------------------------------------------
# kind -> (particle code, wall flags or 0, a reflux handler)
KINDS = {"wall_record": (-4, TALLY | RECORD, False), "wall": (-6, TALLY, False), "absorb": (ABSORB, 0, False),
         "nowhere": (-5, 0, False), "reflux": (-3, 0, True), "reflect": (REFLECT, 0, False), "self": (0, 0, False)}


def parked_pairings():
    """[(first kind, second kind, particle codes, {wall code: flags}, has a reflux handler)]: the other faces reflect, or
    belong to this same domain opposite a face that does (source_ref.parked_pairings)"""
    out = []
    for a in KINDS:
        for b in KINDS:
            opposite = lambda kind: 0 if kind == "self" else REFLECT
            codes = [KINDS[a][0], KINDS[b][0], REFLECT, opposite(a), opposite(b), REFLECT]
            walled = {KINDS[k][0]: KINDS[k][1] for k in (a, b) if KINDS[k][1]}
            out.append((a, b, codes, walled, KINDS[a][2] or KINDS[b][2]))
    return out


PARKED_HANDLERS = [(-3, F(0.11), F(0.04))]
