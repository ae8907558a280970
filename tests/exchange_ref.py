"""What tests/test_exchange_ref.py (CPU) and tests/test_gpu_exchange.py (GPU) share: a reference WORLD of a few domains on
the CPU, and the seeded inputs of the exchange cases.

A world holds domains built from pyorc arrays -- grid, species arrays, mover lists, accumulator, a field array for rhob --
wired by the particle codes of their faces: a code >= 0 that is not the domain's own rank names the domain across that face
(old-vpic_amd/engine.py: make_grid), and what leaves through face f arrives through face (f + 3) % 6 there.  Its operations
are the oracle's own, which restate the reference's boundary_p.c operation by operation (oracle/vpic_oracle.c):
push = orc_advance_p, pack = orc_boundary_p_pack with room for every mover, inject = orc_boundary_p_inject per species.
It has no capacities and never overflows: an exchange that takes the device several rounds because a message was full is
compared with it by totals.  With a fixed-point scale it also carries the exact integer sums of every deposit
(pyorc.fixed_accumulator / finalize, as tests/det_exact.py does for one push).

Nothing here touches a GPU."""
import contextlib
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
import det_exact as X  # noqa: E402

L = importlib.import_module("old-vpic_amd.layout")

ABSORB, REFLECT = L.ABSORB_PARTICLES, L.REFLECT_PARTICLES
DT = X.DT
GRIDS = [(4, 4, 4), (5, 3, 2), (9, 2, 6), (1, 4, 3)]
N_HOT = 2000                                   # particles per species and domain in the statistical cases
PATTERN_COUNTS = [1, 63, 64, 65, 300]          # movers through one face in the pattern cases
P_WORDS = ("dx", "dy", "dz", "i", "ux", "uy", "uz", "q")
P_TAGGED = P_WORDS + ("tag", "tag2")
INJ_WORDS = ("dx", "dy", "dz", "i", "ux", "uy", "uz", "q", "dispx", "dispy", "dispz", "sp_id")
DISP = ("dispx", "dispy", "dispz")
Q_M = [-1.0, 0.5, -0.25, 2.0]                  # charge to mass of up to four species
TAGGED = [True, False, True, False]            # "four species, two of which carry tags"

# particle codes of the faces -x -y -z +x +y +z, per rank, of the worlds the cases use
WORLDS = {
    # two slabs cut in x, periodic in y and z: the one geometry that is a consistent cut of a periodic box (2 nx, ny, nz)
    "slabs": [[1, 0, 0, 1, 0, 0], [0, 1, 1, 0, 1, 1]],
    # every face of either domain belongs to the other: movers through all six faces, corners that take three rounds
    "all_shared": [[1] * 6, [0] * 6],
    # domain 0 absorbs on -x and on both z faces, sends through +x; y wraps onto itself.  Domain 1 reflects elsewhere.
    "absorbing": [[ABSORB, 0, ABSORB, 1, 0, ABSORB], [0, REFLECT, REFLECT, REFLECT, REFLECT, REFLECT]],
    # one shared face only (+x of 0 / -x of 1), the rest reflects: the pattern cases count movers through exactly that face
    "one_face": [[REFLECT, REFLECT, REFLECT, 1, REFLECT, REFLECT], [0, REFLECT, REFLECT, REFLECT, REFLECT, REFLECT]],
}


# ---- multisets of records, bit for bit -------------------------------------------------------------------------------------
def rows(a, names):
    """The words `names` of every record of a as one uint64 matrix [n, len(names)] (floats by their bits), rows sorted"""
    if len(a) == 0:
        return np.zeros((0, len(names)), np.uint64)
    cols = [np.ascontiguousarray(a[n]).view("u%d" % a.dtype[n].itemsize).astype(np.uint64) for n in names]
    m = np.stack(cols, 1)
    return m[np.lexsort(m.T[::-1])]


def same_multiset(a, b, names):
    ra, rb = rows(a, names), rows(b, names)
    return ra.shape == rb.shape and bool(np.array_equal(ra, rb))


def sub_multiset(a, b, names):
    """every record of a is one of b's, as often at the most"""
    ra, rb = rows(a, names), rows(b, names)
    keys = np.unique(np.concatenate([ra, rb]), axis=0, return_inverse=True)[1].reshape(-1)
    ka, kb = keys[:len(ra)], keys[len(ra):]
    n = int(keys.max()) + 1 if len(keys) else 0
    return bool(np.all(np.bincount(ka, minlength=n) <= np.bincount(kb, minlength=n)))


def all_different(a, names):
    r = rows(a, names)
    return len(r) < 2 or bool(np.any(r[1:] != r[:-1], axis=1).all())


def mover_pairs(p, pm):
    """(particle at the mover's slot, displacement left) as one structured array of injector records with sp_id 0: the
    form in which movers are compared as multisets (slots differ between the device and the reference)"""
    out = np.zeros(len(pm), L.particle_injector_t)
    for c in P_WORDS:
        out[c] = p[c][pm["i"]]
    for c in DISP:
        out[c] = pm[c]
    return out


# ---- the world -------------------------------------------------------------------------------------------------------------
class Domain:
    def __init__(self, rank, dims, pbc, dt):
        nx, ny, nz = dims
        self.rank, self.dims, self.pbc = rank, dims, list(pbc)
        self.args = (nx, ny, nz, float(nx), float(ny), float(nz), np.float32(dt))
        self.kw = dict(pbc=list(pbc), rank=rank)
        self.og = pyorc.make_grid(*self.args, **self.kw)
        self.fi = np.zeros(self.og.nv, L.interpolator_t)
        self.f = np.zeros(self.og.nv, L.field_t)
        self.a = np.zeros(self.og.nv + 1, L.accumulator_t)
        self.a64 = np.zeros((self.og.nv, 12), np.int64)
        self.species = []

    def shared(self, face):
        return self.pbc[face] >= 0 and self.pbc[face] != self.rank

    def add_species(self, q_m, p, room):
        s = dict(q_m=q_m, p=np.zeros(room, L.particle_t), np=len(p), pm=np.zeros(room, L.particle_mover_t), nm=0)
        s["p"][:len(p)] = p
        self.species.append(s)
        return len(self.species) - 1

    def live(self, k):
        s = self.species[k]
        return s["p"][:s["np"]]

    def movers(self, k):
        s = self.species[k]
        return s["pm"][:s["nm"]]


class World:
    """domains[rank] of equal dims with the face codes of WORLDS[name] (or `name` itself, a list of six codes per rank);
    scale: the fixed-point scale of a deterministic comparison, or None"""

    def __init__(self, name, dims, dt=DT, fi_seed=7, scale=None):
        codes = WORLDS[name] if isinstance(name, str) else name
        self.domains = [Domain(r, dims, pbc, dt) for r, pbc in enumerate(codes)]
        self.scale = scale
        if fi_seed is not None:
            for d in self.domains:
                d.fi = X.interpolator(d.og, seed=fi_seed + d.rank)

    @contextlib.contextmanager
    def _sums(self, d):
        if self.scale is None:
            yield
        else:
            with pyorc.fixed_accumulator(d.og, self.scale) as (a64, _):
                yield
                d.a64 += a64

    def push(self, rank, k):
        d = self.domains[rank]
        s = d.species[k]
        with self._sums(d):
            s["nm"] = pyorc.advance_p(s["p"], s["np"], s["q_m"], s["pm"], d.a, d.fi, d.og)
        return s["nm"]

    def pack(self, rank, species=None):
        """the movers of the species listed (default: all) leave: per face the injector records, species after species"""
        d = self.domains[rank]
        out = [[] for _ in range(6)]
        for k in (range(len(d.species)) if species is None else species):
            s = d.species[k]
            if s["nm"] == 0:
                continue
            s["np"], per_face = pyorc.boundary_p_pack(s["p"], s["np"], s["pm"], s["nm"], k, d.f, d.og, s["nm"])
            s["nm"] = 0
            for f in range(6):
                out[f].append(per_face[f])
        return [np.concatenate(o) if o else np.zeros(0, L.particle_injector_t) for o in out]

    def inject(self, rank, records):
        d = self.domains[rank]
        for k, s in enumerate(d.species):
            mine = np.ascontiguousarray(records[records["sp_id"] == k])
            if len(mine):
                with self._sums(d):
                    s["np"], s["nm"] = pyorc.boundary_p_inject(s["p"], s["np"], s["pm"], s["nm"], mine, d.a, d.og)

    def destination(self, rank, face):
        return self.domains[rank].pbc[face], (face + 3) % 6

    def round(self, species=None):
        """one round for every domain: pack, then deliver.  Returns {(rank, face): records} of the messages that carry any."""
        sent = {}
        for d in self.domains:
            per_face = self.pack(d.rank, species)
            for f in range(6):
                assert d.shared(f) or len(per_face[f]) == 0
                if len(per_face[f]):
                    sent[(d.rank, f)] = per_face[f]
        for (rank, f), rec in sent.items():
            self.inject(self.destination(rank, f)[0], rec)
        return sent

    def exchange(self, max_rounds=6):
        """rounds until no mover is left anywhere; returns the list of their messages"""
        rounds = []
        for _ in range(max_rounds):
            if not any(s["nm"] for d in self.domains for s in d.species):
                return rounds
            rounds.append(self.round())
        raise AssertionError("movers left after %d rounds" % max_rounds)

    def finalized(self, rank):
        """the accumulator of a deterministic engine: finalize() of the exact sums"""
        return pyorc.finalize(self.domains[rank].a64, self.scale)


# ---- seeded inputs -----------------------------------------------------------------------------------------------------------
def hot(seed, dims, n=N_HOT, u=X.HOT, q0=-X.Q0, first_tag=1, tagged=True):
    p = X.particles(seed, n, dims, u, q0=q0, first_tag=first_tag)
    if not tagged:
        p["tag"] = 0
    return p


def through_face(seed, n, dims, face, q0=-X.Q0, first_tag=1, tagged=True):
    """n particles in the cell layer on `face`, 0.1 from it, on their way through it at |u| = 2 along the normal (1.7 per
    step at DT) and 1e-3 across, away from the other faces of their cells: each becomes exactly one mover for that face."""
    nx, ny, nz = dims
    rng = np.random.default_rng(seed)
    axis, hi = face % 3, face >= 3
    p = np.zeros(n, L.particle_t)
    for c in ("dx", "dy", "dz"):
        p[c] = rng.uniform(-0.5, 0.5, n).astype(np.float32)
    for c in ("ux", "uy", "uz"):
        p[c] = (1e-3 * rng.standard_normal(n)).astype(np.float32)
    xyz = [rng.integers(1, m + 1, n) for m in (nx, ny, nz)]
    xyz[axis][:] = dims[axis] if hi else 1
    p["i"] = L.voxel(xyz[0], xyz[1], xyz[2], nx, ny, nz)
    p["d" + "xyz"[axis]] = (0.9 if hi else -0.9) + rng.uniform(-0.05, 0.05, n).astype(np.float32)
    p["u" + "xyz"[axis]] = (2.0 if hi else -2.0) + rng.uniform(-0.05, 0.05, n).astype(np.float32)
    p["q"] = (q0 * rng.uniform(0.5, 1.5, n)).astype(np.float32)
    p["tag"] = (np.arange(n) + first_tag) if tagged else 0
    return p


def corner_particle(dims, first_tag=1):
    """One particle in the last cell of the grid that meets the +x face after 0.1, the +y face after 0.2 and the +z face
    after 0.3 of the 1.05 it travels along every axis: three rounds in a world whose six faces are shared."""
    nx, ny, nz = dims
    p = np.zeros(1, L.particle_t)
    p["dx"], p["dy"], p["dz"] = 0.9, 0.8, 0.7
    p["ux"] = p["uy"] = p["uz"] = 2.0
    p["i"] = L.voxel(nx, ny, nz, nx, ny, nz)
    p["q"] = np.float32(-0.0123456)             # (CORNER_Q: no other particle of a case has it)
    p["tag"] = first_tag
    return p


def interleaved(records, seed=3):
    """the records of a message in a seeded random order: species mixed record by record"""
    return np.ascontiguousarray(records[np.random.default_rng(seed).permutation(len(records))])


def species_in_windows(records, width=64):
    """the largest number of different species among `width` consecutive records"""
    s = records["sp_id"]
    return max((len(np.unique(s[k:k + width])) for k in range(0, max(len(s) - width, 0) + 1)), default=0)


def faces_of_movers(d, k):
    """the face each mover of species k of domain d sits on, in list order: the first face 0..5 whose test of
    boundary_p.c:304-309 holds (-1: none)"""
    s = d.species[k]
    p = s["p"][s["pm"]["i"][:s["nm"]]]
    face = np.full(len(p), -1)
    for f in reversed(range(6)):
        c, hi = "xyz"[f % 3], f >= 3
        cond = (p["d" + c] == 1) & (p["u" + c] > 0) if hi else (p["d" + c] == -1) & (p["u" + c] < 0)
        face[cond] = f
    return face


def four_species_world(name, dims, seed=100, n=N_HOT, scale=None, dt=DT, room=None, q0s=None):
    """A world of two domains with four hot species each (Q_M, TAGGED); every particle of the world has its own bits."""
    w = World(name, dims, dt=dt, scale=scale)
    for d in w.domains:
        for k in range(4):
            q0 = -X.Q0 * (k + 1) if q0s is None else q0s[k]
            p = hot(seed + 10 * d.rank + k, dims, n=n, q0=q0, first_tag=1 + 10 ** 6 * (4 * d.rank + k), tagged=TAGGED[k])
            d.add_species(Q_M[k], p, room or 4 * n)
    return w


def pattern_world(dims, n, scale=None):
    """world "one_face": domain 0 holds n particles on their way through +x and 200 cold ones, domain 1 100 cold ones"""
    w = World("one_face", dims, scale=scale)
    cold = [hot(21, dims, n=200, u=X.COLD, first_tag=1), hot(23, dims, n=100, u=X.COLD, first_tag=5001)]
    for c in cold:                                          # (in the middle half of their cells: none of them reaches a face)
        for x in ("dx", "dy", "dz"):
            c[x] *= np.float32(0.5)
    p = np.concatenate([cold[0], through_face(22 + n, n, dims, 3, first_tag=1001)])
    w.domains[0].add_species(Q_M[0], p, 2 * len(p) + 64)
    w.domains[1].add_species(Q_M[0], cold[1], 2 * len(p) + 164)
    return w


CORNER_Q = np.float32(-0.0123456)


def corner_world(dims, scale=None):
    """world "all_shared" with one species: N_HOT hot particles per domain and the corner particle in domain 0"""
    w = World("all_shared", dims, scale=scale)
    c = corner_particle(dims, first_tag=9 * 10 ** 6)
    w.domains[0].add_species(Q_M[0], np.concatenate([hot(31, dims, first_tag=1), c]), 4 * N_HOT)
    w.domains[1].add_species(Q_M[0], hot(32, dims, first_tag=10 ** 6), 4 * N_HOT)
    assert not np.any(np.concatenate([w.domains[0].live(0)[:-1], w.domains[1].live(0)])["q"] == CORNER_Q)
    return w


def absorbing_world(dims, scale=None):
    """world "absorbing" with one hot species per domain"""
    w = World("absorbing", dims, scale=scale)
    w.domains[0].add_species(Q_M[0], hot(41, dims, first_tag=1), 4 * N_HOT)
    w.domains[1].add_species(Q_M[0], hot(42, dims, first_tag=10 ** 6), 4 * N_HOT)
    return w


def absorbed_addends(d, k):
    """What the absorbing faces of domain d will add to rhob when species k's movers are packed, from the reference's own
    accumulate_rhob one particle at a time: (node indices int64[m, 8], addends float32[m, 8]) of the m absorbed movers"""
    s = d.species[k]
    face = faces_of_movers(d, k)
    gone = np.array([f < 0 or d.pbc[f] == ABSORB for f in face], bool)
    idx = s["pm"]["i"][:s["nm"]][gone]
    nx, ny, _ = d.dims
    sy, sz = nx + 2, (nx + 2) * (ny + 2)
    off = np.array([0, 1, sy, sy + 1, sz, sz + 1, sz + sy, sz + sy + 1])
    nodes = s["p"]["i"][idx].astype(np.int64)[:, None] + off[None, :]
    w = np.zeros((len(idx), 8), np.float32)
    f = np.zeros(d.og.nv, L.field_t)
    for m, i in enumerate(idx):
        f["rhob"][nodes[m]] = 0
        pyorc.accumulate_rhob(f, s["p"][i:i + 1], d.og)
        w[m] = f["rhob"][nodes[m]]
    return nodes, w


def rhob_bound(nv, nodes, w):
    """(exact sums float64[nv], bound float64[nv]) per node: a float sum of n addends in any order is within
    gamma_n sum |w| of the exact one, gamma_n = n u / (1 - n u), u = 2^-24"""
    exact, mag, n = np.zeros(nv), np.zeros(nv), np.zeros(nv)
    np.add.at(exact, nodes.reshape(-1), w.astype(np.float64).reshape(-1))
    np.add.at(mag, nodes.reshape(-1), np.abs(w.astype(np.float64)).reshape(-1))
    np.add.at(n, nodes.reshape(-1), (w.reshape(-1) != 0).astype(np.float64))
    u = 2.0 ** -24
    return exact, n * u / (1 - n * u) * mag
