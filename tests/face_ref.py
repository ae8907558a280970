"""A reference world for the face messages domains exchange with OTHER domains (include/vpic_hip.h: _pack_tang_b / _pack_jf /
_pack_rho / _pack_face_message / _pack_hydro, their unpacks, the _local_adjust_* and _synchronize_*_self pieces).  CPU only.

A world is a gpx x gpy x gpz decomposition of a box into equal bricks, rank = ix + gpx * (iy + gpy * iz); every brick has a
field_t and a hydro_t array, and the world moves them with the oracle's own pieces (oracle/pyorc.py) in the order
old-vpic_amd/domain.py calls them: the local adjustment first, then the axes x, y, z, and per axis the _self piece on every
domain followed by "every domain packs both directions, then every domain unpacks both" (the _self piece does nothing on a
domain whose two faces of the axis are not both its own, so calling it everywhere also shows that it leaves such a domain
alone).  `schedule(family)` is that order as a list of Piece records; a test applies the same record to this world and to
the engines and compares after every one.  The world keeps every message it packed in `msgs[(sender, dir)]`.

A message travelling in direction `dir` (0..5 = -x -y -z +x +y +z) leaves through face `dir` of the sender, goes to
fbc[dir] of the sender, and is unpacked there with the same `dir`.

Families: tang_b, jf, rho, msg0 (normal E), msg1 (div_b_err), msg2 (tangential E and normal B, with err), hydro.

Inputs, two generators (both pairwise different over the whole world, `assert_distinct`, so that a value read from the
wrong voxel, component or domain cannot compare equal):
  exact    every float word of the field arrays (and, separately, of the hydro arrays) of the world is k * 2^-6 for a
           different integer k with |k| <= (number of such words), signs mixed.  The largest world of the tests has
           2^17.4 of them, so |value| < 2^11.4: a sum of eight of them doubled is a multiple of 2^-6 below 2^15.4
           (22 bits), an average of eight a multiple of 2^-9 below 2^11.4 (21 bits) -- exact in float; a difference of
           two such averages has 22 bits, its square 44 -- exact in double.  The sum of the squares of one piece is exact
           while it stays below 2^35 (multiples of 2^-18): `exact_err` recomputes it in integers and asserts that room
           for the inputs at hand.  So every sum is the same in any order.
  general  standard normal draws times 10^U(-5, 2), redrawn until every word is finite with 1e-6 <= |v| <= 1e3: roundings
           (and a contracted multiply-add) show.

gather(): the one-domain array a world's bricks stand for.  A word of a brick belongs to the global array over exactly its
component's mesh extent (edge components 1..n along their own axis and 1..n+1 along the others, face components the other
way round, nodes 1..n+1 on all three axes).  Quantities neighbours hold partial sums of (jf, rhof, the 14 hydro moments:
unpacked with weights 1, 1) are ADDED onto the global word; quantities every neighbour holds a copy of that the exchange
averages (rhob with its half weights, and cB / E / tca of kind 2) take the MEAN of the copies (1, 2, 4 or 8 of them, so
the mean is exact on exact inputs)."""
import collections
import ctypes as C
import functools
import importlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import pyorc  # noqa: E402

L = importlib.import_module("old-vpic_amd.layout")

WALLS = {"pec": L.PEC_FIELDS, "symmetric": L.SYMMETRIC_FIELDS, "pmc": L.PMC_FIELDS, "absorb": L.ABSORB_FIELDS}
FIELD_FLOATS = [n for n in L.field_t.names if L.field_t[n] == np.float32]
FIELD_IDS = [n for n in L.field_t.names if L.field_t[n] == np.uint16]
HYDRO_FLOATS = list(L.hydro_t.names[:14])
assert len(FIELD_FLOATS) == 16 and len(FIELD_IDS) == 8 and L.hydro_t.itemsize == 64
CELL = (0.5, 0.25, 1.0)            # cell sizes of every world (any uniform mesh gives the weights 1, 1 and 1/2, 1/2)
DT = np.float32(0.1)
GUARD_WORD = np.uint32(0xFFFFFFFF)  # a NaN pattern no input holds
GUARD_WORDS = 256

Piece = collections.namedtuple("Piece", "op rank arg src")   # op: adjust | self (arg axis) | pack (arg dir) | unpack (arg dir, src sender)


def words(a):
    """any array as its raw uint32 words"""
    return np.ascontiguousarray(a).view(np.uint32).reshape(-1)


def float_words(a):
    """the float words of a field_t / hydro_t array (for hydro_t all 16, the two pad words included)"""
    w = np.ascontiguousarray(a).view(np.uint32).reshape(len(a), -1)
    return w[:, :16].reshape(-1)


def assert_distinct(w, what=""):
    w = np.asarray(w).reshape(-1)
    assert len(np.unique(w)) == len(w), (what, "words repeat", len(w) - len(np.unique(w)))


# ---- families -----------------------------------------------------------------------------------------------------------------
class Family:
    """array: 'f' or 'h'; adjust(a, g), self_(a, g, axis) -> err or None; count(g, d); c_pack / c_unpack: the oracle's C
    entry points taking (buf, a, g[, kind], d) / (a, buf, g[, kind], d); by_axis: the exchange goes axis by axis (False:
    every shared direction at once, as exchange_tang_b does); err: the unpack returns a squared-difference sum"""

    def __init__(self, name, array, count, c_pack, c_unpack, kind=None, adjust=None, self_=None, by_axis=True, err=False):
        self.name, self.array, self.count, self.c_pack, self.c_unpack = name, array, count, c_pack, c_unpack
        self.kind, self.adjust, self.self_, self.by_axis, self.err = kind, adjust, self_, by_axis, err


def _msg_family(kind):
    return Family("msg%d" % kind, "f", functools.partial(_msg_count, kind), "orc_pack_msg", "orc_unpack_msg", kind=kind,
                  adjust=pyorc.local_adjust_tang_e_norm_b if kind == 2 else None,
                  self_=pyorc.synchronize_tang_e_norm_b_self if kind == 2 else None, err=kind == 2)


def _msg_count(kind, g, d):
    return pyorc.msg_count(g, kind, d)


FAMILIES = {f.name: f for f in (
    Family("tang_b", "f", pyorc.tang_b_count, "orc_pack_tang_b", "orc_unpack_tang_b", by_axis=False),
    Family("jf", "f", pyorc.tang_b_count, "orc_pack_jf", "orc_unpack_jf", adjust=pyorc.local_adjust_jf, self_=pyorc.synchronize_jf_self),
    Family("rho", "f", pyorc.rho_count, "orc_pack_rho", "orc_unpack_rho", adjust=pyorc.local_adjust_rho, self_=pyorc.synchronize_rho_self),
    _msg_family(0), _msg_family(1), _msg_family(2),
    Family("hydro", "h", pyorc.hydro_count, "orc_pack_hydro", "orc_unpack_hydro", adjust=pyorc.local_adjust_hydro,
           self_=pyorc.synchronize_hydro_self),
)}


def closed_count(name, n, d):
    """floats of a message of family `name` in direction d on a brick of n = (nx, ny, nz) cells: include/vpic_hip.h and
    remote.c:69, :546, :150, :223, :318, hydro.c:40 without the leading cell-size float"""
    a = d % 3
    nY, nZ = n[(a + 1) % 3], n[(a + 2) % 3]
    return {"tang_b": nY * (nZ + 1) + nZ * (nY + 1), "jf": nY * (nZ + 1) + nZ * (nY + 1), "rho": 2 * (nY + 1) * (nZ + 1),
            "msg0": (nY + 1) * (nZ + 1), "msg1": nY * nZ, "msg2": nY * nZ + 2 * nY * (nZ + 1) + 2 * nZ * (nY + 1),
            "hydro": 14 * (nY + 1) * (nZ + 1)}[name]


def squared_terms(n, d):
    """how many squared differences a kind-2 message in direction d adds to err: one per cB and per E word"""
    a = d % 3
    nY, nZ = n[(a + 1) % 3], n[(a + 2) % 3]
    return nY * nZ + nY * (nZ + 1) + nZ * (nY + 1)


def err_mask(n, d):
    """which floats of a kind-2 message enter err: the cB block, then the first of every (e, tca) pair"""
    a = d % 3
    nY, nZ = n[(a + 1) % 3], n[(a + 2) % 3]
    m = np.zeros(closed_count("msg2", n, d), bool)
    m[:nY * nZ] = True
    m[nY * nZ::2] = True
    assert int(m.sum()) == squared_terms(n, d)
    return m


# ---- meshes -------------------------------------------------------------------------------------------------------------------
# component -> (mesh, own axis); extents per axis as inclusive (lo, hi)
MESH = {}
for _a, _x in enumerate("xyz"):
    for _c in ("e", "tca", "jf"):
        MESH[_c + _x] = ("edge", _a)
    MESH["cb" + _x] = ("face", _a)
for _c in ("rhof", "rhob", "div_e_err"):
    MESH[_c] = ("node", None)
MESH["div_b_err"] = ("cell", None)
for _c in HYDRO_FLOATS:
    MESH[_c] = ("node", None)


def extent(n, mesh, ca):
    """inclusive (lo, hi) per axis of the words a brick of n cells owns of a component (field_advance.h:60-70)"""
    out = []
    for d in range(3):
        if mesh == "node":
            hi = n[d] + 1
        elif mesh == "cell":
            hi = n[d]
        elif mesh == "edge":
            hi = n[d] if d == ca else n[d] + 1
        else:
            hi = n[d] + 1 if d == ca else n[d]
        out.append((1, hi))
    return out


def view3(a, name, n):
    """component `name` of a field_t / hydro_t array as [z, y, x] (a view)"""
    return a[name].reshape(n[2] + 2, n[1] + 2, n[0] + 2)


def slab(ext, shift=(0, 0, 0)):
    """index of view3 for inclusive extents, moved by `shift` cells"""
    return tuple(slice(ext[d][0] + shift[d], ext[d][1] + 1 + shift[d]) for d in (2, 1, 0))


def plane(ext, axis, p):
    e = list(ext)
    e[axis] = (p, p)
    return e


# ---- the world ----------------------------------------------------------------------------------------------------------------
class Domain:
    pass


class World:
    """gp = (gpx, gpy, gpz) bricks of n = (nx, ny, nz) cells; walls: {axis: wall name} for axes whose two outer faces are
    walls of that kind (the others are periodic); inputs "general" or "exact" from `seed`."""

    def __init__(self, gp, n, walls=None, inputs="general", seed=1):
        self.gp, self.n, self.walls, self.inputs = tuple(gp), tuple(n), dict(walls or {}), inputs
        self.domains, self.msgs = [], {}
        nranks = gp[0] * gp[1] * gp[2]
        for rank in range(nranks):
            d = Domain()
            d.rank = rank
            d.c = (rank % gp[0], (rank // gp[0]) % gp[1], rank // (gp[0] * gp[1]))
            d.fbc = [self._neighbour(d.c, f) for f in range(6)]
            pbc = [b if b >= 0 else L.REFLECT_PARTICLES for b in d.fbc]
            d.args = (n[0], n[1], n[2], n[0] * CELL[0], n[1] * CELL[1], n[2] * CELL[2], DT)
            d.kw = dict(fbc=d.fbc, pbc=pbc, rank=rank)
            d.g = pyorc.make_grid(*d.args, **d.kw)
            self.domains.append(d)
        self.nv = self.domains[0].g.nv
        fw, hw, ids = generate(inputs, seed, nranks, self.nv)
        for d in self.domains:
            d.f0, d.h0 = np.zeros(self.nv, L.field_t), np.zeros(self.nv, L.hydro_t)
            for k, name in enumerate(FIELD_FLOATS):
                d.f0[name] = fw[d.rank, :, k]
            for k, name in enumerate(FIELD_IDS):
                d.f0[name] = ids[d.rank, :, k]
            d.h0.view(np.float32).reshape(self.nv, 16)[...] = hw[d.rank]
        self.reset()

    def _neighbour(self, c, f):
        a, hi = f % 3, f >= 3
        if (c[a] == self.gp[a] - 1) if hi else (c[a] == 0):
            if a in self.walls:
                return WALLS[self.walls[a]]
        cc = list(c)
        cc[a] = (c[a] + (1 if hi else -1)) % self.gp[a]
        return cc[0] + self.gp[0] * (cc[1] + self.gp[1] * cc[2])

    def reset(self):
        """every array back to its input, the messages forgotten"""
        for d in self.domains:
            d.f, d.h = d.f0.copy(), d.h0.copy()
        self.msgs = {}

    def shared(self, rank, d):
        """direction d of `rank` goes to ANOTHER domain"""
        b = self.domains[rank].fbc[d]
        return b >= 0 and b != rank

    def array(self, fam, rank):
        d = self.domains[rank]
        return d.f if FAMILIES[fam].array == "f" else d.h

    def one_domain_grid(self):
        """(args, kw) of the one domain the world stands for"""
        N = [self.gp[a] * self.n[a] for a in range(3)]
        fbc = [WALLS[self.walls[f % 3]] if f % 3 in self.walls else 0 for f in range(6)]
        pbc = [b if b >= 0 else L.REFLECT_PARTICLES for b in fbc]
        return (N[0], N[1], N[2], N[0] * CELL[0], N[1] * CELL[1], N[2] * CELL[2], DT), dict(fbc=fbc, pbc=pbc, rank=0)

    # -- the call order --
    def schedule(self, fam):
        F, ranks, out = FAMILIES[fam], range(len(self.domains)), []
        if F.adjust:
            out += [Piece("adjust", r, None, None) for r in ranks]
        for dirs in ([(a, a + 3) for a in range(3)] if F.by_axis else [tuple(range(6))]):
            if F.self_:
                out += [Piece("self", r, dirs[0], None) for r in ranks]
            sends = [(r, d) for r in ranks for d in dirs if self.shared(r, d)]
            out += [Piece("pack", r, d, None) for r, d in sends]
            # every domain unpacks what arrived, in the order of the directions
            out += sorted((Piece("unpack", self.domains[r].fbc[d], d, r) for r, d in sends), key=lambda p: (p.rank, p.arg))
        return out

    def apply(self, fam, piece):
        """one piece on the reference arrays; returns the err of the piece (0.0 where the piece has none)"""
        F, d = FAMILIES[fam], self.domains[piece.rank]
        a = self.array(fam, piece.rank)
        if piece.op == "adjust":
            F.adjust(a, d.g)
        elif piece.op == "self":
            return float(F.self_(a, d.g, piece.arg) or 0.0)
        elif piece.op == "pack":
            self.msgs[(piece.rank, piece.arg)] = pack(F, a, d.g, piece.arg)
        else:
            return unpack(F, a, self.msgs[(piece.src, piece.arg)], d.g, piece.arg)
        return 0.0

    def run(self, fam):
        """the whole schedule; returns err per rank"""
        err = [0.0] * len(self.domains)
        for p in self.schedule(fam):
            err[p.rank] += self.apply(fam, p)
        return err


def pack(F, a, g, d):
    """the oracle's pack into a buffer filled with the NaN pattern, with a guard behind it: returns exactly count floats,
    every one written, nothing behind them touched"""
    n = F.count(g, d)
    buf = np.full(n + GUARD_WORDS, GUARD_WORD, np.uint32)
    fn = getattr(pyorc.lib(), F.c_pack)
    args = (buf.ctypes.data_as(C.c_void_p), a.ctypes.data_as(C.c_void_p), C.byref(g)) + ((F.kind,) if F.kind is not None else ()) + (d,)
    k = fn(*args)
    assert k == n, (F.name, d, "packed", k, "count", n)
    assert not np.any(buf[:n] == GUARD_WORD), (F.name, d, "floats of the message left unwritten")
    assert np.all(buf[n:] == GUARD_WORD), (F.name, d, "written behind count")
    return buf[:n].view(np.float32).copy()


def unpack(F, a, msg, g, d):
    msg = np.ascontiguousarray(msg, np.float32)
    assert len(msg) == F.count(g, d)
    fn = getattr(pyorc.lib(), F.c_unpack)               # (orc_unpack_msg's double restype is set by pyorc.lib())
    args = (a.ctypes.data_as(C.c_void_p), msg.ctypes.data_as(C.c_void_p), C.byref(g)) + ((F.kind,) if F.kind is not None else ()) + (d,)
    r = fn(*args)
    return float(r) if F.err else 0.0


def exact_err(msg, before, n, d):
    """the err of unpacking the kind-2 message `msg` onto a plane that read `before` (the same plane packed as a kind-2
    message), summed in integers: for exact inputs only.  Asserts that the sum has room in a double."""
    m = err_mask(n, d)
    diff = (msg.astype(np.float64) - before.astype(np.float64))[m] * 2.0 ** 9
    k = np.rint(diff).astype(np.int64)
    assert np.all(k == diff), "not multiples of 2^-9"
    s = sum(int(v) * int(v) for v in k)
    assert s < 1 << 53
    return s / 2.0 ** 18


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def generate(inputs, seed, nranks, nv):
    """(field floats [nranks, nv, 16], hydro floats [nranks, nv, 16], material ids uint16 [nranks, nv, 8]); all float words
    of the two float arrays together pairwise different"""
    rng = np.random.default_rng(seed)
    half = nranks * nv * 16
    total = 2 * half
    if inputs == "exact":
        k = np.concatenate([rng.permutation(np.arange(1, half + 1, dtype=np.int64)) for _ in range(2)])   # fields, then hydro
        k[rng.random(total) < 0.5] *= -1
        v = (k * 2.0 ** -6).astype(np.float32)
        assert np.all(v.astype(np.float64) * 64 == k)
    else:
        assert inputs == "general"
        v = np.zeros(total, np.float32)
        bad = np.ones(total, bool)
        while bad.any():
            m = int(bad.sum())
            v[bad] = (rng.standard_normal(m) * 10.0 ** rng.uniform(-5, 2, m)).astype(np.float32)
            mag = np.abs(v)
            bad = ~np.isfinite(v) | (mag < 1e-6) | (mag > 1e3)
            _, first = np.unique(v.view(np.uint32), return_index=True)
            dup = np.ones(total, bool)
            dup[first] = False
            bad |= dup
    v = v.reshape(2, nranks, nv, 16)
    assert_distinct(v[0].view(np.uint32), inputs + " fields")
    assert_distinct(v[1].view(np.uint32), inputs + " hydro")
    ids = rng.integers(1, 8, (nranks, nv, 8)).astype(np.uint16)
    return v[0], v[1], ids


# ---- gather -------------------------------------------------------------------------------------------------------------------
GATHER = {"jf": ("f", {"jfx": "sum", "jfy": "sum", "jfz": "sum"}),
          "rho": ("f", {"rhof": "sum", "rhob": "mean"}),
          "msg2": ("f", {c + x: "mean" for c in ("cb", "e", "tca") for x in "xyz"}),
          "hydro": ("h", {c: "sum" for c in HYDRO_FLOATS})}


def gather(w, fam, arrays=None):
    """the one-domain array (field_t or hydro_t, zero outside the family's components) that the bricks' `arrays` (default:
    the world's current ones) stand for"""
    which, comps = GATHER[fam]
    (NX, NY, NZ, *_), _ = w.one_domain_grid()
    N = (NX, NY, NZ)
    out = np.zeros(L.nv(*N), L.field_t if which == "f" else L.hydro_t)
    for name, how in comps.items():
        ext = extent(w.n, *MESH[name])
        acc = np.zeros((NZ + 2, NY + 2, NX + 2), np.float64)
        cnt = np.zeros(acc.shape, np.int64)
        for d in w.domains:
            a = arrays[d.rank] if arrays is not None else w.array(fam, d.rank)
            shift = tuple(d.c[k] * w.n[k] for k in range(3))
            acc[slab(ext, shift)] += view3(a, name, w.n)[slab(ext)]
            cnt[slab(ext, shift)] += 1
        assert set(np.unique(cnt)) <= {0, 1, 2, 4, 8}
        if how == "mean":
            acc = acc / np.maximum(cnt, 1)
        res = acc.astype(np.float32)
        assert np.all(res.astype(np.float64) == acc), "the gather is exact on exact inputs only"
        view3(out, name, N)[...] = res
    return out


def owned_equal(w, fam, one, arrays=None):
    """number of owned words of the bricks (over each component's mesh extent) that differ from the one-domain array `one`"""
    which, comps = GATHER[fam]
    (NX, NY, NZ, *_), _ = w.one_domain_grid()
    bad = 0
    for name in comps:
        ext = extent(w.n, *MESH[name])
        for d in w.domains:
            a = arrays[d.rank] if arrays is not None else w.array(fam, d.rank)
            shift = tuple(d.c[k] * w.n[k] for k in range(3))
            got = view3(a, name, w.n)[slab(ext)].view(np.uint32)
            ref = view3(one, name, (NX, NY, NZ))[slab(ext, shift)].view(np.uint32)
            bad += int(np.count_nonzero(got != ref))
    return bad


# ---- ghost planes of the copied kinds ------------------------------------------------------------------------------------------
def copied_planes(fam, n, d):
    """[(component, extents of the sender's plane, extents of the receiver's ghost plane)] of a tang_b / msg0 / msg1 message
    travelling in direction d between bricks of n cells"""
    a = d % 3
    src, dst = (1, n[a] + 1) if d < 3 else (n[a], 0)
    if fam == "tang_b":
        comps = [("cb" + "xyz"[(a + t) % 3], extent(n, "face", (a + t) % 3)) for t in (1, 2)]
    elif fam == "msg0":
        comps = [("e" + "xyz"[a], extent(n, "node", None))]
    else:
        assert fam == "msg1"
        comps = [("div_b_err", extent(n, "cell", None))]
    return [(c, plane(e, a, src), plane(e, a, dst)) for c, e in comps]


# ---- the worlds and sizes of the tests -------------------------------------------------------------------------------------------
def case_id(gp, n, walls):
    return "%dx%dx%d-%dx%dx%d" % (tuple(gp) + tuple(n)) + "".join("-%s%s" % (v, "xyz"[k]) for k, v in sorted((walls or {}).items()))


def _cases():
    """(gp, n, walls): every world of the issue with the brick sizes that make every piece meet a one-cell axis as the
    message axis and as each tangential axis, and one brick of the large family per world family"""
    small, thin, one = (5, 3, 2), [(1, 4, 3), (3, 1, 2), (2, 3, 1)], (1, 1, 1)
    big = {0: (2, 17, 16), 1: (16, 2, 17), 2: (17, 16, 2)}        # by cut axis: a large plane normal to it
    out = []
    for a in range(3):                                            # two slabs
        gp = tuple(2 if k == a else 1 for k in range(3))
        out += [(gp, n, None) for n in [small] + thin + [one, big[a]]]
    for gp, b in (((2, 2, 1), (17, 16, 2)), ((1, 2, 2), (2, 17, 16)), ((2, 1, 2), (16, 2, 17))):   # edge rows through two passes
        out += [(gp, n, None) for n in [small] + thin + [one, b]]
    out += [((2, 2, 2), n, None) for n in [small] + thin + [one, (17, 16, 2)]]                      # corners through three
    for a in range(3):                                            # walls on the cut axis, every kind
        gp = tuple(2 if k == a else 1 for k in range(3))
        for j, wall in enumerate(WALLS):
            sizes = [small, thin[a], thin[(a + 1 + j % 2) % 3]] + ([one] if j == 0 else []) + ([big[a]] if j == 1 else [])
            out += [(gp, n, {a: wall}) for n in sizes]
    return out


CASES = _cases()
CASE_IDS = [case_id(*c) for c in CASES]
FAMILY_WORLDS = [((2, 1, 1), (5, 3, 2), None), ((1, 2, 1), (3, 1, 2), None), ((1, 1, 2), (2, 3, 1), None), ((2, 2, 1), (1, 4, 3), None),
                 ((1, 2, 2), (5, 3, 2), None), ((2, 1, 2), (1, 1, 1), None), ((2, 2, 2), (5, 3, 2), None), ((2, 2, 2), (1, 1, 1), None),
                 ((2, 1, 1), (17, 16, 2), {0: "pec"}), ((1, 2, 1), (5, 3, 2), {1: "symmetric"}), ((1, 1, 2), (2, 3, 1), {2: "pmc"}),
                 ((2, 1, 1), (1, 4, 3), {0: "absorb"})]          # one (and a thin one) per family for the device-against-device check
