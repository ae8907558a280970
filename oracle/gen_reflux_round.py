"""TEST INFRASTRUCTURE: golden vectors of the DISPATCH around the custom particle boundary handler -- the reference's own
boundary_p (src/species_advance/standard/boundary_p.c:78-505) from the COMPILED REFERENCE (oracle/_ref/libvpic_ref.so) on
one 6 x 5 x 4 domain whose faces carry handler codes: maxwellian_reflux registered twice through add_boundary (codes -3 and
-4, different temperatures), a third code (-5) registered nowhere, and in a second world absorbing, reflecting and
self-periodic faces beside them.  Movers sit on all six faces, and hand-placed ones on two and three faces at once, so that
the face order and the fall-through of :240-316 decide what becomes of them.  The numbers the handler drew are learned
from a twin generator seeded alike, read in the reference's order: movers last to first, three per handler call
(mt_frand, mt_frandn, mt_frandn); they are stored as a table indexed by the particle's slot in its array (the rule of
orc_boundary_p_reflux_round and of the engine's vpic_hip_set_reflux_draws).
-> tests/golden/reflux_round.npz.  Needs the compiled reference (python oracle/gen_reflux_round.py)."""
import ctypes as C
import importlib
import itertools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import pyref as R  # noqa: E402

L = importlib.import_module("old-vpic_amd.layout")
NX, NY, NZ = 6, 5, 4
LX, LY, LZ, DT = 6.0, 7.5, 3.0, 0.3            # unequal cell sizes: dx = 1, dy = 1.5, dz = 0.75
HANDLERS = [(-3, 0.11, 0.04), (-4, 0.3, 0.2)]  # (code, ut_para, ut_perp); -5 is registered nowhere
SELF = 0                                       # this same domain (the periodic neighbour stays in place)
WORLDS = {
    "handlers": [-3, -4, -5, -4, -3, -5],
    "mixed": [-3, L.ABSORB_PARTICLES, L.REFLECT_PARTICLES, -5, -4, SELF],
}
N_REST, N_FACE, N_PAIR, N_CORNER = 150, 20, 4, 2
Q0 = -0.01


class Params(C.Structure):                    # boundary.h: maxwellian_reflux_t
    _fields_ = [("ut_perp", C.c_float * 32), ("ut_para", C.c_float * 32)]


def parked(rng, faces):
    """one particle on all of `faces` at once (different axes), leaving through each: (dx dy dz, cell x y z, ux uy uz)"""
    d = rng.uniform(-0.9, 0.9, 3)
    c = [rng.integers(1, n + 1) for n in (NX, NY, NZ)]
    u = 0.8 * rng.standard_normal(3)
    for f in faces:
        axis, hi = f % 3, f >= 3
        d[axis] = 1.0 if hi else -1.0
        u[axis] = abs(u[axis]) + 0.05 if hi else -abs(u[axis]) - 0.05
        c[axis] = (NX, NY, NZ)[axis] if hi else 1
    return d, c, u


def world(l, name, pbc, seed):
    rng = np.random.default_rng(seed)
    g = R.new_periodic_grid(NX, NY, NZ, LX, LY, LZ, np.float32(DT))
    l.IUO_add_boundary.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    for code, para, perp in HANDLERS:
        par = Params()
        par.ut_para[0], par.ut_perp[0] = para, perp                       # (the species below has id 0)
        assert l.IUO_add_boundary(g, C.cast(l.maxwellian_reflux, C.c_void_p), C.byref(par), C.sizeof(par)) == code
    # set_pbc refuses a code that names no handler (grid/ops.c:208-209), so a third handler is registered while the faces
    # are set and the grid's handler count is put back to two afterwards: boundary_p then meets code -5 with nb == 2,
    # the case its `(nn>=0) & (nn<nb)` test (:272) is there for
    par = Params()
    assert l.IUO_add_boundary(g, C.cast(l.maxwellian_reflux, C.c_void_p), C.byref(par), C.sizeof(par)) == -5
    for face, code in enumerate(pbc):
        if code != SELF:
            R.set_face_bc(g, face, L.PEC_FIELDS, code)
    layout = (C.c_int * 32)()
    l.ref_layout(layout)
    nb = C.c_int.from_address(g + layout[19])                            # offsetof(grid_t, nb), oracle/ref_shim.c
    assert nb.value == 3
    nb.value = len(HANDLERS)
    # the movers' particles: one face, two faces (every pairing of faces on different axes), three (corners)
    sets = [(f,) for f in range(6) for _ in range(N_FACE)]
    sets += [fs for fs in itertools.combinations(range(6), 2) if fs[0] % 3 != fs[1] % 3 for _ in range(N_PAIR)]
    sets += [fs for fs in itertools.combinations(range(6), 3) if len({f % 3 for f in fs}) == 3 for _ in range(N_CORNER)]
    n_mv = len(sets)
    n = N_REST + n_mv
    p = np.zeros(n, L.particle_t)
    for c in ("dx", "dy", "dz"):
        p[c] = rng.uniform(-1, 1, n).astype(np.float32)
    for c in ("ux", "uy", "uz"):
        p[c] = (0.8 * rng.standard_normal(n)).astype(np.float32)
    p["i"] = L.voxel(rng.integers(1, NX + 1, n), rng.integers(1, NY + 1, n), rng.integers(1, NZ + 1, n), NX, NY, NZ)
    p["q"] = (np.float32(Q0) * (1 + np.arange(n) * 2.0 ** -14)).astype(np.float32)   # a different charge each: identifies the particle
    p["tag"] = np.arange(n) + 1
    slots = np.sort(rng.choice(n, n_mv, replace=False))               # the movers' list ascends, as advance_p leaves it
    faces = np.full((n_mv, 3), -1, np.int32)
    for k, fs in enumerate([sets[j] for j in rng.permutation(n_mv)]):
        d, c, u = parked(rng, fs)
        s = slots[k]
        p["dx"][s], p["dy"][s], p["dz"][s] = d
        p["ux"][s], p["uy"][s], p["uz"][s] = u
        p["i"][s] = L.voxel(c[0], c[1], c[2], NX, NY, NZ)
        faces[k, :len(fs)] = fs
    pm = np.zeros(n_mv, L.particle_mover_t)
    for c in ("dispx", "dispy", "dispz"):
        pm[c] = (0.3 * rng.uniform(-1, 1, n_mv)).astype(np.float32)
    pm["i"] = slots
    assert len(np.unique(p["q"])) == n

    l.new_mt_rng.restype = C.c_void_p
    l.mt_frand.restype = C.c_float
    l.mt_frandn.restype = C.c_float
    rng_a, rng_b = l.new_mt_rng(77 + seed), l.new_mt_rng(77 + seed)
    sp = l.ref_new_species(C.c_float(-1.0), 2 * n, 2 * n, 1)             # id 0
    pt, mt = L.particle_t, L.particle_mover_t
    C.memmove((C.c_char * (pt.itemsize * n)).from_address(l.ref_species_p(R.V(sp))), p.ctypes.data, pt.itemsize * n)
    C.memmove((C.c_char * (mt.itemsize * n_mv)).from_address(l.ref_species_pm(R.V(sp))), pm.ctypes.data, mt.itemsize * n_mv)
    l.ref_species_set_counts(R.V(sp), n, n_mv)
    nv = L.nv(NX, NY, NZ)
    f, a = np.zeros(nv, L.field_t), np.zeros(nv, L.accumulator_t)
    l.boundary_p(R.V(sp), R._p(f), R._p(a), R.V(g), R.V(rng_a))
    np_out, nm_out = l.ref_species_np(R.V(sp)), l.ref_species_nm(R.V(sp))
    out_p = np.frombuffer((C.c_char * (pt.itemsize * np_out)).from_address(l.ref_species_p(R.V(sp))), dtype=pt).copy()
    out_pm = np.frombuffer((C.c_char * (mt.itemsize * max(nm_out, 1))).from_address(l.ref_species_pm(R.V(sp))), dtype=mt).copy()[:nm_out]
    # the handler's calls: the injected particles are the tail of the array, appended from the LAST injector made to the
    # first (:477-496); the injectors were made walking the movers last to first.  So call k made tail[::-1][k].
    n_inj = np_out - (n - n_mv)
    tail = out_p[np_out - n_inj:]
    out_p["tag"][np_out - n_inj:] = 0                                  # (an injector record has no tag fields: untouched memory)
    out_p["tag2"][np_out - n_inj:] = 0
    draws = np.zeros((n, 3), np.float32)
    slot_of_q = {float(q): s for s, q in enumerate(p["q"])}
    for k in range(n_inj):
        s = slot_of_q[float(tail[::-1][k]["q"])]
        assert s in slots and not draws[s].any()
        draws[s] = [l.mt_frand(R.V(rng_b)), l.mt_frandn(R.V(rng_b)), l.mt_frandn(R.V(rng_b))]
    print("%s: %d particles, %d movers -> %d refluxed, %d absorbed, %d movers left; |rhob| sum %.4g"
          % (name, n, n_mv, n_inj, n_mv - n_inj, nm_out, float(np.abs(f["rhob"]).sum())))
    return {name + "_" + k: v for k, v in dict(pbc=np.array(pbc, np.int32), p=p, pm=pm, faces=faces, draws=draws, out_p=out_p,
                                               out_pm=out_pm, n_inj=np.array(n_inj), rhob=f["rhob"].copy(), a=a).items()}


def main():
    l = R.lib()
    out = dict(dims=np.array([NX, NY, NZ]), box=np.array([LX, LY, LZ, DT]), handlers=np.array(HANDLERS, np.float64),
               worlds=np.array(sorted(WORLDS)))
    for k, name in enumerate(sorted(WORLDS)):
        out.update(world(l, name, WORLDS[name], 5 + k))
    dst = os.path.join(ROOT, "tests", "golden", "reflux_round.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main()
