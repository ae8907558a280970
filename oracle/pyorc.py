"""ctypes binding of oracle/libvpic_oracle.so (TEST INFRASTRUCTURE, see vpic_oracle.h)."""
import contextlib
import ctypes as C
import importlib
import math
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
L = importlib.import_module("old-vpic_amd.layout")


class Grid(C.Structure):
    """orc_grid_t"""
    _fields_ = [("dt", C.c_float), ("cvac", C.c_float), ("eps0", C.c_float), ("damp", C.c_float),
                ("dx", C.c_float), ("dy", C.c_float), ("dz", C.c_float),
                ("rdx", C.c_float), ("rdy", C.c_float), ("rdz", C.c_float),
                ("nx", C.c_int), ("ny", C.c_int), ("nz", C.c_int),
                ("fbc", C.c_int * 6), ("pbc", C.c_int * 6), ("rank", C.c_int)]

    @property
    def nv(self):
        return (self.nx + 2) * (self.ny + 2) * (self.nz + 2)


def make_grid(nx, ny, nz, lx, ly, lz, dt, cvac=1.0, eps0=1.0, damp=0.0, fbc=None, pbc=None, rank=0):
    """Cell sizes the way partition_periodic_box computes them (src/grid/partition.c:60-66):
    double arithmetic, then stored as float."""
    g = Grid()
    g.dt, g.cvac, g.eps0, g.damp = dt, cvac, eps0, damp
    g.dx, g.dy, g.dz = lx / nx, ly / ny, lz / nz
    g.rdx, g.rdy, g.rdz = nx / lx, ny / ly, nz / lz
    g.nx, g.ny, g.nz = nx, ny, nz
    g.rank = rank
    for f in range(6):
        g.fbc[f] = rank if fbc is None else fbc[f]
        g.pbc[f] = rank if pbc is None else pbc[f]
    return g


_lib = None


def lib():
    global _lib
    if _lib is None:
        so = os.path.join(HERE, "libvpic_oracle.so")
        src = os.path.join(HERE, "vpic_oracle.c")
        if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
            subprocess.check_call(["make", "-s", "-C", HERE, "oracle"])
        _lib = C.CDLL(so)
        _lib.orc_energy_p.restype = C.c_double
        _lib.orc_synchronize_tang_e_norm_b_local.restype = C.c_double
        _lib.orc_synchronize_tang_e_norm_b_self.restype = C.c_double
        _lib.orc_unpack_msg.restype = C.c_double
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def load_interpolator(fi, f, g):
    lib().orc_load_interpolator(_p(fi), _p(f), C.byref(g))


def clear_accumulators(a, g, n_pipeline=0):
    lib().orc_clear_accumulators(_p(a), C.byref(g), n_pipeline)


def reduce_accumulators(a, g, n_pipeline):
    lib().orc_reduce_accumulators(_p(a), C.byref(g), n_pipeline)


def unload_accumulator(f, a, g):
    lib().orc_unload_accumulator(_p(f), _p(a), C.byref(g))


def advance_p(p, np_, q_m, pm, a, fi, g, n_pipeline=0):
    return lib().orc_advance_p(_p(p), int(np_), C.c_float(q_m), _p(pm), len(pm), _p(a), _p(fi), C.byref(g), n_pipeline)


def center_p(p, np_, q_m, fi, g):
    lib().orc_center_p(_p(p), int(np_), C.c_float(q_m), _p(fi), C.byref(g))


def uncenter_p(p, np_, q_m, fi, g):
    lib().orc_uncenter_p(_p(p), int(np_), C.c_float(q_m), _p(fi), C.byref(g))


def sort_p(p, np_, partition, g, out_of_place=1):
    lib().orc_sort_p(_p(p), int(np_), _p(partition), C.byref(g), out_of_place)


def energy_p(p, np_, q_m, fi, g):
    return lib().orc_energy_p(_p(p), int(np_), C.c_float(q_m), _p(fi), C.byref(g))


def energy_f(f, m, g):
    en = np.zeros(6, np.float64)
    lib().orc_energy_f(_p(en), _p(f), _p(m), C.byref(g))
    return en


def vacuum_coefficients():
    m = np.zeros(1, L.material_coefficient_t)
    lib().orc_vacuum_coefficients(_p(m))
    return m


def material_coefficients(props, dt, eps0=1.0):
    """props: [n, 9] floats (eps xyz, mu xyz, sigma xyz) -> n coefficient records (sfa.c:145-177)."""
    props = np.ascontiguousarray(props, np.float32)
    m = np.zeros(len(props), L.material_coefficient_t)
    for k in range(len(props)):
        lib().orc_material_coefficients(C.c_void_p(m.ctypes.data + k * m.itemsize), props[k].ctypes.data_as(C.c_void_p),
                                        C.c_float(dt), C.c_float(eps0))
    return m


def clear_jf(f, g):
    lib().orc_clear_jf(_p(f), C.byref(g))


def advance_b(f, g, frac):
    lib().orc_advance_b(_p(f), C.byref(g), C.c_float(frac))


def advance_e(f, m, g):
    lib().orc_advance_e(_p(f), _p(m), C.byref(g))


def clear_rhof(f, g):
    lib().orc_clear_rhof(_p(f), C.byref(g))


def accumulate_rho_p(f, p, np_, g):
    lib().orc_accumulate_rho_p(_p(f), _p(p), int(np_), C.byref(g))


def synchronize_rho_local(f, g):
    lib().orc_synchronize_rho_local(_p(f), C.byref(g))


def accumulate_rhob(f, p, g):
    """boundary_p.c:9-71 for every particle of p."""
    for k in range(len(p)):
        lib().orc_accumulate_rhob(_p(f), C.c_void_p(p.ctypes.data + k * p.itemsize), C.byref(g))


def compute_rhob(f, m, g):
    lib().orc_compute_rhob(_p(f), _p(m), C.byref(g))


def compute_curl_b(f, m, g):
    lib().orc_compute_curl_b(_p(f), _p(m), C.byref(g))


def synchronize_tang_e_norm_b_local(f, g):
    return lib().orc_synchronize_tang_e_norm_b_local(_p(f), C.byref(g))


def compute_div_e_err(f, m, g):
    lib().orc_compute_div_e_err(_p(f), _p(m), C.byref(g))


def _rms(fn, f, g):
    s = np.zeros(2, np.float64)
    fn(_p(s), _p(f), C.byref(g))
    return float(g.eps0 * np.sqrt(s[0] / s[1]))          # compute_rms_div_e_err.c:156-159 on one domain


def compute_rms_div_e_err(f, g):
    return _rms(lib().orc_rms_div_e_err_local, f, g)


def clean_div_e(f, m, g):
    lib().orc_clean_div_e(_p(f), _p(m), C.byref(g))


def compute_div_b_err(f, g):
    lib().orc_compute_div_b_err(_p(f), C.byref(g))


def compute_rms_div_b_err(f, g):
    return _rms(lib().orc_rms_div_b_err_local, f, g)


def clean_div_b(f, g):
    lib().orc_clean_div_b(_p(f), C.byref(g))


def clear_hydro(h, g):
    lib().orc_clear_hydro(_p(h), C.byref(g))


def accumulate_hydro_p(h, p, np_, q_m, fi, g):
    lib().orc_accumulate_hydro_p(_p(h), _p(p), int(np_), C.c_float(q_m), _p(fi), C.byref(g))


def synchronize_hydro_local(h, g):
    lib().orc_synchronize_hydro_local(_p(h), C.byref(g))


def local_adjust_hydro(h, g):
    lib().orc_local_adjust_hydro(_p(h), C.byref(g))


def hydro_count(g, d):
    return lib().orc_hydro_count(C.byref(g), d)


def pack_hydro(h, g, d):
    buf = np.zeros(hydro_count(g, d), np.float32)
    lib().orc_pack_hydro(_p(buf), _p(h), C.byref(g), d)
    return buf


def unpack_hydro(h, buf, g, d):
    lib().orc_unpack_hydro(_p(h), _p(np.ascontiguousarray(buf, np.float32)), C.byref(g), d)


def synchronize_hydro_self(h, g, axis):
    """One axis of synchronize_hydro for faces the domain shares with itself (hydro.c:28-163): both planes are packed
    before either is added to."""
    if g.fbc[axis] != g.rank or g.fbc[axis + 3] != g.rank:
        return
    lo, hi = pack_hydro(h, g, axis), pack_hydro(h, g, axis + 3)
    unpack_hydro(h, lo, g, axis)
    unpack_hydro(h, hi, g, axis + 3)


def local_adjust_rho(f, g):
    lib().orc_local_adjust_rho(_p(f), C.byref(g))


def synchronize_rho_self(f, g, axis):
    lib().orc_synchronize_rho_self(_p(f), C.byref(g), axis)


def rho_count(g, d):
    return lib().orc_rho_count(C.byref(g), d)


def pack_rho(f, g, d):
    buf = np.zeros(rho_count(g, d), np.float32)
    lib().orc_pack_rho(_p(buf), _p(f), C.byref(g), d)
    return buf


def unpack_rho(f, buf, g, d):
    lib().orc_unpack_rho(_p(f), _p(np.ascontiguousarray(buf, np.float32)), C.byref(g), d)


def msg_count(g, kind, d):
    return lib().orc_msg_count(C.byref(g), kind, d)


def pack_msg(f, g, kind, d):
    buf = np.zeros(msg_count(g, kind, d), np.float32)
    lib().orc_pack_msg(_p(buf), _p(f), C.byref(g), kind, d)
    return buf


def unpack_msg(f, buf, g, kind, d):
    return lib().orc_unpack_msg(_p(f), _p(np.ascontiguousarray(buf, np.float32)), C.byref(g), kind, d)


def local_adjust_tang_e_norm_b(f, g):
    lib().orc_local_adjust_tang_e_norm_b(_p(f), C.byref(g))


def synchronize_tang_e_norm_b_self(f, g, axis):
    return lib().orc_synchronize_tang_e_norm_b_self(_p(f), C.byref(g), axis)


def rms_local(f, g, which):
    s = np.zeros(2, np.float64)
    (lib().orc_rms_div_e_err_local if which == "e" else lib().orc_rms_div_b_err_local)(_p(s), _p(f), C.byref(g))
    return float(s[0]), float(s[1])


def synchronize_jf_local(f, g):
    lib().orc_synchronize_jf_local(_p(f), C.byref(g))


def synchronize_jf_self(f, g, axis):
    """One axis of synchronize_jf for faces the domain shares with itself (remote.c:477-500)."""
    if g.fbc[axis] != g.rank or g.fbc[axis + 3] != g.rank:
        return
    lo, hi = pack_jf(f, g, axis), pack_jf(f, g, axis + 3)
    unpack_jf(f, lo, g, axis)
    unpack_jf(f, hi, g, axis + 3)


def tang_b_count(g, d):
    return lib().orc_tang_b_count(C.byref(g), d)


def pack_tang_b(f, g, d):
    buf = np.zeros(tang_b_count(g, d), np.float32)
    lib().orc_pack_tang_b(_p(buf), _p(f), C.byref(g), d)
    return buf


def unpack_tang_b(f, buf, g, d):
    lib().orc_unpack_tang_b(_p(f), _p(buf), C.byref(g), d)


def pack_jf(f, g, d):
    buf = np.zeros(tang_b_count(g, d), np.float32)
    lib().orc_pack_jf(_p(buf), _p(f), C.byref(g), d)
    return buf


def unpack_jf(f, buf, g, d):
    lib().orc_unpack_jf(_p(f), _p(buf), C.byref(g), d)


def local_adjust_jf(f, g):
    lib().orc_local_adjust_jf(_p(f), C.byref(g))


def move_p(p, pm1, a, g):
    """orc_move_p on particle pm1['i'] of p (in place); returns 1 when it stopped on a face."""
    return lib().orc_move_p(_p(p), _p(pm1), _p(a), C.byref(g))


def boundary_p_pack(p, np_, pm, nm, sp_id, f, g, cap):
    outs = [np.zeros(cap, L.particle_injector_t) for _ in range(6)]
    ptrs = (C.c_void_p * 6)(*[o.ctypes.data for o in outs])
    ns = (C.c_int * 6)()
    new_np = lib().orc_boundary_p_pack(_p(p), int(np_), _p(pm), int(nm), sp_id, _p(f), C.byref(g), ptrs, ns, cap)
    return new_np, [o[:ns[k]] for k, o in enumerate(outs)]


def maxwellian_reflux(draws, p, pm, g, ut_para, ut_perp, face, sp_id=0):
    """orc_maxwellian_reflux for mover record pm (one element) of particle array p; returns the injector record."""
    out = np.zeros(1, L.particle_injector_t)
    d = np.ascontiguousarray(draws, np.float32)
    part = p[int(pm["i"][0]):int(pm["i"][0]) + 1]
    lib().orc_maxwellian_reflux(_p(d), _p(part), _p(pm), C.byref(g), C.c_float(ut_para), C.c_float(ut_perp), int(face), int(sp_id), _p(out))
    return out[0]


def maxwellian_reflux_draw(draws, ut_para, ut_perp, face):
    """orc_maxwellian_reflux_draw: (u normal to the face, the two tangential ones) of one handler call, float32[3]"""
    u = np.zeros(3, np.float32)
    d = np.ascontiguousarray(draws, np.float32)
    lib().orc_maxwellian_reflux_draw(_p(d), C.c_float(ut_para), C.c_float(ut_perp), int(face), _p(u))
    return u


def maxwellian_reflux_from_u(u, p, pm, g, sp_id=0):
    """orc_maxwellian_reflux_from_u for mover record pm (one element) of particle array p with the new momentum
    u = (ux, uy, uz) in the grid's axes; returns the injector record."""
    out = np.zeros(1, L.particle_injector_t)
    part = p[int(pm["i"][0]):int(pm["i"][0]) + 1]
    lib().orc_maxwellian_reflux_from_u(C.c_float(u[0]), C.c_float(u[1]), C.c_float(u[2]), _p(part), _p(pm), C.byref(g), int(sp_id), _p(out))
    return out[0]


def boundary_p_reflux_round(p, pm, sp_id, f, a, g, handlers, draws, u_normal=None):
    """orc_boundary_p_reflux_round on copies: p the species' particles in array order, pm its movers, handlers a list of
    (code, ut_para, ut_perp) for THIS species, draws float32[n, 3] indexed by array slot, u_normal None or float32[len(pm)].
    rhob is added to f and the deposits to a (in place).  Returns (particles after the round: survivors, then the
    refluxed ones; new movers; injectors; the index in pm of the mover behind each injector; the face whose handler made it)."""
    nm = len(pm)
    out = np.zeros(len(p) + 1, L.particle_t)
    out[:len(p)] = p
    mv = np.zeros(max(nm, 1), L.particle_mover_t)
    mv[:nm] = pm
    codes = np.array([h[0] for h in handlers], np.int32)
    para = np.array([h[1] for h in handlers], np.float32)
    perp = np.array([h[2] for h in handlers], np.float32)
    d = np.ascontiguousarray(draws, np.float32).reshape(-1, 3)
    un = None if u_normal is None else np.ascontiguousarray(u_normal, np.float32)
    assert un is None or len(un) == nm
    inj, who, face = np.zeros(max(nm, 1), L.particle_injector_t), np.zeros(max(nm, 1), np.int32), np.zeros(max(nm, 1), np.int32)
    nm_c, ni_c = C.c_int(nm), C.c_int(0)
    new_np = lib().orc_boundary_p_reflux_round(_p(out), len(p), _p(mv), C.byref(nm_c), int(sp_id), _p(f), _p(a), C.byref(g),
                                               _p(codes), _p(para), _p(perp), len(codes), _p(d), len(d),
                                               None if un is None else _p(un), _p(inj), _p(who), _p(face), C.byref(ni_c))
    return out[:new_np], mv[:nm_c.value], inj[:ni_c.value], who[:ni_c.value], face[:ni_c.value]


def child_langmuir(p, np_, pm, nm, component, n_emit, ut_perp, ut_para, q_m, fi, f, a, g, draws):
    """orc_child_langmuir; returns (new np, new nm)."""
    nm_c = C.c_int(nm)
    comp = np.ascontiguousarray(component, np.int32)
    d = np.ascontiguousarray(draws, np.float64)
    new_np = lib().orc_child_langmuir(_p(p), int(np_), len(p), _p(pm), C.byref(nm_c), len(pm), _p(comp), len(comp), int(n_emit),
                                      C.c_float(ut_perp), C.c_float(ut_para), C.c_float(q_m), _p(fi), _p(f), _p(a), C.byref(g), _p(d))
    return new_np, nm_c.value


def boundary_p_inject(p, np_, pm, nm, inj, a, g):
    nm_c = C.c_int(nm)
    inj = np.ascontiguousarray(inj)
    new_np = lib().orc_boundary_p_inject(_p(p), int(np_), _p(pm), C.byref(nm_c), _p(inj), len(inj), _p(a), C.byref(g))
    return new_np, nm_c.value


# ---- the exact reference of the engine's deterministic accumulation (include/vpic_hip.h: vpic_hip_set_accumulation) ----
def fixed_scale(q_ref):
    """The engine's fixed-point scale for reference charge q_ref > 0 (for q_ref <= 0 the engine takes the largest |q| the
    host has put into any species so far): a power of two that puts a deposit of 4.2 q_ref near 2^37."""
    return 2.0 ** (37 - math.frexp(4.2 * q_ref)[1])


@contextlib.contextmanager
def fixed_accumulator(g, scale):
    """While the block runs, advance_p / move_p / boundary_p_inject / child_langmuir also sum every deposit as the integer
    llrint(v * scale): yields (a64 int64[nv, 12], streaks int32[nv]); the switch is cleared on the way out, always."""
    a64, streaks = np.zeros((g.nv, 12), np.int64), np.zeros(g.nv, np.int32)
    lib().orc_set_fixed_accumulator(_p(a64), _p(streaks), C.c_double(scale))
    try:
        yield a64, streaks
    finally:
        lib().orc_set_fixed_accumulator(None, None, C.c_double(0.0))


def finalize(a64, scale):
    """accumulator_t[nv] of the integer sums a64[nv, 12]: each converted int64 -> double (which rounds above 2^53), times
    the exact 1 / scale, rounded to float -- what the engine's acc_finalize leaves in a cleared accumulator."""
    a = (np.ascontiguousarray(a64, np.int64).astype(np.float64) * (1.0 / scale)).astype(np.float32)
    return np.ascontiguousarray(a.reshape(-1, 12)).view(L.accumulator_t).reshape(-1)


# ---- ... and of its deterministic hydro moments and rho (csrc/moments.hip) ----
class FixedMoments:
    """What fixed_moments yields: the integer sums h64[nv, 14] / r64[nv], the sums of the absolute values of the same
    integers habs64 / rabs64, the contributions per node count (hydro) / rcount (rho), skipped[2] (contributions out of
    the fixed-point range: hydro, rho), and the scales they were taken at"""

    def __init__(self, g, scales14, rho_scale):
        nv = g.nv
        self.scales = np.ascontiguousarray(scales14, np.float64)
        self.rho_scale = float(rho_scale)
        assert self.scales.shape == (14,)
        self.h64, self.habs64 = np.zeros((nv, 14), np.int64), np.zeros((nv, 14), np.int64)
        self.r64, self.rabs64 = np.zeros(nv, np.int64), np.zeros(nv, np.int64)
        self.count, self.rcount = np.zeros(nv, np.int32), np.zeros(nv, np.int32)
        self.skipped = np.zeros(2, np.int64)


@contextlib.contextmanager
def fixed_moments(g, scales14, rho_scale):
    """While the block runs, accumulate_hydro_p / accumulate_rho_p also sum every contribution they add to a node as the
    integer llrint(c * scale) -- scales14 for the 14 moments, rho_scale for the weights of rho: yields a FixedMoments;
    the switch is cleared on the way out, always.  The float results are what they are without it."""
    m = FixedMoments(g, scales14, rho_scale)
    lib().orc_set_fixed_moments(_p(m.h64), _p(m.habs64), _p(m.count), _p(m.r64), _p(m.rabs64), _p(m.rcount), _p(m.skipped),
                                _p(m.scales), C.c_double(m.rho_scale))
    try:
        yield m
    finally:
        lib().orc_set_fixed_moments(None, None, None, None, None, None, None, None, C.c_double(0.0))


def finalize_moments(prev, sums, scales):
    """What moments_finalize_kernel leaves in the float array `prev` (hydro_t[nv] with sums int64[nv, 14] and 14 scales, or
    float32[nv] with sums int64[nv] and one scale): per word with a non-zero sum, prev + float32(float64(sum) * (1 / scale))
    added in float32; a word whose sum is zero is left as it is.  Returns a new array."""
    s = np.ascontiguousarray(sums, np.int64).reshape(len(sums), -1)
    inv = 1.0 / np.asarray(scales, np.float64).reshape(-1)               # exact: the scales are powers of two
    assert inv.shape == (s.shape[1],)
    add = (s.astype(np.float64) * inv).astype(np.float32)
    out = np.array(prev)                                                 # a contiguous copy
    w = out.view(np.float32).reshape(len(s), -1)[:, :s.shape[1]]
    w[...] = np.where(s != 0, w + add, w)
    return out


def step(f, fi, a, m, species, g, sort=False, clean_e=False, clean_b=False, sync_shared=False, det_scale=None):
    """One vpic_simulation::advance() of a single self-periodic / locally bounded domain
    (src/vpic/advance.cxx:38-214 without emitters, collisions, injection and div cleaning).
    species: list of dicts {p, np, q_m, pm, partition}.  Returns nothing; arrays updated in place.
    det_scale: the step of an engine in deterministic accumulation -- once every species is pushed and its movers are
    handled, the accumulator is replaced by finalize() of the exact integer sums at that scale."""
    if det_scale is not None:
        with fixed_accumulator(g, det_scale) as (a64, _):
            _push(f, fi, a, species, g, sort)
            a[:g.nv] = finalize(a64, det_scale)
    else:
        _push(f, fi, a, species, g, sort)
    _fields(f, fi, a, m, species, g, clean_e, clean_b, sync_shared)


def _push(f, fi, a, species, g, sort):
    clear_accumulators(a, g)
    for sp in species:
        if sort:
            sort_p(sp["p"], sp["np"], sp["partition"], g)
    for sp in species:
        sp["nm"] = advance_p(sp["p"], sp["np"], sp["q_m"], sp["pm"], a, fi, g)
    for k, sp in enumerate(species):
        if sp["nm"]:
            sp["np"], _ = boundary_p_pack(sp["p"], sp["np"], sp["pm"], sp["nm"], k, f, g, sp["nm"])
            sp["nm"] = 0


def _fields(f, fi, a, m, species, g, clean_e, clean_b, sync_shared):
    clear_jf(f, g)
    unload_accumulator(f, a, g)
    synchronize_jf_local(f, g)
    advance_b(f, g, 0.5)
    advance_e(f, m, g)
    advance_b(f, g, 0.5)
    if clean_e:                                             # advance.cxx:151-173
        accumulate_rho(f, species, g)
        compute_div_e_err(f, m, g)
        if compute_rms_div_e_err(f, g) > 0:
            clean_div_e(f, m, g)
            compute_div_e_err(f, m, g)
            if compute_rms_div_e_err(f, g) > 0:
                clean_div_e(f, m, g)
    if clean_b:                                             # advance.cxx:177-195
        compute_div_b_err(f, g)
        if compute_rms_div_b_err(f, g) > 0:
            clean_div_b(f, g)
            compute_div_b_err(f, g)
            if compute_rms_div_b_err(f, g) > 0:
                clean_div_b(f, g)
    if sync_shared:                                         # advance.cxx:199-207
        synchronize_tang_e_norm_b_local(f, g)
    load_interpolator(fi, f, g)


def accumulate_rho(f, species, g):
    clear_rhof(f, g)
    for sp in species:
        accumulate_rho_p(f, sp["p"], sp["np"], g)
    synchronize_rho_local(f, g)


def initialize_fields(f, m, species, g):
    """initialize.cxx:32-76 on one domain."""
    synchronize_tang_e_norm_b_local(f, g)
    compute_div_b_err(f, g)
    clean_div_b(f, g)
    compute_curl_b(f, m, g)
    accumulate_rho(f, species, g)
    compute_rhob(f, m, g)
    compute_div_e_err(f, m, g)
    if compute_rms_div_e_err(f, g) > 0:
        clean_div_e(f, m, g)
    synchronize_tang_e_norm_b_local(f, g)
