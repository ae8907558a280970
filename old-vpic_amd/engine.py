"""Host-side mirror of the reference's kernel-level interface over the resident HIP engine.

Method names and argument meaning follow the reference's L3 C functions
(src/species_advance/standard/spa.h:23-123, src/sf_interface/sf_interface.h:83-163,
field_advance_methods_t in src/field_advance/field_advance.h:185-302); arrays cross this boundary
in the reference's own array-of-struct layouts (layout.py).  Everything computes on the GPU
through libvpic_hip.so; errors raise VpicHipError (the reference would print and exit(1),
src/util/util_base.h:213-219).
"""
import collections
import ctypes as C

import numpy as np

from . import layout as L
from ._lib import lib
from .cool import COOL_DRY, CoolDesc, CoolResult  # noqa: F401


class VpicHipError(RuntimeError):
    pass


class GridDesc(C.Structure):
    """vpic_hip_grid_t (include/vpic_hip.h) -- what the kernels read from grid_t (src/grid/grid.h:112-167)."""
    _fields_ = [("dt", C.c_float), ("cvac", C.c_float), ("eps0", C.c_float), ("damp", C.c_float),
                ("dx", C.c_float), ("dy", C.c_float), ("dz", C.c_float),
                ("rdx", C.c_float), ("rdy", C.c_float), ("rdz", C.c_float),
                ("nx", C.c_int32), ("ny", C.c_int32), ("nz", C.c_int32),
                ("fbc", C.c_int32 * 6), ("pbc", C.c_int32 * 6), ("rank", C.c_int32)]

    @property
    def nv(self):
        return L.nv(self.nx, self.ny, self.nz)


class SpectrumParams(C.Structure):
    """vpic_hip_spectrum_t (include/vpic_hip.h)"""
    _fields_ = [("n_lin", C.c_int32), ("n_log", C.c_int32), ("d_lin", C.c_double), ("log_lo", C.c_double), ("d_log", C.c_double)]


class DistAxis(C.Structure):
    """vpic_hip_dist_axis_t"""
    _fields_ = [("coord", C.c_int32), ("n", C.c_int32), ("lo", C.c_double), ("d", C.c_double)]


class DistRange(C.Structure):
    """vpic_hip_dist_range_t"""
    _fields_ = [("coord", C.c_int32), ("pad", C.c_int32), ("lo", C.c_double), ("hi", C.c_double)]


class DistDesc(C.Structure):
    """vpic_hip_dist_t (include/vpic_hip.h)"""
    _fields_ = [("n_axes", C.c_int32), ("n_sel", C.c_int32), ("axis", DistAxis * 2), ("sel", DistRange * 4)]


assert C.sizeof(DistDesc) == 152
DIST_COORDS = {"x": 0, "y": 1, "z": 2, "ux": 3, "uy": 4, "uz": 5, "ke": 6, "log10_ke": 7}    # VPIC_HIP_COORD_*
# in the frame of the local magnetic field, from the interpolator as it is loaded (VPIC_HIP_COORD_U_PAR ..).  VPIC_HIP_COORD_PITCH
# is "cos_pitch" here: it IS the cosine, and the name "pitch" stays unknown (KeyError), which callers and tests rely on.
FIELD_COORDS = {"u_par": 16, "u_perp": 17, "cos_pitch": 18, "mu": 19, "b": 20, "e_par": 21}
DIST_MAX_BINS, DIST_LDS_BINS = 1 << 22, 8192                                                   # VPIC_HIP_DIST_*


class DistValue(C.Structure):
    """vpic_hip_dist_value_t (include/vpic_hip.h): val = (f0 * f1) * f2 in units of quantum"""
    _fields_ = [("factor", C.c_int32 * 3), ("pad", C.c_int32), ("quantum", C.c_double)]


assert C.sizeof(DistValue) == 24
# the factors of a per-bin sum beyond the coordinates (VPIC_HIP_FACTOR_*); "log10_ke" is an axis and a range only
VALUE_FACTORS = {"one": 32, "q": 33, "edotv": 34, "epar_vpar": 35}
DIST_MAX_VALUES = 4                                                                            # VPIC_HIP_DIST_MAX_VALUES
DistSums = collections.namedtuple("DistSums", "counts isums sums refused")


# the coordinates and factors of a CELL of the grid (VPIC_HIP_CELL_*, numbered from 64: no particle code is one of them):
# the cell's centre, the 16 float words of field_t by their member names, the 14 of hydro_t as "hydro.<member>", the fields
# at the cell's centre, what derives from them, and "one" (a factor only)
CELL_FIELD_WORDS = ("ex", "ey", "ez", "div_e_err", "cbx", "cby", "cbz", "div_b_err", "tcax", "tcay", "tcaz", "rhob", "jfx", "jfy", "jfz", "rhof")
CELL_HYDRO_WORDS = ("jx", "jy", "jz", "rho", "px", "py", "pz", "ke", "txx", "tyy", "tzz", "tyz", "tzx", "txy")
CELL_COORDS = {"x": 64, "y": 65, "z": 66}
CELL_COORDS.update({name: 72 + w for w, name in enumerate(CELL_FIELD_WORDS)})                  # VPIC_HIP_CELL_F0 + word
CELL_COORDS.update({"hydro." + name: 88 + w for w, name in enumerate(CELL_HYDRO_WORDS)})       # VPIC_HIP_CELL_H0 + word
CELL_COORDS.update({name: 104 + k for k, name in enumerate(("ex_c", "ey_c", "ez_c", "bx_c", "by_c", "bz_c", "jx_c", "jy_c", "jz_c"))})
CELL_COORDS.update({name: 113 + k for k, name in enumerate(("e_c", "b_c", "e_par_c", "j_par_c", "jdote_c"))})
CELL_FACTORS = {"one": 127}                                                                     # VPIC_HIP_CELL_ONE


class SelectDesc(C.Structure):
    """vpic_hip_select_t (include/vpic_hip.h)"""
    _fields_ = [("n_sel", C.c_int32), ("flags", C.c_int32), ("sel", DistRange * 4),
                ("tag_lo", C.c_int64), ("tag_hi", C.c_int64), ("tag_every", C.c_int64), ("tag_phase", C.c_int64)]


assert C.sizeof(SelectDesc) == 136
class CollisionDesc(C.Structure):
    """vpic_hip_collision_t (include/vpic_hip.h)"""
    _fields_ = [("sp_a", C.c_int), ("sp_b", C.c_int), ("m_a", C.c_float), ("m_b", C.c_float), ("wq_a", C.c_float), ("wq_b", C.c_float),
                ("cvar", C.c_float), ("dt", C.c_float), ("seed", C.c_uint32), ("call", C.c_uint32)]


assert C.sizeof(CollisionDesc) == 40
SELECT_TAG_RANGE, SELECT_TAG_EVERY = 1, 2                                                      # VPIC_HIP_SELECT_*
WallTally = collections.namedtuple("WallTally", "count isum_q isum_qke sum_q sum_qke refused")
WallRecords = collections.namedtuple("WallRecords", "records dropped")
SelectResult = collections.namedtuple("SelectResult", "count particles fields index")
PARTICLE_COORDS = dict(DIST_COORDS, **FIELD_COORDS)                 # VPIC_HIP_COORD_* by name
PARTICLE_FACTORS = dict(PARTICLE_COORDS, **VALUE_FACTORS)            # ("log10_ke" is passed on and refused by the library)
CELL_FACTOR_CODES = dict(CELL_COORDS, **CELL_FACTORS)


def _set_ranges(desc, select, coords=PARTICLE_COORDS):
    """the (coord, lo, hi) ranges of `select`, coordinates by name in `coords` (KeyError for an unknown one), into desc.sel
    (vpic_hip_dist_range_t[4])"""
    for k, (coord, lo, hi) in enumerate(select):
        desc.sel[k] = DistRange(coords[coord], 0, float(lo), float(hi))


def _dist_desc(what, coords, axes, select):
    """vpic_hip_dist_t of one or two (coord, lo, d, n) axes and up to four (coord, lo, hi) ranges, coordinates by name in
    `coords` (KeyError for an unknown one)."""
    axes, select = list(axes), list(select)
    if len(axes) not in (1, 2) or len(select) > 4:
        raise ValueError(what + ": one or two axes and at most four ranges")
    d = DistDesc(len(axes), len(select))
    for k, (coord, lo, width, n) in enumerate(axes):
        d.axis[k] = DistAxis(coords[coord], int(n), float(lo), float(width))
    _set_ranges(d, select, coords)
    return d


def _dist_values(what, least, codes, values):
    """(vpic_hip_dist_value_t[max(n, 1)], n) of `least` to four ((factor, ...), quantum) values, one to three factors each by name
    in `codes` (KeyError for an unknown one); codes["one"] fills a value up to three factors"""
    values = list(values)
    if not least <= len(values) <= DIST_MAX_VALUES or any(not 1 <= len(f) <= 3 for f, _ in values):
        raise ValueError(what + " values of one to three factors each")
    v = (DistValue * max(len(values), 1))()
    for k, (factors, quantum) in enumerate(values):
        c = [codes[name] for name in factors]
        c += [codes["one"]] * (3 - len(c))
        v[k] = DistValue((C.c_int32 * 3)(*c), 0, float(quantum))
    return v, len(values)


def dist_desc(axes, select=()):
    """the descriptor of a species distribution: the coordinates of a particle"""
    return _dist_desc("distribution", PARTICLE_COORDS, axes, select)


def cell_dist_desc(axes, select=()):
    """the descriptor of a cell distribution: the coordinates of a cell ("one" is a factor only)"""
    return _dist_desc("cell_distribution", CELL_COORDS, axes, select)


def dist_values(values):
    """one to four values of a species distribution; a factor is "one", "q", "edotv", "epar_vpar" or a particle coordinate"""
    return _dist_values("distribution_sums: one to four", 1, PARTICLE_FACTORS, values)[0]


def cell_dist_values(values):
    """(array, n) of zero to four values of a cell distribution; a factor is "one" or a coordinate of a cell"""
    return _dist_values("cell_distribution: at most four", 0, CELL_FACTOR_CODES, values)


def select_desc(select=(), tag_range=None, tag_every=None):
    """vpic_hip_select_t of up to four (coord, lo, hi) ranges, tag_range = (lo, hi) and tag_every = (every, phase)."""
    select = list(select)
    if len(select) > 4:
        raise ValueError("select: at most four ranges")
    d = SelectDesc(len(select), 0)
    _set_ranges(d, select)
    if tag_range is not None:
        d.flags |= SELECT_TAG_RANGE
        d.tag_lo, d.tag_hi = int(tag_range[0]), int(tag_range[1])
    if tag_every is not None:
        d.flags |= SELECT_TAG_EVERY
        d.tag_every, d.tag_phase = int(tag_every[0]), int(tag_every[1])
    return d


def make_grid(nx, ny, nz, lx, ly, lz, dt, cvac=1.0, eps0=1.0, damp=0.0, fbc=None, pbc=None, rank=0):
    """A box domain.  Cell sizes are formed as partition_periodic_box does
    (src/grid/partition.c:60-66): double arithmetic, stored as float."""
    g = GridDesc()
    g.dt, g.cvac, g.eps0, g.damp = dt, cvac, eps0, damp
    g.dx, g.dy, g.dz = lx / nx, ly / ny, lz / nz
    g.rdx, g.rdy, g.rdz = nx / lx, ny / ly, nz / lz
    g.nx, g.ny, g.nz = nx, ny, nz
    g.rank = rank
    for f in range(6):
        g.fbc[f] = rank if fbc is None else fbc[f]
        g.pbc[f] = rank if pbc is None else pbc[f]
    return g


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class Engine:
    """One rectangular domain resident on one GPU."""

    device_type = "cuda"   # where exchange buffers handed to pack_*/unpack_*/inject must live

    def __init__(self, grid, device=-1):
        self._l = lib()
        self.grid = grid
        h = C.c_void_p()
        if self._l.vpic_hip_create(C.byref(h), C.byref(grid), device):
            raise VpicHipError(self._l.vpic_hip_last_error().decode())
        self._h = h
        self.nv = grid.nv
        self._n_sp = 0                                                # species created through new_species
        self._wall_quanta, self._wall_record_cap = None, 0           # what wall_setup was given

    def close(self):
        if getattr(self, "_h", None):
            self._l.vpic_hip_destroy(self._h)
            self._h = None

    __del__ = close

    def _ck(self, rc):
        if rc:
            raise VpicHipError(self._l.vpic_hip_last_error().decode())

    def _arr(self, a, dtype, n=None):
        a = np.ascontiguousarray(a, dtype=dtype)
        if n is not None and len(a) < n:
            raise VpicHipError(f"array of {len(a)} entries, need {n}")
        return a

    # ---- host mirrors ----
    def set_fields(self, f):
        f = self._arr(f, L.field_t, self.nv)
        self._ck(self._l.vpic_hip_set_fields(self._h, _ptr(f)))

    def get_fields(self):
        f = np.zeros(self.nv, L.field_t)
        self._ck(self._l.vpic_hip_get_fields(self._h, _ptr(f)))
        return f

    def set_interpolator(self, fi):
        fi = self._arr(fi, L.interpolator_t, self.nv)
        self._ck(self._l.vpic_hip_set_interpolator(self._h, _ptr(fi)))

    def get_interpolator(self):
        fi = np.zeros(self.nv, L.interpolator_t)
        self._ck(self._l.vpic_hip_get_interpolator(self._h, _ptr(fi)))
        return fi

    def set_accumulator(self, a):
        a = self._arr(a, L.accumulator_t, self.nv)
        self._ck(self._l.vpic_hip_set_accumulator(self._h, _ptr(a)))

    def get_accumulator(self):
        a = np.zeros(self.nv, L.accumulator_t)
        self._ck(self._l.vpic_hip_get_accumulator(self._h, _ptr(a)))
        return a

    def set_material_coefficients(self, m):
        m = self._arr(m, L.material_coefficient_t)
        self._ck(self._l.vpic_hip_set_material_coefficients(self._h, _ptr(m), len(m)))

    def set_vacuum(self):
        """One vacuum material (src/field_advance/standard/sfa.c:145-177 with eps=mu=1, sigma=0)."""
        m = np.zeros(1, L.material_coefficient_t)
        for n in ("decayx", "decayy", "decayz", "drivex", "drivey", "drivez", "rmux", "rmuy", "rmuz",
                  "nonconductive", "epsx", "epsy", "epsz"):
            m[n] = 1.0
        self.set_material_coefficients(m)

    # ---- species ----
    def new_species(self, q_m, max_np, max_nm):
        sp = self._l.vpic_hip_species_create(self._h, q_m, int(max_np), int(max_nm))
        if sp < 0:
            raise VpicHipError(self._l.vpic_hip_last_error().decode())
        self._n_sp = max(self._n_sp, sp + 1)
        return sp

    def set_particles(self, sp, p):
        p = self._arr(p, L.particle_t)
        self._ck(self._l.vpic_hip_species_set_particles(self._h, sp, _ptr(p), len(p)))

    def emit(self, sp, components, n_emit_per_face, ut_perp, ut_para, coef=32.0 / 81.0, thresh=0.0, seed=1):
        c = np.ascontiguousarray(components, np.int32)
        self._ck(self._l.vpic_hip_emit(self._h, sp, _ptr(c), len(c), n_emit_per_face, ut_perp, ut_para, coef, thresh, seed))

    def inject_aged(self, inj, tags=None):
        """Appends the injector records inj (particle_injector_t[n], sp_id names the species) and finishes their moves, as
        boundary_p does for arrivals; tags: int64[n, 2] (tag, tag2) the particles bring along, or None."""
        inj = self._arr(inj, L.particle_injector_t)
        t = None if tags is None else np.ascontiguousarray(tags, np.int64).reshape(len(inj), 2)
        self._ck(self._l.vpic_hip_inject_aged(self._h, _ptr(inj), None if t is None else _ptr(t), len(inj)))

    def accumulate_rhob(self, p, q_scale=1.0):
        p = self._arr(p, L.particle_t)
        self._ck(self._l.vpic_hip_accumulate_rhob(self._h, _ptr(p), len(p), q_scale))

    def set_maxwellian_reflux(self, code, ut_para, ut_perp, seed=1):
        a, b = np.ascontiguousarray(ut_para, np.float32), np.ascontiguousarray(ut_perp, np.float32)
        self._ck(self._l.vpic_hip_set_maxwellian_reflux(self._h, int(code), _ptr(a), _ptr(b), len(a), int(seed)))

    # ---- absorbing walls that tally and record what they take (include/vpic_hip.h: vpic_hip_wall_*) ----
    def wall_setup(self, q_quantum, qke_quantum, record_cap=0):
        """(Re)allocates and zeroes the tally table and the record buffer; the quanta of the sums of q and of q * ke."""
        self._ck(self._l.vpic_hip_wall_setup(self._h, q_quantum, qke_quantum, int(record_cap)))
        self._wall_quanta, self._wall_record_cap = (float(q_quantum), float(qke_quantum)), int(record_cap)

    def set_wall(self, code, record=False, tally=True):
        """Makes the particle boundary code a wall: ABSORB_PARTICLES itself or a code <= -3.  tally=False and
        record=False unregister it."""
        flags = (L.WALL_TALLY if tally or record else 0) | (L.WALL_RECORD if record else 0)
        self._ck(self._l.vpic_hip_set_wall(self._h, int(code), flags))

    def wall_tally(self, clear=False):
        """WallTally(count, isum_q, isum_qke: int64[7, n_sp]; sum_q, sum_qke: isum * quantum, float64; refused:
        int64[7, n_sp, 2]).  Rows 0..5: the faces -x -y -z +x +y +z where they are walls; row 6: everything else absorbed."""
        n_sp = self._n_sp
        if self._wall_quanta is None:                                # (the sums below need the quanta)
            raise VpicHipError("wall_tally before this Engine's wall_setup")
        t = np.zeros((L.WALL_ROWS, max(n_sp, 1)), L.wall_tally_t)
        self._ck(self._l.vpic_hip_wall_tally(self._h, _ptr(t), max(n_sp, 1), bool(clear)))
        t = t[:, :n_sp]
        iq, iqke = t["isum"][..., 0].copy(), t["isum"][..., 1].copy()
        return WallTally(t["count"].copy(), iq, iqke, iq * self._wall_quanta[0], iqke * self._wall_quanta[1], t["refused"].copy())

    def wall_records(self, clear=True, cap=None):
        """WallRecords(records: layout.wall_record_t in buffer order, dropped: records that did not fit into the device
        buffer since it was last cleared).  cap: read at most so many (default: the buffer's capacity)."""
        n, dropped = C.c_int64(0), C.c_int64(0)
        if cap is None:
            cap = self._wall_record_cap
        out = np.zeros(int(cap), L.wall_record_t)
        self._ck(self._l.vpic_hip_wall_records(self._h, _ptr(out) if cap else None, int(cap), C.byref(n), C.byref(dropped), bool(clear)))
        return WallRecords(out[:n.value], int(dropped.value))

    def set_reflux_draws(self, draws):
        """Test mode: draws[k] = (uniform, normal, normal) for the particle at index k of its species' array."""
        d = np.ascontiguousarray(draws, np.float32).reshape(-1, 3)
        self._ck(self._l.vpic_hip_set_reflux_draws(self._h, _ptr(d), len(d)))

    def set_emit_draws(self, draws):
        """Test mode of emit(): draws[slot] = six numbers, slot = component index * n_emit_per_face + k."""
        d = np.ascontiguousarray(draws, np.float64).reshape(-1, 6)
        self._ck(self._l.vpic_hip_set_emit_draws(self._h, _ptr(d), len(d)))

    def set_movers(self, sp, pm):
        pm = self._arr(pm, L.particle_mover_t)
        self._ck(self._l.vpic_hip_species_set_movers(self._h, sp, _ptr(pm), len(pm)))

    def append_particles(self, sp, p):
        p = self._arr(p, L.particle_t)
        self._ck(self._l.vpic_hip_species_append_particles(self._h, sp, _ptr(p), len(p)))

    def get_particles(self, sp):
        n = self.np(sp)
        p = np.zeros(n, L.particle_t)
        self._ck(self._l.vpic_hip_species_get_particles(self._h, sp, _ptr(p), n))
        return p

    def get_particles_range(self, sp, first, count):
        p = np.zeros(count, L.particle_t)
        self._ck(self._l.vpic_hip_species_get_particles_range(self._h, sp, _ptr(p), int(first), int(count)))
        return p

    def load_maxwellian(self, sp, ppc, seed, q, u=(0.0, 0.0, 0.0), vth=0.0):
        """ppc synthetic particles in every interior cell (device-side loader)."""
        self._ck(self._l.vpic_hip_species_load_maxwellian(self._h, sp, int(ppc), int(seed), q, u[0], u[1], u[2], vth))

    def load_profile(self, sp, count, q, ud=None, uth=None, *, seed, stream=0, global_dims=None, offset=(0, 0, 0),
                     flip=False, tags=None, append=False):
        """Load a species on the device from per-cell tables (include/vpic_hip.h: vpic_hip_species_load_profile, THE RULE).
        count, q and the entries of the triples ud (drift gamma beta) and uth (thermal spread of u) are scalars or numpy
        arrays shaped [tz, ty, tx], every extent 1 or the grid's; they are broadcast against each other to one shape.
        global_dims / offset: the whole grid (x, y, z) and this domain's first cell in it (default: this grid is the whole
        one).  tags=tag0 numbers the particles tag0, tag0 + 1, ... in the call's order.  Returns the particles loaded."""
        g = self.grid
        tabs = [np.asarray(count), np.asarray(q)]
        for triple in (ud, uth):
            if triple is not None and len(triple) != 3:
                raise VpicHipError("load_profile: ud and uth are triples (x, y, z)")
            tabs += [None if triple is None or triple[a] is None else np.asarray(triple[a]) for a in range(3)]
        for t in tabs:
            if t is not None and t.ndim not in (0, 3):
                raise VpicHipError(f"load_profile: a table is a scalar or shaped [tz, ty, tx], got shape {t.shape}")
        try:
            shape = np.broadcast_shapes(*[(1, 1, 1) if t is None or t.ndim == 0 else t.shape for t in tabs])
        except ValueError as err:
            raise VpicHipError(f"load_profile: the tables do not broadcast to one shape ({err})") from None
        keep = [None if t is None else np.ascontiguousarray(np.broadcast_to(t, shape), np.int32 if k == 0 else np.float32)
                for k, t in enumerate(tabs)]
        if not np.array_equal(keep[0], np.broadcast_to(tabs[0], shape)):
            raise VpicHipError("load_profile: count holds values that are not 32-bit integers")
        d = np.zeros(1, L.load_t)
        addr = [0 if t is None else t.ctypes.data for t in keep]
        d["count"], d["q"], d["ud"], d["uth"] = addr[0], addr[1], addr[2:5], addr[5:8]
        d["tdim"] = shape[::-1]
        d["gdim"] = (g.nx, g.ny, g.nz) if global_dims is None else tuple(int(v) for v in global_dims)
        d["goff"] = tuple(int(v) for v in offset)
        d["seed"], d["stream"] = int(seed) & 0xffffffff, int(stream) & 0xffffffff
        d["flags"] = (L.LOAD_APPEND if append else 0) | (L.LOAD_FLIP if flip else 0) | (L.LOAD_TAGS if tags is not None else 0)
        d["tag0"] = 0 if tags is None else int(tags)
        n = C.c_int64(0)
        self._ck(self._l.vpic_hip_species_load_profile(self._h, int(sp), _ptr(d), C.byref(n)))
        return int(n.value)

    def set_load_draws(self, draws):
        """Test mode of load_profile(): draws[m] = (x0, x1, x2, n0, n1, n2, U) for the particle at place m of a call's load,
        float32[n, 7]; None switches back to the device's generator."""
        if draws is None:
            self._ck(self._l.vpic_hip_set_load_draws(self._h, None, 0))
            return
        d = np.ascontiguousarray(draws, np.float32).reshape(-1, 7)
        self._ck(self._l.vpic_hip_set_load_draws(self._h, _ptr(d), len(d)))

    def np(self, sp):
        return int(self._l.vpic_hip_species_np(self._h, sp))

    def nm(self, sp):
        return int(self._l.vpic_hip_species_nm(self._h, sp))

    def get_movers(self, sp):
        n = self.nm(sp)
        pm = np.zeros(n, L.particle_mover_t)
        self._ck(self._l.vpic_hip_species_get_movers(self._h, sp, _ptr(pm), n))
        return pm

    def get_partition(self, sp):
        part = np.zeros(self.nv + 1, np.int32)
        self._ck(self._l.vpic_hip_species_get_partition(self._h, sp, _ptr(part)))
        return part

    def get_tile_partition(self, sp):
        """tpart[64 * tiles + 1] of the engine's own order (include/vpic_hip.h, vpic_hip_species_get_tile_partition)."""
        n = C.c_int64()
        self._ck(self._l.vpic_hip_species_get_tile_partition(self._h, sp, None, C.byref(n)))
        t = np.zeros(n.value, np.int32)
        self._ck(self._l.vpic_hip_species_get_tile_partition(self._h, sp, _ptr(t), C.byref(n)))
        return t

    # ---- kernels (reference names) ----
    def load_interpolator(self):
        self._ck(self._l.vpic_hip_load_interpolator(self._h))

    def clear_accumulators(self):
        self._ck(self._l.vpic_hip_clear_accumulators(self._h))

    def reduce_accumulators(self):
        self._ck(self._l.vpic_hip_reduce_accumulators(self._h))

    def unload_accumulator(self):
        self._ck(self._l.vpic_hip_unload_accumulator(self._h))

    def set_push_mode(self, mode):
        """'exact' (default: the reference's scalar arithmetic, bit for bit) or 'fast' (include/vpic_hip.h)."""
        if mode == "exact" and not hasattr(self._l, "vpic_hip_set_push_mode"):
            return                                          # an older build of the ABI (VPIC_HIP_LIB, A/B timing): exact is all it has
        self._ck(self._l.vpic_hip_set_push_mode(self._h, {"exact": 0, "fast": 1}[mode]))

    def set_accumulation(self, mode, q_ref=0.0):
        """'float' (default) or 'deterministic' (64-bit fixed-point sums: bit-identical from run to run): include/vpic_hip.h."""
        self._ck(self._l.vpic_hip_set_accumulation(self._h, {"float": 0, "deterministic": 1}[mode], q_ref))

    def advance_p(self, sp):
        """Returns the number of movers, like the reference's advance_p."""
        self._ck(self._l.vpic_hip_advance_p(self._h, sp))
        return self.nm(sp)

    # ---- the exchange that keeps its counts on the device (include/vpic_hip.h: vpic_hip_exchange_*) ----
    def advance_p_async(self, sp):
        self._ck(self._l.vpic_hip_advance_p_async(self._h, sp))

    def advance_p_phase(self, sp, phase):
        """phase 1: the tiles on the faces shared with other domains and the appended particles; 2: the other tiles."""
        self._ck(self._l.vpic_hip_advance_p_phase(self._h, sp, int(phase)))

    def capacity(self, sp):
        """(extent, max_np, max_nm): array slots in use (live particles + dead slots) and the capacities."""
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        self._ck(self._l.vpic_hip_species_capacity(self._h, sp, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def reserve(self, sp, max_np, max_nm):
        self._ck(self._l.vpic_hip_species_reserve(self._h, sp, int(max_np), int(max_nm)))

    def exchange_begin(self):
        self._ck(self._l.vpic_hip_exchange_begin(self._h))

    @staticmethod
    def exchange_message_bytes(cap):
        return 16 + 48 * int(cap)

    def exchange_pack(self, msg_ptrs, caps, mover_cap, species=None):
        """msg_ptrs / caps: per face 0..5, a device pointer (or 0) and the payload capacity of its message;
        species: the species whose movers are packed (default: all)."""
        m = (C.c_void_p * 6)(*[p or None for p in msg_ptrs])
        c = (C.c_int32 * 6)(*[int(x) for x in caps])
        if species is None:
            self._ck(self._l.vpic_hip_exchange_pack(self._h, m, c, int(mover_cap)))
        else:
            mask = sum(1 << int(k) for k in species)
            self._ck(self._l.vpic_hip_exchange_pack_species(self._h, mask, m, c, int(mover_cap)))

    def exchange_inject(self, msg_ptr, cap):
        self._ck(self._l.vpic_hip_exchange_inject(self._h, msg_ptr, int(cap)))

    def exchange_finish(self, recv_ptrs):
        """The one synchronisation of the particle exchange.  Returns the headers of the received messages
        ([count, wanted, 0, 0] each); np / nm of every species are current on the host afterwards."""
        n = len(recv_ptrs)
        r = (C.c_void_p * max(n, 1))(*recv_ptrs)
        h = (C.c_int32 * (4 * max(n, 1)))()
        flags = C.c_int32()
        self._ck(self._l.vpic_hip_exchange_finish(self._h, r, n, h, C.byref(flags)))
        self.exchange_flags = flags.value
        return [list(h[4 * k:4 * k + 4]) for k in range(n)]

    def advance_e_part(self, part):
        self._ck(self._l.vpic_hip_advance_e_part(self._h, int(part)))

    def stream_wait_event(self, hip_event):
        self._ck(self._l.vpic_hip_stream_wait_event(self._h, hip_event))

    def sort_p(self, sp):
        self._ck(self._l.vpic_hip_sort_p(self._h, sp))

    def sort_advance_p(self, sp):
        """sort_p then advance_p as one call (the push does the sort's moving when it can: vpic_hip_sort_advance_p)."""
        self._ck(self._l.vpic_hip_sort_advance_p(self._h, sp))
        return self.nm(sp)

    def energy_p(self, sp):
        e = C.c_double()
        self._ck(self._l.vpic_hip_energy_p(self._h, sp, C.byref(e)))
        return e.value

    # ---- binary Coulomb collisions (include/vpic_hip.h: vpic_hip_collide) ----
    def collide(self, sp_a, sp_b=None, *, m_a, m_b=None, wq_a, wq_b=None, cvar, dt, seed, call, relativistic=False):
        """Takizuka-Abe collisions of the particles of species sp_a among themselves (sp_b None or sp_a) or with those of
        sp_b, cell by cell on the device; only ux, uy, uz of the two species change.  m: mass of a physical particle, wq:
        1 / |charge of a physical particle| (a macro-particle weighs |q| * wq), cvar = (q_a q_b)^2 ln(Lambda) / (8 pi eps0^2
        c^3), dt the time the call stands for, (seed, call) the counter of its random stream.  Non-relativistic (|u| << 1)
        unless relativistic=True, which takes the pair of Perez et al. 2012 (vpic_hip_collide_relativistic: the same pairing,
        draws and weight rule, the pair turned in its centre-of-momentum frame in double, sum m u and sum m gamma kept);
        rank-local, at most COLLIDE_MAX_CELL particles of a species per cell; a species whose cell ranges are not exact is
        sorted first (collide_stats()["sorted_first"]).  A copy of the species' particles held on the host is stale afterwards."""
        if sp_b is None:
            sp_b = sp_a
        same = int(sp_b) == int(sp_a)
        d = CollisionDesc(int(sp_a), int(sp_b), float(m_a), float(m_a if m_b is None and same else m_b if m_b is not None else -1.0),
                          float(wq_a), float(wq_a if wq_b is None and same else wq_b if wq_b is not None else -1.0),
                          float(cvar), float(dt), int(seed) & 0xffffffff, int(call) & 0xffffffff)
        call_ = self._l.vpic_hip_collide_relativistic if relativistic else self._l.vpic_hip_collide
        self._ck(call_(self._h, C.byref(d)))

    def collide_stats(self):
        """dict of the last collide call: cells with a pair, pairs scattered, pairs skipped (no relative velocity), pairs
        of which not both particles were updated (unequal weights), the fullest cell (particles of one species), whether a
        species was sorted first, and the kernel instance that ran ("wave", "group" or None)."""
        out = (C.c_int64 * 6)()
        self._ck(self._l.vpic_hip_collide_stats(self._h, out))
        inst = C.c_int(0)
        self._ck(self._l.vpic_hip_collide_instance(self._h, C.byref(inst)))
        d = dict(zip(("cells", "pairs", "skipped", "one_sided", "fullest_cell", "sorted_first"), [int(v) for v in out]))
        d["instance"] = (None, "wave", "group")[inst.value]
        return d

    def set_collide_draws(self, draws):
        """Test mode of collide(): draws[i] = (normal, cos phi, sin phi, uniform) for the pair whose first particle is at index
        i of its species' array, float32[n, 4]; None switches back to the device's counter stream."""
        if draws is None:
            self._ck(self._l.vpic_hip_set_collide_draws(self._h, None, 0))
            return
        d = np.ascontiguousarray(draws, np.float32).reshape(-1, 4)
        self._ck(self._l.vpic_hip_set_collide_draws(self._h, _ptr(d), len(d)))

    # ---- radiative cooling (include/vpic_hip.h: vpic_hip_species_cool) ----
    def cool(self, sp, sync, ic=0.0, quantum=2.0 ** -40, dry=False, cells=False):
        """Synchrotron losses and Compton drag of one species on the device, one pass that changes ux, uy, uz and nothing
        else: sync = tau0 (q / m c)^2 and ic = (4/3) sigma_T U_ph / (m c), each times the time the call stands for (the
        header states the rule operation by operation).  The fields are those of the interpolator as it is loaded at the
        call.  Returns CoolResult(isum, energy, cell_isums, stats): isum the energy the drag took, sum |q| (gamma - gamma'),
        as an exact integer sum in units of quantum (the same in every array order), energy = isum * quantum, cell_isums
        int64[nv] the same per voxel (cells=True) or None, stats a dict of seen, changed, refused (for the tally: |val /
        quantum| >= 2^32) and left_alone (a result that is not finite).  dry=True returns the same tallies and writes
        nothing.  A copy of the species' particles held on the host is stale afterwards."""
        d = CoolDesc(float(sync), float(ic), float(quantum), COOL_DRY if dry else 0, 0)
        isum = C.c_int64()
        cell = np.zeros(self.nv, np.int64) if cells else None
        self._ck(self._l.vpic_hip_species_cool(self._h, int(sp), C.byref(d), C.byref(isum), _ptr(cell) if cells else None))
        return CoolResult(isum.value, isum.value * float(quantum), cell, self.cool_stats())

    def cool_stats(self):
        """dict of the last cool call: live particles seen, particles whose momenta changed in any bit (dry: would have),
        particles refused for the tally, particles left alone."""
        out = (C.c_int64 * 4)()
        self._ck(self._l.vpic_hip_species_cool_stats(self._h, out))
        return dict(zip(("seen", "changed", "refused", "left_alone"), [int(v) for v in out]))

    # ---- energy spectra (include/vpic_hip.h: vpic_hip_energy_spectrum) ----
    def energy_spectrum(self, sp, n_lin=0, d_lin=0.0, n_log=0, log_lo=0.0, d_log=0.0):
        """(lin_counts[n_lin, nv] uint32, log_counts[n_log] uint64) of the species' kinetic energies; None for a part
        not asked for (n_lin == 0 / n_log == 0)."""
        prm = SpectrumParams(int(n_lin), int(n_log), float(d_lin), float(log_lo), float(d_log))
        lin = np.zeros((n_lin, self.nv), np.uint32) if n_lin > 0 else None
        log = np.zeros(n_log, np.uint64) if n_log > 0 else None
        self._ck(self._l.vpic_hip_energy_spectrum(self._h, int(sp), C.byref(prm), _ptr(lin) if n_lin > 0 else None,
                                                  _ptr(log) if n_log > 0 else None))
        return lin, log

    def energy_bands(self, sp, n_lin, d_lin):
        """float32[n_lin, nv]: every voxel's share of its particles per linear energy band, ghost voxels filled from
        their interior neighbours (what the production deck's energy diagnostic writes)."""
        prm = SpectrumParams(int(n_lin), 0, float(d_lin), 0.0, 0.0)
        bands = np.zeros((max(int(n_lin), 0), self.nv), np.float32)
        self._ck(self._l.vpic_hip_energy_bands(self._h, int(sp), C.byref(prm), _ptr(bands)))
        return bands

    def energy_spectrum_stats(self):
        """(particles counted, window misses) of the last energy_spectrum / energy_bands call."""
        out = (C.c_int64 * 2)()
        self._ck(self._l.vpic_hip_energy_spectrum_stats(self._h, out))
        return int(out[0]), int(out[1])

    # ---- phase-space distributions (include/vpic_hip.h: vpic_hip_species_distribution) ----
    def distribution(self, sp, axes, select=()):
        """uint64[n0] or uint64[n1, n0]: the histogram of the species over one or two axes (coord, lo, d, n) -- n bins of
        width d from lo; coord one of "x", "y", "z" (cells from the low corner of the interior), "ux", "uy", "uz", "ke",
        "log10_ke", or in the frame of the local magnetic field "u_par", "u_perp", "cos_pitch" (the cosine of the pitch angle),
        "mu" (u_perp^2 / 2|cB|), "b" (|cB|), "e_par", which use the interpolator AS IT IS LOADED at the call
        (load_interpolator first for the current fields) -- of the particles inside every (coord, lo, hi) range of
        `select`, whose coordinates are the same twelve."""
        d = dist_desc(axes, select)
        n0, n1 = max(d.axis[0].n, 0), max(d.axis[1].n, 0) if d.n_axes == 2 else 1
        counts = np.zeros(min(n0 * n1, DIST_MAX_BINS), np.uint64)        # (a descriptor the library refuses is refused below)
        self._ck(self._l.vpic_hip_species_distribution(self._h, int(sp), C.byref(d), _ptr(counts) if counts.size else None))
        return counts.reshape(n1, n0) if d.n_axes == 2 else counts

    def distribution_stats(self):
        """(live particles seen, kept by the selection, counted, added through global memory) of the last distribution call."""
        out = (C.c_int64 * 4)()
        self._ck(self._l.vpic_hip_species_distribution_stats(self._h, out))
        return tuple(int(v) for v in out)

    def distribution_sums(self, sp, axes, values, select=()):
        """DistSums(counts, isums, sums, refused): beside the histogram of `distribution` (counts, the same bit for bit),
        per-bin sums of up to four values over the particles counted.  values: ((factor, ...), quantum) each, one to three
        factors whose product is the particle's value: a coordinate of `distribution` other than "log10_ke", "one",
        "q" (the particle's macro-charge, its weight), "edotv" (E . u / gamma) or "epar_vpar" (e_par u_par / gamma).
        isums int64[n_val, n0] or [n_val, n1, n0]: the sum of rint(value / quantum), exact integers -- the same in every
        order of the array and additive across ranks; sums = isums * quantum (float64); refused int64[n_val]: particles
        whose |value / quantum| is 2^32 or more or NaN, which add nothing to that value."""
        d = dist_desc(axes, select)
        v = dist_values(values)
        n0, n1 = max(d.axis[0].n, 0), max(d.axis[1].n, 0) if d.n_axes == 2 else 1
        bins = min(n0 * n1, DIST_MAX_BINS)                               # (a descriptor the library refuses is refused below)
        counts = np.zeros(bins, np.uint64)
        isums = np.zeros((len(v), bins), np.int64)
        self._ck(self._l.vpic_hip_species_distribution_sums(self._h, int(sp), C.byref(d), v, len(v), _ptr(counts) if bins else None,
                                                            _ptr(isums) if bins else None))
        shape = (n1, n0) if d.n_axes == 2 else (n0,)
        isums = isums.reshape((len(v),) + shape)
        quanta = np.array([x.quantum for x in v]).reshape((len(v),) + (1,) * len(shape))
        return DistSums(counts.reshape(shape), isums, isums * quanta, np.array(self.distribution_sums_stats()[4:4 + len(v)], np.int64))

    def distribution_sums_stats(self):
        """(live particles seen, kept by the selection, counted, added through global memory, refused for value 0, 1, 2, 3)
        of the last distribution_sums call."""
        out = (C.c_int64 * 8)()
        self._ck(self._l.vpic_hip_species_distribution_sums_stats(self._h, out))
        return tuple(int(x) for x in out)

    # ---- cell distributions (include/vpic_hip.h: vpic_hip_cell_distribution) ----
    def cell_distribution(self, axes, values=(), select=()):
        """DistSums(counts, isums, sums, refused) over the nx ny nz interior CELLS of the grid, shaped like distribution_sums:
        the histogram over one or two axes (coord, lo, d, n) of the cells inside every (coord, lo, hi) range of `select`, and
        per-bin sums of zero to four values ((factor, ...), quantum).  Coordinates: "x", "y", "z" (the cell's centre in
        cells: lo 0, d 1, n nx is one bin per column); the words of the field record at the cell's voxel by field_t's member
        names, "ex" .. "rhof"; those of the hydro record, "hydro.jx" .. "hydro.txy" (the hydro array must exist:
        clear_hydro, set_hydro or accumulate_hydro_p first); the fields at the cell's centre from the field array as
        load_interpolator forms them, "ex_c" .. "bz_c", and the current likewise, "jx_c" .. "jz_c"; "e_c", "b_c" (moduli),
        "e_par_c", "j_par_c" (along B), "jdote_c" (J . E).  A factor is any of them or "one".  Integers throughout: the
        same on either path, additive across ranks; refused int64[n_val]: cells whose |value / quantum| is 2^32 or more or
        NaN, which add nothing to that value.  Nothing the engine holds is changed."""
        d = cell_dist_desc(axes, select)
        v, n_val = cell_dist_values(values)
        n0, n1 = max(d.axis[0].n, 0), max(d.axis[1].n, 0) if d.n_axes == 2 else 1
        bins = min(n0 * n1, DIST_MAX_BINS)                               # (a descriptor the library refuses is refused below)
        counts = np.zeros(bins, np.uint64)
        isums = np.zeros((n_val, bins), np.int64)
        self._ck(self._l.vpic_hip_cell_distribution(self._h, C.byref(d), v if n_val else None, n_val, _ptr(counts) if bins else None,
                                                    _ptr(isums) if bins and n_val else None))
        shape = (n1, n0) if d.n_axes == 2 else (n0,)
        isums = isums.reshape((n_val,) + shape)
        quanta = np.array([v[k].quantum for k in range(n_val)]).reshape((n_val,) + (1,) * len(shape))
        return DistSums(counts.reshape(shape), isums, isums * quanta, np.array(self.cell_distribution_stats()[4:4 + n_val], np.int64))

    def cell_distribution_stats(self):
        """(cells seen, kept by the ranges, counted, counted through global memory, refused for value 0, 1, 2, 3) of the last
        cell_distribution call."""
        out = (C.c_int64 * 8)()
        self._ck(self._l.vpic_hip_cell_distribution_stats(self._h, out))
        return tuple(int(x) for x in out)

    # ---- selected particles (include/vpic_hip.h: vpic_hip_species_select) ----
    def select_count(self, sp, select=(), tag_range=None, tag_every=None):
        """how many live particles of the species lie inside every (coord, lo, hi) range of `select` and have the tags
        asked for: tag_range = (lo, hi) keeps lo <= tag < hi, tag_every = (every, phase) keeps tag % every == phase.
        The coordinates are those of `distribution`, "u_par", "u_perp", "cos_pitch", "mu", "b" and "e_par" included, which
        use the interpolator as it is loaded at the call."""
        d = select_desc(select, tag_range, tag_every)
        n = C.c_int64()
        self._ck(self._l.vpic_hip_species_select_count(self._h, int(sp), C.byref(d), C.byref(n)))
        return n.value

    def select(self, sp, select=(), tag_range=None, tag_every=None, cap=None, fields=False, index=False):
        """SelectResult(count, particles, fields, index) of those particles, in the order of the species' array:
        particles particle_t[n]; fields float32[n, 6], (ex, ey, ez, cbx, cby, cbz) at the particle from the interpolator
        as it is loaded, or None; index int64[n], the particle's place in the array, or None.  n = count, or
        min(count, cap) when a cap is given (count is the number kept either way); without one the particles are counted
        first and the arrays sized exactly.  A range over "u_par", "u_perp", "cos_pitch", "mu", "b" or "e_par" uses the same
        interpolator as `fields` does: the one loaded at the call."""
        d = select_desc(select, tag_range, tag_every)
        if cap is None:
            cap = self.select_count(sp, select, tag_range, tag_every)
        cap = int(cap)
        room = max(cap, 0)
        p = np.zeros(room, L.particle_t)
        f = np.zeros((room, 6), np.float32) if fields else None
        i = np.zeros(room, np.int64) if index else None
        n = C.c_int64()
        self._ck(self._l.vpic_hip_species_select(self._h, int(sp), C.byref(d), cap, _ptr(p), _ptr(f) if fields else None,
                                                 _ptr(i) if index else None, C.byref(n)))
        m = min(n.value, room)
        return SelectResult(n.value, p[:m], f[:m] if fields else None, i[:m] if index else None)

    def select_stats(self):
        """(live particles seen, kept, records written, chunks the array was cut into) of the last select / select_count call."""
        out = (C.c_int64 * 4)()
        self._ck(self._l.vpic_hip_species_select_stats(self._h, out))
        return tuple(int(v) for v in out)

    def center_p(self, sp):
        self._ck(self._l.vpic_hip_center_p(self._h, sp))

    def uncenter_p(self, sp):
        self._ck(self._l.vpic_hip_uncenter_p(self._h, sp))

    # ---- hydro moments (sf_interface.h:83-163, spa.h:115-123) --------------------------------------
    def clear_hydro(self):
        self._ck(self._l.vpic_hip_clear_hydro(self._h))

    def accumulate_hydro_p(self, sp, select=(), tag_range=None, tag_every=None):
        """adds the species' hydro moments to the engine's hydro array; with a selection -- (coord, lo, hi) ranges,
        tag_range = (lo, hi), tag_every = (every, phase): the arguments of `select`, the same coordinate names -- only the
        particles that `select` would return add (include/vpic_hip.h: vpic_hip_accumulate_hydro_p_select; the ranges
        look at the stored momenta and the interpolator as it is loaded, the species is left as it is)."""
        if not select and tag_range is None and tag_every is None:
            self._ck(self._l.vpic_hip_accumulate_hydro_p(self._h, sp))
            return
        d = select_desc(select, tag_range, tag_every)
        self._ck(self._l.vpic_hip_accumulate_hydro_p_select(self._h, int(sp), C.byref(d)))

    def moments_stats(self):
        """(live particles summed, added through an LDS window, added through global memory, contributions out of the
        fixed-point range) of the last accumulate_hydro_p / accumulate_rho_p call (include/vpic_hip.h)."""
        out = (C.c_int64 * 4)()
        self._ck(self._l.vpic_hip_moments_stats(self._h, out))
        return tuple(int(v) for v in out)

    def synchronize_hydro(self):
        self._ck(self._l.vpic_hip_synchronize_hydro(self._h))

    def set_hydro(self, h):
        h = np.ascontiguousarray(h, L.hydro_t)
        assert len(h) == self.nv
        self._ck(self._l.vpic_hip_set_hydro(self._h, _ptr(h)))

    def get_hydro(self):
        h = np.zeros(self.nv, L.hydro_t)
        self._ck(self._l.vpic_hip_get_hydro(self._h, _ptr(h)))
        return h

    def dump_gather(self, what, layout, words=(), strides=(1, 1, 1)):
        """Payload of field_dump (what 0) / hydro_dump (what 1) as uint32 words; layout 0 band
        [len(words), nz/sz+2, ny/sy+2, nx/sx+2], 1 interleaved records with the boundary entries,
        2 hydro_dump's interleaved shape (dump.cxx:1116-1552)."""
        W = 20 if what == 0 else 16
        no = [n // s for n, s in zip((self.grid.nx, self.grid.ny, self.grid.nz), strides)]
        dim = [n + (0 if layout == 2 else 2) for n in no]
        shape = (len(words), dim[2], dim[1], dim[0]) if layout == 0 else (dim[2], dim[1], dim[0], W)
        out = np.zeros(shape, np.uint32)
        w = np.asarray(words, np.int32)
        self._ck(self._l.vpic_hip_dump_gather(self._h, what, layout, _ptr(w), len(w), int(strides[0]),
                                              int(strides[1]), int(strides[2]), _ptr(out), out.nbytes))
        return out

    # ---- divergence cleaning family and charge densities (field_advance.h:242-302, spa.h:108-113) ----
    def clear_rhof(self):
        self._ck(self._l.vpic_hip_clear_rhof(self._h))

    def accumulate_rho_p(self, sp):
        self._ck(self._l.vpic_hip_accumulate_rho_p(self._h, sp))

    def synchronize_rho(self):
        self._ck(self._l.vpic_hip_synchronize_rho(self._h))

    def compute_rhob(self):
        self._ck(self._l.vpic_hip_compute_rhob(self._h))

    def compute_curl_b(self):
        self._ck(self._l.vpic_hip_compute_curl_b(self._h))

    def synchronize_tang_e_norm_b(self):
        err = C.c_double()
        self._ck(self._l.vpic_hip_synchronize_tang_e_norm_b(self._h, C.byref(err)))
        return err.value

    def compute_div_e_err(self):
        self._ck(self._l.vpic_hip_compute_div_e_err(self._h))

    def compute_rms_div_e_err(self):
        r = C.c_double()
        self._ck(self._l.vpic_hip_compute_rms_div_e_err(self._h, C.byref(r)))
        return r.value

    def clean_div_e(self):
        self._ck(self._l.vpic_hip_clean_div_e(self._h))

    def compute_div_b_err(self):
        self._ck(self._l.vpic_hip_compute_div_b_err(self._h))

    def compute_rms_div_b_err(self):
        r = C.c_double()
        self._ck(self._l.vpic_hip_compute_rms_div_b_err(self._h, C.byref(r)))
        return r.value

    def clean_div_b(self):
        self._ck(self._l.vpic_hip_clean_div_b(self._h))

    def clear_jf(self):
        self._ck(self._l.vpic_hip_clear_jf(self._h))

    def clear_jf_unload_accumulator(self):
        self._ck(self._l.vpic_hip_clear_jf_unload_accumulator(self._h))

    def synchronize_jf(self):
        self._ck(self._l.vpic_hip_synchronize_jf(self._h))

    def local_adjust_jf(self):
        self._ck(self._l.vpic_hip_local_adjust_jf(self._h))

    def synchronize_jf_self(self, axis):
        self._ck(self._l.vpic_hip_synchronize_jf_self(self._h, axis))

    def advance_b(self, frac):
        self._ck(self._l.vpic_hip_advance_b(self._h, frac))

    def advance_e(self):
        self._ck(self._l.vpic_hip_advance_e(self._h))

    def energy_f(self):
        en = np.zeros(6, np.float64)
        self._ck(self._l.vpic_hip_energy_f(self._h, _ptr(en)))
        return en

    def boundary_p_pack(self):
        self._ck(self._l.vpic_hip_boundary_p_pack(self._h))
        ns = (C.c_int32 * 6)()
        self._ck(self._l.vpic_hip_boundary_p_counts(self._h, ns))
        return list(ns)

    def send_buffer(self, face):
        return self._l.vpic_hip_boundary_p_send_buffer(self._h, face)

    def get_injectors(self, face, dev_ptr):
        self._ck(self._l.vpic_hip_boundary_p_get_injectors(self._h, face, dev_ptr))

    def boundary_p_inject(self, dev_ptr, n):
        self._ck(self._l.vpic_hip_boundary_p_inject(self._h, dev_ptr, int(n)))

    def face_count(self, d):
        return self._l.vpic_hip_face_count(self._h, d)

    def pack_tang_b(self, d, dev_ptr):
        self._ck(self._l.vpic_hip_pack_tang_b(self._h, d, dev_ptr))

    def unpack_tang_b(self, d, dev_ptr):
        self._ck(self._l.vpic_hip_unpack_tang_b(self._h, d, dev_ptr))

    def pack_jf(self, d, dev_ptr):
        self._ck(self._l.vpic_hip_pack_jf(self._h, d, dev_ptr))

    def unpack_jf(self, d, dev_ptr):
        self._ck(self._l.vpic_hip_unpack_jf(self._h, d, dev_ptr))

    # pieces of the divergence-cleaning family for domains that share faces with other domains
    def local_adjust_rho(self):
        self._ck(self._l.vpic_hip_local_adjust_rho(self._h))

    def synchronize_rho_self(self, axis):
        self._ck(self._l.vpic_hip_synchronize_rho_self(self._h, axis))

    def rho_count(self, d):
        return self._l.vpic_hip_rho_count(self._h, d)

    def pack_rho(self, d, dev_ptr):
        self._ck(self._l.vpic_hip_pack_rho(self._h, d, dev_ptr))

    def unpack_rho(self, d, dev_ptr):
        self._ck(self._l.vpic_hip_unpack_rho(self._h, d, dev_ptr))

    # ... and of the hydro moments (sf_interface/hydro.c:28-200)
    def local_adjust_hydro(self):
        self._ck(self._l.vpic_hip_local_adjust_hydro(self._h))

    def synchronize_hydro_self(self, axis):
        self._ck(self._l.vpic_hip_synchronize_hydro_self(self._h, axis))

    def hydro_count(self, d):
        return self._l.vpic_hip_hydro_count(self._h, d)

    def pack_hydro(self, d, dev_ptr):
        self._ck(self._l.vpic_hip_pack_hydro(self._h, d, dev_ptr))

    def unpack_hydro(self, d, dev_ptr):
        self._ck(self._l.vpic_hip_unpack_hydro(self._h, d, dev_ptr))

    def message_count(self, kind, d):
        return self._l.vpic_hip_face_message_count(self._h, kind, d)

    def pack_message(self, kind, d, dev_ptr):
        self._ck(self._l.vpic_hip_pack_face_message(self._h, kind, d, dev_ptr))

    def unpack_message(self, kind, d, dev_ptr):
        """Returns the squared-difference sum of a kind-2 message, 0.0 otherwise."""
        err = C.c_double()
        self._ck(self._l.vpic_hip_unpack_face_message(self._h, kind, d, dev_ptr, C.byref(err)))
        return err.value

    def local_adjust_tang_e_norm_b(self):
        self._ck(self._l.vpic_hip_local_adjust_tang_e_norm_b(self._h))

    def synchronize_tang_e_norm_b_self(self, axis):
        err = C.c_double()
        self._ck(self._l.vpic_hip_synchronize_tang_e_norm_b_self(self._h, axis, C.byref(err)))
        return err.value

    def rms_div_e_err_local(self):
        l2 = (C.c_double * 2)()
        self._ck(self._l.vpic_hip_rms_div_e_err_local(self._h, l2))
        return l2[0], l2[1]

    def rms_div_b_err_local(self):
        l2 = (C.c_double * 2)()
        self._ck(self._l.vpic_hip_rms_div_b_err_local(self._h, l2))
        return l2[0], l2[1]

    def sort_due(self, sp, max_interval=0):
        """Adaptive sorting: should species sp be sorted before its next advance_p?"""
        d = C.c_int()
        self._ck(self._l.vpic_hip_sort_due(self._h, sp, int(max_interval), C.byref(d)))
        return bool(d.value)

    def set_sort_order(self, order):
        """'reference' (by voxel, the default) or 'engine' (tile order where it applies): include/vpic_hip.h."""
        self._ck(self._l.vpic_hip_set_sort_order(self._h, {"reference": 0, "engine": 1}[order]))

    def species_order(self, sp):
        """'none', 'voxel' (partition valid) or 'tile' (include/vpic_hip.h, vpic_hip_species_sort_order)."""
        o = C.c_int(0)
        self._ck(self._l.vpic_hip_species_sort_order(self._h, sp, C.byref(o)))
        return ("none", "voxel", "tile")[o.value]

    def species_stats(self, sp):
        """dict of what the engine knows about the species' last push and its sorts (include/vpic_hip.h, vpic_hip_species_stats)"""
        out = (C.c_int64 * 8)()
        self._ck(self._l.vpic_hip_species_stats(self._h, int(sp), out))
        return dict(zip(("crossed", "fullest_tile", "missed_runs", "sorts", "early_sorts", "too_clumped_for_tiles", "by_tile_only", "dead_slots"), [int(v) for v in out]))

    def measure_disorder(self, sp):
        f = C.c_double()
        self._ck(self._l.vpic_hip_measure_disorder(self._h, sp, C.byref(f)))
        return f.value

    def step(self, step, sort_interval=0):
        self._ck(self._l.vpic_hip_step(self._h, int(step), int(sort_interval)))

    def sync(self):
        self._ck(self._l.vpic_hip_sync(self._h))

    def stream(self):
        return self._l.vpic_hip_stream(self._h)

    def profile_enable(self, on=True):
        self._ck(self._l.vpic_hip_profile_enable(self._h, int(on)))

    def profile_read(self):
        ms, n, parts = C.c_double(), C.c_int64(), C.c_int64()
        self._ck(self._l.vpic_hip_profile_read(self._h, C.byref(ms), C.byref(n), C.byref(parts)))
        return ms.value, n.value, parts.value

    def profile_read_species(self, sp):
        """the plain advance_p launches of one species: (ms, launches, particles)"""
        ms, n, parts = C.c_double(), C.c_int64(), C.c_int64()
        self._ck(self._l.vpic_hip_profile_read_species(self._h, int(sp), C.byref(ms), C.byref(n), C.byref(parts)))
        return ms.value, n.value, parts.value

    def profile_read_sorting(self):
        """the launches of advance_p that sorted the species as they pushed it (vpic_hip_step, fixed interval): booked apart"""
        ms, n, parts = C.c_double(), C.c_int64(), C.c_int64()
        self._ck(self._l.vpic_hip_profile_read_sorting(self._h, C.byref(ms), C.byref(n), C.byref(parts)))
        return ms.value, n.value, parts.value
