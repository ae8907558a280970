/* vpic_hip.h -- C ABI of the MI355X-native VPIC inner-loop engine (libvpic_hip.so).
 *
 * Plain C: pointers and sizes only.  Two groups of entry points:
 *
 *  (1) RESIDENT ENGINE (vpic_hip_*): the production path.  All per-step state lives in HBM in
 *      the engine's own layout (cell-sorted SoA particles, SoA Yee fields, AoS interpolator and
 *      accumulator arrays); host arrays in the reference's AoS layouts are mirrors that are
 *      copied in/out on demand at the seams where the reference lets user code look at them
 *      (src/vpic/advance.cxx:67,83-85,123,141,233).  One engine = one rectangular domain = one
 *      GPU.  Each function names the reference function it replaces.
 *
 *  (2) DROP-IN KERNELS (vpic_hip_ref_*, see vpic_hip_dropin.h): the reference's own L3 C
 *      signatures over host AoS arrays (src/species_advance/standard/spa.h:23-123,
 *      src/sf_interface/sf_interface.h:83-163, field_advance_methods_t in
 *      src/field_advance/field_advance.h:185-302), implemented by upload -> HIP kernel ->
 *      download.  Parity tests call through these so they read like calls of the reference.
 *
 * Return convention of group (1): 0 on success, non-zero on error with a message available from
 * vpic_hip_last_error().  Nothing here ever falls back to a CPU implementation: if no HIP device
 * is usable every entry point fails.  Group (2) follows the reference's convention instead
 * (src/util/util_base.h:213-219: message on stderr, exit(1)).
 */
#ifndef VPIC_HIP_H
#define VPIC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
#define VPIC_HIP_STATIC_ASSERT(c, msg) static_assert(c, msg)
extern "C" {
#else
#define VPIC_HIP_STATIC_ASSERT(c, msg) _Static_assert(c, msg)
#endif

/* ---- the reference's host-visible struct layouts (byte for byte) ---------------------------- */

/* src/species_advance/species_advance.h:28-34 */
typedef struct vpic_particle {
  float dx, dy, dz;      /* cell-relative position on [-1,1] */
  int32_t i;             /* voxel, FORTRAN index over (0:nx+1,0:ny+1,0:nz+1) */
  float ux, uy, uz;      /* normalised momentum */
  float q;               /* macro-particle charge */
  int64_t tag, tag2;     /* never touched by the kernels */
} vpic_particle_t;
/* src/species_advance/species_advance.h:39-42 */
typedef struct vpic_particle_mover { float dispx, dispy, dispz; int32_t i; } vpic_particle_mover_t;
/* src/species_advance/species_advance.h:48-55 */
typedef struct vpic_particle_injector {
  float dx, dy, dz; int32_t i; float ux, uy, uz, q; float dispx, dispy, dispz; int32_t sp_id;
} vpic_particle_injector_t;
/* src/sf_interface/sf_interface.h:45-58 */
typedef struct vpic_interpolator {
  float ex, dexdy, dexdz, d2exdydz;
  float ey, deydz, deydx, d2eydzdx;
  float ez, dezdx, dezdy, d2ezdxdy;
  float cbx, dcbxdx, cby, dcbydy, cbz, dcbzdz;
  float _pad[2];
} vpic_interpolator_t;
/* src/sf_interface/sf_interface.h:68-77 */
typedef struct vpic_accumulator { float jx[4], jy[4], jz[4]; } vpic_accumulator_t;
/* src/sf_interface/sf_interface.h:28-38 */
typedef struct vpic_hydro {
  float jx, jy, jz, rho;     /* <q v f>, <q f> */
  float px, py, pz, ke;      /* <p f>, <m c^2 (gamma-1) f> */
  float txx, tyy, tzz;       /* <p_i v_i f> */
  float tyz, tzx, txy;       /* <p_i v_j f> */
  float _pad[2];
} vpic_hydro_t;
/* src/field_advance/field_advance.h:159-171 */
typedef struct vpic_field {
  float ex, ey, ez, div_e_err;
  float cbx, cby, cbz, div_b_err;
  float tcax, tcay, tcaz, rhob;
  float jfx, jfy, jfz, rhof;
  uint16_t ematx, ematy, ematz, nmat;
  uint16_t fmatx, fmaty, fmatz, cmat;
} vpic_field_t;
/* src/field_advance/standard/sfa_private.h:24-32 */
typedef struct vpic_material_coefficient {
  float decayx, drivex, decayy, drivey, decayz, drivez;
  float rmux, rmuy, rmuz, nonconductive, epsx, epsy, epsz, pad[3];
} vpic_material_coefficient_t;

VPIC_HIP_STATIC_ASSERT(sizeof(vpic_particle_t) == 48 && offsetof(vpic_particle_t, i) == 12 &&
                       offsetof(vpic_particle_t, ux) == 16 && offsetof(vpic_particle_t, q) == 28 &&
                       offsetof(vpic_particle_t, tag) == 32 && offsetof(vpic_particle_t, tag2) == 40,
                       "particle_t layout");
VPIC_HIP_STATIC_ASSERT(sizeof(vpic_particle_mover_t) == 16, "particle_mover_t layout");
VPIC_HIP_STATIC_ASSERT(sizeof(vpic_particle_injector_t) == 48, "particle_injector_t layout");
VPIC_HIP_STATIC_ASSERT(sizeof(vpic_interpolator_t) == 80 && offsetof(vpic_interpolator_t, ey) == 16 &&
                       offsetof(vpic_interpolator_t, ez) == 32 && offsetof(vpic_interpolator_t, cbx) == 48 &&
                       offsetof(vpic_interpolator_t, cby) == 56 && offsetof(vpic_interpolator_t, cbz) == 64,
                       "interpolator_t layout");
VPIC_HIP_STATIC_ASSERT(sizeof(vpic_accumulator_t) == 48, "accumulator_t layout");
VPIC_HIP_STATIC_ASSERT(sizeof(vpic_hydro_t) == 64 && offsetof(vpic_hydro_t, txx) == 32, "hydro_t layout");
VPIC_HIP_STATIC_ASSERT(sizeof(vpic_field_t) == 80 && offsetof(vpic_field_t, cbx) == 16 &&
                       offsetof(vpic_field_t, tcax) == 32 && offsetof(vpic_field_t, jfx) == 48 &&
                       offsetof(vpic_field_t, rhof) == 60 && offsetof(vpic_field_t, ematx) == 64 &&
                       offsetof(vpic_field_t, fmatx) == 72 && offsetof(vpic_field_t, cmat) == 78,
                       "field_t layout");
VPIC_HIP_STATIC_ASSERT(sizeof(vpic_material_coefficient_t) == 64, "material_coefficient layout");

/* Boundary codes: src/grid/grid.h:56-69 */
enum { VPIC_PEC_FIELDS = -1, VPIC_SYMMETRIC_FIELDS = -2, VPIC_PMC_FIELDS = -3, VPIC_ABSORB_FIELDS = -4 };
enum { VPIC_REFLECT_PARTICLES = -1, VPIC_ABSORB_PARTICLES = -2 };

/* ---- (1) resident engine ------------------------------------------------------------------- */

/* One rectangular domain.  Replaces what the kernels read from grid_t (src/grid/grid.h:112-167).
 * The 6*nv neighbor[] table is generated from one code per face (order -x,-y,-z,+x,+y,+z, as in
 * neighbor[6v+f], src/grid/ops.c:74-97), exactly what size_grid + join_grid + set_fbc + set_pbc
 * build for box decks:
 *   fbc[f] >= 0: fields on this face are shared with domain fbc[f] (== rank: periodic onto itself)
 *   fbc[f] <  0: local field boundary code (VPIC_PEC_FIELDS ...)
 *   pbc[f] >= 0: particles crossing go to domain pbc[f] (== rank: wrap locally)
 *   pbc[f] <  0: VPIC_REFLECT_PARTICLES / VPIC_ABSORB_PARTICLES                              */
typedef struct vpic_hip_grid {
  float dt, cvac, eps0, damp;
  float dx, dy, dz, rdx, rdy, rdz;
  int32_t nx, ny, nz;
  int32_t fbc[6], pbc[6];
  int32_t rank;
} vpic_hip_grid_t;

typedef struct vpic_hip_engine vpic_hip_engine_t;

const char *vpic_hip_last_error(void);
/* A caller whose host arrays are demand-paged (protected while the engine owns the data) registers a function that
 * makes [p, p+bytes) resident -- and writable when for_write -- : every entry point given a host array calls it before a
 * HIP copy touches the range (a copy engine that meets a protected page faults the GPU instead of raising SIGSEGV). */
typedef void (*vpic_hip_host_access_fn)(const void *p, size_t bytes, int for_write);
void vpic_hip_set_host_access_hook(vpic_hip_host_access_fn fn);
int  vpic_hip_device_count(void);
/* device < 0: use the current HIP device */
int  vpic_hip_create(vpic_hip_engine_t **e, const vpic_hip_grid_t *g, int device);
void vpic_hip_destroy(vpic_hip_engine_t *e);
int  vpic_hip_sync(vpic_hip_engine_t *e);
void *vpic_hip_stream(vpic_hip_engine_t *e);                 /* hipStream_t the kernels run on */
int  vpic_hip_nv(const vpic_hip_engine_t *e);                /* (nx+2)(ny+2)(nz+2) */

/* host AoS mirrors <-> device (new_field / new_interpolator / new_accumulators arrays of the
 * reference, src/sf_interface/sf_interface.c:13-83, src/field_advance/standard/sfa.c:56-73) */
int vpic_hip_set_fields(vpic_hip_engine_t *e, const vpic_field_t *f);            /* nv entries */
int vpic_hip_get_fields(vpic_hip_engine_t *e, vpic_field_t *f);
int vpic_hip_set_interpolator(vpic_hip_engine_t *e, const vpic_interpolator_t *fi);
int vpic_hip_get_interpolator(vpic_hip_engine_t *e, vpic_interpolator_t *fi);
int vpic_hip_set_accumulator(vpic_hip_engine_t *e, const vpic_accumulator_t *a);
int vpic_hip_get_accumulator(vpic_hip_engine_t *e, vpic_accumulator_t *a);
/* new_material_coefficients (src/field_advance/standard/sfa.c:80-177): table of n materials */
int vpic_hip_set_material_coefficients(vpic_hip_engine_t *e, const vpic_material_coefficient_t *m, int n);

/* species (new_species, src/species_advance/species_advance.c:21-63).  Returns the id >= 0. */
int vpic_hip_species_create(vpic_hip_engine_t *e, float q_m, int64_t max_np, int64_t max_nm);
int vpic_hip_species_set_particles(vpic_hip_engine_t *e, int sp, const vpic_particle_t *p, int64_t np);
/* One emission step of a surface emitter (src/emitter/child-langmuir.c:43-97, ccube.c, ivory.c; advance.cxx:83-84):
 * components[k] = (local voxel << 5) | BOUNDARY code of the emitting face (emitter.h:12-16).  A face whose normal
 * field pulls the species out and reaches thresh_e_norm emits n_emit_per_face particles sharing the charge
 * eps0 dY dZ dt sqrt(coef |q_m E^3| / dX) -- coef 32/81 (child_langmuir), 1 (ccube), 1/6 (ivory) -- with the
 * models' momentum and age distributions; their charge, negated, goes to rhob; they are moved for the rest of
 * the step.  Random numbers from the device's counter-based stream (seed, call). */
int vpic_hip_emit(vpic_hip_engine_t *e, int sp, const int32_t *components, int n, int n_emit_per_face,
                  float ut_perp, float ut_para, float coef, float thresh_e_norm, uint32_t seed);
/* inject_particle with an age (src/vpic/misc.cxx:93-103): n injector records in HOST memory -- position, voxel,
 * momentum, charge, the displacement still to be travelled, species -- are appended to their species and moved
 * (deposits go to the accumulator, a particle stopped by a face becomes a mover); tags: 2 per record or NULL */
int vpic_hip_inject_aged(vpic_hip_engine_t *e, const vpic_particle_injector_t *inj, const int64_t *tags, int n);
/* accumulate_rhob (boundary_p.c:9-71) for n particles handed over in host memory: q_scale * q of each is spread
 * over the 8 nodes of its cell and added to rhob (inject_particle with update_rhob passes -1, misc.cxx:87-91) */
int vpic_hip_accumulate_rhob(vpic_hip_engine_t *e, const vpic_particle_t *p, int64_t n, float q_scale);
/* A custom particle boundary handler of the maxwellian_reflux kind (src/boundary/maxwellian_reflux.c:47-175) for
 * the faces whose particle code is `code` (<= -3: what add_boundary returns, grid.h:68-69): a particle that hits
 * such a face comes back at once with a momentum drawn from the flux of a Maxwellian at the wall -- normal
 * component sqrt(2) ut_para sqrt(-log U), tangential ones ut_perp N(0,1), per species -- and moves on for the
 * rest of its step.  Random numbers come from a counter-based generator on the device (seed, call, species,
 * mover): statistically the reference's handler, not its stream; its uniforms lie strictly inside (0, 1)
 * (csrc/unit_draw.h), so the normal component is never exactly zero.  The faces a mover sits on are tried in the order
 * -x -y -z +x +y +z; a face whose code has no parameters claims nothing and the next face is tried, and a mover that
 * no face took is absorbed into rhob (boundary_p.c:268-277, :312-316).  Up to 4 codes; the same code again replaces
 * its parameters.  A code that is a wall (vpic_hip_set_wall, below) is refused. */
int vpic_hip_set_maxwellian_reflux(vpic_hip_engine_t *e, int code, const float *ut_para, const float *ut_perp, int n_species, uint32_t seed);
/* Parity tests: the three numbers the handler draws per refluxed particle (mt_frand, mt_frandn, mt_frandn:
 * maxwellian_reflux.c:120-122) from a table indexed by the particle's position in its species' array (3 floats each)
 * instead of the engine's counter-based generator; n_particles = 0 switches back.  The arithmetic in this mode, float
 * throughout, one rounding per operation (no contraction), d = the three draws of the particle's slot, h the handler:
 *   u0 = (ut_para[h] * (+-sqrt2f)) * sqrtf(-logf(d[0]))     (- on the faces +x +y +z; sqrt2f the float nearest sqrt 2)
 *   u1 = ut_perp[h] * d[1],  u2 = ut_perp[h] * d[2]          (u0 along the face's axis, u1 and u2 on the next two, cyclically)
 *   dd = (g.dx * dispx, g.dy * dispy, g.dz * dispz),  r = (ux ux + uy uy) + uz uz of the OLD momentum
 *   ratio = sqrtf(((1 + r) * ((ddx ddx + ddy ddy) + ddz ddz)) / ((1 + ((nux nux + nuy nuy) + nuz nuz)) * (FLT_MIN + r)))
 *   new displacement = ((nux * ratio) * rdx, (nuy * ratio) * rdy, (nuz * ratio) * rdz); position, cell and charge are kept,
 * and the injector finishes its move like an arrival (no tags).  Only logf is not correctly rounded: given u0, every
 * other number is the same on any IEEE machine (oracle/vpic_oracle.h: orc_maxwellian_reflux_from_u). */
int vpic_hip_set_reflux_draws(vpic_hip_engine_t *e, const float *draws, int64_t n_particles);
/* ABSORBING WALLS THAT TALLY AND RECORD what they take (the reference's absorb_tally and link_boundary handlers,
 * src/boundary/absorb_tally.c and link.c, and the same for the plain absorbing faces).
 * A WALL is a particle boundary code registered with vpic_hip_set_wall: VPIC_ABSORB_PARTICLES itself (the plain absorbing
 * faces are tallied) or a code <= -3 (what add_boundary returns).  At most 4 codes are walls, and a code is never a wall
 * and a maxwellian_reflux handler at once.
 * Who is absorbed where.  Every mover is looked at once per round (vpic_hip_boundary_p_pack, vpic_hip_exchange_pack*), the
 * faces f = 0..5 (-x -y -z +x +y +z) in turn.  Face f is MET when the stored position component on its axis is exactly -1
 * (f < 3) or +1 (f >= 3) and the momentum component on that axis is < 0 or > 0 respectively (boundary_p.c:304-309).  At the
 * first met face whose code is a wall or VPIC_ABSORB_PARTICLES the mover is absorbed AT THAT FACE.  Every other code behaves
 * as without walls: a face shared with another domain sends, a registered reflux code refluxes, and a reflecting face, a
 * face of this same domain or a code <= -3 registered nowhere pass the mover on to the next face.  A mover that no face took
 * is absorbed at face 6, "none".  Absorption itself is what it is without walls: accumulate_rhob, then removal (on the
 * device-resident exchange: a dead slot).
 * Tallies.  One table [7][n_species] of vpic_hip_wall_tally_t.  Row f < 6 takes the particles absorbed at face f when that
 * face's code is a wall; row 6 takes EVERY OTHER particle absorbed while at least one wall is registered (plain absorbing
 * faces that are not registered, and face "none"): the rows together account for every absorption.  Per absorbed particle,
 * in IEEE double, every operation rounded once and unfused:
 *   count += 1
 *   val0 = (double)q
 *   val1 = (double)q * ke,   ke = sqrt(((1 + ux ux) + uy uy) + uz uz) - 1    (VPIC_HIP_COORD_KE's expression)
 *   for k = 0, 1:  t = val_k / quantum_k;  fabs(t) < 4294967296.0 ?  isum[k] += llrint(t)  :  refused[k] += 1
 * (a NaN is refused; a refused particle is still counted and still absorbed) -- the rule of
 * vpic_hip_species_distribution_sums word for word.  The sums are integers: the same bits in any mover order, on either
 * exchange path, and additive across domains.  The caller reads and clears them; nothing else does.  |llrint(t)| < 2^32,
 * so a table left running for more than 2^31 absorptions in one row can wrap its 64-bit sums.
 * Records.  One device buffer of record_cap vpic_hip_wall_record_t.  A particle absorbed at a face whose wall was
 * registered with VPIC_HIP_WALL_RECORD is appended as it is stored at that moment (offsets, voxel, momenta, charge), with
 * its two tags (0 for a species without tags), the face and the species index.  A record that does not fit is dropped and
 * counted in `dropped`; the tally still takes the particle, and nothing is written past the buffer.  Records of an earlier
 * call precede those of a later one; the order within a call is unspecified. */
typedef struct vpic_hip_wall_tally { int64_t count; int64_t isum[2]; int64_t refused[2]; } vpic_hip_wall_tally_t;
typedef struct vpic_hip_wall_record { float dx, dy, dz; int32_t i; float ux, uy, uz, q; int64_t tag, tag2; int32_t face, sp; } vpic_hip_wall_record_t;
VPIC_HIP_STATIC_ASSERT(sizeof(vpic_hip_wall_tally_t) == 40, "a wall tally is five 64-bit words");
VPIC_HIP_STATIC_ASSERT(sizeof(vpic_hip_wall_record_t) == 56, "a wall record is 56 bytes");
enum { VPIC_HIP_WALL_TALLY = 1, VPIC_HIP_WALL_RECORD = 2 };
enum { VPIC_HIP_WALL_ROWS = 7, VPIC_HIP_WALL_MAX = 4 };
/* (Re)allocates the tally table and the record buffer and zeroes both (the registered walls stay).  quantum_q and
 * quantum_qke: the quanta of isum[0] and isum[1], positive and finite; record_cap >= 0, 0: no record buffer. */
int vpic_hip_wall_setup(vpic_hip_engine_t *e, double quantum_q, double quantum_qke, int64_t record_cap);
/* Makes `code` a wall (flags: VPIC_HIP_WALL_TALLY, VPIC_HIP_WALL_RECORD, which implies TALLY), replaces the flags of a
 * code that already is one, or with flags 0 unregisters it.  Refused: a code that is not VPIC_ABSORB_PARTICLES or <= -3,
 * a code that is a maxwellian_reflux handler, a fifth code, unknown flag bits, a call before vpic_hip_wall_setup. */
int vpic_hip_set_wall(vpic_hip_engine_t *e, int code, int flags);
/* out[7 * n_species], as out[row * n_species + sp]; n_species >= the engine's species count (the columns beyond it are
 * zero).  clear != 0: the table restarts at zero. */
int vpic_hip_wall_tally(vpic_hip_engine_t *e, vpic_hip_wall_tally_t *out, int n_species, int clear);
/* Copies up to `cap` records in buffer order into out (may be NULL when cap is 0); *n: how many were copied, *dropped:
 * how many did not fit into the device buffer since it was last cleared.  clear != 0: the cursor and `dropped` restart. */
int vpic_hip_wall_records(vpic_hip_engine_t *e, vpic_hip_wall_record_t *out, int64_t cap, int64_t *n, int64_t *dropped, int clear);
/* The same for vpic_hip_emit: six numbers per emitted-particle slot (slot = component index * n_emit_per_face + k), in
 * the model's draw order (child-langmuir.c:60-75: mt_drand_c, mt_drand_c, mt_drandn x 3, mt_drand_c0).
 * The arithmetic of a slot in this mode, d[0..5] its six double draws; X the face's axis, Y and Z the next two cyclically;
 * dir = +1 on the faces -x -y -z (emission towards +X), -1 on +x +y +z; every operation rounded once, no contraction:
 *   the face emits when (float) q_m * (dir * E_X) > 0 and |E_X| >= thresh_e_norm, E_X the interpolator's ex / ey / ez of the voxel
 *   position on the face and momenta, from the double draws with ONE rounding each (as the reference has them):
 *     pos_X = -dir, pos_Y = (float)(2 d[0] - 1), pos_Z = (float)(2 d[1] - 1)
 *     u_X = (float)(dir * |(double)ut_para * d[2]|), u_Y = (float)((double)ut_perp * d[3]), u_Z = (float)((double)ut_perp * d[4])
 *   the charge, in float with sqrtf, left to right:
 *     q = ((((eps0 * d_Y) * d_Z) * dt) * sqrtf((coef * |((q_m * E_X) * E_X) * E_X|) / d_X)) / (float)n_emit_per_face, negated for q_m < 0
 *   the age, in float:  age = (float)d[5];  age *= (cvac * dt) / sqrtf(((ux ux + uy uy) + uz uz) + 1)      (x, y, z order)
 *   the displacements:  disp_k = (u_k * age) * rd_k,  k = x, y, z
 *   rhob receives accumulate_rhob (boundary_p.c:9-71) of the position on the face with charge -q: w0 = (float)(0.125 *
 *   (double)(-q) * (double)rdx * (double)rdy * (double)rdz) -- one double product, rounded once -- and the trilinear weights
 *   from it in float, doubled on the domain's surface planes, added to the 8 nodes with float atomics (any order).
 * The injector then finishes its move like an arrival.  The reference differs in the last bits of q and disp: it takes the
 * root of the charge law and the age in double and divides by the cell size (DESIGN.md section 4 bounds the difference). */
int vpic_hip_set_emit_draws(vpic_hip_engine_t *e, const double *draws, int64_t n_slots);
/* n more particles at the end of the list (particles a deck injects while the run is under way,
 * vpic.hxx:463-486); pending movers keep their particle indices */
int vpic_hip_species_append_particles(vpic_hip_engine_t *e, int sp, const vpic_particle_t *p, int64_t n);
int vpic_hip_species_get_particles(vpic_hip_engine_t *e, int sp, vpic_particle_t *p, int64_t cap);
int vpic_hip_species_get_particles_range(vpic_hip_engine_t *e, int sp, vpic_particle_t *p, int64_t from, int64_t count);   /* particles [from, from+count) */
/* How advance_p covers a species of np particles when its workgroups take 256*iters particles each: launches of at most
 * 2^30 particles (32-bit byte offsets inside a launch) that start on workgroup boundaries.  Pure host arithmetic;
 * returns the number of segments (< 0: bad arguments). */
int vpic_hip_push_plan(int64_t np, int iters, int64_t *start, int32_t *count, uint32_t *grid, int max_segments);
/* Synthetic loader for benchmark-sized species: ppc particles in every interior cell, uniform in
 * the cell, drifting Maxwellian momenta -- what a deck's `repeat(N) inject_particle(...)` loop does
 * (src/vpic/vpic.hxx:491-505), on the device with a counter-based generator.  The loaded particles carry tag = tag2 = 0,
 * whatever tags the species held before. */
int vpic_hip_species_load_maxwellian(vpic_hip_engine_t *e, int sp, int ppc, uint32_t seed, float q,
                                     float ux, float uy, float uz, float vth);
/* A species loaded on the device from per-cell tables, the same particles for any decomposition of the global grid.
 * (The synthetic loader above keys its draws with a 32-bit particle index times 9, so its streams repeat from 477 M
 * particles of a species on; it stays as it is because the benchmark and the tests that pin its draws rest on it.)
 *
 * Tables are HOST arrays of tdim[0] * tdim[1] * tdim[2] entries, x fastest; every tdim entry is 1 (the table does not vary
 * along that axis) or the grid's extent; all tables of a call share tdim and are uploaded as given.  A NULL ud / uth
 * table reads 0.  count[] macro-particles go into each cell, each of charge q[]; ud is the cell's drift as gamma_d beta_d,
 * uth the spread of the momentum u = gamma beta in the drift's rest frame.
 *
 * THE RULE (old-vpic_amd/csrc/load_rule.h; tests/load_ref.py restates it in numpy):
 *   Generator, Philox-4x32-10: M0 = 0xD2511F53, M1 = 0xCD9E8D57, W0 = 0x9E3779B9, W1 = 0xBB67AE85.  One round on counter
 *   (c0,c1,c2,c3) and key (k0,k1): p0 = M0 * c0, p1 = M1 * c2 as 64-bit products; the new counter is
 *   (hi(p1) ^ c1 ^ k0, lo(p1), hi(p0) ^ c3 ^ k1, lo(p0)).  Ten rounds; before each of rounds 2 to 10, k0 += W0 and k1 += W1
 *   in uint32 arithmetic.  (Counter 0, key 0 gives 6627e8d5 e169c58d bc57ac4c 9b00dbd8.)
 *   Keys and counters: the key is (seed, stream).  A particle is named by its global cell c = gx + GX * (gy + GY * gz)
 *   (global cell coordinates from 0, c 64-bit: g = goff + local cell) and its number j within the cell for this call, from
 *   0.  Block b (0 or 1) is philox((lo32(c), hi32(c), j, b), key); the words r0..r3 (block 0) and r4..r7 (block 1) are the
 *   particle's draws.  Rank, array order and launch shape do not enter.
 *   From draws to numbers (unit_open: ((float)(r >> 8) + 0.5f) * 2^-24, at most 1 - 2^-24):  x_k = unit_open(r_k), k = 0, 1, 2;
 *   n0 = R1 cos(2 pi unit_open(r4)), n1 = R1 sin(2 pi unit_open(r4)) with R1 = sqrt(-2 log unit_open(r3));
 *   n2 = sqrt(-2 log unit_open(r5)) cos(2 pi unit_open(r6));  U = unit_open(r7).  The normals use the device's own float
 *   log, cos and sin and are specified statistically, as the draws of vpic_hip_collide are; x_k and U are exact.  With
 *   vpic_hip_set_load_draws (parity tests) the seven floats (x0, x1, x2, n0, n1, n2, U) are read from draws[7 m .. 7 m + 6],
 *   m the particle's place within the call's load (below).
 *   From numbers to the particle, every operation rounded once, uncontracted, parentheses as written:
 *     dx = 2.f * x0 - 1.f, dy and dz likewise (strictly inside (-1, 1)); voxel i = (cx+1) + sy (cy+1) + sz (cz+1); q the
 *     cell's table value.  Momentum in IEEE double from the float tables, / and sqrt correctly rounded:
 *       w_k = (double)uth_k[cell] * (double)n_k;   gw = sqrt(1 + ((w0 w0 + w1 w1) + w2 w2))
 *       D_k = (double)ud_k[cell];                   D2 = (D0 D0 + D1 D1) + D2 D2
 *       if D2 == 0: u_k = w_k.  Otherwise:
 *         gd = sqrt(1 + D2);  wD = (w0 D0 + w1 D1) + w2 D2
 *         with VPIC_HIP_LOAD_FLIP, if (-wD) / (gd * gw) > (double)U:  t = (2 * wD) / D2;  w_k = w_k - t * D_k;  wD = -wD
 *           (Zenitani's flipping method, Phys. Plasmas 22, 042116 (2015): the boosted population has the right density in
 *           the lab frame; a no-op in the non-relativistic limit)
 *         f = ((gd - 1) * wD) / D2 + gw;   u_k = w_k + f * D_k
 *       ux, uy, uz = (float)u_0, (float)u_1, (float)u_2
 *     Tags with VPIC_HIP_LOAD_TAGS: tag = tag0 + m, tag2 = 0; otherwise the new particles' tags read 0.
 *   Order: the call's particles are ordered by ascending voxel, and by ascending j within a cell: m = offset[cell] + j,
 *   offset the exclusive sum of the counts in that order.
 *
 * Without VPIC_HIP_LOAD_APPEND the call replaces the species and leaves it as a by-voxel sort_p does: the array in voxel
 * order, partition[] written (ghost voxels as empty ranges), vpic_hip_species_sort_order 1.  With it the particles go
 * behind the species' extent, booked as vpic_hip_species_append_particles books them (several populations in one species).
 * q_max rises to the largest |q| of a cell with a non-zero count; the species is chargeless when every such q is 0 (and, with
 * APPEND, it was before); has_tags follows the TAGS flag (with APPEND, a species that had tags keeps them).
 * Refused with nothing touched (vpic_hip_last_error names the argument): a NULL d, count or q; an unknown sp; a tdim
 * entry neither 1 nor the grid's extent; goff < 0 or goff + n > gdim; a negative count; a non-finite q, ud or uth; a
 * negative uth; unknown flag bits; a total above 2^31 - 1 or beyond the free capacity; a draws table shorter than the
 * total; a species with pending movers.  *n_loaded (may be NULL): the particles the call added. */
#define VPIC_HIP_LOAD_APPEND 1
#define VPIC_HIP_LOAD_FLIP 2
#define VPIC_HIP_LOAD_TAGS 4
typedef struct {
  const int32_t *count;        /* macro-particles per cell, >= 0 */
  const float *q;              /* charge of each macro-particle of the cell */
  const float *ud[3], *uth[3]; /* drift gamma beta and thermal spread of u, by x y z; a NULL table reads 0 */
  int32_t tdim[3];             /* extents of EVERY table along x, y, z: each 1 (broadcast) or the grid's n; x fastest */
  int64_t gdim[3], goff[3];    /* the global grid and this domain's first cell in it */
  uint32_t seed, stream; int32_t flags; int64_t tag0;
} vpic_hip_load_t;
VPIC_HIP_STATIC_ASSERT(sizeof(vpic_hip_load_t) == 152, "vpic_hip_load_t layout");
int vpic_hip_species_load_profile(vpic_hip_engine_t *e, int sp, const vpic_hip_load_t *d, int64_t *n_loaded);
/* parity mode of the call above: seven floats per particle place m replace the generator's numbers; n = 0 switches back */
int vpic_hip_set_load_draws(vpic_hip_engine_t *e, const float *draws, int64_t n);
int64_t vpic_hip_species_np(vpic_hip_engine_t *e, int sp);               /* live particles */
/* extent = array slots in use (live particles + the dead slots the device-resident exchange leaves until the next sort),
 * and the capacities; _reserve enlarges them between steps (boundary_p.c:416-448 grows by 1.3125 when it runs out) */
int vpic_hip_species_capacity(vpic_hip_engine_t *e, int sp, int64_t *extent, int64_t *max_np, int64_t *max_nm);
int vpic_hip_species_reserve(vpic_hip_engine_t *e, int sp, int64_t max_np, int64_t max_nm);
int64_t vpic_hip_species_nm(vpic_hip_engine_t *e, int sp);
/* movers left by the last advance_p, ascending in particle index (src/species_advance/standard/
 * boundary_p.c:168-176 requires that order) */
int vpic_hip_species_get_movers(vpic_hip_engine_t *e, int sp, vpic_particle_mover_t *pm, int64_t cap);
/* hand a mover list to the engine (what a caller of boundary_p holds in sp->pm / sp->nm) */
int vpic_hip_species_set_movers(vpic_hip_engine_t *e, int sp, const vpic_particle_mover_t *pm, int64_t nm);
/* partition[nv+1] as sort_p leaves it (src/species_advance/standard/sort_p.c:48-58) */
int vpic_hip_species_get_partition(vpic_hip_engine_t *e, int sp, int32_t *partition);
/* the same for the engine's own order (vpic_hip_set_sort_order(e, 1), by 4x4x4-cell tile, cell by cell within a tile): where
 * every cell of every tile began at the species' last sort, tpart[64 * tiles + 1] with tiles = ceil(nx/4) ceil(ny/4) ceil(nz/4),
 * key = 64 * tile + (z & 3) << 4 | (y & 3) << 2 | (x & 3) of the cell (x - 1, y - 1, z - 1).  *count: entries written (call
 * with tpart = NULL to learn it).  Valid while vpic_hip_species_sort_order says 2; a species sorted by tile only has its
 * tiles' first entries right and nothing to say about the cells inside. */
int vpic_hip_species_get_tile_partition(vpic_hip_engine_t *e, int sp, int32_t *tpart, int64_t *count);

/* kernels, named after the reference functions they replace */
int vpic_hip_load_interpolator(vpic_hip_engine_t *e);       /* sf_interface/load_interpolator.cxx:284-369 */
int vpic_hip_clear_accumulators(vpic_hip_engine_t *e);      /* sf_interface/clear_accumulators.c:26-49 */
int vpic_hip_reduce_accumulators(vpic_hip_engine_t *e);     /* sf_interface/reduce_accumulators.cxx:143-165: one accumulator here, nothing to reduce */
int vpic_hip_unload_accumulator(vpic_hip_engine_t *e);      /* sf_interface/unload_accumulator.cxx:81-121 */
/* Arithmetic of advance_p.  EXACT (default): the reference's scalar pipeline, operation for operation
 * (advance_p.cxx:68-177 compiled without contraction, true divides and sqrtf): every particle bit-identical.
 * FAST: contracted multiply-adds and 1-ulp v_rsq_f32 / v_rcp_f32 instead of the correctly rounded sequences --
 * what the reference's own V4 pipelines do with rsqrt / rcp estimates (src/util/v4/v4_sse.hxx:914-939, selected
 * by its shipped machine configs); momenta within 8 ulp of the scalar pipeline per step. */
#define VPIC_HIP_PUSH_EXACT 0
#define VPIC_HIP_PUSH_FAST  1
int vpic_hip_set_push_mode(vpic_hip_engine_t *e, int mode);
/* How deposits are summed.  0 (default): float sums (LDS and global float atomics): accumulators agree with the reference's
 * to 2e-6 of the largest entry and differ from run to run at the 1e-7 level (the order of the additions is the machine's).
 * 1: DETERMINISTIC -- every deposit is rounded to 64-bit fixed point (scale 2^k chosen from q_ref, the |charge| of a typical
 * macro-particle; <= 0: the largest charge the host has put into a species so far) and summed as an integer in LDS and in
 * HBM, so accumulators, jf, rhof and everything downstream are bit-identical from run to run whatever the array order,
 * the scheduling or the order messages arrive in.  The reference is reproducible by construction (private accumulators
 * reduced in a fixed order, sf_interface/reduce_accumulators.cxx:37-55); this mode is how the engine gets there.  Particle
 * results are the same in both modes.
 * THE RULE of the push's deposits, a contract (tests/test_gpu_det_exact.py holds every word of the accumulator to it, on
 * every instance of advance_p and on the injection path; oracle/vpic_oracle.h, orc_set_fixed_accumulator, and pyorc.fixed_scale
 * / finalize are its CPU restatement, pinned on the compiled reference by tests/test_det_ref.py):
 *   - the scale is the power of two  scale = 2^(37 - ex),  4.2 q = m 2^ex with 0.5 <= m < 1 (frexp),  where q is q_ref when
 *     q_ref > 0 and otherwise the largest |q| that has gone into any species so far (set / appended / injected particles, and
 *     arrivals from other domains once _exchange_finish has booked them) at the moment the first deterministic kernel after this
 *     call adds; it then stays until the next vpic_hip_set_accumulation.  A domain that knows no charge at all when the first
 *     message arrives takes the largest finite |q| of that message's records (one extra read-back, once);
 *   - each of the 12 floats v of each straight streak -- formed operation by operation as the reference's scalar code forms them
 *     (advance_p.cxx:131-162 for a particle that stays in its cell, move_p.c:76-100 for every segment of one that does not,
 *     its v5 with the last multiply in double), uncontracted, in either push mode -- becomes the integer rint(v * scale),
 *     to nearest even (v * scale is exact in double), and is added to the 64-bit word of its voxel and component;
 *   - reading the accumulator (or unloading it) rounds each word once, float((double)word * (1 / scale)), and ADDS it to the
 *     float accumulator, which clear_accumulators zeroes: a word whose sum is zero leaves +0.0 there.  (int64 -> double rounds
 *     above 2^53: two roundings there.)
 *   Which instance pushes a species, the order of its array, the windows, the tail, stale tiles: none of them changes a word.
 *   Range: |v * scale| < 2^51 per deposit (the largest deposit a macro-particle makes, 4.2 |q|, stays below it up to
 *   |q| = 2^14 q_ref) and at most 2^26 deposits of the reference size per word; beyond it the conversion wraps silently.
 *   No lower limit: charges far below q_ref lose resolution (a quantum is 2^-37 of 4.2 q_ref), nothing else.
 * The hydro moments join the guarantee: accumulate_hydro_p sums every one of a particle's 8 x 14 contributions as a 64-bit
 * fixed-point integer too (one power-of-two scale per moment and call, from the species' largest macro-particle charge, its
 * q_m, the cell volume and c: policy.h, moment_scales) and rounds each sum once into the float array, so two runs write the
 * same hydro dumps bit for bit, whatever order the arrays are in and whichever path summed them; species are added in the
 * caller's order.  The fixed-point words take 14 x 8 bytes per voxel (1.9 GB at 256^3), allocated by the first
 * deterministic accumulate_hydro_p and freed with the engine.  A species in tile order is summed tile by tile in LDS without
 * being reordered; one that the engine would push in tile order is sorted by tile first, as before a deterministic push; any
 * other species (and every one under VPIC_HIP_MOMENTS_TILED=0) is summed with one global 64-bit atomic per contribution,
 * which is slow and correct.
 * THE RULE of the moments, a contract (tests/test_gpu_moments_exact.py holds every word of the hydro array and of rhof to
 * it; oracle/vpic_oracle.h, orc_set_fixed_moments, and pyorc.finalize_moments are its CPU restatement):
 *   - each of the 8 x 14 floats c a particle adds (hydro_p.c:133-158, operation by operation, uncontracted) becomes the
 *     integer rint(c * scale_m), to nearest even; the 14 scales are those of policy.h: moment_scales for the LARGEST |q|
 *     that has ever gone into the species -- set, appended, injected, loaded, emitted, or ARRIVED from another domain
 *     (_exchange_inject, booked by _exchange_finish; _boundary_p_inject: tests/test_gpu_exchange.py) -- also after that
 *     particle has left (absorbed, sent away), so a species keeps its scales for the run; a species that never received a charge takes
 *     q_ref; a selection (accumulate_hydro_p_select) takes the whole species' scales;
 *   - accumulate_rho_p does the same with the 8 weights (rho_p.c:43-84) at the scale of the push's deposits moved by a
 *     power of two: scale 2^-ex, 8 r8V = m 2^ex (frexp), r8V the float 1 / (8 dV);
 *   - every call rounds each non-zero sum once, float((double)sum * (1 / scale)), and ADDS it in float to what the array
 *     holds; a word whose sum is zero is left as it is.  So species added one after the other round once each.
 * Limits of the guarantee: rhob (the charge absorbing faces and emitters leave behind, which div-E cleaning reads) is summed
 * with float atomics in both modes; a single deposit beyond 2^14 x 4.2 q_ref (|x * scale| >= 2^51) wraps in the fixed-point
 * conversion -- give q_ref the LARGEST macro-particle charge of the run when charges differ by orders of magnitude.  The
 * hydro moments convert for every particle with |u| <= 2^12 (2^20 particles of the largest charge at |u| <= 2^7 fit one
 * sum); a contribution that does not convert (|u| of the order of 2^12 and above: 2^15 for the largest charge) is counted
 * and never wraps: accumulate_hydro_p then adds nothing, clears its fixed-point words and fails with an error that names the
 * range (vpic_hip_moments_stats: out[3]).  Float mode has no such limit. */
int vpic_hip_set_accumulation(vpic_hip_engine_t *e, int mode, double q_ref);
int vpic_hip_advance_p(vpic_hip_engine_t *e, int sp);       /* species_advance/standard/advance_p.cxx:399-472 (+move_p.c); movers: vpic_hip_species_nm */
/* A mover names its particle by array index, so no call reorders a species while movers of it are pending (_species_nm > 0, or
 * between the two phases of its push): vpic_hip_sort_p -- and every call that would have to sort, such as _species_get_particles
 * of a species with dead slots -- fails and leaves the species, its movers and its books as they were, the ordering
 * _exchange_begin does before a deterministic push passes such a species by, and a call that pushes (_advance_p,
 * _sort_advance_p, _step) begins a new mover list, so it drops what is left of the old one before it orders the species. */
int vpic_hip_sort_p(vpic_hip_engine_t *e, int sp);
/* sort_p followed by advance_p of the same species, as ONE call: when the sort is by tile and cell and finds the counts the
 * push before it took (vpic_hip_species_sort_hint), the push writes every particle straight to its sorted place in the
 * second buffer instead of sorting first (the order is that of the cells before this push: sort_p.c:48-101 applied one step
 * earlier) -- where that is the cheaper way for this species: the engine times both ways (a species whose particles have spread
 * between sorts is better sorted first) and keeps to the cheaper one; the particles and the order are the same either way.
 * Otherwise exactly vpic_hip_sort_p + vpic_hip_advance_p.  vpic_hip_step does the same by itself. */
int vpic_hip_sort_advance_p(vpic_hip_engine_t *e, int sp);
/* the species' next advance_p also takes the histogram of the sort that follows it (the caller knows the next step sorts;
 * vpic_hip_step does this by itself): that sort then starts at its scan.  Anything that changes the species in between
 * makes the sort count for itself again. */
int vpic_hip_species_sort_hint(vpic_hip_engine_t *e, int sp);          /* species_advance/standard/sort_p.c:16-102 */
int vpic_hip_energy_p(vpic_hip_engine_t *e, int sp, double *energy); /* species_advance/standard/energy_p.cxx:124-157 (local part) */

/* ---- binary Coulomb collisions of the particles of one species, or of two, cell by cell (csrc/collide.hip) ----
 * The device counterpart of a deck's user_particle_collisions (src/vpic/advance.cxx:41-67: between the sort and the push).
 * The reference ships the hook and no operator; this is the operator of Takizuka & Abe (J. Comput. Phys. 25, 205, 1977):
 * the particles of a cell are paired at random and every pair is turned in its centre-of-mass frame by a random small
 * angle.  It is NON-RELATIVISTIC in u (u is taken for the velocity in units of c: valid for |u| << 1; there is no Lorentz
 * factor anywhere), rank-local (a cell's particles are all on this rank), and its result depends on the order of the array
 * within a cell (the pairing is by position in the cell's range): statistically the same in any order, bit for bit only
 * for the same array.  The relativistic (Perez) form of the pair is vpic_hip_collide_relativistic, below.
 * THE RULE, a contract (tests/collide_ref.py restates it in numpy; tests/test_gpu_collide.py holds every word to it):
 *   mix32(x):  x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16   (uint32, a bijection)
 *   Cells are the interior voxels v = x + (nx+2) * (y + (ny+2) * z), 1 <= x <= nx ...; the particles of species s in cell v
 *   are a contiguous range of its array (see "exact ranges" below), k = 0 .. n_s - 1 the position inside the range.
 *   c0_s = mix32((seed ^ mix32(call * 0x9e3779b9 + s)) + mix32(rank * 0x85ebca6b + v))    (uint32 arithmetic; s the species
 *          id, rank the grid's, v the VOXEL in either array order)
 *   key_s(k) = mix32(c0_s + k): no two keys of a range tie.  perm_s[r] = the k whose key is the r-th smallest.
 *   Pairs of ONE species (sp_a == sp_b), n particles in the cell, N = n:
 *     n < 2: none.  n even: pair j = (perm[2j], perm[2j+1]), j = 0 .. n/2 - 1.
 *     n odd: with p0, p1, p2 = perm[0], perm[1], perm[2]: pairs 0, 1, 2 = (p0,p1), (p1,p2), (p2,p0), applied in that order,
 *       each with s2 halved; then pair 3 + m = (perm[3 + 2m], perm[4 + 2m]), m = 0 .. (n-3)/2 - 1.
 *   Pairs of TWO species: L is the species with more particles in the cell (sp_a on a tie), S the other; n_S == 0: none.
 *     pair j = (L[perm_L[j]], S[perm_S[j mod n_S]]), j = 0 .. n_L - 1; pairs that share their S particle are applied in
 *     ascending j.  N = min(n_a, n_b).
 *   The first-named particle of a pair is its FIRST particle; no particle is the first one of two pairs.
 *   Per pair (first f, second s), IEEE float, every operation rounded once, unfused, / and sqrt correctly rounded, the
 *   parentheses as written:
 *     w = fabsf(q) * wq of its species (the number of physical particles a macro-particle stands for)
 *     gx = ux_f - ux_s, gy, gz likewise;  gq = gx*gx + gy*gy;  g2 = gq + gz*gz;  gm = sqrt(g2);  gp = sqrt(gq)
 *     gm == 0: the pair is skipped (and counted); otherwise
 *     m_ab = (m_a * m_b) / (m_a + m_b);  V = (dx * dy) * dz of the grid
 *     s2 = (((cvar * max(w_f, w_s)) * (float)N) * dt) / (((V * m_ab) * m_ab) * ((gm * gm) * gm));  in the triple s2 = 0.5f * s2
 *     d = draw_N * sqrt(s2);  t = d * d
 *     t < 2^64:  sin_t = (2 * d) / (1 + t),  omc = (2 * t) / (1 + t)      (d = tan(theta / 2); omc = 1 - cos theta)
 *     otherwise (a NaN included):  sin_t = 0,  omc = 2
 *     sc = sin_t * cos_phi;  ss = sin_t * sin_phi
 *     gp != 0:  ax = gx / gp;  ay = gy / gp
 *               Dx = ((ax * gz) * sc - (ay * gm) * ss) - gx * omc
 *               Dy = ((ay * gz) * sc + (ax * gm) * ss) - gy * omc
 *               Dz = (-(gp * sc)) - gz * omc
 *     gp == 0:  Dx = gm * sc;  Dy = gm * ss;  Dz = -(gz * omc)         (gz with its sign: |g + D| = |g|)
 *     u_f = u_f + (m_ab / m_f) * D   componentwise, done iff  w_s >= w_f || U * w_f < w_s
 *     u_s = u_s - (m_ab / m_s) * D   componentwise, done iff  w_f >= w_s || U * w_s < w_f
 *   so that a light macro-particle is always turned and a heavy one with probability w_light / w_heavy (momentum and
 *   energy are then conserved on average only; with equal weights exactly, up to rounding).
 *   Draws: four numbers per pair, (draw_N, cos_phi, sin_phi, U).  Normally from the counter stream of the pair: with c0 of
 *   the first particle's species and j the pair's number above, r_i = mix32(mix32(c0 ^ 0x2545f491) + 4 j + i), i = 0 .. 3,
 *   unit(r) = ((float)(r >> 8) + 0.5f) / 2^24: draw_N = sqrt(-2 log unit(r_0)) cos(2 pi unit(r_1)), phi = 2 pi unit(r_2),
 *   U = unit(r_3) -- the device's own log, cos and sin: statistically specified, not bit for bit.  Same array, seed and
 *   call: same result.  With vpic_hip_set_collide_draws (parity tests) they are read from draws[4 i .. 4 i + 3], i the first
 *   particle's index in its species' array; the table must cover the longer of the two arrays.
 * cvar = (q_a q_b)^2 ln(Lambda) / (8 pi eps0^2 c^3) in the deck's units, q and m those of a PHYSICAL particle; dt the time
 * this call stands for (the collision interval times the grid's dt).
 * What the call touches: ux, uy, uz of the two species and nothing else -- positions, voxels, charges, tags, the order of the
 * arrays, partition[] / tpart[], the push's pending histogram and windows stay as they are; host mirrors go stale as after a
 * push.  Exact ranges: a species sorted by voxel with partition[] valid, or in tile order by cell with nothing appended and
 * no dead slots, is collided where it lies when a checking pass (4 B per particle) finds every particle inside the range of
 * its own voxel; any other (never sorted, sorted by tile only, appended to, with dead slots, pushed since the sort so that a
 * particle left its cell, a sort pending inside the next push) is SORTED FIRST, in the order the engine would sort it into
 * now and never by tile only; a pending sort inside the push is carried out as a plain sort.  A cell that holds more than
 * VPIC_HIP_COLLIDE_MAX_CELL particles of one species makes the call fail before any momentum is written (a sort it needed
 * has then happened).  Two kernel instances, chosen from the fullest cell: a wavefront per cell while both species have at
 * most 64 there, a workgroup per cell (the cell's momenta, weights and keys in LDS) above.
 * Fails (non-zero, vpic_hip_last_error names the argument) on a NULL c, an unknown sp_a / sp_b, m_a / m_b / wq_a / wq_b not
 * above 0, cvar or dt negative (or NaN), a draws table shorter than an array; nothing is touched then. */
typedef struct { int sp_a, sp_b;            /* sp_a == sp_b: collisions within one species (m_b, wq_b are then not read) */
                 float m_a, m_b;            /* mass of a physical particle of each species */
                 float wq_a, wq_b;          /* weight of a macro-particle = |q| * wq  (wq = 1 / |charge of a physical particle|) */
                 float cvar;                /* (q_a q_b)^2 ln(Lambda) / (8 pi eps0^2 c^3) in the deck's units */
                 float dt;                  /* the time this call stands for (interval * grid dt) */
                 uint32_t seed, call; } vpic_hip_collision_t;
VPIC_HIP_STATIC_ASSERT(sizeof(vpic_hip_collision_t) == 40, "vpic_hip_collision_t layout");
#define VPIC_HIP_COLLIDE_MAX_CELL 1024       /* particles of ONE species in one cell: 6 LDS words each, 48 KB for two species at the cap */
int vpic_hip_collide(vpic_hip_engine_t *e, const vpic_hip_collision_t *c);
/* The last call: out[0] cells with a pair, out[1] pairs scattered, out[2] pairs skipped (gm == 0), out[3] pairs of which only
 * one particle (or neither) was updated (weights), out[4] the fullest cell (particles of one species), out[5] 1 if the call
 * sorted a species first. */
int vpic_hip_collide_stats(vpic_hip_engine_t *e, int64_t out[6]);
/* ... and the kernel instance its launch was: 1 a wavefront per cell, 2 a workgroup per cell, 0 none (nothing to collide, or
 * the call failed before its launch).  VPIC_HIP_COLLIDE_INSTANCE=group (read when the engine is created; tests) takes the
 * workgroup instance for every launch; =wave is the default choice and cannot be forced on a cell of more than 64. */
int vpic_hip_collide_instance(vpic_hip_engine_t *e, int *instance);
/* parity tests: the four draws of every pair from a table in host memory, 4 floats per particle index (see above); n = 0
 * switches back to the counter stream */
int vpic_hip_set_collide_draws(vpic_hip_engine_t *e, const float *draws, int64_t n);
/* ---- the same collisions with the RELATIVISTIC pair of Perez et al., Phys. Plasmas 19, 083104 (2012), sections II A and B ----
 * u is the momentum per mass in units of c, as everywhere else in this library.  The pair is taken to its centre-of-momentum
 * frame, turned there by an angle whose variance carries the relativistic factors, and taken back: every pair of equal
 * weights keeps m_f u_f + m_s u_s and m_f gamma_f + m_s gamma_s (up to rounding).  An opt-in model: vpic_hip_collide is
 * bit for bit what it was.
 * SHARED with vpic_hip_collide, word for word (THE RULE above): the descriptor and its argument errors, the exact ranges or
 * the sort first, the cap, mix32, the cells, c0, the keys and perm, the pairs of one species (the triple of an odd cell with
 * s2 halved), the L / S pairs of two species, N, w, the first particle of a pair, the four draws per pair and where they
 * come from (counter stream or vpic_hip_set_collide_draws), the weight rule (do_f, do_s below are the two conditions above),
 * the order in which pairs that share a particle are applied, what the call touches, the two kernel instances,
 * vpic_hip_collide_stats (out[2] also counts the pairs the two skips below leave alone) and vpic_hip_collide_instance.
 * Only PER PAIR differs.  (tests/collide_rel_ref.py restates it in numpy; tests/test_gpu_collide_rel.py holds every word to it.)
 *   Per pair (first f, second s): the float momenta, masses, weights w, cvar, dt, V = (dx * dy) * dz (that float product), N
 *   and the four draws are promoted to double; every operation below is IEEE double, rounded once, unfused, / and sqrt
 *   correctly rounded, the parentheses as written; the two new momenta are rounded to float once each, at the end.
 *     ux_f == ux_s && uy_f == uy_s && uz_f == uz_s (compared as floats): the pair is skipped (and counted); otherwise
 *     g_f = sqrt(1 + ((ux_f*ux_f + uy_f*uy_f) + uz_f*uz_f));  g_s likewise                              (the Lorentz factors)
 *     e_f = m_f * g_f;  e_s = m_s * g_s;  E = e_f + e_s;  rE = 1 / E
 *     vx = (m_f*ux_f + m_s*ux_s) * rE;  vy, vz likewise                     (v_C = P / E, the velocity of the pair's frame)
 *     gC = 1 / sqrt(1 - ((vx*vx + vy*vy) + vz*vz));  kC = (gC * gC) / (gC + 1)      (kC = (gC - 1) / v_C^2 without its cancellation)
 *     vu_f = (vx*ux_f + vy*uy_f) + vz*uz_f;  vu_s likewise
 *     c_f = kC * vu_f - gC * g_f
 *     px = m_f * (ux_f + c_f * vx);  py, pz likewise                      (p*, the first particle's momentum in that frame)
 *     es_f = m_f * (gC * (g_f - vu_f));  es_s = m_s * (gC * (g_s - vu_s))                   (m gamma* of each in that frame)
 *     pq = px*px + py*py;  p2 = pq + pz*pz;  pm = sqrt(p2);  gp = sqrt(pq)
 *     pm == 0: the pair is skipped (and counted); otherwise
 *     r = (es_f * es_s) / (pm * pm) + 1
 *     s2 = ((((cvar * max(w_f, w_s)) * N) * dt) * (((gC * pm) * rE) * (r * r))) / (V * (e_f * e_s));  in the triple s2 = 0.5 * s2
 *          (max(w_f, w_s) taken of the floats.  Perez eq. 21: the variance of tan(theta / 2); for |u| -> 0 it is the s2 above)
 *     d = draw_N * sqrt(s2);  t = d * d
 *     t < 2^64:  sin_t = (2 * d) / (1 + t),  omc = (2 * t) / (1 + t);   otherwise (a NaN included):  sin_t = 0,  omc = 2
 *     sc = sin_t * cos_phi;  ss = sin_t * sin_phi
 *     gp != 0:  ax = px / gp;  ay = py / gp
 *               Dx = ((ax * pz) * sc - (ay * pm) * ss) - px * omc
 *               Dy = ((ay * pz) * sc + (ax * pm) * ss) - py * omc
 *               Dz = (-(gp * sc)) - pz * omc
 *     gp == 0:  Dx = pm * sc;  Dy = pm * ss;  Dz = -(pz * omc)
 *     qx = px + Dx;  qy, qz likewise                                                   (p* turned: |q| = |p*|)
 *     kvq = kC * ((vx*qx + vy*qy) + vz*qz)
 *     a_f = kvq + es_f * gC;   u_f = (float)((q + v * a_f) * (1 / m_f))      componentwise, ((qx + vx * a_f) * (1 / m_f)), done iff do_f
 *     a_s = es_s * gC - kvq;   u_s = (float)((v * a_s - q) * (1 / m_s))      componentwise, ((vx * a_s - qx) * (1 / m_s)), done iff do_s
 * Limits.  Rank-local, dependent on the order of the array within a cell, capped at VPIC_HIP_COLLIDE_MAX_CELL, all as above.
 * The double boost is meant for |u| from about 1e-3 to about 1e3; the tests cover 1e-3 .. 30.  Upwards the boost loses
 * gC^2 ulps of double in the pair's sum m u and sum m gamma (g_f - v_C.u_f cancels: 1e-10 of E at gC = 1e3, a thousandth of
 * a float ulp) and 1 - v_C^2 rounds to 0 near gC = 1e8.  Below |u| ~ 1e-3 the result is still right to float rounding in u, but the
 * energy of a pair is carried as m gamma and kept only to about 1e-16 m gamma / (its kinetic energy): 2e-5 of the kinetic
 * energy at |u| = 1e-4 and a mass ratio of 1836.  vpic_hip_collide is the better tool there.  Not included: the
 * low-temperature and maximum-frequency correction of Perez section II C, and a computed Coulomb logarithm (cvar carries
 * ln(Lambda) as before). */
int vpic_hip_collide_relativistic(vpic_hip_engine_t *e, const vpic_hip_collision_t *c);

/* ---- radiative cooling of one species: synchrotron losses and Compton drag (csrc/cool.hip) ----
 * Another stage for a deck's user_particle_collisions (between the sort and the push): one pass over a species that changes
 * ux, uy, uz and nothing else.  The model is the leading terms of the Landau-Lifshitz radiation-reaction force, in the form
 * radiative PIC codes use, plus the Thomson drag of an isotropic photon bath.  u is the momentum per mass in units of c, v =
 * u / gamma; E and cB are as the field array holds them.  The caller folds every unit into two numbers:
 *   sync = tau0 (q / m c)^2 times the time the call stands for, tau0 = q^2 / (6 pi eps0 m c^3) of a PHYSICAL particle; then
 *          du = sync { (E + v x cB) x cB + (v.E) E - gamma^2 [ (E + v x cB)^2 - (v.E)^2 ] v }
 *   ic   = (4/3) sigma_T U_ph / (m c) times that time (U_ph the energy density of the photons): du = -ic gamma u
 * THE RULE, a contract (tests/cool_ref.py restates it in numpy; tests/test_gpu_cool.py holds every word to it).
 *   Per live particle: 0 <= i < nv; dead slots (i = -1) are skipped, particles appended since the last sort are included, a
 *   particle in a ghost voxel uses that voxel's record.  ex .. cbz are the float fields at the particle exactly as
 *   vpic_hip_species_select below states them, from the interpolator AS IT IS LOADED at the call, then promoted to double
 *   Ex .. Bz; ux, uy, uz are promoted.  Everything after that is IEEE double, every operation rounded once, unfused, / and
 *   sqrt correctly rounded, the parentheses as written:
 *     u2 = (ux*ux + uy*uy) + uz*uz;   g = sqrt(1 + u2);   rg = 1 / g;   vx = ux*rg;  vy = uy*rg;  vz = uz*rg
 *     Lx = Ex + (vy*Bz - vz*By);   Ly = Ey + (vz*Bx - vx*Bz);   Lz = Ez + (vx*By - vy*Bx)
 *     vE = (vx*Ex + vy*Ey) + vz*Ez
 *     Ax = (Ly*Bz - Lz*By) + vE*Ex;   Ay = (Lz*Bx - Lx*Bz) + vE*Ey;   Az = (Lx*By - Ly*Bx) + vE*Ez
 *     L2 = (Lx*Lx + Ly*Ly) + Lz*Lz;   chi = L2 - vE*vE;   chi < 0: chi = 0   (a NaN stays a NaN)
 *     D  = g * (sync*chi + ic);   den = 1 + D              (gamma^2 v = gamma u: the drag term is -D u, taken implicitly)
 *     nx = (ux + sync*Ax) / den;  ny, nz likewise;   ux' = (float)nx,  uy', uz' likewise   (one rounding each)
 *     D, nx, ny or nz not finite: the particle is LEFT ALONE -- nothing written, nothing tallied, counted in out[3]
 *     u2n = (ux'*ux' + uy'*uy') + uz'*uz' of the promoted new floats;   g1 = sqrt(1 + u2n)
 *     val = (double)fabsf(q) * ((u2 - u2n) / (g + g1))     (|q| (gamma - gamma'), without the cancellation)
 *     t = val / quantum;  fabs(t) < 2^32: the particle adds llrint(t) (to nearest, ties to even) to *energy and, when
 *     cell_energy is given, to cell_energy[i]; otherwise (a NaN included) it adds nothing and is counted in out[2] -- its
 *     momenta are still written
 * *energy is the energy the drag took from the species, in units of quantum: a signed sum of integers (with E present the
 * retained terms can give a slow particle energy), so it is bit-identical in every array order and launch shape and adds
 * exactly across ranks.  sum |q| (gamma - 1) before the call minus the same after equals *energy * quantum to half a quantum
 * per particle.  cell_energy (nv words in host memory, or NULL) is the same per voxel: the map of the emitted power.  With
 * VPIC_HIP_COOL_DRY the same tallies are returned and no byte of the species changes.
 * Range of validity.  The drag term is implicit: D may be anything, and |u'| -> 0 as D -> inf.  The A term is explicit: the
 * operator is meant for sync (|E| + |cB|)^2 << 1, which every physical setting satisfies by many orders; above that a slow
 * particle overshoots.  First order in the time the call stands for, and an operator split from the push: the stored momenta
 * are half a step behind the fields, as they are for the collisions.  No quantum corrections, no photons.
 * What the call touches: ux, uy, uz of sp and nothing else.  No cell changes, so positions, voxels, q, tags, the order of the
 * array, partition[] / tpart[], the push's pending histogram and a sort pending inside the next push all stay valid; host
 * mirrors go stale as after a push.
 * Fails (non-zero, vpic_hip_last_error names the argument, nothing is touched -- the species, the last statistics and the
 * caller's arrays) on a bad sp, a NULL c or energy, sync or ic negative or not finite, quantum not positive and finite, unknown
 * flag bits, or a device allocation that fails (the scratch belongs to the engine and grows on demand: 8 bytes per voxel).
 * "Nothing is touched" holds for these two kinds of failure, which come before the launch; a runtime error behind them (a
 * launch or a copy that fails) also returns non-zero and leaves the last statistics alone, but momenta may have been written. */
enum { VPIC_HIP_COOL_DRY = 1 };              /* tally only: no momentum is written */
typedef struct { double sync, ic, quantum; int32_t flags, pad; } vpic_hip_cool_t;
VPIC_HIP_STATIC_ASSERT(sizeof(vpic_hip_cool_t) == 32, "vpic_hip_cool_t layout");
int vpic_hip_species_cool(vpic_hip_engine_t *e, int sp, const vpic_hip_cool_t *c, int64_t *energy, int64_t *cell_energy);
/* The last call: out[0] live particles seen, out[1] particles whose three new floats differ from the stored ones in any bit
 * (in a dry run: those that would), out[2] particles refused for the tally, out[3] particles left alone. */
int vpic_hip_species_cool_stats(vpic_hip_engine_t *e, int64_t out[4]);

/* ---- energy spectra of a species (the diagnostic of decks/trecon-part/energy.cxx, computed where the particles are) ----
 * One pass over the species' stored momenta (no half-step field correction, unlike energy_p).  Per live particle
 * (dead slots are skipped, particles appended since the last sort are included), energy.cxx:96-108 restated:
 *   ke   = sqrt(((1 + ux^2) + uy^2) + uz^2) - 1, the float momenta promoted to double, every operation in double, unfused
 *          (energy.cxx:99 as C++ evaluates it squares in float first: a particle within a float rounding, about 1e-7
 *          relative, of a band or bin edge may be counted next door there)
 *   band = (int)(ke / d_lin), clamped to n_lin - 1                       (:102-104, counted in the particle's voxel)
 *   bin  = (int)((log10(ke) - log_lo) / d_log + 1), counted when 0 <= bin <= n_log - 1   (:107-108)
 * The conversion to int truncates toward zero, so bin 0 also collects values in (-1, 0); ke == 0 counts in no bin.
 * The caller computes the constants (the deck mixes float and double in them: dke = emax * (vth * vth / 2.0) / nex,
 * log_lo = log10(eminp) of a float eminp, dloge a float) and hands them over as doubles.
 * Counts are integers: the result is the same bit for bit whatever order the array is in and whichever kernel
 * pushed it.  The reference counts in float (dist[...]++, edist[k]++), which stops increasing at 2^24; the helper of
 * the deck host (vpic_simulation::energy_spectrum) converts these counts to float, so its output equals the
 * reference's only while every count is below 2^24 -- above that, this one is the correct one. */
typedef struct {
  int32_t n_lin;   /* linear bands per voxel (the deck's nex); 0: none            */
  int32_t n_log;   /* bins of the log spectrum (the deck's nbin = 800); 0: none  */
  double  d_lin;   /* band width in units of ke (the deck's dke)                 */
  double  log_lo;  /* log10 of the lowest energy, as the caller computed it      */
  double  d_log;   /* bin width in log10(ke) (the deck's dloge, promoted)        */
} vpic_hip_spectrum_t;
VPIC_HIP_STATIC_ASSERT(sizeof(vpic_hip_spectrum_t) == 32, "vpic_hip_spectrum_t layout");
/* most log bins a call takes: a workgroup keeps them as 32-bit counters in LDS (16 KB) beside its four wavefronts'
 * windows of linear bands (up to 12 KB each) */
#define VPIC_HIP_SPECTRUM_MAX_LOG 4096
/* counts only: lin_counts[k*nv + voxel] (uint32, n_lin*nv, ghosts zero), log_counts[n_log] (uint64); host arrays,
 * either may be NULL (that part is then not computed).  Fails on a bad sp, a NULL s, a negative count, a width that
 * is not positive, or n_log above VPIC_HIP_SPECTRUM_MAX_LOG. */
int vpic_hip_energy_spectrum(vpic_hip_engine_t *e, int sp, const vpic_hip_spectrum_t *s,
                             uint32_t *lin_counts, uint64_t *log_counts);
/* the per-voxel bands as energy.cxx writes them (:116-162): float bands[k*nv + voxel] = (float)((double)count /
 * (double)n_voxel), n_voxel the sum of the voxel's bands (0 where that is 0); then every ghost voxel takes the
 * bands of the interior voxel that clamping each of its indices into [1, n] gives.  (The reference's loop normalises and
 * copies in one sweep, so a ghost on a LOW face copies its neighbour before that one has been normalised and keeps raw
 * counts; here every ghost holds normalised bands.)  n_log is ignored. */
int vpic_hip_energy_bands(vpic_hip_engine_t *e, int sp, const vpic_hip_spectrum_t *s, float *bands);
/* the last call of either: out[0] particles counted, out[1] particles whose linear band was added in global memory
 * because their voxel was outside the LDS window of their wavefront (spectrum.hip).  0 for a species in voxel or tile
 * order whose every 64 consecutive particles lie within 64 sort keys (within two consecutive tiles when it is sorted by
 * tile only); particles that moved or were appended since the sort may miss, an array in no order misses almost
 * always, more than 48 bands have no window and always miss.  Misses cost time, never the result. */
int vpic_hip_energy_spectrum_stats(vpic_hip_engine_t *e, int64_t out[2]);

/* ---- phase-space distributions of a species: a 1-D or 2-D histogram over position, momentum, kinetic energy and
 * the coordinates in the frame of the local magnetic field, optionally of the particles inside a region, computed where the particles are (csrc/distribution.hip) ----
 * One pass over those of the species' arrays that the descriptor names (x-ux reads i, dx, ux: 12 B per particle).
 * Everything below is IEEE double, every operation rounded once, unfused.  Per live particle -- 0 <= i < nv; dead
 * slots (i = -1) are skipped, particles appended since the last sort are included:
 *   X, Y, Z   position in cells from the low corner of the domain's interior: the voxel i = cx + sy * (cy + (ny+2) * cz),
 *             sy = nx + 2, is decoded, and X = (double)(cx - 1) + ((double)dx + 1.0) * 0.5; Y and Z likewise.  X lies in
 *             [0, nx]; a particle whose voxel is in a ghost layer falls outside that interval by the same formula.  The
 *             units are local cells because vpic_hip_grid_t has no origin: the caller folds the origin and the cell size
 *             into lo and d (vpic_simulation::distribution of the deck host does, from physical units).
 *   UX, UY, UZ the stored float momenta promoted to double
 *   KE        sqrt(((1 + ux^2) + uy^2) + uz^2) - 1 with the promoted momenta (as vpic_hip_energy_spectrum)
 *   LOG10_KE  log10(KE); KE == 0 gives -inf, which lies in no bin
 * In the frame of the local magnetic field (codes 16 to 21; 8 to 15 are unknown): ex, ey, ez, cbx, cby, cbz are the
 * fields at the particle exactly as vpic_hip_species_select below states them -- float, every operation rounded once,
 * unfused, from the interpolator AS IT IS LOADED at the call, of the particle's voxel (a particle in a ghost voxel uses
 * that voxel's record) -- then promoted to double as Ex, Ey, Ez, Bx, By, Bz; ux, uy, uz are promoted as for UX..UZ.
 * Everything after that is IEEE double, every operation rounded once, unfused, summed from the left:
 *     b2    = (Bx*Bx + By*By) + Bz*Bz          B     = sqrt(b2)
 *     udotb = (ux*Bx + uy*By) + uz*Bz          U_PAR = udotb / B
 *     u2    = (ux*ux + uy*uy) + uz*uz
 *     perp2 = u2 - U_PAR*U_PAR                 p2    = perp2 < 0 ? 0.0 : perp2      (a NaN stays a NaN)
 *     U_PERP = sqrt(p2)
 *     PITCH  = U_PAR / sqrt(u2)                (the cosine of the pitch angle)
 *     MU     = p2 / (2.0 * B)                  (u_perp^2 / 2|cB|: the magnetic moment per unit mass, in code units)
 *     E_PAR  = ((Ex*Bx + Ey*By) + Ez*Bz) / B
 *   No special cases, the quotients produce the edge values: B == 0 gives B = 0 and NaN for the other five; u == 0 gives
 *   U_PAR = U_PERP = MU = 0 and PITCH = NaN.  A NaN lies in no bin and in no range.  The momenta are the stored ones
 *   (time-centring is the caller's business: vpic_hip_center_p first, as for a particle dump); cB is in the units the
 *   field array holds.  A descriptor that names one of the six reads, beside the particle arrays, 24 bytes of the
 *   voxel's interpolator record per live particle (all 72 with E_PAR); one that names none reads what it always read.
 * Selection: the particle is kept when lo <= c < hi holds for every one of the n_sel ranges (0 to 4 of them).
 * Bin: per axis t = (c - lo) / d; a kept particle is counted when t >= 0 && t < n on every axis (so a NaN is never
 * counted), in bin (int)t.  Nothing is clamped into the end bins.  counts[b1 * n0 + b0], n1 = 1 when n_axes == 1.
 * Counters are integers (32-bit per workgroup or wavefront in LDS, 64-bit in global memory): the result is the same
 * bit for bit whatever order the array is in and whichever kernel pushed it. */
enum { VPIC_HIP_COORD_X = 0, VPIC_HIP_COORD_Y, VPIC_HIP_COORD_Z,
       VPIC_HIP_COORD_UX, VPIC_HIP_COORD_UY, VPIC_HIP_COORD_UZ,
       VPIC_HIP_COORD_KE, VPIC_HIP_COORD_LOG10_KE,                                            /* 0..7 */
       VPIC_HIP_COORD_U_PAR = 16, VPIC_HIP_COORD_U_PERP, VPIC_HIP_COORD_PITCH, VPIC_HIP_COORD_MU,
       VPIC_HIP_COORD_B, VPIC_HIP_COORD_E_PAR };                                              /* 16..21 */
typedef struct { int32_t coord, n; double lo, d; } vpic_hip_dist_axis_t;        /* n bins of width d from lo */
typedef struct { int32_t coord, pad; double lo, hi; } vpic_hip_dist_range_t;    /* keep particles with lo <= c < hi */
typedef struct {
  int32_t n_axes, n_sel;                  /* 1 or 2 axes; 0 to 4 ranges */
  vpic_hip_dist_axis_t axis[2];
  vpic_hip_dist_range_t sel[4];
} vpic_hip_dist_t;
VPIC_HIP_STATIC_ASSERT(sizeof(vpic_hip_dist_axis_t) == 24 && sizeof(vpic_hip_dist_range_t) == 24 && sizeof(vpic_hip_dist_t) == 152,
                       "vpic_hip_dist_t layout");
#define VPIC_HIP_DIST_MAX_BINS (1 << 22)     /* n0 * n1: 32 MB of uint64 at the most */
/* Up to this many bins (n0 * n1) every workgroup keeps the whole histogram in its LDS as 32-bit counters and adds
 * it to global memory once, at the end: 32 KB, so that five workgroups of four wavefronts share a CU's 160 KB. */
#define VPIC_HIP_DIST_LDS_BINS 8192
/* counts: n0 * n1 uint64 in host memory.  Fails (non-zero, vpic_hip_last_error) on a bad sp, a NULL d or counts,
 * n_axes other than 1 or 2, n_sel outside 0..4, an unknown coordinate, n < 1, a d that is not positive and finite,
 * or n0 * n1 above VPIC_HIP_DIST_MAX_BINS. */
int vpic_hip_species_distribution(vpic_hip_engine_t *e, int sp, const vpic_hip_dist_t *d, uint64_t *counts);
/* The last call: out[0] live particles seen, out[1] particles kept by the selection, out[2] particles counted (the
 * sum of counts), out[3] particles added through global memory because their bin was outside what their workgroup or
 * wavefront held in LDS.  Three paths (distribution.hip):
 *   n0 * n1 <= VPIC_HIP_DIST_LDS_BINS: the whole histogram is in LDS, out[3] is 0 always.
 *   Larger, and an axis is X, Y or Z (the first such axis is "the position axis", of width d cells per bin): every
 *     wavefront keeps an LDS window of W consecutive bins of the position axis by all bins of the other axis, W at least
 *     the ceil(4 / d) + 1 bins that the four cells of a tile can touch, and moves it to the first bin of the tile its
 *     particles are in, at most twice per 64 particles.  This path is taken when W x the other axis' bins fit in 3072
 *     words, which they do for a position axis with bins one cell wide or wider and up to 512 bins on the other axis
 *     (half a cell: 256).  Then out[3] is 0 for a species in voxel order or in tile order (by cell or by tile only)
 *     whose every 64 consecutive particles lie in at most two voxels (two tiles when sorted by tile only) -- at least
 *     64 particles in every occupied voxel is enough.  Particles that moved or were appended since the sort may miss;
 *     an array in no order misses almost always.  (A species in tile order is walked tile by tile, the tiles that share
 *     their bins of the position axis by the same wavefront; the rule is the same.)
 *   Otherwise (a large momentum-momentum histogram, position bins too fine for a window): every counted particle is
 *     added in global memory, the lanes of a wavefront that share a bin adding once together, and out[3] == out[2].
 * Misses cost time, never the result. */
int vpic_hip_species_distribution_stats(vpic_hip_engine_t *e, int64_t out[4]);

/* ---- per-bin sums of particle quantities: beside the count of every bin of a histogram, up to four sums over the
 * particles counted in it, as exact integers (csrc/distribution.hip) ----
 * The descriptor d is vpic_hip_species_distribution's: axes, ranges, live and dead slots and the counted test are
 * exactly those, and counts[] (which may be NULL) equals, bit for bit, what that call returns for the same d.
 * A value is the product of three factors.  A factor is a VPIC_HIP_COORD_* code other than LOG10_KE -- the coordinate
 * as stated above; LOG10_KE stays an axis and a range only, the device's and the host's log10 may differ in the last
 * bit -- or one of the four codes below.  Everything is IEEE double, every operation rounded once, unfused:
 *   ONE        1.0 (fills the factors a value does not use: x * 1.0 is x)
 *   Q          (double)q, the stored float macro-charge of the particle -- its weight.  The q array is read only when
 *              a value names it (4 B per particle).
 *     gamma  = sqrt(((1 + ux*ux) + uy*uy) + uz*uz)      (KE's expression before the - 1; ux, uy, uz promoted)
 *   EDOTV      ((Ex*ux + Ey*uy) + Ez*uz) / gamma         Ex, Ey, Ez the float fields at the particle as
 *              vpic_hip_species_select forms them, promoted to double: E . v in units of c
 *   EPAR_VPAR  (E_PAR * U_PAR) / gamma                   with E_PAR and U_PAR as stated above: the share of E . v
 *              that the field along B does
 *   EDOTV and EPAR_VPAR read all 72 bytes of the voxel's interpolator record, as E_PAR does, and run in the kernel
 *   instances of the field coordinates; so does every value that names one of those.
 * Value k of a COUNTED particle:  val = (f0 * f1) * f2,  t = val / quantum.  When fabs(t) < 4294967296.0 (2^32) the
 * particle adds llrint(t) -- round to nearest, ties to even -- to its bin of sums[k]; otherwise (a NaN included) it adds
 * nothing to value k and is counted as refused for it: it is still counted in counts[], and the other values still
 * take it.  A species holds fewer than 2^31 particles and every addend is below 2^32 in magnitude, so no int64 sum can
 * wrap.  quantum is the resolution the caller asks for: at the coarsest 2^-32 of the largest |val| it expects (a coarser
 * one cannot be had: larger values are refused), finer where the values allow.  sum of val over a bin = sums * quantum
 * to within half a quantum per particle.  The sums are integers: they are the same bit for bit whatever order the
 * array is in and on either path below, and the sums of several ranks add exactly. */
enum { VPIC_HIP_FACTOR_ONE = 32, VPIC_HIP_FACTOR_Q, VPIC_HIP_FACTOR_EDOTV, VPIC_HIP_FACTOR_EPAR_VPAR };   /* 32..35 */
typedef struct { int32_t factor[3]; int32_t pad; double quantum; } vpic_hip_dist_value_t;   /* val = (f0 * f1) * f2, in units of quantum */
VPIC_HIP_STATIC_ASSERT(sizeof(vpic_hip_dist_value_t) == 24, "vpic_hip_dist_value_t layout");
#define VPIC_HIP_DIST_MAX_VALUES 4
/* counts: n0 * n1 uint64 in host memory, or NULL; sums: n_val * n0 * n1 int64 in host memory, sums[k * n0*n1 + b1*n0 + b0].
 * Fails (non-zero, vpic_hip_last_error) on everything vpic_hip_species_distribution fails on (but for the NULL counts),
 * n_val outside 1..VPIC_HIP_DIST_MAX_VALUES, a NULL v or sums, an unknown factor or LOG10_KE as a factor, or a quantum
 * that is not positive and finite.  Returns 0 when particles were refused: the caller reads the statistics.  The species,
 * its order, its bookkeeping and the host mirrors are left exactly as they were. */
int vpic_hip_species_distribution_sums(vpic_hip_engine_t *e, int sp, const vpic_hip_dist_t *d,
                                       const vpic_hip_dist_value_t *v, int n_val, uint64_t *counts, int64_t *sums);
/* The last call: out[0..3] as vpic_hip_species_distribution_stats (live particles seen, kept, counted, counted through
 * global memory), out[4 + k] the particles refused for value k (0 for k >= n_val).  Two paths (distribution.hip):
 *   n0 * n1 * (1 + 2 n_val) <= VPIC_HIP_DIST_LDS_BINS -- the 32-bit counts and n_val rows of 64-bit sums fit the 32 KB
 *     of the histogram's LDS path: every workgroup keeps all of them in LDS (64-bit LDS integer atomics for the sums) and
 *     adds them to global memory once, at the end; out[3] is 0.  That is 2730, 1638, 1170, 910 bins for 1 to 4 values.
 *   Larger: every counted particle adds in global memory, the lanes of a wavefront that share a bin combining first,
 *     and out[3] == out[2].  (There is no sliding window for sums: a position axis makes no difference.) */
int vpic_hip_species_distribution_sums_stats(vpic_hip_engine_t *e, int64_t out[8]);

/* ---- cell distributions: the histogram and the exact per-bin sums above, over the CELLS OF THE GRID instead of the
 * particles of a species (csrc/cell_dist.hip, csrc/cell_coords.h) ----
 * The descriptors are vpic_hip_dist_t and vpic_hip_dist_value_t unchanged: 1 or 2 axes, 0 to 4 ranges lo <= c < hi,
 * val = (f0 * f1) * f2 in units of quantum.  Their coord and factor codes are the VPIC_HIP_CELL_* below, numbered from 64
 * so that no particle code (VPIC_HIP_COORD_*, VPIC_HIP_FACTOR_*) is one of them: a particle code is an unknown coordinate.
 * Items: the nx * ny * nz interior cells, 1 <= cx <= nx, 1 <= cy <= ny, 1 <= cz <= nz, voxel v = cx + sy * (cy + (ny+2) * cz),
 *   sy = nx + 2, sz = sy * (ny + 2).  A ghost voxel is never an item (and is read only as the +1 neighbour of an interior cell:
 *   every read is inside the array).
 * Per cell:
 *   X, Y, Z     the cell's centre in local cells: X = (double)(cx - 1) + 0.5, Y and Z likewise.  An axis lo = 0, d = 1,
 *               n = nx has one bin per column of cells, exactly.
 *   F_EX .. F_RHOF (VPIC_HIP_CELL_F0 + word)   the 16 float words of vpic_field_t at voxel v, in its order, promoted to
 *               double; each at its own place on the Yee mesh, attributed to cell v.
 *   H_JX .. H_TXY (VPIC_HIP_CELL_H0 + word)    the 14 float words of the engine's hydro record (vpic_hydro_t) at voxel v --
 *               node values -- promoted to double.  A descriptor that names one fails when the hydro array was never
 *               allocated (nothing has cleared, set, read or accumulated it).
 *   Cell-centre fields from the FIELD ARRAY, in float, every operation rounded once, unfused, the expressions of
 *   load_interpolator (src/sf_interface/load_interpolator.cxx:75-120):
 *     EX_C = 0.25f * ((w3 + w0) + (w1 + w2))   w0 = ex[v], w1 = ex[v+sy], w2 = ex[v+sz], w3 = ex[v+sy+sz]
 *     EY_C   the same over                      ey[v], ey[v+sz], ey[v+1], ey[v+sz+1]
 *     EZ_C   the same over                      ez[v], ez[v+1], ez[v+sy], ez[v+1+sy]
 *     BX_C = 0.5f * (cbx[v+1] + cbx[v])         BY_C pairs v with v+sy, BZ_C with v+sz
 *     JX_C, JY_C, JZ_C   the expressions of EX_C, EY_C, EZ_C over jfx, jfy, jfz
 *   then promoted to double as Ex, Ey, Ez, Bx, By, Bz, Jx, Jy, Jz.  Of a freshly loaded interpolator EX_C .. BZ_C equal
 *   ex, ey, ez, cbx, cby, cbz of the cell's record bit for bit; the call reads the field array, never the interpolator,
 *   so they are never stale.
 *   Derived, IEEE double, every operation rounded once, unfused, summed from the left:
 *     E_C     = sqrt((Ex*Ex + Ey*Ey) + Ez*Ez)          B_C = sqrt((Bx*Bx + By*By) + Bz*Bz)
 *     E_PAR_C = ((Ex*Bx + Ey*By) + Ez*Bz) / B_C        J_PAR_C = ((Jx*Bx + Jy*By) + Jz*Bz) / B_C
 *     JDOTE_C = (Jx*Ex + Jy*Ey) + Jz*Ez
 *   No special cases: B_C == 0 gives NaN for E_PAR_C and J_PAR_C.  A NaN lies in no bin and in no range.
 *   ONE         1.0; a factor only (as an axis or a range it is an unknown coordinate).
 * Selection, bins, values and refusals are vpic_hip_species_distribution_sums' word for word: a cell is kept when
 * lo <= c < hi for every range; per axis t = (c - lo) / d, a kept cell is counted when t >= 0 && t < n on every axis, in bin
 * (int)t, nothing clamped; value k of a counted cell, t = val / quantum, adds llrint(t) to its bin of sums[k] when
 * fabs(t) < 4294967296.0 and otherwise (a NaN included) is refused for value k alone -- the cell stays counted and the other
 * values take it.  A grid holds fewer than 2^31 cells: no int64 sum can wrap.  Counts and sums are integers: the same bit
 * for bit on either path below, and the sums of several ranks add exactly.
 * Only the component arrays the descriptor names are read (4 bytes per cell and raw word, the two or four neighbour words
 * of a centred field, 16 bytes per four hydro words).  Fields, hydro, interpolator and every species are left as they were. */
enum { VPIC_HIP_CELL_X = 64, VPIC_HIP_CELL_Y, VPIC_HIP_CELL_Z,                                /* 64..66 */
       VPIC_HIP_CELL_F0 = 72,                                                                  /* 72..87: F0 + word of vpic_field_t */
       VPIC_HIP_CELL_F_EX = 72, VPIC_HIP_CELL_F_EY, VPIC_HIP_CELL_F_EZ, VPIC_HIP_CELL_F_DIV_E_ERR,
       VPIC_HIP_CELL_F_CBX, VPIC_HIP_CELL_F_CBY, VPIC_HIP_CELL_F_CBZ, VPIC_HIP_CELL_F_DIV_B_ERR,
       VPIC_HIP_CELL_F_TCAX, VPIC_HIP_CELL_F_TCAY, VPIC_HIP_CELL_F_TCAZ, VPIC_HIP_CELL_F_RHOB,
       VPIC_HIP_CELL_F_JFX, VPIC_HIP_CELL_F_JFY, VPIC_HIP_CELL_F_JFZ, VPIC_HIP_CELL_F_RHOF,
       VPIC_HIP_CELL_H0 = 88,                                                                  /* 88..101: H0 + word of vpic_hydro_t */
       VPIC_HIP_CELL_H_JX = 88, VPIC_HIP_CELL_H_JY, VPIC_HIP_CELL_H_JZ, VPIC_HIP_CELL_H_RHO,
       VPIC_HIP_CELL_H_PX, VPIC_HIP_CELL_H_PY, VPIC_HIP_CELL_H_PZ, VPIC_HIP_CELL_H_KE,
       VPIC_HIP_CELL_H_TXX, VPIC_HIP_CELL_H_TYY, VPIC_HIP_CELL_H_TZZ,
       VPIC_HIP_CELL_H_TYZ, VPIC_HIP_CELL_H_TZX, VPIC_HIP_CELL_H_TXY,
       VPIC_HIP_CELL_EX_C = 104, VPIC_HIP_CELL_EY_C, VPIC_HIP_CELL_EZ_C,                       /* 104..112 */
       VPIC_HIP_CELL_BX_C, VPIC_HIP_CELL_BY_C, VPIC_HIP_CELL_BZ_C,
       VPIC_HIP_CELL_JX_C, VPIC_HIP_CELL_JY_C, VPIC_HIP_CELL_JZ_C,
       VPIC_HIP_CELL_E_C = 113, VPIC_HIP_CELL_B_C, VPIC_HIP_CELL_E_PAR_C, VPIC_HIP_CELL_J_PAR_C,
       VPIC_HIP_CELL_JDOTE_C,                                                                  /* 113..117 */
       VPIC_HIP_CELL_ONE = 127 };                                                              /* a factor only */
/* counts: n0 * n1 uint64 in host memory, counts[b1 * n0 + b0], or NULL when n_val > 0; sums: n_val * n0 * n1 int64 in host
 * memory, sums[k * n0*n1 + b1*n0 + b0]; n_val 0 .. VPIC_HIP_DIST_MAX_VALUES, v and sums may be NULL when it is 0.
 * Fails (non-zero, vpic_hip_last_error, no output written) on a NULL d, both outputs NULL, a NULL counts with n_val == 0,
 * n_axes other than 1 or 2, n_sel outside 0..4, an unknown code, n < 1, a d that is not positive and finite, n0 * n1 above
 * VPIC_HIP_DIST_MAX_BINS, n_val outside 0..VPIC_HIP_DIST_MAX_VALUES, a NULL v or sums with n_val > 0, a quantum that is not
 * positive and finite, or a hydro code without a hydro array.  Returns 0 when cells were refused: the caller reads the
 * statistics. */
int vpic_hip_cell_distribution(vpic_hip_engine_t *e, const vpic_hip_dist_t *d, const vpic_hip_dist_value_t *v, int n_val,
                               uint64_t *counts, int64_t *sums);
/* The last call: out[0] cells seen (nx * ny * nz), out[1] cells kept by the ranges, out[2] cells counted (the sum of
 * counts), out[3] cells counted through global memory, out[4 + k] cells refused for value k (0 for k >= n_val).  Two paths,
 * with the budget of vpic_hip_species_distribution_sums (cell_dist.hip):
 *   n0 * n1 * (1 + 2 n_val) <= VPIC_HIP_DIST_LDS_BINS: every workgroup keeps the 32-bit counts and n_val rows of 64-bit
 *     sums in LDS and adds them to global memory once, at the end; out[3] is 0.
 *   Larger: every counted cell adds in global memory, the lanes of a wavefront that share a bin combining first, and
 *     out[3] == out[2].  (No sliding window.) */
int vpic_hip_cell_distribution_stats(vpic_hip_engine_t *e, int64_t out[8]);

/* ---- selected particles of a species: those inside up to four ranges and with the tags asked for, gathered into dense
 * arrays where the particles are, so that only they come to the host (csrc/select.hip) ----
 * Live particles: 0 <= i < nv; dead slots (i = -1) are skipped, particles appended since the last sort are included.
 * Coordinates and ranges are exactly those of vpic_hip_species_distribution above: IEEE double, every operation
 *   rounded once, unfused; a particle is inside a range when lo <= c < hi, so a NaN is never kept.  The six
 *   coordinates in the frame of the local field are ranges like the others, from the same interpolator as `fields`.
 * Tags: `tag` is the particle's FIRST tag (vpic_particle_t::tag).  A species whose tag arrays were never allocated
 *   (no non-zero tag was ever uploaded) behaves as if every tag were 0, and the call allocates nothing for it.
 *     VPIC_HIP_SELECT_TAG_RANGE  keep when tag_lo <= tag < tag_hi
 *     VPIC_HIP_SELECT_TAG_EVERY  keep when ((tag % tag_every) + tag_every) % tag_every == tag_phase, % as in C: the
 *                                non-negative remainder, for negative tags too
 * Combination: a particle is kept when every one of the n_sel ranges and every enabled tag condition holds (no range
 *   and no flag: every live particle).
 * Order: record k is the k-th kept particle in increasing array index (stable), index[k] that array index (it counts
 *   dead slots: below the extent that vpic_hip_species_capacity reports).  Two calls on an unchanged species return
 *   identical bytes.
 * p[k]: the particle as vpic_hip_species_get_particles would return it, all 48 bytes, both tags.
 * fields[6k .. 6k+5]: ex, ey, ez, cbx, cby, cbz at the particle, from the interpolator AS IT IS LOADED at the call
 *   (the caller runs vpic_hip_load_interpolator when it wants the current fields).  The arithmetic is that of
 *   advance_p.cxx:74-82 without the qdt_2mc factor, in float, every operation rounded once, unfused; f is the
 *   interpolator of the particle's voxel:
 *     ex  = (f.ex + dy*f.dexdy) + dz*(f.dexdz + dy*f.d2exdydz)
 *     ey  = (f.ey + dz*f.deydz) + dx*(f.deydx + dz*f.d2eydzdx)
 *     ez  = (f.ez + dx*f.dezdx) + dy*(f.dezdy + dx*f.d2ezdxdy)
 *     cbx = f.cbx + dx*f.dcbxdx,  cby = f.cby + dy*f.dcbydy,  cbz = f.cbz + dz*f.dcbzdz
 * Outputs and cap: p, fields and index are host arrays of cap records each (48 bytes, six floats, one int64); any of
 *   them may be NULL, and that part is then neither computed nor copied.  *count is ALWAYS the number of kept
 *   particles; only the first min(*count, cap) records are written, and the call still returns 0: the caller compares
 *   *count with cap.
 * The species is read and nothing about it changes: no compaction (its dead slots stay), its order, tile partition,
 *   sort bookkeeping and pending histogram stay, no host mirror becomes resident.
 * Fails (non-zero, vpic_hip_last_error) on a bad sp, a NULL s or count, n_sel outside 0..4, an unknown coordinate,
 * unknown flag bits, (TAG_EVERY) tag_every < 1 or tag_phase outside [0, tag_every), cap < 0, or a device allocation
 * that fails (the device arrays belong to the engine and grow on demand: 1 bit per particle, 12 bytes per 2048
 * particles, and 48 + 24 + 8 bytes per record written for the parts asked for). */
enum { VPIC_HIP_SELECT_TAG_RANGE = 1, VPIC_HIP_SELECT_TAG_EVERY = 2 };
typedef struct {
  int32_t n_sel, flags;                 /* 0 to 4 ranges; VPIC_HIP_SELECT_* bits */
  vpic_hip_dist_range_t sel[4];         /* as in vpic_hip_dist_t: keep when lo <= c < hi for every range */
  int64_t tag_lo, tag_hi;               /* TAG_RANGE: keep when tag_lo <= tag < tag_hi */
  int64_t tag_every, tag_phase;         /* TAG_EVERY: keep when ((tag % every) + every) % every == phase */
} vpic_hip_select_t;
VPIC_HIP_STATIC_ASSERT(sizeof(vpic_hip_select_t) == 136, "vpic_hip_select_t layout");
/* the count alone: the marking pass and the scan, nothing is written */
int vpic_hip_species_select_count(vpic_hip_engine_t *e, int sp, const vpic_hip_select_t *s, int64_t *count);
int vpic_hip_species_select(vpic_hip_engine_t *e, int sp, const vpic_hip_select_t *s, int64_t cap,
                            vpic_particle_t *p, float *fields, int64_t *index, int64_t *count);
/* The last call of either: out[0] live particles seen, out[1] particles kept, out[2] records written (min(kept, cap);
 * 0 for select_count and when every output array was NULL), out[3] the chunks (of 2048 particles) the array was cut
 * into. */
int vpic_hip_species_select_stats(vpic_hip_engine_t *e, int64_t out[4]);
int vpic_hip_center_p(vpic_hip_engine_t *e, int sp);        /* species_advance/standard/center_p.cxx: u(-1/2) -> u(0) */
int vpic_hip_uncenter_p(vpic_hip_engine_t *e, int sp);      /* species_advance/standard/uncenter_p.cxx:154-177: u(0) -> u(-1/2) */
int vpic_hip_clear_jf(vpic_hip_engine_t *e);                /* field_advance/standard/sfa.c:188-211 */
int vpic_hip_clear_jf_unload_accumulator(vpic_hip_engine_t *e);   /* the two calls in one pass (advance.cxx:109-110 makes them back to back): same values, bit for bit */
int vpic_hip_synchronize_jf(vpic_hip_engine_t *e);          /* field_advance/standard/remote.c:416-506: local_adjust_jf + faces shared with itself */
/* the pieces of synchronize_jf for a domain that shares some faces with other domains: the local
 * adjustment (local.c:335-368), then per axis IN ORDER x, y, z (remote.c:284-289) either
 * _synchronize_jf_self (both faces wrap onto this domain) or pack_jf / exchange / unpack_jf */
int vpic_hip_local_adjust_jf(vpic_hip_engine_t *e);
int vpic_hip_synchronize_jf_self(vpic_hip_engine_t *e, int axis);
int vpic_hip_advance_b(vpic_hip_engine_t *e, float frac);   /* field_advance/standard/advance_b.c:74-161 */
int vpic_hip_advance_e(vpic_hip_engine_t *e);               /* field_advance/standard/advance_e.c:87-330 (ghosts of faces shared with other domains must be in place) */
/* advance_e in two launches so that the exchange of the remote tangential-B ghosts overlaps the first
 * (advance_e.c:114,153,191-197 does the same around begin/end_remote_ghost_tang_b): part 1 = local ghosts + the planes
 * x = 2..nx, part 2 = the planes x = 1 and nx+1 + the local adjustment (0 = everything, = vpic_hip_advance_e). */
int vpic_hip_advance_e_part(vpic_hip_engine_t *e, int part);
/* make the engine's stream wait for a HIP event recorded on another stream (the communication stream) */
int vpic_hip_stream_wait_event(vpic_hip_engine_t *e, void *hip_event);
int vpic_hip_energy_f(vpic_hip_engine_t *e, double *en6);   /* field_advance/standard/energy_f.c:139-179 (local part) */
/* boundary_p (species_advance/standard/boundary_p.c:77-505), split at the message boundary:
 *   _pack   : classify the movers of every species; absorbed ones go to rhob and are removed,
 *             emigrants are removed and written to the per-face device buffers
 *   _counts : how many injectors wait in each face's send buffer
 *   _inject : append n injectors (device pointer, e.g. a receive buffer) and finish their moves */
int vpic_hip_boundary_p_pack(vpic_hip_engine_t *e);
/* The same exchange without a round trip to the host per phase (multi-GPU driver): mover counts, particle counts
 * and injector counts stay in device memory; a message to the neighbour across face f is a device buffer
 * { int32 header[4] = {injectors in the payload, injectors wanted, 0, 0}; vpic_particle_injector_t payload[cap] }
 * (16 + 48 cap bytes, _exchange_message_bytes) that is sent WHOLE, so both ends know its size without exchanging
 * counts first (boundary_p.c:333-337 sends the count ahead of the payload).  Per step:
 *   _advance_p_async (every species) ; _exchange_begin ; per round { _exchange_pack -> send / receive ->
 *   _exchange_inject per received message } ; _exchange_finish -- the ONE synchronisation: np / nm of every species
 *   and the headers of the received messages come to the host.  Removed particles leave dead slots (index -1) that every
 *   kernel skips and the next sort drops; *flags: 1 = a round had more movers than its kernels were launched for, 2 = a
 *   message was full -- in both cases the movers concerned are still on their lists (_species_nm > 0) and the caller offers
 *   them again with larger messages (the header's `wanted` > `count` tells both ends of a message); a species out of
 *   particle or mover slots is an error (reserve earlier: _species_reserve).
 * Faces that belong to no other domain behave as in _boundary_p_pack, absorbing walls that tally and record
 * (vpic_hip_set_wall) included; maxwellian_reflux handlers are not served (they create local injectors): _exchange_pack
 * refuses an engine that has one. */
int vpic_hip_advance_p_async(vpic_hip_engine_t *e, int sp);
/* The overlap of the exchange with the push (north star; the reference's begin / interior / end pattern,
 * field_advance/standard/advance_e.c:114,153,191-197, applied to boundary_p.c:341-384).  A species in the engine's tile
 * order is pushed in two launches: phase 1 = the tiles on the faces shared with other domains and the particles appended
 * since the sort (every particle that can leave the domain this step, up to stragglers), phase 2 = the other tiles.
 * Between the two the caller packs THAT species' movers (_exchange_pack_species) and starts their transfer on its
 * communication stream; stragglers of phase 2 travel in the later rounds, which carry all species.  A species that is not
 * in tile order is pushed whole by phase 1 (phase 2 then does nothing).  phase 0 = _advance_p_async. */
int vpic_hip_advance_p_phase(vpic_hip_engine_t *e, int sp, int phase);
/* _exchange_pack for the species whose bit is set in species_mask only (messages per species: species k is on the wire
 * while species k+1 is pushed).  A shared face given no message (null / capacity 0) is closed for the round: the movers
 * bound for it stay alive and parked (flag 2, _species_nm > 0 after _finish), the other faces are served as usual, and a
 * message the face is given in a later round -- of the same _exchange_begin ... _exchange_finish or of the next -- is
 * filled from its first slot, with a header that counts that round's movers only. */
int vpic_hip_exchange_pack_species(vpic_hip_engine_t *e, uint32_t species_mask, void *const dev_msg[6], const int32_t cap[6], int mover_cap);
int vpic_hip_exchange_begin(vpic_hip_engine_t *e);
int vpic_hip_exchange_pack(vpic_hip_engine_t *e, void *const dev_msg[6], const int32_t cap[6], int mover_cap);
int vpic_hip_exchange_inject(vpic_hip_engine_t *e, const void *dev_msg, int cap);
int vpic_hip_exchange_finish(vpic_hip_engine_t *e, const void *const *dev_msgs, int n_msgs /* <= 192 (more is an argument error): per-species rounds and recovery rounds x 6 faces x sent and received, and spare */, int32_t *headers /* 4 per message */, int32_t *flags);
int vpic_hip_boundary_p_counts(vpic_hip_engine_t *e, int32_t ns[6]);
void *vpic_hip_boundary_p_send_buffer(vpic_hip_engine_t *e, int face);          /* device vpic_particle_injector_t[] */
/* copy the injectors waiting on `face` (counts from _counts) into a device buffer of the caller */
int vpic_hip_boundary_p_get_injectors(vpic_hip_engine_t *e, int face, void *dev_dst);
int vpic_hip_boundary_p_inject(vpic_hip_engine_t *e, const void *dev_injectors, int n);
/* face messages for domains that share a face with ANOTHER domain (remote.c:61-134, 416-506);
 * dir = direction of travel 0..5; buf = device float buffer of vpic_hip_face_count floats */
int vpic_hip_face_count(const vpic_hip_engine_t *e, int dir);
int vpic_hip_pack_tang_b(vpic_hip_engine_t *e, int dir, void *dev_buf);
int vpic_hip_unpack_tang_b(vpic_hip_engine_t *e, int dir, const void *dev_buf);
int vpic_hip_pack_jf(vpic_hip_engine_t *e, int dir, void *dev_buf);
int vpic_hip_unpack_jf(vpic_hip_engine_t *e, int dir, const void *dev_buf);

/* ---- divergence cleaning family and charge densities ---------------------------
 * Slots of field_advance_methods_t (src/field_advance/field_advance.h:242-302) and accumulate_rho_p
 * (src/species_advance/standard/spa.h:108-113).  As with synchronize_jf, the plain names handle the
 * local faces and the faces a domain shares with itself; a domain that shares faces with OTHER
 * domains calls the pieces (local adjustment, then per axis in order x, y, z either _self or
 * pack / exchange / unpack). */
int vpic_hip_clear_rhof(vpic_hip_engine_t *e);                       /* sfa.c:213-234 */
int vpic_hip_accumulate_rho_p(vpic_hip_engine_t *e, int sp);         /* species_advance/standard/rho_p.c:23-86 (float atomics: sums in another order) */
int vpic_hip_synchronize_rho(vpic_hip_engine_t *e);                  /* remote.c:533-622 */
int vpic_hip_local_adjust_rho(vpic_hip_engine_t *e);                 /* local.c:368-445: rhof then rhob */
int vpic_hip_synchronize_rho_self(vpic_hip_engine_t *e, int axis);
int vpic_hip_rho_count(const vpic_hip_engine_t *e, int dir);         /* floats of a rho message, remote.c:546 */
int vpic_hip_pack_rho(vpic_hip_engine_t *e, int dir, void *dev_buf);
int vpic_hip_unpack_rho(vpic_hip_engine_t *e, int dir, const void *dev_buf);
int vpic_hip_compute_rhob(vpic_hip_engine_t *e);                     /* compute_rhob.c:74-206 */
int vpic_hip_compute_curl_b(vpic_hip_engine_t *e);                   /* compute_curl_b.c:78-318 */
int vpic_hip_synchronize_tang_e_norm_b(vpic_hip_engine_t *e, double *err);   /* remote.c:298-414; *err = this domain's sum of squared differences */
int vpic_hip_compute_div_e_err(vpic_hip_engine_t *e);                /* compute_div_e_err.c:72-207 */
int vpic_hip_clean_div_e(vpic_hip_engine_t *e);                      /* clean_div_e.c:79-187 */
int vpic_hip_compute_div_b_err(vpic_hip_engine_t *e);                /* compute_div_b_err.c:62-92 */
int vpic_hip_clean_div_b(vpic_hip_engine_t *e);                      /* clean_div_b.c:79-247 */
/* Face messages of the family for faces shared with ANOTHER domain (device buffers of
 * _face_message_count floats).  kind 0: normal E (remote.c:136-207), to be in place before
 * _compute_div_e_err / _compute_rhob; kind 1: div_b_err (remote.c:209-281), before _clean_div_b;
 * kind 2: tangential E and normal B (remote.c:298-414): the receiver averages and *err gets the sum
 * of squared differences.  (_compute_curl_b needs the tang_b ghosts of _pack_tang_b.)  The pieces of
 * synchronize_tang_e_norm_b for such a domain: _local_adjust_tang_e_norm_b, then per axis in order
 * x, y, z either _synchronize_tang_e_norm_b_self or pack / exchange / unpack. */
enum { VPIC_HIP_MSG_NORM_E = 0, VPIC_HIP_MSG_DIV_B = 1, VPIC_HIP_MSG_TANG_E_NORM_B = 2 };
int vpic_hip_face_message_count(const vpic_hip_engine_t *e, int kind, int dir);
int vpic_hip_pack_face_message(vpic_hip_engine_t *e, int kind, int dir, void *dev_buf);
int vpic_hip_unpack_face_message(vpic_hip_engine_t *e, int kind, int dir, const void *dev_buf, double *err);
int vpic_hip_local_adjust_tang_e_norm_b(vpic_hip_engine_t *e);
int vpic_hip_synchronize_tang_e_norm_b_self(vpic_hip_engine_t *e, int axis, double *err);
/* local2[0] = weighted sum of squares * dV, local2[1] = volume of this domain: the two numbers the
 * reference sums over ranks (compute_rms_div_e_err.c:156-158, compute_rms_div_b_err.c:90-92) ... */
int vpic_hip_rms_div_e_err_local(vpic_hip_engine_t *e, double *local2);
int vpic_hip_rms_div_b_err_local(vpic_hip_engine_t *e, double *local2);
/* ... and eps0*sqrt(local2[0]/local2[1]) for a run of one domain */
int vpic_hip_compute_rms_div_e_err(vpic_hip_engine_t *e, double *rms);
int vpic_hip_compute_rms_div_b_err(vpic_hip_engine_t *e, double *rms);

/* ---- hydro moments: sf_interface.h:83-163, spa.h:115-123 ------------------------
 * The engine owns one hydro_t array (allocated on first use); a caller accumulates a species into
 * it, synchronises it and reads it back, as dump.cxx:63-70 does per species. */
int vpic_hip_clear_hydro(vpic_hip_engine_t *e);                      /* sf_interface.c:29-36 */
int vpic_hip_accumulate_hydro_p(vpic_hip_engine_t *e, int sp);       /* species_advance/standard/hydro_p.c:24-176 (uses the loaded interpolator; float atomics, or fixed point: vpic_hip_set_accumulation) */
/* The last accumulate_hydro_p / accumulate_rho_p call: out[0] live particles summed, out[1] particles added through the LDS
 * window of their tile (a species in tile order is summed tile by tile and keeps its order), out[2] particles added through
 * global memory (appended since the sort, drifted out of their tile's window, or a species that is not in tile order), out[3]
 * contributions outside the fixed-point range of the deterministic mode (vpic_hip_set_accumulation).  Waits for the stream. */
int vpic_hip_moments_stats(vpic_hip_engine_t *e, int64_t out[4]);
/* ---- the hydro moments of a SELECTION of a species: what accumulate_hydro_p does -- the same arithmetic per particle
 * (csrc/moments_device.h), the same engine-owned hydro array -- where only the particles add that
 * vpic_hip_species_select would return for the same descriptor and species at that moment (csrc/moments.hip) ----
 * Which particles are kept: a particle is kept when every one of the n_sel ranges holds (lo <= c < hi; a NaN is in no
 *   range) and every enabled tag condition holds.  The coordinates are those of vpic_hip_species_distribution, bit for
 *   bit: the same double arithmetic, the six in the frame of the local field included.  The fields at the particle come
 *   from the interpolator AS IT IS LOADED at the call.  A species whose tag arrays were never allocated behaves as if
 *   every tag were 0, as for vpic_hip_species_select.
 * Momenta: the coordinates use the STORED momenta, as every other selection does; the moments use the momenta advanced
 *   by half a step, as hydro_p.c does.  A caller who wants both at the same time level runs vpic_hip_center_p first, as
 *   for a particle dump.
 * Voxels at the top of the array: accumulate_hydro_p skips particles in the ghost voxels at the top of the array
 *   (i >= nv - (nx+2)(ny+2) - (nx+2) - 1: the 8 nodes of such a cell are not all inside the array); they stay skipped.
 * Order and ownership: the species is read and left as it is; the call never sorts or reorders it, not even in
 *   deterministic mode.  A species in tile order whose partition is valid and that has no pending movers is summed by the
 *   tile pass plus the tail pass; any other goes through the per-particle pass over the whole array (in float mode too:
 *   never the by-cell route, which sorts by voxel).
 * Deterministic mode (vpic_hip_set_accumulation): the fixed-point scale is that of the whole-species call -- from the
 *   species' largest |q|, not from the kept particles -- so the sums are bit-identical to those of accumulate_hydro_p on
 *   a species of the same q_m and largest |q| that holds exactly the kept particles.  The same refusal applies to
 *   contributions out of range: nothing is added and an error is returned.
 * vpic_hip_moments_stats after this call: out[0] particles kept and summed, out[1] of them added through LDS, out[2]
 *   through global memory (out[1] + out[2] == out[0]), out[3] contributions out of the fixed-point range.  out[0] equals
 *   what vpic_hip_species_select_count returns for the same descriptor, except for kept particles in the skipped ghost
 *   voxels at the top of the array, which select counts and this call does not sum.
 * A chargeless species (tracer copies) adds nothing, as in accumulate_hydro_p.
 * Fails (non-zero, vpic_hip_last_error) on a bad sp, a NULL s, n_sel outside 0..4, an unknown coordinate, unknown flag
 * bits, (TAG_EVERY) tag_every < 1 or tag_phase outside [0, tag_every): the checks of vpic_hip_species_select.  The
 * hydro array is then unchanged.  There is no accumulate_rho_p twin: rho of the selection is moment 3 of the array. */
int vpic_hip_accumulate_hydro_p_select(vpic_hip_engine_t *e, int sp, const vpic_hip_select_t *s);
int vpic_hip_synchronize_hydro(vpic_hip_engine_t *e);                /* sf_interface/hydro.c:28-163: local adjustment + faces shared with itself */
int vpic_hip_local_adjust_hydro(vpic_hip_engine_t *e);               /* sf_interface/hydro.c:165-200 */
int vpic_hip_synchronize_hydro_self(vpic_hip_engine_t *e, int axis);
int vpic_hip_hydro_count(const vpic_hip_engine_t *e, int dir);       /* floats of a hydro face message (14 per node) */
int vpic_hip_pack_hydro(vpic_hip_engine_t *e, int dir, void *dev_buf);
int vpic_hip_unpack_hydro(vpic_hip_engine_t *e, int dir, const void *dev_buf);
int vpic_hip_set_hydro(vpic_hip_engine_t *e, const vpic_hydro_t *h);
int vpic_hip_get_hydro(vpic_hip_engine_t *e, vpic_hydro_t *h);

/* Payload of the reference's field_dump / hydro_dump (src/vpic/dump.cxx:1116-1364, 1366-1552), gathered
 * on the device so that only the selected, strided bytes cross PCIe.
 *   what   : VPIC_HIP_DUMP_FIELDS (records of 20 32-bit words) or VPIC_HIP_DUMP_HYDRO (16 words; the
 *            state left by accumulate_hydro_p / synchronize_hydro)
 *   layout : VPIC_HIP_DUMP_BAND        out = [nwords][nz/sz+2][ny/sy+2][nx/sx+2] words; word w of a
 *                                      record is taken as the reference does, `((uint32_t*)&rec)[w]`
 *                                      (w up to 23 for fields: 16-19 hold two material ids each, 20-23
 *                                      alias the next record, dump.cxx:1200-1203; past the last
 *                                      record they read as 0 here)
 *            VPIC_HIP_DUMP_INTERLEAVE  out = [nz/sz+2][ny/sy+2][nx/sx+2] whole records (dump.cxx:1331-1357)
 *            VPIC_HIP_DUMP_INTERLEAVE_INNER  hydro_dump's interleaved shape as written: [nz/sz][ny/sy]
 *                                      [nx/sx] records at offsets 0, s-1, 2s-1, ...; with unit strides
 *                                      the first nx*ny*nz records of the array (dump.cxx:1518-1543)
 * Output index i of an axis with n cells, n/s outputs: 0 -> 0, n/s+1 -> n+1, else i when all three
 * strides are 1 and i*s-1 otherwise -- also on an axis whose own stride is 1, as the reference does
 * (dump.cxx:1262-1273).  Strides must divide nx, ny, nz.  `out` is HOST memory of out_bytes. */
enum { VPIC_HIP_DUMP_FIELDS = 0, VPIC_HIP_DUMP_HYDRO = 1 };
enum { VPIC_HIP_DUMP_BAND = 0, VPIC_HIP_DUMP_INTERLEAVE = 1, VPIC_HIP_DUMP_INTERLEAVE_INNER = 2 };
int vpic_hip_dump_gather(vpic_hip_engine_t *e, int what, int layout, const int32_t *words, int nwords,
                         int sx, int sy, int sz, void *out, size_t out_bytes);

/* ---- the GPU-aware transport: RCCL point-to-point over xGMI, one rank per GPU ---------------------------------------
 * What the reference's port layer does with MPI (src/util/mp/dmp/mp_dmp.c:241-266 mp_begin_send / mp_begin_recv;
 * src/grid/grid_comm.c:7-78): a non-blocking send and receive per shared face, all faces posted together, waited for
 * where the data is needed.  Here the buffers are DEVICE memory (the engine's pack_* / exchange_pack_* outputs), the
 * transfers run on a communication stream of the communicator's own and are ordered against the engine's stream with
 * events: _start returns at once, _finish makes the ENGINE'S STREAM (not the host) wait.  The process launcher (MPI,
 * torch.distributed.run ...) only carries the 128-byte id from rank 0 to the others.  A rank may send to itself (the
 * reference self-sends across a periodic axis it owns alone, grid_comm.c:17-19,49): a 1-rank communicator is valid.
 * RCCL is loaded with dlopen by the first of these calls; one rank per device (RCCL refuses to share one). */
#define VPIC_HIP_COMM_ID_BYTES 128
typedef struct vpic_hip_comm vpic_hip_comm_t;
int vpic_hip_comm_unique_id(void *id128);                       /* rank 0; broadcast the bytes to every rank */
int vpic_hip_comm_create(vpic_hip_comm_t **c, vpic_hip_engine_t *e, const void *id128, int nranks, int rank);
int vpic_hip_comm_destroy(vpic_hip_comm_t *c);
/* post n_send + n_recv messages as ONE group behind everything the engine's stream holds so far; messages between a pair of
 * ranks match in the order listed (list by direction 0..5 on every rank); *token names the exchange for _finish (at most
 * 64 exchanges may be pending) */
int vpic_hip_comm_start(vpic_hip_comm_t *c, int n_send, const void *const *sbuf, const size_t *sbytes, const int *speer,
                        int n_recv, void *const *rbuf, const size_t *rbytes, const int *rpeer, int *token);
int vpic_hip_comm_finish(vpic_hip_comm_t *c, int token);        /* the engine's stream waits for that exchange */
int vpic_hip_comm_stats(vpic_hip_comm_t *c, int64_t *messages_sent, int64_t *bytes_sent);
/* timing of the exchanges with events (bench.py's `exchange` block): on = 1 starts and clears, 0 stops, -1 only reads; returns
 * the sums so far -- time on the communication stream, time the engine's stream stood still for the exchanges, their number
 * (call when the device is idle: it waits for the events) */
int vpic_hip_comm_timing(vpic_hip_comm_t *c, int on, double *exchange_ms, double *exposed_ms, int64_t *exchanges);

/* staging helpers for a host whose transport moves host memory (plain MPI): device scratch buffers
 * for the pack / unpack / inject calls above, and copies ordered after / before the engine's work */
void *vpic_hip_device_alloc(vpic_hip_engine_t *e, size_t bytes);
void vpic_hip_device_free(vpic_hip_engine_t *e, void *p);
int vpic_hip_copy_to_host(vpic_hip_engine_t *e, void *host, const void *dev, size_t bytes);
int vpic_hip_copy_from_host(vpic_hip_engine_t *e, void *dev, const void *host, size_t bytes);

/* one vpic_simulation::advance() of a domain that needs no other domain (src/vpic/advance.cxx:
 * 38-214: clear_accumulators, sort when due, advance_p all species, boundary_p, clear_jf, unload,
 * synchronize_jf, advance_b half, advance_e, advance_b half, load_interpolator).
 * sort_interval == 0: never sort; sort_interval < 0: ADAPTIVE, at the latest every -sort_interval
 * steps -- the engine times each species' sorts and pushes with HIP events and sorts a species again
 * as soon as its last push cost at least the average cost per step of the current cycle, the sort
 * included (sorting changes the array order only, not the physics). */
int vpic_hip_step(vpic_hip_engine_t *e, int64_t step, int sort_interval);

/* the adaptive decision for one species, for hosts that drive the steps themselves: *due = 1 when
 * species sp should be sorted before its next advance_p (first call: always; it also switches the
 * event timing of sort_p / advance_p on) */
int vpic_hip_sort_due(vpic_hip_engine_t *e, int sp, int max_interval, int *due);
int vpic_hip_measure_disorder(vpic_hip_engine_t *e, int sp, double *fraction);   /* descents of the voxel index / particle (sampled) */
/* The order the species' array is in: 0 = none known (loaded, uploaded, or moved on since a sort by voxel),
 * 1 = sorted by voxel and partition[] valid (sort_p.c:48-58), 2 = TILE order: grouped by 4x4x4-cell tile, what the
 * engine's own sort policy (vpic_hip_sort_due / vpic_hip_step with sort_interval < 0) gives a species whose particles
 * mostly leave their cell every step; advance_p then runs one workgroup per tile with the tile and its halo as LDS
 * window.  No result depends on the order; partition[] exists for order 1 only. */
int vpic_hip_species_sort_order(vpic_hip_engine_t *e, int sp, int *order);
/* what the engine knows about a species' last advance_p and its sorting, for diagnostics (bench.py, tools): out[0] particles
 * that left their cell, out[1] particles in the fullest tile at the last tile sort, out[2] runs of deposits that missed their
 * tile's LDS window, out[3] sorts so far, out[4] sorts vpic_hip_step made ahead of a fixed interval, out[5] 1 when the species
 * was found too clumped for the tile order, out[6] 1 when it is sorted by tile only, out[7] dead slots.  Values the device
 * publishes without being waited for: a launch or two old. */
int vpic_hip_species_stats(vpic_hip_engine_t *e, int sp, int64_t out[8]);
/* Who chooses the order vpic_hip_sort_p sorts into: 0 (default) = the reference's, by voxel (sort_p.c:48-58; partition[]
 * valid afterwards); 1 = the engine: TILE order for charged species of up to 2^30 particles.  A species whose sorts are
 * asked for by vpic_hip_sort_due's policy is sorted the engine's way in either mode. */
int vpic_hip_set_sort_order(vpic_hip_engine_t *e, int order);

/* HIP-event timing of the advance_p launches on the engine's stream (bench.py roofline leg) */
int vpic_hip_profile_enable(vpic_hip_engine_t *e, int on);
int vpic_hip_profile_read(vpic_hip_engine_t *e, double *advance_p_ms, int64_t *launches, int64_t *particles);
/* The same for the launches of advance_p that SORT the species as they push it (vpic_hip_step, fixed sort interval: a sort
 * that finds the counts the push before it took writes every particle to its sorted place instead of sorting first --
 * sort_p.c:48-101's result, one step stale, for 12 more bytes per particle): booked apart from the plain launches above. */
int vpic_hip_profile_read_sorting(vpic_hip_engine_t *e, double *advance_p_ms, int64_t *launches, int64_t *particles);
/* ... and the plain launches of ONE species (a deck whose species differ: charged against charge-0 tracer copies) */
int vpic_hip_profile_read_species(vpic_hip_engine_t *e, int sp, double *advance_p_ms, int64_t *launches, int64_t *particles);

#ifdef __cplusplus
}
#endif
#endif /* VPIC_HIP_H */
