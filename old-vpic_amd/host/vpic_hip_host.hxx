// vpic_hip_host.hxx -- a host for the reference's INPUT DECK API on top of the resident HIP engine.
//
// An input deck of the reference is C++ that is compiled INTO member functions of class
// vpic_simulation (src/deck_wrapper.cxx:16-36,541) and uses that class's members and helpers as
// free names (src/vpic/vpic.hxx:126-555).  This header provides a class of the same name with the
// members and helpers such decks use, so that a deck source file compiles unchanged against it:
//
//   hipcc/g++ -DINPUT_DECK=<deck.cxx> host/main.cxx host/deck_wrapper.cxx host/vpic_hip_host.cxx \
//       -Iinclude -Iold-vpic_amd/host -Lold-vpic_amd -lvpic_hip
//
// The time step (src/vpic/advance.cxx:13-244) runs on the GPU; the host arrays the deck can see
// (field, interpolator, species->p) are MIRRORS of the device state, kept coherent ON DEMAND: while the
// engine works they are inaccessible pages; the first access from a deck hook brings that array over,
// a first write marks it dirty, and when the hook returns dirty arrays go back to the device
// (vpic_hip_host.cxx, "host mirrors on demand").  A deck therefore reads and edits fields and particles
// in user_diagnostics / user_field_injection / user_current_injection / user_particle_injection /
// user_particle_collisions exactly as it does in the reference, and pays only for what it touches;
// species->np is current in every hook.  The library announces every host range a HIP copy is about to touch
// (vpic_hip_set_host_access_hook), so a twin handed one of these arrays finds it resident.
//
// Scope: box decks -- periodic, conducting/reflecting or absorbing faces (define_periodic_grid /
// define_reflecting_grid / define_absorbing_grid, set_domain_*_bc) -- on one rank or, built with
// -DVPIC_HIP_HOST_MPI, cut into gpx x gpy x gpz equal bricks over MPI ranks (one GPU each); any number of species, also
// species a deck takes off species_list and advances itself (tracers); any number of materials
// (anisotropic eps / mu / sigma, set_region_material); set_region_field; divergence cleaning; every
// dump of the reference (energies, fields, hydro, particles, grid, species, materials, the strided
// field_dump / hydro_dump with their .vpc header) and restart files (dump_restart, `restart <fbase>`).
// Particles a deck injects while the run is under way (inject_particle / inject_particle_raw from
// user_particle_injection) reach the device at the end of that call.  The custom particle boundaries the reference ships
// (add_boundary): maxwellian_reflux, absorb_tally and link_boundary; surface emitters with the child_langmuir / ccube / ivory laws.
// Not there: particle boundary handlers of a deck's own, set_region_bc.  Unsupported calls stop with the reference's ERROR convention (message, exit(1)).
// uniform_rand() is the reference's generator (MT19937 + its 53-bit open-interval conversion,
// src/util/mtrand/mtrand.c:69-76,240, mtrand_conv.h:61); maxwellian_rand() uses Box-Muller on it
// instead of the reference's 256-layer ziggurat (whose tables are a data file of the reference), so
// decks that draw normals load statistically equivalent, not identical, particles.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>
#include <map>

#include "vpic_hip.h"
#include "vpic_hip_dropin.h"
#include "FileIO.hxx"

// ---- the reference's type names ---------------------------------------------------------------
typedef vpic_particle_t particle_t;
typedef vpic_particle_mover_t particle_mover_t;
typedef vpic_particle_injector_t particle_injector_t;
typedef vpic_interpolator_t interpolator_t;
typedef vpic_accumulator_t accumulator_t;
typedef vpic_field_t field_t;
typedef vpic_material_coefficient_t material_coefficient_t;
typedef vpic_grid_t grid_t;
typedef vpic_species_t species_t;
typedef uint16_t material_id;
enum { invalid_material_id = 65535 };
typedef int32_t species_id;

enum { anti_symmetric_fields = -1, pec_fields = -1, metal_fields = -1, symmetric_fields = -2,
       pmc_fields = -3, absorb_fields = -4, reflect_particles = -1, absorb_particles = -2 };
#define BOUNDARY(i, j, k) (((i) + 1) + 3 * (((j) + 1) + 3 * ((k) + 1)))
#define INDEX_FORTRAN_3(x, y, z, xl, xh, yl, yh, zl, zh) \
  ((x) - (xl) + ((xh) - (xl) + 1) * ((y) - (yl) + ((yh) - (yl) + 1) * ((z) - (zl))))
#define LIST_FOR_EACH(n, list) for ((n) = (list); (n) != NULL; (n) = (n)->next)

#define ERROR(args) do { fprintf(stderr, "Error at %s(%i):\n\t", __FILE__, __LINE__); vpic_host_log args; fprintf(stderr, "\n"); exit(1); } while (0)
#define WARNING(args) do { fprintf(stderr, "Warning at %s(%i):\n\t", __FILE__, __LINE__); vpic_host_log args; fprintf(stderr, "\n"); } while (0)
#define MESSAGE(args) do { fprintf(stderr, "%s(%i): ", __FILE__, __LINE__); vpic_host_log args; fprintf(stderr, "\n"); } while (0)
void vpic_host_log(const char *fmt, ...);
// demand-mode mirrors: make a block safe to hand to the kernel (write / fwrite) -- see vpic_hip_host.cxx
void vpic_host_touch(const void *p, size_t bytes);
inline size_t vpic_host_fwrite(const void *p, size_t size, size_t n, FILE *f) { vpic_host_touch(p, size * n); return fwrite(p, size, n, f); }
#define BEGIN_PRIMITIVE do
#define END_PRIMITIVE while (0)

// src/field_advance/field_advance.h:185-302: the slots a deck can reach through
// field_advance->method (hot slots are the HIP twins; the rest is not on the path yet)
struct field_advance_methods_t {
  void (*advance_b)(field_t *, const grid_t *, float);
  void (*advance_e)(field_t *, const material_coefficient_t *, const grid_t *);
  void (*energy_f)(double *, const field_t *, const material_coefficient_t *, const grid_t *);
  void (*clear_jf)(field_t *, const grid_t *);
  void (*synchronize_jf)(field_t *, const grid_t *);
};
extern field_advance_methods_t standard_field_advance[1];
struct field_advance_t {
  field_t *f;
  material_coefficient_t *m;
  grid_t *g;
  field_advance_methods_t method[1];
};

// energy_p with the reference's signature (src/species_advance/standard/spa.h:101-106).  When the
// arrays are the simulation's own mirrors it is answered from the resident state (no transfer).
double energy_p(const particle_t *p0, int np, float q_m, const interpolator_t *f0, const grid_t *g);

struct mt_rng_t { uint32_t state[624]; int next; };

// ---- field_dump / hydro_dump vocabulary of the decks (src/vpic/vpic.hxx:44-124, src/util/BitField.hxx) ----
// bit k of a field mask selects 32-bit word k of field_t, of a hydro mask word k of hydro_t
const uint32_t all = 0xffffffff;
const uint32_t electric = 7u << 0, div_e_err = 1u << 3, magnetic = 7u << 4, div_b_err = 1u << 7, tca = 7u << 8,
               rhob = 1u << 11, current = 7u << 12, rhof = 1u << 15, emat = 7u << 16, nmat = 1u << 19,
               fmat = 7u << 20, cmat = 1u << 23;
const uint32_t current_density = 7u << 0, charge_density = 1u << 3, momentum_density = 7u << 4, ke_density = 1u << 7,
               stress_tensor = 63u << 8;
const size_t total_field_variables = 24, total_field_groups = 12, total_hydro_variables = 14, total_hydro_groups = 5;

class BitField {
  uint32_t bits_;
public:
  BitField(uint32_t setbits = 0xffffffff) : bits_(setbits) {}
  uint32_t set(uint32_t mask) { return bits_ |= mask; }
  uint32_t clear(uint32_t mask) { return bits_ &= ~mask; }
  uint32_t setbit(size_t bit) { return bits_ |= (uint32_t)1 << bit; }
  uint32_t clearbit(size_t bit) { return bits_ &= ~((uint32_t)1 << bit); }
  bool bitset(size_t bit) const { return (bits_ >> bit) & 1u; }
  bool bitclear(size_t bit) const { return !bitset(bit); }
  size_t bitsum(const size_t *indeces, size_t size) const { size_t n = 0; for (size_t i = 0; i < size; i++) n += bitset(indeces[i]); return n; }
  size_t bitsum() const { size_t n = 0; for (size_t i = 0; i < 32; i++) n += bitset(i); return n; }
};
enum DumpFormat { band = 0, band_interleave = 1 };
struct DumpParameters {
  void output_variables(uint32_t mask) { output_vars.set(mask); }   // ORs into the default all-ones mask, as the reference does
  BitField output_vars;
  size_t stride_x, stride_y, stride_z;
  DumpFormat format;
  char name[128], baseDir[128], baseFileName[128];
};

// ---- the L3 entry points decks call directly (tracer decks: decks/trecon-part/tracer.cxx:76-107) ----
// Same signatures as the reference (species_advance.h:103-122, spa.h:23-66, sf_interface.h:112-114).
// When the arrays belong to a species of the running simulation the work is done on the resident
// engine (no PCIe traffic): advance_p launches that species' push and returns 0 (the movers stay on
// the device); boundary_p runs the engine's particle exchange for every resident species that has
// movers pending (a no-op when none has: the deck's repeated calls cost nothing); sort_p sorts on
// the device.  For any other arrays the drop-in twins of vpic_hip_dropin.h run (arrays over PCIe).
species_t *new_species(const char *name, float q_m, int max_local_np, int max_local_nm, int sort_interval,
                       int sort_out_of_place, species_t **sp_list);
species_t *find_species_id(species_id id, species_t *sp_list);
species_t *find_species_name(const char *name, species_t *sp_list);
accumulator_t *new_accumulators(const grid_t *g);
int advance_p(particle_t *p0, int np, const float q_m, particle_mover_t *pm, int max_nm, accumulator_t *a0,
              const interpolator_t *f0, const grid_t *g);
void boundary_p(species_t *sp_list, field_t *f, accumulator_t *a0, const grid_t *g, mt_rng_t *rng);
void sort_p(species_t *sp, const grid_t *g);

// Custom particle boundary handlers (src/boundary/boundary.h, src/grid/grid.h:170-190): a deck fills a
// maxwellian_reflux_t, registers it with add_boundary( grid, maxwellian_reflux, &params ) and gives the code it
// gets back (<= -3) to set_domain_particle_bc.  maxwellian_reflux here is only the handler's NAME: the work is
// done on the device (vpic_hip_set_maxwellian_reflux).
// absorb_tally and link_boundary (boundary.h:35-59) are absorbing walls that tally and record on the device
// (include/vpic_hip.h: vpic_hip_wall_*).  Codes are -(k + 3) in registration order across all kinds (add_boundary.c:31);
// grid->boundary[k].params holds the copy of handler k's parameters, which a deck reads as in the reference:
//   ((absorb_tally_t *)grid->boundary[-code - 3].params)->nabs[j]
// nabs is brought up to date once per step, after the step's particle exchange: for the species in id[], the particles
// absorbed at the faces of this domain that carry the handler's code; a species absorbed there that is not in id[] stops
// the run with the reference's message.  link_boundary writes the reference's file, <fbase>.<rank>, created at the first
// step that absorbs something there (a file that already exists stops the run), "%% %17.0f\n" of n_out at that moment and
// one line "%d %e %e %e %e %e %e %e\n" per particle (species id, x, y, z, ux, uy, uz, q; link.c:53-67); n_out grows by the
// lines written.  As in the reference the file is ONE per process: a second link handler writes into the first one's.
// Other handlers are refused.
// LIMIT: the engine serves 4 wall codes (VPIC_HIP_WALL_MAX).  A deck may register up to 4 absorb_tally / link_boundary
// handlers in all (maxwellian_reflux handlers do not count; they have 4 of their own); a fifth stops the run at its start
// with a message that says so.  With fewer than 4 the plainly absorbing faces (absorb_particles) are tallied face by face
// as well; with exactly 4 there is no code left for them: what they absorb is counted under face 6 with the movers no
// face took, a warning says so at the start, and wall_tally() for such a face stops the run instead of answering zero.
// The quanta of the walls' exact sums (vpic_hip_wall_setup) are chosen when the run starts from the largest |q| loaded
// on any rank, qmax (1 when nothing is charged): charge in units of qmax 2^-30, q * ke in units of qmax 2^-24 -- no
// loaded charge can be refused, nor one four times heavier, nor q * ke below ke = 256; what is refused all the same is
// reported in the closing timing line.
typedef struct maxwellian_reflux { float ut_perp[32], ut_para[32]; } maxwellian_reflux_t;
typedef struct absorb_tally { int nspec; species_id id[32]; int nabs[32]; } absorb_tally_t;
typedef struct link_boundary { char fbase[256]; double n_out; } link_boundary_t;
typedef void (*boundary_handler_t)(void);
typedef vpic_boundary_t boundary_t;
void maxwellian_reflux(void);
void absorb_tally(void);
void link_boundary(void);
int vpic_host_add_boundary(grid_t *g, boundary_handler_t handler, const void *params, int size);
#define add_boundary(g, bh, ip) vpic_host_add_boundary((g), (boundary_handler_t)(bh), (ip), (int)sizeof(*(ip)))

// Surface emitters (src/emitter/emitter.h, emitter.c:5-73; deck macros define_surface_emitter / define_volume_emitter):
// an emitter is a list of (voxel, face) components, a species and an emission model with its parameters.  The
// three models of the reference -- child_langmuir, ccube, ivory -- are NAMES here; vpic_simulation::advance
// runs them on the device (vpic_hip_emit) where the reference calls them (advance.cxx:83-84).
#define COMPONENT_ID(local_cell, component_type) (((local_cell) << 5) | (component_type))
#define EXTRACT_LOCAL_CELL(component_id) ((component_id) >> 5)
#define EXTRACT_COMPONENT_TYPE(component_id) ((component_id) & 31)
#define MAX_EMISSION_MODEL_SIZE 1024
typedef void (*emission_model_t)(void);
typedef struct emitter {
  int *component;
  int n_component, max_component;
  species_t *sp;
  emission_model_t emission_model;
  char model_parameters[MAX_EMISSION_MODEL_SIZE];
  struct emitter *next;
  char name[1];
} emitter_t;
typedef struct child_langmuir { int n_emit_per_face; float ut_perp, ut_para; } child_langmuir_t;
typedef struct ccube { int n_emit_per_face; float ut_perp, ut_para, thresh_e_norm; } ccube_t;
typedef struct ivory { int n_emit_per_face; float ut_perp, ut_para, thresh_e_norm; } ivory_t;
void child_langmuir(void);
void ccube(void);
void ivory(void);
emitter_t *new_emitter(const char *name, species_t *sp, emission_model_t emission_model, int max_component, emitter_t **e_list);
emitter_t *find_emitter_name(const char *name, emitter_t *e_list);

// the mp_* calls decks make on grid->mp (src/util/mp/mp.h): elapsed wall clock (max over ranks),
// barrier, finalize, the blocking int send / receive of the turnstile macros
double mp_elapsed(void *mp);
void mp_barrier(void *mp);
void mp_finalize(void *mp);
void mp_send_i(int *buf, int n, int dst, void *mp);
void mp_recv_i(int *buf, int n, int src, void *mp);

// message passing between domains (vpic_hip_host.cxx): with -DVPIC_HIP_HOST_MPI one MPI rank per
// domain / GPU, brick decompositions; without it a single domain
void vpic_host_mp_init(int *argc, char ***argv);
void vpic_host_mp_finalize(void);
int vpic_host_mp_rank(void);
int vpic_host_mp_nproc(void);

class vpic_simulation {
public:
  vpic_simulation();
  ~vpic_simulation();
  void initialize(int argc, char **argv);
  void restart(const char *fbase);          // continue from the files dump_restart wrote (main: `deck.exe restart <fbase>`)
  int advance(void);
  void finalize(void);
  void sync(void) { if (engine) vpic_hip_sync(engine); }   // wait for the device (main: before the wall clock is read)
  inline double rank(void) { return vpic_host_mp_rank(); }
  inline double nproc(void) { return vpic_host_mp_nproc(); }

  // ---- what decks use as free names (src/vpic/vpic.hxx:151-555) ------------------------------
  int verbose, step, num_step, num_comm_round, status_interval;
  int clean_div_e_interval, clean_div_b_interval, sync_shared_interval;
  double quota;
  int restart_interval, hydro_interval, field_interval, particle_interval;
  mt_rng_t *rng;
  grid_t *grid;
  species_t *species_list;
  emitter_t *emitter_list;
  field_advance_t *field_advance;
  field_t *field;
  interpolator_t *interpolator;
  accumulator_t *accumulator;
  char user_global[16384];

  // HIP-specific knobs a deck may set (defaults can also come from the environment:
  // VPIC_HIP_MIRROR_INTERVAL, VPIC_HIP_ADAPTIVE_SORT)
  int hip_mirror_interval;      // kept for restart files of earlier versions (unused)
  int hip_adaptive_sort;        // 1 (default): the engine decides when a species is sorted (vpic_hip_sort_due), the deck's
                                // sort_interval is the upper bound; 0: exactly every sort_interval steps
  void hip_sync_mirrors(void);  // refresh them now
  void hip_upload_mirrors(void);// push host-side edits of field / particles back to the device
  void mirror_download(int kind, int sp);   // demand mode (VPIC_HIP_MIRROR=demand), see vpic_hip_host.cxx

  void define_periodic_grid(double xl, double yl, double zl, double xh, double yh, double zh,
                            double gnx, double gny, double gnz, double gpx, double gpy, double gpz);
  void define_reflecting_grid(double xl, double yl, double zl, double xh, double yh, double zh,
                              double gnx, double gny, double gnz, double gpx, double gpy, double gpz);
  void define_absorbing_grid(double xl, double yl, double zl, double xh, double yh, double zh,
                             double gnx, double gny, double gnz, double gpx, double gpy, double gpz, int pbc);
  void set_domain_field_bc(int boundary, int fbc);
  void set_domain_particle_bc(int boundary, int pbc);
  material_id define_material(const char *name, double eps, double mu = 1, double sigma = 0, double zeta = 0);
  material_id define_material(const char *name, double epsx, double epsy, double epsz, double mux, double muy, double muz,
                              double sigmax, double sigmay, double sigmaz, double zetax = 0, double zetay = 0, double zetaz = 0);
  material_id lookup_material(const char *name);
  void finalize_field_advance(field_advance_methods_t *fam = standard_field_advance);
  species_t *define_species(const char *name, double q_m, double max_local_np, double max_local_nm,
                            double sort_interval, double sort_out_of_place);
  species_t *find_species(const char *name);
  void inject_particle(species_t *sp, double x, double y, double z, double ux, double uy, double uz,
                       double q, int64_t tag, double age = 0, int update_rhob = 1);
  void inject_particle_raw(species_t *sp, float dx, float dy, float dz, int32_t i, float ux, float uy, float uz, float q);
  void seed_rand(double seed);
  double uniform_rand(double low, double high);
  double maxwellian_rand(double dev);
  void dump_energies(const char *fname, int append = 1);
  // binary dumps with the V0 header (dump.cxx:190-329, dumpmacros.h:10-48): same bytes as the
  // reference writes for the same state; particles are time-centred by center_p on the way out
  void dump_fields(const char *fbase, int ftag = 1);
  void dump_hydro(const char *sp_name, const char *fbase, int ftag = 1);
  void dump_particles(const char *sp_name, const char *fbase, int ftag = 1);
  // text / grid dumps (dump.cxx:82-187) and the strided, banded dumps read by the reference's
  // visualisation tools (dump.cxx:929-1552); the field / hydro payloads are gathered on the device
  void dump_species(const char *fname);
  void dump_materials(const char *fname);
  void dump_grid(const char *fbase);
  int dump_mkdir(const char *dname);
  int dump_cwd(char *dname, size_t size);
  void global_header(const char *base, std::vector<DumpParameters *> dumpParams);
  void create_field_list(char *strlist, DumpParameters &dumpParams);
  void create_hydro_list(char *strlist, DumpParameters &dumpParams);
  void dump_restart(const char *fbase, int fname_tag = 1);
  void field_dump(DumpParameters &dumpParams);
  void hydro_dump(const char *speciesname, DumpParameters &dumpParams);
  // ... of the particles a selection keeps (vpic_hip_accumulate_hydro_p_select, include/vpic_hip.h): the same file -- header,
  // strides, band or interleave -- holding the moments of the kept particles only.  Position ranges are in PHYSICAL units,
  // converted as select_particles() converts them; ranges in the frame of the local field pass through untouched and, like
  // every range, look at the stored momenta and at the interpolator on the device as it stands at that point of the step.
  // Every rank sums its own particles and synchronize_hydro joins the faces as for the whole species.  The particle
  // mirror does not become resident.
  void hydro_dump(const char *speciesname, DumpParameters &dumpParams, const vpic_hip_select_t *s);
  size_t px, py, pz;            // domain topology (vpic.hxx:171)
  inline double courant_length(double lx, double ly, double lz, double nx, double ny, double nz) {
    double w0, w1 = 0;
    if (nx > 1) w0 = nx / lx, w1 += w0 * w0;
    if (ny > 1) w0 = ny / ly, w1 += w0 * w0;
    if (nz > 1) w0 = nz / lz, w1 += w0 * w0;
    return sqrt(1 / w1);
  }
  inline double trunc_granular(double a, double b) { return b * int(a / b); }

  // resident-engine answers for diagnostics on the simulation's own arrays
  bool owns(const particle_t *p0) const;
  int resident_id(const particle_t *p0) const;      // engine species id of a resident particle array, or -1
  vpic_hip_engine_t *resident_engine(void) { return engine; }
  void resident_advance_p(int id);                  // push one resident species; its movers wait for ...
  void resident_boundary_p(void);                   // ... the exchange of every resident species with pending movers
  double resident_energy_p(const particle_t *p0);
  // What the absorbing walls of this domain took of a species since the run began (restarts included): face 0..5 (-x -y -z
  // +x +y +z), where that face carries an absorb_tally or link_boundary handler or -- in a deck that has such a handler --
  // is plainly absorbing; face 6: every other particle absorbed.  count, charge (the sum of q) and energy (the sum of
  // q * ke, ke = gamma - 1) in the deck's units, from exact integer sums (include/vpic_hip.h).  Any pointer may be NULL.
  // Zero throughout in a deck without such handlers.  A plainly absorbing face of a deck with 4 handlers is not tallied
  // by itself (LIMIT above): asking for it is an ERROR.
  void wall_tally(int face, species_t *sp, int64_t *count, double *charge, double *energy);
  // The energy diagnostic of the production deck (decks/trecon-part/energy.cxx:89-162) from the resident state, in place
  // of a loop over sp->p, which would download the whole species: bands[k * nv + voxel] (nex * nv floats, or NULL) the
  // share of the voxel's particles in each of nex linear bands of width dke, ghost voxels filled from their interior
  // neighbours; spectrum[k] (nbin floats, or NULL) the particles per bin of width dloge in log10(ke) above log_lo =
  // log10(eminp).  The particle mirror does not become resident.  Counted as include/vpic_hip.h says
  // (vpic_hip_energy_spectrum): in integers -- the floats written here equal the reference's while every count is
  // below 2^24, where the reference's float counters stop.  Only once the run has started (the engine owns the particles).
  void energy_spectrum(species_t *sp, int nex, double dke, float *bands, int nbin, double log_lo, double dloge, float *spectrum);
  // A 1-D or 2-D histogram of a species over position, momentum and kinetic energy, of the particles inside up to four
  // ranges, from the resident state (vpic_hip_species_distribution, include/vpic_hip.h: the descriptor, the arithmetic,
  // counts[b1 * n0 + b0]).  Unlike the C ABI this takes PHYSICAL units for position axes and ranges (lo, d, hi of an X, Y
  // or Z coordinate in the units of grid->x0 and grid->dx); they are converted to the cells of this rank's domain as
  // (lo - grid->x0) / grid->dx and d / grid->dx, in double.  counts[] holds this rank's particles only: every rank bins
  // against the same physical edges and integer counts add exactly, so a deck on several ranks sums them (as energy.cxx
  // does with its own).  The particle mirror does not become resident.  Only once the run has started.
  // The coordinates in the frame of the local magnetic field -- VPIC_HIP_COORD_U_PAR, _U_PERP, _PITCH, _MU, _B, _E_PAR, as
  // axes and as ranges, here and in select_particles -- are passed through untouched (they have no physical-unit form:
  // momenta are u, cB and E are in the units the field array holds).  They use the interpolator on the device, which
  // advance() has loaded for the current fields when user_diagnostics runs, and the stored momenta.
  void distribution(species_t *sp, const vpic_hip_dist_t *d, uint64_t *counts);
  // The same histogram with up to four per-bin sums of particle quantities beside it, as exact integers
  // (vpic_hip_species_distribution_sums, include/vpic_hip.h: the factors, the arithmetic, the quantum, the refusals;
  // sums[k * n0*n1 + b1*n0 + b0], counts may be NULL).  Axes and ranges are in PHYSICAL units, converted exactly as
  // distribution() converts them.  The FACTORS pass through in engine units: momenta are u, VPIC_HIP_FACTOR_Q is the
  // particle's q as stored, E and cB are in the units the field array holds -- and a position used as a factor is in LOCAL
  // CELLS of this rank's domain (it has no origin), so a deck that wants a moment in x forms it from the bins.  This rank's
  // particles only: int64 sums of several ranks add exactly, in any order (MPI_SUM over MPI_INT64_T), as the counts do.
  // A particle refused for a value (|value / quantum| >= 2^32, or NaN) is reported by vpic_hip_species_distribution_sums_stats,
  // not by this call.  The particle mirror does not become resident.  Only once the run has started.
  void distribution_sums(species_t *sp, const vpic_hip_dist_t *d, const vpic_hip_dist_value_t *v, int n_val, uint64_t *counts, int64_t *sums);
  // A 1-D or 2-D histogram over the CELLS of this rank's domain with up to four exact per-bin sums beside it, from the
  // field and hydro arrays on the device, in place of a loop over field(x,y,z) that downloads the whole array
  // (vpic_hip_cell_distribution, include/vpic_hip.h: the VPIC_HIP_CELL_* codes, the arithmetic, the quantum, the refusals;
  // counts[b1 * n0 + b0] or NULL beside values, sums[k * n0*n1 + b1*n0 + b0], n_val 0 to 4).  Axes and ranges over
  // VPIC_HIP_CELL_X, _Y, _Z are in PHYSICAL units -- the cell's centre, grid->x0 + (cx - 0.5) grid->dx -- converted exactly as
  // distribution() converts them; every other code is in the units the arrays hold, and a position used as a FACTOR is in
  // local cells.  The hydro codes read the hydro array as the last hydro_dump / dump_hydro left it.  The field array is the
  // device's: what a hook has written to `field` reaches it when the hook returns.  This rank's cells only: every rank bins
  // against the same physical edges, and int64 sums of several ranks add exactly, in any order (MPI_SUM over MPI_INT64_T),
  // as the counts do.  Cells refused for a value are reported by vpic_hip_cell_distribution_stats.  No mirror becomes
  // resident.  Only once the run has started.
  void cell_distribution(const vpic_hip_dist_t *d, const vpic_hip_dist_value_t *v, int n_val, uint64_t *counts, int64_t *sums);
  // The particles of a species inside up to four ranges and with the tags asked for, from the resident state, in place of
  // a loop over sp->p that tests every particle (vpic_hip_species_select, include/vpic_hip.h: the descriptor, the order,
  // the arithmetic of the fields).  Returns how many particles are kept; the first min(that, cap) of them are written, in
  // the order of the species' array: p[k] the particle, fields[6k .. 6k+5] ex, ey, ez, cbx, cby, cbz at it from the
  // interpolator as it stands on the device, index[k] its place in the device's array (not in sp->p once that has been
  // downloaded: a download drops dead slots).  Any of the three may be NULL.  Position ranges are in PHYSICAL units,
  // converted as distribution() converts them.  This rank's particles only.  The particle mirror does not become resident.
  // Only once the run has started.
  int64_t select_particles(species_t *sp, const vpic_hip_select_t *s, int64_t cap, particle_t *p, float *fields, int64_t *index);
  // Binary Coulomb collisions (Takizuka & Abe) of the particles of species a among themselves (b NULL or a) or with those of
  // b, cell by cell on the device (vpic_hip_collide, include/vpic_hip.h: the model, the pairing, the arithmetic, the limits --
  // non-relativistic unless prm.relativistic, rank-local, at most VPIC_HIP_COLLIDE_MAX_CELL particles of a species per cell).  For
  // begin_particle_collisions: the call does its work on the steps that are multiples of prm.interval and returns at once
  // on the others; the host derives wq = 1 / |charge|, dt = interval * grid->dt and the stream's call counter = step.  What
  // a hook has written to sp->p before the call reaches the device first; afterwards the particle mirrors are stale like
  // after a push, and none is brought to the host.  A species whose cells are not exact ranges of its array (any that was
  // pushed since its sort) is sorted by the call, and a sort that was due this step is then not made again.
  struct collide_params_t {
    double m_a, m_b;          // mass of a physical particle of a, of b (b == a: m_b and q_b are not read)
    double q_a, q_b;          // charge of a physical particle (the macro-particle's weight is |q| / |charge|)
    double cvar;              // (q_a q_b)^2 ln(Lambda) / (8 pi eps0^2 c^3) in the deck's units
    int interval;             // collide every `interval` steps, for the time interval * dt
    unsigned seed;
    int relativistic;         // 0: vpic_hip_collide (|u| << 1); non-zero: vpic_hip_collide_relativistic (hot plasmas; include/vpic_hip.h gives the range of |u|).  An initialiser of seven values leaves it 0
  };
  void collide(species_t *a, species_t *b, const collide_params_t &prm);
  // Radiative cooling of a species on the device: synchrotron losses and the Compton drag of an isotropic photon bath
  // (vpic_hip_species_cool, include/vpic_hip.h: the model, the arithmetic, its range of validity), in place of a hook that
  // walks sp->p and the interpolator on the host.  For begin_particle_collisions: the call does its work on the steps that
  // are multiples of prm.interval, for the time interval * grid->dt, and returns at once with 0 on the others.  Returns the
  // energy the drag took from the species, sum |q| (gamma - gamma'), as isum * quantum: an exact integer sum, so the
  // returns of the ranks add exactly; cell_energy (grid->nv words, or NULL) takes the same per voxel in units of quantum.
  // With dry the tallies are returned and no momentum is written.  What a hook has written to sp->p or to the interpolator
  // before the call reaches the device first; afterwards the particle mirrors are stale like after a push, and none is
  // brought to the host.  Running totals are the deck's business: its globals travel in the restart file.
  struct cool_params_t {
    double sync_rate;         // tau0 (q / m c)^2 per unit time, tau0 = q^2 / (6 pi eps0 m c^3) of a physical particle
    double ic_rate;           // (4/3) sigma_T U_ph / (m c) per unit time
    int interval;             // cool every `interval` steps, for the time interval * dt
    double quantum;           // the unit of the integer sums
    int dry;                  // non-zero: tally only
  };
  double cool(species_t *sp, const cool_params_t &prm, int64_t *cell_energy = NULL);
  int64_t particle_mirror_downloads(void) const;    // whole-species downloads into the host mirrors so far (diagnostics, tests)
  int64_t particle_mirror_uploads(void) const;      // particles that went from a host mirror to the device so far
  // A species loaded on the device from per-cell tables (vpic_hip_species_load_profile, include/vpic_hip.h: THE RULE, the
  // flags, what is refused): what a deck's `repeat( n ) inject_particle( ... )` loop over a profile does, without a host
  // record per particle.  The tables are this rank's own (tdim: 1 or the local grid's extent per axis); the host fills
  // gdim and goff from its place in the decomposition, so every rank's particles are those of the uncut run.  Usable from
  // begin_initialization (carried out when the run starts, behind the upload of what the deck injected on the host; the
  // tables are copied) and from the hooks (carried out at once).  sp->np follows; sp->p goes stale, as after a push.
  void load_species_profile(species_t *sp, const vpic_hip_load_t &d);
  bool resident_energy_f(double *en, const field_t *f);

private:
  vpic_hip_engine_t *engine;
  std::vector<species_t *> species_order;    // engine species id = position
  std::vector<vpic_material_coefficient_t> materials;
  struct material_rec { std::string name; float eps[3], mu[3], sigma[3]; };
  std::vector<material_rec> material_records;
  void banded_dump(int what, int dump_type, int sp_id, float q_m, DumpParameters &dumpParams);
  bool mirrors_current;
  bool movers_pending;          // a push has run since the last particle exchange
  std::vector<char> sort_pending;   // species whose sort is due and not yet carried out (advance(): done by the push or by the first look at the species)
  void pending_sort(int id);
  std::vector<std::vector<particle_t> > injected;   // particles a deck injects while the run is under way, per species
  std::vector<particle_injector_t> injected_aged; std::vector<int64_t> injected_aged_tags;   // ... with an age (misc.cxx:93-103)
  std::vector<particle_t> injected_rhob;            // ... those whose charge, negated, goes to rhob (update_rhob)
  void flush_injected(void);
  void run_emitters(void);
  struct profile_load_t { species_t *sp; vpic_hip_load_t d; std::vector<int32_t> count; std::vector<float> tab[7]; };   // q, ud x y z, uth x y z
  std::vector<profile_load_t> pending_loads;        // load_species_profile calls made before the engine existed
  void run_profile_load(const profile_load_t &l);
public:
  int boundary_kind(int k) const;                   // of grid->boundary[k]: 0 maxwellian_reflux, 1 absorb_tally, 2 link_boundary
  int n_boundaries(int kind) const;
private:
  // absorbing walls (absorb_tally, link_boundary): the codes of this domain's faces, the quanta, the totals since the run
  // began as [7][species] {count, isum q, isum q ke, refused q, refused q ke}, and the records' staging buffer
  int wall_pbc[6]; bool walls_on, plain_faces_tallied; double wall_quantum[2]; int64_t wall_record_cap;
  std::vector<int64_t> wall_totals;
  std::vector<vpic_hip_wall_record_t> wall_records;
  void start_walls(void);
  void refresh_walls(void);                         // once per step: nabs, the link file
  void queue_injected(species_t *sp, const particle_t &p);
  void box(double xl, double yl, double zl, double xh, double yh, double zh, int nx, int ny, int nz, int pbc, int fbc);
  void slab(double gx0, double gy0, double gz0, double gx1, double gy1, double gz1, int gnx, int gny, int gnz,
            int gpx, int gpy, int gpz, int pbc, int fbc, bool periodic);
  // exchanges with the neighbouring domains (vpic_hip_host.cxx); face_rank[f] = rank sharing face f (this rank itself when
  // it sends to itself across a periodic axis), or -1
  int face_rank[6];
  int hip_transport;                        // XPORT_*: none, MPI with host staging, RCCL on device buffers
  bool hip_deterministic;                   // fixed-point accumulation (VPIC_HIP_DETERMINISTIC; the default of decks that clean div E)
  bool hip_resident_exchange;               // particle exchange: device-resident and overlapped with the push / the reference's protocol
  vpic_hip_comm_t *comm;
  struct XBuf { void *dev; size_t bytes; std::vector<char> host; XBuf() : dev(NULL), bytes(0) {} };
  std::map<int, XBuf> xbufs;                // device message buffers (and their host twins for the staged transport) by (kind, direction, tag)
  void *xbuf(int kind, int d, int tag, size_t bytes);
  std::vector<char> &xhost_of(void *dev);
  struct XferSet { const void *s[6]; size_t ns[6]; void *r[6]; size_t nr[6]; };   // by travel direction; 0 bytes: no message
  int x_start(const XferSet &x);
  void x_finish(int token);
  template <class Pack, class Unpack> void plane_exchange(int axis, size_t bytes, Pack pack, Unpack unpack, int tag = 50);
  struct XRound { int token, tag; void *ms[6], *mr[6]; int cs[6], cr[6]; };
  struct XHeader { int kind, tag, d, count, wanted; };
  std::map<int, int> x_caps;                // message capacities (injectors) by (kind, direction, species or -1)
  std::vector<double> x_np_max;
  int x_mover_cap, x_flags; long x_messages, x_syncs, x_recoveries;
  int &x_cap(int kind, int d, int k);
  XRound x_round(int tag, const int cs[6], const int cr[6], int mover_cap, uint32_t species_mask);
  void x_land(const XRound &r);
  void x_read_back(const std::vector<XRound> &log, std::vector<XHeader> &H);
  void x_recover(std::vector<XHeader> &H);
  void x_make_room(void);
  void x_exchange_rounds(int rounds);
  void x_push_and_exchange(const std::vector<char> &listed);
  void x_advance_e(void);
public:
  const char *transport_name(void) const;
private:
  bool shared(int axis) const;              // the faces of this axis (one or both) belong to other ranks
  bool multi(void) const;
  int topo_index[3], topo_size[3];          // this rank's brick in the gpx x gpy x gpz decomposition
  void x_boundary_p(void);
  void x_tang_b(void);
  struct XFamily {                          // the public C functions of a message family that is summed over shared planes
    int (*whole)(vpic_hip_engine_t *), (*adjust)(vpic_hip_engine_t *), (*count)(const vpic_hip_engine_t *, int);
    int (*pack)(vpic_hip_engine_t *, int, void *), (*unpack)(vpic_hip_engine_t *, int, const void *), (*self)(vpic_hip_engine_t *, int);
  };
  void x_synchronize(const XFamily &f);
  void x_synchronize_jf(void);
  void x_synchronize_rho(void);
  void x_synchronize_hydro(void);
  double x_message(int kind);
  double x_message(int kind, int axis);
  double x_synchronize_tang_e_norm_b(void);
  double x_rms(bool e_field);
  void x_accumulate_rho(void);
  void x_compute_div_e_err(void);
  void x_compute_rhob(void);
  void x_clean_div_b(void);
  void x_compute_curl_b(void);
  void describe(vpic_hip_grid_t &d);
  void create_engine(void);
  void start_demand_mirrors(void);
  void mirrors_stale(void);
  void mirrors_after_user_code(void);

  // the deck's bodies (src/deck_wrapper.cxx:16-36)
  void user_initialization(int argc, char **argv);
  void user_particle_injection(void);
  void user_current_injection(void);
  void user_field_injection(void);
  void user_diagnostics(void);
  void user_particle_collisions(void);
};

extern vpic_simulation *vpic_host_current;   // the one simulation of the process
