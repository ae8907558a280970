// engine.h -- internal declarations of the resident MI355X engine (not part of the C ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <vector>
#include "vpic_hip.h"
#include "policy.h"
#include "moments_device.h"

namespace vpichip {

// ---- error plumbing ------------------------------------------------------------------------
void set_error(const char *fmt, ...);
#define VH_CHECK(expr)                                                                     \
  do {                                                                                     \
    hipError_t _e = (expr);                                                                \
    if (_e != hipSuccess) {                                                                \
      vpichip::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
      return 1;                                                                            \
    }                                                                                      \
  } while (0)
#define VH_FAIL(...) do { vpichip::set_error(__VA_ARGS__); return 1; } while (0)

// ---- device-side views ---------------------------------------------------------------------
// Geometry every kernel needs.  Voxel v = x + sy*(y + (ny+2)*z), sy = nx+2, sz = sy*(ny+2)
// (src/util/util_base.h:158-159).
struct GridK {
  int nx, ny, nz, sy, sz, nv;
  int fbc[6], pbc[6];
  int rank;
};

// Yee fields, struct-of-arrays over voxels.  Component order = float order inside field_t
// (src/field_advance/field_advance.h:159-171).
enum { F_EX = 0, F_EY, F_EZ, F_DIV_E_ERR, F_CBX, F_CBY, F_CBZ, F_DIV_B_ERR,
       F_TCAX, F_TCAY, F_TCAZ, F_RHOB, F_JFX, F_JFY, F_JFZ, F_RHOF, F_NCOMP };
enum { M_EMATX = 0, M_EMATY, M_EMATZ, M_NMAT, M_FMATX, M_FMATY, M_FMATZ, M_CMAT, M_NCOMP };
struct FieldsK {
  float *c[F_NCOMP];
  uint16_t *m[M_NCOMP];   // material ids; all null when the table holds a single material
};

// Particles of one species, kept (approximately) cell-sorted: one array of 16-byte POSITION RECORDS {dx, dy, dz, i} -- the
// cell as the bit pattern of the fourth float, as WaveQueue::pos_i (push.hip) carries it -- and the four 4-byte arrays
// ux, uy, uz, q.  Position and cell travel together wherever they change together: a cell-crosser's final state is one
// 16-byte store.  32 bytes per particle, as the vpic_particle_t of the C ABI: its first 16 bytes are this record.
struct ParticlesK {
  float4 *r;
  float *ux, *uy, *uz, *q;
};
__host__ __device__ __forceinline__ float4 make_record(float dx, float dy, float dz, int i) {
  union { int i; float f; } w; w.i = i;
  return make_float4(dx, dy, dz, w.f);
}
// the cell word alone (kernels that need only keys, or only whether a slot is dead: i < 0): a 4-byte access at a 16-byte stride
__device__ __forceinline__ int record_cell(const float4 *r, long long k) { return __float_as_int(r[k].w); }
__device__ __forceinline__ int record_cell(const float4 &v) { return __float_as_int(v.w); }
__device__ __forceinline__ void record_set_cell(float4 *r, long long k, int i) { r[k].w = __int_as_float(i); }
__host__ __device__ __forceinline__ ParticlesK offset_particles(const ParticlesK &p, int64_t at) {
  ParticlesK o = p;
  o.r += at; o.ux += at; o.uy += at; o.uz += at; o.q += at;
  return o;
}

// What the cell-crossing path of advance_p needs and the push loop does not (push.hip); one
// record per species in device memory, written when the species is created.
struct DrainParams {
  int nx, ny, nz, sy, sz, rank, max_nm;
  unsigned mul_sz;                   // v / sz == umulhi(v, mul_sz) >> (shifts >> 8) for 0 <= v < 2^31 (magic_div)
  int pbc[6];
  unsigned mul_sy, shifts;           // v / sy == umulhi(v, mul_sy) >> (shifts & 255)
  vpic_particle_mover_t *pm;
  int *nm_counter;
};

// Division of a non-negative int by a fixed d >= 2 as multiply-high and shift: with
// p = 31 + ceil(log2 d) and M = floor(2^p / d) + 1 < 2^32, floor(v * M / 2^p) == v / d for all
// 0 <= v < 2^31 (the error M*d - 2^p is in (0, d], so v * error < 2^p).
inline void magic_div(unsigned d, unsigned &mul, unsigned &shift) {
  unsigned l = 0;
  while ((1ull << l) < d) l++;
  const unsigned p = 31 + l;
  mul = (unsigned)(((unsigned long long)1 << p) / d + 1);
  shift = p - 32;
}

// device counters (ints, Engine::counters): [0] movers of a species beyond MAX_SPECIES (drop-in twins), [8..13]
// injectors per face, [14] holes, [15] fills, [16+s] np of species s while particles are exchanged, [48+s] movers of
// species s (written by advance_p and by the injection), [80] species that received charge, [81] overflow flags,
// [82] movers parked because their message was full, [83] the largest |q| of a message looked at ahead of its injection, [96+s] dead slots of species s (removals of the resident exchange),
// [128+s] the largest finite |q| an injection appended to species s, as the bits of that float (boundary_inject_kernel)
enum { C_NM = 0, C_DISORDER = 1, C_LOCAL = 2, C_SEND = 8, C_HOLES = 14, C_FILLS = 15, C_NP = 16, C_NMS = 48, C_CHARGED = 80, C_OVER = 81, C_RETRY = 82, C_QMSG = 83, C_NHOLE = 96, C_QTOP = 128, C_TOTAL = 160 };
constexpr int MAX_SPECIES = 32;
constexpr int HEADER_BASE = 256, MAX_HEADERS = 192;   // Engine::host_counters: [0, C_TOTAL) the counters, [HEADER_BASE, + 4 x MAX_HEADERS) message headers
constexpr int RETRY_CAP = 1 << 16;                     // movers a step may park because a message was full (vpic_hip_exchange_*)
// C_OVER bits: 1 more movers than a round's kernels were launched for (the rest waits for the next round), 2 a message was
// full (the movers are parked and offered again), 4 a species ran out of particle slots, 8 of mover slots, 16 more
// parked movers than RETRY_CAP (4, 8, 16: particles were lost)
static_assert(C_NMS + MAX_SPECIES == C_CHARGED && C_NP + MAX_SPECIES == C_NMS && C_NHOLE + MAX_SPECIES == C_QTOP && C_QTOP + MAX_SPECIES == C_TOTAL && C_TOTAL <= HEADER_BASE, "counter layout");     // species tables handed to kernels by value (boundary_p), per-species host slots

struct Species {
  float q_m = 0;
  // largest |charge| of a macro-particle that has EVER gone into this species -- set, appended or injected by the host, loaded
  // or emitted on the device (k_emit reads the largest emitted |q| back) -- also after that particle has left: the fixed-point
  // scales of the deterministic mode follow it (tests/test_gpu_moments_exact.py: "tail_holes", test_emitted_charges_count).
  // Arrivals from another domain count too: the injection kernel keeps the largest |q| it appended per species in a counter
  // word (C_QTOP) and k_exchange_finish / k_boundary_p_inject book it (tests/test_gpu_exchange.py: charge bookkeeping).
  float q_max = 0;
  int64_t np = 0, max_np = 0, nm = 0, max_nm = 0;
  // Dead slots among [0, np): the device-resident exchange removes a particle by marking its slot (i = -1) instead of
  // back-filling from the end of the array (boundary_p.c:264), so that the tile order survives and nothing moves under a
  // push that is still to come; every kernel that walks the array skips them, the next sort drops them (np -= n_holes).
  int64_t n_holes = 0;
  ParticlesK p{}, aux{};             // aux: second buffer for the out-of-place sort
  DrainParams *drain_k = nullptr;
  // adaptive sorting (vpic_hip_step, sort_interval < 0): events around the last push [0,1] and sort [2,3]
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  bool push_timed = false, sort_timed = false;
  Policy pol;                        // what the sort and push decisions remember (policy.h)
  int64_t *tag = nullptr, *tag2 = nullptr, *tag_aux = nullptr, *tag2_aux = nullptr;
  bool has_tags = false;             // tags all zero until a non-zero one is uploaded
  unsigned *crossed_dev = nullptr, *crossed_host = nullptr, *crossed_host_dev = nullptr;   // per-launch counters (device shards; the pinned words, policy.h: PinnedWord)
  bool chargeless = false;           // every particle has q == 0 (tracer copies): advance_p skips all deposition
  vpic_particle_mover_t *pm = nullptr;
  int *nm_dev = nullptr;             // this species' mover counter in Engine::counters
  int *partition = nullptr;          // nv+1, valid after sort_p
  bool partition_valid = false;
  // TILE order (crossing-heavy species under the adaptive sort policy; particles.hip, push.hip): the array is grouped by
  // 4x4x4-cell tile, cell by cell within a tile; tpart[tile * 64 + cell] is where that cell's particles began at the
  // sort.  Particles appended since then sit behind n_sorted.
  int *tpart = nullptr; int64_t tpart_count = 0;
  int *ttail = nullptr;              // the same for the particles appended since (regrouped by tile before every advance_p: k_tail_sort)
  bool tail_sorted = false;
  // The histogram of the NEXT sort taken by the push that precedes it (round 3): advance_p counts every particle's final cell
  // in the tile order's keys (LDS counters per window cell, flushed with the accumulators), so that the sort starts at its
  // scan.  hist_request: asked for by the step driver (the next step sorts); hist_valid: hist[] describes the array as it is
  // (anything that adds, removes or moves particles afterwards clears it and the sort counts for itself).
  int *hist = nullptr; int64_t hist_count = 0; bool hist_request = false, hist_valid = false;
  bool tail_regrouped = false;       // this step's push takes the appended particles by tile (decided by its first launch)
  // THE SORT INSIDE THE PUSH (round 3, push.hip: advance_p_kernel<.., SORT>).  A sort by tile and cell that finds the counts of
  // the push before it (hist_valid) moves nothing: k_sort_p sets fuse_pending, and the next k_advance_p writes every particle
  // it pushes to its SORTED place in the second buffer -- places from the scan of hist[] (tpart2: where every key begins in
  // the new order; Engine::sort_next: the cursors) -- then swaps the buffers.  The order is that of the cells BEFORE that
  // push (what hist[] counted).  crossed_host[PW_SORT_CHECK]: cursors that did not end where the next key begins (0 when the counts
  // matched the array; checked by the species' next push, which fails loudly otherwise).
  int *tpart2 = nullptr; int64_t tpart2_count = 0; bool fuse_pending = false;
  bool phase_pending = false;        // vpic_hip_advance_p_phase: the first launch ran, the interior tiles are still to be pushed
  bool tile_valid = false, adaptive = false;   // adaptive: the engine's own policy asks for the sorts (vpic_hip_sort_due)
  int64_t n_sorted = 0;
  bool coarse_sorted = false;     // the last tile sort was by tile only
  // the pairs of events of the measurements of Policy::sort_push_ms (sp_kind: which one is under way) and hint_push_ms
  hipEvent_t sp_ev[2] = {nullptr, nullptr}; int sp_kind = -1;
  hipEvent_t hp_ev[2] = {nullptr, nullptr}; bool hp_pending = false;
};

// tiles of TILE_EDGE^3 cells over the interior (the last one of an axis may be partial)
constexpr int TILE_CELLS = TILE_EDGE * TILE_EDGE * TILE_EDGE;
struct TileK {
  int sy, sz, ntx, nty, ntz, ntiles;
  unsigned mul_sy, sh_sy, mul_sz, sh_sz;     // magic_div of the voxel strides
  int mx, my, mz;                            // the last interior cell of every axis, from 0 (nx - 1, ny - 1, nz - 1)
};
TileK make_tile_k(const GridK &g);

// the cell (cx, cy, cz) of a voxel, ghost layers included (interior cells from 1): two divisions by the voxel strides
__device__ __forceinline__ void voxel_cell(int voxel, const TileK &t, int &cx, int &cy, int &cz) {
  cz = (int)(__umulhi((unsigned)voxel, t.mul_sz) >> t.sh_sz);
  const int rem = voxel - cz * t.sz;
  cy = (int)(__umulhi((unsigned)rem, t.mul_sy) >> t.sh_sy);
  cx = rem - cy * t.sy;
}

// sort key of a voxel: its own index (the reference's order, sort_p.c:48-58), or tile-major (TILE): tile by tile,
// cell by cell within the tile
template <bool TILE>
__device__ __forceinline__ int sort_key(int voxel, const TileK &t) {
  if (!TILE) return voxel;
  int cx, cy, cz;
  voxel_cell(voxel, t, cx, cy, cz);
  // particles live in interior voxels (1..n); an index in a ghost layer (the reference's sort_p takes any voxel) is
  // counted with the nearest interior cell instead of indexing outside the tables (the nearest cell that EXISTS: up to
  // the grid's last cell, not the last tile's -- a partial tile's cells beyond the grid hold nothing in any order)
  const int x = min(max(cx - 1, 0), t.mx), y = min(max(cy - 1, 0), t.my), z = min(max(cz - 1, 0), t.mz);
  const int tile = ((z >> 2) * t.nty + (y >> 2)) * t.ntx + (x >> 2);
  return tile * TILE_CELLS + ((z & 3) << 4 | (y & 3) << 2 | (x & 3));
}

// ---- pieces the passes over one species share (spectrum.hip, distribution.hip, moments.hip, select.hip) ---------------------
// the lanes for which `on` holds add 1 to word[a]; those that share the first such lane's word add once, together
// (a cold beam puts a whole wavefront in one word; more rounds of this, word by word, measured slower than letting the
// others add for themselves)
template <typename T>
__device__ __forceinline__ void add_together(T *word, int a, bool on, int lane) {
  const unsigned long long any = __ballot(on);
  if (!any) return;
  const int lead = __ffsll((long long)any) - 1;
  const int a0 = __builtin_amdgcn_readlane(a, lead);
  const unsigned long long same = __ballot(on && a == a0);
  if (on) {
    if (a != a0) atomicAdd(word + a, (T)1);
    else if (lane == lead) atomicAdd(word + a, (T)__popcll(same));
  }
}

// ---- ... and the per-bin sums (distribution.hip, cell_dist.hip) ----
// From this many lanes in the first counted lane's bin on they add their addends up across the wavefront and that lane
// adds once (a cold beam puts a whole wavefront in one word, and adds to one word are served one after the other); fewer
// add for themselves, which costs less than the six exchanges of a 64-bit word the adding-up takes per value.
constexpr int SUMS_TOGETHER_MIN = 8;

// the lanes for which `on` holds add `x` to word[a]; together: those of `same` (the lanes that share lane lead's word)
// add once
__device__ __forceinline__ void add_sums_together(unsigned long long *word, int a, long long x, bool on, bool together,
                                                  unsigned long long same, int lead, int lane) {
  bool mine = on;
  if (together) {
    const bool shared = same >> lane & 1ull;
    long long s = shared ? x : 0;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m);
    if (shared) { mine = lane == lead; x = s; }
  }
  if (mine && x) atomicAdd(word + a, (unsigned long long)x);                 // (two's complement: the unsigned add is the signed one)
}

// THE SLIDING WINDOW of a wavefront: `n_slots` consecutive positions (sort keys, bins of a position axis) x `stride` counters
// in LDS, [slot * stride + offset], from position `base` on.  Per pass of 64 particles the lanes whose position is inside the
// window add there; if some are not, the window is flushed (flush(base): the caller adds it to global memory and clears it)
// and moved to place(left), `left` being the lanes still waiting, and they try again, twice at the most; when more than
// half the wavefront still misses after that, the window stays where it is for the next WINDOW_BACKOFF passes (an array in
// no order: the window cannot help, and flushing it every pass would only cost).  A lane with pos < 0 never asks for a
// slide.  Returns whether this lane is still waiting: the caller adds it to global memory and counts a miss.
constexpr int WINDOW_BACKOFF = 16;
struct SlideWindow {
  int base = 0, backoff = 0;
  bool placed = false;               // the window has been given a place
};
template <typename Place, typename Flush>
__device__ __forceinline__ bool window_add(SlideWindow &w, unsigned *win, int n_slots, int stride, int pos, int offset, bool pending, int lane,
                                           Place place, Flush flush) {
  for (int round = 0; round < 3; round++) {
    if (round > 0) {
      const unsigned long long left = __ballot(pending && pos >= 0);
      if (!left) break;
      if (w.backoff > 0) { w.backoff--; break; }
      if (w.placed) flush(w.base);
      w.base = place(left);
      w.placed = true;
    }
    const bool hit = w.placed && pending && pos >= w.base && pos < w.base + n_slots;
    add_together(win, (pos - w.base) * stride + offset, hit, lane);
    if (hit) pending = false;
    if (round == 2 && __popcll(__ballot(pending)) > 32) w.backoff = WINDOW_BACKOFF;
  }
  return pending;
}

// Environment knobs (experiments and tests; none is needed in production), read ONCE when the engine is created
// (tools/README.md lists them): no entry point of the hot path calls getenv.
struct Knobs {
  int window = 0;                  // VPIC_HIP_WINDOW: 0 unset, 't' tile order, 'w' / 'n' the reference's order with the wide / narrow row window
  int tile_coarse = -1;            // VPIC_HIP_TILE_COARSE: -1 unset, 0 / 1
  long long tail_sort_min = 4096;  // VPIC_HIP_TAIL_SORT_MIN
  bool no_tail_sort = false;       // VPIC_HIP_NO_TAIL_SORT
  int iters = 0;                   // VPIC_HIP_ITERS (row windows: passes per wavefront)
  int ablate = 0;                  // VPIC_HIP_ABLATE (honoured by builds with -DVPIC_HIP_ABLATION only)
  bool policy_debug = false;       // VPIC_HIP_POLICY_DEBUG
  int follow = -1;                 // VPIC_HIP_FOLLOW=0|1: the tile window never / always follows the tile's particles (default: once deposits miss)
  int fuse_in_step = -1;           // VPIC_HIP_SORT_IN_PUSH=0|1: a species that is due is never / always (where it can be) sorted inside its push (Species::fuse_pending); default: whichever measured cheaper (engine.hip: sort_and_push)
  bool old_sort = false;           // VPIC_HIP_OLD_SORT: the wavefront-level count / scatter kernels of rounds 1-2 (A/B timing)
  int stage = -1;                  // VPIC_HIP_STAGE=0|1: advance_p never / always parks a pass's positions until its crossers are done (default: hot species only; push.hip)
  int follow_from = 16;            // VPIC_HIP_FOLLOW_FROM: missed runs per tile in one launch from which the windows follow (tuning)
  bool early_sort = true;         // VPIC_HIP_EARLY_SORT=0: vpic_hip_step keeps to the deck's sort interval whatever the deposits miss (A/B timing)
  int unload_tiled = 1;            // VPIC_HIP_UNLOAD_TILED: clear_jf + unload_accumulator 0 one thread per voxel through L1 / L2 (rounds 2-3), 2 through LDS tiles, 1 (default) tiles on grids large enough to fill the chip with them
  int field_tiles = 0;             // VPIC_HIP_FIELD_TILES: advance_b / advance_e (one material) 0 (default) one thread per voxel through L1 / L2, 2 through LDS tiles, 1 tiles on grids large enough to fill the chip with them -- measured TWICE as slow (fields.hip)
  bool rho_per_particle = false, hydro_per_particle = false;   // VPIC_HIP_RHO_PER_PARTICLE, VPIC_HIP_HYDRO_PER_PARTICLE
  bool collide_group = false;      // VPIC_HIP_COLLIDE_INSTANCE=group: vpic_hip_collide launches the workgroup-per-cell instance whatever the fullest cell (tests)
  bool moments_tiled = true;       // VPIC_HIP_MOMENTS_TILED=0: accumulate_hydro_p / accumulate_rho_p never sum by tile (policy.h: plan_moments; A/B timing)
};
Knobs read_knobs();

// "grow a scratch buffer": at least `want` elements of device memory, or (grow_pinned) of pinned host memory; what it held is dropped
template <typename T, bool PINNED = false>
inline int grow(T *&buf, size_t &have, size_t want) {
  if (want <= have) return 0;
  (void)(PINNED ? hipHostFree(buf) : hipFree(buf)); buf = nullptr; have = 0;
  VH_CHECK(PINNED ? hipHostMalloc((void **)&buf, want * sizeof(T), hipHostMallocDefault) : hipMalloc((void **)&buf, want * sizeof(T)));
  have = want;
  return 0;
}
template <typename T> inline int grow_pinned(T *&buf, size_t &have, size_t want) { return grow<T, true>(buf, have, want); }

// The statistics of a diagnostic's last call: WORDS 64-bit words its kernels add to on the device (four; eight for the
// per-bin sums), the pinned words they come back through, and what was read.  One word more, behind them, is
// k_check_tile_partition's flag (never read back).
template <int WORDS>
struct DiagStats {
  unsigned long long *dev = nullptr, *host = nullptr;
  int64_t last[WORDS] = {};
  bool pending = false;              // a caller that defers its read (moments.hip) says so here
  // before a call's kernels: allocated by the first call, zeroed on the stream
  int begin(hipStream_t stream) {
    if (!dev) VH_CHECK(hipMalloc((void **)&dev, (WORDS + 1) * sizeof(unsigned long long)));
    if (!host) VH_CHECK(hipHostMalloc((void **)&host, WORDS * sizeof(unsigned long long), hipHostMallocDefault));
    VH_CHECK(hipMemsetAsync(dev, 0, (WORDS + 1) * sizeof(unsigned long long), stream));
    return 0;
  }
  // behind them: copied, the stream waited for, last[] filled
  int read(hipStream_t stream) {
    VH_CHECK(hipMemcpyAsync(host, dev, WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
    VH_CHECK(hipStreamSynchronize(stream));
    for (int j = 0; j < WORDS; j++) last[j] = (int64_t)host[j];
    pending = false;
    return 0;
  }
  unsigned *bad_partition() const { return reinterpret_cast<unsigned *>(dev + WORDS); }
  void release() { (void)hipFree(dev); (void)hipHostFree(host); dev = host = nullptr; }
};

// The result of a histogram with per-bin sums (distribution.hip: one for the species; cell_dist.hip: one for the cells),
// allocated by the first call and grown on demand: the 64-bit counts and the n_val rows of 64-bit sums on the device, the
// pinned buffers they come back through (each as long as its device twin), and the statistics {seen, kept, counted,
// through global memory, refused for value 0 .. 3}.
struct HistResult {
  unsigned long long *counts = nullptr, *counts_host = nullptr, *sums = nullptr, *sums_host = nullptr;
  size_t bins = 0, words = 0;        // what counts / counts_host and sums / sums_host hold
  DiagStats<8> stats;
  static int grow_pair(unsigned long long *&dev, unsigned long long *&host, size_t &have, size_t want) {
    size_t dev_have = have;
    return grow(dev, dev_have, want) || grow_pinned(host, have, want);
  }
  int grow_counts(size_t n_bins) { return grow_pair(counts, counts_host, bins, n_bins); }
  int grow_sums(size_t n_words) { return grow_pair(sums, sums_host, words, n_words); }
  // before a call's kernel: room for n_bins counts and n_words sums, then statistics, counts and sums zeroed on the stream
  int begin(size_t n_bins, size_t n_words, hipStream_t stream) {
    if (grow_counts(n_bins) || grow_sums(n_words) || stats.begin(stream)) return 1;
    VH_CHECK(hipMemsetAsync(counts, 0, n_bins * sizeof(unsigned long long), stream));
    if (n_words) VH_CHECK(hipMemsetAsync(sums, 0, n_words * sizeof(unsigned long long), stream));
    return 0;
  }
  // behind it: counts, sums and statistics copied, the stream waited for, stats.last[] filled
  int read(size_t n_bins, size_t n_words, hipStream_t stream) {
    VH_CHECK(hipMemcpyAsync(counts_host, counts, n_bins * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
    if (n_words) VH_CHECK(hipMemcpyAsync(sums_host, sums, n_words * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
    return stats.read(stream);
  }
  void release() {
    (void)hipFree(counts); (void)hipHostFree(counts_host); (void)hipFree(sums); (void)hipHostFree(sums_host);
    counts = counts_host = sums = sums_host = nullptr; bins = words = 0;
    stats.release();
  }
};

struct Engine {
  int device = 0;
  Knobs knobs;
  hipStream_t stream = nullptr;
  vpic_hip_grid_t grid{};
  GridK gk{};
  FieldsK f{};
  float *field_block = nullptr;      // one allocation backing f.c[]
  uint16_t *mat_block = nullptr;
  vpic_material_coefficient_t *mc = nullptr;
  int n_mat = 0;
  vpic_interpolator_t *fi = nullptr;
  vpic_accumulator_t *acc = nullptr;
  std::vector<Species> species;
  bool engine_order = false;          // vpic_hip_set_sort_order: sorts asked for through the ABI may use the engine's own order (TILE)
  bool push_fast = false;             // advance_p arithmetic: false = the reference's scalar pipeline bit for bit, true = FAST (push.hip)
  bool can_strand = false;           // some face absorbs or belongs to another domain: advance_p may leave movers
  // Deterministic accumulation (vpic_hip_set_accumulation; push_device.h, Window<4>): deposits are summed as 64-bit fixed-point
  // integers in acc64 (12 words per voxel, value = word / acc_scale); acc_finalize rounds the sums into the float accumulator
  // (`acc`, what unload_accumulator and the host see) once per step.  rho64: the same for accumulate_rho_p.
  bool det_acc = false, acc64_dirty = false;
  double acc_scale = 0, acc_qref = 0;
  unsigned long long *acc64 = nullptr, *rho64 = nullptr;

  // scratch
  char *stage = nullptr; size_t stage_bytes = 0;       // AoS <-> SoA staging
  int *counters = nullptr;                             // small device ints (mover count, ...)
  void *acc_block = nullptr;                           // allocation behind `acc`
  bool time_kernels = false;                           // adaptive sorting in use: time every sort_p / advance_p with events
  int *host_miss = nullptr;                            // pinned: sampled descent count (vpic_hip_measure_disorder)
  void *hydro = nullptr; float *hydro_buf[2] = {nullptr, nullptr};   // hydro_t[nv] + face messages, allocated on first use
  int *host_counters = nullptr;                        // pinned mirror
  double *dsum = nullptr; double *host_dsum = nullptr; // reduction partials
  size_t dsum_count = 0;
  int *sort_next = nullptr;                            // nv+1
  int *scan_tmp = nullptr; size_t scan_tmp_count = 0;
  float *face_buf[2] = {nullptr, nullptr}; size_t face_buf_count = 0;
  vpic_particle_injector_t *send_buf[6] = {}; int64_t send_cap = 0;
  // custom particle boundary handlers of the maxwellian_reflux kind (src/boundary/maxwellian_reflux.c)
  struct Reflux { int code; float ut_para[MAX_SPECIES], ut_perp[MAX_SPECIES]; };
  std::vector<Reflux> reflux;
  uint32_t reflux_seed = 0; uint32_t reflux_calls = 0;
  float *reflux_draws = nullptr; int64_t reflux_draws_n = 0;
  double *emit_draws = nullptr; int64_t emit_draws_n = 0;      // test mode: the emission model's draws per emitted-particle slot   // test mode: the handlers' draws per particle index
  // absorbing walls that tally and record (vpic_hip_wall_*): the registered codes, the quanta of the two sums, the table
  // [VPIC_HIP_WALL_ROWS][MAX_SPECIES] and the record buffer with its cursor {records wanted since the last clear}
  struct Wall { int code, flags; };
  std::vector<Wall> walls;
  bool wall_ready = false;                                     // vpic_hip_wall_setup has run
  double wall_quantum[2] = {0, 0};
  vpic_hip_wall_tally_t *wall_table = nullptr;
  vpic_hip_wall_record_t *wall_rec = nullptr; int64_t wall_rec_cap = 0;
  unsigned long long *wall_cursor = nullptr;
  vpic_particle_injector_t *local_buf = nullptr; int64_t local_cap = 0;   // injectors that re-enter this same domain
  int32_t send_count[6] = {};
  int *hole_list = nullptr, *fill_list = nullptr, *tail_flag = nullptr; int64_t list_cap = 0;
  // device-resident exchange (vpic_hip_exchange_*): species table, message table, whether tail_flag is all zero
  void *sp_table_dev = nullptr, *sp_table_host = nullptr, *xmsg_dev = nullptr, *xmsg_host = nullptr; bool tail_clean = false; unsigned xmsg_turn = 0;
  void *retry_buf = nullptr;          // RETRY_CAP parked movers {mover, species}
  // tiles that touch a face shared with another domain [0] (every particle that can leave the domain this step is in one of
  // them or in the appended tail) and the others [1]: vpic_hip_advance_p_phase pushes the first group, lets the exchange
  // start, and pushes the second behind it
  int *tile_list[2] = {nullptr, nullptr}; int tile_list_n[2] = {0, 0};

  // energy spectra (spectrum.hip), allocated by the first call: the linear bands' counters and their normalised form
  // (n_lin x nv), the log bins and the pinned words they come back through; statistics {particles counted, window misses}
  unsigned *spec_lin = nullptr; float *spec_bands = nullptr; size_t spec_lin_words = 0;   // (spec_bands is as long as spec_lin)
  unsigned long long *spec_log = nullptr, *spec_log_host = nullptr;                          // VPIC_HIP_SPECTRUM_MAX_LOG words each
  DiagStats<4> spec_stats;
  // phase-space distributions of a species and the per-bin sums beside them (distribution.hip): one result block.  The
  // counts-only call (vpic_hip_species_distribution) writes into its counts too and keeps statistics of its own, {seen,
  // kept, counted, misses}, so that a sums call leaves them alone
  HistResult species_hist;
  DiagStats<4> dist_stats;
  // cell distributions (cell_dist.hip): the same over the cells of the grid
  HistResult cell_hist;
  // hydro moments and rho summed by tile (moments.hip), allocated by the first call: the fixed-point words of the
  // deterministic hydro sums (14 per voxel, zero between calls); statistics {live, through LDS, through global memory, out
  // of range} (mom_stats.pending: the last call's are still on the device, not read yet)
  unsigned long long *hydro64 = nullptr;
  DiagStats<4> mom_stats;
  // selected particles (select.hip), allocated by the first call and grown on demand: one keep bit per particle, the
  // kept count and the 64-bit offset of every chunk, the device output arrays (records, six floats per record, indices);
  // statistics {live particles seen, kept, written, chunks}
  unsigned long long *sel_mask = nullptr, *sel_offsets = nullptr; unsigned *sel_counts = nullptr;
  size_t sel_mask_n = 0, sel_offsets_n = 0, sel_counts_n = 0;
  vpic_particle_t *sel_p = nullptr; float *sel_f = nullptr; int64_t *sel_i = nullptr; size_t sel_p_n = 0, sel_f_n = 0, sel_i_n = 0;
  DiagStats<4> sel_stats;

  // binary collisions (collide.hip), allocated by the first call: the test mode's draws (4 floats per particle index), the
  // words its kernels write on the device and the pinned words they come back through (COLLIDE_WORDS), what the last call
  // left (vpic_hip_collide_stats) and the instance it launched (policy.h: CollideInstance as 0 / 1 / 2)
  float *collide_draws = nullptr; int64_t collide_draws_n = 0;
  unsigned long long *collide_dev = nullptr, *collide_host = nullptr;
  int64_t collide_last[6] = {0, 0, 0, 0, 0, 0}; int collide_instance = 0;
  // radiative cooling (cool.hip), allocated by the first call that asks for them and grown on demand: the per-voxel sums
  // and the pinned words they come back through; statistics {seen, changed, refused, left alone, the species' sum}
  unsigned long long *cool_cells = nullptr, *cool_cells_host = nullptr; size_t cool_cells_n = 0;
  DiagStats<8> cool_stats;
  // species loaded from per-cell tables (load.hip), allocated by the first call and grown on demand: the parity mode's draws
  // (7 floats per particle place) and the call's tables as uploaded
  float *load_draws = nullptr; int64_t load_draws_n = 0;
  char *load_tab = nullptr; size_t load_tab_bytes = 0;

  hipEvent_t step_done[4] = {}; int64_t steps_enqueued = 0;   // vpic_hip_step: the host stays at most two steps ahead of the device
  // profiling
  bool profile = false;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pool;
  size_t ev_used = 0;
  std::vector<int64_t> ev_particles;
  std::vector<char> ev_kind;                 // 1: a launch that sorts as it pushes (Species::fuse_pending): booked apart
  std::vector<int> ev_species;               // whose launch (vpic_hip_profile_read_species)
  double prof_sp_ms[MAX_SPECIES] = {}; int64_t prof_sp_launches[MAX_SPECIES] = {}, prof_sp_particles[MAX_SPECIES] = {};   // the plain launches, by species
  double prof_ms = 0; int64_t prof_launches = 0, prof_particles = 0;
  double prof_sort_ms = 0; int64_t prof_sort_launches = 0, prof_sort_particles = 0;
};

int ensure_stage(Engine *e, size_t bytes);
int acc_prepare_det(Engine *e, double q_arriving = 0);      // deterministic mode: allocate / scale the fixed-point accumulator before a kernel adds to it
                                                             // (q_arriving: the largest |q| of injector records about to be appended, looked at only while no other charge is known)
int acc_finalize(Engine *e);         // ... and round its sums into the float accumulator before anything reads that
void host_will_read(const void *p, size_t bytes);   // see engine.hip: called before a HIP copy reads / writes caller memory
void host_will_write(void *p, size_t bytes);
constexpr int PUSH_TILE = 64;          // particles per wavefront pass of the push kernel (push.hip)
constexpr int64_t PARTICLE_PAD = 2048;   // allocation granularity of the particle arrays (every kernel guards its accesses by np)
int alloc_particles(ParticlesK &p, int64_t n);
void free_particles(ParticlesK &p);

// kernels (one translation unit each)
int k_fields_from_aos(Engine *e, const vpic_field_t *host);
int k_fields_to_aos(Engine *e, vpic_field_t *host);
int k_load_interpolator(Engine *e);
int k_unload_accumulator(Engine *e);
int k_clear_jf(Engine *e);
int k_clear_jf_unload_accumulator(Engine *e);
int k_synchronize_jf_local(Engine *e);
int k_synchronize_jf_self(Engine *e, int axis);
int k_advance_b(Engine *e, float frac);
int k_advance_e(Engine *e, int part = 0);   // part: see AdvanceEParams (fields.hip)
int k_energy_f(Engine *e, double *en6);
int k_clear_rhof(Engine *e);
int k_accumulate_rho_p(Engine *e, Species &s, bool wants_tile);     // moments.hip; wants_tile: the engine would push the species in tile order
int k_rho_p_untiled(Engine *e, Species &s, bool by_cell);           // the float paths of a species that is not in tile order
int k_compute_div_e_err(Engine *e);
int k_compute_rhob(Engine *e);
int k_rms_div_e_err_local(Engine *e, double *local2);
int k_rms_div_b_err_local(Engine *e, double *local2);
int k_clean_div_e(Engine *e);
int k_compute_div_b_err(Engine *e);
int k_clean_div_b(Engine *e);
int k_compute_curl_b(Engine *e);
// face messages (fields.hip): what one reference routine sends per face.  The public kinds 0 .. 2 of vpic_hip_*_face_message are
// FAM_NORM_E + kind.
enum { FAM_TANG_B = 0, FAM_JF, FAM_RHO, FAM_HYDRO, FAM_NORM_E, FAM_DIV_B, FAM_TANG_E_NORM_B, FAM_COUNT };
int k_msg_count(const Engine *e, int fam, int dir);                 // floats in the message of face `dir`
int k_pack_msg(Engine *e, int fam, int dir, float *buf);
int k_unpack_msg(Engine *e, int fam, int dir, const float *buf);
int k_local_adjust(Engine *e, int fam);
int k_synchronize_self(Engine *e, int fam, int axis);
int k_synchronize_local(Engine *e, int fam, double *err = nullptr);
int k_err_begin(Engine *e);
int k_err_read(Engine *e, double *err);
int ensure_hydro(Engine *e);
int k_dump_gather(Engine *e, int what, int layout, const int32_t *words, int nwords, int sx, int sy, int sz, void *out, size_t out_bytes);
int k_clear_hydro(Engine *e);
int k_accumulate_hydro_p(Engine *e, Species &s, bool wants_tile);   // moments.hip
int k_accumulate_hydro_p_select(Engine *e, Species &s, const vpic_hip_select_t &d);   // ... of the particles a checked selection keeps
int k_hydro_p_untiled(Engine *e, Species &s, bool by_cell);
HydroConsts hydro_consts(const Engine *e, const Species &s);
int k_moments_stats(Engine *e, int64_t out[4]);
// tpart[] of a species in tile order: usable at all (host), and a partition of [0, n_sorted) (device: *bad is set where not; moments.hip)
int k_check_tile_partition(Engine *e, const Species &s, unsigned *bad);
inline bool tile_partition_usable(const Species &s, const TileK &t) {
  return s.tile_valid && s.tpart && s.tpart_count >= (int64_t)t.ntiles * TILE_CELLS + 1 && s.n_sorted >= 0 && s.n_sorted <= s.np;
}

int k_particles_from_aos(Engine *e, Species &s, const vpic_particle_t *host, int64_t n_new, int64_t at = 0, bool any_voxel = false);   // any_voxel: ghost voxels pass too (a test hook's: such a species may be sorted, never pushed)
int k_particles_to_aos(Engine *e, Species &s, vpic_particle_t *host, int64_t cap, int64_t from = 0, int64_t count = -1);
int k_load_maxwellian(Engine *e, Species &s, int ppc, unsigned seed, float q, float ux, float uy, float uz, float vth);
int ensure_tags(Engine *e, Species &s);                                          // the species' tag arrays, zeroed when first allocated
int k_load_profile(Engine *e, Species &s, const vpic_hip_load_t &d, int64_t *n_loaded);   // load.hip: checks, uploads, scans, generates
int k_energy_p(Engine *e, Species &s, double *energy);
int k_center_p(Engine *e, Species &s, bool uncenter);
int k_energy_spectrum(Engine *e, Species &s, const vpic_hip_spectrum_t &sp);   // into Engine::spec_lin / spec_log / spec_log_host; waits for the stream
int k_energy_bands(Engine *e, int n_lin);                                        // Engine::spec_lin -> spec_bands
int k_species_distribution(Engine *e, Species &s, const vpic_hip_dist_t &d);     // into the counts of Engine::species_hist and dist_stats; waits for the stream
int k_species_distribution_sums(Engine *e, Species &s, const vpic_hip_dist_t &d, const vpic_hip_dist_value_t *v, int n_val);   // ... into all of species_hist
int k_cell_distribution(Engine *e, const vpic_hip_dist_t &d, const vpic_hip_dist_value_t *v, int n_val);   // cell_dist.hip: into Engine::cell_hist; waits for the stream
// select.hip: launches 1 and 2 (count_only: no masks), and launch 3 into Engine::sel_p / sel_f / sel_i where asked for; waits for the stream
int k_species_select(Engine *e, Species &s, const vpic_hip_select_t &d, int64_t cap, bool want_p, bool want_f, bool want_i, bool count_only);
// collide.hip: the checking pass, the sorts it asks for, the launch; wants_tile_a / _b: the order a sort of that species would produce now;
// relativistic: the pair of vpic_hip_collide_relativistic
int k_collide(Engine *e, const vpic_hip_collision_t &c, bool wants_tile_a, bool wants_tile_b, bool relativistic);
// cool.hip: one pass over the species (a checked descriptor); the sums into Engine::cool_stats and, with cells, cool_cells_host; waits for the stream
int k_species_cool(Engine *e, Species &s, const vpic_hip_cool_t &c, bool cells);
int k_sort_p(Engine *e, Species &s, bool tile_order = false, bool may_fuse = false);   // may_fuse: the caller pushes the species next (see Species::fuse_pending)
int k_sort_scan(Engine *e, const int *counts, int *starts, int n1);                  // exclusive scan of counts[0..n1) into starts[] and Engine::sort_next[]
int k_sort_check(Engine *e, Species &s, const int *starts, int n1);                    // every cursor ended where the next key begins? (PW_SORT_CHECK; the next push fails loudly otherwise)
int k_sort_finish(Engine *e, Species &s, bool tile_order, bool coarse);                // what follows a sort's scatter (buffers swapped, bookkeeping)
int k_tail_sort(Engine *e, Species &s);
int k_measure_disorder(Engine *e, Species &s, int slot);
int k_boundary_p_pack(Engine *e);
int k_exchange_begin(Engine *e);
int k_exchange_pack(Engine *e, void *const msg[6], const int32_t cap[6], int mover_cap, uint32_t species_mask = ~0u);
int k_compact(Engine *e, Species &s);          // drop the dead slots of a species (a sort in the order it is in)
int k_species_reserve(Engine *e, Species &s, int64_t max_np, int64_t max_nm);
int k_exchange_inject(Engine *e, const void *msg, int cap);
int k_exchange_finish(Engine *e, const void *const *recv, int n_recv, int32_t *headers_out, int32_t *flags_out);
int k_advance_p(Engine *e, Species &s, bool async = false, int phase = 0);   // async: the mover count stays on the device (vpic_hip_exchange_*); phase: see vpic_hip_advance_p_phase
int k_boundary_p_inject(Engine *e, const vpic_particle_injector_t *inj, int n, const int64_t *tags = nullptr);
int k_emit(Engine *e, int sp, const int32_t *host_components, int n, int n_emit, float ut_perp, float ut_para, float coef, float thresh, unsigned seed);
int k_inject_aged(Engine *e, const vpic_particle_injector_t *host_inj, const int64_t *host_tags, int n);
int k_accumulate_rhob(Engine *e, const vpic_particle_t *host, int64_t n, float q_scale);

// g.pbc[face] with a run-time face: a dynamically indexed kernel-argument array would be copied
// to scratch memory, a select chain stays in scalar registers.
__device__ __forceinline__ int pbc_of(const GridK &g, int face) {
  return face == 0 ? g.pbc[0] : face == 1 ? g.pbc[1] : face == 2 ? g.pbc[2]
       : face == 3 ? g.pbc[3] : face == 4 ? g.pbc[4] : g.pbc[5];
}

// XCD-aware logical block id: blocks are dealt round-robin over the 8 XCDs (b and b+8 share
// one), so give each XCD a contiguous range of logical blocks -- neighbouring tiles then share
// an L2.  Speed only: any mapping is correct.
__device__ __forceinline__ unsigned xcd_block(unsigned b, unsigned nb) {
  const unsigned per = nb >> 3;
  if (per == 0 || (nb & 7)) return b;
  return (b & 7) * per + (b >> 3);
}

}  // namespace vpichip

// the opaque handle of the C ABI is the engine itself
struct vpic_hip_engine : public vpichip::Engine {};
