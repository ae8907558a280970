// moments.hip -- accumulate_hydro_p (14 moments per node) and accumulate_rho_p (1) of a species, summed BY TILE where the
// species is in tile order, and as 64-bit fixed-point integers in deterministic mode (vpic_hip_set_accumulation): the sums
// are then bit-identical whatever the order of the array, the scheduling or the path taken.  policy.h (plan_moments) says
// which path a call takes; what one particle adds is stated in moments_device.h, the same for every kernel of the engine.
//   tile pass   one workgroup per tile j walks [tpart[64 j], tpart[64 (j + 1)]) of the sorted part with coalesced loads.  LDS
//               holds the nodes of the tile's cells and of one cell more on every side (7 x 7 x 7 nodes x the moments: 38.4 KB
//               in 64-bit words, 19.2 KB in floats); a particle whose cell is inside adds there, any other (particles drift out
//               of their tile between sorts) straight to global memory; at the end the non-zero words go to global memory.
//   tail pass   one thread per particle over [n_sorted, np) -- or over the whole array, for a species that is not in tile
//               order and may not be sorted, and where tpart[] turns out not to be a partition (k_check_tile_partition,
//               defined here and shared with distribution.hip) -- with global atomics.
//   finalize    (fixed point) hydro[v].m += (float)(sum / scale_m), one rounding per word and call, and the word is zeroed.
// The array is not reordered and nothing the push or the next sort relies on is touched.
// accumulate_hydro_p_select: the same passes over the same array, in instances (SEL) in which a particle that the selection
// (dist_coords.h: the ranges and the tag conditions of vpic_hip_species_select) does not keep adds nothing; the instances
// without a selection are the code they were.
#include "engine.h"
#include "push_device.h"
#include "dist_coords.h"
#include <algorithm>
#include <math.h>

namespace vpichip {

constexpr int MOM_WX = TILE_EDGE + 3;                    // nodes per edge of the window: the tile's cells, one more on either side, + 1
constexpr int MOM_SLOTS = MOM_WX * MOM_WX * MOM_WX;      // (odd: the moments of one node lie in different banks)
constexpr int MOM_TAIL_BLOCKS = 4096;

struct MomK {
  ParticlesK p;
  const float4 *fi;
  const int *tpart; const unsigned *bad;                 // bad: set when tpart[] is no partition (null: no tile pass ran)
  long long n_sorted, np;
  int sy, sz, nv_safe;                                   // nv_safe: voxels below it have all 8 nodes of their cell inside the arrays
  TileK t;
  HydroConsts h;
  double scale[HYDRO_MOMENTS];                           // fixed point: per moment ([0] alone for rho)
  unsigned long long *stats;                             // live particles, through LDS, through global memory, contributions out of range
};
// the selection of an instance: none (today's code), ranges in the box frame, ranges that name a coordinate in the frame of the
// local field (dist_coords.h: FIELDS); the kernels' argument carries the descriptor only where there is one
enum { MOM_SEL_NONE = 0, MOM_SEL_BOX = 1, MOM_SEL_FIELD = 2 };
template <int SEL> struct MomKS : MomK { SelectK sel; const int64_t *tag; };   // tag: null when every tag reads 0
template <> struct MomKS<MOM_SEL_NONE> : MomK {};
static_assert(sizeof(MomKS<MOM_SEL_NONE>) == sizeof(MomK), "the instances without a selection take the argument they took");

// tpart[] is a partition of [0, n_sorted): non-decreasing from 0, within n_sorted (*bad is set where it is not)
__global__ __launch_bounds__(256)
void check_tile_partition_kernel(const int *__restrict__ tpart, int ntiles, long long n_sorted, unsigned *__restrict__ bad) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= ntiles) return;
  const long long b0 = tpart[(size_t)j * TILE_CELLS], b1 = j + 1 < ntiles ? (long long)tpart[(size_t)(j + 1) * TILE_CELLS] : n_sorted;
  if (b0 < 0 || b0 > b1 || b1 > n_sorted || (j == 0 && b0 != 0)) atomicOr(bad, 1u);
}
int k_check_tile_partition(Engine *e, const Species &s, unsigned *bad) {
  const int ntiles = make_tile_k(e->gk).ntiles;
  hipLaunchKernelGGL(check_tile_partition_kernel, dim3((ntiles + 255) / 256), dim3(256), 0, e->stream, (const int *)s.tpart, ntiles,
                     (long long)s.n_sorted, bad);
  VH_CHECK(hipGetLastError());
  return 0;
}

// one contribution: a float add, or rounded to fixed point and added as an integer (what does not convert is counted, not added)
__device__ __forceinline__ void mom_add(float *word, float x, double, unsigned &) { atomicAdd(word, x); }
__device__ __forceinline__ void mom_add(unsigned long long *word, float x, double scale, unsigned &n_range) {
  if (fabs((double)x * scale) < 2251799813685248.0) atomicAdd(word, to_fixed(x, scale));    // 2^51 (push_device.h); false for a NaN
  else n_range++;
}

// words per voxel in global memory: hydro_t is 14 floats and two of padding, everything else is packed
template <int NM, typename ACC> struct MomLayout { static constexpr int STRIDE = NM; };
template <> struct MomLayout<HYDRO_MOMENTS, float> { static constexpr int STRIDE = HYDRO_STRIDE; };

struct MomCount { unsigned live = 0, lds = 0, global = 0, range = 0; };

// particle idx: its NM x 8 contributions into the window (lx, ly, lz: its cell within the window, when WINDOW and inside) or
// into global memory.  SEL: only a particle the selection keeps (the coordinates of dist_coords.h from the STORED momenta and the
// voxel's interpolator record, which a kept particle reads once: for its coordinates, where they need it, and for its moments)
// is counted and adds; any other returns before a contribution is formed.
template <int NM, typename ACC, bool WINDOW, int SEL>
__device__ __forceinline__ void moments_of_particle(const MomKS<SEL> &K, ACC *__restrict__ out, ACC *s_win, long long idx, int bx, int by, int bz, MomCount &n) {
  const float4 rec = K.p.r[idx];
  const int voxel = record_cell(rec);
  if (voxel < 0 || voxel >= K.nv_safe) return;            // i < 0: a dead slot (engine.h, Species::n_holes)
  HydroP P;
  if constexpr (SEL != MOM_SEL_NONE) {
    static_assert(NM == HYDRO_MOMENTS, "a selection is for the hydro moments");
    constexpr bool FIELDS = SEL == MOM_SEL_FIELD;
    if (K.sel.use_tag && !select_tag_ok(K.sel.s, K.tag ? K.tag[idx] : 0)) return;          // (uniform: the tags are read when a flag is set)
    const DistRaw r{voxel, rec.x, rec.y, rec.z, K.p.ux[idx], K.p.uy[idx], K.p.uz[idx]};
    InterpK f;
    if (FIELDS) f = load_interp(K.fi, voxel);
    if (K.sel.s.n_sel > 0) {
      const DistField df = FIELDS ? DistField{f.b0, f.b1, f.ex, f.ey, f.ez} : DistField{};
      int cx = 0, cy = 0, cz = 0;
      const DistCoords v = dist_coords<FIELDS>(r, df, K.sel.need, K.t, cx, cy, cz);
      if (!dist_in_ranges<FIELDS>(v, K.sel.s.sel, K.sel.s.n_sel)) return;
    }
    if (!FIELDS) f = load_interp(K.fi, voxel);
    n.live++;
    hydro_particle(r.dx, r.dy, r.dz, r.ux, r.uy, r.uz, K.p.q[idx], f, K.h, P);
  } else {
    n.live++;
    if constexpr (NM == HYDRO_MOMENTS)
      hydro_particle(rec.x, rec.y, rec.z, K.p.ux[idx], K.p.uy[idx], K.p.uz[idx], K.p.q[idx], load_interp(K.fi, voxel), K.h, P);
    else
      node_weights(rec.x, rec.y, rec.z, K.p.q[idx], K.h.r8V, P.w);
  }
  bool inside = false;
  int slot0 = 0;
  if (WINDOW) {
    int cx, cy, cz;
    voxel_cell(voxel, K.t, cx, cy, cz);
    const unsigned lx = (unsigned)(cx - bx), ly = (unsigned)(cy - by), lz = (unsigned)(cz - bz);
    inside = lx < (unsigned)(MOM_WX - 1) && ly < (unsigned)(MOM_WX - 1) && lz < (unsigned)(MOM_WX - 1);
    slot0 = (int)(lx + MOM_WX * (ly + MOM_WX * lz));
  }
  unsigned range = 0;
  // (the selected instances count without a branch: the two increments below, one on either path, become an indexed store
  // into MomCount in scratch memory in the tile instances, which the instances without a selection keep as they were compiled)
  if constexpr (SEL != MOM_SEL_NONE) { n.lds += inside ? 1u : 0u; n.global += inside ? 0u : 1u; }
  if (WINDOW && inside) {
#pragma unroll
    for (int nd = 0; nd < 8; nd++) {
      float c[NM];
      if constexpr (NM == HYDRO_MOMENTS) hydro_node(P, P.w[nd], K.h.mc_q, c); else c[0] = P.w[nd];
      const int slot = slot0 + (nd & 1) + ((nd >> 1) & 1) * MOM_WX + (nd >> 2) * MOM_WX * MOM_WX;
#pragma unroll
      for (int k = 0; k < NM; k++) mom_add(&s_win[k * MOM_SLOTS + slot], c[k], K.scale[k], range);
    }
    if constexpr (SEL == MOM_SEL_NONE) n.lds++;
  } else {
    ACC *g = out + (size_t)voxel * MomLayout<NM, ACC>::STRIDE;
#pragma unroll
    for (int nd = 0; nd < 8; nd++) {
      float c[NM];
      if constexpr (NM == HYDRO_MOMENTS) hydro_node(P, P.w[nd], K.h.mc_q, c); else c[0] = P.w[nd];
      ACC *m = g + (size_t)((nd & 1) + ((nd >> 1) & 1) * K.sy + (nd >> 2) * K.sz) * MomLayout<NM, ACC>::STRIDE;
#pragma unroll
      for (int k = 0; k < NM; k++) mom_add(m + k, c[k], K.scale[k], range);
    }
    if constexpr (SEL == MOM_SEL_NONE) n.global++;
  }
  n.range += range;
}

__device__ __forceinline__ void publish_counts(const MomCount &n, unsigned long long *__restrict__ stats) {
  unsigned v[4] = {n.live, n.lds, n.global, n.range};
#pragma unroll
  for (int j = 0; j < 4; j++) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v[j] += __shfl_xor(v[j], m);
    if ((threadIdx.x & 63) == 0 && v[j]) atomicAdd(&stats[j], (unsigned long long)v[j]);
  }
}

template <int NM, typename ACC, int SEL = MOM_SEL_NONE>
__global__ __launch_bounds__(256)
void moments_tile_kernel(MomKS<SEL> K, ACC *__restrict__ out) {
  __shared__ ACC s_win[NM * MOM_SLOTS];
  if (*K.bad) return;                                      // (the tail pass takes the whole array)
  const int j = blockIdx.x;
  for (int w = threadIdx.x; w < NM * MOM_SLOTS; w += 256) s_win[w] = (ACC)0;
  __syncthreads();
  // the window begins at the node of the cell before the tile's first on every axis (voxel coordinates: interior cells from 1)
  const int tz = j / (K.t.ntx * K.t.nty), trem = j - tz * (K.t.ntx * K.t.nty), ty = trem / K.t.ntx, tx = trem - ty * K.t.ntx;
  const int bx = TILE_EDGE * tx, by = TILE_EDGE * ty, bz = TILE_EDGE * tz;
  const long long begin = K.tpart[(size_t)j * TILE_CELLS];
  const long long end = j + 1 < K.t.ntiles ? (long long)K.tpart[(size_t)(j + 1) * TILE_CELLS] : K.n_sorted;
  MomCount n;
  for (long long idx = begin + threadIdx.x; idx < end; idx += 256) moments_of_particle<NM, ACC, true, SEL>(K, out, s_win, idx, bx, by, bz, n);
  __syncthreads();
  // the non-zero words of the window (only nodes inside the arrays can be: nv_safe)
  for (int w = threadIdx.x; w < NM * MOM_SLOTS; w += 256) {
    const int slot = w / NM, k = w - slot * NM;
    const ACC v = s_win[k * MOM_SLOTS + slot];
    if (v != (ACC)0) {
      const int lz = slot / (MOM_WX * MOM_WX), r = slot - lz * (MOM_WX * MOM_WX), ly = r / MOM_WX, lx = r - ly * MOM_WX;
      const size_t node = (size_t)(bx + lx) + (size_t)(by + ly) * K.sy + (size_t)(bz + lz) * K.sz;
      atomicAdd(out + node * MomLayout<NM, ACC>::STRIDE + k, v);
    }
  }
  publish_counts(n, K.stats);
}

template <int NM, typename ACC, int SEL = MOM_SEL_NONE>
__global__ __launch_bounds__(256)
void moments_tail_kernel(MomKS<SEL> K, ACC *__restrict__ out) {
  const long long from = K.bad && *K.bad ? 0 : K.n_sorted;
  MomCount n;
  for (long long idx = from + (long long)blockIdx.x * 256 + threadIdx.x; idx < K.np; idx += (long long)gridDim.x * 256)
    moments_of_particle<NM, ACC, false, SEL>(K, out, nullptr, idx, 0, 0, 0, n);
  publish_counts(n, K.stats);
}

struct MomInvScales { double s[HYDRO_MOMENTS]; };
// the exact sums, rounded once into the float array; the words are zero again afterwards
template <int NM>
__global__ __launch_bounds__(256)
void moments_finalize_kernel(float *__restrict__ out, unsigned long long *__restrict__ sums, int nv, MomInvScales inv) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= nv) return;
#pragma unroll
  for (int k = 0; k < NM; k++) {
    const long long s = (long long)sums[(size_t)v * NM + k];
    if (s) { out[(size_t)v * MomLayout<NM, float>::STRIDE + k] += (float)((double)s * inv.s[k]); sums[(size_t)v * NM + k] = 0; }
  }
}

// the kernels of one call: `tiled`: tile pass + tail pass; otherwise the per-particle pass over the whole array
template <int NM, typename ACC, int SEL = MOM_SEL_NONE>
static int launch_moments(Engine *e, Species &s, MomKS<SEL> &K, ACC *out, bool tiled) {
  if (e->mom_stats.begin(e->stream)) return 1;
  K.p = s.p; K.fi = reinterpret_cast<const float4 *>(e->fi); K.np = s.np;
  K.sy = e->gk.sy; K.sz = e->gk.sz; K.nv_safe = e->gk.nv - e->gk.sz - e->gk.sy - 1;
  K.t = make_tile_k(e->gk);
  K.stats = e->mom_stats.dev;
  K.tpart = nullptr; K.bad = nullptr; K.n_sorted = 0;
  if (s.np > 0) {
    if (tiled) {
      K.tpart = s.tpart; K.bad = e->mom_stats.bad_partition(); K.n_sorted = s.n_sorted;
      if (k_check_tile_partition(e, s, e->mom_stats.bad_partition())) return 1;
      hipLaunchKernelGGL((moments_tile_kernel<NM, ACC, SEL>), dim3((unsigned)K.t.ntiles), dim3(256), 0, e->stream, K, out);
    }
    // (a tpart[] that is no partition sends the whole array through this pass: sized for that)
    const unsigned nb = (unsigned)std::min<long long>(MOM_TAIL_BLOCKS, (s.np + 255) / 256);
    hipLaunchKernelGGL((moments_tail_kernel<NM, ACC, SEL>), dim3(nb), dim3(256), 0, e->stream, K, out);
    VH_CHECK(hipGetLastError());
  }
  e->mom_stats.pending = true;                             // (read when somebody asks: read_moments_stats)
  return 0;
}

static int read_moments_stats(Engine *e) { return e->mom_stats.pending ? e->mom_stats.read(e->stream) : 0; }
int k_moments_stats(Engine *e, int64_t out[4]) {
  if (read_moments_stats(e)) return 1;
  for (int j = 0; j < 4; j++) out[j] = e->mom_stats.last[j];
  return 0;
}
// a call that took one of the float paths of push.hip / fields.hip: every live particle through global memory
static void book_untiled(Engine *e, const Species &s) {
  int64_t *last = e->mom_stats.last;
  e->mom_stats.pending = false;
  last[0] = last[2] = s.np - s.n_holes; last[1] = last[3] = 0;
}

static MomentPlan plan_for(Engine *e, Species &s, bool wants_tile, bool per_particle_knob) {
  const TileK tk = make_tile_k(e->gk);
  MomentInputs in;
  in.det = e->det_acc; in.tile_valid = s.tile_valid; in.wants_tile = wants_tile;
  in.tpart_ok = tile_partition_usable(s, tk);
  in.per_particle_knob = per_particle_knob; in.tiled_knob = e->knobs.moments_tiled;
  in.np = s.np; in.nm = s.nm; in.nv = e->gk.nv;
  return plan_moments(in);
}

// the 14 hydro moments of the species through the kernels of this file (`tiled`: launch_moments), in floats or -- deterministic
// mode -- in fixed point at the scale of the species' q_max, rounded once into the float array; what: the caller, for the message
template <int SEL>
static int hydro_sums(Engine *e, Species &s, MomKS<SEL> &K, bool tiled, const char *what) {
  K.h = hydro_consts(e, s);
  if (!e->det_acc) return launch_moments<HYDRO_MOMENTS, float, SEL>(e, s, K, reinterpret_cast<float *>(e->hydro), tiled);
  const size_t words = (size_t)HYDRO_MOMENTS * (size_t)e->gk.nv;
  if (!e->hydro64) {
    VH_CHECK(hipMalloc((void **)&e->hydro64, sizeof(unsigned long long) * words));
    VH_CHECK(hipMemsetAsync(e->hydro64, 0, sizeof(unsigned long long) * words, e->stream));
  }
  const MomentScales ms = moment_scales(s.q_max > 0 ? (double)s.q_max : e->acc_qref, s.q_m, K.h.r8V, K.h.c);
  MomInvScales inv;
  for (int k = 0; k < HYDRO_MOMENTS; k++) { K.scale[k] = ms.scale[k]; inv.s[k] = 1.0 / ms.scale[k]; }
  if (launch_moments<HYDRO_MOMENTS, unsigned long long, SEL>(e, s, K, e->hydro64, tiled)) return 1;
  if (read_moments_stats(e)) return 1;                       // (one wait per deterministic call: get_hydro follows)
  if (e->mom_stats.last[3] > 0) {
    VH_CHECK(hipMemsetAsync(e->hydro64, 0, sizeof(unsigned long long) * words, e->stream));
    VH_FAIL("%s: %lld contributions are out of the fixed-point range of the deterministic sums (a momentum |u| of the order of 2^12 and above); nothing was added",
            what, (long long)e->mom_stats.last[3]);
  }
  hipLaunchKernelGGL(moments_finalize_kernel<HYDRO_MOMENTS>, dim3((unsigned)((e->gk.nv + 255) / 256)), dim3(256), 0, e->stream,
                     reinterpret_cast<float *>(e->hydro), e->hydro64, e->gk.nv, inv);
  VH_CHECK(hipGetLastError());
  return 0;
}

int k_accumulate_hydro_p(Engine *e, Species &s, bool wants_tile) {
  if (ensure_hydro(e)) return 1;
  const MomentPlan pl = plan_for(e, s, wants_tile, e->knobs.hydro_per_particle);
  if (!e->det_acc && pl.path != MomentPath::tiled) {
    book_untiled(e, s);
    return s.np == 0 ? 0 : k_hydro_p_untiled(e, s, pl.path == MomentPath::cells);
  }
  if (pl.sort_by_tile_first && k_sort_p(e, s, true)) return 1;
  MomKS<MOM_SEL_NONE> K{};
  return hydro_sums(e, s, K, pl.path == MomentPath::tiled, "accumulate_hydro_p");
}

// ... of the particles a (checked) selection keeps: the species is read and left as it is, in either mode (policy.h:
// plan_moments_select), and the fixed-point scale is the whole species'
template <int SEL>
static int hydro_sums_select(Engine *e, Species &s, const vpic_hip_select_t &d, bool tiled) {
  MomKS<SEL> K{};
  K.sel = make_select_k(d);
  K.tag = s.has_tags ? s.tag : nullptr;                      // never allocated: every tag reads 0
  return hydro_sums(e, s, K, tiled, "accumulate_hydro_p_select");
}
int k_accumulate_hydro_p_select(Engine *e, Species &s, const vpic_hip_select_t &d) {
  if (ensure_hydro(e)) return 1;
  MomentInputs in;
  in.det = e->det_acc; in.tile_valid = s.tile_valid; in.tpart_ok = tile_partition_usable(s, make_tile_k(e->gk));
  in.tiled_knob = e->knobs.moments_tiled; in.np = s.np; in.nm = s.nm; in.nv = e->gk.nv;
  const bool tiled = plan_moments_select(in).path == MomentPath::tiled;
  unsigned need = 0;
  for (int r = 0; r < d.n_sel; r++) need |= 1u << d.sel[r].coord;
  return need & NEED_FIELD ? hydro_sums_select<MOM_SEL_FIELD>(e, s, d, tiled) : hydro_sums_select<MOM_SEL_BOX>(e, s, d, tiled);
}

int k_accumulate_rho_p(Engine *e, Species &s, bool wants_tile) {
  if (s.np == 0 || s.chargeless) { book_untiled(e, s); e->mom_stats.last[0] = e->mom_stats.last[2] = 0; return 0; }   // charge-0 copies add nothing
  const MomentPlan pl = plan_for(e, s, wants_tile, e->knobs.rho_per_particle);
  if (!e->det_acc && pl.path != MomentPath::tiled) { book_untiled(e, s); return k_rho_p_untiled(e, s, pl.path == MomentPath::cells); }
  if (pl.sort_by_tile_first && k_sort_p(e, s, true)) return 1;
  MomKS<MOM_SEL_NONE> K{};
  K.h.r8V = 0.125 * e->grid.rdx * e->grid.rdy * e->grid.rdz;   // rho_p.c:37
  if (!e->det_acc) return launch_moments<1, float>(e, s, K, e->f.c[F_RHOF], true);
  // deterministic: fixed-point sums in rho64, then one rounding into rhof (the species are added to rhof one after the other,
  // in the caller's order); the scale is the accumulator's, moved to where a weight of 8 r8V |q| lands
  if (acc_prepare_det(e)) return 1;
  const size_t nv = (size_t)e->gk.nv;
  if (!e->rho64) { VH_CHECK(hipMalloc(&e->rho64, sizeof(unsigned long long) * nv)); VH_CHECK(hipMemsetAsync(e->rho64, 0, sizeof(unsigned long long) * nv, e->stream)); }
  int ex = 0; (void)frexp(8.0 * (double)K.h.r8V, &ex);
  K.scale[0] = ldexp(e->acc_scale, -ex);                       // a weight is at most 8 r8V |q|
  MomInvScales inv{}; inv.s[0] = 1.0 / K.scale[0];
  if (launch_moments<1, unsigned long long>(e, s, K, e->rho64, pl.path == MomentPath::tiled)) return 1;
  hipLaunchKernelGGL(moments_finalize_kernel<1>, dim3((unsigned)((nv + 255) / 256)), dim3(256), 0, e->stream, e->f.c[F_RHOF], e->rho64, (int)nv, inv);
  VH_CHECK(hipGetLastError());
  return 0;
}

}  // namespace vpichip
