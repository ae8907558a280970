// select.hip -- the particles of one species that lie inside up to four ranges over position, momentum, kinetic
// energy and the coordinates in the frame of the local magnetic field, and satisfy up to two conditions on their tag, gathered into dense arrays in the order of the species' array
// (vpic_hip_species_select; include/vpic_hip.h states the semantics and the arithmetic).  Three launches, and kernel
// boundaries are the only ordering between workgroups -- no workgroup ever waits for a word that another one writes:
//   1  select_mark_kernel   streams the arrays the descriptor needs, stores one keep bit per particle and one kept
//                           count per chunk of SEL_CHUNK particles
//   2  select_scan_kernel   one workgroup: the exclusive scan of the chunk counts into 64-bit offsets, and the total
//   3  select_write_kernel  re-reads the bits (no coordinate), and the kept lanes gather their particle, the fields at
//                           it and its index to where the scan says
// The scratch buffers grow with engine.h's grow<T>; the statistics go through its DiagStats like every diagnostic's.
#include "dist_coords.h"
#include <algorithm>

namespace vpichip {

constexpr int SEL_WAVES = 4;                               // wavefronts per workgroup
constexpr int SEL_CHUNK = 2048;                            // particles per chunk: SEL_GROUPS keep masks, one count
constexpr int SEL_GROUPS = SEL_CHUNK / 64;
constexpr int SEL_PASSES = SEL_CHUNK / (64 * SEL_WAVES);   // passes of a workgroup over one chunk
constexpr int SEL_MAX_BLOCKS = 4096;                       // workgroups of launches 1 and 3 (each takes every gridDim.x-th chunk)
static_assert(SEL_CHUNK % 256 == 0 && SEL_GROUPS <= 64, "a chunk is a multiple of 256 particles whose masks one wavefront scans");

// Launch 1.  Chunk c is particles [c * SEL_CHUNK, (c + 1) * SEL_CHUNK) of the array; wavefront w of the workgroup
// takes the groups of 64 particles w, w + 4, ... of it.  MASKS: the keep masks are stored (mask[] holds SEL_GROUPS
// words for every chunk, the last chunk's beyond np included: zero).  tag: null when every tag reads 0.
// FIELDS: a range names a coordinate in the frame of the local field (dist_coords.h).  As in distribution.hip, the
// particle loads then run two passes ahead and the gather of the interpolator record (by live lanes only) one.
template <bool MASKS, bool FIELDS>
__global__ __launch_bounds__(64 * SEL_WAVES)
void select_mark_kernel(ParticlesK p, const int64_t *__restrict__ tag, long long np, long long n_chunks, SelectK k, GridK g, TileK t,
                        unsigned long long *__restrict__ mask, unsigned *__restrict__ counts, unsigned long long *__restrict__ stats,
                        const vpic_interpolator_t *__restrict__ fi) {
  __shared__ unsigned s_kept[SEL_WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned long long n_seen = 0;
  for (long long c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const long long first = c * SEL_CHUNK + threadIdx.x;
    unsigned n_kept = 0;
    DistRaw next = dist_load<FIELDS>(p, first, np, k.need), next2{};
    DistField f{}, f_next{};
    if (FIELDS) {
      next2 = dist_load<FIELDS>(p, first + 64 * SEL_WAVES, np, k.need);
      f_next = dist_gather(fi, next.voxel, g.nv, k.need);
    }
    long long next_tag = (k.use_tag && tag && first < np) ? tag[first] : 0;
#pragma unroll 2
    for (int pass = 0; pass < SEL_PASSES; pass++) {
      const DistRaw r = next;
      const long long r_tag = next_tag;
      if (FIELDS) {
        f = f_next;
        next = next2;
        f_next = dist_gather(fi, next.voxel, g.nv, k.need);                    // (behind the chunk's last pass: voxel -1, nothing is read)
        next2 = pass + 2 < SEL_PASSES ? dist_load<FIELDS>(p, first + (long long)(pass + 2) * (64 * SEL_WAVES), np, k.need)
                                      : DistRaw{-1, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      }
      if (pass + 1 < SEL_PASSES) {
        const long long idx = first + (long long)(pass + 1) * (64 * SEL_WAVES);
        if (!FIELDS) next = dist_load<FIELDS>(p, idx, np, k.need);
        next_tag = (k.use_tag && tag && idx < np) ? tag[idx] : 0;
      }
      const bool live = r.voxel >= 0 && r.voxel < g.nv;                      // i < 0: a dead slot (engine.h, Species::n_holes)
      n_seen += __popcll(__ballot(live));
      bool kept = live;
      if (k.s.n_sel > 0 && __any(live)) {
        DistCoords v{};
        int cx = 0, cy = 0, cz = 0;
        if (live) v = dist_coords<FIELDS>(r, f, k.need, t, cx, cy, cz);
        kept = live && dist_in_ranges<FIELDS>(v, k.s.sel, k.s.n_sel);
      }
      if (k.use_tag) kept = kept && select_tag_ok(k.s, r_tag);
      const unsigned long long m = __ballot(kept);
      n_kept += __popcll(m);
      if (MASKS && lane == 0) mask[c * SEL_GROUPS + pass * SEL_WAVES + wave] = m;
    }
    if (lane == 0) s_kept[wave] = n_kept;
    __syncthreads();
    if (threadIdx.x == 0) counts[c] = s_kept[0] + s_kept[1] + s_kept[2] + s_kept[3];
    __syncthreads();                                                         // (s_kept is written again for the next chunk)
  }
  if (lane == 0 && n_seen) atomicAdd(&stats[0], n_seen);
}
static_assert(SEL_WAVES == 4, "select_mark_kernel adds four wavefronts' counts");

// Launch 2: one workgroup of 256 walks the counts 256 at a time; offsets[c] = kept particles before chunk c, stats[1] the total.
__global__ __launch_bounds__(256)
void select_scan_kernel(const unsigned *__restrict__ counts, long long n_chunks, unsigned long long *__restrict__ offsets,
                        unsigned long long *__restrict__ stats) {
  __shared__ unsigned long long s_wave[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned long long carry = 0;
  for (long long base = 0; base < n_chunks; base += 256) {
    const long long c = base + threadIdx.x;
    const unsigned long long mine = c < n_chunks ? counts[c] : 0;
    unsigned long long incl = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const unsigned long long up = __shfl_up(incl, d);
      if (lane >= d) incl += up;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    unsigned long long before = carry;
    for (int w = 0; w < wave; w++) before += s_wave[w];
    if (c < n_chunks) offsets[c] = before + incl - mine;
    carry += s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    __syncthreads();
  }
  if (threadIdx.x == 0) stats[1] = carry;
}

// Launch 3.  Kept particle number d (in array order) of the species goes to record d while d < cap.  Any of out_p,
// out_f, out_i may be null; tag: null when every tag reads 0.
__global__ __launch_bounds__(64 * SEL_WAVES)
void select_write_kernel(ParticlesK p, const int64_t *__restrict__ tag, const int64_t *__restrict__ tag2, long long n_chunks,
                         const unsigned long long *__restrict__ mask, const unsigned *__restrict__ counts,
                         const unsigned long long *__restrict__ offsets, const vpic_interpolator_t *__restrict__ fi,
                         long long cap, vpic_particle_t *__restrict__ out_p, float *__restrict__ out_f, long long *__restrict__ out_i) {
  __shared__ unsigned long long s_mask[SEL_GROUPS];
  __shared__ unsigned s_before[SEL_GROUPS];                                  // kept in the chunk's earlier groups
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (long long c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const long long offset = (long long)offsets[c];
    if (counts[c] == 0 || offset >= cap) continue;                           // (the same for the whole workgroup)
    if (wave == 0) {
      const unsigned long long m = lane < SEL_GROUPS ? mask[c * SEL_GROUPS + lane] : 0;
      const unsigned mine = (unsigned)__popcll(m);
      unsigned incl = mine;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const unsigned up = __shfl_up(incl, d);
        if (lane >= d) incl += up;
      }
      if (lane < SEL_GROUPS) { s_mask[lane] = m; s_before[lane] = incl - mine; }
    }
    __syncthreads();
    for (int pass = 0; pass < SEL_PASSES; pass++) {
      const int group = pass * SEL_WAVES + wave;
      const unsigned long long m = s_mask[group];
      if (!(m >> lane & 1ull)) continue;
      const long long dest = offset + s_before[group] + __popcll(m & ((1ull << lane) - 1ull));
      if (dest >= cap) continue;
      const long long idx = c * SEL_CHUNK + (long long)group * 64 + lane;    // (below np: the bit is set for live particles only)
      const float4 pos = p.r[idx];
      const int voxel = record_cell(pos);
      const float dx = pos.x, dy = pos.y, dz = pos.z;
      if (out_p) {
        float4 *rec = reinterpret_cast<float4 *>(out_p + dest);              // 48 bytes: three 16-byte stores
        rec[0] = make_float4(dx, dy, dz, __int_as_float(voxel));
        rec[1] = make_float4(p.ux[idx], p.uy[idx], p.uz[idx], p.q[idx]);
        const long long t1 = tag ? tag[idx] : 0, t2 = tag ? tag2[idx] : 0;
        *reinterpret_cast<ulonglong2 *>(rec + 2) = make_ulonglong2((unsigned long long)t1, (unsigned long long)t2);
      }
      if (out_f) {
        // advance_p.cxx:74-82 without qdt_2mc: float, every operation rounded once (the library is built unfused)
        const float4 *q = reinterpret_cast<const float4 *>(fi + voxel);
        const float4 fx = q[0], fy = q[1], fz = q[2], fb = q[3];             // {ex, dexdy, dexdz, d2exdydz} ... {cbx, dcbxdx, cby, dcbydy}
        const float2 fc = *reinterpret_cast<const float2 *>(q + 4);          // {cbz, dcbzdz}
        float2 *o = reinterpret_cast<float2 *>(out_f + 6 * dest);
        o[0] = make_float2((fx.x + dy * fx.y) + dz * (fx.z + dy * fx.w), (fy.x + dz * fy.y) + dx * (fy.z + dz * fy.w));
        o[1] = make_float2((fz.x + dx * fz.y) + dy * (fz.z + dx * fz.w), fb.x + dx * fb.y);
        o[2] = make_float2(fb.z + dy * fb.w, fc.x + dz * fc.y);
      }
      if (out_i) out_i[dest] = idx;
    }
    __syncthreads();                                                         // (s_mask is written again for the next chunk)
  }
}

// Launches 1 and 2, and launch 3 when want_p / want_f / want_i ask for an output and a record is to be written: the
// first min(kept, cap) records are then in Engine::sel_p / sel_f / sel_i (device).  Waits for the stream; fills
// Engine::sel_stats.last.  count_only: launch 1 stores no masks.  Reads the species and changes nothing about it.
int k_species_select(Engine *e, Species &s, const vpic_hip_select_t &d, int64_t cap, bool want_p, bool want_f, bool want_i, bool count_only) {
  const SelectK k = make_select_k(d);
  const long long np = s.np, n_chunks = (np + SEL_CHUNK - 1) / SEL_CHUNK;
  const int64_t *tag = s.has_tags ? s.tag : nullptr;                         // never allocated: every tag reads 0
  if (grow(e->sel_counts, e->sel_counts_n, (size_t)n_chunks) || grow(e->sel_offsets, e->sel_offsets_n, (size_t)n_chunks)) return 1;
  if (!count_only && grow(e->sel_mask, e->sel_mask_n, (size_t)n_chunks * SEL_GROUPS)) return 1;
  if (e->sel_stats.begin(e->stream)) return 1;
  const unsigned nb = (unsigned)std::min<long long>(n_chunks, SEL_MAX_BLOCKS);
  const TileK tk = make_tile_k(e->gk);
  if (n_chunks > 0) {
    // ranges that name no field coordinate run the instances they always ran
    auto mark = k.need & NEED_FIELD ? (count_only ? select_mark_kernel<false, true> : select_mark_kernel<true, true>)
                                    : (count_only ? select_mark_kernel<false, false> : select_mark_kernel<true, false>);
    hipLaunchKernelGGL(mark, dim3(nb), dim3(64 * SEL_WAVES), 0, e->stream, s.p, tag, np, n_chunks, k, e->gk, tk,
                       count_only ? nullptr : e->sel_mask, e->sel_counts, e->sel_stats.dev, (const vpic_interpolator_t *)e->fi);
    VH_CHECK(hipGetLastError());
    hipLaunchKernelGGL(select_scan_kernel, dim3(1), dim3(256), 0, e->stream, (const unsigned *)e->sel_counts, n_chunks, e->sel_offsets, e->sel_stats.dev);
    VH_CHECK(hipGetLastError());
  }
  if (e->sel_stats.read(e->stream)) return 1;              // {seen, kept}; [2] and [3] are filled in below
  int64_t *last = e->sel_stats.last;
  const int64_t n_out = std::min(last[1], cap);
  int64_t written = 0;
  if (!count_only && n_out > 0 && (want_p || want_f || want_i)) {
    if (want_p && grow(e->sel_p, e->sel_p_n, (size_t)n_out)) return 1;
    if (want_f && grow(e->sel_f, e->sel_f_n, (size_t)n_out * 6)) return 1;
    if (want_i && grow(e->sel_i, e->sel_i_n, (size_t)n_out)) return 1;
    hipLaunchKernelGGL(select_write_kernel, dim3(nb), dim3(64 * SEL_WAVES), 0, e->stream, s.p, tag, (const int64_t *)s.tag2, n_chunks,
                       (const unsigned long long *)e->sel_mask, (const unsigned *)e->sel_counts, (const unsigned long long *)e->sel_offsets,
                       (const vpic_interpolator_t *)e->fi, (long long)cap, want_p ? e->sel_p : nullptr, want_f ? e->sel_f : nullptr,
                       want_i ? (long long *)e->sel_i : nullptr);
    VH_CHECK(hipGetLastError());
    written = n_out;
  }
  last[2] = written; last[3] = n_chunks;
  return 0;
}

}  // namespace vpichip
