// load.hip -- vpic_hip_species_load_profile: a species loaded on the device from per-cell tables (count, charge, drift,
// thermal spread), the same particles for any decomposition of the global grid.  THE RULE is stated in include/vpic_hip.h
// and written once in load_rule.h; this file is the checks, the scan and the generating kernel.
//
// What a deck's `repeat(n) inject_particle(...)` loop over a profile does (decks/trecon-part/turbulence.cxx:518-620: a drift
// that turns with z, momenta boosted into the drift frame), without a host record per particle.
#include "engine.h"
#include "load_rule.h"
#include <cmath>
#include <cstring>
#include <algorithm>
#include <vector>

namespace vpichip {

// the tables of a call as the kernels see them: device pointers (null: reads 0) and the strides of a local cell
// (cx, cy, cz) from 0 into every table -- 0 along an axis the tables do not vary along
struct LoadK {
  const int *count;
  const float *q, *ud[3], *uth[3];
  int tsx, tsy, tsz;
  long long g0x, g0y, g0z, GX, GY;                  // this domain's first cell in the global grid, and that grid's extents
  unsigned seed, stream;
  int flip;
  const float *draws;                               // parity mode: 7 floats per particle place
  long long tag0;
};

// counts over the VOXELS of the grid, ghost voxels (and the entry behind the last) as 0: their exclusive scan is
// partition[] as sort_p.c:48-58 leaves it, and the offset of every cell in the call's order
__global__ __launch_bounds__(256)
void load_counts_kernel(int *__restrict__ per_voxel, int nv, GridK g, TileK t, LoadK k) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v > nv) return;
  int n = 0;
  if (v < nv) {
    int cx, cy, cz;
    voxel_cell(v, t, cx, cy, cz);
    if ((unsigned)(cx - 1) < (unsigned)g.nx && (unsigned)(cy - 1) < (unsigned)g.ny && (unsigned)(cz - 1) < (unsigned)g.nz)
      n = k.count[(cx - 1) * k.tsx + (cy - 1) * k.tsy + (cz - 1) * k.tsz];
  }
  per_voxel[v] = n;
}

// the voxel whose range holds place m: the largest v in [lo, hi) with off[v] <= m, given off[lo] <= m < off[hi]
template <typename T>
__device__ __forceinline__ int holding_voxel(const T *off, int lo, int hi, int m) {
  while (hi - lo > 1) {
    const int mid = lo + ((hi - lo) >> 1);
    if (off[mid] <= m) lo = mid; else hi = mid;
  }
  return lo;
}

// One thread per particle place m, 256 consecutive places per workgroup.  The workgroup searches off[] twice at full depth
// (the voxels of its first and last place); every thread then searches the span between them -- in LDS while it is short,
// in global memory when a run of empty voxels makes it long.  tags: 0 none, 1 tag0 + m, 2 zeros (a species that has tags
// receives particles without).
constexpr int LOAD_SPAN = 256;                      // voxels of a workgroup's span held in LDS (1 KiB): one per place, as in a grid at one particle per voxel
__global__ __launch_bounds__(256)
void load_profile_kernel(ParticlesK p, int64_t *__restrict__ tag, int64_t *__restrict__ tag2, int tags,
                         const int *__restrict__ off, int nv, int total, TileK t, LoadK k) {
  __shared__ int s_span[2];
  __shared__ int s_off[LOAD_SPAN + 2];
  const int m0 = (int)(blockIdx.x * 256u);
  const int m_last = min(m0 + 255, total - 1);
  if (threadIdx.x == 0) s_span[0] = holding_voxel(off, 0, nv, m0);
  if (threadIdx.x == 64) s_span[1] = holding_voxel(off, 0, nv, m_last);
  __syncthreads();
  const int v0 = s_span[0], v1 = s_span[1], span = v1 - v0;
  const bool in_lds = span < LOAD_SPAN;
  if (in_lds) {
    for (int a = threadIdx.x; a <= span + 1; a += 256) s_off[a] = off[v0 + a];       // (v1 + 1 <= nv: off[] has nv + 1 entries)
    __syncthreads();
  }
  const int m = m0 + (int)threadIdx.x;
  if (m >= total) return;
  int v, first;
  if (in_lds) { const int a = holding_voxel(s_off, 0, span + 1, m); v = v0 + a; first = s_off[a]; }
  else { v = holding_voxel(off, v0, v1 + 1, m); first = off[v]; }
  int cx, cy, cz;
  voxel_cell(v, t, cx, cy, cz);
  cx -= 1; cy -= 1; cz -= 1;
  const int at = cx * k.tsx + cy * k.tsy + cz * k.tsz;
  const uint64_t cell = load_global_cell((uint64_t)(k.g0x + cx), (uint64_t)(k.g0y + cy), (uint64_t)(k.g0z + cz), (uint64_t)k.GX, (uint64_t)k.GY);
  float d[7];
  if (k.draws) {
#pragma unroll
    for (int a = 0; a < 7; a++) d[a] = k.draws[7ll * m + a];
  } else {
    uint32_t r[8];
    load_words(cell, (uint32_t)(m - first), k.seed, k.stream, r);
    load_numbers(r, d);
  }
  float uth[3], ud[3], u[3];
#pragma unroll
  for (int a = 0; a < 3; a++) { uth[a] = k.uth[a] ? k.uth[a][at] : 0.f; ud[a] = k.ud[a] ? k.ud[a][at] : 0.f; }
  const float n[3] = {d[3], d[4], d[5]};
  load_momentum(uth, ud, n, d[6], k.flip != 0, u);
  p.r[m] = make_record(load_offset(d[0]), load_offset(d[1]), load_offset(d[2]), v);
  p.ux[m] = u[0]; p.uy[m] = u[1]; p.uz[m] = u[2]; p.q[m] = k.q[at];
  if (tags) { tag[m] = tags == 1 ? k.tag0 + m : 0; tag2[m] = 0; }
}

int k_load_profile(Engine *e, Species &s, const vpic_hip_load_t &d, int64_t *n_loaded) {
  const GridK &g = e->gk;
  const int n[3] = {g.nx, g.ny, g.nz};
  // ---- the refusals: nothing is touched before the last of them ----
  if (!d.count) VH_FAIL("load_profile: count is NULL");
  if (!d.q) VH_FAIL("load_profile: q is NULL");
  if (d.flags & ~(VPIC_HIP_LOAD_APPEND | VPIC_HIP_LOAD_FLIP | VPIC_HIP_LOAD_TAGS)) VH_FAIL("load_profile: flags = %d has unknown bits", d.flags);
  const bool append = d.flags & VPIC_HIP_LOAD_APPEND, with_tags = d.flags & VPIC_HIP_LOAD_TAGS;
  for (int a = 0; a < 3; a++) {
    if (d.tdim[a] != 1 && d.tdim[a] != n[a]) VH_FAIL("load_profile: tdim[%d] = %d is neither 1 nor the grid's %d", a, d.tdim[a], n[a]);
    if (d.goff[a] < 0) VH_FAIL("load_profile: goff[%d] = %lld is negative", a, (long long)d.goff[a]);
    if (d.goff[a] > d.gdim[a] - n[a]) VH_FAIL("load_profile: goff[%d] + %d = %lld is beyond gdim[%d] = %lld", a, n[a], (long long)d.goff[a] + n[a], a, (long long)d.gdim[a]);
  }
  if ((double)d.gdim[0] * (double)d.gdim[1] * (double)d.gdim[2] >= 9.2e18) VH_FAIL("load_profile: gdim holds more than 2^63 cells");
  const int64_t T = (int64_t)d.tdim[0] * d.tdim[1] * d.tdim[2], cells = (int64_t)g.nx * g.ny * g.nz, mult = cells / T;
  const size_t count_bytes = sizeof(int32_t) * (size_t)T, table_bytes = sizeof(float) * (size_t)T;
  host_will_read(d.count, count_bytes); host_will_read(d.q, table_bytes);
  for (int a = 0; a < 3; a++) { host_will_read(d.ud[a], table_bytes); host_will_read(d.uth[a], table_bytes); }
  int64_t sum = 0;
  float q_top = 0;
  for (int64_t c = 0; c < T; c++) {
    if (d.count[c] < 0) VH_FAIL("load_profile: count[%lld] = %d is negative", (long long)c, d.count[c]);
    if (!std::isfinite(d.q[c])) VH_FAIL("load_profile: q[%lld] is not finite", (long long)c);
    for (int a = 0; a < 3; a++) {
      if (d.ud[a] && !std::isfinite(d.ud[a][c])) VH_FAIL("load_profile: ud[%d][%lld] is not finite", a, (long long)c);
      if (d.uth[a] && !std::isfinite(d.uth[a][c])) VH_FAIL("load_profile: uth[%d][%lld] is not finite", a, (long long)c);
      if (d.uth[a] && d.uth[a][c] < 0) VH_FAIL("load_profile: uth[%d][%lld] = %g is negative", a, (long long)c, (double)d.uth[a][c]);
    }
    sum += d.count[c];
    if (d.count[c] > 0) q_top = std::max(q_top, fabsf(d.q[c]));
  }
  const int64_t total = sum * mult, at = append ? s.np : 0;
  if (total > 2147483647ll) VH_FAIL("load_profile: the counts add up to %lld particles, more than 2^31 - 1", (long long)total);
  if (at + total > s.max_np) VH_FAIL("load_profile: %lld particles behind %lld exceed max_np = %lld", (long long)total, (long long)at, (long long)s.max_np);
  if (e->load_draws_n > 0 && e->load_draws_n < total) VH_FAIL("load_profile: the draws table holds %lld particles, the counts add up to %lld", (long long)e->load_draws_n, (long long)total);
  if (s.nm > 0 || s.phase_pending) VH_FAIL("load_profile: the species has %lld pending movers", (long long)s.nm);
  if (n_loaded) *n_loaded = total;
  if (append && total == 0) return 0;                    // (as an append of no particles)

  // ---- the tables, as given, in one upload ----
  const float *tabs[7] = {d.q, d.ud[0], d.ud[1], d.ud[2], d.uth[0], d.uth[1], d.uth[2]};
  size_t bytes = count_bytes;
  for (const float *tab : tabs) if (tab) bytes += table_bytes;
  std::vector<char> host(bytes);
  memcpy(host.data(), d.count, count_bytes);
  if (grow(e->load_tab, e->load_tab_bytes, bytes)) return 1;
  LoadK k;
  memset(&k, 0, sizeof(k));
  k.count = reinterpret_cast<const int *>(e->load_tab);
  const float *dev[7];
  size_t used = count_bytes;
  for (int a = 0; a < 7; a++) {
    dev[a] = nullptr;
    if (!tabs[a]) continue;
    memcpy(host.data() + used, tabs[a], table_bytes);
    dev[a] = reinterpret_cast<const float *>(e->load_tab + used);
    used += table_bytes;
  }
  VH_CHECK(hipMemcpyAsync(e->load_tab, host.data(), bytes, hipMemcpyHostToDevice, e->stream));
  k.q = dev[0];
  for (int a = 0; a < 3; a++) { k.ud[a] = dev[1 + a]; k.uth[a] = dev[4 + a]; }
  k.tsx = d.tdim[0] > 1 ? 1 : 0; k.tsy = d.tdim[1] > 1 ? d.tdim[0] : 0; k.tsz = d.tdim[2] > 1 ? d.tdim[0] * d.tdim[1] : 0;
  k.g0x = d.goff[0]; k.g0y = d.goff[1]; k.g0z = d.goff[2]; k.GX = d.gdim[0]; k.GY = d.gdim[1];
  k.seed = d.seed; k.stream = d.stream; k.flip = (d.flags & VPIC_HIP_LOAD_FLIP) ? 1 : 0;
  k.draws = e->load_draws_n > 0 ? e->load_draws : nullptr;
  k.tag0 = d.tag0;

  // ---- the scan: counts per voxel -> partition[] (of a species that is appended to: scratch, it is not valid afterwards) ----
  const TileK tk = make_tile_k(g);
  const int nv = g.nv;
  if (!s.partition) VH_CHECK(hipMalloc(&s.partition, sizeof(int) * (nv + 1)));
  hipLaunchKernelGGL(load_counts_kernel, dim3((unsigned)(nv / 256 + 1)), dim3(256), 0, e->stream, e->sort_next, nv, g, tk, k);
  VH_CHECK(hipGetLastError());
  if (k_sort_scan(e, e->sort_next, s.partition, nv + 1)) return 1;

  // ---- the particles ----
  int tags = 0;
  if (with_tags) { if (ensure_tags(e, s)) return 1; tags = 1; }
  else if (append && s.has_tags) tags = 2;
  else if (!append && s.has_tags) {                      // the species loses its tags: whoever switches them on again finds zeros
    VH_CHECK(hipMemsetAsync(s.tag, 0, sizeof(int64_t) * s.max_np, e->stream));
    VH_CHECK(hipMemsetAsync(s.tag2, 0, sizeof(int64_t) * s.max_np, e->stream));
  }
  if (total > 0) {
    hipLaunchKernelGGL(load_profile_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, e->stream, offset_particles(s.p, at),
                       tags ? s.tag + at : nullptr, tags ? s.tag2 + at : nullptr, tags, (const int *)s.partition, nv, (int)total, tk, k);
    VH_CHECK(hipGetLastError());
  }
  VH_CHECK(hipStreamSynchronize(e->stream));             // (`host` and the caller's tables are free again)

  // ---- the books ----
  s.q_max = std::max(s.q_max, q_top);
  if (append) {                                          // as k_particles_from_aos behind the extent
    s.chargeless = q_top == 0 && (s.np == 0 || s.chargeless);
    if (with_tags) s.has_tags = true;
    s.np = at + total; s.partition_valid = false; s.hist_valid = false;
    return 0;
  }
  // as k_sort_p / k_sort_finish leave a species sorted by voxel
  s.chargeless = total > 0 && q_top == 0;
  s.has_tags = with_tags;
  s.np = total; s.nm = 0; s.n_holes = 0; s.hist_valid = false; s.fuse_pending = false; s.tail_sorted = false;
  s.partition_valid = true; s.tile_valid = false; s.n_sorted = s.np; s.coarse_sorted = false;
  if (s.crossed_dev) VH_CHECK(hipMemsetAsync(s.crossed_dev + 2, 0, sizeof(unsigned), e->stream));
  s.pol.new_cycle(false);
  return 0;
}

}  // namespace vpichip
