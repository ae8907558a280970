// cell_dist.hip -- a 1-D or 2-D histogram over the interior CELLS of the grid with up to four exact per-bin sums beside it
// (vpic_hip_cell_distribution; include/vpic_hip.h states the arithmetic): the descriptor, the counted test, the quantised
// 64-bit sums and the refusals of the per-bin sums of a species (distribution.hip), over coordinates of a cell -- its
// centre, the raw words of its field and hydro records, the fields at its centre by load_interpolator's expressions and
// what derives from them (cell_coords.h).  One lane per interior cell, grid-stride, x fastest: consecutive lanes read
// consecutive floats of every component array the descriptor names and of no other.  Every counter is an integer: the
// result does not depend on how the cells are dealt out nor on the path.  Which path a descriptor takes is the host
// decision of the species' sums (policy.h, plan_distribution_sums); how many workgroups, plan_cell_groups.
#include "cell_coords.h"

namespace vpichip {

constexpr int CELL_WAVES = 4;                  // wavefronts per workgroup

struct CellDistK {
  vpic_hip_dist_t d;
  vpic_hip_dist_value_t v[VPIC_HIP_DIST_MAX_VALUES];
  unsigned long long need;                     // cell_coords.h: the codes of the axes, the ranges and the factors, and what they are formed from
  int n0, n1, n_val;
};

// One pass over the interior cells; a workgroup takes 64 * CELL_WAVES consecutive cells at a time.
//   DIST_LDS: the workgroup's LDS holds n_val rows of 64-bit sums, then the 32-bit counts; added to global memory at the end.
//   DIST_GLOBAL: every counted cell adds to counts[] and sums[].
// Integer adds: any order and any grouping of them gives the same words.
// stats: cells seen, kept by the ranges, counted, counted through global memory, then the cells refused for each value.
template <int PATH>
__global__ __launch_bounds__(64 * CELL_WAVES)
void cell_distribution_kernel(FieldsK f, const float *__restrict__ hydro, CellGridK c, CellDistK k,
                              unsigned long long *__restrict__ counts, unsigned long long *__restrict__ sums,
                              unsigned long long *__restrict__ stats) {
  extern __shared__ unsigned long long s_cell_sums[];
  const int lane = threadIdx.x & 63;
  const int bins = k.n0 * k.n1;
  unsigned *s_counts = reinterpret_cast<unsigned *>(s_cell_sums + k.n_val * bins);
  if (PATH == DIST_LDS) {
    for (int j = threadIdx.x; j < k.n_val * bins; j += 64 * CELL_WAVES) s_cell_sums[j] = 0;
    for (int j = threadIdx.x; j < bins; j += 64 * CELL_WAVES) s_counts[j] = 0;
    __syncthreads();
  }
  unsigned long long n_seen = 0, n_kept = 0, n_counted = 0, n_refused[VPIC_HIP_DIST_MAX_VALUES] = {0, 0, 0, 0};
  const long long stride = (long long)gridDim.x * (64 * CELL_WAVES);
  for (long long at = (long long)blockIdx.x * (64 * CELL_WAVES) + (threadIdx.x & ~63); at < c.cells; at += stride) {
    const long long idx = at + lane;
    const bool live = idx < c.cells;                                         // (a wavefront whose first cell is inside: some lane is live)
    n_seen += __popcll(__ballot(live));
    int cx, cy, cz;                                                          // (a lane behind the last cell reads the last cell and counts nothing)
    const int voxel = cell_voxel(live ? (int)idx : c.cells - 1, c, cx, cy, cz);
    const CellCoords v = cell_coords(cell_load(f, hydro, voxel, c, k.need), cx, cy, cz, k.need);
    const bool kept = live && cell_in_ranges(v, k.d.sel, k.d.n_sel);
    n_kept += __popcll(__ballot(kept));
    bool counted = kept;
    int b0 = 0, b1 = 0;
    {
      const double t0 = (cell_coord(v, k.d.axis[0].coord) - k.d.axis[0].lo) / k.d.axis[0].d;
      counted = counted && t0 >= 0.0 && t0 < (double)k.n0;
      b0 = counted ? (int)t0 : 0;
    }
    if (k.d.n_axes == 2) {
      const double t1 = (cell_coord(v, k.d.axis[1].coord) - k.d.axis[1].lo) / k.d.axis[1].d;
      counted = counted && t1 >= 0.0 && t1 < (double)k.n1;
      b1 = counted ? (int)t1 : 0;
    }
    const unsigned long long counted_mask = __ballot(counted);
    n_counted += __popcll(counted_mask);
    if (!counted_mask) continue;
    const int a = b1 * k.n0 + b0;                                            // (below bins; 0 for a lane that is not counted)
    if (PATH == DIST_LDS) add_together(s_counts, a, counted, lane);
    else add_together(counts, a, counted, lane);

    const int lead = __ffsll((long long)counted_mask) - 1;
    const int a0 = __builtin_amdgcn_readlane(a, lead);
    const unsigned long long same = __ballot(counted && a == a0);
    const bool together = __popcll(same) >= SUMS_TOGETHER_MIN;
#pragma unroll
    for (int j = 0; j < VPIC_HIP_DIST_MAX_VALUES; j++) {
      if (j >= k.n_val) break;
      const vpic_hip_dist_value_t &val = k.v[j];
      const double product = (cell_coord(v, val.factor[0]) * cell_coord(v, val.factor[1])) * cell_coord(v, val.factor[2]);
      const double tq = product / val.quantum;
      const bool taken = counted && fabs(tq) < 4294967296.0;                 // (a NaN is refused)
      n_refused[j] += __popcll(__ballot(counted && !taken));
      const long long addend = taken ? llrint(tq) : 0;
      if (PATH == DIST_LDS) add_sums_together(s_cell_sums + j * bins, a, addend, taken, together, same, lead, lane);
      else add_sums_together(sums + (size_t)j * bins, a, addend, taken, together, same, lead, lane);
    }
  }
  if (lane == 0 && n_seen) {
    atomicAdd(&stats[0], n_seen);
    if (n_kept) atomicAdd(&stats[1], n_kept);
    if (n_counted) atomicAdd(&stats[2], n_counted);
    if (PATH == DIST_GLOBAL && n_counted) atomicAdd(&stats[3], n_counted);
#pragma unroll
    for (int j = 0; j < VPIC_HIP_DIST_MAX_VALUES; j++)
      if (n_refused[j]) atomicAdd(&stats[4 + j], n_refused[j]);
  }
  if (PATH == DIST_LDS) {
    __syncthreads();
    for (int j = threadIdx.x; j < bins; j += 64 * CELL_WAVES)
      if (s_counts[j]) atomicAdd(&counts[j], (unsigned long long)s_counts[j]);
    for (int j = threadIdx.x; j < k.n_val * bins; j += 64 * CELL_WAVES)
      if (s_cell_sums[j]) atomicAdd(&sums[j], s_cell_sums[j]);
  }
}

// the histogram and the sums of a checked descriptor into Engine::cell_counts / cell_host and cell_sums / cell_sums_host, the
// eight statistics into cell_last, after the stream has been waited for
int k_cell_distribution(Engine *e, const vpic_hip_dist_t &d, const vpic_hip_dist_value_t *v, int n_val) {
  CellDistK k{};
  k.d = d;
  k.n0 = d.axis[0].n; k.n1 = d.n_axes == 2 ? d.axis[1].n : 1;
  k.n_val = n_val;
  for (int a = 0; a < d.n_axes; a++) k.need |= cell_code_need(d.axis[a].coord);
  for (int r = 0; r < d.n_sel; r++) k.need |= cell_code_need(d.sel[r].coord);
  for (int j = 0; j < n_val; j++) {
    k.v[j] = v[j];
    for (int c = 0; c < 3; c++) k.need |= cell_code_need(v[j].factor[c]);
  }
  if ((k.need & CELL_NEED_HYDRO) && !e->hydro) VH_FAIL("cell distribution: a hydro code, and the hydro array was never allocated");
  const size_t bins = (size_t)k.n0 * (size_t)k.n1, words = bins * (size_t)n_val;
  const DistSumsPlan pl = plan_distribution_sums((long long)bins, n_val, VPIC_HIP_DIST_LDS_BINS);
  if (grow(e->cell_counts, e->cell_bins, bins) || grow_pinned(e->cell_host, e->cell_host_bins, bins) ||
      grow(e->cell_sums, e->cell_sums_words, words + 1) || grow_pinned(e->cell_sums_host, e->cell_sums_host_words, words + 1)) return 1;   // (+ 1: never an empty buffer)
  if (!e->cell_stats) VH_CHECK(hipMalloc((void **)&e->cell_stats, CELL_DIST_STATS * sizeof(unsigned long long)));
  if (!e->cell_stats_host) VH_CHECK(hipHostMalloc((void **)&e->cell_stats_host, CELL_DIST_STATS * sizeof(unsigned long long), hipHostMallocDefault));
  VH_CHECK(hipMemsetAsync(e->cell_stats, 0, CELL_DIST_STATS * sizeof(unsigned long long), e->stream));
  VH_CHECK(hipMemsetAsync(e->cell_counts, 0, bins * sizeof(unsigned long long), e->stream));
  if (words) VH_CHECK(hipMemsetAsync(e->cell_sums, 0, words * sizeof(unsigned long long), e->stream));
  const CellGridK c = make_cell_grid_k(e->gk);
  const long long groups = plan_cell_groups(c.cells, 64 * CELL_WAVES);
  const size_t lds = sizeof(unsigned) * (size_t)pl.words;
  auto kernel = pl.path == DIST_LDS ? cell_distribution_kernel<DIST_LDS> : cell_distribution_kernel<DIST_GLOBAL>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)groups), dim3(64 * CELL_WAVES), lds, e->stream, e->f, (const float *)e->hydro, c, k,
                     e->cell_counts, e->cell_sums, e->cell_stats);
  VH_CHECK(hipGetLastError());
  VH_CHECK(hipMemcpyAsync(e->cell_host, e->cell_counts, bins * sizeof(unsigned long long), hipMemcpyDeviceToHost, e->stream));
  if (words) VH_CHECK(hipMemcpyAsync(e->cell_sums_host, e->cell_sums, words * sizeof(unsigned long long), hipMemcpyDeviceToHost, e->stream));
  VH_CHECK(hipMemcpyAsync(e->cell_stats_host, e->cell_stats, CELL_DIST_STATS * sizeof(unsigned long long), hipMemcpyDeviceToHost, e->stream));
  VH_CHECK(hipStreamSynchronize(e->stream));
  for (int j = 0; j < CELL_DIST_STATS; j++) e->cell_last[j] = (int64_t)e->cell_stats_host[j];
  return 0;
}

}  // namespace vpichip
