// hist_device.h -- the steps the histogram kernels share (distribution.hip: a species' counts and its per-bin sums;
// cell_dist.hip: the cells' counts and sums; include/vpic_hip.h states the one arithmetic of all three): the counted
// test, the values of a bin's sums, the LDS block of the sums' kernels and the statistics.  What a coordinate or a factor
// IS stays with the caller (dist_coords.h, cell_coords.h): it comes in as a functor over the code, so that a select chain
// stays a select chain.
#pragma once
#include "engine.h"
#include <math.h>

namespace vpichip {

// the head DistSumsK and CellDistK share (their `need` masks are of different types)
struct HistK {
  vpic_hip_dist_t d;
  vpic_hip_dist_value_t v[VPIC_HIP_DIST_MAX_VALUES];
  int n0, n1, n_val;                           // bins per axis (n1 = 1 for one axis), values
};
// (host) of a checked descriptor and its n_val checked values
inline void fill_hist_k(HistK &k, const vpic_hip_dist_t &d, const vpic_hip_dist_value_t *v, int n_val) {
  k.d = d;
  k.n0 = d.axis[0].n; k.n1 = d.n_axes == 2 ? d.axis[1].n : 1;
  k.n_val = n_val;
  for (int j = 0; j < n_val; j++) k.v[j] = v[j];
}

// THE COUNTED TEST: a kept lane is counted when (coordinate - lo) / d of every axis, in double, is in [0, n); its bin is
// the truncation.  a = b1 * n0 + b0 is below n0 * n1, and 0 for a lane that is not counted.
struct HistBin { bool counted; int b0, b1, a; };
template <typename Coord>
__device__ __forceinline__ HistBin hist_bin(bool kept, const vpic_hip_dist_t &d, int n0, int n1, Coord coord) {
  HistBin h{kept, 0, 0, 0};
  {
    const double t0 = (coord(d.axis[0].coord) - d.axis[0].lo) / d.axis[0].d;
    h.counted = h.counted && t0 >= 0.0 && t0 < (double)n0;
    h.b0 = h.counted ? (int)t0 : 0;
  }
  if (d.n_axes == 2) {
    const double t1 = (coord(d.axis[1].coord) - d.axis[1].lo) / d.axis[1].d;
    h.counted = h.counted && t1 >= 0.0 && t1 < (double)n1;
    h.b1 = h.counted ? (int)t1 : 0;
  }
  h.a = h.b1 * n0 + h.b0;
  return h;
}

// THE VALUES of a pass in which some lane is counted (counted_mask, not 0): value j is the product of its three factors,
// from the left, over its quantum, rounded to the nearest even integer; |t| >= 2^32 is refused and counted in n_refused[j].
// rows: n_val rows of `bins` 64-bit sums, in LDS or in global memory.
template <typename Factor>
__device__ __forceinline__ void hist_add_values(const HistK &k, int bins, const HistBin &h, unsigned long long counted_mask, Factor factor,
                                                unsigned long long *rows, unsigned long long (&n_refused)[VPIC_HIP_DIST_MAX_VALUES], int lane) {
  const int lead = __ffsll((long long)counted_mask) - 1;
  const int a0 = __builtin_amdgcn_readlane(h.a, lead);
  const unsigned long long same = __ballot(h.counted && h.a == a0);
  const bool together = __popcll(same) >= SUMS_TOGETHER_MIN;
#pragma unroll
  for (int j = 0; j < VPIC_HIP_DIST_MAX_VALUES; j++) {
    if (j >= k.n_val) break;
    const vpic_hip_dist_value_t &val = k.v[j];
    const double product = (factor(val.factor[0]) * factor(val.factor[1])) * factor(val.factor[2]);
    const double tq = product / val.quantum;
    const bool taken = h.counted && fabs(tq) < 4294967296.0;                 // (a NaN is refused)
    n_refused[j] += __popcll(__ballot(h.counted && !taken));
    const long long addend = taken ? llrint(tq) : 0;
    add_sums_together(rows + (size_t)j * bins, h.a, addend, taken, together, same, lead, lane);
  }
}

// THE LDS BLOCK of a workgroup of THREADS threads: n_val rows of 64-bit sums, then the 32-bit counts (policy.h,
// plan_distribution_sums, sizes it); cleared before the pass, added to global memory behind it (the non-zero words only)
template <int THREADS>
__device__ __forceinline__ void hist_lds_clear(unsigned long long *s_sums, unsigned *s_counts, int n_val, int bins) {
  for (int j = threadIdx.x; j < n_val * bins; j += THREADS) s_sums[j] = 0;
  for (int j = threadIdx.x; j < bins; j += THREADS) s_counts[j] = 0;
  __syncthreads();
}
template <int THREADS>
__device__ __forceinline__ void hist_lds_flush(const unsigned long long *s_sums, const unsigned *s_counts, int n_val, int bins,
                                               unsigned long long *__restrict__ counts, unsigned long long *__restrict__ sums) {
  __syncthreads();
  for (int j = threadIdx.x; j < bins; j += THREADS)
    if (s_counts[j]) atomicAdd(&counts[j], (unsigned long long)s_counts[j]);
  for (int j = threadIdx.x; j < n_val * bins; j += THREADS)
    if (s_sums[j]) atomicAdd(&sums[j], s_sums[j]);
}

// THE STATISTICS of a wavefront, added once by its first lane: seen, kept by the ranges, counted, through global memory
// (the counts' window: misses), then -- the sums' kernels only, n_refused not null -- refused for each value
__device__ __forceinline__ void hist_publish(unsigned long long *__restrict__ stats, int lane, unsigned long long n_seen, unsigned long long n_kept,
                                             unsigned long long n_counted, unsigned long long n_global, const unsigned long long *n_refused = nullptr) {
  if (lane == 0 && n_seen) {
    atomicAdd(&stats[0], n_seen);
    if (n_kept) atomicAdd(&stats[1], n_kept);
    if (n_counted) atomicAdd(&stats[2], n_counted);
    if (n_global) atomicAdd(&stats[3], n_global);
    if (n_refused) {
#pragma unroll
      for (int j = 0; j < VPIC_HIP_DIST_MAX_VALUES; j++)
        if (n_refused[j]) atomicAdd(&stats[4 + j], n_refused[j]);
    }
  }
}

}  // namespace vpichip
