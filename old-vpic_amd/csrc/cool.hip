// cool.hip -- radiative cooling of one species: the leading terms of the Landau-Lifshitz force (synchrotron losses) and
// the Thomson drag of an isotropic photon bath (vpic_hip_species_cool; include/vpic_hip.h states THE RULE, operation by
// operation, and tests/cool_ref.py restates it in numpy).  One streaming launch over [0, np): per particle the 16-byte
// record, the three momenta, q and the 72 bytes of its voxel's interpolator record are read and 12 bytes are written.
// The loads (dist_load, dist_load_q) and the gather are dist_coords.h's, and so are the fields at the particle (dist_b_at,
// dist_e_at): there is no second statement of them here.  Everything behind them is double, unfused (the library is
// built -ffp-contract=off).  The species' sum is an integer per lane, added up across the wavefront behind the loop, one add per wavefront; the
// per-voxel sums are 64-bit global adds after the lanes that share a voxel have combined (add_sums_together, engine.h).
#include "dist_coords.h"
#include <algorithm>

namespace vpichip {

constexpr int COOL_WAVES = 4;                              // wavefronts per workgroup
constexpr int COOL_THREADS = 64 * COOL_WAVES;
constexpr int COOL_MAX_BLOCKS = 1024;                      // each thread takes every (gridDim.x * COOL_THREADS)-th particle
constexpr int COOL_TOGETHER_ROUNDS = 2;                    // voxels of a pass whose lanes combine before they add (a sorted species: one or two)
// what the pass asks of dist_load and dist_gather: the momenta and the whole record, E included
constexpr unsigned COOL_NEED = NEED_FIELD;
enum { COOL_SEEN = 0, COOL_CHANGED, COOL_REFUSED, COOL_ALONE, COOL_SUM };

struct CoolK { double sync, ic, quantum; };

// DRY: no momentum is written.  CELLS: cells[nv] takes the per-voxel sums.
template <bool DRY, bool CELLS>
__global__ __launch_bounds__(COOL_THREADS)
void cool_kernel(ParticlesK p, long long np, CoolK k, int nv, const vpic_interpolator_t *__restrict__ fi,
                 unsigned long long *__restrict__ cells, unsigned long long *__restrict__ stats) {
  const int lane = threadIdx.x & 63;
  const long long stride = (long long)gridDim.x * COOL_THREADS;
  long long idx = (long long)blockIdx.x * COOL_THREADS + threadIdx.x;
  unsigned long long n_seen = 0, n_changed = 0, n_refused = 0, n_alone = 0;
  long long sum = 0;
  DistRaw next = dist_load<true>(p, idx, np, COOL_NEED);
  float next_q = dist_load_q(p, idx, np, VAL_Q);
  // (idx - lane is the same for the whole wavefront: every lane of it makes the same passes)
  for (; idx - lane < np; idx += stride) {
    const DistRaw r = next;
    const float q = next_q;
    const DistField f = dist_gather(fi, r.voxel, nv, COOL_NEED);               // (by live lanes only)
    next = dist_load<true>(p, idx + stride, np, COOL_NEED);
    next_q = dist_load_q(p, idx + stride, np, VAL_Q);
    const bool live = r.voxel >= 0 && r.voxel < nv;                            // i < 0: a dead slot (engine.h, Species::n_holes)
    n_seen += __popcll(__ballot(live));
    bool tallied = false;
    long long addend = 0;
    if (live) {
      const float3 el = dist_e_at(r, f), cb = dist_b_at(r, f);
      const double Ex = (double)el.x, Ey = (double)el.y, Ez = (double)el.z, Bx = (double)cb.x, By = (double)cb.y, Bz = (double)cb.z;
      const double ux = (double)r.ux, uy = (double)r.uy, uz = (double)r.uz;
      const double u2 = (ux * ux + uy * uy) + uz * uz, g = sqrt(1.0 + u2), rg = 1.0 / g;
      const double vx = ux * rg, vy = uy * rg, vz = uz * rg;
      const double Lx = Ex + (vy * Bz - vz * By), Ly = Ey + (vz * Bx - vx * Bz), Lz = Ez + (vx * By - vy * Bx);
      const double vE = (vx * Ex + vy * Ey) + vz * Ez;
      const double Ax = (Ly * Bz - Lz * By) + vE * Ex, Ay = (Lz * Bx - Lx * Bz) + vE * Ey, Az = (Lx * By - Ly * Bx) + vE * Ez;
      const double L2 = (Lx * Lx + Ly * Ly) + Lz * Lz;
      double chi = L2 - vE * vE;
      if (chi < 0.0) chi = 0.0;                                                // (a NaN stays a NaN)
      const double D = g * (k.sync * chi + k.ic), den = 1.0 + D;
      const double nx = (ux + k.sync * Ax) / den, ny = (uy + k.sync * Ay) / den, nz = (uz + k.sync * Az) / den;
      if (isfinite(D) && isfinite(nx) && isfinite(ny) && isfinite(nz)) {
        const float fx = (float)nx, fy = (float)ny, fz = (float)nz;
        if (__float_as_uint(fx) != __float_as_uint(r.ux) || __float_as_uint(fy) != __float_as_uint(r.uy) ||
            __float_as_uint(fz) != __float_as_uint(r.uz)) n_changed++;
        if (!DRY) { p.ux[idx] = fx; p.uy[idx] = fy; p.uz[idx] = fz; }
        const double wx = (double)fx, wy = (double)fy, wz = (double)fz;
        const double u2n = (wx * wx + wy * wy) + wz * wz, g1 = sqrt(1.0 + u2n);
        const double val = (double)fabsf(q) * ((u2 - u2n) / (g + g1));
        const double t = val / k.quantum;
        tallied = fabs(t) < 4294967296.0;                                      // (a NaN is refused)
        if (tallied) { addend = llrint(t); sum += addend; }
        else n_refused++;
      } else n_alone++;
    }
    if (CELLS) {
      // the lanes of the first tallied lane's voxel add once, then those of the next voxel; what is left adds for itself
      bool pending = tallied;
#pragma unroll
      for (int round = 0; round < COOL_TOGETHER_ROUNDS; round++) {
        const unsigned long long any = __ballot(pending);
        if (!any) break;
        const int lead = __ffsll((long long)any) - 1;
        const int v0 = __builtin_amdgcn_readlane(r.voxel, lead);
        const bool shared = pending && r.voxel == v0;
        const unsigned long long same = __ballot(shared);
        add_sums_together(cells, r.voxel, addend, shared, __popcll(same) >= SUMS_TOGETHER_MIN, same, lead, lane);
        pending = pending && !shared;
      }
      if (pending && addend) atomicAdd(cells + r.voxel, (unsigned long long)addend);
    }
  }
  // per-lane counts and the per-lane sum, added up across the wavefront: its first lane adds once
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    sum += __shfl_xor(sum, m);
    n_changed += __shfl_xor(n_changed, m);
    n_refused += __shfl_xor(n_refused, m);
    n_alone += __shfl_xor(n_alone, m);
  }
  if (lane == 0 && n_seen) {
    atomicAdd(&stats[COOL_SEEN], n_seen);
    if (n_changed) atomicAdd(&stats[COOL_CHANGED], n_changed);
    if (n_refused) atomicAdd(&stats[COOL_REFUSED], n_refused);
    if (n_alone) atomicAdd(&stats[COOL_ALONE], n_alone);
    if (sum) atomicAdd(&stats[COOL_SUM], (unsigned long long)sum);             // (two's complement: the unsigned add is the signed one)
  }
}

// One launch and the read of its sums.  Every allocation comes before the launch: a failure leaves the species alone.
// Fills Engine::cool_stats.last ({seen, changed, refused, left alone, the sum}) and, with cells, cool_cells_host[nv].
int k_species_cool(Engine *e, Species &s, const vpic_hip_cool_t &c, bool cells) {
  const long long np = s.np;
  const size_t nv = (size_t)e->gk.nv;
  if (cells && HistResult::grow_pair(e->cool_cells, e->cool_cells_host, e->cool_cells_n, nv)) return 1;
  if (e->cool_stats.begin(e->stream)) return 1;
  if (cells) VH_CHECK(hipMemsetAsync(e->cool_cells, 0, nv * sizeof(unsigned long long), e->stream));
  if (np > 0) {
    const bool dry = (c.flags & VPIC_HIP_COOL_DRY) != 0;
    const unsigned nb = (unsigned)std::min<long long>((np + COOL_THREADS - 1) / COOL_THREADS, COOL_MAX_BLOCKS);
    auto kernel = dry ? (cells ? cool_kernel<true, true> : cool_kernel<true, false>) : (cells ? cool_kernel<false, true> : cool_kernel<false, false>);
    hipLaunchKernelGGL(kernel, dim3(nb), dim3(COOL_THREADS), 0, e->stream, s.p, np, CoolK{c.sync, c.ic, c.quantum}, e->gk.nv,
                       (const vpic_interpolator_t *)e->fi, cells ? e->cool_cells : nullptr, e->cool_stats.dev);
    VH_CHECK(hipGetLastError());
  }
  if (cells) VH_CHECK(hipMemcpyAsync(e->cool_cells_host, e->cool_cells, nv * sizeof(unsigned long long), hipMemcpyDeviceToHost, e->stream));
  return e->cool_stats.read(e->stream);
}

}  // namespace vpichip
