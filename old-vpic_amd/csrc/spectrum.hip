// spectrum.hip -- kinetic-energy spectra of one species from the resident SoA arrays (vpic_hip_energy_spectrum,
// vpic_hip_energy_bands; include/vpic_hip.h).  What the production deck's diagnostic computes on the host
// (decks/trecon-part/energy.cxx:96-108 the counting, :116-162 the normalisation and the ghost fill), as one
// streaming pass over i, ux, uy, uz (16 B per particle).  Every counter is an integer: the result does not depend
// on the order of the array nor on which kernel instance pushed it.  The window's size and the launch shape are host
// decisions in policy.h (spectrum_window, plan_chunks); the window protocol, add_together and the statistics block are
// the ones every pass over a species uses (engine.h).
#include "engine.h"

namespace vpichip {

constexpr int SPEC_WAVES = 4;                  // wavefronts per workgroup

struct SpectrumK {
  int n_lin, n_log, win;                       // win: sort keys per window (policy.h, spectrum_window; 0: no window, every particle adds to global memory)
  double d_lin, log_lo, d_log;
};

// the window of linear bands: `win` consecutive sort keys x n_lin counters, [slot * n_lin + band]
// (sort keys: engine.h, sort_key -- by voxel, or tile-major when the species is in tile order)

// voxel of a sort key (the inverse of sort_key<TILE>), or -1 where the key names no interior voxel (a cell of a
// partial tile beyond the grid, a key past the last voxel)
template <bool TILE>
__device__ __forceinline__ int voxel_of_key(int key, const GridK &g, const TileK &t) {
  if (!TILE) return key < g.nv ? key : -1;
  const int tile = key >> 6, c = key & 63;
  if (tile >= t.ntiles) return -1;
  const int tz = tile / (t.ntx * t.nty), r = tile - tz * (t.ntx * t.nty), ty = r / t.ntx, tx = r - ty * t.ntx;
  const int x = 4 * tx + (c & 3) + 1, y = 4 * ty + ((c >> 2) & 3) + 1, z = 4 * tz + (c >> 4) + 1;
  if (x > g.nx || y > g.ny || z > g.nz) return -1;
  return x + g.sy * y + g.sz * z;
}

// add a wavefront's window to the global counters and clear it (the non-zero entries only)
template <bool TILE>
__device__ __forceinline__ void flush_window(unsigned *win, int base, const SpectrumK &k, const GridK &g, const TileK &t,
                                             unsigned *__restrict__ lin, int lane) {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");                     // (the other lanes' adds to the window are in LDS order before these reads)
  for (int slot = lane; slot < k.win; slot += 64) {
    const int voxel = voxel_of_key<TILE>(base + slot, g, t);
    for (int b = 0; b < k.n_lin; b++) {
      const unsigned c = win[slot * k.n_lin + b];
      if (c) {
        if (voxel >= 0) atomicAdd(lin + (size_t)b * g.nv + voxel, c);
        win[slot * k.n_lin + b] = 0;
      }
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
}

// One pass over the species.  Every wavefront takes a contiguous chunk of the array and keeps its own window in LDS,
// so nothing but the log histogram needs a workgroup barrier.  Per pass of 64 particles: the lanes whose key is inside
// the window add there; if some are not, the window is flushed and moved to the key of the first of them (in an
// ordered array the smallest), and they try again, twice at the most (two slides: 64 particles that straddle a
// boundary between tiles, or the ghost voxels between two rows or planes, still all hit); what does not fit then adds
// to global memory and is counted as a miss (the protocol: engine.h, window_add).
// stats[0]: live particles seen, stats[1]: misses.
template <bool TILE>
__global__ __launch_bounds__(64 * SPEC_WAVES)
void energy_spectrum_kernel(const float4 *__restrict__ prec, const float *__restrict__ pux, const float *__restrict__ puy,
                            const float *__restrict__ puz, long long np, long long chunk, SpectrumK k, GridK g, TileK t,
                            unsigned *__restrict__ lin, unsigned long long *__restrict__ logc,
                            unsigned long long *__restrict__ stats) {
  extern __shared__ unsigned s_mem[];
  unsigned *s_log = s_mem;                                                   // n_log counters of the workgroup
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned *win = s_mem + k.n_log + wave * (k.win * k.n_lin);                // this wavefront's window
  for (int j = threadIdx.x; j < k.n_log + SPEC_WAVES * k.win * k.n_lin; j += 64 * SPEC_WAVES) s_mem[j] = 0;
  __syncthreads();

  const long long w = (long long)blockIdx.x * SPEC_WAVES + wave;
  const long long begin = w * chunk, end = begin + chunk < np ? begin + chunk : np;
  SlideWindow w_state;
  unsigned long long n_seen = 0, n_miss = 0;
  for (long long at = begin; at < end; at += 64) {
    const long long idx = at + lane;
    const int voxel = idx < end ? record_cell(prec, idx) : -1;   // (the cell word of the position record: a 16-byte stride)
    const bool live = voxel >= 0 && voxel < g.nv;                            // i < 0: a dead slot (engine.h, Species::n_holes)
    n_seen += __popcll(__ballot(live));
    if (!__any(live)) continue;
    double ke = 0;
    if (live) {
      const float ux = pux[idx], uy = puy[idx], uz = puz[idx];
      // energy.cxx:99-100 as include/vpic_hip.h states it: the float momenta promoted, then everything in double, summed from the left
      const double gam2 = ((1.0 + (double)ux * (double)ux) + (double)uy * (double)uy) + (double)uz * (double)uz;
      ke = sqrt(gam2) - 1.0;
    }
    if (k.n_log > 0 && live) {
      // energy.cxx:107-108: the conversion truncates toward zero, so bin 0 takes (-1, 1); ke == 0 gives -inf and no bin
      const double x = (log10(ke) - k.log_lo) / k.d_log + 1.0;
      if (x > -1.0 && x < (double)k.n_log) atomicAdd(&s_log[(int)x], 1u);
    }
    if (k.n_lin > 0) {
      int band = 0, key = 0;
      bool pending = live;
      if (live) {
        // energy.cxx:102-103
        const double q = ke / k.d_lin;
        band = q < (double)(k.n_lin - 1) ? (int)q : k.n_lin - 1;
        if (band < 0) band = 0;
        key = sort_key<TILE>(voxel, t);
        if (TILE) {
          // sort_key files a voxel of a ghost layer under the nearest interior cell: such a particle is counted in
          // its own voxel, through global memory
          int cx, cy, cz;
          voxel_cell(voxel, t, cx, cy, cz);
          if (cx < 1 || cx > g.nx || cy < 1 || cy > g.ny || cz < 1 || cz > g.nz) key = -1;
        }
      }
      // the window goes to the key of the first lane still waiting (in an ordered array the smallest); key < 0 never slides it
      if (k.win > 0)
        pending = window_add(w_state, win, k.win, k.n_lin, key, band, pending, lane,
          [&](unsigned long long left) {
            const int first = __builtin_amdgcn_readlane(key, __ffsll((long long)left) - 1);
            return TILE ? first & ~63 : first;                               // a tile's cells come in any order when it is sorted by tile only
          },
          [&](int base) { flush_window<TILE>(win, base, k, g, t, lin, lane); });
      if (pending) atomicAdd(lin + (size_t)band * g.nv + voxel, 1u);
      n_miss += __popcll(__ballot(pending));
    }
  }
  if (k.n_lin > 0 && k.win > 0 && w_state.placed) flush_window<TILE>(win, w_state.base, k, g, t, lin, lane);
  if (lane == 0 && n_seen) { atomicAdd(&stats[0], n_seen); if (n_miss) atomicAdd(&stats[1], n_miss); }
  __syncthreads();
  for (int j = threadIdx.x; j < k.n_log; j += 64 * SPEC_WAVES)
    if (s_log[j]) atomicAdd(&logc[j], (unsigned long long)s_log[j]);
}

// energy.cxx:116-162, one thread per voxel: every voxel's bands over the sum of its bands, a ghost voxel takes the
// bands of the interior voxel next to it (each index clamped into [1, n])
__global__ __launch_bounds__(256)
void energy_bands_kernel(const unsigned *__restrict__ lin, float *__restrict__ bands, int n_lin, GridK g) {
  const int v = blockIdx.x * 256 + threadIdx.x;
  if (v >= g.nv) return;
  const int z = v / g.sz, r = v - z * g.sz, y = r / g.sy, x = r - y * g.sy;
  const int xs = min(max(x, 1), g.nx), ys = min(max(y, 1), g.ny), zs = min(max(z, 1), g.nz);
  const int src = xs + g.sy * ys + g.sz * zs;
  unsigned long long n = 0;
  for (int b = 0; b < n_lin; b++) n += lin[(size_t)b * g.nv + src];
  for (int b = 0; b < n_lin; b++)
    bands[(size_t)b * g.nv + v] = n ? (float)((double)lin[(size_t)b * g.nv + src] / (double)n) : 0.f;
}

// counts of species s into Engine::spec_lin / spec_log (device); the log counts land in spec_log_host (pinned), after the
// stream has been waited for
int k_energy_spectrum(Engine *e, Species &s, const vpic_hip_spectrum_t &sp) {
  const size_t lin_words = (size_t)sp.n_lin * (size_t)e->gk.nv;
  if (!e->spec_log) VH_CHECK(hipMalloc((void **)&e->spec_log, VPIC_HIP_SPECTRUM_MAX_LOG * sizeof(unsigned long long)));
  if (!e->spec_log_host) VH_CHECK(hipHostMalloc((void **)&e->spec_log_host, VPIC_HIP_SPECTRUM_MAX_LOG * sizeof(unsigned long long), hipHostMallocDefault));
  size_t bands_words = e->spec_lin_words;                                     // (the two grow together: one size for both)
  if (grow(e->spec_lin, e->spec_lin_words, lin_words) || grow(e->spec_bands, bands_words, lin_words)) { e->spec_lin_words = 0; return 1; }
  if (e->spec_stats.begin(e->stream)) return 1;
  SpectrumK k{};
  k.n_lin = sp.n_lin; k.n_log = sp.n_log; k.d_lin = sp.d_lin; k.log_lo = sp.log_lo; k.d_log = sp.d_log;
  k.win = spectrum_window(sp.n_lin);
  if (lin_words) VH_CHECK(hipMemsetAsync(e->spec_lin, 0, lin_words * sizeof(unsigned), e->stream));
  if (sp.n_log) VH_CHECK(hipMemsetAsync(e->spec_log, 0, (size_t)sp.n_log * sizeof(unsigned long long), e->stream));
  if (s.np > 0) {
    const Chunks ch = plan_chunks(s.np, SPEC_WAVES);
    const size_t lds = sizeof(unsigned) * ((size_t)sp.n_log + (size_t)SPEC_WAVES * k.win * sp.n_lin);
    const TileK tk = make_tile_k(e->gk);
    auto kernel = s.tile_valid ? energy_spectrum_kernel<true> : energy_spectrum_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)ch.groups), dim3(64 * SPEC_WAVES), lds, e->stream, (const float4 *)s.p.r, s.p.ux, s.p.uy, s.p.uz,
                       (long long)s.np, ch.chunk, k, e->gk, tk, e->spec_lin, e->spec_log, e->spec_stats.dev);
    VH_CHECK(hipGetLastError());
  }
  if (sp.n_log) VH_CHECK(hipMemcpyAsync(e->spec_log_host, e->spec_log, (size_t)sp.n_log * sizeof(unsigned long long), hipMemcpyDeviceToHost, e->stream));
  return e->spec_stats.read(e->stream);
}

int k_energy_bands(Engine *e, int n_lin) {
  hipLaunchKernelGGL(energy_bands_kernel, dim3((e->gk.nv + 255) / 256), dim3(256), 0, e->stream, e->spec_lin, e->spec_bands, n_lin, e->gk);
  VH_CHECK(hipGetLastError());
  return 0;
}

}  // namespace vpichip
