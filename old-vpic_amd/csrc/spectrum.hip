// spectrum.hip -- kinetic-energy spectra of one species from the resident SoA arrays (vpic_hip_energy_spectrum,
// vpic_hip_energy_bands; include/vpic_hip.h).  What the production deck's diagnostic computes on the host
// (decks/trecon-part/energy.cxx:96-108 the counting, :116-162 the normalisation and the ghost fill), as one
// streaming pass over i, ux, uy, uz (16 B per particle).  Every counter is an integer: the result does not depend
// on the order of the array nor on which kernel instance pushed it.
#include "engine.h"

namespace vpichip {

constexpr int SPEC_WAVES = 4;                  // wavefronts per workgroup
constexpr int SPEC_WIN_WORDS = 3072;           // LDS words a wavefront's window of linear bands may take (12 KB)
constexpr int SPEC_WIN_KEYS = 128;             // ... and the most sort keys it spans
constexpr int SPEC_BACKOFF = 16;               // passes a wavefront leaves its window where it is after a slide did not help

struct SpectrumK {
  int n_lin, n_log, win;                       // win: sort keys per window (0: no window, every particle adds to global memory)
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
// to global memory and is counted as a miss.  When more than half the wavefront still misses after that, the
// window stays where it is for the next SPEC_BACKOFF passes (an array in no order: the window cannot help, and
// flushing it every pass would only cost).
// stats[0]: live particles seen, stats[1]: misses.
template <bool TILE>
__global__ __launch_bounds__(64 * SPEC_WAVES)
void energy_spectrum_kernel(const int *__restrict__ pi, const float *__restrict__ pux, const float *__restrict__ puy,
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
  int base = 0, backoff = 0;
  bool placed = false;                                                       // the window has been given a place
  unsigned long long n_seen = 0, n_miss = 0;
  for (long long at = begin; at < end; at += 64) {
    const long long idx = at + lane;
    const int voxel = idx < end ? pi[idx] : -1;
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
          const int cz = (int)(__umulhi((unsigned)voxel, t.mul_sz) >> t.sh_sz), rem = voxel - cz * t.sz;
          const int cy = (int)(__umulhi((unsigned)rem, t.mul_sy) >> t.sh_sy), cx = rem - cy * t.sy;
          if (cx < 1 || cx > g.nx || cy < 1 || cy > g.ny || cz < 1 || cz > g.nz) key = -1;
        }
      }
      for (int round = 0; round < 3 && k.win > 0; round++) {
        if (round > 0) {
          const unsigned long long left = __ballot(pending && key >= 0);
          if (!left) break;
          if (backoff > 0) { backoff--; break; }
          if (placed) flush_window<TILE>(win, base, k, g, t, lin, lane);
          const int first = __builtin_amdgcn_readlane(key, __ffsll((long long)left) - 1);
          base = TILE ? first & ~63 : first;                                 // a tile's cells come in any order when it is sorted by tile only
          placed = true;
        }
        const bool hit = placed && pending && key >= base && key < base + k.win;
        if (hit) {
          // most of a wavefront is in one voxel and one band: the lanes that share the first hit's word add once, together
          // (more rounds of this, word by word, measured slower than letting the others add for themselves)
          const int a = (key - base) * k.n_lin + band;
          const int lead = __ffsll((long long)__ballot(hit)) - 1, a0 = __shfl(a, lead);
          const unsigned long long same = __ballot(a == a0);
          if (a != a0) atomicAdd(win + a, 1u);
          else if (lane == lead) atomicAdd(win + a, (unsigned)__popcll(same));
          pending = false;
        }
        if (round == 2 && __popcll(__ballot(pending)) > 32) backoff = SPEC_BACKOFF;
      }
      if (pending) atomicAdd(lin + (size_t)band * g.nv + voxel, 1u);
      n_miss += __popcll(__ballot(pending));
    }
  }
  if (k.n_lin > 0 && k.win > 0 && placed) flush_window<TILE>(win, base, k, g, t, lin, lane);
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

static int ensure_spectrum(Engine *e, size_t lin_words, size_t log_words) {
  if (!e->spec_stats) {
    VH_CHECK(hipMalloc((void **)&e->spec_stats, 2 * sizeof(unsigned long long)));
    VH_CHECK(hipHostMalloc((void **)&e->spec_host, (2 + VPIC_HIP_SPECTRUM_MAX_LOG) * sizeof(unsigned long long), hipHostMallocDefault));
    VH_CHECK(hipMalloc((void **)&e->spec_log, VPIC_HIP_SPECTRUM_MAX_LOG * sizeof(unsigned long long)));
  }
  (void)log_words;
  if (lin_words > e->spec_lin_words) {
    (void)hipFree(e->spec_lin); (void)hipFree(e->spec_bands);
    e->spec_lin = nullptr; e->spec_bands = nullptr; e->spec_lin_words = 0;
    VH_CHECK(hipMalloc((void **)&e->spec_lin, lin_words * sizeof(unsigned)));
    VH_CHECK(hipMalloc((void **)&e->spec_bands, lin_words * sizeof(float)));
    e->spec_lin_words = lin_words;
  }
  return 0;
}

// counts of species s into Engine::spec_lin / spec_log (device); the statistics land in spec_host[0..1], the log
// counts in spec_host[2..] (pinned), after the stream has been waited for
int k_energy_spectrum(Engine *e, Species &s, const vpic_hip_spectrum_t &sp) {
  const size_t lin_words = (size_t)sp.n_lin * (size_t)e->gk.nv;
  if (ensure_spectrum(e, lin_words, (size_t)sp.n_log)) return 1;
  SpectrumK k{};
  k.n_lin = sp.n_lin; k.n_log = sp.n_log; k.d_lin = sp.d_lin; k.log_lo = sp.log_lo; k.d_log = sp.d_log;
  if (sp.n_lin > 0) {
    k.win = SPEC_WIN_WORDS / sp.n_lin;
    k.win = k.win >= SPEC_WIN_KEYS ? SPEC_WIN_KEYS : k.win >= 64 ? 64 : 0;   // (a tile's 64 keys at least, or no window)
  }
  VH_CHECK(hipMemsetAsync(e->spec_stats, 0, 2 * sizeof(unsigned long long), e->stream));
  if (lin_words) VH_CHECK(hipMemsetAsync(e->spec_lin, 0, lin_words * sizeof(unsigned), e->stream));
  if (sp.n_log) VH_CHECK(hipMemsetAsync(e->spec_log, 0, (size_t)sp.n_log * sizeof(unsigned long long), e->stream));
  if (s.np > 0) {
    const long long per_group = 64ll * SPEC_WAVES * 16;
    long long nb = (s.np + per_group - 1) / per_group;
    if (nb > 2048) nb = 2048;
    const long long waves = nb * SPEC_WAVES;
    const long long chunk = ((s.np + waves - 1) / waves + 63) / 64 * 64;
    const size_t lds = sizeof(unsigned) * ((size_t)sp.n_log + (size_t)SPEC_WAVES * k.win * sp.n_lin);
    const TileK tk = make_tile_k(e->gk);
    auto kernel = s.tile_valid ? energy_spectrum_kernel<true> : energy_spectrum_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)nb), dim3(64 * SPEC_WAVES), lds, e->stream, s.p.i, s.p.ux, s.p.uy, s.p.uz,
                       (long long)s.np, chunk, k, e->gk, tk, e->spec_lin, e->spec_log, e->spec_stats);
    VH_CHECK(hipGetLastError());
  }
  VH_CHECK(hipMemcpyAsync(e->spec_host, e->spec_stats, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, e->stream));
  if (sp.n_log) VH_CHECK(hipMemcpyAsync(e->spec_host + 2, e->spec_log, (size_t)sp.n_log * sizeof(unsigned long long), hipMemcpyDeviceToHost, e->stream));
  VH_CHECK(hipStreamSynchronize(e->stream));
  e->spec_last[0] = (int64_t)e->spec_host[0]; e->spec_last[1] = (int64_t)e->spec_host[1];
  return 0;
}

int k_energy_bands(Engine *e, int n_lin) {
  hipLaunchKernelGGL(energy_bands_kernel, dim3((e->gk.nv + 255) / 256), dim3(256), 0, e->stream, e->spec_lin, e->spec_bands, n_lin, e->gk);
  VH_CHECK(hipGetLastError());
  return 0;
}

}  // namespace vpichip
