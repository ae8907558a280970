// distribution.hip -- a 1-D or 2-D histogram of one species over position, momentum and kinetic energy, optionally of
// the particles inside a region (vpic_hip_species_distribution; include/vpic_hip.h states the arithmetic).  One
// streaming pass over those SoA arrays the descriptor names (x-ux: i, dx, ux, 12 B per particle).  Every counter is
// an integer: the result does not depend on the order of the array nor on which kernel instance pushed it.
#include "dist_coords.h"
#include <algorithm>

namespace vpichip {

constexpr int DIST_WAVES = 4;                  // wavefronts per workgroup
constexpr int DIST_WIN_WORDS = 3072;           // LDS words a wavefront's window may take (12 KB)
constexpr int DIST_WIN_SPARE_WORDS = 2048;     // ... and up to where it is given DIST_WIN_SPARE bins more than a tile touches
constexpr int DIST_WIN_SPARE = 3;
constexpr long long DIST_ITEM_PARTICLES = 32768;   // DistTiles: particles a wavefront takes on average, at the most
constexpr int DIST_BACKOFF = 16;               // passes a wavefront leaves its window where it is after a slide did not help
enum { DIST_LDS = 0, DIST_WINDOW = 1, DIST_GLOBAL = 2 };

struct DistK {
  vpic_hip_dist_t d;
  unsigned need;                               // bit c: coordinate c is used by an axis or a range
  int n0, n1;                                  // bins per axis (n1 = 1 for one axis)
  int pos_axis, win, n_other;                  // DIST_WINDOW: which axis slides, bins of it per window, bins of the other axis
};

// DIST_WINDOW on a species in tile order: which particles a wavefront takes.  All tiles with the same tile index along
// the position axis (a "column") touch the same few bins of it, so a wavefront that takes `group` tiles of ONE column
// moves its window once and flushes it once for all of them -- a flush adds every non-zero word of the window to global
// memory, and with one tile per flush (a contiguous chunk of the array) that is one global add for every two
// particles of the headline case.  Tile j holds particles [tpart[64 j], tpart[64 (j + 1)]) of the sorted part
// [0, n_sorted); what was appended since is shared out in contiguous chunks among the wavefronts behind `item_waves`.
// Only speed depends on what tpart[] means: dist_check_tiles_kernel makes sure that it is a partition (non-decreasing
// from 0, within n_sorted), and where it is not, every wavefront takes a contiguous chunk of `fallback_chunk`.
struct DistTiles {
  const int *tpart;                            // null: contiguous chunks (the kernel's `chunk` argument)
  const unsigned *bad;                         // set by dist_check_tiles_kernel
  long long n_sorted, tail_chunk, fallback_chunk;
  int axis, n_col, members, group, groups_per_col, items, item_waves;   // axis: 0 x, 1 y, 2 z; members: tiles per column
};

__global__ __launch_bounds__(256)
void dist_check_tiles_kernel(const int *__restrict__ tpart, int ntiles, long long n_sorted, unsigned *__restrict__ bad) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= ntiles) return;
  const long long b0 = tpart[(size_t)j * TILE_CELLS], b1 = j + 1 < ntiles ? (long long)tpart[(size_t)(j + 1) * TILE_CELLS] : n_sorted;
  if (b0 < 0 || b0 > b1 || b1 > n_sorted || (j == 0 && b0 != 0)) atomicOr(bad, 1u);
}

// the lanes for which `on` holds add 1 to word[a]; those that share the first such lane's word add once, together
// (a cold beam puts a whole wavefront in one word)
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

// add a wavefront's window to the global counters and clear it (the non-zero entries only)
__device__ __forceinline__ void flush_dist_window(unsigned *win, int base, const DistK &k, unsigned long long *__restrict__ counts, int lane) {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");                     // (the other lanes' adds to the window are in LDS order before these reads)
  const int n_pos = k.pos_axis == 0 ? k.n0 : k.n1;
  const int stride_pos = k.pos_axis == 0 ? 1 : k.n0, stride_other = k.pos_axis == 0 ? k.n0 : 1;   // counts[b1 * n0 + b0]
  if (k.n_other >= 64) {
    // slot by slot: no division
    const int slots = min(k.win, n_pos - base);
    for (int slot = 0; slot < slots; slot++) {
      unsigned *row = win + slot * k.n_other;
      unsigned long long *out = counts + (long long)(base + slot) * stride_pos;
      for (int other = lane; other < k.n_other; other += 64) {
        const unsigned c = row[other];
        if (c) { atomicAdd(out + (long long)other * stride_other, (unsigned long long)c); row[other] = 0; }
      }
    }
  } else {
    for (int j = lane; j < k.win * k.n_other; j += 64) {
      const unsigned c = win[j];
      if (c) {
        const int slot = j / k.n_other, other = j - slot * k.n_other;
        if (base + slot < n_pos) atomicAdd(counts + (long long)(base + slot) * stride_pos + (long long)other * stride_other, (unsigned long long)c);
        win[j] = 0;
      }
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
}

// One pass over the species; every wavefront takes a contiguous chunk of the array.
//   DIST_LDS: the workgroup's LDS holds the whole histogram (uint32), added to counts[] at the end.
//   DIST_WINDOW: every wavefront keeps k.win consecutive bins of the position axis x all bins of the other axis in LDS.
//     Per pass of 64 particles the lanes whose position bin is inside the window add there; if some are not, the window
//     is flushed and moved to where the lowest TILE among them begins (the bin of the low edge of the four cells that
//     hold the particle's cell: k.win bins from there hold everything the tile can touch, so a species in tile order
//     slides once per tile), and they try again, twice at the most (64 particles that straddle two tiles, or the end
//     of one row of voxels and the beginning of the next, still all hit); what does not fit then adds to global memory
//     and is counted as a miss.  When more than half the wavefront still misses after that, the window stays where it is
//     for the next DIST_BACKOFF passes (an array in no order).
//   DIST_GLOBAL: every counted particle adds to counts[] and is counted as a miss.
// stats: live particles seen, kept by the selection, counted, misses.
template <int PATH>
__global__ __launch_bounds__(64 * DIST_WAVES)
void species_distribution_kernel(ParticlesK p, long long np, long long chunk, DistK k, DistTiles tl, GridK g, TileK t,
                                 unsigned long long *__restrict__ counts, unsigned long long *__restrict__ stats) {
  extern __shared__ unsigned s_dist[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lds_words = PATH == DIST_LDS ? k.n0 * k.n1 : PATH == DIST_WINDOW ? DIST_WAVES * k.win * k.n_other : 0;
  unsigned *win = s_dist + (PATH == DIST_WINDOW ? wave * (k.win * k.n_other) : 0);
  if (PATH != DIST_GLOBAL) {
    for (int j = threadIdx.x; j < lds_words; j += 64 * DIST_WAVES) s_dist[j] = 0;
    __syncthreads();
  }

  // what this wavefront takes: one contiguous chunk, or (DistTiles) up to `group` tiles of one column
  const long long w = (long long)blockIdx.x * DIST_WAVES + wave;
  long long chunk_begin = w * chunk, chunk_end = chunk_begin + chunk < np ? chunk_begin + chunk : np;
  int n_seg = 1, col = 0, first_member = 0;
  bool by_tile = false;
  if (PATH == DIST_WINDOW && tl.tpart) {
    if (*tl.bad) {
      chunk_begin = w * tl.fallback_chunk; chunk_end = chunk_begin + tl.fallback_chunk < np ? chunk_begin + tl.fallback_chunk : np;
    } else if (w < tl.items) {
      by_tile = true;
      col = (int)w / tl.groups_per_col;
      first_member = ((int)w - col * tl.groups_per_col) * tl.group;
      n_seg = min(tl.group, tl.members - first_member);
    } else if (w >= tl.item_waves) {
      chunk_begin = tl.n_sorted + (w - tl.item_waves) * tl.tail_chunk;
      chunk_end = chunk_begin + tl.tail_chunk < np ? chunk_begin + tl.tail_chunk : np;
    } else {
      n_seg = 0;
    }
  }
  int base = 0, backoff = 0;
  bool placed = false;                                                       // the window has been given a place
  unsigned long long n_seen = 0, n_kept = 0, n_counted = 0, n_miss = 0;
  for (int seg = 0; seg < n_seg; seg++) {
  long long begin = chunk_begin, end = chunk_end;
  if (PATH == DIST_WINDOW && by_tile) {
    // member m of column col: the other two tile indices, x before y before z
    const int m = first_member + seg;
    int tx, ty, tz;
    if (tl.axis == 0) { tx = col; ty = m % t.nty; tz = m / t.nty; }
    else if (tl.axis == 1) { ty = col; tx = m % t.ntx; tz = m / t.ntx; }
    else { tz = col; tx = m % t.ntx; ty = m / t.ntx; }
    const int tile = (tz * t.nty + ty) * t.ntx + tx;
    begin = tl.tpart[(size_t)tile * TILE_CELLS];
    end = tile + 1 < t.ntiles ? (long long)tl.tpart[(size_t)(tile + 1) * TILE_CELLS] : tl.n_sorted;
  }
  DistRaw next = dist_load(p, begin + lane, end, k.need);
  for (long long at = begin; at < end; at += 64) {
    const DistRaw r = next;
    next = dist_load(p, at + 64 + lane, end, k.need);
    const int voxel = r.voxel;
    const bool live = voxel >= 0 && voxel < g.nv;                            // i < 0: a dead slot (engine.h, Species::n_holes)
    n_seen += __popcll(__ballot(live));
    if (!__any(live)) continue;
    DistCoords v{};
    int cell_pos = 0;                                                        // DIST_WINDOW: the particle's cell along the position axis, from 0
    if (live) {
      int cx = 0, cy = 0, cz = 0;
      v = dist_coords(r, k.need, t, cx, cy, cz);                             // (dist_coords.h)
      if (PATH == DIST_WINDOW) {
        const int c = k.pos_axis == 0 ? k.d.axis[0].coord : k.d.axis[1].coord;
        cell_pos = (c == VPIC_HIP_COORD_X ? cx : c == VPIC_HIP_COORD_Y ? cy : cz) - 1;
      }
    }
    const bool kept = live && dist_in_ranges(v, k.d.sel, k.d.n_sel);
    n_kept += __popcll(__ballot(kept));
    bool counted = kept;
    int b0 = 0, b1 = 0;
    {
      const double t0 = (dist_coord(v, k.d.axis[0].coord) - k.d.axis[0].lo) / k.d.axis[0].d;
      counted = counted && t0 >= 0.0 && t0 < (double)k.n0;
      b0 = counted ? (int)t0 : 0;
    }
    if (k.d.n_axes == 2) {
      const double t1 = (dist_coord(v, k.d.axis[1].coord) - k.d.axis[1].lo) / k.d.axis[1].d;
      counted = counted && t1 >= 0.0 && t1 < (double)k.n1;
      b1 = counted ? (int)t1 : 0;
    }
    const unsigned long long counted_mask = __ballot(counted);
    n_counted += __popcll(counted_mask);
    if (!counted_mask) continue;
    const int a_global = b1 * k.n0 + b0;                                     // (below VPIC_HIP_DIST_MAX_BINS)

    if (PATH == DIST_LDS) {
      add_together(s_dist, a_global, counted, lane);
    } else if (PATH == DIST_GLOBAL) {
      add_together(counts, a_global, counted, lane);
      n_miss += __popcll(counted_mask);
    } else {
      const int pos = k.pos_axis == 0 ? b0 : b1, other = k.pos_axis == 0 ? b1 : b0;
      bool pending = counted;
      for (int round = 0; round < 3; round++) {
        if (round > 0) {
          if (!__any(pending)) break;
          if (backoff > 0) { backoff--; break; }
          if (placed) flush_dist_window(win, base, k, counts, lane);
          int lowest = 0x7fffffff;                                           // the bin in which the lowest tile still waiting begins
          if (pending) {
            const double lo = k.pos_axis == 0 ? k.d.axis[0].lo : k.d.axis[1].lo, d = k.pos_axis == 0 ? k.d.axis[0].d : k.d.axis[1].d;
            const double tt = ((double)(cell_pos & ~(TILE_EDGE - 1)) - lo) / d;   // (a ghost cell, -1, belongs to the four cells from -4)
            lowest = tt >= 0.0 ? (int)tt : 0;                                // (below pos: the tile begins at or below the particle)
          }
#pragma unroll
          for (int m = 32; m >= 1; m >>= 1) lowest = min(lowest, __shfl_xor(lowest, m));
          base = lowest;
          placed = true;
        }
        const bool hit = placed && pending && pos >= base && pos < base + k.win;
        add_together(win, (pos - base) * k.n_other + other, hit, lane);
        if (hit) pending = false;
        if (round == 2 && __popcll(__ballot(pending)) > 32) backoff = DIST_BACKOFF;
      }
      if (pending) atomicAdd(counts + a_global, 1ull);
      n_miss += __popcll(__ballot(pending));
    }
  }
  }
  if (PATH == DIST_WINDOW && placed) flush_dist_window(win, base, k, counts, lane);
  if (lane == 0 && n_seen) {
    atomicAdd(&stats[0], n_seen);
    if (n_kept) atomicAdd(&stats[1], n_kept);
    if (n_counted) atomicAdd(&stats[2], n_counted);
    if (n_miss) atomicAdd(&stats[3], n_miss);
  }
  if (PATH == DIST_LDS) {
    __syncthreads();
    for (int j = threadIdx.x; j < lds_words; j += 64 * DIST_WAVES)
      if (s_dist[j]) atomicAdd(&counts[j], (unsigned long long)s_dist[j]);
  }
}

static int ensure_distribution(Engine *e, size_t bins) {
  if (!e->dist_stats) VH_CHECK(hipMalloc((void **)&e->dist_stats, 5 * sizeof(unsigned long long)));   // ([4]: DistTiles::bad)
  if (bins > e->dist_bins) {
    (void)hipFree(e->dist_counts); (void)hipHostFree(e->dist_host);
    e->dist_counts = nullptr; e->dist_host = nullptr; e->dist_bins = 0;
    VH_CHECK(hipMalloc((void **)&e->dist_counts, bins * sizeof(unsigned long long)));
    VH_CHECK(hipHostMalloc((void **)&e->dist_host, (4 + bins) * sizeof(unsigned long long), hipHostMallocDefault));
    e->dist_bins = bins;
  }
  return 0;
}

// which of the three paths a (checked) descriptor takes, and the window's shape (include/vpic_hip.h states the rule)
static int plan_distribution(const vpic_hip_dist_t &d, DistK &k) {
  k.d = d;
  k.n0 = d.axis[0].n; k.n1 = d.n_axes == 2 ? d.axis[1].n : 1;
  k.need = 0;
  for (int a = 0; a < d.n_axes; a++) k.need |= 1u << d.axis[a].coord;
  for (int s = 0; s < d.n_sel; s++) k.need |= 1u << d.sel[s].coord;
  k.pos_axis = 0; k.win = 0; k.n_other = 1;
  if ((long long)k.n0 * k.n1 <= VPIC_HIP_DIST_LDS_BINS) return DIST_LDS;
  int pa = -1;
  for (int a = d.n_axes - 1; a >= 0; a--) if (d.axis[a].coord <= VPIC_HIP_COORD_Z) pa = a;
  if (pa < 0) return DIST_GLOBAL;
  const int n_pos = pa == 0 ? k.n0 : k.n1, n_other = pa == 0 ? k.n1 : k.n0;
  const double tile_bins = ceil((double)TILE_EDGE / d.axis[pa].d) + 1.0;      // bins the cells of one tile can touch
  if (!(tile_bins * n_other <= (double)DIST_WIN_WORDS)) return DIST_GLOBAL;
  int win = (int)tile_bins;
  if ((win + DIST_WIN_SPARE) * n_other <= DIST_WIN_SPARE_WORDS) win += DIST_WIN_SPARE;   // fewer slides along a row of voxels, while it is cheap
  if (win > n_pos) win = n_pos;
  k.pos_axis = pa; k.win = win; k.n_other = n_other;
  return DIST_WINDOW;
}

// the histogram of species s into Engine::dist_counts (device) and, behind four words of statistics, Engine::dist_host
// (pinned), after the stream has been waited for
int k_species_distribution(Engine *e, Species &s, const vpic_hip_dist_t &d) {
  DistK k{};
  const int path = plan_distribution(d, k);
  const size_t bins = (size_t)k.n0 * (size_t)k.n1;
  if (ensure_distribution(e, bins)) return 1;
  VH_CHECK(hipMemsetAsync(e->dist_stats, 0, 5 * sizeof(unsigned long long), e->stream));
  VH_CHECK(hipMemsetAsync(e->dist_counts, 0, bins * sizeof(unsigned long long), e->stream));
  if (s.np > 0) {
    const long long per_group = 64ll * DIST_WAVES * 16;
    long long nb = (s.np + per_group - 1) / per_group;
    if (nb > 2048) nb = 2048;
    const long long waves = nb * DIST_WAVES;
    const long long chunk = ((s.np + waves - 1) / waves + 63) / 64 * 64;
    const size_t lds = sizeof(unsigned) * (path == DIST_LDS ? bins : path == DIST_WINDOW ? (size_t)DIST_WAVES * k.win * k.n_other : 0);
    const TileK tk = make_tile_k(e->gk);
    DistTiles tl{};
    if (path == DIST_WINDOW && s.tile_valid && s.tpart && s.n_sorted > 0 && s.n_sorted <= s.np &&
        s.tpart_count >= (int64_t)tk.ntiles * TILE_CELLS + 1) {
      // tiles per wavefront: 8 (a flush per 8 tiles), more on grids of more than 65 536 tiles, fewer while that leaves
      // a wavefront more than DIST_ITEM_PARTICLES on average (too few wavefronts for the chip)
      tl.axis = d.axis[k.pos_axis].coord;
      tl.n_col = tl.axis == 0 ? tk.ntx : tl.axis == 1 ? tk.nty : tk.ntz;
      tl.members = tk.ntiles / tl.n_col;
      tl.group = std::min(tl.members, std::max(8, (tk.ntiles + 8191) / 8192));
      while (tl.group > 1 && (long long)tl.n_col * ((tl.members + tl.group - 1) / tl.group) * DIST_ITEM_PARTICLES < s.n_sorted)
        tl.group = (tl.group + 1) / 2;
      tl.groups_per_col = (tl.members + tl.group - 1) / tl.group;
      tl.items = tl.n_col * tl.groups_per_col;
    }
    if (tl.items > 0 && (tl.items >= 4096 || (long long)tl.items * DIST_ITEM_PARTICLES >= s.n_sorted)) {   // (else: contiguous chunks)
      tl.tpart = s.tpart; tl.bad = (const unsigned *)(e->dist_stats + 4); tl.n_sorted = s.n_sorted;
      const long long item_groups = (tl.items + DIST_WAVES - 1) / DIST_WAVES;
      tl.item_waves = (int)(item_groups * DIST_WAVES);
      const long long tail = s.np - s.n_sorted;
      const long long tail_groups = tail > 0 ? std::min(2048ll, (tail + per_group - 1) / per_group) : 0;
      if (tail_groups) tl.tail_chunk = ((tail + tail_groups * DIST_WAVES - 1) / (tail_groups * DIST_WAVES) + 63) / 64 * 64;
      nb = item_groups + tail_groups;
      tl.fallback_chunk = ((s.np + nb * DIST_WAVES - 1) / (nb * DIST_WAVES) + 63) / 64 * 64;
      hipLaunchKernelGGL(dist_check_tiles_kernel, dim3((tk.ntiles + 255) / 256), dim3(256), 0, e->stream, s.tpart, tk.ntiles,
                         (long long)s.n_sorted, (unsigned *)(e->dist_stats + 4));
      VH_CHECK(hipGetLastError());
    }
    auto kernel = path == DIST_LDS ? species_distribution_kernel<DIST_LDS>
                : path == DIST_WINDOW ? species_distribution_kernel<DIST_WINDOW> : species_distribution_kernel<DIST_GLOBAL>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)nb), dim3(64 * DIST_WAVES), lds, e->stream, s.p, (long long)s.np, chunk, k, tl, e->gk, tk,
                       e->dist_counts, e->dist_stats);
    VH_CHECK(hipGetLastError());
  }
  VH_CHECK(hipMemcpyAsync(e->dist_host, e->dist_stats, 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost, e->stream));
  VH_CHECK(hipMemcpyAsync(e->dist_host + 4, e->dist_counts, bins * sizeof(unsigned long long), hipMemcpyDeviceToHost, e->stream));
  VH_CHECK(hipStreamSynchronize(e->stream));
  for (int j = 0; j < 4; j++) e->dist_last[j] = (int64_t)e->dist_host[j];
  return 0;
}

}  // namespace vpichip
