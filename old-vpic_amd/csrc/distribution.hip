// distribution.hip -- a 1-D or 2-D histogram of one species over position, momentum, kinetic energy and the coordinates
// in the frame of the local magnetic field (u_par, u_perp, pitch, mu, |cB|, E_par), optionally of the particles inside a region (vpic_hip_species_distribution; include/vpic_hip.h states the arithmetic).  One
// streaming pass over those SoA arrays the descriptor names (x-ux: i, dx, ux, 12 B per particle).  Every counter is
// an integer: the result does not depend on the order of the array nor on which kernel instance pushed it.
// Which path a descriptor takes, the window's shape and how tiles are dealt to wavefronts are host decisions in policy.h
// (plan_distribution, plan_dist_tiles, plan_chunks); the window protocol, add_together, the check of the tile partition
// and the statistics block are the ones every pass over a species uses (engine.h).
// Behind the histograms: the per-bin sums of particle quantities (vpic_hip_species_distribution_sums), kernel instances of their
// own over the same loads and coordinates; 64-bit integer sums, in LDS while they fit (policy.h, plan_distribution_sums).
// The counted test, the values of the sums, their LDS block and the statistics are hist_device.h's, which the cells'
// histograms (cell_dist.hip) use too; both calls answer through Engine::species_hist (engine.h, HistResult), the counts-only
// call through its counts and Engine::dist_stats.
#include "dist_coords.h"
#include "hist_device.h"
#include <algorithm>

namespace vpichip {

constexpr int DIST_WAVES = 4;                  // wavefronts per workgroup

struct DistK {
  vpic_hip_dist_t d;
  unsigned need;                               // bit c: coordinate c is used by an axis or a range
  int n0, n1;                                  // bins per axis (n1 = 1 for one axis)
  int pos_axis, win, n_other;                  // DIST_WINDOW (policy.h, plan_distribution): which axis slides, bins of it per window, bins of the other axis
};

// DIST_WINDOW on a species in tile order: which particles a wavefront takes (policy.h, plan_dist_tiles).  Tile j holds
// particles [tpart[64 j], tpart[64 (j + 1)]) of the sorted part [0, n_sorted).  Only speed depends on what tpart[] means:
// k_check_tile_partition makes sure that it is a partition, and where it is not, every wavefront takes a contiguous
// chunk of `fallback_chunk`.
struct DistTiles {
  const int *tpart;                            // null: contiguous chunks (the kernel's `chunk` argument)
  const unsigned *bad;                         // set by k_check_tile_partition
  long long n_sorted, tail_chunk, fallback_chunk;
  int axis, n_col, members, group, groups_per_col, items, item_waves;   // axis: 0 x, 1 y, 2 z; members: tiles per column
};

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
//     and is counted as a miss (the protocol: engine.h, window_add).
//   DIST_GLOBAL: every counted particle adds to counts[] and is counted as a miss.
// stats: live particles seen, kept by the selection, counted, misses.
// FIELDS: the descriptor names a coordinate in the frame of the local field (dist_coords.h); every path, the walk by
//   tile and the statistics are the same.  The particle loads then run TWO passes ahead and the gather of the
//   interpolator record one: pass n + 1's gather is issued at the top of pass n, when its voxels (asked for a pass ago)
//   have arrived, so that it is in flight during pass n's arithmetic as the particle loads are.  fi is not read otherwise.
template <int PATH, bool FIELDS>
__global__ __launch_bounds__(64 * DIST_WAVES)
void species_distribution_kernel(ParticlesK p, long long np, long long chunk, DistK k, DistTiles tl, GridK g, TileK t,
                                 unsigned long long *__restrict__ counts, unsigned long long *__restrict__ stats,
                                 const vpic_interpolator_t *__restrict__ fi) {
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
  SlideWindow w_state;
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
  DistRaw next = dist_load<FIELDS>(p, begin + lane, end, k.need), next2{};
  DistField f{}, f_next{};
  if (FIELDS) {
    next2 = dist_load<FIELDS>(p, begin + 64 + lane, end, k.need);
    f_next = dist_gather(fi, next.voxel, g.nv, k.need);
  }
  for (long long at = begin; at < end; at += 64) {
    const DistRaw r = next;
    if (FIELDS) {
      f = f_next;
      next = next2;
      f_next = dist_gather(fi, next.voxel, g.nv, k.need);
      next2 = dist_load<FIELDS>(p, at + 128 + lane, end, k.need);
    } else {
      next = dist_load<FIELDS>(p, at + 64 + lane, end, k.need);
    }
    const int voxel = r.voxel;
    const bool live = voxel >= 0 && voxel < g.nv;                            // i < 0: a dead slot (engine.h, Species::n_holes)
    n_seen += __popcll(__ballot(live));
    if (!__any(live)) continue;
    DistCoords v{};
    int cell_pos = 0;                                                        // DIST_WINDOW: the particle's cell along the position axis, from 0
    if (live) {
      int cx = 0, cy = 0, cz = 0;
      v = dist_coords<FIELDS>(r, f, k.need, t, cx, cy, cz);                            // (dist_coords.h)
      if (PATH == DIST_WINDOW) {
        const int c = k.pos_axis == 0 ? k.d.axis[0].coord : k.d.axis[1].coord;
        cell_pos = (c == VPIC_HIP_COORD_X ? cx : c == VPIC_HIP_COORD_Y ? cy : cz) - 1;
      }
    }
    const bool kept = live && dist_in_ranges<FIELDS>(v, k.d.sel, k.d.n_sel);
    n_kept += __popcll(__ballot(kept));
    const HistBin h = hist_bin(kept, k.d, k.n0, k.n1, [&](int coord) { return dist_coord<FIELDS>(v, coord); });
    const bool counted = h.counted;
    const unsigned long long counted_mask = __ballot(counted);
    n_counted += __popcll(counted_mask);
    if (!counted_mask) continue;
    const int a_global = h.a;                                                // (below VPIC_HIP_DIST_MAX_BINS)

    if (PATH == DIST_LDS) {
      add_together(s_dist, a_global, counted, lane);
    } else if (PATH == DIST_GLOBAL) {
      add_together(counts, a_global, counted, lane);
      n_miss += __popcll(counted_mask);
    } else {
      const int pos = k.pos_axis == 0 ? h.b0 : h.b1, other = k.pos_axis == 0 ? h.b1 : h.b0;
      // the window goes to the bin in which the lowest tile still waiting begins
      const bool pending = window_add(w_state, win, k.win, k.n_other, pos, other, counted, lane,
        [&](unsigned long long left) {
          int lowest = 0x7fffffff;
          if (left >> lane & 1ull) {
            const double lo = k.pos_axis == 0 ? k.d.axis[0].lo : k.d.axis[1].lo, d = k.pos_axis == 0 ? k.d.axis[0].d : k.d.axis[1].d;
            const double tt = ((double)(cell_pos & ~(TILE_EDGE - 1)) - lo) / d;   // (a ghost cell, -1, belongs to the four cells from -4)
            lowest = tt >= 0.0 ? (int)tt : 0;                                // (below pos: the tile begins at or below the particle)
          }
#pragma unroll
          for (int m = 32; m >= 1; m >>= 1) lowest = min(lowest, __shfl_xor(lowest, m));
          return lowest;
        },
        [&](int base) { flush_dist_window(win, base, k, counts, lane); });
      if (pending) atomicAdd(counts + a_global, 1ull);
      n_miss += __popcll(__ballot(pending));
    }
  }
  }
  if (PATH == DIST_WINDOW && w_state.placed) flush_dist_window(win, w_state.base, k, counts, lane);
  hist_publish(stats, lane, n_seen, n_kept, n_counted, n_miss);
  if (PATH == DIST_LDS) {
    __syncthreads();
    for (int j = threadIdx.x; j < lds_words; j += 64 * DIST_WAVES)
      if (s_dist[j]) atomicAdd(&counts[j], (unsigned long long)s_dist[j]);
  }
}

// the histogram of species s into the counts of Engine::species_hist (which the sums' call fills too), its four statistics
// into Engine::dist_stats, after the stream has been waited for
int k_species_distribution(Engine *e, Species &s, const vpic_hip_dist_t &d) {
  DistK k{};
  k.d = d;
  k.n0 = d.axis[0].n; k.n1 = d.n_axes == 2 ? d.axis[1].n : 1;
  for (int a = 0; a < d.n_axes; a++) k.need |= 1u << d.axis[a].coord;
  for (int r = 0; r < d.n_sel; r++) k.need |= 1u << d.sel[r].coord;
  const int n[2] = {k.n0, k.n1};
  const double width[2] = {d.axis[0].d, d.axis[1].d};
  const bool position[2] = {d.axis[0].coord <= VPIC_HIP_COORD_Z, d.n_axes == 2 && d.axis[1].coord <= VPIC_HIP_COORD_Z};
  const DistPlan pl = plan_distribution(d.n_axes, n, width, position, VPIC_HIP_DIST_LDS_BINS);
  k.pos_axis = pl.pos_axis; k.win = pl.win; k.n_other = pl.n_other;
  const int path = pl.path;
  const size_t bins = (size_t)k.n0 * (size_t)k.n1;
  HistResult &h = e->species_hist;
  if (h.grow_counts(bins) || e->dist_stats.begin(e->stream)) return 1;
  VH_CHECK(hipMemsetAsync(h.counts, 0, bins * sizeof(unsigned long long), e->stream));
  if (s.np > 0) {
    const Chunks ch = plan_chunks(s.np, DIST_WAVES);
    long long nb = ch.groups;
    const size_t lds = sizeof(unsigned) * (path == DIST_LDS ? bins : path == DIST_WINDOW ? (size_t)DIST_WAVES * k.win * k.n_other : 0);
    const TileK tk = make_tile_k(e->gk);
    DistTiles tl{};
    if (path == DIST_WINDOW) {
      const int axis = d.axis[k.pos_axis].coord;
      const DistTilePlan tp = plan_dist_tiles(tk.ntx, tk.nty, tk.ntz, axis, tile_partition_usable(s, tk), s.n_sorted, s.np, DIST_WAVES);
      if (tp.n_col) tl.axis = axis;
      tl.n_col = tp.n_col; tl.members = tp.members; tl.group = tp.group; tl.groups_per_col = tp.groups_per_col; tl.items = tp.items;
      if (tp.by_tile) {
        tl.tpart = s.tpart; tl.bad = e->dist_stats.bad_partition(); tl.n_sorted = s.n_sorted;
        tl.item_waves = tp.item_waves; tl.tail_chunk = tp.tail_chunk; tl.fallback_chunk = tp.fallback_chunk;
        nb = tp.groups;
        if (k_check_tile_partition(e, s, e->dist_stats.bad_partition())) return 1;
      }
    }
    // a descriptor that names no field coordinate runs the instances it always ran
    auto kernel = k.need & NEED_FIELD
      ? (path == DIST_LDS ? species_distribution_kernel<DIST_LDS, true>
         : path == DIST_WINDOW ? species_distribution_kernel<DIST_WINDOW, true> : species_distribution_kernel<DIST_GLOBAL, true>)
      : (path == DIST_LDS ? species_distribution_kernel<DIST_LDS, false>
         : path == DIST_WINDOW ? species_distribution_kernel<DIST_WINDOW, false> : species_distribution_kernel<DIST_GLOBAL, false>);
    hipLaunchKernelGGL(kernel, dim3((unsigned)nb), dim3(64 * DIST_WAVES), lds, e->stream, s.p, (long long)s.np, ch.chunk, k, tl, e->gk, tk,
                       h.counts, e->dist_stats.dev, (const vpic_interpolator_t *)e->fi);
    VH_CHECK(hipGetLastError());
  }
  VH_CHECK(hipMemcpyAsync(h.counts_host, h.counts, bins * sizeof(unsigned long long), hipMemcpyDeviceToHost, e->stream));
  return e->dist_stats.read(e->stream);
}

// ---- per-bin sums of particle quantities (vpic_hip_species_distribution_sums; include/vpic_hip.h states the arithmetic) ----
struct DistSumsK : HistK {
  unsigned need, vneed;                        // need: as DistK::need, the factors' coordinates included; vneed: VAL_* (dist_coords.h)
};

// One pass over the species, every wavefront a contiguous chunk, as species_distribution_kernel walks it (the same loads
// ahead, the same coordinates, the same counted test), plus q when a value names it.
//   DIST_LDS: the workgroup's LDS holds n_val rows of 64-bit sums, then the 32-bit counts; added to global memory at the end.
//   DIST_GLOBAL: every counted particle adds to counts[] and sums[] and is counted as a miss.
// Integer adds: any order and any grouping of them gives the same words.
// stats: live particles seen, kept by the selection, counted, misses, then the particles refused for each value.
template <int PATH, bool FIELDS>
__global__ __launch_bounds__(64 * DIST_WAVES)
void species_distribution_sums_kernel(ParticlesK p, long long np, long long chunk, DistSumsK k, GridK g, TileK t,
                                      unsigned long long *__restrict__ counts, unsigned long long *__restrict__ sums,
                                      unsigned long long *__restrict__ stats, const vpic_interpolator_t *__restrict__ fi) {
  extern __shared__ unsigned long long s_sums[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int bins = k.n0 * k.n1;
  unsigned *s_counts = reinterpret_cast<unsigned *>(s_sums + k.n_val * bins);
  if (PATH == DIST_LDS) hist_lds_clear<64 * DIST_WAVES>(s_sums, s_counts, k.n_val, bins);
  const long long w = (long long)blockIdx.x * DIST_WAVES + wave;
  const long long begin = w * chunk, end = begin + chunk < np ? begin + chunk : np;
  unsigned long long n_seen = 0, n_kept = 0, n_counted = 0, n_refused[VPIC_HIP_DIST_MAX_VALUES] = {0, 0, 0, 0};
  DistRaw next = dist_load<FIELDS>(p, begin + lane, end, k.need), next2{};
  float q_next = dist_load_q(p, begin + lane, end, k.vneed), q_next2 = 0.f;
  DistField f{}, f_next{};
  if (FIELDS) {
    next2 = dist_load<FIELDS>(p, begin + 64 + lane, end, k.need);
    q_next2 = dist_load_q(p, begin + 64 + lane, end, k.vneed);
    f_next = dist_gather(fi, next.voxel, g.nv, k.need);
  }
  for (long long at = begin; at < end; at += 64) {
    const DistRaw r = next;
    const float q = q_next;
    if (FIELDS) {
      f = f_next;
      next = next2; q_next = q_next2;
      f_next = dist_gather(fi, next.voxel, g.nv, k.need);
      next2 = dist_load<FIELDS>(p, at + 128 + lane, end, k.need);
      q_next2 = dist_load_q(p, at + 128 + lane, end, k.vneed);
    } else {
      next = dist_load<FIELDS>(p, at + 64 + lane, end, k.need);
      q_next = dist_load_q(p, at + 64 + lane, end, k.vneed);
    }
    const bool live = r.voxel >= 0 && r.voxel < g.nv;
    n_seen += __popcll(__ballot(live));
    if (!__any(live)) continue;
    DistCoords v{};
    if (live) {
      int cx = 0, cy = 0, cz = 0;
      v = dist_coords<FIELDS>(r, f, k.need, t, cx, cy, cz);
    }
    const bool kept = live && dist_in_ranges<FIELDS>(v, k.d.sel, k.d.n_sel);
    n_kept += __popcll(__ballot(kept));
    const HistBin h = hist_bin(kept, k.d, k.n0, k.n1, [&](int coord) { return dist_coord<FIELDS>(v, coord); });
    const unsigned long long counted_mask = __ballot(h.counted);
    n_counted += __popcll(counted_mask);
    if (!counted_mask) continue;
    if (PATH == DIST_LDS) add_together(s_counts, h.a, h.counted, lane);
    else add_together(counts, h.a, h.counted, lane);
    const DistExtra x = dist_extra<FIELDS>(r, f, q, v, k.vneed);
    hist_add_values(k, bins, h, counted_mask, [&](int code) { return dist_factor<FIELDS>(v, x, code); },
                    PATH == DIST_LDS ? s_sums : sums, n_refused, lane);
  }
  hist_publish(stats, lane, n_seen, n_kept, n_counted, PATH == DIST_GLOBAL ? n_counted : 0, n_refused);
  if (PATH == DIST_LDS) hist_lds_flush<64 * DIST_WAVES>(s_sums, s_counts, k.n_val, bins, counts, sums);
}

// the histogram, the sums and the eight statistics of species s into Engine::species_hist, after the stream has been waited for
int k_species_distribution_sums(Engine *e, Species &s, const vpic_hip_dist_t &d, const vpic_hip_dist_value_t *v, int n_val) {
  DistSumsK k{};
  fill_hist_k(k, d, v, n_val);
  for (int a = 0; a < d.n_axes; a++) k.need |= 1u << d.axis[a].coord;
  for (int r = 0; r < d.n_sel; r++) k.need |= 1u << d.sel[r].coord;
  for (int j = 0; j < n_val; j++)
    for (int c = 0; c < 3; c++) dist_factor_need(v[j].factor[c], k.need, k.vneed);
  const size_t bins = (size_t)k.n0 * (size_t)k.n1, words = bins * (size_t)n_val;
  const DistSumsPlan pl = plan_distribution_sums((long long)bins, n_val, VPIC_HIP_DIST_LDS_BINS);
  HistResult &h = e->species_hist;
  if (h.begin(bins, words, e->stream)) return 1;
  if (s.np > 0) {
    const Chunks ch = plan_chunks(s.np, DIST_WAVES);
    const size_t lds = sizeof(unsigned) * (size_t)pl.words;
    const bool fields = (k.need & NEED_FIELD) != 0;
    auto kernel = fields ? (pl.path == DIST_LDS ? species_distribution_sums_kernel<DIST_LDS, true> : species_distribution_sums_kernel<DIST_GLOBAL, true>)
                         : (pl.path == DIST_LDS ? species_distribution_sums_kernel<DIST_LDS, false> : species_distribution_sums_kernel<DIST_GLOBAL, false>);
    hipLaunchKernelGGL(kernel, dim3((unsigned)ch.groups), dim3(64 * DIST_WAVES), lds, e->stream, s.p, (long long)s.np, ch.chunk, k, e->gk,
                       make_tile_k(e->gk), h.counts, h.sums, h.stats.dev, (const vpic_interpolator_t *)e->fi);
    VH_CHECK(hipGetLastError());
  }
  return h.read(bins, words, e->stream);
}

}  // namespace vpichip
