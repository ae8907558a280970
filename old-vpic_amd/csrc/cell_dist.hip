// cell_dist.hip -- a 1-D or 2-D histogram over the interior CELLS of the grid with up to four exact per-bin sums beside it
// (vpic_hip_cell_distribution; include/vpic_hip.h states the arithmetic): the descriptor of the per-bin sums of a species
// (distribution.hip) and, by the same code (hist_device.h), their counted test, quantised 64-bit sums, refusals, LDS block
// and statistics, over coordinates of a cell -- its centre, the raw words of its field and hydro records, the fields at its
// centre by load_interpolator's expressions and what derives from them (cell_coords.h).  One lane per interior cell,
// grid-stride, x fastest: consecutive lanes read consecutive floats of every component array the descriptor names and of
// no other.  Every counter is an integer: the result does not depend on how the cells are dealt out nor on the path.
// Which path a descriptor takes is the host decision of the species' sums (policy.h, plan_distribution_sums); how many
// workgroups, plan_cell_groups.  The call answers through Engine::cell_hist (engine.h, HistResult).
#include "cell_coords.h"
#include "hist_device.h"

namespace vpichip {

constexpr int CELL_WAVES = 4;                  // wavefronts per workgroup

struct CellDistK : HistK {
  unsigned long long need;                     // cell_coords.h: the codes of the axes, the ranges and the factors, and what they are formed from
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
  if (PATH == DIST_LDS) hist_lds_clear<64 * CELL_WAVES>(s_cell_sums, s_counts, k.n_val, bins);
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
    const HistBin h = hist_bin(kept, k.d, k.n0, k.n1, [&](int code) { return cell_coord(v, code); });
    const unsigned long long counted_mask = __ballot(h.counted);
    n_counted += __popcll(counted_mask);
    if (!counted_mask) continue;
    if (PATH == DIST_LDS) add_together(s_counts, h.a, h.counted, lane);
    else add_together(counts, h.a, h.counted, lane);
    hist_add_values(k, bins, h, counted_mask, [&](int code) { return cell_coord(v, code); }, PATH == DIST_LDS ? s_cell_sums : sums, n_refused, lane);
  }
  hist_publish(stats, lane, n_seen, n_kept, n_counted, PATH == DIST_GLOBAL ? n_counted : 0, n_refused);
  if (PATH == DIST_LDS) hist_lds_flush<64 * CELL_WAVES>(s_cell_sums, s_counts, k.n_val, bins, counts, sums);
}

// the histogram, the sums and the eight statistics of a checked descriptor into Engine::cell_hist, after the stream has been
// waited for
int k_cell_distribution(Engine *e, const vpic_hip_dist_t &d, const vpic_hip_dist_value_t *v, int n_val) {
  CellDistK k{};
  fill_hist_k(k, d, v, n_val);
  for (int a = 0; a < d.n_axes; a++) k.need |= cell_code_need(d.axis[a].coord);
  for (int r = 0; r < d.n_sel; r++) k.need |= cell_code_need(d.sel[r].coord);
  for (int j = 0; j < n_val; j++)
    for (int c = 0; c < 3; c++) k.need |= cell_code_need(v[j].factor[c]);
  if ((k.need & CELL_NEED_HYDRO) && !e->hydro) VH_FAIL("cell distribution: a hydro code, and the hydro array was never allocated");
  const size_t bins = (size_t)k.n0 * (size_t)k.n1, words = bins * (size_t)n_val;
  const DistSumsPlan pl = plan_distribution_sums((long long)bins, n_val, VPIC_HIP_DIST_LDS_BINS);
  HistResult &h = e->cell_hist;
  if (h.grow_sums(words + 1) || h.begin(bins, words, e->stream)) return 1;   // (+ 1: never an empty buffer)
  const CellGridK c = make_cell_grid_k(e->gk);
  const long long groups = plan_cell_groups(c.cells, 64 * CELL_WAVES);
  const size_t lds = sizeof(unsigned) * (size_t)pl.words;
  auto kernel = pl.path == DIST_LDS ? cell_distribution_kernel<DIST_LDS> : cell_distribution_kernel<DIST_GLOBAL>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)groups), dim3(64 * CELL_WAVES), lds, e->stream, e->f, (const float *)e->hydro, c, k,
                     h.counts, h.sums, h.stats.dev);
  VH_CHECK(hipGetLastError());
  return h.read(bins, words, e->stream);
}

}  // namespace vpichip
