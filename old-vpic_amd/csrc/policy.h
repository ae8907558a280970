// policy.h -- the engine's host decisions over plain values: the sort and the push (vpic_hip_step, sort_p, advance_p), whose
// callers read their HIP events and pinned words once and hand in what they read, the moments, the collisions (collide.hip),
// and the launch shapes of the passes over one species (spectrum.hip, distribution.hip).  Plain C++17, no HIP: tests/policy_check.cpp builds it with the
// host compiler alone.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <math.h>
#include <algorithm>

namespace vpichip {

constexpr int TILE_EDGE = 4;   // cells per edge of a tile (TILE order, engine.h)

// the words a species' kernels publish behind their launches into mapped pinned memory (Species::crossed_host): crossers of
// the last push, particles of the fullest tile at the last tile sort, cursors of the last sort that did not end where the next
// key begins (Species::fuse_pending), runs that missed the tile windows in the last push, the sort cycle that push belonged to
enum PinnedWord { PW_CROSSERS = 0, PW_FULLEST_TILE, PW_SORT_CHECK, PW_MISSED, PW_CYCLE };

// What the decisions about one species remember (Species::pol).
struct Policy {
  // adaptive sorting (vpic_hip_step, sort_interval < 0; see sort_due): cost of a sort, and sum / number of the push times
  // since the last sort (ms)
  bool sorted_once = false;
  double t_sort = 0, t_sum = 0; int n_push = 0;
  double t_last = 0, growth_first = 0; int n_cycle = 0;   // n_cycle: sorts so far
  // (one set per sort flavour, see flavour_cost: [0] by cell within a tile or by voxel, [1] by tile only)
  double t_hist[2][32] = {{0}}; int n_hist[2] = {0, 0};                // ... the push times of earlier cycles by position in the cycle
  double s_hist[2][33] = {{0}}; int sorted_after = 0;          // ... what a sort cost after n pushes (more steps, more disorder), pushes before the last sort
  double c_hist[2][34] = {{0}}; double prev_sum = 0;           // ... measured cost per step (sort included) of whole cycles of n pushes; push time of the last whole cycle
  bool coarse_order = false;      // tile sorts group this species by tile only (particles.hip)
  // ... chosen by measurement when the engine's sort policy times the cycles: cost per step of whole cycles in either
  // flavour ([0] by cell within a tile, [1] by tile only; 0 = not on record), cycles since the flavour last changed
  double flavour_cost[2] = {0, 0}; int flavour_cycles = 0;
  // ... inside the push or before it: decided by MEASUREMENT (engine.hip: sort_and_push).  A species whose cells move as one (cold
  // beams) lands in its new order in long runs and the sorting launch beats sort + push (29.7 ms against 20 + 16.8 at 256^3 x
  // 64 ppc); one whose particles have spread (the same deck from step ~120 on) writes runs of two and loses (60 against 20 +
  // 18.5).  ms of this species' sort + push in either way (0: not on record), the choice made last
  float sort_push_ms[2] = {0, 0}; bool sp_last = true;
  // ... and of the push that counted for the sort (the last, slowest plain launch of the cycle): the yardstick that says whether
  // sorting before the push is worth a first try -- 20 + 17 ms against 27-30 inside the push where the counting launch took
  // 17.6 (ratio 1.6: no), 20 + 18.5 against 60 where it took 24 (2.5: yes)
  float hint_push_ms = 0;
  bool wide_window = false;       // advance_p instance with the double-precision LDS window (crossing-heavy species; push.hip)
  bool tile_unbalanced = false;   // the fullest tile alone would keep its workgroup busy several times longer than a balanced launch takes
  double cross_frac = 0;          // fraction of the particles that left their cell in the last advance_p (one launch behind)
  int64_t np_pushed_last = 0;     // particles of the previous advance_p launch (denominator of the crossing fraction)
  int64_t early_sorts = 0;        // sorts vpic_hip_step made ahead of a fixed interval because the deposits had begun to miss the windows

  // a sort has finished (k_sort_finish): a new cycle begins
  void new_cycle(bool tile_order) {
    if (tile_order) tile_unbalanced = false;          // the push looks at the fullest tile of THIS sort
    sorted_once = true; sorted_after = n_push; prev_sum = t_sum; t_sum = 0; n_push = 0; n_cycle++;
    if (tile_order) flavour_cycles++;
  }
};

// The adaptive decision for one species (vpic_hip_step, vpic_hip_sort_due): books the times of the last sort and push
// (sort_ms, push_ms: < 0 when not timed since) and says whether to sort before the next push.
inline bool sort_due(Policy &s, double sort_ms, double push_ms, bool coarse_sorted, bool tile_valid, int max_interval, bool debug) {
  bool due = false;
  if (const double ms = sort_ms; ms >= 0) {
    s.t_sort = ms;
    const int fl = coarse_sorted ? 1 : 0;                  // (a sort right after a change of flavour is booked to the new one: one stray sample)
    if (s.sorted_after >= 1 && s.sorted_after <= 32) { s.s_hist[fl][s.sorted_after] = ms; s.c_hist[fl][s.sorted_after] = (ms + s.prev_sum) / s.sorted_after; }
    // cost per step of the cycle this sort closed, booked to the flavour it ran in (cycles right after a change of
    // flavour still carry the other one's disorder and are not counted)
    if (s.sorted_after >= 1 && tile_valid && s.flavour_cycles >= 2) {
      const int f = coarse_sorted ? 1 : 0;
      const double c = (ms + s.prev_sum) / s.sorted_after;
      s.flavour_cost[f] = s.flavour_cost[f] > 0 ? 0.5 * (s.flavour_cost[f] + c) : c;
    }
  }
  if (const double ms = push_ms; ms >= 0) {
    // predicted cost of the NEXT push: the last one plus the growth to expect.  Push times grow faster than linearly
    // once particles outrun the LDS window (a ballistic plasma leaves a tile's halo after a few steps and every deposit
    // outside costs twelve global atomics), so the growth is the one an EARLIER cycle saw at this position when one got
    // that far; otherwise the growth seen last (within this cycle, or -- after one push -- the first growth of the
    // latest cycle that had two).  Every 64th cycle forgets the recorded growths, so that one that has died down gets
    // measured again.
    const int at = s.n_push;                            // position of the push just timed within its cycle
    const int fl = coarse_sorted ? 1 : 0;
    double *t_hist = s.t_hist[fl], *s_hist = s.s_hist[fl], *c_hist = s.c_hist[fl]; int &n_hist = s.n_hist[fl];
    double growth = 0;
    if (at >= 1) { growth = ms - s.t_last; if (at == 1) s.growth_first = growth; }
    else if ((s.n_cycle & 63) != 63) growth = s.growth_first;
    if ((s.n_cycle & 63) == 63) n_hist = 0;
    if (at + 1 < n_hist && at + 1 < 32) growth = std::max(growth, t_hist[at + 1] - t_hist[at]);
    if (at < 32) { t_hist[at] = ms; if (n_hist < at + 1) n_hist = at + 1; }
    s.t_last = ms;
    s.t_sum += ms; s.n_push++;
    // Sort now, after n pushes, or after one more?  Whichever has the lower cost per step, the sort included.  The sort
    // is dearer the longer it is put off (the disorder it undoes grows: 2.4 ms after one step of a vth = 0.6 c species,
    // 4.5 after three), so its cost is the one seen at that cycle length when there is one on record.
    const int n = s.n_push;
    const double t_next = ms + (growth > 0 ? growth : 0);
    const double sort_now = (n <= 32 && s_hist[n] > 0) ? s_hist[n] : s.t_sort;
    double sort_later = (n + 1 <= 32 && s_hist[n + 1] > 0) ? s_hist[n + 1] : sort_now;
    if (sort_later < sort_now) sort_later = sort_now;
    if ((s.n_cycle & 63) == 63) sort_later = sort_now;
    due = (sort_later + s.t_sum + t_next) * n >= (sort_now + s.t_sum) * (n + 1);
    // What whole cycles of n and of n + 1 pushes actually cost per step, when both are on record, overrules the
    // prediction; and every eighth cycle is ended one push earlier than the last one when no cycle of that length is on record yet (the
    // prediction cannot know what a sort costs after fewer steps than it has ever been put off).
    if ((s.n_cycle & 63) == 63) for (int k = 0; k < 34; k++) c_hist[k] = 0;
    if (n <= 32 && c_hist[n] > 0 && c_hist[n + 1] > 0) due = c_hist[n] <= c_hist[n + 1];
    else if (!due && n <= 32 && c_hist[n] == 0 && (s.n_cycle & 7) == 7 && n == s.sorted_after - 1) due = true;   // one push earlier than last time
    if (debug) fprintf(stderr, "sort policy: n=%d T=%.3f T_next=%.3f S_now=%.3f S_later=%.3f sum=%.3f c[n]=%.3f c[n+1]=%.3f flavour %d (%.3f / %.3f per step) -> %s\n", n, ms, t_next, sort_now, sort_later, s.t_sum, n <= 32 ? c_hist[n] : 0.0, n <= 32 ? c_hist[n + 1] : 0.0, (int)coarse_sorted, s.flavour_cost[0], s.flavour_cost[1], due ? "sort" : "go on");
  }
  if (!s.sorted_once || (max_interval > 0 && s.n_push >= max_interval)) due = true;
  return due;
}

// Which order a sort asked for through the ABI produces: TILE (true) or the reference's by voxel.  engine_choice: the caller
// has left the choice to the engine (vpic_hip_set_sort_order(e, 1), or the engine's own sort policy consulted); window: the
// VPIC_HIP_WINDOW knob; min_axis: the fewest cells of the grid along an axis.
inline bool wants_tile_order(const Policy &s, int64_t np, int window, int min_axis, bool engine_choice) {
  if (np > ((int64_t)1 << 30)) return false;   // one launch: 32-bit byte offsets into the arrays
  // (a chargeless species -- tracer copies -- is pushed without a window in any order; grouped by tile its interpolator
  // gathers stay local, and the sort by tile only costs a quarter of the sort by voxel on a hot species: k_sort_p)
  if (window == 't') return true;
  if (window == 'w' || window == 'n') return false;
  // a grid thinner than a tile on some axis (2-D decks: ny = 1) would give every workgroup a quarter tile or less of work;
  // the row windows of the reference's order serve those
  if (min_axis < TILE_EDGE) return false;
  // see plan_push: one tile held far more than its share at the last tile sort; every 32nd sort looks again
  if (s.tile_unbalanced && (s.n_cycle & 31) != 31) return false;
  return engine_choice;
}

// A species that is due, sorted and pushed: the sort INSIDE the push (true) or before it, whichever took less time for this
// species when it was last tried (sort_push_ms, read by the caller); the loser is tried again every eighth sort.
inline bool sort_inside_push(Policy &s, bool debug) {
  if (s.sort_push_ms[1] == 0) s.sp_last = true;        // [1] inside the push, [0] before it
  else if (s.sort_push_ms[0] == 0)
    // before the push for the first time: when the launch that sorted took more than 1.9 x the one that counted for it (see
    // Policy::hint_push_ms; a short run of a cold deck never pays for the experiment), or at the sixteenth sort at the latest
    s.sp_last = !((s.hint_push_ms > 0 && s.sort_push_ms[1] > 1.9f * s.hint_push_ms) || (s.n_cycle & 15) == 15);
  else { s.sp_last = s.sort_push_ms[1] <= s.sort_push_ms[0]; if ((s.n_cycle & 7) == 7) s.sp_last = !s.sp_last; }
  if (debug) fprintf(stderr, "sort and push: inside %.2f ms, before %.2f ms, the push that counted %.2f ms -> %s\n", (double)s.sort_push_ms[1], (double)s.sort_push_ms[0], (double)s.hint_push_ms, s.sp_last ? "inside" : "before");
  return s.sp_last;
}

// A fixed interval that outlasts the windows: once the species' particles have left what their tiles' windows can follow
// (three cells: ~27 steps of the two-stream beams), every deposit is twelve global atomics and a launch costs four times
// what it should (round 3: sort_interval = 40 ran at 14 G pushes/s).  The runs that missed the windows in the last launch
// (PW_MISSED: stale by a launch or two, which is early enough) cost ~0.17 ns and more each (they pile up on the same few
// accumulators: round 3 measured +50 ms per launch), a sort ~18 ps per particle: when one launch missed more than 32 runs per
// tile -- half of where the windows stop following (publish_counter_kernel) -- and at least two steps are left, sort now.
// (cycle, PW_CYCLE: the sort cycle the count was taken in -- the host runs ahead of the device, and a count from before the
// last sort must not trigger another)
inline bool early_sort(Policy &s, int64_t missed, unsigned cycle, int64_t left, int64_t ntiles, int64_t np) {
  // ... and the steps left must pay for it: a missed run costs ~0.34 ns (39.3 against 34.1 ms per step at 7.4e6 of them per
  // launch, profiles/r04_sort_interval_40_step_by_step.txt), an unscheduled sort ~19 ps per particle (it cannot happen inside
  // the push), and the misses grow: sort when misses x steps left exceed a 27th of the particles.  (The heated two-stream
  // deck at interval 10 reaches 32 runs per tile three steps before its scheduled sort: not worth one of its own.)
  if (cycle == (unsigned)s.n_cycle && left >= 2 && missed > 32ll * ntiles && missed * left * 27 > np) { s.early_sorts++; return true; }
  return false;
}

// k_sort_p: what the sort of a species asked for (tile_order; may_fuse: the caller pushes it next) is, and which count it takes.
// counts_ready: the push before counted for this sort (Species::hist_valid, big enough); tile_coarse, old_sort: knobs
struct SortInputs {
  bool tile_order = false, may_fuse = false, adaptive = false, chargeless = false, has_tags = false, tile_valid = false, coarse_sorted = false;
  bool counts_ready = false, det_acc = false, time_kernels = false, old_sort = false; int tile_coarse = -1; int64_t np = 0, n_sorted = 0;
};
// coarse: by tile only; fuse: inside the push that follows (nothing moves now); counted: from the push's counts; by_wave, count_by_wave: the
// scatter and count a wavefront at a time
struct SortPlan { bool coarse = false, fuse = false, counted = false, by_wave = false, count_by_wave = false; };
inline SortPlan plan_sort(Policy &s, const SortInputs &in) {
  SortPlan pl;
  // by tile only: species most of whose particles change cell every step (the push keeps the fraction); VPIC_HIP_TILE_COARSE=0|1 overrides
  // (measured, 128^3 x 32 ppc two-stream with adaptive sorting: vth = 0.6 c 7.6 -> 5.8 ms per step, 0.24 c 5.8 -> 4.8, 0.1 c
  // even, cold beams 3 % slower by tile only: the switch is at a fifth of the particles crossing per step)
  // Which of the two is a matter of sizes too (3 M particles per species at 50 ppc, the production deck at test size: by
  // tile only is 20 % SLOWER), so where the engine's sort policy times the cycles it is decided by measurement: the
  // other flavour is tried for a few cycles now and then, the cheaper one per step is kept (sort_due records the costs).
  // Without timings: by tile only from a fifth of the particles crossing per step.
  if (in.tile_order) {
    // (a species of a few million particles does not fill the GPU with 2048-particle workgroups: there the count's serial
    // LDS chains and the unordered push are slower -- not even tried below 8 M)
    const bool eligible = in.np >= ((int64_t)8 << 20) && (s.cross_frac > 0.20 || (s.coarse_order && s.cross_frac > 0.15));
    if (!eligible) { s.coarse_order = false; s.flavour_cost[0] = s.flavour_cost[1] = 0; s.flavour_cycles = 0; }
    else if (!in.adaptive) s.coarse_order = true;
    else {
      const int cur = s.coarse_order ? 1 : 0, other = 1 - cur;
      bool change = false;
      if ((s.n_cycle & 127) == 127) s.flavour_cost[other] = 0;                       // look again now and then
      if (s.flavour_cycles >= 4 && s.flavour_cost[cur] > 0) {
        if (s.flavour_cost[other] == 0) change = true;                                // never tried (or forgotten): try it
        else if (s.flavour_cost[other] < 0.97 * s.flavour_cost[cur]) change = true;   // on record and cheaper
      }
      if (change) {
        s.coarse_order = !s.coarse_order; s.flavour_cycles = 0;
      }
    }
  }
  pl.coarse = in.tile_order && (s.coarse_order || in.chargeless);   // (nothing to deposit: no runs of equal cells to keep together)
  if (in.tile_order && in.tile_coarse >= 0) pl.coarse = in.tile_coarse != 0;
  // The sort inside the push: by tile and cell, counted by the push before, the species as that push left it, and the caller
  // pushes it next -- then nothing moves here.  (Not for: tags, which ride outside the push; the deterministic mode and the
  // phased push, which run other instances; the adaptive policy, which times sort and push apart.)
  pl.fuse = in.may_fuse && in.tile_order && !pl.coarse && in.tile_valid && !in.coarse_sorted && !s.tile_unbalanced && in.counts_ready &&
            !in.has_tags && !in.det_acc && !in.time_kernels && !in.old_sort && in.np <= ((int64_t)1 << 30) && in.np == in.n_sorted;
  // Which count / scatter: a workgroup at a time (LDS table of up to 512 distinct keys per 2048 particles), or -- for a hot
  // species in the reference's order, where a chunk's particles sit in nearly as many voxels as there are particles and
  // the count's table would overflow into one global atomic per particle -- the COUNT a wavefront at a time (measured, 67 M
  // particles at vth = 0.6 c by voxel: count 2.4 ms against 1.8; the scatter stays by workgroup there, 2.7 ms against 7.3)
  pl.by_wave = in.old_sort;
  pl.count_by_wave = pl.by_wave || (!in.tile_order && s.cross_frac > 0.15);
  // the push before this sort may have counted already (Species::hist, push.hip): then the sort starts at its scan
  pl.counted = in.tile_order && !pl.coarse && in.counts_ready;
  return pl;
}

// k_advance_p: which advance_p_kernel instance a push launches, and with what
struct PushInputs {
  int phase = 0;                               // vpic_hip_advance_p_phase: 0 the whole species, 1 / 2 its boundary / interior tiles
  int64_t np = 0, n_sorted = 0; double ppc = 0;
  unsigned crossers = 0, fullest_tile = 0;     // the pinned words PW_CROSSERS, PW_FULLEST_TILE
  int window = 0, iters = 0, stage = -1; int64_t tail_sort_min = 0; bool no_tail_sort = false;   // knobs
  int wx[2] = {0, 0}, wmargin = 0, threads = 0, max_iters = 0;   // row windows' cells (narrow, wide), margin, workgroup, most passes
  bool tile_valid = false, chargeless = false, coarse_sorted = false, det_acc = false, time_kernels = false;
  bool fuse_pending = false, hist_request = false, hist_valid = false, fuse_buffers = false;   // fuse_buffers: second buffer and tpart2 allocated
};
enum class PushInstance { chargeless, det_tile_only, det_tile, det_row, tile_only, tile_sort, tile_hist, tile, row_wide, row_narrow };
// tiled: one workgroup per tile; fuse: the sort inside this push; sort_first: one was pending and cannot be (sort the ordinary
// way, then push); regroup_tail: the appended particles by tile first (k_tail_sort); hist: count for the next sort; det: deterministic
struct PushPlan {
  bool tiled = false, fuse = false, sort_first = false, regroup_tail = false, hist = false, det = false; int stage = 0;
  PushInstance instance = PushInstance::row_narrow;
};

// Which row window, and passes per wavefront: a workgroup's chunk should span a little less than the LDS window (measured,
// tools/iters_sweep.sh: 32 ppc best at 6 passes, 64 ppc at 12, 512 ppc at 64; one pass too many and the chunk overflows the window)
inline int push_passes(Policy &s, const PushInputs &in) {
  // Which window: the crossing fraction of this species' previous launch (a pinned word the device wrote behind
  // that launch; a stale value only delays the switch) with hysteresis; VPIC_HIP_WINDOW=wide|narrow overrides.
  if (in.phase != 2) {
    const double frac = s.np_pushed_last > 0 ? (double)in.crossers / (double)s.np_pushed_last : 0.0;
    s.cross_frac = frac;
    if (frac > 0.30) s.wide_window = true; else if (frac < 0.20) s.wide_window = false;
    if (in.window == 'w') s.wide_window = true; else if (in.window == 'n') s.wide_window = false;
    s.np_pushed_last = in.np;
  }
  const int wx = in.wx[s.wide_window ? 1 : 0];
  const int it = (int)(0.9 * (wx - 2 * in.wmargin) * in.ppc / in.threads);
  if (in.iters > 0) return in.iters;   // tuning experiments
  return it < 1 ? 1 : it > in.max_iters ? in.max_iters : it;
}

// the rest, once push_passes' passes have split the species into n_seg launches
inline PushPlan plan_push(Policy &s, const PushInputs &in, int n_seg) {
  PushPlan pl;
  // A tile is one workgroup's work.  When the fullest tile alone would take several times what the whole launch takes
  // if balanced (1280 workgroups run at a time: 256 CUs x 5), the species is too clumped for tiles: this launch falls
  // back to the row windows and the next sort to the reference's order.  (The count is the last tile sort's, read from
  // pinned memory without waiting: a stale value only delays the switch.)
  // (phase 2 keeps what phase 1 decided: the word is written by the sort's kernels while the host runs ahead of them, and a
  // flip between the two launches of one push would leave the interior tiles unpushed with the boundary movers on the wire)
  if (in.phase != 2 && in.tile_valid && (double)in.fullest_tile * 1280.0 > 4.0 * (double)in.np && in.fullest_tile > 65536u) s.tile_unbalanced = true;
  pl.tiled = in.phase == 2 ? true : (in.tile_valid && !s.tile_unbalanced && !in.chargeless && n_seg == 1);   // (phase 2 only runs behind a phase 1 that split the tiles: phase_pending)
  // the positions of a pass wait for its crossers (STAGE instances: species sorted by tile only, charge-0 copies) when the
  // queue fills every other pass anyway -- from a third of the particles crossing per step on (a colder species would pay
  // for half-empty batches: two drains where one did); VPIC_HIP_STAGE=0|1 overrides
  pl.stage = in.stage >= 0 ? in.stage : (s.cross_frac > 0.33 ? 1 : 0);
  // the sort inside the push (Species::fuse_pending) -- not after all when a tile turned out overfull, the next step sorts too and
  // this push must count for it, ...
  pl.fuse = in.fuse_pending && pl.tiled && !in.coarse_sorted && in.phase == 0 && !in.det_acc && !in.hist_request && in.hist_valid &&
            in.fuse_buffers && in.np == in.n_sorted && !in.time_kernels;
  pl.sort_first = in.fuse_pending && !pl.fuse;
  const int64_t behind = in.np > in.n_sorted ? in.np - in.n_sorted : 0;
  pl.regroup_tail = pl.tiled && behind >= in.tail_sort_min && behind > 0 && !in.no_tail_sort;   // a handful costs less pushed as it is (tests lower the threshold)
  // the histogram of the next sort (Species::hist): tile order by cell, one launch, float sums, no tile anywhere near 2^15 particles
  pl.hist = !pl.fuse && in.hist_request && pl.tiled && !in.coarse_sorted && in.phase == 0 && !(in.det_acc && !in.chargeless) &&
            (uint64_t)in.fullest_tile + (uint64_t)behind < 30000u;   // (16-bit counters per window cell: the fullest tile AND whatever share of the appended particles its workgroup takes)
  // deterministic accumulation: the kernels add into the engine's 64-bit fixed-point accumulator (engine.hip, acc_finalize)
  pl.det = in.det_acc && !in.chargeless;
  pl.instance = in.chargeless ? PushInstance::chargeless
              : pl.det ? (pl.tiled ? (in.coarse_sorted ? PushInstance::det_tile_only : PushInstance::det_tile) : PushInstance::det_row)
              : !pl.tiled ? (s.wide_window ? PushInstance::row_wide : PushInstance::row_narrow)
              : in.coarse_sorted ? PushInstance::tile_only : pl.fuse ? PushInstance::tile_sort : pl.hist ? PushInstance::tile_hist : PushInstance::tile;
  return pl;
}

// ---- the streaming passes over one species (spectrum.hip, distribution.hip): every wavefront takes a contiguous chunk -------
// chunk of each of `waves` wavefronts that share n particles, a multiple of 64
inline long long chunk_for(long long n, long long waves) { return ((n + waves - 1) / waves + 63) / 64 * 64; }
// workgroups of waves_per_group wavefronts for np > 0 particles: 16 passes of 64 per wavefront, 2048 workgroups at the most
struct Chunks { long long groups = 0, chunk = 0; };
inline Chunks plan_chunks(long long np, int waves_per_group) {
  Chunks c;
  const long long per_group = 64ll * waves_per_group * 16;
  c.groups = std::min(2048ll, (np + per_group - 1) / per_group);
  c.chunk = chunk_for(np, c.groups * waves_per_group);
  return c;
}

// spectrum.hip: sort keys per window of linear bands (0: no window, every particle adds to global memory)
constexpr int SPEC_WIN_WORDS = 3072;           // LDS words a wavefront's window of linear bands may take (12 KB)
constexpr int SPEC_WIN_KEYS = 128;             // ... and the most sort keys it spans
inline int spectrum_window(int n_lin) {
  if (n_lin <= 0) return 0;
  const int win = SPEC_WIN_WORDS / n_lin;
  return win >= SPEC_WIN_KEYS ? SPEC_WIN_KEYS : win >= 64 ? 64 : 0;   // (a tile's 64 keys at least, or no window)
}

// distribution.hip: which of the three paths a (checked) descriptor takes, and the window's shape (include/vpic_hip.h states
// the rule).  n[a], d[a], position[a]: bins, bin width and "is X, Y or Z" of axis a (n[1] = 1 for one axis); lds_bins:
// VPIC_HIP_DIST_LDS_BINS
constexpr int DIST_WIN_WORDS = 3072;           // LDS words a wavefront's window may take (12 KB)
constexpr int DIST_WIN_SPARE_WORDS = 2048;     // ... and up to where it is given DIST_WIN_SPARE bins more than a tile touches
constexpr int DIST_WIN_SPARE = 3;
enum { DIST_LDS = 0, DIST_WINDOW = 1, DIST_GLOBAL = 2 };
struct DistPlan { int path = DIST_LDS, pos_axis = 0, win = 0, n_other = 1; };   // DIST_WINDOW: which axis slides, bins of it per window, bins of the other axis
inline DistPlan plan_distribution(int n_axes, const int n[2], const double d[2], const bool position[2], int lds_bins) {
  DistPlan pl;
  if ((long long)n[0] * n[1] <= lds_bins) return pl;
  pl.path = DIST_GLOBAL;
  int pa = -1;
  for (int a = n_axes - 1; a >= 0; a--) if (position[a]) pa = a;
  if (pa < 0) return pl;
  const int n_pos = n[pa], n_other = n[1 - pa];
  const double tile_bins = ceil((double)TILE_EDGE / d[pa]) + 1.0;             // bins the cells of one tile can touch
  if (!(tile_bins * n_other <= (double)DIST_WIN_WORDS)) return pl;
  int win = (int)tile_bins;
  if ((win + DIST_WIN_SPARE) * n_other <= DIST_WIN_SPARE_WORDS) win += DIST_WIN_SPARE;   // fewer slides along a row of voxels, while it is cheap
  if (win > n_pos) win = n_pos;
  pl.path = DIST_WINDOW; pl.pos_axis = pa; pl.win = win; pl.n_other = n_other;
  return pl;
}

// distribution.hip, the per-bin sums (vpic_hip_species_distribution_sums): which of the two paths bins x n_val values take,
// and the LDS words of it.  A bin holds one 32-bit count and n_val 64-bit sums, 1 + 2 n_val words; the whole histogram stays
// in LDS while that fits the words the counts alone may take (lds_words: VPIC_HIP_DIST_LDS_BINS, 32 KB -- the budget of
// the histogram's LDS path: five workgroups of four wavefronts to a CU's 160 KB, which is the 5 waves per SIMD the
// instances without field factors reach by their registers; those with them reach 3, profiles/dist_sums_resources.txt -- so
// LDS never lowers the occupancy).  Everything larger adds in global memory: the sums have no sliding window.
struct DistSumsPlan { int path = DIST_LDS; long long words = 0; };           // words: 32-bit LDS words (0 for DIST_GLOBAL)
inline DistSumsPlan plan_distribution_sums(long long bins, int n_val, int lds_words) {
  DistSumsPlan pl;
  const long long words = bins * (1 + 2 * (long long)n_val);
  if (words <= lds_words) pl.words = words; else pl.path = DIST_GLOBAL;
  return pl;
}

// cell_dist.hip: the workgroups of the pass over the interior cells.  A workgroup takes per_group consecutive cells at a
// time and strides over the rest; as many workgroups as the cells fill, so that a grid of six cells launches one and no
// workgroup is idle, and 2048 at the most (eight to a CU: 256^3 cells are 32 rounds of each, and the LDS path's final adds
// to global memory, one per non-empty word and workgroup, stay few beside the cells).
inline long long plan_cell_groups(long long cells, int per_group) {
  return std::max(1ll, std::min(2048ll, (cells + per_group - 1) / per_group));
}

// DIST_WINDOW on a species in tile order: which particles a wavefront takes.  All tiles with the same tile index along
// the position axis (a "column") touch the same few bins of it, so a wavefront that takes `group` tiles of ONE column
// moves its window once and flushes it once for all of them -- a flush adds every non-zero word of the window to global
// memory, and with one tile per flush (a contiguous chunk of the array) that is one global add for every two
// particles of the headline case.  Wavefront w < items takes members [(w % groups_per_col) * group, + group) of column
// w / groups_per_col; what was appended since the sort, [n_sorted, np), is shared out in contiguous chunks of tail_chunk
// among the wavefronts from item_waves on (a whole number of workgroups: those between items and item_waves take nothing).
// by_tile false: contiguous chunks (plan_chunks).  fallback_chunk: every wavefront's chunk where tpart[] turns out not to be a
// partition (k_check_tile_partition).
constexpr long long DIST_ITEM_PARTICLES = 32768;   // particles a wavefront takes on average, at the most
struct DistTilePlan {
  bool by_tile = false;
  int n_col = 0, members = 0, group = 0, groups_per_col = 0, items = 0, item_waves = 0;   // members: tiles per column
  long long groups = 0, tail_chunk = 0, fallback_chunk = 0;                             // groups: workgroups of the launch
};
// axis: 0 x, 1 y, 2 z; usable: tile_partition_usable (engine.h)
inline DistTilePlan plan_dist_tiles(int ntx, int nty, int ntz, int axis, bool usable, long long n_sorted, long long np, int waves_per_group) {
  DistTilePlan pl;
  if (!usable || n_sorted <= 0) return pl;
  // tiles per wavefront: 8 (a flush per 8 tiles), more on grids of more than 65 536 tiles, fewer while that leaves
  // a wavefront more than DIST_ITEM_PARTICLES on average (too few wavefronts for the chip)
  const int ntiles = ntx * nty * ntz;
  pl.n_col = axis == 0 ? ntx : axis == 1 ? nty : ntz;
  pl.members = ntiles / pl.n_col;
  pl.group = std::min(pl.members, std::max(8, (ntiles + 8191) / 8192));
  while (pl.group > 1 && (long long)pl.n_col * ((pl.members + pl.group - 1) / pl.group) * DIST_ITEM_PARTICLES < n_sorted)
    pl.group = (pl.group + 1) / 2;
  pl.groups_per_col = (pl.members + pl.group - 1) / pl.group;
  pl.items = pl.n_col * pl.groups_per_col;
  // still too few wavefronts for the particles (and not a chip's worth of them either): contiguous chunks
  if (!(pl.items >= 4096 || (long long)pl.items * DIST_ITEM_PARTICLES >= n_sorted)) return pl;
  pl.by_tile = true;
  const long long item_groups = (pl.items + waves_per_group - 1) / waves_per_group;
  pl.item_waves = (int)(item_groups * waves_per_group);
  const Chunks tail = np > n_sorted ? plan_chunks(np - n_sorted, waves_per_group) : Chunks();
  pl.tail_chunk = tail.chunk;
  pl.groups = item_groups + tail.groups;
  pl.fallback_chunk = chunk_for(np, pl.groups * waves_per_group);
  return pl;
}

// accumulate_hydro_p / accumulate_rho_p (moments.hip): how the moments of one species are summed.
//   tiled         one workgroup per tile of a species in tile order (LDS window of the tile's nodes), what was appended
//                 since the sort one thread per particle; the array is not reordered
//   per_particle  one thread per particle over the whole array, global atomics (64-bit ones in deterministic mode: slow)
//   cells         the float path of the reference's order: sorted by voxel first (which costs the tile order), one thread per voxel
// tpart_ok: tile_valid, tpart[] allocated for this grid, n_sorted within np (whether tpart[] IS a partition is checked on
// the device; where it is not, everything goes through the per-particle pass); wants_tile: the engine would push the species
// in tile order (wants_tile_order); per_particle_knob: VPIC_HIP_HYDRO_PER_PARTICLE resp. VPIC_HIP_RHO_PER_PARTICLE;
// tiled_knob: VPIC_HIP_MOMENTS_TILED (0: the deterministic sums per particle, the float sums as before there was a tile path)
struct MomentInputs {
  bool det = false, tile_valid = false, tpart_ok = false, wants_tile = false, per_particle_knob = false, tiled_knob = true;
  int64_t np = 0, nm = 0, nv = 0;
};
enum class MomentPath { tiled, per_particle, cells };
struct MomentPlan { MomentPath path = MomentPath::per_particle; bool sort_by_tile_first = false; };
inline MomentPlan plan_moments(const MomentInputs &in) {
  MomentPlan pl;
  // the float path of a species that is not in tile order: from a few particles per voxel on, by cell (it sorts by voxel)
  const MomentPath untiled_float = in.np >= 4 * in.nv && in.nm == 0 && !in.per_particle_knob ? MomentPath::cells : MomentPath::per_particle;
  if (!in.tiled_knob) { pl.path = in.det ? MomentPath::per_particle : untiled_float; return pl; }
  if (in.tile_valid && in.tpart_ok && in.nm == 0) { pl.path = MomentPath::tiled; return pl; }
  if (!in.det) { pl.path = untiled_float; return pl; }
  // deterministic: a species the engine pushes in tile order is put (back) into it, as before a deterministic push
  if (in.nm == 0 && in.np > 0 && in.wants_tile) { pl.path = MomentPath::tiled; pl.sort_by_tile_first = true; }
  return pl;
}

// accumulate_hydro_p_select: the moments of a selection READ the species and leave it as it is, so no plan of theirs sorts,
// in either accumulation mode, and the float sums never take the by-cell route (which sorts by voxel).  A species in tile order
// with a partition on record and no movers in flight is summed by tile (tile pass + tail pass), any other -- also under
// VPIC_HIP_MOMENTS_TILED=0 -- by the per-particle pass over the whole array.
inline MomentPlan plan_moments_select(const MomentInputs &in) {
  MomentPlan pl;
  pl.path = in.tiled_knob && in.tile_valid && in.tpart_ok && in.nm == 0 ? MomentPath::tiled : MomentPath::per_particle;
  return pl;
}

// vpic_hip_collide (collide.hip): where the two species are collided and by which kernel instance.
// A species has EXACT cell ranges when it is sorted by voxel with partition[] valid, or in tile order by cell (not by tile only)
// with nothing appended (n_sorted == np), no dead slots, no sort pending inside its next push -- and the checking pass, once
// it has run, found every particle inside the range of its own voxel (check_failed: it ran and did not; a push since the
// sort that moved a particle out of its cell shows there).  Such a species is collided where it lies; any other is sorted
// first (in the order the engine would sort it into now, never by tile only: the caller's business) and checked again.
// fullest: particles of this species in its fullest cell, as the checking pass counted them (0 before it has run).
struct CollideSpecies {
  bool partition_valid = false, tile_valid = false, coarse_sorted = false, fuse_pending = false, check_failed = false;
  int64_t np = 0, n_sorted = 0, n_holes = 0, fullest = 0;
};
enum class CollideInstance { none, wave, group };   // a wavefront per cell (both species at most COLLIDE_WAVE_CELL there), a workgroup per cell
constexpr int COLLIDE_WAVE_CELL = 64;
struct CollidePlan { bool sort_a = false, sort_b = false, over_cap = false; CollideInstance instance = CollideInstance::none; };
inline bool collide_ranges_exact(const CollideSpecies &s) {
  if (s.np == 0) return true;                                                  // nothing to pair: no range is read
  if (s.check_failed || s.n_holes > 0 || s.fuse_pending) return false;
  if (s.tile_valid) return !s.coarse_sorted && s.n_sorted == s.np;
  return s.partition_valid;
}
// same: sp_a == sp_b (b is then not looked at); cap: VPIC_HIP_COLLIDE_MAX_CELL; force_group: VPIC_HIP_COLLIDE_INSTANCE=group
inline CollidePlan plan_collide(const CollideSpecies &a, const CollideSpecies &b, bool same, int cap, bool force_group) {
  CollidePlan pl;
  pl.sort_a = !collide_ranges_exact(a);
  pl.sort_b = !same && !collide_ranges_exact(b);
  const int64_t fullest = same ? a.fullest : std::max(a.fullest, b.fullest);
  pl.over_cap = fullest > cap;
  if (pl.sort_a || pl.sort_b || pl.over_cap || fullest == 0) return pl;        // (nothing is launched before the ranges are exact)
  pl.instance = fullest <= COLLIDE_WAVE_CELL && !force_group ? CollideInstance::wave : CollideInstance::group;
  return pl;
}

// Fixed-point scales of the 14 hydro moments in deterministic mode (jx jy jz rho px py pz ke txx tyy tzz tyz tzx txy): one
// power of two each, chosen per call from the species' largest macro-particle charge q_max, its q_m, r8V = 1 / (8 dV) and c.
// A particle's weight on a node is at most W = 8 r8V q_max, |v| < c, and its time-centred momentum is |u|, so ONE contribution
// is at most B(|u|):
//   jx jy jz   W c                     rho   W
//   px py pz   W |c / q_m| |u|         ke    W |c / q_m| c |u|   (ke_mc = c u^2 / (gamma + 1) < c |u|)
//   txx .. txy W |c / q_m| c |u|       (p_i v_j)
// The off-diagonal stresses tyz tzx txy reach half of their bound only: |u_i u_j| / gamma <= (u_i^2 + u_j^2) / (2 gamma) <
// |u| / 2 (gamma > |u|).  So the largest contribution at |u| = 1 is R = part B(1), part = 1/2 for those three and 1 elsewhere.
// With R (1 + 2^-16) = m 2^ex, 1/2 <= m < 1 (frexp), the scale is 2^(36 - ex), the largest power of two the sum below allows:
// a contribution as large as a particle of weight W at |u| = 1 can make it lands in [2^35, 2^36), strictly below 2^36 by the
// 2^-16 (the kernel's float arithmetic rounds W, gamma and the products by parts in 2^24 each, a few of them: 2^-16 covers
// that).  Then
//   - a unit contribution is at 2^28 or higher (2^35), so half a quantum is 2^-36 of it or less;
//   - a contribution at |u| <= 2^12 is below 2^36 2^12 = 2^48 < 2^51: it converts (to_fixed needs |x scale| < 2^51; the
//     kernel counts what does not and the call fails -- from |u| = 2^15 on for weight W, sooner never);
//   - 2^20 particles of charge q_max at |u| <= 2^7 sum to less than 2^20 2^7 2^36 = 2^63: they fit one signed word.
// The scale sits at the top of what the sum allows because the small moments of a fast species need it: at |u| = 2^12 along x a
// tyz contribution is u_y u_z / gamma ~ 2^-15 of the unit, and a node's sum of a couple of hundred of them, signs mixed, is
// held to 2e-6 of itself by the tests (tests/test_gpu_moments.py: test_range) -- a dozen quanta at this scale.
// Nothing to scale (a chargeless species, q_m = 0): scale 1, every contribution is 0.
constexpr int N_HYDRO_MOMENTS = 14;
struct MomentScales { double scale[N_HYDRO_MOMENTS], bound[N_HYDRO_MOMENTS], part[N_HYDRO_MOMENTS]; };   // bound: B of each moment; part: the share of it a contribution reaches
inline MomentScales moment_scales(double q_max, double q_m, double r8V, double c) {
  MomentScales ms;
  const double W = 8.0 * fabs(r8V) * fabs(q_max), mc_q = q_m != 0 ? fabs(c / q_m) : 0.0;
  for (int k = 0; k < N_HYDRO_MOMENTS; k++) {
    const double B = k < 3 ? W * c : k == 3 ? W : k < 7 ? W * mc_q : W * mc_q * c;
    int ex = 0;
    ms.bound[k] = B;
    ms.part[k] = k >= 11 ? 0.5 : 1.0;
    ms.scale[k] = 1.0;
    if (B > 0 && B < HUGE_VAL) { (void)frexp(B * ms.part[k] * (1.0 + ldexp(1.0, -16)), &ex); ms.scale[k] = ldexp(1.0, 36 - ex); }
  }
  return ms;
}

}  // namespace vpichip
