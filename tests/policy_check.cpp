// The engine's host decisions (old-vpic_amd/csrc/policy.h) -- sort, push, and the launch shapes of the passes over one
// species -- on the host: one case per rule the code states.
// usage: policy_check [case ...] (no case: all of them; --list: their names).  Prints "ok <case>" or "FAIL <case>: ..." lines.
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <vector>
#include "policy.h"

using namespace vpichip;

static int failures;
static const char *current;
#define CHECK(cond)                                                                           \
  do {                                                                                        \
    if (!(cond)) { printf("FAIL %s: line %d: %s\n", current, __LINE__, #cond); failures++; }   \
  } while (0)

// a species as the push finds it: tile order, one launch, nothing pending
static PushInputs push_in() {
  PushInputs in;
  in.np = in.n_sorted = 10000000; in.ppc = 32;
  in.wx[0] = 62; in.wx[1] = 42; in.wmargin = 4; in.threads = 256; in.max_iters = 64;
  in.tail_sort_min = 4096;
  in.tile_valid = true;
  return in;
}
static SortInputs sort_in() {
  SortInputs in;
  in.tile_order = true; in.np = in.n_sorted = (int64_t)16 << 20;
  return in;
}
// a policy that has sorted before (not in any of the cycles with a rule of their own)
static Policy sorted_policy() {
  Policy p;
  p.sorted_once = true; p.n_cycle = 1; p.t_sort = 10;
  return p;
}

static void row_window() {
  Policy p; PushInputs in = push_in(); in.np = 1000;
  push_passes(p, in);
  CHECK(!p.wide_window && p.cross_frac == 0 && p.np_pushed_last == 1000);   // the first push: nothing crossed yet
  in.crossers = 301; push_passes(p, in); CHECK(p.wide_window && p.cross_frac == 0.301);
  in.crossers = 250; push_passes(p, in); CHECK(p.wide_window);              // held between 0.20 and 0.30
  in.crossers = 200; push_passes(p, in); CHECK(p.wide_window);
  in.crossers = 199; push_passes(p, in); CHECK(!p.wide_window);
  in.crossers = 300; push_passes(p, in); CHECK(!p.wide_window);             // held
  in.crossers = 0; in.window = 'w'; push_passes(p, in); CHECK(p.wide_window);
  in.crossers = 1000; in.window = 'n'; push_passes(p, in); CHECK(!p.wide_window);
  in.window = 0; in.phase = 2; in.crossers = 900; p.np_pushed_last = 1000;  // phase 2 keeps what phase 1 decided
  push_passes(p, in); CHECK(!p.wide_window && p.cross_frac == 1.0);
}

static void passes_per_wavefront() {
  Policy p; PushInputs in = push_in();
  CHECK(push_passes(p, in) == 6);                        // 0.9 * (62 - 8) * 32 / 256 = 6.08
  p.np_pushed_last = in.np; in.crossers = (unsigned)(0.5 * in.np);
  CHECK(push_passes(p, in) == 3 && p.wide_window);       // 0.9 * (42 - 8) * 32 / 256 = 3.83
  in.ppc = 64; CHECK(push_passes(p, in) == 7);
  in.ppc = 1; CHECK(push_passes(p, in) == 1);            // clamped to [1, PUSH_ITERS]
  in.ppc = 4096; CHECK(push_passes(p, in) == 64);
  in.iters = 9; CHECK(push_passes(p, in) == 9);          // VPIC_HIP_ITERS
}

static void tile_imbalance() {
  Policy p; PushInputs in = push_in(); in.np = in.n_sorted = 1000000;   // 4 * np / 1280 = 3125: the second bound decides
  in.fullest_tile = 65536; CHECK(plan_push(p, in, 1).tiled && !p.tile_unbalanced);
  in.fullest_tile = 65537; CHECK(!plan_push(p, in, 1).tiled && p.tile_unbalanced);
  in.fullest_tile = 0; CHECK(!plan_push(p, in, 1).tiled && p.tile_unbalanced);   // stays set ...
  p.new_cycle(false); CHECK(p.tile_unbalanced);                                  // ... through a sort by voxel
  p.new_cycle(true); CHECK(!p.tile_unbalanced && plan_push(p, in, 1).tiled);     // until a tile sort clears it
  in.np = in.n_sorted = 100000000;                                               // 4 * np / 1280 = 312500
  in.fullest_tile = 312500; CHECK(plan_push(p, in, 1).tiled);
  in.fullest_tile = 312501; CHECK(!plan_push(p, in, 1).tiled);
  p = Policy(); in.tile_valid = false; plan_push(p, in, 1); CHECK(!p.tile_unbalanced);
  in.tile_valid = true; in.phase = 2; CHECK(plan_push(p, in, 1).tiled && !p.tile_unbalanced);   // phase 2: always tiled, never looks
  in.phase = 0; in.fullest_tile = 0;
  CHECK(!plan_push(p, in, 2).tiled);                     // tiled: one launch only
  in.chargeless = true; CHECK(!plan_push(p, in, 1).tiled);
  in.chargeless = false; in.tile_valid = false; CHECK(!plan_push(p, in, 1).tiled);
}

static void stage() {
  Policy p; PushInputs in = push_in();
  p.cross_frac = 0.331; CHECK(plan_push(p, in, 1).stage == 1);
  p.cross_frac = 0.329; CHECK(plan_push(p, in, 1).stage == 0);
  in.stage = 0; p.cross_frac = 0.9; CHECK(plan_push(p, in, 1).stage == 0);   // VPIC_HIP_STAGE
  in.stage = 1; p.cross_frac = 0; CHECK(plan_push(p, in, 1).stage == 1);
}

static void histogram() {
  Policy p; PushInputs in = push_in(); in.hist_request = true;
  in.fullest_tile = 29999; CHECK(plan_push(p, in, 1).hist);
  in.fullest_tile = 30000; CHECK(!plan_push(p, in, 1).hist);
  in.fullest_tile = 29000; in.np = in.n_sorted + 1000; CHECK(!plan_push(p, in, 1).hist);   // the fullest tile and the appended ones
  in.np = in.n_sorted + 999; CHECK(plan_push(p, in, 1).hist);
  in.np = in.n_sorted; in.fullest_tile = 0;
  in.det_acc = true; CHECK(!plan_push(p, in, 1).hist);   // not under deterministic charged pushes
  in.det_acc = false; in.coarse_sorted = true; CHECK(!plan_push(p, in, 1).hist);
  in.coarse_sorted = false; in.phase = 1; CHECK(!plan_push(p, in, 1).hist);
  in.phase = 0; in.hist_request = false; CHECK(!plan_push(p, in, 1).hist);
  in.hist_request = true; CHECK(!plan_push(p, in, 2).hist);                              // not tiled
}

static void sort_inside_fallback() {
  Policy p; PushInputs in = push_in();
  in.fuse_pending = true; in.hist_valid = true; in.fuse_buffers = true;
  PushPlan pl = plan_push(p, in, 1); CHECK(pl.fuse && !pl.sort_first && pl.instance == PushInstance::tile_sort);
  in.hist_request = true; pl = plan_push(p, in, 1); CHECK(!pl.fuse && pl.sort_first);   // the next step sorts too
  in.hist_request = false; in.time_kernels = true; CHECK(plan_push(p, in, 1).sort_first);
  in.time_kernels = false; in.np = in.n_sorted + 1; CHECK(plan_push(p, in, 1).sort_first);
  in.np = in.n_sorted; in.fuse_pending = false; pl = plan_push(p, in, 1); CHECK(!pl.fuse && !pl.sort_first);
}

static void tail_regrouping() {
  Policy p; PushInputs in = push_in();
  in.np = in.n_sorted + 4096; CHECK(plan_push(p, in, 1).regroup_tail);
  in.np = in.n_sorted + 4095; CHECK(!plan_push(p, in, 1).regroup_tail);
  in.np = in.n_sorted + 4096; in.no_tail_sort = true; CHECK(!plan_push(p, in, 1).regroup_tail);
  in.no_tail_sort = false; in.tail_sort_min = 0; in.np = in.n_sorted; CHECK(!plan_push(p, in, 1).regroup_tail);   // nothing behind
}

// the ladder k_advance_p walked before the instances had names
static PushInstance ladder(bool chargeless, bool det, bool tiled, bool coarse_sorted, bool fuse, bool hist, bool wide) {
  if (chargeless) return PushInstance::chargeless;
  if (det && tiled && coarse_sorted) return PushInstance::det_tile_only;
  if (det && tiled) return PushInstance::det_tile;
  if (det) return PushInstance::det_row;
  if (tiled && coarse_sorted) return PushInstance::tile_only;
  if (tiled && fuse) return PushInstance::tile_sort;
  if (tiled && hist) return PushInstance::tile_hist;
  if (tiled) return PushInstance::tile;
  if (wide) return PushInstance::row_wide;
  return PushInstance::row_narrow;
}
static void instance() {
  bool seen[10] = {};
  for (int m = 0; m < 512; m++) {
    Policy p; PushInputs in = push_in();
    in.chargeless = m & 1; in.det_acc = m & 2; in.tile_valid = m & 4; in.coarse_sorted = m & 8;
    in.fuse_pending = m & 16; in.hist_valid = in.fuse_buffers = true; in.hist_request = m & 32; p.wide_window = m & 64;
    in.phase = (m >> 7) & 1; const int n_seg = (m & 256) ? 2 : 1;
    const PushPlan pl = plan_push(p, in, n_seg);
    CHECK(pl.det == (in.det_acc && !in.chargeless));
    CHECK(pl.instance == ladder(in.chargeless, pl.det, pl.tiled, in.coarse_sorted, pl.fuse, pl.hist, p.wide_window));
    seen[(int)pl.instance] = true;
  }
  for (bool b : seen) CHECK(b);                          // every instance is reachable
  Policy p; PushInputs in = push_in(); in.phase = 2; in.det_acc = true;
  CHECK(plan_push(p, in, 1).instance == PushInstance::det_tile);
}

static void tile_order() {
  Policy p;
  CHECK(wants_tile_order(p, 1000, 0, 4, true));
  CHECK(!wants_tile_order(p, 1000, 0, 4, false));        // the caller kept the reference's order
  CHECK(wants_tile_order(p, (int64_t)1 << 30, 0, 4, true));
  CHECK(!wants_tile_order(p, ((int64_t)1 << 30) + 1, 0, 4, true));
  CHECK(!wants_tile_order(p, ((int64_t)1 << 30) + 1, 't', 4, true));
  CHECK(!wants_tile_order(p, 1000, 0, 3, true));         // a grid axis thinner than a tile
  CHECK(wants_tile_order(p, 1000, 't', 1, false));       // VPIC_HIP_WINDOW=tile
  CHECK(!wants_tile_order(p, 1000, 'w', 8, true) && !wants_tile_order(p, 1000, 'n', 8, true));
  p.tile_unbalanced = true;
  for (int c = 0; c < 64; c++) { p.n_cycle = c; CHECK(wants_tile_order(p, 1000, 0, 4, true) == (c % 32 == 31)); }
}

static void flavour() {
  Policy p; SortInputs in = sort_in();
  p.cross_frac = 0.21; CHECK(plan_sort(p, in).coarse && p.coarse_order);       // without timings: by tile only
  p.cross_frac = 0.16; CHECK(plan_sort(p, in).coarse);                          // 0.15 while coarse
  p.cross_frac = 0.14; CHECK(!plan_sort(p, in).coarse && !p.coarse_order);
  p.cross_frac = 0.19; CHECK(!plan_sort(p, in).coarse);                         // 0.20 while not
  p.cross_frac = 0.9; in.np = ((int64_t)8 << 20) - 1; CHECK(!plan_sort(p, in).coarse);   // from 8 M particles
  in.np = (int64_t)8 << 20; CHECK(plan_sort(p, in).coarse);
  p.flavour_cost[0] = 3; p.flavour_cycles = 5; p.coarse_order = false; in.np = 0; plan_sort(p, in);
  CHECK(p.flavour_cost[0] == 0 && p.flavour_cycles == 0);                       // not eligible: forgotten
  in.np = (int64_t)8 << 20; in.tile_order = false; p.coarse_order = true; CHECK(!plan_sort(p, in).coarse && p.coarse_order);
  in.tile_order = true; in.chargeless = true; p.cross_frac = 0; CHECK(plan_sort(p, in).coarse);   // nothing to deposit
  in.tile_coarse = 0; CHECK(!plan_sort(p, in).coarse);                          // VPIC_HIP_TILE_COARSE
  in.chargeless = false; in.tile_coarse = 1; CHECK(plan_sort(p, in).coarse && !p.coarse_order);
  // measured: the other flavour after >= 4 cycles of this one, when untried or < 0.97 x
  in.tile_coarse = -1; in.adaptive = true; p = sorted_policy(); p.cross_frac = 0.5;
  p.flavour_cost[0] = 10; p.flavour_cycles = 3; CHECK(!plan_sort(p, in).coarse);
  p.flavour_cycles = 4; CHECK(plan_sort(p, in).coarse && p.flavour_cycles == 0);   // untried: try it
  p.flavour_cost[1] = 10; p.flavour_cost[0] = 9.75; p.flavour_cycles = 4; CHECK(plan_sort(p, in).coarse);   // 0.975 x: stays
  p.flavour_cost[0] = 9.65; CHECK(!plan_sort(p, in).coarse && p.flavour_cycles == 0);                         // 0.965 x: back
  p.flavour_cost[1] = 9.7; p.flavour_cycles = 4; p.n_cycle = 127;                  // every 128th cycle the other one is forgotten
  CHECK(plan_sort(p, in).coarse && p.flavour_cost[1] == 0);
  p = sorted_policy(); p.cross_frac = 0.5; p.flavour_cycles = 9; CHECK(!plan_sort(p, in).coarse);   // nothing on record of this one
  p.new_cycle(true); CHECK(p.flavour_cycles == 10);
  p.new_cycle(false); CHECK(p.flavour_cycles == 10);
}

static void sort_plan() {
  Policy p; SortInputs in = sort_in(); in.may_fuse = true; in.tile_valid = true; in.counts_ready = true;
  SortPlan pl = plan_sort(p, in); CHECK(pl.fuse && pl.counted && !pl.coarse);
  in.has_tags = true; CHECK(!plan_sort(p, in).fuse);
  in.has_tags = false; in.det_acc = true; CHECK(!plan_sort(p, in).fuse);
  in.det_acc = false; in.time_kernels = true; CHECK(!plan_sort(p, in).fuse);
  in.time_kernels = false; in.coarse_sorted = true; CHECK(!plan_sort(p, in).fuse);
  in.coarse_sorted = false; in.np = in.n_sorted + 1; CHECK(!plan_sort(p, in).fuse);
  in.np = in.n_sorted; p.tile_unbalanced = true; CHECK(!plan_sort(p, in).fuse);
  p.tile_unbalanced = false; in.tile_valid = false; pl = plan_sort(p, in); CHECK(!pl.fuse && pl.counted);
  in.counts_ready = false; CHECK(!plan_sort(p, in).counted);
  in.tile_order = false; p.cross_frac = 0.151; CHECK(plan_sort(p, in).count_by_wave);   // by voxel, hot: count by wavefront
  p.cross_frac = 0.149; CHECK(!plan_sort(p, in).count_by_wave);
  in.old_sort = true; pl = plan_sort(p, in); CHECK(pl.by_wave && pl.count_by_wave);
}

static void sort_inside_or_before() {
  Policy p = sorted_policy();
  CHECK(sort_inside_push(p, false));                     // the first time: inside
  p.sort_push_ms[1] = 19.1f; p.hint_push_ms = 10; CHECK(!sort_inside_push(p, false));   // > 1.9 x the push that counted
  p.sort_push_ms[1] = 18.9f; CHECK(sort_inside_push(p, false));
  p.hint_push_ms = 0; p.sort_push_ms[1] = 100; CHECK(sort_inside_push(p, false));
  p.n_cycle = 15; CHECK(!sort_inside_push(p, false));   // ... or at the sixteenth cycle
  p.n_cycle = 31; CHECK(!sort_inside_push(p, false));
  p.n_cycle = 1; p.sort_push_ms[1] = 20; p.sort_push_ms[0] = 25; CHECK(sort_inside_push(p, false));   // the cheaper one
  p.sort_push_ms[0] = 15; CHECK(!sort_inside_push(p, false));
  p.n_cycle = 7; CHECK(sort_inside_push(p, false));     // flipped every 8th cycle
  p.n_cycle = 15; CHECK(sort_inside_push(p, false));
  p.sort_push_ms[0] = 25; CHECK(!sort_inside_push(p, false) && !p.sp_last);
}

static bool pushes(Policy &p, std::vector<double> ms, int max_interval = 0) {
  bool due = false;
  for (double t : ms) due = sort_due(p, -1, t, false, true, max_interval, false);
  return due;
}
static void sort_due_rule() {
  Policy p;
  CHECK(sort_due(p, -1, -1, false, true, 0, false));     // before the first sort
  // (S_later + sum + T_next) n >= (S_now + sum) (n + 1), S = 10: pushes of 5, 7, 9 ms -> T_next 5, 9, 11
  p = sorted_policy(); CHECK(!pushes(p, {5})); CHECK(!pushes(p, {7})); CHECK(pushes(p, {9}));
  CHECK(p.n_push == 3 && p.t_sum == 21 && p.growth_first == 2);
  p = sorted_policy(); CHECK(!pushes(p, {5, 5, 5, 5, 5, 5}));                // flat pushes never pay for a sort
  p = sorted_policy(); CHECK(!pushes(p, {5, 5, 5}, 4)); CHECK(pushes(p, {5}, 4));   // max_interval
  // the sort's cost after n pushes when on record: dearer later, due a push earlier; never cheaper later
  p = sorted_policy(); p.s_hist[0][2] = 10; p.s_hist[0][3] = 12; CHECK(!pushes(p, {5})); CHECK(pushes(p, {7}));
  p = sorted_policy(); p.s_hist[0][3] = 10; p.s_hist[0][4] = 5; CHECK(pushes(p, {5, 7, 9}));
  // whole cycles of n and n + 1 pushes on record overrule the prediction
  p = sorted_policy(); p.c_hist[0][3] = 8; p.c_hist[0][4] = 7.5; CHECK(!pushes(p, {5, 7, 9}));
  p = sorted_policy(); p.c_hist[0][1] = 7; p.c_hist[0][2] = 7.5; CHECK(pushes(p, {5}));
  // ... but only the current flavour's
  p = sorted_policy(); p.c_hist[1][1] = 7; p.c_hist[1][2] = 7.5; CHECK(!pushes(p, {5}));
  // every 8th cycle ends one push earlier than the last
  p = sorted_policy(); p.n_cycle = 7; p.sorted_after = 3; CHECK(!pushes(p, {5})); CHECK(pushes(p, {5}));
  p = sorted_policy(); p.n_cycle = 6; p.sorted_after = 3; CHECK(!pushes(p, {5, 5}));
  // every 64th cycle forgets the histories
  p = sorted_policy(); p.n_cycle = 63; p.c_hist[0][1] = 7; p.c_hist[0][2] = 7.5; p.n_hist[0] = 5;
  CHECK(!pushes(p, {5}) && p.c_hist[0][1] == 0 && p.n_hist[0] == 1);
  // growth seen by an earlier cycle at the same position
  p = sorted_policy(); p.t_hist[0][0] = 5; p.t_hist[0][1] = 25; p.n_hist[0] = 2; CHECK(pushes(p, {5}));
  // a sort closes a cycle: its cost is booked to the cycle length and (after two cycles of a flavour) to the flavour
  p = sorted_policy(); pushes(p, {5, 5, 5}); p.flavour_cycles = 2; p.new_cycle(true);
  CHECK(p.sorted_after == 3 && p.prev_sum == 15 && p.n_push == 0 && p.t_sum == 0 && p.n_cycle == 2);
  sort_due(p, 6, -1, false, true, 0, false);
  CHECK(p.t_sort == 6 && p.s_hist[0][3] == 6 && p.c_hist[0][3] == 7 && p.flavour_cost[0] == 7);
  sort_due(p, 12, -1, false, true, 0, false);
  CHECK(p.flavour_cost[0] == 8);                         // (7 + 9) / 2
  sort_due(p, 12, -1, true, false, 0, false);
  CHECK(p.s_hist[1][3] == 12 && p.flavour_cost[1] == 0); // not in tile order: no flavour cost
}

static void early() {
  Policy p = sorted_policy();                            // 100 tiles: more than 3200 missed runs
  CHECK(early_sort(p, 3201, 1, 2, 100, 170000) && p.early_sorts == 1);   // 3201 x 2 x 27 = 172854
  CHECK(!early_sort(p, 3201, 1, 2, 100, 173000));
  CHECK(!early_sort(p, 3200, 1, 2, 100, 1000));
  CHECK(!early_sort(p, 3201, 1, 1, 100, 1000));          // at least two steps left
  CHECK(!early_sort(p, 3201, 0, 2, 100, 1000));          // a count from another cycle
  CHECK(!early_sort(p, 3201, ~0u, 2, 100, 1000));
  CHECK(p.early_sorts == 1);
}

// ---- the passes over one species (spectrum.hip, distribution.hip) ----
static void chunks() {
  const int W = 4;
  const long long G = 64ll * W * 16;
  for (long long np : {1ll, 63ll, 64ll, G, G + 1, 2048 * G, 2048 * G + 1, (1ll << 31) - 8192}) {
    const Chunks c = plan_chunks(np, W);
    // what k_energy_spectrum and k_species_distribution each wrote out before they shared this
    long long nb = (np + G - 1) / G;
    if (nb > 2048) nb = 2048;
    const long long waves = nb * W, chunk = ((np + waves - 1) / waves + 63) / 64 * 64;
    CHECK(c.groups == nb && c.chunk == chunk);
    CHECK(c.groups >= 1 && c.groups <= 2048 && c.chunk % 64 == 0 && c.groups * W * c.chunk >= np);
  }
  CHECK(plan_chunks(G, W).groups == 1 && plan_chunks(G + 1, W).groups == 2 && plan_chunks(2048 * G + 1, W).groups == 2048);
}

static void spectrum_window_rule() {
  // 3072 / n_lin keys: 128 of them while there are that many, 64 while there are that many, else no window
  CHECK(spectrum_window(1) == 128 && spectrum_window(24) == 128);     // 3072 / 24 = 128
  CHECK(spectrum_window(25) == 64 && spectrum_window(48) == 64);      // 122, 64
  CHECK(spectrum_window(49) == 0 && spectrum_window(3073) == 0);      // 62, 0
  CHECK(spectrum_window(0) == 0);                                     // no linear bands
}

static DistPlan dist_plan(int n0, double d0, bool pos0, int n1 = 1, double d1 = 1, bool pos1 = false, int lds_bins = 8192) {   // 8192: VPIC_HIP_DIST_LDS_BINS
  const int n[2] = {n0, n1}; const double d[2] = {d0, d1}; const bool pos[2] = {pos0, pos1};
  return plan_distribution(n1 > 1 || pos1 ? 2 : 1, n, d, pos, lds_bins);
}
static void distribution_path() {
  // the whole histogram in LDS up to VPIC_HIP_DIST_LDS_BINS bins, whatever the axes
  CHECK(dist_plan(8192, 1, true).path == DIST_LDS && dist_plan(128, 1, true, 64, 1, false).path == DIST_LDS);
  CHECK(dist_plan(8193, 1, false).path == DIST_GLOBAL && dist_plan(128, 1, false, 65, 1, false).path == DIST_GLOBAL);   // no position axis
  // a position axis first: half a cell per bin, ceil(4 / 0.5) + 1 = 9 bins x 256 = 2304 words; no room for the spare three
  DistPlan pl = dist_plan(256, 0.5, true, 256, 0.01, false);
  CHECK(pl.path == DIST_WINDOW && pl.pos_axis == 0 && pl.win == 9 && pl.n_other == 256);
  // ... second: ceil(4 / 0.75) + 1 = 7 bins x 100, and the spare three
  pl = dist_plan(100, 0.01, false, 126, 0.75, true);
  CHECK(pl.path == DIST_WINDOW && pl.pos_axis == 1 && pl.win == 10 && pl.n_other == 100);
  // both: the first one slides
  pl = dist_plan(128, 1, true, 128, 1, true);
  CHECK(pl.path == DIST_WINDOW && pl.pos_axis == 0 && pl.win == 8 && pl.n_other == 128);
  // a tile's bins x the other axis: at 3072 words the window, above global adds (0.9 cells: 6 bins; 2 cells: 3 bins)
  CHECK(dist_plan(64, 0.9, true, 512, 1, false).path == DIST_WINDOW && dist_plan(64, 0.9, true, 512, 1, false).win == 6);
  CHECK(dist_plan(64, 0.9, true, 513, 1, false).path == DIST_GLOBAL);
  CHECK(dist_plan(1024, 1, false, 64, 2.0, true).path == DIST_WINDOW && dist_plan(1025, 1, false, 64, 2.0, true).path == DIST_GLOBAL);
  // the three spare bins: granted while (5 + 3) x the other axis stays within 2048 words
  CHECK(dist_plan(64, 1, true, 256, 1, false).win == 8 && dist_plan(64, 1, true, 257, 1, false).win == 5);
  CHECK(dist_plan(64, 1, true, 257, 1, false).path == DIST_WINDOW);
  // win never exceeds the axis (with VPIC_HIP_DIST_LDS_BINS as it is such a histogram is held in LDS: a lower bound shows it)
  pl = dist_plan(4, 1, true, 8, 1, false, 16);
  CHECK(pl.path == DIST_WINDOW && pl.win == 4 && pl.n_other == 8);
  CHECK(dist_plan(8, 1, true, 8, 1, false, 16).win == 8 && dist_plan(9, 1, true, 8, 1, false, 16).win == 8);
}

// every wavefront of the launch as species_distribution_kernel<DIST_WINDOW> deals them (distribution.hip: "what this wavefront takes")
static void walk_dist_tiles(int ntx, int nty, int ntz, int axis, long long n_sorted, long long np, bool expect_by_tile) {
  const int W = 4, ntiles = ntx * nty * ntz;
  const DistTilePlan pl = plan_dist_tiles(ntx, nty, ntz, axis, true, n_sorted, np, W);
  CHECK(pl.by_tile == expect_by_tile);
  if (!pl.by_tile) return;
  CHECK(pl.item_waves % W == 0 && pl.item_waves >= pl.items && pl.item_waves < pl.items + W);
  CHECK(pl.n_col * pl.members == ntiles && pl.groups_per_col * pl.n_col == pl.items);
  std::vector<int> taken(ntiles, 0);
  long long tail_to = n_sorted, fallback_to = 0;
  const long long waves = pl.groups * W;
  for (long long w = 0; w < waves; w++) {
    CHECK(w * pl.fallback_chunk == fallback_to || w * pl.fallback_chunk >= np);   // the fallback chunks follow one another from 0 on
    fallback_to = std::max(fallback_to, std::min(w * pl.fallback_chunk + pl.fallback_chunk, np));
    if (w < pl.items) {
      const int col = (int)w / pl.groups_per_col, first_member = ((int)w - col * pl.groups_per_col) * pl.group;
      const int n_seg = std::min(pl.group, pl.members - first_member);
      CHECK(n_seg >= 1);                                   // no item is empty
      for (int seg = 0; seg < n_seg; seg++) {
        const int m = first_member + seg;
        int tx, ty, tz;
        if (axis == 0) { tx = col; ty = m % nty; tz = m / nty; }
        else if (axis == 1) { ty = col; tx = m % ntx; tz = m / ntx; }
        else { tz = col; tx = m % ntx; ty = m / ntx; }
        CHECK(tx >= 0 && tx < ntx && ty >= 0 && ty < nty && tz >= 0 && tz < ntz);
        const int tile = (tz * nty + ty) * ntx + tx;
        if (tile >= 0 && tile < ntiles) taken[tile]++;
      }
    } else if (w >= pl.item_waves) {
      const long long begin = n_sorted + (w - pl.item_waves) * pl.tail_chunk;
      CHECK(begin == tail_to || begin >= np);              // the chunks follow one another from n_sorted on
      tail_to = std::max(tail_to, std::min(begin + pl.tail_chunk, np));
    }
  }
  for (int c : taken) CHECK(c == 1);                       // every tile exactly once
  CHECK(tail_to == np && fallback_to == np);               // [n_sorted, np) and, where tpart[] is no partition, [0, np)
  CHECK(pl.fallback_chunk % 64 == 0 && pl.tail_chunk % 64 == 0 && (pl.tail_chunk > 0) == (np > n_sorted));
  CHECK(pl.groups == pl.item_waves / W + (np > n_sorted ? plan_chunks(np - n_sorted, W).groups : 0));
}
static void distribution_tiles() {
  const int grids[3][3] = {{1, 1, 1}, {3, 2, 1}, {24, 2, 2}};
  for (auto &g : grids)
    for (int axis = 0; axis < 3; axis++) {
      const long long items_most = (long long)g[0] * g[1] * g[2];              // with one tile per wavefront
      walk_dist_tiles(g[0], g[1], g[2], axis, 1000, 1000, true);               // a few particles, nothing appended
      walk_dist_tiles(g[0], g[1], g[2], axis, 1000, 1000 + 64 * 4 * 16 * 3 + 1, true);   // ... four workgroups' worth appended
      walk_dist_tiles(g[0], g[1], g[2], axis, items_most * DIST_ITEM_PARTICLES, items_most * DIST_ITEM_PARTICLES + 5, true);   // group halved down to 1
      // fallback (i): more than DIST_ITEM_PARTICLES per wavefront even with one tile each, and fewer than 4096 wavefronts
      walk_dist_tiles(g[0], g[1], g[2], axis, items_most * DIST_ITEM_PARTICLES + 1, items_most * DIST_ITEM_PARTICLES + 1, false);
    }
  // the group is halved only as far as needed: 24 columns of 4 tiles, 10^6 particles -> two tiles per wavefront
  DistTilePlan pl = plan_dist_tiles(24, 2, 2, 0, true, 1000000, 1000000, 4);
  CHECK(pl.by_tile && pl.group == 2 && pl.groups_per_col == 2 && pl.items == 48 && pl.item_waves == 48 && pl.tail_chunk == 0);
  pl = plan_dist_tiles(24, 2, 2, 0, true, 1000, 1000, 4);
  CHECK(pl.group == 4 && pl.items == 24);
  // 4096 wavefronts fill the chip whatever they hold: by tile
  walk_dist_tiles(64, 64, 1, 0, 200000000, 200000000, true);
  CHECK(plan_dist_tiles(64, 64, 1, 0, true, 200000000, 200000000, 4).items == 4096);
  // fallback (ii): tpart[] is not usable, or nothing is sorted
  CHECK(!plan_dist_tiles(3, 2, 1, 0, false, 1000, 1000, 4).by_tile && plan_dist_tiles(3, 2, 1, 0, false, 1000, 1000, 4).items == 0);
  CHECK(!plan_dist_tiles(3, 2, 1, 0, true, 0, 1000, 4).by_tile);
}

static const std::vector<std::pair<const char *, std::function<void()>>> cases = {
  {"row_window", row_window}, {"passes_per_wavefront", passes_per_wavefront}, {"tile_imbalance", tile_imbalance},
  {"stage", stage}, {"histogram", histogram}, {"sort_inside_fallback", sort_inside_fallback}, {"tail_regrouping", tail_regrouping},
  {"instance", instance}, {"tile_order", tile_order}, {"flavour", flavour}, {"sort_plan", sort_plan},
  {"sort_inside_or_before", sort_inside_or_before}, {"sort_due_rule", sort_due_rule}, {"early_sort", early},
  {"chunks", chunks}, {"spectrum_window", spectrum_window_rule}, {"distribution_path", distribution_path}, {"distribution_tiles", distribution_tiles},
};

int main(int argc, char **argv) {
  if (argc > 1 && !strcmp(argv[1], "--list")) { for (auto &c : cases) printf("%s\n", c.first); return 0; }
  int ran = 0;
  for (auto &c : cases) {
    bool want = argc == 1;
    for (int k = 1; k < argc; k++) want = want || !strcmp(argv[k], c.first);
    if (!want) continue;
    const int before = failures;
    current = c.first; c.second(); ran++;
    if (failures == before) printf("ok %s\n", c.first);
  }
  return failures || ran == 0 ? 1 : 0;
}
