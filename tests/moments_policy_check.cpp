// How accumulate_hydro_p / accumulate_rho_p are dispatched and scaled (old-vpic_amd/csrc/policy.h: plan_moments,
// moment_scales) on the host: one case per rule.
// usage: moments_policy_check [case ...] (no case: all of them; --list: their names; --scales q_max q_m r8V c: the base-2
// logarithms of the 14 fixed-point scales, one line).  Prints "ok <case>" or "FAIL <case>: ..." lines.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <vector>
#include "policy.h"

using namespace vpichip;

static int failures;
static const char *current;
#define CHECK(cond)                                                                           \
  do {                                                                                        \
    if (!(cond)) { printf("FAIL %s: line %d: %s\n", current, __LINE__, #cond); failures++; }   \
  } while (0)

// a species in tile order with a partition on record, nothing in flight, 24 particles per voxel
static MomentInputs tile_ordered() {
  MomentInputs in;
  in.tile_valid = in.tpart_ok = in.wants_tile = true;
  in.nv = 540; in.np = 24 * 540;
  return in;
}
static bool is(const MomentPlan &pl, MomentPath path, bool sort_first = false) { return pl.path == path && pl.sort_by_tile_first == sort_first; }

// tile order, a partition, no movers: by tile, in float and in deterministic mode, nothing is sorted
static void tile_order_sums_by_tile() {
  MomentInputs in = tile_ordered();
  CHECK(is(plan_moments(in), MomentPath::tiled));
  in.det = true; CHECK(is(plan_moments(in), MomentPath::tiled));
  in.per_particle_knob = true; CHECK(is(plan_moments(in), MomentPath::tiled));   // the knobs of the untiled float paths do not reach it
  in.np = 1; CHECK(is(plan_moments(in), MomentPath::tiled));                     // ... nor does the number of particles
  in.np = 0; CHECK(is(plan_moments(in), MomentPath::tiled));
}

// movers in flight, or no usable partition: not by tile
static void tile_order_needs_partition_and_no_movers() {
  MomentInputs in = tile_ordered();
  in.nm = 1; CHECK(is(plan_moments(in), MomentPath::per_particle));
  in.det = true; CHECK(is(plan_moments(in), MomentPath::per_particle));         // (and no sort while movers are in flight)
  in = tile_ordered(); in.tpart_ok = false; CHECK(is(plan_moments(in), MomentPath::cells));
  in.det = true; CHECK(is(plan_moments(in), MomentPath::tiled, true));            // deterministic: sorted by tile again
}

// deterministic, not in tile order, the engine would push it in tile order: sorted by tile first, then by tile
static void deterministic_sorts_by_tile_first() {
  MomentInputs in = tile_ordered(); in.det = true; in.tile_valid = in.tpart_ok = false;
  CHECK(is(plan_moments(in), MomentPath::tiled, true));
  in.np = 1; CHECK(is(plan_moments(in), MomentPath::tiled, true));
}

// deterministic, not in tile order, and the tile order is not the engine's choice (or movers, or nothing to sort): per particle
static void deterministic_falls_back_to_per_particle() {
  MomentInputs in = tile_ordered(); in.det = true; in.tile_valid = in.tpart_ok = false;
  in.wants_tile = false; CHECK(is(plan_moments(in), MomentPath::per_particle));
  in.wants_tile = true; in.nm = 3; CHECK(is(plan_moments(in), MomentPath::per_particle));
  in.nm = 0; in.np = 0; CHECK(is(plan_moments(in), MomentPath::per_particle));
}

// float mode, not in tile order: the path there was before -- by cell (sorted by voxel) from 4 particles per voxel on
static void float_untiled_is_the_old_path() {
  MomentInputs in = tile_ordered(); in.tile_valid = in.tpart_ok = false;
  CHECK(is(plan_moments(in), MomentPath::cells));
  in.wants_tile = false; CHECK(is(plan_moments(in), MomentPath::cells));
  in.np = 4 * in.nv; CHECK(is(plan_moments(in), MomentPath::cells));
  in.np = 4 * in.nv - 1; CHECK(is(plan_moments(in), MomentPath::per_particle));
  in.np = 24 * in.nv; in.nm = 1; CHECK(is(plan_moments(in), MomentPath::per_particle));
  in.nm = 0; in.per_particle_knob = true; CHECK(is(plan_moments(in), MomentPath::per_particle));   // VPIC_HIP_HYDRO_PER_PARTICLE / _RHO_
}

// VPIC_HIP_MOMENTS_TILED=0: deterministic per particle always, float as before there was a tile path
static void knob() {
  MomentInputs in = tile_ordered(); in.tiled_knob = false;
  CHECK(is(plan_moments(in), MomentPath::cells));
  in.np = 3 * in.nv; CHECK(is(plan_moments(in), MomentPath::per_particle));
  in.np = 24 * in.nv; in.per_particle_knob = true; CHECK(is(plan_moments(in), MomentPath::per_particle));
  in.per_particle_knob = false; in.det = true; CHECK(is(plan_moments(in), MomentPath::per_particle));
  in.tile_valid = in.tpart_ok = false; CHECK(is(plan_moments(in), MomentPath::per_particle));         // no sort either
}

// (q_max, q_m, r8V, c) of the GPU test's deck (tests/test_gpu_moments.py: unit cells, |q| up to 0.015, q_m = -1) and of
// BASELINE configs[3] (the reconnection deck at 256 x 256 x 128, 64 per cell: c = 1, q_m = +-1 at mi_me = 1, cubic cells of
// 1000 d_i / 256, a macro-particle of charge n0 dV / 64), and two far-off ones
struct Deck { double q_max, q_m, r8V, c; };
static std::vector<Deck> decks() {
  const double dV = pow(1000.0 / 256.0, 3);
  return {{0.015, -1.0, 0.125, 1.0}, {dV / 64.0, 1.0, 0.125 / dV, 1.0}, {dV / 64.0, -1.0, 0.125 / dV, 1.0},
          {3e-7, 1.0 / 1836.0, 4e3, 299792458.0}, {7e5, -40.0, 1e-9, 0.01}};
}
static bool momentum_scaled(int k) { return k >= 4; }       // px .. txy grow with |u|; jx jy jz rho do not

// every contribution of a particle with |u| <= 2^12 converts: |x scale| < 2^51
static void scales_convert() {
  for (const Deck &d : decks()) {
    const MomentScales ms = moment_scales(d.q_max, d.q_m, d.r8V, d.c);
    for (int k = 0; k < N_HYDRO_MOMENTS; k++) {
      CHECK(ms.bound[k] > 0 && ms.scale[k] == ldexp(1.0, ilogb(ms.scale[k])));             // one power of two
      CHECK(ms.bound[k] * (momentum_scaled(k) ? 4096.0 : 1.0) * ms.scale[k] < ldexp(1.0, 51));
    }
  }
}
// 2^20 particles of charge q_max at |u| <= 2^7 fit one 64-bit sum.  What such a particle adds is the table's bound, except
// to the off-diagonal stresses, where it is half of it at the most: |u_i u_j| / gamma <= (u_i^2 + u_j^2) / (2 gamma) < |u| / 2
// (sampled below over directions of u, so that the half is not taken on trust).
static void scales_sum() {
  for (const Deck &d : decks()) {
    const MomentScales ms = moment_scales(d.q_max, d.q_m, d.r8V, d.c);
    for (int k = 0; k < N_HYDRO_MOMENTS; k++) {
      CHECK(ms.part[k] == (k >= 11 ? 0.5 : 1.0));
      CHECK(ldexp(1.0, 20) * ms.bound[k] * ms.part[k] * (momentum_scaled(k) ? 128.0 : 1.0) * ms.scale[k] < ldexp(1.0, 63));
    }
  }
  for (int a = 0; a <= 64; a++)
    for (int b = 0; b <= 64; b++) {
      const double th = M_PI * a / 64.0, ph = 2.0 * M_PI * b / 64.0;
      for (double u : {1e-3, 1.0, 128.0, 4096.0}) {
        const double ux = u * sin(th) * cos(ph), uy = u * sin(th) * sin(ph), uz = u * cos(th), g = sqrt(1.0 + u * u);
        CHECK(fabs(uy * uz) / g < 0.5 * u && fabs(uz * ux) / g < 0.5 * u && fabs(ux * uy) / g < 0.5 * u);
      }
    }
}
// a unit contribution (weight W, |u| = 1) lands at 2^28 or higher
static void scales_resolve() {
  for (const Deck &d : decks()) {
    const MomentScales ms = moment_scales(d.q_max, d.q_m, d.r8V, d.c);
    for (int k = 0; k < N_HYDRO_MOMENTS; k++) CHECK(ms.bound[k] * ms.scale[k] >= ldexp(1.0, 28));
    // the bounds are the table's: W c, W, W |c / q_m|, W |c / q_m| c
    const double W = 8 * d.r8V * d.q_max, mc_q = fabs(d.c / d.q_m);
    CHECK(ms.bound[0] == W * d.c && ms.bound[2] == W * d.c && ms.bound[3] == W && ms.bound[4] == W * mc_q && ms.bound[6] == W * mc_q);
    CHECK(ms.bound[7] == W * mc_q * d.c && ms.bound[8] == W * mc_q * d.c && ms.bound[13] == W * mc_q * d.c);
  }
  // nothing to scale: a chargeless species, q_m = 0
  const MomentScales none = moment_scales(0, -1, 0.125, 1), massless = moment_scales(0.01, 0, 0.125, 1);
  for (int k = 0; k < N_HYDRO_MOMENTS; k++) CHECK(none.scale[k] == 1.0);
  CHECK(massless.scale[3] > 1.0 && massless.scale[4] == 1.0);
}

static const std::vector<std::pair<const char *, std::function<void()>>> cases = {
  {"tile_order_sums_by_tile", tile_order_sums_by_tile}, {"tile_order_needs_partition_and_no_movers", tile_order_needs_partition_and_no_movers},
  {"deterministic_sorts_by_tile_first", deterministic_sorts_by_tile_first},
  {"deterministic_falls_back_to_per_particle", deterministic_falls_back_to_per_particle},
  {"float_untiled_is_the_old_path", float_untiled_is_the_old_path}, {"knob", knob},
  {"scales_convert", scales_convert}, {"scales_sum", scales_sum}, {"scales_resolve", scales_resolve},
};

int main(int argc, char **argv) {
  if (argc > 1 && !strcmp(argv[1], "--list")) { for (auto &c : cases) printf("%s\n", c.first); return 0; }
  if (argc == 6 && !strcmp(argv[1], "--scales")) {
    const MomentScales ms = moment_scales(atof(argv[2]), atof(argv[3]), atof(argv[4]), atof(argv[5]));
    for (int k = 0; k < N_HYDRO_MOMENTS; k++) printf("%d%c", ilogb(ms.scale[k]), k + 1 < N_HYDRO_MOMENTS ? ' ' : '\n');
    return 0;
  }
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
