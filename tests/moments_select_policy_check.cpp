// How accumulate_hydro_p_select is dispatched (old-vpic_amd/csrc/policy.h: plan_moments_select) on the host: one case per
// rule.  The moments of a selection read the species and leave it as it is, so no plan sorts.
// usage: moments_select_policy_check [case ...] (no case: all of them; --list: their names).  Prints "ok <case>" or
// "FAIL <case>: ..." lines.
#include <cstdio>
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
static bool is(const MomentPlan &pl, MomentPath path) { return pl.path == path && !pl.sort_by_tile_first; }

// tile order, a partition, no movers: tile pass + tail pass, in either accumulation mode, whatever the size and the knobs of the
// untiled float paths
static void tile_valid_is_tiled() {
  for (bool det : {false, true}) {
    MomentInputs in = tile_ordered(); in.det = det;
    CHECK(is(plan_moments_select(in), MomentPath::tiled));
    in.per_particle_knob = true; CHECK(is(plan_moments_select(in), MomentPath::tiled));
    in.wants_tile = false; CHECK(is(plan_moments_select(in), MomentPath::tiled));
    in.np = 1; CHECK(is(plan_moments_select(in), MomentPath::tiled));
    in.np = 0; CHECK(is(plan_moments_select(in), MomentPath::tiled));
  }
}

// anything else -- no tile order, no usable partition, movers in flight, VPIC_HIP_MOMENTS_TILED=0 -- is the per-particle pass
static void anything_else_is_per_particle() {
  for (bool det : {false, true}) {
    MomentInputs in = tile_ordered(); in.det = det; in.tile_valid = false;
    CHECK(is(plan_moments_select(in), MomentPath::per_particle));
    in = tile_ordered(); in.det = det; in.tpart_ok = false;
    CHECK(is(plan_moments_select(in), MomentPath::per_particle));
    in = tile_ordered(); in.det = det; in.tile_valid = in.tpart_ok = false;
    CHECK(is(plan_moments_select(in), MomentPath::per_particle));
    in = tile_ordered(); in.det = det; in.nm = 1;
    CHECK(is(plan_moments_select(in), MomentPath::per_particle));
    in = tile_ordered(); in.det = det; in.tiled_knob = false;
    CHECK(is(plan_moments_select(in), MomentPath::per_particle));
  }
}

// every combination of the inputs: never a sort, never the by-cell route (which sorts by voxel) -- also where the whole-species
// plan would take one of them
static void never_a_sort() {
  int whole_species_sorts = 0;
  for (int bits = 0; bits < 128; bits++)
    for (int64_t np : {(int64_t)0, (int64_t)1, (int64_t)4 * 540 - 1, (int64_t)4 * 540, (int64_t)24 * 540})
      for (int64_t nm : {(int64_t)0, (int64_t)3}) {
        MomentInputs in;
        in.det = bits & 1; in.tile_valid = bits & 2; in.tpart_ok = bits & 4; in.wants_tile = bits & 8;
        in.per_particle_knob = bits & 16; in.tiled_knob = bits & 32; in.nv = bits & 64 ? 540 : 1;
        in.np = np; in.nm = nm;
        const MomentPlan pl = plan_moments_select(in);
        CHECK(!pl.sort_by_tile_first && pl.path != MomentPath::cells);
        CHECK((pl.path == MomentPath::tiled) == (in.tiled_knob && in.tile_valid && in.tpart_ok && nm == 0));
        const MomentPlan whole = plan_moments(in);
        whole_species_sorts += whole.sort_by_tile_first || whole.path == MomentPath::cells;
      }
  CHECK(whole_species_sorts > 0);            // (the sweep reaches inputs at which accumulate_hydro_p sorts)
}

static const std::vector<std::pair<const char *, std::function<void()>>> cases = {
  {"tile_valid_is_tiled", tile_valid_is_tiled}, {"anything_else_is_per_particle", anything_else_is_per_particle},
  {"never_a_sort", never_a_sort},
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
