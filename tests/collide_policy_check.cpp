// Where vpic_hip_collide collides a species and by which kernel instance (old-vpic_amd/csrc/policy.h: plan_collide,
// collide_ranges_exact) on the host: one case per rule.
// usage: collide_policy_check [case ...] (no case: all of them; --list: their names).  Prints "ok <case>" or "FAIL <case>: ..." lines.
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

constexpr int CAP = 1024;
// 13 440 particles sorted by voxel, partition[] valid; checked, the fullest cell holds 64
static CollideSpecies by_voxel() {
  CollideSpecies s;
  s.partition_valid = true; s.np = s.n_sorted = 13440; s.fullest = 64;
  return s;
}
// ... in tile order by cell, nothing appended, no dead slots
static CollideSpecies by_tile() {
  CollideSpecies s;
  s.tile_valid = true; s.np = s.n_sorted = 13440; s.fullest = 64;
  return s;
}
static bool in_place(const CollidePlan &pl, CollideInstance inst) { return !pl.sort_a && !pl.sort_b && !pl.over_cap && pl.instance == inst; }
static bool sorts_a_only(const CollidePlan &pl) { return pl.sort_a && !pl.sort_b && pl.instance == CollideInstance::none; }

static void exact_voxel_ranges_collide_in_place() {
  CHECK(in_place(plan_collide(by_voxel(), by_voxel(), true, CAP, false), CollideInstance::wave));
  CHECK(in_place(plan_collide(by_voxel(), by_voxel(), false, CAP, false), CollideInstance::wave));
  CollideSpecies before = by_voxel(); before.fullest = 0;                     // before the checking pass: no sort, nothing launched yet
  CHECK(in_place(plan_collide(before, before, true, CAP, false), CollideInstance::none));
  CollideSpecies junk; junk.np = 5;                                            // sp_a == sp_b: b is not looked at
  CHECK(in_place(plan_collide(by_voxel(), junk, true, CAP, false), CollideInstance::wave));
}
static void exact_tile_ranges_collide_in_place() {
  CHECK(in_place(plan_collide(by_tile(), by_tile(), true, CAP, false), CollideInstance::wave));
  CHECK(in_place(plan_collide(by_tile(), by_voxel(), false, CAP, false), CollideInstance::wave));    // the two species may be in different orders
  CHECK(in_place(plan_collide(by_voxel(), by_tile(), false, CAP, false), CollideInstance::wave));
  CollideSpecies empty;                                                        // a species that holds nothing has no range to be wrong
  CHECK(!plan_collide(by_tile(), empty, false, CAP, false).sort_b);
}
static void sorts_first_unsorted() {
  CollideSpecies s; s.np = 13440;
  CHECK(sorts_a_only(plan_collide(s, by_voxel(), true, CAP, false)));
  const CollidePlan pl = plan_collide(by_voxel(), s, false, CAP, false);
  CHECK(!pl.sort_a && pl.sort_b && pl.instance == CollideInstance::none);
  CollideSpecies pushed = by_voxel(); pushed.partition_valid = false;          // a push since the sort by voxel drops partition[]
  CHECK(sorts_a_only(plan_collide(pushed, pushed, true, CAP, false)));
}
static void sorts_first_tile_only() {
  CollideSpecies s = by_tile(); s.coarse_sorted = true;
  CHECK(sorts_a_only(plan_collide(s, s, true, CAP, false)));
  CHECK(sorts_a_only(plan_collide(s, by_tile(), false, CAP, false)));
}
static void sorts_first_tail() {
  CollideSpecies s = by_tile(); s.np = s.n_sorted + 1;
  CHECK(sorts_a_only(plan_collide(s, s, true, CAP, false)));
}
static void sorts_first_holes() {
  CollideSpecies s = by_tile(); s.n_holes = 1;
  CHECK(sorts_a_only(plan_collide(s, s, true, CAP, false)));
  s = by_voxel(); s.n_holes = 300;
  CHECK(sorts_a_only(plan_collide(s, s, true, CAP, false)));
}
static void sorts_first_failed_check() {
  CollideSpecies s = by_tile(); s.check_failed = true;                         // a push since the sort moved a particle out of its cell
  CHECK(sorts_a_only(plan_collide(s, s, true, CAP, false)));
  s = by_voxel(); s.check_failed = true;
  CHECK(sorts_a_only(plan_collide(s, s, true, CAP, false)));
  s.fullest = CAP + 1;                                                         // (a count taken from ranges that are not exact refuses nothing yet)
  CHECK(plan_collide(s, s, true, CAP, false).sort_a);
}
static void sorts_first_pending_fused_sort() {
  CollideSpecies s = by_tile(); s.fuse_pending = true;                         // tile_valid is set, the array is still to be sorted by the push
  CHECK(sorts_a_only(plan_collide(s, s, true, CAP, false)));
}
static void instance_by_fullest_cell() {
  CollideSpecies a = by_voxel(), b = by_tile();
  a.fullest = 64; b.fullest = 64; CHECK(in_place(plan_collide(a, b, false, CAP, false), CollideInstance::wave));
  a.fullest = 65; CHECK(in_place(plan_collide(a, b, false, CAP, false), CollideInstance::group));
  a.fullest = 3; b.fullest = 65; CHECK(in_place(plan_collide(a, b, false, CAP, false), CollideInstance::group));
  CHECK(in_place(plan_collide(a, b, true, CAP, false), CollideInstance::wave));                  // within a: b's cells do not count
  a.fullest = CAP; CHECK(in_place(plan_collide(a, a, true, CAP, false), CollideInstance::group));
  a.fullest = 2; CHECK(in_place(plan_collide(a, a, true, CAP, true), CollideInstance::group));   // VPIC_HIP_COLLIDE_INSTANCE=group
  a.fullest = 0; CHECK(in_place(plan_collide(a, a, true, CAP, true), CollideInstance::none));    // nothing to pair
}
static void over_the_cap_is_an_error() {
  CollideSpecies a = by_voxel(), b = by_tile();
  a.fullest = CAP + 1;
  CollidePlan pl = plan_collide(a, a, true, CAP, false);
  CHECK(pl.over_cap && pl.instance == CollideInstance::none && !pl.sort_a);
  a.fullest = 5; b.fullest = CAP + 1;
  pl = plan_collide(a, b, false, CAP, false);
  CHECK(pl.over_cap && pl.instance == CollideInstance::none);
  CHECK(!plan_collide(a, b, true, CAP, false).over_cap);
}

static const std::vector<std::pair<const char *, std::function<void()>>> cases = {
  {"exact_voxel_ranges_collide_in_place", exact_voxel_ranges_collide_in_place},
  {"exact_tile_ranges_collide_in_place", exact_tile_ranges_collide_in_place},
  {"sorts_first_unsorted", sorts_first_unsorted}, {"sorts_first_tile_only", sorts_first_tile_only},
  {"sorts_first_tail", sorts_first_tail}, {"sorts_first_holes", sorts_first_holes},
  {"sorts_first_failed_check", sorts_first_failed_check}, {"sorts_first_pending_fused_sort", sorts_first_pending_fused_sort},
  {"instance_by_fullest_cell", instance_by_fullest_cell}, {"over_the_cap_is_an_error", over_the_cap_is_an_error},
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
