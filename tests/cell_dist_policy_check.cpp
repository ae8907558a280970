// The host decisions of the cell distributions (old-vpic_amd/csrc/policy.h): how many workgroups the pass over the interior
// cells launches (plan_cell_groups), and which path a descriptor without values takes (plan_distribution_sums with n_val 0,
// which the species' sums never ask for): one case per rule.
// usage: cell_dist_policy_check [case ...] (no case: all of them; --list: their names).  Prints "ok <case>" or
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

static const int LDS_WORDS = 8192, PER_GROUP = 256;

// a grid of a few cells launches one workgroup, and no grid launches a workgroup without a cell of its own
static void no_idle_workgroup() {
  CHECK(plan_cell_groups(6, PER_GROUP) == 1 && plan_cell_groups(1, PER_GROUP) == 1 && plan_cell_groups(256, PER_GROUP) == 1);
  CHECK(plan_cell_groups(257, PER_GROUP) == 2 && plan_cell_groups(76050, PER_GROUP) == 298);
  for (long long cells = 1; cells <= 600000; cells += 977) {
    const long long groups = plan_cell_groups(cells, PER_GROUP);
    CHECK(groups >= 1 && (groups - 1) * PER_GROUP < cells);
  }
}

// large grids stride: 2048 workgroups at the most, 256^3 cells in 32 rounds of each
static void capped() {
  CHECK(plan_cell_groups(2048ll * PER_GROUP, PER_GROUP) == 2048 && plan_cell_groups(2048ll * PER_GROUP + 1, PER_GROUP) == 2048);
  CHECK(plan_cell_groups(256ll * 256 * 256, PER_GROUP) == 2048 && 256ll * 256 * 256 / (2048 * PER_GROUP) == 32);
  CHECK(plan_cell_groups((1ll << 31) - 1, PER_GROUP) == 2048);
}

// a histogram alone (no values): 8192 bins are in LDS, 8193 are not
static void no_values() {
  const DistSumsPlan at = plan_distribution_sums(8192, 0, LDS_WORDS);
  CHECK(at.path == DIST_LDS && at.words == 8192);
  const DistSumsPlan beyond = plan_distribution_sums(8193, 0, LDS_WORDS);
  CHECK(beyond.path == DIST_GLOBAL && beyond.words == 0);
  CHECK(plan_distribution_sums(1, 0, LDS_WORDS).words == 1);
}

static const std::vector<std::pair<const char *, std::function<void()>>> cases = {
  {"no_idle_workgroup", no_idle_workgroup}, {"capped", capped}, {"no_values", no_values},
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
