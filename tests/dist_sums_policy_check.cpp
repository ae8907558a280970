// Which path the per-bin sums of a histogram take (old-vpic_amd/csrc/policy.h: plan_distribution_sums) on the host: one case
// per rule.  A bin holds a 32-bit count and n_val 64-bit sums, 1 + 2 n_val LDS words; the whole histogram stays in LDS while
// that fits VPIC_HIP_DIST_LDS_BINS = 8192 words, everything larger adds in global memory.
// usage: dist_sums_policy_check [case ...] (no case: all of them; --list: their names).  Prints "ok <case>" or
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

static const int LDS_WORDS = 8192;

// n_val from 1 to 4: the last bin count in LDS and the first beyond it, by the word count
static void boundary_per_value_count() {
  const long long last[5] = {0, 2730, 1638, 1170, 910};    // floor(8192 / (1 + 2 n_val))
  for (int n_val = 1; n_val <= 4; n_val++) {
    const long long per_bin = 1 + 2 * n_val;
    CHECK(last[n_val] == LDS_WORDS / per_bin);
    const DistSumsPlan in = plan_distribution_sums(last[n_val], n_val, LDS_WORDS);
    CHECK(in.path == DIST_LDS && in.words == last[n_val] * per_bin && in.words <= LDS_WORDS);
    const DistSumsPlan out = plan_distribution_sums(last[n_val] + 1, n_val, LDS_WORDS);
    CHECK(out.path == DIST_GLOBAL && out.words == 0);
  }
}

// the boundary word count itself: 8192 words are in (one value does not divide it; a budget that it does divide shows the <=)
static void boundary_word_count() {
  const DistSumsPlan at = plan_distribution_sums(2048, 1, 3 * 2048);
  CHECK(at.path == DIST_LDS && at.words == 3 * 2048);
  CHECK(plan_distribution_sums(2049, 1, 3 * 2048).path == DIST_GLOBAL);
  CHECK(plan_distribution_sums(1024, 4, 9 * 1024).path == DIST_LDS);
  CHECK(plan_distribution_sums(1024, 4, 9 * 1024 - 1).path == DIST_GLOBAL);
}

// the LDS path never takes more bytes than the counts of the histogram's own LDS path do (32 KB), whatever the shape
static void lds_never_above_budget() {
  for (int n_val = 1; n_val <= 4; n_val++)
    for (long long bins = 1; bins <= 9000; bins++) {
      const DistSumsPlan pl = plan_distribution_sums(bins, n_val, LDS_WORDS);
      CHECK((pl.path == DIST_LDS) == (bins * (1 + 2 * n_val) <= LDS_WORDS));
      CHECK(pl.path != DIST_WINDOW);
      if (pl.path == DIST_LDS) CHECK(4 * pl.words <= 32768 && pl.words == bins * (1 + 2 * n_val));
    }
}

// the cap of the histogram, 2^22 bins, with four values: global
static void largest_histogram() {
  const DistSumsPlan pl = plan_distribution_sums(1ll << 22, 4, LDS_WORDS);
  CHECK(pl.path == DIST_GLOBAL && pl.words == 0);
}

static const std::vector<std::pair<const char *, std::function<void()>>> cases = {
  {"boundary_per_value_count", boundary_per_value_count}, {"boundary_word_count", boundary_word_count},
  {"lds_never_above_budget", lds_never_above_budget}, {"largest_histogram", largest_histogram},
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
