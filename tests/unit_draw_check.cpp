// The interval of the particle sources' generator (old-vpic_amd/csrc/unit_draw.h) on the host: unit_open must lie strictly
// inside (0, 1) for every 32-bit input, or sqrtf(-logf(draw)) gives a refluxed or emitted particle a normal momentum of
// exactly zero.  unit_open reads only r >> 8, so all 2^24 values of it are every case there is; the ends of the 32-bit range
// and the low bits are walked besides.
// usage: unit_draw_check [case ...] (no case: all of them; --list: their names).  Prints "ok <case>" or "FAIL <case>: ..." lines.
//        unit_draw_check --mix32 x ... prints mix32 of each x (decimal), one per line, for a restatement to be held against.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <vector>
#include "unit_draw.h"

using namespace vpichip;

static int failures;
static const char *current;
#define CHECK(cond)                                                                           \
  do {                                                                                        \
    if (!(cond)) { printf("FAIL %s: line %d: %s\n", current, __LINE__, #cond); failures++; }   \
  } while (0)

// every value of r >> 8: inside (0, 1), never decreasing, and the draw of before the clamp wherever that was below 1
static void every_value_is_strictly_inside() {
  float before = 0.f;
  int reported = 0;
  for (uint32_t top = 0; top < (1u << 24); top++) {
    const float x = unit_open(top << 8);
    if (!(x > 0.f && x < 1.f) && reported++ < 4) {
      printf("FAIL %s: r >> 8 == %u gives %.9g\n", current, top, (double)x);
      failures++;
    }
    const float plain = ((float)top + 0.5f) * (1.f / 16777216.f);
    if (plain < 1.f) CHECK(x == plain);
    // the loader's map keeps the unclamped value: 1 at the top draw alone
    CHECK(unit_top_closed(top << 8) == plain && plain > 0.f && (plain == 1.f) == (top == (1u << 24) - 1u));
    CHECK(x >= before);
    before = x;
  }
  CHECK(unit_open(0u) == 0x1p-25f);                                   // the smallest: 0.5 * 2^-24
  CHECK(unit_open(0xffffff00u) == UNIT_OPEN_MAX && UNIT_OPEN_MAX == std::nextafterf(1.f, 0.f));
}

// the ends of the 32-bit range, and the eight low bits, which never matter
static void ends_of_the_range_and_the_low_bits() {
  const uint32_t ends[] = {0u, 1u, 0xffu, 0x100u, 0x7fffffffu, 0x80000000u, 0xfffffeffu, 0xffffff00u, 0xfffffffeu, 0xffffffffu};
  for (uint32_t r : ends) {
    const float x = unit_open(r);
    CHECK(x > 0.f && x < 1.f);
    for (uint32_t low = 0; low < 256u; low++) CHECK(unit_open((r & ~0xffu) | low) == x);
  }
  // what the sources make of the extreme draws: finite, and not zero at the top
  CHECK(std::sqrt(-std::log(unit_open(0xffffffffu))) > 0.f);
  CHECK(std::isfinite(std::sqrt(-std::log(unit_open(0u)))));
}

static const std::vector<std::pair<const char *, std::function<void()>>> cases = {
  {"every_value_is_strictly_inside", every_value_is_strictly_inside},
  {"ends_of_the_range_and_the_low_bits", ends_of_the_range_and_the_low_bits},
};

int main(int argc, char **argv) {
  if (argc > 1 && !strcmp(argv[1], "--list")) { for (auto &c : cases) printf("%s\n", c.first); return 0; }
  if (argc > 1 && !strcmp(argv[1], "--mix32")) {
    for (int k = 2; k < argc; k++) printf("%u\n", mix32((uint32_t)strtoul(argv[k], nullptr, 10)));
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
