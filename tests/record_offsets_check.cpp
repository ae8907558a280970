// Where advance_p_kernel finds a particle (old-vpic_amd/csrc/record_offsets.h) on the host, at the limits: one case per rule.
// A position record is 16 bytes, so a byte offset from the start of the array wraps from 2^28 particles on; every
// workgroup addresses from a 64-bit base at its first particle instead.
// usage: record_offsets_check [case ...] (no case: all of them; --list: their names).  Prints "ok <case>" or "FAIL <case>: ..." lines.
#include <cstdio>
#include <cstring>
#include <functional>
#include <vector>
#include "record_offsets.h"

using namespace vpichip;

static int failures;
static const char *current;
#define CHECK(cond)                                                                           \
  do {                                                                                        \
    if (!(cond)) { printf("FAIL %s: line %d: %s\n", current, __LINE__, #cond); failures++; }   \
  } while (0)

// what the hardware adds up: a 64-bit scalar base and a 32-bit unsigned byte offset
static uint64_t reached(uint64_t base, uint32_t off) { return base + (uint64_t)off; }

// the last tile of a 2^30-particle launch: first = 2^30 - 4096, its last particle 2^30 - 1
static void tile_at_the_top_of_a_launch() {
  const int first = (1 << 30) - 4096, idx = (1 << 30) - 1;
  CHECK(record_offset(idx, first) == 4095u * 16u);
  CHECK(record_base_bytes(first) == ((uint64_t)first) * 16u && record_base_bytes(first) > 0xffffffffull);   // beyond any 32-bit offset
  CHECK(reached(record_base_bytes(first), record_offset(idx, first)) == (uint64_t)idx * 16u);
  CHECK(reached(word_base_bytes(first), word_offset(idx, first)) == (uint64_t)idx * 4u);
  CHECK((uint64_t)((uint32_t)idx << RECORD_SHIFT) != (uint64_t)idx * 16u);      // the offset from the array's start is what wraps
  // the same particle as a queued cell-crosser (the queue keeps the launch's idx) and as the first of the tile
  CHECK(record_offset(first, first) == 0u && word_offset(first, first) == 0u);
  CHECK(span_in_reach(first, (int64_t)idx + 1));
}

// the reference's order, a species of 2^31 - 8192 particles: launch segments on rebased arrays, workgroup `chunk` of a
// segment begins at chunk * per_chunk
static void reference_order_at_the_largest_species() {
  const int64_t max_np = ((int64_t)1 << 31) - 8192;
  const int iters_of[4] = {1, 3, 16, 64};
  for (int iters : iters_of) {
    const int64_t per_chunk = 256 * (int64_t)iters, seg = push_segment_particles(per_chunk);
    CHECK(seg > 0 && seg % per_chunk == 0 && (seg + PASS_LANES - 1) * 4 < ((int64_t)1 << 32));
    int n_seg = 0;
    for (int64_t at = 0; at < max_np; at += seg, n_seg++) {
      const int64_t c = max_np - at < seg ? max_np - at : seg;                  // the segment's particles: np of its launch
      const int64_t chunks = (c + per_chunk - 1) / per_chunk;
      const int64_t first64 = (chunks - 1) * per_chunk;                         // the last workgroup's first particle
      CHECK(first64 >= 0 && first64 < ((int64_t)1 << 31));                      // `first` is an int in the kernel
      const int first = (int)first64, last = (int)(c - 1);
      const uint64_t base = record_base_bytes(at) + record_base_bytes(first);   // the launch's rebased array, then the workgroup's base
      CHECK(reached(base, record_offset(last, first)) == (uint64_t)(at + last) * 16u);
      CHECK(reached(base, record_offset(first + (int)per_chunk - 1 + 0, first)) == (uint64_t)(at + first + per_chunk - 1) * 16u);   // a full chunk's last slot
      CHECK(record_offset(first + (int)per_chunk + PASS_LANES - 1, first) == (uint32_t)(per_chunk + PASS_LANES - 1) * 16u);         // no wrap anywhere near
      CHECK(span_in_reach(first, first + per_chunk));
      CHECK(load_slot(first + (int)per_chunk - 1, first, (int)c) == (last < first + per_chunk - 1 ? last : first + (int)per_chunk - 1) - first);
    }
    CHECK(n_seg == 2 || n_seg == 3);
  }
}

// lanes behind the last particle: they LOAD particle np - 1 and STORE into the padding behind it, from the same base
static void padding_lanes_behind_np() {
  const int first = (1 << 30) - 4096, np = (1 << 30) - 5;                       // the last pass holds 59 particles
  const int pass = first + ((np - 1 - first) / 64) * 64;
  for (int lane = 0; lane < 64; lane++) {
    const int idx = pass + lane;
    const int slot = load_slot(idx, first, np);
    CHECK(slot >= 0 && slot == (idx < np ? idx : np - 1) - first);
    CHECK(reached(record_base_bytes(first), (uint32_t)slot << RECORD_SHIFT) == (uint64_t)(idx < np ? idx : np - 1) * 16u);
    CHECK(reached(record_base_bytes(first), record_offset(idx, first)) == (uint64_t)idx * 16u);   // the store: slot idx itself
    CHECK(reached(word_base_bytes(first), word_offset(idx, first)) == (uint64_t)idx * 4u);
  }
  CHECK(load_slot(np + 62, first, np) == np - 1 - first);
  // a species of one particle, a workgroup that begins at it
  CHECK(load_slot(0, 0, 1) == 0 && load_slot(63, 0, 1) == 0 && record_offset(63, 0) == 63u * 16u);
}

// what one base reaches: 2^28 records, the lanes of a last pass included
static void reach_of_a_base() {
  CHECK(RECORD_REACH == ((int64_t)1 << 28));
  CHECK(span_in_reach(0, RECORD_REACH - PASS_LANES));
  CHECK(!span_in_reach(0, RECORD_REACH - PASS_LANES + 1));
  CHECK(span_in_reach(((int64_t)1 << 30) - 4096, (int64_t)1 << 30));
  const int first = 5, idx = first + (int)(RECORD_REACH - 1);                   // the last slot a base reaches
  CHECK(reached(record_base_bytes(first), record_offset(idx, first)) == (uint64_t)idx * 16u);
  CHECK(record_offset(idx, first) == 0xfffffff0u);
}

// the launch that sorts as it pushes: a destination anywhere in the second buffer
static void sort_destination_anywhere() {
  const uint64_t base = 0x7f0000000000ull;
  CHECK(record_address(base, 0u) == base);
  CHECK(record_address(base, (1u << 30) - 1u) == base + (((uint64_t)1 << 30) - 1) * 16u);
  CHECK(record_address(base, 1u << 28) == base + ((uint64_t)1 << 32));          // where a 32-bit offset would be back at 0
  CHECK(record_address(base, 0x7fffdfffu) == base + (uint64_t)0x7fffdfffu * 16u);   // 2^31 - 8192 - 1
}

static const std::vector<std::pair<const char *, std::function<void()>>> cases = {
  {"tile_at_the_top_of_a_launch", tile_at_the_top_of_a_launch},
  {"reference_order_at_the_largest_species", reference_order_at_the_largest_species},
  {"padding_lanes_behind_np", padding_lanes_behind_np},
  {"reach_of_a_base", reach_of_a_base},
  {"sort_destination_anywhere", sort_destination_anywhere},
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
