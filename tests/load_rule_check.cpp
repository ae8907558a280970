// THE RULE of vpic_hip_species_load_profile (old-vpic_amd/csrc/load_rule.h) on the host, for tests/test_load_rule.py to hold
// == to the numpy restatement tests/load_ref.py.  Build: g++ -O2 -ffp-contract=off (every operation rounded once).
// usage: load_rule_check < slots.  A slot is one line of unsigned decimal words:
//   gx gy gz GX GY  cx cy cz nx ny  j seed stream flip  uth0 uth1 uth2 ud0 ud1 ud2 (float bits)  x0 x1 x2 n0 n1 n2 U (float bits)
// (g: the global cell's coordinates, c: the local cell's, from 0).  Per slot it prints one line:
//   cell voxel | generator mode: dx dy dz U (float bits) | draws mode: dx dy dz ux uy uz (float bits)
// The generator mode's normals go through the host's logf / cosf / sinf and are not printed: they are specified statistically.
// This is also the program to build with -fsanitize=address,undefined for a sanitizer run of the rule.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include "load_rule.h"

using namespace vpichip;

static uint32_t bits(float x) { uint32_t u; memcpy(&u, &x, 4); return u; }
static float from_bits(uint32_t u) { float x; memcpy(&x, &u, 4); return x; }

int main() {
  unsigned long long g[5], j;
  int c[5], flip;
  uint32_t seed, stream, tab[6], draw[7];
  int slots = 0;
  for (;;) {
    if (scanf("%llu %llu %llu %llu %llu %d %d %d %d %d %llu %" SCNu32 " %" SCNu32 " %d", &g[0], &g[1], &g[2], &g[3], &g[4],
              &c[0], &c[1], &c[2], &c[3], &c[4], &j, &seed, &stream, &flip) != 14) break;
    for (auto &t : tab) if (scanf("%" SCNu32, &t) != 1) return 2;
    for (auto &d : draw) if (scanf("%" SCNu32, &d) != 1) return 2;
    const uint64_t cell = load_global_cell(g[0], g[1], g[2], g[3], g[4]);
    const int sy = c[3] + 2, sz = sy * (c[4] + 2);
    uint32_t r[8];
    load_words(cell, (uint32_t)j, seed, stream, r);
    float gen[7];
    load_numbers(r, gen);
    printf("%" PRIu64 " %d | %u %u %u %u |", cell, load_voxel(c[0], c[1], c[2], sy, sz), bits(load_offset(gen[0])), bits(load_offset(gen[1])),
           bits(load_offset(gen[2])), bits(gen[6]));
    float uth[3], ud[3], n[3], u[3];
    for (int a = 0; a < 3; a++) { uth[a] = from_bits(tab[a]); ud[a] = from_bits(tab[3 + a]); n[a] = from_bits(draw[3 + a]); }
    load_momentum(uth, ud, n, from_bits(draw[6]), flip != 0, u);
    printf(" %u %u %u %u %u %u\n", bits(load_offset(from_bits(draw[0]))), bits(load_offset(from_bits(draw[1]))), bits(load_offset(from_bits(draw[2]))),
           bits(u[0]), bits(u[1]), bits(u[2]));
    slots++;
  }
  return slots ? 0 : 1;
}
