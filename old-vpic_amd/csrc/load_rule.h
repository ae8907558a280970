// load_rule.h -- THE RULE of vpic_hip_species_load_profile (include/vpic_hip.h states it word for word): the Philox-4x32-10
// block of a particle named by (global cell, number within the cell), the map from its eight words to a position and
// three normals, and the double arithmetic that turns a cell's thermal spread and drift into a momentum.  The arithmetic
// alone, so that it compiles on the host as well (tests/load_rule_check.cpp holds it == to tests/load_ref.py); every
// operation is rounded once, with the parentheses as written: build with -ffp-contract=off.
#pragma once
#include <math.h>
#include <stdint.h>
#include "unit_draw.h"

namespace vpichip {

constexpr uint32_t PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u, PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;

// Philox-4x32-10 (Salmon, Moraes, Dror, Shaw, SC'11): c[0..3] the counter in, the block out
VH_UNIT_HD void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
#if defined(__clang__)
#pragma unroll
#endif
  for (int round = 0; round < 10; round++) {
    if (round > 0) { k0 += PHILOX_W0; k1 += PHILOX_W1; }
    const uint64_t p0 = (uint64_t)PHILOX_M0 * c[0], p1 = (uint64_t)PHILOX_M1 * c[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
    c[0] = n0; c[1] = (uint32_t)p1; c[2] = n2; c[3] = (uint32_t)p0;
  }
}

// the global cell of a domain's local cell (from 0) and its voxel in the domain (ghost layer of one cell: interior from 1)
VH_UNIT_HD uint64_t load_global_cell(uint64_t gx, uint64_t gy, uint64_t gz, uint64_t GX, uint64_t GY) { return gx + GX * (gy + GY * gz); }
VH_UNIT_HD int load_voxel(int cx, int cy, int cz, int sy, int sz) { return (cx + 1) + sy * (cy + 1) + sz * (cz + 1); }

// the eight words of particle j of global cell c: block b = philox((lo32(c), hi32(c), j, b), (seed, stream))
VH_UNIT_HD void load_words(uint64_t cell, uint32_t j, uint32_t seed, uint32_t stream, uint32_t r[8]) {
#if defined(__clang__)
#pragma unroll
#endif
  for (int b = 0; b < 2; b++) {
    uint32_t c[4] = {(uint32_t)cell, (uint32_t)(cell >> 32), j, (uint32_t)b};
    philox4x32_10(c, seed, stream);
    r[4 * b] = c[0]; r[4 * b + 1] = c[1]; r[4 * b + 2] = c[2]; r[4 * b + 3] = c[3];
  }
}

// The seven numbers of a particle (x0, x1, x2, n0, n1, n2, U) from its words.  x_k and U are exact; the normals use the
// caller's own logf / cosf / sinf and are specified statistically.
VH_UNIT_HD void load_numbers(const uint32_t r[8], float d[7]) {
  d[0] = unit_open(r[0]); d[1] = unit_open(r[1]); d[2] = unit_open(r[2]);
  const float r1 = sqrtf(-2.f * logf(unit_open(r[3])));
  float s1, c1;
  sincosf(6.2831853f * unit_open(r[4]), &s1, &c1);            // (one argument reduction for the pair)
  d[3] = r1 * c1; d[4] = r1 * s1;
  d[5] = sqrtf(-2.f * logf(unit_open(r[5]))) * cosf(6.2831853f * unit_open(r[6]));
  d[6] = unit_open(r[7]);
}

// offset of a uniform draw in its cell, strictly inside (-1, 1)
VH_UNIT_HD float load_offset(float x) { return 2.f * x - 1.f; }

// The momentum: thermal part w_k = uth_k n_k in the drift's rest frame, boosted by the drift D = gamma_d beta_d; flip:
// Zenitani's flipping method (Phys. Plasmas 22, 042116, 2015) with the uniform draw U.
VH_UNIT_HD void load_momentum(const float uth[3], const float ud[3], const float n[3], float U, bool flip, float u[3]) {
  double w0 = (double)uth[0] * (double)n[0], w1 = (double)uth[1] * (double)n[1], w2 = (double)uth[2] * (double)n[2];
  const double gw = sqrt(1 + ((w0 * w0 + w1 * w1) + w2 * w2));
  const double D0 = (double)ud[0], D1 = (double)ud[1], D2 = (double)ud[2];
  const double DD = (D0 * D0 + D1 * D1) + D2 * D2;
  if (DD == 0) { u[0] = (float)w0; u[1] = (float)w1; u[2] = (float)w2; return; }
  const double gd = sqrt(1 + DD);
  double wD = (w0 * D0 + w1 * D1) + w2 * D2;
  if (flip && (-wD) / (gd * gw) > (double)U) {
    const double t = (2 * wD) / DD;
    w0 = w0 - t * D0; w1 = w1 - t * D1; w2 = w2 - t * D2;
    wD = -wD;
  }
  const double f = ((gd - 1) * wD) / DD + gw;
  u[0] = (float)(w0 + f * D0); u[1] = (float)(w1 + f * D1); u[2] = (float)(w2 + f * D2);
}

}  // namespace vpichip
