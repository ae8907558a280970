// cell_coords.h -- the coordinates of a CELL of the grid and the ranges over them (include/vpic_hip.h, VPIC_HIP_CELL_*, states
// the arithmetic: the centred fields in float by load_interpolator's expressions, everything derived in IEEE double, every
// operation rounded once, unfused), as dist_coords.h holds a particle's: one place for what cell_dist.hip loads, forms and
// looks up by code.
#pragma once
#include "engine.h"
#include <math.h>

namespace vpichip {

// bit (code - VPIC_HIP_CELL_X) of a 64-bit `need` mask: the code is used by an axis, a range or a factor, or by a code
// that is formed from it (cell_code_need)
constexpr unsigned long long cell_bit(int code) { return 1ull << (code - VPIC_HIP_CELL_X); }
constexpr unsigned long long CELL_NEED_POS = 7ull;
constexpr unsigned long long CELL_NEED_E = cell_bit(VPIC_HIP_CELL_EX_C) | cell_bit(VPIC_HIP_CELL_EY_C) | cell_bit(VPIC_HIP_CELL_EZ_C);
constexpr unsigned long long CELL_NEED_B = cell_bit(VPIC_HIP_CELL_BX_C) | cell_bit(VPIC_HIP_CELL_BY_C) | cell_bit(VPIC_HIP_CELL_BZ_C);
constexpr unsigned long long CELL_NEED_J = cell_bit(VPIC_HIP_CELL_JX_C) | cell_bit(VPIC_HIP_CELL_JY_C) | cell_bit(VPIC_HIP_CELL_JZ_C);
constexpr unsigned long long CELL_NEED_HYDRO = 0x3fffull << (VPIC_HIP_CELL_H0 - VPIC_HIP_CELL_X);
static_assert(VPIC_HIP_CELL_F0 - VPIC_HIP_CELL_X == 8 && VPIC_HIP_CELL_H0 - VPIC_HIP_CELL_X == 24 && VPIC_HIP_CELL_EX_C - VPIC_HIP_CELL_X == 40 &&
              VPIC_HIP_CELL_E_C - VPIC_HIP_CELL_X == 49 && VPIC_HIP_CELL_JDOTE_C - VPIC_HIP_CELL_X == 53 && VPIC_HIP_CELL_ONE - VPIC_HIP_CELL_X == 63 &&
              VPIC_HIP_CELL_F_RHOF == VPIC_HIP_CELL_F0 + F_RHOF && VPIC_HIP_CELL_H_TXY == VPIC_HIP_CELL_H0 + 13, "the cell codes fill one 64-bit mask");

// (host) a code an axis or a range may name; a factor may name ONE too
inline bool cell_known_coord(int c) {
  return (c >= VPIC_HIP_CELL_X && c <= VPIC_HIP_CELL_Z) || (c >= VPIC_HIP_CELL_F0 && c <= VPIC_HIP_CELL_H_TXY) ||
         (c >= VPIC_HIP_CELL_EX_C && c <= VPIC_HIP_CELL_JDOTE_C);
}
inline bool cell_known_factor(int c) { return cell_known_coord(c) || c == VPIC_HIP_CELL_ONE; }
// (host) the `need` bits of one known code: its own, and those of the centred fields a derived one is formed from
inline unsigned long long cell_code_need(int code) {
  unsigned long long need = cell_bit(code);
  if (code == VPIC_HIP_CELL_E_C) need |= CELL_NEED_E;
  if (code == VPIC_HIP_CELL_B_C) need |= CELL_NEED_B;
  if (code == VPIC_HIP_CELL_E_PAR_C) need |= CELL_NEED_E | CELL_NEED_B;
  if (code == VPIC_HIP_CELL_J_PAR_C) need |= CELL_NEED_J | CELL_NEED_B;
  if (code == VPIC_HIP_CELL_JDOTE_C) need |= CELL_NEED_J | CELL_NEED_E;
  return need;
}

// the interior cells in x-fastest order: cell index -> (cx, cy, cz) from 1, by magic_div of nx and nx * ny (a divisor of 1
// has no magic: the quotient is the dividend)
struct CellGridK {
  int nx, ny, nz, sy, sz;
  int cells;                                   // nx * ny * nz (below 2^31: nv is an int)
  int nxy;                                     // nx * ny
  unsigned mul_x, sh_x, mul_xy, sh_xy;
};
inline CellGridK make_cell_grid_k(const GridK &g) {
  CellGridK c{};
  c.nx = g.nx; c.ny = g.ny; c.nz = g.nz; c.sy = g.sy; c.sz = g.sz;
  c.nxy = g.nx * g.ny; c.cells = c.nxy * g.nz;
  if (c.nx > 1) magic_div((unsigned)c.nx, c.mul_x, c.sh_x);
  if (c.nxy > 1) magic_div((unsigned)c.nxy, c.mul_xy, c.sh_xy);
  return c;
}
__device__ __forceinline__ int cell_voxel(int idx, const CellGridK &c, int &cx, int &cy, int &cz) {
  const int z0 = c.nxy > 1 ? (int)(__umulhi((unsigned)idx, c.mul_xy) >> c.sh_xy) : idx;
  const int rem = idx - z0 * c.nxy;
  const int y0 = c.nx > 1 ? (int)(__umulhi((unsigned)rem, c.mul_x) >> c.sh_x) : rem;
  cx = rem - y0 * c.nx + 1; cy = y0 + 1; cz = z0 + 1;
  return cx + c.sy * cy + c.sz * cz;
}

// What one lane reads of one cell: only the words `need` names.  The loads do not wait for one another; nothing is used
// before all of them are asked for.
struct CellRaw {
  float f[F_NCOMP];                            // the raw words of the field record at v
  float h[16];                                 // ... of the hydro record (14 words and its padding)
  float e[3][4], j[3][4], b[3][2];             // w0 .. w3 of EX_C, EY_C, EZ_C; of JX_C ..; w0, w1 of BX_C ..
};

// w0 .. w3 of a centred E-like component `axis` (0 x, 1 y, 2 z) of array a at voxel v
__device__ __forceinline__ void cell_load4(const float *__restrict__ a, int v, int axis, const CellGridK &c, float (&w)[4]) {
  // ex: v, v+sy, v+sz, v+sy+sz;  ey: v, v+sz, v+1, v+sz+1;  ez: v, v+1, v+sy, v+1+sy
  const int s1 = axis == 0 ? c.sy : axis == 1 ? c.sz : 1, s2 = axis == 0 ? c.sz : axis == 1 ? 1 : c.sy;
  w[0] = a[v]; w[1] = a[v + s1]; w[2] = a[v + s2]; w[3] = a[v + s1 + s2];
}

// v: an INTERIOR voxel (every neighbour read is at most in the high ghost layer)
__device__ __forceinline__ CellRaw cell_load(const FieldsK &f, const float *__restrict__ hydro, int v, const CellGridK &c, unsigned long long need) {
  CellRaw r{};
#pragma unroll
  for (int w = 0; w < F_NCOMP; w++)
    if (need & cell_bit(VPIC_HIP_CELL_F0 + w)) r.f[w] = f.c[w][v];
#pragma unroll
  for (int a = 0; a < 3; a++) {
    if (need & cell_bit(VPIC_HIP_CELL_EX_C + a)) cell_load4(f.c[F_EX + a], v, a, c, r.e[a]);
    if (need & cell_bit(VPIC_HIP_CELL_JX_C + a)) cell_load4(f.c[F_JFX + a], v, a, c, r.j[a]);
    if (need & cell_bit(VPIC_HIP_CELL_BX_C + a)) {
      const float *cb = f.c[F_CBX + a];
      r.b[a][0] = cb[v]; r.b[a][1] = cb[v + (a == 0 ? 1 : a == 1 ? c.sy : c.sz)];
    }
  }
  if (need & CELL_NEED_HYDRO) {                // a 64-byte record: four float4, those that hold a named word
    const float4 *q = reinterpret_cast<const float4 *>(hydro) + 4 * (size_t)v;
#pragma unroll
    for (int k = 0; k < 4; k++)
      if (need & (0xfull << (VPIC_HIP_CELL_H0 - VPIC_HIP_CELL_X + 4 * k)) & CELL_NEED_HYDRO) {
        const float4 t = q[k];
        r.h[4 * k] = t.x; r.h[4 * k + 1] = t.y; r.h[4 * k + 2] = t.z; r.h[4 * k + 3] = t.w;
      }
  }
  return r;
}
static_assert(sizeof(vpic_hydro_t) == 64, "a hydro record is four float4");

// (Scalars, not arrays: a select chain over the elements of an array is turned back into an indexed read of it, and an
// array that is indexed by a register lives in scratch memory.)
struct CellCoords {
  double x, y, z;
  float f0, f1, f2, f3, f4, f5, f6, f7, f8, f9, f10, f11, f12, f13, f14, f15;   // the raw words of the field record
  float h0, h1, h2, h3, h4, h5, h6, h7, h8, h9, h10, h11, h12, h13;            // ... of the hydro record
  float c0, c1, c2, c3, c4, c5, c6, c7, c8;                                      // EX_C .. JZ_C in float
  double e, b, e_par, j_par, jdote;
};

__device__ __forceinline__ float cell_centre4(const float (&w)[4]) { return 0.25f * ((w[3] + w[0]) + (w[1] + w[2])); }

// the coordinates `need` names of interior cell (cx, cy, cz)
__device__ __forceinline__ CellCoords cell_coords(const CellRaw &r, int cx, int cy, int cz, unsigned long long need) {
  CellCoords v{};
  if (need & CELL_NEED_POS) {
    v.x = (double)(cx - 1) + 0.5; v.y = (double)(cy - 1) + 0.5; v.z = (double)(cz - 1) + 0.5;
  }
  v.f0 = r.f[0]; v.f1 = r.f[1]; v.f2 = r.f[2]; v.f3 = r.f[3]; v.f4 = r.f[4]; v.f5 = r.f[5]; v.f6 = r.f[6]; v.f7 = r.f[7];
  v.f8 = r.f[8]; v.f9 = r.f[9]; v.f10 = r.f[10]; v.f11 = r.f[11]; v.f12 = r.f[12]; v.f13 = r.f[13]; v.f14 = r.f[14]; v.f15 = r.f[15];
  v.h0 = r.h[0]; v.h1 = r.h[1]; v.h2 = r.h[2]; v.h3 = r.h[3]; v.h4 = r.h[4]; v.h5 = r.h[5]; v.h6 = r.h[6]; v.h7 = r.h[7];
  v.h8 = r.h[8]; v.h9 = r.h[9]; v.h10 = r.h[10]; v.h11 = r.h[11]; v.h12 = r.h[12]; v.h13 = r.h[13];
  v.c0 = cell_centre4(r.e[0]); v.c1 = cell_centre4(r.e[1]); v.c2 = cell_centre4(r.e[2]);
  v.c3 = 0.5f * (r.b[0][1] + r.b[0][0]); v.c4 = 0.5f * (r.b[1][1] + r.b[1][0]); v.c5 = 0.5f * (r.b[2][1] + r.b[2][0]);
  v.c6 = cell_centre4(r.j[0]); v.c7 = cell_centre4(r.j[1]); v.c8 = cell_centre4(r.j[2]);
  const double ex = (double)v.c0, ey = (double)v.c1, ez = (double)v.c2, bx = (double)v.c3, by = (double)v.c4, bz = (double)v.c5;
  const double jx = (double)v.c6, jy = (double)v.c7, jz = (double)v.c8;
  if (need & cell_bit(VPIC_HIP_CELL_E_C)) v.e = sqrt((ex * ex + ey * ey) + ez * ez);
  if (need & (cell_bit(VPIC_HIP_CELL_B_C) | cell_bit(VPIC_HIP_CELL_E_PAR_C) | cell_bit(VPIC_HIP_CELL_J_PAR_C))) {
    const double b = sqrt((bx * bx + by * by) + bz * bz);                    // no special case: B == 0 gives what the quotients give
    v.b = b;
    if (need & cell_bit(VPIC_HIP_CELL_E_PAR_C)) v.e_par = ((ex * bx + ey * by) + ez * bz) / b;
    if (need & cell_bit(VPIC_HIP_CELL_J_PAR_C)) v.j_par = ((jx * bx + jy * by) + jz * bz) / b;
  }
  if (need & cell_bit(VPIC_HIP_CELL_JDOTE_C)) v.jdote = (jx * ex + jy * ey) + jz * ez;
  return v;
}

// one link of a select chain, by value: the condition is uniform, the values stay in registers
__device__ __forceinline__ float cell_sel(bool take, float a, float otherwise) { return take ? a : otherwise; }
__device__ __forceinline__ double cell_sel(bool take, double a, double otherwise) { return take ? a : otherwise; }

// a coordinate or a factor of a checked descriptor by its code (uniform: a select chain within the code's group, as
// dist_coord's over a particle's)
__device__ __forceinline__ double cell_coord(const CellCoords &v, int code) {
  const int k = code - VPIC_HIP_CELL_X;
  if (k < VPIC_HIP_CELL_F0 - VPIC_HIP_CELL_X) return cell_sel(k == 0, v.x, cell_sel(k == 1, v.y, v.z));
  if (k < VPIC_HIP_CELL_H0 - VPIC_HIP_CELL_X) {
    const int w = k - (VPIC_HIP_CELL_F0 - VPIC_HIP_CELL_X);
    float r = v.f0;
    r = cell_sel(w == 1, v.f1, r); r = cell_sel(w == 2, v.f2, r); r = cell_sel(w == 3, v.f3, r); r = cell_sel(w == 4, v.f4, r);
    r = cell_sel(w == 5, v.f5, r); r = cell_sel(w == 6, v.f6, r); r = cell_sel(w == 7, v.f7, r); r = cell_sel(w == 8, v.f8, r);
    r = cell_sel(w == 9, v.f9, r); r = cell_sel(w == 10, v.f10, r); r = cell_sel(w == 11, v.f11, r); r = cell_sel(w == 12, v.f12, r);
    r = cell_sel(w == 13, v.f13, r); r = cell_sel(w == 14, v.f14, r); r = cell_sel(w == 15, v.f15, r);
    return (double)r;
  }
  if (k < VPIC_HIP_CELL_EX_C - VPIC_HIP_CELL_X) {
    const int w = k - (VPIC_HIP_CELL_H0 - VPIC_HIP_CELL_X);
    float r = v.h0;
    r = cell_sel(w == 1, v.h1, r); r = cell_sel(w == 2, v.h2, r); r = cell_sel(w == 3, v.h3, r); r = cell_sel(w == 4, v.h4, r);
    r = cell_sel(w == 5, v.h5, r); r = cell_sel(w == 6, v.h6, r); r = cell_sel(w == 7, v.h7, r); r = cell_sel(w == 8, v.h8, r);
    r = cell_sel(w == 9, v.h9, r); r = cell_sel(w == 10, v.h10, r); r = cell_sel(w == 11, v.h11, r); r = cell_sel(w == 12, v.h12, r);
    r = cell_sel(w == 13, v.h13, r);
    return (double)r;
  }
  if (k < VPIC_HIP_CELL_E_C - VPIC_HIP_CELL_X) {
    const int w = k - (VPIC_HIP_CELL_EX_C - VPIC_HIP_CELL_X);
    float r = v.c0;
    r = cell_sel(w == 1, v.c1, r); r = cell_sel(w == 2, v.c2, r); r = cell_sel(w == 3, v.c3, r); r = cell_sel(w == 4, v.c4, r);
    r = cell_sel(w == 5, v.c5, r); r = cell_sel(w == 6, v.c6, r); r = cell_sel(w == 7, v.c7, r); r = cell_sel(w == 8, v.c8, r);
    return (double)r;
  }
  return cell_sel(code == VPIC_HIP_CELL_E_C, v.e, cell_sel(code == VPIC_HIP_CELL_B_C, v.b, cell_sel(code == VPIC_HIP_CELL_E_PAR_C, v.e_par,
         cell_sel(code == VPIC_HIP_CELL_J_PAR_C, v.j_par, cell_sel(code == VPIC_HIP_CELL_JDOTE_C, v.jdote, 1.0)))));   // (ONE)
}

__device__ __forceinline__ bool cell_in_range(const CellCoords &v, const vpic_hip_dist_range_t &r) {
  const double c = cell_coord(v, r.coord);
  return c >= r.lo && c < r.hi;
}

// lo <= c < hi for every one of the n_sel ranges (0 to 4; a NaN is in no range)
__device__ __forceinline__ bool cell_in_ranges(const CellCoords &v, const vpic_hip_dist_range_t (&sel)[4], int n_sel) {
  bool in = true;
  if (n_sel > 0) in = in && cell_in_range(v, sel[0]);
  if (n_sel > 1) in = in && cell_in_range(v, sel[1]);
  if (n_sel > 2) in = in && cell_in_range(v, sel[2]);
  if (n_sel > 3) in = in && cell_in_range(v, sel[3]);
  return in;
}

}  // namespace vpichip
