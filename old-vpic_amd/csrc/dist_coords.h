// dist_coords.h -- the coordinates of a particle and the ranges over them (include/vpic_hip.h states the arithmetic:
// IEEE double, every operation rounded once, unfused), shared by the diagnostics that take a vpic_hip_dist_range_t --
// the histograms of distribution.hip and the selection of select.hip -- so that the two cannot drift apart.
#pragma once
#include "engine.h"
#include <math.h>

namespace vpichip {

// bit c of a `need` mask: coordinate c is used by an axis or a range
constexpr unsigned NEED_POS = 7u, NEED_KE = 3u << VPIC_HIP_COORD_KE;

struct DistCoords { double x, y, z, ux, uy, uz, ke, log_ke; };

// a select chain: the coordinate number is uniform, the values stay in registers
__device__ __forceinline__ double dist_coord(const DistCoords &v, int coord) {
  return coord == VPIC_HIP_COORD_X ? v.x : coord == VPIC_HIP_COORD_Y ? v.y : coord == VPIC_HIP_COORD_Z ? v.z
       : coord == VPIC_HIP_COORD_UX ? v.ux : coord == VPIC_HIP_COORD_UY ? v.uy : coord == VPIC_HIP_COORD_UZ ? v.uz
       : coord == VPIC_HIP_COORD_KE ? v.ke : v.log_ke;
}

__device__ __forceinline__ bool dist_in_range(const DistCoords &v, const vpic_hip_dist_range_t &r) {
  const double c = dist_coord(v, r.coord);
  return c >= r.lo && c < r.hi;
}

// lo <= c < hi for every one of the n_sel ranges (0 to 4; a NaN is in no range)
__device__ __forceinline__ bool dist_in_ranges(const DistCoords &v, const vpic_hip_dist_range_t (&sel)[4], int n_sel) {
  bool in = true;
  if (n_sel > 0) in = in && dist_in_range(v, sel[0]);
  if (n_sel > 1) in = in && dist_in_range(v, sel[1]);
  if (n_sel > 2) in = in && dist_in_range(v, sel[2]);
  if (n_sel > 3) in = in && dist_in_range(v, sel[3]);
  return in;
}

// what one lane reads of one particle (only the arrays the descriptor needs)
struct DistRaw { int voxel; float dx, dy, dz, ux, uy, uz; };

// The loads of a pass do not wait for one another (a dead slot's other words are read and not used), and the main loops
// ask for the next pass's before they work on this one's.
__device__ __forceinline__ DistRaw dist_load(const ParticlesK &p, long long idx, long long end, unsigned need) {
  DistRaw r{-1, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (idx < end) {
    r.voxel = p.i[idx];
    if (need & 1u) r.dx = p.dx[idx];
    if (need & 2u) r.dy = p.dy[idx];
    if (need & 4u) r.dz = p.dz[idx];
    if (need & (NEED_KE | 1u << VPIC_HIP_COORD_UX)) r.ux = p.ux[idx];
    if (need & (NEED_KE | 1u << VPIC_HIP_COORD_UY)) r.uy = p.uy[idx];
    if (need & (NEED_KE | 1u << VPIC_HIP_COORD_UZ)) r.uz = p.uz[idx];
  }
  return r;
}

// The coordinates that `need` names of a LIVE particle (0 <= r.voxel < nv); cx, cy, cz: the decoded voxel, ghost layer
// included (set when a position is needed, otherwise left alone).
__device__ __forceinline__ DistCoords dist_coords(const DistRaw &r, unsigned need, const TileK &t, int &cx, int &cy, int &cz) {
  DistCoords v{};
  if (need & NEED_POS) {
    voxel_cell(r.voxel, t, cx, cy, cz);
    if (need & 1u) v.x = (double)(cx - 1) + ((double)r.dx + 1.0) * 0.5;
    if (need & 2u) v.y = (double)(cy - 1) + ((double)r.dy + 1.0) * 0.5;
    if (need & 4u) v.z = (double)(cz - 1) + ((double)r.dz + 1.0) * 0.5;
  }
  v.ux = (double)r.ux; v.uy = (double)r.uy; v.uz = (double)r.uz;
  if (need & NEED_KE) {
    // as spectrum.hip: summed from the left
    v.ke = sqrt(((1.0 + v.ux * v.ux) + v.uy * v.uy) + v.uz * v.uz) - 1.0;
    if (need & 1u << VPIC_HIP_COORD_LOG10_KE) v.log_ke = log10(v.ke);
  }
  return v;
}

}  // namespace vpichip
