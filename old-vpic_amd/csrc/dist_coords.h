// dist_coords.h -- the coordinates of a particle and the ranges over them (include/vpic_hip.h states the arithmetic:
// IEEE double, every operation rounded once, unfused), shared by the diagnostics that take a vpic_hip_dist_range_t --
// the histograms of distribution.hip, the selection of select.hip and the selected moments of moments.hip -- so that they
// cannot drift apart.
#pragma once
#include "engine.h"
#include <math.h>

namespace vpichip {

// bit c of a `need` mask: coordinate c is used by an axis or a range
constexpr unsigned NEED_POS = 7u, NEED_KE = 3u << VPIC_HIP_COORD_KE;
// The coordinates in the frame of the local magnetic field (U_PAR .. E_PAR).  Every one of them needs B at the particle,
// and with it the three offsets (not the voxel's decode: that stays with X, Y, Z); E_PAR alone needs E; all but B and
// E_PAR need the momenta.  They run in kernel instances of their own (FIELDS): a descriptor without them runs the code
// it always ran.
constexpr unsigned NEED_FIELD = 0x3fu << VPIC_HIP_COORD_U_PAR, NEED_FIELD_E = 1u << VPIC_HIP_COORD_E_PAR;
constexpr unsigned NEED_FIELD_U = NEED_FIELD & ~(1u << VPIC_HIP_COORD_B | NEED_FIELD_E);
constexpr unsigned NEED_FIELD_PERP = 1u << VPIC_HIP_COORD_U_PERP | 1u << VPIC_HIP_COORD_MU;
static_assert(VPIC_HIP_COORD_U_PAR == 16 && VPIC_HIP_COORD_E_PAR == 21 && NEED_FIELD == 0x3f0000u, "the field coordinates are bits 16 to 21");

struct DistCoords { double x, y, z, ux, uy, uz, ke, log_ke, u_par, u_perp, pitch, mu, b, e_par; };

// a select chain: the coordinate number is uniform, the values stay in registers
template <bool FIELDS>
__device__ __forceinline__ double dist_coord(const DistCoords &v, int coord) {
  if (FIELDS) {
    if (coord >= VPIC_HIP_COORD_U_PAR)
      return coord == VPIC_HIP_COORD_U_PAR ? v.u_par : coord == VPIC_HIP_COORD_U_PERP ? v.u_perp : coord == VPIC_HIP_COORD_PITCH ? v.pitch
           : coord == VPIC_HIP_COORD_MU ? v.mu : coord == VPIC_HIP_COORD_B ? v.b : v.e_par;
  }
  return coord == VPIC_HIP_COORD_X ? v.x : coord == VPIC_HIP_COORD_Y ? v.y : coord == VPIC_HIP_COORD_Z ? v.z
       : coord == VPIC_HIP_COORD_UX ? v.ux : coord == VPIC_HIP_COORD_UY ? v.uy : coord == VPIC_HIP_COORD_UZ ? v.uz
       : coord == VPIC_HIP_COORD_KE ? v.ke : v.log_ke;
}

template <bool FIELDS>
__device__ __forceinline__ bool dist_in_range(const DistCoords &v, const vpic_hip_dist_range_t &r) {
  const double c = dist_coord<FIELDS>(v, r.coord);
  return c >= r.lo && c < r.hi;
}

// lo <= c < hi for every one of the n_sel ranges (0 to 4; a NaN is in no range)
template <bool FIELDS>
__device__ __forceinline__ bool dist_in_ranges(const DistCoords &v, const vpic_hip_dist_range_t (&sel)[4], int n_sel) {
  bool in = true;
  if (n_sel > 0) in = in && dist_in_range<FIELDS>(v, sel[0]);
  if (n_sel > 1) in = in && dist_in_range<FIELDS>(v, sel[1]);
  if (n_sel > 2) in = in && dist_in_range<FIELDS>(v, sel[2]);
  if (n_sel > 3) in = in && dist_in_range<FIELDS>(v, sel[3]);
  return in;
}

// what one lane reads of one particle (only the arrays the descriptor needs)
struct DistRaw { int voxel; float dx, dy, dz, ux, uy, uz; };

// The loads of a pass do not wait for one another (a dead slot's other words are read and not used), and the main loops
// ask for the next pass's before they work on this one's.
template <bool FIELDS>
__device__ __forceinline__ DistRaw dist_load(const ParticlesK &p, long long idx, long long end, unsigned need) {
  DistRaw r{-1, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const bool u = FIELDS && (need & NEED_FIELD_U);
  if (idx < end) {
    const float4 rec = p.r[idx];                          // (position and cell are one 16-byte record: engine.h)
    r.voxel = record_cell(rec); r.dx = rec.x; r.dy = rec.y; r.dz = rec.z;
    if (u || (need & (NEED_KE | 1u << VPIC_HIP_COORD_UX))) r.ux = p.ux[idx];
    if (u || (need & (NEED_KE | 1u << VPIC_HIP_COORD_UY))) r.uy = p.uy[idx];
    if (u || (need & (NEED_KE | 1u << VPIC_HIP_COORD_UZ))) r.uz = p.uz[idx];
  }
  return r;
}

// What a FIELDS instance reads of the interpolator record of the particle's voxel: the 24 bytes of B always, the 48 of
// E only when E_PAR is named.
struct DistField { float4 b; float2 c; float4 ex, ey, ez; };   // {cbx, dcbxdx, cby, dcbydy}, {cbz, dcbzdz}, {ex, dexdy, dexdz, d2exdydz}, ...

// The gather of one pass.  Only a live lane (0 <= voxel < nv) forms an address: a dead slot, a lane behind the end of
// its chunk (voxel -1) and i >= nv read nothing.  The main loops issue it one pass ahead, as soon as that pass's
// voxels have arrived and before the arithmetic of the pass in hand.
__device__ __forceinline__ DistField dist_gather(const vpic_interpolator_t *__restrict__ fi, int voxel, int nv, unsigned need) {
  DistField f{};
  if (voxel >= 0 && voxel < nv) {
    const float4 *q = reinterpret_cast<const float4 *>(fi + voxel);
    f.b = q[3];
    f.c = *reinterpret_cast<const float2 *>(q + 4);
    if (need & NEED_FIELD_E) { f.ex = q[0]; f.ey = q[1]; f.ez = q[2]; }
  }
  return f;
}
static_assert(sizeof(vpic_interpolator_t) == 80, "an interpolator record is five float4");

// THE FIELDS AT THE PARTICLE as select_write_kernel forms them (advance_p.cxx:74-82 without qdt_2mc: float, every operation
// rounded once, unfused), of a gathered record: the one statement behind the field coordinates, the factors and cool.hip
// (select_write_kernel keeps its own, over the words it loads itself)
__device__ __forceinline__ float3 dist_b_at(const DistRaw &r, const DistField &f) {
  return make_float3(f.b.x + r.dx * f.b.y, f.b.z + r.dy * f.b.w, f.c.x + r.dz * f.c.y);
}
__device__ __forceinline__ float3 dist_e_at(const DistRaw &r, const DistField &f) {
  return make_float3((f.ex.x + r.dy * f.ex.y) + r.dz * (f.ex.z + r.dy * f.ex.w),
                     (f.ey.x + r.dz * f.ey.y) + r.dx * (f.ey.z + r.dz * f.ey.w),
                     (f.ez.x + r.dx * f.ez.y) + r.dy * (f.ez.z + r.dx * f.ez.w));
}

// The coordinates that `need` names of a LIVE particle (0 <= r.voxel < nv); cx, cy, cz: the decoded voxel, ghost layer
// included (set when a position is needed, otherwise left alone).  f: its voxel's record (FIELDS instances only).
template <bool FIELDS>
__device__ __forceinline__ DistCoords dist_coords(const DistRaw &r, const DistField &f, unsigned need, const TileK &t, int &cx, int &cy, int &cz) {
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
  if (FIELDS) {
    // the fields at the particle as select_write_kernel forms them (float, unfused), then double, summed from the left;
    // no special case: B == 0 and u == 0 give what the quotients give
    const float3 cb = dist_b_at(r, f);
    const double bx = (double)cb.x, by = (double)cb.y, bz = (double)cb.z;
    const double b = sqrt((bx * bx + by * by) + bz * bz);
    v.b = b;
    if (need & NEED_FIELD_U) {
      const double u_par = ((v.ux * bx + v.uy * by) + v.uz * bz) / b;
      const double u2 = (v.ux * v.ux + v.uy * v.uy) + v.uz * v.uz;
      v.u_par = u_par;
      if (need & NEED_FIELD_PERP) {
        const double perp2 = u2 - u_par * u_par;
        const double p2 = perp2 < 0.0 ? 0.0 : perp2;                            // (a NaN stays a NaN)
        if (need & 1u << VPIC_HIP_COORD_U_PERP) v.u_perp = sqrt(p2);
        if (need & 1u << VPIC_HIP_COORD_MU) v.mu = p2 / (2.0 * b);
      }
      if (need & 1u << VPIC_HIP_COORD_PITCH) v.pitch = u_par / sqrt(u2);
    }
    if (need & NEED_FIELD_E) {
      const float3 el = dist_e_at(r, f);
      v.e_par = (((double)el.x * bx + (double)el.y * by) + (double)el.z * bz) / b;
    }
  }
  return v;
}

// ---- the factors of a per-bin sum beyond the coordinates (vpic_hip_species_distribution_sums: VPIC_HIP_FACTOR_*) ----
// bits of a `vneed` mask: which of them a value names.  What they share with the coordinates they ask for through `need`
// (dist_factor_need): the momenta through KE's bit, the whole record and E_PAR, U_PAR through those coordinates' bits, so
// that dist_load, dist_gather and dist_coords serve them as they are; EDOTV and EPAR_VPAR therefore run in FIELDS instances.
constexpr unsigned VAL_Q = 1u, VAL_EDOTV = 2u, VAL_EPAR_VPAR = 4u;
// (host) the `need` and `vneed` bits of one factor code of a checked value
inline void dist_factor_need(int code, unsigned &need, unsigned &vneed) {
  if (code < VPIC_HIP_FACTOR_ONE) { need |= 1u << code; return; }
  if (code == VPIC_HIP_FACTOR_Q) vneed |= VAL_Q;
  if (code == VPIC_HIP_FACTOR_EDOTV) { vneed |= VAL_EDOTV; need |= 1u << VPIC_HIP_COORD_KE | NEED_FIELD_E; }
  if (code == VPIC_HIP_FACTOR_EPAR_VPAR) { vneed |= VAL_EPAR_VPAR; need |= 1u << VPIC_HIP_COORD_KE | NEED_FIELD_E | 1u << VPIC_HIP_COORD_U_PAR; }
}

struct DistExtra { double q, edotv, epar_vpar; };

// the q of one pass, read only when a value names it
__device__ __forceinline__ float dist_load_q(const ParticlesK &p, long long idx, long long end, unsigned vneed) {
  return (vneed & VAL_Q) && idx < end ? p.q[idx] : 0.f;
}

// Of a LIVE particle whose coordinates v dist_coords has formed under dist_factor_need's bits.  E at the particle is
// formed again by dist_e_at (the same float operations give the same floats).
template <bool FIELDS>
__device__ __forceinline__ DistExtra dist_extra(const DistRaw &r, const DistField &f, float q, const DistCoords &v, unsigned vneed) {
  DistExtra x{};
  x.q = (double)q;
  if (FIELDS && (vneed & (VAL_EDOTV | VAL_EPAR_VPAR))) {
    const double gamma = sqrt(((1.0 + v.ux * v.ux) + v.uy * v.uy) + v.uz * v.uz);   // KE's expression before the - 1
    if (vneed & VAL_EDOTV) {
      const float3 el = dist_e_at(r, f);
      x.edotv = (((double)el.x * v.ux + (double)el.y * v.uy) + (double)el.z * v.uz) / gamma;
    }
    if (vneed & VAL_EPAR_VPAR) x.epar_vpar = (v.e_par * v.u_par) / gamma;
  }
  return x;
}

// a select chain over the factor codes, as dist_coord over the coordinates (the code is uniform)
template <bool FIELDS>
__device__ __forceinline__ double dist_factor(const DistCoords &v, const DistExtra &x, int code) {
  if (code >= VPIC_HIP_FACTOR_ONE)
    return code == VPIC_HIP_FACTOR_ONE ? 1.0 : code == VPIC_HIP_FACTOR_Q ? x.q
         : FIELDS && code == VPIC_HIP_FACTOR_EDOTV ? x.edotv : x.epar_vpar;
  return dist_coord<FIELDS>(v, code);
}

// ---- a whole selection (vpic_hip_select_t): the ranges and the tag conditions, for select.hip and the selected moments of
// moments.hip ----
struct SelectK {
  vpic_hip_select_t s;
  unsigned need;                                           // as DistK::need: the coordinates the ranges name
  int use_tag;                                             // a tag condition is enabled (the flags of s)
};
// (host) of a checked descriptor
inline SelectK make_select_k(const vpic_hip_select_t &d) {
  SelectK k{};
  k.s = d;
  for (int r = 0; r < d.n_sel; r++) k.need |= 1u << d.sel[r].coord;
  k.use_tag = (d.flags & (VPIC_HIP_SELECT_TAG_RANGE | VPIC_HIP_SELECT_TAG_EVERY)) != 0;
  return k;
}

// the tag conditions of a descriptor (all enabled ones must hold)
__device__ __forceinline__ bool select_tag_ok(const vpic_hip_select_t &s, long long tag) {
  bool ok = true;
  if (s.flags & VPIC_HIP_SELECT_TAG_RANGE) ok = ok && tag >= s.tag_lo && tag < s.tag_hi;
  if (s.flags & VPIC_HIP_SELECT_TAG_EVERY) {
    long long r = tag % s.tag_every;                       // (|r| < every: r + every cannot overflow)
    if (r < 0) r += s.tag_every;
    ok = ok && r == s.tag_phase;
  }
  return ok;
}

}  // namespace vpichip
