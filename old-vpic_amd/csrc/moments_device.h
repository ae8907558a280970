// moments_device.h -- what one particle adds to the hydro moments and to rho, stated ONCE: the per-particle kernel and the
// per-cell kernel of push.hip / fields.hip and the tile kernels of moments.hip all take their numbers from here, operation
// for operation (species_advance/standard/hydro_p.c:24-176, rho_p.c:43-84; no contraction: csrc/Makefile).
#pragma once
#include <hip/hip_runtime.h>

namespace vpichip {

constexpr int HYDRO_MOMENTS = 14;       // jx jy jz rho px py pz ke txx tyy tzz tyz tzx txy (hydro_t; two floats of padding follow)
constexpr int HYDRO_STRIDE = 16;

struct HydroConsts { float qdt_2mc, qdt_4mc2, c, r8V, mc_q; };   // hydro_p.c:49-53
struct InterpK { float4 ex, ey, ez, b0; float2 b1; };            // interpolator_t of one voxel
__device__ __forceinline__ InterpK load_interp(const float4 *__restrict__ fi, int voxel) {
  const float4 *f = fi + (size_t)voxel * 5;
  return InterpK{f[0], f[1], f[2], f[3], *reinterpret_cast<const float2 *>(f + 4)};
}

// the time-centred momentum and velocity of a particle, its kinetic energy per mc, and its eight trilinear weights
struct HydroP { float ux, uy, uz, vx, vy, vz, ke_mc, w[8]; };

// rho_p.c:43-84 / hydro_p.c:109-131: weight of the particle on the 8 nodes of its cell (x fastest)
__device__ __forceinline__ void node_weights(float dx, float dy, float dz, float q, float r8V, float *w) {
  float t;
  t = dx; w[0] = r8V * q; t *= w[0]; w[1] = w[0] + t; w[0] -= t;
  t = dy; w[3] = 1.f + t; w[2] = w[0] * w[3]; w[3] *= w[1]; t = 1.f - t; w[0] *= t; w[1] *= t;
  t = dz; w[7] = 1.f + t; w[4] = w[0] * w[7]; w[5] = w[1] * w[7]; w[6] = w[2] * w[7]; w[7] *= w[3];
  t = 1.f - t; w[0] *= t; w[1] *= t; w[2] *= t; w[3] *= t;
}

// The particle is time-centred as in center_p (half E kick, half Boris rotation -- with the reference's double-precision
// pieces kept: sqrt in double, the series factor in double).
__device__ __forceinline__ void hydro_particle(float dx, float dy, float dz, float ux, float uy, float uz, float q,
                                               const InterpK &f, const HydroConsts &h, HydroP &o) {
  float vz, ke_mc, w0, w1, w2, w3, w4, w5, w6, w7;
  ux += h.qdt_2mc * ((f.ex.x + dy * f.ex.y) + dz * (f.ex.z + dy * f.ex.w));
  uy += h.qdt_2mc * ((f.ey.x + dz * f.ey.y) + dx * (f.ey.z + dz * f.ey.w));
  uz += h.qdt_2mc * ((f.ez.x + dx * f.ez.y) + dy * (f.ez.z + dx * f.ez.w));
  w5 = f.b0.x + dx * f.b0.y; w6 = f.b0.z + dy * f.b0.w; w7 = f.b1.x + dz * f.b1.y;
  ke_mc = ux * ux + uy * uy + uz * uz;
  vz = (float)sqrt((double)(1.f + ke_mc));                                   // hydro_p.c:86
  ke_mc *= h.c / (vz + 1.f);
  vz = h.c / vz;
  w0 = h.qdt_4mc2 * vz;
  w1 = w5 * w5 + w6 * w6 + w7 * w7;
  w2 = w0 * w0 * w1;
  w3 = (float)((double)w0 * (1. + (1. / 3.) * (double)w2 * (1. + 0.4 * (double)w2)));   // hydro_p.c:92
  w4 = w3 / (1.f + w1 * w3 * w3); w4 += w4;
  w0 = ux + w3 * (uy * w7 - uz * w6);
  w1 = uy + w3 * (uz * w5 - ux * w7);
  w2 = uz + w3 * (ux * w6 - uy * w5);
  ux += w4 * (w1 * w7 - w2 * w6);
  uy += w4 * (w2 * w5 - w0 * w7);
  uz += w4 * (w0 * w6 - w1 * w5);
  o.ux = ux; o.uy = uy; o.uz = uz;
  o.vx = ux * vz; o.vy = uy * vz; o.vz = vz * uz;
  o.ke_mc = ke_mc;
  node_weights(dx, dy, dz, q, h.r8V, o.w);
}

// the 14 products a particle adds to the node it has weight w on (hydro_p.c:133-158)
__device__ __forceinline__ void hydro_node(const HydroP &p, float w, float mc_q, float *m) {
  m[0] = w * p.vx; m[1] = w * p.vy; m[2] = w * p.vz; m[3] = w;
  w *= mc_q; const float ax = w * p.ux, ay = w * p.uy, az = w * p.uz;
  m[4] = ax; m[5] = ay; m[6] = az; m[7] = w * p.ke_mc;
  m[8] = ax * p.vx; m[9] = ay * p.vy; m[10] = az * p.vz;
  m[11] = ay * p.vz; m[12] = az * p.vx; m[13] = ax * p.vy;
}

}  // namespace vpichip
