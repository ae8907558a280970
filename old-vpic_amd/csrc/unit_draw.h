// unit_draw.h -- the counter-based generator of the particle sources (particles.hip: the reflux handlers, the emitter, the
// synthetic loader): a 32-bit mixer and the map from its output to a float strictly inside (0, 1).  The arithmetic alone,
// so that it compiles on the host as well (tests/unit_draw_check.cpp walks every value).
//
// unit_open(r) = ((float)(r >> 8) + 0.5f) * 2^-24, and for r >> 8 == 2^24 - 1 the largest float below 1 instead: the sum
// 16777215.5 is a tie that rounds to 2^24, which would make the result exactly 1.0f -- and sqrtf(-logf(1)) a refluxed or
// emitted particle with a normal momentum of exactly zero, which never leaves its wall (maxwellian_reflux.c:116-118 draws
// from the open interval for this reason).  Every other draw is what it was before the clamp; the smallest is 2^-24.
// unit_top_closed(r) is the map without the clamp, 0 < x <= 1, for the synthetic loader alone: there a draw of 1 is a
// particle on the upper face of its cell (a valid position) or a thermal radius of zero, both harmless, and the loaded
// particles are pinned draw for draw (tests/test_gpu_distribution.py: test_cold_beam_at_size counts the particles on a face)
// and are what the benchmark pushes: they stay what they were.
// (collide.hip keeps its own copy without the clamp: there log(1) = 0 is a scattering angle of zero, harmless, and its
// arithmetic is stated in include/vpic_hip.h and pinned bit for bit by tests/collide_ref.py.)
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define VH_UNIT_HD __host__ __device__ __forceinline__
#else
#define VH_UNIT_HD inline
#endif

namespace vpichip {

constexpr float UNIT_OPEN_MAX = 0x1.fffffep-1f;                     // 1 - 2^-24, the largest float below 1

// lowbias32: a bijection of the 32-bit integers
VH_UNIT_HD uint32_t mix32(uint32_t x) { x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16; return x; }

// 0 < unit_top_closed(r) <= 1: exactly 1 for r >> 8 == 2^24 - 1 and for no other r
VH_UNIT_HD float unit_top_closed(uint32_t r) { return ((float)(r >> 8) + 0.5f) * (1.f / 16777216.f); }

// 0 < unit_open(r) < 1 for every r
VH_UNIT_HD float unit_open(uint32_t r) {
  const float x = unit_top_closed(r);
  return x < UNIT_OPEN_MAX ? x : UNIT_OPEN_MAX;
}

}  // namespace vpichip
