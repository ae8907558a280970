// record_offsets.h -- where advance_p_kernel (push.hip) finds a particle: the arithmetic alone, so that it compiles on
// the host as well (tests/record_offsets_check.cpp drives it at the limits).
//
// The kernel addresses each particle array as (a wave-uniform 64-bit base in scalar registers) + (one 32-bit byte offset per
// lane): the scalar-base form of global_load / global_store.  With 4-byte arrays and the base at the array's start the
// offset idx << 2 reaches 2^30 particles, one launch's worth (vpic_hip_push_plan).  A 16-byte position record does not:
// idx << 4 wraps from 2^28 particles on.  So every workgroup REBASES: the base is the array's start plus the workgroup's
// first particle (64-bit, wave-uniform: `first` of a tile, `first2` of its appended share, chunk * WAVES * wave_span in the
// reference's order) and a lane's offset is relative to it.  What a workgroup reaches from one base -- its own range, the
// lanes of a last, partly filled pass behind it, its queued cell-crossers -- must stay below 2^28 records.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define VH_HD __host__ __device__ __forceinline__
#else
#define VH_HD inline
#endif

namespace vpichip {

constexpr int RECORD_SHIFT = 4, WORD_SHIFT = 2;                   // log2 of the bytes of a position record / of a momentum or charge
constexpr int64_t RECORD_REACH = (int64_t)1 << (32 - RECORD_SHIFT);   // records one base reaches with a 32-bit byte offset
constexpr int PASS_LANES = 64;                                    // a pass addresses up to 63 slots behind its last particle

// the workgroup's base, in BYTES from the start of the record array (64-bit: 2^31 particles are 32 GiB of records)
VH_HD uint64_t record_base_bytes(int64_t first) { return (uint64_t)first << RECORD_SHIFT; }
VH_HD uint64_t word_base_bytes(int64_t first) { return (uint64_t)first << WORD_SHIFT; }
// a lane's byte offset from that base, idx >= first
VH_HD uint32_t record_offset(int idx, int first) { return (uint32_t)(idx - first) << RECORD_SHIFT; }
VH_HD uint32_t word_offset(int idx, int first) { return (uint32_t)(idx - first) << WORD_SHIFT; }
// ... of the slot a lane LOADS: lanes behind the last particle (np - 1) read that one
VH_HD int load_slot(int idx, int first, int np) { return (idx < np - 1 ? idx : np - 1) - first; }
// can a workgroup whose particles are [first, last) address all it touches from its base?
VH_HD bool span_in_reach(int64_t first, int64_t last) { return last - first + PASS_LANES <= RECORD_REACH; }
// SORT: a destination anywhere in the second buffer, as a 64-bit byte offset (one 32 x 32 + 64 bit multiply-add on the device)
VH_HD uint64_t record_address(uint64_t base, uint32_t dst) { return base + (uint64_t)dst * (uint64_t)(1u << RECORD_SHIFT); }

// particles per launch segment of a species pushed in chunks of per_chunk (vpic_hip_push_plan): a launch of c particles
// addresses up to slot c + 62 of the 4-byte arrays from THEIR start, (c + 63) * 4 < 2^32; segments begin on a chunk boundary
VH_HD int64_t push_segment_particles(int64_t per_chunk) { return ((((int64_t)1 << 30) - PASS_LANES) / per_chunk) * per_chunk; }

}  // namespace vpichip
