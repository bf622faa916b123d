// cw_compare.hip.h - what the compare kernels of the three tables share (cw64.hip cw64_compare_kernel, cw_kernels.hip
// cw_compare_kernel, cw_bits.hip cw_bits_compare_kernel): the streaming loads of the image and the two-step reduction of the
// mismatches of a workgroup.
//   low[64]   one word per instance of the workgroup's tile, in LDS, CMP_EQUAL before the first barrier.  A wave that finds the
//             pieces of an instance different notes the lowest differing entry with ONE LDS atomicMin (the lanes are reduced by
//             a ballot first); an equal piece touches nothing.
//   report    after the second barrier wave 0, lane = instance, reads the 64 words: a lane whose word is not CMP_EQUAL does the
//             one global atomicMin(&diff[j], entry) of this workgroup for its instance.  atomicMin returns the old word: the
//             workgroup that sees CMP_EQUAL come back is the first to report the instance and counts it - after a ballot one lane
//             adds the number of such lanes to summary[0] and takes summary[1] down to the lowest of them.  So an instance counts
//             once however many entry tiles found a difference, and an image that matches makes no global atomic at all.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define CMP_EQUAL 0xFFFFFFFFu

typedef uint32_t cmp_u32x4 __attribute__((ext_vector_type(4)));
// the image is read once: streaming (nt) loads
__device__ __forceinline__ uint4 cmp_load16(const uint4 *p) {
    const cmp_u32x4 w = __builtin_nontemporal_load((const cmp_u32x4 *)p);
    return make_uint4(w.x, w.y, w.z, w.w);
}
__device__ __forceinline__ uint64_t cmp_load8(const uint64_t *p) { return __builtin_nontemporal_load(p); }
__device__ __forceinline__ bool cmp_ne(const uint4 &a, const uint4 &b) { return ((a.x ^ b.x) | (a.y ^ b.y) | (a.z ^ b.z) | (a.w ^ b.w)) != 0; }

// wave 0 of the workgroup, all 64 lanes, after the barrier behind the last note: lane l speaks for position j0 + l of the launch
// (`live`: it is one), report0 + j0 + l in the caller's numbering.  `summary` may be nullptr.
__device__ __forceinline__ void cmp_report(const uint32_t *low, uint32_t lane, bool live, uint32_t j0, uint32_t report0,
                                           uint32_t *__restrict__ diff, uint32_t *__restrict__ summary) {
    const uint32_t v = live ? low[lane] : CMP_EQUAL;
    bool fresh = false;
    if (v != CMP_EQUAL) fresh = atomicMin(&diff[j0 + lane], v) == CMP_EQUAL;
    const uint64_t who = __ballot(fresh);
    if (summary && who && lane == (uint32_t)__builtin_ctzll(who)) {
        atomicAdd(&summary[0], (uint32_t)__builtin_popcountll(who));
        atomicMin(&summary[1], report0 + j0 + lane);
    }
}
