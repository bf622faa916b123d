// ubench_ingest.hip - variants of the 32-byte ingest (cw_bits.hip::cw_bits_ingest_kernel) on the default bench line's shape:
// 2^21 instances x 2 048 inputs x 32 bytes = 137 GB in, one 64-bit mask per (group of 64 instances, input) out (emitted layout, sh = 5).
// Every variant must leave the table and the flag words of variant 0 (checksums compared); the last line is a read-only
// ceiling (a grid-stride uint4 sum over the same buffer).
//   hipcc -O3 --offload-arch=gfx950 tools/ubench_ingest.hip -o tools/ubench_ingest && tools/ubench_ingest [log2 batch] [n_in] [line [sh0]]
// `line`: the library's form and the line-once variants only; `sh0`: masks of a group contiguous (sh = 0, what the staged route writes)
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "../circom_amd/csrc/cw_bits_layout.h"

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)

__device__ __forceinline__ uint64_t *bits_group(uint64_t *T, uint64_t slots, uint32_t sh, uint32_t g) {
    return T + (((size_t)(g >> sh) * slots) << sh) + (g & ((1u << sh) - 1u));
}

__global__ void fill_kernel(uint4 *in, size_t n_elems, uint32_t n_in) {        // element e = (instance, input): a bit, rarely a non-bit
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n_elems; e += (size_t)gridDim.x * blockDim.x) {
        uint64_t h = e * 0x9E3779B97F4A7C15ull;
        h ^= h >> 29; h *= 0xBF58476D1CE4E5B9ull; h ^= h >> 32;
        uint4 lo = make_uint4((uint32_t)h & 1u, 0, 0, 0), hi = make_uint4(0, 0, 0, 0);
        if ((h >> 40) == 12345u) { if (h & 2) lo.x = 2; else hi.z = 1; }          // ~1 in 16 M elements is not a bit
        in[2 * e] = lo;
        in[2 * e + 1] = hi;
    }
}

// ---- variant 0: the shipped kernel -------------------------------------------------------------------------------------------
template <int SWAP>
__global__ void __launch_bounds__(64) ingest_v0(const uint4 *__restrict__ in, uint64_t *__restrict__ T, uint64_t slots, uint32_t sh,
                                                uint32_t input_slot0, uint32_t n_in, uint32_t batch, uint64_t *fbmask, uint32_t nchunk) {
    uint32_t g, c;
    if (SWAP) { c = blockIdx.x % nchunk; g = blockIdx.x / nchunk; } else { g = blockIdx.x; c = blockIdx.y; }
    const uint32_t lane = threadIdx.x, k = c * 64 + lane;
    const bool have = k < n_in;
    const uint32_t i0 = g * 64, ni = min(64u, batch - i0);
    uint64_t mine = 0, badmask = 0;
    for (uint32_t ii = 0; ii < ni; ii++) {
        uint4 lo = make_uint4(0, 0, 0, 0), hi = lo;
        if (have) {
            const size_t src = ((size_t)(i0 + ii) * n_in + k) * 2;
            lo = in[src];
            hi = in[src + 1];
        }
        const bool isbit = (lo.x <= 1u) & ((lo.y | lo.z | lo.w | hi.x | hi.y | hi.z | hi.w) == 0u);
        mine |= (uint64_t)(lo.x & 1u) << ii;
        if (__any(!isbit)) badmask |= 1ull << ii;
    }
    if (have) bits_group(T, slots, sh, g)[(size_t)(input_slot0 + k) << sh] = mine;
    if (lane == 0 && badmask) atomicOr((unsigned long long *)&fbmask[g], (unsigned long long)badmask);
}

// ---- variants 1..: the flag stays per lane until the end, full groups run a constant-trip loop unrolled U times ---------------
template <int U, int SWAP, int NT>
__global__ void __launch_bounds__(64) ingest_v1(const uint4 *__restrict__ in, uint64_t *__restrict__ T, uint64_t slots, uint32_t sh,
                                                uint32_t input_slot0, uint32_t n_in, uint32_t batch, uint64_t *fbmask, uint32_t nchunk) {
    uint32_t g, c;
    if (SWAP) { c = blockIdx.x % nchunk; g = blockIdx.x / nchunk; } else { g = blockIdx.x; c = blockIdx.y; }
    const uint32_t lane = threadIdx.x, k = c * 64 + lane;
    const bool have = k < n_in;
    const uint32_t i0 = g * 64, ni = min(64u, batch - i0);
    uint64_t mine = 0, bad = 0;
    const uint4 *p = in + ((size_t)i0 * n_in + (have ? k : 0)) * 2;
    const size_t step = (size_t)n_in * 2;
    if (ni == 64) {
#pragma unroll U
        for (uint32_t ii = 0; ii < 64; ii++) {
            uint4 lo, hi;
            if (NT) {
                const u32x4 a = __builtin_nontemporal_load((const u32x4 *)p), b = __builtin_nontemporal_load((const u32x4 *)p + 1);
                lo = make_uint4(a.x, a.y, a.z, a.w); hi = make_uint4(b.x, b.y, b.z, b.w);
            } else { lo = p[0]; hi = p[1]; }
            p += step;
            const uint32_t rest = lo.y | lo.z | lo.w | hi.x | hi.y | hi.z | hi.w;
            const bool notbit = (lo.x > 1u) | (rest != 0u);
            mine |= (uint64_t)(lo.x & 1u) << ii;
            bad |= (uint64_t)notbit << ii;
        }
    } else {
        for (uint32_t ii = 0; ii < ni; ii++) {
            const uint4 lo = p[0], hi = p[1];
            p += step;
            const uint32_t rest = lo.y | lo.z | lo.w | hi.x | hi.y | hi.z | hi.w;
            mine |= (uint64_t)(lo.x & 1u) << ii;
            bad |= (uint64_t)((lo.x > 1u) | (rest != 0u)) << ii;
        }
    }
    if (have) {
        bits_group(T, slots, sh, g)[(size_t)(input_slot0 + k) << sh] = mine;
        if (bad) atomicOr((unsigned long long *)&fbmask[g], (unsigned long long)bad);
    }
}

// ---- variant: a workgroup of four waves, wave w takes chunk 4 c + w of the same group ------------------------------------------
template <int U>
__global__ void __launch_bounds__(256) ingest_v4w(const uint4 *__restrict__ in, uint64_t *__restrict__ T, uint64_t slots, uint32_t sh,
                                                  uint32_t input_slot0, uint32_t n_in, uint32_t batch, uint64_t *fbmask, uint32_t nchunk4) {
    const uint32_t c = blockIdx.x % nchunk4, g = blockIdx.x / nchunk4;
    const uint32_t k = c * 256 + threadIdx.x;
    const bool have = k < n_in;
    const uint32_t i0 = g * 64, ni = min(64u, batch - i0);
    uint64_t mine = 0, bad = 0;
    const uint4 *p = in + ((size_t)i0 * n_in + (have ? k : 0)) * 2;
    const size_t step = (size_t)n_in * 2;
    if (ni == 64) {
#pragma unroll U
        for (uint32_t ii = 0; ii < 64; ii++) {
            const uint4 lo = p[0], hi = p[1];
            p += step;
            const uint32_t rest = lo.y | lo.z | lo.w | hi.x | hi.y | hi.z | hi.w;
            mine |= (uint64_t)(lo.x & 1u) << ii;
            bad |= (uint64_t)((lo.x > 1u) | (rest != 0u)) << ii;
        }
    } else {
        for (uint32_t ii = 0; ii < ni; ii++) {
            const uint4 lo = p[0], hi = p[1];
            p += step;
            const uint32_t rest = lo.y | lo.z | lo.w | hi.x | hi.y | hi.z | hi.w;
            mine |= (uint64_t)(lo.x & 1u) << ii;
            bad |= (uint64_t)((lo.x > 1u) | (rest != 0u)) << ii;
        }
    }
    if (have) {
        bits_group(T, slots, sh, g)[(size_t)(input_slot0 + k) << sh] = mine;
        if (bad) atomicOr((unsigned long long *)&fbmask[g], (unsigned long long)bad);
    }
}


// ---- variant: every wave starts at its own instance of the group (rotation r): waves that run together then sit in different
// 64 KB records instead of marching through them in step -----------------------------------------------------------------------
template <int U, int SWAP, int ROT>
__global__ void __launch_bounds__(64) ingest_rot(const uint4 *__restrict__ in, uint64_t *__restrict__ T, uint64_t slots, uint32_t sh,
                                                 uint32_t input_slot0, uint32_t n_in, uint32_t batch, uint64_t *fbmask, uint32_t nchunk) {
    uint32_t g, c;
    if (SWAP) { c = blockIdx.x % nchunk; g = blockIdx.x / nchunk; } else { g = blockIdx.x; c = blockIdx.y; }
    const uint32_t lane = threadIdx.x, k = c * 64 + lane;
    const bool have = k < n_in;
    const uint32_t i0 = g * 64, ni = min(64u, batch - i0);
    uint64_t mine = 0, bad = 0;
    const uint4 *base = in + ((size_t)i0 * n_in + (have ? k : 0)) * 2;
    const size_t step = (size_t)n_in * 2;
    if (ni == 64) {
        const uint32_t r = ROT == 1 ? (g * 0x9E3779B1u) >> 26 : ROT == 2 ? ((g * 32u + c) * 0x9E3779B1u) >> 26 : ROT == 3 ? (g & 63u) : (c * 2u) & 63u;
#pragma unroll U
        for (uint32_t ii = 0; ii < 64; ii++) {
            const uint32_t inst = (ii + r) & 63u;
            const uint4 *p = base + inst * step;
            const uint4 lo = p[0], hi = p[1];
            const uint32_t rest = lo.y | lo.z | lo.w | hi.x | hi.y | hi.z | hi.w;
            mine |= (uint64_t)(lo.x & 1u) << inst;
            bad |= (uint64_t)((lo.x > 1u) | (rest != 0u)) << inst;
        }
    } else {
        const uint4 *p = base;
        for (uint32_t ii = 0; ii < ni; ii++) {
            const uint4 lo = p[0], hi = p[1];
            p += step;
            const uint32_t rest = lo.y | lo.z | lo.w | hi.x | hi.y | hi.z | hi.w;
            mine |= (uint64_t)(lo.x & 1u) << ii;
            bad |= (uint64_t)((lo.x > 1u) | (rest != 0u)) << ii;
        }
    }
    if (have) {
        bits_group(T, slots, sh, g)[(size_t)(input_slot0 + k) << sh] = mine;
        if (bad) atomicOr((unsigned long long *)&fbmask[g], (unsigned long long)bad);
    }
}

// ---- variant: a wave takes 128 inputs (4 KiB runs, two masks per lane) ---------------------------------------------------------
template <int U>
__global__ void __launch_bounds__(64) ingest_wide(const uint4 *__restrict__ in, uint64_t *__restrict__ T, uint64_t slots, uint32_t sh,
                                                  uint32_t input_slot0, uint32_t n_in, uint32_t batch, uint64_t *fbmask, uint32_t nchunk2) {
    const uint32_t g = blockIdx.x, c = blockIdx.y, lane = threadIdx.x, k = c * 128 + lane;      // and k + 64
    const uint32_t i0 = g * 64, ni = min(64u, batch - i0);
    uint64_t m0 = 0, m1 = 0, bad = 0;
    const uint4 *p = in + ((size_t)i0 * n_in + k) * 2;
    const size_t step = (size_t)n_in * 2;
    if (k + 64 < n_in + 0u && ni == 64) {
#pragma unroll U
        for (uint32_t ii = 0; ii < 64; ii++) {
            const uint4 lo = p[0], hi = p[1], lo2 = p[128], hi2 = p[129];
            p += step;
            const uint32_t rest = lo.y | lo.z | lo.w | hi.x | hi.y | hi.z | hi.w, rest2 = lo2.y | lo2.z | lo2.w | hi2.x | hi2.y | hi2.z | hi2.w;
            m0 |= (uint64_t)(lo.x & 1u) << ii;
            m1 |= (uint64_t)(lo2.x & 1u) << ii;
            bad |= (uint64_t)((lo.x > 1u) | (rest != 0u) | (lo2.x > 1u) | (rest2 != 0u)) << ii;
        }
        uint64_t *Tg = bits_group(T, slots, sh, g);
        Tg[(size_t)(input_slot0 + k) << sh] = m0;
        Tg[(size_t)(input_slot0 + k + 64) << sh] = m1;
        if (bad) atomicOr((unsigned long long *)&fbmask[g], (unsigned long long)bad);
    }
}


// ---- variant: workgroups of NW waves on consecutive chunks of one group, rotated start ---------------------------------------
template <int U, int NW, int ROT>
__global__ void __launch_bounds__(64 * NW) ingest_nw(const uint4 *__restrict__ in, uint64_t *__restrict__ T, uint64_t slots, uint32_t sh,
                                                     uint32_t input_slot0, uint32_t n_in, uint32_t batch, uint64_t *fbmask, uint32_t nchunkw) {
    const uint32_t c = blockIdx.x % nchunkw, g = blockIdx.x / nchunkw;
    const uint32_t k = c * (64 * NW) + threadIdx.x;
    const bool have = k < n_in;
    const uint32_t i0 = g * 64, ni = min(64u, batch - i0);
    uint64_t mine = 0, bad = 0;
    const uint4 *base = in + ((size_t)i0 * n_in + (have ? k : 0)) * 2;
    const size_t step = (size_t)n_in * 2;
    if (ni == 64) {
        const uint32_t r = ROT ? (g * 0x9E3779B1u) >> 26 : 0u;
#pragma unroll U
        for (uint32_t ii = 0; ii < 64; ii++) {
            const uint32_t inst = (ii + r) & 63u;
            const uint4 *p = base + inst * step;
            const uint4 lo = p[0], hi = p[1];
            const uint32_t rest = lo.y | lo.z | lo.w | hi.x | hi.y | hi.z | hi.w;
            mine |= (uint64_t)(lo.x & 1u) << inst;
            bad |= (uint64_t)((lo.x > 1u) | (rest != 0u)) << inst;
        }
    } else {
        const uint4 *p = base;
        for (uint32_t ii = 0; ii < ni; ii++) {
            const uint4 lo = p[0], hi = p[1];
            p += step;
            const uint32_t rest = lo.y | lo.z | lo.w | hi.x | hi.y | hi.z | hi.w;
            mine |= (uint64_t)(lo.x & 1u) << ii;
            bad |= (uint64_t)((lo.x > 1u) | (rest != 0u)) << ii;
        }
    }
    if (have) {
        bits_group(T, slots, sh, g)[(size_t)(input_slot0 + k) << sh] = mine;
        if (bad) atomicOr((unsigned long long *)&fbmask[g], (unsigned long long)bad);
    }
}

// ---- the line-once map (circom_amd/csrc/cw_bits_layout.h `line_*`): lane = one 16-byte piece, a load instruction = 1 KiB contiguous,
// every 128-byte line touched by exactly one instruction; the walk (workgroup -> (group, 256 inputs), chunks fastest, four waves,
// rotated start, four instances = eight loads per trip) is ingest_nw<4, 4, 1>'s.  Two transports:
//   XPORT 0  plain 16-byte loads into VGPRs
//   XPORT 1  LDS-DMA (global_load_lds_dwordx4) into a ring of D slots of 1 KiB per wave, read back by the lane that asked
//            (ds_read_b128 at slot * 1024 + lane * 16).  The waits are counted by hand from the wave's own loads (hipcc neither
//            sees the asm reads nor orders the DMA against them): cw_bits_layout.h line_ring_*.
// NT: the loads carry the streaming policy.  CEIL: the same traffic with nothing kept (the read-only ceiling of the transport).
struct LineAcc {
    uint64_t bit[2], bad[2];
    uint32_t thr, keep, sum;
    uint32_t bl[2], bh[2], fl[2], fh[2];                             // ROT: the masks as dword pairs, newest instance on top
    template <int CEIL, int ROT> __device__ __forceinline__ void take(int h, const u32x4 v, uint32_t inst) {
        if (CEIL) { sum += v.x ^ v.y ^ v.z ^ v.w; return; }
        if (ROT) {
            // the walk visits the instances in order: shift the masks down by one and put the new bit on top (v_alignbit_b32:
            // {a, b} >> 1, bit 0 of a arrives at bit 31); the rotation is undone once, after the loop
            const uint32_t nz = ((v.x & keep) | v.y) | v.z | v.w, f = nz < 1u ? nz : 1u;
            bl[h] = __builtin_amdgcn_alignbit(bh[h], bl[h], 1);
            bh[h] = __builtin_amdgcn_alignbit(v.x, bh[h], 1);
            fl[h] = __builtin_amdgcn_alignbit(fh[h], fl[h], 1);
            fh[h] = __builtin_amdgcn_alignbit(f, fh[h], 1);
            return;
        }
        bit[h] |= (uint64_t)(v.x & 1u) << inst;
        bad[h] |= (uint64_t)((uint32_t)(v.x > thr) | (uint32_t)((v.y | v.z | v.w) != 0u)) << inst;
    }
    // after `steps` steps from instance `first` (steps = 64: any first; fewer: first = 0)
    __device__ __forceinline__ void unrotate(uint32_t steps, uint32_t first) {
        for (int h = 0; h < 2; h++) {
            const uint64_t b = ((uint64_t)bh[h] << 32) | bl[h], f = ((uint64_t)fh[h] << 32) | fl[h];
            if (steps == 64) {
                bit[h] = first ? (b << first) | (b >> (64 - first)) : b;
                bad[h] = first ? (f << first) | (f >> (64 - first)) : f;
            } else {
                bit[h] = b >> (64 - steps);
                bad[h] = f >> (64 - steps);
            }
        }
    }
};
typedef __attribute__((address_space(3))) void line_lds_t;
typedef __attribute__((address_space(1))) void line_glb_t;
template <int NT> __device__ __forceinline__ void line_dma(const uint4 *src, uint32_t lds_byte) {
    __builtin_amdgcn_global_load_lds((line_glb_t *)src, (line_lds_t *)(uintptr_t)lds_byte, 16, 0, NT ? 2 : 0);
}
template <int NT> __device__ __forceinline__ u32x4 line_load(const uint4 *src) {
    return NT ? __builtin_nontemporal_load((const u32x4 *)src) : *(const u32x4 *)src;
}
// batch b of the ring (loads b * D/2 ..): wait until at most PENDING of the wave's loads are in flight, read the batch's slots,
// wait for the reads, hand the slots to the loads D further on, then use what was read
template <int D, int NT, int CEIL, int ROT, int PENDING, bool REFILL, int HALF>
__device__ __forceinline__ void line_ring_batch_step(uint32_t b, LineAcc &A, const uint4 *base, size_t step, const uint32_t (&o)[2], uint32_t r,
                                                     uint32_t ring, uint32_t lane16) {
    constexpr int BT = D / 2;
    u32x4 v[BT];
    asm volatile("s_waitcnt vmcnt(%0)" ::"i"(PENDING) : "memory");
#pragma unroll
    for (int j = 0; j < BT; j++) asm volatile("ds_read_b128 %0, %1" : "=v"(v[j]) : "v"(ring + (HALF * BT + j) * 1024u + lane16));
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int j = 0; j < BT; j++) asm volatile("" : "+v"(v[j]));
    if (REFILL) {
#pragma unroll
        for (int j = 0; j < BT; j++) {
            const uint32_t n = b * BT + j + D, inst = ((n >> 1) + r) & 63u;
            line_dma<NT>(base + inst * step + o[j & 1], ring + (HALF * BT + j) * 1024u);
        }
    }
#pragma unroll
    for (int j = 0; j < BT; j++) {
        const uint32_t n = b * BT + j;
        A.take<CEIL, ROT>(j & 1, v[j], ((n >> 1) + r) & 63u);
    }
}
extern __shared__ uint4 line_ring_lds[];
template <int XPORT, int NT, int D, int CEIL, int ROT = 0>
__global__ void __launch_bounds__(256) ingest_line(const uint4 *__restrict__ in, uint64_t *__restrict__ T, uint64_t slots, uint32_t sh,
                                                   uint32_t input_slot0, uint32_t n_in, uint32_t batch, uint64_t *fbmask, uint32_t nchunkw,
                                                   uint32_t *sink) {
    using namespace cwlayout;
    const uint32_t c = blockIdx.x % nchunkw, g = blockIdx.x / nchunkw;
    const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t k0 = line_wave_input0(c, wave);
    if (k0 >= n_in) return;                                           // the whole wave: no barrier below
    const uint32_t i0 = g * 64, ni = min(64u, batch - i0);
    const uint32_t p[2] = {line_piece(k0, 0, lane), line_piece(k0, 1, lane)};
    const bool act[2] = {line_piece_active(p[0], n_in), line_piece_active(p[1], n_in)};
    // an inactive lane reads the wave's first piece again (valid memory, a line the wave reads anyway) and drops it
    const uint32_t o[2] = {act[0] ? p[0] : 2u * k0, act[1] ? p[1] : 2u * k0};
    const uint4 *base = in + (size_t)i0 * n_in * 2;
    const size_t step = (size_t)n_in * 2;
    LineAcc A;
    A.bit[0] = A.bit[1] = A.bad[0] = A.bad[1] = 0; A.sum = 0;
    A.thr = line_piece_half(lane) ? 0u : 1u;
    A.keep = line_piece_half(lane) ? 0xFFFFFFFFu : 0xFFFFFFFEu;
    A.bl[0] = A.bl[1] = A.bh[0] = A.bh[1] = A.fl[0] = A.fl[1] = A.fh[0] = A.fh[1] = 0;
    if (ni == 64) {
        const uint32_t r = line_group_start(g);
        if (XPORT == 0) {
#pragma unroll 4
            for (uint32_t ii = 0; ii < 64; ii++) {
                const uint32_t inst = line_instance(ii, r);
                const uint4 *q = base + inst * step;
                const u32x4 v0 = line_load<NT>(q + o[0]), v1 = line_load<NT>(q + o[1]);
                A.take<CEIL, ROT>(0, v0, inst);
                A.take<CEIL, ROT>(1, v1, inst);
            }
        } else {
            constexpr uint32_t BT = line_ring_batch(D), NB = LINE_RING_LOADS / BT;
            static_assert(D % 4 == 0 && LINE_RING_LOADS % D == 0 && NB % 2 == 0, "whole rounds of the ring, both loads of an instance in one batch");
            static_assert(line_ring_pending(D, 0) == BT && line_ring_pending(D, NB - 3) == BT && line_ring_refills(D, NB - 3), "steady state");
            static_assert(line_ring_pending(D, NB - 2) == BT && !line_ring_refills(D, NB - 2), "the last batch but one");
            static_assert(line_ring_pending(D, NB - 1) == 0 && !line_ring_refills(D, NB - 1), "the last batch");
            const uint32_t ring = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint4 *)line_ring_lds + wave * (D * 1024u);
            const uint32_t lane16 = lane * 16u;
#pragma unroll
            for (uint32_t n = 0; n < D; n++) line_dma<NT>(base + line_instance(n >> 1, r) * step + o[n & 1], ring + line_ring_slot(n, D) * 1024u);
            for (uint32_t b = 0; b + 2 < NB; b += 2) {
                line_ring_batch_step<D, NT, CEIL, ROT, BT, true, 0>(b, A, base, step, o, r, ring, lane16);
                line_ring_batch_step<D, NT, CEIL, ROT, BT, true, 1>(b + 1, A, base, step, o, r, ring, lane16);
            }
            line_ring_batch_step<D, NT, CEIL, ROT, BT, false, 0>(NB - 2, A, base, step, o, r, ring, lane16);
            line_ring_batch_step<D, NT, CEIL, ROT, 0, false, 1>(NB - 1, A, base, step, o, r, ring, lane16);
        }
    } else {
        const uint4 *q = base;
        for (uint32_t ii = 0; ii < ni; ii++) {
            const u32x4 v0 = line_load<0>(q + o[0]), v1 = line_load<0>(q + o[1]);
            q += step;
            A.take<CEIL, ROT>(0, v0, ii);
            A.take<CEIL, ROT>(1, v1, ii);
        }
    }
    if (CEIL) {
        if (A.sum == 0x12345678u) *sink = A.sum;
        return;
    }
    if (ROT) A.unrotate(ni, ni == 64 ? line_group_start(g) : 0u);
#pragma unroll
    for (int h = 0; h < 2; h++) {
        if (!act[h]) A.bit[h] = A.bad[h] = 0;
        A.bad[h] |= (uint64_t)__shfl_xor((unsigned long long)A.bad[h], 1);            // the odd lane's half of the same input
    }
    if (!line_piece_half(lane)) {
        uint64_t *Tg = bits_group(T, slots, sh, g);
#pragma unroll
        for (int h = 0; h < 2; h++)
            if (act[h]) Tg[(size_t)(input_slot0 + line_piece_input(p[h])) << sh] = A.bit[h];
        const uint64_t bad = A.bad[0] | A.bad[1];
        if (bad) atomicOr((unsigned long long *)&fbmask[g], (unsigned long long)bad);
    }
}

// ---- read-only ceiling ------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) read_only(const uint4 *__restrict__ in, size_t n16, uint32_t *sink) {
    uint32_t acc = 0;
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * 256;
    for (; i + 3 * stride < n16; i += 4 * stride) {
        const uint4 a = in[i], b = in[i + stride], c = in[i + 2 * stride], d = in[i + 3 * stride];
        acc += a.x ^ a.y ^ a.z ^ a.w ^ b.x ^ b.y ^ b.z ^ b.w ^ c.x ^ c.y ^ c.z ^ c.w ^ d.x ^ d.y ^ d.z ^ d.w;
    }
    for (; i < n16; i += stride) { const uint4 a = in[i]; acc += a.x ^ a.y ^ a.z ^ a.w; }
    if (acc == 0x12345678u) *sink = acc;
}

__global__ void checksum_kernel(const uint64_t *a, size_t n, unsigned long long *out) {
    unsigned long long s = 0, x = 0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        s += a[i] * (2 * i + 1);
        x ^= a[i] + i;
    }
    atomicAdd(&out[0], s);
    atomicXor(&out[1], x);
}

struct Ctx {
    uint4 *in; uint64_t *T, *fb; uint64_t slots; uint32_t sh, n_in, batch, groups, nchunk; size_t t_words;
    unsigned long long *cs;
};

static void sums(Ctx &c, unsigned long long out[4]) {
    CK(hipMemset(c.cs, 0, 32));
    hipLaunchKernelGGL(checksum_kernel, dim3(4096), dim3(256), 0, 0, c.T, c.t_words, c.cs);
    hipLaunchKernelGGL(checksum_kernel, dim3(256), dim3(256), 0, 0, c.fb, (size_t)c.groups, c.cs + 2);
    CK(hipMemcpy(out, c.cs, 32, hipMemcpyDeviceToHost));
}

template <class F> static void run(const char *name, Ctx &c, F launch, const unsigned long long *want, unsigned long long *got_out) {
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    CK(hipMemset(c.T, 0, c.t_words * 8)); CK(hipMemset(c.fb, 0, (size_t)c.groups * 8));
    launch();
    CK(hipDeviceSynchronize());
    unsigned long long got[4];
    sums(c, got);
    if (got_out) for (int i = 0; i < 4; i++) got_out[i] = got[i];
    bool same = true;
    if (want) for (int i = 0; i < 4; i++) same &= got[i] == want[i];
    float best = 1e30f, tot = 0;
    const int reps = 6;
    for (int r = 0; r < reps; r++) {
        CK(hipEventRecord(e0, 0));
        launch();
        CK(hipEventRecord(e1, 0));
        CK(hipEventSynchronize(e1));
        float ms; CK(hipEventElapsedTime(&ms, e0, e1));
        best = ms < best ? ms : best; tot += ms;
    }
    const double bytes = (double)c.batch * c.n_in * 32.0;
    printf("%-44s avg %8.3f ms  best %8.3f ms  %7.1f GB/s (best %7.1f)  %s\n", name, tot / reps, best, bytes / (tot / reps) * 1e-6, bytes / best * 1e-6,
           want ? (same ? "same table + flags" : "DIFFERENT") : "reference");
    fflush(stdout);
}

int main(int argc, char **argv) {
    const int lb = argc > 1 ? atoi(argv[1]) : 21;
    Ctx c;
    c.n_in = argc > 2 ? (uint32_t)atoi(argv[2]) : 2048u;
    c.sh = argc > 4 && !strcmp(argv[4], "sh0") ? 0u : 5u;             // sh0: the interpreter's layout, which is also the staging masks'
    c.batch = 1u << lb; c.slots = c.n_in + 3; c.groups = (c.batch + 63) / 64; c.nchunk = (c.n_in + 63) / 64;
    const size_t n_elems = (size_t)c.batch * c.n_in;
    c.t_words = (size_t)((c.groups + 31) / 32) * c.slots * 32;
    CK(hipMalloc(&c.in, n_elems * 32)); CK(hipMalloc(&c.T, c.t_words * 8)); CK(hipMalloc(&c.fb, (size_t)c.groups * 8)); CK(hipMalloc(&c.cs, 32));
    hipLaunchKernelGGL(fill_kernel, dim3(65536), dim3(256), 0, 0, c.in, n_elems, c.n_in);
    CK(hipDeviceSynchronize());
    printf("batch %u x %u inputs, table shift %u: %.1f GB in, table %.1f MB\n", c.batch, c.n_in, c.sh, n_elems * 32.0 * 1e-9, c.t_words * 8.0 * 1e-6);
    unsigned long long ref[4];
    const dim3 g2(c.groups, c.nchunk), g1(c.groups * c.nchunk);
#define ARGS c.in, c.T, c.slots, c.sh, 3u, c.n_in, c.batch, c.fb
    run("v0 shipped (grid groups x chunks)", c, [&] { hipLaunchKernelGGL(ingest_v0<0>, g2, dim3(64), 0, 0, ARGS, c.nchunk); }, nullptr, ref);
    const bool line_only = argc > 3 && !strcmp(argv[3], "line");      // the library's kernel and the line-once variants only
    uint32_t *sink; CK(hipMalloc(&sink, 4));
#define NWRUN(U, NW, ROT, name) { const uint32_t ncw = (c.n_in + 64 * NW - 1) / (64 * NW); \
        run(name, c, [&] { hipLaunchKernelGGL((ingest_nw<U, NW, ROT>), dim3(c.groups * ncw), dim3(64 * NW), 0, 0, ARGS, ncw); }, ref, nullptr); }
#define LINERUN(X, NT, D, name) LINERUNR(X, NT, D, 0, name)
#define LINERUNR(X, NT, D, ROT, name) { const uint32_t ncw = (c.n_in + 255) / 256; \
        run(name, c, [&] { hipLaunchKernelGGL((ingest_line<X, NT, D, 0, ROT>), dim3(c.groups * ncw), dim3(256), X ? 4 * D * 1024 : 0, 0, ARGS, ncw, sink); }, ref, nullptr); }
#define LINECEIL(X, NT, D, name) { const uint32_t ncw = (c.n_in + 255) / 256; \
        run(name, c, [&] { hipLaunchKernelGGL((ingest_line<X, NT, D, 1>), dim3(c.groups * ncw), dim3(256), X ? 4 * D * 1024 : 0, 0, ARGS, ncw, sink); }, nullptr, nullptr); }
    if (argc > 3 && !line_only) { printf("usage: ubench_ingest [log2 batch] [n_in] [line [sh0]]\n"); return 2; }
    // the gate of the line-once variants: the library's kernel first, between and last, so its own spread inside the process shows
    NWRUN(4, 4, 1, "nw: 4 waves, rot hash(g), unroll 4 (library)")
    LINERUN(0, 0, 8, "line: plain loads")
    LINERUN(0, 1, 8, "line: plain loads, nt")
    LINERUN(1, 0, 4, "line: LDS-DMA, ring 4")
    LINERUN(1, 0, 8, "line: LDS-DMA, ring 8")
    LINERUN(1, 0, 16, "line: LDS-DMA, ring 16")
    NWRUN(4, 4, 1, "nw: 4 waves, rot hash(g), unroll 4 (library)")
    LINERUN(1, 1, 4, "line: LDS-DMA, ring 4, nt")
    LINERUN(1, 1, 8, "line: LDS-DMA, ring 8, nt")
    LINERUN(1, 1, 16, "line: LDS-DMA, ring 16, nt")
    LINERUNR(0, 1, 8, 1, "line: plain loads, nt, masks by rotation")
    LINERUNR(1, 1, 8, 1, "line: LDS-DMA, ring 8, nt, masks by rotation")
    LINERUNR(1, 1, 16, 1, "line: LDS-DMA, ring 16, nt, masks by rotation")
    LINECEIL(0, 1, 8, "line, read only: plain loads, nt")
    LINECEIL(1, 1, 8, "line, read only: LDS-DMA, ring 8, nt")
    NWRUN(4, 4, 1, "nw: 4 waves, rot hash(g), unroll 4 (library)")
    if (line_only) return 0;
    run("v0 chunks fastest", c, [&] { hipLaunchKernelGGL(ingest_v0<1>, g1, dim3(64), 0, 0, ARGS, c.nchunk); }, ref, nullptr);
    run("lane flags, unroll 4", c, [&] { hipLaunchKernelGGL((ingest_v1<4, 0, 0>), g2, dim3(64), 0, 0, ARGS, c.nchunk); }, ref, nullptr);
    run("lane flags, unroll 8", c, [&] { hipLaunchKernelGGL((ingest_v1<8, 0, 0>), g2, dim3(64), 0, 0, ARGS, c.nchunk); }, ref, nullptr);
    run("lane flags, unroll 8, chunks fastest", c, [&] { hipLaunchKernelGGL((ingest_v1<8, 1, 0>), g1, dim3(64), 0, 0, ARGS, c.nchunk); }, ref, nullptr);
    run("lane flags, unroll 8, nontemporal", c, [&] { hipLaunchKernelGGL((ingest_v1<8, 0, 1>), g2, dim3(64), 0, 0, ARGS, c.nchunk); }, ref, nullptr);
    run("lane flags, unroll 8, nontemporal, chunks fastest", c, [&] { hipLaunchKernelGGL((ingest_v1<8, 1, 1>), g1, dim3(64), 0, 0, ARGS, c.nchunk); }, ref, nullptr);
    const uint32_t nchunk4 = (c.n_in + 255) / 256;
    run("4 waves per workgroup, unroll 4", c, [&] { hipLaunchKernelGGL(ingest_v4w<4>, dim3(c.groups * nchunk4), dim3(256), 0, 0, ARGS, nchunk4); }, ref, nullptr);
    run("4 waves per workgroup, unroll 8", c, [&] { hipLaunchKernelGGL(ingest_v4w<8>, dim3(c.groups * nchunk4), dim3(256), 0, 0, ARGS, nchunk4); }, ref, nullptr);
    run("rot by hash(g), unroll 8", c, [&] { hipLaunchKernelGGL((ingest_rot<8, 0, 1>), g2, dim3(64), 0, 0, ARGS, c.nchunk); }, ref, nullptr);
    run("rot by hash(g, c), unroll 8", c, [&] { hipLaunchKernelGGL((ingest_rot<8, 0, 2>), g2, dim3(64), 0, 0, ARGS, c.nchunk); }, ref, nullptr);
    run("rot by hash(g), unroll 8, chunks fastest", c, [&] { hipLaunchKernelGGL((ingest_rot<8, 1, 1>), g1, dim3(64), 0, 0, ARGS, c.nchunk); }, ref, nullptr);
    run("rot by hash(g, c), unroll 8, chunks fastest", c, [&] { hipLaunchKernelGGL((ingest_rot<8, 1, 2>), g1, dim3(64), 0, 0, ARGS, c.nchunk); }, ref, nullptr);
    run("rot by g & 63, unroll 8, chunks fastest", c, [&] { hipLaunchKernelGGL((ingest_rot<8, 1, 3>), g1, dim3(64), 0, 0, ARGS, c.nchunk); }, ref, nullptr);
    run("rot by 2 c, unroll 8, chunks fastest", c, [&] { hipLaunchKernelGGL((ingest_rot<8, 1, 4>), g1, dim3(64), 0, 0, ARGS, c.nchunk); }, ref, nullptr);
    if (c.n_in % 128 == 0) {
        run("128 inputs per wave, unroll 8", c, [&] { hipLaunchKernelGGL(ingest_wide<8>, dim3(c.groups, c.n_in / 128), dim3(64), 0, 0, ARGS, c.n_in / 128); }, ref, nullptr);
    }
    NWRUN(8, 1, 1, "nw: 1 wave, rot hash(g), unroll 8")
    NWRUN(4, 1, 1, "nw: 1 wave, rot hash(g), unroll 4")
    NWRUN(16, 1, 1, "nw: 1 wave, rot hash(g), unroll 16")
    NWRUN(8, 2, 1, "nw: 2 waves, rot hash(g), unroll 8")
    NWRUN(8, 4, 1, "nw: 4 waves, rot hash(g), unroll 8")
    NWRUN(4, 4, 1, "nw: 4 waves, rot hash(g), unroll 4")
    NWRUN(2, 4, 1, "nw: 4 waves, rot hash(g), unroll 2")
    NWRUN(8, 8, 1, "nw: 8 waves, rot hash(g), unroll 8")
    NWRUN(4, 8, 1, "nw: 8 waves, rot hash(g), unroll 4")
    NWRUN(8, 16, 1, "nw: 16 waves, rot hash(g), unroll 8")
    NWRUN(4, 16, 1, "nw: 16 waves, rot hash(g), unroll 4")
    NWRUN(8, 8, 0, "nw: 8 waves, no rotation, unroll 8")
    NWRUN(8, 16, 0, "nw: 16 waves, no rotation, unroll 8")
    run("v0 shipped, again", c, [&] { hipLaunchKernelGGL(ingest_v0<0>, g2, dim3(64), 0, 0, ARGS, c.nchunk); }, ref, nullptr);
    {   // read-only ceiling
        hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
        for (int blocks : {2048, 8192, 32768}) {
            float tot = 0;
            for (int r = 0; r < 5; r++) {
                CK(hipEventRecord(e0, 0));
                hipLaunchKernelGGL(read_only, dim3(blocks), dim3(256), 0, 0, c.in, n_elems * 2, sink);
                CK(hipEventRecord(e1, 0)); CK(hipEventSynchronize(e1));
                float ms; CK(hipEventElapsedTime(&ms, e0, e1));
                if (r) tot += ms;
            }
            printf("read-only uint4 sum, %5d workgroups x 256          avg %8.3f ms  %7.1f GB/s\n", blocks, tot / 4, n_elems * 32.0 / (tot / 4) * 1e-6);
        }
    }
    return 0;
}
