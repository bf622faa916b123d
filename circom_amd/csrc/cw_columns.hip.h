// cw_columns.hip.h — the device part of input columns (cw_set_inputs_range*, cw_set_input_column*; host part: cw_columns.h).
// Source rows with a stride and an element of W bytes become runs of n x EB bytes inside the rows of n_inputs x EB bytes of the
// batch's own bulk image d_in: a strided copy that widens.  EB is the image's element: 32 bytes for the 256-bit schedule and
// the bit-plane batches (instantiated in cw_kernels.hip, values taken as they stand), 8 bytes for the 64-bit runtime
// (instantiated in cw64.hip, beside the reduction it reuses: R::wrap for an 8-byte value, R::reduce4 for a 32-byte one).
//
//   index   one flat index t over count x (pieces of a run), the index of cw_rows_expand_kernel: j = t / pieces, p = t - j * pieces -
//           the only division.  A piece is 16 bytes of the destination for EB = 32 (two lanes per value: lane 2 k holds words
//           0..3, lane 2 k + 1 words 4..7 of value k) and one 8-byte value for EB = 8.  Consecutive lanes hold consecutive pieces
//           of one instance's run, so a wave's store is 1 KiB (512 bytes for EB = 8) of contiguous bytes wherever n allows, and
//           runs of several instances share a wave when n is small - each lane then lies in its own instance's row.
//   loads   W = 32 -> EB = 32: the lane's own 16 bytes, 1 KiB contiguous per wave.  W <= 8 -> EB = 32: the even lane loads the
//           value (one instruction of W bytes), the odd lane stores zeros.  EB = 8: one lane per value, W bytes (32: two
//           16-byte loads) each, contiguous over the wave.  Nothing of a row is read behind its n values.
//   offsets 64 bits throughout: j * stride and j * dst_stride pass 2^32 at the benchmark's batch.
//   stride  0 is the broadcast form: every instance reads the same n values; the address depends on the lane's piece alone, so
//           the waves that follow the first find their n x W bytes in the cache.
//   grid    one dimension, at most 2^20 workgroups, grid-stride beyond; nothing depends on n or count without that bound.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define CW_COLUMNS_BLOCK 256

// EB = 32: the values are canonical by the rule of cw_set_inputs (reduced by the caller); nothing is reduced here
struct CwColumnsAsIs {
    static __device__ __forceinline__ uint64_t wrap(uint64_t v) { return v; }
    static __device__ __forceinline__ uint64_t reduce4(uint64_t w0, uint64_t, uint64_t, uint64_t) { return w0; }
};

template <int W>
__device__ __forceinline__ uint64_t cw_columns_load(const uint8_t *p) {
    if (W == 1) return *p;
    if (W == 2) return *(const uint16_t *)p;
    if (W == 4) return *(const uint32_t *)p;
    return *(const uint64_t *)p;
}

template <int W, int EB, typename R>
__global__ void __launch_bounds__(CW_COLUMNS_BLOCK) cw_columns_kernel(const uint8_t *__restrict__ src, size_t stride, uint32_t n, uint32_t count,
                                                                      uint8_t *__restrict__ dst, size_t dst_stride) {
    static_assert((W == 1 || W == 2 || W == 4 || W == 8 || W == 32) && (EB == 8 || EB == 32), "element widths");
    constexpr uint32_t PIECE = EB == 32 ? 16 : 8;
    const uint64_t pieces = (uint64_t)n * (EB / PIECE), total = (uint64_t)count * pieces;
    for (uint64_t t = (uint64_t)blockIdx.x * CW_COLUMNS_BLOCK + threadIdx.x; t < total; t += (uint64_t)gridDim.x * CW_COLUMNS_BLOCK) {
        const uint64_t j = t / pieces, p = t - j * pieces;
        const uint8_t *row = src + j * stride;
        uint8_t *out = dst + j * dst_stride + p * PIECE;
        if (EB == 32) {
            uint4 v = make_uint4(0, 0, 0, 0);
            if (W == 32)
                v = *(const uint4 *)(row + p * 16);
            else if (!(p & 1)) {
                const uint64_t x = cw_columns_load<W>(row + (p >> 1) * W);
                v.x = (uint32_t)x;
                v.y = (uint32_t)(x >> 32);
            }
            *(uint4 *)out = v;
        } else {
            uint64_t r;
            if (W == 32) {
                const uint4 a = *(const uint4 *)(row + p * 32), b = *(const uint4 *)(row + p * 32 + 16);
                r = R::reduce4(((uint64_t)a.y << 32) | a.x, ((uint64_t)a.w << 32) | a.z, ((uint64_t)b.y << 32) | b.x, ((uint64_t)b.w << 32) | b.z);
            } else {
                r = cw_columns_load<W>(row + p * W);
                if (W == 8) r = R::wrap(r);
            }
            *(uint64_t *)out = r;
        }
    }
}

// One launch: src (aligned to W, 16 for W = 32; so is a non-zero stride) -> dst (aligned to 16 / 8, so is dst_stride), `count`
// instances.  The caller has checked the widths and alignments (cw_columns.h); hipErrorInvalidValue for what it must not send.
template <int EB, typename R>
static hipError_t cw_columns_launch(hipStream_t s, const void *src, size_t stride, uint32_t n, uint32_t count, uint32_t w, void *dst,
                                    size_t dst_stride) {
    const size_t a = w == 32 ? 16 : w, da = EB == 32 ? 16 : 8;
    if (!(w == 1 || w == 2 || w == 4 || w == 8 || w == 32)) return hipErrorInvalidValue;
    if ((uintptr_t)src % a || stride % a || (stride && stride < (size_t)n * w)) return hipErrorInvalidValue;
    if ((uintptr_t)dst % da || dst_stride % da || dst_stride < (size_t)n * EB) return hipErrorInvalidValue;
    const uint64_t total = (uint64_t)count * n * (EB == 32 ? 2 : 1);
    if (!total) return hipSuccess;
    const uint64_t need = (total + CW_COLUMNS_BLOCK - 1) / CW_COLUMNS_BLOCK;
    const dim3 grid(need < (1u << 20) ? (uint32_t)need : 1u << 20), block(CW_COLUMNS_BLOCK);     // grid-stride beyond that
    const uint8_t *in = (const uint8_t *)src;
    uint8_t *out = (uint8_t *)dst;
    switch (w) {
    case 1: hipLaunchKernelGGL((cw_columns_kernel<1, EB, R>), grid, block, 0, s, in, stride, n, count, out, dst_stride); break;
    case 2: hipLaunchKernelGGL((cw_columns_kernel<2, EB, R>), grid, block, 0, s, in, stride, n, count, out, dst_stride); break;
    case 4: hipLaunchKernelGGL((cw_columns_kernel<4, EB, R>), grid, block, 0, s, in, stride, n, count, out, dst_stride); break;
    case 8: hipLaunchKernelGGL((cw_columns_kernel<8, EB, R>), grid, block, 0, s, in, stride, n, count, out, dst_stride); break;
    default: hipLaunchKernelGGL((cw_columns_kernel<32, EB, R>), grid, block, 0, s, in, stride, n, count, out, dst_stride); break;
    }
    return hipGetLastError();
}
