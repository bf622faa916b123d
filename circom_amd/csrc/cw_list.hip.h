// cw_list.hip.h - the length of an instance list as the by-index egress kernels of the three tables see it (cw64.hip
// cw64_egress_kernel, cw_kernels.hip cw_gather_many_kernel, cw_bits.hip cw_bits_gather_kernel, each with AT = true).
#pragma once
#include <stdint.h>

// A launch holds `count` list positions, its first being position pos0 of the caller's list.  With d_n the list ends at *d_n
// (a count the device made, cw_select_instances_device): the launch then holds min(count, *d_n - pos0) positions, none when the
// list ends before pos0.  Wave-uniform: a scalar load.
__device__ __forceinline__ uint32_t cw_list_limit(uint32_t count, uint32_t pos0, const uint32_t *__restrict__ d_n) {
    if (!d_n) return count;
    const uint32_t dn = *d_n, left = dn > pos0 ? dn - pos0 : 0u;
    return left < count ? left : count;
}
