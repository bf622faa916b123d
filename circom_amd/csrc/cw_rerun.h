// cw_rerun.h — the walk over the re-run instances of a bit-plane batch.  `fb_inst` lists, in ascending order, the instances
// the 256-bit side batch holds: position k of the side batch is instance fb_inst[k].  Consecutive instances sit at consecutive
// positions, so a maximal run of them leaves the side batch in ONE bulk call.  No HIP in here: tests/host/rerun_test.cpp.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

// For every maximal run of consecutive instances, clipped to the window [first, first + count): fn(pos, len, off) with the
// side-batch position of the run's first instance inside the window, the number of instances, and the offset of that instance
// from `first`.  A non-zero return of fn ends the walk and is returned.  (64-bit sums: first + count may be 2^32.)
template <typename F>
static inline int cw_rerun_runs(const std::vector<uint32_t> &fb_inst, uint32_t first, uint32_t count, F &&fn) {
    const uint64_t end = (uint64_t)first + count;
    for (size_t k = 0; k < fb_inst.size();) {
        size_t e = k + 1;
        while (e < fb_inst.size() && fb_inst[e] == fb_inst[e - 1] + 1) e++;
        const uint64_t lo = std::max<uint64_t>(fb_inst[k], first), hi = std::min<uint64_t>((uint64_t)fb_inst[e - 1] + 1, end);
        if (lo < hi)
            if (int rc = fn((uint32_t)(k + (lo - fb_inst[k])), (uint32_t)(hi - lo), (uint32_t)(lo - first))) return rc;
        k = e;
    }
    return 0;
}
