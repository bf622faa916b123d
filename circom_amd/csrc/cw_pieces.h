// cw_pieces.h — the walk over `count` items in consecutive pieces of at most `per`: what a kernel launcher does with a grid
// dimension's limit (65 535 blocks, or 65 535 tiles of 64 instances) and what a bulk transfer does with its staging buffer
// (piece_rows in cw_host.cpp).  No HIP in here: tests/host/pieces_test.cpp.
#pragma once
#include <algorithm>
#include <cstdint>

// fn(offset, n) for the pieces [0, n0), [n0, n0 + n1), ... of [0, count): every n is `per` but the last, which is the
// remainder.  A non-zero return of fn ends the walk and is returned (an int for the host loops, a hipError_t for the
// launchers); count == 0 makes no call; per == 0 is taken as 1.  (The running offset is 64 bits wide: offset + per may
// pass 2^32 for a count next to it.)
template <typename F>
static inline auto cw_pieces(uint32_t count, uint32_t per, F &&fn) -> decltype(fn(uint32_t(), uint32_t())) {
    const uint64_t step = std::max<uint32_t>(per, 1);
    for (uint64_t at = 0; at < count; at += step)
        if (auto rc = fn((uint32_t)at, (uint32_t)std::min<uint64_t>(step, count - at))) return rc;
    return {};
}
