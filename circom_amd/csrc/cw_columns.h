// cw_columns.h — the host part of input columns (cw_set_inputs_range*, cw_set_input_column*, include/circom_amd.h): the inputs
// k0 .. k0 + n - 1 of EVERY instance from one array the caller holds per signal.  Instance j's values are the n little-endian
// unsigned integers of elem_bytes in {1, 2, 4, 8, 32} at values + j * stride; stride == 0 is the broadcast form (every instance
// takes the same n values), any other stride is at least n * elem_bytes, and nothing of a row is read behind its n values.
// Here: the argument checks, the coverage bitmap (one bit per input: which inputs a column has covered since the column state
// was opened) with its count, the widening of one value to a 32-byte cell for the staging image of a host-only batch, and the
// repacking of host rows of any stride into dense ones, which is what the device kernel reads (cw_columns.hip.h
// cw_columns_kernel).  No HIP in here: tests/host/columns_test.cpp.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

static inline bool cw_columns_width_ok(uint32_t eb) { return eb == 1 || eb == 2 || eb == 4 || eb == 8 || eb == 32; }
static inline size_t cw_columns_row_bytes(uint32_t n, uint32_t eb) { return (size_t)n * eb; }   // bytes of a row that carry values

// nullptr, or why the call is CW_EINVAL: width, then stride, then (device form) alignment.  The pointer is compared, never read.
// The device form wants d_values and a non-zero stride to be multiples of elem_bytes, and multiples of 16 for 32-byte elements
// (the kernel loads a value, or half of a 32-byte one, with one instruction); the host form takes any alignment.
static inline const char *cw_columns_check(const void *values, size_t stride, uint32_t n, uint32_t eb, bool device) {
    if (!cw_columns_width_ok(eb)) return "elem_bytes must be 1, 2, 4, 8 or 32";
    if (stride && stride < cw_columns_row_bytes(n, eb)) return "stride is shorter than the n * elem_bytes bytes of a row (0 = the broadcast form)";
    if (device) {
        const size_t a = eb == 32 ? 16 : eb;
        if ((uintptr_t)values % a) return eb == 32 ? "the device values of 32-byte elements must be 16-byte aligned" : "the device values must be aligned to elem_bytes";
        if (stride % a) return eb == 32 ? "the stride of device rows of 32-byte elements must be a multiple of 16" : "the stride of device rows must be a multiple of elem_bytes";
    }
    return nullptr;
}
// the range forms: k0 + n may pass 2^32
static inline const char *cw_columns_check_range(uint32_t k0, uint32_t n, uint32_t n_inputs) {
    return (uint64_t)k0 + n > n_inputs ? "input range out of the circuit's main inputs" : nullptr;
}

// Which inputs the columns have covered.  cover() returns how many of [k0, k0 + n) were not covered before.
struct CwColumnCover {
    std::vector<uint64_t> bits;
    uint32_t n_inputs = 0, missing = 0;
    void open(uint32_t n_in) {
        n_inputs = missing = n_in;
        bits.assign(((size_t)n_in + 63) / 64, 0);
    }
    bool covered(uint32_t k) const { return (bits[k >> 6] >> (k & 63)) & 1u; }
    uint32_t cover(uint32_t k0, uint32_t n) {
        uint32_t fresh = 0;
        for (uint64_t k = k0, end = (uint64_t)k0 + n; k < end;) {
            const uint32_t bit = (uint32_t)(k & 63);
            const uint64_t span = end - k < 64 - bit ? end - k : 64 - bit;       // the part of [k, end) inside this word
            const uint64_t mask = (span == 64 ? ~0ull : ((1ull << span) - 1)) << bit;
            uint64_t &w = bits[k >> 6];
            fresh += (uint32_t)__builtin_popcountll(mask & ~w);
            w |= mask;
            k += span;
        }
        missing -= fresh;
        return fresh;
    }
};

// one value of `eb` bytes -> the 32-byte little-endian cell of the host staging image: zero-extended, unreduced
static inline void cw_columns_widen(const uint8_t *value, uint32_t eb, uint8_t cell[32]) {
    memcpy(cell, value, eb);
    memset(cell + eb, 0, 32 - eb);
}

// `count` rows of `stride` bytes -> out[count][n * eb], dense.  Nothing of a source row is read past its n values (a row may end
// where its allocation ends).
static inline void cw_columns_repack(const uint8_t *values, size_t stride, uint32_t n, uint32_t eb, size_t count, uint8_t *out) {
    const size_t row = cw_columns_row_bytes(n, eb);
    if (!row) return;
    for (size_t j = 0; j < count; j++) memcpy(out + j * row, values + j * stride, row);
}
