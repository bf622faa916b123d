// cw_rows.h — the host part of boolean inputs as packed rows (cw_set_inputs_rows*, include/circom_amd.h): instance j's inputs are
// the first ceil(n_in / 8) bytes of rows + j * stride, input k is bit k & 7 of byte k >> 3, or bit 7 - (k & 7) with
// CW_ROWS_MSB_FIRST (the order of np.unpackbits, and the order in which circomlib's SHA-256 reads a message).  Here: the bit of
// input k, the checks of flags, stride and alignment, and the repacking of host rows of any stride into rows of whole 8-byte
// words, which is what the device kernels read (cw_bits.hip cw_bits_rows_to_masks_kernel, cw_kernels.hip cw_rows_expand_kernel).
// No HIP in here: tests/host/rows_test.cpp.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

#define CW_ROWS_FLAG_MSB 1u                            // = CW_ROWS_MSB_FIRST (cw_host.cpp asserts it)

static inline size_t cw_rows_bytes(uint32_t n_in) { return ((size_t)n_in + 7) / 8; }    // bytes of a row that carry inputs
static inline size_t cw_rows_words(uint32_t n_in) { return ((size_t)n_in + 63) / 64; }  // 8-byte words the device form reads per row

static inline unsigned cw_rows_bit(const uint8_t *row, uint32_t k, bool msb) {
    return (row[k >> 3] >> (msb ? 7u - (k & 7u) : (k & 7u))) & 1u;
}

// nullptr, or why the call is CW_EINVAL.  The device pointer is compared, never read.
static inline const char *cw_rows_check_flags(uint32_t flags) {
    return flags & ~CW_ROWS_FLAG_MSB ? "unknown flag bit (CW_ROWS_MSB_FIRST is the only one)" : nullptr;
}
static inline const char *cw_rows_check_host(size_t stride, uint32_t n_in) {
    return stride < cw_rows_bytes(n_in) ? "stride is shorter than the ceil(n_inputs / 8) bytes of a row" : nullptr;
}
static inline const char *cw_rows_check_device(const void *d_rows, size_t stride, uint32_t n_in) {
    if ((uintptr_t)d_rows & 7) return "the device rows must be 8-byte aligned";
    if (stride & 7) return "the stride of device rows must be a multiple of 8";
    if (stride < 8 * cw_rows_words(n_in)) return "the stride of device rows is shorter than 8 * ceil(n_inputs / 64): the last word of a row must lie inside it";
    return nullptr;
}

// `count` rows of `stride` bytes -> out[count][8 * cw_rows_words(n_in)]: the ceil(n_in / 8) bytes that carry inputs, then zeros up
// to the word.  Nothing of a source row is read past those bytes (a row may end where its allocation ends); the bits of the last
// byte past n_in are copied as they are - every consumer ignores them.
static inline void cw_rows_repack(const uint8_t *rows, size_t stride, uint32_t n_in, size_t count, uint8_t *out) {
    const size_t used = cw_rows_bytes(n_in), row = 8 * cw_rows_words(n_in);
    for (size_t j = 0; j < count; j++) {
        memcpy(out + j * row, rows + j * stride, used);
        memset(out + j * row + used, 0, row - used);
    }
}

// ---- witness bits OUT as packed rows (cw_get_witness_rows*) ----
// The same row layout for results: entry entry0 + k of the witness list is bit k & 7 (msb: 7 - (k & 7)) of byte k >> 3 of row j,
// 1 if and only if the value is 1.  The device kernels write rows of whole 8-byte words with zero pad bits; the host form copies
// the ceil(n / 8) bytes that carry entries out of those into the caller's rows.
// nullptr, or why the call is CW_EINVAL (64-bit sums: entry0 + n and first + count may pass 2^32).
static inline const char *cw_rows_check_range(uint32_t entry0, uint32_t n, uint32_t n_witness, uint32_t first, uint32_t count, uint32_t batch) {
    if ((uint64_t)entry0 + n > n_witness) return "entry range out of the witness list";
    if ((uint64_t)first + count > batch) return "instance range out of the batch";
    return nullptr;
}
// the word that reports a value which is not 0 or 1: compared, never read; nullptr is allowed
static inline const char *cw_rows_check_word(const void *d_word) {
    return (uintptr_t)d_word & 3 ? "the device word must be 4-byte aligned" : nullptr;
}
// staged[count][8 * cw_rows_words(n)] -> `count` caller rows of `stride` bytes: exactly ceil(n / 8) bytes of each row are written,
// every other byte of `rows` stays as it was (a row may end where its allocation ends)
static inline void cw_rows_scatter(const uint8_t *staged, uint32_t n, size_t count, uint8_t *rows, size_t stride) {
    const size_t used = cw_rows_bytes(n), row = 8 * cw_rows_words(n);
    if (!used) return;
    for (size_t j = 0; j < count; j++) memcpy(rows + j * stride, staged + j * row, used);
}
