// cw_select.h — the host part of instance lists (include/circom_amd.h): cw_select_instances* picks the instances whose status
// word matches (status & mask) == want, in ascending order, and cw_get_witnesses_at* hands out the witnesses of a LIST of
// instances, out[j][k] = entry entry0 + k of instance idx[j].  Here: the argument checks (ranges without a 32-bit wrap, the
// alignments of the device pointers), the validation of a host list, the piece arithmetic of the host form, and the geometry of
// the select kernels (cw_kernels.hip cw_select_*): count blocks of SEL_BLOCK instances, one scan over the block counts.
// No HIP in here: tests/host/select_test.cpp.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace cwsel {

constexpr uint32_t SEL_BLOCK = 2048;                 // instances per count block: 256 threads x 8 rounds of a wave's 64
constexpr uint32_t SCAN_WIDTH = 1024;                // block counts the scan's single workgroup takes per pass of its loop
constexpr uint32_t NONE = 0xFFFFFFFFu;               // *d_bad of a clean list

static inline uint32_t n_blocks(uint32_t batch) { return batch / SEL_BLOCK + (batch % SEL_BLOCK != 0); }

// nullptr, or why the call is CW_EINVAL.  Device pointers are compared, never read.
static inline const char *check_select_device(const void *d_idx, const void *d_n) {
    if (!d_idx || !d_n) return "null argument";
    if (((uintptr_t)d_idx | (uintptr_t)d_n) & 3) return "d_idx and d_n must be 4-byte aligned";
    return nullptr;
}
// the entry range (a 64-bit sum: entry0 + n may pass 2^32)
static inline const char *check_entries(uint32_t entry0, uint32_t n, uint32_t n_witness) {
    return (uint64_t)entry0 + n > n_witness ? "entry range out of the witness list" : nullptr;
}
// the device form's pointers: the image leaves in 16-byte stores (32-byte elements) or 8-byte stores; the list, its device
// length and the word are read and written as 32-bit words.  d_n_idx and d_bad may be null.
static inline const char *check_at_device(const void *d_idx, const void *d_n_idx, const void *d_out, const void *d_bad, uint32_t elem_bytes) {
    if (!d_idx || !d_out) return "null argument";
    if ((uintptr_t)d_idx & 3) return "d_idx must be 4-byte aligned";
    if ((uintptr_t)d_n_idx & 3) return "d_n_idx must be 4-byte aligned";
    if ((uintptr_t)d_out & (elem_bytes == 8 ? 7 : 15))
        return elem_bytes == 8 ? "the device image must be 8-byte aligned" : "the device image must be 16-byte aligned";
    if ((uintptr_t)d_bad & 3) return "d_bad must be 4-byte aligned";
    return nullptr;
}
// a host list: the first position whose index is not an instance of the batch, or -1.  Exactly n_idx words are read.
static inline int64_t first_bad_position(const uint32_t *idx, uint32_t n_idx, uint32_t batch) {
    for (uint32_t j = 0; j < n_idx; j++)
        if (idx[j] >= batch) return j;
    return -1;
}

// The host form stages pieces of whole rows (row = n x elem_bytes bytes of one list position) in the batch's staging buffer:
// 256 MiB worth, not more than n_idx, at least one - and, since the list of a piece is uploaded next to it, a piece of rows
// that are a few bytes each stays below 2^24 positions.
static inline uint32_t piece_rows(size_t row, uint32_t n_idx) {
    const size_t by_bytes = ((size_t)256 << 20) / std::max<size_t>(row, 1);
    return (uint32_t)std::max<size_t>(1, std::min<size_t>(std::min<size_t>(n_idx, by_bytes), (size_t)1 << 24));
}
// where piece `done` begins in the caller's image, and its bytes (64-bit arithmetic)
static inline uint8_t *piece_at(uint8_t *out, size_t row, uint32_t done) { return out + (size_t)done * row; }
static inline size_t piece_bytes(size_t row, uint32_t m) { return (size_t)m * row; }
// the staging buffer of a piece: the rows, then (4-byte aligned: a row is a multiple of 8 bytes) the piece's list
static inline size_t staging_bytes(size_t row, uint32_t per) { return (size_t)per * row + (size_t)per * 4; }

}  // namespace cwsel
