// cw_compare.h — the host part of the witness compare (include/circom_amd.h, cw_compare_witnesses* / cw_compare_wtns*): an image of
// witnesses, image[j][k] = entry entry0 + k of instance first + j, is compared byte by byte with what the egress of the batch
// would write there; diff[j] = the lowest differing entry or EQUAL, summary = {instances with a difference, the lowest of them}.
// Here: the argument checks (ranges without a 32-bit wrap, the alignments of the device pointers), the piece arithmetic of the
// host form (the image of a piece, its verdict words and the summary share the batch's staging buffer) and the verdict itself as
// the CPU states it: the first differing entry of two rows, and how verdicts fold into a summary.
// No HIP in here: tests/host/compare_test.cpp.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>

namespace cwcmp {

constexpr uint32_t EQUAL = 0xFFFFFFFFu;              // diff[j] of an equal run; summary[1] when no instance differs

// nullptr, or why the call is CW_EINVAL.  64-bit sums: entry0 + n and first + count may pass 2^32.
static inline const char *check_range(uint32_t entry0, uint32_t n, uint32_t n_witness, uint32_t first, uint32_t count, uint32_t batch) {
    if ((uint64_t)entry0 + n > n_witness) return "entry range out of the witness list";
    if ((uint64_t)first + count > batch) return "instance range out of the batch";
    return nullptr;
}
// the device form's pointers, compared and never read: the image is loaded in 16-byte pieces (32-byte elements) or 8-byte
// values; the verdict words and the summary are 32-bit words.  d_summary may be null.
static inline const char *check_device(const void *d_image, const void *d_diff, const void *d_summary, uint32_t elem_bytes) {
    if ((uintptr_t)d_image & (elem_bytes == 8 ? 7 : 15))
        return elem_bytes == 8 ? "the device image must be 8-byte aligned" : "the device image must be 16-byte aligned";
    if ((uintptr_t)d_diff & 3) return "d_diff must be 4-byte aligned";
    if ((uintptr_t)d_summary & 3) return "d_summary must be 4-byte aligned";
    return nullptr;
}

// The host form stages pieces of whole rows (row = n x elem_bytes bytes of one instance): 256 MiB worth, not more than `count`,
// at least one.  Behind the rows of a piece (rounded up to 16 bytes) lie its verdict words, then the two summary words.
static inline uint32_t piece_rows(size_t row, uint32_t count) {
    const size_t by_bytes = ((size_t)256 << 20) / std::max<size_t>(row, 1);
    return (uint32_t)std::max<size_t>(1, std::min<size_t>(count, by_bytes));
}
static inline size_t diff_offset(size_t row, uint32_t per) { return ((size_t)per * row + 15) & ~(size_t)15; }
static inline size_t summary_offset(size_t row, uint32_t per) { return diff_offset(row, per) + (size_t)per * 4; }
static inline size_t staging_bytes(size_t row, uint32_t per) { return summary_offset(row, per) + 8; }
// where piece `done` begins in the caller's image (64-bit arithmetic)
static inline const uint8_t *piece_at(const uint8_t *image, size_t row, uint32_t done) { return image + (size_t)done * row; }

// The verdict of one instance: the lowest entry0 + k, k < n, at which the elem_bytes bytes of the two rows differ, or EQUAL.
// Bytes are compared; nothing is reduced.
static inline uint32_t first_diff(const uint8_t *want, const uint8_t *image, uint32_t entry0, uint32_t n, uint32_t elem_bytes) {
    for (uint32_t k = 0; k < n; k++)
        if (memcmp(want + (size_t)k * elem_bytes, image + (size_t)k * elem_bytes, elem_bytes)) return entry0 + k;
    return EQUAL;
}
// summary = {0, EQUAL}, then fold(summary, first + j, diff[j]) for every instance of the range: each instance counts once
static inline void clear(uint32_t summary[2]) { summary[0] = 0; summary[1] = EQUAL; }
static inline void fold(uint32_t summary[2], uint32_t instance, uint32_t diff) {
    if (diff == EQUAL) return;
    summary[0]++;
    summary[1] = std::min(summary[1], instance);
}
// the summaries of two disjoint ranges
static inline void merge(uint32_t summary[2], const uint32_t part[2]) {
    summary[0] += part[0];
    summary[1] = std::min(summary[1], part[1]);
}

}  // namespace cwcmp
