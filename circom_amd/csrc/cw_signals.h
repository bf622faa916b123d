// cw_signals.h — the host part of signal columns out (cw_get_signals_range*, cw_sym_find, include/circom_amd.h): the signals
// signal0 .. signal0 + n - 1 (signal ids, not witness-list positions) of the instances [first, first + count) as rows of narrow
// little-endian elements in the caller's record layout, the mirror image of the input columns (cw_columns.h).  Here: the argument
// checks in the order the header states, the scatter of dense staged rows into rows of any stride, and the one walk over a .sym
// file that cw_explain and cw_sym_find share.  No HIP in here.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace cwsig {

constexpr uint32_t NONE = 0xFFFFFFFFu;                                          // the word of a call in which every value fitted

static inline bool width_ok(uint32_t eb) { return eb == 1 || eb == 2 || eb == 4 || eb == 8 || eb == 32; }
static inline size_t row_bytes(uint32_t n, uint32_t eb) { return (size_t)n * eb; }   // the bytes of a row that are written

// nullptr, or why the call is CW_EINVAL: width, then the ranges (no 32-bit wrap), then the stride, then (device form) the
// alignments.  The pointers are compared, never read.  The device form wants d_values and stride to be multiples of elem_bytes,
// multiples of 16 for 32-byte elements (the kernels store a value, or half of a 32-byte one, with one instruction), and the word
// on a 4-byte boundary; the host form takes any alignment.
static inline const char *check(uint32_t signal0, uint32_t n, uint32_t n_signals, uint32_t first, uint32_t count, uint32_t batch,
                                const void *values, size_t stride, uint32_t eb, const void *d_word, bool device) {
    if (!width_ok(eb)) return "elem_bytes must be 1, 2, 4, 8 or 32";
    if ((uint64_t)signal0 + n > n_signals) return "signal range out of the circuit's signals";
    if ((uint64_t)first + count > batch) return "instance range out of the batch";
    if (stride < row_bytes(n, eb)) return "stride is shorter than the n * elem_bytes bytes of a row";
    if (device) {
        const size_t a = eb == 32 ? 16 : eb;
        if ((uintptr_t)values % a) return eb == 32 ? "the device values of 32-byte elements must be 16-byte aligned" : "the device values must be aligned to elem_bytes";
        if (stride % a) return eb == 32 ? "the stride of device rows of 32-byte elements must be a multiple of 16" : "the stride of device rows must be a multiple of elem_bytes";
        if ((uintptr_t)d_word & 3) return "the device word must be 4-byte aligned";
    }
    return nullptr;
}

// staged[count][n * eb], dense -> `count` rows of `stride` bytes: exactly n * eb bytes of a row are written
static inline void scatter(const uint8_t *staged, uint32_t n, uint32_t eb, size_t count, uint8_t *values, size_t stride) {
    const size_t row = row_bytes(n, eb);
    if (!row) return;
    for (size_t j = 0; j < count; j++) memcpy(values + j * stride, staged + j * row, row);
}

// The walk over the text of a .sym file (constraint_writers sym format, "id,witness,component,name" per line): fn(id, name) for
// every line that has its three commas; other lines are skipped.
template <typename F>
static inline void sym_walk(const std::vector<uint8_t> &buf, F &&fn) {
    size_t i = 0;
    while (i < buf.size()) {
        size_t e = i;
        while (e < buf.size() && buf[e] != '\n') e++;
        std::string line((const char *)buf.data() + i, e - i);
        i = e + 1;
        size_t c1 = line.find(','), c2 = line.find(',', c1 + 1), c3 = line.find(',', c2 + 1);
        if (c1 == std::string::npos || c2 == std::string::npos || c3 == std::string::npos) continue;
        fn(strtoul(line.c_str(), nullptr, 10), line.substr(c3 + 1));
    }
}
// does the line's name belong to `name`: the name itself, an element name[..] or a member name.x
static inline bool sym_matches(const std::string &line_name, const std::string &name) {
    if (line_name.compare(0, name.size(), name) != 0) return false;
    return line_name.size() == name.size() || line_name[name.size()] == '[' || line_name[name.size()] == '.';
}
// The ids of the matching lines: *lo = the lowest, *n = how many (distinct), *gap = 0 or the first id above *lo that is missing
// from the run although a higher one matched.  false: nothing matched.
static inline bool sym_find(const std::vector<uint8_t> &buf, const std::string &name, uint32_t *lo, uint32_t *n, uint64_t *gap) {
    std::vector<unsigned long> ids;
    sym_walk(buf, [&](unsigned long id, const std::string &nm) {
        if (sym_matches(nm, name)) ids.push_back(id);
    });
    if (ids.empty()) return false;
    std::sort(ids.begin(), ids.end());
    ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
    *lo = (uint32_t)ids[0];
    *n = (uint32_t)ids.size();
    *gap = 0;
    for (size_t k = 1; k < ids.size(); k++)
        if (ids[k] != ids[k - 1] + 1) {
            *gap = (uint64_t)ids[k - 1] + 1;
            break;
        }
    return true;
}

}  // namespace cwsig
