// cw_r1cs_products.h — the host part of cw_get_r1cs_products*: the three linear forms A.w, B.w, C.w of every constraint, out as
// out[j][p][k] (instance first + j; the p-th selected part in the order A, B, C; constraint row0 + k), cw_element_bytes each.
//
// The check's own term streams do not serve: the 256-bit stream is in processing order with boolean rows folded into their
// hosts, select forms and equality rows (cw_r1cs_plan.h), the bit-plane check works on truth tables and chunks, and the 64-bit
// list has end flags but no row index.  So ONE plain plan per circuit is derived from what the loaders keep:
//   rowptr[3 n + 1]   constraint k of the .r1cs FILE (the numbering of cw_get_r1cs_first_bad and cw_explain), part p: the terms
//                     rowptr[3 k + p] .. rowptr[3 k + p + 1]
//   terms             2 words {slot, coefficient id} (256-bit table: the ids of r_coef into r_ctab; bit table: the bit-table slot
//                     and the id of the canonical coefficient in r_cctab) or 4 words {slot, 0, coefficient lo, hi} (64-bit)
// and the kernels (cw_products_kernel, cw_bits_products_kernel, cw64_products_kernel) walk it with scalar loads.
// No HIP in here: tests/host/r1cs_products_test.cpp.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "cw_pieces.h"

namespace cwprod {

constexpr uint32_t PART_A = 1u, PART_B = 2u, PART_C = 4u, PART_ALL = 7u;
constexpr uint32_t ROWS64 = 64, ROWS256 = 16;        // constraints per workgroup: 8-byte values / 32-byte values (both tables)
constexpr uint32_t GRID_Y = 65535u;                  // row tiles per launch

struct Plan {
    std::vector<uint32_t> rowptr;     // 3 n + 1
    std::vector<uint32_t> terms;      // `words` per term
    uint32_t words = 2;
    size_t n_terms() const { return terms.size() / words; }
};

static inline uint32_t n_parts(uint32_t parts) { return (parts & 1u) + ((parts >> 1) & 1u) + ((parts >> 2) & 1u); }

// nullptr, or why the call is CW_EINVAL: the part mask, then the rows, then the instances (64-bit sums: row0 + n_rows and
// first + count may pass 2^32)
static inline const char *check_range(uint32_t parts, uint32_t row0, uint32_t n_rows, uint32_t n_constraints, uint32_t first, uint32_t count,
                                      uint32_t batch) {
    if (parts == 0 || (parts & ~PART_ALL)) return "parts must be a non-empty combination of CW_R1CS_A, CW_R1CS_B, CW_R1CS_C";
    if ((uint64_t)row0 + n_rows > n_constraints) return "row range out of the constraint system";
    if ((uint64_t)first + count > batch) return "instance range out of the batch";
    return nullptr;
}
// the device image: compared, never read.  8-byte elements want 8 bytes, 32-byte elements leave in 16-byte stores
static inline const char *check_device(const void *d_out, uint32_t elem_bytes) {
    const uintptr_t mask = elem_bytes == 8 ? 7 : 15;
    if ((uintptr_t)d_out & mask) return elem_bytes == 8 ? "the device image must be 8-byte aligned" : "the device image must be 16-byte aligned";
    return nullptr;
}
// bytes of one instance of the image / of `count` of them (64-bit arithmetic)
static inline size_t instance_bytes(uint32_t parts, uint32_t n_rows, uint32_t elem_bytes) { return (size_t)n_parts(parts) * n_rows * elem_bytes; }

// The 256-bit loader's arrays are in PROCESSING order: row j of r_ptr is constraint r_orig[j] & 0x7FFFFFFF of the file (bit 31
// marks a pure equality row).  The plan is the inverse permutation applied: file order, every term as the loader stored it.
// `map` (bit tables): slot -> bit-table slot, the batch's own signal map.  An r_orig that is no permutation gives an empty plan.
static inline Plan build(const std::vector<uint32_t> &r_ptr, const std::vector<uint32_t> &r_slot, const std::vector<uint32_t> &r_id,
                         const std::vector<uint32_t> &r_orig, const std::vector<uint32_t> *map) {
    Plan p;
    const size_t n = r_orig.size();
    if (r_ptr.size() != 3 * n + 1 || r_id.size() != r_slot.size()) return p;
    std::vector<uint32_t> where(n, 0xFFFFFFFFu);                     // file index -> processing index
    for (size_t j = 0; j < n; j++) {
        const uint32_t k = r_orig[j] & 0x7FFFFFFFu;
        if (k >= n || where[k] != 0xFFFFFFFFu) return p;
        where[k] = (uint32_t)j;
    }
    p.rowptr.reserve(3 * n + 1);
    p.rowptr.push_back(0);
    p.terms.reserve(r_slot.size() * 2);
    for (size_t k = 0; k < n; k++) {
        const size_t j = where[k];
        for (int part = 0; part < 3; part++) {
            for (uint32_t t = r_ptr[3 * j + part]; t < r_ptr[3 * j + part + 1]; t++) {
                const uint32_t s = r_slot[t];
                if (map && s >= map->size()) return Plan();
                p.terms.push_back(map ? (*map)[s] : s);
                p.terms.push_back(r_id[t]);
            }
            p.rowptr.push_back((uint32_t)(p.terms.size() / 2));
        }
    }
    return p;
}

// The 64-bit loader's list: {slot, part | last term of its constraint << 2, coefficient lo, hi}, constraints in file order, parts
// in the order A, B, C.  A constraint without any term was given ONE term of coefficient 0 on the constant wire so that it closes
// a row; a lone zero coefficient is worth 0 wherever it came from and is left out.
static inline Plan build64(const std::vector<uint32_t> &terms64, uint32_t n_constraints) {
    Plan p;
    p.words = 4;
    p.rowptr.reserve((size_t)3 * n_constraints + 1);
    p.rowptr.push_back(0);
    size_t t = 0;
    const size_t nt = terms64.size() / 4;
    for (uint32_t k = 0; k < n_constraints; k++) {
        const size_t t0 = t;
        while (t < nt && !(terms64[4 * t + 1] & 4u)) t++;
        if (t == nt) return Plan();                                  // the list ends inside a constraint
        t++;
        const bool filler = t - t0 == 1 && terms64[4 * t0] == 0 && (terms64[4 * t0 + 1] & 3u) == 2 && !terms64[4 * t0 + 2] && !terms64[4 * t0 + 3];
        size_t u = t0;
        for (uint32_t part = 0; part < 3; part++) {
            for (; u < t && (terms64[4 * u + 1] & 3u) == part; u++) {
                if (filler) continue;
                p.terms.insert(p.terms.end(), {terms64[4 * u], 0u, terms64[4 * u + 2], terms64[4 * u + 3]});
            }
            p.rowptr.push_back((uint32_t)(p.terms.size() / 4));
        }
        if (u != t) return Plan();                                   // parts out of order
    }
    if (t != nt) return Plan();
    return p;
}

// The launches of one call: a workgroup takes `tile` consecutive rows, the row tiles are gridDim.y (at most 65 535), so a range
// leaves in pieces of 65 535 * tile rows: fn(offset of the piece in the range, its rows).  Sha256(2048) has 63 802 tiles of 16.
template <typename F>
static inline auto row_pieces(uint32_t n_rows, uint32_t tile, F &&fn) -> decltype(fn(uint32_t(), uint32_t())) {
    return cw_pieces(n_rows, GRID_Y * tile, fn);
}
static inline uint32_t row_tiles(uint32_t rows, uint32_t tile) { return rows / tile + (rows % tile != 0); }

// The host form stages pieces of whole instances (cw_pieces over `count`): the device image of the instances [done, done + m) of
// the call has the layout of the caller's, so the staged piece is copied to piece_at(out, ..., done) as it stands, piece_bytes of
// it.  Consecutive pieces tile the caller's image: nothing between them, nothing behind the last.
static inline uint8_t *piece_at(uint8_t *out, size_t inst_bytes, uint32_t done) { return out + (size_t)done * inst_bytes; }
static inline size_t piece_bytes(size_t inst_bytes, uint32_t m) { return (size_t)m * inst_bytes; }

}  // namespace cwprod
