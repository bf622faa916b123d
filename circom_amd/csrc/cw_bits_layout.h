// cw_bits_layout.h — index arithmetic of the bit table (cw_bits.hip), HIP-free: the element formula of both table layouts and the
// walk of the whole-row input writer (cw_bits_masks_to_table_rows_kernel).  The kernels and tests/host/bits_rows_layout_test.cpp
// (which replays the writer thread by thread on the CPU) compile these same lines.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CW_LAYOUT_FN __host__ __device__ inline
#else
#define CW_LAYOUT_FN inline
#endif

namespace cwlayout {

// Two layouts share every kernel through the shift `sh` (a launch parameter):
//   sh = 0   T[group][slot]                      the interpreter's table: a group's slots are consecutive uint64
//   sh = 5   T[chunk][slot][group in chunk]      the emitted code's table: a chunk = 32 groups = 2 048 instances, a slot of a
//                                                chunk = one 256-byte row
// The slots of group g are (1 << sh) uint64 apart, starting at element group_base(slots, sh, g).
CW_LAYOUT_FN size_t group_base(uint64_t slots, uint32_t sh, uint32_t g) {
    return (((size_t)(g >> sh) * slots) << sh) + (g & ((1u << sh) - 1u));
}
// element (group g, slot s)
CW_LAYOUT_FN size_t element(uint64_t slots, uint32_t sh, uint32_t g, uint64_t s) {
    return group_base(slots, sh, g) + ((size_t)s << sh);
}

// ---- the whole-row input writer (sh = 5 only) ------------------------------------------------------------------------------
// A workgroup of ROWS_THREADS threads owns a tile of ROWS_GROUPS groups (one chunk) x ROWS_INPUTS inputs, staged in LDS as
// tile[ROWS_GROUPS][ROWS_STRIDE] of 8-byte words.
constexpr uint32_t ROWS_SH = 5;
constexpr uint32_t ROWS_GROUPS = 32, ROWS_INPUTS = 64, ROWS_STRIDE = 65, ROWS_THREADS = 256;
constexpr uint32_t ROWS_WAVES = ROWS_THREADS / 64;
constexpr uint32_t ROWS_LOADS = ROWS_GROUPS / ROWS_WAVES;                       // loads per thread
constexpr uint32_t ROWS_STORES = ROWS_GROUPS * ROWS_INPUTS / ROWS_THREADS;      // stores per thread
constexpr uint32_t ROWS_LDS_BYTES = ROWS_GROUPS * ROWS_STRIDE * 8;
static_assert(ROWS_GROUPS == (1u << ROWS_SH) && ROWS_LOADS == 8 && ROWS_STORES == 8 && ROWS_LDS_BYTES == 16640, "the tile of the row writer");

struct RowsCell { uint32_t gl, kk; };                                           // group in the chunk, input in the tile
// read: load j of thread t takes input (t & 63) of the group (t >> 6) + 4 j: a wave's load is 64 consecutive masks of one group
CW_LAYOUT_FN RowsCell rows_read_cell(uint32_t thread, uint32_t j) { return RowsCell{(thread >> 6) + ROWS_WAVES * j, thread & 63u}; }
// write: store r of thread t takes cell r * 256 + t of the tile counted rows (inputs) first: 32 consecutive threads = one 256-byte
// row of the table, the workgroup's store instruction r = the eight rows 8 r .. 8 r + 7
CW_LAYOUT_FN RowsCell rows_write_cell(uint32_t thread, uint32_t r) {
    const uint32_t idx = r * ROWS_THREADS + thread;
    return RowsCell{idx & (ROWS_GROUPS - 1u), idx >> ROWS_SH};
}
CW_LAYOUT_FN uint32_t rows_tile_word(RowsCell c) { return c.gl * ROWS_STRIDE + c.kk; }
// the mask of a group as the table holds it: instances of the last group beyond the batch read as 0
CW_LAYOUT_FN uint64_t rows_live_mask(uint32_t batch, uint32_t g) {
    const uint32_t live = batch - g * 64u;
    return live < 64u ? (1ull << live) - 1ull : ~0ull;
}

}  // namespace cwlayout
