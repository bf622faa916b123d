// cw_bits_layout.h — index arithmetic of the bit table (cw_bits.hip), HIP-free: the element formula of both table layouts and the
// walk of the whole-row input writer (cw_bits_masks_to_table_rows_kernel), the lane map and the LDS ring of the 32-byte ingest
// (cw_bits_ingest_kernel).  The kernels and tests/host/bits_rows_layout_test.cpp / bits_ingest_line_test.cpp (which replay the
// writer and the ingest thread by thread on the CPU) compile these same lines.
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

// ---- the 32-byte ingest, every line read by one instruction (tools/ubench_ingest.hip `ingest_line`) -------------------------
// The walk of cw_bits_ingest_kernel (workgroup = LINE_WAVES waves on consecutive 64-input runs of one group, chunks fastest, the
// group's own first instance) with another lane map: within a wave's 2 KiB run of one instance, lane l of load h (h = 0, 1) takes
// the 16-byte piece 64 h + l of the run, the low (even piece) or high (odd piece) half of input k0 + 32 h + l / 2.  One load
// instruction is 1 KiB contiguous and every 128-byte line belongs to exactly one instruction.  Pieces are counted from the start
// of the instance's record (piece p = half p & 1 of input p >> 1); pieces at or beyond 2 n_in are inactive lanes.
// tests/host/bits_ingest_line_test.cpp replays these lines thread by thread.
constexpr uint32_t LINE_WAVES = 4, LINE_WAVE_INPUTS = 64, LINE_LOADS = 2, LINE_GROUP = 64;
constexpr uint32_t LINE_WG_INPUTS = LINE_WAVES * LINE_WAVE_INPUTS;
CW_LAYOUT_FN uint32_t line_wave_input0(uint32_t chunk, uint32_t wave) { return chunk * LINE_WG_INPUTS + wave * LINE_WAVE_INPUTS; }
CW_LAYOUT_FN uint32_t line_piece(uint32_t k0, uint32_t h, uint32_t lane) { return 2u * k0 + 64u * h + lane; }
CW_LAYOUT_FN bool line_piece_active(uint32_t piece, uint32_t n_in) { return piece < 2u * n_in; }
CW_LAYOUT_FN uint32_t line_piece_input(uint32_t piece) { return piece >> 1; }
CW_LAYOUT_FN uint32_t line_piece_half(uint32_t piece) { return piece & 1u; }
// the order of the instances: a full group starts at its own instance, a ragged last group walks 0 .. ni - 1
CW_LAYOUT_FN uint32_t line_group_start(uint32_t g) { return (g * 0x9E3779B1u) >> 26; }
CW_LAYOUT_FN uint32_t line_instance(uint32_t ii, uint32_t start) { return (ii + start) & (LINE_GROUP - 1u); }
// what one piece contributes to its lane's masks: `bit` counts on even pieces only; `bad` = the piece makes the value something
// other than 0 / 1.  The odd lane's `bad` is OR-ed into its even neighbour's after the loop.
CW_LAYOUT_FN uint32_t line_bit(uint32_t half, uint32_t x) { return half ? 0u : x & 1u; }
CW_LAYOUT_FN uint32_t line_bad(uint32_t half, uint32_t x, uint32_t y, uint32_t z, uint32_t w) {
    return (uint32_t)(x > (half ? 0u : 1u)) | (uint32_t)((y | z | w) != 0u);
}
// The LDS ring of the LDS-DMA transport (full groups only): load n = 2 ii + h of a wave (n < LINE_RING_LOADS) lands in slot n % D of
// the wave's ring of D slots of 1 KiB, lane l's piece at byte 16 l of the slot.  The wave works in batches of D / 2 loads: D loads
// are issued ahead; before batch b (loads b D/2 .. b D/2 + D/2 - 1) is read, at most line_ring_pending(D, b) of the wave's own
// loads may still be in flight (the vmcnt immediate: loads return in order); after the batch has been read, and the reads have
// returned, its slots take the loads D further on (line_ring_refills: while there are any).
constexpr uint32_t LINE_RING_LOADS = LINE_LOADS * LINE_GROUP, LINE_SLOT_BYTES = 1024;
CW_LAYOUT_FN constexpr uint32_t line_ring_slot(uint32_t n, uint32_t depth) { return n % depth; }
CW_LAYOUT_FN constexpr uint32_t line_ring_batch(uint32_t depth) { return depth / 2u; }
CW_LAYOUT_FN constexpr uint32_t line_ring_issued(uint32_t depth, uint32_t b) {           // loads issued when batch b is read
    return (b + 2u) * line_ring_batch(depth) < LINE_RING_LOADS ? (b + 2u) * line_ring_batch(depth) : LINE_RING_LOADS;
}
CW_LAYOUT_FN constexpr uint32_t line_ring_pending(uint32_t depth, uint32_t b) {
    return line_ring_issued(depth, b) - (b + 1u) * line_ring_batch(depth);
}
CW_LAYOUT_FN constexpr bool line_ring_refills(uint32_t depth, uint32_t b) { return (b + 2u) * line_ring_batch(depth) < LINE_RING_LOADS; }
CW_LAYOUT_FN constexpr uint32_t line_ring_byte(uint32_t slot, uint32_t lane) { return slot * LINE_SLOT_BYTES + lane * 16u; }

}  // namespace cwlayout
