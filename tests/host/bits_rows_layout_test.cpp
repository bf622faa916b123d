// Stand-alone test of cw_bits_layout.h (circom_amd/csrc): the walk of the whole-row input writer of the emitted code's bit table
// (cw_bits.hip cw_bits_masks_to_table_rows_kernel), replayed thread by thread on the CPU with the header's own index functions.
// tests/test_bits_rows_layout_host.py builds it with -fsanitize=address,undefined and runs it: the masks, the LDS tile and the
// table live in heap blocks of exactly their sizes, so a read or a write one element off is an error of the run.
//   - every input row of the table, all 32 group columns of every chunk (the padding groups' columns too), is written exactly once
//   - every (group < n_groups, k < n_in) lands at the address the table formula gives and carries masks[g][k], the last group
//     masked to its live instances
//   - the padding groups' columns hold 0
//   - no address outside the input rows is written
#include <cstdio>
#include <cstdlib>
#include <memory>

#include "../../circom_amd/csrc/cw_bits_layout.h"

using namespace cwlayout;

static long n_cases = 0;
#define CHECK(x)                                                        \
    do {                                                                \
        n_cases++;                                                      \
        if (!(x)) {                                                     \
            fprintf(stderr, "%s:%d: CHECK(%s) failed (n_groups %u, n_in %u, batch %u)\n", __FILE__, __LINE__, #x, n_groups, n_in, batch); \
            return 1;                                                   \
        }                                                               \
    } while (0)

static uint64_t model_mask(uint32_t g, uint32_t k) {                     // every bit position is 1 somewhere: the top bits too
    uint64_t x = ((uint64_t)g << 32 | k) * 0x9E3779B97F4A7C15ull + 0xD1B54A32D192ED03ull;
    x ^= x >> 29;
    x *= 0xBF58476D1CE4E5B9ull;
    return (x ^ (x >> 32)) | (1ull << 63);
}

static const uint64_t UNTOUCHED = 0xA5A5A5A5A5A5A5A5ull;

// one launch of the writer: grid (chunks, ceil(n_in / 64)), 256 threads, as cwk_bits_ingest_packed forms it
static int replay(uint32_t n_groups, uint32_t n_in, uint32_t batch, uint64_t slots, uint32_t input_slot0) {
    const uint32_t chunks = (n_groups + ROWS_GROUPS - 1) / ROWS_GROUPS, ktiles = (n_in + ROWS_INPUTS - 1) / ROWS_INPUTS;
    const size_t n_masks = (size_t)n_groups * n_in, n_table = (size_t)chunks * ROWS_GROUPS * slots;
    std::unique_ptr<uint64_t[]> masks(new uint64_t[n_masks]), T(new uint64_t[n_table]), tile(new uint64_t[ROWS_LDS_BYTES / 8]);
    std::unique_ptr<uint32_t[]> written(new uint32_t[n_table]()), staged(new uint32_t[ROWS_LDS_BYTES / 8]);
    for (uint32_t g = 0; g < n_groups; g++)
        for (uint32_t k = 0; k < n_in; k++) masks[(size_t)g * n_in + k] = model_mask(g, k);
    for (size_t a = 0; a < n_table; a++) T[a] = UNTOUCHED;
    for (uint32_t chunk = 0; chunk < chunks; chunk++)
        for (uint32_t ky = 0; ky < ktiles; ky++) {
            const uint32_t k0 = ky * ROWS_INPUTS;
            for (uint32_t w = 0; w < ROWS_LDS_BYTES / 8; w++) staged[w] = 0;
            // read: global -> tile
            for (uint32_t t = 0; t < ROWS_THREADS; t++)
                for (uint32_t j = 0; j < ROWS_LOADS; j++) {
                    const RowsCell c = rows_read_cell(t, j);
                    CHECK(c.gl < ROWS_GROUPS && c.kk < ROWS_INPUTS);
                    const uint32_t g = chunk * ROWS_GROUPS + c.gl, k = k0 + c.kk;
                    uint64_t v = 0;
                    if (k < n_in) {                                     // as the kernel: a padding group loads the last real group's mask and drops it
                        v = masks[(size_t)(g < n_groups ? g : n_groups - 1u) * n_in + k];
                        v = g < n_groups ? v & rows_live_mask(batch, g) : 0;
                    }
                    CHECK(rows_tile_word(c) < ROWS_LDS_BYTES / 8);
                    tile[rows_tile_word(c)] = v;
                    staged[rows_tile_word(c)]++;
                }
            // (barrier) every cell of the 32 x 64 tile was staged once; the 65th word of a row is padding and never touched
            for (uint32_t gl = 0; gl < ROWS_GROUPS; gl++)
                for (uint32_t kk = 0; kk < ROWS_STRIDE; kk++) CHECK(staged[gl * ROWS_STRIDE + kk] == (kk < ROWS_INPUTS ? 1u : 0u));
            // write: tile -> table
            for (uint32_t t = 0; t < ROWS_THREADS; t++)
                for (uint32_t r = 0; r < ROWS_STORES; r++) {
                    const RowsCell c = rows_write_cell(t, r);
                    CHECK(c.gl < ROWS_GROUPS && c.kk < ROWS_INPUTS && staged[rows_tile_word(c)] == 1);
                    if (k0 + c.kk >= n_in) continue;
                    const size_t at = element(slots, ROWS_SH, chunk * ROWS_GROUPS + c.gl, (uint64_t)input_slot0 + k0 + c.kk);
                    CHECK(at < n_table);
                    // the formula as the emitted code reads the table: T[chunk][slot][group in chunk]
                    CHECK(at == ((((size_t)chunk * slots + input_slot0 + k0 + c.kk) << 5) + c.gl));
                    T[at] = tile[rows_tile_word(c)];
                    written[at]++;
                }
            // a store instruction of the workgroup (all threads, one r) is 2 KiB contiguous: eight consecutive rows
            if (k0 + ROWS_INPUTS <= n_in)
                for (uint32_t r = 0; r < ROWS_STORES; r++) {
                    const size_t first = element(slots, ROWS_SH, chunk * ROWS_GROUPS, (uint64_t)input_slot0 + k0 + r * 8);
                    for (uint32_t t = 0; t < ROWS_THREADS; t++) {
                        const RowsCell c = rows_write_cell(t, r);
                        CHECK(element(slots, ROWS_SH, chunk * ROWS_GROUPS + c.gl, (uint64_t)input_slot0 + k0 + c.kk) == first + t);
                    }
                }
        }
    // the table afterwards
    for (uint32_t chunk = 0; chunk < chunks; chunk++)
        for (uint64_t s = 0; s < slots; s++)
            for (uint32_t gl = 0; gl < ROWS_GROUPS; gl++) {
                const size_t at = (((size_t)chunk * slots + s) << 5) + gl;
                const uint32_t g = chunk * ROWS_GROUPS + gl;
                const bool input_row = s >= input_slot0 && s < (uint64_t)input_slot0 + n_in;
                if (!input_row) {
                    CHECK(written[at] == 0 && T[at] == UNTOUCHED);
                    continue;
                }
                CHECK(written[at] == 1);
                const uint32_t k = (uint32_t)(s - input_slot0);
                if (g >= n_groups) {
                    CHECK(T[at] == 0);
                    continue;
                }
                uint64_t want = model_mask(g, k);
                if (g == n_groups - 1 && batch - g * 64u < 64u) want &= (1ull << (batch - g * 64u)) - 1ull;
                CHECK(T[at] == want);
                CHECK(at == element(slots, ROWS_SH, g, s) && at == group_base(slots, ROWS_SH, g) + ((size_t)s << ROWS_SH));
            }
    return 0;
}

int main() {
    const uint32_t groups[] = {1, 2, 32, 34, 64}, inputs[] = {1, 63, 64, 120, 384};
    uint32_t n_groups = 0, n_in = 0, batch = 0;
    // the interpreter's layout through the same formula: a group's slots are consecutive
    CHECK(element(100, 0, 7, 5) == 705 && group_base(100, 0, 7) == 700);
    CHECK(element(100, 5, 37, 5) == ((((size_t)1 * 100 + 5) << 5) + 5));
    CHECK(rows_live_mask(64, 0) == ~0ull && rows_live_mask(69, 1) == 31 && rows_live_mask(200, 1) == ~0ull);
    int shapes = 0;
    for (uint32_t ng : groups)
        for (uint32_t ni : inputs)
            for (uint32_t last : {64u, 5u}) {                           // a full last group; a last group of 5 instances
                n_groups = ng;
                n_in = ni;
                batch = (ng - 1) * 64 + last;
                if (replay(ng, ni, batch, (uint64_t)3 + ni + 9, 3)) return 1;
                shapes++;
            }
    printf("bits rows layout ok: %d shapes, %ld checks\n", shapes, n_cases);
    return 0;
}
