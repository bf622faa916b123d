// Stand-alone test of cw_bits_layout.h (circom_amd/csrc): the lane map and the LDS ring of the 32-byte ingest
// (cw_bits.hip cw_bits_ingest_kernel: lane = one 16-byte piece, every line read by one instruction), replayed thread by thread on
// the CPU with the header's own index functions.  tests/test_bits_ingest_line_host.py builds it with -fsanitize=address,undefined
// and runs it: the image of a group lives in a heap block of exactly its size, so a read one piece off is an error of the run.
//   - every (instance, input) of the group contributes exactly one low and one high piece
//   - no piece is read at or beyond 2 n_in or beyond the group's last instance (an inactive lane re-reads its wave's first piece)
//   - a ring slot is read only after the wait that covers its load, holds that load when it is read, and is re-targeted only
//     after it was read (ring depths 4, 8, 16; full groups)
//   - the masks the even lanes store after the fold equal the plain definition: bit = low bit of the value, bad = value not 0 / 1
// Input counts 1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 300; groups of 1, 63, 64 instances.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../circom_amd/csrc/cw_bits_layout.h"

using namespace cwlayout;

static long n_cases = 0;
static uint32_t n_in = 0, ni = 0, depth = 0, group = 0;
#define CHECK(x)                                                        \
    do {                                                                \
        n_cases++;                                                      \
        if (!(x)) {                                                     \
            fprintf(stderr, "%s:%d: CHECK(%s) failed (n_in %u, ni %u, ring %u, group %u)\n", __FILE__, __LINE__, #x, n_in, ni, depth, group); \
            return 1;                                                   \
        }                                                               \
    } while (0)

struct Piece { uint32_t d[4]; };

// the image of one group: [ni][n_in][2 pieces].  Mostly bits; about one value in 16 is something else: 2, a high bit of dword 0,
// or a 1 in exactly one of dwords 1 .. 7 (so values that are non-zero only in the high half, or only above dword 0, occur)
static void fill(std::vector<Piece> &img) {
    for (uint32_t i = 0; i < ni; i++)
        for (uint32_t k = 0; k < n_in; k++) {
            uint64_t h = ((uint64_t)(group * 64u + i) << 32 | k) * 0x9E3779B97F4A7C15ull + 0xD1B54A32D192ED03ull;
            h ^= h >> 29; h *= 0xBF58476D1CE4E5B9ull; h ^= h >> 32;
            Piece lo = {{(uint32_t)h & 1u, 0, 0, 0}}, hi = {{0, 0, 0, 0}};
            if (((h >> 8) & 15u) == 0) {
                const uint32_t what = (uint32_t)(h >> 16) % 10u;
                if (what == 0) lo.d[0] = 2;
                else if (what == 1) lo.d[0] |= 0x80000000u;
                else if (what == 2) lo.d[0] = 3;
                else if (what < 6) lo.d[what - 2] = 1;                   // dwords 1 .. 3
                else hi.d[what - 6] = 1;                                 // dwords 4 .. 7
            }
            img[((size_t)i * n_in + k) * 2] = lo;
            img[((size_t)i * n_in + k) * 2 + 1] = hi;
        }
}

struct Lane {
    uint64_t bit[2] = {0, 0}, bad[2] = {0, 0};
};

static int take(Lane &L, uint32_t h, uint32_t lane, const Piece &v, uint32_t inst) {
    const uint32_t half = line_piece_half(lane);
    CHECK(inst < 64);
    L.bit[h] |= (uint64_t)(v.d[0] & 1u) << inst;                         // as the kernel: the odd lanes' `bit` is never stored
    L.bad[h] |= (uint64_t)line_bad(half, v.d[0], v.d[1], v.d[2], v.d[3]) << inst;
    CHECK(line_bit(half, v.d[0]) == (half ? 0u : (v.d[0] & 1u)));
    return 0;
}

// one group (its workgroups: chunks of LINE_WG_INPUTS inputs x LINE_WAVES waves), as cwk_bits_ingest forms the grid
static int replay() {
    const size_t n_pieces = (size_t)ni * n_in * 2;
    std::vector<Piece> img_v(n_pieces);
    fill(img_v);
    std::unique_ptr<Piece[]> img(new Piece[n_pieces]);                  // exactly the group's bytes
    memcpy(img.get(), img_v.data(), n_pieces * sizeof(Piece));
    std::vector<uint32_t> seen(n_pieces, 0), stored(n_in, 0);
    std::vector<uint64_t> mask(n_in, 0);
    uint64_t fbmask = 0;
    const uint32_t n_chunks = (n_in + LINE_WG_INPUTS - 1) / LINE_WG_INPUTS;
    const size_t step = (size_t)n_in * 2;
    for (uint32_t c = 0; c < n_chunks; c++)
        for (uint32_t wave = 0; wave < LINE_WAVES; wave++) {
            const uint32_t k0 = line_wave_input0(c, wave);
            if (k0 >= n_in) continue;
            Lane L[64];
            uint32_t o[64][2];
            bool act[64][2];
            for (uint32_t lane = 0; lane < 64; lane++)
                for (uint32_t h = 0; h < LINE_LOADS; h++) {
                    const uint32_t p = line_piece(k0, h, lane);
                    act[lane][h] = line_piece_active(p, n_in);
                    o[lane][h] = act[lane][h] ? p : 2u * k0;
                    CHECK(o[lane][h] < 2u * n_in);
                    if (act[lane][h]) {
                        CHECK(line_piece_input(p) == k0 + 32u * h + lane / 2u && line_piece_input(p) < n_in && line_piece_half(p) == (lane & 1u));
                    }
                }
            // a load instruction of the wave is 1 KiB contiguous: lane l + 1 takes the piece behind lane l's
            for (uint32_t h = 0; h < LINE_LOADS; h++)
                for (uint32_t lane = 1; lane < 64; lane++) CHECK(line_piece(k0, h, lane) == line_piece(k0, h, 0) + lane);
            CHECK(line_piece(k0, 1, 0) == line_piece(k0, 0, 63) + 1);
            auto mark = [&](uint32_t inst, uint32_t lane, uint32_t h) {
                if (act[lane][h]) seen[(size_t)inst * step + o[lane][h]]++;
            };
            if (ni == LINE_GROUP) {
                const uint32_t r = line_group_start(group), D = depth, BT = line_ring_batch(D), NB = LINE_RING_LOADS / BT;
                CHECK(r < 64 && LINE_RING_LOADS % D == 0 && BT * 2 == D);
                std::vector<Piece> ring((size_t)D * 64);
                std::vector<int> holds(D, -1);                           // the load a slot was last targeted with
                std::vector<bool> was_read(D, true);
                uint32_t issued = 0;
                auto dma = [&](uint32_t n) -> int {
                    const uint32_t slot = line_ring_slot(n, D), inst = line_instance(n >> 1, r), h = n & 1u;
                    CHECK(n == issued && slot < D && was_read[slot]);    // in order; the slot's previous load was read
                    CHECK(inst < ni);
                    for (uint32_t lane = 0; lane < 64; lane++) {
                        CHECK(line_ring_byte(slot, lane) + 16 <= D * LINE_SLOT_BYTES && line_ring_byte(slot, lane) % 16 == 0);
                        ring[line_ring_byte(slot, lane) / 16] = img[(size_t)inst * step + o[lane][h]];
                    }
                    holds[slot] = (int)n;
                    was_read[slot] = false;
                    issued++;
                    return 0;
                };
                for (uint32_t n = 0; n < D; n++)
                    if (dma(n)) return 1;
                for (uint32_t b = 0; b < NB; b++) {
                    // s_waitcnt vmcnt(pending): loads return in order, so the first issued - pending have landed
                    CHECK(issued == line_ring_issued(D, b));
                    const uint32_t pending = line_ring_pending(D, b);
                    CHECK(pending <= issued && issued - pending >= (b + 1) * BT && pending < 64);
                    Piece v[64][16];
                    CHECK(BT <= 16);
                    for (uint32_t j = 0; j < BT; j++) {
                        const uint32_t n = b * BT + j, slot = line_ring_slot(n, D);
                        CHECK(n < issued - pending && holds[slot] == (int)n && !was_read[slot]);
                        for (uint32_t lane = 0; lane < 64; lane++) v[lane][j] = ring[line_ring_byte(slot, lane) / 16];
                        was_read[slot] = true;
                    }
                    // (s_waitcnt lgkmcnt(0)) then the refills
                    CHECK(line_ring_refills(D, b) == ((b + 2) * BT < LINE_RING_LOADS));
                    if (line_ring_refills(D, b))
                        for (uint32_t j = 0; j < BT; j++)
                            if (dma(b * BT + j + D)) return 1;
                    for (uint32_t j = 0; j < BT; j++) {
                        const uint32_t n = b * BT + j, inst = line_instance(n >> 1, r), h = n & 1u;
                        for (uint32_t lane = 0; lane < 64; lane++) {
                            if (take(L[lane], h, lane, v[lane][j], inst)) return 1;
                            mark(inst, lane, h);
                        }
                    }
                }
                CHECK(issued == LINE_RING_LOADS);
                for (uint32_t s = 0; s < D; s++) CHECK(was_read[s]);
            } else {
                for (uint32_t ii = 0; ii < ni; ii++)
                    for (uint32_t h = 0; h < LINE_LOADS; h++)
                        for (uint32_t lane = 0; lane < 64; lane++) {
                            if (take(L[lane], h, lane, img[(size_t)ii * step + o[lane][h]], ii)) return 1;
                            mark(ii, lane, h);
                        }
            }
            // the fold and the stores
            for (uint32_t h = 0; h < LINE_LOADS; h++) {
                uint64_t bad[64];
                for (uint32_t lane = 0; lane < 64; lane++) {
                    if (!act[lane][h]) L[lane].bit[h] = L[lane].bad[h] = 0;
                    bad[lane] = L[lane].bad[h];
                }
                for (uint32_t lane = 0; lane < 64; lane++) L[lane].bad[h] = bad[lane] | bad[lane ^ 1u];
            }
            for (uint32_t lane = 0; lane < 64; lane += 2) {
                for (uint32_t h = 0; h < LINE_LOADS; h++)
                    if (act[lane][h]) {
                        const uint32_t k = line_piece_input(line_piece(k0, h, lane));
                        CHECK(k < n_in);
                        mask[k] = L[lane].bit[h];
                        stored[k]++;
                    }
                fbmask |= L[lane].bad[0] | L[lane].bad[1];
            }
            // the even lanes of a store instruction write consecutive masks
            for (uint32_t h = 0; h < LINE_LOADS; h++)
                for (uint32_t lane = 2; lane < 64; lane += 2)
                    CHECK(line_piece_input(line_piece(k0, h, lane)) == line_piece_input(line_piece(k0, h, 0)) + lane / 2u);
        }
    // coverage and the plain definition
    for (size_t a = 0; a < n_pieces; a++) CHECK(seen[a] == 1);
    uint64_t want_fb = 0;
    for (uint32_t k = 0; k < n_in; k++) {
        CHECK(stored[k] == 1);
        uint64_t want = 0;
        for (uint32_t i = 0; i < ni; i++) {
            const Piece &lo = img[((size_t)i * n_in + k) * 2], &hi = img[((size_t)i * n_in + k) * 2 + 1];
            const uint32_t rest = lo.d[1] | lo.d[2] | lo.d[3] | hi.d[0] | hi.d[1] | hi.d[2] | hi.d[3];
            want |= (uint64_t)(lo.d[0] & 1u) << i;
            want_fb |= (uint64_t)((lo.d[0] > 1u) | (rest != 0u)) << i;
        }
        CHECK(mask[k] == want);
    }
    CHECK(fbmask == want_fb);
    return 0;
}

int main() {
    const uint32_t inputs[] = {1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 300}, sizes[] = {1, 63, 64};
    static_assert(LINE_WG_INPUTS == 256 && LINE_RING_LOADS == 128 && LINE_SLOT_BYTES == 1024, "the workgroup and the ring");
    static_assert(line_ring_pending(16, 0) == 8 && line_ring_pending(16, 14) == 8 && line_ring_pending(16, 15) == 0, "the vmcnt immediates of a ring of 16");
    int shapes = 0;
    bool any_bad = false;
    for (uint32_t n : inputs)
        for (uint32_t s : sizes)
            for (uint32_t g : {0u, 1u, 37u})
                for (uint32_t d : {4u, 8u, 16u}) {
                    if (s != LINE_GROUP && d != 16u) continue;           // a ragged group does not use the ring
                    n_in = n; ni = s; group = g; depth = d;
                    if (replay()) return 1;
                    shapes++;
                }
    // the image does hold values that are not bits (the flag path is exercised)
    {
        n_in = 300; ni = 64; group = 0;
        std::vector<Piece> img((size_t)ni * n_in * 2);
        fill(img);
        for (const Piece &p : img) any_bad |= p.d[0] > 1u || p.d[1] || p.d[2] || p.d[3];
        CHECK(any_bad);
    }
    printf("bits ingest line ok: %d shapes, %ld checks\n", shapes, n_cases);
    return 0;
}
