// Stand-alone test of cw_select.h (circom_amd/csrc), the HIP-free host part of instance lists (cw_select_instances*,
// cw_get_witnesses_at*): the argument checks (entry ranges without a 32-bit wrap, the alignments of every device pointer), the
// validation of a host list, the piece arithmetic of the host form and the geometry of the select kernels.
// tests/test_select_host.py builds it with -fsanitize=address,undefined and runs it: every list lives in a heap block of exactly
// its words, so one word read too many is an error of the run.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../circom_amd/csrc/cw_pieces.h"
#include "../../circom_amd/csrc/cw_select.h"

static int n_cases = 0;
#define CHECK(x)                                                        \
    do {                                                                \
        n_cases++;                                                      \
        if (!(x)) {                                                     \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #x); \
            return 1;                                                   \
        }                                                               \
    } while (0)

// a list that ENDS where its allocation ends
static std::unique_ptr<uint32_t[]> exact_list(const std::vector<uint32_t> &v) {
    std::unique_ptr<uint32_t[]> p(new uint32_t[v.size()]);
    if (!v.empty()) memcpy(p.get(), v.data(), v.size() * 4);
    return p;
}

static int run() {
    using namespace cwsel;
    const void *A16 = (const void *)4096, *A8 = (const void *)4104, *A4 = (const void *)4100, *A2 = (const void *)4098, *A1 = (const void *)4097;
    // select, device form: both pointers, 4-byte aligned
    CHECK(!check_select_device(A4, A4) && !check_select_device(A16, A8));
    CHECK(check_select_device(nullptr, A4) && check_select_device(A4, nullptr) && check_select_device(nullptr, nullptr));
    CHECK(check_select_device(A2, A4) && check_select_device(A4, A2) && check_select_device(A1, A4) && check_select_device(A4, A1));
    // entries: entry0 + n against the witness list, sums past 2^32
    CHECK(!check_entries(0, 0, 0) && !check_entries(0, 4, 4) && !check_entries(4, 0, 4) && !check_entries(3, 1, 4) && !check_entries(1, 3, 4));
    CHECK(check_entries(3, 2, 4) && check_entries(0, 5, 4) && check_entries(5, 0, 4) && check_entries(4, 1, 4));
    CHECK(check_entries(0xFFFFFFFFu, 2, 4) && check_entries(2, 0xFFFFFFFFu, 4) && check_entries(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu));
    CHECK(!check_entries(0, 0xFFFFFFFFu, 0xFFFFFFFFu) && !check_entries(0xFFFFFFFEu, 1, 0xFFFFFFFFu) && check_entries(0xFFFFFFFEu, 2, 0xFFFFFFFFu));
    // egress, device form: list and image are needed, the count and the word are optional; 16 bytes for 32-byte elements, 8 for 8
    CHECK(!check_at_device(A4, nullptr, A16, nullptr, 32) && !check_at_device(A4, A4, A16, A4, 32) && !check_at_device(A4, A4, A8, A4, 8));
    CHECK(!check_at_device(A4, nullptr, A16, nullptr, 8));
    CHECK(check_at_device(nullptr, A4, A16, A4, 32) && check_at_device(A4, A4, nullptr, A4, 32) && check_at_device(nullptr, nullptr, nullptr, nullptr, 8));
    CHECK(check_at_device(A2, A4, A16, A4, 32) && check_at_device(A1, A4, A16, A4, 8));                  // the list
    CHECK(check_at_device(A4, A2, A16, A4, 32) && check_at_device(A4, A1, A8, A4, 8));                   // its device length
    CHECK(check_at_device(A4, A4, A8, A4, 32) && check_at_device(A4, A4, A4, A4, 32) && check_at_device(A4, A4, A2, A4, 32)); // the image, 32-byte elements
    CHECK(check_at_device(A4, A4, A4, A4, 8) && check_at_device(A4, A4, A2, A4, 8) && check_at_device(A4, A4, A1, A4, 8));    // 8-byte elements
    CHECK(check_at_device(A4, A4, A16, A2, 32) && check_at_device(A4, A4, A8, A1, 8));                   // the word
    // the list is looked at before the image, the image before the word
    CHECK(check_at_device(A2, A4, A8, A2, 32) == check_at_device(A2, A4, A16, A4, 32));
    CHECK(check_at_device(A4, A4, A8, A2, 32) == check_at_device(A4, A4, A8, A4, 32));

    // a host list: the first position that is no instance; exactly n_idx words are read (the lists end with their allocation)
    {
        auto l = exact_list({0, 4, 2, 4, 1});
        CHECK(first_bad_position(l.get(), 5, 5) == -1 && first_bad_position(l.get(), 5, 4) == 1 && first_bad_position(l.get(), 5, 2) == 1);
        CHECK(first_bad_position(l.get(), 1, 1) == -1 && first_bad_position(l.get(), 0, 0) == -1 && first_bad_position(l.get(), 5, 0) == 0);
        CHECK(first_bad_position(l.get() + 2, 3, 4) == 1 && first_bad_position(l.get() + 4, 1, 2) == -1 && first_bad_position(l.get() + 4, 1, 1) == 0);
    }
    {
        auto l = exact_list({7, 7, 7, 8});                       // the index equal to the batch at the last word of the block
        CHECK(first_bad_position(l.get(), 4, 8) == 3 && first_bad_position(l.get(), 3, 8) == -1 && first_bad_position(l.get(), 4, 9) == -1);
        auto m = exact_list({0xFFFFFFFFu});
        CHECK(first_bad_position(m.get(), 1, 0xFFFFFFFFu) == 0 && first_bad_position(m.get(), 1, 5) == 0);
        auto e = exact_list({});
        CHECK(first_bad_position(e.get(), 0, 5) == -1 && first_bad_position(nullptr, 0, 5) == -1);
    }
    {
        std::vector<uint32_t> big(100000);
        for (size_t i = 0; i < big.size(); i++) big[i] = (uint32_t)(i * 7919u % 100000u);
        auto l = exact_list(big);
        CHECK(first_bad_position(l.get(), 100000, 100000) == -1);
        l[99999] = 100000;
        CHECK(first_bad_position(l.get(), 100000, 100000) == 99999 && first_bad_position(l.get(), 99999, 100000) == -1);
        l[313] = 0x80000000u;
        CHECK(first_bad_position(l.get(), 100000, 100000) == 313);
    }

    // pieces of the host form: 256 MiB of whole rows, at least one row, never more than the list, at most 2^24 positions
    CHECK(piece_rows(32, 10) == 10 && piece_rows(32, 1) == 1 && piece_rows(0, 7) == 7);
    CHECK(piece_rows((size_t)256 << 20, 10) == 1 && piece_rows(((size_t)256 << 20) + 1, 10) == 1 && piece_rows((size_t)1 << 40, 3) == 1);
    CHECK(piece_rows((size_t)128 << 20, 10) == 2 && piece_rows((size_t)100 << 20, 10) == 2 && piece_rows(8, 0xFFFFFFFFu) == (1u << 24));
    CHECK(piece_rows(32, 0xFFFFFFFFu) == (1u << 23) && piece_rows(5017888, 2097152) == 53);
    {
        // the walk covers the list once, in order, and every piece fits the staging buffer sized for `per`
        const size_t row = 5017888;                               // the --O1 witness of the default line, 32-byte elements
        const uint32_t n_idx = 1000, per = piece_rows(row, n_idx);
        uint64_t seen = 0;
        uint32_t pieces = 0;
        uint8_t *base = (uint8_t *)0x10000;
        const int rc = cw_pieces(n_idx, per, [&](uint32_t done, uint32_t m) {
            if (done != seen || m > per || piece_bytes(row, m) + (size_t)m * 4 > staging_bytes(row, per)) return 1;
            if (piece_at(base, row, done) != base + (size_t)done * row) return 2;
            seen += m;
            pieces++;
            return 0;
        });
        CHECK(rc == 0 && seen == n_idx && pieces == (n_idx + per - 1) / per && per == 53);
    }
    // offsets past 2^32 bytes stay 64 bits wide
    CHECK(piece_at((uint8_t *)nullptr, (size_t)1 << 20, 0xFFFFFFFFu) == (uint8_t *)(((size_t)1 << 20) * 0xFFFFFFFFull));
    CHECK(piece_bytes((size_t)1 << 20, 0x10000u) == ((size_t)1 << 36) && staging_bytes(8, 1u << 24) == ((size_t)12 << 24));
    CHECK(staging_bytes(32, 3) == 108 && staging_bytes(8, 1) == 12 && (staging_bytes(8, 5) - 5 * 4) % 4 == 0);

    // the geometry of the select kernels
    CHECK(n_blocks(0) == 0 && n_blocks(1) == 1 && n_blocks(2048) == 1 && n_blocks(2049) == 2 && n_blocks(2097152) == 1024);
    CHECK(n_blocks(0xFFFFFFFFu) == (1u << 21) && n_blocks(0xFFFFF800u) == (1u << 21) - 1 && n_blocks(0xFFFFF801u) == (1u << 21));
    CHECK(SEL_BLOCK == 2048 && SCAN_WIDTH == 1024 && NONE == 0xFFFFFFFFu);
    return 0;
}

int main() {
    if (int rc = run()) return rc;
    printf("select ok: %d checks\n", n_cases);
    return 0;
}
