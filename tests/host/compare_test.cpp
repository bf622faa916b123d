// Stand-alone test of cw_compare.h (circom_amd/csrc), the HIP-free host part of the witness compare (cw_compare_witnesses*,
// cw_compare_wtns*): the argument checks (ranges without a 32-bit wrap, the alignments of every device pointer), the piece
// arithmetic of the host form (rows, verdict words and summary in one staging buffer) and the CPU statement of the verdict - the
// first differing entry of two rows - with the fold into a summary.
// tests/test_compare_host.py builds it with -fsanitize=address,undefined and runs it: every row lives in a heap block of exactly
// its bytes, so one byte read too many is an error of the run.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../../circom_amd/csrc/cw_pieces.h"
#include "../../circom_amd/csrc/cw_compare.h"

static int n_cases = 0;
#define CHECK(x)                                                        \
    do {                                                                \
        n_cases++;                                                      \
        if (!(x)) {                                                     \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #x); \
            return 1;                                                   \
        }                                                               \
    } while (0)

// a row that ENDS where its allocation ends
static std::unique_ptr<uint8_t[]> exact_row(const std::vector<uint8_t> &v) {
    std::unique_ptr<uint8_t[]> p(new uint8_t[v.size()]);
    if (!v.empty()) memcpy(p.get(), v.data(), v.size());
    return p;
}

static int run() {
    using namespace cwcmp;
    const void *A16 = (const void *)4096, *A8 = (const void *)4104, *A4 = (const void *)4100, *A2 = (const void *)4098, *A1 = (const void *)4097;
    // ranges: entry0 + n against the witness list, first + count against the batch, sums past 2^32; the entries are looked at first
    CHECK(!check_range(0, 0, 0, 0, 0, 0) && !check_range(0, 4, 4, 0, 300, 300) && !check_range(4, 0, 4, 300, 0, 300) && !check_range(3, 1, 4, 299, 1, 300));
    CHECK(check_range(3, 2, 4, 0, 1, 1) && check_range(0, 5, 4, 0, 1, 1) && check_range(5, 0, 4, 0, 1, 1));
    CHECK(check_range(0, 4, 4, 0, 2, 1) && check_range(0, 4, 4, 1, 1, 1) && check_range(0, 4, 4, 2, 0, 1));
    CHECK(check_range(0xFFFFFFFFu, 2, 4, 0, 1, 1) && check_range(2, 0xFFFFFFFFu, 4, 0, 1, 1) && check_range(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0, 0, 0));
    CHECK(check_range(0, 4, 4, 0xFFFFFFFFu, 2, 300) && check_range(0, 4, 4, 2, 0xFFFFFFFFu, 300) && check_range(0, 0, 0, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu));
    CHECK(!check_range(0, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFEu, 1, 0xFFFFFFFFu) && check_range(0xFFFFFFFEu, 2, 0xFFFFFFFFu, 0, 0, 0));
    CHECK(check_range(5, 0, 4, 2, 0, 1) == check_range(5, 0, 4, 0, 0, 1) && check_range(5, 0, 4, 2, 0, 1) != check_range(0, 4, 4, 2, 0, 1));
    // device pointers: 16 bytes for 32-byte elements, 8 for 8; the words on 4; the summary is optional
    CHECK(!check_device(A16, A4, nullptr, 32) && !check_device(A16, A4, A4, 32) && !check_device(A8, A4, A4, 8) && !check_device(A16, A16, A8, 8));
    CHECK(check_device(A8, A4, A4, 32) && check_device(A4, A4, A4, 32) && check_device(A2, A4, A4, 32) && check_device(A1, A4, A4, 32));
    CHECK(check_device(A4, A4, A4, 8) && check_device(A2, A4, A4, 8) && check_device(A1, A4, A4, 8));
    CHECK(check_device(A16, A2, A4, 32) && check_device(A16, A1, A4, 32) && check_device(A8, A2, nullptr, 8));
    CHECK(check_device(A16, A4, A2, 32) && check_device(A16, A4, A1, 32) && check_device(A8, A4, A2, 8));
    // the image is looked at before the verdict words, those before the summary
    CHECK(check_device(A8, A2, A2, 32) == check_device(A8, A4, A4, 32) && check_device(A16, A2, A2, 32) == check_device(A16, A2, A4, 32));

    // pieces of the host form: 256 MiB of whole rows, at least one row, never more than the range
    CHECK(piece_rows(32, 10) == 10 && piece_rows(32, 1) == 1 && piece_rows(0, 7) == 7);
    CHECK(piece_rows((size_t)256 << 20, 10) == 1 && piece_rows(((size_t)256 << 20) + 1, 10) == 1 && piece_rows((size_t)1 << 40, 3) == 1);
    CHECK(piece_rows((size_t)128 << 20, 10) == 2 && piece_rows(32, 0xFFFFFFFFu) == (1u << 23) && piece_rows(5017888, 2097152) == 53);
    // the staging buffer: rows, then (16-byte aligned) the verdict words, then the summary
    CHECK(diff_offset(32, 3) == 96 && summary_offset(32, 3) == 108 && staging_bytes(32, 3) == 116);
    CHECK(diff_offset(8, 1) == 16 && summary_offset(8, 1) == 20 && staging_bytes(8, 1) == 28);
    CHECK(diff_offset(24, 5) == 128 && diff_offset(0, 5) == 0 && staging_bytes(0, 5) == 28);
    CHECK(diff_offset((size_t)1 << 20, 0x10000u) == ((size_t)1 << 36) && summary_offset(8, 1u << 24) == ((size_t)12 << 24));
    {
        // the walk covers the range once, in order, and every piece fits the staging buffer sized for `per`
        const size_t row = 5017888;                               // the --O1 witness of the default line, 32-byte elements
        const uint32_t count = 1000, per = piece_rows(row, count);
        uint64_t seen = 0;
        uint32_t pieces = 0;
        const uint8_t *base = (const uint8_t *)0x10000;
        const int rc = cw_pieces(count, per, [&](uint32_t done, uint32_t m) {
            if (done != seen || m > per || (size_t)m * row > diff_offset(row, per)) return 1;
            if (diff_offset(row, per) % 16 || summary_offset(row, per) - diff_offset(row, per) < (size_t)m * 4) return 2;
            if (piece_at(base, row, done) != base + (size_t)done * row) return 3;
            seen += m;
            pieces++;
            return 0;
        });
        CHECK(rc == 0 && seen == count && pieces == (count + per - 1) / per && per == 53);
    }
    CHECK(piece_at((const uint8_t *)nullptr, (size_t)1 << 20, 0xFFFFFFFFu) == (const uint8_t *)(((size_t)1 << 20) * 0xFFFFFFFFull));

    // the verdict: the first differing entry of two rows, bytes compared; exactly n * eb bytes of each row are read
    for (uint32_t eb : {8u, 32u}) {
        const uint32_t n = 70;
        std::vector<uint8_t> v((size_t)n * eb);
        for (size_t i = 0; i < v.size(); i++) v[i] = (uint8_t)(i * 131u + 7u);
        auto want = exact_row(v);
        {
            auto img = exact_row(v);
            CHECK(first_diff(want.get(), img.get(), 0, n, eb) == EQUAL && first_diff(want.get(), img.get(), 5, n, eb) == EQUAL);
            CHECK(first_diff(want.get(), img.get(), 0, 0, eb) == EQUAL && first_diff(nullptr, nullptr, 9, 0, eb) == EQUAL);
        }
        for (uint32_t k : {0u, 15u, 16u, 63u, 64u, n - 1})
            for (uint32_t byte : {0u, eb / 2 - 1, eb / 2, eb - 1}) {
                auto img = exact_row(v);
                img[(size_t)k * eb + byte] ^= 0x80;
                CHECK(first_diff(want.get(), img.get(), 0, n, eb) == k && first_diff(want.get(), img.get(), 3, n, eb) == 3 + k);
                CHECK(first_diff(want.get(), img.get(), 0, k, eb) == EQUAL && first_diff(want.get(), img.get(), 0, k + 1, eb) == k);
                // a range that begins behind the tamper does not see it
                if (k + 1 < n)
                    CHECK(first_diff(want.get() + (size_t)(k + 1) * eb, img.get() + (size_t)(k + 1) * eb, k + 1, n - k - 1, eb) == EQUAL);
            }
        {
            // several tampers: the lowest entry, whatever the order of the writes
            auto img = exact_row(v);
            img[(size_t)40 * eb + 1] ^= 1;
            img[(size_t)3 * eb + eb - 1] ^= 1;
            CHECK(first_diff(want.get(), img.get(), 0, n, eb) == 3);
            auto img2 = exact_row(v);
            img2[(size_t)3 * eb + eb - 1] ^= 1;
            img2[(size_t)40 * eb + 1] ^= 1;
            CHECK(first_diff(want.get(), img2.get(), 0, n, eb) == 3 && first_diff(want.get(), img2.get(), 10, n, eb) == 13);
        }
        {
            // an image that differs in every element
            std::vector<uint8_t> w(v);
            for (uint32_t k = 0; k < n; k++) w[(size_t)k * eb] ^= 1;
            auto img = exact_row(w);
            CHECK(first_diff(want.get(), img.get(), 17, n, eb) == 17);
        }
    }
    {
        // nothing is repaired: v + q is not v (here q = 2^64 - 2^32 + 1, v = 5, 32-byte elements), a bit is 0 or 1 and nothing else
        uint8_t a[32] = {5}, b2[32] = {6, 0, 0, 0, 0xFF, 0xFF, 0xFF, 0xFF, 0}, one[32] = {1}, two[32] = {2}, high[32] = {1};
        high[31] = 1;
        CHECK(first_diff(a, b2, 0, 1, 32) == 0 && first_diff(one, two, 7, 1, 32) == 7 && first_diff(one, high, 0, 1, 32) == 0);
        CHECK(first_diff(a, a, 0, 1, 32) == EQUAL);
    }

    // the summary: every instance that differs counts once; the lowest of them
    {
        uint32_t s[2] = {77, 77};
        clear(s);
        CHECK(s[0] == 0 && s[1] == EQUAL);
        fold(s, 37, EQUAL);
        CHECK(s[0] == 0 && s[1] == EQUAL);
        fold(s, 90, 3);
        fold(s, 38, 0);
        fold(s, 39, EQUAL);
        fold(s, 237, 0xFFFFFFFEu);
        CHECK(s[0] == 3 && s[1] == 38);
        uint32_t t[2], u[2] = {2, 5};
        clear(t);
        merge(t, s);
        CHECK(t[0] == 3 && t[1] == 38);
        merge(t, u);
        CHECK(t[0] == 5 && t[1] == 5);
        uint32_t none[2];
        clear(none);
        merge(t, none);
        CHECK(t[0] == 5 && t[1] == 5 && EQUAL == 0xFFFFFFFFu);
    }
    return 0;
}

int main() {
    if (int rc = run()) return rc;
    printf("compare ok: %d checks\n", n_cases);
    return 0;
}
