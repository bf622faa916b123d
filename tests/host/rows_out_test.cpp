// Stand-alone test of the output half of cw_rows.h (circom_amd/csrc): witness bits out as packed rows (cw_get_witness_rows*) - the
// range and word checks next to the flag / stride / alignment checks the calls share with the input side, and the copy of staged
// rows of whole 8-byte words into caller rows of any stride.  tests/test_rows_out_host.py builds it with
// -fsanitize=address,undefined and runs it: every destination lives in a heap block of exactly the bytes the header may write,
// so one byte too many is an error of the run.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "../../circom_amd/csrc/cw_rows.h"

static int n_cases = 0;
#define CHECK(x)                                                        \
    do {                                                                \
        n_cases++;                                                      \
        if (!(x)) {                                                     \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #x); \
            return 1;                                                   \
        }                                                               \
    } while (0)

// the model: bit (j, k) from a linear congruential sequence
static unsigned model_bit(size_t j, uint32_t k) { return (unsigned)(((j * 2654435761u + k * 40503u + (j ^ k)) >> 7) & 1u); }

// what a device kernel leaves in the staging buffer: rows of whole words, the entries' bits, pad bits 0
static std::vector<uint8_t> staged_rows(uint32_t n, size_t count, bool msb) {
    const size_t row = 8 * cw_rows_words(n);
    std::vector<uint8_t> s(count * row, 0);
    for (size_t j = 0; j < count; j++)
        for (uint32_t k = 0; k < n; k++)
            if (model_bit(j, k)) s[j * row + (k >> 3)] |= (uint8_t)(1u << (msb ? 7 - (k & 7) : (k & 7)));
    return s;
}

static int run() {
    // ranges: entry0 + n against the witness list, first + count against the batch, sums past 2^32
    CHECK(!cw_rows_check_range(0, 0, 0, 0, 0, 0) && !cw_rows_check_range(0, 4, 4, 0, 5, 5) && !cw_rows_check_range(4, 0, 4, 5, 0, 5));
    CHECK(!cw_rows_check_range(3, 1, 4, 4, 1, 5) && cw_rows_check_range(3, 2, 4, 0, 5, 5) && cw_rows_check_range(0, 5, 4, 0, 5, 5));
    CHECK(cw_rows_check_range(0, 4, 4, 0, 6, 5) && cw_rows_check_range(0, 4, 4, 5, 1, 5) && cw_rows_check_range(5, 0, 4, 0, 1, 5));
    CHECK(cw_rows_check_range(0xFFFFFFFFu, 2, 4, 0, 1, 5) && cw_rows_check_range(2, 0xFFFFFFFFu, 4, 0, 1, 5));
    CHECK(cw_rows_check_range(0, 1, 4, 0xFFFFFFFFu, 2, 5) && cw_rows_check_range(0, 1, 4, 2, 0xFFFFFFFFu, 5));
    CHECK(!cw_rows_check_range(0, 0xFFFFFFFFu, 0xFFFFFFFFu, 0, 0xFFFFFFFFu, 0xFFFFFFFFu));
    // the entry range is looked at first
    CHECK(cw_rows_check_range(0, 5, 4, 0, 6, 5) == cw_rows_check_range(0, 5, 4, 0, 1, 5));
    // the word: 4-byte aligned, nullptr allowed
    CHECK(!cw_rows_check_word(nullptr) && !cw_rows_check_word((const void *)4096) && !cw_rows_check_word((const void *)4100));
    CHECK(cw_rows_check_word((const void *)4097) && cw_rows_check_word((const void *)4098) && cw_rows_check_word((const void *)4099));
    // the checks shared with the input side, at the sizes of a range of n entries
    CHECK(!cw_rows_check_flags(0) && !cw_rows_check_flags(CW_ROWS_FLAG_MSB) && cw_rows_check_flags(2) && cw_rows_check_flags(0x80000001u));
    CHECK(!cw_rows_check_host(1, 7) && !cw_rows_check_host(1, 8) && cw_rows_check_host(1, 9) && !cw_rows_check_host(0, 0));
    CHECK(!cw_rows_check_device((const void *)4096, 8, 64) && cw_rows_check_device((const void *)4096, 8, 65) &&
          !cw_rows_check_device((const void *)4096, 16, 65) && cw_rows_check_device((const void *)4100, 16, 65) &&
          cw_rows_check_device((const void *)4096, 20, 65) && !cw_rows_check_device((const void *)4096, 0, 0));
    // staged rows -> caller rows: odd strides, the last row ends with its allocation, every byte of the destination that carries
    // no entry stays as it was, the spare bits of the last byte are the staged zeros; both bit orders
    for (uint32_t n : {1u, 7u, 8u, 9u, 45u, 63u, 64u, 65u, 129u}) {
        const size_t used = cw_rows_bytes(n), row = 8 * cw_rows_words(n);
        for (size_t stride : {used, used + 1, used + 3, used + 13}) {
            for (int msb = 0; msb < 2; msb++) {
                const size_t count = 67, total = (count - 1) * stride + used;
                const std::vector<uint8_t> src = staged_rows(n, count, msb);
                std::unique_ptr<uint8_t[]> dst(new uint8_t[total]);
                for (size_t i = 0; i < total; i++) dst[i] = 0xA5;
                cw_rows_scatter(src.data(), n, count, dst.get(), stride);
                bool ok = true;
                for (size_t j = 0; j < count; j++) {
                    for (uint32_t k = 0; k < n; k++) ok = ok && cw_rows_bit(dst.get() + j * stride, k, msb) == model_bit(j, k);
                    for (uint32_t k = n; k < 8 * used; k++) ok = ok && cw_rows_bit(dst.get() + j * stride, k, msb) == 0;
                    for (size_t t = used; t < stride && j * stride + t < total; t++) ok = ok && dst[j * stride + t] == 0xA5;
                    ok = ok && memcmp(dst.get() + j * stride, src.data() + j * row, used) == 0;
                }
                CHECK(ok);
            }
        }
    }
    // a piece in the middle of a larger destination: the rows in front of it and behind it stay
    {
        const uint32_t n = 45;
        const size_t used = cw_rows_bytes(n), stride = used + 3;
        const std::vector<uint8_t> src = staged_rows(n, 3, true);
        std::vector<uint8_t> dst(7 * stride, 0xA5);
        cw_rows_scatter(src.data(), n, 3, dst.data() + 2 * stride, stride);
        bool ok = true;
        for (size_t i = 0; i < dst.size(); i++) {
            const size_t j = i / stride, t = i % stride;
            if (j < 2 || j >= 5 || t >= used) ok = ok && dst[i] == 0xA5;
        }
        CHECK(ok);
    }
    // no rows, no entries: nothing is read or written
    cw_rows_scatter(nullptr, 0, 0, nullptr, 0);
    cw_rows_scatter(nullptr, 0, 5, nullptr, 3);
    std::unique_ptr<uint8_t[]> one(new uint8_t[1]);
    cw_rows_scatter(one.get(), 45, 0, one.get(), 5);
    return 0;
}

int main() {
    int rc = run();
    if (rc == 0) printf("rows out ok: %d checks\n", n_cases);
    return rc;
}
