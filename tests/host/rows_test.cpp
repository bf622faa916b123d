// Stand-alone test of cw_rows.h (circom_amd/csrc): boolean inputs as packed rows - the bit of input k in both bit orders, the
// checks of flags, stride and alignment, and the repacking of host rows of any stride into rows of whole 8-byte words.
// tests/test_rows_host.py builds it with -fsanitize=address,undefined and runs it: every source row lives in a heap block of
// exactly the bytes the header may read, so one byte too many is an error of the run.
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

// the model: the bits of `count` instances, bit (j, k) from a linear congruential sequence
static unsigned model_bit(size_t j, uint32_t k) { return (unsigned)(((j * 2654435761u + k * 40503u + (j ^ k)) >> 7) & 1u); }

// rows of `stride` bytes in a block of exactly (count - 1) * stride + ceil(n / 8) bytes: the last row ends with the allocation;
// pad bytes and the spare bits of the last byte are all ones
static std::unique_ptr<uint8_t[]> make_rows(uint32_t n, size_t count, size_t stride, bool msb) {
    const size_t used = cw_rows_bytes(n), total = count ? (count - 1) * stride + used : 0;
    std::unique_ptr<uint8_t[]> p(new uint8_t[total ? total : 1]);
    for (size_t i = 0; i < total; i++) p[i] = 0xFF;
    for (size_t j = 0; j < count; j++)
        for (uint32_t k = 0; k < n; k++)
            if (!model_bit(j, k)) p[j * stride + (k >> 3)] &= (uint8_t)~(1u << (msb ? 7 - (k & 7) : (k & 7)));
    return p;
}

static int run() {
    // sizes
    CHECK(cw_rows_bytes(0) == 0 && cw_rows_bytes(1) == 1 && cw_rows_bytes(8) == 1 && cw_rows_bytes(9) == 2 && cw_rows_bytes(45) == 6);
    CHECK(cw_rows_words(0) == 0 && cw_rows_words(1) == 1 && cw_rows_words(64) == 1 && cw_rows_words(65) == 2 && cw_rows_words(129) == 3);
    CHECK(cw_rows_bytes(0xFFFFFFFFu) == 0x20000000u && cw_rows_words(0xFFFFFFFFu) == 0x4000000u);
    // the bit of input k for both orders, at k = 0, 7, 8, 63, 64, n - 1, each alone in an otherwise clear / set row
    for (uint32_t n : {66u, 129u, 2048u}) {
        for (uint32_t k : {0u, 7u, 8u, 63u, 64u, n - 1}) {
            for (int msb = 0; msb < 2; msb++) {
                std::vector<uint8_t> row(cw_rows_bytes(n), 0);
                row[k >> 3] = (uint8_t)(1u << (msb ? 7 - (k & 7) : (k & 7)));
                bool only = true;
                for (uint32_t t = 0; t < n; t++) only = only && cw_rows_bit(row.data(), t, msb) == (t == k ? 1u : 0u);
                CHECK(only);
                for (uint8_t &x : row) x = (uint8_t)~x;
                only = true;
                for (uint32_t t = 0; t < n; t++) only = only && cw_rows_bit(row.data(), t, msb) == (t == k ? 0u : 1u);
                CHECK(only);
            }
        }
    }
    // the two orders name the ends of a byte
    const uint8_t b80 = 0x80, b01 = 0x01;
    CHECK(cw_rows_bit(&b80, 0, true) == 1 && cw_rows_bit(&b80, 7, false) == 1 && cw_rows_bit(&b80, 0, false) == 0);
    CHECK(cw_rows_bit(&b01, 7, true) == 1 && cw_rows_bit(&b01, 0, false) == 1 && cw_rows_bit(&b01, 0, true) == 0);
    // checks
    CHECK(!cw_rows_check_flags(0) && !cw_rows_check_flags(CW_ROWS_FLAG_MSB) && cw_rows_check_flags(2) && cw_rows_check_flags(3) &&
          cw_rows_check_flags(0x80000000u));
    CHECK(!cw_rows_check_host(6, 45) && cw_rows_check_host(5, 45) && !cw_rows_check_host(0, 0) && !cw_rows_check_host(1000, 45));
    CHECK(!cw_rows_check_device((const void *)4096, 8, 45) && !cw_rows_check_device((const void *)4104, 16, 45));
    CHECK(cw_rows_check_device((const void *)(4096 + 4), 8, 45) && cw_rows_check_device((const void *)4096, 12, 45));
    CHECK(cw_rows_check_device((const void *)4096, 8, 66) && !cw_rows_check_device((const void *)4096, 16, 66) &&
          cw_rows_check_device((const void *)4096, 16, 129) && !cw_rows_check_device((const void *)4096, 24, 129));
    CHECK(!cw_rows_check_device((const void *)4096, 0, 0));
    // repacking: odd strides, a last row that ends with its allocation, spare bytes and bits all ones; the output's pad is zero
    // and every bit of every instance survives, in both orders
    for (uint32_t n : {1u, 45u, 64u, 66u, 129u}) {
        const size_t used = cw_rows_bytes(n), row = 8 * cw_rows_words(n);
        for (size_t stride : {used, used + 1, used + 3, used + 13}) {
            for (int msb = 0; msb < 2; msb++) {
                const size_t count = 67;
                std::unique_ptr<uint8_t[]> src = make_rows(n, count, stride, msb);
                std::unique_ptr<uint8_t[]> out(new uint8_t[count * row]);
                for (size_t i = 0; i < count * row; i++) out[i] = 0xA5;
                cw_rows_repack(src.get(), stride, n, count, out.get());
                bool ok = true;
                for (size_t j = 0; j < count; j++) {
                    for (uint32_t k = 0; k < n; k++) {
                        ok = ok && cw_rows_bit(src.get() + j * stride, k, msb) == model_bit(j, k);
                        ok = ok && cw_rows_bit(out.get() + j * row, k, msb) == model_bit(j, k);
                    }
                    for (size_t t = used; t < row; t++) ok = ok && out[j * row + t] == 0;
                }
                CHECK(ok);
            }
        }
    }
    // no rows, no inputs: nothing is read or written
    cw_rows_repack(nullptr, 0, 0, 0, nullptr);
    std::unique_ptr<uint8_t[]> one(new uint8_t[1]);
    cw_rows_repack(one.get(), 5, 45, 0, one.get());
    return 0;
}

int main() {
    int rc = run();
    if (rc == 0) printf("rows ok: %d checks\n", n_cases);
    return rc;
}
