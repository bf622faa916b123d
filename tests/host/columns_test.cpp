// Stand-alone test of cw_columns.h (circom_amd/csrc): input columns - the argument checks in their stated order, the coverage
// bitmap and its count, the widening of one value to a 32-byte cell, and the repacking of host rows of any stride into dense ones.
// tests/test_columns_host.py builds it with -fsanitize=address,undefined and runs it: every source image lives in a heap block
// of exactly the bytes the header may read (the last row ends with the allocation), so one byte too many is an error of the run.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "../../circom_amd/csrc/cw_columns.h"

static int n_cases = 0;
#define CHECK(x)                                                        \
    do {                                                                \
        n_cases++;                                                      \
        if (!(x)) {                                                     \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #x); \
            return 1;                                                   \
        }                                                               \
    } while (0)

// the model: byte t of value (j, k)
static uint8_t model_byte(size_t j, uint32_t k, uint32_t t) { return (uint8_t)((j * 131u + k * 29u + t * 7u + 3u) ^ (j >> 3)); }

// rows of `stride` bytes in a block of exactly (count - 1) * stride + n * eb bytes; pad bytes are 0xA5
static std::unique_ptr<uint8_t[]> make_rows(uint32_t n, uint32_t eb, size_t count, size_t stride) {
    const size_t used = cw_columns_row_bytes(n, eb), total = count ? (count - 1) * stride + used : 0;
    std::unique_ptr<uint8_t[]> p(new uint8_t[total ? total : 1]);
    for (size_t i = 0; i < total; i++) p[i] = 0xA5;
    for (size_t j = 0; j < count; j++)
        for (uint32_t k = 0; k < n; k++)
            for (uint32_t t = 0; t < eb; t++) p[j * stride + (size_t)k * eb + t] = model_byte(j, k, t);
    return p;
}

static int run() {
    const void *const a4096 = (const void *)4096;
    // widths
    for (uint32_t eb = 0; eb < 70; eb++) CHECK(cw_columns_width_ok(eb) == (eb == 1 || eb == 2 || eb == 4 || eb == 8 || eb == 32));
    CHECK(cw_columns_row_bytes(0, 32) == 0 && cw_columns_row_bytes(70, 2) == 140 && cw_columns_row_bytes(0xFFFFFFFFu, 32) == 0x1FFFFFFFE0ull);
    // the checks, in their order: width, stride, alignment
    CHECK(cw_columns_check(a4096, 0, 5, 3, false) && cw_columns_check(a4096, 0, 5, 16, true) && cw_columns_check(a4096, 0, 5, 0, false));
    for (uint32_t eb : {1u, 2u, 4u, 8u, 32u}) {
        const size_t row = 5 * eb;
        CHECK(!cw_columns_check(a4096, row, 5, eb, false) && !cw_columns_check(a4096, row + 1, 5, eb, false));
        CHECK(!cw_columns_check(a4096, 0, 5, eb, false) && !cw_columns_check(a4096, 0, 5, eb, true));       // the broadcast form
        CHECK(cw_columns_check(a4096, row - 1, 5, eb, false) && cw_columns_check(a4096, 1, 5, eb, true));
        CHECK(!cw_columns_check((const void *)(4096 + 1), row + 3, 5, eb, false));                           // the host form: any alignment
        CHECK(!cw_columns_check(a4096, row, 5, eb, true) && !cw_columns_check(a4096, row + (eb == 32 ? 16 : eb), 5, eb, true));
        if (eb > 1) {
            CHECK(cw_columns_check((const void *)(4096 + 1), row, 5, eb, true) && cw_columns_check(a4096, row + 1, 5, eb, true));
            CHECK(cw_columns_check((const void *)(4096 + 1), 0, 5, eb, true));                               // broadcast: the pointer still counts
        }
        CHECK(!cw_columns_check(a4096, 0, 0, eb, true) && !cw_columns_check(a4096, row, 0, eb, true));      // no values: nothing to be short of
    }
    // 32-byte elements want 16, not 32
    CHECK(!cw_columns_check((const void *)(4096 + 16), 160 + 16, 5, 32, true) && cw_columns_check((const void *)(4096 + 8), 160, 5, 32, true) &&
          cw_columns_check((const void *)(4096 + 4), 160, 5, 32, true) && cw_columns_check(a4096, 160 + 8, 5, 32, true));
    // a bad width is named before a bad stride, a bad stride before a bad alignment
    CHECK(cw_columns_check((const void *)(4096 + 1), 1, 5, 3, true) == cw_columns_check(a4096, 0, 5, 3, false));
    CHECK(cw_columns_check((const void *)(4096 + 1), 1, 5, 8, true) == cw_columns_check(a4096, 1, 5, 8, false));
    // the range: 64-bit sum
    CHECK(!cw_columns_check_range(0, 76, 76) && cw_columns_check_range(1, 76, 76) && !cw_columns_check_range(76, 0, 76) &&
          cw_columns_check_range(77, 0, 76) && cw_columns_check_range(0xFFFFFFFFu, 2, 76) && cw_columns_check_range(2, 0xFFFFFFFFu, 76));
    // coverage: against a plain array of flags, ranges that begin and end inside, on and across the 64-bit words
    for (uint32_t n_in : {1u, 63u, 64u, 65u, 76u, 200u}) {
        CwColumnCover c;
        c.open(n_in);
        std::vector<uint8_t> flag(n_in, 0);
        CHECK(c.missing == n_in && c.bits.size() == (n_in + 63) / 64);
        const uint32_t cuts[][2] = {{0, 0}, {n_in / 2, 1}, {0, 1}, {n_in - 1, 1}, {n_in / 3, n_in / 3}, {0, n_in / 2}, {n_in / 2, n_in - n_in / 2}, {0, n_in}};
        bool ok = true;
        for (auto &r : cuts) {
            uint32_t fresh = 0;
            for (uint32_t k = r[0]; k < r[0] + r[1]; k++) fresh += !flag[k], flag[k] = 1;
            ok = ok && c.cover(r[0], r[1]) == fresh;
            uint32_t left = 0;
            for (uint32_t k = 0; k < n_in; k++) left += !flag[k], ok = ok && c.covered(k) == (flag[k] != 0);
            ok = ok && c.missing == left;
        }
        CHECK(ok && c.missing == 0);
        for (size_t w = 0; w < c.bits.size(); w++)               // no bit past n_inputs
            CHECK(c.bits[w] == (w + 1 < c.bits.size() || n_in % 64 == 0 ? ~0ull : (1ull << (n_in % 64)) - 1));
        c.open(n_in);                                             // opening again empties it
        CHECK(c.missing == n_in && !c.covered(n_in - 1));
    }
    {
        CwColumnCover c;                                          // a circuit without inputs
        c.open(0);
        CHECK(c.missing == 0 && c.bits.empty() && c.cover(0, 0) == 0);
    }
    // widening: zero-extended, unreduced, nothing read past the value
    for (uint32_t eb : {1u, 2u, 4u, 8u, 32u}) {
        std::unique_ptr<uint8_t[]> v(new uint8_t[eb]);
        for (uint32_t t = 0; t < eb; t++) v[t] = 0xFF;
        uint8_t cell[32];
        for (uint8_t &x : cell) x = 0xA5;
        cw_columns_widen(v.get(), eb, cell);
        bool ok = true;
        for (uint32_t t = 0; t < 32; t++) ok = ok && cell[t] == (t < eb ? 0xFF : 0);
        CHECK(ok);
    }
    // repacking: odd strides, a last row that ends with its allocation, pad bytes 0xA5; every byte of every value survives
    for (uint32_t eb : {1u, 2u, 4u, 8u, 32u}) {
        for (uint32_t n : {1u, 5u, 70u}) {
            const size_t row = cw_columns_row_bytes(n, eb);
            for (size_t stride : {row, row + 1, row + 3, row + 13}) {
                const size_t count = 67;
                std::unique_ptr<uint8_t[]> src = make_rows(n, eb, count, stride);
                std::unique_ptr<uint8_t[]> out(new uint8_t[count * row]);
                cw_columns_repack(src.get(), stride, n, eb, count, out.get());
                bool ok = true;
                for (size_t j = 0; j < count; j++)
                    for (uint32_t k = 0; k < n; k++)
                        for (uint32_t t = 0; t < eb; t++) ok = ok && out[j * row + (size_t)k * eb + t] == model_byte(j, k, t);
                CHECK(ok);
            }
        }
    }
    // no rows, no values: nothing is read or written
    cw_columns_repack(nullptr, 0, 0, 8, 0, nullptr);
    std::unique_ptr<uint8_t[]> one(new uint8_t[1]);
    cw_columns_repack(one.get(), 5, 0, 8, 3, one.get());
    cw_columns_repack(one.get(), 5, 5, 1, 0, one.get());
    return 0;
}

int main() {
    int rc = run();
    if (rc == 0) printf("columns ok: %d checks\n", n_cases);
    return rc;
}
