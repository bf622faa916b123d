// Stand-alone test of cw_r1cs_products.h (circom_amd/csrc), the HIP-free host part of cw_get_r1cs_products*: the checks of the
// part mask, the row range and the instance range, the alignment of a device image, the plan in file order out of the loaders'
// arrays (a processing permutation undone; the 64-bit list with its end flags), the split of a row range into launch pieces and
// the place of a staged piece of instances in the caller's image.  tests/test_r1cs_products_host.py builds it with
// -fsanitize=address,undefined and runs it: every vector is a heap block of exactly its size, one element too many is an error
// of the run.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <numeric>
#include <vector>

#include "../../circom_amd/csrc/cw_r1cs_products.h"

static int n_cases = 0;
#define CHECK(x)                                                        \
    do {                                                                \
        n_cases++;                                                      \
        if (!(x)) {                                                     \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #x); \
            return 1;                                                   \
        }                                                               \
    } while (0)

using cwprod::check_device;
using cwprod::check_range;

// a constraint system in FILE order: row k, part p has (k * 7 + p * 3) % 5 terms {slot, id}, numbered so that every term is unique
struct Sys {
    std::vector<uint32_t> ptr{0}, slot, id;
};
static Sys file_system(uint32_t n) {
    Sys s;
    for (uint32_t k = 0; k < n; k++)
        for (uint32_t p = 0; p < 3; p++) {
            for (uint32_t t = 0; t < (k * 7 + p * 3) % 5; t++) {
                s.slot.push_back(1000 * k + 10 * p + t);
                s.id.push_back(0x80000000u ^ (77 * k + 5 * p + t));
            }
            s.ptr.push_back((uint32_t)s.slot.size());
        }
    return s;
}

static int run() {
    // ---- the part mask, then the rows, then the instances ----
    CHECK(!check_range(1, 0, 0, 0, 0, 0, 0) && !check_range(7, 0, 4, 4, 0, 5, 5) && !check_range(5, 4, 0, 4, 5, 0, 5));
    CHECK(check_range(0, 0, 4, 4, 0, 5, 5) && check_range(8, 0, 4, 4, 0, 5, 5) && check_range(15, 0, 4, 4, 0, 5, 5) &&
          check_range(0x80000001u, 0, 4, 4, 0, 5, 5));
    for (uint32_t parts = 1; parts < 8; parts++) CHECK(!check_range(parts, 1, 3, 4, 4, 1, 5));
    CHECK(check_range(3, 3, 2, 4, 0, 5, 5) && check_range(3, 0, 5, 4, 0, 5, 5) && check_range(3, 5, 0, 4, 0, 5, 5));
    CHECK(check_range(3, 0, 4, 4, 0, 6, 5) && check_range(3, 0, 4, 4, 5, 1, 5) && check_range(3, 0, 4, 4, 6, 0, 5));
    CHECK(check_range(3, 0xFFFFFFFFu, 2, 4, 0, 1, 5) && check_range(3, 2, 0xFFFFFFFFu, 4, 0, 1, 5));          // no 32-bit wrap
    CHECK(check_range(3, 0, 1, 4, 0xFFFFFFFFu, 2, 5) && check_range(3, 0, 1, 4, 2, 0xFFFFFFFFu, 5));
    CHECK(!check_range(7, 0, 0xFFFFFFFFu, 0xFFFFFFFFu, 0, 0xFFFFFFFFu, 0xFFFFFFFFu));
    CHECK(check_range(0, 9, 9, 4, 9, 9, 5) == check_range(0, 0, 1, 4, 0, 1, 5));                               // the mask is looked at first
    CHECK(check_range(3, 0, 5, 4, 0, 6, 5) == check_range(3, 0, 5, 4, 0, 1, 5));                               // then the rows
    CHECK(check_range(3, 0, 5, 4, 0, 6, 5) != check_range(3, 0, 4, 4, 0, 6, 5));
    CHECK(cwprod::n_parts(1) == 1 && cwprod::n_parts(2) == 1 && cwprod::n_parts(4) == 1 && cwprod::n_parts(5) == 2 && cwprod::n_parts(7) == 3);
    // ---- the device image: 8 bytes for 8-byte elements, 16 otherwise; compared, never read ----
    CHECK(!check_device((const void *)4096, 8) && !check_device((const void *)4104, 8) && check_device((const void *)4100, 8) &&
          check_device((const void *)4097, 8));
    CHECK(!check_device((const void *)4096, 32) && check_device((const void *)4104, 32) && check_device((const void *)4100, 32) &&
          !check_device((const void *)4112, 32));
    // ---- 64-bit sizes ----
    CHECK(cwprod::instance_bytes(7, 0x40000000u, 32) == (size_t)3 * 0x40000000u * 32 && cwprod::instance_bytes(5, 3, 8) == 48);
    CHECK(cwprod::piece_bytes(cwprod::instance_bytes(7, 1000000, 32), 70000) == (size_t)70000 * 3 * 1000000 * 32);

    // ---- the plan out of arrays in processing order: every permutation gives the file's system back ----
    for (uint32_t n : {1u, 2u, 17u, 64u, 65u}) {
        const Sys f = file_system(n);
        for (uint32_t mul : {1u, 3u, 7u}) {                          // processing row j = file row (j * mul + 5) % n, coprime for these n
            if (n % mul == 0 && n > 1 && mul > 1) continue;
            Sys pr;
            std::vector<uint32_t> orig(n);
            for (uint32_t j = 0; j < n; j++) {
                const uint32_t k = (uint32_t)(((uint64_t)j * mul + 5) % n);
                orig[j] = k | (j % 3 == 0 ? 0x80000000u : 0u);       // the equality mark is not part of the index
                for (uint32_t p = 0; p < 3; p++) {
                    for (uint32_t t = f.ptr[3 * k + p]; t < f.ptr[3 * k + p + 1]; t++) {
                        pr.slot.push_back(f.slot[t]);
                        pr.id.push_back(f.id[t]);
                    }
                    pr.ptr.push_back((uint32_t)pr.slot.size());
                }
            }
            const cwprod::Plan p = cwprod::build(pr.ptr, pr.slot, pr.id, orig, nullptr);
            CHECK(p.words == 2 && p.rowptr == f.ptr && p.n_terms() == f.slot.size());
            bool ok = true;
            for (size_t t = 0; t < f.slot.size(); t++) ok = ok && p.terms[2 * t] == f.slot[t] && p.terms[2 * t + 1] == f.id[t];
            CHECK(ok);
            // a slot map (bit tables): applied to every term, an index past it refuses the plan
            std::vector<uint32_t> map(1000 * n + 30);
            for (size_t s = 0; s < map.size(); s++) map[s] = (uint32_t)(3 + 2 * s);
            const cwprod::Plan q = cwprod::build(pr.ptr, pr.slot, pr.id, orig, &map);
            ok = q.rowptr == f.ptr;
            for (size_t t = 0; ok && t < f.slot.size(); t++) ok = q.terms[2 * t] == 3 + 2 * f.slot[t] && q.terms[2 * t + 1] == f.id[t];
            CHECK(ok);
            if (!f.slot.empty()) {
                map.resize(*std::max_element(f.slot.begin(), f.slot.end()));
                CHECK(cwprod::build(pr.ptr, pr.slot, pr.id, orig, &map).rowptr.empty());
            }
            // an r_orig that is no permutation, arrays that do not fit: no plan
            std::vector<uint32_t> twice(orig);
            if (n > 1) {
                twice[0] = twice[1];
                CHECK(cwprod::build(pr.ptr, pr.slot, pr.id, twice, nullptr).rowptr.empty());
            }
            twice = orig;
            twice[0] = n;
            CHECK(cwprod::build(pr.ptr, pr.slot, pr.id, twice, nullptr).rowptr.empty());
            std::vector<uint32_t> shortptr(pr.ptr.begin(), pr.ptr.end() - 1);
            CHECK(cwprod::build(shortptr, pr.slot, pr.id, orig, nullptr).rowptr.empty());
        }
    }
    // ---- the 64-bit list: {slot, part | end << 2, lo, hi}; an empty constraint is ONE filler term, which is left out ----
    {
        std::vector<uint32_t> t64;
        auto term = [&](uint32_t slot, uint32_t part, uint64_t co) { t64.insert(t64.end(), {slot, part, (uint32_t)co, (uint32_t)(co >> 32)}); };
        auto end = [&]() { t64[t64.size() - 3] |= 4u; };
        term(5, 0, 3); term(6, 0, 0xFFFFFFFF00000000ull); term(7, 1, 1); term(8, 2, 9); end();      // row 0: 2 + 1 + 1
        term(0, 2, 0); end();                                                                        // row 1: the filler
        term(9, 1, 4); end();                                                                        // row 2: B only
        term(0, 2, 0); term(3, 2, 0); end();                                                         // row 3: two zero terms are the file's
        term(2, 0, 0); end();                                                                        // row 4: a lone zero term in A is the file's
        const cwprod::Plan p = cwprod::build64(t64, 5);
        const std::vector<uint32_t> want_ptr{0, 2, 3, 4, 4, 4, 4, 4, 5, 5, 5, 5, 7, 8, 8, 8};
        CHECK(p.words == 4 && p.rowptr == want_ptr && p.n_terms() == 8);
        CHECK(p.terms[0] == 5 && p.terms[2] == 3 && p.terms[3] == 0 && p.terms[4] == 6 && p.terms[6] == 0 && p.terms[7] == 0xFFFFFFFFu);
        CHECK(p.terms[4 * 4] == 9 && p.terms[4 * 4 + 2] == 4 && p.terms[4 * 7] == 2 && p.terms[4 * 7 + 2] == 0);
        CHECK(cwprod::build64(t64, 4).rowptr.empty() && cwprod::build64(t64, 6).rowptr.empty());       // the count must fit the list
        std::vector<uint32_t> cut(t64.begin(), t64.end() - 4);
        cut[cut.size() - 3] &= ~4u;
        CHECK(cwprod::build64(cut, 4).rowptr.empty());                                                // ends inside a constraint
        std::vector<uint32_t> swapped(t64);
        std::swap(swapped[1], swapped[4 * 2 + 1]);                                                    // B in front of A
        CHECK(cwprod::build64(swapped, 5).rowptr.empty());
        const cwprod::Plan none = cwprod::build64(std::vector<uint32_t>(), 0);
        CHECK(none.rowptr.size() == 1 && none.terms.empty());
    }
    // ---- launch pieces: at most 65 535 tiles per launch, consecutive, complete ----
    struct Case { uint32_t n, tile; };
    for (const Case c : {Case{1, 16}, Case{16, 16}, Case{17, 16}, Case{65535u * 16, 16}, Case{65535u * 16 + 1, 16}, Case{1020832, 16},
                         Case{3 * 65535u * 16 + 5, 16}, Case{65535u * 64 + 63, 64}, Case{65535u * 64 * 2, 64}, Case{0xFFFFFFFFu, 64}, Case{0, 16}}) {
        uint64_t at = 0;
        uint32_t launches = 0;
        bool ok = true;
        const int rc = cwprod::row_pieces(c.n, c.tile, [&](uint32_t off, uint32_t m) {
            ok = ok && off == at && m >= 1 && cwprod::row_tiles(m, c.tile) <= cwprod::GRID_Y && (uint64_t)off + m <= c.n;
            ok = ok && (off + (uint64_t)m == c.n || m == cwprod::GRID_Y * c.tile);     // every piece but the last is full
            at += m;
            launches++;
            return 0;
        });
        CHECK(rc == 0 && ok && at == c.n && launches == (c.n + (uint64_t)cwprod::GRID_Y * c.tile - 1) / ((uint64_t)cwprod::GRID_Y * c.tile));
    }
    CHECK(cwprod::row_tiles(1, 16) == 1 && cwprod::row_tiles(16, 16) == 1 && cwprod::row_tiles(17, 16) == 2 && cwprod::row_tiles(0, 16) == 0 &&
          cwprod::row_tiles(0xFFFFFFFFu, 64) == 0x4000000u);
    CHECK(cwprod::row_tiles(1020832, 16) == 63802);                                   // Sha256(2048): one launch
    int stopped = 0;
    CHECK(cwprod::row_pieces(3 * 65535u * 16, 16, [&](uint32_t, uint32_t) { return ++stopped == 2 ? 7 : 0; }) == 7 && stopped == 2);
    // ---- staged pieces of whole instances land where the caller's image has them: the pieces tile it ----
    for (uint32_t per : {1u, 2u, 5u, 67u, 100u}) {
        const uint32_t count = 67, n_rows = 5;
        const size_t inst = cwprod::instance_bytes(5, n_rows, 8), total = (size_t)count * inst;
        std::unique_ptr<uint8_t[]> out(new uint8_t[total]);
        for (size_t i = 0; i < total; i++) out[i] = 0xA5;
        size_t covered = 0;
        bool ok = true;
        cw_pieces(count, per, [&](uint32_t done, uint32_t m) {
            std::unique_ptr<uint8_t[]> staged(new uint8_t[cwprod::piece_bytes(inst, m)]);     // what the device piece holds
            for (size_t i = 0; i < cwprod::piece_bytes(inst, m); i++) staged[i] = (uint8_t)((done * inst + i) * 31 >> 3);
            ok = ok && cwprod::piece_at(out.get(), inst, done) == out.get() + covered;
            memcpy(cwprod::piece_at(out.get(), inst, done), staged.get(), cwprod::piece_bytes(inst, m));
            covered += cwprod::piece_bytes(inst, m);
            return 0;
        });
        for (size_t i = 0; i < total; i++) ok = ok && out[i] == (uint8_t)(i * 31 >> 3);
        CHECK(ok && covered == total);
    }
    return 0;
}

int main() {
    int rc = run();
    if (rc == 0) printf("r1cs products ok: %d checks\n", n_cases);
    return rc;
}
