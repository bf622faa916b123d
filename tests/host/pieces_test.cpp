// Stand-alone test of cw_pieces (circom_amd/csrc/cw_pieces.h): `count` items in consecutive pieces of at most `per`, the walk
// of every split kernel launch and every staged bulk transfer.  tests/test_pieces_host.py builds it with
// -fsanitize=address,undefined and runs it.
#include <cstdio>
#include <utility>
#include <vector>

#include "../../circom_amd/csrc/cw_pieces.h"

typedef std::vector<std::pair<uint32_t, uint32_t>> Pieces;             // (offset, length)

static Pieces walk(uint32_t count, uint32_t per) {
    Pieces out;
    int rc = cw_pieces(count, per, [&](uint32_t off, uint32_t n) {
        out.emplace_back(off, n);
        return 0;
    });
    if (rc != 0) out.clear();
    return out;
}
// what the walk promises, without storing 2^32 / per pieces: consecutive (so strictly increasing) offsets from 0, every piece
// `per` long but the last, which is the remainder, and the lengths sum to `count`
static bool well_formed(uint32_t count, uint32_t per) {
    uint64_t next = 0, calls = 0;
    bool ok = true;
    int rc = cw_pieces(count, per, [&](uint32_t off, uint32_t n) {
        ok = ok && off == next && n >= 1 && n <= per && (n == per || (uint64_t)off + n == count);
        next = (uint64_t)off + n;
        calls++;
        return 0;
    });
    return rc == 0 && ok && next == count && calls == ((uint64_t)count + per - 1) / per;
}

static int n_cases = 0;
#define CHECK(x)                                                        \
    do {                                                                \
        n_cases++;                                                      \
        if (!(x)) {                                                     \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #x); \
            return 1;                                                   \
        }                                                               \
    } while (0)

enum Err { ERR_NONE = 0, ERR_LAUNCH = 98 };                            // a launcher's return type: an enumeration whose 0 is success

static int run() {
    for (uint32_t per : {65535u, 65535u * 64u}) {                      // a grid dimension; the same in tiles of 64 instances
        CHECK(walk(0, per).empty());
        CHECK((walk(1, per) == Pieces{{0, 1}}));
        CHECK((walk(per - 1, per) == Pieces{{0, per - 1}}));
        CHECK((walk(per, per) == Pieces{{0, per}}));
        CHECK((walk(per + 1, per) == Pieces{{0, per}, {per, 1}}));
        CHECK((walk(2 * per, per) == Pieces{{0, per}, {per, per}}));
        CHECK((walk(2 * per + 1, per) == Pieces{{0, per}, {per, per}, {2 * per, 1}}));
        for (uint32_t count : {0u, 1u, per - 1, per, per + 1, 2 * per, 2 * per + 1}) CHECK(well_formed(count, per));
    }
    // the largest count: a 32-bit `done += per` passes 2^32 behind the last piece and starts again
    const uint32_t top = 0xFFFFFFFFu, per = 65535u * 64u;
    CHECK(well_formed(top, per));
    const Pieces p = walk(top, per);
    CHECK(p.size() == 1025 && p.back() == std::make_pair(1024u * per, top - 1024u * per));
    CHECK(well_formed(top, 65535u) && well_formed(top, top) && well_formed(top, top - 1));
    // per larger than count: one piece
    CHECK((walk(5, 64) == Pieces{{0, 5}}));
    CHECK((walk(70001, top) == Pieces{{0, 70001}}));
    // per = 0 is taken as 1
    CHECK((walk(2, 0) == Pieces{{0, 1}, {1, 1}}));
    // a non-zero return ends the walk and comes back, in the callback's own type
    int calls = 0;
    CHECK(cw_pieces(3 * per, per, [&](uint32_t, uint32_t) { return ++calls == 2 ? -7 : 0; }) == -7 && calls == 2);
    calls = 0;
    CHECK(cw_pieces(3 * per, per, [&](uint32_t, uint32_t) { return ++calls == 2 ? ERR_LAUNCH : ERR_NONE; }) == ERR_LAUNCH && calls == 2);
    CHECK(cw_pieces(0, per, [&](uint32_t, uint32_t) { return ERR_LAUNCH; }) == ERR_NONE);
    return 0;
}

int main() {
    int rc = run();
    if (rc == 0) printf("pieces ok: %d checks\n", n_cases);
    return rc;
}
