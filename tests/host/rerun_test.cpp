// Stand-alone test of cw_rerun_runs (circom_amd/csrc/cw_rerun.h): the runs of consecutive re-run instances of a bit-plane
// batch, clipped to a window of instances.  tests/test_rerun.py builds it with -fsanitize=address,undefined and runs it.
#include <cstdio>
#include <tuple>

#include "../../circom_amd/csrc/cw_rerun.h"

typedef std::vector<std::tuple<uint32_t, uint32_t, uint32_t>> Runs;   // (side-batch position, length, offset from `first`)

static Runs walk(const std::vector<uint32_t> &list, uint32_t first, uint32_t count) {
    Runs out;
    int rc = cw_rerun_runs(list, first, count, [&](uint32_t pos, uint32_t len, uint32_t off) {
        out.emplace_back(pos, len, off);
        return 0;
    });
    if (rc != 0) out.clear();
    return out;
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

static int run() {
    const std::vector<uint32_t> odd = {3, 64, 65, 129};                // the runs {3}, {64, 65}, {129}
    CHECK((walk(odd, 0, 130) == Runs{{0, 1, 3}, {1, 2, 64}, {3, 1, 129}}));
    CHECK(walk(odd, 4, 60).empty());                                   // [4, 64): between the first two runs
    CHECK((walk(odd, 64, 1) == Runs{{1, 1, 0}}));                      // the head of a run
    CHECK((walk(odd, 65, 65) == Runs{{2, 1, 0}, {3, 1, 64}}));         // its tail: the position moves with the clip
    std::vector<uint32_t> all(10);
    for (uint32_t i = 0; i < 10; i++) all[i] = i;                      // the side batch is the whole batch
    CHECK((walk(all, 2, 3) == Runs{{2, 3, 0}}));
    CHECK((walk(all, 0, 10) == Runs{{0, 10, 0}}));
    CHECK(walk({}, 0, 130).empty());                                   // nothing was re-run
    CHECK(walk(odd, 3, 0).empty() && walk(all, 0, 0).empty());         // an empty window
    // the last instances a batch can have: first + count and instance + 1 reach 2^32 - 1 and, one further, 2^32
    const std::vector<uint32_t> top = {7, 0xFFFFFFFDu, 0xFFFFFFFEu};
    CHECK((walk(top, 0xFFFFFFF0u, 15) == Runs{{1, 2, 13}}));
    CHECK((walk(top, 0xFFFFFFFEu, 1) == Runs{{2, 1, 0}}));
    CHECK((walk(top, 0, 0xFFFFFFFFu) == Runs{{0, 1, 7}, {1, 2, 0xFFFFFFFDu}}));
    CHECK((walk({0xFFFFFFFEu, 0xFFFFFFFFu}, 0xFFFFFFFFu, 1) == Runs{{1, 1, 0}}));
    // a non-zero return ends the walk and comes back
    int calls = 0;
    CHECK(cw_rerun_runs(odd, 0, 130, [&](uint32_t, uint32_t, uint32_t) { return ++calls == 2 ? -7 : 0; }) == -7 && calls == 2);
    return 0;
}

int main() {
    int rc = run();
    if (rc == 0) printf("rerun ok: %d checks\n", n_cases);
    return rc;
}
