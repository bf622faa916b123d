// Stand-alone check of circom_amd/csrc/cw_wtns_digest.h + cw_sha256.h (no HIP, no Python in the process; built with the address and
// undefined-behaviour sanitizers by tests/test_wtns_digest_host.py, which writes the case file and passes its path):
//   D <n8> <nWitness> <prime hex> <digest hex> <body hex | ->    replay the lane's word stream from the plan through the shared
//                                                                 compress function - header, phase, carry across blocks, tail, the
//                                                                 extra block at nWitness = 1 (mod 8) - and compare with hashlib's
//                                                                 digest, for every RUN the kernels use
//   H <n8> <nWitness> <prime hex> <header hex>                    the header builder, byte for byte, against a reference .wtns
// and, without a file, the argument checks of both calls and the group arithmetic of the launch.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../circom_amd/csrc/cw_wtns_digest.h"

static int checks = 0, failures = 0;
#define EXPECT(cond)                                                    \
    do {                                                                \
        checks++;                                                       \
        if (!(cond)) {                                                  \
            failures++;                                                 \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
        }                                                               \
    } while (0)

static std::vector<uint8_t> unhex(const std::string &s) {
    std::vector<uint8_t> out;
    if (s == "-") return out;
    for (size_t i = 0; i + 1 < s.size(); i += 2) out.push_back((uint8_t)strtoul(s.substr(i, 2).c_str(), nullptr, 16));
    return out;
}

// the table of one instance: exactly nWitness elements, allocated to the byte, so that a read past the list is a sanitizer error
template <uint32_t EW_, uint32_t H_, uint32_t RUN_>
struct HostSrc {
    static constexpr uint32_t EW = EW_, H = H_, RUN = RUN_;
    struct Raw { uint32_t k; };
    const uint8_t *body;
    uint32_t n_witness, fetched = 0;
    Raw fetch(uint32_t k) {
        EXPECT(k < n_witness);
        fetched++;
        return Raw{k};
    }
    void words(const Raw &r, uint32_t w[EW_]) const {
        for (uint32_t i = 0; i < EW_; i++) {
            const uint8_t *p = body + ((size_t)r.k * EW_ + i) * 4;
            w[i] = (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
        }
    }
};

template <class Src>
static std::vector<uint8_t> digest_of(const cwdig::Plan &plan, const uint8_t *body) {
    Src src;
    src.body = body;
    src.n_witness = plan.n_witness;
    uint32_t st[8];
    cwdig::walk(plan, src, st);
    std::vector<uint8_t> d(32);
    for (int i = 0; i < 8; i++) {
        const uint32_t w = cwdig::out_word(st[i]);                       // stored little-endian by the kernels
        for (int k = 0; k < 4; k++) d[4 * i + k] = (uint8_t)(w >> (8 * k));
    }
    return d;
}

static void run_case_file(const char *path) {
    std::ifstream f(path);
    std::string line;
    while (std::getline(f, line)) {
        std::istringstream ss(line);
        std::string kind, prime_hex, a, b;
        uint32_t n8 = 0, nw = 0;
        ss >> kind >> n8 >> nw >> prime_hex >> a;
        if (kind.empty()) continue;
        const std::vector<uint8_t> prime = unhex(prime_hex);
        EXPECT((n8 == 8 || n8 == 32) && prime.size() == n8);
        if (kind == "H") {
            const std::vector<uint8_t> want = unhex(a);
            uint8_t got[cwdig::HDR_MAX];
            const uint32_t len = cwdig::build_header(n8, prime.data(), nw, got);
            EXPECT(len == cwdig::header_bytes(n8) && len == (n8 == 32 ? 76u : 52u) && want.size() == len);
            EXPECT(want.size() == len && !memcmp(got, want.data(), len));
            continue;
        }
        ss >> b;
        const std::vector<uint8_t> want = unhex(a);
        // (a copy of exactly the body's size on the heap: the sanitizer guards both ends)
        const std::vector<uint8_t> body_v = unhex(b);
        uint8_t *body = (uint8_t *)malloc(body_v.size() ? body_v.size() : 1);
        memcpy(body, body_v.data(), body_v.size());
        EXPECT(body_v.size() == (size_t)n8 * nw && want.size() == 32);
        const cwdig::Plan plan = cwdig::make_plan(n8, prime.data(), nw);
        const uint64_t len = cwdig::header_bytes(n8) + (uint64_t)n8 * nw;
        EXPECT(plan.data_words * 4 == len && plan.n_blocks == (len + 9 + 63) / 64);
        if (n8 == 8) EXPECT((plan.n_blocks == len / 64 + 2) == (nw % 8 == 1));           // the extra block
        else EXPECT(plan.n_blocks == len / 64 + 1 && (len % 64 == 12 || len % 64 == 44));
        std::vector<uint8_t> got;
        if (n8 == 32) {
            got = digest_of<HostSrc<8, 19, 1>>(plan, body);
            EXPECT(got == want);
            got = digest_of<HostSrc<8, 19, 4>>(plan, body);               // the bit table's kernel: runs of four blocks
        } else {
            got = digest_of<HostSrc<2, 13, 1>>(plan, body);
            EXPECT(got == want);
            got = digest_of<HostSrc<2, 13, 2>>(plan, body);
        }
        EXPECT(got == want);
        if (got != want) printf("  case n8 = %u, nWitness = %u\n", n8, nw);
        free(body);
    }
}

static void argument_checks() {
    using namespace cwdig;
    EXPECT(check_range(0, 0, 0) == nullptr && check_range(0, 64, 64) == nullptr && check_range(63, 1, 64) == nullptr);
    EXPECT(check_range(0, 65, 64) != nullptr && check_range(64, 1, 64) != nullptr);
    EXPECT(check_range(0xFFFFFFFFu, 2, 64) != nullptr && check_range(2, 0xFFFFFFFFu, 64) != nullptr);     // would wrap in 32 bits
    EXPECT(check_range(0xFFFFFFFFu, 1, 0xFFFFFFFFu) != nullptr && check_range(0xFFFFFFFEu, 1, 0xFFFFFFFFu) == nullptr);
    EXPECT(check_device((void *)(uintptr_t)0x1000) == nullptr && check_device((void *)(uintptr_t)0x1008) != nullptr &&
           check_device((void *)(uintptr_t)0x1001) != nullptr);
    // a wave owns one table group: the groups a range touches
    EXPECT(n_groups(0, 0) == 0 && n_groups(0, 1) == 1 && n_groups(0, 64) == 1 && n_groups(0, 65) == 2);
    EXPECT(n_groups(63, 1) == 1 && n_groups(63, 2) == 2 && n_groups(37, 263) == 5 && n_groups(64, 64) == 1);
    EXPECT(n_groups(1, 0xFFFFFFFFu) == 0x4000000u && n_groups(0, 0xFFFFFFFFu) == 0x4000000u);
    uint8_t prime[32] = {1};
    const Plan p = make_plan(32, prime, 0xFFFFFFFFu);                     // the lengths do not wrap
    EXPECT(p.data_words == 19 + 8ull * 0xFFFFFFFFu && p.n_blocks == (uint32_t)((p.data_words + 18) / 16));
}

int main(int argc, char **argv) {
    argument_checks();
    if (argc > 1) run_case_file(argv[1]);
    if (failures) {
        printf("wtns digest FAILED: %d of %d checks\n", failures, checks);
        return 1;
    }
    printf("wtns digest ok: %d checks\n", checks);
    return 0;
}
