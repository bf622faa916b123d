// cw_wtns_parse (circom_amd/csrc/cw_wtns_read.h), the checked reader behind cw_read_wtns / cw_read_wtns_many, as a stand-alone
// program for the address and undefined-behaviour sanitizers (tests/test_wtns_read_host.py): a good 8-byte and a good 32-byte
// file, the sections swapped, every reason a file is refused, and a good file cut at every byte.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "../../circom_amd/csrc/cw_wtns_read.h"

static int checks = 0;
#define CHECK(x) do { checks++; if (!(x)) { printf("FAILED line %d: %s\n", __LINE__, #x); return 1; } } while (0)

typedef std::vector<uint8_t> Bytes;
static void put(Bytes &b, const void *p, size_t n) { b.insert(b.end(), (const uint8_t *)p, (const uint8_t *)p + n); }
static void put32(Bytes &b, uint32_t v) { put(b, &v, 4); }
static void put64(Bytes &b, uint64_t v) { put(b, &v, 8); }

struct Spec {
    const char *magic = "wtns";
    uint32_t version = 2, n_sections = 2, n8 = 8, n_witness = 5, id1 = 1, id2 = 2;
    Bytes prime;
    bool swapped = false;
    int64_t len1_delta = 0, len2_delta = 0;      // the section's LENGTH FIELD and its payload grow or shrink together
    size_t trailing = 0;
};
static Bytes prime_of(uint32_t n8) {
    const uint64_t gl = 0xFFFFFFFF00000001ull;
    Bytes p(n8, 0);
    if (n8 == 8) memcpy(p.data(), &gl, 8);
    else for (uint32_t i = 0; i < n8; i++) p[i] = (uint8_t)(0x11 + 7 * i);
    return p;
}
static Bytes file_of(const Spec &s) {
    Bytes s1, s2, b;
    put32(s1, s.n8);
    put(s1, s.prime.data(), s.prime.size());
    put32(s1, s.n_witness);
    s1.resize((size_t)((int64_t)s1.size() + s.len1_delta), 0xEE);
    for (size_t i = 0; i < (size_t)s.n_witness * (s.n8 <= 32 ? s.n8 : 8); i++) s2.push_back((uint8_t)(i * 13 + 1));
    s2.resize((size_t)((int64_t)s2.size() + s.len2_delta), 0xEE);
    put(b, s.magic, 4);
    put32(b, s.version);
    put32(b, s.n_sections);
    for (int k = 0; k < 2; k++) {
        const bool first = (k == 0) != s.swapped;
        put32(b, first ? s.id1 : s.id2);
        put64(b, first ? s1.size() : s2.size());
        put(b, first ? s1.data() : s2.data(), first ? s1.size() : s2.size());
    }
    b.resize(b.size() + s.trailing, 0x77);
    return b;
}
// the bytes live in an allocation of exactly their size: a read past the end is the sanitizer's to report
static const char *parse(const Bytes &b, size_t n, uint32_t n8, uint32_t nw, const uint8_t **body, uint8_t **keep) {
    uint8_t *p = (uint8_t *)malloc(n ? n : 1);
    memcpy(p, b.data(), n);
    const Bytes q = prime_of(n8);
    const char *why = cw_wtns_parse(p, n, n8, q.data(), nw, body);
    if (keep) *keep = p;
    else free(p);
    return why;
}
static bool refused(const Spec &s, const char *word, uint32_t n8 = 8, uint32_t nw = 5) {
    const uint8_t *body = nullptr;
    const Bytes b = file_of(s);
    const char *why = parse(b, b.size(), n8, nw, &body, nullptr);
    if (!why || !strstr(why, word)) printf("  got: %s\n", why ? why : "(accepted)");
    return why && strstr(why, word) && body == nullptr;
}

int main() {
    for (uint32_t n8 : {8u, 32u})
        for (bool swapped : {false, true}) {
            Spec s;
            s.n8 = n8;
            s.prime = prime_of(n8);
            s.swapped = swapped;
            const Bytes b = file_of(s);
            const uint8_t *body = nullptr;
            uint8_t *p = nullptr;
            CHECK(parse(b, b.size(), n8, 5, &body, &p) == nullptr);
            CHECK(body != nullptr && body >= p && body + 5 * n8 <= p + b.size());
            for (size_t i = 0; i < (size_t)5 * n8; i++) CHECK(body[i] == (uint8_t)(i * 13 + 1));
            CHECK(swapped ? body == p + 12 + 12 : body + 5 * n8 == p + b.size());
            free(p);
            // cut at every byte: refused, never read past the end
            for (size_t n = 0; n < b.size(); n++) {
                body = nullptr;
                CHECK(parse(b, n, n8, 5, &body, nullptr) != nullptr && body == nullptr);
            }
        }
    Spec g;
    g.prime = prime_of(8);
    { Spec s = g; s.magic = "wtnz"; CHECK(refused(s, "magic")); }
    { Spec s = g; s.magic = "r1cs"; CHECK(refused(s, "magic")); }
    { Spec s = g; s.version = 1; CHECK(refused(s, "version")); }
    { Spec s = g; s.version = 3; CHECK(refused(s, "version")); }
    { Spec s = g; s.n_sections = 1; CHECK(refused(s, "section count")); }
    { Spec s = g; s.n_sections = 3; CHECK(refused(s, "section count")); }
    { Spec s = g; s.id2 = 1; CHECK(refused(s, "twice")); }
    { Spec s = g; s.id1 = 2; CHECK(refused(s, "twice")); }
    { Spec s = g; s.id2 = 3; CHECK(refused(s, "unknown section")); }
    { Spec s = g; s.id1 = 0; CHECK(refused(s, "unknown section")); }
    // n8: a 32-byte file for an 8-byte circuit and the other way round
    { Spec s = g; s.n8 = 32; s.prime = prime_of(32); CHECK(refused(s, "n8")); }
    { Spec s = g; CHECK(refused(s, "n8", 32)); }
    { Spec s = g; s.n8 = 0; s.prime.clear(); CHECK(refused(s, "n8")); }
    { Spec s = g; s.n8 = 0xFFFFFFFFu; CHECK(refused(s, "n8")); }
    { Spec s = g; s.len1_delta = -13; CHECK(refused(s, "shorter than its n8")); }
    { Spec s = g; s.len1_delta = 1; CHECK(refused(s, "header section has the wrong length")); }
    { Spec s = g; s.len1_delta = -1; CHECK(refused(s, "header section has the wrong length")); }
    // the prime: every byte matters
    for (size_t i = 0; i < 8; i++) { Spec s = g; s.prime[i] ^= 1; CHECK(refused(s, "prime")); }
    { Spec s = g; s.n_witness = 4; CHECK(refused(s, "nWitness")); }
    { Spec s = g; s.n_witness = 6; CHECK(refused(s, "nWitness")); }
    { Spec s = g; CHECK(refused(s, "nWitness", 8, 0)); }
    { Spec s = g; s.len2_delta = -1; CHECK(refused(s, "body length")); }
    { Spec s = g; s.len2_delta = 8; CHECK(refused(s, "body length")); }
    { Spec s = g; s.len2_delta = -40; CHECK(refused(s, "body length")); }
    { Spec s = g; s.trailing = 1; CHECK(refused(s, "behind the last section")); }
    { Spec s = g; s.trailing = 64; s.swapped = true; CHECK(refused(s, "behind the last section")); }
    {   // a length field far beyond the file (and beyond size_t arithmetic that adds before it compares)
        Bytes b = file_of(g);
        const uint64_t huge = ~0ull - 3;
        memcpy(&b[12 + 4], &huge, 8);
        const uint8_t *body = nullptr;
        const char *why = parse(b, b.size(), 8, 5, &body, nullptr);
        CHECK(why && strstr(why, "longer than the file"));
    }
    {   // an empty witness is a good file of an empty circuit
        Spec s = g;
        s.n_witness = 0;
        const Bytes b = file_of(s);
        const uint8_t *body = nullptr;
        CHECK(parse(b, b.size(), 8, 0, &body, nullptr) == nullptr);
    }
    printf("wtns read ok: %d checks\n", checks);
    return 0;
}
