// cw_fn64_parse (circom_amd/csrc/cw_fn64.h), the reader and validator of the function section of a 64-bit tape, as a stand-alone
// program for the address and undefined-behaviour sanitizers (tests/test_fn64_host.py): good sections, every reason a section is
// refused, and a small section cut at every byte.
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include "../../circom_amd/csrc/cw_fn64.h"

static int checks = 0;
#define CHECK(x) do { checks++; if (!(x)) { printf("FAILED line %d: %s\n", __LINE__, #x); return 1; } } while (0)

struct Ins { uint32_t op, d, a, b; };
struct Fn { uint32_t n_regs; std::vector<Ins> code; };

static std::vector<uint8_t> section(const std::vector<Fn> &fns) {
    std::vector<uint32_t> w{(uint32_t)fns.size()};
    for (const Fn &f : fns) {
        w.push_back(f.n_regs);
        w.push_back((uint32_t)f.code.size());
        for (const Ins &i : f.code) w.insert(w.end(), {i.op, i.d, i.a, i.b});
    }
    std::vector<uint8_t> b(w.size() * 4);
    memcpy(b.data(), w.data(), b.size());
    return b;
}
// the bytes live in an allocation of exactly their size: a read past the end is the sanitizer's to report
static const char *parse(const std::vector<uint8_t> &b, size_t n, uint32_t n_consts, CwFn64 *out, size_t *used) {
    uint8_t *p = (uint8_t *)malloc(n ? n : 1);
    memcpy(p, b.data(), n);
    const char *why = cw_fn64_parse(p, n, n_consts, out, used);
    free(p);
    return why;
}
static bool refused(const Fn &f, uint32_t n_consts = 3) {
    CwFn64 out;
    size_t used = 0;
    const std::vector<uint8_t> b = section({f});
    return parse(b, b.size(), n_consts, &out, &used) != nullptr;
}

int main() {
    const uint32_t ADD = 1, COPY = 0, LNOT = 23, K = FN_CONST;
    // r4 = r0 + c2; loop: if (!r4) goto end; r5 = arr[r1] (arr = r2..r3); arr[r1] = c0; goto loop; end: ret
    const Fn good{6, {{ADD, 4, 0, K | 2}, {F_JZ, 5, 4, 0}, {F_LDX, 5, 2, 1 | (2u << 16)}, {F_STX, 2, K | 0, 1 | (2u << 16)}, {F_JMP, 1, 0, 0},
                      {F_RET, 0, 0, 0}}};
    const Fn tiny{1, {{LNOT, 0, 0, 0}, {F_JMP, 0, 0, 0}}};           // ends in a jump: fine
    {
        CwFn64 out;
        size_t used = 0;
        std::vector<uint8_t> b = section({good, tiny});
        b.push_back(0xAB);                                           // what follows the section is not its business
        CHECK(parse(b, b.size(), 3, &out, &used) == nullptr);
        CHECK(used == b.size() - 1);
        CHECK(out.tab == (std::vector<uint32_t>{0, 6, 6, 0, 6, 2, 1, 0}));
        CHECK(out.code.size() == 8 * 4 && out.code[0] == ADD && out.code[6 * 4] == LNOT && out.max_regs == 6);
        b = section({});
        CHECK(parse(b, b.size(), 0, &out, &used) == nullptr && used == 4 && out.tab.empty() && out.max_regs == 0);
        // the largest window a function may have
        CHECK(!refused(Fn{65535, {{COPY, 65534, 65534, 0}, {F_LDX, 0, 1, 0 | (65534u << 16)}, {F_RET, 0, 0, 0}}}));
    }
    auto with = [&](size_t i, Ins x) { Fn f = good; f.code[i] = x; return f; };
    CHECK(!refused(good));
    CHECK(refused(with(0, {24, 4, 0, 1})));                          // O_SELECT: no operator of a function body
    CHECK(refused(with(0, {99, 4, 0, 1})));
    CHECK(refused(with(0, {F_DIV, 4, 0, 1})));                       // the 256-bit engine's number: this engine writes O_DIV
    CHECK(refused(with(0, {ADD, 6, 0, 1})));                         // register >= n_regs: destination, a, b
    CHECK(refused(with(0, {ADD, 4, 6, 1})));
    CHECK(refused(with(0, {ADD, 4, 0, 6})));
    CHECK(refused(with(0, {ADD, 4, 0, 0x7FFFFFFFu})));
    CHECK(refused(with(0, {ADD, 4, K | 3, 1})));                     // constant >= n_consts
    CHECK(refused(with(0, {ADD, 4, 0, K | 0x7FFFFFFFu})));
    CHECK(refused(good, 2));
    CHECK(refused(with(1, {F_JZ, 6, 4, 0})));                        // jump target >= n_instructions
    CHECK(refused(with(1, {F_JZ, 5, 6, 0})));
    CHECK(refused(with(1, {F_JZ, 5, K | 3, 0})));
    CHECK(refused(with(4, {F_JMP, 6, 0, 0})));
    CHECK(refused(with(4, {F_JMP, 0xFFFFFFFFu, 0, 0})));
    CHECK(refused(with(2, {F_LDX, 5, 2, 1 | (5u << 16)})));          // base + length leaves the window
    CHECK(refused(with(2, {F_LDX, 5, 6, 1 | (1u << 16)})));
    CHECK(refused(with(2, {F_LDX, 5, 0xFFFFFFFFu, 1 | (2u << 16)})));   // (no wrap-around)
    CHECK(refused(with(2, {F_LDX, 5, 2, 1 | (0u << 16)})));          // an array of no elements
    CHECK(refused(with(2, {F_LDX, 6, 2, 1 | (2u << 16)})));
    CHECK(refused(with(2, {F_LDX, 5, 2, 6 | (2u << 16)})));          // index register
    CHECK(refused(with(3, {F_STX, 5, K | 0, 1 | (2u << 16)})));
    CHECK(refused(with(3, {F_STX, 0xFFFFFFFEu, K | 0, 1 | (2u << 16)})));
    CHECK(refused(with(3, {F_STX, 2, K | 3, 1 | (2u << 16)})));
    CHECK(refused(with(3, {F_STX, 2, 6, 1 | (2u << 16)})));
    CHECK(!refused(with(2, {F_LDX, 5, 2, 1 | (4u << 16)})));         // ... and the longest array that fits
    CHECK(refused(with(5, {COPY, 0, 0, 0})));                        // the program counter could run off the end
    CHECK(refused(with(5, {F_JZ, 0, 0, 0})));
    {
        Fn f = good;
        f.n_regs = 1u << 16;
        CHECK(refused(f));
        f.n_regs = 0;
        CHECK(refused(f));
        f = good;
        f.code.clear();
        CHECK(refused(f));
    }
    {   // counts that promise more than the bytes hold
        CwFn64 out;
        size_t used = 0;
        std::vector<uint8_t> b = section({good});
        uint32_t v = 0xFFFFFFFFu;
        memcpy(b.data(), &v, 4);
        CHECK(parse(b, b.size(), 3, &out, &used) != nullptr);
        b = section({good});
        memcpy(b.data() + 8, &v, 4);
        CHECK(parse(b, b.size(), 3, &out, &used) != nullptr);
        v = 1u << 24;
        memcpy(b.data() + 8, &v, 4);
        CHECK(parse(b, b.size(), 3, &out, &used) != nullptr);
        v = 2;
        b = section({good});
        memcpy(b.data(), &v, 4);                                     // a second function that is not there
        CHECK(parse(b, b.size(), 3, &out, &used) != nullptr);
    }
    {   // cut at every byte
        const std::vector<uint8_t> b = section({good, tiny});
        for (size_t n = 0; n < b.size(); n++) {
            CwFn64 out;
            size_t used = 0;
            CHECK(parse(b, n, 3, &out, &used) != nullptr);
        }
    }
    printf("fn64 ok: %d checks\n", checks);
    return 0;
}
