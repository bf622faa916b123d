// cw_wtns_read.h — the checked reader of a `.wtns` file (writeBinWitness, main.cpp:288-334 / common64/main.cpp) for the calls
// that take witnesses IN (cw_read_wtns, cw_read_wtns_many).  HIP-free and free of the library's own types, so that a stand-alone
// program can run it under the sanitizers (tests/host/wtns_read_test.cpp).  It serves the new reader only: the loaders of
// cw_host.cpp stay as they are.
//
//   "wtns" | u32 version = 2 | u32 sections = 2 | two sections, in either order, each u32 id | u64 length | payload
//   section 1: u32 n8 | the prime, n8 bytes little-endian | u32 nWitness
//   section 2: nWitness x n8 bytes, little-endian elements
//
// One pass over the bytes; every read is preceded by a comparison with what is left.  The file must be the circuit's: its n8,
// its prime, its witness length - and nothing may follow the second section.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

// nullptr: the file is good and *body points at the nWitness x n8 bytes of section 2 inside p[0..n); otherwise the reason.
// `prime`: want_n8 bytes, little-endian.
static inline const char *cw_wtns_parse(const uint8_t *p, size_t n, uint32_t want_n8, const uint8_t *prime, uint32_t want_n_witness,
                                        const uint8_t **body) {
    size_t off = 0;
    auto left = [&]() { return n - off; };
    auto u32 = [&]() { uint32_t v; memcpy(&v, p + off, 4); off += 4; return v; };
    auto u64 = [&]() { uint64_t v; memcpy(&v, p + off, 8); off += 8; return v; };
    if (left() < 12) return "shorter than the 12-byte file header";
    if (memcmp(p, "wtns", 4)) return "bad magic (not a .wtns file)";
    off = 4;
    if (u32() != 2) return "unsupported version (2 expected)";
    if (u32() != 2) return "section count is not 2";
    const uint8_t *sec[3] = {nullptr, nullptr, nullptr};
    uint64_t len[3] = {0, 0, 0};
    for (int s = 0; s < 2; s++) {
        if (left() < 12) return "section header cut short";
        const uint32_t id = u32();
        const uint64_t l = u64();
        if (id != 1 && id != 2) return "unknown section id (1 and 2 expected)";
        if (sec[id]) return "a section appears twice";
        if (l > left()) return "a section is longer than the file";
        sec[id] = p + off;
        len[id] = l;
        off += (size_t)l;
    }
    if (left() != 0) return "bytes behind the last section";
    if (len[1] < 4) return "header section shorter than its n8 field";
    uint32_t n8;
    memcpy(&n8, sec[1], 4);
    if (n8 != want_n8) return "n8 (bytes per element) differs from the circuit's";
    if (len[1] != 8 + (uint64_t)n8) return "header section has the wrong length";
    if (memcmp(sec[1] + 4, prime, n8)) return "the prime differs from the circuit's";
    uint32_t nw;
    memcpy(&nw, sec[1] + 4 + n8, 4);
    if (nw != want_n_witness) return "nWitness differs from the circuit's witness length";
    if (len[2] != (uint64_t)nw * n8) return "body length is not nWitness x n8";
    *body = sec[2];
    return nullptr;
}
