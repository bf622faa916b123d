// cw_wtns_digest.h — witness digests (cw_get_wtns_digests*): SHA-256 of the `.wtns` file of every instance, computed where the
// table lies.  HIP-free: the ONE definition of the file's header bytes (cw_write_wtns* write these bytes too), the plan of the
// message as a stream of 32-bit words, the argument checks, and the walk of one message, lane = instance, which the three kernels
// (cw64.hip, cw_kernels.hip, cw_bits.hip) and tests/host/wtns_digest_test.cpp compile from this same text.
//
// The message of an instance is header | element 0 | ... | element nWitness - 1, elements canonical little-endian of n8 bytes in
// witness-list order.  Header length (44 + n8) and n8 are multiples of 4, so no element word straddles a message word:
//   H words of header, EW words per element, D = H + EW nWitness data words, C = H mod EW
//   n8 = 32:  H = 19, EW = 8, C = 3: block j >= 1 is words 5..7 of element 2j-3 (element -1 = the header's last 12 bytes), all of
//             element 2j-2, words 0..4 of element 2j-1.  L mod 64 is 12 or 44: the padding always fits the last data block.
//   n8 = 8:   H = 13, EW = 2, C = 1: a block begins 4 bytes into element 8j-7.  L mod 64 = 52 + 8 (nWitness mod 8): nWitness = 1
//             (mod 8) leaves 60 bytes, room for the 0x80 but not for the length - one extra block.
// Every block therefore takes its first C words from the block before (the carry) and NE = 16 / EW new elements, e0(j) = (16 j +
// C - H) / EW onwards, whose last C words are the next carry.  Positions before the first element are header words (block 0
// only), positions from D onwards are the padding; both are wave-uniform, since D depends on n8 and nWitness alone.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include "cw_sha256.h"

namespace cwdig {

constexpr uint32_t HDR_MAX = 76, HDR_WORDS_MAX = 19;
constexpr uint32_t header_bytes(uint32_t n8) { return 44u + n8; }

// writeBinWitness (main.cpp:288-334): "wtns", version 2, two sections; section 1 = n8, the prime, nWitness; then the head of
// section 2, whose body is the nWitness elements.  n8 = 32 (76 bytes) or 8 (52 bytes); returns the length.
inline uint32_t build_header(uint32_t n8, const uint8_t *prime, uint32_t n_witness, uint8_t out[HDR_MAX]) {
    uint8_t *p = out;
    auto u32 = [&](uint32_t v) { for (int i = 0; i < 4; i++) *p++ = (uint8_t)(v >> (8 * i)); };
    auto u64 = [&](uint64_t v) { for (int i = 0; i < 8; i++) *p++ = (uint8_t)(v >> (8 * i)); };
    memcpy(p, "wtns", 4);
    p += 4;
    u32(2); u32(2);
    u32(1); u64(8 + (uint64_t)n8);
    u32(n8);
    memcpy(p, prime, n8);
    p += n8;
    u32(n_witness);
    u32(2); u64((uint64_t)n8 * n_witness);
    return (uint32_t)(p - out);
}

// What a kernel needs beside the table, passed by value: the header as big-endian message words and the lengths.
struct Plan {
    uint32_t hdr[HDR_WORDS_MAX];    // header words as SHA-256 reads them (n8 = 8: the first 13)
    uint32_t mid[8];                // n8 = 32: the state behind block 0, which is header words alone - the same for every instance
    uint32_t n8, n_witness;
    uint32_t n_blocks;              // blocks of the padded message: (D + 18) / 16
    uint64_t data_words;            // D
};
inline Plan make_plan(uint32_t n8, const uint8_t *prime, uint32_t n_witness) {
    Plan p;
    memset(&p, 0, sizeof p);
    uint8_t h[HDR_MAX];
    const uint32_t len = build_header(n8, prime, n_witness, h);
    for (uint32_t k = 0; k < len / 4; k++)
        p.hdr[k] = (uint32_t)h[4 * k] << 24 | (uint32_t)h[4 * k + 1] << 16 | (uint32_t)h[4 * k + 2] << 8 | h[4 * k + 3];
    p.n8 = n8;
    p.n_witness = n_witness;
    p.data_words = len / 4 + (uint64_t)(n8 / 4) * n_witness;
    p.n_blocks = (uint32_t)((p.data_words + 18) / 16);        // data, the 0x80 word, two words of length
    if (len >= 64) {
        uint32_t w[16];
        for (int k = 0; k < 16; k++) w[k] = p.hdr[k];
        cwsha::init(p.mid);
        cwsha::compress(p.mid, w);
    }
    return p;
}

// Argument checks of both calls, in the order of the other getters (the caller has refused null pointers): nullptr = fine.
inline const char *check_range(uint32_t first, uint32_t count, uint32_t batch) {
    return (uint64_t)first + count > batch ? "instance range out of the batch" : nullptr;
}
inline const char *check_device(const void *d_out) { return ((uintptr_t)d_out & 15) ? "d_out must be 16-byte aligned" : nullptr; }

// groups of 64 instances a range touches: a wave owns group (first >> 6) + w, w < n_groups(first, count)
inline uint32_t n_groups(uint32_t first, uint32_t count) { return count ? (uint32_t)((((uint64_t)(first & 63u) + count) + 63) >> 6) : 0u; }

// The walk of one message.  Src is the table of the lane's instance:
//   EW, H, RUN         words per element, header words, blocks whose elements are requested together
//   Raw                an element as it was loaded (unconverted: the loads of the next run stay in flight over the rounds)
//   Raw fetch(k)       request entry k of the witness list, k < n_witness
//   void words(raw, w) its EW canonical little-endian words
// A run is RUN consecutive blocks, the first run beginning with the walk's first block.
// The elements of the run after this one are requested before the rounds of this run's first block (RUN = 1: those of block j + 1
// before the rounds of block j).  Entries outside the list are clamped to it and their words replaced, so every index is in range.
template <class Src>
CW_SHA_FN void walk(const Plan &P, Src &src, uint32_t st[8]) {
    constexpr uint32_t EW = Src::EW, H = Src::H, RUN = Src::RUN, NE = 16u / EW, C = H % EW, NR = RUN * NE;
    static_assert(16u % EW == 0 && C < EW && H <= HDR_WORDS_MAX, "the shape of the stream");
    const uint64_t D = P.data_words;
    const uint32_t nw = P.n_witness, nb = P.n_blocks;
    typename Src::Raw cur[NR], nxt[NR];
    uint32_t carry[C ? C : 1u];
    CW_SHA_UNROLL
    for (uint32_t c = 0; c < (C ? C : 1u); c++) carry[c] = 0;
    // entry e0(j) + i for the run that starts at block j, clamped into the list (int64: e0(0) is negative)
    auto entry = [&](uint32_t j, uint32_t i) -> uint32_t {
        const int64_t e = ((int64_t)16 * j + (int64_t)C - (int64_t)H) / (int64_t)EW + i;    // (exact: EW divides 16 j + C - H)
        return e < 0 ? 0u : e >= (int64_t)nw ? nw - 1u : (uint32_t)e;
    };
    // a header of 16 words or more: block 0 is the same for every instance, the host has run it (P.mid) and the walk begins at
    // block 1 with the header's last words as its carry
    constexpr uint32_t J0 = H >= 16 ? 1u : 0u;
    if constexpr (J0 == 1) {
        CW_SHA_UNROLL
        for (uint32_t k = 0; k < 8; k++) st[k] = P.mid[k];
        CW_SHA_UNROLL
        for (uint32_t c = 0; c < C; c++) carry[c] = P.hdr[16 + c];
    } else {
        cwsha::init(st);
    }
    CW_SHA_UNROLL
    for (uint32_t i = 0; i < NR; i++) nxt[i] = cur[i] = src.fetch(entry(J0, i));
    for (uint32_t j = J0; j < nb; j++) {
        if ((j - J0) % RUN == 0 && j + RUN < nb) {
            CW_SHA_UNROLL
            for (uint32_t i = 0; i < NR; i++) nxt[i] = src.fetch(entry(j + RUN, i));
        }
        // x[0 .. 16 + C): the block and the carry behind it
        uint32_t x[16 + C];
        CW_SHA_UNROLL
        for (uint32_t c = 0; c < C; c++) x[c] = carry[c];
        CW_SHA_UNROLL
        for (uint32_t t = 0; t < NE; t++) {
            uint32_t ew[EW];
            src.words(cur[t], ew);
            CW_SHA_UNROLL
            for (uint32_t k = 0; k < EW; k++) x[C + EW * t + k] = cwsha::bswap(ew[k]);
        }
        const uint64_t m0 = (uint64_t)16 * j;
        if ((J0 == 0 && j == 0) || m0 + 16 + C > D) {                    // an edge block: header words, padding, the length
            CW_SHA_UNROLL
            for (uint32_t p = 0; p < 16 + C; p++) {
                const uint64_t m = m0 + p;
                if (J0 == 0 && j == 0 && p < H) x[p] = P.hdr[p];
                else if (p < C) continue;                                // the carry is what the block before made of it
                else if (m == D) x[p] = 0x80000000u;
                else if (m > D) x[p] = 0;
            }
            if (j == nb - 1) {
                x[14] = (uint32_t)(D >> 27);                             // 32 D bits
                x[15] = (uint32_t)(D << 5);
            }
        }
        CW_SHA_UNROLL
        for (uint32_t c = 0; c < C; c++) carry[c] = x[16 + c];
        cwsha::compress(st, x);
        // the window moves on by one block; behind the run's last block the next run takes its place
        CW_SHA_UNROLL
        for (uint32_t i = 0; i + NE < NR; i++) cur[i] = cur[i + NE];
        if ((j + 1 - J0) % RUN == 0) {
            CW_SHA_UNROLL
            for (uint32_t i = 0; i < NR; i++) cur[i] = nxt[i];
        }
    }
}

// the digest bytes of a state word by word: big-endian, the order hashlib and sha256sum print
CW_SHA_FN uint32_t out_word(uint32_t s) { return cwsha::bswap(s); }

#if defined(__HIPCC__)
// Common to the three kernels: a wave owns table group (first >> 6) + blockIdx.x, lane = instance.  A lane outside [first, first +
// count) has computed on the padded table and stores nothing; the others store their digest at out[instance - first] as two
// 16-byte stores, 2 KiB contiguous per wave.
__device__ __forceinline__ uint32_t wave_group(uint32_t first, uint32_t block) { return __builtin_amdgcn_readfirstlane((first >> 6) + block); }
__device__ __forceinline__ void store_digest(uint4 *__restrict__ out, uint32_t first, uint32_t count, uint32_t inst, const uint32_t st[8]) {
    if (inst < first || inst - first >= count) return;
    uint4 *o = out + (size_t)(inst - first) * 2;
    o[0] = make_uint4(out_word(st[0]), out_word(st[1]), out_word(st[2]), out_word(st[3]));
    o[1] = make_uint4(out_word(st[4]), out_word(st[5]), out_word(st[6]), out_word(st[7]));
}
#endif

}  // namespace cwdig
