// cw_sha256.h — the SHA-256 compression function (FIPS 180-4) as ONE text for the device and the host: the digest kernels
// (cw_get_wtns_digests*, cw_wtns_digest.h) run it with lane = message, tests/host/wtns_digest_test.cpp replays it on the CPU.
// Under __HIP_DEVICE_COMPILE__ the rotations, the byte swap, Ch, Maj and the three-way xors are the gfx950 builtins
// (v_alignbit_b32, v_perm_b32, v_bitop3_b32: the back end folds neither behind the rotation builtins itself); the sums become
// v_add3_u32.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CW_SHA_FN __host__ __device__ __forceinline__
#else
#define CW_SHA_FN inline
#endif
#if defined(__clang__)
#define CW_SHA_UNROLL _Pragma("unroll")
#else
#define CW_SHA_UNROLL
#endif

namespace cwsha {

CW_SHA_FN uint32_t rotr(uint32_t x, uint32_t n) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbit(x, x, n);
#else
    return (x >> n) | (x << (32u - n));
#endif
}
// a little-endian table word as the big-endian message word SHA-256 reads
CW_SHA_FN uint32_t bswap(uint32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(0u, x, 0x00010203u);
#else
    return (x >> 24) | ((x >> 8) & 0xFF00u) | ((x << 8) & 0xFF0000u) | (x << 24);
#endif
}
// a ^ b ^ c: one v_bitop3_b32 (truth table 0x96) - behind the rotation builtins the back end does not fold the two xors itself
CW_SHA_FN uint32_t xor3(uint32_t a, uint32_t b, uint32_t c) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96);
#else
    return a ^ b ^ c;
#endif
}
// (truth tables over a = 0xF0, b = 0xCC, c = 0xAA: Ch = (a & b) | (~a & c) = 0xCA, Maj = 0xE8)
CW_SHA_FN uint32_t ch(uint32_t e, uint32_t f, uint32_t g) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_bitop3_b32(e, f, g, 0xCA);
#else
    return (e & f) ^ (~e & g);
#endif
}
CW_SHA_FN uint32_t maj(uint32_t a, uint32_t b, uint32_t c) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_bitop3_b32(a, b, c, 0xE8);
#else
    return (a & b) ^ (a & c) ^ (b & c);
#endif
}
CW_SHA_FN uint32_t bsig0(uint32_t x) { return xor3(rotr(x, 2), rotr(x, 13), rotr(x, 22)); }
CW_SHA_FN uint32_t bsig1(uint32_t x) { return xor3(rotr(x, 6), rotr(x, 11), rotr(x, 25)); }
CW_SHA_FN uint32_t ssig0(uint32_t x) { return xor3(rotr(x, 7), rotr(x, 18), x >> 3); }
CW_SHA_FN uint32_t ssig1(uint32_t x) { return xor3(rotr(x, 17), rotr(x, 19), x >> 10); }

#define CW_SHA_K                                                                                                                    \
    {0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u, 0xd807aa98u, 0x12835b01u, \
     0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u, 0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, \
     0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau, 0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, \
     0x06ca6351u, 0x14292967u, 0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u, \
     0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u, 0x19a4c116u, 0x1e376c08u, \
     0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u, 0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, \
     0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u}

// the initial hash value H(0)
CW_SHA_FN void init(uint32_t st[8]) {
    st[0] = 0x6a09e667u; st[1] = 0xbb67ae85u; st[2] = 0x3c6ef372u; st[3] = 0xa54ff53au;
    st[4] = 0x510e527fu; st[5] = 0x9b05688cu; st[6] = 0x1f83d9abu; st[7] = 0x5be0cd19u;
}

// st += compress(st, w): one 64-byte block, w[0..16) the big-endian message words.  w is the schedule's rolling window of 16
// words and is overwritten.  Fully unrolled: every index is a constant, so state and window stay in registers.
CW_SHA_FN void compress(uint32_t st[8], uint32_t w[16]) {
    constexpr uint32_t K[64] = CW_SHA_K;
    uint32_t a = st[0], b = st[1], c = st[2], d = st[3], e = st[4], f = st[5], g = st[6], h = st[7];
    CW_SHA_UNROLL
    for (int t = 0; t < 64; t++) {
        if (t >= 16) w[t & 15] += ssig1(w[(t - 2) & 15]) + w[(t - 7) & 15] + ssig0(w[(t - 15) & 15]);
        const uint32_t t1 = h + bsig1(e) + ch(e, f, g) + K[t] + w[t & 15];
        const uint32_t t2 = bsig0(a) + maj(a, b, c);
        h = g; g = f; f = e; e = d + t1;
        d = c; c = b; b = a; a = t1 + t2;
    }
    st[0] += a; st[1] += b; st[2] += c; st[3] += d; st[4] += e; st[5] += f; st[6] += g; st[7] += h;
}

}  // namespace cwsha
