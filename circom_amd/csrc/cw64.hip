// cw64.hip — the 64-bit runtime on the device: circuits compiled for `--prime goldilocks` (q = 2^64 - 2^32 + 1).
//
// Reference counterpart: code_producers/src/c_elements/goldilocks/fr.hpp (a field element is a plain uint64, no Montgomery
// form, no tagged representations) with common64/{main,calcwit}.cpp and the value-style emitted code (compute_bucket.rs:353,
// store_bucket.rs:575-657; constants are literals: value_bucket.rs:82-86).  The 256-bit engine (cw_kernels.hip) is built on
// "q is large" (short products without reduction, lazy integer sums, single-limb masks): none of that holds for a 64-bit
// prime, and none of its machinery is needed - a value is ONE register.  So this file is its own small engine:
//
//   value table   V[slot][instance] : uint64, canonical residues, slot 0 = the constant 1, signals, hidden log values, temporaries
//                 (one coalesced 512-byte access per wave and operand)
//   program       the flat witness code, one 32-byte row per operation (hip_elements/lower64.py), wave-uniform
//   one lane = one instance; operators follow the reference's 64-bit library exactly as oracle/field.py restates it for
//   any q (tests/golden/reference_wtns_goldilocks.json: vectors from the reference's own 64-bit runtime, incl. the operator zoo)
#include <hip/hip_runtime.h>
#include "cw_kernels.h"
#include "cw_pieces.h"
#include "cw_r1cs_products.h"
#include "cw_columns.hip.h"
#include "cw_list.hip.h"
#include "cw_compare.hip.h"
#include "cw_wtns_digest.h"

#define GL_P 0xFFFFFFFF00000001ull
#define GL_HALF (GL_P >> 1)

// ---- field arithmetic ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t gl_add(uint64_t a, uint64_t b) {
    const uint64_t s = a + b;
    const bool wrap = s < a;                       // a + b >= 2^64: subtract p = add 2^32 - 1
    uint64_t r = wrap ? s + 0xFFFFFFFFull : s;     // (a, b < p, so the corrected value is < p)
    return r >= GL_P ? r - GL_P : r;
}
__device__ __forceinline__ uint64_t gl_sub(uint64_t a, uint64_t b) { return a >= b ? a - b : a + (GL_P - b); }
__device__ __forceinline__ uint64_t gl_neg(uint64_t a) { return a ? GL_P - a : 0; }
// x = hi 2^64 + lo with 2^64 = 2^32 - 1, 2^96 = -1 (mod p): lo - hi_hi + hi_lo (2^32 - 1)
__device__ __forceinline__ uint64_t gl_reduce128(uint64_t hi, uint64_t lo) {
    const uint64_t hh = hi >> 32, hl = hi & 0xFFFFFFFFull;
    uint64_t t = lo - hh;
    if (lo < hh) t -= 0xFFFFFFFFull;               // borrowed 2^64 = p + 2^32 - 1: take the 2^32 - 1 back (t stays a residue mod p)
    const uint64_t m = hl * 0xFFFFFFFFull;         // < 2^64
    uint64_t r = t + m;
    if (r < t) r += 0xFFFFFFFFull;                 // carried 2^64
    return r >= GL_P ? r - GL_P : r;
}
__device__ __forceinline__ uint64_t gl_mul(uint64_t a, uint64_t b) { return gl_reduce128(__umul64hi(a, b), a * b); }
__device__ __forceinline__ uint64_t gl_pow(uint64_t x, uint64_t e) {
    uint64_t r = 1;
    for (int i = 63; i >= 0; i--) {
        r = gl_mul(r, r);
        if ((e >> i) & 1ull) r = gl_mul(r, x);
    }
    return r;
}
__device__ __forceinline__ uint64_t gl_inv(uint64_t x) { return gl_pow(x, GL_P - 2); }            // Fr_inv: 0 -> 0
__device__ __forceinline__ uint64_t gl_wrap(uint64_t v) { return v >= GL_P ? v - GL_P : v; }     // lboMask is all ones: one subtraction
__device__ __forceinline__ bool gl_lt(uint64_t x, uint64_t y) {                                    // val(x) < val(y), val = x - p iff x > half
    const bool nx = x > GL_HALF, ny = y > GL_HALF;
    return nx == ny ? x < y : nx;
}
__device__ __forceinline__ uint64_t gl_shl(uint64_t x, uint64_t y) {
    if (y < 64) return gl_wrap(x << y);
    const uint64_t k = GL_P - y;                   // a "negative" amount shifts the other way
    return k >= 64 ? 0 : x >> k;
}
__device__ __forceinline__ uint64_t gl_shr(uint64_t x, uint64_t y) {
    if (y < 64) return x >> y;
    const uint64_t k = GL_P - y;
    return k >= 64 ? 0 : gl_wrap(x << k);
}

// a 32-byte little-endian value w0 + w1 2^64 + w2 2^128 + w3 2^192 mod p, whatever its words hold: what cw64_ingest_kernel<32>
// stores and what the input columns of 32-byte elements store (cw_columns.hip.h)
__device__ __forceinline__ uint64_t gl_reduce256(uint64_t w0, uint64_t w1, uint64_t w2, uint64_t w3) {
    uint64_t r = gl_wrap(w0);
    if (w1 | w2 | w3) {
        // 2^64 = 2^32 - 1, 2^128 = (2^32 - 1)^2, 2^192 = (2^32 - 1)^3 (mod p)
        const uint64_t e = 0xFFFFFFFFull, e2 = gl_mul(e, e), e3 = gl_mul(e2, e);
        r = gl_add(r, gl_mul(gl_wrap(w1), e));
        r = gl_add(r, gl_mul(gl_wrap(w2), e2));
        r = gl_add(r, gl_mul(gl_wrap(w3), e3));
    }
    return r;
}

// ---- kernels ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) cw64_init_kernel(uint64_t *V, uint32_t Bp, uint32_t *status, uint32_t *first_bad) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < Bp) {
        V[i] = 1;                                  // slot 0
        status[i] = 0;
        first_bad[i] = 0xFFFFFFFFu;
    }
}
// inputs arrive as [batch][n_in][EB] little-endian values: EB = 32, the boundary's element, or EB = 8, the element of this
// runtime; a value that is not a canonical residue (upper words set, or >= p) is reduced, as Fr_str2element does for what
// loadJson reads.  Lane = instance, blockIdx.y = input: consecutive lanes read values n_in * EB bytes apart.  This is the
// kernel for narrow circuits and for a 32-byte image at an address that is no multiple of 16 (cw64_transpose_in_kernel below).
template <int EB>
__global__ void __launch_bounds__(256) cw64_ingest_kernel(const uint64_t *__restrict__ in, uint64_t *V, uint32_t input_start, uint32_t n_in,
                                                          uint32_t batch, uint32_t Bp) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x, k = blockIdx.y;
    if (i >= batch) return;
    const uint64_t *p = in + ((size_t)i * n_in + k) * (EB / 8);
    V[(size_t)(input_start + k) * Bp + i] = EB == 32 ? gl_reduce256(p[0], p[1], p[2], p[3]) : gl_wrap(p[0]);
}

// row = 8 x u32: w0 = op | dk << 8 | ak << 10 | bk << 12 | ck << 14 (kind 0 = table slot, 2 = constant, 3 = none); dst; a; b; c;
// index of the flat operation (failure reports); 0; 0.  O_CALL: a = function id, b = slot of register 0 of the call's window.
enum : uint32_t { O_COPY = 0, O_ADD, O_SUB, O_MUL, O_DIV, O_IDIV, O_MOD, O_POW, O_NEG, O_SHL, O_SHR, O_BAND, O_BOR, O_BXOR, O_BNOT,
                  O_LT, O_GT, O_LEQ, O_GEQ, O_EQ, O_NEQ, O_LAND, O_LOR, O_LNOT, O_SELECT, O_ASSERT_EQ, O_ASSERT_NZ, O_CALL };
// the operators of the witness language on two values (O_COPY .. O_LNOT): what a row computes and what an instruction of a
// function body computes.  An integer division or modulo by zero sets *fail and yields 0.
__device__ __forceinline__ uint64_t gl_alu(uint32_t op, uint64_t a, uint64_t b, bool *fail) {
    uint64_t d = 0;
    switch (op) {
    case O_COPY: d = a; break;
    case O_ADD: d = gl_add(a, b); break;
    case O_SUB: d = gl_sub(a, b); break;
    case O_MUL: d = gl_mul(a, b); break;
    case O_DIV: d = gl_mul(a, gl_inv(b)); break;
    case O_IDIV: if (b == 0) *fail = true; else d = a / b; break;
    case O_MOD: if (b == 0) *fail = true; else d = a % b; break;
    case O_POW: d = gl_pow(a, b); break;
    case O_NEG: d = gl_neg(a); break;
    case O_SHL: d = gl_shl(a, b); break;
    case O_SHR: d = gl_shr(a, b); break;
    case O_BAND: d = gl_wrap(a & b); break;
    case O_BOR: d = gl_wrap(a | b); break;
    case O_BXOR: d = gl_wrap(a ^ b); break;
    case O_BNOT: d = gl_wrap(~a); break;
    case O_LT: d = gl_lt(a, b); break;
    case O_GT: d = gl_lt(b, a); break;
    case O_LEQ: d = !gl_lt(b, a); break;
    case O_GEQ: d = !gl_lt(a, b); break;
    case O_EQ: d = a == b; break;
    case O_NEQ: d = a != b; break;
    case O_LAND: d = (a != 0) & (b != 0); break;
    case O_LOR: d = (a != 0) | (b != 0); break;
    case O_LNOT: d = a == 0; break;
    default: break;
    }
    return d;
}

// ---- O_CALL: a circom function with run-time control flow, interpreted per lane ----------------------------------------------
// Reference: the emitted C++ of a function is real control flow on Fr_isTrue / Fr_toInt (loop_bucket.rs:76-91,
// branch_bucket.rs:100-122, compute_bucket.rs:361-363, call_bucket.rs:466-533); trip counts differ per input, so the trace cannot
// unroll it.  Structure of cw_call.hip.h eval_call_body, the 256-bit engine's interpreter: every lane has its own program counter;
// per turn the wave executes the instruction of its unfinished lane with the LOWEST counter for all lanes that sit on it, the
// others wait (rtcode.py's bytecode is structured - an `if` jumps forward over its body, a loop jumps back to its head - so lanes
// that took different sides of a branch meet again at its join).  Bytecode: 4 x u32 {opcode, dst, a, b}, opcode = O_COPY ..
// O_LNOT or F_* of cw_tape.h, operand = register or FN_CONST | constant index; cw_fn64.h checked every number when the tape
// was loaded, so nothing here can leave the window, the constant table or the function's code.
//
// A lane fails and carries on, as oracle/tape_eval.py run_function does: an array index >= the array's length reads / writes
// element 0, an integer division or modulo by zero yields 0; after CW_CALL_STEP_LIMIT instructions the lane is flagged and stops.
//
// The register window = n_regs consecutive temporaries of the lane's column, two placements behind fn_get / fn_set:
//   table   register r = V[base + r][instance], as the 256-bit engine has it: every access is a 512-byte access of the wave, a
//           run-time index makes it one row per lane
//   LDS     win[r * 64 + lane] in 8-byte words (dynamic LDS, max_regs * 512 bytes for the workgroup's one wave): the window is
//           copied in from the table when the call begins (one coalesced 512-byte load per register) and copied back when the
//           last lane has returned, so the table stays the only state between rows and both placements leave the same bytes in
//           it.  Banks: a row is 64 words = 128 dwords, a multiple of the 64-dword bank cycle of ds_read_b64 / ds_write_b64, so
//           lane l sits on dword bank 2 l mod 64 WHATEVER register it addresses: the 32 lanes of a half-wave fall on 32 distinct
//           bank pairs, for the wave-uniform register of an ordinary instruction and for the per-lane register of a run-time
//           index alike - no conflicts.  (Arithmetic from the documented bank rules, as the egress and ingest comments below are;
//           nobody has taken a bank-conflict counter pass on this kernel.)
// A lane only ever touches its own column of either placement: no barrier, and lanes past the batch (already returned) are
// never waited for - ballots count the lanes in EXEC only.
extern __shared__ uint64_t cw64_win[];
template <bool LDS>
__device__ __forceinline__ uint64_t fn_get(const uint64_t *W, uint32_t Bp, uint32_t r) {
    return LDS ? cw64_win[r * 64u + threadIdx.x] : W[(size_t)r * Bp];
}
template <bool LDS>
__device__ __forceinline__ void fn_set(uint64_t *W, uint32_t Bp, uint32_t r, uint64_t v) {
    if (LDS) cw64_win[r * 64u + threadIdx.x] = v;
    else W[(size_t)r * Bp] = v;
}
template <bool LDS>
__device__ __forceinline__ uint64_t fn_operand(uint32_t x, const uint64_t *W, uint32_t Bp, const uint64_t *__restrict__ consts) {
    return x & FN_CONST ? consts[x & 0x7FFFFFFFu] : fn_get<LDS>(W, Bp, x);
}
// W = the lane's register 0 (V + base * Bp + instance); returns whether the lane failed
template <bool LDS>
__device__ __forceinline__ bool cw64_call(const uint4 *__restrict__ ftab, const uint4 *__restrict__ fcode, uint32_t fn, uint64_t *W, uint32_t Bp,
                                          const uint64_t *__restrict__ consts) {
    const uint4 ft = ftab[fn];                                          // {first instruction, n instructions, n registers, -}
    const uint4 *code = fcode + ft.x;
    const uint32_t lane = threadIdx.x;
    if (LDS)
        for (uint32_t r = 0; r < ft.z; r++) cw64_win[r * 64u + lane] = W[(size_t)r * Bp];
    uint32_t pc = 0, steps = 0;
    bool done = false, bad = false;
    const int pc_bits = 32 - __builtin_clz(ft.y | 1u);                  // instruction indices are < ft.y (wave-uniform)
    while (__builtin_amdgcn_ballot_w64(!done)) {
        // the lowest program counter among the unfinished lanes, bit by bit with ballots
        uint64_t cand = __builtin_amdgcn_ballot_w64(!done);
        uint32_t cur = 0;
        for (int bit = pc_bits - 1; bit >= 0; bit--) {
            const uint64_t z = __builtin_amdgcn_ballot_w64(!done && ((cand >> lane) & 1ull) && !((pc >> bit) & 1u));
            if (z) cand = z;
            else cur |= 1u << bit;
        }
        if (!done && pc == cur) {
            const uint4 ins = code[cur];                                // wave-uniform
            const uint32_t op = ins.x, d = ins.y;
            pc = cur + 1;
            if (++steps > CW_CALL_STEP_LIMIT) {
                bad = true;
                done = true;
            } else if (op == F_RET) {
                done = true;
            } else if (op == F_JMP) {
                pc = d;
            } else if (op == F_JZ) {
                if (fn_operand<LDS>(ins.z, W, Bp, consts) == 0) pc = d;
            } else if (op == F_LDX || op == F_STX) {
                // Fr_toInt restricted to what an array address can be: [0, length) or "bad" (a "negative" value is >= 2^63)
                const uint64_t iv = fn_get<LDS>(W, Bp, ins.w & 0xFFFFu);
                uint32_t idx = (uint32_t)iv;
                if (iv >= (uint64_t)(ins.w >> 16)) {
                    bad = true;
                    idx = 0;
                }
                if (op == F_LDX) fn_set<LDS>(W, Bp, d, fn_get<LDS>(W, Bp, ins.z + idx));
                else fn_set<LDS>(W, Bp, d + idx, fn_operand<LDS>(ins.z, W, Bp, consts));
            } else {
                const uint64_t a = fn_operand<LDS>(ins.z, W, Bp, consts);
                uint64_t b = 0;
                if (op != O_COPY && op != O_NEG && op != O_BNOT && op != O_LNOT) b = fn_operand<LDS>(ins.w, W, Bp, consts);
                fn_set<LDS>(W, Bp, d, gl_alu(op, a, b, &bad));
            }
        }
    }
    if (LDS)
        for (uint32_t r = 0; r < ft.z; r++) W[(size_t)r * Bp] = cw64_win[r * 64u + lane];
    return bad;
}

// (Round 6 tried requesting the operands of row r + 1 before row r computes, with register forwarding of a value the next row
// reads: 1.15 ms instead of 0.96 ms for Poseidon(2) x 65 536 - the loads of one row already overlap across the waves of a SIMD,
// the extra bookkeeping does not pay; profiles/r06i_bench_poseidon2_goldilocks.json has that run.  The check below is what
// moved the line: 38 -> 59 M witnesses/s.)
// CALLS: 0 = the program has no O_CALL row (no LDS, and the row loop has no branch for one), 1 = register windows in the table,
// 2 = in LDS.  ftab / fcode are read by the other two only.
template <int CALLS>
__global__ void __launch_bounds__(64) cw64_eval_kernel(const uint4 *__restrict__ rows, uint32_t n_rows, const uint64_t *__restrict__ consts,
                                                       uint64_t *V, uint32_t Bp, uint32_t batch, uint32_t *status,
                                                       const uint4 *__restrict__ ftab, const uint4 *__restrict__ fcode) {
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= batch) return;
    uint64_t *Vi = V + i;
    uint32_t st = 0;
    for (uint32_t r = 0; r < n_rows; r++) {
        const uint4 x = rows[2 * r], y = rows[2 * r + 1];               // wave-uniform: scalar loads
        const uint32_t op = x.x & 0xFF, ak = (x.x >> 10) & 3, bk = (x.x >> 12) & 3, ck = (x.x >> 14) & 3;
        if (CALLS && op == O_CALL) {
            if (cw64_call<CALLS == 2>(ftab, fcode, x.z, Vi + (size_t)x.w * Bp, Bp, consts) && !(st & 3u)) st = CW_ST_ARITH | (y.y << 8);
            continue;
        }
        const uint64_t a = ak == 0 ? Vi[(size_t)x.z * Bp] : ak == 2 ? consts[x.z] : 0;
        const uint64_t b = bk == 0 ? Vi[(size_t)x.w * Bp] : bk == 2 ? consts[x.w] : 0;
        uint64_t d = 0;
        bool fail = false;
        switch (op) {
        case O_SELECT: {
            const uint64_t cc = ck == 0 ? Vi[(size_t)y.x * Bp] : ck == 2 ? consts[y.x] : 0;
            d = a != 0 ? b : cc;
            break;
        }
        case O_ASSERT_EQ: fail = a != b; break;
        case O_ASSERT_NZ: fail = a == 0; break;
        default: d = gl_alu(op, a, b, &fail); break;
        }
        if (fail && !(st & 3u))                                      // the first failing check in program order
            st = (op == O_IDIV || op == O_MOD ? CW_ST_ARITH : CW_ST_ASSERT_FAILED) | (y.y << 8);
        if (((x.x >> 8) & 3) == 0 && op != O_ASSERT_EQ && op != O_ASSERT_NZ) Vi[(size_t)x.y * Bp] = d;
    }
    if (st) atomicOr(&status[i], st);
}

// R1CS: constraint k = three runs of (slot, coefficient) terms; A.w * B.w == C.w.  term = {slot, part | last of the constraint
// << 2, coefficient lo, hi}.  A workgroup checks ONE CHUNK of consecutive constraints (chunk = {first term, terms, first row, 0},
// cut at constraint boundaries by the host) for 64 instances: the launch is (groups x chunks) workgroups instead of one
// wave per 64 instances walking the whole system (Poseidon(2): 3 037 dependent load + multiply steps per wave, one wave per
// SIMD: 1.69 ms; chunked: the chip is full and the loads of different chunks overlap).
__global__ void __launch_bounds__(64) cw64_r1cs_kernel(const uint4 *__restrict__ chunks, uint32_t n_chunks, const uint4 *__restrict__ terms,
                                                       const uint64_t *__restrict__ V, uint32_t Bp, uint32_t batch, uint32_t *status,
                                                       uint32_t *first_bad) {
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= batch) return;
    const uint64_t *Vi = V + i;
    uint32_t bad = 0xFFFFFFFFu;
    for (uint32_t cix = blockIdx.y; cix < n_chunks; cix += gridDim.y) {
        const uint4 ch = chunks[cix];
        uint64_t acc[3] = {0, 0, 0};
        uint32_t row = ch.z;
        uint4 x = terms[ch.x];
        uint64_t w = Vi[(size_t)x.x * Bp];
        for (uint32_t t = 0; t < ch.y; t++) {
            const uint4 nx = terms[ch.x + (t + 1 < ch.y ? t + 1 : t)];      // the next term's wire is in flight during the product
            const uint64_t nw = Vi[(size_t)nx.x * Bp];
            const uint64_t pr = gl_mul(w, ((uint64_t)x.w << 32) | x.z);
            const uint32_t part = x.y & 3u;
            acc[0] = part == 0 ? gl_add(acc[0], pr) : acc[0];
            acc[1] = part == 1 ? gl_add(acc[1], pr) : acc[1];
            acc[2] = part == 2 ? gl_add(acc[2], pr) : acc[2];
            if (x.y & 4u) {
                if (gl_mul(acc[0], acc[1]) != acc[2] && row < bad) bad = row;
                row++;
                acc[0] = acc[1] = acc[2] = 0;
            }
            x = nx;
            w = nw;
        }
    }
    if (bad != 0xFFFFFFFFu) {
        atomicMin(&first_bad[i], bad);
        atomicOr(&status[i], CW_ST_R1CS_FAILED);
    }
}

// one instance's witness as 32-byte little-endian values (the boundary's element format; the files are written with n8 = 8)
__global__ void __launch_bounds__(256) cw64_gather_kernel(const uint64_t *__restrict__ V, const uint32_t *__restrict__ w2s, uint32_t n_wit,
                                                          uint32_t Bp, uint32_t first, uint32_t count, uint64_t *out) {
    const uint32_t k = blockIdx.x * 256 + threadIdx.x, j = blockIdx.y;
    if (k >= n_wit || j >= count) return;
    uint64_t *o = out + ((size_t)j * n_wit + k) * 4;
    o[0] = V[(size_t)w2s[k] * Bp + first + j];
    o[1] = o[2] = o[3] = 0;
}

// Bulk egress as a transpose: `count` instances from `first` as [count][n_wit][EB] bytes, EB = 32 (the boundary's element,
// value + 24 zero bytes) or 8 (the .wtns element of this runtime: n8 = 8, common64/main.cpp writeBinWitness).  The gather
// above gives consecutive lanes consecutive ENTRIES: every lane reads another row of V[slot][instance], Bp * 8 bytes from its
// neighbour's - 64 cache lines for 512 useful bytes.  Here a workgroup of four waves owns 64 instances x EG_T entries:
//   read    wave w takes the entries k = w, w + 4, ... of the tile; w2s[k] is wave-uniform and the 64 lanes read 64 consecutive
//           instances of that slot (one 512-byte access, as the evaluation kernel reads its operands); the 16 loads of a wave are
//           issued before the first value is used
//   stage   tile[k][j] in LDS with rows of EG_S = 65 words of 8 bytes.  Row-wise write (ds_write_b64: four groups of 16
//           consecutive lanes, bank = (a/4) % 32): a group writes 16 consecutive words = 32 consecutive dwords, every bank once,
//           whatever the row's start.  Column-wise read (ds_read_b64: two groups of 32 lanes, bank = (a/4) % 64): lane l reads
//           word l' * 65 + j with l' = l (8-byte form) or l / 2 (32-byte form, even lanes only), dword 2 (l' * 65 + j), bank
//           pair 2 ((l' + j) % 32): the 32 (or 16) rows l' of a group fall on distinct pairs.  With rows of 64 words every lane
//           of a group would hit pair 2 (j % 32): 32-way.  (Odd is what matters: 65 is the smallest odd stride >= 64.)
//   write   wave w takes the instances j = w, w + 4, ...; consecutive lanes write consecutive pieces of out[j][k0 .. k0 + EG_T):
//           8-byte form: the 64 values, 512 contiguous bytes (8-byte stores: with n_wit odd a row starts on an 8-byte boundary
//           only); 32-byte form: 16-byte pieces {value, 0} (even lanes) and {0, 0} (odd lanes), 1 KiB contiguous per store,
//           two stores per row of the tile.  `out` must be 16-byte aligned in the 32-byte form.
// Lanes past `count` and entries past n_wit neither read nor write.
//
// AT: egress by index (cw_get_witnesses_at*): out[j][k] = entry k of the range in instance idx[j].  The same tile with list
// positions for instances - the same stage (nothing new in LDS) and the same stores -, but lane l reads V[slot * Bp + idx[j0 + l]]
// instead of first + j0 + l: a vector load per lane, loaded once per thread before the loop over the entries; for an ascending
// dense list the 64 addresses of a read are still one 512-byte run.  `first` is not used.
//   length  `count` positions in this launch, the launch's first being position pos0 of the caller's list, cut at *d_n
//           (cw_list_limit): a workgroup whose tile lies behind the end leaves at once, before its barrier, and rows behind it
//           are not written.
//   bad     a position whose index is >= batch loads nothing and stages zeros: its row is zeros.  After a ballot one lane of the
//           tile's first workgroup reports the lowest such position, pos0 + j0 + l, with atomicMin (`bad` may be nullptr; the
//           caller fills it first).
#define EG_T 64
#define EG_S 65
template <int EB, bool AT>
__global__ void __launch_bounds__(256) cw64_egress_kernel(const uint64_t *__restrict__ V, const uint32_t *__restrict__ w2s, uint32_t n_wit,
                                                          uint32_t Bp, uint32_t first, uint32_t count, uint8_t *__restrict__ out,
                                                          uint32_t batch, const uint32_t *__restrict__ idx, uint32_t pos0,
                                                          const uint32_t *__restrict__ d_n, uint32_t *bad) {
    __shared__ uint64_t tile[EG_T * EG_S];
    const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t k0 = blockIdx.x * EG_T, j0 = blockIdx.y * 64u;
    const uint32_t lim = AT ? cw_list_limit(count, pos0, d_n) : count;
    if (AT && j0 >= lim) return;                                       // the whole workgroup
    const uint32_t nk = n_wit - k0 < EG_T ? n_wit - k0 : EG_T, nj = lim - j0 < 64u ? lim - j0 : 64u;
    bool ok = lane < nj;
    const uint64_t *Vj = V + first + j0 + lane;
    if (AT) {
        const uint32_t inst = ok ? idx[j0 + lane] : 0u;
        const uint64_t off = __ballot(ok && inst >= batch);
        if (bad && off && blockIdx.x == 0 && threadIdx.x == 0) atomicMin(bad, pos0 + j0 + (uint32_t)__builtin_ctzll(off));
        ok = ok && inst < batch;
        Vj = V + (ok ? inst : 0u);
    }
    uint64_t v[EG_T / 4];
#pragma unroll
    for (uint32_t i = 0; i < EG_T / 4; i++) {
        const uint32_t k = wave + 4 * i;
        const uint32_t slot = w2s[k < nk ? k0 + k : k0];             // always an entry of the list: the scalar load needs no branch
        v[i] = k < nk && ok ? Vj[(size_t)slot * Bp] : 0;
    }
#pragma unroll
    for (uint32_t i = 0; i < EG_T / 4; i++) tile[(wave + 4 * i) * EG_S + lane] = v[i];
    __syncthreads();
    for (uint32_t j = wave; j < nj; j += 4) {
        const size_t at = (size_t)(j0 + j) * n_wit + k0;             // first element of this row of the tile in `out`
        if (EB == 8) {
            if (lane < nk) ((uint64_t *)out)[at + lane] = tile[lane * EG_S + j];
        } else {
            uint4 *row = (uint4 *)out + at * 2;
#pragma unroll
            for (uint32_t h = 0; h < 2; h++) {
                const uint32_t p = lane + 64 * h, k = p >> 1;
                if (k < nk) {
                    const uint64_t x = p & 1u ? 0 : tile[k * EG_S + j];
                    row[p] = make_uint4((uint32_t)x, (uint32_t)(x >> 32), 0, 0);
                }
            }
        }
    }
}

// Witness compare (cw_compare_witnesses*): the range egress above with its stores turned into loads and compares.  image[j][k]
// (EB bytes, [count][n_wit]) against entry k of the range (w2s points at its first entry, entry0 in the witness list) of instance
// first + j: diff[j] = min(diff[j], lowest differing entry0 + k), summary as cw_compare.hip.h states it; the caller fills
// diff[0 .. count) and summary first.  The tile, its rows of EG_S words, the read and the stage of cw64_egress_kernel<EB, false>;
// then wave w takes the instances j = w, w + 4, ... and consecutive lanes LOAD consecutive pieces of image[j][k0 .. k0 + EG_T),
// streaming: the 64 values, 512 contiguous bytes (8-byte form), or 16-byte pieces, 1 KiB contiguous per load, two loads per row
// of the tile (32-byte form: an even piece must be {value, 0}, an odd piece zero - the upper 24 bytes count).  Every byte of the
// image is requested by exactly one workgroup; lanes past `count` and entries past n_wit neither read nor write.
//   reduce  the lanes of a load cover ascending entries of ONE instance: after a ballot the lowest differing lane notes its entry
//           in low[] (one LDS atomic per instance and load, none for equal pieces).
template <int EB>
__global__ void __launch_bounds__(256) cw64_compare_kernel(const uint64_t *__restrict__ V, const uint32_t *__restrict__ w2s, uint32_t n_wit,
                                                           uint32_t Bp, uint32_t first, uint32_t count, const uint8_t *__restrict__ image,
                                                           uint32_t entry0, uint32_t report0, uint32_t *__restrict__ diff,
                                                           uint32_t *__restrict__ summary) {
    __shared__ uint64_t tile[EG_T * EG_S];
    __shared__ uint32_t low[64];
    const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t k0 = blockIdx.x * EG_T, j0 = blockIdx.y * 64u;
    const uint32_t nk = n_wit - k0 < EG_T ? n_wit - k0 : EG_T, nj = count - j0 < 64u ? count - j0 : 64u;
    const bool ok = lane < nj;
    const uint64_t *Vj = V + first + j0 + lane;
    if (wave == 0) low[lane] = CMP_EQUAL;
    uint64_t v[EG_T / 4];
#pragma unroll
    for (uint32_t i = 0; i < EG_T / 4; i++) {
        const uint32_t k = wave + 4 * i;
        const uint32_t slot = w2s[k < nk ? k0 + k : k0];             // always an entry of the list: the scalar load needs no branch
        v[i] = k < nk && ok ? Vj[(size_t)slot * Bp] : 0;
    }
#pragma unroll
    for (uint32_t i = 0; i < EG_T / 4; i++) tile[(wave + 4 * i) * EG_S + lane] = v[i];
    __syncthreads();
    // CH rows of the tile at a time: eight loads of a lane are in flight before the first compare
    constexpr uint32_t CH = EB == 8 ? 8 : 4;
    for (uint32_t jb = wave; jb < nj; jb += 4 * CH) {                // (jb, nj and the trip count are wave-uniform)
        if (EB == 8) {
            uint64_t got[CH];
#pragma unroll
            for (uint32_t u = 0; u < CH; u++) {
                const uint32_t j = jb + 4 * u;
                got[u] = 0;
                if (j < nj && lane < nk) got[u] = cmp_load8((const uint64_t *)image + (size_t)(j0 + j) * n_wit + k0 + lane);
            }
#pragma unroll
            for (uint32_t u = 0; u < CH; u++) {
                const uint32_t j = jb + 4 * u;
                if (j < nj) {
                    const uint64_t who = __ballot(lane < nk && got[u] != tile[lane * EG_S + j]);
                    if (who && lane == (uint32_t)__builtin_ctzll(who)) atomicMin(&low[j], entry0 + k0 + lane);
                }
            }
        } else {
            uint4 got[CH][2];
#pragma unroll
            for (uint32_t u = 0; u < CH; u++)
#pragma unroll
                for (uint32_t h = 0; h < 2; h++) {
                    const uint32_t j = jb + 4 * u, p = lane + 64 * h;
                    got[u][h] = make_uint4(0, 0, 0, 0);
                    if (j < nj && (p >> 1) < nk) got[u][h] = cmp_load16((const uint4 *)image + ((size_t)(j0 + j) * n_wit + k0) * 2 + p);
                }
#pragma unroll
            for (uint32_t u = 0; u < CH; u++) {
                const uint32_t j = jb + 4 * u;
                if (j < nj) {
#pragma unroll
                    for (uint32_t h = 0; h < 2; h++) {
                        const uint32_t p = lane + 64 * h, k = p >> 1;
                        bool ne = false;
                        if (k < nk) {
                            const uint64_t x = p & 1u ? 0 : tile[k * EG_S + j];
                            ne = cmp_ne(got[u][h], make_uint4((uint32_t)x, (uint32_t)(x >> 32), 0, 0));
                        }
                        const uint64_t who = __ballot(ne);
                        if (who && lane == (uint32_t)__builtin_ctzll(who)) atomicMin(&low[j], entry0 + k0 + k);
                    }
                }
            }
        }
    }
    __syncthreads();
    if (wave == 0) cmp_report(low, lane, ok, j0, report0, diff, summary);
}

// Witness bits as packed rows (cw_get_witness_rows*): entry k of the list (w2s points at the range's first entry) of instance
// first + j becomes bit k & 63 of word k >> 6 of rows[j] (MSB: the bits of each byte the other way round), 1 if and only if the
// value is 1.  The shape of the egress kernel above: a workgroup of four waves owns 64 instances (blockIdx.x: no 65 535 limit on
// the instances) x 64 words = 4 096 entries (blockIdx.y).
//   read    lane = instance.  Wave w takes the words w, w + 4, ... of the tile and makes, per word, 64 reads of V[w2s[entry]][instance]:
//           the slot is wave-uniform, every read 512 contiguous bytes, 16 of them issued before the first value is used; the word is
//           the OR of (v == 1) << k.  The last word of a range stops at its last entry: the pad bits are 0.
//   report  a value > 1 gives bit 0; after a ballot one lane reports the wave's lowest such instance, report0 + j, with atomicMin:
//           at most one atomic per wave and word.  `word` may be nullptr.
//   stage   tile[instance][word] with rows of EG_S = 65 words, written column-wise and read row-wise: conflict-free by the bank
//           rules written out above (ds_write_b64, groups of 16 lanes, bank = (a/4) % 32: lane i writes word 65 i + w, bank pair
//           2 ((i + w) % 16); ds_read_b64, groups of 32 lanes: 32 consecutive words, every one of the 64 banks once).
//   write   wave w takes the instances w, w + 4, ...; 64 consecutive words of one row per store, 512 contiguous bytes.
// Instances past `count` and words past ceil(n / 64) are neither read nor written.
template <bool MSB>
__global__ void __launch_bounds__(256) cw64_pack_rows_kernel(const uint64_t *__restrict__ V, const uint32_t *__restrict__ w2s, uint32_t n,
                                                             uint32_t Bp, uint32_t first, uint32_t count, uint32_t report0,
                                                             uint64_t *__restrict__ rows, size_t stride_w, uint32_t *word) {
    __shared__ uint64_t tile[64 * EG_S];
    const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t j0 = blockIdx.x * 64u, w0 = blockIdx.y * 64u;
    const uint32_t n_words = (n >> 6) + ((n & 63u) != 0);
    const uint32_t nw = n_words - w0 < 64u ? n_words - w0 : 64u, nj = count - j0 < 64u ? count - j0 : 64u;
    const bool live = lane < nj;
    const uint64_t *Vj = V + first + j0 + (live ? lane : 0u);
    for (uint32_t w = wave; w < nw; w += 4) {
        const uint32_t k0 = (w0 + w) * 64u, ne = n - k0 < 64u ? n - k0 : 64u;
        uint64_t acc = 0;
        bool bad = false;
        for (uint32_t kb = 0; kb < ne; kb += 16) {
            uint64_t v[16];
#pragma unroll
            for (uint32_t i = 0; i < 16; i++) {
                const uint32_t k = kb + i;
                const uint32_t slot = w2s[k < ne ? k0 + k : k0];     // always an entry of the range: the scalar load needs no branch
                v[i] = k < ne && live ? Vj[(size_t)slot * Bp] : 0;
            }
#pragma unroll
            for (uint32_t i = 0; i < 16; i++) {
                acc |= (uint64_t)(v[i] == 1) << (kb + i);
                bad |= v[i] > 1;
            }
        }
        const uint64_t who = __builtin_amdgcn_ballot_w64(bad);
        if (who && word && lane == (uint32_t)__builtin_ctzll(who)) atomicMin(word, report0 + j0 + lane);
        if (MSB) acc = __builtin_bswap64(__builtin_bitreverse64(acc));
        tile[lane * EG_S + w] = acc;
    }
    __syncthreads();
    uint64_t *o = rows + (size_t)j0 * stride_w + w0;
    if (lane < nw)
        for (uint32_t j = wave; j < nj; j += 4) o[(size_t)j * stride_w + lane] = tile[j * EG_S + lane];
}

// Signal columns out (cw_get_signals_range*): value k of row j = signal signal0 + k of instance first + j as a little-endian
// unsigned integer of W bytes (1, 2, 4, 8 or 32) at out + j * stride + k * W.  Here slot = signal id, so there is no list to go
// through.  The tile of the two kernels above: a workgroup of four waves owns 64 instances (blockIdx.y) x EG_T signals (blockIdx.x).
//   read    lane = instance.  Wave w takes the signals w, w + 4, ... of the tile: the slot is wave-uniform, every read 512
//           contiguous bytes, the 16 loads of a wave issued before the first value is used.  Lanes past `count` and signals past
//           n read nothing and count as 0.
//   report  W < 8: a value >= 2^(8 W) leaves as its low W bytes; after a ballot (under the lane's own row condition: a dead
//           lane holds zeros) one lane reports the wave's lowest such instance, report0 + j, with atomicMin - at most one atomic
//           per wave.  `word` may be nullptr; the caller fills it first.  W = 8 and W = 32 hold every residue.
//   stage   tile[signal][instance] with rows of EG_S = 65 words: the row-wise write and the column-wise 8-byte read of
//           cw64_egress_kernel, conflict-free by the bank arithmetic written out there (from the documented bank rules; no
//           bank-conflict counter pass was taken on this kernel).
//   write   wave w takes the instances w, w + 4, ...; consecutive lanes = consecutive values of ONE row: a store covers nk * W
//           contiguous bytes (W < 4: byte / short stores of consecutive lanes, which the memory pipeline merges per line);
//           W = 32: 16-byte pieces {value, 0} / {0, 0}, two stores per row of the tile, as the egress kernel writes them.
//           Nothing is written behind value n - 1 of a row, and no row past `count`.
// `out` and `stride` are multiples of W (of 16 for W = 32).
template <int W>
__global__ void __launch_bounds__(256) cw64_signals_kernel(const uint64_t *__restrict__ V, uint32_t signal0, uint32_t n, uint32_t Bp,
                                                           uint32_t first, uint32_t count, uint32_t report0, uint8_t *__restrict__ out,
                                                           size_t stride, uint32_t *word) {
    __shared__ uint64_t tile[EG_T * EG_S];
    const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t k0 = blockIdx.x * EG_T, j0 = blockIdx.y * 64u;
    const uint32_t nk = n - k0 < EG_T ? n - k0 : EG_T, nj = count - j0 < 64u ? count - j0 : 64u;
    const bool ok = lane < nj;
    const uint64_t *Vj = V + first + j0 + (ok ? lane : 0u);
    uint64_t v[EG_T / 4];
#pragma unroll
    for (uint32_t i = 0; i < EG_T / 4; i++) {
        const uint32_t k = wave + 4 * i;
        const uint32_t slot = signal0 + k0 + (k < nk ? k : 0u);      // always a signal of the range
        v[i] = k < nk && ok ? Vj[(size_t)slot * Bp] : 0;
    }
    bool wide = false;
#pragma unroll
    for (uint32_t i = 0; i < EG_T / 4; i++) {
        if (W < 8) wide |= (v[i] >> (8 * (W & 7))) != 0;
        tile[(wave + 4 * i) * EG_S + lane] = v[i];
    }
    if (W < 8) {
        const uint64_t who = __builtin_amdgcn_ballot_w64(wide);
        if (who && word && lane == (uint32_t)__builtin_ctzll(who)) atomicMin(word, report0 + j0 + lane);
    }
    __syncthreads();
    for (uint32_t j = wave; j < nj; j += 4) {
        uint8_t *row = out + (size_t)(j0 + j) * stride + (size_t)k0 * W;
        if (W == 32) {
#pragma unroll
            for (uint32_t h = 0; h < 2; h++) {
                const uint32_t p = lane + 64 * h, k = p >> 1;
                if (k < nk) {
                    const uint64_t x = p & 1u ? 0 : tile[k * EG_S + j];
                    ((uint4 *)row)[p] = make_uint4((uint32_t)x, (uint32_t)(x >> 32), 0, 0);
                }
            }
        } else if (lane < nk) {
            const uint64_t x = tile[lane * EG_S + j];
            if (W == 8) ((uint64_t *)row)[lane] = x;
            if (W == 4) ((uint32_t *)row)[lane] = (uint32_t)x;
            if (W == 2) ((uint16_t *)row)[lane] = (uint16_t)x;
            if (W == 1) row[lane] = (uint8_t)x;
        }
    }
}

// R1CS products (cw_get_r1cs_products*): out[j][p][k] = the part's sum of coefficient * w[wire] over the terms of constraint
// row0 + k in instance first + j, for the parts of `parts` in the order A, B, C.  The plan (cw_r1cs_products.h) is in FILE order:
// rowptr[3 row + part] .. rowptr[3 row + part + 1] into terms {slot, 0, coefficient lo, hi}.  The shape of the kernels above: a
// workgroup of four waves owns 64 instances (blockIdx.x) x 64 constraints (blockIdx.y).
//   sum     lane = instance.  Wave w takes the rows w, w + 4, ... of the tile; a term is one scalar load of 16 bytes and one
//           512-byte read of V[slot][instance], four of them issued before the first product; gl_mul / gl_add.  An empty part is 0.
//   stage   tile[instance][row] with rows of EG_S = 65 words, written column-wise and read row-wise: the tile and the bank
//           arithmetic of cw64_pack_rows_kernel.  One part after the other: the terms of A, B and C are disjoint runs, so nothing
//           is walked twice and the tile is reused (a barrier on either side of the stores).
//   write   wave w takes the instances w, w + 4, ...; 64 consecutive rows of one instance and part per store, 512 contiguous bytes.
// `out` points at the launch's first row in instance `first`'s image; `image_rows` = rows of the whole call (the stride of a part),
// n_sel = selected parts.  Instances past `count` and rows past n_rows are neither read nor written.
__global__ void __launch_bounds__(256) cw64_products_kernel(const uint64_t *__restrict__ V, const uint32_t *__restrict__ rowptr,
                                                            const uint4 *__restrict__ terms, uint32_t parts, uint32_t n_sel, uint32_t row0,
                                                            uint32_t n_rows, uint32_t image_rows, uint32_t Bp, uint32_t first, uint32_t count,
                                                            uint64_t *__restrict__ out) {
    __shared__ uint64_t tile[64 * EG_S];
    const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t j0 = blockIdx.x * 64u, k0 = blockIdx.y * 64u;
    const uint32_t nk = n_rows - k0 < 64u ? n_rows - k0 : 64u, nj = count - j0 < 64u ? count - j0 : 64u;
    const bool live = lane < nj;
    const uint64_t *Vj = V + first + j0 + (live ? lane : 0u);
    uint64_t *o = out + (size_t)j0 * n_sel * image_rows + k0;
    uint32_t sel = 0;
    for (uint32_t part = 0; part < 3; part++) {
        if (!((parts >> part) & 1u)) continue;
        for (uint32_t k = wave; k < nk; k += 4) {
            const uint32_t *rp = rowptr + (size_t)(row0 + k0 + k) * 3 + part;
            const uint32_t t0 = rp[0], t1 = rp[1];
            uint64_t acc = 0;
            for (uint32_t t = t0; t < t1; t += 4) {
                uint4 x[4];
                uint64_t v[4];
#pragma unroll
                for (uint32_t i = 0; i < 4; i++) {
                    x[i] = terms[t + i < t1 ? t + i : t];            // always a term of the part: the scalar load needs no branch
                    v[i] = Vj[(size_t)x[i].x * Bp];
                }
#pragma unroll
                for (uint32_t i = 0; i < 4; i++)
                    if (t + i < t1) acc = gl_add(acc, gl_mul(v[i], ((uint64_t)x[i].w << 32) | x[i].z));
            }
            tile[lane * EG_S + k] = acc;
        }
        __syncthreads();
        if (lane < nk)
            for (uint32_t j = wave; j < nj; j += 4) o[((size_t)j * n_sel + sel) * image_rows + lane] = tile[j * EG_S + lane];
        __syncthreads();
        sel++;
    }
}

// The transpose INTO the value table, the egress transpose in the other direction, in two uses:
//   bulk ingest (WIT = false): [count][n][EB] bytes of inputs, EB = 32 (the boundary's element) or 8 (this runtime's), input k of
//           instance j into V[slot0 + k][first + j];
//   supplied witnesses (WIT = true; cw_set_witnesses*, cw_read_wtns*): [count][n][EB] bytes of witnesses, EB = 8 (this runtime's
//           .wtns element) or 32, entry k of instance j into V[w2s[k]][first + j] - the mirror image of cw64_egress_kernel.
// cw64_ingest_kernel gives consecutive lanes consecutive INSTANCES: every lane reads another row of the image, n * EB bytes from
// its neighbour's - 64 cache lines for 512 useful bytes, and each of those lines is asked for again by the workgroups of up to
// n other inputs.  Here a workgroup of four waves owns 64 instances x EG_T entries, and no other workgroup requests a byte of
// its part of the image:
//   read    wave w takes the instances j = w, w + 4, ... of the tile; consecutive lanes read consecutive pieces of the row
//           in[j0 + j][k0 .. k0 + EG_T): 8-byte form: the 64 values, 512 contiguous bytes (8-byte loads: with n odd a row
//           starts on an 8-byte boundary only); 32-byte form: 16-byte pieces, lane l holds words {0, 1} (l even) or {2, 3} (l odd)
//           of value l / 2 (+ 32 in the second load), 1 KiB contiguous per load, two loads per row.  `in` must be 8-byte aligned
//           in the 8-byte form and 16-byte aligned in the 32-byte form.  The 16 (32) loads of a wave are issued before the first
//           value is used.
//   reduce  8-byte form: one conditional subtraction of p.  32-byte form: w0 + w1 e + w2 e^2 + w3 e^3 with e = 2^32 - 1 = 2^64
//           (mod p), every word brought below p first.  The even lane forms w0 + w1 e, the odd lane (w2 + w3 e) e^2, and one
//           exchange between neighbours adds the two.  Nearly every real value has words 1..3 zero: a ballot over the wave
//           (even lanes: w1, odd lanes: w2 | w3) skips multiplications and exchange for the whole load - the branch is
//           wave-uniform, and a wave pays for the long form only for the loads that hold such a value.
//   stage   tile[k][j] in LDS with rows of EG_S = 65 words of 8 bytes, the egress kernel's tile written and read the other way
//           round.  Column-wise write (ds_write_b64: four groups of 16 consecutive lanes, bank = (a/4) % 32): lane l writes word
//           l' * 65 + j with l' = l (8-byte form) or l / 2 (32-byte form, even lanes only), dwords 130 l' + 2 j and the next one,
//           bank pair 2 ((l' + j) % 16): the 16 (or 8) rows l' of a group are consecutive and fall on distinct pairs, every
//           bank at most once.  With rows of 64 words all lanes of a group would hit pair 2 (j % 16): 16-way.  Row-wise read
//           (ds_read_b64: two groups of 32 lanes, bank = (a/4) % 64): a group reads 32 consecutive words = 64 consecutive dwords,
//           every bank once, whatever the row's start.
//           (This is arithmetic from the documented bank rules, as the egress comment is: nobody has taken a bank-conflict
//           counter pass on either kernel.)
//   write   wave w takes the entries k = w, w + 4, ...; its 64 lanes store 64 consecutive instances of the entry's slot: one
//           512-byte store, as the evaluation kernel writes its results.  `first` need not be a multiple of 64: a row of V is
//           8-byte aligned wherever it starts.
// Lanes past `count` and entries past n neither read nor write; nothing is read past the end of the image.
// The supplied-witness use differs in the slot and in a check, and in nothing else:
//   write   the slot of entry k0 + k is w2s[k0 + k], not slot0 + k0 + k: wave-uniform, a scalar load with the index clamped to
//           the list as the egress kernel clamps it, the 16 loads of a wave ahead of its 16 stores.  Entry 0 is NOT stored:
//           slot 0 keeps the 1 of cw64_init_kernel, so that the constant terms of the R1CS check stay meaningful for the other
//           wires of a witness whose entry 0 is wrong.
//   check   a checker must not quietly repair what it is given.  The reduced value is stored (the check cannot run without
//           one), and CW_ST_BAD_WITNESS is or'ed into status[first + j] when a value of instance j was not canonical (8-byte
//           form: >= p; 32-byte form: word 0 >= p or any of words 1..3 set) or its entry 0 is not 1.  On the read side a WAVE
//           holds one instance's row of the tile per load: one ballot per load (the 32-byte form's is the ballot that skips the
//           long reduction) sets bit i of a wave-uniform mask, i = the wave's i-th instance, and lane i issues the atomicOr -
//           at most 16 per wave, none for well-formed witnesses.  Another workgroup may report the same instance for another
//           entry tile: or is idempotent.  (The registers of lanes that read nothing stay 0, which no test flags - the entry-0
//           test is under the row's own condition.)
// The bulk ingest pays for none of it: no ballot for `bad`, no atomicOr, no load from w2s (w2s and status are null there).
template <int EB, bool WIT>
__global__ void __launch_bounds__(256) cw64_transpose_in_kernel(const uint8_t *__restrict__ in, uint64_t *__restrict__ V,
                                                                const uint32_t *__restrict__ w2s, uint32_t slot0, uint32_t n, uint32_t Bp,
                                                                uint32_t first, uint32_t count, uint32_t *status) {
    __shared__ uint64_t tile[EG_T * EG_S];
    const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t k0 = blockIdx.x * EG_T, j0 = blockIdx.y * 64u;
    const uint32_t nk = n - k0 < EG_T ? n - k0 : EG_T, nj = count - j0 < 64u ? count - j0 : 64u;
    const bool entry0 = WIT && k0 == 0 && lane == 0;                   // this lane's (first) piece is the head of entry 0
    uint32_t badmask = 0;                                              // bit i: instance wave + 4 i of the tile is malformed (wave-uniform)
    // The loads of a wave stand in ONE block of straight-line code under the lane's own condition, the same for all of them (the
    // row bases are wave-uniform: scalar registers, the lane is the offset).  A condition per load would make every load a branch
    // of its own that waits for its data before the next one is issued.  The last instance tile of a batch (nj < 64) has a row
    // condition too and takes that slower form.
    if (EB == 8) {
        const uint64_t *t0 = (const uint64_t *)in + (size_t)j0 * n + k0;
        uint64_t v[64 / 4] = {};
        if (lane < nk) {
            if (nj == 64u) {
#pragma unroll
                for (uint32_t i = 0; i < 64 / 4; i++) v[i] = t0[(size_t)(wave + 4 * i) * n + lane];
            } else {
#pragma unroll
                for (uint32_t i = 0; i < 64 / 4; i++)
                    if (wave + 4 * i < nj) v[i] = t0[(size_t)(wave + 4 * i) * n + lane];
            }
        }
#pragma unroll
        for (uint32_t i = 0; i < 64 / 4; i++) {
            if (WIT) {
                const bool bad = v[i] >= GL_P || (entry0 && wave + 4 * i < nj && v[i] != 1);
                if (__builtin_amdgcn_ballot_w64(bad)) badmask |= 1u << i;
            }
            tile[lane * EG_S + wave + 4 * i] = gl_wrap(v[i]);
        }
    } else {
        const uint4 *t0 = (const uint4 *)in + ((size_t)j0 * n + k0) * 2;
        const bool odd = lane & 1u;
        uint4 v[64 / 4][2] = {};
        if (nj == 64u && nk == EG_T) {                                 // a full tile: all 32 loads of the wave in one block
#pragma unroll
            for (uint32_t i = 0; i < 64 / 4; i++) {
                v[i][0] = t0[(size_t)(wave + 4 * i) * n * 2 + lane];
                v[i][1] = t0[(size_t)(wave + 4 * i) * n * 2 + lane + 64];
            }
        } else
#pragma unroll
        for (uint32_t h = 0; h < 2; h++) {
            if (((lane + 64 * h) >> 1) < nk) {
                if (nj == 64u) {
#pragma unroll
                    for (uint32_t i = 0; i < 64 / 4; i++) v[i][h] = t0[(size_t)(wave + 4 * i) * n * 2 + lane + 64 * h];
                } else {
#pragma unroll
                    for (uint32_t i = 0; i < 64 / 4; i++)
                        if (wave + 4 * i < nj) v[i][h] = t0[(size_t)(wave + 4 * i) * n * 2 + lane + 64 * h];
                }
            }
        }
        // 2^64 = 2^32 - 1, 2^128 = (2^32 - 1)^2 (mod p)
        const uint64_t e = 0xFFFFFFFFull, e2 = gl_mul(e, e);
#pragma unroll
        for (uint32_t i = 0; i < 64 / 4; i++) {
#pragma unroll
            for (uint32_t h = 0; h < 2; h++) {
                const uint64_t lo = ((uint64_t)v[i][h].y << 32) | v[i][h].x, hi = ((uint64_t)v[i][h].w << 32) | v[i][h].z;
                uint64_t r = gl_wrap(lo);
                if (__builtin_amdgcn_ballot_w64(odd ? (lo | hi) != 0 : hi != 0)) {         // words 1..3 set: the long form (WIT: malformed)
                    if (WIT) badmask |= 1u << i;
                    uint64_t part = gl_add(r, gl_mul(gl_wrap(hi), e));
                    if (odd) part = gl_mul(part, e2);
                    r = gl_add(part, (uint64_t)__shfl_xor((unsigned long long)part, 1));
                }
                if (WIT) {
                    const bool bad = !odd && (lo >= GL_P || (h == 0 && entry0 && wave + 4 * i < nj && lo != 1));
                    if (__builtin_amdgcn_ballot_w64(bad)) badmask |= 1u << i;
                }
                if (!odd) tile[((lane >> 1) + 32 * h) * EG_S + wave + 4 * i] = r;
            }
        }
    }
    if (WIT && lane < 64 / 4 && ((badmask >> lane) & 1u)) atomicOr(&status[first + j0 + wave + 4 * lane], CW_ST_BAD_WITNESS);
    __syncthreads();
    // The write is where the slot differs, and each use keeps its own loop.  The witness list's: unrolled, the 16 scalar loads
    // ahead of the stores, through the lane's own pointer into the row.  The inputs': rolled, the instance added per store.
    // (A 64-bit per-lane value that outlives the barrier costs the 8-byte bulk ingest 24 VGPRs, 42 -> 66: its zero-extended lane
    // is computed above the load block, and the compiler then keeps the zeros of v[] for the lanes past nk and the loaded values
    // in registers of their own, joined by copies, instead of loading over the zeros.)
    if (WIT) {
        uint64_t *Vj = V + first + j0 + lane;
        uint32_t slot[EG_T / 4];
#pragma unroll
        for (uint32_t i = 0; i < EG_T / 4; i++) {
            const uint32_t k = wave + 4 * i;
            slot[i] = w2s[k < nk ? k0 + k : k0];                     // always an entry of the list: the scalar load needs no branch
        }
#pragma unroll
        for (uint32_t i = 0; i < EG_T / 4; i++) {
            const uint32_t k = wave + 4 * i;
            if (k < nk && k0 + k != 0 && lane < nj) Vj[(size_t)slot[i] * Bp] = tile[k * EG_S + lane];
        }
    } else {
        for (uint32_t k = wave; k < nk; k += 4)
            if (lane < nj) V[(size_t)(slot0 + k0 + k) * Bp + first + j0 + lane] = tile[k * EG_S + lane];
    }
}

// ---- launch wrappers -----------------------------------------------------------------------------------------------------
hipError_t cwk64_init(hipStream_t s, void *V, uint32_t Bp, uint32_t *status, uint32_t *first_bad) {
    hipLaunchKernelGGL(cw64_init_kernel, dim3((Bp + 255) / 256), dim3(256), 0, s, (uint64_t *)V, Bp, status, first_bad);
    return hipGetLastError();
}
// elem_bytes = 8 or 32; the input index is a grid dimension: at most 65 535 inputs (cwk64_ingest_tiled has no such limit)
hipError_t cwk64_ingest(hipStream_t s, const void *in, void *V, uint32_t input_start, uint32_t n_in, uint32_t batch, uint32_t Bp,
                        uint32_t elem_bytes) {
    if (elem_bytes != 8 && elem_bytes != 32) return hipErrorInvalidValue;
    if (!n_in) return hipSuccess;
    if (n_in > 65535u) return hipErrorInvalidValue;
    const dim3 grid((batch + 255) / 256, n_in);
    if (elem_bytes == 8)
        hipLaunchKernelGGL(cw64_ingest_kernel<8>, grid, dim3(256), 0, s, (const uint64_t *)in, (uint64_t *)V, input_start, n_in, batch, Bp);
    else
        hipLaunchKernelGGL(cw64_ingest_kernel<32>, grid, dim3(256), 0, s, (const uint64_t *)in, (uint64_t *)V, input_start, n_in, batch, Bp);
    return hipGetLastError();
}
// Input columns (cw_set_inputs_range*, cw_set_input_column*) into this runtime's image of 8-byte values (cw_columns.hip.h): an
// 8-byte value >= p takes the one subtraction of cw64_ingest_kernel<8>, a 32-byte value the reduction of cw64_ingest_kernel<32>
struct Cw64ColumnsReduce {
    static __device__ __forceinline__ uint64_t wrap(uint64_t v) { return gl_wrap(v); }
    static __device__ __forceinline__ uint64_t reduce4(uint64_t w0, uint64_t w1, uint64_t w2, uint64_t w3) { return gl_reduce256(w0, w1, w2, w3); }
};
hipError_t cwk64_columns(hipStream_t s, const void *d_values, size_t stride, uint32_t n, uint32_t count, uint32_t width, void *out,
                         size_t out_stride) {
    return cw_columns_launch<8, Cw64ColumnsReduce>(s, d_values, stride, n, count, width, out, out_stride);
}
// The launches of cw64_transpose_in_kernel: elem_bytes = 8 (`in` 8-byte aligned) or 32 (16-byte aligned); a launch holds at most
// 65 535 tiles of 64 instances (gridDim.y), larger counts are split as cwk64_egress splits them, and nothing more is launched
// behind a launch that failed; the entry tiles are gridDim.x, so n is not limited
static hipError_t transpose_in(bool wit, hipStream_t s, const void *in, void *V, const uint32_t *w2s, uint32_t slot0, uint32_t n, uint32_t Bp,
                               uint32_t first, uint32_t count, uint32_t *status, uint32_t elem_bytes) {
    if (elem_bytes != 8 && elem_bytes != 32) return hipErrorInvalidValue;
    if ((uintptr_t)in & (elem_bytes == 32 ? 15 : 7)) return hipErrorInvalidValue;
    if (!n || !count) return hipSuccess;
    const auto kernel = wit ? (elem_bytes == 8 ? cw64_transpose_in_kernel<8, true> : cw64_transpose_in_kernel<32, true>)
                            : (elem_bytes == 8 ? cw64_transpose_in_kernel<8, false> : cw64_transpose_in_kernel<32, false>);
    return cw_pieces(count, 65535u * 64u, [&](uint32_t done, uint32_t m) {
        hipLaunchKernelGGL(kernel, dim3((n + EG_T - 1) / EG_T, (m + 63) / 64), dim3(256), 0, s,
                           (const uint8_t *)in + (size_t)done * n * elem_bytes, (uint64_t *)V, w2s, slot0, n, Bp, first + done, m, status);
        return hipGetLastError();
    });
}
// bulk inputs [batch][n_in][elem_bytes] into the slots from input_start, all columns of V
hipError_t cwk64_ingest_tiled(hipStream_t s, const void *in, void *V, uint32_t input_start, uint32_t n_in, uint32_t batch, uint32_t Bp,
                              uint32_t elem_bytes) {
    return transpose_in(false, s, in, V, nullptr, input_start, n_in, Bp, 0, batch, nullptr, elem_bytes);
}
// supplied witnesses [count][n_wit][elem_bytes] into the columns first .. first + count of V
hipError_t cwk64_wit_ingest(hipStream_t s, const void *in, void *V, const uint32_t *w2s, uint32_t n_wit, uint32_t Bp, uint32_t first,
                            uint32_t count, uint32_t *status, uint32_t elem_bytes) {
    return transpose_in(true, s, in, V, w2s, 0, n_wit, Bp, first, count, status, elem_bytes);
}
// calls: 0 = no O_CALL row in the program, 1 = register windows in the table, 2 = in LDS (lds_bytes = 512 x the registers of the
// largest function, at most 64 KiB: what a launch gets as dynamic LDS without a function attribute)
hipError_t cwk64_eval(hipStream_t s, const void *rows, uint32_t n_rows, const void *consts, void *V, uint32_t Bp, uint32_t batch,
                      uint32_t *status, const void *ftab, const void *fcode, uint32_t calls, uint32_t lds_bytes) {
    if (calls > 2 || (calls == 2 ? lds_bytes == 0 || lds_bytes > 65536u : lds_bytes != 0)) return hipErrorInvalidValue;
    const dim3 grid((batch + 63) / 64);
#define CW64_EVAL(C) hipLaunchKernelGGL(cw64_eval_kernel<C>, grid, dim3(64), lds_bytes, s, (const uint4 *)rows, n_rows, (const uint64_t *)consts, \
                                        (uint64_t *)V, Bp, batch, status, (const uint4 *)ftab, (const uint4 *)fcode)
    if (calls == 0) CW64_EVAL(0);
    else if (calls == 1) CW64_EVAL(1);
    else CW64_EVAL(2);
#undef CW64_EVAL
    return hipGetLastError();
}
hipError_t cwk64_r1cs(hipStream_t s, const void *chunks, uint32_t n_chunks, const void *terms, const void *V, uint32_t Bp, uint32_t batch,
                      uint32_t *status, uint32_t *first_bad) {
    if (!n_chunks) return hipSuccess;
    hipLaunchKernelGGL(cw64_r1cs_kernel, dim3((batch + 63) / 64, n_chunks < 65535u ? n_chunks : 65535u), dim3(64), 0, s, (const uint4 *)chunks,
                       n_chunks, (const uint4 *)terms, (const uint64_t *)V, Bp, batch, status, first_bad);
    return hipGetLastError();
}
// the instance is a grid dimension: launches of at most 65 535 instances, none behind one that failed
hipError_t cwk64_gather(hipStream_t s, const void *V, const uint32_t *w2s, uint32_t n_wit, uint32_t Bp, uint32_t first, uint32_t count,
                        void *out) {
    if (!n_wit) return hipSuccess;
    return cw_pieces(count, 65535u, [&](uint32_t done, uint32_t n) {
        hipLaunchKernelGGL(cw64_gather_kernel, dim3((n_wit + 255) / 256, n), dim3(256), 0, s, (const uint64_t *)V, w2s, n_wit, Bp, first + done,
                           n, (uint64_t *)out + (size_t)done * n_wit * 4);
        return hipGetLastError();
    });
}
// The launches of cw64_egress_kernel: `count` instances from `first`, or (at) `count` positions of the list idx, cut at *d_n,
// whose indices may name the instances below `batch`.  elem_bytes = 8 or 32 (32: `out` 16-byte aligned; a list also wants an
// 8-byte image 8-byte aligned).  A launch holds at most 65 535 tiles of 64 instances or positions (gridDim.y), larger counts are
// split as above; the entry tiles are gridDim.x, so n_wit is not limited.
static hipError_t egress(bool at, hipStream_t s, const void *V, const uint32_t *w2s, uint32_t n_wit, uint32_t Bp, uint32_t first, uint32_t count,
                         void *out, uint32_t elem_bytes, uint32_t batch, const uint32_t *idx, const uint32_t *d_n, uint32_t *bad) {
    if (elem_bytes != 8 && elem_bytes != 32) return hipErrorInvalidValue;
    if (elem_bytes == 32 && ((uintptr_t)out & 15)) return hipErrorInvalidValue;
    if (at && (((uintptr_t)out & 7) || (((uintptr_t)idx | (uintptr_t)d_n | (uintptr_t)bad) & 3))) return hipErrorInvalidValue;
    if (!n_wit) return hipSuccess;
    const auto kernel = at ? (elem_bytes == 8 ? cw64_egress_kernel<8, true> : cw64_egress_kernel<32, true>)
                           : (elem_bytes == 8 ? cw64_egress_kernel<8, false> : cw64_egress_kernel<32, false>);
    return cw_pieces(count, 65535u * 64u, [&](uint32_t done, uint32_t m) {
        hipLaunchKernelGGL(kernel, dim3((n_wit + EG_T - 1) / EG_T, (m + 63) / 64), dim3(256), 0, s, (const uint64_t *)V, w2s, n_wit, Bp,
                           first + done, m, (uint8_t *)out + (size_t)done * n_wit * elem_bytes, batch, at ? idx + done : nullptr, done, d_n, bad);
        return hipGetLastError();
    });
}
hipError_t cwk64_egress(hipStream_t s, const void *V, const uint32_t *w2s, uint32_t n_wit, uint32_t Bp, uint32_t first, uint32_t count,
                        void *out, uint32_t elem_bytes) {
    return egress(false, s, V, w2s, n_wit, Bp, first, count, out, elem_bytes, 0, nullptr, nullptr, nullptr);
}
// `bad` (or nullptr) takes an atomicMin of the lowest position whose index is >= batch; the caller fills it first.
hipError_t cwk64_egress_at(hipStream_t s, const void *V, const uint32_t *w2s, uint32_t n_wit, uint32_t Bp, uint32_t batch, const uint32_t *d_idx,
                           uint32_t n_idx, const uint32_t *d_n_idx, void *d_out, uint32_t elem_bytes, uint32_t *d_bad) {
    return egress(true, s, V, w2s, n_wit, Bp, 0, n_idx, d_out, elem_bytes, batch, d_idx, d_n_idx, d_bad);
}
// The launches of cw64_compare_kernel: the grid and the pieces of the range egress; `image`, `diff` and report0 move with the
// piece.  elem_bytes = 8 (`image` 8-byte aligned) or 32 (16-byte aligned).
hipError_t cwk64_compare(hipStream_t s, const void *V, const uint32_t *w2s, uint32_t n_wit, uint32_t Bp, uint32_t first, uint32_t count,
                         uint32_t entry0, uint32_t report0, const void *image, uint32_t elem_bytes, uint32_t *diff, uint32_t *summary) {
    if (elem_bytes != 8 && elem_bytes != 32) return hipErrorInvalidValue;
    if (((uintptr_t)image & (elem_bytes == 8 ? 7 : 15)) || (((uintptr_t)diff | (uintptr_t)summary) & 3)) return hipErrorInvalidValue;
    if (!n_wit) return hipSuccess;
    const auto kernel = elem_bytes == 8 ? cw64_compare_kernel<8> : cw64_compare_kernel<32>;
    return cw_pieces(count, 65535u * 64u, [&](uint32_t done, uint32_t m) {
        hipLaunchKernelGGL(kernel, dim3((n_wit + EG_T - 1) / EG_T, (m + 63) / 64), dim3(256), 0, s, (const uint64_t *)V, w2s, n_wit, Bp,
                           first + done, m, (const uint8_t *)image + (size_t)done * n_wit * elem_bytes, entry0, report0 + done, diff + done,
                           summary);
        return hipGetLastError();
    });
}
// packed rows of witness bits: instance tiles in gridDim.x, word tiles of 4 096 entries in gridDim.y: one launch.  `word` (or
// nullptr) takes an atomicMin of report0 + j for every instance j of the launch that held a value > 1; the caller fills it first.
hipError_t cwk64_pack_rows(hipStream_t s, const void *V, const uint32_t *w2s, uint32_t n, uint32_t Bp, uint32_t first, uint32_t count,
                           uint32_t report0, bool msb, void *d_rows, size_t stride, uint32_t *d_word) {
    if (n == 0 || count == 0) return hipSuccess;
    const uint32_t n_words = (n >> 6) + ((n & 63u) != 0);
    if (((uintptr_t)d_rows & 7) || (stride & 7) || stride / 8 < n_words || ((uintptr_t)d_word & 3)) return hipErrorInvalidValue;
    const dim3 grid((count >> 6) + ((count & 63u) != 0), (n_words + 63) / 64);
    if (grid.y > 65535u) return hipErrorInvalidValue;
    const auto kernel = msb ? cw64_pack_rows_kernel<true> : cw64_pack_rows_kernel<false>;
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, s, (const uint64_t *)V, w2s, n, Bp, first, count, report0, (uint64_t *)d_rows, stride / 8,
                       d_word);
    return hipGetLastError();
}
// signal columns out: signal tiles of EG_T in gridDim.x (n is not limited), tiles of 64 instances in gridDim.y - a launch holds at
// most 65 535 of those, a larger count goes in several launches (cw_pieces.h), none behind one that failed.  `word` (or nullptr)
// takes an atomicMin of report0 + j for every instance j that held a value >= 2^(8 elem_bytes); the caller fills it first.
hipError_t cwk64_signals(hipStream_t s, const void *V, uint32_t signal0, uint32_t n, uint32_t Bp, uint32_t first, uint32_t count,
                         uint32_t report0, void *d_values, size_t stride, uint32_t elem_bytes, uint32_t *d_word) {
    if (n == 0 || count == 0) return hipSuccess;
    const size_t a = elem_bytes == 32 ? 16 : elem_bytes;
    const auto kernel = elem_bytes == 1 ? cw64_signals_kernel<1> : elem_bytes == 2 ? cw64_signals_kernel<2> : elem_bytes == 4 ? cw64_signals_kernel<4>
                      : elem_bytes == 8 ? cw64_signals_kernel<8> : elem_bytes == 32 ? cw64_signals_kernel<32> : nullptr;
    if (!kernel || ((uintptr_t)d_values % a) || (stride % a) || stride / elem_bytes < n || ((uintptr_t)d_word & 3)) return hipErrorInvalidValue;
    return cw_pieces(count, 65535u * 64u, [&](uint32_t done, uint32_t m) {
        hipLaunchKernelGGL(kernel, dim3((n + EG_T - 1) / EG_T, (m + 63) / 64), dim3(256), 0, s, (const uint64_t *)V, signal0, n, Bp, first + done,
                           m, report0 + done, (uint8_t *)d_values + (size_t)done * stride, stride, d_word);
        return hipGetLastError();
    });
}
// R1CS products [count][n_sel][n_rows] of 8-byte residues: instance tiles in gridDim.x, row tiles of 64 in gridDim.y, a range of
// more than 65 535 tiles in several launches (cw_r1cs_products.h row_pieces), none behind one that failed
hipError_t cwk64_products(hipStream_t s, const void *V, const uint32_t *rowptr, const void *terms, uint32_t parts, uint32_t row0, uint32_t n_rows,
                          uint32_t Bp, uint32_t first, uint32_t count, void *d_out) {
    const uint32_t n_sel = cwprod::n_parts(parts);
    if (n_rows == 0 || count == 0) return hipSuccess;
    if (n_sel == 0 || (parts & ~cwprod::PART_ALL) || ((uintptr_t)d_out & 7)) return hipErrorInvalidValue;
    return cwprod::row_pieces(n_rows, cwprod::ROWS64, [&](uint32_t off, uint32_t m) {
        hipLaunchKernelGGL(cw64_products_kernel, dim3((count >> 6) + ((count & 63u) != 0), cwprod::row_tiles(m, cwprod::ROWS64)), dim3(256), 0, s,
                           (const uint64_t *)V, rowptr, (const uint4 *)terms, parts, n_sel, row0 + off, m, n_rows, Bp, first, count,
                           (uint64_t *)d_out + off);
        return hipGetLastError();
    });
}

// ---- witness digests (cw_get_wtns_digests*, cw_wtns_digest.h) ----------------------------------------------------------------
// SHA-256 of the .wtns file of every instance, n8 = 8: lane = instance, a wave owns the table group (first >> 6) + blockIdx.x and
// walks the message with cwdig::walk - 8 elements per block, V[w2s[k]][instance], the slot a scalar load, 512 contiguous bytes per
// wave and element; the eight elements of block j + 1 are requested before the rounds of block j.  Also served in the
// supplied-witness state.  Lanes outside [first, first + count) read the padded table (Bp is a multiple of 256) and store nothing.
struct Digest64Src {
    static constexpr uint32_t EW = 2, H = 13, RUN = 1;
    typedef uint64_t Raw;
    const uint64_t *__restrict__ Vj;                      // column of the lane's instance
    const uint32_t *__restrict__ w2s;
    uint32_t Bp;
    __device__ __forceinline__ Raw fetch(uint32_t k) const { return Vj[(size_t)w2s[k] * Bp]; }
    __device__ __forceinline__ void words(const Raw &r, uint32_t w[2]) const {
        w[0] = (uint32_t)r;
        w[1] = (uint32_t)(r >> 32);
    }
};
__global__ void __launch_bounds__(64) cw64_wtns_digest_kernel(const uint64_t *__restrict__ V, const uint32_t *__restrict__ w2s, uint32_t Bp,
                                                              uint32_t first, uint32_t count, uint4 *__restrict__ out, cwdig::Plan plan) {
    const uint32_t inst = cwdig::wave_group(first, blockIdx.x) * 64u + threadIdx.x;
    Digest64Src src{V + inst, w2s, Bp};
    uint32_t st[8];
    cwdig::walk(plan, src, st);
    cwdig::store_digest(out, first, count, inst, st);
}
// digests [count][32] of the instances [first, first + count): one wave per table group of the range; d_out 16-byte aligned
hipError_t cwk64_wtns_digest(hipStream_t s, const void *V, const uint32_t *w2s, uint32_t Bp, uint32_t first, uint32_t count, void *d_out,
                             const cwdig::Plan &plan) {
    if (count == 0) return hipSuccess;
    if (((uintptr_t)d_out & 15) || plan.n8 != 8 || plan.n_witness == 0 || (uint64_t)first + count > Bp) return hipErrorInvalidValue;
    hipLaunchKernelGGL(cw64_wtns_digest_kernel, dim3(cwdig::n_groups(first, count)), dim3(64), 0, s, (const uint64_t *)V, w2s, Bp, first, count,
                       (uint4 *)d_out, plan);
    return hipGetLastError();
}
