// cw_fn64.h — the function section of a version-2 tape of the 64-bit runtime (hip_elements/lower64.py write_tape64), read and
// checked in one pass.  The device interpreter (cw64.hip cw64_call) trusts every number in it: registers address the call's
// window, constants the constant table, jumps the function's own code.  So everything is checked here, once, over plain bytes.
// No HIP in here: tests/host/fn64_test.cpp.
//
//   u32 n_functions | per function { u32 n_regs | u32 n_ins | n_ins x { u32 opcode, dst, a, b } }
//   opcode: 0 .. 23 = the arithmetic operators of the row format (O_COPY .. O_LNOT), or F_JZ / F_JMP / F_LDX / F_STX / F_RET
//   operand: a register number, or FN_CONST | index into the tape's constant table
//   F_LDX dst <- reg[a + reg[idx]], F_STX reg[dst + reg[idx]] <- a: b = idx | length << 16, and the array [base, base + length)
//   lies inside the window
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>
#include "cw_tape.h"

#define CW64_O_CALL 27u                    // row opcode of a call (cw64.hip)
#define CW64_FN_ALU_LAST 23u               // O_LNOT: the last operator a function body may use
#define CW64_FN_MAX_FUNCTIONS (1u << 16)
#define CW64_FN_MAX_INS (1u << 24)         // instructions of all functions together

struct CwFn64 {
    std::vector<uint32_t> tab;             // per function {first instruction, n instructions, n registers, 0}
    std::vector<uint32_t> code;            // 4 words per instruction, all functions concatenated
    uint32_t max_regs = 0;
};

// Parses the section at p[0 .. n).  Returns nullptr and the bytes consumed in *used, or the reason the section is refused.
static inline const char *cw_fn64_parse(const uint8_t *p, size_t n, uint32_t n_consts, CwFn64 *out, size_t *used) {
    size_t off = 0;
    auto u32 = [&](uint32_t *v) {
        if (n - off < 4) return false;
        memcpy(v, p + off, 4);
        off += 4;
        return true;
    };
    uint32_t nf;
    if (!u32(&nf)) return "function section truncated";
    if (nf > CW64_FN_MAX_FUNCTIONS) return "too many functions";
    out->tab.clear();
    out->code.clear();
    out->max_regs = 0;
    for (uint32_t f = 0; f < nf; f++) {
        uint32_t n_regs, n_ins;
        if (!u32(&n_regs) || !u32(&n_ins)) return "function section truncated";
        if (n_regs == 0 || n_regs >= (1u << 16)) return "function: register count";
        if (n_ins == 0 || n_ins > CW64_FN_MAX_INS - out->code.size() / 4) return "function: instruction count";
        if ((n - off) / 16 < n_ins) return "function section truncated";
        const size_t first = out->code.size() / 4;
        out->code.resize((first + n_ins) * 4);
        uint32_t *code = &out->code[first * 4];
        memcpy(code, p + off, (size_t)n_ins * 16);
        off += (size_t)n_ins * 16;
        auto reg_ok = [&](uint32_t r) { return r < n_regs; };
        auto opnd_ok = [&](uint32_t x) { return x & FN_CONST ? (x & 0x7FFFFFFFu) < n_consts : x < n_regs; };
        for (uint32_t i = 0; i < n_ins; i++) {
            const uint32_t op = code[4 * i], d = code[4 * i + 1], a = code[4 * i + 2], b = code[4 * i + 3];
            if (op <= CW64_FN_ALU_LAST) {
                if (!reg_ok(d) || !opnd_ok(a) || !opnd_ok(b)) return "function: operand out of range";
            } else if (op == F_RET) {
            } else if (op == F_JMP) {
                if (d >= n_ins) return "function: jump target";
            } else if (op == F_JZ) {
                if (d >= n_ins) return "function: jump target";
                if (!opnd_ok(a)) return "function: operand out of range";
            } else if (op == F_LDX || op == F_STX) {
                const uint32_t idx = b & 0xFFFFu, len = b >> 16, base = op == F_LDX ? a : d;
                if (!reg_ok(idx) || len == 0 || base >= n_regs || len > n_regs - base) return "function: array leaves the window";
                if (op == F_LDX ? !reg_ok(d) : !opnd_ok(a)) return "function: operand out of range";
            } else
                return "function: unknown opcode";
        }
        const uint32_t last = code[4 * (n_ins - 1)];
        if (last != F_RET && last != F_JMP) return "function: the code can run off its end";
        out->tab.insert(out->tab.end(), {(uint32_t)first, n_ins, n_regs, 0u});
        if (n_regs > out->max_regs) out->max_regs = n_regs;
    }
    *used = off;
    return nullptr;
}
