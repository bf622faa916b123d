"""hip_elements for the 64-bit runtime (`--prime goldilocks`): the flat witness program as one row per operation.

The reference has a second runtime for this prime: `code_producers/src/c_elements/goldilocks/fr.hpp` (a field element is a
plain uint64) with `common64/{main,calcwit}.cpp`, value-style emitted code and a `.dat` without a constants section
(c_code_generator.rs:838-841; constants are literals, value_bucket.rs:82-86).  The 256-bit engine's lowering is built on
"q is large" (reduction-free short products, lazy integer sums, bit extraction, Montgomery radix 2^261) - none of it applies,
and with one register per value none of it is needed: `csrc/cw64.hip` executes the flat code as it stands.

  row = 8 x u32: op | dk << 8 | ak << 10 | bk << 12 | ck << 14 (kind 0 = table slot, 2 = constant, 3 = none); dst; a; b; c;
                 index of the flat operation (what a failed check reports); 0; 0
  slots: signal s = slot s (slot 0 = the constant 1), logged value j = n_signals + j, temporary t = n_signals + n_logv + t

`log(...)`: every logged value is a COPY into a HIDDEN slot behind the circuit's signals (flatten.code_with_log_copies); the
witness list does not name those slots, the tape carries the statements (flatten.log_program) and `cw_get_log` formats them.

Run-time functions (frontend/rtcode.py: loops, branches and array indices that depend on values): a CALL is one row, O_CALL with
a = function id and b = slot of register 0 of the call's window, the run of n_regs consecutive temporaries the flat code
reserves.  The bytecode travels as lower._encode_function writes it for the 256-bit engine - 4 x u32 per instruction, the F_*
numbers of csrc/cw_tape.h, the F_LDX / F_STX packing, FN_CONST | index for a constant operand - with two differences: an
arithmetic instruction carries the 64-bit kernel's own operator number (the flat numbering, O_* of csrc/cw64.hip), and the
field division is O_DIV (F_DIV exists because the 256-bit numbering has no such row).  `native` tags are ignored: the
closed forms are 256-bit foreign-field routines, and the tag's contract is that the body computes the same values.
"""
from __future__ import annotations

import struct

import numpy as np

from .. import opcodes as O
from .writers import hashmap_size, build_hash_map, dat_io_map

GOLDILOCKS = 18446744069414584321
MAGIC = b"CW64"
VERSION = 1             # a circuit with neither CALL nor LOG: the tape it always had, byte for byte
VERSION_FN = 2          # function table, bytecode and log program in front of the rows; n_logv in the last header word
O_CALL = 27             # csrc/cw64.hip
F_JZ, F_JMP, F_LDX, F_STX, F_RET = 100, 101, 102, 103, 104      # csrc/cw_tape.h
FN_CONST = 0x80000000


class Tape64:
    def __init__(self):
        self.rows = None            # uint32 [n_rows, 8]
        self.consts = None          # uint64 [n_consts]
        self.n_signals = self.n_slots = 0
        self.n_logv = 0             # hidden slots n_signals .. n_signals + n_logv - 1: the arguments of the log statements
        self.functions = []         # (n_regs, uint32 [n_ins, 4]) per function
        self.log_prog, self.log_strings = [], []       # as Tape.log_prog / log_strings of the 256-bit lowering


def _encode_function64(fn, cid):
    """rtcode bytecode -> device form (module docstring); constants go through the tape's table"""
    from ..frontend import rtcode as R
    if fn["n_regs"] >= (1 << 16):
        raise ValueError("function %s needs too many registers" % fn["name"])
    consts = fn["consts"]

    def opnd(x):
        if x is None:
            return 0
        return x[1] if x[0] == 'r' else (FN_CONST | cid(consts[x[1]]))

    out = np.zeros((len(fn["code"]), 4), dtype=np.uint32)
    for i, (op, d, a, b) in enumerate(fn["code"]):
        if op == R.F_RET:
            out[i] = (F_RET, 0, 0, 0)
        elif op == R.F_JMP:
            out[i] = (F_JMP, d, 0, 0)
        elif op == R.F_JZ:
            out[i] = (F_JZ, d, opnd(a), 0)
        elif op == R.F_LDX:
            out[i] = (F_LDX, d, a, b[0] | (b[1] << 16))
        elif op == R.F_STX:
            out[i] = (F_STX, d, opnd(a), b[0] | (b[1] << 16))
        else:
            if not O.COPY <= op <= O.LNOT:
                raise ValueError("function %s: operator %d has no place in a function body" % (fn["name"], op))
            out[i] = (op, d, opnd(a), opnd(b))
    return fn["n_regs"], out


def lower64(fc) -> Tape64:
    if fc.fp.q != GOLDILOCKS:
        raise ValueError("the 64-bit runtime serves the Goldilocks prime only")
    ns = fc.n_signals
    code, n_logv = fc.code, 0
    log_prog, log_strings = [], []
    if (code["op"] == O.LOG).any():
        from ..frontend.flatten import log_program, code_with_log_copies
        log_prog, log_strings = log_program(fc), list(fc.log_strings)
        code, n_logv = code_with_log_copies(fc)
    op = code["op"]
    keep = op != O.RUN
    idx = np.nonzero(keep)[0]
    n = len(idx)
    rows = np.zeros((n, 8), dtype=np.uint32)
    t0 = ns + n_logv                # first temporary

    def operand(kk, vv):
        k = code[kk][idx]
        v = code[vv][idx].astype(np.int64)
        kind = np.where(k == O.K_SIG, 0, np.where(k == O.K_TMP, 0, np.where(k == O.K_CONST, 2, 3)))
        val = np.where(k == O.K_TMP, v + t0, np.where(k == O.K_NONE, 0, v))
        return kind.astype(np.uint32), val.astype(np.uint32)

    dk, dv = operand("dk", "dv")
    ak, av = operand("ak", "av")
    bk, bv = operand("bk", "bv")
    ck, cv = operand("ck", "cv")
    no_dst = np.isin(op[idx], list(O.NO_DST))
    dk = np.where(no_dst, 3, dk)
    assert not (dk == 2).any(), "a constant cannot be a destination"
    rows[:, 0] = op[idx].astype(np.uint32) | (dk << 8) | (ak << 10) | (bk << 12) | (ck << 14)
    rows[:, 1] = np.where(dk == 0, dv, 0)
    rows[:, 2], rows[:, 3], rows[:, 4] = av, bv, cv
    rows[:, 5] = idx.astype(np.uint32)
    consts = [int(c) % GOLDILOCKS for c in fc.constants]
    functions = []
    calls = op[idx] == O.CALL
    if calls.any():
        # a = the function id as it stands (operand kind none), b = register 0 of the window (a temporary: already a slot)
        assert (code["bk"][idx][calls] == O.K_TMP).all()
        rows[calls, 0] = O_CALL | (3 << 8) | (3 << 10) | (0 << 12) | (3 << 14)
        rows[calls, 2] = code["av"][idx][calls].astype(np.uint32)
        where = {}
        for i, c in enumerate(consts):
            where.setdefault(c, i)

        def cid(v):
            v = int(v) % GOLDILOCKS
            if v not in where:
                where[v] = len(consts)
                consts.append(v)
            return where[v]
        functions = [_encode_function64(f, cid) for f in fc.functions]
    t = Tape64()
    t.rows = rows
    t.consts = np.asarray(consts, dtype=np.uint64)
    t.n_signals = ns
    t.n_logv = n_logv
    t.n_slots = t0 + max(int(fc.n_temps), 0)
    t.functions = functions
    t.log_prog, t.log_strings = log_prog, log_strings
    return t


def write_tape64(path, fc, t: Tape64):
    """layout (loader: csrc/cw_host.cpp load_tape64, function section: csrc/cw_fn64.h)
        "CW64" | u32 version | u64 prime
        12 x u32: n_signals, n_witness, n_consts, input_start, n_inputs, n_input_names, hashmap_size, n_public_inputs, n_slots,
                  n_rows, io-map templates in the .dat, n_logv (version 1: 0)
        consts          n_consts x u64, canonical residues
        witness2signal  n_witness x u32
        input names     per name  u32 len | bytes | u32 start | u32 size
      version 2 only:
        functions       u32 n_functions | per function { u32 n_regs | u32 n_ins | n_ins x 4 x u32 }
        log program     u32 n_log_statements | per statement { u32 flat operation that ends it | u32 n_items |
                        n_items x { u32 0 | u32 len | bytes   (a string)   or   u32 1 | u32 j   (the j-th logged value) } }
      both:
        rows            n_rows x 8 x u32, to the end of the file
    Version 1 is what a circuit with neither run-time functions nor log statements gets: the file it always had."""
    v2 = bool(t.functions or t.log_prog or t.n_logv)
    with open(path, "wb") as f:
        f.write(MAGIC + struct.pack("<I", VERSION_FN if v2 else VERSION) + struct.pack("<Q", GOLDILOCKS))
        f.write(struct.pack("<12I", fc.n_signals, fc.n_signals, len(t.consts), fc.main_input_start, fc.n_main_inputs, len(fc.inputs),
                            hashmap_size(len(fc.inputs)), fc.n_pub_in, t.n_slots, len(t.rows), len(getattr(fc, "io_map", ())), t.n_logv))
        f.write(t.consts.astype("<u8").tobytes())
        f.write(np.arange(fc.n_signals, dtype="<u4").tobytes())
        for name, start, size in fc.inputs:
            b = name.encode()
            f.write(struct.pack("<I", len(b)) + b + struct.pack("<II", start, size))
        if v2:
            f.write(struct.pack("<I", len(t.functions)))
            for n_regs, fcode in t.functions:
                f.write(struct.pack("<2I", n_regs, len(fcode)) + np.ascontiguousarray(fcode, dtype="<u4").tobytes())
            f.write(struct.pack("<I", len(t.log_prog)))
            for at, items in t.log_prog:
                f.write(struct.pack("<2I", at, len(items)))
                for kind, v in items:
                    if kind == "s":
                        b = t.log_strings[v].encode()
                        f.write(struct.pack("<2I", 0, len(b)) + b)
                    else:
                        f.write(struct.pack("<2I", 1, v))
        f.write(np.ascontiguousarray(t.rows, dtype="<u4").tobytes())


def write_dat64(path, fc):
    """`.dat` as common64/main.cpp reads it (hash map, witness list, io map - no constant table: the reference inlines constants
    as literals for this prime, value_bucket.rs:82-86)"""
    size = hashmap_size(len(fc.inputs))
    with open(path, "wb") as f:
        f.write(b"".join(struct.pack("<QQQ", *e) for e in build_hash_map(fc.inputs, size)))
        f.write(np.arange(fc.n_signals, dtype="<u8").tobytes())
        f.write(dat_io_map(getattr(fc, "io_map", ())))
    return size
