"""Run-time functions and log() in the 64-bit runtime (`--prime goldilocks`): lowering, tape format and loader, on the CPU.

hip_elements/lower64.py writes a CALL as one row (O_CALL = 27: function id, first slot of the register window) and a logged
value as a COPY into a hidden slot behind the circuit's signals; a tape that has either is version 2 and carries the function
table, the bytecode and the log program in front of its rows.  csrc/cw_fn64.h + load_tape64 check every number the device
interpreter will trust.

References.  log(): tests/golden/reference_logs_goldilocks.json is the stdout, exit status and .wtns digest of the reference's own
64-bit runtime (tests/golden/make_golden_goldilocks_logs.py).  Functions: the committed oracle recipe has no 64-bit mode for
run-time functions, so the yardstick is oracle/tape_eval.py eval_flat - its 64-bit operators are pinned by the operator-zoo
goldens (tests/test_goldilocks_oracle.py), its function interpreter by the reference runtime on the 256-bit primes
(tests/test_functions.py) - with plain-integer models beside it (a // b, a % b; _pick_model).  `eval_tape64` below executes the
tape AS WRITTEN (rows, merged constants, encoded bytecode) on Python integers: what the device has to compute, without one."""
import hashlib
import json
import os
import random
import struct

import numpy as np
import pytest

from circom_amd import opcodes as O
from circom_amd.circuits.basic import LogDemo, Multiplier2
from circom_amd.compiler import compile_program
from circom_amd.frontend.dsl import Program, template
from circom_amd.frontend.flatten import flatten
from circom_amd.hip_elements import lower64 as L64
from circom_amd.hip_elements.writers import wtns_bytes
from oracle.field import Field, FieldError
from oracle.tape_eval import eval_flat, check_r1cs, _BIN, _UN
from test_functions import LongDiv, Pick, _pick_model

Q = 18446744069414584321
GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "reference_logs_goldilocks.json")))["cases"]["logdemo"]["vectors"]
BIG_N = 200


def build_big(f, n, sel):
    """a 200-entry local array filled by a loop whose trip count the trace cannot see, read at sel and sel + 1: more registers
    than the LDS placement takes (207 > 128), and sel = 199 reads one past the end"""
    arr = f.array(BIG_N)
    i = f.var(0)
    with f.loop() as L:
        L.break_unless(i.lt(BIG_N))
        arr.store(i, i * n + 1)
        i.set(i + 1)
    return [arr.load(sel) + arr.load(sel + 1)]


@template
def Big(c):
    n = c.input("n")
    sel = c.input("sel")
    out = c.output("out", 2)
    fn = c.function("fill", 2, build_big)
    (v,) = c.call(fn, [n, sel])
    (w,) = c.call(fn, [n + 1, sel])              # a second call: another window
    c.hint(out[0], v)
    c.hint(out[1], w)


def _big_model(n, sel):
    return ((sel * n + 1) + ((sel + 1) * n + 1)) % Q


ZOO_OUTS = 31


def build_zoo(f, a, b):
    """every binary and unary operator of the language inside a function body, constants on either side"""
    E = lambda op, x, y=None: f.emit(op, f.lift(x), None if y is None else f.lift(y))
    return [a + b, a - b, a * b, a / b, a // b, a % b, E(O.POW, a, b & 255), a << b, a >> b, a & b, a | b, a ^ b,
            a.lt(b), a.gt(b), a.leq(b), a.geq(b), a.eq(b), a.neq(b), a.land(b), a.lor(b), -a, E(O.BNOT, a), a.lnot(),
            a + 7, 5 - b, 3 * a, E(O.IDIV, 1000, b), a % 1000, E(O.POW, 3, b & 63), E(O.SHL, 1, b & 63), E(O.DIV, Q - 1, a)]


@template
def FnZoo(c):
    a = c.input("a")
    b = c.input("b")
    out = c.output("out", ZOO_OUTS)
    fn = c.function("zoo", 2, build_zoo)
    vs = c.call(fn, [a, b])
    assert len(vs) == ZOO_OUTS
    for k, v in enumerate(vs):
        c.hint(out[k], v)


def goldilocks(tmpl):
    return Program(tmpl(), prime="goldilocks")


def flat_oracle(fc, row, log=None):
    inp = {fc.main_input_start + k: int(v) for k, v in enumerate(row)}
    return eval_flat(Q, fc.n_signals, fc.n_temps, fc.constants, fc.code, inp, fc.functions, log, fc.log_strings)


def eval_tape64(t, fc, row):
    """the version-2 tape on Python integers: (table slots, status word as the kernel forms it)"""
    f = Field(Q)
    ops = {k: getattr(f, v) for k, v in list(_BIN.items()) + list(_UN.items())}
    consts = [int(c) for c in t.consts]

    def alu(op, a, b):
        try:
            return (a if op == O.COPY else ops[op](a) if op in _UN else ops[op](a, b)), False
        except FieldError:
            return 0, True

    V = [0] * t.n_slots
    V[0] = 1
    for k, v in enumerate(row):
        V[fc.main_input_start + k] = int(v) % Q
    st = 0
    for w in t.rows.tolist():
        op, kinds = w[0] & 0xFF, [(w[0] >> s) & 3 for s in (8, 10, 12, 14)]
        if op == L64.O_CALL:
            n_regs, code = t.functions[w[2]]
            base, pc, bad, steps = w[3], 0, False, 0
            assert base >= t.n_signals + t.n_logv and base + n_regs <= t.n_slots
            val = lambda x: consts[x & 0x7FFFFFFF] if x & L64.FN_CONST else V[base + x]
            while True:
                fop, d, a, b = code[pc].tolist()
                pc += 1
                steps += 1
                assert steps < 1 << 20
                if fop == L64.F_RET:
                    break
                elif fop == L64.F_JMP:
                    pc = d
                elif fop == L64.F_JZ:
                    pc = d if val(a) == 0 else pc
                elif fop in (L64.F_LDX, L64.F_STX):
                    idx, ln = V[base + (b & 0xFFFF)], b >> 16
                    if idx >= ln:
                        bad, idx = True, 0
                    if fop == L64.F_LDX:
                        V[base + d] = V[base + a + idx]
                    else:
                        V[base + d + idx] = val(a)
                else:
                    V[base + d], fl = alu(fop, val(a), val(b))
                    bad = bad or fl
            if bad and not st & 3:
                st = 2 | (w[5] << 8)
            continue
        a, b, c = [V[v] if k == 0 else consts[v] if k == 2 else 0 for k, v in zip(kinds[1:], w[2:5])]
        fail = False
        if op == O.SELECT:
            d = b if a else c
        elif op == O.ASSERT_EQ:
            fail = a != b
        elif op == O.ASSERT_NZ:
            fail = a == 0
        else:
            d, fail = alu(op, a, b)
        if fail and not st & 3:
            st = (2 if op in (O.IDIV, O.MOD) else 1) | (w[5] << 8)
        if kinds[0] == 0 and op not in (O.ASSERT_EQ, O.ASSERT_NZ):
            V[w[1]] = d
    return V, st


def test_oracle_reproduces_the_64_bit_runtimes_log_output():
    fc = flatten(goldilocks(LogDemo))
    assert {(int(v["inputs"]["a"]), int(v["inputs"]["b"])) for v in GOLD} >= {(5, 6), (13, 2), (Q - 1, 7), (0, 0), (Q - 2, Q - 3)}
    for v in GOLD:
        lines = []
        sig, failed = flat_oracle(fc, (v["inputs"]["a"], v["inputs"]["b"]), lines)
        assert "".join(lines) == v["log"]
        assert (failed is None) == v["ok"]
        if v["ok"]:
            assert hashlib.sha256(wtns_bytes(Q, sig)).hexdigest() == v["wtns_sha256"]
        else:
            assert failed == 16


def test_a_circuit_without_calls_and_logs_keeps_its_version_1_tape(tmp_path):
    cp = compile_program(goldilocks(Multiplier2), str(tmp_path), "m2", sym=False)
    fc, t = cp.flat, cp.tape
    raw = open(cp.tape_path, "rb").read()
    assert raw[:8] == b"CW64" + struct.pack("<I", 1) and struct.unpack_from("<12I", raw, 16)[11] == 0
    names = sum(4 + len(n.encode()) + 8 for n, _, _ in fc.inputs)
    assert len(raw) == 16 + 48 + 8 * len(fc.constants) + 4 * fc.n_signals + names + 32 * len(t.rows)
    assert not t.functions and not t.log_prog and t.n_logv == 0


@pytest.mark.parametrize("tmpl", [LongDiv, Pick, LogDemo, Big, FnZoo])
def test_the_tape_as_written_computes_what_the_oracle_computes(tmpl):
    fc = flatten(goldilocks(tmpl))
    t = L64.lower64(fc)
    rnd = random.Random(11)
    rows = {LongDiv: lambda: [rnd.randrange(1 << rnd.randrange(1, 63)), rnd.randrange(1, 1 << rnd.randrange(1, 32))],
            Pick: lambda: [rnd.randrange(Q) for _ in range(8)] + [rnd.randrange(9)],
            LogDemo: lambda: [rnd.choice((13, rnd.randrange(Q))), rnd.randrange(Q)],
            Big: lambda: [rnd.randrange(Q), rnd.choice((199, rnd.randrange(BIG_N)))],
            FnZoo: lambda: [rnd.choice((0, 1, Q - 1, rnd.randrange(Q))), rnd.choice((0, 1, 63, 64, Q - 1, rnd.randrange(Q)))]}[tmpl]
    for _ in range(12):
        row = rows()
        sig, failed = flat_oracle(fc, row)
        V, st = eval_tape64(t, fc, row)
        assert V[:fc.n_signals] == sig, row
        assert (st & 3 == 0) == (failed is None) and (failed is None or st >> 8 == failed), (row, st, failed)
        if tmpl is LongDiv:
            assert sig[1:3] == [row[0] // row[1], row[0] % row[1]] and check_r1cs(Q, fc.constraints, sig) is None
        if tmpl is Pick and row[8] < 8:
            assert sig[1] == _pick_model(Q, row[:8], row[8])
        if tmpl is Big and row[1] < BIG_N - 1:
            assert sig[1:3] == [_big_model(row[0], row[1]), _big_model((row[0] + 1) % Q, row[1])]
        if tmpl is Big and row[1] == BIG_N - 1:
            assert failed == 2
        if tmpl is LogDemo:
            want = []
            flat_oracle(fc, row, want)
            vals = [int(x) for line in want for x in line.split() if x.isdigit()]
            if failed is None:                      # (every logged value; "100%" is no number)
                assert V[fc.n_signals:fc.n_signals + t.n_logv] == vals


def test_version_2_tapes_load_through_the_c_abi(tmp_path):
    from circom_amd import runtime as rt
    for tmpl, n_fn, n_log in ((LongDiv, 1, 0), (Pick, 1, 0), (LogDemo, 0, 7), (Big, 1, 0)):
        cp = compile_program(goldilocks(tmpl), str(tmp_path), tmpl.__name__.lower(), sym=False)
        fc, t = cp.flat, cp.tape
        raw = open(cp.tape_path, "rb").read()
        assert raw[:8] == b"CW64" + struct.pack("<I", 2) and struct.unpack_from("<12I", raw, 16)[11] == t.n_logv
        assert len(t.functions) == n_fn and len(t.log_prog) == n_log and t.n_logv == (8 if tmpl is LogDemo else 0)
        assert t.n_slots == fc.n_signals + t.n_logv + fc.n_temps
        if tmpl is Big:
            assert t.functions[0][0] > 128          # the placement test needs a function the LDS cannot hold
        c = rt.Circuit(cp.tape_path, cp.dat_path, cp.r1cs_path)
        assert (c.q, c.n_signals, c.n_witness) == (Q, fc.n_signals, fc.n_signals)        # hidden slots are no signals
        assert rt.lib().cw_n_log_statements(c.h) == n_log
        assert c.n_rows == len(t.rows) and c.n_constraints == len(fc.constraints)
        b = c.batch(3, device=-1)                                       # host-only: nothing computes
        assert b.call_lds == 0
        with pytest.raises(rt.CwError):
            b.run()
        b.close(); c.close()


def _refused(rt, tmp_path, cp, raw):
    (tmp_path / "bad.cwt").write_bytes(bytes(raw))
    with pytest.raises(rt.CwError) as e:
        rt.Circuit(tmp_path / "bad.cwt", cp.dat_path, cp.r1cs_path)
    assert e.value.code == -1, e.value                                  # CW_EIO


def test_loader_refuses_damaged_function_sections_and_call_rows(tmp_path):
    from circom_amd import runtime as rt
    cp = compile_program(goldilocks(Pick), str(tmp_path), "pick", sym=False)
    fc, t = cp.flat, cp.tape
    rt.Circuit(cp.tape_path, cp.dat_path, cp.r1cs_path).close()
    tape = bytearray(open(cp.tape_path, "rb").read())
    n_regs, code = t.functions[0]
    blob = code.astype("<u4").tobytes()
    at = bytes(tape).index(blob)
    assert struct.unpack_from("<3I", tape, at - 12) == (1, n_regs, len(code))
    op = code[:, 0]
    alu = int(np.nonzero(op <= O.LNOT)[0][0])
    konst = [(i, c) for i in range(len(code)) for c in (2, 3) if op[i] <= O.LNOT and code[i, c] & L64.FN_CONST][0]
    jmp = int(np.nonzero(op == L64.F_JMP)[0][0])
    jz = int(np.nonzero(op == L64.F_JZ)[0][0])
    ldx = int(np.nonzero(op == L64.F_LDX)[0][0])
    stx = int(np.nonzero(op == L64.F_STX)[0][0])
    assert op[-1] == L64.F_RET
    for i, col, val in ((0, 0, 77),                                                 # unknown opcode
                        (alu, 1, n_regs),                                           # destination register beyond the window
                        (konst[0], konst[1], L64.FN_CONST | len(t.consts)),         # constant index beyond the table
                        (jmp, 1, len(code)),                                        # jump past the end
                        (jz, 1, len(code)),
                        (ldx, 3, (code[ldx, 3] & 0xFFFF) | ((n_regs - code[ldx, 2] + 1) << 16)),      # array leaves the window
                        (stx, 3, (code[stx, 3] & 0xFFFF) | ((n_regs - code[stx, 1] + 1) << 16)),
                        (ldx, 3, n_regs | (code[ldx, 3] & 0xFFFF0000)),            # index register beyond the window
                        (len(code) - 1, 0, O.COPY)):                                # the code can run off its end
        bad = code.copy()
        bad[i, col] = val
        t2 = bytearray(tape)
        t2[at:at + len(blob)] = bad.astype("<u4").tobytes()
        _refused(rt, tmp_path, cp, t2)
    t2 = bytearray(tape)
    struct.pack_into("<I", t2, at - 8, 1 << 16)                                     # n_regs >= 2^16
    _refused(rt, tmp_path, cp, t2)
    # the CALL row: function id, window below the temporaries, window past the table
    r = int(np.nonzero((t.rows[:, 0] & 0xFF) == L64.O_CALL)[0][0])
    row_at = len(tape) - (len(t.rows) - r) * 32
    assert struct.unpack_from("<8I", tape, row_at) == tuple(int(x) for x in t.rows[r])
    for word, val in ((2, 1), (3, fc.n_signals - 1), (3, t.n_slots - n_regs + 1)):
        t2 = bytearray(tape)
        struct.pack_into("<I", t2, row_at + 4 * word, val)
        _refused(rt, tmp_path, cp, t2)
    t2 = bytearray(tape)
    struct.pack_into("<I", t2, row_at, 28)                                          # no such row operator
    _refused(rt, tmp_path, cp, t2)
    for cut in (at + 5, at + len(blob) - 1, at - 9):                                # truncated inside the section
        _refused(rt, tmp_path, cp, tape[:cut] + tape[at + len(blob):])
    # a version-1 tape keeps its rule: no row operator above 26, no n_logv
    cp1 = compile_program(goldilocks(Multiplier2), str(tmp_path), "m2", sym=False)
    t1 = bytearray(open(cp1.tape_path, "rb").read())
    for off, val in ((len(t1) - 32, 27 | (3 << 8) | (3 << 10) | (3 << 14)), (16 + 44, 1)):
        t2 = bytearray(t1)
        struct.pack_into("<I", t2, off, val)
        _refused(rt, tmp_path, cp1, t2)
    # hidden slots: the log program has to name exactly n_logv values
    cpl = compile_program(goldilocks(LogDemo), str(tmp_path), "logdemo", sym=False)
    tl = bytearray(open(cpl.tape_path, "rb").read())
    struct.pack_into("<I", tl, 16 + 44, 7)
    _refused(rt, tmp_path, cpl, tl)
