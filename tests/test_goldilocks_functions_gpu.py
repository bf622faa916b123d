"""Run-time functions and log() in the 64-bit runtime ON THE DEVICE (`--prime goldilocks`, csrc/cw64.hip cw64_call).

References (tests/test_goldilocks_functions.py has the CPU side and says why): log() against the stdout of the reference's own
64-bit runtime (tests/golden/reference_logs_goldilocks.json); functions against oracle/tape_eval.py eval_flat - the committed oracle
recipe cannot run functions for this prime - whose 64-bit operators are pinned by the operator-zoo goldens and whose function
interpreter is pinned by the reference runtime on the 256-bit primes, with plain-integer models beside it (a // b, a % b,
_pick_model, math.gcd).

Shapes: one lane short of a wave, a wave, one lane more, several workgroups; both placements of the register window (LDS /
value table, CW64_CALL_LDS read when the batch is created).  The step limit (2^24 instructions per lane) is deliberately not
reached here - LongDiv never gets b = 0: that is a long run, not a test of seconds; the oracle and the loader tests cover the
rule."""
import functools
import hashlib
import io
import json
import math
import os
import random

import numpy as np
import pytest

from circom_amd.circuits.basic import LogDemo
from circom_amd.compiler import compile_program
from oracle.tape_eval import check_r1cs
from test_functions import LongDiv, Pick, _pick_model
from test_goldilocks_functions import Big, BIG_N, FnZoo, GOLD, Q, flat_oracle, goldilocks, _big_model

pytestmark = pytest.mark.gpu
PLACEMENTS = [pytest.param("0", id="table"), pytest.param("1", id="lds")]


def _open(tmp_path, tmpl, name):
    from circom_amd import runtime as rt
    cp = compile_program(goldilocks(tmpl), str(tmp_path), name, sym=False)
    return cp, rt.Circuit(cp.tape_path, cp.dat_path, cp.r1cs_path)


def _witnesses(b):
    """the whole batch as Python integers [instance][witness entry] (one bulk egress; the upper 24 bytes are zero)"""
    w = b.witnesses()
    assert not w[:, :, 8:].any()
    return np.ascontiguousarray(w[:, :, :8]).view("<u8")[:, :, 0].tolist()


@functools.lru_cache(maxsize=None)
def _longdiv_cases():
    from circom_amd.frontend.flatten import flatten
    fc = flatten(goldilocks(LongDiv))
    rnd = random.Random(41)
    # 1 .. 62 trips of either loop per lane; a < 2^62: the relational operators are signed around q / 2
    rows = [[rnd.randrange(1 << rnd.randrange(1, 63)), rnd.randrange(1, 1 << rnd.randrange(1, 32))] for _ in range(300)]
    want = []
    for a, b in rows:
        sig, failed = flat_oracle(fc, (a, b))
        assert failed is None and sig[1:3] == [a // b, a % b] and check_r1cs(Q, fc.constraints, sig) is None
        want.append(sig)
    return rows, want


@pytest.mark.parametrize("placement", PLACEMENTS)
def test_gpu_long_division_in_divergent_lanes(tmp_path, monkeypatch, placement):
    monkeypatch.setenv("CW64_CALL_LDS", placement)
    rows, want = _longdiv_cases()
    cp, c = _open(tmp_path, LongDiv, "longdiv")
    n_regs = cp.tape.functions[0][0]
    for B in (1, 63, 64, 65, 300):
        b = c.batch(B)
        assert b.call_lds == (n_regs * 512 if placement == "1" else 0)
        b.set_inputs(rows[:B])
        b.run(); b.check_r1cs(); b.sync()
        assert (b.status() == 0).all(), (B, b.status())
        got = _witnesses(b)
        assert got == want[:B], B
        assert [g[1:3] for g in got] == [[a // d, a % d] for a, d in rows[:B]]
        b.close()
    c.close()


def test_gpu_run_time_indices_and_both_placements_leave_the_same_table(tmp_path, monkeypatch):
    from test_bitplane import _Hip
    from circom_amd import runtime as rt
    hip = _Hip()
    cp, c = _open(tmp_path, Pick, "pick")
    fc = cp.flat
    rnd = random.Random(42)
    B = 300
    rows = [[rnd.randrange(Q) for _ in range(8)] + [rnd.randrange(9)] for _ in range(B)]
    oracle = [flat_oracle(fc, r) for r in rows]
    assert any(f is not None for _, f in oracle)
    tables = []
    for placement in ("0", "1"):
        monkeypatch.setenv("CW64_CALL_LDS", placement)
        b = c.batch(B)
        assert (b.call_lds != 0) == (placement == "1")
        b.set_inputs(rows)
        b.run(); b.sync()
        st, got = b.status(), _witnesses(b)
        for i, r in enumerate(rows):
            sig, failed = oracle[i]
            if r[8] == 8:                                   # outside the array: flagged with the oracle's flat operation
                assert failed is not None and st[i] == (rt.ST_ARITH | (failed << 8)), (i, st[i])
            else:
                assert failed is None and st[i] == 0 and got[i][1] == _pick_model(Q, r[:8], r[8]), i
            assert got[i] == sig, i                         # a failed lane carries on as the oracle does; its neighbours are untouched
        ptr, n_bytes, bp = b.device_values()
        assert ptr and n_bytes == cp.tape.n_slots * bp * 8
        tables.append(hip.download(ptr, (n_bytes,)))
        b.close()
    assert (tables[0] == tables[1]).all()
    c.close()


def test_gpu_a_function_too_large_for_lds_runs_on_the_table(tmp_path, monkeypatch):
    from circom_amd import runtime as rt
    monkeypatch.setenv("CW64_CALL_LDS", "1")                 # ignored above the limit
    cp, c = _open(tmp_path, Big, "big")
    fc = cp.flat
    assert cp.tape.functions[0][0] > 128
    rnd = random.Random(43)
    B = 130
    rows = [[rnd.randrange(Q), rnd.randrange(BIG_N)] for _ in range(B)]
    rows[5][1] = rows[64][1] = rows[129][1] = BIG_N - 1      # reads element 200 of 200
    rows[6][1], rows[65][1] = 0, BIG_N - 2
    b = c.batch(B)
    assert b.call_lds == 0
    b.set_inputs(rows)
    b.run(); b.sync()
    st, got = b.status(), _witnesses(b)
    for i, (n, sel) in enumerate(rows):
        sig, failed = flat_oracle(fc, (n, sel))
        assert got[i] == sig, i
        if sel == BIG_N - 1:
            assert failed == 2 and st[i] == (rt.ST_ARITH | (2 << 8)), (i, st[i])
        else:
            assert failed is None and st[i] == 0 and got[i][1:3] == [_big_model(n, sel), _big_model((n + 1) % Q, sel)], i
    b.close(); c.close()


@pytest.mark.parametrize("placement", PLACEMENTS)
def test_gpu_every_operator_inside_a_function(tmp_path, monkeypatch, placement):
    from test_opzoo import _operands
    from circom_amd import runtime as rt
    monkeypatch.setenv("CW64_CALL_LDS", placement)
    cp, c = _open(tmp_path, FnZoo, "fnzoo")
    fc = cp.flat
    rows = _operands(Q, 200, 44)
    assert len(rows) >= 31 * 31 + 200
    b = c.batch(len(rows))
    b.set_inputs(rows)
    b.run(); b.sync()
    st, got = b.status(), _witnesses(b)
    flagged = 0
    for i, r in enumerate(rows):
        sig, failed = flat_oracle(fc, r)
        assert got[i] == sig, (i, r)                         # a lane with a division by zero still has every other value
        assert st[i] == (0 if failed is None else rt.ST_ARITH | (failed << 8)), (i, r, st[i])
        assert (failed is not None) == (r[1] == 0)           # a // b, a % b, 1000 // b
        flagged += failed is not None
    assert flagged >= 31
    b.close(); c.close()


def test_gpu_log_of_every_instance(tmp_path):
    from test_bitplane import _Hip
    hip = _Hip()
    cp, c = _open(tmp_path, LogDemo, "logdemo")
    fc = cp.flat
    rows = list(GOLD) * 30
    B = len(rows)
    b = c.batch(B)
    b.set_inputs([[int(v["inputs"]["a"]), int(v["inputs"]["b"])] for v in rows])
    b.run(); b.check_r1cs(); b.sync()
    st = b.status()
    for i, v in enumerate(rows):
        assert (st[i] == 0) == v["ok"], i
        assert b.log(i) == v["log"], i
    b.write_wtns_many(0, B, str(tmp_path / "w%u.wtns"))               # every passing instance, in every wave
    for i, v in enumerate(rows):
        if v["ok"]:
            assert hashlib.sha256((tmp_path / ("w%d.wtns" % i)).read_bytes()).hexdigest() == v["wtns_sha256"], i
    # the hidden slots are no witness entries: the 8-byte bulk form is [B][n_signals] and holds the signals alone
    assert c.n_witness == fc.n_signals and cp.tape.n_logv == 8
    d_out = hip.alloc(B * c.n_witness * 8)
    b.witnesses_device_n8(0, B, d_out)
    b.sync()
    img = hip.download(d_out, (B, c.n_witness), np.uint64)
    for i in (0, 2, 4, B - 1):
        assert rows[i]["ok"] and img[i].tolist() == flat_oracle(fc, (rows[i]["inputs"]["a"], rows[i]["inputs"]["b"]))[0], i
    hip.h.hipFree(d_out)
    b.close(); c.close()


def test_gpu_run_check_replays_the_call_kernel(tmp_path, monkeypatch):
    """cw_run_check on a circuit with a call: plain, captured, replayed - fresh inputs every time.  No placement is forced: ten
    registers take the LDS placement by themselves."""
    from test_bitplane import _Hip
    hip = _Hip()
    monkeypatch.delenv("CW64_CALL_LDS", raising=False)
    cp, c = _open(tmp_path, LongDiv, "longdiv")
    rows, want = _longdiv_cases()
    B = 64
    b = c.batch(B)
    assert b.call_lds == cp.tape.functions[0][0] * 512
    d_in = hip.alloc(B * 2 * 32)
    b.set_inputs_device(d_in)
    for r in range(3):
        part = rows[r * B:(r + 1) * B]
        img = np.frombuffer(b"".join(int(v).to_bytes(32, "little") for row in part for v in row), dtype=np.uint8).copy()
        assert hip.h.hipMemcpy(d_in, img.ctypes.data, img.nbytes, 1) == 0
        b.run_check(); b.sync()
        assert b.graph_captured == (r >= 1), r
        assert (b.status() == 0).all(), (r, b.status())
        assert _witnesses(b) == want[r * B:(r + 1) * B], r
    b.close(); c.close()
    hip.h.hipFree(d_in)


def test_gpu_a_circom_text_with_a_run_time_function(tmp_path):
    from circom_amd import circom, runtime as rt
    from circom_amd import opcodes as O
    src = os.path.join(os.path.dirname(__file__), "circom", "gcd_goldilocks.circom")
    fc, _ = circom.compile_file(src, str(tmp_path), prime="goldilocks", hip=True, out=io.StringIO())
    cp = fc.compiled
    assert len(cp.tape.functions) == 1
    c = rt.Circuit(cp.tape_path, cp.dat_path, cp.r1cs_path)
    rnd = random.Random(45)
    rows = [[rnd.randrange(1, 1 << rnd.randrange(1, 62)) * g, rnd.randrange(1 << rnd.randrange(1, 62)) * g]
            for g in (rnd.randrange(1, 1 << 10) for _ in range(100))]
    rows = [[a % (1 << 62), b % (1 << 62)] for a, b in rows]
    rows[0], rows[1], rows[2], rows[3] = [0, 0], [0, 5], [17, 0], [12, 18]
    b = c.batch(len(rows))
    b.set_inputs(rows)
    b.run(); b.check_r1cs(); b.sync()
    st, got = b.status(), _witnesses(b)
    idiv = int(np.nonzero(fc.code["op"] == O.IDIV)[0][0])
    for i, (x, y) in enumerate(rows):
        sig, failed = flat_oracle(fc, (x, y))
        assert got[i] == sig, i
        if (x, y) == (0, 0):
            assert failed == idiv and st[i] == (rt.ST_ARITH | (idiv << 8)), st[i]      # k <-- 0 \ 0
        else:
            assert failed is None and st[i] == 0 and got[i][1] == math.gcd(x, y), (i, st[i])
    b.close(); c.close()
