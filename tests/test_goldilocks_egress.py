"""Bulk egress of the 64-bit runtime (`--prime goldilocks`): cw_get_witnesses_device / _n8 (csrc/cw64.hip cw64_egress_kernel, a
tiled transpose through LDS), cw_stream_witnesses_device, cw_write_wtns_many, cw_write_wtnsb and cw_explain.

Expected values come from the reference's own 64-bit runtime (tests/golden/reference_wtns_goldilocks.json) or from the oracle
(oracle.tape_eval.eval_flat), never from another call into the library.  The shapes are the ones the kernel can go wrong at:
`first` / `count` that are no multiple of 64, a witness list that is not the identity with an odd and an even length (a row of
the 8-byte image then starts on an 8-byte boundary only), a witness narrower than a tile, more instance tiles than one wave
or workgroup sees, guard bytes on both sides of every image."""
import functools
import hashlib
import json
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
from make_golden import goldilocks_cases                                            # noqa: E402

from circom_amd import wtnsb                                                         # noqa: E402
from circom_amd.compiler import compile_program                                      # noqa: E402
from circom_amd.frontend.dsl import Program, template                                # noqa: E402
from oracle.tape_eval import eval_flat                                               # noqa: E402

GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "reference_wtns_goldilocks.json")))["cases"]
CASES = goldilocks_cases()
Q = 18446744069414584321
CW_EDEVICE, CW_ESTATE = -4, -5
GUARD = 4096


@template
def BadSquare(cx):
    a = cx.input("a")
    out = cx.output("out")
    cx.hint(out, a * a + (a & 1))                                 # wrong for odd a
    cx.enforce(out, a * a, runtime_check=False)


def _badsquare(tmp_path, sym=False):
    return compile_program(Program(BadSquare(), prime="goldilocks"), str(tmp_path), "badsq", sym=sym)


def test_element_size_and_error_codes_without_a_gpu(tmp_path):
    from circom_amd import runtime as rt
    from circom_amd.circuits.basic import Multiplier2
    L = rt.lib()
    assert hasattr(L, "cw_element_bytes") and hasattr(L, "cw_get_witnesses_device_n8")
    cp32 = compile_program(Program(Multiplier2()), str(tmp_path), "m2", sym=False)
    c32 = rt.Circuit(cp32.tape_path, cp32.dat_path, cp32.r1cs_path)
    assert c32.element_bytes == 32
    c32.close()
    mk, _ = CASES["multiplier2"]
    cp = compile_program(mk(), str(tmp_path), "m2g", sym=False)
    c = rt.Circuit(cp.tape_path, cp.dat_path, cp.r1cs_path)
    assert c.element_bytes == 8 and c.q == Q
    b = c.batch(3, device=-1)
    calls = {
        "witnesses_device": lambda: b.witnesses_device(0, 3, 4096),                 # the pointer is never touched: no device
        "witnesses_device_n8": lambda: b.witnesses_device_n8(0, 3, 4096),
        "write_wtns_many": lambda: b.write_wtns_many(0, 3, str(tmp_path / "w%u.wtns")),
        "write_wtnsb": lambda: b.write_wtnsb(tmp_path / "w.wtnsb"),
        "explain": lambda: b.explain(0),
    }
    for name, call in calls.items():
        with pytest.raises(rt.CwError) as e:
            call()
        assert e.value.code == CW_EDEVICE and "not available" not in str(e.value), (name, str(e.value))
    with pytest.raises(rt.CwError) as e:
        b.set_inputs_bits(np.zeros((1, c.n_inputs), dtype=np.uint64))
    assert e.value.code == CW_ESTATE
    b.close(); c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(GOLD))
def test_gpu_goldens_through_the_bulk_file_paths(name, tmp_path):
    from circom_amd import runtime as rt
    mk, _ = CASES[name]
    vecs = GOLD[name]["vectors"]
    cp = compile_program(mk(), str(tmp_path), name, sym=False)
    c = rt.Circuit(cp.tape_path, cp.dat_path, cp.r1cs_path)
    b = c.batch(len(vecs))
    b.set_inputs([[int(v) for v in vec["inputs"]] for vec in vecs])
    b.run(); b.sync()
    assert (b.status() == 0).all(), b.status()
    b.write_wtns_many(0, len(vecs), str(tmp_path / "many%u.wtns"))
    b.write_wtnsb(tmp_path / "all.wtnsb")
    wb = wtnsb.load(tmp_path / "all.wtnsb")
    assert (wb.kind, wb.n8, wb.prime, wb.batch, wb.n_witness) == (0, 8, Q, len(vecs), c.n_witness)
    for i, vec in enumerate(vecs):
        got = (tmp_path / ("many%d.wtns" % i)).read_bytes()
        assert len(got) == vec["wtns_len"] and hashlib.sha256(got).hexdigest() == vec["wtns_sha256"], (name, i)
        assert hashlib.sha256(wb.expand(i)).hexdigest() == vec["wtns_sha256"], (name, i)
    b.close(); c.close()


# ---- Poseidon(2) x 300 against the oracle ------------------------------------------------------------------------------------
B300 = 300


@functools.lru_cache(maxsize=None)
def _poseidon_oracle():
    """(input rows, per instance the oracle's signals): computed once, shared, never modified"""
    from circom_amd.frontend.flatten import flatten
    fc = flatten(CASES["poseidon2"][0]())
    rnd = random.Random(64300)
    rows = tuple(tuple(rnd.randrange(Q) for _ in range(fc.n_main_inputs)) for _ in range(B300))
    sigs = []
    for row in rows:
        sig, failed = eval_flat(Q, fc.n_signals, fc.n_temps, fc.constants, fc.code, {fc.main_input_start + k: v for k, v in enumerate(row)})
        assert failed is None
        sigs.append(sig)
    out = np.array(sigs, dtype=np.uint64)                         # [instance][signal]
    out.setflags(write=False)
    return rows, out


def _poseidon_batch(tmp_path, drop):
    """Poseidon(2) with the witness list 'all signals but the last `drop`', a batch of 300 evaluated and clean"""
    from circom_amd import runtime as rt
    rows, sig = _poseidon_oracle()
    cp = compile_program(CASES["poseidon2"][0](), str(tmp_path), "poseidon2", sym=False)
    c = rt.Circuit(cp.tape_path, cp.dat_path, cp.r1cs_path)
    keep = np.arange(c.n_signals - drop, dtype=np.uint32)
    assert 1 + c.n_public < len(keep) < c.n_witness               # only non-public entries leave the list
    c.set_witness_list(keep)
    assert c.n_witness == len(keep)
    b = c.batch(B300)
    b.set_inputs([list(r) for r in rows])
    b.run(); b.sync()
    assert (b.status() == 0).all()                                # precondition: ALL 300 instances are compared below
    return c, b, sig[:, :len(keep)]


def _guarded(hip, nbytes):
    total = GUARD + nbytes + GUARD
    return hip.upload(np.full(total, 0xA5, dtype=np.uint8)), total


def _check_image(hip, p, total, want64, eb):
    """the bytes between the guards are `want64` ([count][n_wit] uint64) as eb-byte little-endian elements; the guards are intact"""
    raw = hip.download(p, (total,))
    assert (raw[:GUARD] == 0xA5).all() and (raw[-GUARD:] == 0xA5).all(), "guard bytes were written"
    got = raw[GUARD:-GUARD].view("<u8").reshape(want64.shape[0], want64.shape[1], eb // 8)
    assert (got[:, :, 0] == want64).all()
    assert not got[:, :, 1:].any()


@pytest.mark.gpu
@pytest.mark.parametrize("drop", [1, 2])                        # all signals but the last one / the last two: both parities of n_witness
def test_gpu_device_forms_against_the_oracle(drop, tmp_path):
    from test_bitplane import _Hip
    hip = _Hip()
    c, b, want = _poseidon_batch(tmp_path, drop)
    for first, count in ((0, 300), (37, 201), (64, 64), (299, 1)):
        for eb, call in ((32, b.witnesses_device), (8, b.witnesses_device_n8)):
            p, total = _guarded(hip, count * c.n_witness * eb)
            call(first, count, p + GUARD)
            b.sync()
            _check_image(hip, p, total, want[first:first + count], eb)
            hip.h.hipFree(p)
    b.close(); c.close()


@pytest.mark.gpu
def test_gpu_chunked_egress(tmp_path):
    from test_bitplane import _Hip
    hip = _Hip()
    c, b, want = _poseidon_batch(tmp_path, 1)
    first, count, chunk = 37, 150, 41
    row = c.n_witness * 32
    bufs = [hip.alloc(chunk * row), hip.alloc(chunk * row)]
    seen, parts = [], []

    def consume(f, n, ptr, stream):
        seen.append((f, n, ptr))
        parts.append(hip.download(ptr, (n * row,)))               # synchronises the device: the chunk is complete
        return 0

    b.stream_witnesses_device(first, count, chunk, bufs[0], bufs[1], consume)
    assert seen == [(37, 41, bufs[0]), (78, 41, bufs[1]), (119, 41, bufs[0]), (160, 27, bufs[1])]
    got = np.concatenate(parts).view("<u8").reshape(count, c.n_witness, 4)
    assert (got[:, :, 0] == want[first:first + count]).all() and not got[:, :, 1:].any()
    for p in bufs:
        hip.h.hipFree(p)
    b.close(); c.close()


@pytest.mark.gpu
def test_gpu_grid_limits_and_a_witness_narrower_than_a_tile(tmp_path):
    """BadSquare: 3 wires, batch 70 001 (more instances than one grid dimension holds, 1 094 tiles of 64, the last one of 49)"""
    from circom_amd import runtime as rt
    from test_bitplane import _Hip
    hip = _Hip()
    cp = _badsquare(tmp_path)
    c = rt.Circuit(cp.tape_path, cp.dat_path, cp.r1cs_path)
    assert c.n_witness == 3
    B = 70001
    a = [(i * 0x9E3779B97F4A7C15 + 12345) % Q for i in range(B)]
    want = np.array([[1, (x * x + (x & 1)) % Q, x] for x in a], dtype=np.uint64)
    inp = np.zeros((B, 1, 4), dtype="<u8")
    inp[:, 0, 0] = want[:, 2]
    b = c.batch(B)
    b.set_inputs(inp.view(np.uint8))
    b.run(); b.sync()
    assert (b.status() == 0).all()
    for eb, call in ((32, b.witnesses_device), (8, b.witnesses_device_n8)):
        p, total = _guarded(hip, B * 3 * eb)
        call(0, B, p + GUARD)
        b.sync()
        _check_image(hip, p, total, want, eb)
        hip.h.hipFree(p)
    b.close(); c.close()


@pytest.mark.gpu
def test_gpu_explain_names_the_violated_constraint(tmp_path):
    from circom_amd import runtime as rt
    cp = _badsquare(tmp_path, sym=True)
    c = rt.Circuit(cp.tape_path, cp.dat_path, cp.r1cs_path)
    names = {}
    for line in open(cp.sym_path).read().splitlines():
        s, _, _, nm = line.split(",", 3)
        names[int(s)] = nm
    s_out, s_a = 1, cp.flat.main_input_start
    assert names[s_out].endswith("out") and names[s_a].endswith("a")
    ins = [7, 10, Q - 2]                                         # odd, even, odd
    b = c.batch(len(ins))
    b.set_inputs([[x] for x in ins])
    b.run(); b.check_r1cs(); b.sync()
    for i, x in enumerate(ins):
        text = b.explain(i, cp.sym_path)
        assert text.startswith("instance %d: " % i)
        if x & 1:
            assert "constraint 0 of the .r1cs is violated" in text
            assert "%s = %d;" % (names[s_a], x) in text
            assert "%s = %d;" % (names[s_out], (x * x + 1) % Q) in text
            assert [ln[:4] for ln in text.splitlines()[1:4]] == ["  A:", "  B:", "  C:"]
        else:
            assert text == "instance %d: ok\n" % i
    b.close(); c.close()
