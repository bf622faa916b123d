"""Bulk ingest of the 64-bit runtime (`--prime goldilocks`): cw_set_inputs_n8 / cw_set_inputs_device_n8 (8 bytes per value) and the
tiled-transpose ingest kernel behind both element sizes (csrc/cw64.hip cw64_transpose_in_kernel; CW64_INGEST_TILED=0 keeps
cw64_ingest_kernel, =1 forces the transpose wherever the image's alignment allows it).

Expected values come from the reference's own 64-bit runtime (tests/golden/reference_wtns_goldilocks.json), from the oracle
(oracle.tape_eval.eval_flat, which the chain's closed form is checked against here) or from that closed form in Python
integers - never from another ingest path of the library.  The value table is read back through set_witness_list(all signals) +
witnesses_device_n8, which tests/test_goldilocks_egress.py checks against the oracle on its own.

Chain(n): s[0] = x[0], s[k] = s[k-1] x[k] + x[k], out = s[n-1]; signals [1, out, x[0..n), s[0..n)].  Chain(130) x 300 is two
full input tiles plus 2 by four full instance tiles plus 44."""
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

from circom_amd.compiler import compile_program                                      # noqa: E402
from circom_amd.frontend.dsl import Program, template                                # noqa: E402
from oracle.tape_eval import eval_flat                                               # noqa: E402

GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "reference_wtns_goldilocks.json")))["cases"]
CASES = goldilocks_cases()
Q = 18446744069414584321
CW_EINVAL, CW_EINPUT, CW_EDEVICE, CW_ESTATE = -2, -3, -4, -5
EDGE_K = (0, 63, 64, 128, 129)
EDGES8 = (0, 1, Q - 1, Q, Q + 5, 2**64 - 1)
TILED = pytest.mark.parametrize("tiled", ["1", "0"])


@template
def Chain(c, n):
    x = c.input("x", n)
    out = c.output("out")
    s = c.signal("s", n)
    c.set(s[0], x[0] + 0)
    for k in range(1, n):
        c.set(s[k], s[k - 1] * x[k] + x[k])
    c.set(out, s[n - 1] + 0)


@template
def PlusOne(c):
    a = c.input("a")
    out = c.output("out")
    c.set(out, a + 1)


def closed_form(rows):
    """[instance][1, out, x mod p ..., s ...] as uint64 from rows of Python ints of any size"""
    out = np.empty((len(rows), 2 + 2 * len(rows[0])), dtype=np.uint64)
    for i, row in enumerate(rows):
        x = [v % Q for v in row]
        s = [x[0]]
        for v in x[1:]:
            s.append((s[-1] * v + v) % Q)
        out[i] = [1, s[-1]] + x + s
    return out


def _edges32():
    r = random.Random(3201)
    return tuple(EDGES8) + (2**256 - 1, r.getrandbits(256), r.getrandbits(256), 5 << 192, (2**64 - 2) | (9 << 64))


@functools.lru_cache(maxsize=None)
def _chain_case(eb, B, n=130):
    """(input rows, expected table): seeded values, the first instances carry the edge values at the positions EDGE_K.
    Computed once per shape, shared, never modified."""
    r = random.Random(1000 * eb + B)
    edges = EDGES8 if eb == 8 else _edges32()
    rows = [[r.getrandbits(64) if eb == 8 or r.random() < 0.9 else r.getrandbits(256) for _ in range(n)] for _ in range(B)]
    for i in range(min(B, len(edges))):
        for t, k in enumerate(EDGE_K):
            rows[i][k] = edges[(i + t) % len(edges)]
    if B == 1:                                                     # the single instance meets every edge value
        for t, v in enumerate(edges):
            rows[0][7 + 5 * t] = v
    want = closed_form(rows)
    want.setflags(write=False)
    return tuple(tuple(row) for row in rows), want


def _image(rows, eb):
    """the rows as the bytes of a [batch][n][eb] little-endian image"""
    return np.frombuffer(b"".join(int(v).to_bytes(eb, "little") for row in rows for v in row), dtype=np.uint8)


def _circuit(tmp_path, prog, name):
    from circom_amd import runtime as rt
    cp = compile_program(prog, str(tmp_path), name, sym=False)
    c = rt.Circuit(cp.tape_path, cp.dat_path, cp.r1cs_path)
    c.set_witness_list(np.arange(c.n_signals, dtype=np.uint32))    # egress hands out the whole table
    return cp, c


def _table(hip, c, b):
    """the value table of the signals, [instance][signal] uint64; every status word must be 0 first"""
    b.sync()
    st = b.status()
    assert (st == 0).all(), st[st != 0][:8]
    p = hip.alloc(b.n * c.n_witness * 8)
    b.witnesses_device_n8(0, b.n, p)
    b.sync()
    got = hip.download(p, (b.n, c.n_witness), dtype=np.uint64)
    hip.h.hipFree(p)
    return got


def _same(got, want):
    bad = np.argwhere(got != want)
    assert len(bad) == 0, "first differences at (instance, signal): %s" % bad[:8].tolist()


# ---- without a GPU ---------------------------------------------------------------------------------------------------------------
def test_the_library_exports_the_8_byte_setters():
    from circom_amd import runtime as rt
    L = rt.lib()
    assert hasattr(L, "cw_set_inputs_n8") and hasattr(L, "cw_set_inputs_device_n8")


def test_the_chain_closed_form_is_the_oracle():
    from circom_amd.frontend.flatten import flatten
    fc = flatten(Program(Chain(7), prime="goldilocks"))
    r = random.Random(7)
    row = [r.randrange(Q) for _ in range(7)]
    sig, failed = eval_flat(Q, fc.n_signals, fc.n_temps, fc.constants, fc.code, {fc.main_input_start + k: v for k, v in enumerate(row)})
    assert failed is None and fc.main_input_start == 2
    assert sig[:16] == [int(v) for v in closed_form([row])[0]]


def test_host_only_staging_of_the_8_byte_form(tmp_path):
    from circom_amd import runtime as rt
    cp = compile_program(CASES["multiplier2"][0](), str(tmp_path), "m2g", sym=False)
    c = rt.Circuit(cp.tape_path, cp.dat_path, cp.r1cs_path)
    assert c.element_bytes == 8
    b = c.batch(3, device=-1)
    rows = [[3, 11], [Q + 1, 2**64 - 1], [0, Q - 1]]
    assert b.remaining_inputs(1) == 2
    b.set_inputs_n8(rows)
    for i, row in enumerate(rows):
        assert [b.staged_input(i, k) for k in range(2)] == row      # zero-extended, unreduced
        assert b.remaining_inputs(i) == 0
    b.set_inputs_n8(np.array(rows, dtype=np.uint64)[::-1])
    assert b.staged_input(0, 1) == Q - 1
    with pytest.raises(AssertionError):
        b.set_inputs_n8([[1, 2], [3, 4]])
    with pytest.raises(rt.CwError) as e:
        b.set_inputs_device_n8(4100)                                # 8-byte elements at an address that is no multiple of 8
    assert e.value.code == CW_EINVAL
    b.set_inputs_device_n8(4096)                                    # the pointer is never touched: no device
    assert b.remaining_inputs(2) == 0
    with pytest.raises(rt.CwError) as e:
        b.set_inputs_bits(np.zeros((1, c.n_inputs), dtype=np.uint64))
    assert e.value.code == CW_ESTATE
    with pytest.raises(rt.CwError) as e:
        b.run()
    assert e.value.code == CW_EDEVICE
    b.close(); c.close()


def _staged_after_every_bulk_setter(b, n, steps):
    """each step = (setter, rows): afterwards nothing is left to assign, every cell reads back as the value just given
    (zero-extended), and a per-signal assignment is refused as it is after the last input of the reference's setInputSignal"""
    from circom_amd import runtime as rt
    for setter, rows in steps:
        setter(rows)
        for i, row in enumerate(rows):
            assert b.remaining_inputs(i) == 0
            assert [b.staged_input(i, k) for k in range(n)] == list(row), i
        with pytest.raises(rt.CwError) as e:
            b.set_input_signal(0, "x", 0, 1)
        assert e.value.code == CW_EINPUT and "No more signals to be assigned" in str(e.value)


def test_host_only_bulk_setters_in_sequence(tmp_path):
    """set_inputs_n8, set_inputs, set_inputs_n8 on one host-only batch of the chain circuit: the state after each call is that
    call's alone, whichever form came before.  The 32-byte half again on a 256-bit circuit."""
    from circom_amd import runtime as rt
    n, B = 5, 3
    r = random.Random(55)
    cp = compile_program(Program(Chain(n), prime="goldilocks"), str(tmp_path), "chain5g", sym=False)
    c = rt.Circuit(cp.tape_path, cp.dat_path, cp.r1cs_path)
    assert c.element_bytes == 8 and c.n_inputs == n
    b = c.batch(B, device=-1)
    assert b.remaining_inputs(0) == n
    rows8a = [[r.getrandbits(64) for _ in range(n)] for _ in range(B)]
    rows32 = [[r.getrandbits(256) for _ in range(n)] for _ in range(B)]           # unreduced: staged as given
    rows8b = [list(EDGES8[:n])] + [[r.getrandbits(64) for _ in range(n)] for _ in range(B - 1)]
    _staged_after_every_bulk_setter(b, n, [(b.set_inputs_n8, rows8a), (b.set_inputs, rows32), (b.set_inputs_n8, rows8b)])
    b.close(); c.close()
    cp = compile_program(Program(Chain(n)), str(tmp_path), "chain5", sym=False)
    c = rt.Circuit(cp.tape_path, cp.dat_path, cp.r1cs_path)
    assert c.element_bytes == 32
    b = c.batch(B, device=-1)
    rows_a = [[r.randrange(c.q) for _ in range(n)] for _ in range(B)]
    rows_b = [[c.q - 1, 0, 1, 1 << 200, 7]] + [[r.randrange(c.q) for _ in range(n)] for _ in range(B - 1)]
    _staged_after_every_bulk_setter(b, n, [(b.set_inputs_n8, rows_a), (b.set_inputs, rows_b), (b.set_inputs_n8, rows_a)])
    b.close(); c.close()


def test_the_8_byte_setters_are_the_32_byte_ones_for_a_256_bit_circuit(tmp_path):
    from circom_amd import runtime as rt
    from circom_amd.circuits.basic import Multiplier2
    cp = compile_program(Program(Multiplier2()), str(tmp_path), "m2", sym=False)
    c = rt.Circuit(cp.tape_path, cp.dat_path, cp.r1cs_path)
    assert c.element_bytes == 32
    rows = [[3, 11], [c.q - 1, 2**200 + 5]]
    a, b = c.batch(2, device=-1), c.batch(2, device=-1)
    a.set_inputs(rows)
    b.set_inputs_n8(_image(rows, 32))
    for i in range(2):
        assert [b.staged_input(i, k) for k in range(2)] == [a.staged_input(i, k) for k in range(2)] == rows[i]
        assert b.remaining_inputs(i) == 0
    with pytest.raises(AssertionError):
        b.set_inputs_n8(np.zeros((2, 2), dtype=np.uint64))           # an 8-byte image: the wrong size for this circuit
    b.set_inputs_device_n8(4100)                                     # cw_set_inputs_device: no alignment rule of its own
    a.close(); b.close(); c.close()


# ---- on the GPU ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@TILED
@pytest.mark.parametrize("name", sorted(GOLD))
def test_gpu_goldens_through_the_8_byte_form(name, tiled, tmp_path, monkeypatch):
    from circom_amd import runtime as rt
    monkeypatch.setenv("CW64_INGEST_TILED", tiled)
    mk, _ = CASES[name]
    vecs = GOLD[name]["vectors"]
    cp = compile_program(mk(), str(tmp_path), name, sym=False)
    c = rt.Circuit(cp.tape_path, cp.dat_path, cp.r1cs_path)
    b = c.batch(len(vecs))
    b.set_inputs_n8([[int(v) for v in vec["inputs"]] for vec in vecs])
    b.run(); b.sync()
    assert (b.status() == 0).all(), b.status()
    b.write_wtns_many(0, len(vecs), str(tmp_path / "many%u.wtns"))
    for i, vec in enumerate(vecs):
        got = (tmp_path / ("many%d.wtns" % i)).read_bytes()
        assert len(got) == vec["wtns_len"] and hashlib.sha256(got).hexdigest() == vec["wtns_sha256"], (name, i)
    b.close(); c.close()


@pytest.mark.gpu
@TILED
@pytest.mark.parametrize("B", [300, 1])
@pytest.mark.parametrize("eb", [8, 32])
def test_gpu_chain_against_the_closed_form(eb, B, tiled, tmp_path, monkeypatch):
    from test_bitplane import _Hip
    hip = _Hip()
    monkeypatch.setenv("CW64_INGEST_TILED", tiled)
    rows, want = _chain_case(eb, B)
    _, c = _circuit(tmp_path, Program(Chain(130), prime="goldilocks"), "chain130")
    assert c.n_witness == 262
    b = c.batch(B)
    if eb == 8:
        b.set_inputs_n8(np.array(rows, dtype=np.uint64))
    else:
        b.set_inputs(_image(rows, 32))
    b.run()
    _same(_table(hip, c, b), want)
    b.close(); c.close()


@pytest.mark.gpu
@TILED
@pytest.mark.parametrize("eb", [8, 32])
def test_gpu_device_image_on_an_8_byte_boundary(eb, tiled, tmp_path, monkeypatch):
    """the image 8 bytes into an allocation: the 8-byte form keeps the transpose, the 32-byte form takes the other kernel"""
    from test_bitplane import _Hip
    hip = _Hip()
    monkeypatch.setenv("CW64_INGEST_TILED", tiled)
    rows, want = _chain_case(eb, 300)
    _, c = _circuit(tmp_path, Program(Chain(130), prime="goldilocks"), "chain130")
    img = _image(rows, eb)
    p = hip.upload(np.concatenate([np.full(8, 0xA5, dtype=np.uint8), img]))
    assert p % 16 == 0
    b = c.batch(300)
    (b.set_inputs_device_n8 if eb == 8 else b.set_inputs_device)(p + 8)
    b.run()
    _same(_table(hip, c, b), want)
    b.close(); c.close()
    hip.h.hipFree(p)


@pytest.mark.gpu
@pytest.mark.xdist_group("batch_lifetime")
def test_gpu_launch_split_and_a_circuit_narrower_than_a_tile(tmp_path, monkeypatch):
    """out <== a + 1 x (65 535 * 64 + 65): one instance tile more than a launch holds, the last tile of one instance.
    (About 300 MB of device memory for a moment: the test shares the worker of tests/test_batch_lifetime.py, which compares the
    device's free memory before and after its cycles and must not see this come and go from another process.)"""
    from test_bitplane import _Hip
    hip = _Hip()
    monkeypatch.setenv("CW64_INGEST_TILED", "1")
    _, c = _circuit(tmp_path, Program(PlusOne(), prime="goldilocks"), "plusone")
    assert c.n_witness == 3 and c.n_inputs == 1
    B = 65535 * 64 + 65
    a = np.random.default_rng(4194305).integers(0, 1 << 63, size=B, dtype=np.uint64)
    want = np.stack([np.ones(B, dtype=np.uint64), a + np.uint64(1), a], axis=1)        # a + 1 < p: no reduction
    b = c.batch(B)
    b.set_inputs_n8(a.reshape(B, 1))
    b.run()
    got = _table(hip, c, b)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8].tolist()
    b.close(); c.close()


@pytest.mark.gpu
def test_gpu_more_inputs_than_a_grid_dimension(tmp_path, monkeypatch):
    """Chain(65 601) x 3 in automatic mode: 1 026 input tiles, the last one of one input; the lane-per-instance kernel's grid
    cannot hold this circuit (65 535 inputs at most)"""
    from test_bitplane import _Hip
    hip = _Hip()
    monkeypatch.delenv("CW64_INGEST_TILED", raising=False)
    n = 65601
    r = random.Random(65601)
    rows = [[r.getrandbits(64) for _ in range(n)] for _ in range(3)]
    for i in range(3):
        rows[i][0], rows[i][65535], rows[i][65536], rows[i][n - 1] = EDGES8[i], EDGES8[i + 1], EDGES8[i + 2], EDGES8[i + 3]
    _, c = _circuit(tmp_path, Program(Chain(n), prime="goldilocks"), "chain65601")
    assert c.n_inputs == n
    b = c.batch(3)
    b.set_inputs_n8(np.array(rows, dtype=np.uint64))
    b.run()
    _same(_table(hip, c, b), closed_form(rows))
    b.close(); c.close()


@pytest.mark.gpu
@TILED
def test_gpu_run_check_graph_is_keyed_on_the_input_form(tiled, tmp_path, monkeypatch):
    """the same device pointer registered as a 32-byte image, captured, then as an 8-byte image: the graph of the first form is
    dropped, the table holds what the first 300 * 130 words of the buffer say (the chain's constraints hold for any inputs)"""
    from test_bitplane import _Hip
    hip = _Hip()
    monkeypatch.setenv("CW64_INGEST_TILED", tiled)
    rows, want = _chain_case(32, 300)
    img = _image(rows, 32)
    _, c = _circuit(tmp_path, Program(Chain(130), prime="goldilocks"), "chain130")
    p = hip.upload(img)
    b = c.batch(300)
    b.set_inputs_device(p)
    for _ in range(3):
        b.run_check()
    assert b.graph_captured
    _same(_table(hip, c, b), want)
    assert (b.r1cs_first_bad() == 0xFFFFFFFF).all()
    b.set_inputs_device_n8(p)
    b.run_check()
    words = img.view("<u8")[:300 * 130].reshape(300, 130)
    _same(_table(hip, c, b), closed_form([[int(v) for v in row] for row in words]))
    assert (b.r1cs_first_bad() == 0xFFFFFFFF).all()
    b.close(); c.close()
    hip.h.hipFree(p)


@pytest.mark.gpu
@TILED
def test_gpu_a_32_byte_setter_resets_the_form(tiled, tmp_path, monkeypatch):
    from test_bitplane import _Hip
    hip = _Hip()
    monkeypatch.setenv("CW64_INGEST_TILED", tiled)
    rows8, _ = _chain_case(8, 300)
    rows32, want32 = _chain_case(32, 300)
    _, c = _circuit(tmp_path, Program(Chain(130), prime="goldilocks"), "chain130")
    b = c.batch(300)
    b.set_inputs_n8(np.array(rows8, dtype=np.uint64))
    b.set_inputs(_image(rows32, 32))
    b.run()
    _same(_table(hip, c, b), want32)
    b.close(); c.close()
