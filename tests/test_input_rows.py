"""Boolean inputs as packed rows: cw_set_inputs_rows / cw_set_inputs_rows_device (include/circom_amd.h) - instance j's inputs are
the first ceil(n_inputs / 8) bytes of rows + j * stride, input k is bit k & 7 of byte k >> 3 or, CW_ROWS_MSB_FIRST, bit
7 - (k & 7) (np.unpackbits' order: a SHA-256 message as it stands).  Bit-plane batches transpose the bits on the device
(csrc/cw_bits.hip cw_bits_rows_to_masks_kernel: tiles of 64 instances x 64 words), the 64-bit runtime and the 256-bit schedule
expand them to their own image of values (csrc/cw_kernels.hip cw_rows_expand_kernel).

Expected values come from oracle.tape_eval (eval_flat, check_r1cs) and hashlib, never from another call into the library.
`rows_to_masks` below is the numpy model of the transpose; one CPU test checks it against the packbits construction of
bench.py's masks().  The shapes: BitGadget(n), 3 n inputs - 45 (part of one word, no whole number of bytes), 66 (one word + 2
bits), 129 (two words + 1 bit); batches of 1, 63, 64, 65 and 300 instances (one tile less one, one tile, one more, four full
tiles + 44); 70 001 instances for the grid's x dimension."""
import ctypes as C
import functools
import hashlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
from test_bitplane import BitAssert, BitGadget, _Hip                                 # noqa: E402

from circom_amd.circuits.basic import Multiplier2                                    # noqa: E402
from circom_amd.circuits.sha256 import Sha256                                        # noqa: E402
from circom_amd.compiler import compile_program                                      # noqa: E402
from circom_amd.frontend.dsl import Program                                          # noqa: E402
from circom_amd.frontend.flatten import flatten                                      # noqa: E402
from oracle.tape_eval import check_r1cs, eval_flat                                   # noqa: E402

CW_EINVAL, CW_EDEVICE = -2, -4
MSB = 1                                                                              # CW_ROWS_MSB_FIRST
B_MAX = 300


# ---- models ----------------------------------------------------------------------------------------------------------------------
def rows_to_masks(rows, n_in, msb):
    """uint64 masks[ceil(B / 64)][n_in] of packed rows [B][>= ceil(n_in / 8)]: bit i of masks[g][k] = input k of instance
    64 g + i (the layout cw_set_inputs_bits takes); instances past B are 0"""
    B = rows.shape[0]
    bits = np.unpackbits(rows[:, :(n_in + 7) // 8], axis=1, bitorder="big" if msb else "little")[:, :n_in]
    out = np.zeros(((B + 63) // 64, n_in), dtype=np.uint64)
    for i in range(B):
        out[i // 64] |= bits[i].astype(np.uint64) << np.uint64(i % 64)
    return out


def pack_rows(bits, stride, msb):
    """[B][n] bits -> [B][stride] bytes; the spare bits of the last used byte and every pad byte are ones"""
    B, n = bits.shape
    used = (n + 7) // 8
    assert stride >= used
    full = np.ones((B, used * 8), dtype=np.uint8)
    full[:, :n] = bits
    rows = np.full((B, stride), 0xFF, dtype=np.uint8)
    rows[:, :used] = np.packbits(full, axis=1, bitorder="big" if msb else "little")
    return rows


def _bits(n_in, B, seed):
    bits = np.random.default_rng(seed).integers(0, 2, size=(B, n_in), dtype=np.uint8)
    bits[0] = 1                                                   # an instance of ones and one of zeros
    if B > 1:
        bits[1] = 0
    return bits


def _oracle(fc, bits):
    """[B][n_signals][32] canonical little-endian signals of eval_flat on each row of bits; none may fail, and the first and the
    last satisfy the constraint system"""
    q = fc.fp.q
    out = np.zeros((len(bits), fc.n_signals, 32), dtype=np.uint8)
    for i, row in enumerate(bits):
        sig, failed = eval_flat(q, fc.n_signals, fc.n_temps, fc.constants, fc.code,
                                {fc.main_input_start + k: int(v) for k, v in enumerate(row)})
        assert failed is None
        if i in (0, len(bits) - 1):
            assert check_r1cs(q, fc.constraints, sig) is None
        out[i] = np.frombuffer(b"".join(v.to_bytes(32, "little") for v in sig), dtype=np.uint8).reshape(-1, 32)
    out.setflags(write=False)
    return out


# ---- without a GPU ---------------------------------------------------------------------------------------------------------------
def test_the_library_exports_the_row_setters():
    from circom_amd import runtime as rt
    L = rt.lib()
    assert hasattr(L, "cw_set_inputs_rows") and hasattr(L, "cw_set_inputs_rows_device")
    assert rt.ROWS_MSB_FIRST == MSB and hasattr(rt.Batch, "set_inputs_rows") and hasattr(rt.Batch, "set_inputs_rows_device")


@pytest.mark.parametrize("msb", [True, False])
def test_the_model_is_the_packbits_construction(msb):
    """the masks as bench.py's masks() and the tests of cw_set_inputs_bits build them"""
    n, B = 45, 130
    bits = _bits(n, B, 5)
    g = (B + 63) // 64
    blk = np.zeros((g * 64, n), dtype=np.uint8)
    blk[:B] = bits
    m = np.packbits(blk.reshape(g, 64, n), axis=1, bitorder="little")
    want = np.ascontiguousarray(m.transpose(0, 2, 1)).view(np.uint64).reshape(g, n)
    for stride in (6, 9):
        assert (rows_to_masks(pack_rows(bits, stride, msb), n, msb) == want).all()
    assert int(want[2, 0]) == int(bits[128, 0]) | int(bits[129, 0]) << 1


def _host_circuit(tmp_path, kind):
    from circom_amd import runtime as rt
    if kind == "m2":
        cp = compile_program(Program(Multiplier2()), str(tmp_path), "m2", sym=False)
    elif kind == "m2g":
        cp = compile_program(Program(Multiplier2(), prime="goldilocks"), str(tmp_path), "m2g", sym=False)
    else:
        cp = compile_program(Program(BitGadget(15)), str(tmp_path), "bg15h", sym=False, strands=(1,), bits=True, jit=False)
    return rt.Circuit(cp.tape_path, cp.dat_path, cp.r1cs_path)


@pytest.mark.parametrize("kind", ["m2", "m2g", "bg15"])
def test_host_only_staging_and_argument_checks(tmp_path, kind):
    from circom_amd import runtime as rt
    L = rt.lib()
    c = _host_circuit(tmp_path, kind)
    n = c.n_inputs
    assert n == (45 if kind == "bg15" else 2)
    used, B = (n + 7) // 8, 5
    b = c.batch(B, device=-1)
    bits = _bits(n, B, 11)
    for msb in (True, False):
        b2 = c.batch(B, device=-1)
        assert b2.remaining_inputs(B - 1) == n
        b2.set_inputs_rows(pack_rows(bits, used + 3, msb), msb_first=msb)
        for i in range(B):
            assert [b2.staged_input(i, k) for k in range(n)] == bits[i].tolist(), (msb, i)
            assert b2.remaining_inputs(i) == 0
        b2.close()
    rows = pack_rows(bits, used + 3, True)
    p = rows.ctypes.data_as(C.c_void_p)
    call = lambda fn, ptr, stride, flags: fn(b.h, ptr, stride, flags)
    assert call(L.cw_set_inputs_rows, p, used + 3, MSB) == 0
    assert call(L.cw_set_inputs_rows, p, used - 1, MSB) == CW_EINVAL                 # a stride one byte short
    assert call(L.cw_set_inputs_rows, None, used + 3, MSB) == CW_EINVAL
    assert L.cw_set_inputs_rows(None, p, used + 3, MSB) == CW_EINVAL
    assert call(L.cw_set_inputs_rows, p, used + 3, 2) == CW_EINVAL                   # flag bit 2
    assert call(L.cw_set_inputs_rows, p, used + 3, 2 | MSB) == CW_EINVAL
    # the device form: argument checks first (the pointer is never touched), then the device
    w8 = 8 * ((n + 63) // 64)
    assert call(L.cw_set_inputs_rows_device, None, w8, MSB) == CW_EINVAL
    assert call(L.cw_set_inputs_rows_device, C.c_void_p(4096 + 4), w8, MSB) == CW_EINVAL
    assert call(L.cw_set_inputs_rows_device, C.c_void_p(4096), 12, MSB) == CW_EINVAL
    assert call(L.cw_set_inputs_rows_device, C.c_void_p(4096), w8 - 8, MSB) == CW_EINVAL
    assert call(L.cw_set_inputs_rows_device, C.c_void_p(4096), w8, 2) == CW_EINVAL
    assert call(L.cw_set_inputs_rows_device, C.c_void_p(4096), w8, MSB) == CW_EDEVICE
    assert call(L.cw_set_inputs_rows_device, C.c_void_p(4096), w8 + 8, 0) == CW_EDEVICE
    with pytest.raises(rt.CwError) as e:
        b.set_inputs_rows(rows[:, :used - 1].copy())
    assert e.value.code == CW_EINVAL
    with pytest.raises(AssertionError):
        b.set_inputs_rows(rows[:, ::2])                                              # not C-contiguous
    with pytest.raises(AssertionError):
        b.set_inputs_rows(rows[:B - 1])
    b.close(); c.close()


# ---- GPU -------------------------------------------------------------------------------------------------------------------------
class _Dev(_Hip):
    """row images on the device: the image ENDS where its allocation ends, behind a 4 096-byte guard in front"""

    def put(self, p, arr):
        assert self.h.hipMemcpy(p, arr.ctypes.data, arr.nbytes, 1) == 0

    def rows_at_end(self, rows):
        base = self.alloc(4096 + rows.nbytes)
        self.put(base + 4096, rows)
        return base, base + 4096


@pytest.fixture(scope="module")
def hip():
    return _Dev()


@pytest.fixture(scope="module")
def circuits(tmp_path_factory):
    """every circuit of this module, compiled once: name -> (flat circuit, runtime circuit)"""
    from circom_amd import runtime as rt
    made = {}

    def get(name):
        if name not in made:
            d = str(tmp_path_factory.mktemp(name))
            if name.startswith("bg"):
                cp = compile_program(Program(BitGadget(int(name[2:]))), d, name, sym=False, strands=(1,), bits=True, jit=True)
                assert cp.jit is not None
            elif name == "gl15":
                cp = compile_program(Program(BitGadget(15), prime="goldilocks"), d, name, sym=False)
            elif name == "bassert":
                cp = compile_program(Program(BitAssert()), d, name, sym=False, strands=(1,), bits=True, jit=True)
            else:                                                 # (the one-block SHA-256: its lowering is most of that test's time)
                cp = compile_program(Program(Sha256(64)), d, name, sym=False, strands=(1,), bits=True, jit=False)
            c = rt.Circuit(cp.tape_path, cp.dat_path, cp.r1cs_path)
            if name == "gl15":
                c.set_witness_list(np.arange(c.n_signals, dtype=np.uint32))
            assert c.n_witness == cp.flat.n_signals
            made[name] = (cp.flat, c)
        return made[name]

    yield get
    for _, c in made.values():
        c.close()


@functools.lru_cache(maxsize=None)
def _case(n, prime="bn128"):
    """(bits [300][3 n], expected signals [300][n_signals][32]) of BitGadget(n): computed once, shared, never modified; a batch
    of B instances takes the first B"""
    fc = flatten(Program(BitGadget(n), prime=prime) if prime != "bn128" else Program(BitGadget(n)))
    bits = _bits(3 * n, B_MAX, 100 + n)
    bits.setflags(write=False)
    return bits, _oracle(fc, bits)


def _run_and_compare(b, want):
    b.run(); b.check_r1cs(); b.sync()
    st = b.status()
    assert (st == 0).all(), st[st != 0][:8]
    got = b.witnesses()
    bad = np.argwhere((got != want).any(axis=2))
    assert len(bad) == 0, "first differences at (instance, signal): %s" % bad[:8].tolist()


def _every_form(hip, b, bits, want, host=True):
    """both bit orders x {host rows with 3 spare bytes, device rows of whole words, device rows with 8 bytes more}: spare bits and
    pad bytes all ones, the device image at the end of its allocation"""
    n = bits.shape[1]
    for msb in (True, False):
        if host:
            b.set_inputs_rows(pack_rows(bits, (n + 7) // 8 + 3, msb), msb_first=msb)
            _run_and_compare(b, want)
        for extra in (0, 8):
            stride = 8 * ((n + 63) // 64) + extra
            base, p = hip.rows_at_end(pack_rows(bits, stride, msb))
            b.set_inputs_rows_device(p, stride, msb_first=msb)
            _run_and_compare(b, want)
            hip.h.hipFree(base)


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 63, 64, 65, 300])
@pytest.mark.parametrize("n", [15, 22, 43])
@pytest.mark.parametrize("engine", ["interp", "jit"])
def test_gpu_bitplane_rows_at_the_tile_edges(circuits, hip, monkeypatch, engine, n, B):
    monkeypatch.setenv("CW_BITS_JIT", "1" if engine == "jit" else "0")
    fc, c = circuits("bg%d" % n)
    bits, want = _case(n)
    b = c.batch(B)
    assert b.bitmode and b.jit == (engine == "jit") and c.n_inputs == 3 * n
    _every_form(hip, b, bits[:B], want[:B])
    b.close()


@pytest.mark.gpu
def test_gpu_sha256_rows_are_the_messages(circuits, hip):
    """the user story: Sha256(64) x 130, the rows ARE the 8-byte messages"""
    fc, c = circuits("sha64")
    B = 130
    msgs = np.random.default_rng(64).integers(0, 256, size=(B, 8), dtype=np.uint8)
    rev = np.packbits(np.unpackbits(msgs, axis=1, bitorder="little"), axis=1, bitorder="big")    # bits of each byte reversed
    assert rev[0, 0] == int("{:08b}".format(msgs[0, 0])[::-1], 2)
    digest = lambda m: np.unpackbits(np.frombuffer(hashlib.sha256(m.tobytes()).digest(), dtype=np.uint8))
    b = c.batch(B)
    assert b.bitmode and c.n_inputs == 64
    for msb, said in ((True, msgs), (False, rev)):
        for form in ("host", "device"):
            if form == "host":
                b.set_inputs_rows(msgs, msb_first=msb)
            else:
                base, p = hip.rows_at_end(msgs)
                b.set_inputs_rows_device(p, 8, msb_first=msb)
            b.run(); b.check_r1cs(); b.sync()
            assert (b.status() == 0).all()
            pub = b.public_signals()
            for i in range(B):
                assert (pub[i, :256, 0] == digest(said[i])).all() and not pub[i, :256, 1:].any(), (msb, form, i)
            if form == "device":
                hip.h.hipFree(base)
    b.close()


@pytest.mark.gpu
def test_gpu_rows_beyond_65535_groups_of_the_grid(circuits, hip):
    """BitAssert (a === b, out = a b) x 70 001 from device rows of one word: the instance tiles are the grid's x dimension"""
    fc, c = circuits("bassert")
    B = 70001
    assert c.n_inputs == 2
    bits = np.random.default_rng(70001).integers(0, 2, size=(B, 1), dtype=np.uint8).repeat(2, axis=1)
    for i, v in ((0, 1), (65535, 1), (65536, 0), (70000, 1)):
        bits[i] = v
    odd = np.arange(500, B, 997)                                  # a != b: the assertion fails there
    assert not set(odd.tolist()) & {0, 65535, 65536, 70000}
    bits[odd, 1] ^= 1
    model = {}
    for a in (0, 1):
        for v in (0, 1):
            model[a, v] = eval_flat(fc.fp.q, fc.n_signals, fc.n_temps, fc.constants, fc.code,
                                    {fc.main_input_start: a, fc.main_input_start + 1: v})
            assert (model[a, v][1] is not None) == (a != v)
    for msb in (True, False):
        base, p = hip.rows_at_end(pack_rows(bits, 8, msb))
        b = c.batch(B)
        assert b.bitmode
        b.set_inputs_rows_device(p, 8, msb_first=msb)
        b.run(); b.sync()
        st = b.status()
        assert ((st & 1) == (bits[:, 0] != bits[:, 1])).all()
        assert ((st == 0) == (bits[:, 0] == bits[:, 1])).all()
        pub = b.public_signals()
        assert (pub[:, 0, 0] == (bits[:, 0] & bits[:, 1])).all() and not pub[:, 0, 1:].any()
        for i in (0, 65535, 65536, 70000):
            assert b.witness(i) == model[int(bits[i, 0]), int(bits[i, 1])][0], i
        b.close()
        hip.h.hipFree(base)


def _other_engine(circuits, monkeypatch, kind, B):
    """(batch, bits, expected) of BitGadget(15) on an engine that ingests an image of values"""
    if kind == "gl":
        fc, c = circuits("gl15")
        bits, want = _case(15, "goldilocks")
        b = c.batch(B)
        assert c.element_bytes == 8 and not b.bitmode
    else:
        fc, c = circuits("bg15")
        bits, want = _case(15)
        monkeypatch.setenv("CW_BITS", "0")
        b = c.batch(B)
        monkeypatch.delenv("CW_BITS")
        assert c.element_bytes == 32 and not b.bitmode
    return b, bits[:B], want[:B]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,B", [("gl", 65), ("gl", 300), ("wide", 65)])
def test_gpu_rows_on_the_engines_that_ingest_values(circuits, hip, monkeypatch, kind, B):
    b, bits, want = _other_engine(circuits, monkeypatch, kind, B)
    _every_form(hip, b, bits, want)
    b.close()


def _values(bits):
    arr = np.zeros(bits.shape + (32,), dtype=np.uint8)
    arr[:, :, 0] = bits
    return arr


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["bits", "gl", "wide"])
def test_gpu_the_batch_follows_the_latest_setter(circuits, hip, monkeypatch, kind):
    B = 65
    if kind == "bits":
        fc, c = circuits("bg15")
        b = c.batch(B)
        assert b.bitmode
    else:
        b = _other_engine(circuits, monkeypatch, kind, B)[0]
    bits, want = _case(15, "goldilocks" if kind == "gl" else "bn128")
    n = bits.shape[1]
    one, two = (bits[:B], want[:B]), (bits[100:100 + B], want[100:100 + B])
    assert (one[0] != two[0]).any() and (one[1] != two[1]).any()
    b.set_inputs_rows(pack_rows(one[0], (n + 7) // 8, True))
    b.set_inputs(_values(two[0]))
    _run_and_compare(b, two[1])
    b.set_inputs(_values(two[0]))
    base, p = hip.rows_at_end(pack_rows(one[0], 8, False))
    b.set_inputs_rows_device(p, 8, msb_first=False)
    _run_and_compare(b, one[1])
    b.set_inputs_rows(pack_rows(two[0], 9, True))
    _run_and_compare(b, two[1])
    hip.h.hipFree(base)
    b.close()


@pytest.mark.gpu
def test_gpu_run_check_replays_its_graph_over_new_rows(circuits, hip):
    """three steps from the same device pointer with new rows between them: the conversion runs inside each call and writes the
    batch's own masks, so the input key of cw_run_check stays and the graph is captured and replayed"""
    fc, c = circuits("bg15")
    bits, want = _case(15)
    B = 65
    b = c.batch(B)
    base, p = hip.rows_at_end(pack_rows(bits[:B], 8, True))
    for step, first in enumerate((0, 100, 200)):
        hip.put(p, pack_rows(bits[first:first + B], 8, True))
        b.set_inputs_rows_device(p, 8)
        b.run_check(); b.sync()
        assert (b.status() == 0).all()
        assert (b.witnesses() == want[first:first + B]).all(), step
    assert b.graph_captured
    hip.h.hipFree(base)
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["bits", "gl"])
def test_gpu_the_device_rows_are_free_once_the_stream_has_passed_the_call(circuits, hip, monkeypatch, kind):
    B = 65
    if kind == "bits":
        fc, c = circuits("bg15")
        (bits, want), b = _case(15), c.batch(B)
    else:
        b, bits, want = _other_engine(circuits, monkeypatch, kind, B)
    rows = pack_rows(bits[:B], 8, True)
    base, p = hip.rows_at_end(rows)
    b.set_inputs_rows_device(p, 8)
    b.sync()
    hip.put(p, np.random.default_rng(9).integers(0, 256, size=rows.shape, dtype=np.uint8))    # garbage: the bits were taken inside the call
    _run_and_compare(b, want[:B])
    hip.h.hipFree(base)
    b.close()
