"""Witness bits out as packed rows: cw_get_witness_rows / cw_get_witness_rows_device (include/circom_amd.h) - entries
[entry0, entry0 + n) of the witness list for the instances [first, first + count); row j = instance first + j, entry entry0 + k is
bit k & 7 of byte k >> 3 or, CW_ROWS_MSB_FIRST, bit 7 - (k & 7) (np.packbits' order: a SHA-256 digest as it stands); the bit is 1
if and only if the value is 1, and a value that is neither 0 nor 1 is reported through one word (the lowest such instance).
One kernel per table layout: csrc/cw_bits.hip cw_bits_masks_to_rows_kernel (both bit-table layouts), csrc/cw64.hip
cw64_pack_rows_kernel, csrc/cw_kernels.hip cw_pack_rows_kernel - tiles of 64 instances x 64 words of 64 entries.

Expected values come from oracle.tape_eval.eval_flat and hashlib, packed with np.packbits (`model` below), never from another call
into the library.  The shapes: BitGadget(15) has 380 signals (five words + 60 entries), BitGadget(43) more than 1 000; the entry
ranges start and end inside bytes and words, the instance ranges start inside a group of 64 and straddle groups; batches of 65
and 300 (one tile + 1, four tiles + 44); Sha256(64) for more than one word tile; 70 001 instances for the grid's x dimension.
The circuits and the oracle of BitGadget are the ones tests/test_input_rows.py builds (imported: computed once per session)."""
import ctypes as C
import functools
import hashlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
from test_bitplane import BitAssert, BitGadget, _Hip                                 # noqa: E402,F401
from test_input_rows import _bits, _case, pack_rows                                  # noqa: E402

from circom_amd.circuits.basic import Multiplier2                                    # noqa: E402
from circom_amd.circuits.sha256 import Sha256                                        # noqa: E402
from circom_amd.compiler import compile_program                                      # noqa: E402
from circom_amd.frontend.dsl import Program                                          # noqa: E402
from circom_amd.frontend.flatten import flatten                                      # noqa: E402
from oracle.tape_eval import eval_flat                                               # noqa: E402

CW_EINVAL, CW_EDEVICE, CW_ESTATE = -2, -4, -5
MSB = 1                                                                              # CW_ROWS_MSB_FIRST
NONE = 0xFFFFFFFF
RANGES = [(0, 1), (1, 7), (1, 8), (5, 9), (0, 63), (1, 64), (3, 65), (0, 129), (0, None)]   # (entry0, n); None = the whole witness
FOUR_RANGES = [(1, 7), (5, 9), (3, 65), (0, None)]


def inst_ranges(B):
    """(first, count): the whole batch, one instance, a range that ends with the first group, one that straddles two groups, a
    whole group from a group's start, a range that starts inside a group and covers whole ones, the last instance.  At B = 300
    these are (0, 300), (0, 1), (1, 63), (63, 2), (64, 64), (37, 200), (299, 1); a smaller batch clips the counts"""
    return [(0, B), (0, 1), (1, 63), (63, 2), (64, min(64, B - 64)), (37, min(200, B - 37)), (B - 1, 1)]


# ---- model -----------------------------------------------------------------------------------------------------------------------
def is_one(values):
    """[B][n][32] canonical little-endian values -> [B][n] uint8: 1 where the value is 1"""
    return ((values[:, :, 0] == 1) & ~values[:, :, 1:].any(axis=2)).astype(np.uint8)


def not_bool(values):
    """[B][n] bool: the value is neither 0 nor 1"""
    return (values[:, :, 0] > 1) | values[:, :, 1:].any(axis=2)


def model(ones, entry0, n, first, count, msb):
    """[count][ceil(n / 8)] uint8: the rows the calls must produce from ones[instance][entry]; spare bits 0"""
    return np.packbits(ones[first:first + count, entry0:entry0 + n], axis=1, bitorder="big" if msb else "little")


def model_word(bad, entry0, n, first, count):
    hit = np.flatnonzero(bad[first:first + count, entry0:entry0 + n].any(axis=1))
    return first + int(hit[0]) if len(hit) else NONE


# ---- without a GPU ---------------------------------------------------------------------------------------------------------------
def test_the_library_exports_the_row_getters():
    from circom_amd import runtime as rt
    L = rt.lib()
    assert hasattr(L, "cw_get_witness_rows") and hasattr(L, "cw_get_witness_rows_device")
    for name in ("witness_rows", "witness_rows_device", "public_rows"):
        assert hasattr(rt.Batch, name)


@pytest.mark.parametrize("k", [45, 64])
def test_lsb_first_rows_are_the_layout_of_pack_bit_rows(k):
    """public_rows(msb_first=False) is what sharding.pack_bit_rows makes of the 32-byte image of the public signals"""
    import torch
    from circom_amd.sharding import pack_bit_rows
    ones = _bits(k + 1, 70, 7)                                     # entry 0 and k public signals
    image = np.zeros((70, k, 32), dtype=np.uint8)
    image[:, :, 0] = ones[:, 1:]
    want = pack_bit_rows(torch.from_numpy(image)).numpy()
    got = model(ones, 1, k, 0, 70, False)
    assert got.shape == want.shape == (70, (k + 7) // 8) and (got == want).all()
    assert (model(ones, 1, k, 0, 70, True) != want).any()


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
def test_argument_checks_come_before_the_device(tmp_path, kind):
    """a host-only batch: every CW_EINVAL case is CW_EINVAL, and only a call whose arguments are in order reaches CW_EDEVICE"""
    from circom_amd import runtime as rt
    L = rt.lib()
    c = _host_circuit(tmp_path, kind)
    nw, B = c.n_witness, 5
    assert nw >= 4
    b = c.batch(B, device=-1)
    used, w8 = (nw + 7) // 8, 8 * ((nw + 63) // 64)
    rows = np.full((B, used + 3), 0xA5, dtype=np.uint8)
    p = rows.ctypes.data_as(C.c_void_p)
    word = C.c_uint32(123)
    host = lambda e0, n, f, cnt, ptr, stride, flags, h=b.h: L.cw_get_witness_rows(h, e0, n, f, cnt, ptr, stride, flags, C.byref(word))
    dev = lambda e0, n, f, cnt, ptr, stride, flags, dw=None, h=b.h: L.cw_get_witness_rows_device(h, e0, n, f, cnt, ptr, stride, flags, dw)
    d = C.c_void_p(4096)
    for call, ptr, stride in ((host, p, used + 3), (dev, d, w8)):
        assert call(0, nw, 0, B, ptr, stride, MSB, h=None) == CW_EINVAL                 # null batch
        assert call(0, nw, 0, B, None, stride, MSB) == CW_EINVAL                        # null rows
        assert call(0, nw + 1, 0, B, ptr, stride + 8, MSB) == CW_EINVAL                 # entries past the witness list
        assert call(nw, 1, 0, B, ptr, stride, MSB) == CW_EINVAL
        assert call(2, 0xFFFFFFFF, 0, B, ptr, stride, MSB) == CW_EINVAL                 # entry0 + n wraps in 32 bits
        assert call(0, nw, 0, B + 1, ptr, stride, MSB) == CW_EINVAL                     # instances past the batch
        assert call(0, nw, B, 1, ptr, stride, MSB) == CW_EINVAL
        assert call(0, nw, 2, 0xFFFFFFFF, ptr, stride, MSB) == CW_EINVAL
        assert call(0, nw, 0, B, ptr, stride, 2) == CW_EINVAL                           # flag bit 2
        assert call(0, nw, 0, B, ptr, stride, 2 | MSB) == CW_EINVAL
        assert "cw_get_witness_rows" in L.cw_last_error().decode()
    assert host(0, nw, 0, B, p, used - 1, MSB) == CW_EINVAL                             # a stride one byte short
    assert dev(0, nw, 0, B, C.c_void_p(4096 + 4), w8, MSB) == CW_EINVAL                 # alignment of the rows
    assert dev(0, nw, 0, B, d, w8 + 4, MSB) == CW_EINVAL                                # stride no multiple of 8
    assert dev(0, nw, 0, B, d, w8 - 8, MSB) == CW_EINVAL                                # the last word outside the row
    assert dev(0, nw, 0, B, d, w8, MSB, C.c_void_p(8192 + 2)) == CW_EINVAL              # alignment of the word
    # in order: the device comes next (and the state after it - with a device, test_gpu_state_and_empty_ranges)
    assert host(0, nw, 0, B, p, used + 3, MSB) == CW_EDEVICE
    assert host(1, 2, 1, 3, p, 1, 0) == CW_EDEVICE
    assert host(nw, 0, B, 0, p, 0, 0) == CW_EDEVICE
    assert dev(0, nw, 0, B, d, w8, MSB) == CW_EDEVICE
    assert dev(0, nw, 0, B, d, w8 + 8, 0, C.c_void_p(8192 + 4)) == CW_EDEVICE
    assert dev(1, 1, B - 1, 1, d, 8, 0) == CW_EDEVICE
    assert (rows == 0xA5).all() and word.value == 123                                   # nothing was written
    with pytest.raises(rt.CwError) as e:
        b.witness_rows(0, nw + 1)
    assert e.value.code == CW_EINVAL
    with pytest.raises(rt.CwError) as e:
        b.public_rows()
    assert e.value.code == CW_EDEVICE
    b.close(); c.close()


# ---- GPU -------------------------------------------------------------------------------------------------------------------------
class _Dev(_Hip):
    """one arena; a row image ENDS where the arena's allocation ends"""
    SIZE = 4 << 20

    def __init__(self):
        super().__init__()
        self.h.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        self.base = self.alloc(self.SIZE)
        self.word = self.alloc(8)

    def put(self, p, arr):
        assert self.h.hipMemcpy(p, arr.ctypes.data, arr.nbytes, 1) == 0

    def at_end(self, nbytes, fill=0xA5):
        assert nbytes % 8 == 0 and nbytes <= self.SIZE
        p = self.base + self.SIZE - nbytes
        self.put(p, np.full(nbytes, fill, dtype=np.uint8))
        return p

    def rows_device(self, b, entry0, n, first, count, stride, msb, p=None):
        """(rows [count][stride], word) of the device form into 0xA5 bytes at the end of the arena (or at p, as it stands)"""
        if p is None:
            p = self.at_end(count * stride)
        self.put(self.word, np.array([0x12345678], dtype=np.uint32))
        b.witness_rows_device(entry0, n, first, count, p, stride, msb_first=msb, d_not_boolean=self.word)
        return self.download(p, (count, stride)), int(self.download(self.word, 1, np.uint32)[0])


@pytest.fixture(scope="module")
def hip():
    return _Dev()


@pytest.fixture(scope="module")
def circuits(tmp_path_factory):
    """every circuit of this module, compiled once: name -> (flat circuit, runtime circuit); the witness list is every signal"""
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
            elif name == "m2":
                cp = compile_program(Program(Multiplier2()), d, name, sym=False, strands=(1,), pipe=None)    # (one variant: seconds less)
            elif name == "m2mont":
                cp = compile_program(Program(Multiplier2()), d, name, sym=False, strands=(1,), pipe=None, mont=True)
            else:
                cp = compile_program(Program(Sha256(64)), d, name, sym=False, strands=(1,), bits=True, jit=False)
            c = rt.Circuit(cp.tape_path, cp.dat_path, cp.r1cs_path)
            if c.n_witness != cp.flat.n_signals:
                c.set_witness_list(np.arange(c.n_signals, dtype=np.uint32))
            assert c.n_witness == cp.flat.n_signals
            made[name] = (cp.flat, c)
        return made[name]

    yield get
    for _, c in made.values():
        c.close()


def _host_rows(b, entry0, n, first, count, stride, msb):
    """(rows [count][stride], word) of the host form into an array of 0xA5 bytes"""
    from circom_amd import runtime as rt
    rows = np.full((count, stride), 0xA5, dtype=np.uint8)
    word = C.c_uint32(0x12345678)
    rt._chk(rt.lib().cw_get_witness_rows(b.h, entry0, n, first, count, rows.ctypes.data_as(C.c_void_p), stride, MSB if msb else 0, C.byref(word)))
    return rows, word.value


def _check_range(hip, b, ones, bad, entry0, n, first, count, host=True):
    """both bit orders x {host rows with 3 spare bytes, device rows of whole words, device rows with 8 bytes more}"""
    used, w8 = (n + 7) // 8, 8 * ((n + 63) // 64)
    word = model_word(bad, entry0, n, first, count)
    where = (entry0, n, first, count)
    for msb in (True, False):
        want = model(ones, entry0, n, first, count, msb)
        if host:
            rows, got_word = _host_rows(b, entry0, n, first, count, used + 3, msb)
            assert (rows[:, :used] == want).all() and (rows[:, used:] == 0xA5).all() and got_word == word, ("host", msb) + where
        for stride in (w8, w8 + 8):
            rows, got_word = hip.rows_device(b, entry0, n, first, count, stride, msb)
            assert (rows[:, :used] == want).all(), ("device", stride, msb) + where
            assert (rows[:, used:w8] == 0).all() and (rows[:, w8:] == 0xA5).all() and got_word == word, ("device", stride, msb) + where


def _matrix(hip, b, ones, bad, ranges, B):
    nw = ones.shape[1]
    for entry0, n in ranges:
        for first, count in inst_ranges(B):
            _check_range(hip, b, ones[:B], bad[:B], entry0, nw if n is None else n, first, count)


def _feed_and_run(b, bits):
    b.set_inputs_rows(pack_rows(bits, (bits.shape[1] + 7) // 8, True))
    b.run(); b.check_r1cs(); b.sync()
    assert (b.status() == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [15, 43])
@pytest.mark.parametrize("engine", ["interp", "jit"])
def test_gpu_bitplane_rows_at_the_tile_edges(circuits, hip, monkeypatch, engine, n):
    monkeypatch.setenv("CW_BITS_JIT", "1" if engine == "jit" else "0")
    fc, c = circuits("bg%d" % n)
    bits, want = _case(n)
    B = 300
    b = c.batch(B)
    assert b.bitmode and b.jit == (engine == "jit") and b.bits_sh == (5 if engine == "jit" else 0) and c.n_witness > 129
    _feed_and_run(b, bits[:B])
    ones, bad = is_one(want), not_bool(want)
    assert not bad.any() and ones.any() and not ones.all()
    _matrix(hip, b, ones, bad, RANGES, B)
    b.close()


@pytest.mark.gpu
def test_gpu_state_and_empty_ranges(circuits, hip):
    """the state comes last; n == 0 and count == 0 write no row and set the word"""
    from circom_amd import runtime as rt
    L = rt.lib()
    fc, c = circuits("bg15")
    bits, want = _case(15)
    B, nw = 65, c.n_witness
    w8 = 8 * ((nw + 63) // 64)
    b = c.batch(B)
    p = hip.at_end(B * w8)
    with pytest.raises(rt.CwError) as e:
        b.witness_rows(0, nw)
    assert e.value.code == CW_ESTATE and "cw_get_witness_rows before cw_run" in str(e.value)
    with pytest.raises(rt.CwError) as e:
        b.witness_rows_device(0, nw, 0, B, p, w8)
    assert e.value.code == CW_ESTATE and "cw_get_witness_rows_device before cw_run" in str(e.value)
    assert L.cw_get_witness_rows_device(b.h, 0, nw + 1, 0, B, C.c_void_p(p), w8 + 8, 0, None) == CW_EINVAL     # the argument first
    _feed_and_run(b, bits[:B])
    for entry0, n, first, count in ((3, 0, 0, B), (nw, 0, 0, B), (0, nw, 7, 0), (0, nw, B, 0), (0, 0, 0, 0)):
        rows, word = np.full((B, w8), 0xA5, dtype=np.uint8), C.c_uint32(0x12345678)
        assert L.cw_get_witness_rows(b.h, entry0, n, first, count, rows.ctypes.data_as(C.c_void_p), w8, MSB, C.byref(word)) == 0
        assert (rows == 0xA5).all() and word.value == NONE
        rows, word = hip.rows_device(b, entry0, n, first, count, w8, True, p=hip.at_end(B * w8))
        assert word == NONE and (hip.download(hip.base + hip.SIZE - B * w8, B * w8) == 0xA5).all()
    got, word = b.witness_rows(0, 0)
    assert got.shape == (B, 0) and word == NONE
    got, word = b.witness_rows(0, nw, 7, 0)
    assert got.shape == (0, (nw + 7) // 8) and word == NONE
    # the Python forms
    ones = is_one(want)
    got, word = b.witness_rows(1, 17, 3, 40, msb_first=False)
    assert (got == model(ones, 1, 17, 3, 40, False)).all() and word == NONE
    got, word = b.public_rows()
    assert c.n_public == 17 and (got == model(ones, 1, 17, 0, B, True)).all() and word == NONE
    b.close()


@functools.lru_cache(maxsize=None)
def _sha_case():
    """(messages [130][8], is-one rows of the instances 0, 64 and 129 of Sha256(64) from eval_flat)"""
    fc = flatten(Program(Sha256(64)))
    msgs = np.random.default_rng(2048).integers(0, 256, size=(130, 8), dtype=np.uint8)
    ones = {}
    for i in (0, 64, 129):
        inp = np.unpackbits(msgs[i])
        sig, failed = eval_flat(fc.fp.q, fc.n_signals, fc.n_temps, fc.constants, fc.code,
                                {fc.main_input_start + k: int(v) for k, v in enumerate(inp)})
        assert failed is None
        ones[i] = np.array([1 if v == 1 else 0 for v in sig], dtype=np.uint8)
    return msgs, ones


@pytest.mark.gpu
def test_gpu_sha256_whole_witness_and_digests(circuits, hip):
    """more than one word tile: Sha256(64) x 130, the whole witness as rows; the first 32 bytes of the public rows ARE the digest"""
    fc, c = circuits("sha64")
    msgs, ones = _sha_case()
    B, nw = 130, c.n_witness
    assert nw > 8192                                              # at least three word tiles of 4 096 entries
    b = c.batch(B)
    assert b.bitmode and c.n_inputs == 64 and c.n_public >= 256
    b.set_inputs_rows(msgs, msb_first=True)
    b.run(); b.check_r1cs(); b.sync()
    assert (b.status() == 0).all()
    for msb in (True, False):
        got, word = b.witness_rows(0, nw, msb_first=msb)
        assert got.shape == (B, (nw + 7) // 8) and word == NONE
        for i in (0, 64, 129):
            assert (got[i] == np.packbits(ones[i], bitorder="big" if msb else "little")).all(), (msb, i)
    w8 = 8 * ((nw + 63) // 64)
    rows, word = hip.rows_device(b, 0, nw, 0, B, w8, True)
    for i in (0, 64, 129):
        want = np.packbits(ones[i])
        assert (rows[i, :len(want)] == want).all() and not rows[i, len(want):].any(), i
    pub, word = b.public_rows(msb_first=True)
    assert pub.shape == (B, (c.n_public + 7) // 8) and word == NONE
    for i in range(B):
        assert pub[i, :32].tobytes() == hashlib.sha256(msgs[i].tobytes()).digest(), i
    b.close()


@pytest.mark.gpu
def test_gpu_rows_beyond_65535_tiles_of_the_grid(circuits, hip):
    """BitAssert (a === b, out = a b) x 70 001, device rows of one word: the instance tiles are the grid's x dimension.  Where
    a != b the assertion fails and the row comes from the side batch: its values are bits, nothing is reported"""
    fc, c = circuits("bassert")
    B, nw = 70001, c.n_witness
    assert nw == 4 and c.n_public == 1
    a = np.random.default_rng(70001).integers(0, 2, size=(B, 1), dtype=np.uint8).repeat(2, axis=1)
    for i, v in ((0, 1), (65535, 1), (65536, 0), (70000, 1)):
        a[i] = v
    odd = np.arange(500, B, 997)                                  # a != b: the assertion fails there
    a[odd, 1] ^= 1
    assert len(odd) == 70
    b = c.batch(B)
    assert b.bitmode
    b.set_inputs_rows(pack_rows(a, 1, False), msb_first=False)
    b.run(); b.sync()
    st = b.status()
    assert ((st & 1) == (a[:, 0] != a[:, 1])).all()
    for msb in (True, False):
        rows, word = hip.rows_device(b, 0, nw, 0, B, 8, msb)
        entry = lambda k: (rows[:, 0] >> ((7 - k) if msb else k)) & 1
        assert word == NONE
        assert (entry(0) == 1).all() and (entry(1) == (a[:, 0] & a[:, 1])).all()
        assert (entry(2) == a[:, 0]).all() and (entry(3) == a[:, 1]).all()
        assert not (rows[:, 0] & (0x0F if msb else 0xF0)).any() and not rows[:, 1:].any()
    rows, word = hip.rows_device(b, 1, 1, 65530, 4471, 8, True)
    assert word == NONE and (rows[:, 0] == (a[65530:, 0] & a[65530:, 1]) << 7).all()
    b.close()


@functools.lru_cache(maxsize=None)
def _rerun_case():
    """BitGadget(15) x 130 where the instances 5, 64 and 129 have the input `which` equal to 7: (which, inputs [130][45] as
    integers, signals [130][n_signals][32] from eval_flat)"""
    fc = flatten(Program(BitGadget(15)))
    bits, want = _case(15)
    vals = bits[:130].astype(np.int64)
    out = want[:130].copy()
    which = 5                                                     # a[5] = 7 trips no check of the witness code: the oracle's signals are the witness
    for i in (5, 64, 129):
        vals[i, which] = 7
        sig, failed = eval_flat(fc.fp.q, fc.n_signals, fc.n_temps, fc.constants, fc.code,
                                {fc.main_input_start + k: int(v) for k, v in enumerate(vals[i])})
        assert failed is None
        out[i] = np.frombuffer(b"".join(v.to_bytes(32, "little") for v in sig), dtype=np.uint8).reshape(-1, 32)
    return fc.main_input_start + which, vals, out


@pytest.mark.gpu
@pytest.mark.parametrize("engine", ["interp", "jit"])
def test_gpu_rerun_instances_come_from_the_side_batch(circuits, hip, monkeypatch, engine):
    monkeypatch.setenv("CW_BITS_JIT", "1" if engine == "jit" else "0")
    fc, c = circuits("bg15")
    entry7, vals, want = _rerun_case()
    B, nw = 130, c.n_witness
    image = np.zeros((B, c.n_inputs, 32), dtype=np.uint8)
    image[:, :, 0] = vals
    b = c.batch(B)
    assert b.bitmode
    b.set_inputs(image)
    b.run(); b.sync()
    ones, bad = is_one(want), not_bool(want)
    odd = [5, 64, 129]
    assert bad[odd, entry7].all() and not np.delete(bad, odd, axis=0).any() and (ones[odd, entry7] == 0).all()
    # the whole witness: the word is 5, the input's bit is 0, every row is the oracle's
    _check_range(hip, b, ones, bad, 0, nw, 0, B)
    rows, word = b.witness_rows(0, nw, msb_first=False)
    assert word == 5 and not ((rows[odd, entry7 >> 3] >> (entry7 & 7)) & 1).any()
    # a range in which the three instances hold only 0 / 1: nothing is reported, the rows still come from the side batch
    clean = ~bad[odd].any(axis=0)
    clean[entry7] = False
    runs = [(k, int(np.argmin(np.append(clean[k:], False)))) for k in range(nw) if clean[k] and (k == 0 or not clean[k - 1])]
    entry0, n = max(runs, key=lambda r: r[1])
    assert n >= 9 and not (entry0 <= entry7 < entry0 + n)
    assert model_word(bad, entry0, n, 0, B) == NONE
    _check_range(hip, b, ones, bad, entry0, n, 0, B)
    _check_range(hip, b, ones, bad, entry0 + 1, n - 2, 3, 126)
    # the lowest instance WITHIN the range
    assert model_word(bad, 0, nw, 6, 124) == 64
    _check_range(hip, b, ones, bad, 0, nw, 6, 124)
    assert model_word(bad, 0, nw, 65, 65) == 129 and model_word(bad, 0, nw, 65, 64) == NONE
    _check_range(hip, b, ones, bad, 0, nw, 65, 65)
    _check_range(hip, b, ones, bad, 0, nw, 65, 64)
    b.close()


def _value_engine(circuits, monkeypatch, kind, B):
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
    return c, b, bits[:B], want[:B]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,B", [("gl", 65), ("gl", 300), ("wide", 65)])
def test_gpu_rows_of_the_value_engines(circuits, hip, monkeypatch, kind, B):
    c, b, bits, want = _value_engine(circuits, monkeypatch, kind, B)
    _feed_and_run(b, bits)
    ones, bad = is_one(want), not_bool(want)
    assert not bad.any()
    _matrix(hip, b, ones, bad, FOUR_RANGES, B)
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["m2", "m2mont"])
def test_gpu_values_that_are_not_bits_are_reported(circuits, hip, name):
    """Multiplier2 on (1, 1), (3, 11), (0, 5): out = 1, 33, 0 - bits 1, 0, 0, and instance 1 is reported.  The witness is
    [1, out, a, b]: on a Montgomery-form table 1 is R mod q, and nothing is converted"""
    fc, c = circuits(name)
    if name == "m2mont":
        assert c.montgomery
    assert c.n_witness == 4
    inputs = [(1, 1), (3, 11), (0, 5)]
    b = c.batch(3)
    assert not b.bitmode and c.element_bytes == 32
    image = np.zeros((3, 2, 32), dtype=np.uint8)
    image[:, :, 0] = inputs
    b.set_inputs(image)
    b.run(); b.sync()
    assert (b.status() == 0).all()
    values = np.zeros((3, 4, 32), dtype=np.uint8)
    values[:, :, 0] = [[1, x * y, x, y] for x, y in inputs]
    ones, bad = is_one(values), not_bool(values)
    assert ones[:, 1].tolist() == [1, 0, 0] and model_word(bad, 1, 1, 0, 3) == 1
    for entry0, n, first, count in ((1, 1, 0, 3), (0, 4, 0, 3), (1, 1, 0, 1), (1, 1, 2, 1), (2, 2, 2, 1), (2, 1, 0, 3), (0, 1, 0, 3)):
        _check_range(hip, b, ones, bad, entry0, n, first, count)
    got, word = b.witness_rows(1, 1)
    assert got[:, 0].tolist() == [0x80, 0, 0] and word == 1
    assert b.witness_rows(2, 2, 2, 1)[1] == 2 and b.witness_rows(0, 1)[1] == NONE
    b.close()


@pytest.mark.gpu
def test_gpu_supplied_witnesses_leave_as_rows(circuits, hip):
    """64-bit runtime in the supplied-witness state: the rows are the packed supplied image, read through the witness list"""
    fc, c = circuits("gl15")
    B, nw = 65, c.n_witness
    vals = np.random.default_rng(15).integers(0, 2, size=(B, nw), dtype=np.uint64)
    vals[:, 0] = 1
    vals[40, 9] = 5
    vals[64, 200] = c.q - 1
    b = c.batch(B)
    b.set_witnesses(vals)
    image = np.zeros((B, nw, 32), dtype=np.uint8)
    image[:, :, :8] = vals.view(np.uint8).reshape(B, nw, 8)
    ones, bad = is_one(image), not_bool(image)
    assert model_word(bad, 0, nw, 0, B) == 40 and model_word(bad, 10, nw - 10, 0, B) == 64
    for entry0, n in ((0, nw), (10, nw - 10), (1, 7), (10, 150)):
        for first, count in ((0, B), (41, 24), (63, 2)):
            _check_range(hip, b, ones, bad, entry0, n, first, count)
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["bits", "gl"])
def test_gpu_the_rows_are_complete_in_stream_order(circuits, hip, monkeypatch, kind):
    """the device form, then a device-to-device copy on the batch's stream, no synchronisation between them: the copy holds
    complete rows.  A second call with another range into the same buffer overwrites only its own words"""
    B = 65
    if kind == "bits":
        fc, c = circuits("bg15")
        (bits, want), b = _case(15), c.batch(B)
    else:
        c, b, bits, want = _value_engine(circuits, monkeypatch, kind, B)
    _feed_and_run(b, bits[:B])
    ones = is_one(want[:B])
    stride, nbytes = 24, B * 24
    p = hip.at_end(nbytes)
    copy = hip.alloc(nbytes)
    b.witness_rows(0, 1)                                          # (a bit-plane batch: the first egress after a run has waited)
    b.witness_rows_device(0, 129, 0, B, p, stride, msb_first=True)
    assert hip.h.hipMemcpyAsync(copy, p, nbytes, 3, None) == 0     # the batch's stream is the null stream
    got = hip.download(copy, (B, stride))
    first = np.zeros((B, stride), dtype=np.uint8)
    first[:, :17] = model(ones, 0, 129, 0, B, True)
    assert (got == first).all()
    b.witness_rows_device(5, 9, 0, B, p, stride, msb_first=False)
    assert hip.h.hipMemcpyAsync(copy, p, nbytes, 3, None) == 0
    got = hip.download(copy, (B, stride))
    second = first.copy()
    second[:, :8] = 0
    second[:, :2] = model(ones, 5, 9, 0, B, False)
    assert (got == second).all() and (second[:, 8:] == first[:, 8:]).all() and (second[:, :8] != first[:, :8]).any()
    hip.h.hipFree(copy)
    b.close()
