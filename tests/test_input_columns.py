"""Input columns: cw_set_inputs_range(_device), cw_set_input_column(_device), cw_inputs_missing (include/circom_amd.h) - one named
signal, or a range of main inputs, for the WHOLE batch: instance j's n little-endian values of 1, 2, 4, 8 or 32 bytes at
values + j * stride, stride 0 = the same n values for every instance.  The values go into the batch's own bulk image
(csrc/cw_columns.hip.h cw_columns_kernel), which cw_run ingests with the kernels it has.

Expected values never come from the library: they come from the circuit's flat code evaluated by oracle.tape_eval.eval_flat on
the assembled inputs, or (the equivalence tests) from a batch that took the same values through cw_set_inputs(_n8).

The circuit: Cols, inputs s, v[5], m[70] (76 main inputs, m crosses one 64-lane wave), out[0] = the sum of every input times its
own weight, out[1] = out[0] * s: two swapped values or a shifted column change the witness.  bn128 with canonical and with
Montgomery-form tables, and Goldilocks (the 64-bit runtime: an image of 8-byte values, reduction on the device).  BitGadget(15)
serves the bit-plane engine, interpreted and emitted.  Batches of 1, 63, 64, 65 and 300 instances: with 152 (76) pieces of 16
(8) bytes per instance a wave holds parts of up to two (three) instances, and the last workgroup is partly empty."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
from test_bitplane import BitGadget, _Hip                                            # noqa: E402

from circom_amd.circuits.basic import Multiplier2                                    # noqa: E402
from circom_amd.compiler import compile_program                                      # noqa: E402
from circom_amd.frontend.dsl import Program, template                                # noqa: E402
from circom_amd.frontend.flatten import flatten                                      # noqa: E402
from oracle.tape_eval import check_r1cs, eval_flat                                   # noqa: E402

CW_EINVAL, CW_EINPUT, CW_EDEVICE, CW_ESTATE = -2, -3, -4, -5
WIDTHS = (1, 2, 4, 8, 32)
B_MAX = 300
GL_P = 0xFFFFFFFF00000001
# the columns of Cols in the scrambled order the tests set them in: (name, idx0, n, k0)
COLS = (("m", 35, 35, 41), ("s", 0, 1, 0), ("v", 0, 5, 1), ("m", 0, 35, 6))


@template
def Cols(c):
    s = c.input("s")
    v = c.input("v", 5)
    m = c.input("m", 70)
    out = c.output("out", 2)
    acc = s * 3
    for k in range(5):
        acc = acc + v[k] * (5 + k)
    for k in range(70):
        acc = acc + m[k] * (101 + k)
    c.set(out[0], acc)
    c.set(out[1], out[0] * s)


@template
def SquarePlusOne(c):
    x = c.input("x")
    out = c.output("out")
    c.set(out, x * x + 1)


def _prog(kind):
    if kind == "gl":
        return Program(Cols(), prime="goldilocks")
    if kind == "bg15":
        return Program(BitGadget(15))
    return Program(Cols())


# ---- values and their images -------------------------------------------------------------------------------------------------------
def _ints(vals):
    """[B][n][W] little-endian bytes -> [B][n] Python integers"""
    B, n, W = vals.shape
    return [[int.from_bytes(vals[j, k].tobytes(), "little") for k in range(n)] for j in range(B)]


@functools.lru_cache(maxsize=None)
def _values(kind, W):
    """[300][76][W] bytes: random values of W bytes; instance 0 holds the largest value the width (and, for 32-byte values of
    bn128, the rule "canonical") allows, instance 1 zeros.  Goldilocks takes any bytes: the device reduces."""
    rng = np.random.default_rng(1000 * WIDTHS.index(W) + len(kind))
    vals = rng.integers(0, 256, size=(B_MAX, 76, W), dtype=np.uint8)
    vals[0] = 0xFF
    vals[1] = 0
    if W == 32 and kind != "gl":
        vals[:, :, 31] &= 0x1F                                    # < 2^253 < q
        q = flatten(_prog(kind)).fp.q
        vals[0] = np.frombuffer((q - 1).to_bytes(32, "little"), dtype=np.uint8)
    vals.setflags(write=False)
    return vals


def _oracle_of(fc, rows, clean=True):
    """[B][n_signals][32] canonical little-endian signals of eval_flat on each row of integers (taken mod q); with `clean` no
    instance may fail and the first and the last satisfy the constraint system"""
    q = fc.fp.q
    out = np.zeros((len(rows), fc.n_signals, 32), dtype=np.uint8)
    for i, row in enumerate(rows):
        sig, failed = eval_flat(q, fc.n_signals, fc.n_temps, fc.constants, fc.code,
                                {fc.main_input_start + k: int(v) % q for k, v in enumerate(row)})
        if clean:
            assert failed is None
            if i in (0, len(rows) - 1):
                assert check_r1cs(q, fc.constraints, sig) is None
        out[i] = np.frombuffer(b"".join(v.to_bytes(32, "little") for v in sig), dtype=np.uint8).reshape(-1, 32)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _case(kind, W):
    """(values [300][76][W], expected signals [300][n_signals][32]): computed once, shared, never modified; a batch of B
    instances takes the first B"""
    vals = _values(kind, W)
    return vals, _oracle_of(flatten(_prog(kind)), _ints(vals))


def _image(vals, pad):
    """(bytes, stride): rows of n * W + pad bytes, pad bytes 0xA5; the last row ENDS with its values"""
    B, n, W = vals.shape
    stride = n * W + pad
    buf = np.full((B, stride), 0xA5, dtype=np.uint8)
    buf[:, :n * W] = vals.reshape(B, n * W)
    return np.ascontiguousarray(buf.reshape(-1)[:(B - 1) * stride + n * W]), stride


def _pad(W):
    return 16 if W == 32 else 3 * W                               # device strides stay multiples of W (16 for 32-byte values)


# ---- without a GPU ---------------------------------------------------------------------------------------------------------------
def test_the_library_exports_the_column_calls():
    from circom_amd import runtime as rt
    L = rt.lib()
    for name in ("cw_set_inputs_range", "cw_set_inputs_range_device", "cw_set_input_column", "cw_set_input_column_device", "cw_inputs_missing"):
        assert hasattr(L, name), name
    for name in ("set_input_column", "set_input_column_device", "set_inputs_range", "set_inputs_range_device", "inputs_missing"):
        assert hasattr(rt.Batch, name), name


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
def test_host_only_staging(tmp_path, kind):
    """every width, a padded stride whose pad bytes are 0xA5, the broadcast form, every staged cell, the count after each call,
    a column written twice; the values are staged zero-extended and unreduced"""
    from circom_amd import runtime as rt
    L = rt.lib()
    c = _host_circuit(tmp_path, kind)
    names = (("a", 1), ("b", 1)) if kind != "bg15" else (("a", 15), ("b", 15), ("d", 15))
    n_in, B = c.n_inputs, 5
    assert n_in == sum(n for _, n in names)
    rng = np.random.default_rng(7)
    for W in WIDTHS:
        b = c.batch(B, device=-1)
        assert b.inputs_missing() == -1
        want = {}
        left = n_in
        k0 = 0
        for t, (name, n) in enumerate(names):
            vals = rng.integers(0, 256, size=(B, n, W), dtype=np.uint8)
            vals[0] = 0xFF                                        # 2^(8 W) - 1: staged as it stands, whatever the prime
            if t == 1:                                            # the broadcast form: one row for every instance
                img, stride = np.ascontiguousarray(vals[2].reshape(-1)), 0
                vals = np.repeat(vals[2:3], B, axis=0)
            else:
                img, stride = _image(vals, 5)
            assert L.cw_set_input_column(b.h, name.encode(), 0, n, img.ctypes.data_as(C.c_void_p), stride, W) == 0, L.cw_last_error()
            left -= n
            for j in range(B):
                assert b.remaining_inputs(j) == left
                for k in range(n):
                    want[j, k0 + k] = int.from_bytes(vals[j, k].tobytes(), "little")
            k0 += n
        assert b.inputs_missing() == -1                          # no column state on a host-only batch
        for (j, k), v in want.items():
            assert b.staged_input(j, k) == v, (W, j, k)
        # a column again, through the range form and the Python wrapper: overwritten, nothing newly assigned
        again = rng.integers(0, 256, size=(B, names[0][1], W), dtype=np.uint8)
        arr = again if W == 32 else again.reshape(B, -1).view("<u%d" % W) if W > 1 else again[:, :, 0]
        b.set_inputs_range(0, arr)
        for j in range(B):
            assert b.remaining_inputs(j) == 0
            for k in range(names[0][1]):
                assert b.staged_input(j, k) == int.from_bytes(again[j, k].tobytes(), "little")
            assert b.staged_input(j, names[0][1]) == want[j, names[0][1]]
        b.close()
    # part of a signal: only those cells count
    if kind == "bg15":
        b = c.batch(B, device=-1)
        b.set_input_column("b", np.ones((B, 4), dtype=np.uint8), idx0=11)
        assert [b.remaining_inputs(j) for j in range(B)] == [n_in - 4] * B
        assert b.staged_input(B - 1, 15 + 11) == 1 and b.staged_input(0, 15 + 14) == 1
        with pytest.raises(rt.CwError):
            b.staged_input(0, 15 + 10)
        b.set_input_column("b", np.array([1, 0, 1], dtype=np.uint16), idx0=10)          # 1-D: broadcast; one new cell per instance
        assert [b.remaining_inputs(j) for j in range(B)] == [n_in - 5] * B
        assert [b.staged_input(3, 15 + k) for k in (10, 11, 12, 13)] == [1, 0, 1, 1]
        b.close()
    c.close()


@pytest.mark.parametrize("kind", ["m2", "bg15"])
def test_every_check_in_its_order(tmp_path, kind):
    """null / elem_bytes / stride / alignment (CW_EINVAL, the pointer never touched), then the name and the range (CW_EINPUT with
    the texts of cw_set_input_signal; the range forms CW_EINVAL), then the device (a host-only batch: CW_EDEVICE)"""
    from circom_amd import runtime as rt
    L = rt.lib()
    c = _host_circuit(tmp_path, kind)
    n_in = c.n_inputs
    size = 1 if kind == "m2" else 15                              # of signal "a"
    b = c.batch(3, device=-1)
    host = np.zeros(3 * 64 * 32, dtype=np.uint8)
    hp = host.ctypes.data_as(C.c_void_p)
    err = lambda: L.cw_last_error().decode()
    col = lambda fn, name, idx0, n, ptr, stride, eb: fn(b.h, name, idx0, n, ptr, stride, eb)
    rng_ = lambda fn, k0, n, ptr, stride, eb: fn(b.h, k0, n, ptr, stride, eb)
    for fn, ok_ptr in ((L.cw_set_input_column, hp), (L.cw_set_input_column_device, C.c_void_p(4096))):
        dev = fn is L.cw_set_input_column_device
        assert fn(None, b"a", 0, 1, ok_ptr, 0, 1) == CW_EINVAL
        assert col(fn, None, 0, 1, ok_ptr, 0, 1) == CW_EINVAL
        assert col(fn, b"a", 0, 1, None, 0, 1) == CW_EINVAL and "null" in err()
        for eb in (0, 3, 16, 64):
            assert col(fn, b"nobody", 0, 1, ok_ptr, 0, eb) == CW_EINVAL and "elem_bytes" in err()      # before the name
        assert col(fn, b"nobody", 0, 2, ok_ptr, 8, 8) == CW_EINVAL and "stride" in err()
        if dev:
            assert col(fn, b"nobody", 0, 1, C.c_void_p(4096 + 4), 32, 32) == CW_EINVAL and "16-byte aligned" in err()
            assert col(fn, b"nobody", 0, 1, C.c_void_p(4096 + 16), 32 + 8, 32) == CW_EINVAL and "multiple of 16" in err()
            assert col(fn, b"nobody", 0, 1, C.c_void_p(4096 + 4), 8, 8) == CW_EINVAL and "aligned" in err()
            assert col(fn, b"nobody", 0, 1, C.c_void_p(4096), 12, 8) == CW_EINVAL and "multiple" in err()
            assert col(fn, b"nobody", 0, 1, C.c_void_p(4096 + 2), 0, 4) == CW_EINVAL                  # broadcast: the pointer still counts
        assert col(fn, b"nobody", 0, 1, ok_ptr, 0, 1) == CW_EINPUT and err() == "Signal not found: nobody"
        assert col(fn, b"a", size, 1, ok_ptr, 0, 1) == CW_EINPUT and err() == "Input signal array access exceeds the size"
        assert col(fn, b"a", 1, size, ok_ptr, 0, 1) == CW_EINPUT and err() == "Input signal array access exceeds the size"
        assert col(fn, b"a", 0xFFFFFFFF, 2, ok_ptr, 0, 1) == CW_EINPUT                                # no 32-bit wrap
        if dev:
            assert col(fn, b"a", 0, size, ok_ptr, 32 * size + 16, 32) == CW_EDEVICE and "host-only" in err()
            assert col(fn, b"a", 0, size, C.c_void_p(4096 + 16), 0, 32) == CW_EDEVICE
            assert col(fn, b"a", 0, 0, ok_ptr, 0, 1) == CW_EDEVICE                                     # the device comes before "nothing to do"
        else:
            assert col(fn, b"a", 0, size, C.c_void_p(host.ctypes.data + 1), 32 * size + 3, 32) == 0     # any alignment
            assert col(fn, b"a", 0, 0, ok_ptr, 0, 1) == 0 and col(fn, b"a", size, 0, ok_ptr, 0, 8) == 0
    for fn, ok_ptr in ((L.cw_set_inputs_range, hp), (L.cw_set_inputs_range_device, C.c_void_p(4096))):
        dev = fn is L.cw_set_inputs_range_device
        assert fn(None, 0, 1, ok_ptr, 0, 1) == CW_EINVAL
        assert rng_(fn, 0, 1, None, 0, 1) == CW_EINVAL
        assert rng_(fn, n_in, 1, ok_ptr, 0, 5) == CW_EINVAL and "elem_bytes" in err()                   # before the range
        assert rng_(fn, n_in, 2, ok_ptr, 7, 4) == CW_EINVAL and "stride" in err()
        if dev:
            assert rng_(fn, n_in, 1, C.c_void_p(4096 + 4), 32, 32) == CW_EINVAL and "16-byte aligned" in err()
        assert rng_(fn, n_in, 1, ok_ptr, 0, 1) == CW_EINVAL and "range" in err()
        assert rng_(fn, 1, n_in, ok_ptr, 0, 1) == CW_EINVAL and rng_(fn, 0xFFFFFFFF, 2, ok_ptr, 0, 1) == CW_EINVAL
        assert rng_(fn, 0, n_in, ok_ptr, 0, 2) == (CW_EDEVICE if dev else 0)
        assert rng_(fn, n_in, 0, ok_ptr, 0, 2) == (CW_EDEVICE if dev else 0)
    assert L.cw_inputs_missing(None) == -1
    # the Python wrapper: widths from the dtype
    with pytest.raises(AssertionError):
        b.set_input_column("a", np.zeros((3, size), dtype=np.int32))
    with pytest.raises(AssertionError):
        b.set_input_column("a", np.zeros((2, size), dtype=np.uint8))                                    # not the batch's rows
    with pytest.raises(rt.CwError) as e:
        b.set_input_column("a", np.zeros((3, size + 1, 32), dtype=np.uint8))
    assert e.value.code == CW_EINPUT
    b.close(); c.close()


# ---- GPU -------------------------------------------------------------------------------------------------------------------------
class _Dev(_Hip):
    """column images on the device: the image ENDS where its allocation ends, behind a 4 096-byte guard of 0xA5 in front"""

    def at_end(self, img):
        whole = np.concatenate([np.full(4096, 0xA5, dtype=np.uint8), img])
        base = self.alloc(whole.nbytes)
        assert self.h.hipMemcpy(base, whole.ctypes.data, whole.nbytes, 1) == 0
        return base, base + 4096

    def fill(self, p, n, byte):
        junk = np.full(n, byte, dtype=np.uint8)
        assert self.h.hipMemcpy(p, junk.ctypes.data, n, 1) == 0


@pytest.fixture(scope="module")
def hip():
    return _Dev()


@pytest.fixture(scope="module")
def circuits(tmp_path_factory):
    """every circuit of this module, compiled once: name -> (flat circuit, runtime circuit); the witness is every signal"""
    from circom_amd import runtime as rt
    made = {}

    def get(name):
        if name not in made:
            d = str(tmp_path_factory.mktemp(name))
            if name == "canon":
                cp = compile_program(_prog(name), d, name, sym=False, mont=False)
            elif name == "mont":
                cp = compile_program(_prog(name), d, name, sym=False, mont=True)
            elif name == "gl":
                cp = compile_program(_prog(name), d, name, sym=False)
            elif name == "one":
                cp = compile_program(Program(SquarePlusOne(), prime="goldilocks"), d, name, sym=False)
            else:
                cp = compile_program(_prog("bg15"), d, name, sym=False, strands=(1,), bits=True, jit=True)
                assert cp.jit is not None
            c = rt.Circuit(cp.tape_path, cp.dat_path, cp.r1cs_path)
            c.set_witness_list(np.arange(c.n_signals, dtype=np.uint32))
            assert c.n_witness == cp.flat.n_signals
            if name in ("canon", "mont"):
                assert c.montgomery == (name == "mont") and c.element_bytes == 32
            if name == "gl":
                assert c.element_bytes == 8
            made[name] = (cp.flat, c)
        return made[name]

    yield get
    for _, c in made.values():
        c.close()


def _set_columns(hip, b, vals, form, cols=COLS, frees=None):
    """the columns of Cols from `vals` [B][76][W], in the scrambled order; device images with padded strides at the end of their
    allocations (freed by the caller through `frees`), host images with 5 pad bytes of 0xA5"""
    from circom_amd import runtime as rt
    L = rt.lib()
    W = vals.shape[2]
    for name, idx0, n, k0 in cols:
        part = vals[:, k0:k0 + n]
        if form == "host":
            img, stride = _image(part, 5)
            assert L.cw_set_input_column(b.h, name.encode(), idx0, n, img.ctypes.data_as(C.c_void_p), stride, W) == 0, L.cw_last_error()
        else:
            img, stride = _image(part, _pad(W))
            base, p = hip.at_end(img)
            b.set_input_column_device(name, p, n, stride, W, idx0=idx0)
            frees.append(base)


def _compare(b, want, clean=True):
    b.run(); b.check_r1cs(); b.sync()
    if clean:
        st = b.status()
        assert (st == 0).all(), st[st != 0][:8]                  # no run-time check fired and the R1CS check is clean
    got = b.witnesses()
    bad = np.argwhere((got != want).any(axis=2))
    assert len(bad) == 0, "first differences at (instance, signal): %s" % bad[:8].tolist()
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("B", [1, 63, 64, 65, 300])
@pytest.mark.parametrize("kind", ["canon", "mont", "gl"])
def test_gpu_columns_at_the_tile_edges(circuits, hip, kind, B, form):
    fc, c = circuits(kind)
    assert c.n_inputs == 76 and c.input_size("m") == (fc.main_input_start + 6, 70)
    for W in WIDTHS:
        vals, want = _case(kind, W)
        b = c.batch(B)
        assert not b.bitmode and b.inputs_missing() == -1
        frees = []
        _set_columns(hip, b, vals[:B], form, frees=frees)
        assert b.inputs_missing() == 0
        _compare(b, want[:B])
        b.close()
        for base in frees:
            hip.h.hipFree(base)


def _bulk(b, kind, vals, q):
    """the same values through the bulk forms: the 64-bit runtime takes values of up to 8 bytes through cw_set_inputs_n8 (and
    reduces them as the columns do), everything else the 32-byte image - canonical for bn128, as it stands for Goldilocks"""
    B, n, W = vals.shape
    if kind == "gl" and W <= 8:
        wide = np.zeros((B, n, 8), dtype=np.uint8)
        wide[:, :, :W] = vals
        b.set_inputs_n8(wide.reshape(B, n * 8).view("<u8"))
    else:
        wide = np.zeros((B, n, 32), dtype=np.uint8)
        wide[:, :, :W] = vals
        b.set_inputs(wide)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["canon", "mont", "gl"])
def test_gpu_columns_equal_the_bulk_forms_byte_for_byte(circuits, hip, kind):
    fc, c = circuits(kind)
    B = 65
    for W in WIDTHS:
        vals, want = _case(kind, W)
        b = c.batch(B)
        _set_columns(hip, b, vals[:B], "host")
        got = _compare(b, want[:B])
        b2 = c.batch(B)
        _bulk(b2, kind, vals[:B], fc.fp.q)
        b2.run(); b2.check_r1cs(); b2.sync()
        assert b2.witnesses().tobytes() == got.tobytes(), W
        b.close(); b2.close()


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["host", "device"])
def test_gpu_goldilocks_values_are_reduced(circuits, hip, form):
    """8-byte values p, p + 1, 2^64 - 1 and 32-byte values with upper words set: what the _n8 / 32-byte bulk forms make of them,
    and what the oracle computes on the residues"""
    fc, c = circuits("gl")
    B = 65
    for W in (8, 32):
        vals = np.array(_values("gl", W)[:B])
        odd = [GL_P, GL_P + 1, 2**64 - 1, GL_P - 1, 0, 1]
        if W == 32:
            odd = odd + [2**64, 2**128 + 5, (2**192) * 7 + 2**64 - 1, 2**256 - 1, GL_P << 64, (GL_P + 1) << 128, (2**64 - 1) << 192]
        for t, x in enumerate(odd):                               # spread over instances, signals and both halves of m
            vals[(3 * t) % B, (7 * t) % 76] = np.frombuffer(x.to_bytes(W, "little"), dtype=np.uint8)
            vals[B - 1 - t, 75 - t] = np.frombuffer(x.to_bytes(W, "little"), dtype=np.uint8)
        want = _oracle_of(fc, _ints(vals))
        b = c.batch(B)
        frees = []
        _set_columns(hip, b, vals, form, frees=frees)
        got = _compare(b, want)
        b2 = c.batch(B)
        _bulk(b2, "gl", vals, fc.fp.q)
        b2.run(); b2.check_r1cs(); b2.sync()
        assert b2.witnesses().tobytes() == got.tobytes(), W
        b.close(); b2.close()
        for base in frees:
            hip.h.hipFree(base)


@functools.lru_cache(maxsize=None)
def _bit_case():
    """(bits [300][45], expected signals) of BitGadget(15), then the same with a[5] = 7 in three instances"""
    fc = flatten(_prog("bg15"))
    bits = np.random.default_rng(115).integers(0, 2, size=(B_MAX, 45), dtype=np.uint8)
    bits[0], bits[1] = 1, 0
    odd = bits.copy()
    odd[[0, 64, 299], 5] = 7
    bits.setflags(write=False); odd.setflags(write=False)
    return bits, _oracle_of(fc, bits.tolist()), odd, _oracle_of(fc, odd.tolist(), clean=False)


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 65, 300])
@pytest.mark.parametrize("engine", ["interp", "jit"])
def test_gpu_bitplane_columns(circuits, hip, monkeypatch, engine, B):
    """one-byte columns of 0 / 1 into a bit-plane batch; then a[5] = 7 in up to three instances, which the 256-bit schedule re-runs
    from the image the columns wrote: the witness is the oracle's (the status word is not looked at there)"""
    monkeypatch.setenv("CW_BITS_JIT", "1" if engine == "jit" else "0")
    fc, c = circuits("bits")
    bits, want, odd, want_odd = _bit_case()
    b = c.batch(B)
    assert b.bitmode and b.jit == (engine == "jit") and c.n_inputs == 45
    for name, k0 in (("d", 30), ("a", 0), ("b", 15)):
        b.set_input_column(name, bits[:B, k0:k0 + 15])
    assert b.inputs_missing() == 0
    _compare(b, want[:B])
    base, p = hip.at_end(_image(odd[:B, 0:15, None], 1)[0])      # the column `a` again, from the device this time
    b.set_input_column_device("a", p, 15, 16, 1)
    got = _compare(b, want_odd[:B], clean=False)
    assert (got[0] != want[0]).any()                              # the 7 made a difference
    st = b.status()
    plain = np.setdiff1d(np.arange(B), [0, 64, 299])
    assert (st[plain] == 0).all()
    hip.h.hipFree(base)
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["mont", "gl", "bits"])
def test_gpu_the_column_state(circuits, hip, kind):
    from circom_amd import runtime as rt
    fc, c = circuits(kind)
    B = 65
    if kind == "bits":
        bits, want_all = _bit_case()[:2]
        one, two = bits[:B, :, None], bits[100:100 + B, :, None]
        want1, want2 = want_all[:B], want_all[100:100 + B]
        cols = (("d", 0, 15, 30), ("a", 0, 15, 0), ("b", 0, 15, 15))
        upd = ("b", 0, 15, 15)
    else:
        vals, want_all = _case(kind, 4)
        one, two = vals[:B], vals[100:100 + B]
        want1, want2 = want_all[:B], want_all[100:100 + B]
        cols, upd = COLS, ("v", 0, 5, 1)
    n_in = c.n_inputs
    b = c.batch(B)
    assert b.inputs_missing() == -1 and b.remaining_inputs(B - 1) == n_in
    # the count falls call by call; a run with a column missing is refused with the count
    left = n_in
    for col in cols[:-1]:
        _set_columns(hip, b, one, "host", cols=(col,))
        left -= col[2]
        assert b.inputs_missing() == left and b.remaining_inputs(0) == left and b.remaining_inputs(B - 1) == left
    _set_columns(hip, b, one, "host", cols=(cols[0],))            # again: overwritten, nothing new
    assert b.inputs_missing() == left == cols[-1][2]
    with pytest.raises(rt.CwError) as e:
        b.run()
    assert e.value.code == CW_ESTATE and "Not all inputs have been set. %d values missing over the batch" % (left * B) in str(e.value)
    _set_columns(hip, b, one, "host", cols=(cols[-1],))
    assert b.inputs_missing() == 0 and b.remaining_inputs(3) == 0
    _compare(b, want1)
    assert b.inputs_missing() == 0                                # the state survives the run
    # ONE column updated: the others persisted
    mixed = np.array(one)
    mixed[:, upd[3]:upd[3] + upd[2]] = two[:, upd[3]:upd[3] + upd[2]]
    _set_columns(hip, b, mixed, "host", cols=(upd,))
    _compare(b, _oracle_of(fc, [[int.from_bytes(x.tobytes(), "little") for x in row] for row in mixed]))
    # the latest setter wins, both ways: the bulk form ends the column state ...
    wide = np.zeros((B, n_in, 32), dtype=np.uint8)
    wide[:, :, :two.shape[2]] = two
    b.set_inputs(wide)
    assert b.inputs_missing() == -1 and b.remaining_inputs(0) == 0
    _compare(b, want2)
    # ... and a column after it starts from empty coverage
    b.set_inputs(wide)
    _set_columns(hip, b, one, "host", cols=(upd,))
    assert b.inputs_missing() == n_in - upd[2]
    with pytest.raises(rt.CwError) as e:
        b.run()
    assert e.value.code == CW_ESTATE and "%d values missing" % ((n_in - upd[2]) * B) in str(e.value)
    _set_columns(hip, b, one, "host", cols=cols)
    b.set_inputs(wide)
    _compare(b, want2)
    _set_columns(hip, b, one, "host", cols=cols)
    _compare(b, want1)
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["mont", "gl"])
def test_gpu_run_check_replays_its_graph_over_an_updated_column(circuits, hip, kind):
    fc, c = circuits(kind)
    B = 65
    vals, want = _case(kind, 8)
    b = c.batch(B)
    _set_columns(hip, b, vals[:B], "host")
    for _ in range(2):
        b.run_check(); b.sync()
        assert (b.status() == 0).all() and (b.witnesses() == want[:B]).all()
    assert b.graph_captured
    mixed = np.array(vals[:B])
    mixed[:, 6:41] = vals[100:100 + B, 6:41]
    frees = []
    _set_columns(hip, b, mixed, "device", cols=(("m", 0, 35, 6),), frees=frees)
    b.run_check(); b.sync()
    assert b.graph_captured
    assert (b.status() == 0).all()
    assert (b.witnesses() == _oracle_of(fc, _ints(mixed))).all()
    hip.h.hipFree(frees[0])
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["canon", "gl", "bits"])
def test_gpu_the_device_values_are_free_once_the_stream_has_passed_the_call(circuits, hip, kind):
    fc, c = circuits(kind)
    B = 65
    if kind == "bits":
        bits, want = _bit_case()[:2]
        vals, cols = bits[:B, :, None], (("d", 0, 15, 30), ("a", 0, 15, 0), ("b", 0, 15, 15))
    else:
        (vals, want), cols = _case(kind, 32), COLS
    b = c.batch(B)
    frees = []
    _set_columns(hip, b, vals[:B], "device", cols=cols, frees=frees)
    b.sync()
    W = vals.shape[2]
    for base, (_, _, n, _) in zip(frees, cols):
        hip.fill(base + 4096, (B - 1) * (n * W + _pad(W)) + n * W, 0xA5)                # the values were taken inside the call
    _compare(b, want[:B])
    for base in frees:
        hip.h.hipFree(base)
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["mont", "gl"])
def test_gpu_broadcast_from_the_device(circuits, hip, kind):
    """stride 0: s and the first half of m are the same for all 300 instances (the values of instance 7); also from the host"""
    fc, c = circuits(kind)
    B = 300
    for W in (2, 32):
        vals = np.array(_values(kind, W))
        vals[:, 0] = vals[7, 0]
        vals[:, 6:41] = vals[7, 6:41]
        want = _oracle_of(fc, _ints(vals))
        b = c.batch(B)
        frees = []
        _set_columns(hip, b, vals, "device", cols=(COLS[0], COLS[2]), frees=frees)
        for name, idx0, n, k0 in (COLS[1], COLS[3]):
            base, p = hip.at_end(np.ascontiguousarray(vals[7, k0:k0 + n].reshape(-1)))
            b.set_input_column_device(name, p, n, 0, W, idx0=idx0)
            frees.append(base)
        _compare(b, want)
        arr = vals[7, 0:1] if W == 32 else np.ascontiguousarray(vals[7, 0:1].reshape(-1)).view("<u%d" % W)
        b.set_input_column("s", arr, elem_bytes=W)                # the Python wrapper: one dimension less is the broadcast form
        _compare(b, want)
        for base in frees:
            hip.h.hipFree(base)
        b.close()


@pytest.mark.gpu
def test_gpu_a_large_launch(circuits, hip):
    """4 194 305 instances of x -> x^2 + 1 on Goldilocks from a one-byte column: one more instance than 65 535 x 64 + 64 and than
    2^14 workgroups of 256 lanes hold"""
    fc, c = circuits("one")
    B = 4194305
    assert c.n_inputs == 1
    x = ((np.arange(B, dtype=np.uint64) * 7 + 3) & 0xFF).astype(np.uint8).reshape(B, 1)
    b = c.batch(B)
    for form in ("host", "device"):
        col = x if form == "host" else (255 - x)
        if form == "host":
            b.set_input_column("x", col)
        else:
            base, p = hip.at_end(np.ascontiguousarray(col.reshape(-1)))
            b.set_input_column_device("x", p, 1, 1, 1)
        b.run(); b.sync()
        for i in (0, 65535 * 64 - 1, 65535 * 64, 65535 * 64 + 1, B - 1):
            v = int(col[i, 0])
            sig, failed = eval_flat(fc.fp.q, fc.n_signals, fc.n_temps, fc.constants, fc.code, {fc.main_input_start: v})
            assert failed is None and v * v + 1 in sig
            assert b.witness(i) == sig, (form, i)
        if form == "device":
            hip.h.hipFree(base)
    b.close()
