"""Instance lists (include/circom_amd.h): cw_select_instances(_device) picks the instances whose status word satisfies
(status & mask) == want, ascending, on the device; cw_get_witnesses_at(_device)(_n8) hands out the witnesses of a LIST of
instances, out[j][k] = entry entry0 + k of instance idx[j].  Kernels: csrc/cw_kernels.hip cw_select_block_kernel /
cw_select_scan_kernel (count, scan, scatter - three launches) and cw_gather_many_kernel<MONT, true>, csrc/cw64.hip cw64_egress_kernel<EB, true>,
csrc/cw_bits.hip cw_bits_gather_kernel<true>.

Expected values come from oracle.tape_eval (eval_flat, its failed flag, check_r1cs), never from another call into the library;
agreement with np.flatnonzero((b.status() & mask) == want) is asserted as well.  The shapes: BitGadget(15) has 380 signals; the
entry ranges (0, whole), (1, 7), (3, 65), (15, 17) are the edges of the 64-entry and 16-entry tiles (a witness of four entries
clips them); batches of 65, 130 and 300 are one tile of 64 positions + 1, two + 2, four + 44; 2 049 instances are one count block
of the select kernels and a block of one instance, 2 097 153 the smallest batch with a second pass of the scan's loop.  Device outputs are written
into 0xA5 bytes that end at the end of an allocation.

The egress by index is the AT = true instantiation of each table's range kernel (cw64_egress_kernel<EB, false>,
cw_gather_many_kernel<MONT, false>, cw_bits_gather_kernel<false>), so a range and the list of its instances are compared byte for
byte as well, both with the oracle: (first, count) = (0, 300) whole tiles and a last one of 44, (37, 201) and (63, 2) off a group
boundary of the bit table (a shifted window that takes a second group, from both forms), (64, 64) exactly one tile, (299, 1) the
last instance; 4 194 241 instances are the smallest range of the 8 x u32 table that takes a second launch."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
from test_bitplane import BadBit, BitAssert, BitGadget, _Hip                         # noqa: E402,F401
from test_input_rows import _case, pack_rows                                         # noqa: E402
from test_output_rows import _Dev, _rerun_case                                       # noqa: E402

from circom_amd.circuits.basic import Multiplier2                                    # noqa: E402
from circom_amd.compiler import compile_program                                      # noqa: E402
from circom_amd.frontend.dsl import Program                                          # noqa: E402
from circom_amd.frontend.flatten import flatten                                      # noqa: E402
from oracle.tape_eval import check_r1cs, eval_flat                                   # noqa: E402

CW_EINVAL, CW_EDEVICE, CW_ESTATE = -2, -4, -5
NONE = 0xFFFFFFFF
A5 = 0xA5A5A5A5
SYMBOLS = ("cw_select_instances", "cw_select_instances_device", "cw_get_witnesses_at", "cw_get_witnesses_at_n8",
           "cw_get_witnesses_at_device", "cw_get_witnesses_at_device_n8")
RANGES = [(0, None), (1, 7), (3, 65), (15, 17)]                                      # (entry0, n); None = the whole witness
WORDS = [0, 1, 4, 5, NONE]                                                           # masks and wanted words of the sweep


def lists(B):
    """the lists of a batch of B: empty; one instance; the identity; the identity reversed; [63, 64]; 65 positions with a
    repeat; the last instance alone; 130 positions drawn from a fixed seed"""
    rep = np.arange(65) % B
    rep[64] = 3
    out = [[], [7 % B], np.arange(B), np.arange(B)[::-1], [63, 64], rep, [B - 1], np.random.default_rng(130).integers(0, B, size=130)]
    return [np.asarray(x, dtype=np.uint32) for x in out]


def clip(entry0, n, nw):
    """an entry range of the matrix on a witness of nw entries (Multiplier2 has four)"""
    entry0 = min(entry0, nw - 1)
    return entry0, nw - entry0 if n is None else min(n, nw - entry0)


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


# ---- without a GPU ---------------------------------------------------------------------------------------------------------------
def test_the_library_exports_the_six_symbols():
    from circom_amd import runtime as rt
    L = rt.lib()
    for name in SYMBOLS:
        assert hasattr(L, name), name
    for name in ("select", "select_device", "witnesses_at", "witnesses_at_device"):
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
def test_argument_checks_come_before_the_device(tmp_path, kind):
    """a host-only batch: every CW_EINVAL case is CW_EINVAL, only a call whose arguments are in order reaches CW_EDEVICE, and
    nothing is written either way"""
    from circom_amd import runtime as rt
    L = rt.lib()
    c = _host_circuit(tmp_path, kind)
    nw, B = c.n_witness, 5
    assert nw >= 4
    b = c.batch(B, device=-1)
    err = lambda: L.cw_last_error().decode()
    idx = np.full(B, A5, dtype=np.uint32)
    n = C.c_uint32(123)
    # select
    assert L.cw_select_instances(None, 0, 0, _ptr(idx), C.byref(n)) == CW_EINVAL
    assert L.cw_select_instances(b.h, 0, 0, _ptr(idx), None) == CW_EINVAL
    assert L.cw_select_instances(b.h, 0, 0, _ptr(idx), C.byref(n)) == CW_EDEVICE
    assert L.cw_select_instances(b.h, NONE, 0, None, C.byref(n)) == CW_EDEVICE              # idx may be null: it only counts
    d = lambda a: C.c_void_p(a)
    assert L.cw_select_instances_device(None, 0, 0, d(4096), d(8192)) == CW_EINVAL
    assert L.cw_select_instances_device(b.h, 0, 0, None, d(8192)) == CW_EINVAL
    assert L.cw_select_instances_device(b.h, 0, 0, d(4096), None) == CW_EINVAL
    assert L.cw_select_instances_device(b.h, 0, 0, d(4098), d(8192)) == CW_EINVAL and "4-byte" in err()
    assert L.cw_select_instances_device(b.h, 0, 0, d(4096), d(8193)) == CW_EINVAL
    assert L.cw_select_instances_device(b.h, 0, 0, d(4096), d(8196)) == CW_EDEVICE
    assert (idx == A5).all() and n.value == 123
    # egress by index, host forms
    lst = np.array([0, 4, 2, 2], dtype=np.uint32)
    out = np.full((4, nw, 32), 0xA5, dtype=np.uint8)
    for fn in (L.cw_get_witnesses_at, L.cw_get_witnesses_at_n8):
        assert fn(None, 0, nw, _ptr(lst), 4, _ptr(out)) == CW_EINVAL
        assert fn(b.h, 0, nw, None, 4, _ptr(out)) == CW_EINVAL
        assert fn(b.h, 0, nw, _ptr(lst), 4, None) == CW_EINVAL
        assert fn(b.h, 0, nw + 1, _ptr(lst), 4, _ptr(out)) == CW_EINVAL                      # entries past the witness list
        assert fn(b.h, nw, 1, _ptr(lst), 4, _ptr(out)) == CW_EINVAL
        assert fn(b.h, 2, 0xFFFFFFFF, _ptr(lst), 4, _ptr(out)) == CW_EINVAL                  # entry0 + n wraps in 32 bits
        assert fn(b.h, 0xFFFFFFFF, 2, _ptr(lst), 4, _ptr(out)) == CW_EINVAL
        bad = np.array([0, 4, B, 0xFFFFFFFF], dtype=np.uint32)                               # an index equal to the batch: position 2
        assert fn(b.h, 0, nw, _ptr(bad), 4, _ptr(out)) == CW_EINVAL
        assert "idx[2] = %d" % B in err() and "cw_get_witnesses_at" in err()
        assert fn(b.h, 0, nw, _ptr(bad), 2, _ptr(out)) == CW_EDEVICE                         # (the list ends before it)
        assert fn(b.h, 0, nw, _ptr(lst), 4, _ptr(out)) == CW_EDEVICE
        assert fn(b.h, 1, 2, _ptr(lst), 4, _ptr(out)) == CW_EDEVICE
        assert fn(b.h, nw, 0, _ptr(lst), 0, _ptr(out)) == CW_EDEVICE
    assert (out == 0xA5).all()
    # device forms: the image 16-byte aligned for 32-byte elements, 8-byte aligned for the 8-byte element of the 64-bit runtime
    eb = c.element_bytes
    assert eb == (8 if kind == "m2g" else 32)
    for fn, align in ((L.cw_get_witnesses_at_device, 16), (L.cw_get_witnesses_at_device_n8, 8 if eb == 8 else 16)):
        ok = (b.h, 0, nw, d(4096), 4, d(8192), d(1 << 20), d(8196))
        call = lambda k=None, v=None: fn(*[v if i == k else a for i, a in enumerate(ok)])
        assert call(0, None) == CW_EINVAL                                                    # null batch / list / image
        assert call(3, None) == CW_EINVAL and call(6, None) == CW_EINVAL
        assert call(2, nw + 1) == CW_EINVAL and call(1, nw) == CW_EINVAL and call(2, 0xFFFFFFFF) == CW_EINVAL
        assert call(3, d(4098)) == CW_EINVAL and call(5, d(8194)) == CW_EINVAL and call(7, d(8197)) == CW_EINVAL
        assert call(6, d((1 << 20) + align // 2)) == CW_EINVAL and "aligned" in err()
        assert call(6, d((1 << 20) + 4)) == CW_EINVAL
        assert call() == CW_EDEVICE
        assert call(5, None) == CW_EDEVICE and call(7, None) == CW_EDEVICE                   # the count and the word are optional
        assert call(6, d((1 << 20) + align)) == CW_EDEVICE
    # the Python forms
    with pytest.raises(rt.CwError) as e:
        b.witnesses_at([0, B])
    assert e.value.code == CW_EINVAL and "idx[1]" in str(e.value)
    with pytest.raises(rt.CwError) as e:
        b.witnesses_at([0, 1], 0, nw + 1)
    assert e.value.code == CW_EINVAL
    for call in (lambda: b.select(), lambda: b.witnesses_at([0, 1]), lambda: b.witnesses_at([]),
                 lambda: b.select_device(0, 0, 4096, 8192), lambda: b.witnesses_at_device(4096, 2, 1 << 20)):
        with pytest.raises(rt.CwError) as e:
            call()
        assert e.value.code == CW_EDEVICE
    b.close(); c.close()


# ---- GPU -------------------------------------------------------------------------------------------------------------------------
class _Lists(_Dev):
    """_Dev's arena (an image ENDS where the allocation ends) + a list, a count, and index buffers of exactly `batch` words"""

    def __init__(self):
        super().__init__()
        self.list = self.alloc(4 * 4096)
        self.cnt = self.alloc(8)
        self.sel = {}

    def words(self, p, n):
        return self.download(p, n, np.uint32)

    def put_list(self, idx):
        idx = np.ascontiguousarray(idx, dtype=np.uint32)
        assert len(idx) <= 4096
        if len(idx):
            self.put(self.list, idx)
        return self.list

    def sel_buf(self, B):
        """B words of 0xA5 that end at the end of their allocation"""
        if B not in self.sel:
            self.sel[B] = self.alloc(4 * B)
        self.put(self.sel[B], np.full(B, A5, dtype=np.uint32))
        return self.sel[B]

    def at(self, b, idx, entry0, n, eb=32, dn=None, guard=64):
        """the device form into 0xA5 bytes at the end of the arena, `guard` more in front of the image:
        (image [len(idx)][n][eb], the guard bytes, the word)"""
        m = len(idx)
        nbytes = m * n * eb
        p = self.at_end(nbytes + guard) + guard
        self.put_list(idx)
        self.put(self.word, np.array([0x12345678], dtype=np.uint32))
        d_n = None
        if dn is not None:
            self.put(self.cnt, np.array([dn], dtype=np.uint32))
            d_n = self.cnt
        b.witnesses_at_device(self.list, m, p, entry0, n, d_n_idx=d_n, d_bad=self.word, n8=(eb == 8))
        return self.download(p, (m, n, eb)), self.download(p - guard, guard), int(self.words(self.word, 1)[0])


@pytest.fixture(scope="module")
def hip():
    return _Lists()


@pytest.fixture(scope="module")
def circuits(tmp_path_factory):
    """every circuit of this module, compiled once: name -> (flat circuit, runtime circuit); the witness list is every signal"""
    from circom_amd import runtime as rt
    made = {}
    progs = {"bg15": lambda: Program(BitGadget(15)), "bassert": lambda: Program(BitAssert()), "badbit": lambda: Program(BadBit(4)),
             "gl15": lambda: Program(BitGadget(15), prime="goldilocks"), "glassert": lambda: Program(BitAssert(), prime="goldilocks"),
             "glbadbit": lambda: Program(BadBit(4), prime="goldilocks")}

    def get(name):
        if name not in made:
            d = str(tmp_path_factory.mktemp(name))
            if name == "m2mont":
                # (no emitted code: the interpreter keeps the same Montgomery-form table, and the test saves the assembler's seconds)
                cp = compile_program(Program(Multiplier2()), d, name, sym=False, strands=(1,), pipe=None, mont=True, fpjit=False)
            elif name.startswith("gl"):
                cp = compile_program(progs[name](), d, name, sym=False)
            else:
                cp = compile_program(progs[name](), d, name, sym=False, strands=(1,), bits=True, jit=True)
                assert cp.jit is not None
            c = rt.Circuit(cp.tape_path, cp.dat_path, cp.r1cs_path)
            if c.n_witness != cp.flat.n_signals:
                c.set_witness_list(np.arange(c.n_signals, dtype=np.uint32))
            assert c.n_witness == cp.flat.n_signals
            made[name] = (cp.flat, c)
        return made[name]

    yield get
    for _, c in made.values():
        c.close()


def _image(sig):
    return np.frombuffer(b"".join(v.to_bytes(32, "little") for v in sig), dtype=np.uint8).reshape(-1, 32)


def _eval(fc, row):
    return eval_flat(fc.fp.q, fc.n_signals, fc.n_temps, fc.constants, fc.code, {fc.main_input_start + k: int(v) for k, v in enumerate(row)})


@functools.lru_cache(maxsize=None)
def _flat(name):
    return flatten({"bg15": lambda: Program(BitGadget(15)), "gl15": lambda: Program(BitGadget(15), prime="goldilocks"),
                    "bassert": lambda: Program(BitAssert()), "badbit": lambda: Program(BadBit(4)),
                    "glassert": lambda: Program(BitAssert(), prime="goldilocks"), "glbadbit": lambda: Program(BadBit(4), prime="goldilocks"),
                    "m2": lambda: Program(Multiplier2())}[name]())


def _batch(circuits, monkeypatch, kind, B):
    """(runtime circuit, batch, element bytes of the _n8 forms) of BitGadget(15) on one of the engines"""
    if kind in ("interp", "jit"):
        monkeypatch.setenv("CW_BITS_JIT", "1" if kind == "jit" else "0")
        fc, c = circuits("bg15")
        b = c.batch(B)
        assert b.bitmode and b.jit == (kind == "jit") and b.bits_sh == (5 if kind == "jit" else 0)
    elif kind == "wide":
        fc, c = circuits("bg15")
        monkeypatch.setenv("CW_BITS", "0")
        b = c.batch(B)
        monkeypatch.delenv("CW_BITS")
        assert not b.bitmode and c.element_bytes == 32
    else:
        fc, c = circuits("gl15")
        b = c.batch(B)
        assert not b.bitmode and c.element_bytes == 8
    return c, b


def _host_at(b, idx, entry0, n, eb=32):
    """the host form into an array of 0xA5 bytes with 16 spare bytes behind the image: (image, spare)"""
    from circom_amd import runtime as rt
    idx = np.ascontiguousarray(idx, dtype=np.uint32)
    flat = np.full(len(idx) * n * eb + 16, 0xA5, dtype=np.uint8)
    spare = np.zeros(2, dtype=np.uint32)
    fn = rt.lib().cw_get_witnesses_at_n8 if eb == 8 else rt.lib().cw_get_witnesses_at
    rt._chk(fn(b.h, entry0, n, _ptr(idx) if len(idx) else _ptr(spare), len(idx), _ptr(flat)))
    return flat[:-16].reshape(len(idx), n, eb), flat[-16:]


def _check_list(hip, b, want, idx, entry0, n, ebs):
    """host form, device form, device form with a device count below and above n_idx - against want[instance][entry][32]"""
    m = len(idx)
    for eb in ebs:
        exp = want[idx.astype(np.int64), entry0:entry0 + n, :eb] if m else np.zeros((0, n, eb), dtype=np.uint8)
        where = (eb, m, entry0, n)
        got, spare = _host_at(b, idx, entry0, n, eb)
        assert (got == exp).all() and (spare == 0xA5).all(), ("host",) + where
        got, guard, word = hip.at(b, idx, entry0, n, eb)
        assert (got == exp).all() and (guard == 0xA5).all() and word == NONE, ("device",) + where
        if m >= 2:
            dn = m // 2
            got, guard, word = hip.at(b, idx, entry0, n, eb, dn=dn)
            assert (got[:dn] == exp[:dn]).all() and (got[dn:] == 0xA5).all() and (guard == 0xA5).all() and word == NONE, ("d_n_idx",) + where
            got, guard, word = hip.at(b, idx, entry0, n, eb, dn=m + 5)
            assert (got == exp).all() and word == NONE, ("d_n_idx past n_idx",) + where


@pytest.mark.gpu
@pytest.mark.parametrize("kind,B", [("interp", 130), ("interp", 300), ("jit", 130), ("jit", 300), ("wide", 300), ("gl", 65), ("gl", 300)])
def test_gpu_egress_by_index_on_every_layout(circuits, hip, monkeypatch, kind, B):
    c, b = _batch(circuits, monkeypatch, kind, B)
    bits, want = _case(15, "goldilocks" if kind == "gl" else "bn128")
    b.set_inputs_rows(pack_rows(bits[:B], (bits.shape[1] + 7) // 8, True))
    b.run(); b.check_r1cs(); b.sync()
    assert (b.status() == 0).all()
    nw = c.n_witness
    assert nw > 129
    for idx in lists(B):
        for entry0, n in RANGES:
            _check_list(hip, b, want, idx, *clip(entry0, n, nw), ebs=(32, 8) if kind == "gl" else (32,))
    # the Python form; the public signals of a list
    got = b.witnesses_at([B - 1, 0, 0], 1, c.n_public)
    assert got.shape == (3, c.n_public, 32) and (got == want[[B - 1, 0, 0], 1:1 + c.n_public]).all()
    assert (b.witnesses_at(np.arange(B)) == want[:B]).all()
    b.close()


@pytest.mark.gpu
def test_gpu_egress_by_index_converts_a_montgomery_table(circuits, hip):
    fc, c = circuits("m2mont")
    assert c.montgomery and c.n_witness == 4
    B = 65
    rng = np.random.default_rng(65)
    ins = [[int.from_bytes(rng.bytes(32), "little") % c.q for _ in range(2)] for _ in range(B)]
    want = np.stack([_image(_eval(_flat("m2"), row)[0]) for row in ins])
    b = c.batch(B)
    b.set_inputs(ins)
    b.run(); b.sync()
    for idx in lists(B):
        for entry0, n in RANGES:
            _check_list(hip, b, want, idx, *clip(entry0, n, 4), ebs=(32,))
    b.close()


@functools.lru_cache(maxsize=None)
def _odd_case(name, odd):
    """_rerun_case() of the row tests (imported above: instances 5, 64 and 129) for ANY set of instances - the case in which more
    than a quarter of the batch is not boolean needs 43 of them: BitGadget(15) x 130 where the instances `odd` have input 5 equal
    to 7: (inputs [130][45], signals [130][n_signals][32] and the status words after the R1CS check, all from the oracle)"""
    fc = _flat(name)
    bits, want = _case(15, "goldilocks" if name == "gl15" else "bn128")
    vals = bits[:130].astype(np.int64)
    out = want[:130].copy()
    words = np.zeros(130, dtype=np.uint32)
    for i in odd:
        vals[i, 5] = 7
        sig, failed = _eval(fc, vals[i])
        assert failed is None                                     # (a[5] = 7 trips no check of the witness code)
        out[i] = _image(sig)
        words[i] = 0 if check_r1cs(fc.fp.q, fc.constraints, sig) is None else 4
    return vals, out, words


def _run_values(b, c, vals):
    image = np.zeros((len(vals), c.n_inputs, 32), dtype=np.uint8)
    image[:, :, 0] = vals
    b.set_inputs(image)
    b.run(); b.check_r1cs(); b.sync()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["interp", "jit"])
def test_gpu_rerun_instances_are_written_over_from_the_side_batch(circuits, hip, monkeypatch, kind):
    c, b = _batch(circuits, monkeypatch, kind, 130)
    _, vals, want = _rerun_case()                                 # instances 5, 64 and 129 are not boolean
    fc = _flat("bg15")
    words = np.zeros(130, dtype=np.uint32)
    for i in (5, 64, 129):                                        # the oracle's word after the check (a[5] = 7 satisfies the system: 0)
        sig = [int.from_bytes(v.tobytes(), "little") for v in want[i]]
        words[i] = 0 if check_r1cs(fc.fp.q, fc.constraints, sig) is None else 4
    _run_values(b, c, vals)
    nw = c.n_witness
    among = np.array([0, 5, 6, 63, 64, 65, 128, 129, 4, 100], dtype=np.uint32)
    twice = np.array([64, 1, 64, 2, 129], dtype=np.uint32)
    only = np.array([129, 5, 64, 5], dtype=np.uint32)
    for idx in (among, twice, only, np.arange(130, dtype=np.uint32)):
        for entry0, n in RANGES:
            _check_list(hip, b, want, idx, *clip(entry0, n, nw), ebs=(32,))
    assert (b.select(4, 4) == np.flatnonzero(words == 4)).all() and (b.select() == np.flatnonzero(words == 0)).all()
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["interp", "jit"])
def test_gpu_a_side_batch_that_holds_everything_serves_the_list(circuits, hip, monkeypatch, kind):
    """more than a quarter of the instances is not boolean: the whole batch went through the 256-bit schedule"""
    odd = tuple(range(3, 130, 3))
    assert len(odd) > 130 // 4
    c, b = _batch(circuits, monkeypatch, kind, 130)
    vals, want, words = _odd_case("bg15", odd)
    _run_values(b, c, vals)
    nw = c.n_witness
    for idx in (lists(130)[7], np.array([3, 4, 129, 3], dtype=np.uint32)):
        for entry0, n in RANGES:
            _check_list(hip, b, want, idx, *clip(entry0, n, nw), ebs=(32,))
    assert (b.select(4, 4) == np.flatnonzero(words == 4)).all() and (b.select(NONE, 0) == np.flatnonzero(words == 0)).all()
    got, guard, word = hip.at(b, np.array([1, 130, 2], dtype=np.uint32), 0, nw)
    assert word == 1 and not got[1].any() and (got[[0, 2]] == want[[1, 2]]).all()
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["interp", "jit", "wide", "gl"])
def test_gpu_bad_device_indices_give_zero_rows_and_are_reported(circuits, hip, monkeypatch, kind):
    B = 130
    c, b = _batch(circuits, monkeypatch, kind, B)
    if kind == "gl":
        bits, want = _case(15, "goldilocks")
        b.set_inputs_rows(pack_rows(bits[:B], (bits.shape[1] + 7) // 8, True))
        b.run(); b.sync()
    else:
        _, vals, want = _rerun_case()                             # (the bit engine: with a side batch behind it)
        _run_values(b, c, vals)
    nw = c.n_witness
    idx = np.arange(70, dtype=np.uint32)[::-1].copy()
    idx[[9, 66]] = [0xFFFFFFFF, B]
    good = np.delete(np.arange(70), [9, 66])
    for eb in ((32, 8) if kind == "gl" else (32,)):
        for entry0, n in ((0, nw), (3, 65)):
            got, guard, word = hip.at(b, idx, entry0, n, eb)
            assert word == 9 and not got[[9, 66]].any() and (guard == 0xA5).all(), (eb, entry0, n)
            assert (got[good] == want[idx[good].astype(np.int64), entry0:entry0 + n, :eb]).all(), (eb, entry0, n)
            got, guard, word = hip.at(b, idx[10:], entry0, n, eb)
            assert word == 56 and not got[56].any() and (got[:56] == want[idx[10:66].astype(np.int64), entry0:entry0 + n, :eb]).all()
            got, guard, word = hip.at(b, idx, entry0, n, eb, dn=9)            # the list ends before the first bad position
            assert word == NONE and (got[9:] == 0xA5).all() and (got[:9] == want[idx[:9].astype(np.int64), entry0:entry0 + n, :eb]).all()
            got, guard, word = hip.at(b, idx[:9], entry0, n, eb)
            assert word == NONE
    b.close()


# ---- a range and the list of its instances: one kernel per table, the same bytes ---------------------------------------------------
FORMS = [(0, 300), (37, 201), (63, 2), (64, 64), (299, 1)]                           # (first, count) of a batch of 300
GUARD = 64


def _guarded(hip, nbytes, call):
    """`call(p)` writes an image of nbytes into 0xA5 bytes, GUARD more on either side: (image, the 2 x GUARD bytes around it)"""
    p = hip.at_end(nbytes + 2 * GUARD) + GUARD
    call(p)
    return hip.download(p, nbytes), np.concatenate([hip.download(p - GUARD, GUARD), hip.download(p + nbytes, GUARD)])


def _range_and_list(hip, b, want, first, count, nw, ebs):
    """cw_get_witnesses_device(_n8) of [first, first + count), its entries [entry0, entry0 + n) against
    cw_get_witnesses_at_device(_n8) of the list first .. first + count - 1 - and both against want[instance][entry][32]"""
    idx = np.arange(first, first + count, dtype=np.uint32)
    hip.put_list(idx)
    for eb in ebs:
        where = (first, count, eb)
        ranged, guard = _guarded(hip, count * nw * eb, lambda p: (b.witnesses_device_n8 if eb == 8 else b.witnesses_device)(first, count, p))
        ranged = ranged.reshape(count, nw, eb)
        assert (guard == 0xA5).all(), ("range",) + where
        assert (ranged == want[first:first + count, :, :eb]).all(), ("range",) + where
        for entry0, n in (clip(e, m, nw) for e, m in RANGES):
            hip.put(hip.word, np.array([0x12345678], dtype=np.uint32))
            listed, guard = _guarded(hip, count * n * eb,
                                     lambda p: b.witnesses_at_device(hip.list, count, p, entry0, n, d_bad=hip.word, n8=(eb == 8)))
            assert (guard == 0xA5).all() and hip.words(hip.word, 1)[0] == NONE, ("list", entry0, n) + where
            assert listed.tobytes() == ranged[:, entry0:entry0 + n].tobytes(), ("list", entry0, n) + where
            assert (listed.reshape(count, n, eb) == want[first:first + count, entry0:entry0 + n, :eb]).all(), ("list", entry0, n) + where


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["interp", "jit", "wide", "gl"])
def test_gpu_a_range_and_the_list_of_its_instances_are_the_same_bytes(circuits, hip, monkeypatch, kind):
    """on the bit engines (37, 201) and (63, 2) start off a group boundary: the window read is shifted and takes a second group,
    from the range form and from the dense branch of the list form"""
    B = 300
    c, b = _batch(circuits, monkeypatch, kind, B)
    bits, want = _case(15, "goldilocks" if kind == "gl" else "bn128")
    b.set_inputs_rows(pack_rows(bits[:B], (bits.shape[1] + 7) // 8, True))
    b.run(); b.sync()
    assert (b.status() == 0).all()
    for first, count in FORMS:
        _range_and_list(hip, b, want, first, count, c.n_witness, ebs=(32, 8) if kind == "gl" else (32,))
    b.close()


@pytest.mark.gpu
def test_gpu_a_range_and_its_list_convert_a_montgomery_table_alike(circuits, hip):
    fc, c = circuits("m2mont")
    assert c.montgomery and c.n_witness == 4
    B = 300
    rng = np.random.default_rng(300)
    ins = [[int.from_bytes(rng.bytes(32), "little") % c.q for _ in range(2)] for _ in range(B)]
    want = np.stack([_image(_eval(_flat("m2"), row)[0]) for row in ins])
    b = c.batch(B)
    b.set_inputs(ins)
    b.run(); b.sync()
    for first, count in FORMS:
        _range_and_list(hip, b, want, first, count, 4, ebs=(32,))
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["interp", "jit"])
def test_gpu_a_range_and_its_list_agree_on_the_rerun_instances(circuits, hip, monkeypatch, kind):
    """instances 5, 64 and 129 are not boolean: the range form writes their rows over run by run (cw_rerun_runs), the list form in
    one launch through the instance -> side-batch map"""
    c, b = _batch(circuits, monkeypatch, kind, 130)
    _, vals, want = _rerun_case()
    _run_values(b, c, vals)
    for first, count in ((0, 130), (37, 93), (63, 2), (64, 64), (129, 1), (5, 1)):
        _range_and_list(hip, b, want, first, count, c.n_witness, ebs=(32,))
    b.close()


@pytest.mark.gpu
def test_gpu_a_range_of_more_than_65535_tiles_on_the_256_bit_schedule(circuits, hip):
    """Multiplier2 on the 8 x u32 table (Montgomery form), 65 535 x 64 + 1 instances: the smallest batch whose range egress is a
    second launch, of one instance.  Inputs below 2^31: the product is exact in 64 bits.  The image is half a gigabyte"""
    fc, c = circuits("m2mont")
    B = 65535 * 64 + 1
    rng = np.random.default_rng(B)
    ab = rng.integers(0, 1 << 31, size=(B, 2), dtype=np.uint32)
    want = np.zeros((B, 4, 4), dtype=np.uint64)                  # the witness is (1, out, a, b)
    want[:, 0, 0], want[:, 1, 0], want[:, 2:, 0] = 1, ab[:, 0].astype(np.uint64) * ab[:, 1], ab
    b = c.batch(B)
    b.set_inputs_range(0, ab)
    b.run(); b.sync()
    assert (b.status() == 0).all()
    nbytes = B * 4 * 32
    p = hip.alloc(nbytes + 2 * GUARD)
    hip.h.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    assert hip.h.hipMemset(p, 0xA5, nbytes + 2 * GUARD) == 0
    b.witnesses_device(0, B, p + GUARD)
    got = hip.download(p + GUARD, (B, 4, 4), np.uint64)
    guard = np.concatenate([hip.download(p, GUARD), hip.download(p + GUARD + nbytes, GUARD)])
    hip.h.hipFree(p)
    b.close()
    assert (guard == 0xA5).all()
    bad = np.flatnonzero((got != want).any(axis=(1, 2)))
    assert len(bad) == 0, "first rows that differ: %s" % bad[:8].tolist()


# ---- select ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _select_case(name, B):
    """(inputs [B][n_in] of bits, status words before the check, after the check, signals [B][n_signals][32]) of BitAssert /
    BadBit(4): the oracle's, one evaluation per distinct input row.  BitAssert: about one instance in ten has a != b (the
    assertion fails, the row a - b = 0 too: 1, then 5); BadBit(4): the witness code writes a xor b where the constraint wants
    a and b, so the R1CS holds only where every a_k = b_k = 0 - about half of the instances - (0, then 4).  The first and the last
    instance fail, their neighbours are clean"""
    fc = _flat(name)
    rng = np.random.default_rng(B)
    if name.endswith("assert"):
        bits = rng.integers(0, 2, size=(B, 1), dtype=np.uint8).repeat(2, axis=1)
        bits[rng.random(B) < 0.1, 1] ^= 1
        bits[[0, B - 1]] = [0, 1]
        bits[[1, B - 2]] = [1, 1]
    else:
        bits = rng.integers(0, 2, size=(B, 8), dtype=np.uint8)
        bits[rng.random(B) < 0.5] = 0
        bits[[0, B - 1]] = 1
        bits[[1, B - 2]] = 0
    known = {}
    before, after = np.zeros(B, dtype=np.uint32), np.zeros(B, dtype=np.uint32)
    for i, row in enumerate(bits):
        key = row.tobytes()
        if key not in known:
            sig, failed = _eval(fc, row)
            w = 0 if failed is None else 1 | (failed << 8)
            known[key] = (w, w | (0 if check_r1cs(fc.fp.q, fc.constraints, sig) is None else 4), _image(sig))
        before[i], after[i] = known[key][:2]
    sigs = np.stack([known[row.tobytes()][2] for row in bits])
    return bits, before, after, sigs


def _select_both(hip, b, B, mask, want):
    """(host form, count-only form, device form), each checked for what it leaves untouched"""
    from circom_amd import runtime as rt
    L = rt.lib()
    idx, n = np.full(B, A5, dtype=np.uint32), C.c_uint32(A5)
    rt._chk(L.cw_select_instances(b.h, mask, want, _ptr(idx), C.byref(n)))
    assert n.value <= B and (idx[n.value:] == A5).all()
    cnt = C.c_uint32(A5)
    rt._chk(L.cw_select_instances(b.h, mask, want, None, C.byref(cnt)))
    d_idx = hip.sel_buf(B)
    hip.put(hip.cnt, np.array([A5, A5], dtype=np.uint32))
    b.select_device(mask, want, d_idx, hip.cnt)
    got, dn = hip.words(d_idx, B), hip.words(hip.cnt, 2)
    assert dn[0] <= B and dn[1] == A5 and (got[dn[0]:] == A5).all()
    return idx[:n.value], cnt.value, got[:dn[0]]


def _sweep(hip, b, B, words):
    st = b.status()
    assert (st == words).all(), np.flatnonzero(st != words)[:8]
    for mask in WORDS:
        for want in WORDS:
            exp = np.flatnonzero((words & mask) == want)
            host, cnt, dev = _select_both(hip, b, B, mask, want)
            assert len(host) == len(exp) and (host == exp).all() and cnt == len(exp), (mask, want)
            assert len(dev) == len(exp) and (dev == exp).all(), (mask, want)
            assert (exp == np.flatnonzero((st & mask) == want)).all()
    assert (b.select() == np.flatnonzero(words == 0)).all()


def _select_batch(circuits, monkeypatch, engine, circuit, B):
    name = {("gl", "assert"): "glassert", ("gl", "badbit"): "glbadbit"}.get((engine, circuit), "bassert" if circuit == "assert" else "badbit")
    fc, c = circuits(name)
    if engine in ("interp", "jit"):
        monkeypatch.setenv("CW_BITS_JIT", "1" if engine == "jit" else "0")
        b = c.batch(B)
        assert b.bitmode and b.jit == (engine == "jit")
    elif engine == "wide":
        monkeypatch.setenv("CW_BITS", "0")
        b = c.batch(B)
        monkeypatch.delenv("CW_BITS")
        assert not b.bitmode and c.element_bytes == 32
    else:
        b = c.batch(B)
        assert c.element_bytes == 8
    return name, c, b


@pytest.mark.gpu
@pytest.mark.parametrize("B", [300, 2049])
@pytest.mark.parametrize("circuit", ["assert", "badbit"])
@pytest.mark.parametrize("engine", ["interp", "jit", "wide", "gl"])
def test_gpu_select_sweeps_masks_and_words(circuits, hip, monkeypatch, engine, circuit, B):
    name, c, b = _select_batch(circuits, monkeypatch, engine, circuit, B)
    bits, before, after, _ = _select_case(name, B)
    assert {int(w) & 0xFF for w in after} == ({0, 5} if circuit == "assert" else {0, 4}) and (before & 4 == 0).all()
    assert after[0] and after[B - 1] and not after[1] and not after[B - 2]
    b.set_inputs_rows(pack_rows(bits, 1, False), msb_first=False)
    b.run(); b.sync()
    _sweep(hip, b, B, before)                                     # before cw_check_r1cs: the R1CS bit is simply not set
    b.check_r1cs(); b.sync()
    _sweep(hip, b, B, after)
    fb, cap = b.r1cs_first_bad(), b.graph_captured
    b.select(4, 4); b.witnesses_at(b.select(1, 1))
    assert (b.status() == after).all() and (b.r1cs_first_bad() == fb).all() and b.graph_captured == cap
    b.close()


@pytest.mark.gpu
def test_gpu_select_beyond_one_pass_of_the_scan(circuits, hip):
    """2 097 153 instances are 1 025 count blocks, the smallest batch with a second pass of the scan's loop: its running sum is
    carried over, and the last block holds one instance (Goldilocks BitAssert: a table of tens of megabytes)"""
    fc, c = circuits("glassert")
    B = 2097152 + 1                                               # the smallest batch with a 1 025th count block
    rng = np.random.default_rng(B)
    a = rng.integers(0, 2, size=(B, 1), dtype=np.uint8).repeat(2, axis=1)
    a[rng.random(B) < 0.01, 1] ^= 1
    a[[0, B - 1]] = [0, 1]
    a[[1, B - 2, 2097150]] = [1, 1]
    a[2097149] = [1, 0]
    words = {}
    for x, y in ((0, 0), (0, 1), (1, 0), (1, 1)):
        sig, failed = _eval(_flat("glassert"), (x, y))
        words[(x, y)] = 0 if failed is None else 1 | (failed << 8)
    table = np.array([[words[(0, 0)], words[(0, 1)]], [words[(1, 0)], words[(1, 1)]]], dtype=np.uint32)
    exp_words = table[a[:, 0], a[:, 1]]
    b = c.batch(B)
    b.set_inputs_n8(a.astype(np.uint64))
    b.run(); b.sync()
    failed = np.flatnonzero(exp_words & 1)
    assert failed[0] == 0 and failed[-1] == B - 1 and 2097149 in failed and 10000 < len(failed) < 40000
    got = b.select(1, 1)
    assert len(got) == len(failed) and (got == failed).all()
    got = b.select()
    clean = np.flatnonzero(exp_words == 0)
    assert len(got) == len(clean) and (got == clean).all()
    d_idx = hip.sel_buf(B)
    b.select_device(1, 1, d_idx, hip.cnt)
    dev = hip.words(d_idx, B)
    assert hip.words(hip.cnt, 1)[0] == len(failed) and (dev[:len(failed)] == failed).all() and (dev[len(failed):] == A5).all()
    b.close()


# ---- chained, state --------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("circuit", ["assert", "badbit"])
@pytest.mark.parametrize("engine", ["interp", "jit", "wide", "gl"])
def test_gpu_select_feeds_the_egress_without_a_host_read(circuits, hip, monkeypatch, engine, circuit):
    """select_device, then witnesses_at_device with d_n_idx = d_n and n_idx = batch: the image is the oracle's rows of the selected
    instances, the rows behind them are untouched.  On the bit engine the instances whose assertion failed were re-run: their
    rows come from the side batch, and the host never learns which they are"""
    B = 300
    name, c, b = _select_batch(circuits, monkeypatch, engine, circuit, B)
    bits, before, words, want = _select_case(name, B)
    b.set_inputs_rows(pack_rows(bits, 1, False), msb_first=False)
    b.run(); b.check_r1cs(); b.sync()
    nw = c.n_witness
    failed_word = 5 if circuit == "assert" else 4
    for mask, wanted in ((NONE, 0), (failed_word, failed_word), (0, 0)):
        sel = np.flatnonzero((words & mask) == wanted)
        k = len(sel)
        assert 10 < k <= B
        for eb in ((32, 8) if engine == "gl" else (32,)):
            for entry0, n in ((0, nw), (1, c.n_public)):
                p = hip.at_end(B * n * eb)
                d_idx = hip.sel_buf(B)
                hip.put(hip.word, np.array([0x12345678], dtype=np.uint32))
                hip.put(hip.cnt, np.array([A5, A5], dtype=np.uint32))
                b.select_device(mask, wanted, d_idx, hip.cnt)
                b.witnesses_at_device(d_idx, B, p, entry0, n, d_n_idx=hip.cnt, d_bad=hip.word, n8=(eb == 8))
                got = hip.download(p, (B, n, eb))
                assert (got[:k] == want[sel, entry0:entry0 + n, :eb]).all() and (got[k:] == 0xA5).all(), (mask, eb, entry0, n)
                assert hip.words(hip.cnt, 1)[0] == k and hip.words(hip.word, 1)[0] == NONE
    b.close()


@pytest.mark.gpu
def test_gpu_state_comes_last_and_empty_calls_write_nothing(circuits, hip):
    from circom_amd import runtime as rt
    L = rt.lib()
    fc, c = circuits("bg15")
    bits, want = _case(15)
    B, nw = 65, c.n_witness
    b = c.batch(B)
    p = hip.at_end(B * nw * 32)
    calls = {"cw_select_instances": lambda: b.select(), "cw_select_instances_device": lambda: b.select_device(0, 0, hip.sel_buf(B), hip.cnt),
             "cw_get_witnesses_at": lambda: b.witnesses_at([0, 1]), "cw_get_witnesses_at_device": lambda: b.witnesses_at_device(hip.list, 2, p)}
    for who, call in calls.items():
        with pytest.raises(rt.CwError) as e:
            call()
        assert e.value.code == CW_ESTATE and who + " before cw_run" in str(e.value)
    assert L.cw_get_witnesses_at_device(b.h, 0, nw + 1, C.c_void_p(hip.list), 2, None, C.c_void_p(p), None) == CW_EINVAL     # the argument first
    b.set_inputs_rows(pack_rows(bits[:B], (bits.shape[1] + 7) // 8, True))
    b.run(); b.sync()
    for entry0, n, m in ((3, 0, 5), (nw, 0, 5), (0, nw, 0), (0, 0, 0)):
        idx = np.arange(m, dtype=np.uint32)
        got, spare = _host_at(b, idx, entry0, n)
        assert (spare == 0xA5).all()
        hip.put(hip.word, np.array([0x12345678], dtype=np.uint32))
        p = hip.at_end(B * nw * 32)
        b.witnesses_at_device(hip.put_list(idx), m, p, entry0, n, d_bad=hip.word)
        assert (hip.download(p, B * nw * 32) == 0xA5).all() and hip.words(hip.word, 1)[0] == NONE
    assert b.witnesses_at([]).shape == (0, nw, 32) and b.witnesses_at([1, 2], 5, 0).shape == (2, 0, 32)
    b.close()


@pytest.mark.gpu
def test_gpu_a_supplied_table_is_served_once_it_is_complete(circuits, hip):
    """64-bit runtime, supplied witnesses: a gap answers the missing-witnesses text of cw_check_r1cs; after a complete supply both
    calls serve the supplied values and words"""
    from circom_amd import runtime as rt
    fc, c = circuits("gl15")
    B, nw = 65, c.n_witness
    bits, want = _case(15, "goldilocks")
    vals = np.ascontiguousarray(want[:B, :, :8]).view("<u8").reshape(B, nw).copy()
    vals[40, 9] ^= 1                                              # instance 40: no witness of the system any more
    sig40 = [int(v) for v in vals[40]]
    assert check_r1cs(_flat("gl15").fp.q, _flat("gl15").constraints, sig40) is not None
    b = c.batch(B)
    b.set_witnesses(vals[:60])
    assert b.witnesses_missing() == 5
    for who, call in (("cw_select_instances", lambda: b.select()), ("cw_get_witnesses_at", lambda: b.witnesses_at([0, 1])),
                      ("cw_select_instances_device", lambda: b.select_device(0, 0, hip.sel_buf(B), hip.cnt)),
                      ("cw_get_witnesses_at_device", lambda: b.witnesses_at_device(hip.list, 2, hip.at_end(2 * nw * 32)))):
        with pytest.raises(rt.CwError) as e:
            call()
        assert e.value.code == CW_ESTATE and who in str(e.value) and "witnesses missing for 5 instances" in str(e.value)
    b.set_witnesses(vals[60:], first=60)
    assert b.witnesses_missing() == 0
    assert (b.select() == np.arange(B)).all()                     # before the check
    b.check_r1cs(); b.sync()
    st, fb = b.status(), b.r1cs_first_bad()
    assert (b.select(4, 4) == [40]).all() and (b.select() == np.delete(np.arange(B), 40)).all()
    image = np.zeros((B, nw, 32), dtype=np.uint8)
    image[:, :, :8] = vals.view(np.uint8).reshape(B, nw, 8)
    idx = np.array([40, 64, 0, 40], dtype=np.uint32)
    for entry0, n in ((0, nw), (3, 65)):
        _check_list(hip, b, image, idx, entry0, n, ebs=(32, 8))
    assert (b.status() == st).all() and (b.r1cs_first_bad() == fb).all() and b.witnesses_missing() == 0
    b.close()


@pytest.mark.gpu
def test_gpu_a_captured_graph_stays_captured(circuits, hip, monkeypatch):
    fc, c = circuits("gl15")
    bits, want = _case(15, "goldilocks")
    B = 65
    b = c.batch(B)
    img = np.zeros((B, c.n_inputs), dtype=np.uint64)
    img[:] = bits[:B]
    d_in = hip.upload(img)
    b.set_inputs_device_n8(d_in)
    for _ in range(3):
        b.run_check()
    b.sync()
    cap = b.graph_captured
    st = b.status()
    assert (b.select() == np.arange(B)).all() and (b.witnesses_at([64, 0]) == want[[64, 0]]).all()
    assert b.graph_captured == cap and (b.status() == st).all()
    b.run_check(); b.sync()
    assert b.graph_captured == cap and (b.select(0, 0) == np.arange(B)).all()
    b.close()
    hip.h.hipFree(d_in)
