"""Signal columns out on the GPU: cw_get_signals_range(_device) (include/circom_amd.h) - the signals signal0 .. signal0 + n - 1
(signal ids, whether the witness list names them or not) of the instances first .. first + count - 1 as rows of little-endian
elements of 1, 2, 4, 8 or 32 bytes at values + j * stride; only the n * elem_bytes bytes of a row are written, and a value that
does not fit is stored as its low bytes and reported through one word (the lowest such instance).

Expected values never come from another egress of the library: they come from the circuit's flat code evaluated by
oracle.tape_eval.eval_flat (test_input_columns._oracle_of), narrowed here.  A byte-for-byte comparison with b.witnesses() while
the witness list names every signal is a second assertion.

The circuits: Widths - one-byte inputs a[40], their two-byte products p, four-byte q, eight-byte r and sixteen-byte s (169
signals), bn128 with canonical and with Montgomery-form tables and Goldilocks (the 64-bit runtime) - and BitGadget(15) (380
signals) for the bit-plane engine, interpreted and emitted.  The kernels' signal tile T is 64, and 16 for 32-byte elements of
the 8 x u32 table.

More than 65 535 instance tiles in one call (the cw_pieces split of the launchers) is not a few-seconds test and no hook lowers
the piece size: that walk is the host-side arithmetic of csrc/cw_pieces.h, which tests/test_pieces_host.py pins."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
from test_bitplane import BitGadget                                                   # noqa: E402
from test_goldilocks_egress import _badsquare                                         # noqa: E402
from test_input_columns import _Dev, _bit_case, _oracle_of                             # noqa: E402

from circom_amd.compiler import compile_program                                       # noqa: E402
from circom_amd.frontend.dsl import Program, template                                 # noqa: E402
from circom_amd.frontend.flatten import flatten                                       # noqa: E402

CW_EINVAL, CW_EDEVICE, CW_ESTATE = -2, -4, -5
WIDTHS = (1, 2, 4, 8, 32)
NONE = 0xFFFFFFFF
B_MAX = 300
VALUE_KINDS = ("canon", "mont", "gl")
BIT_KINDS = ("interp", "jit")


@template
def Widths(c):
    a = c.input("a", 40)
    s = c.output("s", 8)
    p = c.signal("p", 40)
    q = c.signal("q", 40)
    r = c.signal("r", 40)
    for k in range(40):
        c.set(p[k], a[k] * a[(k + 1) % 40])
    for k in range(40):
        c.set(q[k], p[k] * p[(k + 1) % 40])
    for k in range(40):
        c.set(r[k], q[k] * q[(k + 1) % 40])
    for k in range(8):
        c.set(s[k], r[k] * r[k + 1])


def _prog(kind):
    if kind == "gl":
        return Program(Widths(), prime="goldilocks")
    if kind in BIT_KINDS:
        return Program(BitGadget(15))
    return Program(Widths())


@functools.lru_cache(maxsize=None)
def _case(kind):
    """(flat circuit, inputs [300][n_inputs] of integers, expected signals [300][n_signals][32]): computed once, never modified.
    Widths: every third instance has inputs 0 / 1 - every signal fits one byte -, the others bytes 1 .. 255."""
    fc = flatten(_prog(kind))
    if kind in BIT_KINDS:
        bits, want = _bit_case()[:2]
        return fc, bits, want
    rng = np.random.default_rng(31)
    ins = rng.integers(1, 256, size=(B_MAX, 40), dtype=np.uint16)
    ins[::3] = rng.integers(0, 2, size=ins[::3].shape)
    ins[1] = 255
    ins.setflags(write=False)
    return fc, ins, _oracle_of(fc, ins.tolist())


def _narrow(want, s0, n, first, count, W):
    """(expected bytes [count][n][W], expected word) of the oracle's signals"""
    part = want[first:first + count, s0:s0 + n]
    wide = part[:, :, W:].reshape(count, -1).any(axis=1)
    return part[:, :, :W], (first + int(np.argmax(wide)) if wide.any() else NONE)


@pytest.fixture(scope="module")
def hip():
    return _Dev()


@pytest.fixture(scope="module")
def circuits(tmp_path_factory):
    """(kind, witness list) -> runtime circuit, compiled once; list None = every signal, else the signals below it"""
    from circom_amd import runtime as rt
    made, compiled = {}, {}

    def get(kind, short=None):
        if (kind, short) not in made:
            name = "bits" if kind in BIT_KINDS else kind
            if name not in compiled:
                d = str(tmp_path_factory.mktemp("sig_" + name))
                if name == "bits":
                    compiled[name] = compile_program(_prog(kind), d, name, sym=False, strands=(1,), bits=True, jit=True)
                    assert compiled[name].jit is not None
                elif name == "gl":
                    compiled[name] = compile_program(_prog(kind), d, name, sym=False)
                else:
                    compiled[name] = compile_program(_prog(kind), d, name, sym=False, mont=(name == "mont"))
            cp = compiled[name]
            c = rt.Circuit(cp.tape_path, cp.dat_path, cp.r1cs_path)
            c.set_witness_list(np.arange(c.n_signals if short is None else short, dtype=np.uint32))
            assert c.n_signals == cp.flat.n_signals == _case(kind)[0].n_signals
            if name in ("canon", "mont"):
                assert c.montgomery == (name == "mont") and c.element_bytes == 32
            made[kind, short] = c
        return made[kind, short]

    yield get
    for c in made.values():
        c.close()


def _ran(c, kind, B, monkeypatch, rows=None):
    """a batch of the first B instances of the kind's case (or of `rows`) that has run"""
    if kind in BIT_KINDS:
        monkeypatch.setenv("CW_BITS_JIT", "1" if kind == "jit" else "0")
    ins = _case(kind)[1][:B] if rows is None else rows
    b = c.batch(B)
    if kind in BIT_KINDS:
        assert b.bitmode and b.jit == (kind == "jit")
    else:
        assert not b.bitmode
    b.set_inputs([[int(v) for v in row] for row in ins])
    b.run(); b.sync()
    return b


def _get(b, hip, form, s0, n, first, count, W, want_word=True):
    """the call in one of its two forms into an image prefilled with 0xA5; the bytes outside the values are checked here.
    host: 5 pad bytes per row.  device: the stride padded to the next allowed multiple, the image ENDS where its allocation
    ends, behind a 4 096-byte guard in front.  Returns (values [count][n][W], word or None)."""
    from circom_amd import runtime as rt
    L = rt.lib()
    row = n * W
    if form == "host":
        stride = row + 5
        buf = np.full(max((count - 1) * stride + row, 1), 0xA5, dtype=np.uint8)
        word = C.c_uint32(12345)
        rc = L.cw_get_signals_range(b.h, s0, n, first, count, buf.ctypes.data_as(C.c_void_p), stride, W, C.byref(word) if want_word else None)
        assert rc == 0, L.cw_last_error()
        got_word = word.value if want_word else None
    else:
        stride = row + (16 if W == 32 else W)
        img = np.full(max((count - 1) * stride + row, 16), 0xA5, dtype=np.uint8)
        base, p = hip.at_end(img)
        d_word = hip.upload(np.array([12345], dtype=np.uint32)) if want_word else 0
        b.signals_range_device(s0, n, first, count, p, stride, W, d_word)
        b.sync()
        whole = hip.download(base, 4096 + img.size)
        assert (whole[:4096] == 0xA5).all(), "the guard in front of the image was written"
        buf = whole[4096:]
        got_word = int(hip.download(d_word, 1, np.uint32)[0]) if want_word else None
        hip.h.hipFree(base)
        if want_word:
            hip.h.hipFree(d_word)
    if count == 0 or n == 0:
        assert (buf == 0xA5).all()
        return np.zeros((count, n, W), dtype=np.uint8), got_word
    rows = np.full((count, stride), 0xA5, dtype=np.uint8)
    rows.reshape(-1)[:(count - 1) * stride + row] = buf[:(count - 1) * stride + row]
    assert (buf[(count - 1) * stride + row:] == 0xA5).all()
    assert (rows[:, row:] == 0xA5).all(), "pad bytes of a row were written"
    return rows[:, :row].reshape(count, n, W), got_word


def _check(b, hip, form, want, s0, n, first, count, W, what):
    got, word = _get(b, hip, form, s0, n, first, count, W)
    exp, exp_word = _narrow(want, s0, n, first, count, W)
    bad = np.argwhere((got != exp).any(axis=2))
    assert len(bad) == 0, "%s: first differences at (row, value): %s" % (what, bad[:8].tolist())
    assert word == exp_word, (what, word, exp_word)


def _ranges(B):
    """the whole batch, and an inner range that starts and ends off a multiple of 64"""
    out = [(0, B)]
    if B == 300:
        out.append((70, 150))
    elif B >= 3:
        out.append((1, B - 2))
    return out


def _tile(kind, W):
    return 16 if W == 32 and kind in ("canon", "mont") else 64


# ---- tile edges, untouched bytes, every width, every engine ---------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("B", [1, 63, 64, 65, 300])
@pytest.mark.parametrize("kind", VALUE_KINDS + BIT_KINDS)
def test_gpu_signals_at_the_tile_edges(circuits, hip, monkeypatch, kind, B, form):
    c = circuits(kind)
    fc, _, want = _case(kind)
    n_sig = fc.n_signals
    b = _ran(c, kind, B, monkeypatch)
    for W in WIDTHS:
        T = _tile(kind, W)
        assert n_sig >= 5 + 2 * T + 3
        for n in (1, T - 1, T, T + 1, 2 * T + 3):
            s0 = n_sig - n if n == T + 1 else 5                       # off a multiple of T; one range ends at cw_n_signals
            assert s0 % T != 0
            for first, count in _ranges(B):
                _check(b, hip, form, want, s0, n, first, count, W, (kind, B, form, W, n, first, count))
    # the second assertion: while the witness list names every signal, the 32-byte columns ARE the bulk image
    got, _ = _get(b, hip, form, 0, n_sig, 0, B, 32)
    assert got.tobytes() == b.witnesses().tobytes()
    b.close()


# ---- too wide ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", VALUE_KINDS)
def test_gpu_too_wide_is_the_lowest_instance(circuits, hip, monkeypatch, kind):
    """p = a a' needs two bytes, q four, r eight, s sixteen (bn128): the word at the width below is the lowest instance of the
    range whose value does not fit, at the width itself 0xFFFFFFFF; the low bytes leave either way"""
    c = circuits(kind)
    fc, _, want = _case(kind)
    B, first, count = 65, 3, 60
    cases = [(1, 2, 49, 40), (2, 4, 89, 40), (4, 8, 129, 40)]       # (width, the next one up, signal0, n): p, q, r
    if kind != "gl":
        cases.append((8, 32, 1, 8))                                   # s; a Goldilocks residue always fits eight bytes
    # the premise, on the oracle's values, before the GPU is touched
    for W, up, s0, n in cases:
        wide = want[first:first + count, s0:s0 + n, W:].reshape(count, -1).any(axis=1)
        assert wide.any() and not wide.all() and not wide[0], (kind, W)
        assert _narrow(want, s0, n, first, count, W)[1] == first + int(np.argmax(wide)) > first
        assert _narrow(want, s0, n, first, count, up)[1] == NONE
    b = _ran(c, kind, B, monkeypatch)
    for W, up, s0, n in cases:
        words = []
        for form in ("host", "device"):
            got, word = _get(b, hip, form, s0, n, first, count, W)
            exp, exp_word = _narrow(want, s0, n, first, count, W)
            assert (got == exp).all() and word == exp_word, (kind, form, W, word, exp_word)      # the value mod 2^(8 W)
            words.append(word)
            _check(b, hip, form, want, s0, n, first, count, up, (kind, form, up))                # 0xFFFFFFFF at the next width up
            got, none = _get(b, hip, form, s0, n, first, count, W, want_word=False)              # a NULL word is accepted
            assert none is None and (got == exp).all()
        assert words[0] == words[1]
        # a range of instances that all fit reports nothing: the word is about the range, not the batch
        assert _narrow(want, s0, n, 3, 1, W)[1] == NONE
        _check(b, hip, "device", want, s0, n, 3, 1, W, (kind, W, "one instance"))
    b.close()


# ---- bit-plane batches: the re-run instances come from the side batch ------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("engine", BIT_KINDS)
def test_gpu_bitplane_rerun_rows_are_the_side_batch(circuits, hip, monkeypatch, engine, form):
    """a[5] = 7 in the instances 0, 64 and 299: their rows are the oracle's residues (reported at one byte where they exceed
    it), every other row is bits"""
    c = circuits(engine)
    fc = _case(engine)[0]
    _, _, odd, want_odd = _bit_case()
    B = B_MAX
    hot = want_odd[[0, 64, 299]]
    assert (hot[:, :, 0] > 1).any() or hot[:, :, 1:].any()                                      # not bits
    plain = np.delete(want_odd, [0, 64, 299], axis=0)
    assert not plain[:, :, 1:].any() and (plain[:, :, 0] <= 1).all()
    b = _ran(c, engine, B, monkeypatch, rows=odd)
    for W in WIDTHS:
        for s0, n in ((5, 131), (0, fc.n_signals), (fc.main_input_start + 5, 1)):
            for first, count in ((0, B), (1, B - 1), (64, 1), (65, 234), (200, 100)):
                _check(b, hip, form, want_odd, s0, n, first, count, W, (engine, form, W, s0, n, first, count))
    b.close()


# ---- signals the witness list does not hold ---------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["canon", "interp"])
def test_gpu_signals_outside_the_witness_list(circuits, hip, monkeypatch, kind):
    fc, _, want = _case(kind)
    short = fc.main_input_start + fc.n_main_inputs                                              # constant, outputs, inputs
    c = circuits(kind, short)
    assert c.n_witness == short < c.n_signals
    B = 65
    b = _ran(c, kind, B, monkeypatch)
    assert b.witnesses().shape[1] == short
    for W in (2, 32):
        for form in ("host", "device"):
            _check(b, hip, form, want, short + 3, 70, 1, 63, W, (kind, form, W))
            _check(b, hip, form, want, short - 4, 9, 0, B, W, (kind, form, W, "across the end of the list"))
    b.close()


# ---- the supplied-witness state (64-bit runtime) ------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_supplied_state(circuits, hip):
    from circom_amd import runtime as rt
    fc, _, want = _case("gl")
    short = 60
    c = circuits("gl", short)
    B = 65
    rows = np.ascontiguousarray(want[:B, :short, :8]).reshape(B, short * 8).view("<u8")
    b = c.batch(B)
    with pytest.raises(rt.CwError) as e:
        b.signals_range(1, 4, elem_bytes=8)
    assert e.value.code == CW_ESTATE and "before cw_run" in str(e.value)
    b.set_witnesses(rows[:40])
    assert b.witnesses_missing() == B - 40
    with pytest.raises(rt.CwError) as e:
        b.signals_range(1, 4, elem_bytes=8)
    assert e.value.code == CW_ESTATE and "witnesses missing for %d instances" % (B - 40) in str(e.value)
    b.set_witnesses(rows[40:], first=40)
    assert b.witnesses_missing() == 0
    for form in ("host", "device"):
        for W in (1, 8, 32):
            _check(b, hip, form, want, 5, 50, 1, 63, W, ("supplied", form, W))
            _check(b, hip, form, want, 0, short, 0, B, W, ("supplied, the whole list", form, W))
    for s0, n in ((50, 11), (short, 1), (0, fc.n_signals)):
        with pytest.raises(rt.CwError) as e:
            b.signals_range(s0, n, elem_bytes=8)
        assert e.value.code == CW_ESTATE and "no witness program has run" in str(e.value)
        with pytest.raises(rt.CwError) as e:
            b.signals_range_device(s0, n, 0, B, 4096, n * 8, 8)                                 # the pointer is never touched
        assert e.value.code == CW_ESTATE and "no witness program has run" in str(e.value)
    assert b.witnesses_missing() == 0
    b.close()


# ---- the calls only read -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["mont", "gl"])
def test_gpu_nothing_is_disturbed(circuits, hip, kind):
    c = circuits(kind)
    fc, ins, want = _case(kind)
    B = 65
    b = c.batch(B)
    b.set_inputs([[int(v) for v in row] for row in ins[:B]])
    for _ in range(3):
        b.run_check(); b.sync()
    assert b.graph_captured
    before = (b.status().copy(), b.r1cs_first_bad().copy(), b.graph_captured)
    for form in ("host", "device"):
        _check(b, hip, form, want, 5, 131, 1, 63, 2, (kind, form))
        _check(b, hip, form, want, 0, fc.n_signals, 0, B, 32, (kind, form))
    after = (b.status(), b.r1cs_first_bad(), b.graph_captured)
    assert (before[0] == after[0]).all() and (before[1] == after[1]).all() and before[2] == after[2]
    b.run_check(); b.sync()
    assert b.graph_captured and (b.status() == before[0]).all()
    _check(b, hip, "device", want, 5, 131, 1, 63, 4, (kind, "after the replay"))
    b.close()


# ---- empty calls -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["canon", "gl", "interp"])
def test_gpu_empty_calls(circuits, hip, monkeypatch, kind):
    c = circuits(kind)
    fc = _case(kind)[0]
    B = 65
    b = _ran(c, kind, B, monkeypatch)
    for form in ("host", "device"):
        for s0, n, first, count in ((3, 0, 0, B), (3, 5, 7, 0), (fc.n_signals, 0, B, 0)):
            got, word = _get(b, hip, form, s0, n, first, count, 4)                              # (_get asserts that no byte was written)
            assert word == NONE
            _get(b, hip, form, s0, n, first, count, 32, want_word=False)
    b.close()


# ---- cw_explain reads the .sym file through the shared walk ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_explain_is_unchanged_by_the_shared_sym_walk(tmp_path):
    """the whole text of cw_explain for a violated constraint, rebuilt here from the .sym file and the inputs: out <-- a^2 +
    (a & 1) against the row a * a = out"""
    from circom_amd import runtime as rt
    from test_goldilocks_egress import Q
    cp = _badsquare(tmp_path, sym=True)
    c = rt.Circuit(cp.tape_path, cp.dat_path, cp.r1cs_path)
    names = {}
    for line in open(cp.sym_path).read().splitlines():
        s, _, _, nm = line.split(",", 3)
        names[int(s)] = nm
    assert rt.sym_find(cp.sym_path, names[1]) == (1, 1)
    ins = [7, 10, Q - 2]
    b = c.batch(len(ins))
    b.set_inputs([[x] for x in ins])
    b.run(); b.check_r1cs(); b.sync()
    for i, x in enumerate(ins):
        with_names, without = b.explain(i, cp.sym_path), b.explain(i)
        if not x & 1:
            assert with_names == without == "instance %d: ok\n" % i
            continue
        value = {1: (x * x + 1) % Q, cp.flat.main_input_start: x, 0: 1}
        lines = with_names.splitlines()
        assert lines[0] == "instance %d: constraint 0 of the .r1cs is violated: A*B - C != 0 with" % i and len(lines) == 4
        for part, line, bare in zip("ABC", lines[1:], without.splitlines()[1:]):
            assert line.startswith("  %s:" % part)
            terms = [t for t in line[4:].split(";") if t.strip()]
            bare_terms = [t for t in bare[4:].split(";") if t.strip()]
            assert len(terms) == len(bare_terms) >= 1
            for t, u in zip(terms, bare_terms):
                nm, val = t.strip().split(" = ")
                sig = 0 if nm == "one" else next(s for s, v in names.items() if v == nm)       # a name of the file, never "signal N"
                assert int(val) == value[sig]
                assert u.strip() == ("one" if sig == 0 else "signal %d" % sig) + " = " + val
    b.close(); c.close()
