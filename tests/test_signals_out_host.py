"""Signal columns out without a GPU: cw_get_signals_range(_device) and cw_sym_find (include/circom_amd.h).

On host-only batches (device = -1) of a bn128 circuit, a Goldilocks circuit and a bit-plane circuit every argument check is
reached in the order the header states - null, elem_bytes, the two ranges (no 32-bit wrap), the stride, the alignments of the
device form (CW_EINVAL) - and a well-formed call ends at CW_EDEVICE "host-only": the guard pointer 4096 is never dereferenced.
cw_sym_find is host-only altogether: a .sym file written by compile_program, and hand-written ones."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
from test_bitplane import BitGadget                                                   # noqa: E402
from test_input_columns import _host_circuit                                          # noqa: E402

from circom_amd.compiler import compile_program                                       # noqa: E402
from circom_amd.frontend.dsl import Program                                           # noqa: E402

CW_EIO, CW_EINVAL, CW_EINPUT, CW_EDEVICE, CW_ESTATE = -1, -2, -3, -4, -5
WIDTHS = (1, 2, 4, 8, 32)


def test_the_library_exports_the_signal_calls():
    from circom_amd import runtime as rt
    L = rt.lib()
    for name in ("cw_get_signals_range", "cw_get_signals_range_device", "cw_sym_find"):
        assert hasattr(L, name), name
    for name in ("signals_range", "signals_range_device"):
        assert hasattr(rt.Batch, name), name
    assert callable(rt.sym_find)


@pytest.mark.parametrize("kind", ["m2", "m2g", "bg15"])
def test_every_check_in_its_order(tmp_path, kind):
    from circom_amd import runtime as rt
    L = rt.lib()
    c = _host_circuit(tmp_path, kind)
    n_sig, B = c.n_signals, 3
    assert n_sig >= 4
    b = c.batch(B, device=-1)
    host = np.full(B * n_sig * 32 + 64, 0xA5, dtype=np.uint8)
    hp = C.c_void_p(host.ctypes.data)
    guard = C.c_void_p(4096)
    word = C.c_uint32(7)
    err = lambda: L.cw_last_error().decode()
    for fn, ok_ptr, wp in ((L.cw_get_signals_range, hp, C.byref(word)), (L.cw_get_signals_range_device, guard, C.c_void_p(8192))):
        dev = fn is L.cw_get_signals_range_device
        call = lambda s0, n, first, count, ptr, stride, eb, w=wp: fn(b.h, s0, n, first, count, ptr, stride, eb, w)
        # null
        assert fn(None, 0, 1, 0, 1, ok_ptr, 32, 32, wp) == CW_EINVAL and "null" in err()
        assert call(0, 1, 0, 1, None, 32, 32) == CW_EINVAL and "null" in err()
        # the width comes before the ranges
        for eb in (0, 3, 16, 64):
            assert call(n_sig, 1, B, 1, ok_ptr, 0, eb) == CW_EINVAL and "elem_bytes" in err(), eb
        # the ranges come before the stride; no 32-bit wrap
        assert call(n_sig, 1, 0, 1, ok_ptr, 0, 1) == CW_EINVAL and "signal range" in err()
        assert call(1, n_sig, 0, 1, ok_ptr, 0, 1) == CW_EINVAL and "signal range" in err()
        assert call(0xFFFFFFFF, 2, 0, 1, ok_ptr, 0, 1) == CW_EINVAL and "signal range" in err()
        assert call(2, 0xFFFFFFFF, 0, 1, ok_ptr, 0, 1) == CW_EINVAL and "signal range" in err()
        assert call(0, 1, B, 1, ok_ptr, 0, 1) == CW_EINVAL and "instance range" in err()
        assert call(0, 1, 1, B, ok_ptr, 0, 1) == CW_EINVAL and "instance range" in err()
        assert call(0, 1, 0xFFFFFFFF, 2, ok_ptr, 0, 1) == CW_EINVAL and "instance range" in err()
        assert call(0, 1, 2, 0xFFFFFFFF, ok_ptr, 0, 1) == CW_EINVAL and "instance range" in err()
        # a short stride (there is no broadcast form on the way out: 0 is short) comes before the alignments
        for eb in WIDTHS:
            bad_ptr = C.c_void_p(4096 + 1) if dev else ok_ptr
            assert call(1, 3, 0, B, bad_ptr, 3 * eb - 1, eb) == CW_EINVAL and "stride" in err() and "shorter" in err(), eb
            assert call(1, 3, 0, B, bad_ptr, 0, eb) == CW_EINVAL and "shorter" in err(), eb
        if dev:
            # each misalignment per width: the pointer, the stride, the word
            for eb in WIDTHS:
                a = 16 if eb == 32 else eb
                if a > 1:
                    assert call(1, 2, 0, B, C.c_void_p(4096 + a // 2), 4 * eb, eb) == CW_EINVAL and "aligned" in err(), eb
                    assert call(1, 2, 0, B, guard, 4 * eb + a // 2, eb) == CW_EINVAL and "multiple" in err(), eb
                assert call(1, 2, 0, B, guard, 4 * eb, eb, C.c_void_p(8192 + 2)) == CW_EINVAL and "word" in err(), eb
            assert call(1, 2, 0, B, C.c_void_p(4096 + 16), 64 + 16, 32) == CW_EDEVICE                    # 16, not 32, is what counts
        # then the device: well-formed calls, the empty ones included, with and without a word
        for eb in WIDTHS:
            assert call(0, n_sig, 0, B, ok_ptr, n_sig * eb, eb) == CW_EDEVICE and "host-only" in err(), eb
            assert call(1, 2, 1, 2, ok_ptr, 2 * eb + (16 if eb == 32 else eb), eb, None) == CW_EDEVICE and "host-only" in err(), eb
        assert call(0, 0, 0, B, ok_ptr, 0, 1) == CW_EDEVICE and call(0, 1, 0, 0, ok_ptr, 1, 1) == CW_EDEVICE
        assert call(n_sig, 0, B, 0, ok_ptr, 0, 8) == CW_EDEVICE                                        # empty ranges at the very end
        if not dev:
            assert call(0, 1, 0, 1, C.c_void_p(host.ctypes.data + 1), 35, 32) == CW_EDEVICE             # any alignment
    assert (host == 0xA5).all() and word.value == 7                                                     # nothing was written
    # the Python wrappers end at the same place
    with pytest.raises(rt.CwError) as e:
        b.signals_range(0, 2, elem_bytes=4)
    assert e.value.code == CW_EDEVICE
    with pytest.raises(rt.CwError) as e:
        b.signals_range_device(0, 2, 0, B, 4096, 8, 4)
    assert e.value.code == CW_EDEVICE
    with pytest.raises(rt.CwError) as e:
        b.signals_range(0, 2, elem_bytes=5)
    assert e.value.code == CW_EINVAL
    b.close(); c.close()


@pytest.mark.parametrize("prime", [None, "goldilocks"])
def test_hidden_log_values_are_not_addressable(tmp_path, prime):
    """a circuit with log() statements keeps the logged values in hidden slots behind its signals: the range ends at
    cw_n_signals, not at the end of the table"""
    from circom_amd import runtime as rt
    from circom_amd.circuits.basic import LogDemo
    L = rt.lib()
    cp = compile_program(Program(LogDemo(), prime=prime) if prime else Program(LogDemo()), str(tmp_path), "logdemo", sym=False)
    assert cp.flat.n_log_values == 8                                                                    # there ARE hidden slots
    c = rt.Circuit(cp.tape_path, cp.dat_path, cp.r1cs_path)
    assert L.cw_n_log_statements(c.h) == 7
    n_sig = L.cw_n_signals(c.h)
    assert n_sig == cp.flat.n_signals == c.n_signals
    b = c.batch(2, device=-1)
    err = lambda: L.cw_last_error().decode()
    for fn in (L.cw_get_signals_range, L.cw_get_signals_range_device):
        call = lambda s0, n: fn(b.h, s0, n, 0, 2, C.c_void_p(4096), n * 8, 8, None)
        assert call(0, n_sig + 1) == CW_EINVAL and "signal range" in err()
        assert call(n_sig, 1) == CW_EINVAL and "signal range" in err()
        assert call(n_sig - 1, 2) == CW_EINVAL and "signal range" in err()
        assert call(0, n_sig) == CW_EDEVICE and call(n_sig - 1, 1) == CW_EDEVICE and call(n_sig, 0) == CW_EDEVICE
    b.close(); c.close()


# ---- cw_sym_find -----------------------------------------------------------------------------------------------------------------
def _sym_lines(path):
    out = []
    for line in open(path).read().splitlines():
        s, _, _, nm = line.split(",", 3)
        out.append((int(s), nm))
    return out


def _expect(lines, name):
    ids = sorted({s for s, nm in lines if nm == name or nm.startswith(name + "[") or nm.startswith(name + ".")})
    return ids


def test_sym_find_on_a_compiled_circuit(tmp_path):
    from circom_amd import runtime as rt
    cp = compile_program(Program(BitGadget(15)), str(tmp_path), "bg15s", sym=True, strands=(1,), bits=True, jit=False)
    lines = _sym_lines(cp.sym_path)
    names = [nm for _, nm in lines]
    assert "main.out[0]" in names and "main.a[14]" in names and any(nm.startswith("main.x3.") for nm in names)
    # an array, one element, an input array, a sub-component prefix, one array of a sub-component
    sub_array = next(nm for nm in names if nm.startswith("main.x3.") and nm.endswith("[0]"))[:-3]
    for name, n in (("main.out", 17), ("main.out[3]", 1), ("main.a", 15), ("main.x3", None), (sub_array, None), ("main.sum.out[16]", 1)):
        ids = _expect(lines, name)
        assert ids and ids == list(range(ids[0], ids[0] + len(ids))), name                             # the test's own premise
        assert n is None or len(ids) == n
        assert rt.sym_find(cp.sym_path, name) == (ids[0], len(ids)), name
    assert rt.sym_find(cp.sym_path, "main.out") == (1, 17)                                             # the outputs follow the constant
    assert rt.sym_find(cp.sym_path, "main.a")[0] == cp.flat.main_input_start
    # a prefix of a NAME is not a prefix of the tree: main.o names nothing, main.out[1 not main.out[1] .. main.out[16]
    for missing in ("main.o", "main.out[1", "nobody", "main.out[17]", "main.", ""):
        with pytest.raises(rt.CwError) as e:
            rt.sym_find(cp.sym_path, missing)
        assert e.value.code == CW_EINPUT and str(e.value).endswith("Signal not found: " + missing), missing
    # "main" is every named signal: the file lists every signal behind the constant, so they are one run
    ids = _expect(lines, "main")
    assert ids == list(range(1, cp.flat.n_signals))
    assert rt.sym_find(cp.sym_path, "main") == (1, cp.flat.n_signals - 1)


def test_sym_find_errors(tmp_path):
    from circom_amd import runtime as rt
    L = rt.lib()
    s0, n = C.c_uint32(77), C.c_uint32(78)
    for args in ((None, b"x", C.byref(s0), C.byref(n)), (b"/nonexistent", None, C.byref(s0), C.byref(n)),
                 (b"/nonexistent", b"x", None, C.byref(n)), (b"/nonexistent", b"x", C.byref(s0), None)):
        assert L.cw_sym_find(*args) == CW_EINVAL
    # an unreadable file: a path that is not there, and a directory
    for path in (tmp_path / "absent.sym", tmp_path):
        with pytest.raises(rt.CwError) as e:
            rt.sym_find(path, "main.out")
        assert e.value.code == CW_EIO and str(path) in str(e.value)
    # hand-written: the matches of main.v have a gap at 6 (main.w sits there); lines without three commas are skipped; the order of
    # the lines does not matter, and a line listed twice counts once
    p = tmp_path / "gap.sym"
    p.write_text("1,1,0,main.out\n7,5,0,main.v[3]\n2,2,0,main.v[0]\n3,-1,0,main.v[1]\nnot a line\n4,3,0,main.v[2].x\n5,4,0,main.v[2].y\n"
                 "6,-1,0,main.w\n7,5,0,main.v[3]\n8,6,1,main.sub.in\n9,7,1,main.sub.out,with,commas\n")
    with pytest.raises(rt.CwError) as e:
        rt.sym_find(p, "main.v")
    assert e.value.code == CW_EINVAL and "2 .. 5" in str(e.value) and "6 does not" in str(e.value), str(e.value)
    assert rt.sym_find(p, "main.v[2]") == (4, 2)
    assert rt.sym_find(p, "main.v[3]") == (7, 1)
    assert rt.sym_find(p, "main.w") == (6, 1)
    assert rt.sym_find(p, "main.sub") == (8, 2)
    assert rt.sym_find(p, "main.sub.out,with,commas") == (9, 1)                                        # the name is everything behind the third comma
    assert rt.sym_find(p, "main") == (1, 9)
    assert (s0.value, n.value) == (77, 78)                                                             # a failed call writes neither
