"""Witness compare without a GPU (include/circom_amd.h: cw_compare_witnesses(_n8), cw_compare_witnesses_device(_n8),
cw_compare_wtns, cw_compare_wtns_many): the symbols and the Python forms exist; on host-only batches every CW_EINVAL case is
CW_EINVAL - both 32-bit wraps and each misalignment among them -, nothing is written, and only a call whose arguments are in order
reaches CW_EDEVICE; the file forms read and check their files before they look for the device, so a host-only batch tells a good
file from a bad one.  The HIP-free host part (circom_amd/csrc/cw_compare.h: checks, piece sizing, the CPU statement of the verdict)
is exercised by a stand-alone program (tests/host/compare_test.cpp) built with the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
from test_bitplane import BitGadget                                                  # noqa: E402

from circom_amd.circuits.basic import Multiplier2                                    # noqa: E402
from circom_amd.compiler import compile_program                                      # noqa: E402
from circom_amd.frontend.dsl import Program                                          # noqa: E402
from circom_amd.hip_elements.writers import wtns_bytes                              # noqa: E402
from oracle.field import PRIMES                                                      # noqa: E402

ROOT = Path(__file__).resolve().parents[1]
CW_EIO, CW_EINVAL, CW_EDEVICE = -1, -2, -4
SYMBOLS = ("cw_compare_witnesses", "cw_compare_witnesses_n8", "cw_compare_witnesses_device", "cw_compare_witnesses_device_n8",
           "cw_compare_wtns", "cw_compare_wtns_many")


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def test_the_library_exports_the_six_symbols():
    from circom_amd import runtime as rt
    L = rt.lib()
    for name in SYMBOLS:
        assert hasattr(L, name) and name in rt._SIGS, name
    for name in ("compare_witnesses", "compare_witnesses_device", "compare_wtns", "compare_wtns_many"):
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
    from circom_amd import runtime as rt
    L = rt.lib()
    c = _host_circuit(tmp_path, kind)
    nw, B = c.n_witness, 5
    assert nw >= 4
    b = c.batch(B, device=-1)
    err = lambda: L.cw_last_error().decode()
    eb = c.element_bytes
    assert eb == (8 if kind == "m2g" else 32)
    image = np.zeros((B, nw, 32), dtype=np.uint8)
    diff = np.full(B, 0xA5A5A5A5, dtype=np.uint32)
    summary = np.full(2, 0xA5A5A5A5, dtype=np.uint32)
    # host forms
    for fn in (L.cw_compare_witnesses, L.cw_compare_witnesses_n8):
        ok = (b.h, 0, nw, 0, B, _ptr(image), _ptr(diff), _ptr(summary))
        call = lambda k=None, v=None: fn(*[v if i == k else a for i, a in enumerate(ok)])
        assert call(0, None) == CW_EINVAL and call(5, None) == CW_EINVAL and call(6, None) == CW_EINVAL      # null batch / image / diff
        assert call(2, nw + 1) == CW_EINVAL and "entry range" in err()                                         # entries past the witness list
        assert call(1, nw) == CW_EINVAL and call(1, 1) == CW_EINVAL
        assert call(2, 0xFFFFFFFF) == CW_EINVAL and fn(b.h, 2, 0xFFFFFFFF, 0, B, _ptr(image), _ptr(diff), _ptr(summary)) == CW_EINVAL
        assert call(1, 0xFFFFFFFF) == CW_EINVAL                                                                # entry0 + n wraps in 32 bits
        assert call(4, B + 1) == CW_EINVAL and "instance range" in err()                                       # instances past the batch
        assert call(3, B) == CW_EINVAL and call(3, 1) == CW_EINVAL
        assert call(4, 0xFFFFFFFF) == CW_EINVAL and fn(b.h, 0, nw, 2, 0xFFFFFFFF, _ptr(image), _ptr(diff), _ptr(summary)) == CW_EINVAL
        assert call(3, 0xFFFFFFFF) == CW_EINVAL                                                                # first + count wraps in 32 bits
        assert call() == CW_EDEVICE                                                                            # only a call in order
        assert call(7, None) == CW_EDEVICE                                                                     # the summary is optional
        assert fn(b.h, 1, 2, 1, 3, _ptr(image), _ptr(diff), _ptr(summary)) == CW_EDEVICE
        assert fn(b.h, nw, 0, B, 0, _ptr(image), _ptr(diff), _ptr(summary)) == CW_EDEVICE                      # empty ranges at the end
    # device forms: the image 16-byte aligned for 32-byte elements, 8-byte aligned for the 8-byte element of the 64-bit runtime
    d = lambda a: C.c_void_p(a)
    for fn, align in ((L.cw_compare_witnesses_device, 16), (L.cw_compare_witnesses_device_n8, 8 if eb == 8 else 16)):
        ok = (b.h, 0, nw, 0, B, d(1 << 20), d(8192), d(4096))
        call = lambda k=None, v=None: fn(*[v if i == k else a for i, a in enumerate(ok)])
        assert call(0, None) == CW_EINVAL and call(5, None) == CW_EINVAL and call(6, None) == CW_EINVAL
        assert call(2, nw + 1) == CW_EINVAL and call(1, nw) == CW_EINVAL and call(2, 0xFFFFFFFF) == CW_EINVAL and call(1, 0xFFFFFFFF) == CW_EINVAL
        assert call(4, B + 1) == CW_EINVAL and call(3, B) == CW_EINVAL and call(4, 0xFFFFFFFF) == CW_EINVAL and call(3, 0xFFFFFFFF) == CW_EINVAL
        assert call(5, d((1 << 20) + align // 2)) == CW_EINVAL and "%d-byte aligned" % align in err()          # each misalignment
        assert call(5, d((1 << 20) + 4)) == CW_EINVAL and call(5, d((1 << 20) + 1)) == CW_EINVAL
        assert call(6, d(8194)) == CW_EINVAL and "d_diff" in err() and call(6, d(8193)) == CW_EINVAL
        assert call(7, d(4098)) == CW_EINVAL and "d_summary" in err() and call(7, d(4097)) == CW_EINVAL
        assert call(4, B + 1) == CW_EINVAL and "instance range" in err()                                       # the ranges come before the alignments
        assert fn(b.h, 0, nw, 0, B + 1, d((1 << 20) + 1), d(8192), d(4096)) == CW_EINVAL and "instance range" in err()
        assert call() == CW_EDEVICE
        assert call(7, None) == CW_EDEVICE
        assert call(5, d((1 << 20) + align)) == CW_EDEVICE and call(6, d(8196)) == CW_EDEVICE and call(7, d(4100)) == CW_EDEVICE
    assert (diff == 0xA5A5A5A5).all() and (summary == 0xA5A5A5A5).all()                                        # nothing was written
    # the Python forms
    with pytest.raises(rt.CwError) as e:
        b.compare_witnesses(image[:, :2], entry0=nw - 1)
    assert e.value.code == CW_EINVAL
    with pytest.raises(rt.CwError) as e:
        b.compare_witnesses(image, first=1)
    assert e.value.code == CW_EINVAL
    for call in (lambda: b.compare_witnesses(image), lambda: b.compare_witnesses(image[:0]), lambda: b.compare_witnesses(image[:, :, :eb]),
                 lambda: b.compare_witnesses_device(1 << 20, 8192, 0, B), lambda: b.compare_witnesses_device(1 << 20, 8192, 0, B, d_summary=4096, n8=True)):
        with pytest.raises(rt.CwError) as e:
            call()
        assert e.value.code == CW_EDEVICE
    b.close(); c.close()


@pytest.mark.parametrize("kind", ["m2", "m2g", "bg15"])
def test_file_forms_check_their_files_before_the_device(tmp_path, kind):
    """arguments, files, device: a truncated file and a file of another prime are CW_EIO with the path and the reason on a
    host-only batch, a good file reaches CW_EDEVICE"""
    from circom_amd import runtime as rt
    L = rt.lib()
    c = _host_circuit(tmp_path, kind)
    nw, B = c.n_witness, 3
    b = c.batch(B, device=-1)
    err = lambda: L.cw_last_error().decode()
    q = c.q
    other = PRIMES["bls12381"] if kind != "m2g" else q - 58                  # the same n8, another number
    assert other != q and (other.bit_length() + 63) // 64 == (q.bit_length() + 63) // 64
    good = wtns_bytes(q, [1] + [0] * (nw - 1))
    for i in range(B):
        (tmp_path / ("good_%d.wtns" % i)).write_bytes(good)
        (tmp_path / ("cut_%d.wtns" % i)).write_bytes(good if i != 1 else good[:-1])
        (tmp_path / ("prime_%d.wtns" % i)).write_bytes(good if i != 2 else wtns_bytes(other, [1] + [0] * (nw - 1)))
    enc = lambda name: os.fsencode(str(tmp_path / name))
    diff = np.full(B, 0xA5A5A5A5, dtype=np.uint32)
    summary = np.full(2, 0xA5A5A5A5, dtype=np.uint32)
    # arguments
    assert L.cw_compare_wtns(None, 0, enc("good_0.wtns"), _ptr(diff)) == CW_EINVAL
    assert L.cw_compare_wtns(b.h, 0, None, _ptr(diff)) == CW_EINVAL and L.cw_compare_wtns(b.h, 0, enc("good_0.wtns"), None) == CW_EINVAL
    assert L.cw_compare_wtns(b.h, B, enc("good_0.wtns"), _ptr(diff)) == CW_EINVAL and L.cw_compare_wtns(b.h, 0xFFFFFFFF, enc("good_0.wtns"), _ptr(diff)) == CW_EINVAL
    many = L.cw_compare_wtns_many
    assert many(None, 0, B, enc("good_%d.wtns"), _ptr(diff), _ptr(summary)) == CW_EINVAL
    assert many(b.h, 0, B, None, _ptr(diff), _ptr(summary)) == CW_EINVAL and many(b.h, 0, B, enc("good_%d.wtns"), None, _ptr(summary)) == CW_EINVAL
    assert many(b.h, 0, B + 1, enc("good_%d.wtns"), _ptr(diff), _ptr(summary)) == CW_EINVAL
    assert many(b.h, 2, 0xFFFFFFFF, enc("good_%d.wtns"), _ptr(diff), _ptr(summary)) == CW_EINVAL
    assert many(b.h, 0, B, enc("good.wtns"), _ptr(diff), _ptr(summary)) == CW_EINVAL and "%u / %d" in err()
    assert many(b.h, 0, B, enc("good_%d_%d.wtns"), _ptr(diff), _ptr(summary)) == CW_EINVAL
    assert many(b.h, 0, B, enc("good_%s.wtns"), _ptr(diff), _ptr(summary)) == CW_EINVAL
    # files
    assert L.cw_compare_wtns(b.h, 0, enc("missing.wtns"), _ptr(diff)) == CW_EIO and "missing.wtns" in err()
    assert L.cw_compare_wtns(b.h, 0, enc("cut_1.wtns"), _ptr(diff)) == CW_EIO and "cut_1.wtns" in err() and "longer than the file" in err()
    assert L.cw_compare_wtns(b.h, 1, enc("prime_2.wtns"), _ptr(diff)) == CW_EIO and "prime_2.wtns" in err() and "the prime differs" in err()
    assert many(b.h, 0, B, enc("cut_%d.wtns"), _ptr(diff), _ptr(summary)) == CW_EIO and "cut_1.wtns" in err() and "longer than the file" in err()
    assert many(b.h, 0, B, enc("prime_%u.wtns"), _ptr(diff), _ptr(summary)) == CW_EIO and "prime_2.wtns" in err() and "the prime differs" in err()
    # device: good files, and ranges that end before the bad one
    assert L.cw_compare_wtns(b.h, 2, enc("good_0.wtns"), _ptr(diff)) == CW_EDEVICE
    assert many(b.h, 0, B, enc("good_%d.wtns"), _ptr(diff), _ptr(summary)) == CW_EDEVICE
    assert many(b.h, 0, B, enc("good_%d.wtns"), _ptr(diff), None) == CW_EDEVICE
    assert many(b.h, 0, 1, enc("cut_%d.wtns"), _ptr(diff), _ptr(summary)) == CW_EDEVICE
    assert many(b.h, 0, 2, enc("prime_%d.wtns"), _ptr(diff), _ptr(summary)) == CW_EDEVICE
    assert (diff == 0xA5A5A5A5).all() and (summary == 0xA5A5A5A5).all()
    with pytest.raises(rt.CwError) as e:
        b.compare_wtns(0, tmp_path / "cut_1.wtns")
    assert e.value.code == CW_EIO and "cut_1.wtns" in str(e.value)
    with pytest.raises(rt.CwError) as e:
        b.compare_wtns_many(0, B, str(tmp_path / "good_%d.wtns"))
    assert e.value.code == CW_EDEVICE
    b.close(); c.close()


def test_compare_header_under_the_sanitizers(tmp_path):
    exe = tmp_path / "compare_test"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", str(ROOT / "tests" / "host" / "compare_test.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "compare ok: " in r.stdout
