"""Supplied witnesses on the 64-bit runtime (`--prime goldilocks`): cw_set_witnesses(_n8)(_device)(_n8), cw_read_wtns(_many),
cw_witnesses_missing and `cw_witness --check` - witnesses this batch did not compute go INTO the value table (csrc/cw64.hip
cw64_transpose_in_kernel<EB, true>, the bulk egress transpose the other way, scattering through the witness list) and cw_check_r1cs,
cw_explain and every egress work on them.

Expected values come from the reference's own 64-bit runtime (tests/golden/reference_wtns_goldilocks.json) or from the oracle
(oracle.tape_eval eval_flat / check_r1cs), never from another call into the library.  The shapes are the ones the kernel can go
wrong at: 1 / 63 / 64 / 65 / 300 instances on a witness of 17 tiles + 20 entries, ranges whose `first` is no multiple of 64, a
witness narrower than a tile at 70 001 instances, a witness list that is far from the identity, malformed values at the first
and last lane and row of a tile."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
from make_golden import goldilocks_cases                                            # noqa: E402

from circom_amd.compiler import compile_program                                      # noqa: E402
from circom_amd.frontend.dsl import Program, template                                # noqa: E402
from circom_amd.hip_elements.writers import wtns_bytes                              # noqa: E402
from oracle.tape_eval import eval_flat, check_r1cs                                   # noqa: E402

GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "reference_wtns_goldilocks.json")))["cases"]
CASES = goldilocks_cases()
Q = 18446744069414584321
CW_EIO, CW_EINVAL, CW_EDEVICE, CW_ESTATE = -1, -2, -4, -5
BAD, R1CS = 8, 4
GUARD = 4096
ONLY64 = "supplied witnesses are served by the 64-bit runtime only (--prime goldilocks)"


def _circuit(tmp_path, name, sym=False):
    from circom_amd import runtime as rt
    cp = compile_program(CASES[name][0](), str(tmp_path), name, sym=sym)
    return cp, rt.Circuit(cp.tape_path, cp.dat_path, cp.r1cs_path)


def _oracle():
    """Poseidon(2) over Goldilocks x 300: (input rows, [instance][signal] uint64, read-only), computed once per process and
    shared with tests/test_goldilocks_egress.py"""
    from test_goldilocks_egress import _poseidon_oracle
    return _poseidon_oracle()


def _raises(code, text, call):
    from circom_amd import runtime as rt
    with pytest.raises(rt.CwError) as e:
        call()
    assert e.value.code == code and text in str(e.value), str(e.value)


def _wide(img64):
    """[n][n_witness] uint64 -> the 32-byte form [n][n_witness][4] (upper words zero)"""
    out = np.zeros(img64.shape + (4,), dtype="<u8")
    out[:, :, 0] = img64
    return out


def _set_host32(b, first, img):
    from circom_amd import runtime as rt
    img = np.ascontiguousarray(img)
    rt._chk(rt.lib().cw_set_witnesses(b.h, first, img.shape[0], img.ctypes.data_as(C.c_void_p)))


def _set_device(b, hip, first, img, eb):
    """the image sits at the very END of a device allocation sized to the byte, behind a guard of 0xA5 bytes (a value that
    would pass as a canonical residue: read as data it would land in the table and show in the egress).  hipMalloc rounds
    allocations up, so a read past the end would not fault - it would read what the allocator left there; only the guard in
    front and the comparison of the whole table image afterwards can show a wrong read.  No fault is provoked."""
    raw = np.ascontiguousarray(img).view(np.uint8).reshape(-1)
    assert raw.size == img.shape[0] * img.shape[1] * eb
    buf = np.full(GUARD + raw.size, 0xA5, dtype=np.uint8)
    buf[GUARD:] = raw
    p = hip.upload(buf)
    (b.set_witnesses_device_n8 if eb == 8 else b.set_witnesses_device)(first, img.shape[0], p + GUARD)
    b.sync()                                                       # the buffer may go once the stream has passed the call
    hip.h.hipFree(p)


def _table_n8(b, hip, n_witness):
    """the whole batch as [batch][n_witness] uint64 through cw_get_witnesses_device_n8"""
    p = hip.alloc(b.n * n_witness * 8)
    b.witnesses_device_n8(0, b.n, p)
    b.sync()
    out = hip.download(p, (b.n * n_witness * 8,)).view("<u8").reshape(b.n, n_witness)
    hip.h.hipFree(p)
    return out


# ---- without a GPU -----------------------------------------------------------------------------------------------------------
def test_argument_state_and_file_errors_on_a_host_only_batch(tmp_path):
    from circom_amd import runtime as rt
    from circom_amd.circuits.basic import Multiplier2
    L = rt.lib()
    for name in ("cw_set_witnesses", "cw_set_witnesses_n8", "cw_set_witnesses_device", "cw_set_witnesses_device_n8", "cw_read_wtns",
                 "cw_read_wtns_many", "cw_witnesses_missing"):
        assert hasattr(L, name), name
    assert rt.ST_BAD_WITNESS == BAD
    cp, c = _circuit(tmp_path, "multiplier2")
    b = c.batch(5, device=-1)
    assert b.witnesses_missing() == -1
    host = np.zeros((5, c.n_witness), dtype=np.uint64)
    # range past the batch, every form (device pointers are never touched: there is no device)
    for call in (lambda: b.set_witnesses(host, first=1), lambda: _set_host32(b, 1, _wide(host)),
                 lambda: b.set_witnesses_device(3, 3, 4096), lambda: b.set_witnesses_device_n8(5, 1, 4096),
                 lambda: b.read_wtns(5, tmp_path / "x.wtns"), lambda: b.read_wtns_many(4, 2, tmp_path / "x%u.wtns")):
        _raises(CW_EINVAL, "range", call)
    # alignment: 8 bytes for the 8-byte form, 16 for the 32-byte form
    _raises(CW_EINVAL, "8-byte aligned", lambda: b.set_witnesses_device_n8(0, 5, 4096 + 4))
    _raises(CW_EINVAL, "16-byte aligned", lambda: b.set_witnesses_device(0, 5, 4096 + 8))
    # null
    for fn, args in ((L.cw_set_witnesses, (b.h, 0, 5, None)), (L.cw_set_witnesses_n8, (b.h, 0, 5, None)),
                     (L.cw_set_witnesses_device, (b.h, 0, 5, None)), (L.cw_set_witnesses_device_n8, (b.h, 0, 5, None)),
                     (L.cw_read_wtns, (b.h, 0, None)), (L.cw_read_wtns_many, (b.h, 0, 5, None)), (L.cw_set_witnesses_n8, (None, 0, 5, None))):
        assert fn(*args) == CW_EINVAL
    assert L.cw_witnesses_missing(None) == -1
    _raises(CW_EINVAL, "conversion", lambda: b.read_wtns_many(0, 5, tmp_path / "x.wtns"))
    # well-formed calls get as far as the device
    for call in (lambda: b.set_witnesses(host), lambda: _set_host32(b, 0, _wide(host)), lambda: b.set_witnesses_device(0, 5, 4096),
                 lambda: b.set_witnesses_device_n8(0, 5, 4096 + 8)):
        _raises(CW_EDEVICE, "host-only", call)
    # files are read and checked before the device is needed: a 32-byte file is not this circuit's, a good one is
    (tmp_path / "n32.wtns").write_bytes(wtns_bytes((1 << 255) - 19, [1, 33, 3, 11]))
    _raises(CW_EIO, "n8", lambda: b.read_wtns(0, tmp_path / "n32.wtns"))
    assert "n32.wtns" in L.cw_last_error().decode()
    _raises(CW_EIO, "cannot read", lambda: b.read_wtns(0, tmp_path / "absent.wtns"))
    good = bytes.fromhex(GOLD["multiplier2"]["vectors"][0]["wtns_hex"])
    (tmp_path / "g0.wtns").write_bytes(good)
    _raises(CW_EDEVICE, "host-only", lambda: b.read_wtns(0, tmp_path / "g0.wtns"))
    (tmp_path / "g1.wtns").write_bytes(good[:-1])
    _raises(CW_EIO, "g1.wtns", lambda: b.read_wtns_many(0, 2, tmp_path / "g%u.wtns"))
    # nothing of the above opened the supplied state; a fresh batch still has no table to check (a host-only batch answers
    # for its missing device first, as every computing call of it does; the state error of a device batch is in the GPU part)
    assert b.witnesses_missing() == -1
    with pytest.raises(rt.CwError):
        b.check_r1cs()
    b.close(); c.close()
    # the other engines
    cp32 = compile_program(Program(Multiplier2()), str(tmp_path), "m2_bn128", sym=False)
    c32 = rt.Circuit(cp32.tape_path, cp32.dat_path, cp32.r1cs_path)
    b32 = c32.batch(2, device=-1)
    img = np.zeros((2, c32.n_witness, 32), dtype=np.uint8)
    (tmp_path / "bn.wtns").write_bytes(wtns_bytes(c32.q, [1, 33, 3, 11]))
    for call in (lambda: b32.set_witnesses(img), lambda: rt._chk(L.cw_set_witnesses_n8(b32.h, 0, 2, img.ctypes.data_as(C.c_void_p))),
                 lambda: b32.set_witnesses_device(0, 2, 4096), lambda: b32.set_witnesses_device_n8(0, 2, 4096),
                 lambda: b32.read_wtns(0, tmp_path / "bn.wtns"), lambda: b32.read_wtns_many(0, 2, tmp_path / "bn%u.wtns")):
        _raises(CW_ESTATE, ONLY64, call)
    assert b32.witnesses_missing() == -1
    b32.close(); c32.close()


def test_every_tampered_poseidon_instance_is_caught_by_the_oracle():
    """the precondition of the tamper test below, on the CPU: every wire of Poseidon(2) is constrained, so +1 on any entry
    violates some row"""
    fc, _, _, want = _tampered()
    assert all(w is not None for i, w in enumerate(want) if i not in CLEAN)
    assert all(want[i] is None for i in CLEAN)
    assert len(fc.constraints) > 1000


CLEAN = (0, 63, 64, 299)


def _tampered():
    """(flat circuit, clean [300][n_witness], tampered copy, the oracle's first violated row per instance or None)"""
    from circom_amd.frontend.flatten import flatten
    fc = flatten(CASES["poseidon2"][0]())
    _, sig = _oracle()
    nw = sig.shape[1]
    img = sig.copy()
    for i in range(img.shape[0]):
        if i not in CLEAN:
            k = 1 + (7 * i) % (nw - 1)
            img[i, k] = (int(img[i, k]) + 1) % Q
    want = [check_r1cs(Q, fc.constraints, [int(v) for v in row]) for row in img]
    return fc, sig, img, want


# ---- 1. the reference's own files in, a clean check out ----------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(GOLD))
def test_gpu_golden_files_check_clean_and_come_back_byte_for_byte(name, tmp_path):
    vecs = GOLD[name]["vectors"]
    cp, c = _circuit(tmp_path, name)
    files = []
    if not all(v["wtns_hex"] for v in vecs):                      # the large ones are pinned by their hash: compute, compare, then supply
        a = c.batch(len(vecs))
        a.set_inputs([[int(v) for v in vec["inputs"]] for vec in vecs])
        a.run(); a.sync()
        assert (a.status() == 0).all()
    for i, vec in enumerate(vecs):
        p = tmp_path / ("g%d.wtns" % i)
        if vec["wtns_hex"]:
            p.write_bytes(bytes.fromhex(vec["wtns_hex"]))
        else:
            a.write_wtns(i, p)
        got = p.read_bytes()
        assert len(got) == vec["wtns_len"] and hashlib.sha256(got).hexdigest() == vec["wtns_sha256"], (name, i)
        files.append(got)
    if not all(v["wtns_hex"] for v in vecs):
        a.close()
    b = c.batch(len(vecs))                                       # a SECOND batch: nothing in it was computed
    assert b.witnesses_missing() == -1
    b.read_wtns(0, tmp_path / "g0.wtns")
    assert b.witnesses_missing() == len(vecs) - 1
    b.read_wtns_many(1, len(vecs) - 1, tmp_path / "g%u.wtns")
    assert b.witnesses_missing() == 0
    if c.n_constraints:
        b.check_r1cs()
    b.sync()
    assert (b.status() == 0).all(), b.status()
    b.write_wtns_many(0, len(vecs), str(tmp_path / "back%u.wtns"))
    for i, want in enumerate(files):
        assert (tmp_path / ("back%d.wtns" % i)).read_bytes() == want, (name, i)
        b.write_wtns(i, tmp_path / "one.wtns")
        assert (tmp_path / "one.wtns").read_bytes() == want, (name, i)
    b.close(); c.close()


# ---- 2. tile edges -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 63, 64, 65, 300])
def test_gpu_tile_edges_every_form_whole_and_in_ranges(B, tmp_path):
    """Poseidon(2): 1 108 entries = 17 tiles of 64 + 20.  Source images: see _set_device for what the guard can and cannot show."""
    from test_bitplane import _Hip
    hip = _Hip()
    _, sig = _oracle()
    cp, c = _circuit(tmp_path, "poseidon2")
    nw = c.n_witness
    assert nw == sig.shape[1] == 1108
    want = sig[:B]
    forms = {
        "device8": lambda b, f, img: _set_device(b, hip, f, img, 8),
        "device32": lambda b, f, img: _set_device(b, hip, f, _wide(img), 32),
        "host8": lambda b, f, img: b.set_witnesses(img, first=f),
        "host32": lambda b, f, img: _set_host32(b, f, _wide(img)),
    }
    splits = [[(0, B)]] + ([[(0, 37), (37, 100), (137, B - 137)]] if B == 300 else [])
    for form, supply in forms.items():
        for ranges in splits:
            b = c.batch(B)
            assert b.witnesses_missing() == -1
            left = B
            for first, count in ranges:
                if left < B:
                    _raises(CW_ESTATE, "witnesses missing for %d instances" % left, b.check_r1cs)
                supply(b, first, want[first:first + count])
                left -= count
                assert b.witnesses_missing() == left, (form, first)
            b.check_r1cs(); b.sync()
            assert (b.status() == 0).all(), (form, ranges, b.status())
            assert (b.r1cs_first_bad() == 0xFFFFFFFF).all()
            assert (_table_n8(b, hip, nw) == want).all(), (form, ranges)
            b.close()
    c.close()


@pytest.mark.gpu
def test_gpu_a_witness_narrower_than_a_tile_at_70001_instances(tmp_path):
    from test_bitplane import _Hip
    hip = _Hip()
    cp, c = _circuit(tmp_path, "multiplier2")
    assert c.n_witness == 4
    B = 70001
    a = np.array([(i * 0x9E3779B97F4A7C15 + 12345) % Q for i in range(B)], dtype=object)
    bb = np.array([(i * 0xC2B2AE3D27D4EB4F + 7) % Q for i in range(B)], dtype=object)
    want = np.array([[1, x * y % Q, x, y] for x, y in zip(a, bb)], dtype=np.uint64)
    wrong = (5, 64, 65535, 65536, B - 1)                            # out + 1: the product no longer holds
    img = want.copy()
    for i in wrong:
        img[i, 1] = (int(img[i, 1]) + 1) % Q
    for eb in (8, 32):
        b = c.batch(B)
        _set_device(b, hip, 0, img if eb == 8 else _wide(img), eb)
        assert b.witnesses_missing() == 0
        b.check_r1cs(); b.sync()
        st, fb = b.status(), b.r1cs_first_bad()
        assert sorted(np.nonzero(st)[0].tolist()) == sorted(wrong) and (st[list(wrong)] == R1CS).all() and (fb[list(wrong)] == 0).all()
        assert (_table_n8(b, hip, 4) == img).all()
        b.close()
    c.close()


# ---- 3. the scatter goes through the witness list ------------------------------------------------------------------------------
@template
def Interleaved(cx):
    """hint-only signals that no constraint names between constrained ones: `pad` is the first signal behind the public ones
    (the earliest place the list may drop one), an `h` sits in front of every `t`"""
    pad = cx.input("pad")
    a = cx.input("a")
    b = cx.input("b")
    out = cx.output("out")
    x = a
    for r in range(100):
        h = cx.signal("h%d" % r)
        cx.hint(h, x * 3 + pad + r)
        t = cx.signal("t%d" % r)
        cx.set(t, x * b + r)
        x = t
    cx.set(out, x + a)


@pytest.mark.gpu
def test_gpu_scatter_goes_through_the_witness_list(tmp_path):
    """cw_load resolves the wires of the .r1cs to slots through the list it has THEN (the identity: load_r1cs64), so the list is
    shortened after the load and the check keeps reading the slots of the full system; what is supplied is in list order."""
    from circom_amd import runtime as rt
    from test_bitplane import _Hip
    hip = _Hip()
    cp = compile_program(Program(Interleaved(), prime="goldilocks"), str(tmp_path), "interleaved", sym=False)
    fc = cp.flat
    c = rt.Circuit(cp.tape_path, cp.dat_path, cp.r1cs_path)
    named = {0}
    for parts in fc.constraints:
        for part in parts:
            named |= set(part)
    keep = np.array(sorted(named | set(range(1 + c.n_public))), dtype=np.uint32)
    dropped = sorted(set(range(c.n_signals)) - set(keep.tolist()))
    # on the CPU: the list is far from the identity, from the first entry behind the public ones on, and spans two tiles
    assert fc.main_input_start in dropped and len(dropped) == 101 and len(keep) == 104
    assert (keep != np.arange(len(keep))).sum() >= len(keep) - 2 and keep[1 + c.n_public] != 1 + c.n_public
    c.set_witness_list(keep)
    assert c.n_witness == len(keep)
    B = 130
    sigs = []
    for i in range(B):
        ins = {fc.main_input_start: (i * 977 + 5) % Q, fc.main_input_start + 1: (Q - 1 - i * i) % Q, fc.main_input_start + 2: (i * 0x9E3779B97F4A7C15) % Q}
        sig, failed = eval_flat(Q, fc.n_signals, fc.n_temps, fc.constants, fc.code, ins)
        assert failed is None and check_r1cs(Q, fc.constraints, sig) is None
        sigs.append(sig)
    full = np.array(sigs, dtype=np.uint64)
    img = full[:, keep]
    broken = {3: 2, 64: 57, 129: 103}                              # instance -> list entry that gets + 1
    for i, k in broken.items():
        img[i, k] = (int(img[i, k]) + 1) % Q
    want_row = {i: check_r1cs(Q, fc.constraints, [int(img[i, np.searchsorted(keep, s)]) if s in named else 0 for s in range(fc.n_signals)])
                for i in broken}
    assert all(r is not None for r in want_row.values())
    for eb in (8, 32):
        b = c.batch(B)
        _set_device(b, hip, 0, img if eb == 8 else _wide(img), eb)
        b.check_r1cs(); b.sync()
        st, fb = b.status(), b.r1cs_first_bad()
        for i in range(B):
            assert st[i] == (R1CS if i in broken else 0) and fb[i] == (want_row[i] if i in broken else 0xFFFFFFFF), (eb, i, st[i], fb[i])
        assert (_table_n8(b, hip, len(keep)) == img).all()
        for i in (0, 64, 129):
            assert b.witness(i) == [int(v) for v in img[i]]
            assert [b.signal(i, int(s)) for s in keep[:8]] == [int(v) for v in img[i, :8]]
            assert b.signal(i, int(keep[-1])) == int(img[i, -1])
        _raises(CW_ESTATE, "no witness program has run", lambda: b.signal(0, dropped[0]))
        _raises(CW_ESTATE, "no witness program has run", lambda: b.signal(0, dropped[-1]))
        b.close()
    c.close()


# ---- 4. tampering, instance by instance, against the oracle ----------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_tampered_instances_are_named_with_the_oracles_row(tmp_path):
    from test_bitplane import _Hip
    hip = _Hip()
    fc, sig, img, want = _tampered()
    assert all((w is None) == (i in CLEAN) for i, w in enumerate(want))       # before any GPU call: the oracle flags every tampered one
    cp, c = _circuit(tmp_path, "poseidon2")
    B = img.shape[0]
    for eb in (8, 32):
        b = c.batch(B)
        _set_device(b, hip, 0, img if eb == 8 else _wide(img), eb)
        b.check_r1cs(); b.sync()
        st, fb = b.status(), b.r1cs_first_bad()
        for i in range(B):
            if want[i] is None:
                assert st[i] == 0 and fb[i] == 0xFFFFFFFF, (eb, i, st[i], fb[i])
            else:
                assert st[i] & R1CS and fb[i] == want[i] and not st[i] & BAD and st[i] == R1CS, (eb, i, st[i], fb[i], want[i])
        text = b.explain(7)
        assert text.startswith("instance 7: ") and "constraint %d of the .r1cs is violated" % want[7] in text, text
        assert b.explain(63) == "instance 63: ok\n"
        b.close()
    c.close()


# ---- 5. malformed witnesses --------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_malformed_witnesses_are_flagged_not_repaired(tmp_path):
    from test_bitplane import _Hip
    hip = _Hip()
    _, sig = _oracle()
    cp, c = _circuit(tmp_path, "poseidon2")
    nw = c.n_witness
    B = 130
    last_i, last_k = B - 1, nw - 1
    # 8-byte form: (instance, entry) -> the 64-bit word
    bad8 = {(0, 0): 2, (63, 0): 0, (64, 1): Q, (last_i, last_k): Q + 5, (1, 63): (1 << 64) - 1, (65, 64): Q, (62, last_k): Q + 5, (last_i, 1): (1 << 64) - 1}
    # 32-byte form: -> the four words
    rnd = np.random.default_rng(5)
    v = lambda: int(rnd.integers(0, 1 << 62))
    bad32 = {(0, 0): (2, 0, 0, 0), (63, 0): (0, 0, 0, 0), (64, 0): (1, 0, 0, 1), (0, 1): (v(), 1, 0, 0), (63, 63): (v(), 0, 7, 0), (64, 64): (v(), 0, 0, 1 << 63),
             (last_i, last_k): (v(), v(), v(), v()), (1, last_k): (Q, 0, 0, 0), (last_i, 1): ((1 << 64) - 1, 0, 0, 0), (65, 63): (0, 0, 1, 0), (66, 64): (v(), Q, 0, 0)}
    for eb, bad in ((8, bad8), (32, bad32)):
        img = sig[:B].copy() if eb == 8 else _wide(sig[:B])
        want = sig[:B].copy()
        for (i, k), word in bad.items():
            if eb == 8:
                img[i, k] = word
                val = word
            else:
                img[i, k] = word
                val = sum(int(w) << (64 * n) for n, w in enumerate(word))
            want[i, k] = 1 if k == 0 else val % Q                 # the REDUCED value is stored; slot 0 keeps its 1
        flagged = sorted({i for i, _ in bad})
        b = c.batch(B)
        _set_device(b, hip, 0, img, eb)
        st = b.status()
        assert sorted(np.nonzero(st)[0].tolist()) == flagged and (st[flagged] == BAD).all(), (eb, st[flagged])
        assert (_table_n8(b, hip, nw) == want).all(), eb
        for i in (0, 63, last_i):
            assert b.witness(i) == [int(x) for x in want[i]] and b.signal(i, 0) == 1
        b.check_r1cs(); b.sync()
        st = b.status()
        assert (st[flagged] & BAD).all() and not st[[i for i in range(B) if i not in flagged]].any()
        assert "malformed" in b.explain(0)
        b.close()
    c.close()


# ---- 6. state ----------------------------------------------------------------------------------------------------------------
@template
def Logged(cx):
    a = cx.input("a")
    out = cx.output("out")
    cx.set(out, a * a)
    cx.log("square", out)


@pytest.mark.gpu
def test_gpu_state_run_ends_the_supplied_state_and_run_check_is_a_run(tmp_path):
    from circom_amd import runtime as rt
    from test_bitplane import _Hip
    hip = _Hip()
    rows, sig = _oracle()
    cp, c = _circuit(tmp_path, "poseidon2")
    B = 130
    want = sig[:B]
    junk = want.copy()
    junk[:, 5] = (junk[:, 5] + np.uint64(1)) % np.uint64(Q)
    junk_rows = [check_r1cs(Q, cp.flat.constraints, [int(v) for v in row]) for row in junk]
    assert None not in junk_rows                                   # the oracle: every instance violates some row
    b = c.batch(B)
    _raises(CW_ESTATE, "cw_check_r1cs before cw_run", b.check_r1cs)
    inp = np.zeros((B, c.n_inputs, 4), dtype="<u8")
    inp[:, :, 0] = np.array(rows[:B], dtype=np.uint64)
    d_in = hip.upload(inp.view(np.uint8))
    b.set_inputs_device(d_in)

    def computed():
        b.sync()
        assert b.witnesses_missing() == -1
        assert (b.status() == 0).all() and (b.r1cs_first_bad() == 0xFFFFFFFF).all()
        assert (_table_n8(b, hip, c.n_witness) == want).all()

    # supply -> run: the computed witnesses and statuses
    b.set_witnesses(junk)
    b.check_r1cs(); b.sync()
    assert (b.status() == R1CS).all() and b.r1cs_first_bad().tolist() == junk_rows and b.witnesses_missing() == 0
    b.run(); b.check_r1cs()
    computed()
    # supply -> run_check, three times: plain calls, the capture, the replay of the graph
    for r in range(3):
        b.set_witnesses(junk)
        assert b.witnesses_missing() == 0
        b.run_check()
        assert b.graph_captured == (r >= 1), r
        computed()
    # a partial supply, then run_check: nothing of the supply is left either
    b.set_witnesses(junk[:10], first=3)
    assert b.witnesses_missing() == B - 10
    b.run_check()
    computed()
    # check twice on one supplied table: identical words
    junk2 = want.copy()
    for i in range(0, B, 3):
        k = 1 + (11 * i) % (c.n_witness - 1)
        junk2[i, k] = (int(junk2[i, k]) + 1) % Q
    rows2 = [check_r1cs(Q, cp.flat.constraints, [int(v) for v in row]) for row in junk2]
    assert all((r is not None) == (i % 3 == 0) for i, r in enumerate(rows2))
    junk2[5, 9] = np.uint64(Q)                                     # and a malformed one
    b.set_witnesses(junk2)
    b.check_r1cs(); b.sync()
    st1, fb1 = b.status(), b.r1cs_first_bad()
    b.check_r1cs(); b.sync()
    assert (b.status() == st1).all() and (b.r1cs_first_bad() == fb1).all()
    assert st1[5] & BAD and (st1[::3] == R1CS).all() and not st1[1::3].any() and not np.delete(st1[2::3], 1).any()
    assert fb1[::3].tolist() == rows2[::3]
    # supplying again only adds: the words of the earlier supply stay until the next run or first supply
    b.set_witnesses(want[5:6], first=5)
    assert b.status()[5] == st1[5] and b.witnesses_missing() == 0
    hip.h.hipFree(d_in)
    b.close(); c.close()
    # run -> supply: no witness program has run on THIS table - no log, no hidden signal
    cp = compile_program(Program(Logged(), prime="goldilocks"), str(tmp_path), "logged", sym=False)
    c = rt.Circuit(cp.tape_path, cp.dat_path, cp.r1cs_path)
    b = c.batch(3)
    b.set_inputs([[2], [3], [Q - 1]])
    b.run(); b.sync()
    hidden = c.n_signals                                           # the first hidden log value sits behind the circuit's signals
    assert b.log(1) == "square 9\n" and b.signal(1, hidden) == 9
    b.set_witnesses([[1, 4, 2], [1, 9, 3], [1, 1, Q - 1]])
    _raises(CW_ESTATE, "no witness program has run", lambda: b.log(1))
    _raises(CW_ESTATE, "no witness program has run", lambda: b.signal(1, hidden))
    assert b.signal(1, 1) == 9
    b.check_r1cs(); b.sync()
    assert (b.status() == 0).all()
    b.run(); b.sync()
    assert b.log(2) == "square 1\n" and b.witnesses_missing() == -1
    b.close(); c.close()


# ---- 7. the command line ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_cli_check_mode(tmp_path):
    from circom_amd import runtime as rt
    assert rt.CLI_PATH.exists(), "cw_witness was not built (make -C circom_amd/csrc)"
    cp, c = _circuit(tmp_path, "multiplier2", sym=True)
    c.close()
    prefix = str(tmp_path / "multiplier2")
    assert cp.tape_path == prefix + ".cwt" and cp.sym_path == prefix + ".sym"
    vecs = GOLD["multiplier2"]["vectors"]
    good = [bytes.fromhex(vecs[k]["wtns_hex"]) for k in (0, 3)]
    body = len(good[0]) - 4 * 8                                   # [1, out, a, b], 8 bytes each, at the end of the file
    out = int.from_bytes(good[1][body + 8:body + 16], "little")
    bad = good[1][:body + 8] + ((out + 1) % Q).to_bytes(8, "little") + good[1][body + 16:]
    w = [int.from_bytes(bad[body + 8 * k:body + 8 * k + 8], "little") for k in range(4)]
    assert check_r1cs(Q, cp.flat.constraints, w) == 0
    paths = [str(tmp_path / n) for n in ("a.wtns", "b.wtns", "tampered.wtns")]
    for p, data in zip(paths, good + [bad]):
        open(p, "wb").write(data)
    r = subprocess.run([str(rt.CLI_PATH), "--check", prefix] + paths, capture_output=True, text=True)
    assert r.returncode == 1, (r.stdout, r.stderr)
    lines = r.stdout.splitlines()
    assert lines[:3] == [paths[0] + ": OK", paths[1] + ": OK", paths[2] + ": constraint 0 violated"], r.stdout
    assert "constraint 0 of the .r1cs is violated" in r.stdout and "main.c = %d;" % w[1] in r.stdout, r.stdout
    r = subprocess.run([str(rt.CLI_PATH), "--check", prefix] + paths[:2], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.splitlines() == [paths[0] + ": OK", paths[1] + ": OK"], (r.stdout, r.stderr)
    r = subprocess.run([str(rt.CLI_PATH), "--check", prefix], capture_output=True, text=True)
    assert r.returncode == 2 and "Usage" in r.stderr
    open(paths[1], "wb").write(good[0][:-1])
    r = subprocess.run([str(rt.CLI_PATH), "--check", prefix] + paths[:2], capture_output=True, text=True)
    assert r.returncode == 2 and "b.wtns" in r.stderr, (r.stdout, r.stderr)
