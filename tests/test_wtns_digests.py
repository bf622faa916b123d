"""Witness digests: cw_get_wtns_digests / cw_get_wtns_digests_device (include/circom_amd.h) - out[j] = SHA-256 of the bytes
cw_write_wtns(b, first + j, ..) writes, computed on the device with lane = instance.  Kernels: csrc/cw64.hip
cw64_wtns_digest_kernel, csrc/cw_kernels.hip cw_wtns_digest_kernel<MONT>, csrc/cw_bits.hip cw_bits_wtns_digest_kernel (both table
layouts); the walk of the message and the compression function are csrc/cw_wtns_digest.h and csrc/cw_sha256.h, replayed on the
CPU by tests/test_wtns_digest_host.py.

Expected digests come from hashlib.sha256 over circom_amd.hip_elements.writers.wtns_bytes(q, the oracle's values), or directly
from the reference runtime's wtns_sha256 in tests/golden/ - never from cw_write_wtns or another call into the library (the CLI
test excepted, which is about the two modes of one program agreeing).  The shapes: batches of 1, 63, 64, 65, 130 and 300 are a
partial group, a whole one, one + 1, two + 2, four + 44; the ranges start on and off a group boundary, straddle one, and end with
the batch.  Device images lie between 0xA5 guards at the end of an allocation."""
import ctypes as C
import hashlib
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
from test_input_rows import _case, pack_rows                                         # noqa: E402
from test_output_rows import _Dev, _rerun_case                                       # noqa: E402
from test_instance_lists import _batch, _eval, _flat, _image, circuits               # noqa: E402,F401

from circom_amd.circuits.basic import Multiplier2                                    # noqa: E402
from circom_amd.compiler import compile_program, strands_for                         # noqa: E402
from circom_amd.frontend.dsl import Program, template                                # noqa: E402
from circom_amd.hip_elements.writers import wtns_bytes                              # noqa: E402
from oracle.field import PRIMES                                                      # noqa: E402
from oracle.tape_eval import eval_flat                                               # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = json.load(open(os.path.join(HERE, "golden", "reference_wtns.json")))
GOLD_GL = json.load(open(os.path.join(HERE, "golden", "reference_wtns_goldilocks.json")))
CW_ESTATE = -5
GUARD = 64


def _ints(image, n8=32):
    """[n][32] uint8 canonical little-endian -> list of ints"""
    return [int.from_bytes(image[k, :n8].tobytes(), "little") for k in range(image.shape[0])]


def expected(q, want, entries=None):
    """hashlib over wtns_bytes of every instance of want [B][n_signals][32] (optionally the entries of a witness list)"""
    n8 = 8 if q.bit_length() <= 64 else 32
    if entries is not None:
        want = want[:, np.asarray(entries, dtype=np.int64)]
    B, nw = want.shape[0], want.shape[1]
    head = wtns_bytes(q, [0] * nw)[:44 + n8]                        # the header of a file of nw elements
    assert wtns_bytes(q, _ints(want[0], n8)) == head + want[0, :, :n8].tobytes()
    out = np.zeros((B, 32), dtype=np.uint8)
    for i in range(B):
        out[i] = np.frombuffer(hashlib.sha256(head + want[i, :, :n8].tobytes()).digest(), dtype=np.uint8)
    return out


def ranges(B):
    out = []
    for first, count in ((0, B), (37, B - 37), (63, 2), (64, 64), (B - 1, 1)):
        if count > 0 and first + count <= B and (first, count) not in out:
            out.append((first, count))
    return out


class _Dig(_Dev):
    def digests(self, b, first, count):
        """the device form into 0xA5 bytes between two guards, the second of which ends with the allocation: (digests, guards)"""
        n = count * 32
        p = self.at_end(GUARD + n + GUARD)
        b.wtns_digests_device(first, count, p + GUARD)
        raw = self.download(p, GUARD + n + GUARD)
        return raw[GUARD:GUARD + n].reshape(count, 32), np.concatenate([raw[:GUARD], raw[GUARD + n:]])


@pytest.fixture(scope="module")
def hip():
    return _Dig()


def _check(hip, b, want_digests, B):
    for first, count in ranges(B):
        exp = want_digests[first:first + count]
        got = b.wtns_digests(first, count)
        assert got.shape == (count, 32)
        bad = np.flatnonzero((got != exp).any(axis=1))
        assert len(bad) == 0, ("host", first, count, bad[:8].tolist(), got[bad[0]].tobytes().hex(), exp[bad[0]].tobytes().hex())
        got, guards = hip.digests(b, first, count)
        bad = np.flatnonzero((got != exp).any(axis=1))
        assert len(bad) == 0 and (guards == 0xA5).all(), ("device", first, count, bad[:8].tolist())


# ---- without a GPU ---------------------------------------------------------------------------------------------------------------
def test_the_library_exports_the_two_symbols():
    from circom_amd import runtime as rt
    L = rt.lib()
    for name in ("cw_get_wtns_digests", "cw_get_wtns_digests_device"):
        assert hasattr(L, name) and name in rt._SIGS, name
    assert hasattr(rt.Batch, "wtns_digests") and hasattr(rt.Batch, "wtns_digests_device")


# ---- GPU -------------------------------------------------------------------------------------------------------------------------
_DIGESTS = {}


def _bg15_digests(prime):
    """digests of the 300 instances of BitGadget(15): computed once, shared, never modified"""
    if prime not in _DIGESTS:
        _, want = _case(15, prime)
        _DIGESTS[prime] = expected(PRIMES[prime], want)
        _DIGESTS[prime].setflags(write=False)
    return _DIGESTS[prime]


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 63, 64, 65, 130, 300])
@pytest.mark.parametrize("kind", ["interp", "jit", "wide", "gl"])
def test_gpu_digests_on_every_layout(circuits, hip, monkeypatch, kind, B):
    prime = "goldilocks" if kind == "gl" else "bn128"
    c, b = _batch(circuits, monkeypatch, kind, B)
    bits, _ = _case(15, prime)
    b.set_inputs_rows(pack_rows(bits[:B], (bits.shape[1] + 7) // 8, True))
    b.run(); b.check_r1cs(); b.sync()
    assert (b.status() == 0).all()
    _check(hip, b, _bg15_digests(prime), B)
    b.close()


@template
def Chain(c, n):
    """no output and no public input: a witness list may shrink to the constant alone"""
    a = c.input("a")
    b = c.input("b")
    m = c.signal("m", n)
    c.set(m[0], a * b)
    for k in range(1, n):
        c.set(m[k], m[k - 1] * a + b)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["gl", "wide"])
def test_gpu_digests_follow_the_witness_list(tmp_path, hip, kind):
    """the header's nWitness and the order follow cw_set_witness_list.  64-bit runtime: lists of 1 .. 17 and 25 entries - every
    residue mod 8, the extra tail block (1, 9, 17, 25) and a list of one element; 256-bit schedule: 1, 2, 3 entries and a list
    with gaps (the library takes increasing lists only, so a permuted one cannot be set)."""
    from circom_amd import runtime as rt
    prime = "goldilocks" if kind == "gl" else "bn128"
    q = PRIMES[prime]
    prog = Program(Chain(30), prime=prime) if kind == "gl" else Program(Chain(30))
    # (256-bit schedule without emitted code: the interpreter keeps the same table, and the test saves the assembler's seconds)
    cp = compile_program(prog, str(tmp_path), "chain_" + kind, sym=False, **({} if kind == "gl" else dict(strands=(1,), pipe=None, fpjit=False)))
    fc = cp.flat
    c = rt.Circuit(cp.tape_path, cp.dat_path, cp.r1cs_path)
    assert c.n_public == 0 and fc.n_signals == 33
    B = 65
    rng = np.random.default_rng(33)
    ins = [[int.from_bytes(rng.bytes(32), "little") % q for _ in range(2)] for _ in range(B)]
    want = np.stack([_image(eval_flat(q, fc.n_signals, fc.n_temps, fc.constants, fc.code,
                                      {fc.main_input_start: r[0], fc.main_input_start + 1: r[1]})[0]) for r in ins])
    gaps = [0, 2, 3, 7, 8, 9, 20, 31, 32]
    lists = [list(range(n)) for n in (list(range(1, 18)) + [25] if kind == "gl" else [1, 2, 3])] + [gaps]
    for lst in lists:
        c.set_witness_list(np.asarray(lst, dtype=np.uint32))
        assert c.n_witness == len(lst)
        b = c.batch(B)
        b.set_inputs(ins)
        b.run(); b.sync()
        assert (b.status() == 0).all()
        _check(hip, b, expected(q, want, lst), B)
        b.close()
    c.close()


def _golden_batch(tmp_path, mk, name, vecs, B, at, q, **kw):
    """a batch of B random instances with the golden input vectors at the instances `at`: (circuit, batch, inputs)"""
    from circom_amd import runtime as rt
    cp = compile_program(mk(), str(tmp_path), name, sym=False, **kw)
    c = rt.Circuit(cp.tape_path, cp.dat_path, cp.r1cs_path)
    rng = np.random.default_rng(len(name))
    ins = [[int.from_bytes(rng.bytes(32), "little") % q for _ in range(c.n_inputs)] for _ in range(B)]
    for i, vec in zip(at, vecs):
        ins[i] = [int(v) for v in vec["inputs"]]
    b = c.batch(B)
    b.set_inputs(ins)
    b.run(); b.sync()
    return cp, c, b, ins


def _mg():
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(HERE, "golden", "make_golden.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    return mg


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["poseidon2", "poseidon2_bls12381"])
def test_gpu_digests_of_a_montgomery_table_equal_the_reference_runtimes(tmp_path, hip, name):
    mk, prime, rows = _mg().cases()[name]
    vecs = GOLD["cases"][name]["vectors"][:2]
    cp, c, b, ins = _golden_batch(tmp_path, mk, name, vecs, 130, (1, 129), PRIMES[prime], strands=strands_for(130), jit=False, fpjit=False)
    assert c.montgomery and c.n_witness == 1108
    got = b.wtns_digests()
    for i, vec in zip((1, 129), vecs):
        assert got[i].tobytes().hex() == vec["wtns_sha256"], (name, i)
    # the random instances against the oracle, and the device form of an unaligned range
    fc = cp.flat
    for i in (0, 64, 128):
        sig, failed = eval_flat(c.q, fc.n_signals, fc.n_temps, fc.constants, fc.code, {fc.main_input_start + k: v for k, v in enumerate(ins[i])})
        assert failed is None and got[i].tobytes() == hashlib.sha256(wtns_bytes(c.q, sig)).digest(), (name, i)
    dev, guards = hip.digests(b, 1, 129)
    assert (dev == got[1:]).all() and (guards == 0xA5).all()
    b.close(); c.close()


@pytest.mark.gpu
def test_gpu_digests_of_a_small_montgomery_table(circuits, hip):
    """Multiplier2 with a Montgomery-form table, random full-width inputs, B = 65"""
    fc, c = circuits("m2mont")
    assert c.montgomery and c.n_witness == 4
    B = 65
    rng = np.random.default_rng(65)
    ins = [[int.from_bytes(rng.bytes(32), "little") % c.q for _ in range(2)] for _ in range(B)]
    want = np.stack([_image([1, a * b % c.q, a, b]) for a, b in ins])
    b = c.batch(B)
    b.set_inputs(ins)
    b.run(); b.sync()
    _check(hip, b, expected(c.q, want), B)
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["poseidon2", "opzoo"])
def test_gpu_digests_of_the_64_bit_runtime_equal_the_reference_runtimes(tmp_path, hip, name):
    from make_golden import goldilocks_cases
    mk, rows = goldilocks_cases()[name]
    vecs = GOLD_GL["cases"][name]["vectors"]
    B = max(130, len(vecs))
    at = [1] + list(range(2, len(vecs))) + [B - 1] if len(vecs) > 1 else [1]
    at = at[:len(vecs)]
    cp, c, b, ins = _golden_batch(tmp_path, mk, name, vecs, B, at, PRIMES["goldilocks"])
    assert c.element_bytes == 8 and (name != "poseidon2" or c.n_witness == 1108)
    got = b.wtns_digests()
    for i, vec in zip(at, vecs):
        assert got[i].tobytes().hex() == vec["wtns_sha256"], (name, i)
    dev, guards = hip.digests(b, 1, B - 1)
    assert (dev == got[1:]).all() and (guards == 0xA5).all()
    b.close(); c.close()


@pytest.mark.gpu
def test_gpu_digests_of_a_real_boolean_circuit(tmp_path, hip, monkeypatch):
    """sha256_512 x 130 on the interpreted bit engine: a 13 MB message per lane.  The golden vectors sit inside the batch; two more
    instances are checked against hashlib over the oracle's witness."""
    from circom_amd import runtime as rt
    monkeypatch.setenv("CW_BITS_JIT", "0")
    mk, prime, rows = _mg().cases()["sha256_512"]
    vecs = GOLD["cases"]["sha256_512"]["vectors"][:2]
    cp = compile_program(mk(), str(tmp_path), "sha256_512", sym=False, strands=strands_for(130), jit=False)
    c = rt.Circuit(cp.tape_path, cp.dat_path, cp.r1cs_path)
    B, at = 130, (3, 77)
    bits = np.random.default_rng(512).integers(0, 2, size=(B, c.n_inputs), dtype=np.uint8)
    for i, vec in zip(at, vecs):
        bits[i] = [int(v) for v in vec["inputs"]]
    b = c.batch(B)
    assert b.bitmode and not b.jit
    b.set_inputs_rows(pack_rows(bits, (c.n_inputs + 7) // 8, True))
    b.run(); b.sync()
    assert (b.status() == 0).all()
    got = b.wtns_digests()
    for i, vec in zip(at, vecs):
        assert c.n_witness == vec["n_witness"] and got[i].tobytes().hex() == vec["wtns_sha256"], i
    fc = cp.flat
    for i in (0, 129):
        sig, failed = eval_flat(c.q, fc.n_signals, fc.n_temps, fc.constants, fc.code, {fc.main_input_start + k: int(v) for k, v in enumerate(bits[i])})
        assert failed is None and got[i].tobytes() == hashlib.sha256(wtns_bytes(c.q, sig)).digest(), i
    dev, guards = hip.digests(b, 63, 67)
    assert (dev == got[63:]).all() and (guards == 0xA5).all()
    b.close(); c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("engine", ["interp", "jit"])
def test_gpu_digests_of_rerun_instances_come_from_the_side_batch(circuits, hip, monkeypatch, engine):
    monkeypatch.setenv("CW_BITS_JIT", "1" if engine == "jit" else "0")
    fc, c = circuits("bg15")
    _, vals, want = _rerun_case()
    B = 130
    image = np.zeros((B, c.n_inputs, 32), dtype=np.uint8)
    image[:, :, 0] = vals
    b = c.batch(B)
    assert b.bitmode
    b.set_inputs(image)
    b.run(); b.sync()
    exp = expected(c.q, want)
    clean = _bg15_digests("bn128")[:B]
    odd = [5, 64, 129]
    assert (exp[odd] != clean[odd]).any(axis=1).all() and (np.delete(exp, odd, axis=0) == np.delete(clean, odd, axis=0)).all()
    _check(hip, b, exp, B)                                   # the three from the side batch, their neighbours untouched
    b.close()
    # more than a quarter of the batch is not boolean: the side batch holds everything and serves the range alone
    fcf = _flat("bg15")
    vals2 = vals.copy()
    want2 = want.copy()
    for i in range(0, B, 3):
        vals2[i, 7] = 5 + i
        sig, failed = _eval(fcf, vals2[i])
        want2[i] = _image(sig)
    image[:, :, 0] = vals2
    b = c.batch(B)
    b.set_inputs(image)
    b.run(); b.sync()
    _check(hip, b, expected(c.q, want2), B)
    b.close()


@pytest.mark.gpu
def test_gpu_digests_of_many_workgroups_with_a_ragged_end(tmp_path, hip):
    """Multiplier2 x 70 001: 1 094 waves, the last with one live lane; every digest compared"""
    from circom_amd import runtime as rt
    # (no emitted code: the interpreter keeps the same table, and the test saves the assembler's seconds)
    cp = compile_program(Program(Multiplier2()), str(tmp_path), "m2", sym=False, fpjit=False)
    c = rt.Circuit(cp.tape_path, cp.dat_path, cp.r1cs_path)
    B = 70001
    rng = np.random.default_rng(70001)
    ab = rng.integers(0, 1 << 62, size=(B, 2), dtype=np.uint64)
    image = np.zeros((B, 2, 32), dtype=np.uint8)
    image[:, :, :8] = ab.view(np.uint8).reshape(B, 2, 8)
    b = c.batch(B)
    b.set_inputs(image)
    b.run(); b.sync()
    files = np.zeros((B, 204), dtype=np.uint8)
    files[:, :76] = np.frombuffer(wtns_bytes(c.q, [0] * 4)[:76], dtype=np.uint8)
    files[:, 76] = 1
    prod = [(int(x) * int(y)) % c.q for x, y in ab]
    files[:, 108:140] = np.frombuffer(b"".join(p.to_bytes(32, "little") for p in prod), dtype=np.uint8).reshape(B, 32)
    files[:, 140:204] = image.reshape(B, 64)
    assert files[7].tobytes() == wtns_bytes(c.q, [1, prod[7], int(ab[7, 0]), int(ab[7, 1])])
    exp = np.stack([np.frombuffer(hashlib.sha256(files[i].tobytes()).digest(), dtype=np.uint8) for i in range(B)])
    got = b.wtns_digests()
    bad = np.flatnonzero((got != exp).any(axis=1))
    assert len(bad) == 0, bad[:8].tolist()
    dev, guards = hip.digests(b, 1, B - 1)
    assert (dev == exp[1:]).all() and (guards == 0xA5).all()
    b.close(); c.close()


@pytest.mark.gpu
def test_gpu_state_and_laziness(circuits, hip, monkeypatch):
    from circom_amd import runtime as rt
    L = rt.lib()
    c, b = _batch(circuits, monkeypatch, "gl", 130)
    B = 130
    bits, want = _case(15, "goldilocks")
    exp = _bg15_digests("goldilocks")
    out = np.full((B, 32), 0xA5, dtype=np.uint8)
    # before cw_run
    assert L.cw_get_wtns_digests(b.h, 0, B, out.ctypes.data_as(C.c_void_p)) == CW_ESTATE and "before cw_run" in L.cw_last_error().decode()
    p = hip.at_end(B * 32)
    assert L.cw_get_wtns_digests_device(b.h, 0, B, C.c_void_p(p)) == CW_ESTATE and "before cw_run" in L.cw_last_error().decode()
    assert (out == 0xA5).all() and (hip.download(p, B * 32) == 0xA5).all()
    # a supplied table answers "witnesses missing" until it is complete, then gives the digests of the supplied files
    rows = want[:B, :, :8].copy().view("<u8").reshape(B, -1)
    b.set_witnesses(rows[:70], 0)
    with pytest.raises(rt.CwError) as e:
        b.wtns_digests()
    assert e.value.code == CW_ESTATE and "witnesses missing for 60 instances" in str(e.value)
    b.set_witnesses(rows[70:], 70)
    assert b.witnesses_missing() == 0
    assert (b.wtns_digests() == exp[:B]).all() and b.witnesses_missing() == 0
    # count == 0 writes nothing
    assert L.cw_get_wtns_digests(b.h, 5, 0, out.ctypes.data_as(C.c_void_p)) == 0 and (out == 0xA5).all()
    assert L.cw_get_wtns_digests_device(b.h, B, 0, C.c_void_p(p)) == 0 and (hip.download(p, B * 32) == 0xA5).all()
    b.close()
    # status words and a captured cw_run_check graph are unchanged by the call
    c, b = _batch(circuits, monkeypatch, "gl", B)
    image = np.zeros((B, c.n_inputs, 32), dtype=np.uint8)
    image[:, :, 0] = bits[:B]
    d_in = hip.upload(image)
    b.set_inputs_device(d_in)
    for _ in range(3):
        b.run_check()
    b.sync()
    assert b.graph_captured
    st, fb = b.status().copy(), b.r1cs_first_bad().copy()
    assert (b.wtns_digests() == exp[:B]).all()
    dev, guards = hip.digests(b, 0, B)
    assert (dev == exp[:B]).all() and (guards == 0xA5).all()
    assert b.graph_captured and (b.status() == st).all() and (b.r1cs_first_bad() == fb).all()
    b.run_check(); b.sync()
    assert b.graph_captured and (b.wtns_digests(37, 5) == exp[37:42]).all()
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["interp", "gl"])
def test_gpu_two_batches_on_caller_streams(circuits, hip, monkeypatch, kind):
    """each batch on its own non-blocking stream, nothing waited for until both device forms are enqueued: the digests of either
    are what it gives alone (the oracle's)"""
    prime = "goldilocks" if kind == "gl" else "bn128"
    h = hip.h
    h.hipStreamCreateWithFlags.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
    h.hipStreamSynchronize.argtypes = [C.c_void_p]
    h.hipStreamDestroy.argtypes = [C.c_void_p]
    bits, _ = _case(15, prime)
    exp = _bg15_digests(prime)
    B = 130
    streams, batches, outs = [], [], []
    monkeypatch.setenv("CW_BITS_JIT", "0")
    fc, c = circuits("gl15" if kind == "gl" else "bg15")
    for j in range(2):
        s = C.c_void_p()
        assert h.hipStreamCreateWithFlags(C.byref(s), 1) == 0
        streams.append(s.value)
        batches.append(c.batch(B, stream=s.value))
        outs.append(hip.alloc(B * 32))
    for j, b in enumerate(batches):                            # batch 1 takes the instances the other way round
        rows = bits[:B] if j == 0 else bits[:B][::-1]
        b.set_inputs_rows(pack_rows(np.ascontiguousarray(rows), (bits.shape[1] + 7) // 8, True))
    for b in batches:
        b.run()
    for j, b in enumerate(batches):
        b.wtns_digests_device(0, B, outs[j])
    for s in streams:
        assert h.hipStreamSynchronize(s) == 0
    assert (hip.download(outs[0], (B, 32)) == exp[:B]).all()
    assert (hip.download(outs[1], (B, 32)) == exp[:B][::-1]).all()
    for b in batches:
        b.close()
    for s in streams:
        assert h.hipStreamDestroy(s) == 0


@pytest.mark.gpu
def test_gpu_cli_prints_the_digests_of_the_files_it_writes(tmp_path):
    from circom_amd import runtime as rt
    cp = compile_program(Program(Multiplier2()), str(tmp_path), "multiplier2", sym=False, fpjit=False)
    prefix = os.path.join(str(tmp_path), "multiplier2")
    (tmp_path / "in.json").write_text('[{"a": "3", "b": "11"}, {"a": "5", "b": "7"}]')
    before = sorted(os.listdir(tmp_path))
    r = subprocess.run([str(rt.CLI_PATH), "--sha256", prefix, str(tmp_path / "in.json")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert sorted(os.listdir(tmp_path)) == before                                                # --sha256 wrote no file
    w = subprocess.run([str(rt.CLI_PATH), prefix, str(tmp_path / "in.json"), str(tmp_path / "out_%d.wtns")], capture_output=True, text=True,
                       timeout=120)
    assert w.returncode == 0, w.stdout + w.stderr
    assert sorted(set(os.listdir(tmp_path)) - set(before)) == ["out_0.wtns", "out_1.wtns"]
    lines = r.stdout.splitlines()
    assert lines == ["%s  %d" % (hashlib.sha256((tmp_path / ("out_%d.wtns" % i)).read_bytes()).hexdigest(), i) for i in range(2)]
    assert (tmp_path / "out_0.wtns").read_bytes() == wtns_bytes(PRIMES["bn128"], [1, 33, 3, 11])
