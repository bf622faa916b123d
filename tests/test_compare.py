"""Witness compare on the device (include/circom_amd.h): cw_compare_witnesses(_n8), cw_compare_witnesses_device(_n8),
cw_compare_wtns, cw_compare_wtns_many and `cw_witness --compare`.  image[j][k] = entry entry0 + k of instance first + j is compared
byte by byte with what the egress would write there; diff[j] = the lowest differing entry or 0xFFFFFFFF, summary = {instances
that differ, the lowest of them}.  Kernels: csrc/cw_kernels.hip cw_compare_kernel<MONT>, csrc/cw64.hip cw64_compare_kernel<EB>,
csrc/cw_bits.hip cw_bits_compare_kernel (both table layouts), the reduction in csrc/cw_compare.hip.h.

Expected images come from oracle.tape_eval (eval_flat; wtns_bytes for the files) and expected verdicts from numpy, never from
another call into the library; where tests/golden/ has the circuit, the SHA-256 of the oracle's .wtns is first compared with the
reference runtime's wtns_sha256, so "equal to the image" means "equal to the reference runtime's file".  Agreement with a numpy
compare of cw_get_witnesses is asserted as a second, weaker check.

The shapes: a witness of four entries clips every tile, 28 entries clip the 64-entry tile, 380 are two waves of the bit kernel,
1 108 and 1 130 a second workgroup of it in the element direction; the entry ranges (0, whole), (1, 7), (3, 65), (15, 17) are the
edges of the 16- and 64-entry tiles; the instance ranges of a batch of 300 - (0, 300), (37, 201), (63, 2), (64, 64), (299, 1) -
are whole tiles + one of 44, windows off a group boundary of the bit table, exactly one tile, the last instance.  Device buffers
(the image, d_diff, d_summary) end at the end of their allocation; 0xA5 words lie in front of d_diff and d_summary."""
import ctypes as C
import functools
import hashlib
import importlib.util
import itertools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
from test_bitplane import BitGadget                                                  # noqa: E402
from test_input_rows import _case, pack_rows                                         # noqa: E402
from test_output_rows import _Dev, _rerun_case                                       # noqa: E402
from test_instance_lists import _batch, _eval, _flat, _image, _odd_case, _run_values, circuits, clip   # noqa: E402,F401

from circom_amd.circuits.basic import Multiplier2                                    # noqa: E402
from circom_amd.compiler import compile_program, strands_for                         # noqa: E402
from circom_amd.frontend.dsl import Program                                          # noqa: E402
from circom_amd.frontend.flatten import flatten                                      # noqa: E402
from circom_amd.hip_elements.writers import wtns_bytes                              # noqa: E402
from oracle.field import PRIMES                                                      # noqa: E402
from oracle.tape_eval import eval_flat                                               # noqa: E402

# tests/test_batch_lifetime.py reads the DEVICE's free memory around its cycles; this file's images (half a gigabyte in the
# launch-pieces test) come and go, and in another worker they would fall into that reading.  The same group keeps both files on
# one worker, one after the other.
pytestmark = pytest.mark.xdist_group("batch_lifetime")

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD =json.load(open(os.path.join(HERE, "golden", "reference_wtns.json")))
GOLD_GL = json.load(open(os.path.join(HERE, "golden", "reference_wtns_goldilocks.json")))
CW_EIO, CW_ESTATE = -1, -5
NONE = 0xFFFFFFFF
A5 = 0xA5A5A5A5
GUARD = 64
RANGES = [(0, None), (1, 7), (3, 65), (15, 17)]                                      # (entry0, n); None = the whole witness
FORMS = [(0, 300), (37, 201), (63, 2), (64, 64), (299, 1)]                           # (first, count) of a batch of 300


def forms(B):
    """FORMS for a batch of B: the ranges that fit, the last two moved to the end of the batch"""
    out = []
    for first, count in ((0, B), (37, B - 37 - 62), (63, 2), (64, 64), (B - 1, 1)):
        if count > 0 and first + count <= B and (first, count) not in out:
            out.append((first, count))
    return out


assert forms(300) == FORMS


# ---- what numpy expects ----------------------------------------------------------------------------------------------------------
def exp_diff(want, image, entry0):
    """want, image: [count][n][eb] -> uint32 [count], the lowest differing entry0 + k or NONE"""
    ne = (want != image).any(axis=2)
    return np.where(ne.any(axis=1), ne.argmax(axis=1) + entry0, NONE).astype(np.uint32)


def exp_summary(diff, first):
    bad = np.flatnonzero(diff != NONE)
    return (len(bad), first + int(bad[0]) if len(bad) else NONE)


class _Cmp(_Dev):
    """_Dev's arena, larger: an image ENDS where the arena's allocation ends.  The verdict words are the last `count` words of
    an allocation of NW (0xA5 in front of them), the summary the last two words of its own allocation"""
    SIZE = 16 << 20
    NW = 512

    def __init__(self):
        super().__init__()
        self.dwords = self.alloc(4 * self.NW)
        self.sum = self.alloc(GUARD + 8)

    def load(self, image):
        """the image at the end of the arena, GUARD bytes of 0xA5 in front: its device address"""
        image = np.ascontiguousarray(image)
        p = self.at_end(image.nbytes + GUARD) + GUARD
        if image.nbytes:
            self.put(p, image)
        return p

    def poke(self, p, image, offsets, xor=0x40):
        """flip bits of the bytes at `offsets` of the device image (the host copy stays as it is)"""
        flat = image.reshape(-1)
        for off in offsets:
            self.put(p + int(off), np.array([flat[off] ^ xor], dtype=np.uint8))

    def restore(self, p, image, offsets):
        self.poke(p, image, offsets, 0)

    def run(self, b, p, count, n, entry0, first, eb=32, summary=True):
        """the device form: (diff [count], (summary[0], summary[1]) or None); the words around both are checked"""
        assert count <= self.NW
        self.put(self.dwords, np.full(self.NW, A5, dtype=np.uint32))
        self.put(self.sum, np.full(GUARD // 4 + 2, A5, dtype=np.uint32))
        b.compare_witnesses_device(p, self.dwords + 4 * (self.NW - count), first, count, entry0, n,
                                   d_summary=self.sum + GUARD if summary else None, n8=(eb == 8))
        words = self.download(self.dwords, self.NW, np.uint32)
        s = self.download(self.sum, GUARD // 4 + 2, np.uint32)
        assert (words[:self.NW - count] == A5).all() and (s[:GUARD // 4] == A5).all(), "words in front of d_diff / d_summary were written"
        assert (self.download(p - GUARD, GUARD) == 0xA5).all(), "bytes in front of the image were written"
        if not summary:
            assert (s[GUARD // 4:] == A5).all()
            return words[self.NW - count:], None
        return words[self.NW - count:], (int(s[-2]), int(s[-1]))


@pytest.fixture(scope="module")
def hip():
    return _Cmp()


def _tampers(count, n, eb, full):
    """(instance, entry, byte) of the single-byte tampers: the whole product for the first range of a circuit (and wherever it is
    small), for the others a cut through it in which every PAIR of values of two axes occurs"""
    inst = sorted({j for j in (0, 63, 64, count - 1) if j < count})
    ent = sorted({k for k in (0, 15, 16, 63, 64, n - 1) if k < n})
    byt = (0, 15, 16, 31) if eb == 32 else (0, 7)
    if full or len(ent) < max(len(inst), len(byt)):
        return list(itertools.product(inst, ent, byt))
    # every pair of two axes: the entries times the longer of the other two axes, the shorter one walking along
    if len(byt) >= len(inst):
        return [(inst[(i + j) % len(inst)], k, byte) for i, k in enumerate(ent) for j, byte in enumerate(byt)]
    return [(r, k, byt[(i + j) % len(byt)]) for i, k in enumerate(ent) for j, r in enumerate(inst)]


def _check_range(hip, b, want, first, count, entry0, n, eb, full, host):
    """an equal image, single-byte tampers, the reduction's cases and an image that differs everywhere, for one range"""
    where = (first, count, entry0, n, eb)
    img = np.ascontiguousarray(want[first:first + count, entry0:entry0 + n, :eb])
    p = hip.load(img)
    none = np.full(count, NONE, dtype=np.uint32)
    d, s = hip.run(b, p, count, n, entry0, first, eb)
    assert (d == none).all() and s == (0, NONE), ("equal",) + where + (d[d != NONE][:4].tolist(), s)
    if full:
        d, s = hip.run(b, p, count, n, entry0, first, eb, summary=False)                  # d_summary == NULL
        assert (d == none).all() and s is None, ("no summary",) + where
    for j, k, byte in _tampers(count, n, eb, full):
        off = [(j * n + k) * eb + byte]
        hip.poke(p, img, off)
        d, s = hip.run(b, p, count, n, entry0, first, eb)
        hip.restore(p, img, off)
        exp = none.copy()
        exp[j] = entry0 + k
        assert (d == exp).all() and s == (1, first + j), ("tamper", j, k, byte) + where + (np.flatnonzero(d != NONE)[:4].tolist(), s)
    # the reduction: one instance, several entries - in either order of the writes -, then one entry in each of several tiles
    j = count // 2
    sets = [[3, 40], [40, 3], [5, 70, 140, 300, 600, 1100, n - 1]] if n > 3 else [[n - 1, 0], [0, n - 1]]
    for ks in sets:
        ks = [k for k in ks if k < n]
        offs = [(j * n + k) * eb + (k % eb) for k in ks]
        for off in offs:
            hip.poke(p, img, [off])
        d, s = hip.run(b, p, count, n, entry0, first, eb)
        hip.restore(p, img, offs)
        exp = none.copy()
        exp[j] = entry0 + min(ks)
        assert (d == exp).all() and s == (1, first + j), ("several entries", ks) + where + (d[j], s)
    # an image that differs in every element: every verdict is the range's first entry, every instance counts once
    other = img.copy()
    other.reshape(-1, eb)[np.arange(count * n), np.arange(count * n) % eb] ^= 0x01
    d, s = hip.run(b, hip.load(other), count, n, entry0, first, eb)
    assert (d == entry0).all() and s == (count, first), ("all different",) + where + (s,)
    assert (d == exp_diff(img, other, entry0)).all()
    if host:
        # the host form, staged through the batch's bulk buffer: equal, all different, and a handful of tampered instances
        d, nd, low = b.compare_witnesses(img, entry0, first)
        assert (d == none).all() and (nd, low) == (0, NONE), ("host equal",) + where
        d, nd, low = b.compare_witnesses(other, entry0, first)
        assert (d == entry0).all() and (nd, low) == (count, first), ("host all different",) + where
        some = img.copy()
        for j, k, byte in _tampers(count, n, eb, False):
            some[j, k, byte] ^= 0x80
        d, nd, low = b.compare_witnesses(some, entry0, first)
        exp = exp_diff(img, some, entry0)
        assert (d == exp).all() and (nd, low) == exp_summary(exp, first), ("host tampers",) + where
        # the weaker check: a numpy compare of what cw_get_witnesses hands out
        got = b.witnesses(first, count)[:, entry0:entry0 + n, :eb]
        assert (exp_diff(got, some, entry0) == d).all() and (got == img).all()


def _check_batch(hip, b, want, nw, ebs, B=300):
    for eb in ebs:
        for fi, (first, count) in enumerate(forms(B)):
            for ri, (entry0, n) in enumerate(clip(e, m, nw) for e, m in RANGES):
                _check_range(hip, b, want, first, count, entry0, n, eb, full=(fi == 0 and ri == 0), host=(fi < 2 and ri in (0, 2)))


def _mg():
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(HERE, "golden", "make_golden.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    return mg


@functools.lru_cache(maxsize=None)
def _field_case(name, prime, B=300):
    """(builder, inputs [B][2], signals [B][n_signals][32]) of poseidon2 / opzoo on bn128 / goldilocks: the golden input vectors
    at the head of the batch - the SHA-256 of the oracle's .wtns is the reference runtime's for each -, random instances behind
    them (the second input below the word width: the zoo shifts by it); computed once, shared, never modified"""
    q = PRIMES[prime]
    if prime == "goldilocks":
        from make_golden import goldilocks_cases
        mk, _ = goldilocks_cases()[name]
        vecs = GOLD_GL["cases"][name]["vectors"]
    else:
        mk, _, _ = _mg().cases()[name]
        vecs = GOLD["cases"][name]["vectors"]
    fc = flatten(mk())
    rng = np.random.default_rng(len(name) + q.bit_length())
    ins = [[int.from_bytes(rng.bytes(32), "little") % q, int(rng.integers(0, 64)) if name == "opzoo" else int.from_bytes(rng.bytes(32), "little") % q]
           for _ in range(B)]
    for i, vec in enumerate(vecs):
        ins[i] = [int(v) for v in vec["inputs"]]
    want = np.zeros((B, fc.n_signals, 32), dtype=np.uint8)
    for i, row in enumerate(ins):
        sig, failed = eval_flat(q, fc.n_signals, fc.n_temps, fc.constants, fc.code, {fc.main_input_start + k: v for k, v in enumerate(row)})
        assert failed is None, (name, prime, i)
        if i < len(vecs):
            assert hashlib.sha256(wtns_bytes(q, sig)).hexdigest() == vecs[i]["wtns_sha256"], (name, prime, i)
        want[i] = _image(sig)
    want.setflags(write=False)
    return mk, ins, want


def _field_batch(tmp_path, name, prime, B=300, **kw):
    from circom_amd import runtime as rt
    mk, ins, want = _field_case(name, prime, B)
    cp = compile_program(mk(), str(tmp_path), name, sym=False, **kw)
    c = rt.Circuit(cp.tape_path, cp.dat_path, cp.r1cs_path)
    assert c.n_witness == want.shape[1]
    b = c.batch(B)
    b.set_inputs(ins)
    b.run(); b.sync()
    assert (b.status() == 0).all()
    return c, b, want


# ---- every layout ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_compare_a_witness_of_four_entries(circuits, hip):
    """Multiplier2 on a Montgomery-form table: four entries clip every tile"""
    fc, c = circuits("m2mont")
    assert c.montgomery and c.n_witness == 4
    B = 300
    rng = np.random.default_rng(300)
    ins = [[int.from_bytes(rng.bytes(32), "little") % c.q for _ in range(2)] for _ in range(B)]
    ins[0] = [3, 11]
    want = np.stack([_image(_eval(_flat("m2"), row)[0]) for row in ins])
    vec = GOLD["cases"]["multiplier2"]["vectors"][0]
    assert [int(v) for v in vec["inputs"]] == [3, 11]
    assert hashlib.sha256(wtns_bytes(c.q, [int.from_bytes(v.tobytes(), "little") for v in want[0]])).hexdigest() == vec["wtns_sha256"]
    b = c.batch(B)
    b.set_inputs(ins)
    b.run(); b.sync()
    _check_batch(hip, b, want, 4, (32,))
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["poseidon2", "opzoo"])
def test_gpu_compare_on_the_256_bit_schedule(tmp_path, hip, name):
    """Poseidon(2): a Montgomery-form table of 1 108 entries; the operator zoo: a canonical table of 28"""
    kw = dict(strands=strands_for(300), jit=False, fpjit=False) if name == "poseidon2" else dict(fpjit=False)
    c, b, want = _field_batch(tmp_path, name, "bn128", **kw)
    assert c.montgomery == (1 if name == "poseidon2" else 0) and c.n_witness == (1108 if name == "poseidon2" else 28)
    _check_batch(hip, b, want, c.n_witness, (32,))
    # nothing is repaired: v + q in place of v differs
    img = want[:, :, :].copy()
    j, k = 77, c.n_witness - 2
    v = int.from_bytes(img[j, k].tobytes(), "little")
    img[j, k] = np.frombuffer((v + c.q).to_bytes(32, "little"), dtype=np.uint8)
    d, s = hip.run(b, hip.load(img), 300, c.n_witness, 0, 0)
    assert d[j] == k and s == (1, j) and (np.delete(d, j) == NONE).all()
    b.close(); c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["poseidon2", "opzoo"])
def test_gpu_compare_on_the_64_bit_runtime(tmp_path, hip, name):
    """both element sizes; in the 32-byte form the upper 24 bytes count"""
    c, b, want = _field_batch(tmp_path, name, "goldilocks")
    assert c.element_bytes == 8 and not want[:, :, 8:].any()
    nw = c.n_witness
    _check_batch(hip, b, want, nw, (32, 8))
    q = c.q
    # v + q differs: everywhere in the 32-byte form, in the 8-byte form where it fits (entry 0 is the constant 1)
    img = want.copy()
    j, k = 129, nw - 1
    v = int.from_bytes(img[j, k].tobytes(), "little")
    img[j, k] = np.frombuffer((v + q).to_bytes(32, "little"), dtype=np.uint8)
    d, s = hip.run(b, hip.load(img), 300, nw, 0, 0, 32)
    assert d[j] == k and s == (1, j) and (np.delete(d, j) == NONE).all()
    img8 = np.ascontiguousarray(want[:, :, :8])
    img8[j, 0] = np.frombuffer((1 + q).to_bytes(8, "little"), dtype=np.uint8)
    d, s = hip.run(b, hip.load(img8), 300, nw, 0, 0, 8)
    assert d[j] == 0 and s == (1, j) and (np.delete(d, j) == NONE).all()
    b.close(); c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["interp", "jit", "wide", "gl"])
def test_gpu_compare_bitgadget_on_every_layout(circuits, hip, monkeypatch, kind):
    """BitGadget(15), 380 entries: two waves of the bit kernel, on both bit-table layouts; the same circuit on the 8 x u32 table
    and on the 64-bit runtime"""
    B = 300
    prime = "goldilocks" if kind == "gl" else "bn128"
    c, b = _batch(circuits, monkeypatch, kind, B)
    bits, want = _case(15, prime)
    b.set_inputs_rows(pack_rows(bits[:B], (bits.shape[1] + 7) // 8, True))
    b.run(); b.sync()
    assert (b.status() == 0).all() and c.n_witness == 380
    _check_batch(hip, b, want, 380, (32, 8) if kind == "gl" else (32,))
    if kind in ("interp", "jit"):
        # an element equals the bit only as the 32-byte value 0 or 1: the value 2, the value 3 and a set byte 31 differ, whatever
        # the bit is
        img = want[:B].copy()
        zero = lambda j: int(np.flatnonzero(want[j, :, 0] == 0)[-1])                      # the last entry of instance j that is 0 / 1
        one = lambda j: int(np.flatnonzero(want[j, :, 0] == 1)[-1])
        spots = [(63, zero(63), 0, 2), (64, one(64), 0, 3), (150, zero(150), 31, 0x80), (151, one(151), 31, 1), (299, one(299), 4, 1),
                 (298, zero(298), 16, 1)]
        exp = np.full(B, NONE, dtype=np.uint32)
        for j, k, byte, val in spots:
            assert k > 0 and img[j, k, byte] != val
            img[j, k, byte] = val
            exp[j] = k
        d, s = hip.run(b, hip.load(img), B, 380, 0, 0)
        assert (d == exp).all() and s == (len(spots), 63)
    b.close()


@pytest.mark.gpu
def test_gpu_compare_a_second_workgroup_of_the_bit_kernel(tmp_path, hip, monkeypatch):
    """BitGadget(45): 1 130 entries are a second workgroup of the bit kernel in the element direction (a workgroup holds 1 024)"""
    from circom_amd import runtime as rt
    monkeypatch.setenv("CW_BITS_JIT", "0")
    cp = compile_program(Program(BitGadget(45)), str(tmp_path), "bg45", sym=False, strands=(1,), bits=True, jit=False)
    c = rt.Circuit(cp.tape_path, cp.dat_path, cp.r1cs_path)
    if c.n_witness != cp.flat.n_signals:
        c.set_witness_list(np.arange(c.n_signals, dtype=np.uint32))
    fc = cp.flat
    nw, B = c.n_witness, 130
    assert nw == fc.n_signals and nw > 1024 + 64
    bits = np.random.default_rng(45).integers(0, 2, size=(B, c.n_inputs), dtype=np.uint8)
    want = np.stack([_image(_eval(fc, row)[0]) for row in bits])
    b = c.batch(B)
    assert b.bitmode
    b.set_inputs_rows(pack_rows(bits, (c.n_inputs + 7) // 8, True))
    b.run(); b.sync()
    assert (b.status() == 0).all()
    for fi, (first, count) in enumerate(forms(B)):
        for ri, (entry0, n) in enumerate([(0, nw), (1000, nw - 1000), (1023, 2), (1024, nw - 1024)]):
            _check_range(hip, b, want, first, count, entry0, n, 32, full=(fi == 0 and ri == 0), host=(fi == 0 and ri == 0))
    b.close(); c.close()


# ---- bit-plane batches with re-run instances ---------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["interp", "jit"])
def test_gpu_rerun_instances_are_judged_from_the_side_batch(circuits, hip, monkeypatch, kind):
    """instances 5, 64 and 129 are not boolean: the bit table holds something else for them, the side batch the witness.  An equal
    image is equal for re-run and plain instances alike; a tamper in either kind is found"""
    c, b = _batch(circuits, monkeypatch, kind, 130)
    _, vals, want = _rerun_case()
    _run_values(b, c, vals)
    nw = c.n_witness
    clean = _case(15)[1][:130]
    assert all((want[i] != clean[i]).any() for i in (5, 64, 129))
    for first, count in ((0, 130), (37, 93), (63, 2), (64, 64), (129, 1), (5, 1), (6, 58)):
        for entry0, n in (clip(e, m, nw) for e, m in RANGES):
            img = np.ascontiguousarray(want[first:first + count, entry0:entry0 + n])
            p = hip.load(img)
            d, s = hip.run(b, p, count, n, entry0, first)
            assert (d == NONE).all() and s == (0, NONE), (first, count, entry0, n, np.flatnonzero(d != NONE).tolist())
            inside = sorted({i for i in (5, 64, 129, 6, 65, 128, first) if first <= i < first + count})
            some = img.copy()
            exp = np.full(count, NONE, dtype=np.uint32)
            for t, i in enumerate(inside):
                k = (7 * t + 3) % n
                some[i - first, k, (5 * t) % 32] ^= 0x10
                exp[i - first] = entry0 + k
            d, s = hip.run(b, hip.load(some), count, n, entry0, first)
            assert (d == exp).all() and s == exp_summary(exp, first), (first, count, entry0, n)
            # a re-run instance is not the clean one: the clean row differs from what the side batch computed
            d, s = hip.run(b, hip.load(clean[first:first + count, entry0:entry0 + n]), count, n, entry0, first)
            assert (d == exp_diff(img, clean[first:first + count, entry0:entry0 + n], entry0)).all()
    d, nd, low = b.compare_witnesses(want)
    assert (d == NONE).all() and (nd, low) == (0, NONE)
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["interp", "jit"])
def test_gpu_a_side_batch_that_holds_everything_answers_alone(circuits, hip, monkeypatch, kind):
    odd = tuple(range(3, 130, 3))
    assert len(odd) > 130 // 4
    c, b = _batch(circuits, monkeypatch, kind, 130)
    vals, want, _ = _odd_case("bg15", odd)
    _run_values(b, c, vals)
    nw = c.n_witness
    for first, count in ((0, 130), (37, 93), (129, 1)):
        for entry0, n in (clip(e, m, nw) for e, m in RANGES):
            img = np.ascontiguousarray(want[first:first + count, entry0:entry0 + n])
            d, s = hip.run(b, hip.load(img), count, n, entry0, first)
            assert (d == NONE).all() and s == (0, NONE), (first, count, entry0, n)
            some = img.copy()
            some[count - 1, n - 1, 31] ^= 1
            some[0, 0, 0] ^= 2
            exp = exp_diff(img, some, entry0)
            d, s = hip.run(b, hip.load(some), count, n, entry0, first)
            assert (d == exp).all() and s == exp_summary(exp, first), (first, count, entry0, n)
    b.close()


# ---- state, laziness, read-only ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["interp", "wide", "gl"])
def test_gpu_state_and_read_only(circuits, hip, monkeypatch, kind):
    from circom_amd import runtime as rt
    L = rt.lib()
    B = 130
    prime = "goldilocks" if kind == "gl" else "bn128"
    c, b = _batch(circuits, monkeypatch, kind, B)
    bits, want = _case(15, prime)
    nw = c.n_witness
    img = np.ascontiguousarray(want[:B])
    p = hip.load(img)
    diff = np.full(B, A5, dtype=np.uint32)
    summary = np.full(2, A5, dtype=np.uint32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    # before cw_run
    assert L.cw_compare_witnesses(b.h, 0, nw, 0, B, ptr(img), ptr(diff), ptr(summary)) == CW_ESTATE and "before cw_run" in L.cw_last_error().decode()
    hip.put(hip.dwords, np.full(hip.NW, A5, dtype=np.uint32))
    assert L.cw_compare_witnesses_device(b.h, 0, nw, 0, B, C.c_void_p(p), C.c_void_p(hip.dwords), None) == CW_ESTATE
    assert "before cw_run" in L.cw_last_error().decode()
    assert (diff == A5).all() and (summary == A5).all() and (hip.download(hip.dwords, hip.NW, np.uint32) == A5).all()
    # status words, first-bad rows, a captured graph and the next egress are what they were; before and after cw_check_r1cs
    image = np.zeros((B, c.n_inputs, 32), dtype=np.uint8)
    image[:, :, 0] = bits[:B]
    d_in = hip.upload(image)
    b.set_inputs_device(d_in)
    b.run(); b.sync()
    d, s = hip.run(b, p, B, nw, 0, 0)
    assert (d == NONE).all() and s == (0, NONE)                                           # before cw_check_r1cs
    for _ in range(3):
        b.run_check()
    b.sync()
    captured = b.graph_captured
    st, fb, missing = b.status().copy(), b.r1cs_first_bad().copy(), b.witnesses_missing()
    some = img.copy()
    some[7, 5, 3] ^= 1
    for im, exp in ((img, np.full(B, NONE, dtype=np.uint32)), (some, exp_diff(img, some, 0))):
        d, s = hip.run(b, hip.load(im), B, nw, 0, 0)
        assert (d == exp).all() and s == exp_summary(exp, 0)
        d, nd, low = b.compare_witnesses(im)
        assert (d == exp).all() and (nd, low) == exp_summary(exp, 0)
    assert b.graph_captured == captured and (b.status() == st).all() and (b.r1cs_first_bad() == fb).all() and b.witnesses_missing() == missing
    assert (b.witnesses() == img).all()
    b.run_check(); b.sync()
    assert b.graph_captured == captured and (b.status() == st).all()
    # empty ranges: count == 0 writes no verdict and clears the summary; n == 0 makes every verdict "equal"
    diff[:] = A5
    summary[:] = A5
    assert L.cw_compare_witnesses(b.h, 0, nw, 5, 0, ptr(img), ptr(diff), ptr(summary)) == 0
    assert (diff == A5).all() and summary.tolist() == [0, NONE]
    summary[:] = A5
    assert L.cw_compare_witnesses(b.h, 3, 0, 5, 7, ptr(img), ptr(diff), ptr(summary)) == 0
    assert (diff[:7] == NONE).all() and (diff[7:] == A5).all() and summary.tolist() == [0, NONE]
    d, s = hip.run(b, p, 0, nw, 0, B)
    assert len(d) == 0 and s == (0, NONE)
    d, s = hip.run(b, p, 9, 0, nw, 3)
    assert (d == NONE).all() and s == (0, NONE)
    b.close()


@pytest.mark.gpu
def test_gpu_a_supplied_table_is_served_once_it_is_complete(circuits, hip, monkeypatch):
    from circom_amd import runtime as rt
    B = 130
    c, b = _batch(circuits, monkeypatch, "gl", B)
    _, want = _case(15, "goldilocks")
    img = np.ascontiguousarray(want[:B])
    rows = img[:, :, :8].copy().view("<u8").reshape(B, -1)
    b.set_witnesses(rows[:70], 0)
    with pytest.raises(rt.CwError) as e:
        b.compare_witnesses(img)
    assert e.value.code == CW_ESTATE and "witnesses missing for 60 instances" in str(e.value)
    with pytest.raises(rt.CwError) as e:
        b.compare_witnesses_device(hip.load(img), hip.dwords, 0, B)
    assert e.value.code == CW_ESTATE and "witnesses missing for 60 instances" in str(e.value)
    b.set_witnesses(rows[70:], 70)
    assert b.witnesses_missing() == 0
    for eb in (32, 8):
        im = img[:, :, :eb].copy()
        d, s = hip.run(b, hip.load(im), B, c.n_witness, 0, 0, eb)
        assert (d == NONE).all() and s == (0, NONE)
        im[129, 379, eb - 1] ^= 0x80
        d, s = hip.run(b, hip.load(im), B, c.n_witness, 0, 0, eb)
        assert d[129] == 379 and (d[:129] == NONE).all() and s == (1, 129)
    assert b.witnesses_missing() == 0
    b.close()


# ---- launch pieces ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_a_range_of_more_than_65535_tiles(circuits, hip):
    """Multiplier2 on the 8 x u32 table, 65 535 x 64 + 1 instances: the smallest batch whose range walk is a second launch, of one
    instance.  Inputs below 2^31: the product is exact in 64 bits.  The image is half a gigabyte"""
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
    p = hip.alloc(GUARD + nbytes)                                # the image ends with its allocation
    d_diff = hip.alloc(GUARD + 4 * B)
    hip.h.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    assert hip.h.hipMemset(d_diff, 0xA5, GUARD + 4 * B) == 0
    hip.put(p + GUARD, want)
    hip.put(hip.sum, np.full(GUARD // 4 + 2, A5, dtype=np.uint32))
    b.compare_witnesses_device(p + GUARD, d_diff + GUARD, 0, B, d_summary=hip.sum + GUARD)
    d = hip.download(d_diff, GUARD // 4 + B, np.uint32)
    assert (d[:GUARD // 4] == A5).all() and (d[GUARD // 4:] == NONE).all(), np.flatnonzero(d[GUARD // 4:] != NONE)[:8].tolist()
    assert hip.download(hip.sum + GUARD, 2, np.uint32).tolist() == [0, NONE]
    # a tamper in the last instance (the second launch), one in the last instance of the first launch, one in the very first
    for i, k, byte in ((B - 1, 3, 31), (B - 2, 1, 0), (0, 2, 17)):
        off = (i * 4 + k) * 32 + byte
        hip.put(p + GUARD + off, np.array([want.view(np.uint8).reshape(-1)[off] ^ 0x01], dtype=np.uint8))
    b.compare_witnesses_device(p + GUARD, d_diff + GUARD, 0, B, d_summary=hip.sum + GUARD)
    d = hip.download(d_diff + GUARD, B, np.uint32)
    exp = np.full(B, NONE, dtype=np.uint32)
    exp[[B - 1, B - 2, 0]] = [3, 1, 2]
    assert (d == exp).all(), np.flatnonzero(d != exp)[:8].tolist()
    assert hip.download(hip.sum + GUARD, 2, np.uint32).tolist() == [3, 0]
    # the last instance alone
    b.compare_witnesses_device(p + GUARD + (B - 1) * 128, d_diff + GUARD, B - 1, 1, d_summary=hip.sum + GUARD)
    assert hip.download(d_diff + GUARD, 1, np.uint32)[0] == 3 and hip.download(hip.sum + GUARD, 2, np.uint32).tolist() == [1, B - 1]
    hip.h.hipFree(p)
    hip.h.hipFree(d_diff)
    b.close()


# ---- one batch's egress is the other batch's image -----------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["interp", "jit"])
def test_gpu_cross_engine_compare(circuits, hip, monkeypatch, kind):
    """BitGadget(15) as a bit-plane program and on the 256-bit schedule, the same inputs: cw_get_witnesses_device of one is the
    d_image of the other, both ways.  Then one input bit of one instance is changed in one batch: that instance alone differs, at
    the entry the oracle names"""
    B = 300
    bits, want = _case(15)
    c, bb = _batch(circuits, monkeypatch, kind, B)
    _, bw = _batch(circuits, monkeypatch, "wide", B)
    nw = c.n_witness
    rows = bits[:B].copy()
    for b in (bb, bw):
        b.set_inputs_rows(pack_rows(rows, (rows.shape[1] + 7) // 8, True))
        b.run(); b.sync()
    p = hip.at_end(B * nw * 32 + GUARD) + GUARD
    for src, dst in ((bb, bw), (bw, bb)):
        src.witnesses_device(0, B, p)
        d, s = hip.run(dst, p, B, nw, 0, 0)
        assert (d == NONE).all() and s == (0, NONE)
    assert (hip.download(p, (B, nw, 32)) == want[:B]).all()                               # (and the image is the oracle's)
    i = 201
    rows[i, 4] ^= 1
    sig, failed = _eval(_flat("bg15"), rows[i])
    assert failed is None
    exp = np.full(B, NONE, dtype=np.uint32)
    exp[i] = exp_diff(want[i][None], _image(sig)[None], 0)[0]
    assert exp[i] != NONE
    bw.set_inputs_rows(pack_rows(rows, (rows.shape[1] + 7) // 8, True))
    bw.run(); bw.sync()
    for src, dst in ((bb, bw), (bw, bb)):
        src.witnesses_device(0, B, p)
        d, s = hip.run(dst, p, B, nw, 0, 0)
        assert (d == exp).all() and s == (1, i)
    bb.close(); bw.close()


# ---- files and the command line ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["interp", "wide", "gl"])
def test_gpu_compare_wtns_files(circuits, tmp_path, monkeypatch, kind):
    from circom_amd import runtime as rt
    B = 70
    prime = "goldilocks" if kind == "gl" else "bn128"
    c, b = _batch(circuits, monkeypatch, kind, B)
    bits, want = _case(15, prime)
    b.set_inputs_rows(pack_rows(bits[:B], (bits.shape[1] + 7) // 8, True))
    b.run(); b.sync()
    n8, nw = c.element_bytes, c.n_witness
    head = wtns_bytes(c.q, [0] * nw)[:44 + n8]
    ints = lambda i: [int.from_bytes(v.tobytes(), "little") for v in want[i]]
    assert wtns_bytes(c.q, ints(0)) == head + want[0, :, :n8].tobytes()
    # the batch's own files, then the oracle's files
    b.write_wtns_many(0, B, str(tmp_path / "own_%d.wtns"))
    d, nd, low = b.compare_wtns_many(0, B, str(tmp_path / "own_%d.wtns"))
    assert (d == NONE).all() and (nd, low) == (0, NONE)
    for i in range(B):
        (tmp_path / ("ref_%d.wtns" % i)).write_bytes(head + want[i, :, :n8].tobytes())
    assert (tmp_path / "own_69.wtns").read_bytes() == (tmp_path / "ref_69.wtns").read_bytes()
    d, nd, low = b.compare_wtns_many(0, B, str(tmp_path / "ref_%d.wtns"))
    assert (d == NONE).all() and (nd, low) == (0, NONE)
    d, nd, low = b.compare_wtns_many(37, 33, str(tmp_path / "ref_%u.wtns"))
    assert len(d) == 33 and (d == NONE).all() and (nd, low) == (0, NONE)
    assert b.compare_wtns(69, tmp_path / "ref_69.wtns") == NONE and b.compare_wtns(0, tmp_path / "ref_0.wtns") == NONE
    assert b.compare_wtns(3, tmp_path / "ref_4.wtns") == exp_diff(want[3:4, :, :n8], want[4:5, :, :n8], 0)[0] != NONE
    # one body byte of one file flipped: that instance, that entry
    raw = bytearray((tmp_path / "ref_64.wtns").read_bytes())
    raw[len(head) + 200 * n8 + n8 - 1] ^= 0x20
    (tmp_path / "ref_64.wtns").write_bytes(bytes(raw))
    d, nd, low = b.compare_wtns_many(0, B, str(tmp_path / "ref_%d.wtns"))
    assert d[64] == 200 and (np.delete(d, 64) == NONE).all() and (nd, low) == (1, 64)
    assert b.compare_wtns(64, tmp_path / "ref_64.wtns") == 200
    # a file with a wrong header is CW_EIO with the path and the reason - not a difference
    raw = bytearray(head + want[5, :, :n8].tobytes())
    raw[4] = 3                                                                            # version 3
    (tmp_path / "ref_5.wtns").write_bytes(bytes(raw))
    with pytest.raises(rt.CwError) as e:
        b.compare_wtns_many(0, B, str(tmp_path / "ref_%d.wtns"))
    assert e.value.code == CW_EIO and "ref_5.wtns" in str(e.value) and "version" in str(e.value)
    with pytest.raises(rt.CwError) as e:
        b.compare_wtns(5, tmp_path / "ref_5.wtns")
    assert e.value.code == CW_EIO
    d, nd, low = b.compare_wtns_many(6, 3, str(tmp_path / "ref_%d.wtns"))                   # (a range without it)
    assert (d == NONE).all() and (nd, low) == (0, NONE)
    d, nd, low = b.compare_wtns_many(6, 0, str(tmp_path / "ref_%d.wtns"))
    assert len(d) == 0 and (nd, low) == (0, NONE)
    b.close()


@pytest.mark.gpu
def test_gpu_cli_compare(tmp_path):
    from circom_amd import runtime as rt
    cp = compile_program(Program(Multiplier2()), str(tmp_path), "multiplier2", sym=True, fpjit=False)
    assert os.path.exists(cp.sym_path)
    q = PRIMES["bn128"]
    prefix = os.path.join(str(tmp_path), "multiplier2")
    (tmp_path / "in.json").write_text('[{"a": "3", "b": "11"}, {"a": "5", "b": "7"}, {"a": "2", "b": "2"}]')
    (tmp_path / "one.json").write_text('{"a": "3", "b": "11"}')
    wits = [[1, 33, 3, 11], [1, 35, 5, 7], [1, 4, 2, 2]]
    for i, w in enumerate(wits):
        (tmp_path / ("ref_%d.wtns" % i)).write_bytes(wtns_bytes(q, w))
    before = sorted(os.listdir(tmp_path))
    run = lambda *args: subprocess.run([str(rt.CLI_PATH)] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    r = run("--compare", prefix, tmp_path / "in.json", tmp_path / "ref_%d.wtns")
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.splitlines() == ["instance %d: OK" % i for i in range(3)]
    r = run("--compare", prefix, tmp_path / "in.json", tmp_path / "ref_%01u.wtns")          # a width, as the library's patterns allow
    assert r.returncode == 0 and r.stdout.splitlines() == ["instance %d: OK" % i for i in range(3)], r.stdout + r.stderr
    r = run("--compare", prefix, tmp_path / "one.json", tmp_path / "ref_0.wtns")
    assert r.returncode == 0 and r.stdout.splitlines() == ["instance 0: OK"], r.stdout + r.stderr
    # another calculator's answer differs in entry 1 of instance 1 (and v + q is not v)
    (tmp_path / "ref_1.wtns").write_bytes(wtns_bytes(q, [1, 36, 5, 7]))
    (tmp_path / "ref_2.wtns").write_bytes(wtns_bytes(q, [1, 4, 2, 2 + q]))
    r = run("--compare", prefix, tmp_path / "in.json", tmp_path / "ref_%d.wtns")
    assert r.returncode == 1, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    names = cp.flat.signal_names()
    assert len(lines) == 3 and lines[0] == "instance 0: OK"
    assert lines[1].startswith("instance 1: entry 1 differs") and names[1] in lines[1]
    assert lines[2].startswith("instance 2: entry 3 differs") and names[3] in lines[2]
    os.rename(cp.sym_path, cp.sym_path + ".away")                                        # without the .sym: no name
    r = run("--compare", prefix, tmp_path / "in.json", tmp_path / "ref_%d.wtns")
    assert r.returncode == 1 and r.stdout.splitlines()[1] == "instance 1: entry 1 differs"
    os.rename(cp.sym_path + ".away", cp.sym_path)
    # usage and I/O
    assert run("--compare", prefix, tmp_path / "in.json").returncode == 2
    assert run("--compare", prefix, tmp_path / "in.json", tmp_path / "ref_0.wtns").returncode == 2          # three inputs need a pattern
    assert run("--compare", prefix, tmp_path / "in.json", tmp_path / "absent_%d.wtns").returncode == 2
    (tmp_path / "ref_0.wtns").write_bytes(wtns_bytes(q, wits[0])[:-1])
    r = run("--compare", prefix, tmp_path / "in.json", tmp_path / "ref_%d.wtns")
    assert r.returncode == 2 and "ref_0.wtns" in r.stderr
    assert sorted(os.listdir(tmp_path)) == before                                          # --compare wrote no file
