"""Life cycle of a batch's device memory (csrc/cw_devbuf.h, cw_batch_free): batches of every engine are created, run, checked,
read back and freed over and over; the buffers that grow on demand (side batch + its instance list, the bulk staging, the packed
masks) grow, are reused and go; a batch is freed straight after a replay of its captured graph.  Everything read back is compared
with oracle.tape_eval, and the device must be no fuller after the cycles than before.

Free device memory is read with hipMemGetInfo after hipDeviceSynchronize through the runtime the library itself uses (_Hip:
torch bundles a second HIP runtime, which cannot initialise in a process where the first one already has).  The allowed
difference per test is what the same test measured on the commit before DevBuf (PARENT_DIFF, bytes: module loads and the
runtime's own pools) plus one allocation granule, read from two successive 1-byte hipMallocs; a difference that grows with the
number of cycles fails whatever its size."""
import ctypes as C
import hashlib

import numpy as np
import pytest

from circom_amd.compiler import compile_program
from circom_amd.frontend.dsl import Program
from oracle.tape_eval import eval_flat

pytestmark = [pytest.mark.gpu, pytest.mark.xdist_group("batch_lifetime")]

# largest before/after difference of free device memory of each test on the parent commit, bytes (this file run in one process
# in file order on an MI355X; the first test also pays for the runtime's start: its pools and the library's code objects).
# This commit measured the same nine figures.
PARENT_DIFF = {"strands": 195035136, "pipelined": 0, "emitted": 2097152, "bits": 4194304, "u64": 2097152,
               "side_batch": 41943040, "bulk": 2097152, "pmask": 0, "graph": 4194304}


class _Mem:
    def __init__(self):
        from test_bitplane import _Hip
        self.hip = _Hip()
        self.hip.h.hipMemGetInfo.argtypes = [C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
        a, b = self.hip.alloc(1), self.hip.alloc(1)
        self.granule = abs(b - a)
        self.hip.h.hipFree(a); self.hip.h.hipFree(b)

    def free(self):
        f, t = C.c_size_t(), C.c_size_t()
        assert self.hip.h.hipDeviceSynchronize() == 0
        assert self.hip.h.hipMemGetInfo(C.byref(f), C.byref(t)) == 0
        return f.value

    def check(self, name, before, after, mid=None):
        print("LIFETIME %s: free before %d, after %d, difference %d (half way: %s), granule %d, parent %d" % (
            name, before, after, before - after, None if mid is None else before - mid, self.granule, PARENT_DIFF[name]))
        if mid is not None:
            assert before - mid == before - after, "the difference grows with the number of cycles"
        assert before - after <= PARENT_DIFF[name] + self.granule


@pytest.fixture(scope="module")
def mem():
    return _Mem()


def _oracle(cp, row):
    fc = cp.flat
    sig, failed = eval_flat(fc.fp.q, fc.n_signals, fc.n_temps, fc.constants, fc.code, {fc.main_input_start + k: v for k, v in enumerate(row)})
    assert failed is None
    return sig


def _ints(img):
    return [int.from_bytes(img[k].tobytes(), "little") for k in range(img.shape[0])]


def _circuit(tmp_path, prog, name, **kw):
    from circom_amd import runtime as rt
    cp = compile_program(prog, str(tmp_path), name, sym=False, **kw)
    return cp, rt.Circuit(cp.tape_path, cp.dat_path, cp.r1cs_path)


def _sha_rows(n, seed):
    rng = np.random.default_rng(seed)
    msgs = [rng.bytes(8) for _ in range(n)]
    return msgs, [[(m[k // 8] >> (7 - k % 8)) & 1 for k in range(64)] for m in msgs]


ENGINES = ["strands", "pipelined", "emitted", "bits", "u64"]


@pytest.mark.parametrize("engine", ENGINES)
def test_create_run_check_free_cycles(engine, tmp_path, monkeypatch, mem):
    """(a) one circuit per engine, batch 64, 20 cycles; the figure after 10 cycles must be the figure after 20"""
    from circom_amd.circuits.basic import Multiplier2, Num2Bits
    from circom_amd.circuits.poseidon import Poseidon
    from circom_amd.circuits.sha256 import Sha256
    B = 64
    rng = np.random.default_rng(5)
    if engine == "strands":
        monkeypatch.setenv("CW_PIPE", "0"); monkeypatch.setenv("CW_FP_JIT", "0")
        cp, c = _circuit(tmp_path, Program(Num2Bits(16)), "num2bits16")
        rows = [[int(rng.integers(0, 1 << 16))] for _ in range(B)]
        is_engine = lambda b: b.strands >= 1 and b.pipelined is None and not b.emitted and not b.bitmode
    elif engine == "pipelined":
        monkeypatch.setenv("CW_PIPE", "1")
        cp, c = _circuit(tmp_path, Program(Poseidon(2)), "poseidon2", pipe=(8, 8))
        rows = [[int.from_bytes(rng.bytes(32), "little") % c.q for _ in range(2)] for _ in range(B)]
        is_engine = lambda b: b.pipelined == (8, 8)
    elif engine == "emitted":
        monkeypatch.setenv("CW_PIPE", "0")
        cp, c = _circuit(tmp_path, Program(Multiplier2()), "multiplier2")
        rows = [[int.from_bytes(rng.bytes(32), "little") % c.q for _ in range(2)] for _ in range(B)]
        is_engine = lambda b: b.emitted and b.pipelined is None
    elif engine == "bits":
        cp, c = _circuit(tmp_path, Program(Sha256(64)), "sha256_64", bits=True)
        rows = _sha_rows(B, 6)[1]
        is_engine = lambda b: b.bitmode and not b.jit
    else:
        import os
        import sys
        sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
        from make_golden import goldilocks_cases
        mk, _ = goldilocks_cases()["poseidon2"]
        cp, c = _circuit(tmp_path, mk(), "poseidon2_g")
        rows = [[int(rng.integers(0, 1 << 63)) % c.q for _ in range(c.n_inputs)] for _ in range(B)]
        is_engine = lambda b: b.strands == 0 and not b.bitmode
    sample = (0, 1, B - 1)
    want = {i: _oracle(cp, rows[i]) for i in sample}
    before = mem.free()
    mid = None
    for cycle in range(20):
        b = c.batch(B)
        assert is_engine(b), (b.strands, b.pipelined, b.emitted, b.bitmode)
        b.set_inputs(rows)
        b.run()
        if c.n_constraints:
            b.check_r1cs()
        b.sync()
        assert (b.status() == 0).all(), cycle
        img = b.witnesses()
        for i in sample:
            assert _ints(img[i]) == want[i], (cycle, i)
        b.close()
        if cycle == 9:
            mid = mem.free()
    mem.check(engine, before, mem.free(), mid)
    c.close()


def test_side_batch_comes_grows_and_goes(tmp_path, mem):
    """(b) bit-plane batch of 128: 3 instances with an input that is not a bit (side batch + instance list appear), then 40 (the
    side batch is replaced, the list grows), then none (the side batch is dropped)"""
    from circom_amd.circuits.sha256 import Sha256
    cp, c = _circuit(tmp_path, Program(Sha256(64)), "sha256_64", bits=True)
    B = 128
    rows0 = _sha_rows(B, 7)[1]
    before = mem.free()
    b = c.batch(B)
    assert b.bitmode
    for odd in ([3, 64, 127], list(range(5, 125, 3)), []):
        assert len(odd) in (3, 40, 0)
        rows = [list(r) for r in rows0]
        for i in odd:
            rows[i][i % 64] = 2 + i
        b.set_inputs(rows)
        b.run(); b.check_r1cs(); b.sync()
        st = b.status()
        img = b.witnesses()
        for i in sorted(set(odd[:2] + odd[-1:] + [0, 4, B - 2])):
            fc = cp.flat
            sig, failed = eval_flat(fc.fp.q, fc.n_signals, fc.n_temps, fc.constants, fc.code, {fc.main_input_start + k: v for k, v in enumerate(rows[i])})
            assert (failed is None) == (st[i] & 3 == 0), i
            assert _ints(img[i]) == sig and b.witness(i) == sig, (len(odd), i)
    b.close()
    mem.check("side_batch", before, mem.free())
    c.close()


def test_bulk_staging_grows_once_and_is_reused(tmp_path, mem):
    """(c) cw_get_witnesses with count 64, 256, 64 on a batch of 256: bytes equal the per-instance getter's"""
    from circom_amd.circuits.poseidon import Poseidon
    cp, c = _circuit(tmp_path, Program(Poseidon(2)), "poseidon2")
    B = 256
    rng = np.random.default_rng(8)
    rows = [[int.from_bytes(rng.bytes(32), "little") % c.q for _ in range(2)] for _ in range(B)]
    before = mem.free()
    b = c.batch(B)
    b.set_inputs(rows)
    b.run(); b.check_r1cs(); b.sync()
    assert (b.status() == 0).all()
    one = [b.witness_bytes(i) for i in range(B)]
    assert b.witness(0) == _oracle(cp, rows[0]) and b.witness(B - 1) == _oracle(cp, rows[B - 1])
    for first, count in ((100, 64), (0, 256), (192, 64)):
        assert b.witnesses(first, count).tobytes() == b"".join(one[first:first + count]), (first, count)
    b.close()
    mem.check("bulk", before, mem.free())
    c.close()


def test_packed_masks_are_set_twice(tmp_path, mem):
    """(d) cw_set_inputs_bits twice on one batch: the second call reuses the device copy of the masks"""
    from circom_amd.circuits.sha256 import Sha256
    cp, c = _circuit(tmp_path, Program(Sha256(64)), "sha256_64", bits=True)
    B = 100
    before = mem.free()
    b = c.batch(B)
    assert b.bitmode
    for seed in (9, 10):
        msgs, rows = _sha_rows(B, seed)
        masks = np.zeros(((B + 63) // 64, 64), dtype=np.uint64)
        for i, r in enumerate(rows):
            for k, v in enumerate(r):
                masks[i // 64, k] |= np.uint64(v << (i % 64))
        b.set_inputs_bits(masks)
        b.run(); b.check_r1cs(); b.sync()
        assert (b.status() == 0).all()
        for i in (0, 63, 64, B - 1):
            digest = hashlib.sha256(msgs[i]).digest()
            assert [b.signal(i, 1 + k) for k in range(256)] == [(digest[k // 8] >> (7 - k % 8)) & 1 for k in range(256)], (seed, i)
        assert b.witness(B - 1) == _oracle(cp, rows[B - 1])
    b.close()
    mem.check("pmask", before, mem.free())
    c.close()


def test_free_straight_after_a_graph_replay(tmp_path, mem):
    """(e) cw_run_check until the graph is captured, one replay, then cw_batch_free with no cw_sync in between - a caller's ordinary
    teardown; a fresh batch then computes correct witnesses"""
    from circom_amd.circuits.poseidon import Poseidon
    cp, c = _circuit(tmp_path, Program(Poseidon(2)), "poseidon2")
    B = 256
    rng = np.random.default_rng(12)
    rows = [[int.from_bytes(rng.bytes(32), "little") % c.q for _ in range(2)] for _ in range(B)]
    img = np.frombuffer(b"".join(int(v).to_bytes(32, "little") for r in rows for v in r), dtype=np.uint8)
    before = mem.free()
    d_in = mem.hip.upload(img)
    b = c.batch(B)
    b.set_inputs_device(d_in)
    for _ in range(4):
        b.run_check()
        if b.graph_captured:
            break
    assert b.graph_captured
    b.run_check()                                      # a replay ...
    b.close()                                          # ... and the batch goes while nothing has waited for it
    b = c.batch(B)
    b.set_inputs_device(d_in)
    b.run(); b.check_r1cs(); b.sync()
    assert (b.status() == 0).all()
    for i in (0, 1, B - 1):
        assert b.witness(i) == _oracle(cp, rows[i]), i
    b.close()
    assert mem.hip.h.hipFree(d_in) == 0
    mem.check("graph", before, mem.free())
    c.close()
