"""Several batches of one circuit in flight, each on its own non-blocking HIP stream - the mode every headline number is measured
in - against the stream-ordered contract of include/circom_amd.h: "all work of this batch is enqueued on" the batch's stream, the
device egress forms are "asynchronous on the batch's stream", device inputs, supplied witnesses and index lists are "read in stream
order and may be reused once the batch's stream has passed the call".  On the null stream, where every other test of the suite
runs, everything is serialised with everything: a launch that names stream 0, a host getter that forgets to drain its stream or a
lazily made buffer uploaded on one stream and read on another would all pass there.

Every GPU test: N = 4 batches of one circuit, each on its own stream with its own device input and output buffers.  Instance i of
batch j in round r is a function of (i, j, r) that collides nowhere, so a value from another batch or from the previous round is a
mismatch.  Within a round, batch after batch and with no host synchronisation by the test: new inputs into the batch's buffer with
hipMemcpyAsync on its stream, the step, the device egress forms, a device-to-device copy of each result into a second buffer on
the same stream.  Only then are the streams synchronised and the copies downloaded.

Expected values: for every word, one further batch on the null stream that runs the same inputs alone with a sync() after every
call (it isolates the ordering); and, independently of the library, eval_flat / check_r1cs on 8 instances per batch and round and
hashlib.sha256 for every instance of the SHA circuit.

FlakyChain breaks one row in EVERY instance (a mod n is always a link of the chain), so its verdict is the same everywhere and only
its first-bad rows differ; where a test needs lists that are neither empty nor full it uses MixedChain below, whose instances pass
for about half of the residues.  The CPU part checks these preconditions with the oracle alone."""
import ctypes as C
import functools
import hashlib
import os

import numpy as np
import pytest

from circom_amd.circuits.poseidon import Poseidon
from circom_amd.circuits.sha256 import Sha256
from circom_amd.compiler import compile_program
from circom_amd.frontend.dsl import Program, template
from circom_amd.frontend.flatten import flatten
from oracle.tape_eval import check_r1cs, eval_flat
from test_bitplane import BadBit, _Hip
from test_gpu_parity import FlakyChain

N = 4                      # batches in flight: the hardware queues a process gets by default
F0, CNT = 59, 101          # the odd sub-range of the ranged egress forms: instances 59 .. 159, over two 64-boundaries
NONE = 0xFFFFFFFF
R1CS = 4                   # ST_R1CS_FAILED
# One worker for the GPU tests: the circuits are compiled once, and it is the worker of tests/test_batch_lifetime.py, which reads the
# device's free memory before and after its cycles - this module's buffers of tens of MB must not come and go beside those
GROUP = "batch_lifetime"


@template
def BadSquare(cx):
    """tests/test_run_check_graph.py's: a witness hint that is wrong for odd inputs"""
    a = cx.input("a")
    out = cx.output("out")
    cx.hint(out, a * a + (a & 1))
    cx.enforce(out, a * a, runtime_check=False)


@template
def MixedChain(c, n):
    """FlakyChain with the residue taken mod 2 n - 1: the instances with a mod (2 n - 1) >= n break no link and pass"""
    a = c.input("a")
    b = c.input("b")
    out = c.output("out")
    x = c.signal("x", n + 1)
    c.set(x[0], a + b)
    for k in range(n):
        c.hint(x[k + 1], x[k] * x[k] + b + (a % (2 * n - 1)).eq(k))
        c.enforce(x[k + 1], x[k] * x[k] + b, runtime_check=False)
    c.set(out, x[n] * 3 + x[1])


# ---- circuits and inputs -----------------------------------------------------------------------------------------------------
PROGRAMS = {
    "pos2": lambda: Program(Poseidon(2)),
    "flaky100": lambda: Program(FlakyChain(100)),
    "flaky9m": lambda: Program(FlakyChain(9)),                    # compiled with CW_MONT=1: the fused check's circuit
    "mixed9": lambda: Program(MixedChain(9)),
    "sha64": lambda: Program(Sha256(64)),
    "badbit4": lambda: Program(BadBit(4)),
    "pos2gl": lambda: Program(Poseidon(2), prime="goldilocks"),
    "badsqgl": lambda: Program(BadSquare(), prime="goldilocks"),
}
BITS = ("sha64", "badbit4")
# case -> (circuit, variables at batch creation, instances per batch).  B = 1 093 = 17 groups of 64 + 5, 2 117 = 33 groups + 5.
# BadSquare is one multiplication: only from 16 x 1 093 = 17 488 instances (273 groups + 16) does its step outlast a launch, so
# that a reader on the wrong stream sees a stale result (measured: 0 of 20 trials up to 4 372, 1 at 8 744, 20 at 17 488)
CASES = {
    "interp-poseidon": ("pos2", {"CW_FP_JIT": "0"}, 1093),
    "interp-flaky": ("flaky100", {"CW_FP_JIT": "0"}, 1093),
    "emitted-poseidon": ("pos2", {}, 1093),
    "fused-flaky": ("flaky9m", {"CW_FP_FUSED": "1"}, 1093),
    "bits-interp-sha": ("sha64", {"CW_BITS_JIT": "0"}, 2117),
    "bits-emitted-sha": ("sha64", {"CW_BITS_JIT": "1"}, 2117),
    "gl-poseidon": ("pos2gl", {}, 1093),
    "gl-badsquare": ("badsqgl", {}, 17488),
    # the circuits of (c): verdicts differ from instance to instance
    "wide-mixed": ("mixed9", {}, 1093),
    "bits-interp-badbit": ("badbit4", {"CW_BITS_JIT": "0"}, 1093),
    "bits-emitted-badbit": ("badbit4", {"CW_BITS_JIT": "1"}, 1093),
}
ENGINES = ["interp-poseidon", "interp-flaky", "emitted-poseidon", "fused-flaky", "bits-interp-sha", "bits-emitted-sha", "gl-poseidon",
           "gl-badsquare"]
# (b), bit engines: instance -> (input, value).  Both inputs are bits of message word 0, which SHA-256 only ever adds (words 1 to
# 15 also go through the xors of sigma0 / sigma1, where a value that is no bit turns into field-sized values that fail the adders'
# assertions): the value is carried into the sum and the instance fails no assertion
NONBOOL = {5: (31, 7), -1: (30, 3)}


@functools.lru_cache(maxsize=None)
def _flat(circ):
    return flatten(PROGRAMS[circ]())


def _key(B, j, r):
    """[B] uint64 below 2^40, injective in (i, j, r): i * m_j + 7 r stays below 2^24"""
    i = np.arange(B, dtype=np.uint64)
    return np.uint64(1) + i * np.uint64((7, 11, 13, 19)[j]) + np.uint64(7 * r) + np.uint64((j << 24) + (r << 32))


def _mix(B, j, r):
    """[B] uint64 of well-mixed bits of (i, j, r)"""
    x = _key(B, j, r) * np.uint64(0x9E3779B97F4A7C15)
    return x ^ (x >> np.uint64(29))


@functools.lru_cache(maxsize=None)
def inputs(circ, B, j, r, nonbool=False):
    """[B][n_inputs] of Python ints: the inputs of batch j in round r (computed once, shared, never modified)"""
    k = _key(B, j, r)
    if circ == "sha64":                                           # the message: 8 bytes, the key in the low 40 bits
        m = k | ((_mix(B, j, r) >> np.uint64(40)) << np.uint64(40))
        rows = np.unpackbits(m.astype(">u8").view(np.uint8).reshape(B, 8), axis=1).astype(object)
        if nonbool:
            q = _flat(circ).fp.q
            for i, (col, v) in NONBOOL.items():
                rows[i, col] = v % q
        return rows
    if circ == "badbit4":                                         # 8 bits: zero (the only rows that pass) for two residues in five
        h = _mix(B, j, r)
        byte = np.where((h >> np.uint64(20)) % np.uint64(5) < 2, 0, 1 + (h >> np.uint64(32)) % np.uint64(255)).astype(np.uint8)
        return np.unpackbits(byte.reshape(B, 1), axis=1).astype(object)
    if circ == "badsqgl":                                         # odd (wrong) for two residues of the mixed bits in three
        return (np.uint64(2) * k + ((_mix(B, j, r) >> np.uint64(33)) % np.uint64(3) != 0).astype(np.uint64)).astype(object).reshape(B, 1)
    a = k | ((_mix(B, j, r) >> np.uint64(44)) << np.uint64(40))   # the key below 20 mixed bits: a mod n is spread evenly
    return np.stack([a, np.uint64(3) + np.uint64(5) * a], axis=1).astype(object)


def image(rows):
    """[B][n_inputs][32] uint8, little-endian"""
    B, n = rows.shape
    out = np.zeros((B, n, 32), dtype=np.uint8)
    try:
        out[:, :, :8] = rows.astype(np.uint64).astype("<u8").reshape(B, n, 1).view(np.uint8)
        return out
    except OverflowError:                                         # some value needs more than 8 bytes
        pass
    small = np.array([[int(v) < (1 << 64) for v in row] for row in rows])
    out[:, :, :8] = np.where(small, rows, 0).astype(np.uint64).astype("<u8").reshape(B, n, 1).view(np.uint8)
    for i, k in zip(*np.nonzero(~small)):
        out[i, k] = np.frombuffer(int(rows[i, k]).to_bytes(32, "little"), dtype=np.uint8)
    return out


def digests(rows):
    """[B][32]: hashlib's digest of every message of a sha64 input array (boolean rows only)"""
    msgs = np.packbits(rows.astype(np.uint8), axis=1)
    return np.stack([np.frombuffer(hashlib.sha256(m.tobytes()).digest(), dtype=np.uint8) for m in msgs])


def samples(B, j, r):
    """at least 8 instances: the first, the last, one on each side of a 64-boundary (both inside the ranged egress), four of (i, j, r)"""
    s = [0, B - 1, 63, 64]
    k = 0
    while len(s) < 8:
        i = (7 * j + 13 * r + 101 * k + 5) % B
        k += 1
        if i not in s:
            s.append(i)
    return s


def evaluate(fc, row):
    """(signals, failed assertion or None, first violated row or None) of the oracle"""
    sig, failed = eval_flat(fc.fp.q, fc.n_signals, fc.n_temps, fc.constants, fc.code, {fc.main_input_start + k: int(v) for k, v in enumerate(row)})
    return sig, failed, check_r1cs(fc.fp.q, fc.constraints, sig)


# ---- without a GPU: the preconditions ------------------------------------------------------------------------------------------
def _rounds_of(case):
    return [(j, r) for j in range(N) for r in range(6)]           # (d) uses six rounds, the others fewer


@pytest.mark.parametrize("case", [k for k in CASES if CASES[k][0] not in ("sha64", "badbit4")])
def test_inputs_give_distinct_witnesses_across_batches_and_rounds(case):
    """a value of another batch, or of this batch's previous round, can never pass for the right one: at every sampled instance
    the inputs, the output and the last wire differ between any two (batch, round)"""
    circ, _, B = CASES[case]
    fc = _flat(circ)
    seen = {}
    for j, r in _rounds_of(case):
        rows = inputs(circ, B, j, r)
        assert len({tuple(row) for row in rows.tolist()}) == B
        for i in (0, 63, 64, B - 1):
            sig, failed, _ = evaluate(fc, rows[i])
            assert failed is None
            for wire in (1, fc.main_input_start, fc.n_signals - 1):
                assert seen.setdefault((i, wire, sig[wire]), (j, r)) == (j, r), (i, wire, j, r)
    everything = [inputs(circ, B, j, r)[:, 0] for j, r in _rounds_of(case)]
    assert len(set(np.concatenate(everything).tolist())) == B * len(everything)       # no input value occurs twice anywhere


def test_sha_messages_and_digests_are_distinct_everywhere():
    B = CASES["bits-emitted-sha"][2]
    msgs, digs = set(), set()
    for j, r in _rounds_of("bits-emitted-sha"):
        rows = inputs("sha64", B, j, r)
        msgs |= {m.tobytes() for m in np.packbits(rows.astype(np.uint8), axis=1)}
        digs |= {d.tobytes() for d in digests(rows)}
    assert len(msgs) == len(digs) == B * N * 6


@pytest.mark.parametrize("case", ["wide-mixed", "gl-badsquare", "bits-emitted-badbit", "interp-flaky", "fused-flaky"])
def test_verdicts_differ_within_every_batch(case):
    """MixedChain / BadSquare / BadBit: every batch has passing and failing instances in every round, at most half pass, and the
    pattern differs between any two (batch, round).  FlakyChain: every instance fails (see the module's docstring); its first-bad
    rows take every value the chain has"""
    circ, _, B = CASES[case]
    fc = _flat(circ)
    patterns = []
    for j, r in _rounds_of(case):
        rows = inputs(circ, B, j, r)
        known = {}
        fb = []
        if circ == "badsqgl":                                     # the oracle on every 16th instance: the verdict is the parity of a ...
            for row in rows[5::16].tolist():
                assert (evaluate(fc, row)[2] is None) == (row[0] % 2 == 0)
            patterns.append(np.array([v % 2 == 0 for v in rows[:, 0]]))               # ... which then counts all of them
            assert 1 <= patterns[-1].sum() <= B // 2, (j, r)
            continue
        for row in (rows[3::7] if circ.startswith("flaky") else rows).tolist():       # (a chain of 100 links: every 7th instance)
            key = tuple(row) if circ == "badbit4" else None
            if key is None or key not in known:
                sig, failed, bad = evaluate(fc, row)
                assert failed is None
                known[key] = bad
            fb.append(known[key])
        passed = sum(1 for x in fb if x is None)
        if circ.startswith("flaky"):
            assert passed == 0 and len(set(fb)) >= min(int(circ.rstrip("m")[5:]), 32), (j, r)
        else:
            assert 1 <= passed <= B // 2, (j, r, passed)
        patterns.append(np.array([x is None for x in fb]))
    if not circ.startswith("flaky"):
        for a in range(len(patterns)):
            for b in range(a):
                assert (patterns[a] != patterns[b]).sum() >= B // 8, (a, b)


def test_the_non_boolean_sha_instances_fail_no_assertion():
    """(b) on the bit engines: the side batch must serve these instances, and a failed assertion would end them early"""
    fc = _flat("sha64")
    B = CASES["bits-emitted-sha"][2]
    for j in range(N):
        rows = inputs("sha64", B, j, 3, nonbool=True)
        for i, (col, v) in NONBOOL.items():
            assert rows[i, col] == v % fc.fp.q and rows[i, col] > 1
            sig, failed, bad = evaluate(fc, rows[i])
            assert failed is None, (j, i, failed)
            assert any(s > 1 for s in sig[1 + 256:])              # ... and the value does reach the table


# ---- GPU -----------------------------------------------------------------------------------------------------------------------
class _Streams(_Hip):
    """test_bitplane._Hip (the same libamdhip64.so, no second HIP runtime in the process) with streams and stream-ordered copies.
    Host images are kept alive until the object goes."""

    def __init__(self):
        super().__init__()
        h = self.h
        h.hipStreamCreateWithFlags.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
        h.hipStreamSynchronize.argtypes = [C.c_void_p]
        h.hipStreamDestroy.argtypes = [C.c_void_p]
        h.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        h.hipMemsetAsync.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]
        self.keep, self.bufs, self.streams = [], [], []

    def stream(self):
        s = C.c_void_p()
        assert self.h.hipStreamCreateWithFlags(C.byref(s), 1) == 0                    # hipStreamNonBlocking
        self.streams.append(s.value)
        return s.value

    def buf(self, n):
        p = self.alloc(max(n, 16))
        self.bufs.append(p)
        return p

    def h2d(self, p, arr, stream):
        arr = np.ascontiguousarray(arr)
        self.keep.append(arr)
        assert self.h.hipMemcpyAsync(p, arr.ctypes.data, arr.nbytes, 1, stream) == 0

    def d2d(self, dst, src, n, stream):
        assert self.h.hipMemcpyAsync(dst, src, n, 3, stream) == 0

    def fill(self, p, byte, n, stream):
        assert self.h.hipMemsetAsync(p, byte, n, stream) == 0

    def wait(self, stream):
        assert self.h.hipStreamSynchronize(stream) == 0

    def get(self, p, shape, dtype=np.uint8):
        """blocking copy to the host: the caller has synchronised the stream that wrote p"""
        out = np.zeros(shape, dtype=dtype)
        assert self.h.hipMemcpy(out.ctypes.data, p, out.nbytes, 2) == 0
        return out

    def release(self):
        assert self.h.hipDeviceSynchronize() == 0
        for p in self.bufs:
            self.h.hipFree(p)
        for s in self.streams:
            self.h.hipStreamDestroy(s)
        self.bufs, self.streams, self.keep = [], [], []


@pytest.fixture
def hip():
    h = _Streams()
    yield h
    h.release()


def _compiled(mktemp):
    """(the circuits made so far, get): get(name) -> (flat circuit, runtime circuit), compiled once; the witness list is every signal"""
    from circom_amd import runtime as rt
    made = {}

    def get(name):
        if name not in made:
            d = str(mktemp(name))
            if name in BITS:
                cp = compile_program(PROGRAMS[name](), d, name, sym=False, strands=(1,), bits=True, jit=True)
                assert cp.bittape is not None and cp.jit is not None
            elif name == "flaky9m":
                old = os.environ.get("CW_MONT")
                os.environ["CW_MONT"] = "1"
                try:
                    cp = compile_program(PROGRAMS[name](), d, name)
                finally:
                    os.environ.pop("CW_MONT") if old is None else os.environ.__setitem__("CW_MONT", old)
            else:
                cp = compile_program(PROGRAMS[name](), d, name, sym=False)
            c = rt.Circuit(cp.tape_path, cp.dat_path, cp.r1cs_path)
            if c.n_witness != cp.flat.n_signals:
                c.set_witness_list(np.arange(c.n_signals, dtype=np.uint32))
            assert c.n_witness == cp.flat.n_signals
            made[name] = (cp.flat, c)
        return made[name]

    return made, get


@pytest.fixture(scope="module")
def circuits(tmp_path_factory):
    made, get = _compiled(tmp_path_factory.mktemp)
    yield get
    for _, c in made.values():
        c.close()


class Egress:
    """the device egress forms of one case: name -> (bytes, call(batch, device pointer)), and how to read an image back"""

    def __init__(self, case, c, B, with_select=True, with_wide=True):
        from circom_amd import runtime as rt
        circ = CASES[case][0]
        nw, npub, eb, nc = c.n_witness, c.n_public, c.element_bytes, c.n_constraints
        self.B = B
        self.forms = {}
        if circ != "sha64" and with_wide:                         # (the 204 K-wire image of the SHA circuit stays on the device)
            self.forms["wit"] = ((CNT, nw, 32), np.uint8, lambda b, p: b.witnesses_device(F0, CNT, p))
        if eb == 8:
            self.forms["wit8"] = ((CNT, nw), np.dtype("<u8"), lambda b, p: b.witnesses_device_n8(F0, CNT, p))
        self.forms["pub"] = ((B, npub, 32), np.uint8, lambda b, p: b.public_signals_device(p))
        row0 = min(1, nc - 1)
        rows = min(50, nc - row0)
        self.forms["prod"] = ((CNT, 3, rows, eb), np.uint8,
                              lambda b, p: b.r1cs_products_device(rt.R1CS_A | rt.R1CS_B | rt.R1CS_C, row0, rows, F0, CNT, p))
        if circ in BITS:
            stride = 8 * ((npub + 63) // 64)                      # rows of whole words, then the not-boolean word
            self.forms["rows"] = ((B * stride + 8,), np.uint8,
                                  lambda b, p: b.witness_rows_device(1, npub, 0, B, p, stride, d_not_boolean=p + B * stride))
            self.stride = stride
        if with_select:                                           # the failed instances: [B] indices, then the count
            self.forms["sel"] = ((B + 2,), np.uint32, lambda b, p: b.select_device(R1CS, R1CS, p, p + 4 * B))

    def nbytes(self, name):
        shape, dtype, _ = self.forms[name]
        return int(np.prod(shape)) * np.dtype(dtype).itemsize

    def read(self, hip, name, p):
        shape, dtype, _ = self.forms[name]
        a = hip.get(p, shape, dtype)
        if name == "sel":                                         # the entries behind the count keep whatever they held
            n = int(a[self.B])
            assert n <= self.B
            return a[:n].copy()
        if name == "rows":
            a[self.B * self.stride + 4:] = 0                      # (the word is 4 bytes of the 8)
        return a


class Fleet:
    """N batches of one circuit, each with its own stream, input buffer, egress buffers and the buffers the results are copied to"""

    def __init__(self, hip, monkeypatch, circuits, case, n=N, **egress):
        circ, env, B = CASES[case]
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        self.hip, self.case, self.circ, self.B = hip, case, circ, B
        self.fc, self.c = circuits(circ)
        self.eg = Egress(case, self.c, B, **egress)
        self.in_bytes = B * self.c.n_inputs * 32
        self.streams = [hip.stream() for _ in range(n)]
        self.batches = [self.c.batch(B, stream=s) for s in self.streams]
        self.d_in = [hip.buf(self.in_bytes) for _ in range(n)]
        self.out = [{k: hip.buf(self.eg.nbytes(k)) for k in self.eg.forms} for _ in range(n)]
        self.copy = [{k: hip.buf(self.eg.nbytes(k)) for k in self.eg.forms} for _ in range(n)]
        for b, p in zip(self.batches, self.d_in):
            b.set_inputs_device(p)
        self.check_engine(self.batches[0])

    def check_engine(self, b):
        case, c = self.case, self.c
        if case.startswith("bits"):
            assert b.bitmode and b.jit == ("emitted" in case)
        elif case.startswith("gl"):
            assert c.element_bytes == 8 and not b.bitmode
        else:
            assert c.element_bytes == 32 and not b.bitmode and b.emitted == (not case.startswith("interp")), (b.emitted, case)
            assert b.fused_check or not case.startswith("fused"), "no fused-check program for this circuit"

    def serial(self):
        """the batch that gives the expected values: the null stream, alone, a sync() after every call"""
        b = self.c.batch(self.B)
        self.check_engine(b)
        d_in = self.hip.buf(self.in_bytes)
        b.set_inputs_device(d_in)
        out = {k: self.hip.buf(self.eg.nbytes(k)) for k in self.eg.forms}
        return b, d_in, out

    def rows(self, j, r, nonbool=False):
        return inputs(self.circ, self.B, j, r, nonbool)

    def enqueue(self, j, r, step, nonbool=False, d_in=None, copy=None):
        """one round of batch j, all of it on the batch's stream and none of it waited for"""
        hip, b, s = self.hip, self.batches[j], self.streams[j]
        hip.h2d(d_in or self.d_in[j], image(self.rows(j, r, nonbool)), s)
        step(b)
        self.egress(j, copy)

    def egress(self, j, copy=None):
        hip, b, s = self.hip, self.batches[j], self.streams[j]
        copy = copy or self.copy[j]
        for k, (_, _, call) in self.eg.forms.items():
            call(b, self.out[j][k])
            hip.d2d(copy[k], self.out[j][k], self.eg.nbytes(k), s)

    def collect(self, j, copy=None, host=True):
        """the copies of batch j (its stream is synchronised here), with what the host getters say"""
        self.hip.wait(self.streams[j])
        copy = copy or self.copy[j]
        res = {k: self.eg.read(self.hip, k, copy[k]) for k in self.eg.forms}
        if host:
            b = self.batches[j]
            res["status"], res["first_bad"] = b.status(), b.r1cs_first_bad()
        return res

    def expected(self, ser, j, r, nonbool=False, step=None):
        b, d_in, out = ser
        assert self.hip.h.hipMemcpy(d_in, np.ascontiguousarray(image(self.rows(j, r, nonbool))).ctypes.data, self.in_bytes, 1) == 0
        if step is None:
            b.run(); b.sync()
            b.check_r1cs(); b.sync()
        else:
            step(b); b.sync()
        res = {}
        for k, (_, _, call) in self.eg.forms.items():
            call(b, out[k]); b.sync()
            res[k] = self.eg.read(self.hip, k, out[k])
        res["status"], res["first_bad"] = b.status(), b.r1cs_first_bad()
        return res

    def same(self, got, want, where):
        for k in want:
            if k in got:
                assert got[k].shape == want[k].shape and (got[k] == want[k]).all(), (self.case, k) + tuple(where)

    def oracle(self, res, j, r, nonbool=False, batch=None):
        """the sampled instances (and every digest of the SHA circuit) against eval_flat / check_r1cs / hashlib"""
        fc, c, B = self.fc, self.c, self.B
        rows = self.rows(j, r, nonbool)
        npub = c.n_public
        if self.circ == "sha64":
            good = np.array([i % B for i in NONBOOL] if nonbool else [], dtype=np.int64)
            keep = np.setdiff1d(np.arange(B), good)
            d = digests(np.where(rows > 1, 0, rows))
            stride = self.eg.stride
            got = res["rows"][:B * stride].reshape(B, stride)
            assert (got[keep, :32] == d[keep]).all(), (self.case, "digest", j, r)
            assert (np.packbits(res["pub"][:, :256, 0], axis=1)[keep] == d[keep]).all() and not res["pub"][keep][:, :, 1:].any()
            assert (res["status"][keep] == 0).all()
            for i in good:                                        # served by the side batch on the 256-bit schedule
                sig, failed, bad = evaluate(fc, rows[i])
                assert failed is None
                want = np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in sig[1:1 + npub]), dtype=np.uint8).reshape(npub, 32)
                assert (res["pub"][i] == want).all(), (self.case, "side batch", j, r, int(i))
                assert bool(res["status"][i] & R1CS) == (bad is not None) and (bad is None or res["first_bad"][i] == bad)
            return
        for i in samples(B, j, r):
            sig, failed, bad = evaluate(fc, rows[i])
            assert failed is None
            where = (self.case, j, r, i)
            assert bool(res["status"][i] & R1CS) == (bad is not None), where
            if bad is not None:
                assert res["first_bad"][i] == bad, where
            if "sel" in res:
                assert (i in res["sel"]) == (bad is not None), where
            want = np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in sig), dtype=np.uint8).reshape(-1, 32)
            assert (res["pub"][i] == want[1:1 + npub]).all(), where
            if F0 <= i < F0 + CNT:
                if "wit" in res:
                    assert (res["wit"][i - F0] == want).all(), where
                if "wit8" in res:
                    assert res["wit8"][i - F0].tolist() == list(sig), where
            elif batch is not None:
                assert batch.witness(i) == list(sig), where

    def close(self):
        for b in self.batches:
            b.close()


def _plain(b):
    b.run()
    b.check_r1cs()


def _graph(b):
    b.run_check()


def _interleaved(hip, monkeypatch, circuits, case, step, n_rounds, nonbool_round=None):
    fl = Fleet(hip, monkeypatch, circuits, case)
    ser = fl.serial()
    for r in range(n_rounds):
        nb = r == nonbool_round
        for j in range(N):
            fl.enqueue(j, r, step, nonbool=nb)
            if step is _graph:                                    # the first call is plain, the second captures, then replays
                assert fl.batches[j].graph_captured == (r >= 1), (case, j, r)
        got = [fl.collect(j) for j in range(N)]
        for j in range(N):
            fl.same(got[j], fl.expected(ser, j, r, nb), (j, r))
            fl.oracle(got[j], j, r, nb, batch=fl.batches[j])
    ser[0].close()
    fl.close()


@pytest.mark.gpu
@pytest.mark.xdist_group(GROUP)
@pytest.mark.parametrize("case", ENGINES)
def test_gpu_plain_steps_interleaved(hip, monkeypatch, circuits, case):
    """(a) run(), check_r1cs() and every device egress form of four batches interleaved, four rounds"""
    _interleaved(hip, monkeypatch, circuits, case, _plain, 4)


@pytest.mark.gpu
@pytest.mark.xdist_group(GROUP)
@pytest.mark.parametrize("case", ENGINES)
def test_gpu_graph_steps_interleaved(hip, monkeypatch, circuits, case):
    """(b) the same with run_check(): plain, capture, three replays, the inputs rewritten in place before each (same pointer, new
    bytes).  Bit engines: round 3 carries two instances with an input that is no bit - the side batch is then created on the
    caller's stream, after the replay - and those instances match eval_flat"""
    _interleaved(hip, monkeypatch, circuits, case, _graph, 5, nonbool_round=3 if case.startswith("bits") else None)


@pytest.mark.gpu
@pytest.mark.xdist_group(GROUP)
@pytest.mark.parametrize("case", ["wide-mixed", "gl-badsquare", "bits-interp-badbit", "bits-emitted-badbit"])
def test_gpu_select_chained_into_egress_with_no_host_read(hip, monkeypatch, circuits, case):
    """(c) select_device -> witnesses_at_device (d_n_idx = the select's count) on each batch's stream, another (mask, want) per batch:
    the lists are np.flatnonzero of the serial batch's status words (checked against the oracle), the rows its witnesses"""
    fl = Fleet(hip, monkeypatch, circuits, case, with_select=False, with_wide=False)
    ser = fl.serial()
    B, nw = fl.B, fl.c.n_witness
    words = [(R1CS, R1CS), (NONE, 0), (R1CS, 0), (R1CS | 1, R1CS)]
    d_idx = [hip.buf(4 * B + 8) for _ in range(N)]
    d_rows = [hip.buf(B * nw * 32) for _ in range(N)]
    c_idx = [hip.buf(4 * B + 8) for _ in range(N)]
    c_rows = [hip.buf(B * nw * 32) for _ in range(N)]
    for r in range(3):
        for j in range(N):
            b, s = fl.batches[j], fl.streams[j]
            hip.fill(d_idx[j], 0xA5, 4 * B + 8, s)
            hip.fill(d_rows[j], 0xA5, B * nw * 32, s)
            fl.enqueue(j, r, _plain)
            b.select_device(words[j][0], words[j][1], d_idx[j], d_idx[j] + 4 * B)
            b.witnesses_at_device(d_idx[j], B, d_rows[j], d_n_idx=d_idx[j] + 4 * B)
            hip.d2d(c_idx[j], d_idx[j], 4 * B + 8, s)
            hip.d2d(c_rows[j], d_rows[j], B * nw * 32, s)
        for j in range(N):
            got = fl.collect(j, host=False)
            idx, rows = hip.get(c_idx[j], (B + 2,), np.uint32), hip.get(c_rows[j], (B, nw, 32))
            want = fl.expected(ser, j, r)
            fl.same(got, want, (j, r))
            fl.oracle(dict(got, status=want["status"], first_bad=want["first_bad"]), j, r)
            sel = np.flatnonzero((want["status"] & words[j][0]) == words[j][1])
            assert 0 < len(sel) < B, (case, j, r)
            assert idx[B] == len(sel) and (idx[:len(sel)] == sel).all() and (idx[len(sel):B] == 0xA5A5A5A5).all(), (case, j, r)
            full = ser[0].witnesses()
            assert (rows[:len(sel)] == full[sel]).all() and (rows[len(sel):] == 0xA5).all(), (case, j, r)
    ser[0].close()
    fl.close()


@pytest.mark.gpu
@pytest.mark.xdist_group(GROUP)
@pytest.mark.parametrize("case", ["emitted-poseidon", "fused-flaky", "bits-emitted-sha", "gl-badsquare"])
def test_gpu_double_buffered_inputs(hip, monkeypatch, circuits, case):
    """(d) three run_check() on buffer A (plain, capture, replay), then set_inputs_device(B) and run_check() at once: the captured
    step is dropped while its replay may still be in flight - cw_run_check drains the batch's stream before it destroys the graph -,
    the capture and the replay on B are right, and A's results, copied out before the switch, are A's.  Bit engine: the same
    after device_bits() drops the graph.  All four batches are in flight throughout"""
    fl = Fleet(hip, monkeypatch, circuits, case)
    ser = fl.serial()
    bits = case.startswith("bits")
    steps = 9 if bits else 6
    d_b = [hip.buf(fl.in_bytes) for _ in range(N)]
    copies = [[{k: hip.buf(fl.eg.nbytes(k)) for k in fl.eg.forms} for _ in range(steps)] for _ in range(N)]
    captured = [False, True, True, False, True, True, False, True, True]
    for r in range(steps):
        for j in range(N):
            b = fl.batches[j]
            if r == 3:
                b.set_inputs_device(d_b[j])
            if r == 6:
                assert b.device_bits()[0] and not b.graph_captured
            fl.enqueue(j, r % 6, _graph, d_in=d_b[j] if r >= 3 else None, copy=copies[j][r])
            assert b.graph_captured == captured[r], (case, j, r)
    want = {}
    for j in range(N):
        for r in range(steps):
            got = fl.collect(j, copy=copies[j][r], host=(r == steps - 1))
            if (j, r % 6) not in want:
                want[j, r % 6] = fl.expected(ser, j, r % 6)
            fl.same(got, want[j, r % 6], (j, r))
            if r == steps - 1:
                fl.oracle(got, j, r % 6)
    ser[0].close()
    fl.close()


@pytest.mark.gpu
@pytest.mark.xdist_group(GROUP)
def test_gpu_supplied_witnesses_may_be_overwritten_behind_the_call(hip, circuits):
    """(e) 64-bit engine: set_witnesses_device_n8 from the batch's own buffer, check_r1cs, then garbage over that buffer on the same
    stream - "may be reused once the batch's stream has passed the call".  test_goldilocks_supplied's Poseidon(2) witnesses with
    another tamper set per batch and round; flagged instances and first-bad rows are the oracle's"""
    from test_goldilocks_supplied import Q, _tampered
    fc, sig, img0, want0 = _tampered()
    _, c = circuits("pos2gl")
    B, nw = sig.shape
    assert nw == c.n_witness
    streams = [hip.stream() for _ in range(N)]
    d_w = [hip.buf(B * nw * 8) for _ in range(N)]
    d_sel = [hip.buf(4 * B + 8) for _ in range(N)]
    c_sel = [hip.buf(4 * B + 8) for _ in range(N)]
    garbage = np.full(B * nw * 8, 0xEE, dtype=np.uint8)
    for r in range(2):
        # (new batches every round: an R1CS bit of an earlier check stays set until the next cw_run or the next FIRST supply)
        batches = [c.batch(B, stream=s) for s in streams]
        wants = []
        for j in range(N):
            if (j, r) == (0, 0):
                img, want = img0, want0
            else:
                img = sig.copy()
                tampered = [i for i in range(B) if (i + 3 * j + r) % 4 != 1]
                for i in tampered:
                    k = 1 + (7 * i + 31 * j + 5 * r) % (nw - 1)
                    img[i, k] = (int(img[i, k]) + 1 + j) % Q
                want = [check_r1cs(Q, fc.constraints, [int(v) for v in img[i]]) if i in set(tampered) else None for i in range(B)]
                assert all(want[i] is not None for i in tampered)
            wants.append(want)
            b, s = batches[j], streams[j]
            hip.h2d(d_w[j], img, s)
            b.set_witnesses_device_n8(0, B, d_w[j])
            b.check_r1cs()
            hip.h2d(d_w[j], garbage, s)                           # the stream has passed the call: the buffer is the caller's again
            b.select_device(R1CS, R1CS, d_sel[j], d_sel[j] + 4 * B)
            hip.d2d(c_sel[j], d_sel[j], 4 * B + 8, s)
        for j in range(N):
            hip.wait(streams[j])
            bad = np.array([w is not None for w in wants[j]])
            idx = hip.get(c_sel[j], (B + 2,), np.uint32)
            assert idx[B] == bad.sum() and (idx[:idx[B]] == np.flatnonzero(bad)).all(), (j, r)
            st, fb = batches[j].status(), batches[j].r1cs_first_bad()
            assert ((st & R1CS != 0) == bad).all() and not (st & ~np.uint32(R1CS)).any(), (j, r)
            assert fb[bad].tolist() == [w for w in wants[j] if w is not None], (j, r)
            assert (hip.get(d_w[j], (B * nw * 8,)) == 0xEE).all()
        for b in batches:
            b.close()


@pytest.mark.gpu
@pytest.mark.xdist_group(GROUP)
@pytest.mark.parametrize("case", ["emitted-poseidon", "bits-emitted-sha", "gl-badsquare"])
def test_gpu_a_batch_closed_while_the_others_fly(hip, monkeypatch, circuits, case):
    """(f) batch 1 is closed right after its round has been enqueued (run_check: its replay is in flight): the other three are
    right, and a new batch on the stream it left computes correctly next to them"""
    fl = Fleet(hip, monkeypatch, circuits, case)
    ser = fl.serial()
    for r in range(4):
        for j in range(N):
            if r == 3 and j == 1:
                fl.batches[1] = fl.c.batch(fl.B, stream=fl.streams[1])
                fl.batches[1].set_inputs_device(fl.d_in[1])
            fl.enqueue(j, r, _graph)
            if r == 2 and j == 1:
                fl.batches[1].close()
        for j in range(N):
            if r == 2 and j == 1:
                continue
            got = fl.collect(j)
            fl.same(got, fl.expected(ser, j, r), (j, r))
            fl.oracle(got, j, r)
    ser[0].close()
    fl.close()


@pytest.mark.gpu
@pytest.mark.xdist_group(GROUP)
@pytest.mark.parametrize("case", ["interp-flaky", "emitted-poseidon", "bits-emitted-sha", "gl-badsquare"])
def test_gpu_host_getters_drain_their_own_stream(hip, monkeypatch, circuits, case):
    """(g) batches 1 to 3 have a round enqueued and unsynchronised; batch 0, enqueued and not synchronised either, answers every
    host getter correctly; afterwards batches 1 to 3 are right too"""
    fl = Fleet(hip, monkeypatch, circuits, case)
    ser = fl.serial()
    sha = fl.circ == "sha64"
    B = fl.B
    for r in range(2):
        for j in (1, 2, 3, 0):
            fl.enqueue(j, r, _plain)
        b, p = fl.batches[0], ser[0]
        calls = [lambda x: x.status(), lambda x: x.r1cs_first_bad(), lambda x: x.select(R1CS, R1CS), lambda x: x.select(),
                 lambda x: x.public_signals(), lambda x: x.r1cs_products(7, 0, min(40, fl.c.n_constraints), F0, CNT),
                 lambda x: np.frombuffer(x.explain(B - 1).encode(), dtype=np.uint8), lambda x: np.frombuffer(x.explain(64).encode(), dtype=np.uint8)]
        if not sha:
            calls += [lambda x: x.witnesses(F0, CNT), lambda x: x.witnesses_at(np.array([B - 1, 0, 64, 63, 0], dtype=np.uint32))]
        else:
            calls += [lambda x: x.witnesses_at(np.array([B - 1, 0, 64], dtype=np.uint32), 1, fl.c.n_public), lambda x: x.witness_rows(1, 256)[0]]
        answers = [call(b) for call in calls]                     # nothing has waited for batch 0 so far
        want = fl.expected(ser, 0, r)
        for k, (a, call) in enumerate(zip(answers, calls)):
            e = call(p)
            assert a.shape == e.shape and (a == e).all(), (case, r, k)
        got = dict(fl.collect(0))
        fl.same(got, want, (0, r))
        fl.oracle(got, 0, r, batch=b)
        for j in (1, 2, 3):
            got = fl.collect(j)
            fl.same(got, fl.expected(ser, j, r), (j, r))
            fl.oracle(got, j, r)
    ser[0].close()
    fl.close()
