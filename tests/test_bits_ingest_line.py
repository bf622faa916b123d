"""The 32-byte ingest of the bit-plane path reads every 128-byte line with one streaming LDS-DMA load (cw_bits.hip
cw_bits_ingest_kernel: lane = one 16-byte piece, even lanes the low halves, odd lanes the high halves, one lane exchange after
the loop; the index arithmetic is cw_bits_layout.h's, replayed on the CPU by tests/host/bits_ingest_line_test.cpp).
CW_BITS_INGEST_LINE=0 keeps the previous body (two 16-byte loads per lane and input) for comparison.

Shapes: BitGadget(8) has 24 inputs (one load of a wave, ragged), BitGadget(13) 39 (the second load of a wave starts at input 32,
ragged), BitGadget(100) 300 (a second workgroup per group whose first wave is ragged and whose other waves leave at once).  Batches
1, 63 (one ragged group: the plain walk), 64 (one full group: the ring), 65, 300 (full groups and a ragged last one) and
2 048 + 64 (a second chunk of the emitted code's table).  Both engines; the emitted engine on both routes (CW_BITS_INGEST_STAGED =
0 / 1; the interpreter has one route, the switch does not reach it).

Instance i takes pattern row (i + shift) % P with P odd, so no two groups hold the same masks (a wrong rotation or a wrong half
shows); the oracle (oracle.tape_eval) runs once per pattern row and once per instance that is not boolean.  Every case carries
instances that are not boolean: the value 2 in dword 0, and 2 in each of dwords 0 .. 7 alone (seven of them non-zero only above
dword 0, four only in the high half), at the first input, the last input and input 37 (an odd lane pair of a wave's second load)
where the circuit has it.  Exactly those instances are re-run wide (the `wide` list of cw_write_wtnsb, which is what the flag words
select), and their witnesses are the oracle's.  The two bodies are compared byte for byte on the input rows of the table (all real
groups), the re-run list, statuses and witnesses."""
import numpy as np
import pytest

from circom_amd import wtnsb
from circom_amd.frontend.dsl import Program
from oracle.tape_eval import check_r1cs
from test_bitplane import BitGadget, _Hip, _flat, _gpu, _rand_bits

pytestmark = pytest.mark.gpu

BATCHES = [1, 63, 64, 65, 300, 2048 + 64]
ROUTES = [("interp", None), ("jit", "0"), ("jit", "1")]


class _Ref:
    def __init__(self, tmp, n, name, P, seed):
        self.cp, self.c = _gpu(tmp, Program(BitGadget(n)), name)
        self.fc = self.cp.flat
        self.P = P
        self.pat = _rand_bits(self.fc, P, seed)
        self.pat_img = np.stack([self.image_row(r) for r in self.pat])                 # [P][n_in][32]
        self.pat_want = np.stack([self.expect(r)[0] for r in self.pat])

    @staticmethod
    def image_row(row):
        return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in row), dtype=np.uint8).reshape(len(row), 32)

    def expect(self, row):
        """(witness bytes [n_signals][32], or None when the witness code fails; the oracle's signals)"""
        sig, failed = _flat(self.fc, row)
        if failed is not None:
            return None, sig
        return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in sig), dtype=np.uint8).reshape(len(sig), 32), sig


@pytest.fixture(scope="module", params=[(8, 24, 131), (13, 39, 67), (100, 300, 71)], ids=["24in", "39in", "300in"])
def ref(request, tmp_path_factory):
    n, n_in, P = request.param
    r = _Ref(tmp_path_factory.mktemp("bgl%d" % n), n, "bgl%d" % n, P, 500 + n)
    assert r.c.n_inputs == n_in
    yield r
    r.c.close()


def _odd(ref, B):
    """{instance: (input, value)}: the instances of a batch of B that are not boolean"""
    n_in = ref.c.n_inputs
    inputs = [0, n_in - 1] + ([37] if n_in > 37 else [])
    if B < 9:
        return {B - 1: (0, 2)}
    inst = [int(x) for x in np.linspace(0, B - 1, 9)]
    assert len(set(inst)) == 9
    odd = {inst[0]: (inputs[-1], 2)}
    for d in range(8):
        odd[inst[1 + d]] = (inputs[d % len(inputs)], 2 << (32 * d))
    return odd


def _image(ref, B, shift, odd):
    img = ref.pat_img[(np.arange(B) + shift) % ref.P].copy()
    rows = {}
    for i, (k, v) in odd.items():
        rows[i] = list(ref.pat[(i + shift) % ref.P])
        rows[i][k] = v
        img[i, k] = np.frombuffer(int(v).to_bytes(32, "little"), dtype=np.uint8)
    return img, rows


def _input_rows(ref, b, w):
    """the words of the main inputs' slots in every real group, from the container's copy of the bit table"""
    slots = b.signal_slots()[ref.fc.main_input_start:ref.fc.main_input_start + ref.c.n_inputs].astype(np.int64)
    assert (w.slots, w.shift) == (b.bits_slots, b.bits_sh)
    sh = w.shift
    table = np.asarray(w._table)
    out = []
    for g in range((b.n + 63) // 64):
        base = (((g >> sh) * w.slots) << sh) + (g & ((1 << sh) - 1))
        out.append(table[base + (slots << sh)])
    return np.stack(out)


def _run(ref, B, shift, odd, d_in, tmp_path, tag):
    b = ref.c.batch(B)
    b.set_inputs_device(d_in)
    b.run(); b.check_r1cs(); b.sync()
    p = tmp_path / ("%s.wtnsb" % tag)
    b.write_wtnsb(p)
    w = wtnsb.load(p)
    got = {"status": b.status().copy(), "wit": b.witnesses(), "wide": sorted(w.wide), "rows": _input_rows(ref, b, w), "jit": b.jit}
    assert b.bitmode
    b.close()
    return got


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("engine,staged", ROUTES, ids=["interp", "jit-direct", "jit-staged"])
def test_line_ingest_against_the_oracle_and_the_previous_body(ref, engine, staged, B, monkeypatch, tmp_path):
    from circom_amd import runtime as rt
    monkeypatch.setenv("CW_BITS_JIT", "1" if engine == "jit" else "0")
    if staged is None:
        monkeypatch.delenv("CW_BITS_INGEST_STAGED", raising=False)
    else:
        monkeypatch.setenv("CW_BITS_INGEST_STAGED", staged)
    shift = B % 29
    odd = _odd(ref, B)
    img, rows = _image(ref, B, shift, odd)
    hip = _Hip()
    d_in = hip.upload(img)
    got = {}
    for line in ("0", "1"):
        monkeypatch.setenv("CW_BITS_INGEST_LINE", line)
        got[line] = _run(ref, B, shift, odd, d_in, tmp_path, "line" + line)
    hip.h.hipFree(d_in)
    new, old = got["1"], got["0"]
    assert new["jit"] == (engine == "jit")
    # the new body against the oracle: exactly the odd instances were re-run wide
    assert new["wide"] == sorted(odd)
    st, bulk = new["status"], new["wit"]
    clean = np.ones(B, dtype=bool)
    for i in odd:
        clean[i] = False
        want, sig = ref.expect(rows[i])
        if want is None:
            assert st[i] & 1, i                                  # the reference would abort on this input
            continue
        assert not (st[i] & 1), i
        assert (bulk[i] == want).all(), i
        assert bool(st[i] & rt.ST_R1CS_FAILED) == (check_r1cs(ref.c.q, ref.fc.constraints, sig) is not None), i
    assert (st[clean] == 0).all()
    want_all = ref.pat_want[(np.arange(B) + shift) % ref.P]
    bad = np.nonzero((bulk[clean] != want_all[clean]).any(axis=(1, 2)))[0]
    assert bad.size == 0, bad[:8].tolist()
    # the input rows are the low bits of the image, group by group
    bits = (img[:, :, 0] & 1).astype(np.uint64)
    G = (B + 63) // 64
    pad = np.zeros((G * 64, bits.shape[1]), dtype=np.uint64)
    pad[:B] = bits
    masks = np.bitwise_or.reduce(pad.reshape(G, 64, -1) << np.arange(64, dtype=np.uint64)[None, :, None], axis=1)
    assert (new["rows"] == masks).all()
    # and the previous body's, byte for byte
    assert new["rows"].tobytes() == old["rows"].tobytes()
    assert new["wide"] == old["wide"]
    assert new["status"].tobytes() == old["status"].tobytes()
    assert new["wit"].tobytes() == old["wit"].tobytes()


def test_run_check_plain_capture_and_replay(ref, monkeypatch):
    monkeypatch.setenv("CW_BITS_JIT", "1")
    monkeypatch.delenv("CW_BITS_INGEST_STAGED", raising=False)
    monkeypatch.delenv("CW_BITS_INGEST_LINE", raising=False)
    B = 2048 + 64
    img, _ = _image(ref, B, 3, {})
    hip = _Hip()
    d_in = hip.upload(img)
    b = ref.c.batch(B)
    b.set_inputs_device(d_in)
    seen = []
    for r in range(3):                                           # plain, capture, replay
        b.run_check(); b.sync()
        assert b.graph_captured == (r >= 1), r
        seen.append((b.status().copy(), b.witnesses()))
    assert (seen[0][0] == 0).all() and (seen[0][1] == ref.pat_want[(np.arange(B) + 3) % ref.P]).all()
    assert (seen[2][0] == seen[0][0]).all() and (seen[2][1] == seen[0][1]).all()
    b.close()
    hip.h.hipFree(d_in)
