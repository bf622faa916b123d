"""The input rows of the emitted code's bit table (sh = 5, T[chunk][slot][32 groups]) are written in WHOLE ROWS
(cw_bits.hip cw_bits_masks_to_table_rows_kernel): packed masks and packed rows go through that kernel directly, a 32-byte image
through cw_bits_ingest_kernel into the batch's staging masks and from there through the same kernel (cw_host.cpp bits_run;
CW_BITS_INGEST_STAGED=0 keeps the direct store).  Shapes: BitGadget(40) has 120 inputs = one full tile column of 64 and a ragged
one of 56; 2 117 instances = one full chunk of 32 groups, then a chunk of two groups whose last holds 5 instances; 70 instances =
a chunk that is mostly padding; BitGadget(128) has 384 inputs = six full tile columns, at 2 048 + 64 instances a second chunk
starts.  Every instance is compared with the oracle (oracle.tape_eval), computed once per circuit and shared."""
import numpy as np
import pytest

from circom_amd.frontend.dsl import Program
from oracle.tape_eval import check_r1cs
from test_bitplane import BitGadget, _Hip, _flat, _gpu, _rand_bits

pytestmark = pytest.mark.gpu

B_BIG, B_SMALL = 2117, 70


@pytest.fixture(autouse=True)
def _emitted_engine(monkeypatch):
    monkeypatch.setenv("CW_BITS_JIT", "1")                    # the emitted engine below its batch threshold
    monkeypatch.delenv("CW_BITS_INGEST_STAGED", raising=False)


class _Ref:
    """a circuit, P boolean input rows and what the oracle makes of them.  Instance i of a batch takes row (i + shift) % P: P is odd,
    so the 64 rows of every group of 64 instances start somewhere else and no two groups of a batch hold the same masks, while the
    oracle (milliseconds per instance) runs P times per circuit instead of once per instance of every test."""

    def __init__(self, tmp, n, name, P, seed):
        self.cp, self.c = _gpu(tmp, Program(BitGadget(n)), name)
        self.fc = self.cp.flat
        self.P = P
        self.pat = _rand_bits(self.fc, P, seed)
        self.pat_want = np.stack([self.expect(r)[0] for r in self.pat])

    def expect(self, row):
        """(witness bytes [n_signals][32], or None when the witness code fails; the oracle's signals)"""
        sig, failed = _flat(self.fc, row)
        if failed is not None:
            return None, sig
        return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in sig), dtype=np.uint8).reshape(len(sig), 32), sig

    def rows(self, B, shift=0):
        return [list(self.pat[(i + shift) % self.P]) for i in range(B)]

    def want(self, B, shift=0):
        return self.pat_want[(np.arange(B) + shift) % self.P]


@pytest.fixture(scope="module")
def bg40(tmp_path_factory):
    r = _Ref(tmp_path_factory.mktemp("bg40"), 40, "bg40", 131, 40)
    assert r.c.n_inputs == 120
    yield r
    r.c.close()


@pytest.fixture(scope="module")
def bg128(tmp_path_factory):
    r = _Ref(tmp_path_factory.mktemp("bg128"), 128, "bg128r", 67, 128)
    assert r.c.n_inputs == 384
    yield r
    r.c.close()


def _image(rows):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for r in rows for v in r), dtype=np.uint8).reshape(len(rows), len(rows[0]), 32).copy()


def _packed_masks(rows):
    """uint64 [groups][n_inputs], bit i of masks[g][k] = input k of instance 64 g + i"""
    bits = np.asarray(rows, dtype=np.uint64)
    B, n = bits.shape
    G = (B + 63) // 64
    pad = np.zeros((G * 64, n), dtype=np.uint64)
    pad[:B] = bits
    return np.bitwise_or.reduce(pad.reshape(G, 64, n) << np.arange(64, dtype=np.uint64)[None, :, None], axis=1)


def _check_clean(ref, b, B, shift=0):
    """statuses and full witnesses of every instance against the oracle, public signals against the witness"""
    assert b.bitmode and b.jit
    b.run(); b.check_r1cs(); b.sync()
    assert (b.status() == 0).all()
    bulk = b.witnesses()
    assert bulk.shape == (B, ref.fc.n_signals, 32)
    bad = np.nonzero((bulk != ref.want(B, shift)).any(axis=(1, 2)))[0]
    assert bad.size == 0, bad[:8].tolist()
    assert (b.public_signals() == bulk[:, 1:1 + ref.c.n_public]).all()


@pytest.mark.parametrize("B", [B_BIG, B_SMALL])
@pytest.mark.parametrize("how", ["set_inputs", "set_inputs_device", "set_inputs_bits", "set_inputs_rows"])
def test_every_input_form_fills_the_input_rows(bg40, how, B):
    rows = bg40.rows(B)
    b = bg40.c.batch(B)
    hip = d_in = None
    if how == "set_inputs":
        b.set_inputs(rows)
    elif how == "set_inputs_device":
        hip = _Hip()
        d_in = hip.upload(_image(rows))
        b.set_inputs_device(d_in)
    elif how == "set_inputs_bits":
        b.set_inputs_bits(_packed_masks(rows))
    else:
        b.set_inputs_rows(np.packbits(np.asarray(rows, dtype=np.uint8), axis=1))      # most significant bit first
    _check_clean(bg40, b, B)
    b.close()
    if d_in is not None:
        hip.h.hipFree(d_in)


def _odd_rows(ref, shift=0):
    """B_BIG rows with three inputs that are not bits: their instances are flagged by the ingest and re-run wide"""
    q = ref.c.q
    rows = ref.rows(B_BIG, shift)
    odd = {700: (5, 2),                       # the value 2 in a full group of the full chunk
           2116: (119, q - 1),                # q - 1 at the last input of the 5-instance group
           2050: (7, 1 << 248)}               # only byte 31 set, in the first group of the second chunk
    for i, (k, v) in odd.items():
        rows[i][k] = v
    return rows, odd


def _check_odd(ref, b, rows, odd, shift=0):
    """after run + check_r1cs + sync: the odd instances one by one against the oracle, all others as _check_clean"""
    from circom_amd import runtime as rt
    st = b.status()
    bulk = b.witnesses()
    clean = np.ones(len(rows), dtype=bool)
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
    bad = np.nonzero((bulk[clean] != ref.want(len(rows), shift)[clean]).any(axis=(1, 2)))[0]
    assert bad.size == 0, bad[:8].tolist()
    assert (b.public_signals() == bulk[:, 1:1 + ref.c.n_public]).all()


def test_non_boolean_inputs_are_flagged_and_rerun_wide(bg40):
    rows, odd = _odd_rows(bg40)
    b = bg40.c.batch(B_BIG)
    b.set_inputs(rows)
    b.run(); b.check_r1cs(); b.sync()
    _check_odd(bg40, b, rows, odd)
    b.close()


def test_second_run_of_a_batch_follows_the_second_inputs(bg40):
    """nothing stale from the staging masks, the flag words or the padding columns: the first run is clean, the second has other
    bits everywhere and flagged instances where the first had none, the third is the first again"""
    b = bg40.c.batch(B_BIG)
    b.set_inputs(bg40.rows(B_BIG))
    _check_clean(bg40, b, B_BIG)
    rows2, odd = _odd_rows(bg40, shift=17)
    b.set_inputs(rows2)
    b.run(); b.check_r1cs(); b.sync()
    _check_odd(bg40, b, rows2, odd, shift=17)
    b.set_inputs(bg40.rows(B_BIG))
    _check_clean(bg40, b, B_BIG)
    b.close()


def test_direct_route_and_staged_route_give_the_same_bytes(bg40, monkeypatch):
    got = {}
    rows, odd = _odd_rows(bg40)
    for staged in ("0", "1"):
        monkeypatch.setenv("CW_BITS_INGEST_STAGED", staged)
        b = bg40.c.batch(B_BIG)
        b.set_inputs(rows)
        b.run(); b.check_r1cs(); b.sync()
        got[staged] = (b.status().tobytes(), b.witnesses().tobytes(), b.public_signals().tobytes())
        if staged == "1":
            _check_odd(bg40, b, rows, odd)                       # and the oracle's, not only each other's
        b.close()
    assert got["0"] == got["1"]


def test_run_check_plain_capture_and_replay_on_the_staged_route(bg40):
    hip = _Hip()
    d_in = hip.upload(_image(bg40.rows(B_BIG)))
    b = bg40.c.batch(B_BIG)
    b.set_inputs_device(d_in)
    seen = []
    for r in range(3):                                           # plain, capture, replay
        b.run_check(); b.sync()
        assert b.graph_captured == (r >= 1), r
        seen.append((b.status().copy(), b.witnesses()))
    assert (seen[0][0] == 0).all() and (seen[0][1] == bg40.want(B_BIG)).all()
    assert (seen[2][0] == seen[0][0]).all() and (seen[2][1] == seen[0][1]).all()
    b.close()
    hip.h.hipFree(d_in)


def test_a_second_chunk_starts_at_2048_instances(bg128):
    B = 2048 + 64
    b = bg128.c.batch(B)
    b.set_inputs(bg128.rows(B))
    _check_clean(bg128, b, B)
    b.close()
