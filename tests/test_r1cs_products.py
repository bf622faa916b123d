"""R1CS products out: cw_get_r1cs_products / cw_get_r1cs_products_device (include/circom_amd.h) - out[j][p][k] = the p-th
selected part (A, B, C) of constraint row0 + k of the .r1cs file in instance first + j, cw_element_bytes each, canonical.  One
kernel per table layout: csrc/cw64.hip cw64_products_kernel (tiles of 64 instances x 64 rows), csrc/cw_kernels.hip
cw_products_kernel (canonical and Montgomery-form tables) and csrc/cw_bits.hip cw_bits_products_kernel (both bit-table layouts):
tiles of 64 instances x 16 rows.

Expected values never come from the library: the witness is oracle.tape_eval.eval_flat's (BitGadget's is the one
tests/test_input_rows.py computes once per session, Goldilocks Poseidon's the one of tests/test_goldilocks_egress.py), the
products are sum(co * w[k]) mod q on Python integers from fc.constraints - what oracle.tape_eval.check_r1cs sums.  Every device
image lies between guard bytes, and so does every host image; the guards are compared.

The shapes (counted on the CPU): Poseidon(2) has 1 105 constraints, 862 with an empty A or B, 195 terms on the constant wire
and 780 general coefficients; BitGadget(15) 335 rows of up to 77 terms, BitGadget(43) 951 of up to 217; Multiplier2 one row.  The
row ranges start and end inside tiles of 16 and of 64, the instance ranges are tests/test_output_rows.py's at 65 and 300."""
import ctypes as C
import functools
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
from test_bitplane import BitAssert, BitGadget, _Hip                                 # noqa: E402,F401
from test_input_rows import _case, pack_rows                                         # noqa: E402
from test_output_rows import inst_ranges                                             # noqa: E402

from circom_amd.circuits.basic import Multiplier2                                    # noqa: E402
from circom_amd.circuits.poseidon import Poseidon                                    # noqa: E402
from circom_amd.compiler import compile_program                                      # noqa: E402
from circom_amd.frontend.dsl import Program                                          # noqa: E402
from circom_amd.frontend.flatten import flatten                                      # noqa: E402
from oracle.tape_eval import eval_flat                                               # noqa: E402

CW_EINVAL, CW_EDEVICE, CW_ESTATE = -2, -4, -5
A, B_, C_ = 1, 2, 4                                                                  # CW_R1CS_A / _B / _C
R1CS_FAILED = 4
NONE = 0xFFFFFFFF
GUARD = 4096
ROW_RANGES = [(0, 1), (1, 15), (15, 2), (0, 17), (1, 63), (63, 2), (0, 65), (3, 130), (0, None)]   # (row0, n_rows); None = the whole system
MASKS = [1, 2, 4, 5, 7]
RBITS = 261                                                                          # the table's Montgomery radix 2^261


# ---- model -----------------------------------------------------------------------------------------------------------------------
def products(q, constraints, W):
    """[instances][3][constraints] Python integers: sum(co * w[k]) mod q per part, W = [instances][signals] integers"""
    W = np.asarray(W, dtype=object)
    out = np.zeros((W.shape[0], 3, len(constraints)), dtype=object)
    for k, abc in enumerate(constraints):
        for p, part in enumerate(abc):
            if part:
                acc = 0
                for s, co in part.items():
                    acc = acc + (co % q) * W[:, s]
                out[:, p, k] = acc % q
    return out


def as_bytes(vals, eb):
    """integers -> uint8 [...][eb], little-endian"""
    if eb == 8:
        return np.ascontiguousarray(vals.astype(np.uint64)).view(np.uint8).reshape(vals.shape + (8,))
    raw = b"".join(int(v).to_bytes(32, "little") for v in vals.reshape(-1))
    return np.frombuffer(raw, dtype=np.uint8).reshape(vals.shape + (32,))


def as_ints(image):
    """uint8 [...][eb] -> integers"""
    words = np.ascontiguousarray(image).view("<u8").astype(object)
    return sum(words[..., k] << (64 * k) for k in range(words.shape[-1]))


def signals_of(want):
    """[B][n_signals][32] uint8 (test_input_rows._case) -> [B][n_signals] integers"""
    return as_ints(want)


def select(img, parts, row0, n, first, count):
    sel = [p for p in range(3) if (parts >> p) & 1]
    return img[first:first + count][:, sel][:, :, row0:row0 + n]


@functools.lru_cache(maxsize=None)
def _bg_case(n, prime="bn128"):
    """(flat circuit, input bits [300][3 n], model image [300][3][rows][eb]) of BitGadget(n)"""
    fc = flatten(Program(BitGadget(n), prime=prime) if prime != "bn128" else Program(BitGadget(n)))
    bits, want = _case(n, prime)
    img = as_bytes(products(fc.fp.q, fc.constraints, signals_of(want)), 8 if prime == "goldilocks" else 32)
    img.setflags(write=False)
    return fc, bits, img


@functools.lru_cache(maxsize=None)
def _pos_case(prime, n_inst):
    """(flat circuit, input rows, model image) of Poseidon(2) x n_inst on a 256-bit prime"""
    fc = flatten(Program(Poseidon(2)) if prime == "bn128" else Program(Poseidon(2), prime=prime))
    q = fc.fp.q
    rnd = random.Random(1105)
    rows = [[rnd.randrange(q) for _ in range(fc.n_main_inputs)] for _ in range(n_inst)]
    rows[0], rows[1] = [0] * fc.n_main_inputs, [q - 1] * fc.n_main_inputs
    sigs = []
    for row in rows:
        sig, failed = eval_flat(q, fc.n_signals, fc.n_temps, fc.constants, fc.code, {fc.main_input_start + k: v for k, v in enumerate(row)})
        assert failed is None
        sigs.append(sig)
    img = as_bytes(products(q, fc.constraints, sigs), 32)
    img.setflags(write=False)
    return fc, rows, img


@functools.lru_cache(maxsize=None)
def _glpos_case():
    """the same on Goldilocks, with the oracle tests/test_goldilocks_egress.py shares: (flat circuit, rows, signals, model image)"""
    from test_goldilocks_egress import CASES, _poseidon_oracle
    fc = flatten(CASES["poseidon2"][0]())
    rows, sig = _poseidon_oracle()
    img = as_bytes(products(fc.fp.q, fc.constraints, [[int(v) for v in row] for row in sig]), 8)
    img.setflags(write=False)
    return fc, rows, sig, img


def test_the_circuits_have_the_shapes_the_ranges_are_chosen_for():
    fc = flatten(Program(Poseidon(2)))
    cons = fc.constraints
    assert len(cons) == 1105 and sum(1 for a, b, c in cons if not a or not b) == 862
    assert sum(1 for abc in cons for part in abc for s in part if s == 0) == 195
    assert max(len(part) for abc in cons for part in abc) == 4
    q = fc.fp.q
    assert sum(1 for abc in cons for part in abc for s, co in part.items() if co % q not in (1, q - 1)) == 780
    for n, rows, longest in ((15, 335, 77), (43, 951, 217)):
        cons = flatten(Program(BitGadget(n))).constraints
        assert len(cons) == rows and max(len(part) for abc in cons for part in abc) == longest
    assert len(flatten(Program(Multiplier2())).constraints) == 1


# ---- without a GPU ---------------------------------------------------------------------------------------------------------------
def test_the_library_exports_the_products():
    from circom_amd import runtime as rt
    L = rt.lib()
    assert hasattr(L, "cw_get_r1cs_products") and hasattr(L, "cw_get_r1cs_products_device")
    assert hasattr(rt.Batch, "r1cs_products") and hasattr(rt.Batch, "r1cs_products_device")
    assert (rt.R1CS_A, rt.R1CS_B, rt.R1CS_C) == (1, 2, 4)


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
    """a host-only batch: every CW_EINVAL case is CW_EINVAL, and only a call whose arguments are in order reaches CW_EDEVICE"""
    from circom_amd import runtime as rt
    L = rt.lib()
    c = _host_circuit(tmp_path, kind)
    nc, B, eb = c.n_constraints, 5, c.element_bytes
    assert nc >= 1 and eb == (8 if kind == "m2g" else 32)
    b = c.batch(B, device=-1)
    out = np.full(B * 3 * nc * eb + 16, 0xA5, dtype=np.uint8)
    p = out.ctypes.data_as(C.c_void_p)
    host = lambda parts, r0, n, f, cnt, ptr, h=b.h: L.cw_get_r1cs_products(h, parts, r0, n, f, cnt, ptr)
    dev = lambda parts, r0, n, f, cnt, ptr, h=b.h: L.cw_get_r1cs_products_device(h, parts, r0, n, f, cnt, ptr)
    d = C.c_void_p(4096)
    for call, ptr, name in ((host, p, "cw_get_r1cs_products:"), (dev, d, "cw_get_r1cs_products_device:")):
        assert call(7, 0, nc, 0, B, ptr, h=None) == CW_EINVAL                          # null batch
        assert call(7, 0, nc, 0, B, None) == CW_EINVAL                                 # null image
        for parts in (0, 8, 9, 15, 0x80000001):                                        # no part / a bit outside 7
            assert call(parts, 0, nc, 0, B, ptr) == CW_EINVAL and name in L.cw_last_error().decode()
        assert call(7, 0, nc + 1, 0, B, ptr) == CW_EINVAL                              # rows past the system
        assert call(7, nc, 1, 0, B, ptr) == CW_EINVAL
        assert call(7, nc + 1, 0, 0, B, ptr) == CW_EINVAL
        assert call(7, 1, 0xFFFFFFFF, 0, B, ptr) == CW_EINVAL                          # row0 + n_rows wraps in 32 bits
        assert call(7, 0xFFFFFFFF, 1, 0, B, ptr) == CW_EINVAL
        assert call(7, 0, nc, 0, B + 1, ptr) == CW_EINVAL                              # instances past the batch
        assert call(7, 0, nc, B, 1, ptr) == CW_EINVAL
        assert call(7, 0, nc, B + 1, 0, ptr) == CW_EINVAL
        assert call(7, 0, nc, 2, 0xFFFFFFFF, ptr) == CW_EINVAL                         # first + count wraps
        assert name in L.cw_last_error().decode()
    # alignment of the device image: 8 bytes for 8-byte elements, 16 for 32-byte ones; the range comes first
    assert dev(7, 0, nc, 0, B, C.c_void_p(4096 + 4)) == CW_EINVAL
    assert "aligned" in L.cw_last_error().decode()
    assert dev(7, 0, nc, 0, B, C.c_void_p(4096 + 8)) == (CW_EDEVICE if eb == 8 else CW_EINVAL)
    assert dev(7, 0, nc + 1, 0, B, C.c_void_p(4096 + 4)) == CW_EINVAL and "row range" in L.cw_last_error().decode()
    # in order: the device comes next, the empty ranges included (and the state after it - with a device, below)
    for call, ptr in ((host, p), (dev, d)):
        assert call(7, 0, nc, 0, B, ptr) == CW_EDEVICE
        assert call(1, nc - 1, 1, B - 1, 1, ptr) == CW_EDEVICE
        assert call(5, 0, 0, 0, B, ptr) == CW_EDEVICE and call(5, nc, 0, 0, B, ptr) == CW_EDEVICE
        assert call(2, 0, nc, 3, 0, ptr) == CW_EDEVICE and call(2, 0, nc, B, 0, ptr) == CW_EDEVICE
    assert host(7, 0, nc, 0, B, C.c_void_p(out.ctypes.data + 1)) == CW_EDEVICE         # a host image of any alignment
    assert (out == 0xA5).all()                                                         # nothing was written
    with pytest.raises(rt.CwError) as e:
        b.r1cs_products(parts=8)
    assert e.value.code == CW_EINVAL
    with pytest.raises(rt.CwError) as e:
        b.r1cs_products_device(7, 0, nc, 0, B, 4096)
    assert e.value.code == CW_EDEVICE
    b.close(); c.close()


def _plan_terms(plan, k, p):
    t0, t1 = int(plan["rowptr"][3 * k + p]), int(plan["rowptr"][3 * k + p + 1])
    return plan["terms"][t0:t1]


def _tab(plan, ident):
    return int.from_bytes(plan["ctab"][ident].tobytes(), "little")


@pytest.mark.parametrize("name", ["poseidon2", "bitgadget15"])
def test_the_plan_is_the_constraint_system_in_file_order(tmp_path, name):
    """the 256-bit plan: per constraint of the file and part the same terms as fc.constraints, with the coefficient ids of the
    check's table (0 = +1, 1 = -1, bit 31 = the constant wire and the table's form of the coefficient, else c * 2^261 mod q)"""
    from circom_amd import runtime as rt
    if name == "poseidon2":
        cp = compile_program(Program(Poseidon(2)), str(tmp_path), name, sym=False, strands=(1,), pipe=None, fpjit=False)
    else:
        cp = compile_program(Program(BitGadget(15)), str(tmp_path), name, sym=False, strands=(1,), bits=True, jit=False)
    c = rt.Circuit(cp.tape_path, cp.dat_path, cp.r1cs_path)
    fc, q = cp.flat, cp.flat.fp.q
    assert c.montgomery == (name == "poseidon2")
    plan = c.r1cs_products_plan()
    assert len(plan["rowptr"]) == 3 * len(fc.constraints) + 1 and plan["rowptr"][0] == 0 and plan["terms"].shape[1] == 2
    assert int(plan["rowptr"][-1]) == len(plan["terms"]) == sum(len(part) for abc in fc.constraints for part in abc)
    for k, abc in enumerate(fc.constraints):
        for p, part in enumerate(abc):
            got = []
            for slot, ident in _plan_terms(plan, k, p):
                slot, ident = int(slot), int(ident)
                if ident == 0:
                    co = 1
                elif ident == 1:
                    co = q - 1
                elif ident >> 31:
                    assert slot == 0
                    co = _tab(plan, ident & 0x7FFFFFFF)
                    if c.montgomery:
                        co = co * pow(2, -RBITS, q) % q
                else:
                    co = _tab(plan, ident) * pow(2, -RBITS, q) % q
                got.append((slot, co % q))
            assert sorted(got) == sorted((s, co % q) for s, co in part.items()), (k, p)
    if name == "bitgadget15":
        # the bit-plane plan: the same terms on bit-table slots (a function of the signal; the constant wire is slot 1), canonical
        # coefficients from the table of their own
        bplan = c.r1cs_products_plan(bits=True)
        assert (bplan["rowptr"] == plan["rowptr"]).all()
        slot_of = {0: 1}
        for k, abc in enumerate(fc.constraints):
            for p, part in enumerate(abc):
                wide, bits = _plan_terms(plan, k, p), _plan_terms(bplan, k, p)
                want = sorted((s, co % q) for s, co in part.items())
                assert sorted((int(s), _tab(bplan, int(i))) for (s, _), (_, i) in zip(wide, bits)) == want, (k, p)
                for (s, _), (bs, _) in zip(wide, bits):
                    assert slot_of.setdefault(int(s), int(bs)) == int(bs) and int(bs) != 2
    c.close()


def test_the_64_bit_plan_is_the_constraint_system_in_file_order(tmp_path):
    from circom_amd import runtime as rt
    cp = compile_program(Program(Poseidon(2), prime="goldilocks"), str(tmp_path), "glpos", sym=False)
    c = rt.Circuit(cp.tape_path, cp.dat_path, cp.r1cs_path)
    fc, q = cp.flat, cp.flat.fp.q
    plan = c.r1cs_products_plan()
    assert len(plan["rowptr"]) == 3 * len(fc.constraints) + 1 and plan["terms"].shape[1] == 4 and plan["ctab"].size == 0
    assert int(plan["rowptr"][-1]) == len(plan["terms"]) == sum(len(part) for abc in fc.constraints for part in abc)
    for k, abc in enumerate(fc.constraints):
        for p, part in enumerate(abc):
            got = sorted((int(s), int(lo) | int(hi) << 32) for s, z, lo, hi in _plan_terms(plan, k, p))
            assert got == sorted((s, co % q) for s, co in part.items()), (k, p)
    with pytest.raises(rt.CwError) as e:
        c.r1cs_products_plan(bits=True)
    assert e.value.code == CW_ESTATE
    c.close()


# ---- GPU -------------------------------------------------------------------------------------------------------------------------
class _Dev(_Hip):
    """one arena; every image lies between GUARD bytes of 0xA5 in front and behind, and the call sees 0xA5 where it writes"""
    SIZE = 36 << 20

    def __init__(self):
        super().__init__()
        self.h.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
        self.h.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        self.base = self.alloc(self.SIZE)

    def fill(self, nbytes):
        assert nbytes + 2 * GUARD <= self.SIZE
        assert self.h.hipMemset(self.base, 0xA5, nbytes + 2 * GUARD) == 0
        return self.base + GUARD

    def image(self, nbytes):
        raw = self.download(self.base, nbytes + 2 * GUARD)
        assert (raw[:GUARD] == 0xA5).all() and (raw[GUARD + nbytes:] == 0xA5).all(), "the guard bytes"
        return raw[GUARD:GUARD + nbytes]

    def products(self, b, parts, row0, n, first, count):
        eb, n_sel = b.circuit.element_bytes, bin(parts).count("1")
        nbytes = count * n_sel * n * eb
        b.r1cs_products_device(parts, row0, n, first, count, self.fill(nbytes))
        return self.image(nbytes).reshape(count, n_sel, n, eb)


def _host_products(b, parts, row0, n, first, count):
    from circom_amd import runtime as rt
    eb, n_sel = b.circuit.element_bytes, bin(parts).count("1")
    nbytes = count * n_sel * n * eb
    raw = np.full(nbytes + 2 * GUARD + 1, 0xA5, dtype=np.uint8)
    rt._chk(rt.lib().cw_get_r1cs_products(b.h, parts, row0, n, first, count, C.c_void_p(raw.ctypes.data + GUARD + 1)))   # an odd address
    assert (raw[:GUARD + 1] == 0xA5).all() and (raw[GUARD + 1 + nbytes:] == 0xA5).all(), "the guard bytes"
    return raw[GUARD + 1:GUARD + 1 + nbytes].reshape(count, n_sel, n, eb)


@pytest.fixture(scope="module")
def hip():
    return _Dev()


@pytest.fixture(scope="module")
def circuits(tmp_path_factory):
    """every circuit of this module, compiled once: name -> (flat circuit, runtime circuit)"""
    from circom_amd import runtime as rt
    from test_goldilocks_egress import CASES
    made = {}

    def get(name):
        if name not in made:
            d = str(tmp_path_factory.mktemp(name))
            if name.startswith("bg"):
                cp = compile_program(Program(BitGadget(int(name[2:]))), d, name, sym=False, strands=(1,), bits=True, jit=True)
                assert cp.jit is not None
            elif name == "gl15":
                cp = compile_program(Program(BitGadget(15), prime="goldilocks"), d, name, sym=False)
            elif name == "glpos":
                cp = compile_program(CASES["poseidon2"][0](), d, name, sym=False)
            elif name == "pos":
                cp = compile_program(Program(Poseidon(2)), d, name, sym=False, strands=(1,), pipe=None, fpjit=True)
            elif name == "posbls":
                cp = compile_program(Program(Poseidon(2), prime="bls12381"), d, name, sym=False, strands=(1,), pipe=None, fpjit=True)
            elif name == "bassert":
                cp = compile_program(Program(BitAssert()), d, name, sym=False, strands=(1,), bits=True, jit=True)
            elif name == "m2":
                cp = compile_program(Program(Multiplier2()), d, name, sym=False, strands=(1,), pipe=None)
            else:
                assert name == "m2g"
                cp = compile_program(Program(Multiplier2(), prime="goldilocks"), d, name, sym=False)
            made[name] = (cp.flat, rt.Circuit(cp.tape_path, cp.dat_path, cp.r1cs_path))
        return made[name]

    yield get
    for _, c in made.values():
        c.close()


def _matrix(hip, b, img, B, row_ranges=ROW_RANGES, ranges=None, host=True):
    """every row range x every instance range x every part mask, device form and host form, against the model image"""
    nc = img.shape[2]
    for row0, n in row_ranges:
        n = nc - row0 if n is None else n
        for first, count in (inst_ranges(B) if ranges is None else ranges):
            for parts in MASKS:
                want = select(img, parts, row0, n, first, count)
                got = hip.products(b, parts, row0, n, first, count)
                assert got.shape == want.shape and (got == want).all(), ("device", parts, row0, n, first, count)
                if host:
                    got = _host_products(b, parts, row0, n, first, count)
                    assert (got == want).all(), ("host", parts, row0, n, first, count)


def _run_clean(b, feed):
    feed(b)
    b.run(); b.check_r1cs(); b.sync()
    assert (b.status() == 0).all()


def _feed_bits(bits):
    return lambda b: b.set_inputs_rows(pack_rows(bits, (bits.shape[1] + 7) // 8, True))


@pytest.mark.gpu
@pytest.mark.parametrize("kind,B", [("gl15", 65), ("gl15", 300), ("glpos", 65), ("glpos", 300)])
def test_gpu_goldilocks_at_the_tile_edges(circuits, hip, kind, B):
    fc, c = circuits(kind)
    if kind == "gl15":
        _, bits, img = _bg_case(15, "goldilocks")
        feed = _feed_bits(bits[:B])
    else:
        _, rows, _, img = _glpos_case()
        feed = lambda b: b.set_inputs([list(r) for r in rows[:B]])
    assert c.element_bytes == 8 and img.shape[2] == c.n_constraints
    b = c.batch(B)
    _run_clean(b, feed)
    _matrix(hip, b, img, B)
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind,B", [("wide15", 65), ("wide15", 300), ("pos", 65), ("pos", 300), ("posbls", 65)])
def test_gpu_256_bit_tables_at_the_tile_edges(circuits, hip, monkeypatch, kind, B):
    """the canonical table (BitGadget with CW_BITS=0) and the Montgomery-form table (Poseidon), filled by the emitted rows and by
    the interpreting kernel (CW_FP_JIT=0): the same table, so the same image - compared byte for byte, both against the model"""
    if kind == "wide15":
        fc, c = circuits("bg15")
        _, bits, img = _bg_case(15)
        feed = _feed_bits(bits[:B])
        monkeypatch.setenv("CW_BITS", "0")
    else:
        fc, c = circuits(kind)
        _, rows, img = _pos_case("bn128" if kind == "pos" else "bls12381", B)
        feed = lambda b: b.set_inputs(rows[:B])
    assert c.element_bytes == 32 and img.shape[2] == c.n_constraints and c.montgomery == (kind != "wide15")
    whole = []
    for fp_jit in ("1", "0"):
        monkeypatch.setenv("CW_FP_JIT", fp_jit)
        b = c.batch(B)
        assert not b.bitmode
        if kind != "wide15":
            assert b.emitted == (fp_jit == "1")
        _run_clean(b, feed)
        _matrix(hip, b, img, B, host=fp_jit == "1")
        whole.append(hip.products(b, 7, 0, c.n_constraints, 0, B).copy())
        b.close()
    assert (whole[0] == whole[1]).all() and (whole[0] == img[:B]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("B", [65, 300])
@pytest.mark.parametrize("n", [15, 43])
@pytest.mark.parametrize("engine", ["interp", "jit"])
def test_gpu_bitplane_at_the_tile_edges(circuits, hip, monkeypatch, engine, n, B):
    monkeypatch.setenv("CW_BITS_JIT", "1" if engine == "jit" else "0")
    fc, c = circuits("bg%d" % n)
    _, bits, img = _bg_case(n)
    b = c.batch(B)
    assert b.bitmode and b.jit == (engine == "jit") and b.bits_sh == (5 if engine == "jit" else 0)
    _run_clean(b, _feed_bits(bits[:B]))
    _matrix(hip, b, img, B)
    b.close()


ODD = (5, 63, 128, 150, 151)                       # in the middle of a group, ending one, starting one, a run of two


@functools.lru_cache(maxsize=None)
def _rerun_case():
    """BitGadget(15) x 200 where the instances of ODD have input 5 equal to 7 (it trips no check of the witness code: the
    oracle's signals are the witness): (inputs [200][45], model image [200][3][rows][32])"""
    fc, bits, img = _bg_case(15)
    vals = bits[:200].astype(np.int64)
    img = img[:200].copy()
    q = fc.fp.q
    for i in ODD:
        vals[i, 5] = 7
        sig, failed = eval_flat(q, fc.n_signals, fc.n_temps, fc.constants, fc.code, {fc.main_input_start + k: int(v) for k, v in enumerate(vals[i])})
        assert failed is None
        img[i] = as_bytes(products(q, fc.constraints, [sig]), 32)[0]
    return vals, img


@pytest.mark.gpu
@pytest.mark.parametrize("engine", ["interp", "jit"])
def test_gpu_rerun_instances_come_from_the_side_batch(circuits, hip, monkeypatch, engine):
    """non-boolean inputs: those instances are re-run by the 256-bit side batch, their products are the model's on eval_flat's
    witness for those inputs, and their neighbours' are the bit table's"""
    monkeypatch.setenv("CW_BITS_JIT", "1" if engine == "jit" else "0")
    fc, c = circuits("bg15")
    vals, img = _rerun_case()
    _, _, clean = _bg_case(15)
    B = 200
    assert all((img[i] != clean[i]).any() for i in ODD)
    image = np.zeros((B, c.n_inputs, 32), dtype=np.uint8)
    image[:, :, 0] = vals
    b = c.batch(B)
    assert b.bitmode and b.jit == (engine == "jit")
    b.set_inputs(image)
    b.run(); b.sync()
    ranges = [(0, B), (5, 1), (4, 3), (63, 2), (62, 1), (60, 10), (128, 30), (127, 2), (151, 1), (150, 2), (149, 4), (64, 64), (152, 48)]
    _matrix(hip, b, img, B, row_ranges=[(0, None), (15, 2), (3, 130)], ranges=ranges)
    b.close()


def _violations(image, q):
    """A o B - C mod q per instance and row from an image of all three parts"""
    v = as_ints(image)
    return (v[:, 0] * v[:, 1] - v[:, 2]) % q


@pytest.mark.gpu
def test_gpu_supplied_tampered_witnesses_agree_with_the_check(hip, tmp_path):
    """64-bit runtime, supplied witnesses with one entry off by one in most instances (tests/test_goldilocks_supplied.py): the
    products are the model's on the supplied values; A o B - C from the image is zero in every row where the status word is 0 and
    first non-zero in the row cw_get_r1cs_first_bad names.  A table with gaps answers "witnesses missing"."""
    from circom_amd import runtime as rt
    from test_goldilocks_supplied import CLEAN, _circuit, _tampered
    fc, sig, tampered, want_row = _tampered()
    q = fc.fp.q
    cp, c = _circuit(tmp_path, "poseidon2")
    B, nc = tampered.shape[0], c.n_constraints
    b = c.batch(B)
    with pytest.raises(rt.CwError) as e:
        b.r1cs_products()
    assert e.value.code == CW_ESTATE and "cw_get_r1cs_products before cw_run" in str(e.value)
    b.set_witnesses(tampered[:10], first=3)
    with pytest.raises(rt.CwError) as e:
        b.r1cs_products()
    assert e.value.code == CW_ESTATE and "witnesses missing for %d instances" % (B - 10) in str(e.value)
    with pytest.raises(rt.CwError) as e:
        b.r1cs_products_device(7, 0, nc, 3, 10, hip.fill(0))
    assert e.value.code == CW_ESTATE and "witnesses missing for %d instances" % (B - 10) in str(e.value)
    b.set_witnesses(tampered)
    before = hip.products(b, 7, 0, nc, 0, B).copy()                  # before the check
    b.check_r1cs(); b.sync()
    st, fb = b.status(), b.r1cs_first_bad()
    got = hip.products(b, 7, 0, nc, 0, B)
    assert (got == before).all()
    model = as_bytes(products(q, fc.constraints, [[int(v) for v in row] for row in tampered]), 8)
    assert (got == model).all() and (b.r1cs_products(parts=7) == model).all()
    bad = _violations(got, q)
    for i in range(B):
        rows = np.flatnonzero(bad[i] != 0)
        if st[i] == 0:
            assert i in CLEAN and len(rows) == 0 and fb[i] == NONE, i
        else:
            assert st[i] == R1CS_FAILED and len(rows) and rows[0] == fb[i] == want_row[i], (i, rows[:3], fb[i], want_row[i])
    _matrix(hip, b, model, B, row_ranges=[(1, 63), (3, 130)], ranges=[(0, B), (63, 2), (37, 200)])
    assert (b.status() == st).all() and (b.r1cs_first_bad() == fb).all()
    b.close(); c.close()


@pytest.mark.gpu
def test_gpu_failed_assertions_agree_with_the_check_on_the_256_bit_engine(circuits, hip, monkeypatch):
    """BitAssert (a === b, out = a b) on the 256-bit schedule: where a != b the `===` fails, the check names a row, and that row
    is the first in which A o B - C from the image is not zero; the other instances have zero in every row"""
    fc, c = circuits("bassert")
    q, B = fc.fp.q, 130
    ab = np.random.default_rng(130).integers(0, 2, size=(B, 1), dtype=np.uint8).repeat(2, axis=1)
    odd = [0, 5, 63, 64, 100, 129]
    ab[odd, 1] ^= 1
    image = np.zeros((B, 2, 32), dtype=np.uint8)
    image[:, :, 0] = ab
    monkeypatch.setenv("CW_BITS", "0")
    b = c.batch(B)
    assert not b.bitmode
    b.set_inputs(image)
    b.run(); b.sync()
    before = hip.products(b, 7, 0, c.n_constraints, 0, B).copy()     # between cw_run and cw_check_r1cs
    st0 = b.status()
    b.check_r1cs(); b.sync()
    st, fb = b.status(), b.r1cs_first_bad()
    got = hip.products(b, 7, 0, c.n_constraints, 0, B)
    assert (got == before).all() and ((st & np.uint32(0xFFFFFFFF ^ R1CS_FAILED)) == st0).all()
    sigs = []
    for x, y in ab:
        sig, _ = eval_flat(q, fc.n_signals, fc.n_temps, fc.constants, fc.code, {fc.main_input_start: int(x), fc.main_input_start + 1: int(y)})
        sigs.append(sig)
    assert (got == as_bytes(products(q, fc.constraints, sigs), 32)).all()
    bad = _violations(got, q)
    assert ((st != 0) == np.isin(np.arange(B), odd)).all()
    for i in range(B):
        rows = np.flatnonzero(bad[i] != 0)
        if st[i] == 0:
            assert len(rows) == 0 and fb[i] == NONE, i
        else:
            assert st[i] & R1CS_FAILED and len(rows) and rows[0] == fb[i], (i, rows[:3], fb[i])
    b.close()


@pytest.mark.gpu
def test_gpu_state_and_bystanders(circuits, hip):
    """CW_ESTATE before cw_run; the empty ranges write nothing; the same bytes between cw_run and cw_check_r1cs and after it;
    status words and first-bad rows with and without the call; a captured cw_run_check graph stays captured and replays the same
    witnesses"""
    from circom_amd import runtime as rt
    L = rt.lib()
    fc, c = circuits("bg15")
    _, bits, img = _bg_case(15)
    B, nc = 65, c.n_constraints
    b = c.batch(B)
    with pytest.raises(rt.CwError) as e:
        b.r1cs_products()
    assert e.value.code == CW_ESTATE and "cw_get_r1cs_products before cw_run" in str(e.value)
    with pytest.raises(rt.CwError) as e:
        b.r1cs_products_device(7, 0, nc, 0, B, hip.fill(0))
    assert e.value.code == CW_ESTATE and "cw_get_r1cs_products_device before cw_run" in str(e.value)
    assert L.cw_get_r1cs_products_device(b.h, 7, 0, nc + 1, 0, B, C.c_void_p(hip.base)) == CW_EINVAL        # the argument first
    rows = pack_rows(bits[:B], 8, True)
    b.set_inputs_rows(rows)
    b.run()
    between = hip.products(b, 7, 0, nc, 0, B).copy()
    b.check_r1cs(); b.sync()
    st, fb = b.status(), b.r1cs_first_bad()
    assert (st == 0).all() and (fb == NONE).all()
    after = hip.products(b, 7, 0, nc, 0, B)
    assert (between == after).all() and (after == img[:B]).all()
    assert (b.status() == st).all() and (b.r1cs_first_bad() == fb).all()
    # the empty ranges: CW_OK, nothing written, on both forms
    for parts, row0, n, first, count in ((7, 3, 0, 0, B), (1, nc, 0, 0, B), (5, 0, nc, 7, 0), (2, 0, nc, B, 0), (4, 0, 0, 0, 0)):
        p = hip.fill(64)
        b.r1cs_products_device(parts, row0, n, first, count, p)
        assert (hip.image(64) == 0xA5).all()
        raw = np.full(64, 0xA5, dtype=np.uint8)
        assert L.cw_get_r1cs_products(b.h, parts, row0, n, first, count, raw.ctypes.data_as(C.c_void_p)) == 0 and (raw == 0xA5).all()
    assert b.r1cs_products(n_rows=0).shape == (B, 2, 0, 32) and b.r1cs_products(count=0).shape == (0, 2, nc, 32)
    # the Python form: parts A | B by default, the whole system, the whole batch
    assert (b.r1cs_products() == img[:B, :2]).all()
    assert (b.r1cs_products(parts=C_, row0=15, n_rows=2, first=63, count=2) == select(img, 4, 15, 2, 63, 2)).all()
    b.close()
    # a captured graph: the third cw_run_check with unchanged inputs replays it; the call between the replays changes nothing
    hipr = _Hip()
    p = hipr.upload(np.ascontiguousarray(rows))
    b = c.batch(B)
    b.set_inputs_rows_device(p, 8)
    for _ in range(3):
        b.run_check(); b.sync()
    assert b.graph_captured
    wit = b.witnesses().copy()
    assert (hip.products(b, 7, 0, nc, 0, B) == img[:B]).all() and (b.r1cs_products(parts=7) == img[:B]).all()
    assert b.graph_captured
    b.run_check(); b.sync()
    assert b.graph_captured and (b.witnesses() == wit).all() and (b.status() == 0).all()
    assert (hip.products(b, 7, 0, nc, 0, B) == img[:B]).all()
    hipr.h.hipFree(p)
    b.close()


@pytest.mark.gpu
def test_gpu_a_shortened_witness_list_changes_nothing(hip, tmp_path):
    """cw_set_witness_list shortens egress, not the check, and not the products: the full system is used"""
    from circom_amd import runtime as rt
    cp = compile_program(Program(BitGadget(15), prime="goldilocks"), str(tmp_path), "gl15s", sym=False)
    _, bits, img = _bg_case(15, "goldilocks")
    B = 65
    images = []
    for short in (False, True):
        c = rt.Circuit(cp.tape_path, cp.dat_path, cp.r1cs_path)
        if short:
            c.set_witness_list(np.arange(0, 20, dtype=np.uint32))
            assert c.n_witness == 20
        b = c.batch(B)
        _run_clean(b, _feed_bits(bits[:B]))
        images.append(hip.products(b, 7, 0, c.n_constraints, 0, B).copy())
        assert (b.r1cs_products(parts=5, row0=3, n_rows=130) == select(img, 5, 3, 130, 0, B)).all()
        b.close(); c.close()
    assert (images[0] == images[1]).all() and (images[0] == img[:B]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["m2", "m2g"])
def test_gpu_more_instance_tiles_than_a_grid_dimension_of_rows(circuits, hip, name):
    """Multiplier2 x 70 001 on both value engines: 1 094 instance tiles; the single row is (-a) b = -out, so A = q - a, B = b, C = q - a b"""
    fc, c = circuits(name)
    q, B, eb = fc.fp.q, 70001, c.element_bytes
    assert c.n_constraints == 1
    rng = np.random.default_rng(70001)
    ab = rng.integers(0, 1 << 31, size=(B, 2), dtype=np.uint64)
    for i, v in ((0, (3, 11)), (65535, (1, 1)), (65536, (0, 5)), (70000, (2 ** 31 - 1, 2 ** 31 - 1))):
        ab[i] = v
    image = np.zeros((B, 2, 4), dtype="<u8")
    image[:, :, 0] = ab
    b = c.batch(B)
    b.set_inputs(image.view(np.uint8).reshape(B, 2, 32))
    b.run(); b.check_r1cs(); b.sync()
    assert (b.status() == 0).all()
    a_, b__ = ab[:, 0].astype(object), ab[:, 1].astype(object)
    assert fc.constraints == [({2: q - 1}, {3: 1}, {1: q - 1})] and fc.main_input_start == 2      # the row is (-a) b = -out
    want = as_bytes(products(q, fc.constraints, np.stack([a_ * 0 + 1, (a_ * b__) % q, a_, b__], axis=1)), eb)
    got = hip.products(b, 7, 0, 1, 0, B)
    assert (got == want).all()
    assert as_ints(got[0, :, 0]).tolist() == [q - 3, 11, q - 33]
    assert (b.r1cs_products(parts=7) == want).all()
    assert (hip.products(b, 5, 0, 1, 65530, 4471) == want[65530:, [0, 2]]).all()
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["bits", "gl", "wide"])
def test_gpu_the_image_is_complete_in_stream_order(circuits, hip, monkeypatch, kind):
    """the device form, then a device-to-device copy on the batch's stream, no synchronisation between them: the copy holds the
    complete image.  A second call with another range into the same buffer overwrites only its own bytes"""
    B = 65
    if kind == "gl":
        fc, c = circuits("gl15")
        _, bits, img = _bg_case(15, "goldilocks")
    else:
        fc, c = circuits("bg15")
        _, bits, img = _bg_case(15)
        if kind == "wide":
            monkeypatch.setenv("CW_BITS", "0")
    b = c.batch(B)
    assert b.bitmode == (kind == "bits")
    _run_clean(b, _feed_bits(bits[:B]))
    eb, nc = c.element_bytes, c.n_constraints
    nbytes = B * 3 * nc * eb
    copy = hip.alloc(nbytes)
    b.r1cs_products(n_rows=1, count=1)                            # (a bit-plane batch: the first egress after a run has waited; the plan is up)
    p = hip.fill(nbytes)
    b.r1cs_products_device(7, 0, nc, 0, B, p)
    assert hip.h.hipMemcpyAsync(copy, p, nbytes, 3, None) == 0     # the batch's stream is the null stream
    got = hip.download(copy, nbytes).reshape(B, 3, nc, eb)
    assert (got == img[:B]).all()
    b.r1cs_products_device(B_, 3, 130, 1, 2, p)
    assert hip.h.hipMemcpyAsync(copy, p, nbytes, 3, None) == 0
    got2 = hip.download(copy, nbytes)
    small = 2 * 130 * eb
    assert (got2[:small].reshape(2, 1, 130, eb) == select(img, 2, 3, 130, 1, 2)).all()
    assert (got2[small:] == got.reshape(-1)[small:]).all() and (hip.image(nbytes) == got2).all()
    hip.h.hipFree(copy)
    b.close()
