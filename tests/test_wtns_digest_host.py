"""Witness digests on the CPU (cw_get_wtns_digests*, include/circom_amd.h): the HIP-free plan and the shared SHA-256
(circom_amd/csrc/cw_wtns_digest.h, cw_sha256.h) replayed by a stand-alone program (tests/host/wtns_digest_test.cpp) built with the
address and undefined-behaviour sanitizers and run as a plain executable - the text the three kernels compile.  The expected
digests come from hashlib over writers.wtns_bytes, the expected headers from the reference runtime's files in tests/golden/.
The argument order of the calls themselves is checked on a host-only batch through the library."""
import ctypes as C
import hashlib
import json
import random
import subprocess
from pathlib import Path

import numpy as np
import pytest

from circom_amd import runtime as rt
from circom_amd.hip_elements.writers import wtns_bytes
from oracle.field import PRIMES

ROOT = Path(__file__).resolve().parents[1]
GOLD = json.loads((ROOT / "tests" / "golden" / "reference_wtns.json").read_text())
GOLD_GL = json.loads((ROOT / "tests" / "golden" / "reference_wtns_goldilocks.json").read_text())


def _cases():
    rng = random.Random(20261021)
    lines = []
    for n8, q in ((32, PRIMES["bn128"]), (8, PRIMES["goldilocks"])):
        for nw in list(range(1, 41)) + [1108]:
            vals = [1] + [rng.randrange(q) for _ in range(nw - 1)]
            vals[-1] = q - 1 if nw > 1 else 1                          # every byte of the last element counts
            img = wtns_bytes(q, vals)
            hdr = 44 + n8
            assert len(img) == hdr + n8 * nw
            lines.append("D %d %d %s %s %s" % (n8, nw, q.to_bytes(n8, "little").hex(), hashlib.sha256(img).hexdigest(), img[hdr:].hex()))
    # the header builder against the reference runtime's own files
    for gold, name, prime in ((GOLD, "multiplier2", "bn128"), (GOLD, "multiplier2_bls12381", "bls12381"), (GOLD_GL, "multiplier2", "goldilocks")):
        vec = gold["cases"][name]["vectors"][0]
        q = PRIMES[prime]
        n8 = 8 if prime == "goldilocks" else 32
        img = bytes.fromhex(vec["wtns_hex"])
        assert len(img) == vec["wtns_len"] == 44 + n8 + 4 * n8
        lines.append("H %d 4 %s %s" % (n8, q.to_bytes(n8, "little").hex(), img[:44 + n8].hex()))
    return lines


def test_plan_and_sha256_replayed_on_the_cpu(tmp_path):
    exe = tmp_path / "wtns_digest_test"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", str(ROOT / "tests" / "host" / "wtns_digest_test.cpp"), "-o", str(exe)], check=True)
    lines = _cases()
    assert len(lines) == 2 * 41 + 3
    (tmp_path / "cases.txt").write_text("\n".join(lines) + "\n")
    r = subprocess.run([str(exe), str(tmp_path / "cases.txt")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "wtns digest ok:" in r.stdout
    n = int(r.stdout.split("wtns digest ok:")[1].split()[0])
    assert n > 7 * 82, r.stdout                    # every case was read and checked, not only the checks without a file


def test_argument_order_on_a_host_only_batch(tmp_path):
    from circom_amd.compiler import compile_program
    from circom_amd.frontend.dsl import Program
    from circom_amd.circuits.basic import Multiplier2
    cp = compile_program(Program(Multiplier2()), str(tmp_path), "multiplier2")
    c = rt.Circuit(cp.tape_path, cp.dat_path, cp.r1cs_path)
    b = c.batch(64, device=-1)
    L = rt.lib()
    out = np.zeros((64, 32), dtype=np.uint8)
    ptr = out.ctypes.data_as(C.c_void_p)
    aligned = C.c_void_p(0x7000000)                 # never touched: a host-only batch refuses before it looks at the memory

    def err():
        return L.cw_last_error().decode()
    for fn in (L.cw_get_wtns_digests, L.cw_get_wtns_digests_device):
        assert fn(None, 0, 1, ptr) == -2 and fn(b.h, 0, 1, None) == -2                                 # null
        assert fn(b.h, 0, 65, aligned) == -2 and fn(b.h, 64, 1, aligned) == -2                          # past the batch
        assert fn(b.h, 0xFFFFFFFF, 2, aligned) == -2 and fn(b.h, 2, 0xFFFFFFFF, aligned) == -2          # would wrap in 32 bits
        assert "range" in err()
    assert L.cw_get_wtns_digests_device(b.h, 0, 1, C.c_void_p(0x7000008)) == -2 and "aligned" in err()   # CW_EINVAL before the device
    assert L.cw_get_wtns_digests(b.h, 0, 1, C.c_void_p(out.ctypes.data + 1)) == -4                       # the host form takes any address
    for fn in (L.cw_get_wtns_digests, L.cw_get_wtns_digests_device):
        assert fn(b.h, 0, 64, aligned if fn is L.cw_get_wtns_digests_device else ptr) == -4 and "host-only" in err()
        assert fn(b.h, 0, 0, aligned if fn is L.cw_get_wtns_digests_device else ptr) == -4              # the device comes before `empty`
    with pytest.raises(rt.CwError) as e:
        b.wtns_digests()
    assert e.value.code == -4 and not out.any()
    b.close(); c.close()
