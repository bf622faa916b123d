"""cw_r1cs_products.h (circom_amd/csrc), the HIP-free host part of the R1CS products (cw_get_r1cs_products*), exercised by a
stand-alone program (tests/host/r1cs_products_test.cpp) built with the address and undefined-behaviour sanitizers: the checks of
the part mask and the two ranges, the alignment of a device image, the plan in file order out of the loaders' arrays, the split
of a row range into launches of at most 65 535 tiles, and the place of a staged piece of instances in the caller's image."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]


def test_r1cs_products_checks_plan_pieces_and_staging(tmp_path):
    exe = tmp_path / "r1cs_products_test"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", str(ROOT / "tests" / "host" / "r1cs_products_test.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "r1cs products ok: 150 checks" in r.stdout
