"""cw_rows.h (circom_amd/csrc), the HIP-free host part of boolean inputs as packed rows (cw_set_inputs_rows*), exercised by a
stand-alone program (tests/host/rows_test.cpp) built with the address and undefined-behaviour sanitizers: the bit of input k
for both bit orders at k = 0, 7, 8, 63, 64, n - 1, the flag / stride / alignment checks, and the repacking of rows with odd
strides whose last row ends at the very end of its allocation (pad bytes and spare bits all ones)."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]


def test_rows_bit_order_checks_and_repacking(tmp_path):
    exe = tmp_path / "rows_test"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", str(ROOT / "tests" / "host" / "rows_test.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "rows ok: 123 checks" in r.stdout
