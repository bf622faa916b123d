"""cw_columns.h (circom_amd/csrc), the HIP-free host part of input columns (cw_set_inputs_range*, cw_set_input_column*), exercised
by a stand-alone program (tests/host/columns_test.cpp) built with the address and undefined-behaviour sanitizers: the checks of
width, stride and alignment in their stated order, the coverage bitmap against a plain array of flags at the edges of its 64-bit
words, the widening of one value to a 32-byte cell, and the repacking of rows with odd strides whose last row ends at the very
end of its allocation (pad bytes 0xA5)."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]


def test_columns_checks_coverage_widening_and_repacking(tmp_path):
    exe = tmp_path / "columns_test"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", str(ROOT / "tests" / "host" / "columns_test.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "columns ok: 209 checks" in r.stdout
