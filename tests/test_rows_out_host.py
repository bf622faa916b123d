"""The output half of cw_rows.h (circom_amd/csrc), the HIP-free host part of witness bits as packed rows (cw_get_witness_rows*),
exercised by a stand-alone program (tests/host/rows_out_test.cpp) built with the address and undefined-behaviour sanitizers: the
range and word checks, the flag / stride / alignment checks at the sizes of an entry range, and the copy of staged rows of whole
words into caller rows with odd strides whose last row ends at the very end of its allocation (pad bytes stay as they were)."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]


def test_rows_out_checks_and_the_copy_into_caller_rows(tmp_path):
    exe = tmp_path / "rows_out_test"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", str(ROOT / "tests" / "host" / "rows_out_test.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "rows out ok: 85 checks" in r.stdout
