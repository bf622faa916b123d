"""cw_bits_layout.h (circom_amd/csrc), the HIP-free index arithmetic of the bit table, exercised by a stand-alone program
(tests/host/bits_rows_layout_test.cpp) built with the address and undefined-behaviour sanitizers: the whole-row input writer of
the emitted code's table is replayed thread by thread for n_groups in {1, 2, 32, 34, 64} x n_in in {1, 63, 64, 120, 384}, each with
a full last group and with a last group of 5 instances.  Every input row is written exactly once in all 32 group columns of every
chunk, real groups at the table formula's address with their (masked) mask, padding columns as 0, nothing else is written."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]


def test_row_writer_walk_covers_the_input_rows_exactly_once(tmp_path):
    exe = tmp_path / "bits_rows_layout_test"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", str(ROOT / "tests" / "host" / "bits_rows_layout_test.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "bits rows layout ok: 50 shapes" in r.stdout
