"""cw_bits_layout.h (circom_amd/csrc): the lane map and the LDS ring of the 32-byte ingest (cw_bits_ingest_kernel: lane = one
16-byte piece, every 128-byte line read by one instruction), exercised by a stand-alone program
(tests/host/bits_ingest_line_test.cpp) built with the address and undefined-behaviour sanitizers.  One group is replayed thread by
thread for n_in in {1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 300} x {1, 63, 64} instances x three group numbers (three rotations),
full groups with rings of 4, 8 and 16 slots: every (instance, input) gives exactly one low and one high piece, nothing is read
beyond 2 n_in or the last instance, a ring slot is read after the wait that covers its load and re-targeted only after it was
read, and the folded masks equal the plain definition."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]


def test_line_map_and_ring_cover_every_piece_once(tmp_path):
    exe = tmp_path / "bits_ingest_line_test"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", str(ROOT / "tests" / "host" / "bits_ingest_line_test.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "bits ingest line ok: 165 shapes" in r.stdout
