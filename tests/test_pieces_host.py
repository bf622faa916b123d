"""cw_pieces (circom_amd/csrc/cw_pieces.h), the one walk over `count` items in pieces of at most `per` behind every split
kernel launch and every staged bulk transfer, exercised by a stand-alone program (tests/host/pieces_test.cpp) built with the
address and undefined-behaviour sanitizers: counts around one and two pieces for both launch limits (65 535 and 65 535 x 64),
2^32 - 1 items (where a 32-bit running offset wraps), a piece larger than the count, and a callback that ends the walk."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]


def test_pieces_walk_covers_the_count_once_and_stops_on_error(tmp_path):
    exe = tmp_path / "pieces_test"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", str(ROOT / "tests" / "host" / "pieces_test.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "pieces ok: 37 checks" in r.stdout
