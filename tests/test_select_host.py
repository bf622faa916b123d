"""cw_select.h (circom_amd/csrc), the HIP-free host part of instance lists (cw_select_instances*, cw_get_witnesses_at*), exercised
by a stand-alone program (tests/host/select_test.cpp) built with the address and undefined-behaviour sanitizers: the argument
checks (entry ranges that wrap in 32 bits, every alignment, every refusal), the validation of host lists that end at the very end
of their allocation, the piece arithmetic of the host form and the block geometry of the select kernels."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]


def test_select_checks_lists_and_pieces(tmp_path):
    exe = tmp_path / "select_test"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", str(ROOT / "tests" / "host" / "select_test.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "select ok: 37 checks" in r.stdout
