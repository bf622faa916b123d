"""cw_fn64_parse (circom_amd/csrc/cw_fn64.h): the one pass that reads and checks the function section of a 64-bit tape before
the device interpreter trusts it, exercised by a stand-alone program (tests/host/fn64_test.cpp) built with the address and
undefined-behaviour sanitizers: good sections, every reason for a refusal, a section cut at every byte."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]


def test_function_section_validator(tmp_path):
    exe = tmp_path / "fn64_test"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", str(ROOT / "tests" / "host" / "fn64_test.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "fn64 ok: " in r.stdout
