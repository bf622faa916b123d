"""cw_wtns_parse (circom_amd/csrc/cw_wtns_read.h): the one pass that reads and checks a `.wtns` file before its body goes to
the device as a supplied witness (cw_read_wtns, cw_read_wtns_many), exercised by a stand-alone program
(tests/host/wtns_read_test.cpp) built with the address and undefined-behaviour sanitizers: a good 8-byte and a good 32-byte file,
the sections in either order, every reason for a refusal, a good file cut at every byte."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]


def test_wtns_reader(tmp_path):
    exe = tmp_path / "wtns_read_test"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", str(ROOT / "tests" / "host" / "wtns_read_test.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "wtns read ok: " in r.stdout
