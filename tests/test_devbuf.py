"""DevBuf<T> (circom_amd/csrc/cw_devbuf.h), the owner of every device allocation of the host library, exercised by a
stand-alone program over a counting malloc / free (tests/host/devbuf_test.cpp), built with the address and
undefined-behaviour sanitizers: a double free, a leak or a use after free in the holder ends the program with an error."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]


def test_devbuf_frees_every_allocation_once(tmp_path):
    exe = tmp_path / "devbuf_test"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", str(ROOT / "tests" / "host" / "devbuf_test.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "devbuf ok: 11 allocations, 11 frees" in r.stdout
