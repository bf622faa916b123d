"""cw_rerun_runs (circom_amd/csrc/cw_rerun.h), the one walk over the re-run instances of a bit-plane batch that every egress
patches its image with, exercised by a stand-alone program (tests/host/rerun_test.cpp) built with the address and
undefined-behaviour sanitizers: the runs of {3, 64, 65, 129} under four windows, the identity list, empty list and window,
and instances next to 2^32."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]


def test_rerun_walk_yields_the_clipped_runs(tmp_path):
    exe = tmp_path / "rerun_test"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", str(ROOT / "tests" / "host" / "rerun_test.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "rerun ok: 13 checks" in r.stdout
