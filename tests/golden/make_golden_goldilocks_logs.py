"""`python tests/golden/make_golden_goldilocks_logs.py` -> reference_logs_goldilocks.json: what the reference's own 64-bit runtime
(goldilocks/fr.hpp + common64/{main,calcwit}.cpp, built by oracle/Makefile circuit64 from oracle/emit_ref_cpp.py's 64-bit mode)
prints on stdout for LogDemo over the Goldilocks prime, with the exit status and the digest of the `.wtns` it writes.  For an
instance that fails a run-time check only the lines BEFORE the reference's own failure trace are kept (`log`), as make_golden.py
logs does.  Runs only where the reference tree is; the tests read the committed JSON."""
import hashlib
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from circom_amd.circuits.basic import LogDemo                 # noqa: E402
from circom_amd.frontend.dsl import Program                    # noqa: E402
from circom_amd.frontend.flatten import flatten                # noqa: E402
from oracle import ref_build                                   # noqa: E402

Q = 18446744069414584321


def rows():
    # (13, 2) fails the run-time check (flat operation 16): the process exits there, later statements are not printed
    return [(5, 6), (13, 2), (Q - 1, 7), (0, 0), (Q - 2, Q - 3), (1, Q - 1), (1 << 63, 1 << 32), (12345678901234567890 % Q, 987654321)]


def main():
    fc = flatten(Program(LogDemo(), prime="goldilocks"))
    cli = ref_build.build_circuit64(fc, "logdemo64")
    d = tempfile.mkdtemp(prefix="golden64_logs_")
    vectors = []
    for a, b in rows():
        out = os.path.join(d, "o.wtns")
        if os.path.exists(out):
            os.unlink(out)
        r = ref_build.run_cli64(cli, json.dumps({"a": str(a), "b": str(b)}), out)
        ok = r.returncode == 0
        vectors.append({"inputs": {"a": str(a), "b": str(b)}, "log": r.stdout if ok else r.stdout[:r.stdout.index("Failed assert")], "ok": ok,
                        "wtns_sha256": hashlib.sha256(open(out, "rb").read()).hexdigest() if ok else None})
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_logs_goldilocks.json")
    with open(path, "w") as f:
        json.dump({"generator": "tests/golden/make_golden_goldilocks_logs.py",
                   "runtime": "reference goldilocks/fr.hpp + common64/{main,calcwit}.cpp (oracle/Makefile circuit64)",
                   "cases": {"logdemo": {"prime": "goldilocks", "vectors": vectors}}}, f, indent=1)
    print("wrote", path, len(vectors), "vectors")


if __name__ == "__main__":
    main()
