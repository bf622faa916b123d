#!/usr/bin/env python3
"""Input columns (cw_set_inputs_range_device) timed on the chain circuit of tools/ubench_ingest64.py, on Goldilocks (the batch's
image holds 8-byte values) and on bn128 (32-byte values), x 65 536 instances, n inputs each, n = 1, 64, 1 024:

      x[n] inputs;  s[0] <== x[0];  s[k] <== s[k-1] * x[k] + x[k];  out <== s[n-1]

One column covers all n inputs from a dense device array [batch][n][W], W = 1, 2, 4, 8, 32 bytes (stride n * W).  In the SAME
rounds, the variants taking turns round by round:

  col_W     csrc/cw_columns.hip.h cw_columns_kernel<W, EB>: HIP events on the batch's stream around the call
  copy2d    where W equals the image's element (8 on Goldilocks, 32 on bn128): hipMemcpy2DAsync, device to device, of the same
            rectangle (width n * W bytes, height = batch, the same pitches), the same stream, the same events
  ingest    cw_batch_kernel_ms element 0 (table init + input ingest) of a cw_run of the same batch over the image the columns wrote

--warmup rounds, then --runs timed ones; median (min .. max); beside every form the bytes read + written per second.  Parity:
in the first round a run follows every width, and a seeded sample of instances must equal the chain's closed form on that
width's values.  32-byte values: canonical (< 2^253) on bn128; on Goldilocks 8-byte values zero-extended, what a caller of the
32-byte boundary holds (the kernel's long reduction is a per-lane branch that such values do not take).

  python tools/ubench_columns.py --workdir DIR --compile-only                     # without a GPU: lower the circuits
  python tools/ubench_columns.py --workdir DIR --out profiles/columns_chain_65536.json
"""
import argparse
import ctypes as C
import json
import random
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

from ubench_egress64 import HBM_SPEC, Hip                                            # noqa: E402

WIDTHS = (1, 2, 4, 8, 32)


def chain_program(n, prime):
    from circom_amd.frontend.dsl import Program, template

    @template
    def Chain(c, n):
        x = c.input("x", n)
        out = c.output("out")
        s = c.signal("s", n)
        c.set(s[0], x[0] + 0)
        for k in range(1, n):
            c.set(s[k], s[k - 1] * x[k] + x[k])
        c.set(out, s[n - 1] + 0)

    return Program(Chain(n), prime=prime) if prime != "bn128" else Program(Chain(n))


def compile_chain(workdir, n, prime):
    from circom_amd import compiler
    name = "chain%d_%s" % (n, prime)
    d = Path(workdir) / name
    d.mkdir(parents=True, exist_ok=True)
    paths = [d / (name + ext) for ext in (".cwt", ".dat", ".r1cs")]
    if not all(p.exists() for p in paths):
        cp = compiler.compile_program(chain_program(n, prime), str(d), name, sym=False)
        paths = [Path(cp.tape_path), Path(cp.dat_path), Path(cp.r1cs_path)]
    return paths


def closed_form(q, row):
    """[1, out, x mod q ...] of one instance in Python integers"""
    x = [int(v) % q for v in row]
    s = x[0]
    for v in x[1:]:
        s = (s * v + v) % q
    return [1, s] + x


def figures(ms, n_read, n_written):
    med = statistics.median(ms)
    rate = (n_read + n_written) / (med * 1e-3)
    return {"ms_median": round(med, 5), "ms_min": round(min(ms), 5), "ms_max": round(max(ms), 5), "runs": len(ms), "bytes_read": n_read,
            "bytes_written": n_written, "bytes_per_s": round(rate), "fraction_of_hbm_spec": round(rate / HBM_SPEC, 4)}


def values(prime, n, B, W):
    """[B][n][W] bytes"""
    rng = np.random.default_rng(1000 * n + W)
    if W < 32:
        return rng.integers(0, 256, size=(B, n, W), dtype=np.uint8)
    v = np.zeros((B, n, 32), dtype=np.uint8)
    if prime == "bn128":
        v[:] = rng.integers(0, 256, size=(B, n, 32), dtype=np.uint8)
        v[:, :, 31] &= 0x1F
    else:
        v[:, :, :8] = rng.integers(0, 256, size=(B, n, 8), dtype=np.uint8)
    return v


def measure(rt, hip, stream, paths, prime, n, B, runs, warmup, sample):
    circ = rt.Circuit(*[str(p) for p in paths])
    eb = circ.element_bytes
    assert eb == (8 if prime == "goldilocks" else 32) and circ.n_inputs == n and circ.input_start == 2
    circ.set_witness_list(np.arange(2 + n, dtype=np.uint32))         # the constant, out, the inputs
    host, dev = {}, {}
    for W in WIDTHS:
        host[W] = values(prime, n, B, W)
        dev[W] = hip.alloc(host[W].nbytes)
        hip.ok(hip.h.hipMemcpy(dev[W], host[W].ctypes.data, host[W].nbytes, 1))
    d_copy = hip.alloc(B * n * eb)
    b = circ.batch(B, stream=stream)
    b.set_timing(True)
    hip.h.hipMemcpy2DAsync.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p]
    names = ["col_%d" % W for W in WIDTHS] + ["copy2d_%d" % eb]
    ev = {k: (hip.event(), hip.event()) for k in names}
    ms = {k: [] for k in names + ["ingest"]}
    for r in range(warmup + runs):
        for W in WIDTHS:
            e0, e1 = ev["col_%d" % W]
            hip.ok(hip.h.hipEventRecord(e0, stream))
            b.set_inputs_range_device(0, dev[W], n, n * W, W)
            hip.ok(hip.h.hipEventRecord(e1, stream))
            if r == 0:                                                # parity: this width's values reach the witness
                b.run(); b.sync()
                assert (b.status() == 0).all()
                for i in sample:
                    want = closed_form(circ.q, [int.from_bytes(host[W][i, k].tobytes(), "little") for k in range(n)])
                    assert b.witness(i) == want, (prime, n, W, i)
        e0, e1 = ev["copy2d_%d" % eb]
        hip.ok(hip.h.hipEventRecord(e0, stream))
        hip.ok(hip.h.hipMemcpy2DAsync(d_copy, n * eb, dev[eb], n * eb, n * eb, B, 3, stream))
        hip.ok(hip.h.hipEventRecord(e1, stream))
        b.run(); b.sync()
        t_ingest = b.kernel_ms()["ingest"]
        if r >= warmup:
            for k in names:
                t = C.c_float()
                hip.ok(hip.h.hipEventElapsedTime(C.byref(t), ev[k][0], ev[k][1]))
                ms[k].append(t.value)
            ms["ingest"].append(t_ingest)
    assert (hip.download(d_copy, B * n * eb) == host[eb].reshape(-1)).all()
    out = {"col_%d" % W: figures(ms["col_%d" % W], B * n * W, B * n * eb) for W in WIDTHS}
    out["copy2d_%d" % eb] = figures(ms["copy2d_%d" % eb], B * n * eb, B * n * eb)
    out["ingest"] = figures(ms["ingest"], B * n * eb, B * n * eb)
    same = out["col_%d" % eb]["ms_median"] / out["copy2d_%d" % eb]["ms_median"]
    out["col_over_copy2d"] = round(same, 3)
    b.close(); circ.close()
    for p in list(dev.values()) + [d_copy]:
        hip.h.hipFree(p)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workdir", required=True)
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--n", default="1,64,1024")
    ap.add_argument("--primes", default="goldilocks,bn128")
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--compile-only", action="store_true")
    ap.add_argument("--out", default=None, help="write the JSON result here as well")
    args = ap.parse_args()
    ns = [int(x) for x in args.n.split(",")]
    primes = args.primes.split(",")
    paths = {(p, n): compile_chain(args.workdir, n, p) for p in primes for n in ns}
    if args.compile_only:
        return
    assert args.runs >= 20, "at least 20 timed runs per variant"
    from circom_amd import runtime as rt
    hip = Hip()
    stream = hip.stream()
    sample = sorted(random.Random(5).sample(range(args.batch), 6) + [0, args.batch - 1])
    res = {"tool": "tools/ubench_columns.py", "batch": args.batch, "warmup": args.warmup,
           "timing": "HIP events on the batch's stream around cw_set_inputs_range_device / hipMemcpy2DAsync; cw_batch_kernel_ms element 0 "
                     "= table init + ingest of the cw_run behind them; the variants taking turns round by round; median / min / max",
           "hbm_spec_bytes_per_s": HBM_SPEC, "shapes": {}}
    for p in primes:
        for n in ns:
            f = measure(rt, hip, stream, paths[p, n], p, n, args.batch, args.runs, args.warmup, sample)
            res["shapes"]["%s_n%d" % (p, n)] = f
            print(p, n, json.dumps(f), flush=True)
    res["parity"] = "after every width's column in the first round: status words 0 and the closed form at instances %s" % sample
    print(json.dumps(res))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
