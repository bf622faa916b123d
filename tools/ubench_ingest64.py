#!/usr/bin/env python3
"""Bulk ingest of the 64-bit runtime timed on a chain circuit over Goldilocks x 65 536, n inputs each:

      x[n] inputs;  s[0] <== x[0];  s[k] <== s[k-1] * x[k] + x[k];  out <== s[n-1]

  (a) 32-byte image, CW64_INGEST_TILED=0: cw64_ingest_kernel<32> (lane = instance, one grid row per input)
  (b) 32-byte image, CW64_INGEST_TILED=1: cw64_transpose_in_kernel<32, false> (tiled transpose through LDS)
  (c) 8-byte image,  CW64_INGEST_TILED=1: cw64_transpose_in_kernel<8, false>
  (d) 8-byte image,  CW64_INGEST_TILED=0: cw64_ingest_kernel<8>
  (e) 32-byte image, CW64_INGEST_TILED unset: the kernel the library picks by itself (CW64_INGEST_TILE_MIN)
  (f) 8-byte image,  CW64_INGEST_TILED unset

Every variant is a batch of its own reading the same device image (cw_set_inputs_device / _n8).  Timing: cw_batch_set_timing +
cw_batch_kernel_ms, element ms[0] = table init + ingest of one cw_run (HIP events on the batch's stream; the init kernel is
the same in every variant).  --warmup runs, then --runs timed ones, the variants taking turns run by run; median (min .. max).
Figures per variant and n: ms, bytes read (the image), bytes written (the input rows of the table), (read + written) per
second, that rate against the 8 TB/s HBM specification.  Parity: every variant must leave the same input slots and the same
`out` (read back with cw_get_witnesses_device_n8), and a seeded sample of instances must equal the chain's closed form.
(e) and (f) make the rule behind CW64_INGEST_TILE_MIN checkable from the result: at every n, (e) must not be slower than (a)
beyond the min .. max spread of (a).

  python tools/ubench_ingest64.py --workdir DIR --compile-only                     # without a GPU: lower the circuits
  python tools/ubench_ingest64.py --workdir DIR --out ingest64_chain_65536.json
"""
import argparse
import json
import os
import random
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

from ubench_egress64 import HBM_SPEC, Hip                                            # noqa: E402

Q = 0xFFFFFFFF00000001
VARIANTS = (("a_lane_32", 32, "0"), ("b_tiled_32", 32, "1"), ("c_tiled_8", 8, "1"), ("d_lane_8", 8, "0"), ("e_auto_32", 32, None),
            ("f_auto_8", 8, None))


def chain_program(n):
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

    return Program(Chain(n), prime="goldilocks")


def compile_chain(workdir, n):
    from circom_amd import compiler
    name = "chain%d" % n
    d = Path(workdir) / name
    d.mkdir(parents=True, exist_ok=True)
    paths = [d / (name + ext) for ext in (".cwt", ".dat", ".r1cs")]
    if not all(p.exists() for p in paths):
        cp = compiler.compile_program(chain_program(n), str(d), name, sym=False)
        paths = [Path(cp.tape_path), Path(cp.dat_path), Path(cp.r1cs_path)]
    return paths


def closed_form(row):
    """[1, out, x mod p ...] of one instance in Python integers"""
    x = [int(v) % Q for v in row]
    s = x[0]
    for v in x[1:]:
        s = (s * v + v) % Q
    return [1, s] + x


def figures(ms, n_read, n_written):
    med = statistics.median(ms)
    rate = (n_read + n_written) / (med * 1e-3)
    return {"ms_median": round(med, 5), "ms_min": round(min(ms), 5), "ms_max": round(max(ms), 5), "runs": len(ms), "bytes_read": n_read,
            "bytes_written": n_written, "bytes_per_s": round(rate), "fraction_of_hbm_spec": round(rate / HBM_SPEC, 4)}


def measure(rt, hip, stream, paths, n, B, runs, warmup, sample):
    circ = rt.Circuit(*[str(p) for p in paths])
    assert circ.element_bytes == 8 and circ.n_inputs == n and circ.input_start == 2
    circ.set_witness_list(np.arange(2 + n, dtype=np.uint32))         # the constant, out, the inputs: what the variants must agree on
    x = np.random.default_rng(n).integers(0, 1 << 64, size=(B, n), dtype=np.uint64, endpoint=False)   # a few values are >= p
    img32 = np.zeros((B, n, 4), dtype="<u8")
    img32[:, :, 0] = x
    d = {8: hip.alloc(x.nbytes), 32: hip.alloc(img32.nbytes)}
    hip.ok(hip.h.hipMemcpy(d[8], x.ctypes.data, x.nbytes, 1))
    hip.ok(hip.h.hipMemcpy(d[32], img32.ctypes.data, img32.nbytes, 1))
    del img32
    batches = {}
    for name, eb, tiled in VARIANTS:
        os.environ.pop("CW64_INGEST_TILED", None)                     # read at batch creation
        if tiled is not None:
            os.environ["CW64_INGEST_TILED"] = tiled
        b = circ.batch(B, stream=stream)
        (b.set_inputs_device_n8 if eb == 8 else b.set_inputs_device)(d[eb])
        b.set_timing(True)
        batches[name] = b
    os.environ.pop("CW64_INGEST_TILED", None)
    ms = {name: [] for name in batches}
    for r in range(warmup + runs):
        for name, b in batches.items():
            b.run(); b.sync()
            if r >= warmup:
                ms[name].append(b.kernel_ms()["ingest"])
    out = {name: figures(ms[name], B * n * eb, B * n * 8) for name, eb, _ in VARIANTS}
    # parity: the same input slots and `out` everywhere, the closed form on a seeded sample
    dw = hip.alloc(B * (2 + n) * 8)
    first = None
    for name, b in batches.items():
        assert (b.status() == 0).all(), name
        b.witnesses_device_n8(0, B, dw)
        b.sync()
        got = hip.download(dw, B * (2 + n) * 8).view("<u8").reshape(B, 2 + n)
        if first is None:
            first = got
            for i in random.Random(n).sample(range(B), sample):
                assert [int(v) for v in got[i]] == closed_form(x[i]), (name, n, i)
        else:
            assert np.array_equal(first, got), "%s disagrees with %s at n = %d" % (name, VARIANTS[0][0], n)
        b.close()
    hip.h.hipFree(dw)
    for p in d.values():
        hip.h.hipFree(p)
    circ.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--n", type=int, nargs="+", default=[2, 16, 64, 1024])
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sample", type=int, default=16, help="instances per n compared with the closed form")
    ap.add_argument("--workdir", default=None, help="where the lowered circuits are kept (default: a temporary directory)")
    ap.add_argument("--compile-only", action="store_true")
    ap.add_argument("--box", default=None, help="name of the device, recorded in the result (default: what the HIP runtime calls device 0)")
    ap.add_argument("--out", default=None, help="write the JSON result here as well")
    args = ap.parse_args()
    assert args.runs >= 20, "at least 20 timed runs per variant"
    if args.workdir is None:
        import tempfile
        args.workdir = tempfile.mkdtemp(prefix="ingest64_")
    paths = {n: compile_chain(args.workdir, n) for n in args.n}
    if args.compile_only:
        return
    from circom_amd import runtime as rt
    hip = Hip()
    stream = hip.stream()
    if args.box is None:
        import ctypes as C
        name = C.create_string_buffer(256)
        hip.ok(hip.h.hipDeviceGetName(name, 256, 0))
        args.box = name.value.decode() or "HIP device 0 (the runtime reports no name: pass --box)"
    res = {"tool": "tools/ubench_ingest64.py", "box": args.box, "batch": args.batch, "warmup": args.warmup,
           "timing": "cw_batch_kernel_ms element 0 (table init + ingest) of every cw_run, variants taking turns; median / min / max",
           "bytes": "read = the input image, written = the input rows of the value table (the init kernel's 16 bytes per instance are not counted)",
           "hbm_spec_bytes_per_s": HBM_SPEC, "n": {}}
    for n in args.n:
        res["n"][str(n)] = measure(rt, hip, stream, paths[n], n, args.batch, args.runs, args.warmup, args.sample)
        for name, f in res["n"][str(n)].items():
            print(n, name, json.dumps(f), flush=True)
    res["variants_agree"] = True                                      # measure() asserts it
    print(json.dumps(res))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
