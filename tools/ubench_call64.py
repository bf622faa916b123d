#!/usr/bin/env python3
"""Run-time functions of the 64-bit runtime (csrc/cw64.hip cw64_call): the register window in the value table against the register
window in LDS, on two circuits over Goldilocks:

  longdiv   shift-subtract long division, 10 registers, two loops of 1 .. 62 trips per lane (divergent lanes take turns)
  fill      an array of --fill-n entries filled by a run-time loop and read through a run-time index: --fill-n + 6 registers
            (112, the default: 118 registers, near the 128 the LDS placement takes; 26 and 58 give 32 and 64)

  (a) CW64_CALL_LDS=0: registers are V[base + r][instance]
  (b) CW64_CALL_LDS=1: registers are win[r * 64 + lane] in LDS, copied in at the call and back at its end

Every variant is a batch of its own reading the same device image.  Timing: cw_batch_set_timing + cw_batch_kernel_ms, element
ms[1] = the evaluation kernel of one cw_run (HIP events on the batch's stream).  --warmup runs, then --runs timed ones, the
variants taking turns run by run; median (min .. max).  Parity: both variants must leave the same witnesses (read back with
cw_get_witnesses_device_n8), and a seeded sample of instances must equal the plain-integer model.

  python tools/ubench_call64.py --workdir DIR --compile-only                     # without a GPU: lower the circuits
  python tools/ubench_call64.py --workdir DIR --out call64_mi355x.json
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

from ubench_egress64 import Hip                                                      # noqa: E402

Q = 0xFFFFFFFF00000001
VARIANTS = (("a_table", "0"), ("b_lds", "1"))


def longdiv_program():
    from circom_amd.frontend.dsl import Program, template

    def build(f, a, b):
        q, r, sh, d = f.var(0), f.var(a), f.var(0), f.var(b)
        with f.loop() as L:
            L.break_unless((d << 1).leq(r))
            d.set(d << 1)
            sh.set(sh + 1)
        with f.loop() as L:
            with f.if_(r.geq(d)):
                r.set(r - d)
                q.set(q + (f.lift(1) << sh))
            L.break_unless(sh.neq(0))
            d.set(d >> 1)
            sh.set(sh - 1)
        return [q, r]

    @template
    def LongDiv(c):
        a, b = c.input("a"), c.input("b")
        qo, ro = c.output("q"), c.output("r")
        q, r = c.call(c.function("divmod", 2, build), [a, b])
        c.hint(qo, q)
        c.hint(ro, r)
        c.enforce(qo * b + ro, a)

    return Program(LongDiv(), prime="goldilocks")


def fill_program(n):
    from circom_amd.frontend.dsl import Program, template

    def build(f, m, sel):
        arr = f.array(n)
        i = f.var(0)
        with f.loop() as L:
            L.break_unless(i.lt(n))
            arr.store(i, i * m + 1)
            i.set(i + 1)
        return [arr.load(sel)]

    @template
    def Fill(c):
        m, sel = c.input("m"), c.input("sel")
        out = c.output("out")
        (v,) = c.call(c.function("fill", 2, build), [m, sel])
        c.hint(out, v)

    return Program(Fill(), prime="goldilocks")


def inputs_and_model(name, B, fill_n):
    rnd = random.Random(B)
    if name == "longdiv":                                             # a < 2^62: the relational operators are signed around q / 2
        rows = [[rnd.randrange(1 << rnd.randrange(1, 63)), rnd.randrange(1, 1 << rnd.randrange(1, 32))] for _ in range(B)]
        return rows, lambda r: [1, r[0] // r[1], r[0] % r[1], r[0], r[1]]
    rows = [[rnd.randrange(Q), rnd.randrange(fill_n)] for _ in range(B)]
    return rows, lambda r: [1, (r[1] * r[0] + 1) % Q, r[0], r[1]]


def compile_circuit(workdir, name, prog):
    from circom_amd import compiler
    d = Path(workdir) / name
    d.mkdir(parents=True, exist_ok=True)
    paths = [d / (name + ext) for ext in (".cwt", ".dat", ".r1cs")]
    if not all(p.exists() for p in paths):
        cp = compiler.compile_program(prog, str(d), name, sym=False)
        paths = [Path(cp.tape_path), Path(cp.dat_path), Path(cp.r1cs_path)]
    return paths


def measure(rt, hip, stream, paths, name, B, runs, warmup, sample, fill_n):
    circ = rt.Circuit(*[str(p) for p in paths])
    rows, model = inputs_and_model(name, B, fill_n)
    x = np.asarray(rows, dtype=np.uint64)
    d_in = hip.alloc(x.nbytes)
    hip.ok(hip.h.hipMemcpy(d_in, x.ctypes.data, x.nbytes, 1))
    batches = {}
    for vname, lds in VARIANTS:
        os.environ["CW64_CALL_LDS"] = lds                             # read at batch creation
        b = circ.batch(B, stream=stream)
        assert (b.call_lds != 0) == (lds == "1"), "the circuit's functions do not fit the LDS placement"
        b.set_inputs_device_n8(d_in)
        b.set_timing(True)
        batches[vname] = b
    os.environ.pop("CW64_CALL_LDS", None)
    ms = {vname: [] for vname in batches}
    for r in range(warmup + runs):
        for vname, b in batches.items():
            b.run(); b.sync()
            if r >= warmup:
                ms[vname].append(b.kernel_ms()["eval"])
    out = {}
    dw = hip.alloc(B * circ.n_witness * 8)
    first = None
    for vname, b in batches.items():
        assert (b.status() == 0).all(), vname
        b.witnesses_device_n8(0, B, dw)
        b.sync()
        got = hip.download(dw, B * circ.n_witness * 8).view("<u8").reshape(B, circ.n_witness)
        if first is None:
            first = got
            for i in random.Random(B + 1).sample(range(B), min(sample, B)):
                assert [int(v) for v in got[i]] == model(rows[i]), (name, vname, i)
        else:
            assert np.array_equal(first, got), "%s disagrees with %s on %s" % (vname, VARIANTS[0][0], name)
        med = statistics.median(ms[vname])
        out[vname] = {"ms_median": round(med, 5), "ms_min": round(min(ms[vname]), 5), "ms_max": round(max(ms[vname]), 5), "runs": len(ms[vname]),
                      "lds_bytes_per_workgroup": b.call_lds}
        b.close()
    hip.h.hipFree(dw)
    hip.h.hipFree(d_in)
    circ.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, nargs="+", default=[1024, 65536])
    ap.add_argument("--fill-n", type=int, default=112)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sample", type=int, default=64, help="instances per circuit and batch compared with the plain-integer model")
    ap.add_argument("--workdir", default=None, help="where the lowered circuits are kept (default: a temporary directory)")
    ap.add_argument("--compile-only", action="store_true")
    ap.add_argument("--box", default=None, help="name of the device, recorded in the result (default: what the HIP runtime calls device 0)")
    ap.add_argument("--out", default=None, help="write the JSON result here as well")
    args = ap.parse_args()
    assert args.runs >= 20, "at least 20 timed runs per variant"
    if args.workdir is None:
        import tempfile
        args.workdir = tempfile.mkdtemp(prefix="call64_")
    progs = {"longdiv": longdiv_program(), "fill": fill_program(args.fill_n)}
    paths = {name: compile_circuit(args.workdir, name if name == "longdiv" else "fill%d" % args.fill_n, p) for name, p in progs.items()}
    regs = {name: p.functions[0].n_regs for name, p in progs.items()}
    if args.compile_only:
        print(json.dumps({"registers": regs}))
        return
    from circom_amd import runtime as rt
    hip = Hip()
    stream = hip.stream()
    if args.box is None:
        import ctypes as C
        dev = C.create_string_buffer(256)
        hip.ok(hip.h.hipDeviceGetName(dev, 256, 0))
        args.box = dev.value.decode() or "HIP device 0 (the runtime reports no name: pass --box)"
    res = {"tool": "tools/ubench_call64.py", "box": args.box, "warmup": args.warmup, "registers": regs,
           "timing": "cw_batch_kernel_ms element 1 (the evaluation kernel) of every cw_run, variants taking turns; median / min / max",
           "circuits": {}}
    for name in progs:
        res["circuits"][name] = {}
        for B in args.batch:
            res["circuits"][name][str(B)] = measure(rt, hip, stream, paths[name], name, B, args.runs, args.warmup, args.sample, args.fill_n)
            for vname, f in res["circuits"][name][str(B)].items():
                print(name, B, vname, json.dumps(f), flush=True)
    res["variants_agree"] = True                                      # measure() asserts it
    print(json.dumps(res))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
