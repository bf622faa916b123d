#!/usr/bin/env python3
"""R1CS products out (cw_get_r1cs_products_device) timed on one workload per run.  In the SAME run, the variants taking turns round
by round, HIP events on the batch's stream around each:

  (a) products_ab      parts A | B of the row range for every instance
  (b) products_abc     parts A | B | C
  (c) memcpy_dtod_ab / memcpy_dtod_abc   hipMemcpyDtoD (async, the same stream) of the same number of bytes

and, beside them, the yardstick from code this tool does not touch: ms[2] of cw_batch_kernel_ms after cw_check_r1cs on the same
batch with the stand-alone check forced (CW_FP_FUSED=0; CW_R1CS_AUDIT=1 for the emitted bit engine) - it forms the same sums over
the WHOLE system and writes nothing.  The expectation to report against is "about the check's time (scaled to the row range) plus
the copy's".

Workloads:
  poseidon2_bn128 / poseidon2_goldilocks   Poseidon(2) x 65 536, the whole system (1 105 rows)
  sha256_2048                              the metric's circuit x 2 097 152 on the emitted bit engine, rows [--row0, --row0 + --rows):
                                           the whole system (1 020 832 rows) would be 196 TB; 128 rows are 17 / 26 GB.  The circuit
                                           comes from the artefact cache build() leaves in the tree (bench.get_compiled)

--warmup rounds, then --runs timed ones; median (min .. max), bytes written per second.  Parity: A o B = C at every row of a few
instances, computed from the image on Python integers.

  python tools/ubench_r1cs_products.py --workload poseidon2_bn128 --out profiles/r1cs_products_poseidon2_bn128.json
"""
import argparse
import glob
import json
import os
import statistics
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

HBM_SPEC = 8.0e12


def figures(ms, n_written):
    med = statistics.median(ms)
    rate = n_written / (med * 1e-3)
    return {"ms_median": round(med, 5), "ms_min": round(min(ms), 5), "ms_max": round(max(ms), 5), "runs": len(ms), "bytes_written": n_written,
            "bytes_written_per_s": round(rate), "fraction_of_hbm_spec": round(rate / HBM_SPEC, 4)}


def timed(stream, ev, fn):
    ev[0].record(stream)
    fn()
    ev[1].record(stream)
    stream.synchronize()
    return ev[0].elapsed_time(ev[1])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workload", choices=("poseidon2_bn128", "poseidon2_goldilocks", "sha256_2048"), required=True)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=None, help="instances (default: 65 536, sha256_2048: the metric's 2 097 152)")
    ap.add_argument("--row0", type=int, default=4096, help="sha256_2048: first row of the range")
    ap.add_argument("--rows", type=int, default=128, help="sha256_2048: rows of the range")
    ap.add_argument("--cache-dir", default=None)
    ap.add_argument("--out", default=None, help="write the JSON result here as well")
    args = ap.parse_args()
    assert args.runs >= 20, "at least 20 timed runs per variant"
    os.environ["CW_FP_FUSED"] = "0"                     # the stand-alone check is the yardstick
    os.environ["CW_R1CS_AUDIT"] = "1"
    import torch
    from circom_amd import runtime as rt
    from circom_amd.compiler import compile_program
    from circom_amd.frontend.dsl import Program
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    if args.workload == "sha256_2048":
        import bench
        in_tree = glob.glob(str(ROOT / "*" / "cache" / ("sha256_2048_s*_%s" % bench.artefact_fingerprint())))
        cache_root = args.cache_dir or (os.path.dirname(in_tree[0]) if in_tree
                                        else os.path.join(tempfile.gettempdir(), "cw_bench_cache_%d" % os.getuid()))
        B = args.batch or bench.DEFAULT_BATCH["sha256_2048"]
        cp, _, _ = bench.get_compiled("sha256_2048", B, cache_root, 0, None, flat=False)
        circ = rt.Circuit(cp.tape_path, cp.dat_path, cp.r1cs_path)
        row0, n_rows = args.row0, args.rows
        d_msgs = torch.randint(0, 256, (B, circ.n_inputs // 8), dtype=torch.uint8, device=dev, generator=gen)
        b = circ.batch(B, stream=stream.cuda_stream)
        assert b.bitmode
        b.set_inputs_rows_device(d_msgs.data_ptr(), circ.n_inputs // 8, msb_first=True)
        engine = "bit-plane, emitted" if b.jit else "bit-plane, interpreter"
    else:
        from circom_amd.circuits.poseidon import Poseidon
        gl = args.workload.endswith("goldilocks")
        d = tempfile.mkdtemp(prefix="cw_ubench_products_")
        cp = compile_program(Program(Poseidon(2), prime="goldilocks") if gl else Program(Poseidon(2)), d, "poseidon2", sym=False)
        circ = rt.Circuit(cp.tape_path, cp.dat_path, cp.r1cs_path)
        B = args.batch or 65536
        row0, n_rows = 0, circ.n_constraints
        rng = np.random.default_rng(1)
        image = np.zeros((B, circ.n_inputs, 4), dtype="<u8")
        image[:, :, 0] = rng.integers(0, 1 << 62, size=(B, circ.n_inputs), dtype=np.uint64)
        b = circ.batch(B, stream=stream.cuda_stream)
        b.set_inputs(image.view(np.uint8).reshape(B, circ.n_inputs, 32))
        engine = "64-bit runtime" if gl else "256-bit schedule, %s table" % ("Montgomery-form" if circ.montgomery else "canonical")
    eb, q = circ.element_bytes, circ.q
    b.set_timing(True)
    b.run(); b.check_r1cs(); b.sync()
    assert (b.status() == 0).all()
    checks = [b.kernel_ms()["check"]]
    for _ in range(8):                                  # the same check again on the same table: the median of nine
        b.check_r1cs(); b.sync()
        checks.append(b.kernel_ms()["check"])
    assert (b.status() == 0).all()
    check_ms = statistics.median(checks)
    nbytes = {2: B * 2 * n_rows * eb, 3: B * 3 * n_rows * eb}
    d_out = torch.full((nbytes[3],), 0xA5, dtype=torch.uint8, device=dev)
    d_copy = torch.empty_like(d_out)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    sample = [0, 1, B // 2 + 63, B - 1]
    ms = {"a_products_ab": [], "b_products_abc": [], "c_memcpy_dtod_ab": [], "c_memcpy_dtod_abc": []}
    with torch.cuda.stream(stream):
        for r in range(args.warmup + args.runs):
            ta = timed(stream, ev, lambda: b.r1cs_products_device(3, row0, n_rows, 0, B, d_out.data_ptr()))
            tca = timed(stream, ev, lambda: d_copy[:nbytes[2]].copy_(d_out[:nbytes[2]], non_blocking=True))
            tb = timed(stream, ev, lambda: b.r1cs_products_device(7, row0, n_rows, 0, B, d_out.data_ptr()))
            tcb = timed(stream, ev, lambda: d_copy.copy_(d_out, non_blocking=True))
            if r == 0:
                img = d_out.view(B, 3, n_rows, eb)
                for i in sample:                                     # a clean instance: A o B = C at every row
                    v = img[i].cpu().numpy().view("<u8").astype(object)
                    v = sum(v[..., k] << (64 * k) for k in range(v.shape[-1]))
                    assert not ((v[0] * v[1] - v[2]) % q).any(), i
            if r >= args.warmup:
                ms["a_products_ab"].append(ta); ms["b_products_abc"].append(tb)
                ms["c_memcpy_dtod_ab"].append(tca); ms["c_memcpy_dtod_abc"].append(tcb)
    assert torch.equal(d_copy, d_out)
    res = {"tool": "tools/ubench_r1cs_products.py", "box": torch.cuda.get_device_name(0), "workload": args.workload, "batch": B,
           "engine": engine, "element_bytes": eb, "constraints": circ.n_constraints, "row0": row0, "n_rows": n_rows, "warmup": args.warmup,
           "timing": "HIP events on the batch's stream around each call, the variants taking turns round by round; median / min / max",
           "hbm_spec_bytes_per_s": HBM_SPEC,
           "check_r1cs_ms": round(float(check_ms), 5),
           "check_r1cs": "cw_batch_kernel_ms ms[2], median of nine stand-alone cw_check_r1cs over ALL %d rows (CW_FP_FUSED=0, CW_R1CS_AUDIT=1)" % circ.n_constraints,
           "check_r1cs_ms_scaled_to_the_range": round(float(check_ms) * n_rows / circ.n_constraints, 5),
           "variants": {"a_products_ab": figures(ms["a_products_ab"], nbytes[2]), "b_products_abc": figures(ms["b_products_abc"], nbytes[3]),
                        "c_memcpy_dtod_ab": figures(ms["c_memcpy_dtod_ab"], nbytes[2]),
                        "c_memcpy_dtod_abc": figures(ms["c_memcpy_dtod_abc"], nbytes[3])},
           "parity": "A o B = C at every row of the range in the instances %s, on Python integers from the image" % sample}
    for tag, parts in (("ab", "a_products_ab"), ("abc", "b_products_abc")):
        yard = res["check_r1cs_ms_scaled_to_the_range"] + res["variants"]["c_memcpy_dtod_" + tag]["ms_median"]
        res["variants"][parts]["over_check_plus_copy"] = round(res["variants"][parts]["ms_median"] / yard, 3)
    for name, f in res["variants"].items():
        print(name, json.dumps(f), flush=True)
    print(json.dumps(res))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
    b.close(); circ.close()


if __name__ == "__main__":
    main()
