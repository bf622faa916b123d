#!/usr/bin/env python3
"""Witness compare (cw_compare_witnesses_device(_n8)) timed beside the egress it mirrors, in ONE process, the variants taking
turns round by round, HIP events on the batch's stream around each call; --warmup rounds, then --runs timed ones; median
(min .. max).

  (a) compare_equal       the compare of an image that equals the batch's witnesses: the fill of the verdict words, the table read,
                          the image read, no global atomic
  (b) compare_different   the compare of an image that differs in EVERY element (byte 0 of each flipped): the worst case of the
                          reduction - every lane finds a mismatch, every workgroup reports every instance
  (c) egress              cw_get_witnesses_device(_n8) of the same range into a second buffer: the same bytes the other way
  (d) digest              sha256_2048 only: cw_get_wtns_digests_device of the same instances
The figure to judge the kernels by is (a) / (c).  The verdicts of (a) and (b) are checked in the same run.

  --workload poseidon2_bn128        Poseidon(2) x 65 536, Montgomery-form table, 32-byte elements
  --workload poseidon2_goldilocks   Poseidon(2) x 65 536 on the 64-bit runtime, 8- and 32-byte elements
  --workload sha256_2048            the --O1 witness (cw_set_witness_list) of --range (8 192) instances of the metric's circuit on
                                    the emitted bit engine, inside a batch of 2 097 152; the artefact cache build() leaves in the
                                    tree is needed (the workload is skipped with a message otherwise)
  --workload all                    the three, one after the other (the default)

  python tools/ubench_compare.py --out profiles/compare_mi355x.json
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

NONE = 0xFFFFFFFF


def figures(ms, nbytes):
    med = statistics.median(ms)
    return {"ms_median": round(med, 5), "ms_min": round(min(ms), 5), "ms_max": round(max(ms), 5), "runs": len(ms),
            "image_bytes": nbytes, "image_bytes_per_s": round(nbytes / (med * 1e-3))}


def timed(stream, ev, fn):
    ev[0].record(stream)
    fn()
    ev[1].record(stream)
    stream.synchronize()
    return ev[0].elapsed_time(ev[1])


def measure(args, torch, stream, ev, b, circ, first, count, eb, digest):
    """the variants for the instances [first, first + count) of a batch that has run, elements of eb bytes"""
    dev = torch.device("cuda:0")
    nw = circ.n_witness
    row = nw * eb
    n8 = eb != 32
    d_img = torch.empty((count, nw, eb), dtype=torch.uint8, device=dev)
    d_out = torch.empty((count, nw, eb), dtype=torch.uint8, device=dev)
    d_diff = torch.zeros(count, dtype=torch.int32, device=dev)
    d_sum = torch.zeros(2, dtype=torch.int32, device=dev)
    d_dig = torch.empty((count, 32), dtype=torch.uint8, device=dev) if digest else None
    torch.cuda.synchronize()
    egress_to = lambda t: (b.witnesses_device_n8 if n8 else b.witnesses_device)(first, count, t.data_ptr())
    compare = lambda: b.compare_witnesses_device(d_img.data_ptr(), d_diff.data_ptr(), first, count, 0, nw, d_summary=d_sum.data_ptr(), n8=n8)
    flip = lambda: d_img[:, :, 0].bitwise_xor_(1)                      # byte 0 of every element
    ms = {"a_compare_equal": [], "b_compare_different": [], "c_egress": []}
    if digest:
        ms["d_digest"] = []
    with torch.cuda.stream(stream):
        egress_to(d_img)
        stream.synchronize()
        for r in range(args.warmup + args.runs):
            ta = timed(stream, ev, compare)
            if r == 0:
                assert bool((d_diff == -1).all()) and d_sum.tolist() == [0, -1], "an equal image was not found equal"
            flip()
            tb = timed(stream, ev, compare)
            if r == 0:
                assert bool((d_diff == 0).all()) and (d_sum.to(torch.int64) & NONE).tolist() == [count, first], "the all-different image"
            flip()
            tc = timed(stream, ev, lambda: egress_to(d_out))
            td = timed(stream, ev, lambda: b.wtns_digests_device(first, count, d_dig.data_ptr())) if digest else None
            if r >= args.warmup:
                ms["a_compare_equal"].append(ta); ms["b_compare_different"].append(tb); ms["c_egress"].append(tc)
                if digest:
                    ms["d_digest"].append(td)
        assert torch.equal(d_img, d_out), "the image and the egress of the same range differ"
    nbytes = count * row
    out = {"first": first, "instances": count, "n_witness": nw, "element_bytes": eb, "variants": {k: figures(v, nbytes) for k, v in ms.items()}}
    med = lambda k: out["variants"][k]["ms_median"]
    out["compare_equal_over_egress"] = round(med("a_compare_equal") / med("c_egress"), 4)
    out["compare_different_over_equal"] = round(med("b_compare_different") / med("a_compare_equal"), 4)
    if digest:
        out["digest_over_compare_equal"] = round(med("d_digest") / med("a_compare_equal"), 2)
    del d_img, d_out
    torch.cuda.empty_cache()
    return out


def poseidon(args, torch, stream, ev, gl):
    from circom_amd import runtime as rt
    from circom_amd.circuits.poseidon import Poseidon
    from circom_amd.compiler import compile_program
    from circom_amd.frontend.dsl import Program
    d = tempfile.mkdtemp(prefix="cw_ubench_compare_")
    cp = compile_program(Program(Poseidon(2), prime="goldilocks") if gl else Program(Poseidon(2)), d, "poseidon2", sym=False)
    circ = rt.Circuit(cp.tape_path, cp.dat_path, cp.r1cs_path)
    B = args.batch or 65536
    rng = np.random.default_rng(1)
    image = np.zeros((B, circ.n_inputs, 4), dtype="<u8")
    image[:, :, 0] = rng.integers(0, 1 << 62, size=(B, circ.n_inputs), dtype=np.uint64)
    b = circ.batch(B, stream=stream.cuda_stream)
    b.set_inputs(image.view(np.uint8).reshape(B, circ.n_inputs, 32))
    b.run(); b.sync()
    assert (b.status() == 0).all()
    res = {"engine": "64-bit runtime" if gl else "256-bit schedule, %s table" % ("Montgomery-form" if circ.montgomery else "canonical"), "batch": B}
    res["elements"] = {str(eb): measure(args, torch, stream, ev, b, circ, 0, B, eb, False) for eb in ((8, 32) if gl else (32,))}
    b.close(); circ.close()
    return res


def sha256_2048(args, torch, stream, ev):
    import bench
    from circom_amd import runtime as rt
    name = "sha256_2048"
    in_tree = glob.glob(str(ROOT / "*" / "cache" / ("sha256_2048_s*_%s" % bench.artefact_fingerprint())))
    if not (in_tree or args.cache_dir):
        return {"skipped": "the cached artefacts of sha256_2048 are not in the tree (build() makes them)"}
    B = args.batch or bench.DEFAULT_BATCH[name]
    cp, _, _ = bench.get_compiled(name, B, args.cache_dir or os.path.dirname(in_tree[0]), 0, None)
    o1 = bench._o1_size(cp.flat)
    w2s = bench._o1_size.witness2signal
    assert w2s is not None, o1
    circ = rt.Circuit(cp.tape_path, cp.dat_path, cp.r1cs_path)
    circ.set_witness_list(w2s)
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    d_msgs = torch.randint(0, 256, (B, circ.n_inputs // 8), dtype=torch.uint8, device=dev, generator=gen)
    torch.cuda.synchronize()
    b = circ.batch(B, stream=stream.cuda_stream)
    assert b.bitmode
    b.set_inputs_rows_device(d_msgs.data_ptr(), circ.n_inputs // 8, msb_first=True)
    b.run(); b.sync()
    first, count = 64 * 1000 + 37, min(args.range, B)                # off a group boundary, inside the batch
    if first + count > B:
        first = 0
    res = {"engine": "bit-plane, emitted" if b.jit else "bit-plane, interpreter", "batch": B, "witness": "--O1 (cw_set_witness_list)", "o1": o1}
    res["elements"] = {"32": measure(args, torch, stream, ev, b, circ, first, count, 32, True)}
    b.close(); circ.close()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workload", choices=("poseidon2_bn128", "poseidon2_goldilocks", "sha256_2048", "all"), default="all")
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=None)
    ap.add_argument("--range", type=int, default=8192, help="sha256_2048: instances of the sub-range")
    ap.add_argument("--cache-dir", default=None)
    ap.add_argument("--out", default=None, help="write the JSON result here as well; a file this tool wrote on the same part is "
                                                  "extended by the workloads of this run (one workload per run)")
    args = ap.parse_args()
    assert args.runs >= 20, "at least 20 timed runs per variant"
    import torch
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    res = {"tool": "tools/ubench_compare.py", "box": torch.cuda.get_device_name(0), "warmup": args.warmup,
           "timing": "one process; HIP events on the batch's stream around each call, the variants taking turns round by round; "
                     "median / min / max of --runs", "workloads": {}}
    names = ("poseidon2_bn128", "poseidon2_goldilocks", "sha256_2048") if args.workload == "all" else (args.workload,)
    if args.out and os.path.exists(args.out):                          # one workload per run: the file gathers them
        old = json.loads(Path(args.out).read_text())
        if old.get("tool") == res["tool"] and old.get("box") == res["box"] and old.get("warmup") == res["warmup"]:
            res["workloads"].update(old.get("workloads", {}))
    for name in names:
        if name == "sha256_2048":
            res["workloads"][name] = sha256_2048(args, torch, stream, ev)
        else:
            res["workloads"][name] = poseidon(args, torch, stream, ev, name.endswith("goldilocks"))
        print(name, json.dumps(res["workloads"][name]), flush=True)
        if args.out:                                                   # (kept after every workload: a later one may be cut short)
            Path(args.out).parent.mkdir(parents=True, exist_ok=True)
            Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
