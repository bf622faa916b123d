#!/usr/bin/env python3
"""Witness bits out as packed rows (cw_get_witness_rows_device) timed at the metric's shape, Sha256(2048) x 2 097 152 on the
emitted engine: the 256 public signals of every instance are the digests, 64 MB as rows and 17 GB as 32-byte elements.  In the
SAME run, the variants taking turns round by round, HIP events on the batch's stream around each:

  (a) public_rows      cw_get_witness_rows_device(entries 1 .. 256, every instance): cw_bits_masks_to_rows_kernel reads 64 MB of
                       masks and writes 64 MB of rows
  (b) public_elements  cw_get_public_device at the same shape: the same masks out as 17 GB of 32-byte elements
  (c) memcpy_dtod      hipMemcpyDtoD (async, the same stream) of the 64 MB of rows

With --o1 (minutes of host time: the circuit is traced and simplified) the witness list becomes the --O1 witness of the metric
circuit and two more variants are timed on a second batch:

  (d) o1_rows          the whole witness of every instance as rows (156 809 wires x 2 097 152 instances: 41 GB)
  (e) o1_elements      cw_get_witnesses_device for --o1-instances instances of it (8 192: 41 GB as elements as well)

--warmup rounds, then --runs timed ones; median (min .. max), bytes read + written per second.  Parity: the word is 0xFFFFFFFF
and the first 32 bytes of the rows of a few instances are hashlib's digest of their messages.  The circuit comes from the
artefact cache build() leaves in the tree (bench.get_compiled; --cache-dir names another); where that is not at hand the tool
lowers Sha256(512) and runs it x 2^20 - the result says which shape it is.

  python tools/ubench_rows_out.py --out profiles/rows_out_sha256_2048.json
"""
import argparse
import glob
import hashlib
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


def figures(ms, n_read, n_written):
    med = statistics.median(ms)
    rate = (n_read + n_written) / (med * 1e-3)
    return {"ms_median": round(med, 5), "ms_min": round(min(ms), 5), "ms_max": round(max(ms), 5), "runs": len(ms), "bytes_read": n_read,
            "bytes_written": n_written, "bytes_per_s": round(rate), "fraction_of_hbm_spec": round(rate / HBM_SPEC, 4)}


def pick_shape(cache_root):
    """(workload, batch, cached): the metric's shape when its artefacts of this source are in the cache"""
    import bench
    fp = bench.artefact_fingerprint()
    for d in glob.glob(os.path.join(cache_root, "sha256_2048_s*_%s" % fp)):
        if os.path.exists(os.path.join(d, "done")):
            return "sha256_2048", bench.DEFAULT_BATCH["sha256_2048"], True
    return "sha256_512", 1 << 20, False


def timed(stream, ev, fn):
    ev[0].record(stream)
    fn()
    ev[1].record(stream)
    stream.synchronize()
    return ev[0].elapsed_time(ev[1])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=None, help="instances (default: the shape's own)")
    ap.add_argument("--cache-dir", default=None)
    ap.add_argument("--o1", action="store_true", help="variants (d) and (e): the --O1 witness as rows and as elements")
    ap.add_argument("--o1-instances", type=int, default=8192, help="instances of variant (e)")
    ap.add_argument("--out", default=None, help="write the JSON result here as well")
    args = ap.parse_args()
    assert args.runs >= 20, "at least 20 timed runs per variant"
    import torch
    import bench
    from circom_amd import runtime as rt
    in_tree = glob.glob(str(ROOT / "*" / "cache" / ("sha256_2048_s*_%s" % bench.artefact_fingerprint())))
    cache_root = args.cache_dir or (os.path.dirname(in_tree[0]) if in_tree
                                    else os.path.join(tempfile.gettempdir(), "cw_bench_cache_%d" % os.getuid()))
    workload, B, cached = pick_shape(cache_root)
    B = args.batch or B
    cp, _, _ = bench.get_compiled(workload, B, cache_root, 0, None, flat=args.o1)
    circ = rt.Circuit(cp.tape_path, cp.dat_path, cp.r1cs_path)
    n, npub = circ.n_inputs, circ.n_public
    assert n % 64 == 0 and npub >= 256
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    d_msgs = torch.randint(0, 256, (B, n // 8), dtype=torch.uint8, device=dev, generator=gen)     # the messages themselves
    sample = [0, 1, B // 2 + 63, B - 1]
    digests = {i: hashlib.sha256(d_msgs[i].cpu().numpy().tobytes()).digest() for i in sample}
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    NONE = 0xFFFFFFFF

    def stepped_batch():
        b = circ.batch(B, stream=stream.cuda_stream)
        assert b.bitmode
        b.set_inputs_rows_device(d_msgs.data_ptr(), n // 8, msb_first=True)
        b.run(); b.sync()
        assert (b.status() == 0).all()
        return b

    b = stepped_batch()
    pub_stride = 8 * ((npub + 63) // 64)
    d_rows = torch.full((B, pub_stride), 0xA5, dtype=torch.uint8, device=dev)
    d_copy = torch.empty_like(d_rows)
    d_word = torch.zeros(2, dtype=torch.int32, device=dev)
    d_elems = torch.empty((B, npub, 32), dtype=torch.uint8, device=dev)
    ms = {"a_public_rows": [], "b_public_elements": [], "c_memcpy_dtod": []}
    with torch.cuda.stream(stream):
        for r in range(args.warmup + args.runs):
            ta = timed(stream, ev, lambda: b.witness_rows_device(1, npub, 0, B, d_rows.data_ptr(), pub_stride, msb_first=True,
                                                                 d_not_boolean=d_word.data_ptr()))
            tb = timed(stream, ev, lambda: b.public_signals_device(d_elems.data_ptr()))
            tc = timed(stream, ev, lambda: d_copy.copy_(d_rows, non_blocking=True))
            if r == 0:
                assert (int(d_word[0].item()) & NONE) == NONE
                for i, dg in digests.items():
                    assert d_rows[i, :32].cpu().numpy().tobytes() == dg, i
                    assert d_elems[i, :256, 0].cpu().numpy().tolist() == np.unpackbits(np.frombuffer(dg, dtype=np.uint8)).tolist(), i
            if r >= args.warmup:
                ms["a_public_rows"].append(ta); ms["b_public_elements"].append(tb); ms["c_memcpy_dtod"].append(tc)
    assert torch.equal(d_copy, d_rows)
    groups = (B + 63) // 64
    rows_bytes = B * pub_stride
    res = {"tool": "tools/ubench_rows_out.py", "box": torch.cuda.get_device_name(0), "workload": workload, "batch": B, "n_public": npub,
           "engine": "emitted" if b.jit else "interpreter",
           "metric_shape": bool(cached and workload == "sha256_2048" and B == bench.DEFAULT_BATCH["sha256_2048"]), "warmup": args.warmup,
           "timing": "HIP events on the batch's stream around each call, the variants taking turns round by round; median / min / max",
           "hbm_spec_bytes_per_s": HBM_SPEC,
           "variants": {"a_public_rows": figures(ms["a_public_rows"], groups * npub * 8, rows_bytes),
                        "b_public_elements": figures(ms["b_public_elements"], groups * npub * 8, B * npub * 32),
                        "c_memcpy_dtod": figures(ms["c_memcpy_dtod"], rows_bytes, rows_bytes)},
           "parity": "word 0xFFFFFFFF; rows and elements of the instances %s are hashlib's digests of their messages" % sample}
    del d_elems, d_copy
    b.close()
    if args.o1:
        from circom_amd.frontend.circom_simplify import simplify_o1
        w2s = np.asarray(simplify_o1(cp.flat).witness2signal, dtype=np.uint32)
        circ.set_witness_list(w2s)
        b1 = stepped_batch()
        nw, K = circ.n_witness, min(args.o1_instances, B)
        stride = 8 * ((nw + 63) // 64)
        d_all = torch.empty((B, stride), dtype=torch.uint8, device=dev)
        d_el = torch.empty((K, nw, 32), dtype=torch.uint8, device=dev)
        ms1 = {"d_o1_rows": [], "e_o1_elements": []}
        with torch.cuda.stream(stream):
            for r in range(args.warmup + args.runs):
                td = timed(stream, ev, lambda: b1.witness_rows_device(0, nw, 0, B, d_all.data_ptr(), stride, msb_first=False,
                                                                      d_not_boolean=d_word.data_ptr()))
                te = timed(stream, ev, lambda: b1.witnesses_device(0, K, d_el.data_ptr()))
                if r == 0:
                    assert (int(d_word[0].item()) & NONE) == NONE
                    for i in (0, K - 1):                            # the rows of an instance against its elements
                        want = np.packbits(d_el[i, :, 0].cpu().numpy(), bitorder="little")
                        assert not d_el[i, :, 1:].any().item() and (d_all[i, :len(want)].cpu().numpy() == want).all(), i
                if r >= args.warmup:
                    ms1["d_o1_rows"].append(td); ms1["e_o1_elements"].append(te)
        res["o1"] = {"wires": int(nw), "rows_instances": B, "elements_instances": K}
        res["variants"]["d_o1_rows"] = figures(ms1["d_o1_rows"], groups * nw * 8, B * stride)
        res["variants"]["e_o1_elements"] = figures(ms1["e_o1_elements"], ((K + 63) // 64) * nw * 8, K * nw * 32)
        b1.close()
    for name, f in res["variants"].items():
        print(name, json.dumps(f), flush=True)
    print(json.dumps(res))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
    circ.close()


if __name__ == "__main__":
    main()
