#!/usr/bin/env python3
"""Boolean inputs as packed rows (cw_set_inputs_rows_device) timed at the metric's shape, Sha256(2048) x 2 097 152: the rows are
the 256-byte messages, instance after instance (512 MB), and the bit transpose of csrc/cw_bits.hip writes the 512 MB of masks
cw_bits_ingest_packed_kernel reads.  In the SAME run, the variants taking turns round by round:

  (a) rows_to_masks   cw_bits_rows_to_masks_kernel alone: HIP events on the batch's stream around cw_set_inputs_rows_device
  (b) memcpy_dtod     hipMemcpyDtoD (async, the same stream, the same events) of the same bytes: 512 MB read, 512 MB written
  (c) packed_step     cw_batch_kernel_ms element 0 (table init + cw_bits_ingest_packed_kernel) of the cw_run behind (a)
  (d) ingest_32       the same element of a cw_run of the SAME batch from the 32-byte image (cw_set_inputs_device): 137 GB read

--warmup rounds, then --runs timed ones; median (min .. max).  Parity: after a step of either kind every status word is 0 and
the outputs of a few instances are hashlib's digest of their rows.  The circuit comes from the artefact cache build() leaves
in the tree (bench.get_compiled; --cache-dir names another); where that is not at hand the tool lowers Sha256(512) and runs it x 2^20 - the result
says which shape it is.

  python tools/ubench_rows_ingest.py --out profiles/rows_ingest_sha256_2048.json
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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=None, help="instances (default: the shape's own)")
    ap.add_argument("--cache-dir", default=None)
    ap.add_argument("--no-ingest-32", action="store_true", help="leave variant (d) out (its image is 32 bytes per input bit)")
    ap.add_argument("--out", default=None, help="write the JSON result here as well")
    args = ap.parse_args()
    assert args.runs >= 20, "at least 20 timed runs per variant"
    import torch
    import bench
    from circom_amd import runtime as rt
    # build()'s cache is the directory of the tree that holds this source's sha256_2048 artefacts; bench.py's own fallback otherwise
    in_tree = glob.glob(str(ROOT / "*" / "cache" / ("sha256_2048_s*_%s" % bench.artefact_fingerprint())))
    cache_root = args.cache_dir or (os.path.dirname(in_tree[0]) if in_tree
                                    else os.path.join(tempfile.gettempdir(), "cw_bench_cache_%d" % os.getuid()))
    workload, B, cached = pick_shape(cache_root)
    B = args.batch or B
    cp, _, _ = bench.get_compiled(workload, B, cache_root, 0, None, flat=False)
    circ = rt.Circuit(cp.tape_path, cp.dat_path, cp.r1cs_path)
    n = circ.n_inputs
    assert n % 64 == 0
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    d_rows = torch.randint(0, 256, (B, n // 8), dtype=torch.uint8, device=dev, generator=gen)     # the messages themselves
    d_copy = torch.empty_like(d_rows)
    d_img32 = None
    if not args.no_ingest_32:
        # one 32-byte value per message bit, most significant bit of a byte first, built in slices: the image only ever exists in HBM
        d_img32 = torch.zeros((B, n, 32), dtype=torch.uint8, device=dev)
        step = max(1, (1 << 28) // n)
        shifts = torch.arange(7, -1, -1, dtype=torch.uint8, device=dev)
        for i in range(0, B, step):
            part = d_rows[i:i + step]
            d_img32[i:i + step, :, 0] = ((part.unsqueeze(2) >> shifts) & 1).reshape(part.shape[0], n)
    torch.cuda.synchronize()
    b = circ.batch(B, stream=stream.cuda_stream)
    assert b.bitmode
    b.set_timing(True)
    sample = [0, 1, B // 2 + 63, B - 1]
    h_rows = {i: d_rows[i].cpu().numpy().tobytes() for i in sample}

    def parity(what):
        assert (b.status() == 0).all(), what
        for i, msg in h_rows.items():
            want = np.unpackbits(np.frombuffer(hashlib.sha256(msg).digest(), dtype=np.uint8)).tolist()
            assert [b.signal(i, 1 + k) for k in range(256)] == want, (what, i)

    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    ms = {"a_rows_to_masks": [], "b_memcpy_dtod": [], "c_packed_step": [], "d_ingest_32": []}
    with torch.cuda.stream(stream):
        for r in range(args.warmup + args.runs):
            ev[0].record(stream)
            b.set_inputs_rows_device(d_rows.data_ptr(), n // 8, msb_first=True)
            ev[1].record(stream)
            b.run(); b.sync()
            t_packed = b.kernel_ms()["ingest"]
            if r == 0:
                parity("rows")
            ev[2].record(stream)
            d_copy.copy_(d_rows, non_blocking=True)
            ev[3].record(stream)
            stream.synchronize()
            t32 = None
            if d_img32 is not None:
                b.set_inputs_device(d_img32.data_ptr())
                b.run(); b.sync()
                t32 = b.kernel_ms()["ingest"]
                if r == 0:
                    parity("32-byte image")
            if r >= args.warmup:
                ms["a_rows_to_masks"].append(ev[0].elapsed_time(ev[1]))
                ms["b_memcpy_dtod"].append(ev[2].elapsed_time(ev[3]))
                ms["c_packed_step"].append(t_packed)
                if t32 is not None:
                    ms["d_ingest_32"].append(t32)
    assert torch.equal(d_copy, d_rows)
    rows_bytes, mask_bytes = B * (n // 8), ((B + 63) // 64) * n * 8
    res = {"tool": "tools/ubench_rows_ingest.py", "box": torch.cuda.get_device_name(0), "workload": workload, "batch": B, "n_inputs": n,
           "metric_shape": bool(cached and workload == "sha256_2048" and B == bench.DEFAULT_BATCH["sha256_2048"]),
           "warmup": args.warmup,
           "timing": "HIP events on the batch's stream (a, b); cw_batch_kernel_ms element 0 = table init + ingest (c, d); the variants "
                     "taking turns round by round; median / min / max",
           "hbm_spec_bytes_per_s": HBM_SPEC,
           "variants": {"a_rows_to_masks": figures(ms["a_rows_to_masks"], rows_bytes, mask_bytes),
                        "b_memcpy_dtod": figures(ms["b_memcpy_dtod"], rows_bytes, rows_bytes),
                        "c_packed_step": figures(ms["c_packed_step"], mask_bytes, mask_bytes)}}
    if ms["d_ingest_32"]:
        res["variants"]["d_ingest_32"] = figures(ms["d_ingest_32"], B * n * 32, mask_bytes)
    res["parity"] = "status words 0 and hashlib digests at instances %s after a step from rows and from the 32-byte image" % sample
    for name, f in res["variants"].items():
        print(name, json.dumps(f), flush=True)
    print(json.dumps(res))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
    b.close(); circ.close()


if __name__ == "__main__":
    main()
