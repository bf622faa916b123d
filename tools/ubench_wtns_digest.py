#!/usr/bin/env python3
"""Witness digests (cw_get_wtns_digests_device) timed beside what they replace, in the SAME run, the variants taking turns round
by round, HIP events on the batch's stream around each call; --warmup rounds, then --runs timed ones; median (min .. max).

  (a) digest          cw_get_wtns_digests_device of the whole batch, and of the range of (b) when that is smaller
  (b) egress          cw_get_witnesses_device(_n8) of a range into a device buffer - the bytes the digest avoids writing; the range
                      is the whole batch, or as many instances as --egress-gib of image hold
  (c) hashlib_host    hashlib.sha256 over ONE instance's file image on the host (wall clock), scaled to the batch and labelled as
                      extrapolated - what a caller does today, after the egress and the copy to the host
  (d) valu_fraction   blocks/s x the VALU instructions of one block's loop body (--valu-per-block, from the disassembly: NOTES) as
                      a fraction of the full-rate VALU figure of profiles/r03_ubench_isa.json (wave instructions/s, v_add_u32)
Parity: the digests of the first and the last instance of the batch against hashlib over their egressed images, in the same run.

  --workload poseidon2_bn128 | poseidon2_goldilocks   Poseidon(2) x 65 536 (Montgomery-form table / 64-bit runtime)
  --workload sha256_512                               Sha256(512) x 4 096 on the interpreted bit engine
  --workload sha256_2048                              the metric's circuit x 2 097 152 on the emitted bit engine, digests of a
                                                      sub-range of --range (8 192) instances; the artefact cache build() leaves in
                                                      the tree is needed (the workload is skipped with a message otherwise)

  python tools/ubench_wtns_digest.py --workload poseidon2_bn128 --out profiles/wtns_digests_poseidon2_bn128.json
"""
import argparse
import glob
import hashlib
import json
import os
import statistics
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def figures(ms):
    return {"ms_median": round(statistics.median(ms), 5), "ms_min": round(min(ms), 5), "ms_max": round(max(ms), 5), "runs": len(ms)}


def timed(stream, ev, fn):
    ev[0].record(stream)
    fn()
    ev[1].record(stream)
    stream.synchronize()
    return ev[0].elapsed_time(ev[1])


def full_rate_valu():
    rows = json.loads((ROOT / "profiles" / "r03_ubench_isa.json").read_text())
    return max(r["wave_inst_per_s"] for r in rows if r.get("kind") == "valu" and r.get("op") == "v_add_u32")


def measure(args, torch, stream, ev, b, circ, first, count):
    """the variants for the instances [first, first + count) of a batch that has run"""
    from circom_amd.hip_elements.writers import wtns_bytes
    dev = torch.device("cuda:0")
    n8, nw = circ.element_bytes, circ.n_witness
    row = nw * n8
    k_egress = max(1, min(count, int(args.egress_gib * (1 << 30)) // row))
    d_dig = torch.full((count, 32), 0xA5, dtype=torch.uint8, device=dev)
    d_dig_k = torch.full((k_egress, 32), 0xA5, dtype=torch.uint8, device=dev)
    d_img = torch.empty((k_egress, row), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    egress = (lambda: b.witnesses_device_n8(first, k_egress, d_img.data_ptr())) if n8 == 8 else (lambda: b.witnesses_device(first, k_egress, d_img.data_ptr()))
    ms = {"a_digest": [], "a_digest_egress_range": [], "b_egress": []}
    with torch.cuda.stream(stream):
        for r in range(args.warmup + args.runs):
            ta = timed(stream, ev, lambda: b.wtns_digests_device(first, count, d_dig.data_ptr()))
            tk = timed(stream, ev, lambda: b.wtns_digests_device(first, k_egress, d_dig_k.data_ptr()))
            tb = timed(stream, ev, egress)
            if r >= args.warmup:
                ms["a_digest"].append(ta); ms["a_digest_egress_range"].append(tk); ms["b_egress"].append(tb)
    # parity and (c): hashlib over the images of the range's first and last egressed instance
    head = wtns_bytes(circ.q, [0] * nw)[:44 + n8]
    dig = d_dig.cpu().numpy()
    host_s = []
    for j in (0, k_egress - 1):
        img = head + d_img[j].cpu().numpy().tobytes()
        t0 = time.perf_counter()
        want = hashlib.sha256(img).digest()
        host_s.append(time.perf_counter() - t0)
        assert dig[j].tobytes() == want, "digest of instance %d differs from hashlib over its image" % (first + j)
    assert torch.equal(d_dig[:k_egress], d_dig_k)
    plan_bytes = 44 + n8 + row
    blocks = (plan_bytes + 9 + 63) // 64
    a = figures(ms["a_digest"])
    out = {"first": first, "instances": count, "n_witness": nw, "element_bytes": n8, "file_bytes": plan_bytes, "blocks_per_instance": blocks,
           "egress_instances": k_egress,
           "variants": {"a_digest": a, "a_digest_egress_range": figures(ms["a_digest_egress_range"]), "b_egress": figures(ms["b_egress"])}}
    sec = a["ms_median"] * 1e-3
    out["a_message_bytes_per_s"] = round(count * plan_bytes / sec)
    wave_blocks = ((first % 64 + count + 63) // 64) * blocks                      # blocks of a wave of 64 lanes
    out["a_wave_blocks_per_s"] = round(wave_blocks / sec)
    be = out["variants"]["b_egress"]
    be["bytes_written"] = k_egress * row
    be["bytes_written_per_s"] = round(k_egress * row / (be["ms_median"] * 1e-3))
    out["b_egress_extrapolated_to_the_range_ms"] = round(be["ms_median"] * count / k_egress, 3)
    out["c_hashlib_host"] = {"one_instance_s": round(min(host_s), 6), "extrapolated_to_the_range_s": round(min(host_s) * count, 3),
                             "note": "extrapolated: one instance hashed on one host core, times the instances of the range"}
    rate = full_rate_valu()
    out["d_valu"] = {"valu_per_block": args.valu_per_block, "full_rate_wave_inst_per_s": rate,
                     "fraction_of_full_rate": round(wave_blocks / sec * args.valu_per_block / rate, 4)}
    del d_img
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workload", choices=("poseidon2_bn128", "poseidon2_goldilocks", "sha256_512", "sha256_2048"), required=True)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=None)
    ap.add_argument("--range", type=int, default=8192, help="sha256_2048: instances of the sub-range")
    ap.add_argument("--egress-gib", type=float, default=4.0, help="largest image of variant (b)")
    ap.add_argument("--valu-per-block", type=int, default=1400, help="VALU instructions of one block's loop body (disassembly)")
    ap.add_argument("--cache-dir", default=None)
    ap.add_argument("--out", default=None, help="write the JSON result here as well")
    args = ap.parse_args()
    assert args.runs >= 20, "at least 20 timed runs per variant"
    import torch
    from circom_amd import runtime as rt
    from circom_amd.compiler import compile_program
    from circom_amd.frontend.dsl import Program
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    res = {"tool": "tools/ubench_wtns_digest.py", "box": torch.cuda.get_device_name(0), "workload": args.workload, "warmup": args.warmup,
           "timing": "HIP events on the batch's stream around each call, the variants taking turns round by round; median / min / max "
                     "(hashlib: wall clock of one instance, extrapolated)"}
    d = tempfile.mkdtemp(prefix="cw_ubench_digest_")
    rng = np.random.default_rng(1)
    if args.workload.startswith("poseidon2"):
        from circom_amd.circuits.poseidon import Poseidon
        gl = args.workload.endswith("goldilocks")
        cp = compile_program(Program(Poseidon(2), prime="goldilocks") if gl else Program(Poseidon(2)), d, "poseidon2", sym=False)
        circ = rt.Circuit(cp.tape_path, cp.dat_path, cp.r1cs_path)
        B = args.batch or 65536
        image = np.zeros((B, circ.n_inputs, 4), dtype="<u8")
        image[:, :, 0] = rng.integers(0, 1 << 62, size=(B, circ.n_inputs), dtype=np.uint64)
        b = circ.batch(B, stream=stream.cuda_stream)
        b.set_inputs(image.view(np.uint8).reshape(B, circ.n_inputs, 32))
        b.run(); b.sync()
        assert (b.status() == 0).all()
        res["engine"] = "64-bit runtime" if gl else "256-bit schedule, %s table" % ("Montgomery-form" if circ.montgomery else "canonical")
        first, count = 0, B
    else:
        import bench
        name = args.workload
        if name == "sha256_2048":
            in_tree = glob.glob(str(ROOT / "*" / "cache" / ("sha256_2048_s*_%s" % bench.artefact_fingerprint())))
            if not (in_tree or args.cache_dir):
                print(json.dumps(dict(res, skipped="the cached artefacts of sha256_2048 are not in the tree (build() makes them)")))
                return
            B = args.batch or bench.DEFAULT_BATCH[name]
            cp, _, _ = bench.get_compiled(name, B, args.cache_dir or os.path.dirname(in_tree[0]), 0, None)
            first, count = 64 * 1000 + 37, min(args.range, B)                # off a group boundary, inside the batch
        else:
            from circom_amd.circuits.sha256 import Sha256
            B = args.batch or 4096
            cp = compile_program(Program(Sha256(512)), d, name, sym=False, bits=True, jit=False)
            first, count = 0, B
        circ = rt.Circuit(cp.tape_path, cp.dat_path, cp.r1cs_path)
        gen = torch.Generator(device=dev)
        gen.manual_seed(1)
        d_msgs = torch.randint(0, 256, (B, circ.n_inputs // 8), dtype=torch.uint8, device=dev, generator=gen)
        torch.cuda.synchronize()
        b = circ.batch(B, stream=stream.cuda_stream)
        assert b.bitmode
        b.set_inputs_rows_device(d_msgs.data_ptr(), circ.n_inputs // 8, msb_first=True)
        b.run(); b.sync()
        if first + count > B:
            first = 0
        res["engine"] = "bit-plane, emitted" if b.jit else "bit-plane, interpreter"
    res["batch"] = B
    res.update(measure(args, torch, stream, ev, b, circ, first, count))
    b.close(); circ.close()
    print(json.dumps(res))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
