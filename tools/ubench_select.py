#!/usr/bin/env python3
"""Instance lists (cw_select_instances_device, cw_get_witnesses_at_device) timed against existing code in the SAME run, the variants
taking turns round by round, HIP events on the batch's stream around each call; --warmup rounds, then --runs timed ones; median
(min .. max).

Egress by index (--workload poseidon2_goldilocks | poseidon2_bn128 | sha256_2048):
  (a) range       the existing range call at the same shape: cw_get_witnesses_device(_n8) / cw_get_public_device
  (b) identity    cw_get_witnesses_at_device(_n8) with the list 0, 1, 2, ...: the same stores, one 4-byte load per thread more
  (c) every_2nd   the list 0, 2, 4, ... (half the positions): the reads stop being contiguous
  (d) random      a seeded random list of the same length as (c)
  poseidon2_*   Poseidon(2) x 65 536, the whole witness; Goldilocks in both element sizes (8 and 32 bytes)
  sha256_2048   the metric's circuit x 2 097 152 on the emitted bit engine: the public signals of the whole batch (entry0 = 1,
                n = n_public) and, with --o1 (minutes of host time: the circuit is traced and simplified), --o1-instances instances
                of the --O1 witness.  The circuit comes from the artefact cache build() leaves in the tree (bench.get_compiled)
Parity: (b) is compared byte for byte with (a), (c) and (d) with the rows of (a) they name.

Select (--workload select): BitAssert on Goldilocks x --batch (2 097 152) instances whose status words are 0 or 1:
  (a) select_failed / select_clean   cw_select_instances_device with mask = want = 1 / mask = ~0, want = 0
  (b) memcpy_dtod                    a device-to-device copy (torch's copy_ on the batch's stream) of a device IMAGE of the batch's
                                     status words, 4 bytes per instance, uploaded from cw_get_status for each case - the C ABI does
                                     not hand out the address of the words themselves; the select reads them once per launch of
                                     its count and its scatter kernel
  (c) status_flatnonzero             what a caller does today: cw_get_status + np.flatnonzero, by wall clock
for the cases all clean, 1 % failed at random, everything failed.  Parity: the list against np.flatnonzero of cw_get_status.

  python tools/ubench_select.py --workload select --out profiles/select_status.json
"""
import argparse
import glob
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

HBM_SPEC = 8.0e12


def figures(ms, n_written=None):
    med = statistics.median(ms)
    out = {"ms_median": round(med, 5), "ms_min": round(min(ms), 5), "ms_max": round(max(ms), 5), "runs": len(ms)}
    if n_written is not None:
        rate = n_written / (med * 1e-3)
        out.update({"bytes_written": n_written, "bytes_written_per_s": round(rate), "fraction_of_hbm_spec": round(rate / HBM_SPEC, 4)})
    return out


def timed(stream, ev, fn):
    ev[0].record(stream)
    fn()
    ev[1].record(stream)
    stream.synchronize()
    return ev[0].elapsed_time(ev[1])


def egress_shape(torch, stream, ev, args, b, B, entry0, n, eb, range_call, n8):
    """the four variants for entries [entry0, entry0 + n) of B instances, eb bytes per element"""
    dev = torch.device("cuda:0")
    half = B // 2
    d_ident = torch.arange(B, dtype=torch.int32, device=dev)
    d_second = torch.arange(0, 2 * half, 2, dtype=torch.int32, device=dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(2)
    d_rand = torch.randint(0, B, (half,), dtype=torch.int32, device=dev, generator=gen)
    d_a = torch.full((B, n * eb), 0xA5, dtype=torch.uint8, device=dev)
    d_b = torch.full((B, n * eb), 0x5A, dtype=torch.uint8, device=dev)
    d_c = torch.empty((half, n * eb), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()                        # (the fills above ran on torch's current stream, not on the batch's)
    at = lambda lst, m, out: b.witnesses_at_device(lst.data_ptr(), m, out.data_ptr(), entry0, n, n8=n8)
    ms = {"a_range": [], "b_identity": [], "c_every_2nd": [], "d_random": []}
    with torch.cuda.stream(stream):
        for r in range(args.warmup + args.runs):
            ta = timed(stream, ev, lambda: range_call(d_a.data_ptr()))
            tb = timed(stream, ev, lambda: at(d_ident, B, d_b))
            if r == 0:
                assert torch.equal(d_a, d_b), "the identity list does not reproduce the range call"
            tc = timed(stream, ev, lambda: at(d_second, half, d_c))
            if r == 0:
                assert torch.equal(d_c, d_a[0:2 * half:2]), "every second instance"
            td = timed(stream, ev, lambda: at(d_rand, half, d_c))
            if r == 0:
                assert torch.equal(d_c, d_a[d_rand.long()]), "the random list"
            if r >= args.warmup:
                ms["a_range"].append(ta); ms["b_identity"].append(tb); ms["c_every_2nd"].append(tc); ms["d_random"].append(td)
    full, part = B * n * eb, half * n * eb
    out = {"entry0": entry0, "n": n, "element_bytes": eb, "positions": {"a_range": B, "b_identity": B, "c_every_2nd": half, "d_random": half},
           "variants": {"a_range": figures(ms["a_range"], full), "b_identity": figures(ms["b_identity"], full),
                        "c_every_2nd": figures(ms["c_every_2nd"], part), "d_random": figures(ms["d_random"], part)}}
    a, bb = out["variants"]["a_range"], out["variants"]["b_identity"]
    out["identity_over_range"] = round(bb["ms_median"] / a["ms_median"], 4)
    out["ranges_overlap"] = not (bb["ms_min"] > a["ms_max"] or a["ms_min"] > bb["ms_max"])
    del d_a, d_b, d_c
    return out


def run_egress(args, torch, rt):
    from circom_amd.compiler import compile_program
    from circom_amd.frontend.dsl import Program
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    res = {"shapes": {}}
    if args.workload == "sha256_2048":
        import bench
        in_tree = glob.glob(str(ROOT / "*" / "cache" / ("sha256_2048_s*_%s" % bench.artefact_fingerprint())))
        cache_root = args.cache_dir or (os.path.dirname(in_tree[0]) if in_tree
                                        else os.path.join(tempfile.gettempdir(), "cw_bench_cache_%d" % os.getuid()))
        B = args.batch or bench.DEFAULT_BATCH["sha256_2048"]
        cp, _, _ = bench.get_compiled("sha256_2048", B, cache_root, 0, None, flat=args.o1)
        circ = rt.Circuit(cp.tape_path, cp.dat_path, cp.r1cs_path)
        gen = torch.Generator(device=dev)
        gen.manual_seed(1)
        d_msgs = torch.randint(0, 256, (B, circ.n_inputs // 8), dtype=torch.uint8, device=dev, generator=gen)

        def stepped():
            b = circ.batch(B, stream=stream.cuda_stream)
            assert b.bitmode
            b.set_inputs_rows_device(d_msgs.data_ptr(), circ.n_inputs // 8, msb_first=True)
            b.run(); b.sync()
            return b
        b = stepped()
        res["engine"] = "bit-plane, emitted" if b.jit else "bit-plane, interpreter"
        res["shapes"]["public_signals_of_the_batch"] = egress_shape(torch, stream, ev, args, b, B, 1, circ.n_public, 32,
                                                                    lambda p: b.public_signals_device(p), False)
        b.close()
        if args.o1:
            from circom_amd.frontend.circom_simplify import simplify_o1
            circ.set_witness_list(np.asarray(simplify_o1(cp.flat).witness2signal, dtype=np.uint32))
            b = stepped()
            K = min(args.o1_instances, B)
            res["shapes"]["o1_witness_%d_instances" % K] = egress_shape(torch, stream, ev, args, b, K, 0, circ.n_witness, 32,
                                                                        lambda p: b.witnesses_device(0, K, p), False)
            b.close()
    else:
        from circom_amd.circuits.poseidon import Poseidon
        gl = args.workload.endswith("goldilocks")
        d = tempfile.mkdtemp(prefix="cw_ubench_select_")
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
        res["engine"] = "64-bit runtime" if gl else "256-bit schedule, %s table" % ("Montgomery-form" if circ.montgomery else "canonical")
        nw = circ.n_witness
        if gl:
            res["shapes"]["witness_8_bytes"] = egress_shape(torch, stream, ev, args, b, B, 0, nw, 8, lambda p: b.witnesses_device_n8(0, B, p), True)
        res["shapes"]["witness_32_bytes"] = egress_shape(torch, stream, ev, args, b, B, 0, nw, 32, lambda p: b.witnesses_device(0, B, p), False)
        b.close()
    res["batch"] = B
    circ.close()
    return res


def run_select(args, torch, rt):
    from circom_amd.compiler import compile_program
    from circom_amd.frontend.dsl import Program, template

    @template
    def BitAssert(c):
        """a === b on two inputs, out = a b: the status word is 1 where a != b"""
        x = c.input("a")
        y = c.input("b")
        out = c.output("out")
        c.enforce(x, y)
        c.set(out, x * y)
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    d = tempfile.mkdtemp(prefix="cw_ubench_select_")
    cp = compile_program(Program(BitAssert(), prime="goldilocks"), d, "glassert", sym=False)
    circ = rt.Circuit(cp.tape_path, cp.dat_path, cp.r1cs_path)
    B = args.batch or 2097152
    b = circ.batch(B, stream=stream.cuda_stream)
    d_idx = torch.full((B,), -1, dtype=torch.int32, device=dev)
    d_n = torch.zeros(2, dtype=torch.int32, device=dev)
    d_words = torch.zeros(B, dtype=torch.int32, device=dev)
    d_copy = torch.empty_like(d_words)
    torch.cuda.synchronize()
    rng = np.random.default_rng(3)
    res = {"batch": B, "engine": "64-bit runtime", "status_bytes": 4 * B, "cases": {}}
    for case, p_fail in (("all_clean", 0.0), ("one_percent_failed", 0.01), ("everything_failed", 1.0)):
        a = rng.integers(0, 2, size=(B, 1), dtype=np.uint64).repeat(2, axis=1)
        a[rng.random(B) < p_fail, 1] ^= 1                                    # a != b: the assertion fails there
        b.set_inputs_n8(a)
        b.run(); b.sync()
        st = b.status()
        failed = np.flatnonzero(st & 1)
        assert (failed == np.flatnonzero(a[:, 0] != a[:, 1])).all()
        d_words.copy_(torch.from_numpy(st.view(np.int32)))                   # the yardstick copies THESE words
        torch.cuda.synchronize()
        ms = {"a_select_failed": [], "a_select_clean": [], "b_memcpy_dtod": [], "c_status_flatnonzero_wall": []}
        with torch.cuda.stream(stream):
            for r in range(args.warmup + args.runs):
                tf = timed(stream, ev, lambda: b.select_device(1, 1, d_idx.data_ptr(), d_n.data_ptr()))
                if r == 0:
                    k = int(d_n[0].item())
                    assert k == len(failed) and (d_idx[:k].cpu().numpy().astype(np.uint32) == failed).all(), case
                tc = timed(stream, ev, lambda: b.select_device(0xFFFFFFFF, 0, d_idx.data_ptr(), d_n.data_ptr()))
                if r == 0:
                    assert int(d_n[0].item()) == B - len(failed), case
                tm = timed(stream, ev, lambda: d_copy.copy_(d_words, non_blocking=True))
                t0 = time.perf_counter()
                got = np.flatnonzero(b.status() & 1)
                tw = (time.perf_counter() - t0) * 1e3
                assert len(got) == len(failed)
                if r >= args.warmup:
                    ms["a_select_failed"].append(tf); ms["a_select_clean"].append(tc); ms["b_memcpy_dtod"].append(tm)
                    ms["c_status_flatnonzero_wall"].append(tw)
        assert torch.equal(d_copy.cpu(), torch.from_numpy(st.view(np.int32)))
        res["cases"][case] = {"failed": int(len(failed)), "variants": {k: figures(v) for k, v in ms.items()}}
    b.close(); circ.close()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workload", choices=("poseidon2_bn128", "poseidon2_goldilocks", "sha256_2048", "select"), required=True)
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=None, help="instances (default: 65 536; sha256_2048 and select: 2 097 152)")
    ap.add_argument("--o1", action="store_true", help="sha256_2048: also --o1-instances instances of the --O1 witness")
    ap.add_argument("--o1-instances", type=int, default=8192)
    ap.add_argument("--cache-dir", default=None)
    ap.add_argument("--out", default=None, help="write the JSON result here as well")
    args = ap.parse_args()
    assert args.runs >= 20, "at least 20 timed runs per variant"
    import torch
    from circom_amd import runtime as rt
    res = {"tool": "tools/ubench_select.py", "box": torch.cuda.get_device_name(0), "workload": args.workload, "warmup": args.warmup,
           "timing": "HIP events on the batch's stream around each call, the variants taking turns round by round; median / min / max "
                     "(status_flatnonzero: wall clock)", "hbm_spec_bytes_per_s": HBM_SPEC}
    res.update(run_select(args, torch, rt) if args.workload == "select" else run_egress(args, torch, rt))
    print(json.dumps(res))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
