#!/usr/bin/env python3
"""Signal columns out (cw_get_signals_range_device) timed against the existing paths for the same bytes, all in ONE process, HIP
events on the batch's stream around each call, the variants taking turns round by round:

  Poseidon(2) x 65 536, bn128 (Montgomery-form table) and Goldilocks (64-bit runtime), the witness list naming every signal:
    signals_32       every signal as 32-byte elements
    signals_8        every signal as 8-byte elements (bn128: the low 8 bytes, the word reports)
    at_identity_32   cw_get_witnesses_at_device over the identity list for the same signals: the existing path for those bytes
    memcpy_dtod      hipMemcpyDtoD of the 32-byte image
  Sha256(2048) at the benchmark batch, emitted bit engine (--workload / --batch name another shape of bench.py; the artefacts
  come from the cache build() leaves in the tree, or are lowered here):
    digest_bytes     the 256 output bits (signals 1 .. 256) as one-byte values
    public_elements  cw_get_public_device: the same signals as 32-byte elements, 32 times the bytes
    internal_4096    a run of 4 096 consecutive internal signals that the --O1 witness list (simplify_o1's witness2signal) does
                     not hold, as one-byte values: no other bulk call reaches them.  The result records the run and how many
                     of its signals the list holds (0 where such a run exists)

No threshold is put on a time.  --warmup rounds, then --runs timed ones; median (min .. max).

  python tools/ubench_signals_out.py --out profiles/signals_out_mi355x.json
"""
import argparse
import glob
import hashlib
import json
import os
import statistics
import sys
import tempfile
import traceback
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def figures(ms, n_written):
    med = statistics.median(ms)
    return {"ms_median": round(med, 5), "ms_min": round(min(ms), 5), "ms_max": round(max(ms), 5), "runs": len(ms),
            "bytes_written": int(n_written), "written_bytes_per_s": round(n_written / (med * 1e-3))}


def timed(stream, ev, fn):
    ev[0].record(stream)
    fn()
    ev[1].record(stream)
    stream.synchronize()
    return ev[0].elapsed_time(ev[1])


def rounds(args, stream, ev, variants, first_round=None):
    ms = {k: [] for k in variants}
    for r in range(args.warmup + args.runs):
        for k, fn in variants.items():
            t = timed(stream, ev, fn)
            if r >= args.warmup:
                ms[k].append(t)
        if r == 0 and first_round:
            first_round()
    return ms


def poseidon(args, torch, rt, prime, stream, ev):
    from circom_amd.circuits.poseidon import Poseidon
    from circom_amd.compiler import compile_program
    from circom_amd.frontend.dsl import Program
    d = tempfile.mkdtemp(prefix="cw_sigout_")
    cp = compile_program(Program(Poseidon(2), prime="goldilocks") if prime == "goldilocks" else Program(Poseidon(2)), d, "poseidon2_" + prime, sym=False)
    circ = rt.Circuit(cp.tape_path, cp.dat_path, cp.r1cs_path)
    ns = circ.n_signals
    circ.set_witness_list(np.arange(ns, dtype=np.uint32))
    B = args.poseidon_batch
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(1)
    ins = np.zeros((B, circ.n_inputs, 32), dtype=np.uint8)
    ins[:, :, :7] = rng.integers(0, 256, size=(B, circ.n_inputs, 7), dtype=np.uint8)
    b = circ.batch(B, stream=stream.cuda_stream)
    b.set_inputs(ins)
    b.run(); b.sync()
    assert (b.status() == 0).all()
    d32 = torch.zeros((B, ns, 32), dtype=torch.uint8, device=dev)
    d_at = torch.zeros((B, ns, 32), dtype=torch.uint8, device=dev)
    d8 = torch.zeros((B, ns, 8), dtype=torch.uint8, device=dev)
    d_copy = torch.empty_like(d32)
    d_idx = torch.arange(B, dtype=torch.int32, device=dev)
    d_word = torch.zeros(2, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    variants = {
        "signals_32": lambda: b.signals_range_device(0, ns, 0, B, d32.data_ptr(), ns * 32, 32),
        "signals_8": lambda: b.signals_range_device(0, ns, 0, B, d8.data_ptr(), ns * 8, 8, d_word.data_ptr()),
        "at_identity_32": lambda: b.witnesses_at_device(d_idx.data_ptr(), B, d_at.data_ptr(), 0, ns),
        "memcpy_dtod": lambda: d_copy.copy_(d32, non_blocking=True),
    }

    def parity():
        assert torch.equal(d32, d_at), "the 32-byte columns differ from cw_get_witnesses_at_device"
        assert torch.equal(d8, d32[:, :, :8].contiguous()), "the 8-byte columns are not the low bytes"

    with torch.cuda.stream(stream):
        ms = rounds(args, stream, ev, variants, parity)
    out = {"prime": prime, "batch": B, "signals": int(ns), "element_bytes": circ.element_bytes,
           "variants": {"signals_32": figures(ms["signals_32"], B * ns * 32), "signals_8": figures(ms["signals_8"], B * ns * 8),
                        "at_identity_32": figures(ms["at_identity_32"], B * ns * 32), "memcpy_dtod": figures(ms["memcpy_dtod"], B * ns * 32)},
           "parity": "signals_32 == at_identity_32 byte for byte; signals_8 == their low 8 bytes"}
    b.close(); circ.close()
    return out


def o1_run(args, flat, ns, want):
    """(signal0, n, held, list length): the first run of `want` consecutive signal ids behind the main inputs that the --O1
    witness list (frontend/circom_simplify.simplify_o1, or --o1-list: its witness2signal saved with numpy) holds fewest of -
    none, where such a run exists"""
    if args.o1_list:
        w2s = np.load(args.o1_list).astype(np.int64)
    else:
        from circom_amd.frontend.circom_simplify import simplify_o1
        w2s = np.asarray(simplify_o1(flat).witness2signal, dtype=np.int64)
    assert w2s.min() == 0 and w2s.max() < ns and (np.diff(w2s) > 0).all()
    held = np.zeros(ns + 1, dtype=np.int64)
    held[w2s + 1] = 1
    cum = np.cumsum(held)                                            # cum[k] = listed signals below id k
    lo = flat.main_input_start + flat.n_main_inputs
    n = min(want, ns - lo)
    inside = cum[lo + n:ns + 1] - cum[lo:ns + 1 - n]                 # listed signals of [s, s + n) for s = lo ..
    s0 = lo + int(np.argmin(inside))
    return s0, n, int(inside.min()), int(len(w2s))


def sha256(args, torch, rt, stream, ev):
    import bench
    fp = bench.artefact_fingerprint()
    workload = args.workload
    in_tree = glob.glob(str(ROOT / "*" / "cache" / ("%s_s*_%s" % (workload, fp))))
    cache_root = args.cache_dir or (os.path.dirname(in_tree[0]) if in_tree else os.path.join(tempfile.gettempdir(), "cw_bench_cache_%d" % os.getuid()))
    B = args.batch or bench.DEFAULT_BATCH[workload]
    cp, _, _ = bench.get_compiled(workload, B, cache_root, 0, None)   # (lowers the circuit where the cache does not hold it: minutes)
    circ = rt.Circuit(cp.tape_path, cp.dat_path, cp.r1cs_path)
    n, npub, ns = circ.n_inputs, circ.n_public, circ.n_signals
    assert npub >= 256
    run0, run_n, run_held, o1_len = o1_run(args, cp.flat, ns, 4096)
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    d_msgs = torch.randint(0, 256, (B, n // 8), dtype=torch.uint8, device=dev, generator=gen)
    sample = [0, 1, B // 2 + 63, B - 1]
    digests = {i: hashlib.sha256(d_msgs[i].cpu().numpy().tobytes()).digest() for i in sample}
    b = circ.batch(B, stream=stream.cuda_stream)
    assert b.bitmode
    b.set_inputs_rows_device(d_msgs.data_ptr(), n // 8, msb_first=True)
    b.run(); b.sync()
    assert (b.status() == 0).all()
    d_dig = torch.full((B, 256), 0xA5, dtype=torch.uint8, device=dev)
    d_int = torch.full((B, run_n), 0xA5, dtype=torch.uint8, device=dev)
    d_elems = torch.empty((B, npub, 32), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    variants = {
        "digest_bytes": lambda: b.signals_range_device(1, 256, 0, B, d_dig.data_ptr(), 256, 1),
        "public_elements": lambda: b.public_signals_device(d_elems.data_ptr()),
        "internal_4096": lambda: b.signals_range_device(run0, run_n, 0, B, d_int.data_ptr(), run_n, 1),
    }

    def parity():
        for i, dg in digests.items():
            assert d_dig[i].cpu().numpy().tolist() == np.unpackbits(np.frombuffer(dg, dtype=np.uint8)).tolist(), i
        assert torch.equal(d_dig, d_elems[:, :256, 0].contiguous())
        assert int(d_int.max().item()) <= 1
        for i in (0, B - 1):
            assert [b.signal(i, run0 + k) for k in (0, 1, run_n - 1)] == [int(d_int[i, k].item()) for k in (0, 1, run_n - 1)]

    with torch.cuda.stream(stream):
        ms = rounds(args, stream, ev, variants, parity)
    out = {"workload": workload, "batch": B, "signals": int(ns), "engine": "emitted" if b.jit else "interpreter",
           "benchmark_shape": bool(workload == "sha256_2048" and B == bench.DEFAULT_BATCH["sha256_2048"]),
           "internal_run": {"signal0": int(run0), "n": int(run_n), "held_by_the_o1_witness_list": run_held, "o1_witness_list": o1_len},
           "variants": {"digest_bytes": figures(ms["digest_bytes"], B * 256), "public_elements": figures(ms["public_elements"], B * npub * 32),
                        "internal_4096": figures(ms["internal_4096"], B * run_n)},
           "parity": "digest bytes of the instances %s are hashlib's digests; digest_bytes == byte 0 of public_elements; the internal "
                     "run is 0 / 1 and equals cw_get_signal at its corners" % sample}
    out["digest_bytes_not_slower_than_public_elements"] = bool(out["variants"]["digest_bytes"]["ms_median"] <= out["variants"]["public_elements"]["ms_median"])
    b.close(); circ.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=None, help="instances of the SHA-256 part (default: the shape's own)")
    ap.add_argument("--poseidon-batch", type=int, default=65536)
    ap.add_argument("--workload", default="sha256_2048", help="the SHA-256 circuit of bench.py to run (default: the benchmark's)")
    ap.add_argument("--o1-list", default=None, help="witness2signal of the --O1 system as a .npy file (default: simplified here, minutes)")
    ap.add_argument("--cache-dir", default=None)
    ap.add_argument("--out", default=None, help="write the JSON result here as well")
    args = ap.parse_args()
    import torch
    from circom_amd import runtime as rt
    stream = torch.cuda.Stream(device=torch.device("cuda:0"))
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    res = {"tool": "tools/ubench_signals_out.py", "box": torch.cuda.get_device_name(0), "warmup": args.warmup,
           "timing": "HIP events on the batch's stream around each call, the variants taking turns round by round; median / min / max"}
    parts = (("poseidon2_bn128", lambda: poseidon(args, torch, rt, "bn128", stream, ev)),
             ("poseidon2_goldilocks", lambda: poseidon(args, torch, rt, "goldilocks", stream, ev)),
             ("sha256", lambda: sha256(args, torch, rt, stream, ev)))
    failed = False
    for name, part in parts:
        try:
            res[name] = part()
        except Exception:                                            # a part that could not be measured is recorded as such
            failed = True
            res[name] = {"error": traceback.format_exc()[-1500:]}
            print(name, json.dumps(res[name]), flush=True)
            break                                                    # nothing more is started on the device behind a failure
        print(name, json.dumps(res[name]), flush=True)
    print(json.dumps(res))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1) + "\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
