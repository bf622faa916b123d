#!/usr/bin/env python3
"""Bulk egress of the 64-bit runtime timed on Poseidon(2) over Goldilocks x 65 536 (the bench line's shape for that engine):

  (a) cw_get_witnesses_device, 32-byte elements, CW64_EGRESS_TILED=0: cw64_gather_kernel (consecutive lanes = consecutive entries)
  (b) cw_get_witnesses_device, 32-byte elements, cw64_egress_kernel (tiled transpose through LDS)
  (c) cw_get_witnesses_device_n8, 8-byte elements, cw64_egress_kernel
  (y) the project's yardstick for a 32-byte transpose: cw_get_witnesses_device of Poseidon(2) on bn128, same batch

The batch is evaluated once; every form is warmed up and then timed launch by launch with HIP events on the batch's stream
(median, min, max of --launches launches).  Figures: ms, bytes written per second, that rate against the 8 TB/s HBM
specification, witnesses per second.  (a) and (b) are checked to have written the same bytes, (c) the same values.

  python tools/ubench_egress64.py --workdir DIR --compile-only                     # without a GPU: lower the two circuits
  python tools/ubench_egress64.py --workdir DIR --out egress64_poseidon2_65536.json
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

HBM_SPEC = 8.0e12


class Hip:
    """events, a stream and buffers through the HIP runtime the library itself uses"""

    def __init__(self):
        self.h = C.CDLL("libamdhip64.so")
        self.h.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.h.hipFree.argtypes = [C.c_void_p]
        self.h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.h.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
        self.h.hipStreamSynchronize.argtypes = [C.c_void_p]
        self.h.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
        self.h.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
        self.h.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]

    def ok(self, rc):
        assert rc == 0, "HIP error %d" % rc

    def alloc(self, n):
        p = C.c_void_p()
        self.ok(self.h.hipMalloc(C.byref(p), n))
        return p.value

    def stream(self):
        s = C.c_void_p()
        self.ok(self.h.hipStreamCreate(C.byref(s)))
        return s.value

    def event(self):
        e = C.c_void_p()
        self.ok(self.h.hipEventCreate(C.byref(e)))
        return e

    def download(self, p, nbytes):
        out = np.zeros(nbytes, dtype=np.uint8)
        self.ok(self.h.hipDeviceSynchronize())
        self.ok(self.h.hipMemcpy(out.ctypes.data, p, nbytes, 2))
        return out


def compile_circuits(workdir):
    from circom_amd import compiler
    from circom_amd.circuits.poseidon import Poseidon
    from circom_amd.frontend.dsl import Program
    out = {}
    for name, prog in (("poseidon2_goldilocks", lambda: Program(Poseidon(2), prime="goldilocks")), ("poseidon2_bn128", lambda: Program(Poseidon(2)))):
        d = Path(workdir) / name
        d.mkdir(parents=True, exist_ok=True)
        paths = [d / (name + ext) for ext in (".cwt", ".dat", ".r1cs")]
        if not all(p.exists() for p in paths):
            cp = compiler.compile_program(prog(), str(d), name, sym=False)
            paths = [Path(cp.tape_path), Path(cp.dat_path), Path(cp.r1cs_path)]
        out[name] = paths
    return out


def timed(hip, stream, launch, launches, warmup):
    for _ in range(warmup):
        launch()
    hip.ok(hip.h.hipStreamSynchronize(stream))
    evs = [(hip.event(), hip.event()) for _ in range(launches)]
    for e0, e1 in evs:
        hip.ok(hip.h.hipEventRecord(e0, stream))
        launch()
        hip.ok(hip.h.hipEventRecord(e1, stream))
    hip.ok(hip.h.hipStreamSynchronize(stream))
    ms = []
    for e0, e1 in evs:
        t = C.c_float()
        hip.ok(hip.h.hipEventElapsedTime(C.byref(t), e0, e1))
        ms.append(float(t.value))
        hip.h.hipEventDestroy(e0); hip.h.hipEventDestroy(e1)
    return ms


def figures(ms, nbytes, batch):
    med = statistics.median(ms)
    rate = nbytes / (med * 1e-3)
    return {"ms_median": round(med, 5), "ms_min": round(min(ms), 5), "ms_max": round(max(ms), 5), "launches": len(ms), "bytes_written": nbytes,
            "bytes_per_s": round(rate), "fraction_of_hbm_spec": round(rate / HBM_SPEC, 4), "witnesses_per_s": round(batch / (med * 1e-3))}


def evaluated_batch(circ, batch, stream, seed):
    b = circ.batch(batch, stream=stream)
    rng = np.random.default_rng(seed)
    inp = np.zeros((batch, circ.n_inputs, 4), dtype="<u8")
    inp[:, :, 0] = rng.integers(0, 1 << 62, size=(batch, circ.n_inputs), dtype=np.uint64)     # below both primes
    b.set_inputs(inp.view(np.uint8))
    b.run(); b.sync()
    assert (b.status() == 0).all(), "failed instances"
    return b


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--workdir", default=None, help="where the lowered circuits are kept (default: a temporary directory)")
    ap.add_argument("--compile-only", action="store_true")
    ap.add_argument("--box", default=os.uname().nodename, help="name of the machine, recorded in the result")
    ap.add_argument("--out", default=None, help="write the JSON result here as well")
    args = ap.parse_args()
    assert args.launches >= 20, "at least 20 launches per form"
    if args.workdir is None:
        import tempfile
        args.workdir = tempfile.mkdtemp(prefix="egress64_")
    paths = compile_circuits(args.workdir)
    if args.compile_only:
        return
    from circom_amd import runtime as rt
    hip = Hip()
    stream = hip.stream()
    B = args.batch
    res = {"tool": "tools/ubench_egress64.py", "box": args.box, "batch": B, "warmup": args.warmup,
           "timing": "HIP events on the batch's stream around every launch; median / min / max", "hbm_spec_bytes_per_s": HBM_SPEC, "forms": {}}

    circ = rt.Circuit(*[str(p) for p in paths["poseidon2_goldilocks"]])
    os.environ["CW64_EGRESS_TILED"] = "0"                          # read at batch creation: this batch keeps the gather
    b_gather = evaluated_batch(circ, B, stream, 1)
    del os.environ["CW64_EGRESS_TILED"]
    b_tiled = evaluated_batch(circ, B, stream, 1)                  # the same inputs
    nw = circ.n_witness
    res["circuit"] = {"name": "Poseidon(2) on Goldilocks", "n_witness": nw, "n_signals": circ.n_signals, "element_bytes": circ.element_bytes}
    d32, d32b, d8 = hip.alloc(B * nw * 32), hip.alloc(B * nw * 32), hip.alloc(B * nw * 8)
    forms = (("a_gather_32", lambda: b_gather.witnesses_device(0, B, d32), 32),
             ("b_tiled_32", lambda: b_tiled.witnesses_device(0, B, d32b), 32),
             ("c_tiled_8", lambda: b_tiled.witnesses_device_n8(0, B, d8), 8))
    for name, launch, eb in forms:
        ms = timed(hip, stream, launch, args.launches, args.warmup)
        res["forms"][name] = figures(ms, B * nw * eb, B)
        print(name, json.dumps(res["forms"][name]), flush=True)
    img_a = hip.download(d32, B * nw * 32).view("<u8").reshape(B, nw, 4)
    img_b = hip.download(d32b, B * nw * 32).view("<u8").reshape(B, nw, 4)
    img_c = hip.download(d8, B * nw * 8).view("<u8").reshape(B, nw)
    res["images_agree"] = bool((img_a == img_b).all() and (img_a[:, :, 0] == img_c).all() and not img_a[:, :, 1:].any())
    assert res["images_agree"], "the three forms disagree"
    res["b_over_a_speedup"] = round(res["forms"]["a_gather_32"]["ms_median"] / res["forms"]["b_tiled_32"]["ms_median"], 3)
    del img_a, img_b, img_c
    b_gather.close(); b_tiled.close(); circ.close()
    for p in (d32, d32b, d8):
        hip.h.hipFree(p)

    circ = rt.Circuit(*[str(p) for p in paths["poseidon2_bn128"]])
    b = evaluated_batch(circ, B, stream, 2)
    nw = circ.n_witness
    d = hip.alloc(B * nw * 32)
    ms = timed(hip, stream, lambda: b.witnesses_device(0, B, d), args.launches, args.warmup)
    res["forms"]["y_bn128_32"] = dict(figures(ms, B * nw * 32, B), n_witness=nw, bitmode=b.bitmode)
    print("y_bn128_32", json.dumps(res["forms"]["y_bn128_32"]), flush=True)
    b.close(); circ.close()
    hip.h.hipFree(d)

    line = json.dumps(res)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
