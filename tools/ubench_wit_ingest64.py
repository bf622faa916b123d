#!/usr/bin/env python3
"""Supplied witnesses of the 64-bit runtime timed on Poseidon(2) over Goldilocks x 65 536 (1 108 entries per witness):

  (a) cw_set_witnesses_device_n8, 8-byte elements:  cw64_transpose_in_kernel<8, true>
  (b) cw_set_witnesses_device,    32-byte elements: cw64_transpose_in_kernel<32, true>
  (y) the yardstick from the same run: cw64_egress_kernel for the same ranges, cw_get_witnesses_device_n8 / cw_get_witnesses_device

One batch is evaluated and its witnesses streamed out (8-byte and 32-byte image); a second batch of the same circuit takes them
back in.  Before anything is timed: egress -> supply -> egress must round-trip byte for byte in both element widths, and the
supplied batch must check clean.  Then every form is warmed up (--warmup launches; the first supply also runs the table's init
kernel, inside the warm-up) and timed launch by launch with HIP events on the batch's stream: median (min .. max) of --launches
launches.  Figures: ms, bytes read + bytes written per second, that rate against the 8 TB/s HBM specification.

  python tools/ubench_wit_ingest64.py --workdir DIR --compile-only                     # without a GPU: lower the circuit
  python tools/ubench_wit_ingest64.py --workdir DIR --out profiles/wit_ingest64_poseidon2_65536.json
"""
import argparse
import json
import os
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

from ubench_egress64 import HBM_SPEC, Hip, compile_circuits, evaluated_batch, timed   # noqa: E402


def figures(ms, n_read, n_written, batch):
    med = statistics.median(ms)
    rate = (n_read + n_written) / (med * 1e-3)
    return {"ms_median": round(med, 5), "ms_min": round(min(ms), 5), "ms_max": round(max(ms), 5), "launches": len(ms), "bytes_read": n_read,
            "bytes_written": n_written, "bytes_per_s": round(rate), "fraction_of_hbm_spec": round(rate / HBM_SPEC, 4),
            "witnesses_per_s": round(batch / (med * 1e-3))}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--workdir", default=None, help="where the lowered circuit is kept (default: a temporary directory)")
    ap.add_argument("--compile-only", action="store_true")
    ap.add_argument("--box", default=os.uname().nodename, help="name of the machine, recorded in the result")
    ap.add_argument("--out", default=None, help="write the JSON result here as well")
    args = ap.parse_args()
    assert args.launches >= 20, "at least 20 launches per form"
    if args.workdir is None:
        import tempfile
        args.workdir = tempfile.mkdtemp(prefix="wit_ingest64_")
    paths = compile_circuits(args.workdir)["poseidon2_goldilocks"]
    if args.compile_only:
        return
    from circom_amd import runtime as rt
    hip = Hip()
    stream = hip.stream()
    B = args.batch
    circ = rt.Circuit(*[str(p) for p in paths])
    nw = circ.n_witness
    res = {"tool": "tools/ubench_wit_ingest64.py", "box": args.box, "batch": B, "warmup": args.warmup,
           "timing": "HIP events on the batch's stream around every launch; median / min / max",
           "bytes": "supply: read = the image, written = the listed rows of the value table but slot 0; egress: the other way round",
           "hbm_spec_bytes_per_s": HBM_SPEC,
           "circuit": {"name": "Poseidon(2) on Goldilocks", "n_witness": nw, "n_signals": circ.n_signals, "element_bytes": circ.element_bytes}}
    src = evaluated_batch(circ, B, stream, 1)
    dst = {8: circ.batch(B, stream=stream), 32: circ.batch(B, stream=stream)}     # one per width: each round trip fills an untouched table
    d = {8: hip.alloc(B * nw * 8), 32: hip.alloc(B * nw * 32)}
    back = {8: hip.alloc(B * nw * 8), 32: hip.alloc(B * nw * 32)}
    egress = {8: src.witnesses_device_n8, 32: src.witnesses_device}
    supply = {8: dst[8].set_witnesses_device_n8, 32: dst[32].set_witnesses_device}
    egress_back = {8: dst[8].witnesses_device_n8, 32: dst[32].witnesses_device}
    # egress -> supply -> egress, byte for byte; the supplied table checks clean
    for eb in (8, 32):
        egress[eb](0, B, d[eb])
        supply[eb](0, B, d[eb])
        assert dst[eb].witnesses_missing() == 0
        egress_back[eb](0, B, back[eb])
        dst[eb].check_r1cs(); dst[eb].sync()
        assert (dst[eb].status() == 0).all(), "the supplied batch does not check clean (%d-byte form)" % eb
        a, b = hip.download(d[eb], B * nw * eb), hip.download(back[eb], B * nw * eb)
        assert a.any() and np.array_equal(a, b), "egress -> supply -> egress differs (%d-byte form)" % eb
        del a, b
    res["round_trip_byte_for_byte"] = True
    res["forms"] = {}
    table = B * (nw - 1) * 8                                         # entry 0 is not stored
    for name, launch, eb in (("a_supply_8", lambda: supply[8](0, B, d[8]), 8), ("b_supply_32", lambda: supply[32](0, B, d[32]), 32)):
        ms = timed(hip, stream, launch, args.launches, args.warmup)
        res["forms"][name] = figures(ms, B * nw * eb, table, B)
        print(name, json.dumps(res["forms"][name]), flush=True)
    for name, launch, eb in (("y_egress_8", lambda: egress[8](0, B, d[8]), 8), ("y_egress_32", lambda: egress[32](0, B, d[32]), 32)):
        ms = timed(hip, stream, launch, args.launches, args.warmup)
        res["forms"][name] = figures(ms, B * nw * 8, B * nw * eb, B)
        print(name, json.dumps(res["forms"][name]), flush=True)
    for b in dst.values():
        b.sync()
        assert (b.status() == 0).all()
        b.close()
    src.close(); circ.close()
    for p in list(d.values()) + list(back.values()):
        hip.h.hipFree(p)
    print(json.dumps(res))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
