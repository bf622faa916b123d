"""ctypes binding of the C ABI (include/circom_amd.h -> circom_amd/lib/libcircom_amd.so).

Host-side mirror of the reference's runtime objects: `Circuit` ~ Circom_Circuit (circom.hpp:36-43),
`Batch` ~ Circom_CalcWit (calcwit.hpp:17-66) for B instances.  There is no CPU fallback: if the HIP
library is missing or no GPU is present, computing calls raise.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from pathlib import Path

import numpy as np

_HERE = Path(__file__).resolve().parent
LIB_PATH = Path(os.environ["CW_LIB"]).resolve() if os.environ.get("CW_LIB") else _HERE / "lib" / "libcircom_amd.so"   # CW_LIB: diagnostics builds

ST_OK, ST_ASSERT_FAILED, ST_ARITH, ST_R1CS_FAILED, ST_BAD_WITNESS = 0, 1, 2, 4, 8
ROWS_MSB_FIRST = 1      # CW_ROWS_MSB_FIRST
R1CS_A, R1CS_B, R1CS_C = 1, 2, 4     # CW_R1CS_A / _B / _C: the parts of cw_get_r1cs_products


class CwError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("circom_amd error %d: %s" % (code, msg))
        self.code = code


CLI_PATH = _HERE / "bin" / "cw_witness"     # process-level drop-in (csrc/cw_cli.cpp), built with the library


def build_library(force: bool = False) -> Path:
    """Compile the HIP extension in-tree for gfx950 (hipcc cross-compiles without a GPU)."""
    srcs = [_HERE / "csrc" / n for n in ("cw_kernels.hip", "cw_bits.hip", "cw64.hip", "cw_host.cpp", "cw_cli.cpp", "cw_kernels.h",
                                         "cw_tape.h", "cw_r1cs_plan.h", "cw_bits_host.h", "cw_bits_layout.h", "cw_devbuf.h", "cw_rerun.h", "cw_pieces.h", "cw_rows.h", "cw_columns.h", "cw_columns.hip.h", "cw_select.h", "cw_signals.h", "cw_fn64.h", "cw_wtns_read.h", "cw_compare.h", "cw_compare.hip.h", "cw_wtns_digest.h", "cw_sha256.h", "fp256.hip.h", "cw_rowops.hip.h", "cw_list.hip.h", "cw_call.hip.h")]
    outs = [LIB_PATH, CLI_PATH]
    if not force and all(o.exists() and all(o.stat().st_mtime >= s.stat().st_mtime for s in srcs) for o in outs):
        return LIB_PATH
    subprocess.run(["make", "-j4", "-C", str(_HERE / "csrc")], check=True, capture_output=True)
    return LIB_PATH


_lib = None

_SIGS = {
    "cw_last_error": (C.c_char_p, []),
    "cw_version": (C.c_char_p, []),
    "cw_load": (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(C.c_void_p)]),
    "cw_free": (None, [C.c_void_p]),
    "cw_n_signals": (C.c_uint32, [C.c_void_p]),
    "cw_io_map_size": (C.c_uint32, [C.c_void_p]),
    "cw_io_map_offset": (C.c_int64, [C.c_void_p, C.c_uint32, C.c_uint32]),
    "cw_bus_map_size": (C.c_uint32, [C.c_void_p]),
    "cw_bus_field": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32] + [C.POINTER(C.c_uint32)] * 4),
    "cw_n_witness": (C.c_uint32, [C.c_void_p]),
    "cw_n_inputs": (C.c_uint32, [C.c_void_p]),
    "cw_set_witness_list": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.c_uint32]),
    "cw_input_start": (C.c_uint32, [C.c_void_p]),
    "cw_n_constraints": (C.c_uint32, [C.c_void_p]),
    "cw_n_public": (C.c_uint32, [C.c_void_p]),
    "cw_n_rows": (C.c_uint64, [C.c_void_p]),
    "cw_n_mmul": (C.c_uint64, [C.c_void_p]),
    "cw_prime": (None, [C.c_void_p, C.c_char_p]),
    "cw_input_size": (C.c_int64, [C.c_void_p, C.c_char_p, C.POINTER(C.c_uint32)]),
    "cw_batch_create": (C.c_int, [C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.POINTER(C.c_void_p)]),
    "cw_batch_free": (None, [C.c_void_p]),
    "cw_batch_size": (C.c_uint32, [C.c_void_p]),
    "cw_batch_strands": (C.c_uint32, [C.c_void_p]),
    "cw_circuit_montgomery": (C.c_int, [C.c_void_p]),
    "cw_batch_pipelined": (C.c_uint32, [C.c_void_p]),
    "cw_batch_emitted": (C.c_uint32, [C.c_void_p]),
    "cw_batch_lanes": (C.c_uint32, [C.c_void_p]),
    "cw_batch_bitmode": (C.c_int, [C.c_void_p]),
    "cw_bits_info": (C.c_int, [C.c_void_p, C.c_void_p]),
    "cw_bits_r1cs_plan_stats": (C.c_int, [C.c_void_p, C.c_void_p]),
    "cw_device_bits": (C.c_void_p, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "cw_set_input_signal": (C.c_int, [C.c_void_p, C.c_uint32, C.c_char_p, C.c_uint32, C.c_char_p]),
    "cw_set_inputs_json": (C.c_int, [C.c_void_p, C.c_uint32, C.c_char_p]),
    "cw_set_inputs": (C.c_int, [C.c_void_p, C.c_void_p]),
    "cw_set_inputs_device": (C.c_int, [C.c_void_p, C.c_void_p]),
    "cw_set_inputs_n8": (C.c_int, [C.c_void_p, C.c_void_p]),
    "cw_set_inputs_device_n8": (C.c_int, [C.c_void_p, C.c_void_p]),
    "cw_set_inputs_bits": (C.c_int, [C.c_void_p, C.c_void_p]),
    "cw_set_inputs_bits_device": (C.c_int, [C.c_void_p, C.c_void_p]),
    "cw_set_inputs_rows": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32]),
    "cw_set_inputs_rows_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32]),
    "cw_set_inputs_range": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t, C.c_uint32]),
    "cw_set_inputs_range_device": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t, C.c_uint32]),
    "cw_set_input_column": (C.c_int, [C.c_void_p, C.c_char_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t, C.c_uint32]),
    "cw_set_input_column_device": (C.c_int, [C.c_void_p, C.c_char_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t, C.c_uint32]),
    "cw_inputs_missing": (C.c_int64, [C.c_void_p]),
    "cw_stream_witnesses_device": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cw_signal_slots": (C.POINTER(C.c_uint32), [C.c_void_p]),
    "cw_batch_signal_slots": (C.POINTER(C.c_uint32), [C.c_void_p]),
    "cw_batch_bits_layout": (C.c_int, [C.c_void_p, C.c_void_p]),
    "cw_get_staged_input": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_char_p]),
    "cw_remaining_inputs": (C.c_int64, [C.c_void_p, C.c_uint32]),
    "cw_run": (C.c_int, [C.c_void_p]),
    "cw_check_r1cs": (C.c_int, [C.c_void_p]),
    "cw_run_check": (C.c_int, [C.c_void_p]),
    "cw_batch_graph_captured": (C.c_int, [C.c_void_p]),
    "cw_emitted_checks_match": (C.c_int, [C.c_void_p]),
    "cw_batch_set_timing": (C.c_int, [C.c_void_p, C.c_int]),
    "cw_batch_kernel_ms": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "cw_batch_kernel_ms_mean": (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int)]),
    "cw_sync": (C.c_int, [C.c_void_p]),
    "cw_get_status": (C.c_int, [C.c_void_p, C.c_void_p]),
    "cw_get_witness": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p]),
    "cw_get_witnesses": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]),
    "cw_get_witnesses_device": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]),
    "cw_get_witnesses_device_n8": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]),
    "cw_element_bytes": (C.c_uint32, [C.c_void_p]),
    "cw_batch_call_lds": (C.c_uint32, [C.c_void_p]),
    "cw_get_public": (C.c_int, [C.c_void_p, C.c_void_p]),
    "cw_get_public_device": (C.c_int, [C.c_void_p, C.c_void_p]),
    "cw_get_witness_rows": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t, C.c_uint32, C.POINTER(C.c_uint32)]),
    "cw_get_witness_rows_device": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p]),
    "cw_get_signals_range": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t, C.c_uint32, C.POINTER(C.c_uint32)]),
    "cw_get_signals_range_device": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p]),
    "cw_sym_find": (C.c_int, [C.c_char_p, C.c_char_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "cw_get_signal": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_char_p]),
    "cw_write_wtns": (C.c_int, [C.c_void_p, C.c_uint32, C.c_char_p]),
    "cw_get_r1cs_first_bad": (C.c_int, [C.c_void_p, C.c_void_p]),
    "cw_get_r1cs_products": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]),
    "cw_get_r1cs_products_device": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]),
    "cw_select_instances": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(C.c_uint32)]),
    "cw_select_instances_device": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
    "cw_get_witnesses_at": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]),
    "cw_get_witnesses_at_n8": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p]),
    "cw_get_witnesses_at_device": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cw_get_witnesses_at_device_n8": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cw_get_wtns_digests": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]),
    "cw_get_wtns_digests_device": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]),
    "cw_compare_witnesses": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cw_compare_witnesses_n8": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cw_compare_witnesses_device": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cw_compare_witnesses_device_n8": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cw_compare_wtns": (C.c_int, [C.c_void_p, C.c_uint32, C.c_char_p, C.c_void_p]),
    "cw_compare_wtns_many": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_char_p, C.c_void_p, C.c_void_p]),
    "cw_write_wtns_many": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_char_p]),
    "cw_write_wtnsb": (C.c_int, [C.c_void_p, C.c_char_p]),
    "cw_set_witnesses": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]),
    "cw_set_witnesses_n8": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]),
    "cw_set_witnesses_device": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]),
    "cw_set_witnesses_device_n8": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]),
    "cw_read_wtns": (C.c_int, [C.c_void_p, C.c_uint32, C.c_char_p]),
    "cw_read_wtns_many": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_char_p]),
    "cw_witnesses_missing": (C.c_int64, [C.c_void_p]),
    "cw_explain": (C.c_int, [C.c_void_p, C.c_uint32, C.c_char_p, C.c_char_p, C.c_size_t]),
    "cw_n_log_statements": (C.c_uint32, [C.c_void_p]),
    "cw_get_log": (C.c_int64, [C.c_void_p, C.c_uint32, C.c_char_p, C.c_size_t]),
    "cw_r1cs_plan_stats": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]),
    "cw_r1cs_stream_plan": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cw_r1cs_products_plan": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cw_device_values": (C.c_void_p, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]),
    "cw_fp_mul_bench": (C.c_int, [C.c_char_p, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.POINTER(C.c_float)]),
    "cw_bits_eval_bench": (C.c_int, [C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32,
                                     C.c_uint32, C.c_uint32, C.POINTER(C.c_float)]),
    "cw_fp_op": (C.c_int, [C.c_char_p, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                           C.c_void_p, C.c_void_p]),
}


def lib():
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            raise CwError(-4, "HIP extension %s is not built (run __graft_entry__.build()); "
                              "there is no CPU fallback" % LIB_PATH)
        L = C.CDLL(str(LIB_PATH))
        for name, (res, args) in _SIGS.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def _chk(rc):
    if rc != 0:
        raise CwError(rc, lib().cw_last_error().decode())


def fe_to_bytes(values, n=None) -> bytes:
    return b"".join(int(v).to_bytes(32, "little") for v in values)


def bytes_to_ints(buf: bytes):
    return [int.from_bytes(buf[i:i + 32], "little") for i in range(0, len(buf), 32)]


class Circuit:
    def __init__(self, tape_path, dat_path=None, r1cs_path=None):
        h = C.c_void_p()
        enc = lambda p: None if p is None else os.fsencode(str(p))
        _chk(lib().cw_load(enc(tape_path), enc(dat_path), enc(r1cs_path), C.byref(h)))
        self.h = h
        L = lib()
        self.n_signals = L.cw_n_signals(h)
        self.emitted_checks_match = bool(L.cw_emitted_checks_match(h))    # False: the .r1cs is not the one the emitted checks were built from
        self.n_witness = L.cw_n_witness(h)
        self.n_inputs = L.cw_n_inputs(h)
        self.input_start = L.cw_input_start(h)
        self.n_constraints = L.cw_n_constraints(h)
        self.n_public = L.cw_n_public(h)
        self.n_rows = L.cw_n_rows(h)
        self.n_mmul = L.cw_n_mmul(h)
        self.montgomery = bool(L.cw_circuit_montgomery(h))     # the device value table holds x * 2^261 mod q
        buf = C.create_string_buffer(32)
        L.cw_prime(h, buf)
        self.q = int.from_bytes(buf.raw, "little")
        self.element_bytes = L.cw_element_bytes(h)              # n8 of the .wtns files: 8 for the 64-bit runtime, 32 otherwise

    def set_witness_list(self, signals):
        """egress of every batch created from now on hands out these signals (the witness of a simplified system: `--O1`,
        frontend/circom_simplify.py); evaluation and R1CS check stay on the full system"""
        arr = np.ascontiguousarray(signals, dtype=np.uint32)
        _chk(lib().cw_set_witness_list(self.h, arr.ctypes.data_as(C.POINTER(C.c_uint32)), len(arr)))
        self.n_witness = lib().cw_n_witness(self.h)

    def bits_info(self) -> dict:
        """shape of the bit-plane program ({} when the circuit has none)"""
        out = (C.c_uint64 * 8)()
        _chk(lib().cw_bits_info(self.h, out))
        if not out[0]:
            return {}
        return dict(zip(("vrows", "slots_per_group", "ring", "gate_lanes", "row_loads", "row_flushes", "cache"), [int(x) for x in out[1:8]]))

    def bits_r1cs_plan_stats(self) -> dict:
        out = (C.c_uint64 * 8)()
        _chk(lib().cw_bits_r1cs_plan_stats(self.h, out))
        return dict(zip(("trivial_rows", "lut_rows", "int_rows", "word_terms", "bit_blocks", "contiguous_blocks", "field_rows", "int_stream_words"),
                        [int(x) for x in out]))

    def input_size(self, name: str):
        start = C.c_uint32()
        n = lib().cw_input_size(self.h, name.encode(), C.byref(start))
        return (None, None) if n < 0 else (start.value, n)

    def close(self):
        if self.h:
            lib().cw_free(self.h)
            self.h = None

    def r1cs_plan_stats(self, batch: int = 65536, chunks: int = 0, entries: int = 0) -> dict:
        """Build + hazard-check the R1CS kernel's LDS staging plan on the host (no GPU needed)."""
        out = (C.c_uint64 * 8)()
        _chk(lib().cw_r1cs_plan_stats(self.h, batch, chunks, entries, out))
        keys = ("chunks", "loads", "terms", "filler_loads", "distinct_wires", "entries", "depth")
        return dict(zip(keys, [int(x) for x in out]))

    def r1cs_products_plan(self, bits: bool = False) -> dict:
        """The plan Batch.r1cs_products walks, in the order of the .r1cs file (host only; csrc/cw_r1cs_products.h):
        rowptr [3 n + 1], terms [n_terms][2] ({slot, coefficient id}; 64-bit runtime: [n_terms][4] {slot, 0, lo, hi}), ctab [ids][8]"""
        sizes = (C.c_uint64 * 4)()
        _chk(lib().cw_r1cs_products_plan(self.h, 1 if bits else 0, sizes, None, None, None))
        arrs = [np.zeros(int(sizes[k]), dtype=np.uint32) for k in range(3)]
        _chk(lib().cw_r1cs_products_plan(self.h, 1 if bits else 0, sizes, *[a.ctypes.data_as(C.c_void_p) for a in arrs]))
        return {"rowptr": arrs[0], "terms": arrs[1].reshape(-1, int(sizes[3])), "ctab": arrs[2].reshape(-1, 8)}

    def r1cs_stream_plan(self, terms_per_chunk: int = 192, no_bool: bool = False, no_fold: bool = False) -> dict:
        """The term stream of the default R1CS check kernel, as the batch uploads it (host only; csrc/cw_r1cs_plan.h)."""
        import numpy as np
        flags = (1 if no_bool else 0) | (2 if no_fold else 0)
        sizes = (C.c_uint64 * 8)()
        _chk(lib().cw_r1cs_stream_plan(self.h, terms_per_chunk, flags, sizes, None, None, None, None))
        arrs = [np.zeros(int(sizes[k]), dtype=np.uint32) for k in range(4)]
        _chk(lib().cw_r1cs_stream_plan(self.h, terms_per_chunk, flags, sizes, *[a.ctypes.data_as(C.c_void_p) for a in arrs]))
        return {"chunk": arrs[0].reshape(-1, 4), "terms": arrs[1].reshape(-1, 2), "row_orig": arrs[2], "ctab": arrs[3].reshape(-1, 8),
                "n_terms": int(sizes[4]), "n_folded": int(sizes[5]), "n_bitsel": int(sizes[6]), "n_chunks": int(sizes[7])}

    def batch(self, batch: int, device: int = 0, stream=None) -> "Batch":
        return Batch(self, batch, device, stream)


class Batch:
    def __init__(self, circuit: Circuit, batch: int, device: int = 0, stream=None):
        self.circuit = circuit
        self.n = batch
        h = C.c_void_p()
        _chk(lib().cw_batch_create(circuit.h, device, batch, C.c_void_p(stream or 0), C.byref(h)))
        self.h = h
        self.strands = lib().cw_batch_strands(h)
        pp = lib().cw_batch_pipelined(h)
        self.pipelined = (pp & 0xFF, pp >> 8) if pp else None     # (rows per batch, loads per batch) of the pipelined variant
        self.lanes = lib().cw_batch_lanes(h)
        em = lib().cw_batch_emitted(h)
        self.emitted = bool(em)              # the variant's rows run as emitted code (hip_elements/fpjit.py)
        self.fused_check = em == 2           # ... which also recomputes the R1CS rows it covers
        self.bitmode = bool(lib().cw_batch_bitmode(h))
        self.call_lds = lib().cw_batch_call_lds(h)      # 64-bit runtime: bytes of LDS per workgroup for function register windows (0: table / none)
        lay = (C.c_uint64 * 4)()
        _chk(lib().cw_batch_bits_layout(h, lay))
        # bit table of this batch: element (group g, slot s) = T[(((g >> sh) * slots + s) << sh) + (g & ((1 << sh) - 1))]
        self.bits_slots, self.bits_sh, self.bits_groups, self.jit = int(lay[0]), int(lay[1]), int(lay[2]), bool(lay[3])

    def bits_index(self, group: int, slot: int) -> int:
        """uint64 index of (group, slot) in the table behind cw_device_bits"""
        sh = self.bits_sh
        return (((group >> sh) * self.bits_slots + slot) << sh) + (group & ((1 << sh) - 1))

    def device_bits(self):
        """(device pointer, bytes, slots per group) of the bit table (cw_device_bits); taking it makes the next check_r1cs audit
        the whole table - the caller may have changed it"""
        nb, spg = C.c_uint64(), C.c_uint64()
        p = lib().cw_device_bits(self.h, C.byref(nb), C.byref(spg))
        return (int(p) if p else 0), int(nb.value), int(spg.value)

    def signal_slots(self) -> np.ndarray:
        p = lib().cw_batch_signal_slots(self.h)
        return np.ctypeslib.as_array(p, shape=(self.circuit.n_signals,)).copy() if p else None

    def close(self):
        if self.h:
            lib().cw_batch_free(self.h)
            self.h = None

    # -- inputs -------------------------------------------------------------------------------------
    def set_input_signal(self, instance: int, name: str, idx: int, value: int):
        _chk(lib().cw_set_input_signal(self.h, instance, name.encode(), idx, int(value).to_bytes(32, "little")))

    def set_inputs_json(self, instance: int, text: str):
        _chk(lib().cw_set_inputs_json(self.h, instance, text.encode()))

    def set_inputs(self, arr):
        """arr: uint8 array [batch, n_inputs, 32] (canonical LE) or a list of lists of ints."""
        if not isinstance(arr, np.ndarray):
            arr = np.frombuffer(b"".join(fe_to_bytes(row) for row in arr), dtype=np.uint8)
        arr = np.ascontiguousarray(arr, dtype=np.uint8)
        assert arr.size == self.n * self.circuit.n_inputs * 32, "input array has the wrong size"
        _chk(lib().cw_set_inputs(self.h, arr.ctypes.data_as(C.c_void_p)))

    def set_inputs_n8(self, arr):
        """the bulk form with the circuit's own element (cw_set_inputs_n8).  64-bit runtime: a uint64 array [batch, n_inputs] or a
        list of lists of ints below 2^64 (values >= p are reduced on the device); any other circuit: what set_inputs takes."""
        if self.circuit.element_bytes == 32:
            return self.set_inputs(arr)
        arr = np.ascontiguousarray(np.asarray(arr, dtype=np.uint64), dtype="<u8")
        assert arr.size == self.n * self.circuit.n_inputs, "input array has the wrong size"
        _chk(lib().cw_set_inputs_n8(self.h, arr.ctypes.data_as(C.c_void_p)))

    def set_inputs_bits(self, masks):
        """packed boolean inputs: uint64 [groups][n_inputs], bit i of masks[g][k] = input k of instance 64 g + i"""
        arr = np.ascontiguousarray(masks, dtype=np.uint64)
        assert arr.shape == ((self.n + 63) // 64, self.circuit.n_inputs), arr.shape
        _chk(lib().cw_set_inputs_bits(self.h, arr.ctypes.data_as(C.c_void_p)))

    def set_inputs_bits_device(self, dptr: int):
        _chk(lib().cw_set_inputs_bits_device(self.h, C.c_void_p(dptr)))

    def set_inputs_rows(self, arr, msb_first: bool = True):
        """boolean inputs as packed rows, every engine (cw_set_inputs_rows): a C-contiguous uint8 array [batch][>= ceil(n_inputs / 8)],
        row j = the inputs of instance j, input k = bit 7 - (k & 7) of byte k >> 3 (msb_first: np.unpackbits' order, a SHA-256
        message as it stands) or bit k & 7.  The row stride is the array's."""
        assert isinstance(arr, np.ndarray) and arr.dtype == np.uint8 and arr.ndim == 2, "a 2-D uint8 array"
        assert arr.flags["C_CONTIGUOUS"], "the rows must be C-contiguous"
        assert arr.shape[0] == self.n, arr.shape                      # (a row that is too short is the library's CW_EINVAL)
        _chk(lib().cw_set_inputs_rows(self.h, arr.ctypes.data_as(C.c_void_p), arr.shape[1], ROWS_MSB_FIRST if msb_first else 0))

    def set_inputs_rows_device(self, dptr: int, stride: int, msb_first: bool = True):
        """the same from device memory: 8-byte aligned, stride a multiple of 8 and >= 8 * ceil(n_inputs / 64); converted inside the
        call in stream order (cw_set_inputs_rows_device)"""
        _chk(lib().cw_set_inputs_rows_device(self.h, C.c_void_p(dptr), stride, ROWS_MSB_FIRST if msb_first else 0))

    def _column_rows(self, arr, elem_bytes):
        """(array kept alive, n, stride, elem_bytes) of the values of a column: [batch][n] of uint8 / uint16 / uint32 / uint64, or
        [batch][n][32] uint8 (32-byte little-endian values); one dimension less ([n], or [n][32] with elem_bytes=32) is the
        broadcast form, stride 0.  The row stride is the array's first stride (a view of a wider array keeps its padding); the
        values of a row are contiguous."""
        arr = np.asarray(arr)
        assert arr.dtype in (np.uint8, np.uint16, np.uint32, np.uint64), "uint8 / uint16 / uint32 / uint64 values"
        arr = arr.astype(arr.dtype.newbyteorder("<"), copy=False)
        wide = elem_bytes == 32 if elem_bytes is not None else (arr.dtype == np.uint8 and arr.ndim == 3)
        if wide:
            assert arr.dtype == np.uint8 and arr.ndim in (2, 3) and arr.shape[-1] == 32, "32-byte values: a trailing axis of 32 uint8"
            eb, dims = 32, arr.ndim - 1
        else:
            eb, dims = arr.dtype.itemsize, arr.ndim
            assert elem_bytes in (None, eb), "elem_bytes does not match the dtype"
        assert dims in (1, 2), "[n] (broadcast) or [batch][n] values"
        if dims == 1:
            arr = np.ascontiguousarray(arr)
            return arr, arr.shape[0], 0, eb
        assert arr.shape[0] == self.n, arr.shape
        n = arr.shape[1]
        dense = np.empty(arr.shape, dtype=arr.dtype).strides
        if arr.strides[1:] != dense[1:] or arr.strides[0] < n * eb:     # the values of a row are not contiguous, or rows overlap
            arr = np.ascontiguousarray(arr)
        return arr, n, arr.strides[0], eb

    def set_input_column(self, name: str, arr, idx0: int = 0, elem_bytes: int | None = None):
        """elements idx0 .. idx0 + n - 1 of input signal `name` for EVERY instance (cw_set_input_column).  arr: [batch][n] of
        uint8 / uint16 / uint32 / uint64, or [batch][n][32] uint8 for 32-byte little-endian values - the width comes from the
        dtype; a 1-D array of length n is the broadcast form (every instance takes the same n values; 32-byte values: [n][32]
        with elem_bytes=32).  A scalar signal is a column of n = 1."""
        arr, n, stride, eb = self._column_rows(arr, elem_bytes)
        ptr = arr.ctypes.data_as(C.c_void_p) if arr.size else C.cast(C.create_string_buffer(8), C.c_void_p)
        _chk(lib().cw_set_input_column(self.h, name.encode(), idx0, n, ptr, stride, eb))

    def set_input_column_device(self, name: str, dptr: int, n: int, stride: int, elem_bytes: int, idx0: int = 0):
        """the same from device memory: instance j's n values of elem_bytes at dptr + j * stride (stride 0: broadcast); dptr and
        stride multiples of elem_bytes (16 for 32-byte values).  Converted inside the call, in stream order: the buffer is free
        once the batch's stream has passed the call (cw_set_input_column_device)"""
        _chk(lib().cw_set_input_column_device(self.h, name.encode(), idx0, n, C.c_void_p(dptr), stride, elem_bytes))

    def set_inputs_range(self, k0: int, arr, elem_bytes: int | None = None):
        """inputs k0 .. k0 + n - 1 (main-input order) of every instance; arr as set_input_column takes it (cw_set_inputs_range)"""
        arr, n, stride, eb = self._column_rows(arr, elem_bytes)
        ptr = arr.ctypes.data_as(C.c_void_p) if arr.size else C.cast(C.create_string_buffer(8), C.c_void_p)
        _chk(lib().cw_set_inputs_range(self.h, k0, n, ptr, stride, eb))

    def set_inputs_range_device(self, k0: int, dptr: int, n: int, stride: int, elem_bytes: int):
        _chk(lib().cw_set_inputs_range_device(self.h, k0, n, C.c_void_p(dptr), stride, elem_bytes))

    def inputs_missing(self) -> int:
        """inputs no column has covered yet; -1 when the batch is not in the column state (cw_inputs_missing)"""
        return lib().cw_inputs_missing(self.h)

    def stream_witnesses_device(self, first: int, count: int, chunk: int, d_buf0: int, d_buf1: int, consume):
        """consume(first, count, d_chunk, stream) -> int, called once per chunk (cw_stream_witnesses_device)"""
        CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p)
        cb = CB(lambda user, f, n, ptr, st: int(consume(f, n, ptr, st) or 0))
        _chk(lib().cw_stream_witnesses_device(self.h, first, count, chunk, C.c_void_p(d_buf0), C.c_void_p(d_buf1), cb, None))

    def set_inputs_device(self, dptr: int):
        _chk(lib().cw_set_inputs_device(self.h, C.c_void_p(dptr)))

    def set_inputs_device_n8(self, dptr: int):
        """device image [batch][n_inputs][element_bytes], 8-byte aligned (cw_set_inputs_device_n8)"""
        _chk(lib().cw_set_inputs_device_n8(self.h, C.c_void_p(dptr)))

    def staged_input(self, instance: int, k: int) -> int:
        buf = C.create_string_buffer(32)
        _chk(lib().cw_get_staged_input(self.h, instance, k, buf))
        return int.from_bytes(buf.raw, "little")

    def remaining_inputs(self, instance: int) -> int:
        return lib().cw_remaining_inputs(self.h, instance)

    # -- witnesses in (64-bit runtime: check witnesses this batch did not compute) ------------------------
    def set_witnesses(self, rows, first: int = 0):
        """supply witnesses for the instances first .. first + len(rows): lists of ints or an array [count][n_witness] in
        witness-list order (cw_set_witnesses_n8 when the circuit's element is 8 bytes - values must be below 2^64 -, else
        cw_set_witnesses).  Values that are not canonical are stored reduced and flagged ST_BAD_WITNESS."""
        nw = self.circuit.n_witness
        if self.circuit.element_bytes == 8:
            arr = np.ascontiguousarray(np.asarray(rows, dtype=np.uint64), dtype="<u8").reshape(-1, nw)
            _chk(lib().cw_set_witnesses_n8(self.h, first, arr.shape[0], arr.ctypes.data_as(C.c_void_p)))
            return
        if not isinstance(rows, np.ndarray):
            rows = np.frombuffer(b"".join(fe_to_bytes(row) for row in rows), dtype=np.uint8)
        arr = np.ascontiguousarray(rows, dtype=np.uint8)
        assert arr.size % (nw * 32) == 0, "witness array has the wrong size"
        _chk(lib().cw_set_witnesses(self.h, first, arr.size // (nw * 32), arr.ctypes.data_as(C.c_void_p)))

    def set_witnesses_device(self, first: int, count: int, dptr: int):
        """device image [count][n_witness][32], 16-byte aligned, read in stream order inside the call (cw_set_witnesses_device)"""
        _chk(lib().cw_set_witnesses_device(self.h, first, count, C.c_void_p(dptr)))

    def set_witnesses_device_n8(self, first: int, count: int, dptr: int):
        """device image [count][n_witness][8], 8-byte aligned (cw_set_witnesses_device_n8)"""
        _chk(lib().cw_set_witnesses_device_n8(self.h, first, count, C.c_void_p(dptr)))

    def read_wtns(self, instance: int, path):
        _chk(lib().cw_read_wtns(self.h, instance, os.fsencode(str(path))))

    def read_wtns_many(self, first: int, count: int, pattern):
        """`pattern`: one %u / %d = the instance number, as write_wtns_many"""
        _chk(lib().cw_read_wtns_many(self.h, first, count, os.fsencode(str(pattern))))

    def witnesses_missing(self) -> int:
        """instances not supplied yet; -1 when the batch is not in the supplied state"""
        return lib().cw_witnesses_missing(self.h)

    # -- compute ------------------------------------------------------------------------------------
    def run(self):
        _chk(lib().cw_run(self.h))

    def check_r1cs(self):
        _chk(lib().cw_check_r1cs(self.h))

    def run_check(self):
        """run() + check_r1cs() as one launch: captured as a HIP graph on the second call, replayed afterwards (cw_run_check)"""
        _chk(lib().cw_run_check(self.h))

    @property
    def graph_captured(self) -> bool:
        return bool(lib().cw_batch_graph_captured(self.h))

    def sync(self):
        _chk(lib().cw_sync(self.h))

    def set_timing(self, on=True):
        """HIP events around the parts of run() / check_r1cs() on this batch's stream (cw_batch_set_timing)"""
        _chk(lib().cw_batch_set_timing(self.h, 2 if on == "history" else 1 if on else 0))

    def kernel_ms(self):
        """{"ingest": ms, "eval": ms, "check": ms} of the last run / check (None: that part has not run); drains the stream"""
        out = (C.c_float * 3)()
        _chk(lib().cw_batch_kernel_ms(self.h, out))
        return {k: (float(v) if v >= 0 else None) for k, v in zip(("ingest", "eval", "check"), out)}

    def kernel_ms_mean(self):
        """the same parts averaged over every run since set_timing("history") (cw_batch_kernel_ms_mean): ({part: ms | None},
        {part: runs averaged over})"""
        out, cnt = (C.c_float * 3)(), (C.c_int * 3)()
        _chk(lib().cw_batch_kernel_ms_mean(self.h, out, cnt))
        names = ("ingest", "eval", "check")
        return {k: (float(v) if v >= 0 else None) for k, v in zip(names, out)}, {k: int(n) for k, n in zip(names, cnt)}

    # -- results ------------------------------------------------------------------------------------
    def status(self) -> np.ndarray:
        out = np.zeros(self.n, dtype=np.uint32)
        _chk(lib().cw_get_status(self.h, out.ctypes.data_as(C.c_void_p)))
        return out

    def r1cs_first_bad(self) -> np.ndarray:
        out = np.zeros(self.n, dtype=np.uint32)
        _chk(lib().cw_get_r1cs_first_bad(self.h, out.ctypes.data_as(C.c_void_p)))
        return out

    def r1cs_products(self, parts: int = R1CS_A | R1CS_B, row0: int = 0, n_rows: int | None = None, first: int = 0,
                      count: int | None = None) -> np.ndarray:
        """A.w, B.w, C.w of the constraints [row0, row0 + n_rows) of the .r1cs file for the instances [first, first + count), every
        engine (cw_get_r1cs_products): uint8 [count][P][n_rows][element_bytes], P = the parts of `parts` (R1CS_A | R1CS_B | R1CS_C)
        in the order A, B, C, canonical little-endian residues"""
        n_rows = self.circuit.n_constraints - row0 if n_rows is None else n_rows
        count = self.n - first if count is None else count
        n_sel = bin(parts & 7).count("1")
        out = np.zeros((max(count, 0), n_sel, max(n_rows, 0), self.circuit.element_bytes), dtype=np.uint8)
        # (an empty array has no address worth passing: the library refuses a null pointer before it looks at the ranges)
        ptr = out.ctypes.data_as(C.c_void_p) if out.size else C.cast(C.create_string_buffer(8), C.c_void_p)
        _chk(lib().cw_get_r1cs_products(self.h, parts, row0, n_rows, first, count, ptr))
        return out

    def r1cs_products_device(self, parts: int, row0: int, n_rows: int, first: int, count: int, d_ptr: int) -> None:
        """the same into device memory: [count][P][n_rows][element_bytes] at d_ptr, aligned to 8 bytes (64-bit runtime) or 16;
        asynchronous on the batch's stream (cw_get_r1cs_products_device)"""
        _chk(lib().cw_get_r1cs_products_device(self.h, parts, row0, n_rows, first, count, C.c_void_p(d_ptr)))

    # -- instance lists: select by status on the device, egress by index ------------------------------------
    def select(self, mask: int = 0xFFFFFFFF, want: int = 0) -> np.ndarray:
        """the instances whose status word satisfies (status & mask) == want, ascending, uint32 (cw_select_instances); the
        defaults select the clean instances, mask = want = ST_R1CS_FAILED those that failed the check"""
        idx = np.zeros(self.n, dtype=np.uint32)
        n = C.c_uint32(0)
        _chk(lib().cw_select_instances(self.h, mask & 0xFFFFFFFF, want & 0xFFFFFFFF, idx.ctypes.data_as(C.c_void_p), C.byref(n)))
        return idx[:n.value].copy()

    def select_device(self, mask: int, want: int, d_idx: int, d_n: int) -> None:
        """the same into device memory: d_idx has room for `batch` uint32, d_n is one uint32, both 4-byte aligned; asynchronous on
        the batch's stream (cw_select_instances_device)"""
        _chk(lib().cw_select_instances_device(self.h, mask & 0xFFFFFFFF, want & 0xFFFFFFFF, C.c_void_p(d_idx), C.c_void_p(d_n)))

    def witnesses_at(self, idx, entry0: int = 0, n: int | None = None) -> np.ndarray:
        """uint8 [len(idx)][n][32]: entries [entry0, entry0 + n) of the witness list of the instances idx[j], in the list's order
        (any order, repeats allowed), canonical little-endian (cw_get_witnesses_at); n=None: up to the end of the witness"""
        idx = np.ascontiguousarray(idx, dtype=np.uint32).reshape(-1)
        n = self.circuit.n_witness - entry0 if n is None else n
        out = np.zeros((len(idx), max(n, 0), 32), dtype=np.uint8)
        # (an empty array has no address worth passing: the library refuses a null pointer before it looks at the ranges)
        spare = C.create_string_buffer(8)
        ptr = out.ctypes.data_as(C.c_void_p) if out.size else C.cast(spare, C.c_void_p)
        iptr = idx.ctypes.data_as(C.c_void_p) if idx.size else C.cast(spare, C.c_void_p)
        _chk(lib().cw_get_witnesses_at(self.h, entry0, n, iptr, len(idx), ptr))
        return out

    def witnesses_at_device(self, d_idx: int, n_idx: int, d_out: int, entry0: int = 0, n: int | None = None, d_n_idx: int | None = None,
                            d_bad: int | None = None, n8: bool = False) -> None:
        """the same from a device list into device memory: [n_idx][n][32] at d_out (16-byte aligned), or, n8=True,
        [n_idx][n][circuit.element_bytes].  d_n_idx: device address of a uint32, the list ends at min(n_idx, that) - the d_n of
        select_device; d_bad: device address of a uint32 that takes the lowest position whose index is out of the batch (its row
        is zeros) or 0xFFFFFFFF.  Launched inside the call, in stream order (cw_get_witnesses_at_device(_n8))"""
        n = self.circuit.n_witness - entry0 if n is None else n
        fn = lib().cw_get_witnesses_at_device_n8 if n8 else lib().cw_get_witnesses_at_device
        _chk(fn(self.h, entry0, n, C.c_void_p(d_idx), n_idx, C.c_void_p(d_n_idx) if d_n_idx else None, C.c_void_p(d_out),
                C.c_void_p(d_bad) if d_bad else None))

    def witness_bytes(self, instance: int) -> bytes:
        out = np.zeros(self.circuit.n_witness * 32, dtype=np.uint8)
        _chk(lib().cw_get_witness(self.h, instance, out.ctypes.data_as(C.c_void_p)))
        return out.tobytes()

    def witness(self, instance: int):
        return bytes_to_ints(self.witness_bytes(instance))

    def public_signals(self) -> np.ndarray:
        """[batch][n_public][32] uint8: outputs then public inputs of main, for every instance."""
        out = np.zeros((self.n, self.circuit.n_public, 32), dtype=np.uint8)
        _chk(lib().cw_get_public(self.h, out.ctypes.data_as(C.c_void_p)))
        return out

    def public_signals_device(self, d_ptr: int) -> None:
        """Same, written to device memory at `d_ptr` (batch * n_public * 32 bytes)."""
        _chk(lib().cw_get_public_device(self.h, C.c_void_p(d_ptr)))

    def witness_rows(self, entry0: int, n: int, first: int = 0, count: int | None = None, msb_first: bool = True):
        """witness bits as packed rows, every engine (cw_get_witness_rows): (uint8 array [count][ceil(n / 8)], word).  Row j =
        instance first + j, entry entry0 + k of the witness list = bit 7 - (k & 7) of byte k >> 3 (msb_first: np.packbits' order,
        a SHA-256 digest as it stands) or bit k & 7; the bit is 1 iff the value is 1.  word: 0xFFFFFFFF, or the lowest instance
        of the range that held a value other than 0 and 1 (its bit is 0)."""
        count = self.n - first if count is None else count
        out = np.zeros((count, (n + 7) // 8), dtype=np.uint8)
        word = C.c_uint32(0)
        # (an empty array has no address worth passing: the library refuses a null pointer before it looks at the range)
        ptr = out.ctypes.data_as(C.c_void_p) if out.size else C.cast(C.byref(word), C.c_void_p)
        _chk(lib().cw_get_witness_rows(self.h, entry0, n, first, count, ptr, out.shape[1], ROWS_MSB_FIRST if msb_first else 0, C.byref(word)))
        return out, word.value

    def witness_rows_device(self, entry0: int, n: int, first: int, count: int, d_ptr: int, stride: int, msb_first: bool = True,
                            d_not_boolean: int = 0) -> None:
        """the same into device memory: d_ptr 8-byte aligned, stride a multiple of 8 and >= 8 * ceil(n / 64), 8 * ceil(n / 64)
        bytes per row written, pad bits 0; d_not_boolean: 0 or the 4-byte aligned device address of the word; asynchronous on the
        batch's stream (cw_get_witness_rows_device)"""
        _chk(lib().cw_get_witness_rows_device(self.h, entry0, n, first, count, C.c_void_p(d_ptr), stride, ROWS_MSB_FIRST if msb_first else 0,
                                              C.c_void_p(d_not_boolean) if d_not_boolean else None))

    def signals_range(self, signal0: int, n: int, first: int = 0, count: int | None = None, elem_bytes: int = 32):
        """signal columns out, every engine (cw_get_signals_range): ([count][n] array of uint8 / uint16 / uint32 / uint64, or
        [count][n][32] uint8 for elem_bytes = 32; word).  Row j = instance first + j, value k = signal signal0 + k (a signal id,
        whether the witness list names it or not), the canonical residue narrowed to elem_bytes little-endian bytes.  word:
        0xFFFFFFFF, or the lowest instance of the range that held a value >= 2 ** (8 * elem_bytes) (its low bytes are stored)."""
        count = self.n - first if count is None else count
        dt = {1: np.uint8, 2: np.dtype("<u2"), 4: np.dtype("<u4"), 8: np.dtype("<u8")}.get(elem_bytes, np.uint8)
        out = np.zeros((count, n, 32) if elem_bytes == 32 else (count, n), dtype=dt)
        word = C.c_uint32(0)
        # (an empty array has no address worth passing: the library refuses a null pointer before it looks at the range)
        ptr = out.ctypes.data_as(C.c_void_p) if out.size else C.cast(C.byref(word), C.c_void_p)
        _chk(lib().cw_get_signals_range(self.h, signal0, n, first, count, ptr, n * elem_bytes, elem_bytes, C.byref(word)))
        return out, word.value

    def signals_range_device(self, signal0: int, n: int, first: int, count: int, d_ptr: int, stride: int, elem_bytes: int = 32,
                             d_too_wide: int = 0) -> None:
        """the same into device memory: row j at d_ptr + j * stride, d_ptr and stride multiples of elem_bytes (of 16 for 32), only
        the n * elem_bytes bytes of a row are written; d_too_wide: 0 or the 4-byte aligned device address of the word;
        asynchronous on the batch's stream (cw_get_signals_range_device)"""
        _chk(lib().cw_get_signals_range_device(self.h, signal0, n, first, count, C.c_void_p(d_ptr), stride, elem_bytes,
                                               C.c_void_p(d_too_wide) if d_too_wide else None))

    def public_rows(self, msb_first: bool = True):
        """entries 1 .. n_public of every instance as packed rows: (uint8 [batch][ceil(n_public / 8)], word).  msb_first=False is
        exactly the layout sharding.pack_bit_rows makes of the 32-byte image; for a Sha256(n) circuit the first 32 bytes of a row
        with msb_first=True are the digest"""
        return self.witness_rows(1, self.circuit.n_public, 0, self.n, msb_first)

    def witnesses(self, first: int = 0, count: int | None = None) -> np.ndarray:
        """[count][n_witness][32] uint8, canonical little-endian values (bulk egress, one device transpose)."""
        count = self.n - first if count is None else count
        out = np.zeros((count, self.circuit.n_witness, 32), dtype=np.uint8)
        _chk(lib().cw_get_witnesses(self.h, first, count, out.ctypes.data_as(C.c_void_p)))
        return out

    def witnesses_device(self, first: int, count: int, d_ptr: int) -> None:
        """canonical values of `count` instances written to device memory at d_ptr ([count][n_witness][32])"""
        _chk(lib().cw_get_witnesses_device(self.h, first, count, C.c_void_p(d_ptr)))

    def witnesses_device_n8(self, first: int, count: int, d_ptr: int) -> None:
        """the same with the element of the .wtns files ([count][n_witness][circuit.element_bytes]): 8 bytes per value for
        circuits of the 64-bit runtime, witnesses_device for every other"""
        _chk(lib().cw_get_witnesses_device_n8(self.h, first, count, C.c_void_p(d_ptr)))

    def wtns_digests(self, first: int = 0, count: int | None = None) -> np.ndarray:
        """uint8 [count][32]: hashlib.sha256(the bytes write_wtns(first + j, ..) would write).digest() of every instance of the
        range, computed on the device (cw_get_wtns_digests); no witness leaves it"""
        count = self.n - first if count is None else count
        out = np.zeros((max(count, 0), 32), dtype=np.uint8)
        # (an empty array has no address worth passing: the library refuses a null pointer before it looks at the range)
        ptr = out.ctypes.data_as(C.c_void_p) if out.size else C.cast(C.create_string_buffer(8), C.c_void_p)
        _chk(lib().cw_get_wtns_digests(self.h, first, count, ptr))
        return out

    def wtns_digests_device(self, first: int, count: int, dptr: int) -> None:
        """the same into device memory: [count][32] at dptr, 16-byte aligned; asynchronous on the batch's stream
        (cw_get_wtns_digests_device)"""
        _chk(lib().cw_get_wtns_digests_device(self.h, first, count, C.c_void_p(dptr)))

    def compare_witnesses(self, image, entry0: int = 0, first: int = 0):
        """an image of witnesses against the batch, on the device (cw_compare_witnesses(_n8)): image is uint8 [count][n][eb], eb =
        32 or circuit.element_bytes, image[j][k] = entry entry0 + k of instance first + j.  Returns (diff, n_diff, lowest): diff
        uint32 [count], the lowest entry whose bytes differ from what the egress would write or 0xFFFFFFFF; n_diff the instances
        that differ; lowest the first of them (first + j) or 0xFFFFFFFF"""
        image = np.ascontiguousarray(image, dtype=np.uint8)
        if image.ndim != 3 or image.shape[2] not in (32, self.circuit.element_bytes):
            raise ValueError("image must be [count][n][32] or [count][n][element_bytes] bytes")
        count, n, eb = image.shape
        diff = np.zeros(count, dtype=np.uint32)
        summary = np.zeros(2, dtype=np.uint32)
        # (an empty array has no address worth passing: the library refuses a null pointer before it looks at the ranges)
        spare = C.create_string_buffer(8)
        iptr = image.ctypes.data_as(C.c_void_p) if image.size else C.cast(spare, C.c_void_p)
        dptr = diff.ctypes.data_as(C.c_void_p) if diff.size else C.cast(spare, C.c_void_p)
        fn = lib().cw_compare_witnesses if eb == 32 else lib().cw_compare_witnesses_n8
        _chk(fn(self.h, entry0, n, first, count, iptr, dptr, summary.ctypes.data_as(C.c_void_p)))
        return diff, int(summary[0]), int(summary[1])

    def compare_witnesses_device(self, d_image: int, d_diff: int, first: int, count: int, entry0: int = 0, n: int | None = None,
                                 d_summary: int | None = None, n8: bool = False) -> None:
        """the same from device memory into device memory: [count][n][32] at d_image (16-byte aligned) or, n8=True,
        [count][n][circuit.element_bytes]; d_diff: count uint32; d_summary: 0 / None or the address of two uint32.  The call fills
        and writes both itself, in stream order; asynchronous on the batch's stream (cw_compare_witnesses_device(_n8))"""
        n = self.circuit.n_witness - entry0 if n is None else n
        fn = lib().cw_compare_witnesses_device_n8 if n8 else lib().cw_compare_witnesses_device
        _chk(fn(self.h, entry0, n, first, count, C.c_void_p(d_image), C.c_void_p(d_diff), C.c_void_p(d_summary) if d_summary else None))

    def compare_wtns(self, instance: int, path) -> int:
        """one .wtns file against instance `instance`: the lowest differing entry or 0xFFFFFFFF (cw_compare_wtns); a file that is
        not the circuit's raises CwError (CW_EIO) with the path and the reason"""
        diff = C.c_uint32(0)
        _chk(lib().cw_compare_wtns(self.h, instance, os.fsencode(str(path)), C.byref(diff)))
        return diff.value

    def compare_wtns_many(self, first: int, count: int, pattern: str):
        """the files pattern % (first + j) against the instances of the range (cw_compare_wtns_many): (diff, n_diff, lowest) as
        compare_witnesses returns them"""
        diff = np.zeros(max(count, 0), dtype=np.uint32)
        summary = np.zeros(2, dtype=np.uint32)
        dptr = diff.ctypes.data_as(C.c_void_p) if diff.size else C.cast(C.create_string_buffer(8), C.c_void_p)
        _chk(lib().cw_compare_wtns_many(self.h, first, count, os.fsencode(str(pattern)), dptr, summary.ctypes.data_as(C.c_void_p)))
        return diff, int(summary[0]), int(summary[1])

    def device_values(self):
        """(device pointer, bytes, padded batch) of the value table (cw_device_values; layout: include/circom_amd.h)"""
        n, bp = C.c_uint64(), C.c_uint32()
        p = lib().cw_device_values(self.h, C.byref(n), C.byref(bp))
        return p, n.value, bp.value

    def signal(self, instance: int, slot: int) -> int:
        buf = C.create_string_buffer(32)
        _chk(lib().cw_get_signal(self.h, instance, slot, buf))
        return int.from_bytes(buf.raw, "little")

    def write_wtns_many(self, first: int, count: int, pattern: str):
        _chk(lib().cw_write_wtns_many(self.h, first, count, os.fsencode(str(pattern))))

    def write_wtnsb(self, path):
        """the whole batch as one compact container (circom_amd/wtnsb.py reads / expands it)"""
        _chk(lib().cw_write_wtnsb(self.h, os.fsencode(str(path))))

    def explain(self, instance: int, sym_path=None) -> str:
        buf = C.create_string_buffer(1 << 16)
        _chk(lib().cw_explain(self.h, instance, None if sym_path is None else os.fsencode(str(sym_path)), buf, len(buf)))
        return buf.value.decode()

    def write_wtns(self, instance: int, path, witness2signal=None):
        """witness2signal: the kept signals of a simplified constraint system (`--O1`: frontend/circom_simplify.py, the
        `<name>.w2s` file of the driver): the file then holds the witness of THAT system - the entries of the full witness at
        these positions, which is what the reference binary writes when its `.dat` carries the list (main.cpp:288-334)"""
        _chk(lib().cw_write_wtns(self.h, instance, os.fsencode(str(path))))
        if witness2signal is not None:
            from .frontend.circom_simplify import reduce_wtns
            with open(path, "rb") as f:
                full = f.read()
            with open(path, "wb") as f:
                f.write(reduce_wtns(full, witness2signal))

    def log(self, instance: int) -> str:
        """what the reference binary prints on stdout for this instance (its log(...) statements)"""
        n = lib().cw_get_log(self.h, instance, None, 0)
        if n < 0:
            _chk(int(n))
        buf = C.create_string_buffer(int(n) + 1)
        n = lib().cw_get_log(self.h, instance, buf, len(buf))
        if n < 0:
            _chk(int(n))
        return buf.value.decode()


def sym_find(sym_path, name: str):
    """(signal0, n): the run of signal ids a .sym file lists under `name` - the name itself, its elements name[..] and its
    members name.x - as cw_get_signals_range takes it (cw_sym_find; host-only, no batch needed)"""
    s0, n = C.c_uint32(0), C.c_uint32(0)
    _chk(lib().cw_sym_find(os.fspath(sym_path).encode(), name.encode(), C.byref(s0), C.byref(n)))
    return s0.value, n.value


def fp_mul_bench(q: int, a: np.ndarray, b: np.ndarray, iters: int, device: int = 0):
    """a, b: uint8 [n,32].  Returns (out uint8 [n,32], milliseconds)."""
    n = a.shape[0]
    out = np.zeros_like(a)
    ms = C.c_float()
    _chk(lib().cw_fp_mul_bench(q.to_bytes(32, "little"), device, n, iters, a.ctypes.data_as(C.c_void_p),
                               b.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), C.byref(ms)))
    return out, ms.value


def fp_op(q: int, dop: int, a, b, c, device: int = 0):
    """Element-wise device op on lists of ints; returns (list of ints, status array)."""
    n = len(a)
    A = np.frombuffer(fe_to_bytes(a), dtype=np.uint8)
    B = np.frombuffer(fe_to_bytes(b), dtype=np.uint8)
    Cc = np.frombuffer(fe_to_bytes(c), dtype=np.uint8)
    out = np.zeros(n * 32, dtype=np.uint8)
    st = np.zeros(n, dtype=np.uint32)
    _chk(lib().cw_fp_op(q.to_bytes(32, "little"), device, dop, n, A.ctypes.data_as(C.c_void_p),
                        B.ctypes.data_as(C.c_void_p), Cc.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p),
                        st.ctypes.data_as(C.c_void_p)))
    return bytes_to_ints(out.tobytes()), st
