/* circom_amd.h — C ABI of the MI355X-native batched witness calculator for circom circuits.
 *
 * Drop-in boundary.  circom has no plugin registry; the emitted C++ calculator is
 * reached through four concrete seams.  Each entry point below names the reference interface it
 * replaces (paths relative to the iden3/circom tree, v2.2.3):
 *
 *   seam 3 (runtime)   code_producers/src/c_elements/common/calcwit.hpp:17-66  class Circom_CalcWit
 *                      code_producers/src/c_elements/common/circom.hpp:36-43,79-87  Circom_Circuit + get_*()
 *   seam 4 (process)   code_producers/src/c_elements/common/main.cpp:22-124 loadCircuit,
 *                      :243-286 loadJson, :288-334 writeBinWitness, :336-373 main
 *
 * Differences forced by batching: one `cw_batch` holds B independent instances (the reference runs one
 * process per input); a failed `===`/assert does not abort (assert_bucket.rs:75-77) but is reported in
 * the per-instance status word; everything is plain pointers + sizes, caller owns host buffers, the
 * library owns device memory.  All functions return 0 on success or a negative CW_E* code;
 * cw_last_error() gives the message (thread-local).  No function is thread-safe on the same handle.
 */
#ifndef CIRCOM_AMD_H
#define CIRCOM_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CW_OK 0
#define CW_EIO (-1)        /* file missing / unreadable / malformed */
#define CW_EINVAL (-2)     /* bad argument */
#define CW_EINPUT (-3)     /* input error: signal not found / assigned twice / wrong count (calcwit.cpp:51-97) */
#define CW_EDEVICE (-4)    /* HIP error */
#define CW_ESTATE (-5)     /* call out of order (e.g. run before all inputs are set) */

typedef struct cw_circuit cw_circuit; /* replaces Circom_Circuit (circom.hpp:36-43) + compiled-in tables */
typedef struct cw_batch cw_batch;     /* replaces Circom_CalcWit (calcwit.hpp:17-66), x B instances */

/* instance status word (cw_get_status) */
#define CW_ST_OK 0u
#define CW_ST_ASSERT_FAILED 1u /* a `===` / assert() did not hold */
#define CW_ST_ARITH 2u         /* `\` or `%` by zero (reference: GMP abort, generic/fr.cpp:2835-2875), run-away function */
/* bits 8..31 of a word with bit 0 or 1 set: index of the failing operation in the circuit's flat witness program.  When
   several checks of an instance fail, the one with the smallest index is reported whatever the schedule's row order and
   strand count - the check the reference's sequential program stops at (assert_bucket.rs:75-77, calcwit.cpp:104-114). */
#define CW_ST_R1CS_FAILED 4u   /* set by cw_check_r1cs */
#define CW_ST_BAD_WITNESS 8u   /* a SUPPLIED witness (cw_set_witnesses*, cw_read_wtns*) was malformed: a value that is not a canonical
                                  residue, or an entry 0 that is not 1.  Bits 4..7 are unused. */

const char *cw_last_error(void);
const char *cw_version(void);

/* ---- circuit (loadCircuit, main.cpp:22-124; the nine get_*() of circom.hpp:79-87) -------------- */
/* tape_path: <name>.cwt (hip_elements schedule); dat_path: <name>.dat (reference layout, hash map +
 * witness list are read from it; may be NULL -> taken from the tape); r1cs_path: <name>.r1cs or NULL. */
int cw_load(const char *tape_path, const char *dat_path, const char *r1cs_path, cw_circuit **out);
void cw_free(cw_circuit *c);
uint32_t cw_n_signals(const cw_circuit *c);          /* get_total_signal_no() */
/* get_size_of_io_map(): template instances of Mixed component clusters described in the .dat's io-map section
 * (c_code_generator.rs:681-738; Circom_Circuit::templateInsId2IOSignalInfo, circom.hpp:41), and the local offset of io
 * signal `signal_code` of one of them (-1: unknown).  The evaluator resolves every access at trace time; the table is
 * read, validated and exposed because the file format carries it. */
uint32_t cw_io_map_size(const cw_circuit *c);
int64_t cw_io_map_offset(const cw_circuit *c, uint32_t template_id, uint32_t signal_code);
/* get_size_of_bus_field_map(): bus instances described in the .dat's bus-field map (c_code_generator.rs:740-794;
 * Circom_Circuit::busInsId2FieldInfo, circom.hpp:42; reader main.cpp:95-121), and one field of one of them: its offset inside
 * the bus, the size of one element, the id of the field's own bus (0: a signal, as the reference writes it) and the number of
 * dimensions behind the first.  Read, validated and exposed because the file format carries it (CW_EINVAL: no such field). */
uint32_t cw_bus_map_size(const cw_circuit *c);
int cw_bus_field(const cw_circuit *c, uint32_t bus_id, uint32_t field, uint32_t *offset, uint32_t *size, uint32_t *field_bus_id,
                 uint32_t *n_lengths);
uint32_t cw_n_witness(const cw_circuit *c);          /* get_size_of_witness() */
uint32_t cw_n_inputs(const cw_circuit *c);           /* get_main_input_signal_no() */
/* The witness of a SIMPLIFIED constraint system (the reference's default --O1, constraint_list/src/constraint_simplification.rs,
 * keeps a subset of the signals; the emitted calculator writes those: witness2signal of the .dat, calcwit.hpp:54-56,
 * main.cpp:288-334).  `signals`: n strictly increasing signal ids starting with 0; the first 1 + cw_n_public entries stay as
 * they are.  Evaluation and R1CS check keep working on the full system cw_load was given; every egress of batches created
 * AFTER this call (cw_get_witness(es)(_device), cw_write_wtns(_many), cw_write_wtnsb) hands out these entries, and
 * cw_n_witness() returns n.  CW_EINVAL while any batch of the circuit is alive: a batch sizes its device images of the list
 * when it is created, so the list is fixed before the first cw_batch_create (or after the last cw_batch_free). */
int cw_set_witness_list(cw_circuit *c, const uint32_t *signals, uint32_t n);
/* 1 unless the .r1cs given to cw_load is NOT the constraint system the tape's emitted checks were built from (the tape records
 * CRC-32 and length of that file's constraint section): then the fused checks / covered rows / audit program are not used and
 * the stand-alone kernels check every row of the file that was loaded.  (No reference counterpart: its runtime never checks.) */
int cw_emitted_checks_match(const cw_circuit *c);
uint32_t cw_input_start(const cw_circuit *c);        /* get_main_input_signal_start() */
uint32_t cw_n_constraints(const cw_circuit *c);      /* from the .r1cs header, 0 if none loaded */
uint32_t cw_n_public(const cw_circuit *c);     /* nPubOut + nPubIn of the r1cs header */
uint64_t cw_n_rows(const cw_circuit *c);             /* schedule length */
uint64_t cw_n_mmul(const cw_circuit *c);             /* Montgomery multiplications per instance in the schedule */
void cw_prime(const cw_circuit *c, uint8_t le32[32]); /* Fr_q (fr.hpp) */
/* n8 of the circuit's .wtns files (writeBinWitness: the prime's byte length): 8 for circuits of the 64-bit runtime
 * (--prime goldilocks, common64/main.cpp), 32 otherwise */
uint32_t cw_element_bytes(const cw_circuit *c);
/* 64-bit runtime, circuits that call run-time functions (loops, branches, array indices that depend on values): bytes of LDS
 * per workgroup that hold the functions' register windows; 0 = the windows live in the value table, or the circuit has no such
 * function.  LDS is used when no function needs more than 10 registers - the largest window that never lowers the number of
 * resident waves; the measurements are in NOTES.md.  CW64_CALL_LDS=0 / 1 in the environment of cw_batch_create forces a
 * placement (1 is ignored above 128 registers: 64 KiB).  Both placements compute the same table. */
uint32_t cw_batch_call_lds(const cw_batch *b);
/* getInputSignalSize(h) (calcwit.cpp:99-102): size of input `name`, or -1 */
int64_t cw_input_size(const cw_circuit *c, const char *name, uint32_t *start_slot);

/* ---- batch (Circom_CalcWit ctor calcwit.cpp:26-45) -------------------------------------------------- */
/* device: HIP device ordinal; batch: number of instances; stream: a hipStream_t (as void*) all work of
 * this batch is enqueued on, NULL = the null stream.  device < 0 creates a host-only batch: inputs can be
 * staged and validated, every computing call fails with CW_EDEVICE (there is no CPU fallback). */
int cw_batch_create(cw_circuit *c, int device, uint32_t batch, void *stream, cw_batch **out);
void cw_batch_free(cw_batch *b);
uint32_t cw_batch_size(const cw_batch *b);
/* strands (waves cooperating on the same 64 instances) of the schedule variant picked for this batch */
uint32_t cw_batch_strands(const cw_batch *b);
/* 0, or (rows per batch | loads per batch << 8) when the batch runs the pipelined single-wave variant of the schedule
   (LDS result ring + load lists issued one batch ahead: hip_elements/pipe.py; CW_PIPE=0/1 overrides the choice) */
uint32_t cw_batch_pipelined(const cw_batch *b);
/* 1 when the rows of the picked variant run as EMITTED gfx950 code (hip_elements/fpjit.py: the counterpart of the reference's
   per-template C++, compiler/src/circuit_design/template.rs:174-474 - operand loads, a call of the operator's body and the
   stores of every row as straight-line code), 2 when that code also carries the R1CS check of the rows it covers (recomputed
   from the stored wires behind the rows that produce them; chosen for throughput-bound batches, CW_FP_FUSED=0/1 overrides;
   cw_check_r1cs then merges its findings and streams only the remaining rows), 0 when cw_eval_kernel interprets the rows.
   CW_FP_JIT=0 forces the interpreter. */
uint32_t cw_batch_emitted(const cw_batch *b);
/* instances per workgroup (64, 32 or 16) the evaluation kernel uses for this batch */
uint32_t cw_batch_lanes(const cw_batch *b);
/* 1 if this batch runs the bit-plane program (circuits whose signals are all boolean for 0/1 inputs: one bit per
 * signal per instance, replaces the short-int paths of the tagged FrElement, generic/fr.cpp:416-439,900-917);
 * instances whose inputs are not 0/1 are transparently re-run by the 256-bit schedule.  CW_BITS=0 disables it. */
int cw_batch_bitmode(const cw_batch *b);
/* shape of the circuit's bit-plane program: out = {present, vrows, bit-table slots per group of 64 instances, LDS ring
 * rows, gate lanes, row loads, row flushes, LDS cache rows} (all zero when the circuit has none) */
int cw_bits_info(const cw_circuit *c, uint64_t out[8]);
/* host-only: shape of the R1CS check plan over the bit table: out = {rows that hold by construction, LUT-class rows,
 * integer-class rows, terms read as whole 32-bit words, blocks of 8 single-bit terms, of which on 8 consecutive slots,
 * field-class rows, words of the integer-class stream} */
int cw_bits_r1cs_plan_stats(const cw_circuit *c, uint64_t out[8]);

/* setInputSignal(h, i, val) (calcwit.cpp:77-97) for one instance; `name` is hashed with FNV-1a
 * (calcwit.cpp:17-24).  val = canonical 32-byte little-endian value, reduced mod q by the caller. */
int cw_set_input_signal(cw_batch *b, uint32_t instance, const char *name, uint32_t idx, const uint8_t val[32]);
/* loadJson (main.cpp:243-286, value grammar json2FrElements :144-188, nesting qualify_input :221-241)
 * for one instance from JSON text. */
int cw_set_inputs_json(cw_batch *b, uint32_t instance, const char *json_text);
/* Bulk: all instances at once, [batch][n_inputs][32] canonical LE values in main-input slot order
 * (slot = cw_input_start() + k).  Marks every input of every instance as set. */
int cw_set_inputs(cw_batch *b, const uint8_t *le32);
/* Same, but `d_le32` is a DEVICE pointer (HBM-resident inputs; no host copy).  The buffer is read by cw_run (stream
 * order) and, in bit-plane batches, once more by the first cw_sync / getter after it - instances whose inputs are not 0/1
 * are re-run by the 256-bit schedule from these bytes - so it must stay unmodified until then. */
int cw_set_inputs_device(cw_batch *b, const void *d_le32);
/* The same two with the circuit's own element: [batch][n_inputs][cw_element_bytes] little-endian values.  For the 64-bit
 * runtime (--prime goldilocks) that is 8 bytes per value - what a Goldilocks prover holds; the 32-byte image is three
 * quarters zeros.  For circuits whose element is 32 bytes these ARE cw_set_inputs / cw_set_inputs_device.
 *   values     need not be canonical: a value >= p is reduced on the device (one subtraction), as Fr_str2element reduces what
 *              loadJson reads; the 32-byte forms reduce all four words the same way.  On a host-only batch the host form stages
 *              each value zero-extended to 32 bytes, unreduced (cw_get_staged_input).
 *   alignment  d_le8 must be 8-byte aligned (CW_EINVAL otherwise; the pointer is not touched before cw_run).  A 32-byte device
 *              image should be 16-byte aligned, as hipMalloc returns it: another address is served by the slower
 *              lane-per-instance kernel.
 *   lifetime   cw_set_inputs_n8 copies and synchronises before it returns; d_le8 is read by cw_run in stream order and
 *              must stay unmodified until that run has finished (the rule of cw_set_inputs_device).
 *   size       64-bit runtime: from CW64_INGEST_TILE_MIN inputs upwards (cw_host.cpp, a measured threshold), and always beyond
 *              65 535 inputs, both element sizes enter through one tiled transpose (cw64.hip cw64_transpose_in_kernel), which
 *              has no limit on the number of inputs.  Only a 32-byte image at an address that is no multiple of 16 is still
 *              limited to 65 535 inputs (CW_EDEVICE from cw_run).
 * Any other setter puts the batch back on the 32-byte form.  CW64_INGEST_TILED=0 / 1, read at cw_batch_create, forces the
 * lane-per-instance / the tiled kernel (A/B timing, tools/ubench_ingest64.py); beyond 65 535 inputs =0 is ignored, the
 * lane-per-instance kernel cannot hold such a circuit. */
int cw_set_inputs_n8(cw_batch *b, const void *le8);
int cw_set_inputs_device_n8(cw_batch *b, const void *d_le8);
/* Bit-plane batches (cw_batch_bitmode) only: PACKED boolean inputs, uint64 masks[groups][n_inputs], groups =
 * ceil(batch / 64), bit i of masks[g][k] = main input k of instance 64 g + i.  The reference reads one JSON number per
 * bit (main.cpp:243-286); the 32-byte-per-value bulk form moves 256 bytes per input BIT of a SHA-256 circuit, this form
 * one bit.  cw_set_inputs_bits copies from host memory; the _device form keeps reading the caller's device buffer
 * (same lifetime rule as cw_set_inputs_device).  CW_ESTATE for batches on the 256-bit schedule and for circuits of the
 * 64-bit runtime (--prime goldilocks) - the only entry points that runtime does not serve. */
int cw_set_inputs_bits(cw_batch *b, const uint64_t *masks);
int cw_set_inputs_bits_device(cw_batch *b, const void *d_masks);
/* Boolean inputs as packed ROWS, every engine: the bytes a caller holds.  Instance j's inputs are the first ceil(n_inputs / 8)
 * bytes of rows + j * stride; input k (main-input slot order, as in the other bulk forms) is bit k & 7 of byte k >> 3, or, with
 * CW_ROWS_MSB_FIRST, bit 7 - (k & 7): the order of numpy's unpackbits and the order in which circomlib's SHA-256 reads a message,
 * so a caller of a Sha256(n) circuit passes the messages themselves.  Bits past n_inputs and bytes of a row past
 * ceil(n_inputs / 8) are ignored; any other flag bit is CW_EINVAL; n_inputs == 0 is CW_OK.  Both calls mark every input of every
 * instance as set.  The masks above are the TRANSPOSE of this layout; here the device transposes.
 *   host form    any stride >= ceil(n_inputs / 8), any alignment; copies in pieces and synchronises before it returns.  On a
 *                host-only batch each bit is staged as a 32-byte value 0 / 1 (cw_get_staged_input returns the bit).
 *   device form  d_rows 8-byte aligned, stride a multiple of 8 and at least 8 * ceil(n_inputs / 64) - the last 8-byte word of a
 *                row lies inside the row -, CW_EINVAL otherwise (the pointer is not touched).  The conversion kernel is launched
 *                INSIDE the call, in stream order: the buffer may be reused once the batch's stream has passed the call - the rule
 *                of cw_set_witnesses_device, not the deferred one of cw_set_inputs_device.  A host-only batch answers CW_EDEVICE
 *                after the argument checks.
 *   engines      bit-plane batches: one tiled bit transpose (csrc/cw_bits.hip cw_bits_rows_to_masks_kernel) writes the batch's own
 *                masks, and the batch continues as after cw_set_inputs_bits_device.  64-bit runtime and 256-bit schedule: the bits
 *                are expanded to the batch's own image of values 0 / 1 (8 / 32 bytes each), which cw_run ingests as it ingests
 *                cw_set_inputs_n8 / cw_set_inputs - correct and simple, one value per bit; a caller who does not know which engine
 *                cw_batch_create picked can rely on this form.
 * Every call checks in this order: null / range / flags / alignment (CW_EINVAL), then the device. */
#define CW_ROWS_MSB_FIRST 1u
int cw_set_inputs_rows(cw_batch *b, const uint8_t *rows, size_t stride, uint32_t flags);
int cw_set_inputs_rows_device(cw_batch *b, const void *d_rows, size_t stride, uint32_t flags);
/* Input COLUMNS, every engine: one named signal (or a range of main inputs) for the WHOLE batch, from the array the caller
 * already holds per signal - leaf[batch], pathElements[batch][20], sig[batch][3] - in host or device memory.  The caller needs
 * neither the slot order nor an interleaved image, widens nothing itself, and updates one signal between two steps without
 * rebuilding the rest.  cw_set_inputs_range* name the inputs k0 .. k0 + n - 1 in main-input order (as in the bulk forms);
 * cw_set_input_column* name the elements idx0 .. idx0 + n - 1 of input signal `name`, the lookup of cw_set_input_signal and
 * cw_input_size.
 *   layout     instance j's values are the n little-endian unsigned integers of elem_bytes in {1, 2, 4, 8, 32} at
 *              values + j * stride.  stride == 0 is the BROADCAST form: every instance takes the same n values (a Merkle root, a
 *              public parameter).  Any other stride is at least n * elem_bytes; bytes of a row behind the n values are never read.
 *   values     widths 1 to 8 are canonical for every 4-limb prime.  64-bit runtime (--prime goldilocks): an 8-byte value >= p
 *              is reduced with one subtraction, as cw_set_inputs_n8 reduces it, and a 32-byte value over all four words.  Every
 *              other engine takes a 32-byte value by the rule of cw_set_inputs: canonical, reduced by the caller.
 *   target     the batch's own bulk image, [batch][n_inputs][element] with the element of 8 bytes on the 64-bit runtime and 32
 *              bytes otherwise, at [j][k0 + k].  cw_run ingests that image with the kernels it has (Montgomery conversion, tiled
 *              transpose, bit-plane ingest), so the calls are correct on every engine by construction; the instances of a
 *              bit-plane batch whose values are not 0 / 1 are re-run by the 256-bit schedule from those bytes, as after
 *              cw_set_inputs.  A bit-plane batch therefore pays 32 bytes per input BIT here and allocates batch * n_inputs * 32
 *              bytes with its first column: large boolean batches belong to cw_set_inputs_rows* and cw_set_inputs_bits*.
 *   state      the first range / column call on a batch whose inputs come from anything else opens the COLUMN STATE: nothing is
 *              covered.  Each call covers [k0, k0 + n) for every instance; covering an input again overwrites it (a bulk form:
 *              there is no "assigned twice").  cw_inputs_missing: the inputs no column has covered yet, -1 when the batch is not
 *              in the column state; cw_remaining_inputs(b, i) returns the same count for every i.  cw_run with inputs missing
 *              answers CW_ESTATE "Not all inputs have been set. N values missing over the batch", N = missing inputs x batch.
 *              The state SURVIVES cw_run and cw_run_check: a later step updates any subset of columns and the rest of the image
 *              stands.  The input key of cw_run_check's graph does not change, so a captured graph is replayed over the new
 *              values.  Every other setter ends the column state (the latest setter wins); a column call after it starts from
 *              empty coverage.
 *   lifetime   the rule of cw_set_inputs_rows*.  The device forms launch the conversion (csrc/cw_columns.hip.h cw_columns_kernel)
 *              INSIDE the call, in stream order: the buffer may be reused once the batch's stream has passed the call.  The host
 *              forms take any alignment, stage dense rows through a device buffer in pieces and synchronise before they return.
 *              A bit-plane batch that has run first waits for that run and collects the instances to re-run (what the first
 *              cw_sync / getter after cw_run does), since that step reads the image a column is about to change.
 *   checks     in this order: a null pointer, elem_bytes, a stride shorter than the row, and, device forms, d_values or a
 *              non-zero stride that is no multiple of elem_bytes (of 16 for 32-byte elements): CW_EINVAL - the pointer is never
 *              touched.  Then the name and the range: CW_EINPUT "Signal not found: <name>" / "Input signal array access exceeds
 *              the size" (idx0 + n beyond the signal); the range forms: k0 + n > cw_n_inputs is CW_EINVAL.  Then the device: a
 *              host-only batch answers CW_EDEVICE to the device forms.  n == 0 is CW_OK and covers nothing.
 *   host-only  the host forms stage each value into the staging image of the per-signal setters, zero-extended to 32 bytes and
 *              unreduced, for every instance: cw_get_staged_input returns it, cw_remaining_inputs falls by the cells that were
 *              not assigned before.  There is no column state on such a batch.
 *   not here   instance sub-ranges (a column always spans the batch); writing the value table or the packed masks directly;
 *              supplied witnesses (cw_set_witnesses*). */
int cw_set_inputs_range(cw_batch *b, uint32_t k0, uint32_t n, const void *values, size_t stride, uint32_t elem_bytes);
int cw_set_inputs_range_device(cw_batch *b, uint32_t k0, uint32_t n, const void *d_values, size_t stride, uint32_t elem_bytes);
int cw_set_input_column(cw_batch *b, const char *name, uint32_t idx0, uint32_t n, const void *values, size_t stride, uint32_t elem_bytes);
int cw_set_input_column_device(cw_batch *b, const char *name, uint32_t idx0, uint32_t n, const void *d_values, size_t stride,
                               uint32_t elem_bytes);
int64_t cw_inputs_missing(const cw_batch *b);
/* read back input k (slot cw_input_start()+k) of one instance as staged by the two per-signal setters */
int cw_get_staged_input(cw_batch *b, uint32_t instance, uint32_t k, uint8_t out[32]);
/* getRemaingInputsToBeSet() (calcwit.hpp:50-52) of one instance */
int64_t cw_remaining_inputs(const cw_batch *b, uint32_t instance);

/* run(ctx) (calcwit.cpp:6,71-75) for all instances: ingest + schedule evaluation, asynchronous on the
 * batch's stream.  Fails with CW_ESTATE if some instance still has unset inputs (main.cpp:352-355). */
int cw_run(cw_batch *b);
/* A*w o B*w = C*w over the loaded .r1cs for all instances (second kernel of the north-star). */
int cw_check_r1cs(cw_batch *b);
/* cw_run + cw_check_r1cs as one launch: the second call with unchanged input pointers captures the launches of both into a HIP graph
 * on the batch's stream, later calls replay it (a step of a small batch is a dozen kernel launches of microseconds each - the host
 * sets the pace otherwise).  Same results, same errors, same asynchrony as the two calls; falls back to them while timing marks are
 * on, while host-set inputs await their copy, with CW_NO_GRAPH set, or if the capture fails.  The graph is dropped when the
 * batch's input pointer changes or the caller takes the raw table pointer.  cw_batch_graph_captured: 1 once replaying.
 * (No reference counterpart: the reference's run + snarkjs' `wtns check` are two processes per witness.) */
int cw_run_check(cw_batch *b);
int cw_batch_graph_captured(const cw_batch *b);
/* Event timing of the parts of cw_run / cw_check_r1cs on the batch's stream (HIP events recorded where the kernels are launched;
 * no reference counterpart: the reference's runtime is one process per witness - this is what bench.py's roofline figures read).
 * cw_batch_kernel_ms drains the stream and returns, for the LAST run / check: ms[0] = table init + input ingest, ms[1] = the
 * evaluation kernel(s), ms[2] = the R1CS check; -1 for a part that has not run since timing was switched on. */
int cw_batch_set_timing(cw_batch *b, int on);
int cw_batch_kernel_ms(cw_batch *b, float ms[3]);
/* on = 2 keeps the marks of the last 64 runs of the batch; cw_batch_kernel_ms_mean averages each part over every run recorded
 * since (counts[k] = how many): the kernels' durations INSIDE a timed region, other batches in flight beside them - the figure
 * a rocprofv3 kernel-trace average of the same region reproduces. */
int cw_batch_kernel_ms_mean(cw_batch *b, float ms[3], int counts[3]);
int cw_sync(cw_batch *b);

/* results (synchronise the stream first) */
int cw_get_status(cw_batch *b, uint32_t *status /* [batch] */);
/* getWitness(i) + Fr_toLongNormal for all witness positions (main.cpp:326-332): [n_witness][32] */
int cw_get_witness(cw_batch *b, uint32_t instance, uint8_t *out);
/* bulk form for provers: `count` instances from `first`, [count][n_witness][32], one device-side transpose */
int cw_get_witnesses(cw_batch *b, uint32_t first, uint32_t count, uint8_t *out);
/* the same to DEVICE memory (no host copy): what a GPU prover consumes.  Asynchronous on the batch's stream, except that
 * the first egress after a cw_run of a bit-plane batch waits for the evaluation (it has to know which instances were
 * re-run by the 256-bit schedule; every egress serves those from there). */
int cw_get_witnesses_device(cw_batch *b, uint32_t first, uint32_t count, void *d_out);
/* the same with the element of the circuit's .wtns files: [count][n_witness][cw_element_bytes], canonical little-endian.
 * For the 64-bit runtime that is 8 bytes per value - what a Goldilocks prover reads; the 32-byte image is three quarters
 * zeros.  Same state and range checks; for circuits whose element is 32 bytes it IS cw_get_witnesses_device.
 * 64-bit runtime: both forms are one tiled transpose (cw64.hip cw64_egress_kernel; d_out of the 32-byte form should be
 * 16-byte aligned, as hipMalloc returns it - another address is served by the slower per-entry gather). */
int cw_get_witnesses_device_n8(cw_batch *b, uint32_t first, uint32_t count, void *d_out);
/* chunked form: `chunk` instances at a time into d_buf0 / d_buf1 in turn ([chunk][n_witness][32] each, every engine); `consume` is called
 * after each chunk's transpose has been enqueued on the batch's stream (passed as `stream`, a hipStream_t): work enqueued
 * there sees the chunk complete and orders the library's next write to that buffer behind itself.  Non-zero return of
 * `consume` aborts with CW_ESTATE.  (writeBinWitness's loop over getWitness(i), main.cpp:326-332, for a consumer that
 * cannot hold B x 32 MB.)  Size the chunk generously where memory allows: on the bit-plane path a launch of 8 or more groups of
 * 64 instances writes faster (4.8 -> 5.2-6.3 TB/s on the 156 809-wire --O1 witness of the metric circuit). */
typedef int (*cw_chunk_fn)(void *user, uint32_t first, uint32_t count, void *d_chunk, void *stream);
int cw_stream_witnesses_device(cw_batch *b, uint32_t first, uint32_t count, uint32_t chunk, void *d_buf0, void *d_buf1,
                               cw_chunk_fn consume, void *user);
/* public signals (main's outputs, then its public inputs = witness positions 1..cw_n_public) of EVERY instance,
 * [batch][n_public][32]: to host memory, or to device memory for a multi-GPU gather */
int cw_get_public(cw_batch *b, uint8_t *out);
int cw_get_public_device(cw_batch *b, void *d_out);
/* Witness bits OUT as packed ROWS, every engine: the mirror image of cw_set_inputs_rows*.  The call covers the entries
 * [entry0, entry0 + n) of the witness list (cw_set_witness_list order, as every other egress) for the instances
 * [first, first + count).  Row j starts at rows + j * stride and belongs to instance first + j; entry entry0 + k is bit k & 7 of
 * byte k >> 3, or, with CW_ROWS_MSB_FIRST, bit 7 - (k & 7): numpy's packbits and the order of a SHA-256 digest - entries 1 .. 256
 * of a Sha256(n) batch, most significant bit first, ARE hashlib.sha256(message).digest().  The bit is 1 if and only if the value
 * is 1: a boolean witness leaves in 1/256 of the bytes of cw_get_witnesses(_device).
 *   not boolean  a value that is neither 0 nor 1 gives bit 0 and is reported through one word: 0xFFFFFFFF when every value read
 *                was 0 or 1, else the lowest instance index OF THE BATCH, within the range, that held such a value.
 *                not_boolean / d_not_boolean may be NULL; the device word must be 4-byte aligned.  The call writes the word
 *                itself, in stream order: a fill kernel, then atomicMin.
 *   host form    any stride >= ceil(n / 8), any alignment.  Exactly ceil(n / 8) bytes per row are written, the spare bits of the
 *                last one are 0, every other byte of `rows` stays as it was.  Copies in pieces and synchronises before it returns.
 *   device form  d_rows 8-byte aligned, stride a multiple of 8 and at least 8 * ceil(n / 64), CW_EINVAL otherwise (the pointer is
 *                not touched).  8 * ceil(n / 64) bytes per row are written, pad bits 0; the bytes of a row behind them stay as they
 *                were.  Asynchronous on the batch's stream - with the one exception of every device egress: the first one after a
 *                cw_run of a bit-plane batch waits for the evaluation (the instances to re-run are known only then).
 *   empty        n == 0 or count == 0: CW_OK, no row is written, the word (if given) becomes 0xFFFFFFFF.
 *   errors       entry0 + n > cw_n_witness, first + count > batch, an unknown flag bit, a stride or an alignment as above:
 *                CW_EINVAL.  Checked in the order of the other getters: null / range / flags / alignment (CW_EINVAL), then the
 *                device (a host-only batch: CW_EDEVICE), then the state ("... before cw_run": CW_ESTATE).
 *   engines      bit-plane batches: one tiled bit transpose of the table's masks (csrc/cw_bits.hip cw_bits_masks_to_rows_kernel,
 *                both table layouts); the rows of instances the 256-bit side batch re-ran are written over from there.  64-bit
 *                runtime (csrc/cw64.hip cw64_pack_rows_kernel), also in the supplied-witness state, and the 256-bit schedule
 *                (csrc/cw_kernels.hip cw_pack_rows_kernel, canonical and Montgomery-form tables): the same tile, a compare per
 *                value.  A caller who does not know which engine cw_batch_create picked can rely on this form. */
int cw_get_witness_rows(cw_batch *b, uint32_t entry0, uint32_t n, uint32_t first, uint32_t count, uint8_t *rows, size_t stride,
                        uint32_t flags, uint32_t *not_boolean);
int cw_get_witness_rows_device(cw_batch *b, uint32_t entry0, uint32_t n, uint32_t first, uint32_t count, void *d_rows, size_t stride,
                               uint32_t flags, void *d_not_boolean);
/* Signal COLUMNS out, every engine: the mirror image of cw_set_inputs_range* / cw_set_input_column*.  Every bulk egress above is
 * addressed through the witness list and hands out the circuit's element; these two take a range of SIGNAL IDS - whether the
 * witness list names them or not: at --O1 most signals are not in it - and the caller's record layout: a stride and a narrow
 * little-endian element.  The verdict bit of a verifier, the bytes of a digest, a 64-bit index leave at their own width, for the
 * whole batch, in one call.
 *   layout       the n values of instance first + j are little-endian unsigned integers of elem_bytes in {1, 2, 4, 8, 32} and
 *                start at values + j * stride; value k is signal signal0 + k.  The ids are those of cw_get_signal,
 *                cw_signal_slots, the first column of the .sym file (cw_sym_find) and the wire numbers of the .r1cs of an
 *                unsimplified system, up to cw_n_signals - 1; the hidden log values and temporaries behind them are not
 *                addressable.  stride >= n * elem_bytes: there is no broadcast form on the way out.  Exactly n * elem_bytes
 *                bytes of a row are written and every other byte of the image stays as it was, so a caller fills the fields of
 *                an array of records with one call per field.  Offsets are 64-bit throughout.
 *   values       the canonical residue < q.  A table of Montgomery forms is converted on the way out, as every egress does; the
 *                8-byte residue of the 64-bit runtime is zero-extended for elem_bytes == 32.  A bit-plane batch delivers 0 / 1,
 *                and for the instances its 256-bit side batch re-ran what that batch holds, which may be any residue.
 *   too wide     a value >= 2^(8 elem_bytes) is stored as its low elem_bytes bytes and reported through one word: 0xFFFFFFFF when
 *                every value read fitted, else the lowest instance index OF THE BATCH, within the range, that held such a value -
 *                the contract and the mechanism of not_boolean in cw_get_witness_rows*: the call writes the word itself, in
 *                stream order, a fill kernel, then atomicMin.  too_wide / d_too_wide may be NULL; the device word must be 4-byte
 *                aligned.  elem_bytes == 32 never reports, and neither does elem_bytes == 8 on the 64-bit runtime.
 *   host form    any alignment.  The image is staged in pieces through the batch's bulk buffer and copied row by row into
 *                place, only the n * elem_bytes bytes of a row; synchronises before it returns.
 *   device form  d_values and stride multiples of elem_bytes (of 16 for 32-byte elements), CW_EINVAL otherwise (the pointer is
 *                not touched).  Asynchronous on the batch's stream - with the one exception of every device egress: the first
 *                one after a cw_run of a bit-plane batch waits for the evaluation.
 *   empty        n == 0 or count == 0: CW_OK, no byte of the image is written, the word (if given) becomes 0xFFFFFFFF.
 *   errors       in the order of the other getters: a null batch or image; elem_bytes outside the five widths; signal0 + n >
 *                cw_n_signals or first + count > batch (no 32-bit wrap); a stride shorter than the row; the alignments of the
 *                device form: CW_EINVAL.  Then the device (a host-only batch: CW_EDEVICE), then the state: CW_ESTATE "... before
 *                cw_run" for a batch that has neither run nor been supplied, "witnesses missing for N instances" for a supplied
 *                table with gaps, and on a complete supplied table the answer of cw_get_signal when the range names a signal
 *                the witness list does not hold (no witness program has run there).
 *   lifetime     the calls only read the table: status words, first-bad rows, timing marks, a captured cw_run_check graph and the
 *                supplied state stay as they were; before or after cw_check_r1cs.
 *   memory       a bit-plane batch reads its signal -> slot map on the device (cw_batch_signal_slots, 4 bytes per signal) and,
 *                where it has re-run instances, the instance -> side-batch map that cw_get_witnesses_at* makes (4 bytes per
 *                instance, uploaded on first use after a resolve, freed with the batch).  The host form grows the bulk buffer.
 *   engines      64-bit runtime (csrc/cw64.hip cw64_signals_kernel, also in the supplied-witness state), 256-bit schedule
 *                (csrc/cw_kernels.hip cw_signals_kernel, canonical and Montgomery-form tables): lane = instance on the read,
 *                the tile turned through LDS, consecutive lanes = consecutive values of one row on the write.  Bit-plane batches
 *                (csrc/cw_bits.hip cw_bits_signals_kernel, both table layouts): lane = signal, a value is one bit of a mask, no
 *                LDS; the rows of the instances the side batch re-ran are written over from there in one launch.
 *   not here     a scattered list of signal ids (one call per run of ids, as on the input side); instance lists; big-endian
 *                elements.
 * cw_sym_find is host-only and needs no batch: the lowest signal id and the count of the lines of a .sym file
 * ("id,witness,component,name" per line, as cw_explain reads it) whose name is `name` itself or begins with `name[` or `name.` -
 * "main.out" names all 256 bits of a Sha256 output, "main.h.out[3]" one signal.  CW_EIO when the file cannot be read, CW_EINPUT
 * "Signal not found: <name>" when nothing matches, CW_EINVAL when the matching ids are not one consecutive run (the message names
 * the first gap). */
int cw_get_signals_range(cw_batch *b, uint32_t signal0, uint32_t n, uint32_t first, uint32_t count, void *values, size_t stride,
                         uint32_t elem_bytes, uint32_t *too_wide);
int cw_get_signals_range_device(cw_batch *b, uint32_t signal0, uint32_t n, uint32_t first, uint32_t count, void *d_values, size_t stride,
                                uint32_t elem_bytes, void *d_too_wide);
int cw_sym_find(const char *sym_path, const char *name, uint32_t *signal0, uint32_t *n);
/* one signal of one instance (signalValues[slot]) */
int cw_get_signal(cw_batch *b, uint32_t instance, uint32_t slot, uint8_t out[32]);
/* writeBinWitness (main.cpp:288-334).  Every write is checked, here and in the two calls below: a file that could not be
 * written in full (a full disk) is CW_EIO "short write: <path>". */
int cw_write_wtns(cw_batch *b, uint32_t instance, const char *path);
/* `count` .wtns files from one bulk device transpose; `pattern` = printf pattern with one %u (instance number).  The files
 * are the ones cw_write_wtns writes (n8 = cw_element_bytes: the 64-bit runtime's rows leave the device 8 bytes per value). */
int cw_write_wtns_many(cw_batch *b, uint32_t first, uint32_t count, const char *pattern);
/* The whole batch as ONE compact container (<name>.wtnsb): field elements (n8 = cw_element_bytes) for 256-bit and 64-bit batches, the BIT TABLE (1 bit per
 * distinct signal value and instance + the slot of every witness element + full values of the instances the 256-bit schedule
 * re-ran) for bit-plane batches.  Format: csrc/cw_host.cpp at cw_write_wtnsb; reader / expander circom_amd/wtnsb.py
 * (`expand(i)` = the bytes cw_write_wtns writes for instance i, main.cpp:288-334). */
int cw_write_wtnsb(cw_batch *b, const char *path);
/* ---- witnesses IN: check witnesses this batch did not compute (64-bit runtime) ------------------------------------------
 * The `.wtns` files of another calculator (the reference runtime, an older build, another machine), or an image streamed out
 * earlier with cw_get_witnesses_device(_n8), go back into the value table, and cw_check_r1cs, cw_explain and every egress work
 * on them - the batch counterpart of `snarkjs wtns check`.  The image is [count][n_witness][element] little-endian in the order
 * of the circuit's witness list (cw_set_witness_list), element = 32 bytes (cw_set_witnesses, _device) or cw_element_bytes = 8
 * (the _n8 forms, the files); instance j of the image is instance first + j of the batch.  One tiled transpose on the device
 * (csrc/cw64.hip cw64_transpose_in_kernel<EB, true>), the mirror image of the bulk egress.
 *   validation  nothing is repaired quietly.  The value stored is the reduced one (the check needs a residue), and
 *               CW_ST_BAD_WITNESS is set in the instance's status word when a value was not canonical (>= p; in the 32-byte
 *               form also: any of the upper three words set) or entry 0 is not 1.  Entry 0 is not stored: the constant wire
 *               stays 1, so the constant terms of the check stay meaningful for the other wires.
 *   state       the FIRST supply since cw_batch_create or since the last cw_run clears every status word and first-bad row and
 *               the coverage record; the batch is then "supplied".  Later supplies add coverage.  An instance supplied twice is
 *               overwritten; a CW_ST_BAD_WITNESS bit (or a CW_ST_R1CS_FAILED bit of an earlier check) it had stays set until
 *               the next cw_run or the next first supply.  cw_witnesses_missing: instances not covered yet, -1 when the batch
 *               is not in the supplied state.  cw_check_r1cs answers CW_ESTATE "witnesses missing for N instances" until that
 *               is 0; run twice on the same table it gives the same words.  cw_run ends the supplied state, and so does
 *               cw_run_check: plain or replayed from its graph it begins with the table's init and the ingest of the INPUTS, so
 *               it computes the batch's own witnesses over whatever was supplied.
 *   served      cw_get_status, cw_get_r1cs_first_bad, cw_explain, cw_get_witness(es)(_device)(_n8), cw_stream_witnesses_device,
 *               cw_get_public(_device), cw_get_witness_rows(_device), cw_write_wtns(_many), cw_write_wtnsb read the table through the witness list and work
 *               unchanged.  No witness program has run on a supplied table: cw_get_signal of a signal the witness list does not
 *               name and cw_get_log answer CW_ESTATE (temporaries and hidden log values were never written).  With a shortened
 *               witness list the check is meaningful when the .r1cs names listed signals only.
 *   lifetime    the host forms and the file forms copy in pieces and synchronise before they return.  The device forms launch
 *               the kernel inside the call: the buffer is read in stream order and may be reused once the batch's stream has
 *               passed the call - nothing is deferred to a later call, unlike cw_set_inputs_device.
 *   alignment   d_le8: 8 bytes, d_le32: 16 bytes, CW_EINVAL otherwise (the pointer is not touched).
 *   files       cw_read_wtns / cw_read_wtns_many (`pattern`: one %u / %d = the instance number, as cw_write_wtns_many) check
 *               magic, version, the two sections in either order, n8 = cw_element_bytes, the circuit's prime, nWitness =
 *               cw_n_witness, a body of exactly nWitness x n8 bytes and nothing behind it (csrc/cw_wtns_read.h); each refusal
 *               is CW_EIO with the path and the reason.  Many files go to the device as one image per 256 MiB.
 *   engines     circuits of the 256-bit schedule and bit-plane circuits answer CW_ESTATE "supplied witnesses are served by the
 *               64-bit runtime only (--prime goldilocks)".
 * Every call checks in this order: null / range / alignment (CW_EINVAL), engine (CW_ESTATE), [the files (CW_EIO)], device. */
int cw_set_witnesses(cw_batch *b, uint32_t first, uint32_t count, const uint8_t *le32);
int cw_set_witnesses_n8(cw_batch *b, uint32_t first, uint32_t count, const void *le8);
int cw_set_witnesses_device(cw_batch *b, uint32_t first, uint32_t count, const void *d_le32);
int cw_set_witnesses_device_n8(cw_batch *b, uint32_t first, uint32_t count, const void *d_le8);
int cw_read_wtns(cw_batch *b, uint32_t instance, const char *path);
int cw_read_wtns_many(cw_batch *b, uint32_t first, uint32_t count, const char *pattern);
int64_t cw_witnesses_missing(const cw_batch *b);
/* human-readable trace of one instance into out[out_len]: decoded status word and, for a violated constraint, its index
 * and every wire with its name from <name>.sym (may be NULL) and value — the batch counterpart of the trace the
 * reference prints before aborting (c_code_generator.rs:461-468, calcwit.cpp:104-114) */
int cw_explain(cw_batch *b, uint32_t instance, const char *sym_path, char *out, size_t out_len);
/* log(...) statements of the circuit (LogBucket, compiler/src/intermediate_representation/log_bucket.rs:105-162: the
 * emitted calculator prints every argument with printf - values through Fr_element2str - one blank between arguments
 * and a newline per statement).  A batched run has no console per instance: the schedule keeps every logged value in
 * the table (hidden signals behind the circuit's own; cw_n_signals does not count them) and cw_get_log formats what the
 * reference binary prints on stdout for ONE instance, up to its first failed run-time check (where the reference process
 * exits).  Returns the length of the text or a negative CW_E* code; stores at most out_len - 1 characters + NUL.
 * Both engines serve it: circuits of the 64-bit runtime (--prime goldilocks) keep their logged values in hidden 8-byte slots. */
uint32_t cw_n_log_statements(const cw_circuit *c);
int64_t cw_get_log(cw_batch *b, uint32_t instance, char *out, size_t out_len);
/* first violated constraint per instance after cw_check_r1cs: [batch], 0xFFFFFFFF = none */
int cw_get_r1cs_first_bad(cw_batch *b, uint32_t *row);
/* R1CS products OUT, every engine: the three linear forms A.w, B.w, C.w of every constraint - what a Groth16 prover builds first
 * (A.w and B.w over all constraints, then C.w = A.w o B.w and the NTT), what a Spartan / Nova style prover needs all of, and what
 * shows on which side a violated row is off.  Every check kernel forms them and throws them away; here they leave the device
 * without the witness leaving it first.
 *   image        out[j][p][k]: instance first + j; the p-th selected part of `parts` (CW_R1CS_A | CW_R1CS_B | CW_R1CS_C) in the
 *                order A, B, C; constraint row0 + k in the order of the .r1cs file - the numbering of cw_get_r1cs_first_bad and
 *                cw_explain.  Dense: count x popcount(parts) x n_rows elements, offsets in 64-bit arithmetic.
 *   element      cw_element_bytes(c) bytes (8 for the 64-bit runtime, 32 otherwise): the canonical little-endian residue < q.  A
 *                table of Montgomery forms is converted on the way out, as every other egress does.
 *   value        the sum of coefficient x w[wire] over the terms of that part of that row as the .r1cs given to cw_load states
 *                them: an empty part is 0, a term on wire 0 is its coefficient, a coefficient >= q (where the loader accepts
 *                one) counts reduced.  The full system is used whatever cw_set_witness_list says: the list shortens egress.
 *   errors       in the order of the other getters: a null batch or pointer; parts == 0 or a bit outside 7; row0 + n_rows >
 *                cw_n_constraints or first + count > batch (no 32-bit wrap); device form: d_out not aligned to 8 bytes (64-bit
 *                runtime) or 16 bytes (the pointer is not touched): CW_EINVAL.  Then the device (a host-only batch: CW_EDEVICE),
 *                then the state: CW_ESTATE "... before cw_run" for a batch that has neither run nor been supplied, "witnesses
 *                missing for N instances" for a supplied table with gaps, as cw_check_r1cs answers.
 *   empty        n_rows == 0 or count == 0: CW_OK, nothing is written.
 *   lifetime     the host form copies in pieces through a staging buffer and synchronises before it returns.  The device form
 *                is asynchronous on the batch's stream - with the one exception of every device egress: the first one after a
 *                cw_run of a bit-plane batch waits for the evaluation.  The call only reads the table: status words, first-bad
 *                rows, a captured cw_run_check graph and the supplied state stay as they were; before or after cw_check_r1cs.
 *   memory       the plan (row pointers in file order, plain term lists: csrc/cw_r1cs_products.h) goes to the device with the
 *                batch's FIRST call, which drains the stream once, and is freed with the batch; a batch that never asks pays
 *                nothing.
 *   engines      64-bit runtime (csrc/cw64.hip cw64_products_kernel, also in the supplied-witness state), 256-bit schedule
 *                (csrc/cw_kernels.hip cw_products_kernel, canonical and Montgomery-form tables), bit-plane batches
 *                (csrc/cw_bits.hip cw_bits_products_kernel, both table layouts: a select per term, no multiplication; the
 *                instances the 256-bit side batch re-ran are written over from there).  Lane = instance, the tile turned
 *                through LDS: every store is 512 contiguous bytes of one instance's run of rows. */
#define CW_R1CS_A 1u
#define CW_R1CS_B 2u
#define CW_R1CS_C 4u
int cw_get_r1cs_products(cw_batch *b, uint32_t parts, uint32_t row0, uint32_t n_rows, uint32_t first, uint32_t count, uint8_t *out);
int cw_get_r1cs_products_device(cw_batch *b, uint32_t parts, uint32_t row0, uint32_t n_rows, uint32_t first, uint32_t count, void *d_out);
/* ---- instance lists: select by status on the device, egress by index, every engine --------------------------------------------
 * Every egress above takes a contiguous range of instances.  A real batch is not uniformly good: a prover wants the witnesses of
 * the clean instances as ONE dense image, an operator those of the failed ones.  cw_select_instances* makes the list on the
 * device, cw_get_witnesses_at* hands out the witnesses of a list; chained through device memory the host reads neither the 4
 * bytes per instance of cw_get_status nor the count.
 *   select       the instances i with (status[i] & mask) == want, ascending, as uint32_t; status[i] is exactly the word
 *                cw_get_status returns for i (bit-plane batches: the side batch's word for an instance it re-ran).  mask = ~0u,
 *                want = 0: the clean instances; mask = want = CW_ST_R1CS_FAILED: those that failed the check; mask = want = 0:
 *                all.  idx / d_idx have room for cw_batch_size entries; only the first *n are written, the rest keep their
 *                bytes.  idx may be NULL (the host form then only counts); the device form needs both pointers, 4-byte aligned.
 *                Before cw_check_r1cs the R1CS bit is simply not set.
 *   image        out[j][k]: entry entry0 + k of the witness list (cw_set_witness_list order, as every other egress) of instance
 *                idx[j], j < n_idx, k < n.  Dense: n_idx x n elements, offsets in 64-bit arithmetic.  The list may be in any
 *                order and may name an instance twice.  The public signals of the listed instances: entry0 = 1, n = cw_n_public.
 *   element      32 bytes, or cw_element_bytes in the _n8 forms (8 for the 64-bit runtime; for every other circuit they ARE the
 *                32-byte calls): the canonical little-endian residue < q.  A table of Montgomery forms is converted on the way
 *                out, as every other egress does.
 *   host form    every index is validated before anything is touched: an index >= cw_batch_size is CW_EINVAL and the message
 *                names its position.  The image is copied in pieces through a staging buffer; synchronises before it returns.
 *   device form  the kernels are launched INSIDE the call: d_idx is read in stream order and may be reused once the batch's
 *                stream has passed the call (the rule of cw_set_witnesses_device).  The host cannot see the list, so nothing is
 *                read out of bounds: a position whose index is >= cw_batch_size gets a row of zeros, and the lowest such position
 *                goes to *d_bad (optional, 4-byte aligned; 0xFFFFFFFF for a clean list; the call writes the word itself, in
 *                stream order: a fill kernel, then atomicMin).  d_n_idx (optional, 4-byte aligned): the list ends at
 *                min(n_idx, *d_n_idx), read on the device; rows behind it are not written.  So d_idx and d_n of
 *                cw_select_instances_device feed the egress, n_idx = cw_batch_size, without the host reading the count: the grid
 *                is sized by n_idx, workgroups behind the device count leave at once.  d_out: 16-byte aligned (8 bytes for the
 *                8-byte element).
 *   errors       in the order of the other getters: a null batch or pointer, entry0 + n > cw_n_witness (no 32-bit wrap), an index
 *                of a host list out of the batch, an alignment as above (the pointer is not touched): CW_EINVAL.  Then the device
 *                (a host-only batch: CW_EDEVICE), then the state: CW_ESTATE "... before cw_run" for a batch that has neither run
 *                nor been supplied, "witnesses missing for N instances" for a supplied table with gaps, as cw_check_r1cs answers.
 *   empty        n == 0 or n_idx == 0: CW_OK, no row is written; *d_bad (if given) becomes 0xFFFFFFFF.
 *   lifetime     the host forms synchronise before they return.  The device forms are asynchronous on the batch's stream - with
 *                the one exception of every device egress: the first call after a cw_run of a bit-plane batch waits for the
 *                evaluation.  The calls only read: status words, first-bad rows, a captured cw_run_check graph and the supplied
 *                state stay as they were.
 *   memory       the select kernels keep 4 bytes per 2 048 instances (and the host form its list) with the batch; a bit-plane
 *                batch uploads its instance -> side-batch map (4 bytes per instance) with the first call after a resolve.  All of
 *                it is made on first use and freed with the batch; a batch that never asks pays nothing.
 *   engines      select: csrc/cw_kernels.hip cw_select_block_kernel / cw_select_scan_kernel - count, scan, scatter as three
 *                launches, no workgroup waits for another - for every engine.  Egress: 64-bit runtime (csrc/cw64.hip
 *                cw64_egress_kernel<EB, true>, also in the supplied-witness state), 256-bit schedule (csrc/cw_kernels.hip
 *                cw_gather_many_kernel<MONT, true>, canonical and Montgomery-form tables), bit-plane batches (csrc/cw_bits.hip
 *                cw_bits_gather_kernel<true>, both table layouts; the rows of the instances the 256-bit side batch re-ran are written
 *                over from there in one launch).  The tiles and stores of the range kernels, the column taken from the list. */
int cw_select_instances(cw_batch *b, uint32_t mask, uint32_t want, uint32_t *idx, uint32_t *n);
int cw_select_instances_device(cw_batch *b, uint32_t mask, uint32_t want, void *d_idx, void *d_n);
int cw_get_witnesses_at(cw_batch *b, uint32_t entry0, uint32_t n, const uint32_t *idx, uint32_t n_idx, uint8_t *out);
int cw_get_witnesses_at_n8(cw_batch *b, uint32_t entry0, uint32_t n, const uint32_t *idx, uint32_t n_idx, uint8_t *out);
int cw_get_witnesses_at_device(cw_batch *b, uint32_t entry0, uint32_t n, const void *d_idx, uint32_t n_idx, const void *d_n_idx,
                               void *d_out, void *d_bad);
int cw_get_witnesses_at_device_n8(cw_batch *b, uint32_t entry0, uint32_t n, const void *d_idx, uint32_t n_idx, const void *d_n_idx,
                                  void *d_out, void *d_bad);
/* ---- witness digests: SHA-256 of every instance's .wtns on the device, every engine ------------------------------------------
 * This project states correctness as the SHA-256 of a `.wtns` file (tests/golden/: wtns_sha256 of what the reference runtime
 * wrote).  These calls compute that hash where the table lies: 32 bytes per instance leave the device instead of the witness.
 * A caller compares a whole batch with a list of reference hashes or with another machine's batch, content-addresses or
 * deduplicates witnesses, keeps an audit record - and no witness is moved.
 *   digest       out[j] = the 32 digest bytes, in the order hashlib.sha256(..).digest() and sha256sum give them, of exactly the
 *                bytes cw_write_wtns(b, first + j, path) writes at that moment: the header of writeBinWitness (main.cpp:288-334)
 *                with n8 = cw_element_bytes, the circuit's prime and nWitness = the CURRENT cw_n_witness (a list shortened by
 *                cw_set_witness_list counts), then the canonical little-endian elements in witness-list order.  A table of
 *                Montgomery forms is converted on the way, as every egress does.  Digests are produced whatever the status
 *                word says, as the file calls do.
 *   errors       in the order of the other getters: a null batch or pointer; first + count > batch (no 32-bit wrap); device
 *                form: d_out not 16-byte aligned (the pointer is not touched): CW_EINVAL.  Then the device (a host-only batch:
 *                CW_EDEVICE), then the state: CW_ESTATE "... before cw_run" for a batch that has neither run nor been supplied,
 *                "witnesses missing for N instances" for a supplied table with gaps, as cw_get_r1cs_products answers; a complete
 *                supplied table is served.
 *   empty        count == 0: CW_OK, nothing is written.
 *   lifetime     the device form is asynchronous on the batch's stream - with the one exception of every device egress: the
 *                first one after a cw_run of a bit-plane batch waits for the evaluation.  The host form stages pieces in the
 *                batch's bulk buffer and synchronises before it returns.  The calls only read the table: status words, first-bad
 *                rows, the timing marks, a captured cw_run_check graph and the supplied state stay as they were.
 *   engines      lane = instance, one wave per table group of 64 instances; SHA-256 is serial per message, so a small batch of
 *                huge witnesses is bound by the latency of one lane.  64-bit runtime (csrc/cw64.hip cw64_wtns_digest_kernel,
 *                also in the supplied-witness state), 256-bit schedule (csrc/cw_kernels.hip cw_wtns_digest_kernel, canonical and
 *                Montgomery-form tables), bit-plane batches (csrc/cw_bits.hip cw_bits_wtns_digest_kernel, both table layouts; the
 *                digests of the instances the 256-bit side batch re-ran are written over from there).  One text of the header
 *                bytes, the message walk and the compression function serves the kernels, the file writers and the CPU replay
 *                (csrc/cw_wtns_digest.h, csrc/cw_sha256.h).
 *   not here     an index-list form; one message split over lanes; other hash functions. */
int cw_get_wtns_digests(cw_batch *b, uint32_t first, uint32_t count, uint8_t *out);
int cw_get_wtns_digests_device(cw_batch *b, uint32_t first, uint32_t count, void *d_out);
/* ---- witness compare: an image or .wtns files against the batch, on the device, every engine ---------------------------------
 * This project states correctness as byte equality with another calculator's `.wtns`.  These calls apply that measure to a whole
 * batch where the table lies: the table is read once, the image once, four bytes per instance are written, and the first
 * differing entry is named - which a digest cannot do.  Witness programs are deterministic, so "equal to what this batch computes
 * from the same inputs" is the verdict on another calculator's witnesses for every engine (cw_set_witnesses* serves the 64-bit
 * runtime only); one batch's cw_get_witnesses_device image is another batch's compare image (emitted code against the
 * interpreter, the bit-plane program against the 256-bit schedule).
 *   image        image[j][k]: entry entry0 + k of the witness list (cw_set_witness_list order, as every egress) of instance
 *                first + j, j < count, k < n.  Dense: count x n elements, offsets in 64-bit arithmetic.
 *   element      32 bytes, or cw_element_bytes in the _n8 forms (8 for the 64-bit runtime; for every other circuit they ARE the
 *                32-byte calls).
 *   verdict      diff[j] = the lowest entry0 + k for which the element's bytes in the image differ from the bytes
 *                cw_get_witnesses_device(_n8) would write there at that moment; 0xFFFFFFFF: the run is equal.  BYTES are compared,
 *                nothing is reduced or repaired: an image value v + q differs from v; in the 32-byte form of the 64-bit runtime
 *                the upper 24 bytes must be zero; for a bit-plane batch an element equals the bit only as the 32-byte value 0 or
 *                1.  A table of Montgomery forms is converted on the way, as every egress does.  Verdicts are produced whatever
 *                the status word says, as the file and digest calls do.
 *   summary      optional.  summary[0] = the instances of the range with a difference, each counted once; summary[1] = the
 *                lowest of them as first + j, or 0xFFFFFFFF.
 *   errors       in the order of the other getters: a null batch, image or diff; entry0 + n > cw_n_witness or first + count >
 *                batch (no 32-bit wrap); device form: d_image not aligned to 16 bytes (8 bytes for the 8-byte element), d_diff or
 *                d_summary not to 4 (the pointers are not touched): CW_EINVAL.  Then the device (a host-only batch: CW_EDEVICE),
 *                then the state: CW_ESTATE "... before cw_run" for a batch that has neither run nor been supplied, "witnesses
 *                missing for N instances" for a supplied table with gaps; a complete supplied table is served.
 *   empty        count == 0: CW_OK, diff is not written, summary becomes {0, 0xFFFFFFFF}.  n == 0 with count > 0:
 *                diff[0 .. count) becomes 0xFFFFFFFF.
 *   lifetime     the device form launches INSIDE the call and writes d_diff[0 .. count) and d_summary itself, in stream order: a
 *                fill, then the compare.  The image is read in stream order and may be reused once the batch's stream has passed
 *                the call.  Asynchronous - with the one exception of every device egress: the first call after a cw_run of a
 *                bit-plane batch waits for the evaluation.  The host form stages pieces of whole rows in the batch's bulk buffer
 *                (the piece's verdict words behind them) and synchronises before it returns.  The calls only read the table:
 *                status words, first-bad rows, the timing marks, a captured cw_run_check graph and the supplied state stay as
 *                they were; before or after cw_check_r1cs.
 *   files        cw_compare_wtns / _many: each file goes through the checked reader of cw_read_wtns (csrc/cw_wtns_read.h): a wrong
 *                magic, version, n8, prime, witness length or body size is CW_EIO with the path and the reason - NOT a
 *                difference.  Only the bodies are compared, entry0 = 0 and n = cw_n_witness, the element the files carry.
 *                `pattern` has one %u or %d, as cw_write_wtns_many.  Many files go to the device as one staged image per piece,
 *                not one launch per file.  Checked in the order of cw_read_wtns: arguments, files, device, state - a host-only
 *                batch can tell a good file from a bad one.
 *   memory       the staging buffer of the host forms is the batch's bulk buffer; a bit-plane batch uploads its instance ->
 *                side-batch map (4 bytes per instance) with the first call after a resolve.  A batch that never asks pays nothing.
 *   engines      one kernel per table layout, each the range egress kernel with its store turned into a streaming load and a
 *                compare: lane = instance for the table read, the tile turned through LDS (a ballot window on the bit table),
 *                the image read in 512 B to 1 KiB contiguous pieces of one instance's row, every byte by exactly one workgroup.
 *                64-bit runtime (csrc/cw64.hip cw64_compare_kernel<EB>, also in the supplied-witness state), 256-bit schedule
 *                (csrc/cw_kernels.hip cw_compare_kernel<MONT>, canonical and Montgomery-form tables), bit-plane batches
 *                (csrc/cw_bits.hip cw_bits_compare_kernel, both table layouts; the instances the 256-bit side batch re-ran are
 *                skipped there and judged from the side batch's table in one launch).  The mismatches of a workgroup are reduced
 *                in LDS first (csrc/cw_compare.hip.h): at most one global atomicMin per instance and workgroup, none for an image
 *                that matches; the workgroup that sees 0xFFFFFFFF come back counts the instance.
 *   not here     an index-list form; narrow elements; big-endian images; putting the image INTO the table (that remains
 *                cw_set_witnesses*, 64-bit runtime only). */
int cw_compare_witnesses(cw_batch *b, uint32_t entry0, uint32_t n, uint32_t first, uint32_t count, const uint8_t *image, uint32_t *diff,
                         uint32_t summary[2]);
int cw_compare_witnesses_n8(cw_batch *b, uint32_t entry0, uint32_t n, uint32_t first, uint32_t count, const uint8_t *image, uint32_t *diff,
                            uint32_t summary[2]);
int cw_compare_witnesses_device(cw_batch *b, uint32_t entry0, uint32_t n, uint32_t first, uint32_t count, const void *d_image, void *d_diff,
                                void *d_summary);
int cw_compare_witnesses_device_n8(cw_batch *b, uint32_t entry0, uint32_t n, uint32_t first, uint32_t count, const void *d_image,
                                   void *d_diff, void *d_summary);
int cw_compare_wtns(cw_batch *b, uint32_t instance, const char *path, uint32_t *diff);
int cw_compare_wtns_many(cw_batch *b, uint32_t first, uint32_t count, const char *pattern, uint32_t *diff, uint32_t summary[2]);
/* host-only: build and hazard-check the LDS staging plan of the R1CS check kernel for `chunks` row chunks
   and `entries` 2-KiB LDS entries per wave (0 = the defaults cw_batch_create would pick for `batch`).
   out[8] = {chunks, loads, terms, filler loads, distinct wires, entries, prefetch depth, 0}. */
int cw_r1cs_plan_stats(const cw_circuit *c, uint32_t batch, uint32_t chunks, uint32_t entries, uint64_t out[8]);
/* host-only: the term stream of the default check kernel (csrc/cw_r1cs_plan.h build_stream), as cw_batch_create uploads it, so
   that a test can replay it on the CPU.  flags: 1 = boolean rows b (b - 1) = 0 stay three terms and a product, 2 = boolean rows
   do not ride inside the sum that reads the same bit.  sizes[8] = {words of chunk[], words of terms[], words of row_orig[],
   words of ctab[], terms, boolean rows folded into another row, products replaced by a select, chunks}; a null buffer is not
   written (call once for the sizes).  No reference counterpart (snarkjs `wtns check` is the reference-side check). */
int cw_r1cs_stream_plan(const cw_circuit *c, uint32_t terms_per_chunk, uint32_t flags, uint64_t sizes[8], uint32_t *chunk,
                        uint32_t *terms, uint32_t *row_orig, uint32_t *ctab);
/* host-only: the plan cw_get_r1cs_products walks (csrc/cw_r1cs_products.h), so that a test can compare it with the constraint
   system on the CPU: rowptr[3 n + 1] in the order of the .r1cs file (constraint k, part p: the terms rowptr[3 k + p] ..
   rowptr[3 k + p + 1]) into terms of sizes[3] words: {slot, coefficient id into ctab as cw_r1cs_stream_plan hands it out: 0 = +1,
   1 = -1, bit 31 = the constant wire, entry taken as it stands, else c * 2^261 mod q}; bits != 0: the plan of a bit-plane batch,
   {bit-table slot of the interpreter's table, id of the canonical coefficient in ctab}; 64-bit runtime: {slot, 0, coefficient
   lo, hi}, no ctab.  sizes[4] = {words of rowptr[], words of terms[], words of ctab[], words per term}; a null buffer is not
   written (call once for the sizes). */
int cw_r1cs_products_plan(const cw_circuit *c, uint32_t bits, uint64_t sizes[4], uint32_t *rowptr, uint32_t *terms, uint32_t *ctab);

/* raw device pointers for zero-copy consumers (provers): value table, layout in DESIGN.md.  When cw_circuit_montgomery()
   is 1 the table holds x * 2^261 mod q (the schedule of an arithmetic circuit keeps its signals in Montgomery form, so that
   a product of two signals is one Montgomery product); every other egress (cw_get_witness*, cw_get_signal, cw_write_wtns*,
   cw_get_witnesses_device) returns canonical values, as the reference's Fr_toLongNormal does (main.cpp:326-332).
   64-bit runtime (--prime goldilocks): V[slot][padded batch] of uint64 canonical residues - slot 0 = the constant 1, the
   circuit's signals, the hidden log values, then the temporaries (csrc/cw64.hip). */
void *cw_device_values(cw_batch *b, uint64_t *n_bytes, uint32_t *padded_batch);
int cw_circuit_montgomery(const cw_circuit *c);
/* bit-plane batches: the bit table T[group][slot] (uint64, bit i = instance group*64+i).  Slot 0 / 1 = the constants
 * 0 / 1, main input k = slot 3 + k; every other signal sits in the slot cw_signal_slots() names (signals that are copies
 * of one another share a slot; slots follow the order in which the program produces the values, 32-bit words of
 * consecutive signals keep 32 consecutive slots).  NULL for 256-bit batches (cw_device_values is NULL for bit-plane ones). */
void *cw_device_bits(cw_batch *b, uint64_t *n_bytes, uint64_t *slots_per_group);
/* signal -> bit-table slot, n_signals entries (host memory owned by the circuit), NULL when there is no bit program */
const uint32_t *cw_signal_slots(const cw_circuit *c);
/* A circuit may carry its bit-plane program twice: interpreted (cw_bits_eval_kernel, T[group][slot]) and as EMITTED gfx950
 * code (hip_elements/bitjit.py: the counterpart of the reference's per-circuit <name>.cpp, compiler/src/circuit_design/
 * template.rs:174-474), which batches of >= 2^18 instances run (CW_BITS_JIT=0/1 overrides).  The emitted code has its
 * own table layout and slot map, so a caller of cw_device_bits asks the BATCH:
 *   out = {slots per group (sh = 0) or rows per chunk (sh = 5), sh, groups allocated, 1 if the emitted code runs}
 *   element (group g, slot s) = T[(((g >> sh) * slots + s) << sh) + (g & ((1 << sh) - 1))]   (uint64, bit i = instance 64 g + i)
 * cw_batch_signal_slots: signal -> slot for THIS batch (cw_signal_slots names the interpreter's map).
 * Taking the raw pointer (cw_device_bits) makes the next cw_check_r1cs audit every group from the table instead of
 * trusting the check the emitted code fused into the evaluation. */
int cw_batch_bits_layout(const cw_batch *b, uint64_t out[4]);
const uint32_t *cw_batch_signal_slots(const cw_batch *b);

/* ---- field micro-benchmark + unit-test hooks (Fr_* seam 2: bn128/fr.hpp:28-81) --------------------- */
/* n lanes x iters dependent Montgomery multiplications on the device; out[i] = a[i]*b[i]^iters (raw
 * Montgomery domain).  a,b,out: host [n][32].  ms: kernel time from HIP events. */
int cw_fp_mul_bench(const uint8_t prime_le32[32], int device, uint32_t n, uint32_t iters, const uint8_t *a,
                    const uint8_t *b, uint8_t *out, float *ms);
/* Time the bit-plane evaluation kernel on an arbitrary program (records / command blocks as in the .cwt, validated like
 * a loaded one) for n_groups groups of 64 instances on a zero-filled table: average ms over `iters` launches.  A
 * measurement hook (tools/bits_shape_bench.py), not part of the witness path. */
int cw_bits_eval_bench(int device, uint32_t ring, uint32_t cache, uint32_t n_vrows, uint64_t n_slots, const uint32_t *recs,
                       const uint32_t *cmds, uint32_t n_groups, uint32_t width, uint32_t iters, float *ms);
/* Element-wise device evaluation of one schedule opcode (D_* numbering of cw_tape.h) on n operand
 * pairs — the unit-test hook for the device field functions.  status[n] receives CW_ST_* bits. */
int cw_fp_op(const uint8_t prime_le32[32], int device, uint32_t dop, uint32_t n, const uint8_t *a, const uint8_t *b,
             const uint8_t *c, uint8_t *out, uint32_t *status);

#ifdef __cplusplus
}
#endif
#endif /* CIRCOM_AMD_H */
