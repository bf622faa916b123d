// cw_kernels.h — launch wrappers implemented in cw_kernels.hip
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include "cw_tape.h"
#include "cw_wtns_digest.h"

// `mont`: the value table holds Montgomery forms x R' (lower.py pass A6): init writes R' into the constant-one slot, ingest
// multiplies by R'^2, the gathers by 1, the R1CS check compares mmul(A~, B~) with C~
hipError_t cwk_init(hipStream_t s, void *V, uint32_t Bp, uint32_t *status, uint32_t *first_bad, bool mont, const FpParams &P);
hipError_t cwk_ingest(hipStream_t s, const void *in, void *V, uint32_t input_start, uint32_t n_in, uint32_t batch,
                      uint32_t Bp, bool mont, const FpParams &P);
hipError_t cwk_eval(hipStream_t s, bool full, bool wide_linsum, const CwDRow *rows, const uint32_t *stream_off,
                    const uint64_t *extras, const uint32_t *extra_off, const uint64_t *terms, const uint32_t *term_off,
                    uint32_t n_strands, uint32_t n_lds, void *V, const uint32_t *consts, const uint32_t *lconsts,
                    const uint32_t *fncode, const uint32_t *fntab, uint64_t slot_stride,
                    uint32_t Bp, uint32_t batch, uint32_t lanes, uint32_t prio_mask, uint32_t *status, const FpParams &P);
// pipelined single-wave schedule: rows = device rows (CwPRow, padded by 3 NOPs), loads = (n_rows / nb + 2) * nld words
hipError_t cwk_eval_pipe(hipStream_t s, bool full, bool wide_linsum, uint32_t nb, uint32_t nld, const void *rows, uint32_t n_rows,
                         const uint32_t *loads, const uint64_t *terms, void *V, const uint32_t *consts, const uint32_t *lconsts,
                         uint64_t slot_stride, uint32_t Bp, uint32_t batch, uint32_t lanes, uint32_t *status, const FpParams &P);
hipError_t cwk_fill32(hipStream_t s, uint32_t *p, uint32_t v, size_t n);     // p[0..n) = v, as a kernel (graph-safe)
hipError_t cwk_fused_merge(hipStream_t s, const uint32_t *found, uint32_t batch, uint32_t *status, uint32_t *first_bad);
hipError_t cwk_r1cs(hipStream_t s, const uint32_t *chunk, uint32_t n_chunks, const uint32_t *terms, const uint32_t *ctab,
                    const uint32_t *ctab29, const uint32_t *row_orig, const void *V, uint32_t Bp, uint32_t batch, uint32_t *status,
                    uint32_t *first_bad, bool mont, const FpParams &P);
hipError_t cwk_r1cs_staged(hipStream_t s, const uint32_t *chunk, uint32_t n_chunks, const uint32_t *rec, const uint32_t *terms,
                           const uint32_t *ctab, const uint32_t *ctab29, const uint32_t *row_orig, uint32_t entries, const void *V, uint32_t Bp,
                           uint32_t batch, uint32_t *status, uint32_t *first_bad, bool mont, const FpParams &P);
hipError_t cwk_gather(hipStream_t s, const void *V, const uint32_t *w2s, uint32_t n_wit, uint32_t Bp, uint32_t instance,
                      void *out, bool mont, const FpParams &P);
hipError_t cwk_gather_many(hipStream_t s, const void *V, const uint32_t *w2s, uint32_t n_wit, uint32_t Bp, uint32_t first,
                           uint32_t count, void *out, bool mont, const FpParams &P);
hipError_t cwk_mulbench(hipStream_t s, const void *a, const void *b, void *out, uint32_t n, uint32_t iters,
                        const FpParams &P);
hipError_t cwk_fpop(hipStream_t s, uint32_t op, const void *a, const void *b, const void *c, void *out, uint32_t *status,
                    uint32_t n, const FpParams &P);

// ---- bit-plane path (cw_bits.hip) ----
// `sh` = layout shift of the bit table (cw_bits.hip: 0 = T[group][slot] of the interpreter, 5 = T[chunk][slot][group in chunk]
// of the emitted code); `only` (R1CS audit): groups whose flag word is zero are skipped (nullptr = audit every group)
hipError_t cwk_bits_init(hipStream_t s, void *T, uint64_t slots, uint32_t sh, uint32_t n_groups, void *fbmask, void *r1flag,
                         uint32_t *status, uint32_t *first_bad, uint32_t Bp);
hipError_t cwk_bits_ingest(hipStream_t s, const void *in, void *T, uint64_t slots, uint32_t sh, uint32_t input_slot0, uint32_t n_in,
                           uint32_t batch, void *fbmask);
// the same result by the previous body (two 16-byte loads per lane and input; CW_BITS_INGEST_LINE=0: A/B timing in one process)
hipError_t cwk_bits_ingest_halves(hipStream_t s, const void *in, void *T, uint64_t slots, uint32_t sh, uint32_t input_slot0, uint32_t n_in,
                                  uint32_t batch, void *fbmask);
hipError_t cwk_bits_eval(hipStream_t s, const void *recs, const uint32_t *cmds, uint32_t n_batches, uint32_t ring, uint32_t cache,
                         void *T, uint64_t slots, uint32_t n_groups, uint32_t width, const uint32_t *aslots, uint32_t n_asserts,
                         void *fbmask);
hipError_t cwk_bits_gather(hipStream_t s, const void *T, uint64_t slots, uint32_t sh, const uint32_t *wslot, uint32_t n_wit, uint32_t first,
                           uint32_t count, void *out);
// packed masks[ceil(batch / 64)][n_in] -> the input slots of the table.  sh = 5: cw_bits_masks_to_table_rows_kernel writes whole
// 256-byte rows, every chunk's 32 group columns (the padding groups of the last chunk get zeros); sh = 0: one mask per thread.
// cwk_bits_ingest with (T = masks, slots = n_in, sh = 0, input_slot0 = 0) WRITES that form from a 32-byte image.
hipError_t cwk_bits_ingest_packed(hipStream_t s, const void *masks, void *T, uint64_t slots, uint32_t sh, uint32_t input_slot0, uint32_t n_in,
                                  uint32_t batch);
hipError_t cwk_bits_collect_inputs(hipStream_t s, const void *masks, const void *aos, const uint32_t *inst, uint32_t n_inst,
                                   uint32_t n_in, void *out);
// boolean inputs as packed rows (cw_set_inputs_rows*, cw_rows.h): d_rows 8-byte aligned, stride a multiple of 8 and at least
// 8 * ceil(n_in / 64); input k of instance j = bit k & 7 (msb: 7 - (k & 7)) of byte k >> 3 of row j.
//   cwk_bits_rows_to_masks  the bit transpose into masks[ceil(batch / 64)][n_in], the form cwk_bits_ingest_packed reads
//   cwk_rows_expand         (cw_kernels.hip; any stride >= ceil(n_in / 8), any alignment of d_rows) the image [batch][n_in][elem_bytes]
//                           of values 0 / 1, elem_bytes = 8 or 32, `out` 16-byte aligned: what cwk64_ingest* / cwk_ingest read
hipError_t cwk_bits_rows_to_masks(hipStream_t s, const void *d_rows, size_t stride, uint32_t n_in, uint32_t batch, bool msb, void *d_masks);
hipError_t cwk_rows_expand(hipStream_t s, const void *d_rows, size_t stride, uint32_t n_in, uint32_t batch, bool msb, void *out,
                           uint32_t elem_bytes);
// input columns (cw_set_inputs_range*, cw_set_input_column*; cw_columns.h, cw_columns.hip.h): instance j's n values of `width`
// bytes (1, 2, 4, 8 or 32; little-endian) at d_values + j * stride (0: the same n values for every instance) become the run
// out + j * out_stride of n elements of 32 bytes (cwk_columns: values as they stand) or 8 bytes (cwk64_columns: 8- and 32-byte
// values reduced mod p).  d_values and stride aligned to `width` (16 for 32), out and out_stride to 16 / 8.  One launch.
hipError_t cwk_columns(hipStream_t s, const void *d_values, size_t stride, uint32_t n, uint32_t count, uint32_t width, void *out,
                       size_t out_stride);
hipError_t cwk64_columns(hipStream_t s, const void *d_values, size_t stride, uint32_t n, uint32_t count, uint32_t width, void *out,
                         size_t out_stride);
// witness bits OUT as packed rows (cw_get_witness_rows*, cw_rows.h), one kernel per table layout: entry k of the range (wslot / w2s
// point at its first entry) of instance first + j = bit k & 7 (msb: 7 - (k & 7)) of byte k >> 3 of d_rows + j * stride, 1 iff the
// value is 1; rows of 8 * ceil(n / 64) bytes are written, pad bits 0.  d_rows 8-byte aligned, stride a multiple of 8 and at least
// that.  The two value tables report a value that is neither 0 nor 1 by atomicMin(d_word, report0 + j); d_word may be nullptr, the
// caller fills it (cwk_fill32) first.  A bit table holds no such value.
hipError_t cwk_bits_masks_to_rows(hipStream_t s, const void *T, uint64_t slots, uint32_t sh, const uint32_t *wslot, uint32_t n, uint32_t first,
                                  uint32_t count, bool msb, void *d_rows, size_t stride);
hipError_t cwk64_pack_rows(hipStream_t s, const void *V, const uint32_t *w2s, uint32_t n, uint32_t Bp, uint32_t first, uint32_t count,
                           uint32_t report0, bool msb, void *d_rows, size_t stride, uint32_t *d_word);
hipError_t cwk_pack_rows(hipStream_t s, const void *V, const uint32_t *w2s, uint32_t n, uint32_t Bp, uint32_t first, uint32_t count,
                         uint32_t report0, bool msb, void *d_rows, size_t stride, uint32_t *d_word, bool mont, const FpParams &P);
// signal columns OUT (cw_get_signals_range*, cw_signals.h), one kernel per table layout: value k of row j = signal signal0 + k
// (signal ids, not witness-list positions) of instance first + j, the canonical residue as a little-endian unsigned integer of
// elem_bytes (1, 2, 4, 8 or 32) at d_values + j * stride + k * elem_bytes, j < count; only those n * elem_bytes bytes of a row
// are written.  d_values and stride are multiples of elem_bytes (of 16 for 32).  The two value tables report a value >= 2^(8
// elem_bytes) - stored as its low bytes - by atomicMin(d_word, report0 + j); d_word may be nullptr, the caller fills it
// (cwk_fill32) first.  A bit table (sigslot: the batch's signal -> slot map on the device) holds 0 / 1 only.  cwk_signals with
// `remap` (n_remap entries) reads row j from column remap[first + j] of its table where that is in [0, batch) and leaves every
// other row alone: the rows of a side batch written over those of the bit table, as cwk_gather_at does it for a list.
hipError_t cwk_bits_signals(hipStream_t s, const void *T, uint64_t slots, uint32_t sh, const uint32_t *sigslot, uint32_t signal0, uint32_t n,
                            uint32_t first, uint32_t count, void *d_values, size_t stride, uint32_t elem_bytes);
hipError_t cwk64_signals(hipStream_t s, const void *V, uint32_t signal0, uint32_t n, uint32_t Bp, uint32_t first, uint32_t count,
                         uint32_t report0, void *d_values, size_t stride, uint32_t elem_bytes, uint32_t *d_word);
hipError_t cwk_signals(hipStream_t s, const void *V, uint32_t signal0, uint32_t n, uint32_t Bp, uint32_t first, uint32_t count, uint32_t report0,
                       void *d_values, size_t stride, uint32_t elem_bytes, uint32_t *d_word, bool mont, const FpParams &P, uint32_t batch,
                       const int32_t *remap, uint32_t n_remap);
// R1CS products OUT (cw_get_r1cs_products*, cw_r1cs_products.h), one kernel per table layout: d_out[j][p][k] = the p-th part of
// `parts` (bits 0 / 1 / 2 = A / B / C, in that order) of constraint row0 + k of the .r1cs file in instance first + j, canonical
// residues of 32 bytes (d_out 16-byte aligned) or, 64-bit runtime, 8 bytes (8-byte aligned); dense, count x popcount(parts) x
// n_rows elements.  rowptr / terms: the plan in file order ({slot, coefficient id} / {bit-table slot, id into cctab} / {slot, 0,
// coefficient lo, hi}); ctab / ctab29: the check's coefficient tables.
hipError_t cwk_products(hipStream_t s, const void *V, const uint32_t *rowptr, const uint32_t *terms, const uint32_t *ctab, const uint32_t *ctab29,
                        uint32_t parts, uint32_t row0, uint32_t n_rows, uint32_t Bp, uint32_t first, uint32_t count, void *d_out, bool mont,
                        const FpParams &P);
hipError_t cwk_bits_products(hipStream_t s, const void *T, uint64_t slots, uint32_t sh, const uint32_t *rowptr, const uint32_t *terms,
                             const uint32_t *cctab, uint32_t parts, uint32_t row0, uint32_t n_rows, uint32_t first, uint32_t count, void *d_out,
                             const FpParams &P);
hipError_t cwk64_products(hipStream_t s, const void *V, const uint32_t *rowptr, const void *terms, uint32_t parts, uint32_t row0, uint32_t n_rows,
                          uint32_t Bp, uint32_t first, uint32_t count, void *d_out);
// witness digests (cw_get_wtns_digests*, cw_wtns_digest.h), one kernel per table layout: d_out[j] = the 32 bytes of SHA-256 over the
// .wtns file of instance first + j (header of `plan`, then the entries of w2s / wslot as canonical little-endian elements of
// plan.n8 bytes), j < count; d_out 16-byte aligned.  Lane = instance, one wave per table group of 64 instances that the range
// touches; nothing else is written.
hipError_t cwk_wtns_digest(hipStream_t s, const void *V, const uint32_t *w2s, uint32_t Bp, uint32_t first, uint32_t count, void *d_out,
                           const cwdig::Plan &plan, bool mont, const FpParams &P);
hipError_t cwk_bits_wtns_digest(hipStream_t s, const void *T, uint64_t slots, uint32_t sh, const uint32_t *wslot, uint32_t first, uint32_t count,
                                void *d_out, const cwdig::Plan &plan);
hipError_t cwk64_wtns_digest(hipStream_t s, const void *V, const uint32_t *w2s, uint32_t Bp, uint32_t first, uint32_t count, void *d_out,
                             const cwdig::Plan &plan);
// instance lists (cw_select_instances*, cw_get_witnesses_at*, cw_select.h).
//   cwk_select        d_idx[0 .. *d_n) = the instances i < batch with (w(i) & mask) == want, ascending; w(i) = status[i], or, with
//                     fbidx (instance -> position in the side batch or negative) and fbidx[i] in [0, n_fb), fbstatus[fbidx[i]].
//                     Three launches (count, scan, scatter; no workgroup waits for another); `counts`: scratch of
//                     cwsel::n_blocks(batch) words; d_idx == nullptr: *d_n only.
//   cwk*_at           the range egress kernel of each table layout with a list for the range (cwk_gather_many, cwk_bits_gather,
//                     cwk64_egress: the AT = true instantiations, one launcher body per pair): d_out[j][k] = entry k of the range (wslot / w2s point at its first entry) of
//                     instance d_idx[j], j < min(n_idx, *d_n_idx) (d_n_idx may be nullptr), canonical, 32 bytes (d_out 16-byte
//                     aligned) or, cwk64_egress_at with elem_bytes = 8, 8 bytes (8-byte aligned).  A position whose index is
//                     >= batch gets zeros and atomicMin(d_bad, position); d_bad may be nullptr, the caller fills it first.
//                     cwk_gather_at with `remap` (n_remap entries) reads instance remap[d_idx[j]] of its table and leaves the
//                     rows alone whose entry is negative: the rows of a side batch written over those of the bit table.
hipError_t cwk_select(hipStream_t s, const uint32_t *status, uint32_t batch, uint32_t mask, uint32_t want, const int32_t *fbidx,
                      const uint32_t *fbstatus, uint32_t n_fb, uint32_t *counts, uint32_t *d_idx, uint32_t *d_n);
hipError_t cwk_gather_at(hipStream_t s, const void *V, const uint32_t *w2s, uint32_t n_wit, uint32_t Bp, uint32_t batch, const uint32_t *d_idx,
                         uint32_t n_idx, const uint32_t *d_n_idx, const int32_t *remap, uint32_t n_remap, void *d_out, uint32_t *d_bad,
                         bool mont, const FpParams &P);
hipError_t cwk_bits_gather_at(hipStream_t s, const void *T, uint64_t slots, uint32_t sh, const uint32_t *wslot, uint32_t n_wit, uint32_t batch,
                              const uint32_t *d_idx, uint32_t n_idx, const uint32_t *d_n_idx, void *d_out, uint32_t *d_bad);
hipError_t cwk64_egress_at(hipStream_t s, const void *V, const uint32_t *w2s, uint32_t n_wit, uint32_t Bp, uint32_t batch, const uint32_t *d_idx,
                           uint32_t n_idx, const uint32_t *d_n_idx, void *d_out, uint32_t elem_bytes, uint32_t *d_bad);
// witness compare (cw_compare_witnesses*, cw_compare.h): the range egress kernel of each table layout with its store turned into
// a streaming load and a compare.  image[j][k] = entry k of the range (wslot / w2s point at its first entry, which is entry0 of
// the witness list) of instance first + j, [count][n_wit] elements of 32 bytes (16-byte aligned) or, cwk64_compare with
// elem_bytes = 8, 8 bytes (8-byte aligned).  diff[j] takes atomicMin(lowest differing entry0 + k); the workgroup that finds
// 0xFFFFFFFF there counts the instance: summary[0] += 1, summary[1] = min(.., report0 + j) (`summary` may be nullptr).  The
// caller fills diff[0 .. count) with 0xFFFFFFFF and summary with {0, 0xFFFFFFFF} first.
//   cwk_compare        with `remap` (n_remap entries, indexed by first + j) the kernel reads column remap[first + j] < limit of its
//                      table and leaves alone the positions whose entry is negative: the instances a bit-plane batch re-ran,
//                      judged from the side batch's table
//   cwk_bits_compare   with `fbidx` (the same map) those instances are skipped: they are not judged from the bit table
hipError_t cwk_compare(hipStream_t s, const void *V, const uint32_t *w2s, uint32_t n_wit, uint32_t Bp, uint32_t first, uint32_t count,
                       uint32_t entry0, uint32_t report0, const void *image, const int32_t *remap, uint32_t n_remap, uint32_t limit,
                       uint32_t *diff, uint32_t *summary, bool mont, const FpParams &P);
hipError_t cwk_bits_compare(hipStream_t s, const void *T, uint64_t slots, uint32_t sh, const uint32_t *wslot, uint32_t n_wit, uint32_t first,
                            uint32_t count, uint32_t entry0, uint32_t report0, const void *image, const int32_t *fbidx, uint32_t *diff,
                            uint32_t *summary);
hipError_t cwk64_compare(hipStream_t s, const void *V, const uint32_t *w2s, uint32_t n_wit, uint32_t Bp, uint32_t first, uint32_t count,
                         uint32_t entry0, uint32_t report0, const void *image, uint32_t elem_bytes, uint32_t *diff, uint32_t *summary);
hipError_t cwk_bits_r1cs(hipStream_t s, const void *erecs, uint32_t n_evrows, const uint32_t *chunk, uint32_t n_chunks,
                         const uint32_t *terms, const uint32_t *ctab, const uint32_t *row_orig, const uint32_t *ichunk,
                         uint32_t n_ichunks, const uint32_t *iterms, const uint32_t *itab, const uint32_t *irow_orig, const void *T,
                         uint64_t slots, uint32_t sh, const void *only, uint32_t n_groups, uint32_t batch, uint32_t *status, uint32_t *first_bad,
                         const FpParams &P);

// ---- 64-bit runtime (cw64.hip: --prime goldilocks) ----
// A call that needs several launches (cw_pieces.h: a grid dimension holds 65 535) checks every launch and launches nothing behind
// one that failed; the bit-plane launchers above do the same.
hipError_t cwk64_init(hipStream_t s, void *V, uint32_t Bp, uint32_t *status, uint32_t *first_bad);
// inputs [batch][n_in][elem_bytes], elem_bytes = 8 or 32: lane = instance (n_in <= 65 535) / a tiled transpose (8: `in` 8-byte
// aligned, 32: 16-byte aligned; any n_in)
hipError_t cwk64_ingest(hipStream_t s, const void *in, void *V, uint32_t input_start, uint32_t n_in, uint32_t batch, uint32_t Bp,
                        uint32_t elem_bytes);
hipError_t cwk64_ingest_tiled(hipStream_t s, const void *in, void *V, uint32_t input_start, uint32_t n_in, uint32_t batch, uint32_t Bp,
                              uint32_t elem_bytes);
// calls: 0 = no O_CALL row in the program (ftab / fcode unused), 1 = register windows of run-time functions in the value table,
// 2 = in LDS, lds_bytes = 512 x the registers of the largest function (<= 64 KiB); ftab / fcode: cw_fn64.h
hipError_t cwk64_eval(hipStream_t s, const void *rows, uint32_t n_rows, const void *consts, void *V, uint32_t Bp, uint32_t batch,
                      uint32_t *status, const void *ftab, const void *fcode, uint32_t calls, uint32_t lds_bytes);
hipError_t cwk64_r1cs(hipStream_t s, const void *chunks, uint32_t n_chunks, const void *terms, const void *V, uint32_t Bp, uint32_t batch,
                      uint32_t *status, uint32_t *first_bad);
hipError_t cwk64_gather(hipStream_t s, const void *V, const uint32_t *w2s, uint32_t n_wit, uint32_t Bp, uint32_t first, uint32_t count,
                        void *out);
// bulk egress as a tiled transpose: [count][n_wit][elem_bytes], elem_bytes = 8 or 32 (32: `out` 16-byte aligned)
hipError_t cwk64_egress(hipStream_t s, const void *V, const uint32_t *w2s, uint32_t n_wit, uint32_t Bp, uint32_t first, uint32_t count,
                        void *out, uint32_t elem_bytes);
// supplied witnesses, the same transpose the other way (the kernel of cwk64_ingest_tiled, cw64_transpose_in_kernel, with the
// witness list for the slots): [count][n_wit][elem_bytes] -> V[w2s[k]][first + j], entry 0 excepted; CW_ST_BAD_WITNESS into
// status[first + j] for a value that is not canonical or an entry 0 that is not 1 (8: `in` 8-byte aligned, 32: 16-byte aligned)
hipError_t cwk64_wit_ingest(hipStream_t s, const void *in, void *V, const uint32_t *w2s, uint32_t n_wit, uint32_t Bp, uint32_t first,
                            uint32_t count, uint32_t *status, uint32_t elem_bytes);
