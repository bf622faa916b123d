// cw_bits.hip — bit-plane kernels (gfx950 / CDNA4) for circuits whose signals are all provably boolean.
//
// Reference counterpart: the emitted calculator runs such circuits (SHA-256, Num2Bits gadgets) through the short-int
// paths of the tagged field library (generic/fr.cpp:416-439 mul_s1s2, 696-701, 900-917 add_s1s2, 1799-1988 Fr_band)
// on 40-byte FrElements, one instance at a time.  Here a boolean signal costs ONE BIT per instance:
//
//   bit table   T[group][slot] : uint64, bit i = value of the signal in instance group*64 + i      (HBM)
//               slot 0 = constant 0, slot 1 = constant 1 (all ones), slot 2 reserved, signal s = 3 + s, then temps
//
// and the witness program is a sequence of VROWS (hip_elements/bitsched.py): one wave = one group of 64 instances,
// in a vrow every LANE evaluates one 3-input gate of the network on 64-bit masks (64 gates x 64 instances per ~60
// VALU instructions).  Results go to the wave's LDS ring (entry vrow mod R) and to up to four bit-table slots;
// operands and results are entries of the wave's LDS (result ring + cached rows of the bit table); vector memory moves
// whole rows at batch boundaries.  No barriers: a single wave, in-order LDS and in-order vector memory.
//
// The assumption "main inputs are 0/1" is checked by the ingest kernel; instances that violate it, or trip an
// assertion gate, are flagged in fbmask[group] and re-evaluated by the 256-bit schedule (cw_host.cpp), so every
// result is the reference's for every input.
#include <hip/hip_runtime.h>
#include "cw_kernels.h"
#include "cw_bits_layout.h"
#include "cw_pieces.h"
#include "cw_r1cs_products.h"
#include "fp256.hip.h"
#include "cw_list.hip.h"
#include "cw_compare.hip.h"
#include "cw_wtns_digest.h"


typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// ---- table layout ---------------------------------------------------------------------------------------------------------
// Two layouts share every kernel below through the shift `sh` (a launch parameter):
//   sh = 0   T[group][slot]                      the interpreter's table: a group's slots are consecutive uint64 (rows of 64 slots)
//   sh = 5   T[chunk][slot][group in chunk]      the emitted code's table (hip_elements/bitjit.py): a chunk = 32 groups = 2 048
//                                                instances, a slot of a chunk = one 256-byte row (lane l of the emitting wave
//                                                holds dword l: instances 32 l .. 32 l + 31 of the chunk)
// element (group g, slot s) = T[(((g >> sh) * slots + s) << sh) + (g & ((1 << sh) - 1))]: the slots of a group are
// (1 << sh) uint64 apart, starting at bits_group(T, slots, sh, g).  The formula itself is cw_bits_layout.h's (HIP-free: a host
// test walks the same lines).
__device__ __forceinline__ uint64_t *bits_group(uint64_t *T, uint64_t slots, uint32_t sh, uint32_t g) {
    return T + cwlayout::group_base(slots, sh, g);
}
__device__ __forceinline__ const uint64_t *bits_group(const uint64_t *T, uint64_t slots, uint32_t sh, uint32_t g) {
    return T + cwlayout::group_base(slots, sh, g);
}

// ---- init: constant slots, flags -------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) cw_bits_init_kernel(uint64_t *T, uint64_t slots, uint32_t sh, uint32_t n_groups, uint64_t *fbmask,
                                                            uint64_t *r1flag, uint32_t *status, uint32_t *first_bad, uint32_t Bp) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < n_groups) {
        uint64_t *Tg = bits_group(T, slots, sh, i);
        Tg[(size_t)0 << sh] = 0;
        Tg[(size_t)1 << sh] = ~0ull;
        Tg[(size_t)2 << sh] = 0;
        fbmask[i] = 0;
        if (r1flag) r1flag[i] = 0;
    }
    if (i < Bp) {
        status[i] = 0;
        first_bad[i] = 0xFFFFFFFFu;
    }
}

// ---- ingest: AoS canonical inputs [batch][n_in][32 B] -> one mask per (group, input) -----------------------------------
// (setInputSignal's `signalValues[si] = val`, calcwit.cpp:93, for 64 instances at a time).  A workgroup of four waves handles
// 256 consecutive inputs of one group and walks the group's 64 instances: every pair of load instructions of a wave reads 2 KiB
// contiguous, the workgroup 8 KiB of one instance's 32 n_in-byte record; the value's low bit is shifted into a mask per input,
// beside it a "not a bit" mask (values other than 0/1 flag their instance: one atomicOr per offending lane, none in the loop).
// In the first body (cw_bits_ingest_halves_kernel, below the kernel) thread t owns input c * 256 + t and a wave's 64 masks
// leave as one store instruction; the table below is that body's.
// Order matters more than the loop body (tools/ubench_ingest.hip, profiles/r05n_ubench_ingest*.txt, 137 GB of inputs; a
// read-only uint4 sum of the same buffer reaches 6.45 TB/s on the same box):
//   one wave per workgroup, groups fastest (rounds 3-5)                        24.2 ms   5.69 TB/s
//   the same with 4 / 8 / 16 loads in flight per wave (unrolled, lane flags)    24.3-24.5 (round 3: streaming loads 26.4; round 5:
//                                                                               whole-line loads 24.3-24.7)
//   chunks of one group fastest                                                 28.3 ms: the waves that run together march through
//                                                                               the 64 KB records of their groups in step
//   chunks fastest + every group starts at its own instance (hash(g) & 63)      23.4 ms
//   that, four waves per workgroup on consecutive chunks, unrolled x 4          22.2 ms   6.19 TB/s   <- the walk of both bodies
//   (two waves 22.6, eight 23.2, sixteen 23.3; unrolled x 2 22.9, x 8 22.5; no rotation 24.0-24.4)
// Where the final store lands is the caller's choice of (T, slots, sh, input_slot0).  Into the interpreter's table (sh = 0) a
// wave's store is 512 contiguous bytes.  Into the emitted code's table (sh = 5) its 64 lanes would hit 64 different 256-byte rows,
// 8 bytes each, and the 32 groups that complete a row belong to 32 workgroups that finish at different times: 67 M write requests
// of one 64-byte piece per 8 bytes of payload at the benchmark shape.  An emitted-code batch therefore points this kernel at a
// staging buffer of packed masks (cw_host.cpp bits_run: T = d_stage, slots = n_in, sh = 0, input_slot0 = 0, which IS
// masks[group][k]) and cw_bits_masks_to_table_rows_kernel below writes the table from there in whole rows.  This kernel's source
// and launch geometry are the same on both routes.
//
// HOW THE BYTES TRAVEL (tools/ubench_ingest.hip `ingest_line`, profiles/ingest_line_once_ubench.txt: three processes on the
// 137.44 GB, every form checked against the same table and flag checksums; ms = average of six launches, per process):
//   lane = one input, two 16-byte loads at a lane stride of 32 (the first body)     23.19  22.64  23.18   <- CW_BITS_INGEST_LINE=0
//   lane = one 16-byte piece (below), plain loads                                    24.58  23.64  24.60
//   the same, streaming (nt) loads                                                   21.88  21.57  21.83
//   LDS-DMA into a ring of 4 KiB per wave, default policy                            23.93  22.99  23.95
//   ... 8 KiB                                                                        23.97  23.09  23.99
//   ... 16 KiB                                                                       23.27  22.67  23.25
//   LDS-DMA, nt, ring of 4 KiB per wave                                              21.68  21.25  21.66
//   LDS-DMA, nt, ring of 8 KiB per wave                                              21.64  21.50  21.64
//   LDS-DMA, nt, ring of 16 KiB per wave                                             21.39  21.16  21.40   <- this kernel
//   read only, same map: plain nt loads 19.84 / 20.12 / 19.86; LDS-DMA nt, 8 KiB 19.76 / 20.03 / 19.76 (6.83 - 6.96 TB/s)
// That table is the tool's own layout (sh = 5, the direct route's scattered store), where the first body pays 1.0 - 1.5 ms for its
// stores and this one does not.  With a group's masks contiguous (sh = 0: the staged route, the interpreter's table; part 2 of the
// same file) the first body runs 21.68 / 21.91 / 22.08 and this kernel 21.32 / 22.00 / 21.80: inside the spread of the processes.
// What decided is the library on the benchmark (profiles/ingest_line_once_parent_vs_new.json, three processes each, alternating):
// table init + ingest + row writer 21.90 - 21.92 -> 21.45 - 21.47 ms, the step 32.69 - 32.72 -> 32.25 - 32.27 ms (+1.3 % witnesses/s
// between the nearest runs, own ranges 0.08 %), the emitted kernel behind it 10.74 -> 10.75 ms; FETCH_SIZE of a launch
// 138.04 GB = 1.0044 x the image -> 137.44 GB = 1.0000 x.  Building the masks by rotation (v_alignbit_b32, 7 instead of ~13 VALU
// instructions per piece) changed nothing: the VALU work is not what separates the kernel from the read-only line.
// With two loads of 16 bytes at a stride of 32 both instructions of a pair touch all 16 lines of the wave's 2 KiB run, half of each;
// with eight loads per lane in flight a line can leave the L2 between its halves (the counters showed 1.04 x the image).  Here lane l
// of load h takes piece 64 h + l of the run (cw_bits_layout.h line_*): one instruction = 1 KiB contiguous, a line belongs to one
// instruction, so nothing is read twice and the streaming policy has nothing to lose: it is what moves the time (plain loads in
// this map are slower than the old body).  Even lanes hold the low half of an input (its bit, and "more than 0 / 1"), odd lanes
// the high half (any non-zero dword); one lane exchange after the loop ORs the odd lane's flags into its even neighbour's, the
// even lanes store (32 masks = 256 contiguous bytes per instruction when sh = 0) and raise fbmask.  No cross-lane operation in the loop.
//
// The ring: a wave owns BITS_LINE_RING slots of 1 KiB of LDS; load n = 2 ii + h lands in slot n % BITS_LINE_RING, lane l's piece at
// byte 16 l, and the lane that asked reads it back (ds_read_b128 at slot * 1024 + 16 l: no transposition).  Bank arithmetic of
// the read-back: ds_read_b128 is served in four groups of 16 consecutive lanes; a group reads 256 consecutive bytes = dwords
// 64 q .. 64 q + 63 of the slot, every one of the 64 banks exactly once: no conflict (by the documented bank rules; no counter
// pass was taken).  hipcc neither sees the asm reads nor orders the DMA against them, so the waits are ours
// (cw_bits_layout.h line_ring_*): the wave works in batches of BITS_LINE_RING / 2 loads; `s_waitcnt vmcnt(P)` ahead of a batch's
// reads, P = line_ring_pending = the loads issued BEHIND the batch (the wave issues no other vector memory operation inside the
// loop: the stores and the atomic come after it; loads return in order); `s_waitcnt lgkmcnt(0)` after the reads and ahead of
// the DMAs that re-target their slots.  Checked in the disassembly: each group of ds_read_b128 follows its vmcnt, no
// global_load_lds of a slot stands between that slot's read and the lgkmcnt(0), nothing touches a read's registers before it.
// 16 slots = 16 KiB per wave, 64 KiB per workgroup: two workgroups per CU, 2 waves per SIMD, 32 loads of 1 KiB in flight per SIMD.
// A ragged last group (fewer than 64 instances) walks its instances in order with plain loads of the same map.
// kernel-resource-usage (gfx950):   old body  50 VGPRs, 35 SGPRs, no LDS, 8 waves per SIMD, no scratch
//                                   this      112 VGPRs, 98 SGPRs, 65 536 bytes of LDS, 2 waves per SIMD (the LDS decides), no scratch
#define BITS_INGEST_WAVES 4
#define BITS_LINE_RING 16
static_assert(BITS_INGEST_WAVES == cwlayout::LINE_WAVES, "the workgroup of both ingest bodies");
struct BitsLineAcc {
    uint64_t bit[2], bad[2];
    uint32_t thr;                                                    // even lanes (low halves) 1, odd lanes 0: cwlayout::line_bad
    __device__ __forceinline__ void take(int h, const u32x4 v, uint32_t inst) {
        bit[h] |= (uint64_t)(v.x & 1u) << inst;
        bad[h] |= (uint64_t)((uint32_t)(v.x > thr) | (uint32_t)((v.y | v.z | v.w) != 0u)) << inst;
    }
};
__device__ __forceinline__ void bits_line_dma(const uint4 *src, uint32_t lds_byte) {          // 64 lanes x 16 bytes -> lds_byte + 16 lane, nt
    __builtin_amdgcn_global_load_lds((__attribute__((address_space(1))) void *)src, (__attribute__((address_space(3))) void *)(uintptr_t)lds_byte,
                                     16, 0, 2);
}
// batch b of the ring: wait until at most PENDING of the wave's loads are in flight, read the batch's slots, wait for the reads,
// hand the slots to the loads BITS_LINE_RING further on, then use what was read
template <int PENDING, bool REFILL, int HALF>
__device__ __forceinline__ void bits_line_batch(uint32_t b, BitsLineAcc &A, const uint4 *base, size_t step, const uint32_t (&o)[2], uint32_t r,
                                                uint32_t ring, uint32_t lane16) {
    constexpr int D = BITS_LINE_RING, BT = (int)cwlayout::line_ring_batch(D);
    u32x4 v[BT];
    asm volatile("s_waitcnt vmcnt(%0)" ::"i"(PENDING) : "memory");
#pragma unroll
    for (int j = 0; j < BT; j++)
        asm volatile("ds_read_b128 %0, %1" : "=v"(v[j]) : "v"(ring + cwlayout::line_ring_byte(HALF * BT + j, 0) + lane16));
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int j = 0; j < BT; j++) asm volatile("" : "+v"(v[j]));     // nothing uses a read's registers above the wait
    if (REFILL) {
#pragma unroll
        for (int j = 0; j < BT; j++) {
            const uint32_t n = b * BT + j + D;
            bits_line_dma(base + cwlayout::line_instance(n >> 1, r) * step + o[j & 1], ring + cwlayout::line_ring_byte(HALF * BT + j, 0));
        }
    }
#pragma unroll
    for (int j = 0; j < BT; j++) A.take(j & 1, v[j], cwlayout::line_instance((b * BT + j) >> 1, r));
}
__global__ void __launch_bounds__(64 * BITS_INGEST_WAVES)
cw_bits_ingest_kernel(const uint4 *__restrict__ in, uint64_t *__restrict__ T, uint64_t slots, uint32_t sh, uint32_t input_slot0, uint32_t n_in,
                      uint32_t batch, uint64_t *fbmask, uint32_t n_chunks) {
    using namespace cwlayout;
    constexpr uint32_t D = BITS_LINE_RING, BT = line_ring_batch(D), NB = LINE_RING_LOADS / BT;
    static_assert(D % 4 == 0 && LINE_RING_LOADS % D == 0 && NB % 2 == 0 && NB >= 4, "whole rounds of the ring; both loads of an instance in one batch");
    static_assert(line_ring_pending(D, 0) == BT && line_ring_pending(D, NB - 3) == BT && line_ring_refills(D, NB - 3), "steady state");
    static_assert(line_ring_pending(D, NB - 2) == BT && !line_ring_refills(D, NB - 2), "the last batch but one");
    static_assert(line_ring_pending(D, NB - 1) == 0 && !line_ring_refills(D, NB - 1), "the last batch");
    __shared__ uint4 ring_lds[BITS_INGEST_WAVES * D * (LINE_SLOT_BYTES / 16)];
    const uint32_t c = blockIdx.x % n_chunks, g = blockIdx.x / n_chunks;
    const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t k0 = line_wave_input0(c, wave);
    if (k0 >= n_in) return;                                          // the whole wave; no barrier below
    const uint32_t i0 = g * 64, ni = min(64u, batch - i0);
    const uint32_t p[2] = {line_piece(k0, 0, lane), line_piece(k0, 1, lane)};
    const bool act[2] = {line_piece_active(p[0], n_in), line_piece_active(p[1], n_in)};
    // an inactive lane reads the wave's first piece again (valid memory, a line the wave reads anyway) and drops it at the end
    const uint32_t o[2] = {act[0] ? p[0] : 2u * k0, act[1] ? p[1] : 2u * k0};
    const uint4 *base = in + (size_t)i0 * n_in * 2;
    const size_t step = (size_t)n_in * 2;
    BitsLineAcc A;
    A.bit[0] = A.bit[1] = A.bad[0] = A.bad[1] = 0;
    A.thr = line_piece_half(lane) ? 0u : 1u;
    if (ni == 64) {
        const uint32_t r = line_group_start(g);
        const uint32_t ring = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint4 *)ring_lds + wave * (D * LINE_SLOT_BYTES);
        const uint32_t lane16 = line_ring_byte(0, lane);
#pragma unroll
        for (uint32_t n = 0; n < D; n++) bits_line_dma(base + line_instance(n >> 1, r) * step + o[n & 1], ring + line_ring_byte(line_ring_slot(n, D), 0));
        for (uint32_t b = 0; b + 2 < NB; b += 2) {
            bits_line_batch<BT, true, 0>(b, A, base, step, o, r, ring, lane16);
            bits_line_batch<BT, true, 1>(b + 1, A, base, step, o, r, ring, lane16);
        }
        bits_line_batch<BT, false, 0>(NB - 2, A, base, step, o, r, ring, lane16);
        bits_line_batch<0, false, 1>(NB - 1, A, base, step, o, r, ring, lane16);
    } else {
        const uint4 *q = base;
        for (uint32_t ii = 0; ii < ni; ii++) {
            const u32x4 v0 = *(const u32x4 *)(q + o[0]), v1 = *(const u32x4 *)(q + o[1]);
            q += step;
            A.take(0, v0, ii);
            A.take(1, v1, ii);
        }
    }
#pragma unroll
    for (int h = 0; h < 2; h++) {
        if (!act[h]) A.bit[h] = A.bad[h] = 0;
        A.bad[h] |= (uint64_t)__shfl_xor((unsigned long long)A.bad[h], 1);        // the odd lane holds the other half of the same input
    }
    if (!line_piece_half(lane)) {
        uint64_t *Tg = bits_group(T, slots, sh, g);
#pragma unroll
        for (int h = 0; h < 2; h++)
            if (act[h]) Tg[(size_t)(input_slot0 + line_piece_input(p[h])) << sh] = A.bit[h];
        const uint64_t bad = A.bad[0] | A.bad[1];
        if (bad) atomicOr((unsigned long long *)&fbmask[g], (unsigned long long)bad);
    }
}
// the parent's body (CW_BITS_INGEST_LINE=0): lane = one input, two 16-byte loads at a lane stride of 32
__global__ void __launch_bounds__(64 * BITS_INGEST_WAVES)
cw_bits_ingest_halves_kernel(const uint4 *__restrict__ in, uint64_t *__restrict__ T, uint64_t slots, uint32_t sh, uint32_t input_slot0, uint32_t n_in,
                             uint32_t batch, uint64_t *fbmask, uint32_t n_chunks) {
    const uint32_t c = blockIdx.x % n_chunks, g = blockIdx.x / n_chunks;
    const uint32_t k = c * (64 * BITS_INGEST_WAVES) + threadIdx.x;
    if (k >= n_in) return;                                           // no cross-lane operation below
    const uint32_t i0 = g * 64, ni = min(64u, batch - i0);
    uint64_t mine = 0, bad = 0;
    const uint4 *base = in + ((size_t)i0 * n_in + k) * 2;
    const size_t step = (size_t)n_in * 2;
    if (ni == 64) {
        const uint32_t r = (g * 0x9E3779B1u) >> 26;                  // the group's first instance
#pragma unroll 4
        for (uint32_t ii = 0; ii < 64; ii++) {
            const uint32_t inst = (ii + r) & 63u;
            const uint4 *p = base + inst * step;
            const uint4 lo = p[0], hi = p[1];
            const uint32_t rest = lo.y | lo.z | lo.w | hi.x | hi.y | hi.z | hi.w;
            mine |= (uint64_t)(lo.x & 1u) << inst;
            bad |= (uint64_t)((lo.x > 1u) | (rest != 0u)) << inst;
        }
    } else {
        const uint4 *p = base;
        for (uint32_t ii = 0; ii < ni; ii++) {
            const uint4 lo = p[0], hi = p[1];
            p += step;
            const uint32_t rest = lo.y | lo.z | lo.w | hi.x | hi.y | hi.z | hi.w;
            mine |= (uint64_t)(lo.x & 1u) << ii;
            bad |= (uint64_t)((lo.x > 1u) | (rest != 0u)) << ii;
        }
    }
    bits_group(T, slots, sh, g)[(size_t)(input_slot0 + k) << sh] = mine;
    if (bad) atomicOr((unsigned long long *)&fbmask[g], (unsigned long long)bad);
}

// ---- the gate program ------------------------------------------------------------------------------------------------------
// Program model: hip_elements/bitsched.py (round 3).  The wave's LDS holds a RING of R result rows, a CACHE of C rows of
// the group's bit table and the constants 0 / ~0; every operand and every result of a lane is ONE LDS
// entry named in its 8-byte record:
//   w0 = a_off | K1 | K2 << 1 | b_off << 16        LDS byte offsets (multiples of 8); K1: stage 1 is AND (else XOR),
//   w1 = c_off | dst_off << 16                                                         K2: stage 2 is OR (else XOR)
//   result = K2 ? (u | c) : (u ^ c),  u = K1 ? (a & b) : (a ^ b)          two v_bitop3_b32 per 32 instances
// (bitmap.py maps every 3-input gate of the network onto this primitive; round 2 evaluated a lane-specific 8-bit truth
// table with 8 v_bfe + 14 v_bfi per vrow).  Vector memory moves whole 512-byte ROWS only, at batch boundaries, named in a
// per-batch command block that the wave reads through the scalar cache: row LOADS (bit table -> cache slot: main
// inputs, values that left the cache) and row FLUSHES (cache slot -> bit table: every row exactly once, when complete).
// Round 2's per-lane scattered stores and loads cost 23..48 clocks of the CU's memory pipeline per instruction with
// four waves per CU (tools/ubench_isa) - 2.5 of them per vrow: that was the bound of the kernel.
// W = instances per wave: 64 (one wave per group), or 32 / 16 (2 / 4 independent waves per group, each on its slice of
// every mask: small batches then spread over more CUs).
#define BITS_NB 8
#define BITS_MAX_LOADS 4
#define BITS_MAX_FLUSH 6
#define BITS_CMD_WORDS 24
#define BITS_AHEAD 8          // records are requested this many batches ahead (BITS_AHEAD + 1 register sets of 16 dwords).  vmcnt
                              // retires loads AND stores in order, so a record wait also waits for every row flush issued before the
                              // newest 4 * BITS_AHEAD operations: behind cold caches / TLBs (tools/bits_shape_bench.py with
                              // CW_BENCH_COLD=1) four batches of slack cost 1.31 ms, eight 1.18 (0.90 warm either way)
#ifndef BITS_STORE_AUX
#define BITS_STORE_AUX 2      // cache policy of the row flushes: nt (streaming).  A flushed row is dead for this kernel; with the default
                              // policy the 1.2 GB of rows a launch writes thrashed the 4 MB L2s and the in-order vmcnt made the record
                              // loads wait behind slow stores: 1.24 -> 0.91 ms for Sha256(2048) x 65 536 (tools/bits_shape_bench.py)
#endif
#define BITS_OOR 0xFFFFFFF0u

// v_bitop3_b32 table of a function of (s0, s1, s2): bit (s0 << 2 | s1 << 1 | s2)
constexpr uint32_t bitop3_stage1() {           // (a, b, K) -> K ? a & b : a ^ b
    uint32_t t = 0;
    for (int i = 0; i < 8; i++) {
        const int a = (i >> 2) & 1, b = (i >> 1) & 1, k = i & 1;
        t |= (uint32_t)(k ? (a & b) : (a ^ b)) << i;
    }
    return t;
}
constexpr uint32_t bitop3_stage2() {           // (u, c, K) -> K ? u | c : u ^ c
    uint32_t t = 0;
    for (int i = 0; i < 8; i++) {
        const int u = (i >> 2) & 1, c = (i >> 1) & 1, k = i & 1;
        t |= (uint32_t)(k ? (u | c) : (u ^ c)) << i;
    }
    return t;
}
static_assert(bitop3_stage1() == 0x94u && bitop3_stage2() == 0xBCu, "v_bitop3_b32 tables of the two primitive stages");
__device__ __forceinline__ uint32_t prim32(uint32_t a, uint32_t b, uint32_t c, uint32_t k1, uint32_t k2) {
    const uint32_t u = __builtin_amdgcn_bitop3_b32(a, b, k1, 0x94);
    return __builtin_amdgcn_bitop3_b32(u, c, k2, 0xBC);
}
// 3-input lookup on 64 instances with a wave-uniform or per-lane table (R1CS LUT class): index bit 0 = a, 1 = b, 2 = c
__device__ __forceinline__ uint32_t bfi32(uint32_t m, uint32_t a, uint32_t b) { return (a & m) | (b & ~m); }   // v_bfi_b32
__device__ __forceinline__ uint32_t lut3_32(uint32_t a, uint32_t b, uint32_t c, const uint32_t t[8]) {
    const uint32_t x0 = bfi32(a, t[1], t[0]), x1 = bfi32(a, t[3], t[2]), x2 = bfi32(a, t[5], t[4]), x3 = bfi32(a, t[7], t[6]);
    const uint32_t y0 = bfi32(b, x1, x0), y1 = bfi32(b, x3, x2);
    return bfi32(c, y1, y0);
}
__device__ __forceinline__ uint64_t lut3(uint64_t a, uint64_t b, uint64_t c, uint32_t tt) {
    uint32_t t[8];
#pragma unroll
    for (int m = 0; m < 8; m++) t[m] = (uint32_t)((int32_t)(tt << (31 - m)) >> 31);      // v_bfe_i32: 0 or ~0
    const uint32_t lo = lut3_32((uint32_t)a, (uint32_t)b, (uint32_t)c, t);
    const uint32_t hi = lut3_32((uint32_t)(a >> 32), (uint32_t)(b >> 32), (uint32_t)(c >> 32), t);
    return ((uint64_t)hi << 32) | lo;
}

template <int W> struct BitsMask;
template <> struct BitsMask<64> {
    typedef uint64_t T;
    static __device__ __forceinline__ T lds(uint32_t off) { return *(const __attribute__((address_space(3))) uint64_t *)(uintptr_t)off; }
    static __device__ __forceinline__ void lds_st(uint32_t off, T v) { *(__attribute__((address_space(3))) uint64_t *)(uintptr_t)off = v; }
    static __device__ __forceinline__ T load(__amdgpu_buffer_rsrc_t r, uint32_t off) {
        const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(r, (int)off, 0, 0);
        return ((uint64_t)v.y << 32) | v.x;
    }
    static __device__ __forceinline__ void store(__amdgpu_buffer_rsrc_t r, uint32_t off, T v) {
        const u32x2 x = {(uint32_t)v, (uint32_t)(v >> 32)};
        __builtin_amdgcn_raw_buffer_store_b64(x, r, (int)off, 0, BITS_STORE_AUX);
    }
    static __device__ __forceinline__ T prim(T a, T b, T c, uint32_t k1, uint32_t k2) {
        // one block: the compiler then waits ONCE for the three LDS operands instead of once per stage (a wave alone on
        // its SIMD issues one instruction of any kind per ~4 clocks: s_waitcnt instructions count)
        uint32_t lo, hi;
        asm("v_bitop3_b32 %0, %2, %4, %8 bitop3:0x94\n\t"
            "v_bitop3_b32 %1, %3, %5, %8 bitop3:0x94\n\t"
            "v_bitop3_b32 %0, %0, %6, %9 bitop3:0xbc\n\t"
            "v_bitop3_b32 %1, %1, %7, %9 bitop3:0xbc"
            : "=&v"(lo), "=&v"(hi)
            : "v"((uint32_t)a), "v"((uint32_t)(a >> 32)), "v"((uint32_t)b), "v"((uint32_t)(b >> 32)), "v"((uint32_t)c),
              "v"((uint32_t)(c >> 32)), "v"(k1), "v"(k2));
        return ((uint64_t)hi << 32) | lo;
    }
};
template <> struct BitsMask<32> {
    typedef uint32_t T;
    static __device__ __forceinline__ T lds(uint32_t off) { return *(const __attribute__((address_space(3))) uint32_t *)(uintptr_t)off; }
    static __device__ __forceinline__ void lds_st(uint32_t off, T v) { *(__attribute__((address_space(3))) uint32_t *)(uintptr_t)off = v; }
    static __device__ __forceinline__ T load(__amdgpu_buffer_rsrc_t r, uint32_t off) {
        return __builtin_amdgcn_raw_buffer_load_b32(r, (int)off, 0, 0);
    }
    static __device__ __forceinline__ void store(__amdgpu_buffer_rsrc_t r, uint32_t off, T v) {
        __builtin_amdgcn_raw_buffer_store_b32(v, r, (int)off, 0, 0);
    }
    static __device__ __forceinline__ T prim(T a, T b, T c, uint32_t k1, uint32_t k2) { return prim32(a, b, c, k1, k2); }
};
template <> struct BitsMask<16> {
    typedef uint32_t T;
    static __device__ __forceinline__ T lds(uint32_t off) { return *(const __attribute__((address_space(3))) uint32_t *)(uintptr_t)off; }
    static __device__ __forceinline__ void lds_st(uint32_t off, T v) { *(__attribute__((address_space(3))) uint32_t *)(uintptr_t)off = v; }
    static __device__ __forceinline__ T load(__amdgpu_buffer_rsrc_t r, uint32_t off) {
        return (uint32_t)__builtin_amdgcn_raw_buffer_load_b16(r, (int)off, 0, 0);
    }
    static __device__ __forceinline__ void store(__amdgpu_buffer_rsrc_t r, uint32_t off, T v) {
        __builtin_amdgcn_raw_buffer_store_b16((unsigned short)v, r, (int)off, 0, 0);
    }
    static __device__ __forceinline__ T prim(T a, T b, T c, uint32_t k1, uint32_t k2) { return prim32(a, b, c, k1, k2); }
};

extern __shared__ uint64_t cw_bits_lds[];        // ring rows | cache rows | constants 0, ~0

// One batch = BITS_NB vrows.  When batch b starts the wave requests the records of batch b + BITS_AHEAD (device stream: 4 x 16
// bytes per lane and batch) and the row loads of its command block; the BITS_NB steps then run on registers and LDS
// only (the operands of step k + 1 are read while step k computes: a consumer sits two vrows behind its producer); the
// rows requested by batch b - 1 are written to their cache slots before the last step reads the operands of the next
// batch's first vrow; the flushes of the command block copy cache slots to the bit table when the batch ends.
template <int W>
struct BitsEval {
    typedef BitsMask<W> M;
    typedef typename M::T mask_t;
    __amdgpu_buffer_rsrc_t rsrc, rrecs, rcmds;   // the group's bit table; the record stream; the command blocks
    uint32_t lane8;
    mask_t a, b, c;
    // command blocks travel in ONE VGPR each (lane j = word j, a 96-byte vector load a batch ahead) and are read with
    // v_readlane where a wave-uniform value is needed.  Scalar loads would be the natural fit, but they share the
    // LGKM counter with the LDS and return out of order: with one in flight hipcc turns every LDS wait into
    // lgkmcnt(0) - the pipelined operand reads of the next steps then serialise behind a ~200-clock scalar load.
    uint32_t cprev;

    static __device__ __forceinline__ uint32_t word(const uint4 (&r)[4], int k, int i) {
        const int d = 2 * k + i;
        const uint4 &q = r[d >> 2];
        return (d & 3) == 0 ? q.x : (d & 3) == 1 ? q.y : (d & 3) == 2 ? q.z : q.w;
    }
#ifdef CW_EXP_NOCMD       /* timing experiment only (tools/bits_exp.sh): every command block reads as empty */
    static __device__ __forceinline__ uint32_t cw(uint32_t, int) { return 0; }
#else
    static __device__ __forceinline__ uint32_t cw(uint32_t blk, int j) { return (uint32_t)__builtin_amdgcn_readlane((int)blk, j); }
#endif

    // records of batch b, load j: 1 KiB at (b * 4 + j) * 1024, lane l takes 16 bytes at l * 16 (32-bit lane offset +
    // scalar batch offset)
    __device__ __forceinline__ uint4 rec_load(uint32_t b, int j) const {
        const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rrecs, (int)(lane8 * 2), (int)((b * 4 + j) * 1024u), 0);
        return make_uint4(v.x, v.y, v.z, v.w);
    }
    __device__ __forceinline__ uint32_t cmd_load(uint32_t b) const {
        return __builtin_amdgcn_raw_buffer_load_b32(rcmds, (int)(lane8 >> 1), (int)(b * (BITS_CMD_WORDS * 4u)), 0);
    }

    __device__ __forceinline__ void batch(uint32_t bi, const uint4 (&cur)[4], const uint4 (&nxt)[4], uint4 (&fill)[4],
                                          const uint32_t ccur, uint32_t &cfill,
                                          const mask_t (&lprev)[BITS_MAX_LOADS], mask_t (&lfill)[BITS_MAX_LOADS]) {
        // the rows the PREVIOUS batch completed leave now: the first two (a batch completes 1.4 rows on average) are read
        // from the LDS before anything of this batch is written and stored a step later, without a wait on the spot
        const uint32_t pcounts = cw(cprev, 0), pn = pcounts & 0xFFu, fn = (pcounts >> 8) & 0xFFu;
        const mask_t fv0 = M::lds(cw(cprev, 3 + 2 * BITS_MAX_LOADS) + lane8);          // unused entries are 0: ring row 0
        const mask_t fv1 = M::lds(cw(cprev, 5 + 2 * BITS_MAX_LOADS) + lane8);
        const uint32_t nl = cw(ccur, 0) & 0xFFu;
        // row loads first: when they are awaited (a batch later) the unconditional record loads issued behind them stand
        // between, so the compiler's vmcnt never waits for a request younger than a batch
        if (nl) {                                   // rare (a few row loads per hundred batches): one branch in the common case
#pragma unroll
            for (int j = 0; j < BITS_MAX_LOADS; j++)
                if (j < (int)nl) lfill[j] = M::load(rsrc, cw(ccur, 2 + 2 * j) + lane8);
        }
#ifdef CW_EXP_NORECS      /* timing experiment only (tools/bits_exp.sh): no record fetch, every batch replays the first */
#pragma unroll
        for (int j = 0; j < 4; j++) fill[j] = cur[j];
#else
#pragma unroll
        for (int j = 0; j < 4; j++) fill[j] = rec_load(bi + BITS_AHEAD, j);
#endif
        // the command block travels with the records of its batch (same age in the in-order request queue: the wait for it
        // leaves the newer BITS_AHEAD - 1 batches of requests in flight.  Requested one batch ahead, as the first version of
        // this kernel did, its wait was a vmcnt(0) at the top of every batch: the queue drained 280 times a launch.)
        cfill = cmd_load(bi + BITS_AHEAD);
#pragma unroll
        for (int k = 0; k < BITS_NB; k++) {
            if (k == 1) {
                asm volatile("" ::"v"(fv0), "v"(fv1));          // the two reads are complete HERE on every path
                if (fn) {
                    M::store(rsrc, cw(cprev, 2 + 2 * BITS_MAX_LOADS) + lane8, fv0);
                    if (fn > 1) M::store(rsrc, cw(cprev, 4 + 2 * BITS_MAX_LOADS) + lane8, fv1);
                    if (fn > 2) {
#pragma unroll
                        for (int j = 2; j < BITS_MAX_FLUSH; j++)
                            if (j < (int)fn) M::store(rsrc, cw(cprev, 2 + 2 * BITS_MAX_LOADS + 2 * j) + lane8, M::lds(cw(cprev, 3 + 2 * BITS_MAX_LOADS + 2 * j) + lane8));
                    }
                }
            }
            if (k == BITS_NB - 1 && pn) {
#pragma unroll
                for (int j = 0; j < BITS_MAX_LOADS; j++)
                    if (j < (int)pn) M::lds_st(cw(cprev, 3 + 2 * j) + lane8, lprev[j]);
            }
            const uint32_t n0 = k + 1 < BITS_NB ? word(cur, k + 1 < BITS_NB ? k + 1 : 0, 0) : word(nxt, 0, 0);
            const uint32_t n1 = k + 1 < BITS_NB ? word(cur, k + 1 < BITS_NB ? k + 1 : 0, 1) : word(nxt, 0, 1);
            const mask_t na = M::lds(n0 & 0xFFF8u), nb = M::lds(n0 >> 16), nc = M::lds(n1 & 0xFFFFu);
            // the three reads of step k + 1 are ISSUED before step k computes (left to itself the scheduler put them behind
            // the four v_bitop3: 8 instructions between a read and its wait, ~35 clocks of a lone wave against an LDS latency
            // of ~100; in front there are 17)
            __builtin_amdgcn_sched_barrier(0);
            const uint32_t w0 = word(cur, k, 0), w1 = word(cur, k, 1);
            const uint32_t k1 = (uint32_t)((int32_t)(w0 << 31) >> 31), k2 = (uint32_t)((int32_t)(w0 << 30) >> 31);
            M::lds_st(w1 >> 16, M::prim(a, b, c, k1, k2));
            a = na; b = nb; c = nc;
        }
        cprev = ccur;
    }

    // after the last batch: what it completed, and the row loads it may still hold are dropped (nothing reads them)
    __device__ __forceinline__ void drain() {
        const uint32_t fn = (cw(cprev, 0) >> 8) & 0xFFu;
#pragma unroll
        for (int j = 0; j < BITS_MAX_FLUSH; j++)
            if (j < (int)fn) M::store(rsrc, cw(cprev, 2 + 2 * BITS_MAX_LOADS + 2 * j) + lane8, M::lds(cw(cprev, 3 + 2 * BITS_MAX_LOADS + 2 * j) + lane8));
    }
};

template <int W>
__global__ void __launch_bounds__(64)
cw_bits_eval_kernel(const uint4 *__restrict__ recs, const uint32_t *__restrict__ cmds, uint32_t n_batches, uint32_t const_off,
                    uint64_t *T, uint64_t slots) {
    typedef BitsMask<W> M;
    typedef typename M::T mask_t;
    const uint32_t lane = threadIdx.x, g = blockIdx.x, slice = blockIdx.y;
    char *Tg = (char *)(T + (size_t)g * slots) + slice * (W / 8);
    if (n_batches == 0) return;
    BitsEval<W> E;
    // buffer descriptors (wave-uniform by construction: kernel arguments and blockIdx only); a wave of a narrower slice
    // addresses its bytes of every 8-byte mask through the shifted base
    E.rsrc = __builtin_amdgcn_make_buffer_rsrc(Tg, 0, (int)(uint32_t)(slots * 8 - slice * (W / 8)), 0x00020000);
    E.rrecs = __builtin_amdgcn_make_buffer_rsrc((void *)recs, 0, (int)((n_batches + BITS_AHEAD) * 4096u), 0x00020000);
    E.rcmds = __builtin_amdgcn_make_buffer_rsrc((void *)cmds, 0, (int)((n_batches + BITS_AHEAD) * (BITS_CMD_WORDS * 4u)), 0x00020000);
    E.lane8 = lane * 8;
    // the dynamic LDS of this kernel starts at LDS address 0 (it declares no static LDS): records carry raw LDS offsets
    if (lane == 0) {
        M::lds_st(const_off, (mask_t)0);
        M::lds_st(const_off + 8, (mask_t)~(mask_t)0);
    }
    // every lane's ring entries start as 0 (idle lanes of the first vrows read constants only; a defined value keeps
    // the kernel deterministic when a damaged program names an entry that was never written)
    for (uint32_t o = E.lane8; o < const_off; o += 512) M::lds_st(o, (mask_t)0);
    // the host pads the stream to whole trips of 18 batches and appends BITS_AHEAD empty ones (records are requested
    // BITS_AHEAD batches ahead); nine record sets and two loaded-row sets rotate by NAME through the 18 expansions of
    // the batch body (no register moves)
    uint4 R0[4], R1[4], R2[4], R3[4], R4[4], R5[4], R6[4], R7[4], R8[4];
    mask_t L0[BITS_MAX_LOADS], L1[BITS_MAX_LOADS];
#pragma unroll
    for (int j = 0; j < BITS_MAX_LOADS; j++) L0[j] = L1[j] = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        R0[j] = E.rec_load(0, j);
        R1[j] = E.rec_load(1, j);
        R2[j] = E.rec_load(2, j);
        R3[j] = E.rec_load(3, j);
        R4[j] = E.rec_load(4, j);
        R5[j] = E.rec_load(5, j);
        R6[j] = E.rec_load(6, j);
        R7[j] = E.rec_load(7, j);
    }
    E.cprev = 0;
    uint32_t C0 = E.cmd_load(0), C1 = E.cmd_load(1), C2 = E.cmd_load(2), C3 = E.cmd_load(3), C4 = E.cmd_load(4),
             C5 = E.cmd_load(5), C6 = E.cmd_load(6), C7 = E.cmd_load(7), C8 = 0;
    E.a = M::lds(R0[0].x & 0xFFF8u);
    E.b = M::lds(R0[0].x >> 16);
    E.c = M::lds(R0[0].y & 0xFFFFu);
    static_assert(BITS_AHEAD == 8, "the rotation below is written for 9 record sets");
    for (uint32_t bi = 0; bi < n_batches; bi += 18) {
        E.batch(bi + 0, R0, R1, R8, C0, C8, L0, L1);
        E.batch(bi + 1, R1, R2, R0, C1, C0, L1, L0);
        E.batch(bi + 2, R2, R3, R1, C2, C1, L0, L1);
        E.batch(bi + 3, R3, R4, R2, C3, C2, L1, L0);
        E.batch(bi + 4, R4, R5, R3, C4, C3, L0, L1);
        E.batch(bi + 5, R5, R6, R4, C5, C4, L1, L0);
        E.batch(bi + 6, R6, R7, R5, C6, C5, L0, L1);
        E.batch(bi + 7, R7, R8, R6, C7, C6, L1, L0);
        E.batch(bi + 8, R8, R0, R7, C8, C7, L0, L1);
        E.batch(bi + 9, R0, R1, R8, C0, C8, L1, L0);
        E.batch(bi + 10, R1, R2, R0, C1, C0, L0, L1);
        E.batch(bi + 11, R2, R3, R1, C2, C1, L1, L0);
        E.batch(bi + 12, R3, R4, R2, C3, C2, L0, L1);
        E.batch(bi + 13, R4, R5, R3, C4, C3, L1, L0);
        E.batch(bi + 14, R5, R6, R4, C5, C4, L0, L1);
        E.batch(bi + 15, R6, R7, R5, C6, C5, L1, L0);
        E.batch(bi + 16, R7, R8, R6, C7, C6, L0, L1);
        E.batch(bi + 17, R8, R0, R7, C8, C7, L1, L0);
    }
    E.drain();
}

// instances that tripped an assertion gate: the program gives every assertion value a bit-table slot; a mask that is not
// zero names the instances to be re-run by the 256-bit schedule
__global__ void __launch_bounds__(256)
cw_bits_assert_kernel(const uint64_t *__restrict__ T, uint64_t slots, const uint32_t *__restrict__ aslots, uint32_t n_asserts,
                      uint32_t n_groups, uint64_t *fbmask) {
    const uint32_t g = blockIdx.x * 256 + threadIdx.x;
    if (g >= n_groups) return;
    uint64_t v = 0;
    for (uint32_t i = 0; i < n_asserts; i++) v |= T[(size_t)g * slots + aslots[i]];
    if (v) fbmask[g] |= v;
}

// ---- egress: canonical 32-byte values from the bit table (getWitness + Fr_toLongNormal, main.cpp:326-332) ----------------
// out[j][k] (32 bytes) = value of witness element k in instance first + j.  The kernel is a pure HBM writer: a wave owns
// 32 * BITS_GATHER_RUN consecutive elements and walks 64 instances; lane l holds the mask of element k0 + l / 2 (ONE 8-byte read
// per 2 KiB written, through wslot = sig_slot o w2s composed on the host) and every store instruction writes the 1 KiB that 32
// elements of one instance occupy (global_store_dwordx4, consecutive lanes -> consecutive 16-byte halves).  Round 2's
// kernel ran one thread per element with two dependent index loads per 32 bytes: 0.53 of the HBM peak.
// Round 5 (tools/ubench_egress.hip on the --O1 witness of the default line, 156 809 wires, profiles/r05n_ubench_egress*.txt; a
// one-pass 16-byte fill of the same buffers writes 6.9 TB/s, hipMemsetAsync 6.7): streaming (nt) stores 4.29 TB/s -> plain
// stores 4.7 - 4.8; 8 KiB instead of 4 KiB runs per wave 4.8 - 4.9; with 8 or more groups of 64 instances per launch the grid
// walks the GROUPS fastest (`tiles_fastest`: the workgroups that run together then write the same elements of different instances): 5.1 - 5.8
// for launches of 1 024 instances, 5.4 - 5.5 for 2 048 (elements fastest: 4.5 - 4.9); a sweep in pure address order (one
// instance per workgroup, the mask words re-read from L2) 3.0, rotated starts 4.2 - 5.1, other workgroup sizes 4.6 - 4.8.
#define BITS_GATHER_RUN 8      // consecutive 1 KiB pieces (32 elements each) a wave writes per instance: 8 KiB runs, 32 KiB per block
//
// AT: egress by index (cw_get_witnesses_at*): out[j][k] (32 bytes) = witness element k of the range in instance idx[j].  The same
// tile and stores - a wave owns 32 * BITS_GATHER_RUN elements x 64 list positions and writes whole 1 KiB runs of one position,
// even lanes carrying the bit -, but the 64 positions of a tile may lie in 64 different groups, so there is no window to read:
// the wave FORMS the 64-bit window of an element.  Lane l holds position j0 + l: its instance (loaded once, before the loop over
// the elements), the address of its group (bits_group: both table layouts) and its bit number.  Per element the slot is a scalar
// load (wslot[k], wave-uniform), every lane reads ITS group's word of that slot and a ballot of the lanes' bits is the window,
// bit l = the value at position j0 + l; it is kept by the two lanes that write the element.  For an ascending dense list the 64
// words of a read are one or two distinct addresses.  No LDS.  `first` is not used.
//   dense   a tile whose live positions are all valid and name CONSECUTIVE instances (one ballot decides; what the tiles of an
//           ascending dense list mostly are, the identity list always) has a window to read after all: the range form's read
//           (bits_gather_window) from the tile's first instance - 8 loads per wave instead of 256 scalar loads, 256 vector loads
//           and 256 ballots.
//   grid    as above: with 8 or more tiles of positions per launch the grid walks the positions fastest (`tiles_fastest`).
//   length  `count` positions in this launch, the launch's first being position pos0 of the caller's list, cut at *d_n
//           (cw_list_limit); a wave whose tile lies behind the end leaves at once, rows behind it are not written.
//   bad     a position whose index is >= batch reads nothing and contributes 0 to every ballot: its row is zeros.  One lane of
//           the tile's first wave reports the lowest such position, pos0 + j0 + l, with atomicMin (`bad` may be nullptr; the
//           caller fills it first).
// The rows of the instances the side batch re-ran are written over afterwards (cw_kernels.hip cw_gather_many_kernel<., true>
// with the instance -> side-batch map), in stream order.

// The windows of a run of nj <= 64 consecutive instances from i0, all in the batch: one mask per lane pair (lane l: element
// k0 + r * 32 + l / 2) from the group of i0, shifted down by sh = i0 % 64; the next group's OR-ed in above it when the run
// crosses into that group, 64 - sh < nj (which is then a group of the batch).  A range tile is such a run from first + j0 with
// nj = min(64, count - j0), a dense list tile one from its first instance: for the range, i0 + 64 - sh < first + count is the
// same condition.
__device__ __forceinline__ void bits_gather_window(const uint64_t *__restrict__ T, uint64_t slots, uint32_t lsh,
                                                   const uint32_t *__restrict__ wslot, uint32_t n_wit, uint32_t k0, uint32_t lane,
                                                   uint32_t i0, uint32_t nj, uint64_t (&win)[BITS_GATHER_RUN], bool (&have)[BITS_GATHER_RUN]) {
    const uint32_t g = i0 >> 6, sh = i0 & 63u;
    const bool two = sh && 64u - sh < nj;
#pragma unroll
    for (int r = 0; r < BITS_GATHER_RUN; r++) {
        const uint32_t k = k0 + r * 32 + (lane >> 1);
        have[r] = k < n_wit;
        win[r] = 0;
        if (have[r]) {
            const uint32_t sl = wslot[k];
            win[r] = bits_group(T, slots, lsh, g)[(size_t)sl << lsh] >> sh;
            if (two) win[r] |= bits_group(T, slots, lsh, g + 1)[(size_t)sl << lsh] << (64 - sh);
        }
    }
}
template <bool AT>
__global__ void __launch_bounds__(256)
cw_bits_gather_kernel(const uint64_t *__restrict__ T, uint64_t slots, uint32_t lsh, const uint32_t *__restrict__ wslot, uint32_t n_wit,
                      uint32_t first, uint32_t count, uint4 *__restrict__ out, uint32_t tiles_fastest, uint32_t batch,
                      const uint32_t *__restrict__ idx, uint32_t pos0, const uint32_t *__restrict__ d_n, uint32_t *bad) {
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t bk = tiles_fastest ? blockIdx.y : blockIdx.x, bj = tiles_fastest ? blockIdx.x : blockIdx.y;
    const uint32_t k0 = (bk * 4 + wv) * 32 * BITS_GATHER_RUN;               // this wave's elements
    const uint32_t j0 = bj * 64;                                             // its 64 output instances (list positions)
    const uint32_t lim = AT ? cw_list_limit(count, pos0, d_n) : count;
    if (k0 >= n_wit || (AT && j0 >= lim)) return;
    const uint32_t nj = min(64u, lim - j0);
    uint64_t win[BITS_GATHER_RUN];                                           // bit jj = the value in instance first + j0 + jj (at position j0 + jj)
    bool have[BITS_GATHER_RUN];
    if (!AT) {
        bits_gather_window(T, slots, lsh, wslot, n_wit, k0, lane, first + j0, nj, win, have);
    } else {
        const uint32_t inst = lane < nj ? idx[j0 + lane] : 0u;
        const bool ok = lane < nj && inst < batch;
        const uint64_t off = __ballot(lane < nj && !ok);
        if (bad && off && k0 == 0 && lane == 0) atomicMin(bad, pos0 + j0 + (uint32_t)__builtin_ctzll(off));
        const uint64_t *Tg = bits_group(T, slots, lsh, ok ? inst >> 6 : 0u);
        const uint32_t bit_no = inst & 63u;
        const uint32_t inst0 = __builtin_amdgcn_readfirstlane(inst);        // position j0 is always live
        const bool dense = __ballot(lane < nj && (!ok || inst != inst0 + lane)) == 0;
        if (dense) {
            bits_gather_window(T, slots, lsh, wslot, n_wit, k0, lane, inst0, nj, win, have);
        } else
#pragma unroll
        for (int r = 0; r < BITS_GATHER_RUN; r++) {
            const uint32_t kr = k0 + r * 32;
            have[r] = kr + (lane >> 1) < n_wit;
            win[r] = 0;
            // eight elements at a time: eight slots and eight words in flight before the first ballot.  An element past n_wit takes
            // the slot of the run's first element (always an entry of the list); its window is kept by no lane that writes
            for (uint32_t k8 = 0; k8 < 32 && kr + k8 < n_wit; k8 += 8) {
                uint64_t word[8];
#pragma unroll
                for (uint32_t u = 0; u < 8; u++) {
                    const uint32_t k = kr + k8 + u;
                    const uint32_t sl = wslot[k < n_wit ? k : kr];           // wave-uniform
                    word[u] = ok ? Tg[(size_t)sl << lsh] : 0;
                }
#pragma unroll
                for (uint32_t u = 0; u < 8; u++) {
                    const uint64_t m = __ballot((word[u] >> bit_no) & 1);
                    if ((lane >> 1) == k8 + u) win[r] = m;
                }
            }
        }
    }
    const bool low_half = !(lane & 1);
    uint4 *o = out + ((size_t)j0 * n_wit + k0) * 2 + lane;
    for (uint32_t jj = 0; jj < nj; jj++) {
#pragma unroll
        for (int r = 0; r < BITS_GATHER_RUN; r++) {
            const uint32_t bit = low_half ? (uint32_t)(win[r] >> jj) & 1u : 0u;
            if (have[r]) o[r * 64] = make_uint4(bit, 0u, 0u, 0u);
        }
        o += (size_t)n_wit * 2;
    }
}

// Witness compare (cw_compare_witnesses*): the range egress above with its stores turned into loads and compares.  image[j][k]
// (32 bytes, [count][n_wit]) against the bit of element k of the range (wslot points at its first entry, entry0 in the witness
// list) in instance first + j: diff[j] = min(diff[j], lowest differing entry0 + k), summary as cw_compare.hip.h states it; the
// caller fills diff[0 .. count) and summary first.  The tile, the grid and the windows of cw_bits_gather_kernel<false>
// (bits_gather_window, both table layouts): a wave owns 32 * BITS_GATHER_RUN elements x 64 instances and LOADS whole 1 KiB runs
// of one instance's row, streaming, every byte of the image requested by exactly one wave.  The expected piece is (bit, 0, 0, 0)
// on even lanes and zero on odd lanes: an element equals the bit only as the 32-byte value 0 or 1.  Instances past `count` and
// elements past n_wit neither read nor write.  The windows need no LDS; the 64 words of the reduction are all there is.
//   fbidx   instance -> position in the side batch or negative (nullptr: no side batch).  An instance the side batch re-ran is
//           NOT judged from the bit table - its image row is not even read here: cw_kernels.hip cw_compare_kernel with the same
//           map judges it from the side batch's table, in stream order.
//   reduce  the lanes of a run cover ascending elements of ONE instance, the runs ascend too: one ballot says whether the wave
//           found the instance different at all (well-matching images stop there), then the first run with a differing lane
//           gives the wave's lowest entry, which one lane notes in low[] (one LDS atomic per instance and wave).
__global__ void __launch_bounds__(256)
cw_bits_compare_kernel(const uint64_t *__restrict__ T, uint64_t slots, uint32_t lsh, const uint32_t *__restrict__ wslot, uint32_t n_wit,
                       uint32_t first, uint32_t count, const uint4 *__restrict__ image, uint32_t tiles_fastest, uint32_t entry0,
                       uint32_t report0, const int32_t *__restrict__ fbidx, uint32_t *__restrict__ diff, uint32_t *__restrict__ summary) {
    __shared__ uint32_t low[64];
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t bk = tiles_fastest ? blockIdx.y : blockIdx.x, bj = tiles_fastest ? blockIdx.x : blockIdx.y;
    const uint32_t k0 = (bk * 4 + wv) * 32 * BITS_GATHER_RUN;               // this wave's elements
    const uint32_t j0 = bj * 64;                                             // its 64 instances
    const uint32_t nj = min(64u, count - j0);
    if (wv == 0) low[lane] = CMP_EQUAL;
    __syncthreads();
    if (k0 < n_wit) {                                                        // (no wave leaves before the barriers)
        uint64_t win[BITS_GATHER_RUN];                                       // bit jj = the value in instance first + j0 + jj
        bool have[BITS_GATHER_RUN];
        bits_gather_window(T, slots, lsh, wslot, n_wit, k0, lane, first + j0, nj, win, have);
        const uint64_t rerun = __ballot(fbidx && lane < nj && fbidx[first + j0 + lane] >= 0);
        const bool low_half = !(lane & 1);
        const uint4 *o = image + ((size_t)j0 * n_wit + k0) * 2 + lane;
        for (uint32_t jj = 0; jj < nj; jj++, o += (size_t)n_wit * 2) {
            if ((rerun >> jj) & 1) continue;
            uint4 w[BITS_GATHER_RUN];
#pragma unroll
            for (int r = 0; r < BITS_GATHER_RUN; r++)
                if (have[r]) w[r] = cmp_load16(o + r * 64);
            bool ne[BITS_GATHER_RUN], any = false;
#pragma unroll
            for (int r = 0; r < BITS_GATHER_RUN; r++) {
                const uint32_t bit = low_half ? (uint32_t)(win[r] >> jj) & 1u : 0u;
                ne[r] = have[r] && cmp_ne(w[r], make_uint4(bit, 0u, 0u, 0u));
                any |= ne[r];
            }
            if (__ballot(any)) {
                uint32_t entry = CMP_EQUAL;
#pragma unroll
                for (int r = BITS_GATHER_RUN - 1; r >= 0; r--) {
                    const uint64_t who = __ballot(ne[r]);
                    if (who) entry = entry0 + k0 + r * 32 + ((uint32_t)__builtin_ctzll(who) >> 1);
                }
                if (lane == 0) atomicMin(&low[jj], entry);
            }
        }
    }
    __syncthreads();
    if (wv == 0) cmp_report(low, lane, lane < nj, j0, report0, diff, summary);
}

// packed main inputs (cw_set_inputs_bits*): masks[group][k] -> bit-table slot input_slot0 + k
__global__ void __launch_bounds__(256)
cw_bits_ingest_packed_kernel(const uint64_t *__restrict__ masks, uint64_t *__restrict__ T, uint64_t slots, uint32_t sh, uint32_t input_slot0,
                             uint32_t n_in, uint32_t batch) {
    const uint32_t k = blockIdx.y * 256 + threadIdx.x, g = blockIdx.x;   // (groups in x: 65 536 of them at 2^22 instances)
    if (k >= n_in) return;
    uint64_t m = masks[(size_t)g * n_in + k];
    const uint32_t live = batch - g * 64;                            // instances of the last group beyond the batch read as 0
    if (live < 64) m &= (1ull << live) - 1;
    bits_group(T, slots, sh, g)[(size_t)(input_slot0 + k) << sh] = m;
}
// The same into the emitted code's table (sh = 5, T[chunk][slot][32 groups]) in WHOLE ROWS.  With the kernel above a wave's store
// there is 64 pieces of 8 bytes in 64 different 256-byte rows; here a workgroup of four waves owns a tile of one chunk (32 groups)
// x 64 inputs and transposes it through LDS (index arithmetic: cw_bits_layout.h, replayed on the CPU by
// tests/host/bits_rows_layout_test.cpp).  Grid: chunks in x, tiles of 64 inputs in y.
//   read    wave w takes the groups w, w + 4, .. w + 28 of the chunk, lane l the input k0 + l: a load is 512 contiguous bytes of
//           masks[g][...]; the eight loads stand in one straight-line block ahead of the first LDS write.  Groups >= n_groups
//           (the padding of the last chunk) and inputs >= n_in read as 0; the last real group is masked to its live instances
//   stage   tile[group][input] with rows of 65 words of 8 bytes (16 640 bytes), the padding of cw_bits_rows_to_masks_kernel's tile.
//           Row-wise write (ds_write_b64: four groups of 16 consecutive lanes, bank = (a/4) % 32): 16 consecutive words = 32
//           consecutive dwords, every bank once.  Column-wise read (ds_read_b64: two groups of 32 lanes, bank = (a/4) % 64): the 32
//           lanes of a half-wave have gl = 0 .. 31 at one kk, word 65 gl + kk, dwords 130 gl + 2 kk and the next one, bank pair
//           (2 gl + 2 kk) % 64: 32 distinct pairs.  Zero conflicts in both directions by this arithmetic from the documented bank
//           rules; no bank-conflict counter pass was taken on this kernel.
//   write   store r of thread t is cell r * 256 + t of the tile counted inputs first (kk = idx >> 5, gl = idx & 31): consecutive
//           input slots are consecutive rows of the chunk, so 32 threads write one 256-byte row, a store instruction of the
//           workgroup 2 KiB contiguous, a full tile one contiguous 16 KiB.  Rows of inputs >= n_in are not written.
// The padding groups' columns of the input rows get zeros (valid bits), where the kernel above leaves what the allocation held.
__global__ void __launch_bounds__(cwlayout::ROWS_THREADS)
cw_bits_masks_to_table_rows_kernel(const uint64_t *__restrict__ masks, uint64_t *__restrict__ T, uint64_t slots, uint32_t input_slot0,
                                   uint32_t n_in, uint32_t batch, uint32_t n_groups) {
    using namespace cwlayout;
    __shared__ uint64_t tile[ROWS_GROUPS * ROWS_STRIDE];
    const uint32_t chunk = blockIdx.x, k0 = blockIdx.y * ROWS_INPUTS, g0 = chunk * ROWS_GROUPS;
    uint64_t v[ROWS_LOADS] = {};
    {
        const uint32_t k = k0 + rows_read_cell(threadIdx.x, 0).kk;
        if (k < n_in) {
            // a padding group loads the last real group's mask (valid memory) and drops it: the loads carry no condition of their
            // own, so the compiler keeps all eight in flight in the last chunk too
#pragma unroll
            for (uint32_t j = 0; j < ROWS_LOADS; j++) {
                const uint32_t g = g0 + rows_read_cell(threadIdx.x, j).gl;
                v[j] = masks[(size_t)(g < n_groups ? g : n_groups - 1u) * n_in + k];
            }
#pragma unroll
            for (uint32_t j = 0; j < ROWS_LOADS; j++) {
                const uint32_t g = g0 + rows_read_cell(threadIdx.x, j).gl;
                v[j] = g < n_groups ? v[j] & rows_live_mask(batch, g) : 0;
            }
        }
    }
#pragma unroll
    for (uint32_t j = 0; j < ROWS_LOADS; j++) tile[rows_tile_word(rows_read_cell(threadIdx.x, j))] = v[j];
    __syncthreads();
#pragma unroll
    for (uint32_t r = 0; r < ROWS_STORES; r++) {
        const RowsCell c = rows_write_cell(threadIdx.x, r);
        if (k0 + c.kk < n_in) T[element(slots, ROWS_SH, g0 + c.gl, (uint64_t)input_slot0 + k0 + c.kk)] = tile[rows_tile_word(c)];
    }
}
// canonical inputs of the listed instances from packed masks / from the AoS input image (rows of the side batch that
// re-runs them on the 256-bit schedule): out[j][k] = input k of instance inst[j]
__global__ void __launch_bounds__(256)
cw_bits_collect_inputs_kernel(const uint64_t *__restrict__ masks, const uint4 *__restrict__ aos, const uint32_t *__restrict__ inst,
                              uint32_t n_inst, uint32_t n_in, uint4 *__restrict__ out) {
    const uint32_t k = blockIdx.x * 256 + threadIdx.x, j = blockIdx.y;
    if (k >= n_in || j >= n_inst) return;
    const uint32_t i = inst[j];
    uint4 lo, hi = make_uint4(0, 0, 0, 0);
    if (masks) {
        lo = make_uint4((uint32_t)(masks[(size_t)(i >> 6) * n_in + k] >> (i & 63u)) & 1u, 0, 0, 0);
    } else {
        lo = aos[((size_t)i * n_in + k) * 2];
        hi = aos[((size_t)i * n_in + k) * 2 + 1];
    }
    out[((size_t)j * n_in + k) * 2] = lo;
    out[((size_t)j * n_in + k) * 2 + 1] = hi;
}

// Boolean inputs as packed ROWS (cw_set_inputs_rows*): what a caller holds is the bytes of each instance's message, instance
// after instance; what cw_bits_ingest_packed_kernel reads is the transpose, masks[group][k] with bit i = input k of instance
// 64 group + i.  `rows`: 8-byte aligned, row j at rows + j * stride_w words, input k of a row = bit k & 63 of word k >> 6 once the
// bits of each byte are in ascending order (MSB: they arrive the other way round, most significant bit first).  This is the tiled
// transpose of cw64.hip (cw64_transpose_in_kernel<8, false>) with a 64 x 64 bit matrix in the write stage.  A workgroup of four
// waves owns 64 instances (one group, blockIdx.x: no 65 535 limit on the instances) x 64 words = 4 096 inputs (blockIdx.y):
//   read       wave w takes the instances w, w + 4, ... of the tile; its 64 lanes read 64 consecutive words of ONE row, 512
//              contiguous bytes per load.  The 16 loads of a wave stand in one straight-line block under the lane's own
//              condition (the row bases are wave-uniform); the last instance tile of a batch has a row condition too and takes
//              that slower form.  Words past ceil(n_in / 64) and rows past `batch` are not read and count as 0.
//   stage      tile[instance][word] in LDS with rows of 65 words of 8 bytes, as cw64_egress_kernel's tile.  Row-wise write
//              (ds_write_b64: four groups of 16 consecutive lanes, bank = (a/4) % 32): a group writes 16 consecutive words = 32
//              consecutive dwords, every bank once, whatever the row's start.  Column-wise read (ds_read_b64: two groups of 32
//              lanes, bank = (a/4) % 64): lane l reads word 65 l + w, dwords 130 l + 2 w and the next one, bank pair
//              2 ((l + w) % 32): the 32 rows l of a group fall on distinct pairs.  With rows of 64 words every lane of a group
//              would hit pair 2 (w % 32): 32-way.  Zero conflicts in both directions - by this arithmetic from the documented
//              bank rules; no bank-conflict counter pass was taken on this kernel.
//   transpose  wave w takes the words w, w + 4, ...; lane i holds word x of instance i.  MSB first: the bits inside each byte are
//              reversed (bit-reverse the word, then swap its bytes back).  For k = 0 .. 63 the ballot of bit k of x over the wave
//              IS masks[group][64 word + k], bit i = instance 64 group + i; it is wave-uniform, and lane k keeps it (two selects
//              under lane == k; the compiler forms the 64 lane conditions once, ahead of the loop).  Lanes of instances past the batch hold 0, so the last group's upper bits are 0.
//   write      lane k stores its mask: 64 consecutive entries of masks[group][...], one 512-byte store per word.  Lanes whose
//              input index is >= n_in store nothing.
// Kept apart from the 64-bit transpose on purpose: a shared write stage cost that kernel 24 VGPRs (NOTES).
#define ROWS_S 65
template <bool MSB>
__global__ void __launch_bounds__(256)
cw_bits_rows_to_masks_kernel(const uint64_t *__restrict__ rows, size_t stride_w, uint32_t n_in, uint32_t batch, uint64_t *__restrict__ masks) {
    __shared__ uint64_t tile[64 * ROWS_S];
    const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t g = blockIdx.x, w0 = blockIdx.y * 64u;
    const uint32_t n_words = (n_in >> 6) + ((n_in & 63u) != 0);
    const uint32_t nw = n_words - w0 < 64u ? n_words - w0 : 64u, nj = batch - g * 64u < 64u ? batch - g * 64u : 64u;
    const uint64_t *t0 = rows + (size_t)g * 64u * stride_w + w0;
    uint64_t v[64 / 4] = {};
    if (lane < nw) {
        if (nj == 64u) {
#pragma unroll
            for (uint32_t i = 0; i < 64 / 4; i++) v[i] = t0[(size_t)(wave + 4 * i) * stride_w + lane];
        } else {
#pragma unroll
            for (uint32_t i = 0; i < 64 / 4; i++)
                if (wave + 4 * i < nj) v[i] = t0[(size_t)(wave + 4 * i) * stride_w + lane];
        }
    }
#pragma unroll
    for (uint32_t i = 0; i < 64 / 4; i++) tile[(wave + 4 * i) * ROWS_S + lane] = v[i];
    __syncthreads();
    for (uint32_t w = wave; w < nw; w += 4) {                          // wave-uniform: every lane takes part in the ballots
        uint64_t x = tile[lane * ROWS_S + w];
        if (MSB) x = __builtin_bswap64(__builtin_bitreverse64(x));
        uint64_t keep = 0;
#pragma unroll
        for (uint32_t k = 0; k < 64; k++) {
            const uint64_t m = __builtin_amdgcn_ballot_w64((x >> k) & 1u);
            if (lane == k) keep = m;
        }
        const uint64_t k = (uint64_t)(w0 + w) * 64u + lane;
        if (k < n_in) masks[(size_t)g * n_in + k] = keep;
    }
}

// Witness bits OUT as packed rows (cw_get_witness_rows*): the transpose above in the other direction.  The table holds entry k of
// the witness list as one mask per group, bit i = instance 64 group + i; a caller reads rows[instance][entry], entry entry0 + k
// = bit k & 63 of word k >> 6 of row j (MSB: the bits of each byte the other way round - np.packbits, a SHA-256 digest).
// `wslot` points at entry0 of the composed map sig_slot o w2s.  A workgroup of four waves owns 64 instances (blockIdx.x: no
// 65 535 limit on the instances) x 64 words = 4 096 entries (blockIdx.y):
//   read       wave w takes the words w, w + 4, ... of the tile; lane k loads the mask of entry 64 word + k: one 8-byte read through
//              wslot and bits_group, so both table layouts are served (sh = 0: the 64 slots are wherever the witness list points;
//              sh = 5: 256 bytes apart at least).  Instances first + 64 tile .. need not start a group: the two neighbouring
//              groups are shifted together, as cw_bits_gather_kernel does it, and the second is read only when the range reaches
//              into it.  Lanes whose entry is >= n hold 0: the pad bits of the last word.
//   transpose  for i = 0 .. 63 the ballot of bit i of the masks over the wave IS word `word` of instance i: bit k = entry
//              64 word + k.  It is wave-uniform and lane i keeps it.  MSB first: the bits inside each byte are reversed.
//   stage      tile[instance][word] in LDS with rows of 65 words, the tile of cw_bits_rows_to_masks_kernel used the other way
//              round: column-wise WRITE (ds_write_b64: four groups of 16 consecutive lanes, bank = (a/4) % 32; lane i writes word
//              65 i + w, dwords 130 i + 2 w and the next one, bank pair 2 ((i + w) % 16): the 16 lanes of a group fall on distinct
//              pairs), row-wise READ (ds_read_b64: two groups of 32 lanes, bank = (a/4) % 64; a group reads 32 consecutive words =
//              64 consecutive dwords, every bank once).  Zero conflicts by that arithmetic from the documented bank rules; no
//              bank-conflict counter pass was taken on this kernel.
//   write      wave w takes the instances w, w + 4, ... of the tile; its lanes store 64 consecutive words of ONE row, 512
//              contiguous bytes.  Rows of instances past `count` and words past ceil(n / 64) are neither read nor written.
// A bit table cannot hold a value that is not 0 or 1: this kernel has no word to report through.
template <bool MSB>
__global__ void __launch_bounds__(256)
cw_bits_masks_to_rows_kernel(const uint64_t *__restrict__ T, uint64_t slots, uint32_t lsh, const uint32_t *__restrict__ wslot, uint32_t n,
                             uint32_t first, uint32_t count, uint64_t *__restrict__ rows, size_t stride_w) {
    __shared__ uint64_t tile[64 * ROWS_S];
    const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t j0 = blockIdx.x * 64u, w0 = blockIdx.y * 64u;
    const uint32_t n_words = (n >> 6) + ((n & 63u) != 0);
    const uint32_t nw = n_words - w0 < 64u ? n_words - w0 : 64u, nj = count - j0 < 64u ? count - j0 : 64u;
    const uint32_t i0 = first + j0, g = i0 >> 6, sh = i0 & 63u;
    const bool two = sh && 64u - sh < nj;                                  // instance i0 + 64 - sh, the first of group g + 1, is in the range
    const uint64_t *Tg = bits_group(T, slots, lsh, g), *Tg1 = bits_group(T, slots, lsh, two ? g + 1 : g);
    for (uint32_t w = wave; w < nw; w += 4) {                              // wave-uniform: every lane takes part in the ballots
        const uint64_t k = (uint64_t)(w0 + w) * 64u + lane;
        uint64_t m = 0;
        if (k < n) {
            const size_t at = (size_t)wslot[k] << lsh;
            m = Tg[at] >> sh;
            if (two) m |= Tg1[at] << (64u - sh);
        }
        uint64_t keep = 0;
#pragma unroll
        for (uint32_t i = 0; i < 64; i++) {
            const uint64_t x = __builtin_amdgcn_ballot_w64((m >> i) & 1u);
            if (lane == i) keep = x;
        }
        if (MSB) keep = __builtin_bswap64(__builtin_bitreverse64(keep));
        tile[lane * ROWS_S + w] = keep;
    }
    __syncthreads();
    uint64_t *o = rows + (size_t)j0 * stride_w + w0;
    if (lane < nw)
        for (uint32_t j = wave; j < nj; j += 4) o[(size_t)j * stride_w + lane] = tile[j * ROWS_S + lane];
}

// ---- signal columns out from the bit table (cw_get_signals_range*) --------------------------------------------------------
// Value k of row j = signal signal0 + k of instance first + j, 0 or 1, as a little-endian unsigned integer of W bytes (1, 2, 4, 8
// or 32) at out + (j) * stride + k * W.  A value is one bit of a mask the table already holds per group, so nothing is
// transposed through LDS: lane = signal.  `sigslot` is the batch's signal -> slot map (cw_batch_signal_slots) on the device.
// A workgroup of four waves owns 64 signals (blockIdx.x) x one CHUNK of 32 groups = 2 048 instances (chunk c0 + blockIdx.y, counted
// from instance 0 whatever `first` is); wave w takes the groups 8 w .. 8 w + 7 of the chunk.
//   read    lane k loads the eight masks of slot(signal0 + k0 + k) for the wave's groups.  sh = 5: they are 64 contiguous,
//           64-byte aligned bytes of the slot's 256-byte row - four 16-byte loads -, and the four waves of the workgroup read the
//           whole row between them (the padding groups of the last chunk are part of the allocation).  sh = 0: eight 8-byte
//           loads, `slots` words apart; groups outside the range are not read.
//   write   for each instance i of a group the wave stores (mask >> i) & 1 of its 64 signals as one contiguous run of 64 values:
//           64 W bytes per store (W = 32: two stores of 16-byte pieces, {bit, 0, 0, 0} and zeros).  Only the instances of [first,
//           first + count) are written, nothing behind value n - 1 of a row.
// A bit table holds no value that is too wide: there is no word.  Instances the 256-bit side batch re-ran hold garbage here: the
// host writes them over from there (cw_kernels.hip cw_signals_kernel with the instance -> side-batch map).
template <int W>
__global__ void __launch_bounds__(256)
cw_bits_signals_kernel(const uint64_t *__restrict__ T, uint64_t slots, uint32_t lsh, const uint32_t *__restrict__ sigslot, uint32_t signal0,
                       uint32_t n, uint32_t first, uint32_t count, uint32_t c0, uint8_t *__restrict__ out, size_t stride) {
    const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t k = blockIdx.x * 64u + lane;
    const uint32_t g0 = (c0 + blockIdx.y) * 32u + wave * 8u;               // this wave's eight groups
    const uint64_t end = (uint64_t)first + count, w_lo = (uint64_t)g0 * 64u, w_hi = w_lo + 512u;
    const uint64_t lo = w_lo > first ? w_lo : first, hi = w_hi < end ? w_hi : end;
    if (lo >= hi || k >= n) return;                                        // (no barrier in this kernel)
    const uint32_t sl = sigslot[signal0 + k];
    uint64_t m[8];
    if (lsh == 5u) {
        const uint4 *p = (const uint4 *)(T + cwlayout::element(slots, 5u, g0, sl));
#pragma unroll
        for (uint32_t q = 0; q < 4; q++) {
            const uint4 x = p[q];
            m[2 * q] = (uint64_t)x.x | ((uint64_t)x.y << 32);
            m[2 * q + 1] = (uint64_t)x.z | ((uint64_t)x.w << 32);
        }
    } else {
#pragma unroll
        for (uint32_t q = 0; q < 8; q++) {
            const uint64_t base = (uint64_t)(g0 + q) * 64u;
            m[q] = base < hi && base + 64u > lo ? T[cwlayout::element(slots, lsh, g0 + q, sl)] : 0;
        }
    }
#pragma unroll
    for (uint32_t q = 0; q < 8; q++) {
        const uint64_t base = (uint64_t)(g0 + q) * 64u;
        if (base >= hi || base + 64u <= lo) continue;                      // wave-uniform
        const uint32_t i_lo = lo > base ? (uint32_t)(lo - base) : 0u, i_hi = hi - base < 64u ? (uint32_t)(hi - base) : 64u;
        uint8_t *row = out + (size_t)(base + i_lo - first) * stride + (size_t)k * W;
        for (uint32_t i = i_lo; i < i_hi; i++, row += stride) {
            const uint32_t bit = (uint32_t)(m[q] >> i) & 1u;
            if (W == 32) {
                ((uint4 *)row)[0] = make_uint4(bit, 0u, 0u, 0u);
                ((uint4 *)row)[1] = make_uint4(0u, 0u, 0u, 0u);
            }
            if (W == 8) *(uint64_t *)row = bit;
            if (W == 4) *(uint32_t *)row = bit;
            if (W == 2) *(uint16_t *)row = (uint16_t)bit;
            if (W == 1) *row = (uint8_t)bit;
        }
    }
}

// ---- R1CS products from the bit table (cw_get_r1cs_products*) -------------------------------------------------------------
// out[j][p][k] (32 bytes, canonical) = the part's sum of coefficient * w[wire] over the terms of constraint row0 + k in instance
// first + j, for the parts of `parts` in the order A, B, C.  The plan (cw_r1cs_products.h) is in FILE order: rowptr[3 row + part]
// .. rowptr[3 row + part + 1] into terms {bit-table slot, id of the canonical coefficient in cctab (8 words each)}; the slots are
// the batch's own signal map, so both table layouts are served through bits_group (the constant wire is slot 1, all ones: its
// term is its coefficient; slot 0 holds the signals that are provably 0).  The tile and the store side of cw_products_kernel
// (cw_kernels.hip): a workgroup of four waves owns 64 instances x PRB_TILE constraints, lane = instance, wave w the rows w,
// w + 4, ...  A term is a SCALAR load of the group's mask word - the instances first + 64 tile .. need not start a group: the two
// neighbouring groups are shifted together as cw_bits_masks_to_rows_kernel does it - and lane i adds `bit i ? c : 0`: no
// multiplication at all.  Instances the 256-bit side batch re-ran hold garbage here: the host writes them over from there.
#define PRB_TILE 16
__global__ void __launch_bounds__(256)
cw_bits_products_kernel(const uint64_t *__restrict__ T, uint64_t slots, uint32_t lsh, const uint32_t *__restrict__ rowptr,
                        const uint2 *__restrict__ terms, const uint32_t *__restrict__ cctab, uint32_t parts, uint32_t n_sel, uint32_t row0,
                        uint32_t n_rows, uint32_t image_rows, uint32_t first, uint32_t count, uint4 *__restrict__ out, FpParams P) {
    __shared__ uint4 tile[PRB_TILE][2][65];
    const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t j0 = blockIdx.x * 64u, k0 = blockIdx.y * PRB_TILE;
    const uint32_t nk = n_rows - k0 < PRB_TILE ? n_rows - k0 : PRB_TILE, nj = count - j0 < 64u ? count - j0 : 64u;
    const uint32_t i0 = first + j0, g = i0 >> 6, sh = i0 & 63u;
    const bool two = sh && 64u - sh < nj;                                  // instance i0 + 64 - sh, the first of group g + 1, is in the range
    const uint64_t *Tg = bits_group(T, slots, lsh, g), *Tg1 = bits_group(T, slots, lsh, two ? g + 1 : g);
    constexpr uint32_t PIECES = 2 * PRB_TILE, PER = 64 / PIECES;
    const uint32_t piece = lane % PIECES, sub = lane / PIECES, e = piece >> 1, h = piece & 1;
    uint4 *o = out + ((size_t)j0 * n_sel * image_rows + k0) * 2 + piece;
    uint32_t sel = 0;
    for (uint32_t part = 0; part < 3; part++) {
        if (!((parts >> part) & 1u)) continue;
        for (uint32_t k = wave; k < nk; k += 4) {
            const uint32_t *rp = rowptr + (size_t)(row0 + k0 + k) * 3 + part;
            const uint32_t t1 = rp[1];
            fe acc = fe_zero();
            for (uint32_t t = rp[0]; t < t1; t++) {
                const uint2 x = terms[t];
                const size_t at = (size_t)x.x << lsh;
                uint64_t m = Tg[at] >> sh;
                if (two) m |= Tg1[at] << (64u - sh);
                const bool on = (m >> lane) & 1u;
                fe w;
                FE_UNROLL for (int q = 0; q < 8; q++) w.v[q] = on ? cctab[(size_t)x.y * 8 + q] : 0u;
                acc = fe_add(acc, w, P);
            }
            tile[k][0][lane] = make_uint4(acc.v[0], acc.v[1], acc.v[2], acc.v[3]);
            tile[k][1][lane] = make_uint4(acc.v[4], acc.v[5], acc.v[6], acc.v[7]);
        }
        __syncthreads();
        if (e < nk)
            for (uint32_t ii = wave * PER + sub; ii < nj; ii += 4 * PER) o[((size_t)ii * n_sel + sel) * image_rows * 2] = tile[e][h][ii];
        __syncthreads();
        sel++;
    }
}

// ---- R1CS check on the bit table ---------------------------------------------------------------------------------------------
// Class E: constraints over <= 5 distinct wires.  The host enumerated A*B - C over the 2^k assignments of the wires
// (cw_host.cpp, exact integer arithmetic): the constraint is a 32-entry truth table "violated?".  A vrow checks 64
// constraints for 64 instances: 5 mask loads per lane, four 3-input lookups + three selects.
struct ERec { uint32_t w[5]; uint32_t tt, row, pad; };
__global__ void __launch_bounds__(64)
cw_bits_r1cs_lut_kernel(const uint4 *__restrict__ recs, uint32_t n_vrows, uint32_t vrows_per_chunk, const uint64_t *__restrict__ T,
                        uint64_t slots, uint32_t sh, const uint64_t *__restrict__ only, uint32_t n_groups, uint32_t batch, uint32_t *status,
                        uint32_t *first_bad) {
    const uint32_t lane = threadIdx.x;
    // audit of flagged groups only (the emitted code checked every constraint itself): a few workgroups walk the flag words
    for (uint32_t g = blockIdx.x; g < n_groups; g += gridDim.x) {
    if (only && only[g] == 0) continue;
    const char *Tg = (const char *)bits_group(T, slots, sh, g);
    const uint32_t v0 = blockIdx.y * vrows_per_chunk, v1 = min(n_vrows, v0 + vrows_per_chunk);
    for (uint32_t v = v0; v < v1; v++) {
        const uint4 x = recs[((size_t)v * 64 + lane) * 2], y = recs[((size_t)v * 64 + lane) * 2 + 1];
        const uint64_t w0 = *(const uint64_t *)(Tg + ((size_t)x.x << sh)), w1 = *(const uint64_t *)(Tg + ((size_t)x.y << sh)),
                       w2 = *(const uint64_t *)(Tg + ((size_t)x.z << sh)), w3 = *(const uint64_t *)(Tg + ((size_t)x.w << sh)),
                       w4 = *(const uint64_t *)(Tg + ((size_t)y.x << sh));
        const uint32_t tt = y.y;
        const uint64_t f00 = lut3(w0, w1, w2, tt & 0xFFu), f01 = lut3(w0, w1, w2, (tt >> 8) & 0xFFu),
                       f10 = lut3(w0, w1, w2, (tt >> 16) & 0xFFu), f11 = lut3(w0, w1, w2, tt >> 24);
        const uint64_t lo = (f01 & w3) | (f00 & ~w3), hi = (f11 & w3) | (f10 & ~w3);
        uint64_t viol = (hi & w4) | (lo & ~w4);
        if (__any(viol != 0)) {                                    // rare: report the first bad row of each instance
            const uint32_t row = y.z;
            while (viol) {
                const uint32_t i = g * 64 + (uint32_t)__builtin_ctzll(viol);
                viol &= viol - 1;
                if (i < batch) {
                    atomicMin(&first_bad[i], row);
                    atomicOr(&status[i], CW_ST_R1CS_FAILED);
                }
            }
        }
    }
    }
}

// Class W: any other constraint (long linear rows of BinSum / Bits2Num shape, field-sized coefficients).  One lane =
// one instance; terms are wave-uniform (scalar loads), a wire's mask is ONE 8-byte scalar-cache read for the whole
// wave and each lane picks its bit.  term = {slot byte offset | part (2 bits) << 30, coefficient id}; coefficient
// table = canonical residues; row ends as in cw_r1cs_stream_kernel: (A*B + (q - C)) * R'^-1 == 0.
__global__ void __launch_bounds__(64)
cw_bits_r1cs_wide_kernel(const uint4 *__restrict__ chunk, uint32_t n_chunks, const uint2 *__restrict__ terms,
                         const uint32_t *__restrict__ ctab, const uint32_t *__restrict__ row_orig,
                         const uint64_t *__restrict__ T, uint64_t slots, uint32_t sh, const uint64_t *__restrict__ only,
                         uint32_t n_groups, uint32_t batch, uint32_t *status, uint32_t *first_bad, FpParams P) {
    const uint32_t lane = threadIdx.x;
    for (uint32_t g = blockIdx.x; g < n_groups; g += gridDim.x) {
    const uint32_t i = g * 64 + lane;
    if (only && only[g] == 0) continue;
    const char *Tg = (const char *)bits_group(T, slots, sh, g);
    uint32_t bad = 0xFFFFFFFFu;
    for (uint32_t cix = blockIdx.y; cix < n_chunks; cix += gridDim.y) {
        const uint4 ch = chunk[cix];                                // first term, n terms, -, first row
        const uint2 *tp = terms + ch.x;
        fe A = fe_zero(), B = fe_zero(), cur = fe_zero();
        uint32_t row = ch.w;
        for (uint32_t k = 0; k < ch.y; k++) {
            const uint2 t = tp[k];
            const uint32_t off = t.x & 0x0FFFFFFFu, part = (t.x >> 28) & 3u, last = t.x >> 31, endrow = (t.x >> 30) & 1u;
            const uint64_t m = *(const uint64_t *)(Tg + ((size_t)off << sh));      // wave-uniform address
            const bool bit = (m >> lane) & 1ull;
            const fe cf = fe_from(ctab + (size_t)t.y * 8);
            fe w;
#pragma unroll
            for (int j = 0; j < 8; j++) w.v[j] = bit ? cf.v[j] : 0u;
            cur = fe_add(cur, w, P);
            if (last) {                                             // last term of its part
                if (part == 0) { A = cur; cur = fe_zero(); }
                else if (part == 1) { B = cur; cur = fe_zero(); }
            }
            if (endrow) {
                const fe29 z = fe29_mmul_add(fe_to29(A), fe_to29(B), fe_to29(fe_neg(cur, P)), P);
                uint32_t o = 0;
#pragma unroll
                for (int j = 0; j < 9; j++) o |= z.l[j];
                if (o != 0) {
                    const uint32_t oc = row_orig[row];
                    if (oc < bad) bad = oc;
                }
                row++;
                A = fe_zero(); B = fe_zero(); cur = fe_zero();
            }
        }
    }
    if (bad != 0xFFFFFFFFu && i < batch) {
        atomicMin(&first_bad[i], bad);
        atomicOr(&status[i], CW_ST_R1CS_FAILED);
    }
    }
}

// Class I: every coefficient is a small signed integer (|c| < 2^40, < 2^20 terms per row): the three parts are exact
// 64-bit integer sums and the row holds iff A * B - C == 0 over the integers (|A*B - C| < 2^125 < q, so this IS the test
// modulo q).  SHA-256's `lin === lout` rows (up to 195 terms) live here.  One lane = one instance; the stream is
// wave-uniform (scalar loads).  The host regrouped the terms (cw_bits_host.h): inside a GROUP the coefficients are
// distinct powers of two of one sign within one 32-bit half, so a term costs two VALU instructions — select 0/1 with the
// wire's 64-instance mask as the condition, shift-or it into the group's word — and a group one 64-bit add.
__device__ __forceinline__ uint32_t bits_lane_bit(uint64_t mask) {
    uint32_t r;
    asm("v_cndmask_b32_e64 %0, 0, 1, %1" : "=v"(r) : "s"(mask));      // lane i gets bit i of the (wave-uniform) mask
    return r;
}
// 32 x 32 bit-matrix transpose across the 32 lanes of a half-wave: lane k enters with row k (bit j = element (k, j)) and
// leaves with column k.  Five butterfly stages; stage d exchanges the off-diagonal d x d blocks between lanes k and k ^ d:
// the partner's word arrives through ds_swizzle (xor mask inside groups of 32 lanes: no index register), is ROTATED so
// that the wanted blocks land on the positions this lane gives up (left by d in the lower lane of a pair, right by d in the
// upper one; what the rotation drags into the kept positions is masked out) and merged with one v_bfi: 3 instructions
// per stage (round 2: ~12 - index arithmetic for ds_bpermute, two masked shifts, compare + select).
struct BitsTr {
    uint32_t rot[5], keep[5];                 // per stage: v_alignbit shift (32 - rotate-left amount), mask of the bits this lane keeps
};
__device__ __forceinline__ BitsTr bits_tr_setup(uint32_t lane) {
    BitsTr t;
#pragma unroll
    for (int s = 0; s < 5; s++) {
        const uint32_t d = 16u >> s;
        const uint32_t m = s == 0 ? 0x0000FFFFu : s == 1 ? 0x00FF00FFu : s == 2 ? 0x0F0F0F0Fu : s == 3 ? 0x33333333u : 0x55555555u;
        const bool upper = lane & d;
        t.keep[s] = upper ? ~m : m;
        t.rot[s] = upper ? d : 32u - d;       // v_alignbit_b32(p, p, n) = rotate right by n
    }
    return t;
}
template <int S>
__device__ __forceinline__ uint32_t bits_tr_stage(uint32_t x, const BitsTr &t) {
    constexpr int d = 16 >> S;
    // partner lane ^ d: hipcc turns the small distances into DPP moves (VALU speed), the large ones into LDS-crossbar
    // permutes; five ds_swizzle per word were measured slower (1.73 vs 1.51 ms for the check of Sha256(2048) x 65 536)
    const uint32_t p = (uint32_t)__shfl_xor((int)x, d);
    const uint32_t r = __builtin_amdgcn_alignbit(p, p, t.rot[S]);
    return (x & t.keep[S]) | (r & ~t.keep[S]);                                                // v_bfi_b32
}
__device__ __forceinline__ uint32_t bits_transpose32(uint32_t x, const BitsTr &t) {
    x = bits_tr_stage<0>(x, t);
    x = bits_tr_stage<1>(x, t);
    x = bits_tr_stage<2>(x, t);
    x = bits_tr_stage<3>(x, t);
    return bits_tr_stage<4>(x, t);
}
// the word of every instance from the 32 masks of a whole word (slots s .. s + 31 = bits 0 .. 31): lane l loads the
// (l >> 5)-th dword of mask l & 31 - one coalesced 256-byte load, lanes 0..31 then hold the rows of the instances 0..31
// and lanes 32..63 those of the instances 32..63 - and the transpose hands lane i the word of instance i
__device__ __forceinline__ uint32_t bits_word_load(const uint64_t *__restrict__ Tg, uint32_t sh, uint32_t slot, uint32_t lane) {
    return ((const uint32_t *)(Tg + ((size_t)(slot + (lane & 31u)) << sh)))[lane >> 5];
}
__global__ void __launch_bounds__(64)
cw_bits_r1cs_int_kernel(const uint4 *__restrict__ chunk, uint32_t n_chunks, const uint32_t *__restrict__ words,
                        const uint2 *__restrict__ itab, const uint32_t *__restrict__ row_orig,
                        const uint64_t *__restrict__ T, uint64_t slots, uint32_t sh, const uint64_t *__restrict__ only,
                        uint32_t n_groups, uint32_t batch, uint32_t *status, uint32_t *first_bad) {
    const uint32_t lane = threadIdx.x;
    const BitsTr TR = bits_tr_setup(lane);
    for (uint32_t g = blockIdx.x; g < n_groups; g += gridDim.x) {
    const uint32_t i = g * 64 + lane;
    if (only && only[g] == 0) continue;
    const uint64_t *Tg = bits_group(T, slots, sh, g);
    uint32_t bad = 0xFFFFFFFFu;
    for (uint32_t cix = blockIdx.y; cix < n_chunks; cix += gridDim.y) {
        const uint4 ch = chunk[cix];                                // first word, groups, -, first row
        const uint32_t *wp = words + ch.x;
        int64_t A = 0, B = 0, cur = 0;
        uint32_t row = ch.w;
        for (uint32_t gi = 0; gi < ch.y; gi++) {
            const uint32_t hdr = wp[0];
            const uint32_t nb = hdr & 0xFFu;
            wp++;
            if (hdr & (1u << 15)) {                                 // whole words: nb entries slot | half << 30 | sign << 31 (list padded to 8)
                const uint32_t padded = (nb + 7u) & ~7u;
                uint64_t pos = 0, neg = 0;                          // sums of the words with + / - sign, as 64-bit integers
                for (uint32_t j = 0; j < nb; j += 4) {
                    uint32_t e[4], x[4];
#pragma unroll
                    for (int k = 0; k < 4; k++) e[k] = wp[j + k];
#pragma unroll
                    for (int k = 0; k < 4; k++) x[k] = bits_word_load(Tg, sh, e[k] & 0x3FFFFFFFu, lane);   // padding entries name slot 0: valid memory, unused
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        const uint32_t y = j + k < nb ? bits_transpose32(x[k], TR) : 0u;
                        const uint64_t v = (e[k] & (1u << 30)) ? ((uint64_t)y << 32) : (uint64_t)y;       // wave-uniform choices
                        if (e[k] >> 31) neg += v;
                        else pos += v;
                    }
                }
                cur += (int64_t)(pos - neg);
                wp += padded;
            } else if (!(hdr & (1u << 10))) {
                uint32_t acc = 0;
                for (uint32_t blk = 0; blk < nb; blk++, wp += 8) {
                    uint32_t w[8];
                    uint64_t m[8];
#pragma unroll
                    for (int k = 0; k < 8; k++) w[k] = wp[k];
                    if (w[0] >> 31) {                                          // 8 consecutive slots: one 64-byte scalar load
                        const uint64_t *mp = Tg + ((size_t)((w[0] & 0x7FFFFFFFu) >> 5) << sh);
#pragma unroll
                        for (int k = 0; k < 8; k++) m[k] = mp[(size_t)k << sh];
                    } else {
#pragma unroll
                        for (int k = 0; k < 8; k++) m[k] = Tg[(size_t)(w[k] >> 5) << sh];       // wave-uniform addresses: scalar loads
                    }
#pragma unroll
                    for (int k = 0; k < 8; k++) acc |= bits_lane_bit(m[k]) << (w[k] & 31u);
                }
                const int64_t val = (int64_t)((hdr & (1u << 9)) ? ((uint64_t)acc << 32) : (uint64_t)acc);
                cur += (hdr & (1u << 8)) ? -val : val;
            } else {
                for (uint32_t blk = 0; blk < nb; blk++, wp += 8) {
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        const uint64_t m = Tg[(size_t)wp[2 * k] << sh];
                        const uint2 cw = itab[wp[2 * k + 1]];
                        const int64_t cf = (int64_t)(((uint64_t)cw.y << 32) | cw.x);
                        cur += bits_lane_bit(m) ? cf : 0;
                    }
                }
            }
            if (hdr & (1u << 13)) {                                 // last group of its part
                const uint32_t part = (hdr >> 11) & 3u;
                if (part == 0) { A = cur; cur = 0; }
                else if (part == 1) { B = cur; cur = 0; }
            }
            if (hdr & (1u << 14)) {                                 // end of the row
                const __int128 z = (__int128)A * (__int128)B - (__int128)cur;
                if (z != 0) {
                    const uint32_t oc = row_orig[row];
                    if (oc < bad) bad = oc;
                }
                row++;
                A = 0; B = 0; cur = 0;
            }
        }
    }
    if (bad != 0xFFFFFFFFu && i < batch) {
        atomicMin(&first_bad[i], bad);
        atomicOr(&status[i], CW_ST_R1CS_FAILED);
    }
    }
}

// ---- launch wrappers ---------------------------------------------------------------------------------------------------
hipError_t cwk_bits_init(hipStream_t s, void *T, uint64_t slots, uint32_t sh, uint32_t n_groups, void *fbmask, void *r1flag,
                         uint32_t *status, uint32_t *first_bad, uint32_t Bp) {
    const uint32_t n = n_groups > Bp ? n_groups : Bp;
    hipLaunchKernelGGL(cw_bits_init_kernel, dim3((n + 255) / 256), dim3(256), 0, s, (uint64_t *)T, slots, sh, n_groups,
                       (uint64_t *)fbmask, (uint64_t *)r1flag, status, first_bad, Bp);
    return hipGetLastError();
}
template <class K>
static hipError_t bits_ingest_launch(K kernel, hipStream_t s, const void *in, void *T, uint64_t slots, uint32_t sh, uint32_t input_slot0, uint32_t n_in,
                                     uint32_t batch, void *fbmask) {
    if (n_in == 0 || batch == 0) return hipSuccess;
    const uint32_t per = 64 * BITS_INGEST_WAVES, n_chunks = (n_in + per - 1) / per;
    const uint64_t blocks = (uint64_t)((batch + 63) / 64) * n_chunks;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(kernel, dim3((uint32_t)blocks), dim3(per), 0, s, (const uint4 *)in, (uint64_t *)T, slots, sh, input_slot0, n_in,
                       batch, (uint64_t *)fbmask, n_chunks);
    return hipGetLastError();
}
hipError_t cwk_bits_ingest(hipStream_t s, const void *in, void *T, uint64_t slots, uint32_t sh, uint32_t input_slot0, uint32_t n_in,
                           uint32_t batch, void *fbmask) {
    return bits_ingest_launch(cw_bits_ingest_kernel, s, in, T, slots, sh, input_slot0, n_in, batch, fbmask);
}
hipError_t cwk_bits_ingest_halves(hipStream_t s, const void *in, void *T, uint64_t slots, uint32_t sh, uint32_t input_slot0, uint32_t n_in,
                                  uint32_t batch, void *fbmask) {
    return bits_ingest_launch(cw_bits_ingest_halves_kernel, s, in, T, slots, sh, input_slot0, n_in, batch, fbmask);
}
hipError_t cwk_bits_eval(hipStream_t s, const void *recs, const uint32_t *cmds, uint32_t n_batches, uint32_t ring, uint32_t cache,
                         void *T, uint64_t slots, uint32_t n_groups, uint32_t width, const uint32_t *aslots, uint32_t n_asserts,
                         void *fbmask) {
    const uint32_t const_off = (ring + cache) * 512u;
    const size_t lds = (size_t)const_off + 16;
    typedef void (*kern_t)(const uint4 *, const uint32_t *, uint32_t, uint32_t, uint64_t *, uint64_t);
    kern_t k = width == 16 ? (kern_t)cw_bits_eval_kernel<16> : width == 32 ? (kern_t)cw_bits_eval_kernel<32> : (kern_t)cw_bits_eval_kernel<64>;
    if (lds > 64 * 1024) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k, dim3(n_groups, 64 / width), dim3(64), lds, s, (const uint4 *)recs, cmds, n_batches, const_off, (uint64_t *)T, slots);
    if (n_asserts)
        hipLaunchKernelGGL(cw_bits_assert_kernel, dim3((n_groups + 255) / 256), dim3(256), 0, s, (const uint64_t *)T, slots, aslots, n_asserts,
                           n_groups, (uint64_t *)fbmask);
    return hipGetLastError();
}
// The launches of cw_bits_gather_kernel: `count` instances from `first`, or (at) `count` positions of the list idx, cut at *d_n,
// whose indices may name the instances below `batch` (`out` 16-byte aligned).  Element blocks and tiles of 64 instances or
// positions are the grid's two dimensions, the tiles fastest when a launch has 8 or more of them (see the kernel's comment);
// 65 535 tiles per launch (the grid.y limit when the elements go first), a larger count in several launches, none behind one
// that failed.
static hipError_t bits_gather(bool at, hipStream_t s, const void *T, uint64_t slots, uint32_t sh, const uint32_t *wslot, uint32_t n_wit,
                              uint32_t first, uint32_t count, void *out, uint32_t batch, const uint32_t *idx, const uint32_t *d_n, uint32_t *bad) {
    if (!count || !n_wit) return hipSuccess;
    if (at && (((uintptr_t)out & 15) || (((uintptr_t)idx | (uintptr_t)d_n | (uintptr_t)bad) & 3))) return hipErrorInvalidValue;
    const uint32_t kblocks = (n_wit + 128 * BITS_GATHER_RUN - 1) / (128 * BITS_GATHER_RUN);
    const auto kernel = at ? cw_bits_gather_kernel<true> : cw_bits_gather_kernel<false>;
    return cw_pieces(count, 65535u * 64u, [&](uint32_t done, uint32_t m) {
        const uint32_t tiles = (m + 63) / 64;
        const uint32_t tf = tiles >= 8 && kblocks <= 65535u;
        hipLaunchKernelGGL(kernel, tf ? dim3(tiles, kblocks) : dim3(kblocks, tiles), dim3(256), 0, s, (const uint64_t *)T, slots, sh, wslot,
                           n_wit, first + done, m, (uint4 *)out + (size_t)done * n_wit * 2, tf, batch, at ? idx + done : nullptr, done, d_n, bad);
        return hipGetLastError();
    });
}
hipError_t cwk_bits_gather(hipStream_t s, const void *T, uint64_t slots, uint32_t sh, const uint32_t *wslot, uint32_t n_wit, uint32_t first,
                           uint32_t count, void *out) {
    return bits_gather(false, s, T, slots, sh, wslot, n_wit, first, count, out, 0, nullptr, nullptr, nullptr);
}
// `bad` (or nullptr) takes an atomicMin of the lowest position whose index is >= batch; the caller fills it first.
hipError_t cwk_bits_gather_at(hipStream_t s, const void *T, uint64_t slots, uint32_t sh, const uint32_t *wslot, uint32_t n_wit, uint32_t batch,
                              const uint32_t *d_idx, uint32_t n_idx, const uint32_t *d_n_idx, void *d_out, uint32_t *d_bad) {
    return bits_gather(true, s, T, slots, sh, wslot, n_wit, 0, n_idx, d_out, batch, d_idx, d_n_idx, d_bad);
}
// The launches of cw_bits_compare_kernel: the grid and the pieces of the range egress; `image`, `diff` and report0 move with the
// piece, `fbidx` (or nullptr) is indexed by the batch's instance.
hipError_t cwk_bits_compare(hipStream_t s, const void *T, uint64_t slots, uint32_t sh, const uint32_t *wslot, uint32_t n_wit, uint32_t first,
                            uint32_t count, uint32_t entry0, uint32_t report0, const void *image, const int32_t *fbidx, uint32_t *diff,
                            uint32_t *summary) {
    if (!count || !n_wit) return hipSuccess;
    if (((uintptr_t)image & 15) || (((uintptr_t)diff | (uintptr_t)summary | (uintptr_t)fbidx) & 3)) return hipErrorInvalidValue;
    const uint32_t kblocks = (n_wit + 128 * BITS_GATHER_RUN - 1) / (128 * BITS_GATHER_RUN);
    return cw_pieces(count, 65535u * 64u, [&](uint32_t done, uint32_t m) {
        const uint32_t tiles = (m + 63) / 64;
        const uint32_t tf = tiles >= 8 && kblocks <= 65535u;
        hipLaunchKernelGGL(cw_bits_compare_kernel, tf ? dim3(tiles, kblocks) : dim3(kblocks, tiles), dim3(256), 0, s, (const uint64_t *)T, slots,
                           sh, wslot, n_wit, first + done, m, (const uint4 *)image + (size_t)done * n_wit * 2, tf, entry0, report0 + done, fbidx,
                           diff + done, summary);
        return hipGetLastError();
    });
}
hipError_t cwk_bits_ingest_packed(hipStream_t s, const void *masks, void *T, uint64_t slots, uint32_t sh, uint32_t input_slot0, uint32_t n_in,
                                  uint32_t batch) {
    if (n_in == 0) return hipSuccess;
    // the emitted code's table: whole rows (chunks in x, input tiles in y; beyond 65 535 tiles = 4 194 240 inputs the kernel below
    // still serves the launch)
    if (sh == cwlayout::ROWS_SH && batch && (n_in + cwlayout::ROWS_INPUTS - 1) / cwlayout::ROWS_INPUTS <= 65535u) {
        const uint32_t n_groups = (batch >> 6) + ((batch & 63u) != 0);
        const dim3 grid((n_groups + cwlayout::ROWS_GROUPS - 1) / cwlayout::ROWS_GROUPS, (n_in + cwlayout::ROWS_INPUTS - 1) / cwlayout::ROWS_INPUTS);
        hipLaunchKernelGGL(cw_bits_masks_to_table_rows_kernel, grid, dim3(cwlayout::ROWS_THREADS), 0, s, (const uint64_t *)masks, (uint64_t *)T,
                           slots, input_slot0, n_in, batch, n_groups);
        return hipGetLastError();
    }
    dim3 g((batch + 63) / 64, (n_in + 255) / 256);
    if (g.y > 65535u) return hipErrorInvalidValue;
    hipLaunchKernelGGL(cw_bits_ingest_packed_kernel, g, dim3(256), 0, s, (const uint64_t *)masks, (uint64_t *)T, slots, sh, input_slot0, n_in,
                       batch);
    return hipGetLastError();
}
hipError_t cwk_bits_collect_inputs(hipStream_t s, const void *masks, const void *aos, const uint32_t *inst, uint32_t n_inst,
                                   uint32_t n_in, void *out) {
    if (!n_inst || !n_in) return hipSuccess;
    return cw_pieces(n_inst, 65535u, [&](uint32_t done, uint32_t n) {
        hipLaunchKernelGGL(cw_bits_collect_inputs_kernel, dim3((n_in + 255) / 256, n), dim3(256), 0, s, (const uint64_t *)masks,
                           (const uint4 *)aos, inst + done, n, n_in, (uint4 *)out + (size_t)done * n_in * 2);
        return hipGetLastError();
    });
}
// groups in gridDim.x (2^31 - 1 of them), word tiles of 4 096 inputs in gridDim.y: one launch, no walk over pieces
hipError_t cwk_bits_rows_to_masks(hipStream_t s, const void *d_rows, size_t stride, uint32_t n_in, uint32_t batch, bool msb, void *d_masks) {
    if (n_in == 0 || batch == 0) return hipSuccess;
    const uint32_t n_words = (n_in >> 6) + ((n_in & 63u) != 0);
    if (((uintptr_t)d_rows & 7) || (stride & 7) || stride / 8 < n_words) return hipErrorInvalidValue;
    const dim3 grid((batch >> 6) + ((batch & 63u) != 0), (n_words + 63) / 64);
    if (grid.y > 65535u) return hipErrorInvalidValue;
    if (msb)
        hipLaunchKernelGGL(cw_bits_rows_to_masks_kernel<true>, grid, dim3(256), 0, s, (const uint64_t *)d_rows, stride / 8, n_in, batch,
                           (uint64_t *)d_masks);
    else
        hipLaunchKernelGGL(cw_bits_rows_to_masks_kernel<false>, grid, dim3(256), 0, s, (const uint64_t *)d_rows, stride / 8, n_in, batch,
                           (uint64_t *)d_masks);
    return hipGetLastError();
}
// instance tiles in gridDim.x, word tiles of 4 096 entries in gridDim.y: one launch
hipError_t cwk_bits_masks_to_rows(hipStream_t s, const void *T, uint64_t slots, uint32_t sh, const uint32_t *wslot, uint32_t n, uint32_t first,
                                  uint32_t count, bool msb, void *d_rows, size_t stride) {
    if (n == 0 || count == 0) return hipSuccess;
    const uint32_t n_words = (n >> 6) + ((n & 63u) != 0);
    if (((uintptr_t)d_rows & 7) || (stride & 7) || stride / 8 < n_words) return hipErrorInvalidValue;
    const dim3 grid((count >> 6) + ((count & 63u) != 0), (n_words + 63) / 64);
    if (grid.y > 65535u) return hipErrorInvalidValue;
    const auto kernel = msb ? cw_bits_masks_to_rows_kernel<true> : cw_bits_masks_to_rows_kernel<false>;
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, s, (const uint64_t *)T, slots, sh, wslot, n, first, count, (uint64_t *)d_rows, stride / 8);
    return hipGetLastError();
}
// signal columns out from the bit table: tiles of 64 signals in gridDim.x, the chunks of 2 048 instances that [first, first +
// count) touches in gridDim.y - a launch holds at most 65 535 of those, more go in several launches (cw_pieces.h), none behind one
// that failed.  d_values is the row of instance `first`.
hipError_t cwk_bits_signals(hipStream_t s, const void *T, uint64_t slots, uint32_t sh, const uint32_t *sigslot, uint32_t signal0, uint32_t n,
                            uint32_t first, uint32_t count, void *d_values, size_t stride, uint32_t elem_bytes) {
    if (n == 0 || count == 0) return hipSuccess;
    const size_t a = elem_bytes == 32 ? 16 : elem_bytes;
    const auto kernel = elem_bytes == 1 ? cw_bits_signals_kernel<1> : elem_bytes == 2 ? cw_bits_signals_kernel<2>
                      : elem_bytes == 4 ? cw_bits_signals_kernel<4> : elem_bytes == 8 ? cw_bits_signals_kernel<8>
                      : elem_bytes == 32 ? cw_bits_signals_kernel<32> : nullptr;
    if (!kernel || ((uintptr_t)d_values % a) || (stride % a) || stride / elem_bytes < n) return hipErrorInvalidValue;
    const uint32_t c_lo = first >> 11, c_hi = (uint32_t)(((uint64_t)first + count - 1) >> 11);
    return cw_pieces(c_hi - c_lo + 1, 65535u, [&](uint32_t done, uint32_t m) {
        hipLaunchKernelGGL(kernel, dim3((n + 63) / 64, m), dim3(256), 0, s, (const uint64_t *)T, slots, sh, sigslot, signal0, n, first, count,
                           c_lo + done, (uint8_t *)d_values, stride);
        return hipGetLastError();
    });
}
// R1CS products [count][n_sel][n_rows] of 32-byte canonical residues from the bit table: instance tiles in gridDim.x, row tiles of
// PRB_TILE in gridDim.y, a range of more than 65 535 tiles in several launches (cw_r1cs_products.h row_pieces), none behind one
// that failed
static_assert(PRB_TILE == cwprod::ROWS256, "the row tile of cw_bits_products_kernel");
hipError_t cwk_bits_products(hipStream_t s, const void *T, uint64_t slots, uint32_t sh, const uint32_t *rowptr, const uint32_t *terms,
                             const uint32_t *cctab, uint32_t parts, uint32_t row0, uint32_t n_rows, uint32_t first, uint32_t count, void *d_out,
                             const FpParams &P) {
    const uint32_t n_sel = cwprod::n_parts(parts);
    if (n_rows == 0 || count == 0) return hipSuccess;
    if (n_sel == 0 || (parts & ~cwprod::PART_ALL) || ((uintptr_t)d_out & 15)) return hipErrorInvalidValue;
    return cwprod::row_pieces(n_rows, PRB_TILE, [&](uint32_t off, uint32_t m) {
        hipLaunchKernelGGL(cw_bits_products_kernel, dim3((count >> 6) + ((count & 63u) != 0), cwprod::row_tiles(m, PRB_TILE)), dim3(256), 0, s,
                           (const uint64_t *)T, slots, sh, rowptr, (const uint2 *)terms, cctab, parts, n_sel, row0 + off, m, n_rows, first, count,
                           (uint4 *)d_out + (size_t)off * 2, P);
        return hipGetLastError();
    });
}
hipError_t cwk_bits_r1cs(hipStream_t s, const void *erecs, uint32_t n_evrows, const uint32_t *chunk, uint32_t n_chunks,
                         const uint32_t *terms, const uint32_t *ctab, const uint32_t *row_orig, const uint32_t *ichunk,
                         uint32_t n_ichunks, const uint32_t *iterms, const uint32_t *itab, const uint32_t *irow_orig, const void *T,
                         uint64_t slots, uint32_t sh, const void *only, uint32_t n_groups, uint32_t batch, uint32_t *status, uint32_t *first_bad,
                         const FpParams &P) {
    const uint64_t *onl = (const uint64_t *)only;
    // audit of flagged groups: 1 024 workgroups walk the flag words (a launch of one workgroup per group costs ~14 ns each:
    // 1.4 ms of nothing at 2 M instances)
    const uint32_t gx = onl && n_groups > 1024u ? 1024u : n_groups;
    if (n_evrows) {
        // the kernel is bound by the latency of its 5 mask loads per lane: ~8 waves per SIMD (8192 on the chip) hide it
        uint32_t chunks = onl ? 4u : (8192 + n_groups - 1) / n_groups;
        if (chunks > n_evrows) chunks = n_evrows;
        if (chunks > 65535u) chunks = 65535u;
        if (chunks < 1) chunks = 1;
        const uint32_t per = (n_evrows + chunks - 1) / chunks;
        chunks = (n_evrows + per - 1) / per;
        hipLaunchKernelGGL(cw_bits_r1cs_lut_kernel, dim3(gx, chunks), dim3(64), 0, s, (const uint4 *)erecs, n_evrows, per,
                           (const uint64_t *)T, slots, sh, onl, n_groups, batch, status, first_bad);
    }
    if (n_ichunks) {
        dim3 g(gx, onl ? (n_ichunks < 4u ? n_ichunks : 4u) : n_ichunks < 65535u ? n_ichunks : 65535u);
        hipLaunchKernelGGL(cw_bits_r1cs_int_kernel, g, dim3(64), 0, s, (const uint4 *)ichunk, n_ichunks, iterms,
                           (const uint2 *)itab, irow_orig, (const uint64_t *)T, slots, sh, onl, n_groups, batch, status, first_bad);
    }
    if (n_chunks) {
        dim3 g(gx, onl ? (n_chunks < 4u ? n_chunks : 4u) : n_chunks < 65535u ? n_chunks : 65535u);
        hipLaunchKernelGGL(cw_bits_r1cs_wide_kernel, g, dim3(64), 0, s, (const uint4 *)chunk, n_chunks, (const uint2 *)terms, ctab,
                           row_orig, (const uint64_t *)T, slots, sh, onl, n_groups, batch, status, first_bad, P);
    }
    return hipGetLastError();
}

// ---- witness digests (cw_get_wtns_digests*, cw_wtns_digest.h) ----------------------------------------------------------------
// SHA-256 of the .wtns file of every instance of a bit table (n8 = 32, both layouts): lane = instance, a wave owns the table
// group (first >> 6) + blockIdx.x and walks the message with cwdig::walk.  The 64 instances' bits of an entry are ONE 8-byte
// word, at the address cw_get_signal computes; group and slot are wave-uniform (readfirstlane), so the word is a scalar load and
// the lane's element is (mask >> lane) & 1 in byte 0 of 32.  The load of the mask depends on the load of the slot: both are
// fetched for a run of RUN = 4 blocks (8 entries) at a time - the eight slots, then the eight masks - a run ahead of the rounds,
// so that this latency is paid once per run, not inside every block.  The instances the side batch re-ran are written over by the
// host's walk (cw_host.cpp digest_egress).
struct DigestBitsSrc {
    static constexpr uint32_t EW = 8, H = 19, RUN = 4;
    typedef uint64_t Raw;                                 // the mask of the entry: wave-uniform
    const uint64_t *__restrict__ Tg;                      // the group's slots, (1 << lsh) words apart
    const uint32_t *__restrict__ wslot;
    uint32_t lsh, lane;
    __device__ __forceinline__ Raw fetch(uint32_t k) const {
        const uint32_t sl = __builtin_amdgcn_readfirstlane(wslot[k]);
        return Tg[(size_t)sl << lsh];
    }
    __device__ __forceinline__ void words(const Raw &m, uint32_t w[8]) const {
        w[0] = (uint32_t)(m >> lane) & 1u;
#pragma unroll
        for (int i = 1; i < 8; i++) w[i] = 0;
    }
};
__global__ void __launch_bounds__(64)
cw_bits_wtns_digest_kernel(const uint64_t *__restrict__ T, uint64_t slots, uint32_t lsh, const uint32_t *__restrict__ wslot, uint32_t first,
                           uint32_t count, uint4 *__restrict__ out, cwdig::Plan plan) {
    const uint32_t g = cwdig::wave_group(first, blockIdx.x);
    DigestBitsSrc src{bits_group(T, slots, lsh, g), wslot, lsh, threadIdx.x};
    uint32_t st[8];
    cwdig::walk(plan, src, st);
    cwdig::store_digest(out, first, count, g * 64u + threadIdx.x, st);
}
// digests [count][32] of the instances [first, first + count) as the bit table holds them: one wave per table group of the range
// (every group of the range exists: first + count <= batch); d_out 16-byte aligned
hipError_t cwk_bits_wtns_digest(hipStream_t s, const void *T, uint64_t slots, uint32_t sh, const uint32_t *wslot, uint32_t first, uint32_t count,
                                void *d_out, const cwdig::Plan &plan) {
    if (count == 0) return hipSuccess;
    if (((uintptr_t)d_out & 15) || plan.n8 != 32 || plan.n_witness == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(cw_bits_wtns_digest_kernel, dim3(cwdig::n_groups(first, count)), dim3(64), 0, s, (const uint64_t *)T, slots, sh, wslot,
                       first, count, (uint4 *)d_out, plan);
    return hipGetLastError();
}
