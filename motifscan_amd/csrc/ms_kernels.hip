// ms_kernels.hip -- the pre-filter and nothing else: this object is read back after every compile (check_isa.py: registers and
// spills), and the file's hash decides whether a recorded traffic figure (profiles/pmc_traffic.json) still belongs to the kernel.
//
//   prefilter_f6_kernel  rigorous upper bound of both strand scores for EVERY window (with or without non-ACGT bases) as an
//                     fp6 x fp4 one-hot product on the matrix cores (v_mfma_scale_f32_32x32x64_f8f6f4); emits candidates for the
//                     fp64 stage (ms_fp64.hip).  <2, parked> / <2, dense>: plans of row tiles of 1 or 2 k-blocks; <4, parked>: wide tiles
//
// The packed sequence: ms_device.h; operand tables, quantisation and the proof that no hit is lost: ms_internal.h, ms_plan.cpp.
#include "ms_device.h"

namespace ms {

// ---------------------------------------------------------------------- pre-filter --
//
// The pre-filter on the matrix cores (operand layout, quantisation and the proof that it never loses a hit: ms_internal.h,
// ms_plan.cpp).  Per wave and pass: 128 consecutive window starts (the double pass; 64 in the kernels with wide classes) = four (two)
// 32-column B operands per k-block -- the one-hot image of the lane's bases in fp4, fetched once per class from the pass's one-hot array and
// reused by every row tile -- and per row tile of 32 (motif, strand) rows ONE read of the A operand (fp6: 24 bytes per lane and k-block) and
// 2 NK matrix instructions per 64 window starts.  acc >= +0 (sign bit clear) in any of the 16 result registers of a lane marks a candidate
// (paired rows: bit 22 / bit 10 of the result, ms_internal.h).
//
// ---- candidate hand-off ----
// Candidates are ~2e-4 of the (window, motif) pairs.  One global atomic per find would put every wave of the chip on ONE address
// (measured in round 1: the whole kernel then runs at the ~90 M atomics/s a single word sustains).  Each wave therefore reserves
// BLOCKS of A.cand_block record slots of the global list (one atomicAdd per block) and stores its records straight into its block
// with ballot/mbcnt ranks; slots it leaves unused (fewer than 64 when a block is abandoned, the rest of the last block at the end)
// are written as empty records (flags 0), which rescore_kernel (ms_fp64.hip) skips.  (Rounds 1-2 staged 64 records per wave in LDS and spilled
// them through a called function: at p = 1e-3, ten times the records, that flush was most of the kernel's time.)
// A record is per LANE and per table group: position, group, and one flag bit per field -- rescore_kernel expands the flags.
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) i32x4 lds_i32x4;
typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef int i32x16 __attribute__((ext_vector_type(16)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// What a wave keeps in registers about its candidates: the parking space (below) -- the rest of the hand-off lives in LDS (PfEmit)
struct MfWave {
    uint32_t rq;               // the wave's parking space: its LDS byte address (32-bit address arithmetic: a generic pointer made every entry's address a 64-bit multiply-add); rq_cap entries of kRareEntryWords words
    uint32_t rq_n;             // entries parked (wave-uniform)
    uint32_t rq_cap, rq_flush; // PfArgs::rare_cap; the fill at which the parked entries are decoded
};

// Where a class was when its wave's parking space ran full: row tile t is re-entered (its products are computed again) at operand
// `op` (0 / 1: the windows from g0 / from g0 + 32), past the first `skip` candidate lanes of that operand's event
struct PfResume {
    int t;
    uint32_t op, skip;
    uint32_t sub;              // double pass: the half (0: windows from pass0, 1: from pass0 + 64) whose event did not fit
};

// The wave's place in the global candidate list and the launch's constants, in LDS (one per wave: kPfEmitWords words): only the
// out-of-line decode (pf_flush) works with them, so none of it occupies registers of the scanning loop
struct PfEmit {
    unsigned long long base;   // next free slot of this wave's block in the global candidate list
    uint32_t left;             // slots left in the block
    uint32_t pad0;
    uint64_t *cand;
    unsigned long long *n_cand;
    uint64_t cand_cap, cand_static;
    uint32_t cand_block, pad[3];
};                             // (pf_flush reads it as seven 8-byte words)
static_assert(sizeof(PfEmit) == kPfEmitWords * sizeof(uint32_t), "PfEmit layout");

// bit n of the result = result register 15 - n is non-negative (field n of the lane's table group)
__device__ __forceinline__ uint32_t nonneg_flags(const f32x16 &c) {
    uint32_t m = 0;
#pragma unroll
    for (int j = 0; j < 16; j++) m = __builtin_amdgcn_alignbit(m, (uint32_t) __float_as_int(c[j]), 31);   // (m << 1) | sign
    return ~m & 0xFFFFu;
}

// AND of the 16 sign bits (bit 31 of the result): clear <=> some result register is >= +0.  Eight 3-input ANDs (v_bitop3_b32)
// through one accumulator: the forwarded operand keeps the instruction at two fresh register reads
// (profiles/r03_insp_probe.log: 95 cycles per row tile against 108 for the tree of v_max3_i32 round 2 used).
__device__ __forceinline__ uint32_t all_negative(const f32x16 &c) {
    uint32_t x = (uint32_t) __float_as_int(c[0]) & (uint32_t) __float_as_int(c[1]) & (uint32_t) __float_as_int(c[2]);
#pragma unroll
    for (int i = 3; i < 15; i += 2) x = x & (uint32_t) __float_as_int(c[i]) & (uint32_t) __float_as_int(c[i + 1]);
    return x & (uint32_t) __float_as_int(c[15]);
}

// One record per flagged lane into the wave's block of the global list (E: a register copy of the wave's PfEmit)
__device__ __forceinline__ void emit_rec(PfEmit &E, bool live, int64_t g, uint32_t flags, int32_t group) {
    const bool flagged = live && flags != 0;
    const unsigned long long mask = __ballot(flagged);
    if (mask == 0) return;
    const uint32_t n_new = (uint32_t) __popcll(mask);
    const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t) (mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t) mask, 0u));
    if (n_new > E.left) {                                           // (cand_block >= 64 >= n_new: the next block always fits them)
        const uint32_t lane = threadIdx.x & 63u;
        if (lane < E.left && E.base + lane < E.cand_cap) E.cand[E.base + lane] = 0ULL;      // the abandoned rest of the block: empty records
        unsigned long long b = 0;
        if (lane == 0) b = E.cand_static + atomicAdd(E.n_cand, (unsigned long long) E.cand_block);
        E.base = ((unsigned long long) (uint32_t) __builtin_amdgcn_readfirstlane((int) (b >> 32)) << 32) |
                 (unsigned long long) (uint32_t) __builtin_amdgcn_readfirstlane((int) b);
        E.left = E.cand_block;
    }
    if (flagged && E.base + rank < E.cand_cap) E.cand[E.base + rank] = cand_pack((uint64_t) g, (uint32_t) group, flags);
    E.base += n_new;
    E.left -= n_new;
}

// bits of a paired row's 16 results: field X's flag is bit 22, field Y's bit 10 (ms_internal.h).  Two accumulators of eight registers
// each: m = 2 m | (c & mask) walks a register's two bits upwards one position per register (v_add_u32 + v_bitop3_b32, the fast
// VALU class: profiles/r03b_valu_rate.log).  fx / fy: bit n = result register 15 - n, as nonneg_flags.
__device__ __forceinline__ void pair_flags(const f32x16 &c, uint32_t &fx, uint32_t &fy) {
    uint32_t ma = 0, mb = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        ma = (ma + ma) | ((uint32_t) __float_as_int(c[j]) & kPairMask);
        mb = (mb + mb) | ((uint32_t) __float_as_int(c[8 + j]) & kPairMask);
    }
    // register j <= 7: X at bit 29 - j, Y at bit 17 - j of ma; register 8 + j: the same of mb
    fx = ((ma >> 14) & 0xFF00u) | ((mb >> 22) & 0xFFu);
    fy = ((ma >> 2) & 0xFF00u) | ((mb >> 10) & 0xFFu);
}

// ---- parked candidates ----
// A row tile holds a candidate in about one lane of its 64 windows x 32 rows, but decoding WHICH fields (one or two VALU operations
// per result register) and queueing the record costs the wave the same whether one lane needs it or all 64: in round 3's first
// paired kernel that was 28 % of the pre-filter (profiles/r03b_pf_pair.log), and -- inlined into every class -- the reason the
// kernel spilled registers it reloaded once per class and pass.  So the lanes that hold a candidate only PARK the flag bytes of their
// 16 result registers (park_store below; rounds 3-4: the registers themselves) and a two-word header (position, table group, kind) in
// the wave's LDS space -- two or three stores under the lanes' exec mask -- and when the space runs low the class returns to the one place that calls pf_flush, an ordinary
// (not inlined) function: it decodes the parked entries one per lane and queues the records.  An event with more candidate lanes
// than free entries parks what fits; the class comes back to the same row tile after the flush (PfResume).

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) u32x4 lds_u32x4;
typedef __attribute__((address_space(3))) u32x2 lds_u32x2;
// What a parked entry holds (round 5, second half): not the 16 result registers but the BYTES of them that carry the flags -- paired rows:
// bytes 1 and 2 of every register (bit 10 = field Y's flag, bit 22 = field X's): two registers per word, 8 words; plain rows: byte 3 (the sign),
// four registers per word, 4 words -- put together with v_perm_b32 (8 / 12 vector instructions per event and operand), then two (one) 16-byte
// stores and the 8-byte header instead of four and the header.  A parking store costs the wave ~55-65 cycles whatever its exec mask
// (profiles/r05d_pf_account.log: 2.6 k cycles per pass for 47 store instructions at p = 1e-4, 14.7 k for 220 at p = 1e-3), and a 48-byte
// entry instead of an 80-byte one gives the space 64 entries again beside the one-hot arrays.
__device__ __forceinline__ void park_pack(const f32x16 &c, uint32_t paired, u32x4 &p0, u32x4 &p1) {
    auto u = [&](int j) { return (uint32_t) __float_as_int(c[j]); };
    if (paired) {
        // word j = bytes {1, 2} of register j | bytes {1, 2} of register j + 8  (v_perm_b32: selector bytes 0-3 = the second source's, 4-7 = the first's)
#pragma unroll
        for (int j = 0; j < 4; j++) { p0[j] = __builtin_amdgcn_perm(u(j + 8), u(j), 0x06050201u); p1[j] = __builtin_amdgcn_perm(u(j + 12), u(j + 4), 0x06050201u); }
    } else {
        // word w = byte 3 of registers 4 w ... 4 w + 3
#pragma unroll
        for (int w = 0; w < 4; w++) {
            const uint32_t lo = __builtin_amdgcn_perm(u(4 * w + 1), u(4 * w), 0x0C0C0703u), hi = __builtin_amdgcn_perm(u(4 * w + 3), u(4 * w + 2), 0x0C0C0703u);
            p0[w] = __builtin_amdgcn_perm(hi, lo, 0x05040100u);
        }
        p1 = u32x4{0u, 0u, 0u, 0u};
    }
}
__device__ __forceinline__ void park_put(uint32_t entry_lds, const u32x4 &p0, const u32x4 &p1, uint32_t paired, uint32_t hd0, uint32_t hd1) {
    lds_u32x4 *e = (lds_u32x4 *) (uintptr_t) entry_lds;
    e[0] = p0;
    if (paired) e[1] = p1;
    *(lds_u32x2 *) (e + 2) = u32x2{hd0, hd1};                                   // the header: always at byte 32
}
__device__ __forceinline__ void park_store(uint32_t entry_lds, const f32x16 &c, uint32_t paired, uint32_t hd0, uint32_t hd1) {
    u32x4 p0, p1;
    park_pack(c, paired, p0, p1);
    park_put(entry_lds, p0, p1, paired, hd0, hd1);
}

// Parks the event's candidate lanes number skip, skip + 1, ... while entries are free.  True: all parked (skip is 0 again).
__device__ __forceinline__ bool rare_park(MfWave &W, const f32x16 &c, bool hit, int64_t g, int32_t group, uint32_t paired, uint32_t &skip) {
    const unsigned long long mask = __ballot(hit);
    const uint32_t n_new = (uint32_t) __popcll(mask) - skip, n_free = W.rq_cap - W.rq_n;
    const uint32_t n_take = n_new < n_free ? n_new : n_free;
    const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t) (mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t) mask, 0u)) - skip;   // (wraps for the lanes already parked)
    if (hit && rank < n_take)
        park_store(W.rq + __umul24(W.rq_n + rank, (uint32_t) (kRareEntryWords * 4)), c, paired, (uint32_t) g, (uint32_t) ((uint64_t) g >> 32) | ((uint32_t) group << 8) | (paired << 31));
    W.rq_n += n_take;
    if (n_take < n_new) { skip += n_take; return false; }
    skip = 0;
    return true;
}

// The candidate lanes of a row tile's two operands (hit0 / hit1) into the parking space; R says where to pick up after a flush.
// True: the space ran full, the class must leave for a flush and come back to this row tile.
__device__ __forceinline__ bool rare_park2(MfWave &W, PfResume &R, const f32x16 &c0, const f32x16 &c1, bool hit0, bool hit1, int64_t g0,
                                           int32_t group, uint32_t paired) {
    if (R.op == 0 && __any(hit0) && !rare_park(W, c0, hit0, g0, group, paired, R.skip)) return true;
    R.op = 1;
    if (__any(hit1) && !rare_park(W, c1, hit1, g0 + 32, group, paired, R.skip)) return true;
    R.op = 0;
    return false;
}

// The common case of an event, straight-line: BOTH operands' candidate lanes ranked at once (operand 0's lanes first, as rare_park2
// orders them) and parked with two exec-masked store sequences -- no resumable state, one branch.  Only an event that does not fit
// the free entries (or a class re-entered in the middle of one, R.op / R.skip set) takes rare_park2's piecewise form.  Round 4:
// profiles/r03zz_class_clock.log put the hand-off at ~5.7 k of a wave's ~24.5 k cycles per 64-window pass, ~600 cycles per event,
// most of it the dozen taken branches and scalar bookkeeping of the resumable form.
struct PfLive {                 // which of the lane's two windows lie inside the input: the lane's flags, and the wave's masks (scalar registers, made once per pass)
    bool l0, l1;
    unsigned long long m0, m1;
};
__device__ __forceinline__ bool park_both(MfWave &W, PfResume &R, const f32x16 &c0, const f32x16 &c1, const PfLive &L, bool cand0, bool cand1, int64_t g0,
                                          int32_t group, uint32_t paired) {
    // (the two conditions' masks ANDed as masks: a ballot of `live && cand` turns the AND into a register of 0 / 1 and compares that again --
    // four vector instructions per event, found in the ISA in round 5)
    const unsigned long long m0 = __builtin_amdgcn_ballot_w64(cand0) & L.m0, m1 = __builtin_amdgcn_ballot_w64(cand1) & L.m1;
    const bool hit0 = L.l0 && cand0, hit1 = L.l1 && cand1;
    const uint32_t n0 = (uint32_t) __popcll(m0), n1 = (uint32_t) __popcll(m1);
    if (__builtin_expect((R.op | R.skip) != 0u || W.rq_n + n0 + n1 > W.rq_cap, 0))
        return rare_park2(W, R, c0, c1, hit0, hit1, g0, group, paired);
    const uint32_t rank0 = __builtin_amdgcn_mbcnt_hi((uint32_t) (m0 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t) m0, 0u));
    const uint32_t rank1 = __builtin_amdgcn_mbcnt_hi((uint32_t) (m1 >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t) m1, n0));
    const uint32_t hi = (uint32_t) ((uint64_t) g0 >> 32) | ((uint32_t) group << 8) | (paired << 31);     // (g0 + 32 never carries into bit 32: g0 < 2^34 is a multiple-of-64 base plus lane & 31)
    if (hit0) park_store(W.rq + __umul24(W.rq_n + rank0, (uint32_t) (kRareEntryWords * 4)), c0, paired, (uint32_t) g0, hi);
    if (hit1) park_store(W.rq + __umul24(W.rq_n + rank1, (uint32_t) (kRareEntryWords * 4)), c1, paired, (uint32_t) g0 + 32u, hi);
    W.rq_n += n0 + n1;
    return false;
}

// Decode and queue the n parked entries of a wave (lane i takes entry i).  All lanes of the wave, at a wave-uniform point.  NOT
// inlined, and everything it needs comes through two LDS addresses: its registers are its own business.
typedef __attribute__((address_space(3))) uint32_t lds_u32;
__device__ __attribute__((noinline)) void pf_flush(uint32_t em_lds, uint32_t rq_lds, uint32_t n) {
    const uint32_t lane = threadIdx.x & 63u;
    const bool mine = lane < n;
    lds_u32x2 *em2 = (lds_u32x2 *) (uintptr_t) em_lds;
    PfEmit E;
    {
        const u32x2 w0 = em2[0], w1 = em2[1], w2 = em2[2], w3 = em2[3], w4 = em2[4], w5 = em2[5], w6 = em2[6];
        E.base = ((unsigned long long) w0.y << 32) | w0.x;
        E.left = w1.x;
        E.cand = reinterpret_cast<uint64_t *>(((unsigned long long) w2.y << 32) | w2.x);
        E.n_cand = reinterpret_cast<unsigned long long *>(((unsigned long long) w3.y << 32) | w3.x);
        E.cand_cap = ((unsigned long long) w4.y << 32) | w4.x;
        E.cand_static = ((unsigned long long) w5.y << 32) | w5.x;
        E.cand_block = w6.x;
    }
    // the entry: 8 words of flag bytes (paired rows) or 4 (plain rows), then the header (park_store)
    u32x2 q[4] = {{0u, 0u}, {0u, 0u}, {0u, 0u}, {0u, 0u}}, hd = {0u, 0u};
    if (mine) {
        lds_u32x2 *e = (lds_u32x2 *) (uintptr_t) (rq_lds + lane * (uint32_t) (kRareEntryWords * 4));
        q[0] = e[0]; q[1] = e[1]; q[2] = e[2]; q[3] = e[3];
        hd = e[4];
    }
    const bool paired = (hd.y >> 31) != 0u;
    const int64_t g = (int64_t) (((uint64_t) (hd.y & 0xFFu) << 32) | hd.x);
    const int32_t group = (int32_t) ((hd.y >> 8) & 0x3FFFu);
    // paired: word j = bits 8 ... 23 of result register j (low half) and of register j + 8 (high half): X's flag (bit 22) is bit 14 of its
    // half, Y's (bit 10) bit 2.  fx / fy: bit n = result register 15 - n.  Two accumulators walk the bits upwards one position per word.
    uint32_t lo = 0, hi = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const uint32_t w = (j & 1) ? q[j >> 1].y : q[j >> 1].x;
        lo = (lo + lo) | (w & 0x4004u);
        hi = (hi + hi) | ((w >> 16) & 0x4004u);
    }
    // register j <= 7: X at bit 21 - j, Y at bit 9 - j of lo; register 8 + j: the same of hi
    const uint32_t fx = ((lo >> 6) & 0xFF00u) | ((hi >> 14) & 0xFFu);
    const uint32_t fy = ((lo << 6) & 0xFF00u) | ((hi >> 2) & 0xFFu);
    // plain: word w = the top bytes of result registers 4 w ... 4 w + 3; bit n of the flags = register 15 - n is non-negative.  The four sign
    // bits of a word into a nibble (register 4 w first) by one multiplication: bits 0 / 8 / 16 / 24 x (2^27 + 2^18 + 2^9 + 1) meet at bits 27 ... 24
    uint32_t ms_ = 0;
#pragma unroll
    for (int w = 0; w < 4; w++) {
        const uint32_t t = (((w & 1) ? q[w >> 1].y : q[w >> 1].x) >> 7) & 0x01010101u;
        ms_ = (ms_ << 4) | ((t * 0x08040201u) >> 24 & 0xFu);
    }
    const uint32_t fs = ~ms_ & 0xFFFFu;
    emit_rec(E, mine, g, paired ? fx : fs, group);
    emit_rec(E, mine && paired, g, fy, group + 1);
    if (lane == 0) { em2[0] = u32x2{(uint32_t) E.base, (uint32_t) (E.base >> 32)}; ((lds_u32 *) (uintptr_t) em_lds)[2] = E.left; }
}

// OR of the 16 result patterns: some field of the lane is a candidate <=> (x & kPairMask) != 0.  v_bitop3_b32 by name: left alone
// hipcc picks v_or3_b32, which costs the SIMD 4.4 cycles against 2.7 (profiles/r03b_valu_rate.log)
__device__ __forceinline__ uint32_t or16(const f32x16 &c) {
    uint32_t x = __builtin_amdgcn_bitop3_b32((uint32_t) __float_as_int(c[0]), (uint32_t) __float_as_int(c[1]), (uint32_t) __float_as_int(c[2]), 0xFE);
#pragma unroll
    for (int i = 3; i < 15; i += 2) x = __builtin_amdgcn_bitop3_b32(x, (uint32_t) __float_as_int(c[i]), (uint32_t) __float_as_int(c[i + 1]), 0xFE);
    return x | (uint32_t) __float_as_int(c[15]);
}

// The lane's 8 bases of one k-block half as 32 fp4 one-hot k-slots: two reads of the 256-entry table (byte of four 2-bit codes ->
// 16 k-slots = 8 bytes).  n8 = the 8 bases' non-ACGT bits: such a base is an all-zero column (cscore.c:345-353 "adds nothing").
__device__ __forceinline__ i32x8 onehot_f4(const char *__restrict__ lut, uint32_t c16) {
    const int2 lo = *reinterpret_cast<const int2 *>(lut + ((c16 & 0xFFu) << 3)), hi = *reinterpret_cast<const int2 *>(lut + ((c16 >> 8) << 3));
    return i32x8{lo.x, lo.y, hi.x, hi.y, 0, 0, 0, 0};
}
__device__ __forceinline__ void clear_n(i32x8 &b, uint32_t n8) {
#pragma unroll
    for (int r = 0; r < 4; r++) {                                   // word r = bases 2r (low half) and 2r + 1 (high half)
        const uint32_t two = (n8 >> (2 * r)) & 3u;
        b[r] &= (int) (((two & 1u) ? 0u : 0xFFFFu) | ((two & 2u) ? 0u : 0xFFFF0000u));
    }
}

// What a pass keeps per lane for all its classes: the 64 bases (2-bit codes) from its two window starts g0 and g0 + 32.  Classes of 3
// or 4 k-blocks (motifs of 32 ... 63 columns: rare) read the 32 bases behind them themselves, and every class re-reads the
// non-ACGT bits where it needs them (rare): the narrow classes' hot loops own every register they can get.
struct PassSeq {
    uint64_t cw[2];
    const uint32_t *stg; // the wave's staged sequence words of this pass (LDS): 8 code words, then 4 non-ACGT words, from pass0 on
    bool any_n;          // wave-uniform: some lane sees a non-ACGT base in the 96 bases from g0
};

// ---- the double pass's one-hot array (the kernels for row tiles of 1 or 2 k-blocks; round 5) ----
// Every B operand of a pass is the fp4 one-hot image of EIGHT consecutive bases, 16 bytes, and the image of the bases from x on is the same
// whichever class, k-block, lane half or operand asks for it: paired half-block kb of the window at pass0 + r + 32 o + 64 s is entry
// r + 8 kb + 32 o + 64 s, plain k-block kb entry r + 16 kb + 8 h + 32 o + 64 s.  Rounds 2-4 (and the kernels with wide classes still) build each
// operand where it is used: two reads of the 256-entry table per operand (random 8-byte reads: the LDS array's only bank conflicts, 14 % of its
// busy cycles) and half a dozen vector instructions, ten operands per 64 windows on the benchmark plan.  A double pass builds entries 0 ... 159
// ONCE (lane l: entries l, 64 + l and 128 + (l & 31); non-ACGT bases cleared there), 2560 bytes per wave, and a class fetches its operands with
// one conflict-free ds_read_b128 each at a constant offset from the lane's entry.
constexpr int kOnehotEntries = 160;

// the 32 bases (2-bit codes) / their non-ACGT bits from window start pass0 + r + 32 i, cut out of the staged words (r = lane & 31):
// funnel shifts (v_alignbit_b32: a shift of 0 is the low operand itself, no special case)
__device__ __forceinline__ uint64_t staged_cw(const uint32_t *stg, uint32_t r, int i) {
    const uint32_t w = (r >> 4) + 2 * i, sh = (r & 15u) * 2u;
    const uint32_t lo = __builtin_amdgcn_alignbit(stg[w + 1], stg[w], sh), hi = __builtin_amdgcn_alignbit(stg[w + 2], stg[w + 1], sh);
    return ((uint64_t) hi << 32) | lo;
}
__device__ __forceinline__ uint32_t staged_nw(const uint32_t *stg, uint32_t r, int i) {
    return __builtin_amdgcn_alignbit(stg[9 + i], stg[8 + i], r);
}

// The matrix work of a row tile of TWO blocks.  Such a tile lies in LDS lane-major, 48 bytes per lane (ms_internal.h, f6_word_off): three
// 16-byte reads, of which the first six registers are the block-0 operand and the last six the block-1 operand.  The reads are
// ds_read_b128 because the LDS array is this kernel's second-busiest unit (SQ_LDS_IDX_ACTIVE ~70 % of the CU's cycles): the same 48
// bytes per lane as three strided pair reads (ds_read2st64_b64 on a plane-major tile) take the array 24 cycles instead of 12 -- 16.5-16.6
// against 17.0 ms per 500 Mbase on one box, six ds_read_b64 16.8 (profiles/r04d_a_reads_ab.log).  Rounds 4-5 wrote these products and the
// work hand-out's atomic as hand-written asm blocks; measured side by side in round 6 (profiles/r06b_e2e_ab_summary.log) the compiler's
// form below runs the pre-filter in the same time, so it is the only one.

// a two-block row tile's operands (lane-major, 48 bytes per lane: ms_internal.h) through ordinary LDS reads
__device__ __forceinline__ void load_a2(uint32_t pa, i32x8 &a0, i32x8 &a1) {
    const lds_i32x4 *q = (const lds_i32x4 *) (uintptr_t) pa;
    const i32x4 w0 = q[0], w1 = q[1], w2 = q[2];
    a0 = i32x8{w0[0], w0[1], w0[2], w0[3], w1[0], w1[1], 0, 0};
    a1 = i32x8{w1[2], w1[3], w2[0], w2[1], w2[2], w2[3], 0, 0};
}
__device__ __forceinline__ i32x8 b_of(const i32x4 &b) { return i32x8{b[0], b[1], b[2], b[3], 0, 0, 0, 0}; }
__device__ __forceinline__ void pair_product2_intr(const i32x8 &a0, const i32x8 &a1, const i32x4 &b00, const i32x4 &b10, const i32x4 &b01, const i32x4 &b11,
                                                   int scale0, int scale1, const f32x16 &cc0, const f32x16 &cc1, f32x16 &c0, f32x16 &c1) {
    c0 = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a0, b_of(b00), cc0, 2, 4, 0, scale0, 0, 127);
    c1 = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a0, b_of(b10), cc1, 2, 4, 0, scale1, 0, 127);
    c0 = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a1, b_of(b01), c0, 2, 4, 0, scale0, 0, 127);
    c1 = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a1, b_of(b11), c1, 2, 4, 0, scale1, 0, 127);
}
__device__ __forceinline__ void plain_product2_intr(const i32x8 &a0, const i32x8 &a1, const i32x4 &b00, const i32x4 &b10, const i32x4 &b01, const i32x4 &b11,
                                                    f32x16 &c0, f32x16 &c1) {
    const f32x16 z = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    c0 = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a0, b_of(b00), z, 2, 4, 0, 0, 0, 0);
    c1 = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a0, b_of(b10), z, 2, 4, 0, 0, 0, 0);
    c0 = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a1, b_of(b01), c0, 2, 4, 0, 0, 0, 0);
    c1 = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a1, b_of(b11), c1, 2, 4, 0, 0, 0, 0);
}

// All row tiles of one class of plain rows (NK k-blocks each).
template <int NK>
__device__ __forceinline__ void f6_class(const PfArgs &A, MfWave &W, const char *__restrict__ lds, const char *__restrict__ lut,
                                         uint32_t byte_off, int n_row_tiles, int32_t first_group, const PassSeq &Q,
                                         int64_t pass0, const PfLive &L, PfResume &R) {
    // pass0 = the pass's first window start (wave-uniform: scalar registers); this lane's two window starts are pass0 + r and
    // pass0 + r + 32 with r = lane & 31 -- recomputed where needed (rare paths), not carried
    const uint32_t lane = threadIdx.x & 63u, h = lane >> 5;
    // R.t: the row tile to start at; the class returns early, with the row tile to come back to in R, when the wave's parking space
    // runs low or full (the caller has the parked entries decoded -- ONE call site for all classes -- and comes back)
    constexpr int kStep = NK * kF6BytesPerKb;
    const char *p = lds + byte_off + lane * (NK == 2 ? 48u : 8u) + (uint32_t) R.t * (uint32_t) kStep;
    constexpr int NW = NK > 2 ? 3 : 2;
    // B operands: k-block kb of the window at g0 covers bases 16 kb + 8 h ... + 7 from g0; of the window at g0 + 32 the same from there
    i32x8 b0[NK], b1[NK];
    uint64_t cw[NW];
    cw[0] = Q.cw[0];
    cw[1] = Q.cw[1];
    if constexpr (NW == 3) cw[2] = staged_cw(Q.stg, lane & 31u, 2);
#pragma unroll
    for (int kb = 0; kb < NK; kb++) {
        const int w = kb >> 1, sh = 32 * (kb & 1);
        b0[kb] = onehot_f4(lut, (uint32_t) (cw[w] >> (sh + 16 * h)) & 0xFFFFu);
        b1[kb] = onehot_f4(lut, (uint32_t) (cw[w + 1] >> (sh + 16 * h)) & 0xFFFFu);
    }
    if (Q.any_n) {                                                                // rare, wave-uniform
        uint32_t nw[NW];
#pragma unroll
        for (int i = 0; i < NW; i++) nw[i] = staged_nw(Q.stg, lane & 31u, i);
#pragma unroll
        for (int kb = 0; kb < NK; kb++) {
            const int w = kb >> 1, sh = 16 * (kb & 1);
            const uint32_t keep = (kb == NK - 1 && h) ? 0x7Fu : 0xFFu;            // the row tile's last column carries the bias: never cleared
            clear_n(b0[kb], (nw[w] >> (sh + 8 * h)) & keep);
            clear_n(b1[kb], (nw[w + 1] >> (sh + 8 * h)) & keep);
        }
    }
    const f32x16 z = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    auto product = [&](const char *q, f32x16 &c0, f32x16 &c1) {
        i32x8 a[NK];
#pragma unroll
        for (int kb = 0; kb < NK; kb++) {
            const int2 w0 = *reinterpret_cast<const int2 *>(q + kb * kF6BytesPerKb);
            const int2 w1 = *reinterpret_cast<const int2 *>(q + kb * kF6BytesPerKb + 512);
            const int2 w2 = *reinterpret_cast<const int2 *>(q + kb * kF6BytesPerKb + 1024);
            a[kb] = i32x8{w0.x, w0.y, w1.x, w1.y, w2.x, w2.y, 0, 0};
        }
        // (scale operands 0, 0: the compiler emits the instruction without block scales, v_mfma_f32_32x32x64_f8f6f4 -- scale 2^0)
        c0 = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a[0], b0[0], z, 2, 4, 0, 0, 0, 0);
        c1 = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a[0], b1[0], z, 2, 4, 0, 0, 0, 0);
#pragma unroll
        for (int kb = 1; kb < NK; kb++) {
            c0 = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a[kb], b0[kb], c0, 2, 4, 0, 0, 0, 0);
            c1 = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a[kb], b1[kb], c1, 2, 4, 0, 0, 0, 0);
        }
    };
    // one row tile in flight per wave: with paired rows most instructions belong to four-instruction row tiles, and a second set of
    // 32 accumulators (round 2's two tiles in flight for the narrow classes) costs the whole kernel its registers
    // (ONE loop exit: a class that must leave early -- the parking space ran full inside row tile t: come back to it; or runs low:
    // come back to t + 1 -- sets `back` and ends the loop through its counter, so the hot path is product, inspection, one branch)
    int back = n_row_tiles;
    [[maybe_unused]] uint32_t pa = (uint32_t) (uintptr_t) (__attribute__((address_space(3))) const char *) p;       // the row tile's LDS address
    [[maybe_unused]] i32x4 bq[4];
    if constexpr (NK == 2) {
        bq[0] = i32x4{b0[0][0], b0[0][1], b0[0][2], b0[0][3]}; bq[1] = i32x4{b1[0][0], b1[0][1], b1[0][2], b1[0][3]};
        bq[2] = i32x4{b0[1][0], b0[1][1], b0[1][2], b0[1][3]}; bq[3] = i32x4{b1[1][0], b1[1][1], b1[1][2], b1[1][3]};
    }
    for (int t = R.t; t < n_row_tiles; t++, p += kStep, pa += (uint32_t) kStep) {
        f32x16 c0, c1;
        if constexpr (NK == 2) { i32x8 a0, a1; load_a2(pa, a0, a1); plain_product2_intr(a0, a1, bq[0], bq[1], bq[2], bq[3], c0, c1); }
        else product(p, c0, c1);
        const uint32_t x0 = all_negative(c0), x1 = all_negative(c1);
        if (__builtin_expect(__any((int) (x0 & x1) >= 0), 0)) {
            // rare path (about one row tile in four holds a candidate in some lane): the candidate lanes park their results
            const bool full = park_both(W, R, c0, c1, L, (int) x0 >= 0, (int) x1 >= 0, pass0 + (lane & 31u), first_group + 2 * t + (int32_t) h, 0u);
            if (full || W.rq_n >= W.rq_flush) { back = full ? t : t + 1; t = n_row_tiles; }
        }
    }
    R.t = back;
}

// All row tiles of one class of PAIRED rows (ms_internal.h): NK half-blocks of 8 columns, k-half 0 = field X, k-half 1 = field Y (block
// scales 2^-6 / 2^-18), both k-halves of the B operand = the same 8 bases, accumulators started at the inline constant 4.0, the bias
// column's B slots constant.  A row tile answers for 32 motifs x 2 strands with the 32 result registers that answer for 16 in a
// plain row tile.
template <int NK>
__device__ __forceinline__ void f6_pair_class(const PfArgs &A, MfWave &W, const char *__restrict__ lds, const char *__restrict__ lut,
                                              uint32_t byte_off, int n_row_tiles, int32_t first_group, const PassSeq &Q,
                                              int64_t pass0, const PfLive &L, PfResume &R) {
    const uint32_t lane = threadIdx.x & 63u, h = lane >> 5;
    constexpr int kStep = NK * kF6BytesPerKb;
    const char *p = lds + byte_off + lane * (NK == 2 ? 48u : 8u) + (uint32_t) R.t * (uint32_t) kStep;      // R: see f6_class
    // B operands: half-block kb covers bases 8 kb ... 8 kb + 7 of the window, in both lane halves
    i32x8 b0[NK], b1[NK];
#pragma unroll
    for (int kb = 0; kb < NK; kb++) {
        b0[kb] = onehot_f4(lut, (uint32_t) (Q.cw[0] >> (16 * kb)) & 0xFFFFu);
        b1[kb] = onehot_f4(lut, (uint32_t) (Q.cw[1] >> (16 * kb)) & 0xFFFFu);
    }
    if (Q.any_n) {                                                                // rare, wave-uniform
        const uint32_t nw0 = staged_nw(Q.stg, lane & 31u, 0), nw1 = staged_nw(Q.stg, lane & 31u, 1);
#pragma unroll
        for (int kb = 0; kb < NK; kb++) {
            const uint32_t keep = kb == NK - 1 ? 0x7Fu : 0xFFu;                   // the fields' last column carries the bias: never cleared
            clear_n(b0[kb], (nw0 >> (8 * kb)) & keep);
            clear_n(b1[kb], (nw1 >> (8 * kb)) & keep);
        }
    }
    // the bias column (last column of the last half-block): constant k-slots in place of the base's one-hot image
    b0[NK - 1][3] = (int) (((uint32_t) b0[NK - 1][3] & 0xFFFFu) | (kPairBiasB << 16));
    b1[NK - 1][3] = (int) (((uint32_t) b1[NK - 1][3] & 0xFFFFu) | (kPairBiasB << 16));
    // The two products of a row tile start from DIFFERENT inline constants, 4.0 and 2.0, with block scales one binade apart: the same
    // mantissa layout either way (a constant shared by two instructions is put into 16 registers by hipcc, eight v_mov per row tile)
    const int scale0 = h ? kPairScaleY : kPairScaleX, scale1 = scale0 - 1;
    f32x16 cc0, cc1;
#pragma unroll
    for (int j = 0; j < 16; j++) { cc0[j] = kPairC; cc1[j] = 0.5f * kPairC; }
    auto load_a = [&](const char *q, int kb) {
        const int2 w0 = *reinterpret_cast<const int2 *>(q + kb * kF6BytesPerKb);
        const int2 w1 = *reinterpret_cast<const int2 *>(q + kb * kF6BytesPerKb + 512);
        const int2 w2 = *reinterpret_cast<const int2 *>(q + kb * kF6BytesPerKb + 1024);
        return i32x8{w0.x, w0.y, w1.x, w1.y, w2.x, w2.y, 0, 0};
    };
    auto product = [&](const char *q, f32x16 &c0, f32x16 &c1) {
        // (three half-blocks: the A operands are read one or two at a time -- 6 B operands of 4 registers, 3 A operands of 6 and the
        // 32 results do not fit beside the rest)
        i32x8 a = load_a(q, 0);
        c0 = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b0[0], cc0, 2, 4, 0, scale0, 0, 127);
        c1 = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b1[0], cc1, 2, 4, 0, scale1, 0, 127);
#pragma unroll
        for (int kb = 1; kb < NK; kb++) {
            a = load_a(q, kb);
            c0 = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b0[kb], c0, 2, 4, 0, scale0, 0, 127);
            c1 = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b1[kb], c1, 2, 4, 0, scale1, 0, 127);
        }
    };
    int back = n_row_tiles;                                                         // (one loop exit: see f6_class)
    [[maybe_unused]] uint32_t pa = (uint32_t) (uintptr_t) (__attribute__((address_space(3))) const char *) p;       // the row tile's LDS address
    [[maybe_unused]] i32x4 bq[4];
    if constexpr (NK == 2) {
        bq[0] = i32x4{b0[0][0], b0[0][1], b0[0][2], b0[0][3]}; bq[1] = i32x4{b1[0][0], b1[0][1], b1[0][2], b1[0][3]};
        bq[2] = i32x4{b0[1][0], b0[1][1], b0[1][2], b0[1][3]}; bq[3] = i32x4{b1[1][0], b1[1][1], b1[1][2], b1[1][3]};
    }
    for (int t = R.t; t < n_row_tiles; t++, p += kStep, pa += (uint32_t) kStep) {
        f32x16 c0, c1;
        if constexpr (NK == 2) { i32x8 a0, a1; load_a2(pa, a0, a1); pair_product2_intr(a0, a1, bq[0], bq[1], bq[2], bq[3], scale0, scale1, cc0, cc1, c0, c1); }
        else product(p, c0, c1);
        const uint32_t x0 = or16(c0), x1 = or16(c1);
        if (__builtin_expect(__any(((x0 | x1) & kPairMask) != 0u), 0)) {
            // rare path: the candidate lanes park their results (table groups 4 t + 2 h for field X and + 1 for field Y)
            const bool full = park_both(W, R, c0, c1, L, (x0 & kPairMask) != 0u, (x1 & kPairMask) != 0u, pass0 + (lane & 31u),
                                        first_group + 4 * t + 2 * (int32_t) h, 1u);
            if (full || W.rq_n >= W.rq_flush) { back = full ? t : t + 1; t = n_row_tiles; }
        }
    }
    R.t = back;
}

// ---- dense candidates (round 5): the kernel for cutoffs at which nearly every row tile holds candidates ----
// Parking pays while an event is a lane or a few in a row tile (p = 1e-4: 0.4 hits per 64 windows x 32 rows; p = 1e-3: 4.4 -- there the parked
// form still wins, 31.9 against 34.9 ms per 500 Mbase).  At p = 1e-2 a row tile holds 44: a third of the lanes of both operands park, the
// space is decoded after every event and the hand-off is most of the kernel.  There the flags are decoded IN PLACE for the whole wave -- the
// vector work that costs the same for one lane or 64 is well used -- and the records go straight into the wave's block of the list, its
// place kept in scalar registers (no parking space, no pf_flush): 5.7 against 9.5 ms on the 62.5-Mbase shard (profiles/r05_dense_form.log).
// A scan launches this instantiation (ScanGeom::dense, ms_scan_geom.cpp) when the PREVIOUS scan of the PWM set at these cutoffs and strands found more than
// kDenseHitsPerHalfTile hits per row tile and 64 windows.
struct PfOut {
    unsigned long long base;   // next free slot of this wave's block in the global candidate list
    uint32_t left;             // slots left in the block
};
// one record per flagged lane into the wave's block (ranks by ballot / mbcnt; a block that cannot take them all is abandoned: its rest becomes
// empty records, the next one comes from the counter)
__device__ __forceinline__ void put_recs(const PfArgs &A, PfOut &O, bool flagged, uint64_t rec) {
    const unsigned long long mask = __builtin_amdgcn_ballot_w64(flagged);
    if (mask == 0) return;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t n_new = (uint32_t) __popcll(mask);
    const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t) (mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t) mask, 0u));
    if (n_new > O.left) {                                           // (cand_block >= 64 >= n_new: the next block always fits them)
        if (lane < O.left && O.base + lane < A.cand_cap) A.cand[O.base + lane] = 0ULL;
        unsigned long long b = 0;
        if (lane == 0) b = A.cand_static + atomicAdd(A.n_cand, (unsigned long long) A.cand_block);
        O.base = ((unsigned long long) (uint32_t) __builtin_amdgcn_readfirstlane((int) (b >> 32)) << 32) |
                 (unsigned long long) (uint32_t) __builtin_amdgcn_readfirstlane((int) b);
        O.left = A.cand_block;
    }
    if (flagged && O.base + rank < A.cand_cap) A.cand[O.base + rank] = rec;
    O.base += n_new;
    O.left -= n_new;
}
template <bool PAIRED>
__device__ __forceinline__ void dense_event(const PfArgs &A, PfOut &O, const f32x16 &c0, const f32x16 &c1, const PfLive &L, int64_t g0, int32_t group) {
    if constexpr (PAIRED) {
        uint32_t x0, y0, x1, y1;
        pair_flags(c0, x0, y0);
        pair_flags(c1, x1, y1);
        put_recs(A, O, L.l0 && x0 != 0u, cand_pack((uint64_t) g0, (uint32_t) group, x0));
        put_recs(A, O, L.l0 && y0 != 0u, cand_pack((uint64_t) g0, (uint32_t) group + 1u, y0));
        put_recs(A, O, L.l1 && x1 != 0u, cand_pack((uint64_t) g0 + 32u, (uint32_t) group, x1));
        put_recs(A, O, L.l1 && y1 != 0u, cand_pack((uint64_t) g0 + 32u, (uint32_t) group + 1u, y1));
    } else {
        const uint32_t f0 = nonneg_flags(c0), f1 = nonneg_flags(c1);
        put_recs(A, O, L.l0 && f0 != 0u, cand_pack((uint64_t) g0, (uint32_t) group, f0));
        put_recs(A, O, L.l1 && f1 != 0u, cand_pack((uint64_t) g0 + 32u, (uint32_t) group, f1));
    }
}

// ---- classes of a double pass (kernels without wide classes, round 5) ----
// A row tile's operand is read ONCE for 128 window starts: it is multiplied with the B operands of the windows from pass0 and from
// pass0 + 32, the results are inspected, then the SAME registers are multiplied with those of pass0 + 64 and pass0 + 96.  Why: the pre-filter is power-limited (tools/power_probe.py: ~1240 W of the board's 1400 W over a scan loop, the
// shader clock at 2.25 instead of 2.40 GHz), and with the operand reads of the two-block paired row tiles taken out the SAME cycle count ran
// at 2343 instead of 2188 MHz (profiles/r05_double_pass.log): the LDS reads cost clock, not cycles.  Half the reads, half the row-tile loop
// trips.  The accumulators are the same 32 registers for both halves.
struct PfLive2 { PfLive h[2]; };       // the halves of a double pass: windows from pass0 / from pass0 + 64

// What the halves of a row tile share: inspection result -> the candidate lanes park.  Returns true when the parking space ran full
// inside this half (the class leaves and comes back to row tile t, half s); sets `low` when the space runs low (the class leaves after t).
template <bool PAIRED>
__device__ __forceinline__ bool half_event(MfWave &W, PfResume &R, const f32x16 &c0, const f32x16 &c1, const PfLive &L, uint32_t x0, uint32_t x1,
                                           int64_t g0, int32_t group, bool &low) {
    const bool cand0 = PAIRED ? (x0 & kPairMask) != 0u : (int) x0 >= 0, cand1 = PAIRED ? (x1 & kPairMask) != 0u : (int) x1 >= 0;
    const bool full = park_both(W, R, c0, c1, L, cand0, cand1, g0, group, PAIRED ? 1u : 0u);
    low = low || W.rq_n >= W.rq_flush;
    return full;
}

// All row tiles of one class of PAIRED rows against the 128 window starts of a double pass (hw: the wave's one-hot array of the pass).
template <int NK, bool DENSE>
__device__ __forceinline__ void f6_pair_class2(const PfArgs &A, MfWave &W, PfOut &O, const char *__restrict__ lds, uint32_t byte_off, int n_row_tiles, int32_t first_group,
                                               uint32_t hw, int64_t pass0, const PfLive2 &L, PfResume &R) {
    static_assert(NK == 1 || NK == 2, "paired rows have one or two half-blocks");
    const uint32_t lane = threadIdx.x & 63u, h = lane >> 5, r = lane & 31u;
    constexpr int kStep = NK * kF6BytesPerKb;
    const char *p = lds + byte_off + lane * (NK == 2 ? 48u : 8u) + (uint32_t) R.t * (uint32_t) kStep;
    // B operands: half-block kb of the window at pass0 + r + 32 o + 64 s = entry r + 8 kb + 32 o + 64 s of the one-hot array
    i32x4 b[2][2][NK];
    {
        const lds_i32x4 *e = (const lds_i32x4 *) (uintptr_t) (hw + r * 16u);
#pragma unroll
        for (int sg = 0; sg < 2; sg++)
#pragma unroll
            for (int o = 0; o < 2; o++) {
#pragma unroll
                for (int kb = 0; kb < NK; kb++) b[sg][o][kb] = e[8 * kb + 32 * o + 64 * sg];
                // the bias column (last column of the last half-block): constant k-slots in place of the base's one-hot image
                b[sg][o][NK - 1][3] = (int) (((uint32_t) b[sg][o][NK - 1][3] & 0xFFFFu) | (kPairBiasB << 16));
            }
    }
    const int scale0 = h ? kPairScaleY : kPairScaleX, scale1 = scale0 - 1;         // (see f6_pair_class)
    f32x16 cc0, cc1;
#pragma unroll
    for (int j = 0; j < 16; j++) { cc0[j] = kPairC; cc1[j] = 0.5f * kPairC; }
    int back = n_row_tiles;
    [[maybe_unused]] uint32_t pa = (uint32_t) (uintptr_t) (__attribute__((address_space(3))) const char *) p;
    for (int t = R.t; t < n_row_tiles; t++, p += kStep, pa += (uint32_t) kStep) {
        f32x16 c0, c1;
        [[maybe_unused]] i32x8 a, a1;
        bool stop = false, low = false;
        if constexpr (NK == 2) { load_a2(pa, a, a1); pair_product2_intr(a, a1, b[0][0][0], b[0][1][0], b[0][0][1], b[0][1][1], scale0, scale1, cc0, cc1, c0, c1); }
        else {
            const int2 w0 = *reinterpret_cast<const int2 *>(p), w1 = *reinterpret_cast<const int2 *>(p + 512), w2 = *reinterpret_cast<const int2 *>(p + 1024);
            a = i32x8{w0.x, w0.y, w1.x, w1.y, w2.x, w2.y, 0, 0};
            c0 = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, i32x8{b[0][0][0][0], b[0][0][0][1], b[0][0][0][2], b[0][0][0][3], 0, 0, 0, 0}, cc0, 2, 4, 0, scale0, 0, 127);
            c1 = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, i32x8{b[0][1][0][0], b[0][1][0][1], b[0][1][0][2], b[0][1][0][3], 0, 0, 0, 0}, cc1, 2, 4, 0, scale1, 0, 127);
        }
        if (R.sub == 0u) {
            const uint32_t x0 = or16(c0), x1 = or16(c1);
            if (__builtin_expect(__any(((x0 | x1) & kPairMask) != 0u), DENSE ? 1 : 0)) {
                if constexpr (DENSE) dense_event<true>(A, O, c0, c1, L.h[0], pass0 + r, first_group + 4 * t + 2 * (int32_t) h);
                else if (half_event<true>(W, R, c0, c1, L.h[0], x0, x1, pass0 + r, first_group + 4 * t + 2 * (int32_t) h, low)) { back = t; R.sub = 0u; stop = true; }
            }
        }
        if (!stop) {
            if constexpr (NK == 2) pair_product2_intr(a, a1, b[1][0][0], b[1][1][0], b[1][0][1], b[1][1][1], scale0, scale1, cc0, cc1, c0, c1);
            else {
                c0 = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, i32x8{b[1][0][0][0], b[1][0][0][1], b[1][0][0][2], b[1][0][0][3], 0, 0, 0, 0}, cc0, 2, 4, 0, scale0, 0, 127);
                c1 = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, i32x8{b[1][1][0][0], b[1][1][0][1], b[1][1][0][2], b[1][1][0][3], 0, 0, 0, 0}, cc1, 2, 4, 0, scale1, 0, 127);
            }
            const uint32_t x0 = or16(c0), x1 = or16(c1);
            if (__builtin_expect(__any(((x0 | x1) & kPairMask) != 0u), DENSE ? 1 : 0)) {
                if constexpr (DENSE) dense_event<true>(A, O, c0, c1, L.h[1], pass0 + 64 + r, first_group + 4 * t + 2 * (int32_t) h);
                else if (half_event<true>(W, R, c0, c1, L.h[1], x0, x1, pass0 + 64 + r, first_group + 4 * t + 2 * (int32_t) h, low)) { back = t; R.sub = 1u; stop = true; }
            }
            if (!stop) {
                R.sub = 0u;
                if (low) { back = t + 1; stop = true; }
            }
        }
        if (stop) t = n_row_tiles;
    }
    R.t = back;
}

// ... and of plain rows (one or two k-blocks)
template <int NK, bool DENSE>
__device__ __forceinline__ void f6_class2(const PfArgs &A, MfWave &W, PfOut &O, const char *__restrict__ lds, uint32_t byte_off, int n_row_tiles, int32_t first_group,
                                          uint32_t hw, bool any_n, int64_t pass0, const PfLive2 &L, PfResume &R) {
    static_assert(NK == 1 || NK == 2, "the double pass knows row tiles of one or two k-blocks");
    const uint32_t lane = threadIdx.x & 63u, h = lane >> 5, r = lane & 31u;
    constexpr int kStep = NK * kF6BytesPerKb;
    const char *p = lds + byte_off + lane * (NK == 2 ? 48u : 8u) + (uint32_t) R.t * (uint32_t) kStep;
    // B operands: k-block kb of the window at pass0 + r + 32 o + 64 s covers the bases 16 kb + 8 h ... + 7 behind it: entry r + 8 h + 16 kb + 32 o + 64 s
    i32x4 b[2][2][NK];
    {
        const lds_i32x4 *e = (const lds_i32x4 *) (uintptr_t) (hw + (r + 8u * h) * 16u);
#pragma unroll
        for (int sg = 0; sg < 2; sg++)
#pragma unroll
            for (int o = 0; o < 2; o++) {
#pragma unroll
                for (int kb = 0; kb < NK; kb++) b[sg][o][kb] = e[16 * kb + 32 * o + 64 * sg];
                // rare, wave-uniform: the row tile's last column carries the bias, its base must not read as "no base" (any of the
                // column's four k-slots: they hold the same entry)
                if (any_n && h && ((uint32_t) b[sg][o][NK - 1][3] >> 16) == 0u) b[sg][o][NK - 1][3] |= 0x00020000;
            }
    }
    const f32x16 z = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    int back = n_row_tiles;
    [[maybe_unused]] uint32_t pa = (uint32_t) (uintptr_t) (__attribute__((address_space(3))) const char *) p;
    for (int t = R.t; t < n_row_tiles; t++, p += kStep, pa += (uint32_t) kStep) {
        f32x16 c0, c1;
        [[maybe_unused]] i32x8 a, a1;
        bool stop = false, low = false;
        if constexpr (NK == 2) { load_a2(pa, a, a1); plain_product2_intr(a, a1, b[0][0][0], b[0][1][0], b[0][0][1], b[0][1][1], c0, c1); }
        else {
            const int2 w0 = *reinterpret_cast<const int2 *>(p), w1 = *reinterpret_cast<const int2 *>(p + 512), w2 = *reinterpret_cast<const int2 *>(p + 1024);
            a = i32x8{w0.x, w0.y, w1.x, w1.y, w2.x, w2.y, 0, 0};
            c0 = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, i32x8{b[0][0][0][0], b[0][0][0][1], b[0][0][0][2], b[0][0][0][3], 0, 0, 0, 0}, z, 2, 4, 0, 0, 0, 0);
            c1 = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, i32x8{b[0][1][0][0], b[0][1][0][1], b[0][1][0][2], b[0][1][0][3], 0, 0, 0, 0}, z, 2, 4, 0, 0, 0, 0);
        }
        if (R.sub == 0u) {
            const uint32_t x0 = all_negative(c0), x1 = all_negative(c1);
            if (__builtin_expect(__any((int) (x0 & x1) >= 0), DENSE ? 1 : 0)) {
                if constexpr (DENSE) dense_event<false>(A, O, c0, c1, L.h[0], pass0 + r, first_group + 2 * t + (int32_t) h);
                else if (half_event<false>(W, R, c0, c1, L.h[0], x0, x1, pass0 + r, first_group + 2 * t + (int32_t) h, low)) { back = t; R.sub = 0u; stop = true; }
            }
        }
        if (!stop) {
            if constexpr (NK == 2) plain_product2_intr(a, a1, b[1][0][0], b[1][1][0], b[1][0][1], b[1][1][1], c0, c1);
            else {
                c0 = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, i32x8{b[1][0][0][0], b[1][0][0][1], b[1][0][0][2], b[1][0][0][3], 0, 0, 0, 0}, z, 2, 4, 0, 0, 0, 0);
                c1 = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, i32x8{b[1][1][0][0], b[1][1][0][1], b[1][1][0][2], b[1][1][0][3], 0, 0, 0, 0}, z, 2, 4, 0, 0, 0, 0);
            }
            const uint32_t x0 = all_negative(c0), x1 = all_negative(c1);
            if (__builtin_expect(__any((int) (x0 & x1) >= 0), DENSE ? 1 : 0)) {
                if constexpr (DENSE) dense_event<false>(A, O, c0, c1, L.h[1], pass0 + 64 + r, first_group + 2 * t + (int32_t) h);
                else if (half_event<false>(W, R, c0, c1, L.h[1], x0, x1, pass0 + 64 + r, first_group + 2 * t + (int32_t) h, low)) { back = t; R.sub = 1u; stop = true; }
            }
            if (!stop) {
                R.sub = 0u;
                if (low) { back = t + 1; stop = true; }
            }
        }
        if (stop) t = n_row_tiles;
    }
    R.t = back;
}

// grid = (blocks per tile, tiles); ONE 1024-thread block per CU (16 waves per CU, <= 128 VGPRs): its waves never meet at a barrier
// after the tables are loaded, so against round 2's two 512-thread blocks the only difference is ONE copy of the tables per CU --
// the other ~60 KB of LDS are the waves' parking space for candidates (and room for larger motif sets in one tile).
// Dynamic LDS: operand tables of the tile | B-operand table (kF6LutBytes) | per-wave sequence staging (kPfStageBytes) | per-wave
// PfEmit (kPfEmitBytes) | per-wave one-hot array of the pass (kPfOnehotBytes) | per-wave parking space (what is left, 16 ... 64 entries per wave).
// Work is handed out per WAVE, without a barrier in the loop: a wave's first unit is its own number, every further unit one
// atomicAdd on one of the tile's kPfCounters counter words (64 bytes apart; the blocks are dealt round-robin onto them and a word
// hands out every kPfCounters-th unit), requested before the current unit is scanned (the atomic's latency hides behind the unit);
// a unit = wave_passes x 64 consecutive window starts, sized on the host (ms_scan_geom.cpp).  A block whose CU is still busy with another
// stream's kernel starts late and simply takes fewer units (profiles/r02_stream_coexistence.log, r02_wave_occupancy_ab.log).
// MAXNK: 2 = the kernel for plans whose row tiles all have 1 or 2 k-blocks (motifs of up to 31 columns: every JASPAR-like set);
// 4 = the kernel that also knows row tiles of 3 and 4 k-blocks (its register allocation spills in rare paths).
// DENSE: the dense-candidate form (above), for plans without wide classes.
// (Measured and dropped in rounds 1-2: fetching the next pass's sequence words early, class
// descriptors in registers, waves walking the classes in rotated order, A operands fetched one row tile ahead (again in round 3, for the
// one-k-block class only, after tools/ubench/insp_probe.hip modes 6 / 7 promised -7 %: +6 % in the kernel), s_setprio around the
// matrix instructions, 12 / 20 / 24 waves per CU, 128 windows per wave, a block-wide hand-out behind barriers, one branch per pair
// of row tiles, a real function call for the rare path.)
template <int MAXNK, bool DENSE>
__global__ void __launch_bounds__(kPfThreads, 4) prefilter_f6_kernel(const PfArgs A) {
    static_assert(!DENSE || MAXNK == 2, "the dense-candidate form exists for the double-pass kernel");
    extern __shared__ uint4 lds4[];
    constexpr int NT = kPfThreads;
    const TileDesc *__restrict__ T = A.tiles + blockIdx.y;
    const bool wide = MAXNK > 2 && T->max_nk > 2;
    const uint32_t len16 = T->table_len16;
    const uint4 *__restrict__ src = A.tables + T->table_off16;
    for (uint32_t i = threadIdx.x; i < len16; i += NT) lds4[i] = src[i];
    uint4 *lut4 = lds4 + A.lut_off16;
    {
        // byte of four 2-bit codes -> 16 fp4 k-slots (8 bytes): slot 4 c + code_c = 1.0 (e2m1 code 0x2)
        uint2 *lut2 = reinterpret_cast<uint2 *>(lut4);
        for (uint32_t i = threadIdx.x; i < 256u; i += NT) {
            unsigned long long w = 0;
#pragma unroll
            for (int c = 0; c < 4; c++) w |= 2ULL << (4 * (4 * c + (int) ((i >> (2 * c)) & 3u)));
            lut2[i] = make_uint2((uint32_t) w, (uint32_t) (w >> 32));
        }
    }
    // The tile's class descriptors into LDS, 32 bytes apiece behind the B-operand table: a pass reads them from there, the next class's
    // while the current one runs.  (From global memory they came through VECTOR loads, each followed by s_waitcnt vmcnt(0) -- a wait that
    // also covers the next pass's sequence words in flight.  Measured: no difference in time on the benchmark set, profiles/r04_pf_account.log;
    // kept because the pass loop then holds no vector-memory wait but the staging's own.)
    int *cls_lds = reinterpret_cast<int *>(lut4 + 256 * 8 / 16);
    if (threadIdx.x < (uint32_t) kMaxClasses * 8u) {
        const uint32_t ci = threadIdx.x >> 3, f = threadIdx.x & 7u;
        static_assert(sizeof(ClassDesc) == 20, "ClassDesc layout");
        cls_lds[threadIdx.x] = f < 5u ? reinterpret_cast<const int *>(&T->cls[ci])[f] : 0;
    }
    __syncthreads();
    const char *lds = reinterpret_cast<const char *>(lds4);
    const char *lut = reinterpret_cast<const char *>(lut4);
    const int n_classes = T->n_classes;
    // The wave's number in its block: the same in all its lanes, which the compiler cannot know of threadIdx.x >> 6 -- read from the first
    // lane, it and everything made of it (the wave's LDS spaces, its units) live in scalar registers.  (Left in vector registers -- a dozen
    // of them, live through every pass -- they were what the narrow kernels spilled: rounds 5-13 ran with 11 / 13 spilled registers, reloaded
    // in front of every pass's sequence loads.)
    const uint32_t wv = (uint32_t) __builtin_amdgcn_readfirstlane((int) (threadIdx.x >> 6));
    // every wave OWNS a first block of the candidate list (no atomic: 4096 waves reserving their first block on one counter word
    // cost 45 us, the whole fixed cost of a small scan); further blocks come from the counter, behind the static ones
    MfWave W;
    W.rq = (uint32_t) (uintptr_t) (__attribute__((address_space(3))) void *) (lds4 + A.rare_off16) + wv * (A.rare_cap * (uint32_t) (kRareEntryWords * 4));
    W.rq_cap = A.rare_cap;
    W.rq_flush = A.rare_cap - (A.rare_cap > 32u ? A.rare_cap / 4u : 8u);
    W.rq_n = 0;
    PfEmit *em = reinterpret_cast<PfEmit *>(reinterpret_cast<uint32_t *>(lds4 + A.emit_off16) + wv * (uint32_t) kPfEmitWords);
    const uint32_t em_lds = (uint32_t) (uintptr_t) (__attribute__((address_space(3))) void *) em;
    const uint32_t rq_lds = W.rq;
    if ((threadIdx.x & 63u) == 0) {
        em->base = ((unsigned long long) blockIdx.y * gridDim.x + blockIdx.x) * (NT / 64) * A.cand_block + (unsigned long long) wv * A.cand_block;
        em->left = A.cand_block;
        em->cand = A.cand; em->n_cand = A.n_cand; em->cand_cap = A.cand_cap; em->cand_static = A.cand_static; em->cand_block = A.cand_block;
    }
    PfOut O;                                                                    // DENSE: the wave's place in the candidate list, in scalar registers
    {
        const uint32_t wave = (uint32_t) __builtin_amdgcn_readfirstlane((int) (((uint32_t) blockIdx.y * gridDim.x + blockIdx.x) * (uint32_t) (NT / 64) + wv));
        O.base = (unsigned long long) wave * A.cand_block;
        O.left = A.cand_block;
    }
    const uint32_t lane = threadIdx.x & 63u, r = lane & 31u;

    // The sequence words of a pass, staged per wave in LDS: the wave's window starts and the 32 (wide tiles: 64) bases behind the
    // last one span 16 code words and 8 non-ACGT words from pass0 on in a double pass (8 and 4 in a 64-window pass), which lanes
    // 0 ... 23 (11) fetch -- for the NEXT pass, before the current one is scanned, so that the global loads' latency hides behind a
    // pass of matrix work -- and every lane then cuts its own windows (double pass: its entries of the one-hot array) out of the staged words (rounds 1-2: ten global loads per lane and pass, their
    // latency exposed once per pass: a third of the kernel's time on inputs with few row tiles per pass, profiles/r03_c2_latency.log).
    uint32_t *stg = reinterpret_cast<uint32_t *>(lds4 + A.stage_off16) + wv * kPfStageWords;
    constexpr bool SH = MAXNK == 2;                                             // the double pass with its one-hot array: kernels without wide classes
    const uint32_t hw_lds = (uint32_t) (uintptr_t) (__attribute__((address_space(3))) void *) (lds4 + A.onehot_off16) + wv * (uint32_t) (kOnehotEntries * 16);
    // (32-bit word indices: a set holds <= 2^34 bases = 2^30 code words; the loads then take a scalar base and a 32-bit lane offset)
    const uint32_t n_code_words = (uint32_t) (2 * ((A.n_bases + 31) / 32) + kPadWords), n_mask_words = (uint32_t) ((A.n_bases + 31) / 32 + kPadWords);
    // A pass = PW window starts: 128 in the kernels without wide classes (the double pass: 16 code words and 8 non-ACGT words are staged,
    // 168 bases and their 6 words are needed), 64 in the others (8 + 4 words staged)
    constexpr uint32_t PW = SH ? 128u : 64u, CWP = PW / 16u, NWP = PW / 32u;      // window starts / code words / non-ACGT words per pass
    struct PassWords { uint32_t c, n; };                                        // what lane l loaded: code word l & (2 CWP - 1) and non-ACGT word l & (2 NWP - 1) of the pass
    auto fetch = [&](uint32_t pass, uint32_t ln) -> PassWords {                 // pass = pass0 / PW; ln = the lane's number (the caller's copy: below)
        // every lane loads from both arrays -- the same few cache lines -- through a SCALAR base (the pass is wave-uniform) and a small
        // lane offset: a per-lane 64-bit address costs a register pair that the kernel has not got.  The two results stay two
        // registers until they are staged: choosing between them here would make the wave wait for the loads here
        // (kPadWords >= 16 zero words follow both arrays: only the BASE needs clamping, for the dead passes behind the input's end)
        static_assert(kPadWords >= 16, "the staged words of a pass run up to 16 words past its first");
        const uint32_t bc = pass * CWP < n_code_words - 2u * CWP ? pass * CWP : n_code_words - 2u * CWP, bn = pass * NWP < n_mask_words - 2u * NWP ? pass * NWP : n_mask_words - 2u * NWP;
        typedef const __attribute__((address_space(1))) uint32_t *gptr;          // (a GLOBAL pointer: through an integer it would come back generic)
        auto uniform = [](const uint32_t *q) {                                  // the pointer into scalar registers, whatever the compiler thought of it
            const uint64_t a = reinterpret_cast<uint64_t>(q);
            return (gptr) (((uint64_t) (uint32_t) __builtin_amdgcn_readfirstlane((int) (a >> 32)) << 32) | (uint64_t) (uint32_t) __builtin_amdgcn_readfirstlane((int) a));
        };
        return PassWords{uniform(A.codes + bc)[ln & (2u * CWP - 1u)], uniform(A.nmask + bn)[ln & (2u * NWP - 1u)]};
    };
    auto scan_pass = [&](int64_t pass0) {                                    // 64 window starts of this wave (pass0 ... + 63, wave-uniform) against every class
        // (32-bit: what is left of the input from pass0 on is wave-uniform; a 64-bit position per lane costs two register pairs)
        const int64_t left64 = A.n_bases - pass0;
        const uint32_t left = left64 >= 64 ? 64u : (left64 > 0 ? (uint32_t) left64 : 0u);
        bool live0 = r < left, live1 = r + 32u < left;
        PassSeq Q;
        Q.stg = stg;
        Q.cw[0] = staged_cw(stg, r, 0);
        Q.cw[1] = staged_cw(stg, r, 1);
        const uint32_t nw0 = staged_nw(stg, r, 0), nw1 = staged_nw(stg, r, 1);
        const uint32_t nw2 = wide ? staged_nw(stg, r, 2) : 0u;                           // only classes of 3 or 4 k-blocks reach bases 64 ... 95
        Q.any_n = __any((nw0 | nw1 | nw2) != 0u);
        if (Q.any_n && A.skip_alln) {
            // a window whose bases are ALL non-ACGT (the tile's motifs span <= 32 bases, <= 64 with wide classes) scores 0 on every
            // motif and none reports that (plan: every threshold > 0): such lanes queue nothing, and a pass made of them only --
            // the inside of an assembly gap -- is skipped whole
            const bool dead0 = nw0 == 0xFFFFFFFFu && (!wide || nw1 == 0xFFFFFFFFu);
            const bool dead1 = nw1 == 0xFFFFFFFFu && (!wide || nw2 == 0xFFFFFFFFu);
            live0 = live0 && !dead0;
            live1 = live1 && !dead1;
            if (!__any(live0 || live1)) return;
        }
        const PfLive L{live0, live1, __builtin_amdgcn_ballot_w64(live0), __builtin_amdgcn_ballot_w64(live1)};
        auto read_cd = [&](int i) { return *reinterpret_cast<const int4 *>(cls_lds + 8 * i); };      // {nk, n_row_tiles, base16, first_group}; paired: word 4
        int4 cd4 = read_cd(0);
        int cdp = cls_lds[4];
        for (int i = 0; i < n_classes; i++) {
            ClassDesc cd;                                                         // wave-uniform: into scalar registers
            cd.nk = __builtin_amdgcn_readfirstlane(cd4.x);
            cd.n_row_tiles = __builtin_amdgcn_readfirstlane(cd4.y);
            cd.base16 = (uint32_t) __builtin_amdgcn_readfirstlane(cd4.z);
            cd.first_group = __builtin_amdgcn_readfirstlane(cd4.w);
            cd.paired = __builtin_amdgcn_readfirstlane(cdp);
            if (i + 1 < n_classes) { cd4 = read_cd(i + 1); cdp = cls_lds[8 * (i + 1) + 4]; }      // the next class's, while this one runs
            const uint32_t off = cd.base16 * 16u;
            PfResume R{0, 0u, 0u};
            while (R.t < cd.n_row_tiles) {                                        // a class comes back early when the parking space runs low
                if (cd.paired) {
                    if (cd.nk == 1) f6_pair_class<1>(A, W, lds, lut, off, cd.n_row_tiles, cd.first_group, Q, pass0, L, R);
                    else f6_pair_class<2>(A, W, lds, lut, off, cd.n_row_tiles, cd.first_group, Q, pass0, L, R);
                } else {
                    switch (cd.nk) {
                        case 1: f6_class<1>(A, W, lds, lut, off, cd.n_row_tiles, cd.first_group, Q, pass0, L, R); break;
                        case 2: f6_class<2>(A, W, lds, lut, off, cd.n_row_tiles, cd.first_group, Q, pass0, L, R); break;
                        case 3: if constexpr (MAXNK > 2) f6_class<3>(A, W, lds, lut, off, cd.n_row_tiles, cd.first_group, Q, pass0, L, R); else R.t = cd.n_row_tiles; break;
                        case 4: if constexpr (MAXNK > 2) f6_class<4>(A, W, lds, lut, off, cd.n_row_tiles, cd.first_group, Q, pass0, L, R); else R.t = cd.n_row_tiles; break;
                        default: R.t = cd.n_row_tiles; break;
                    }
                }
                if (W.rq_n >= W.rq_flush) { pf_flush(em_lds, rq_lds, W.rq_n); W.rq_n = 0; }
            }
        }
    };
    auto scan_pass2 = [&](int64_t pass0, bool any_n) {                        // the double pass: 128 window starts of this wave (pass0 ... + 127, wave-uniform) against every class
        const int64_t left64 = A.n_bases - pass0;
        const uint32_t left = left64 >= 128 ? 128u : (left64 > 0 ? (uint32_t) left64 : 0u);
        bool lv[4];
#pragma unroll
        for (int k = 0; k < 4; k++) lv[k] = r + 32u * (uint32_t) k < left;
        const uint32_t *stn = stg + 16;                                          // the staged non-ACGT words
        {
            // the pass's one-hot array (above PassSeq's helpers): lane l makes entries l, 64 + l and 128 + (l & 31) -- the 8 bases from pass0 + entry on,
            // cut out of the staged words with funnel shifts; a non-ACGT base is an all-zero column (any_n: rare, wave-uniform)
            // The three entries do not depend on each other, so they are made side by side, stage by stage: the staged words of all three,
            // then their six table reads, then the three writes -- two LDS round trips where making them one after the other, each behind the
            // non-ACGT branch of the one before, took six.  (The image made arithmetically instead -- word r = the packed 16-bit shift of {2, 2}
            // by four times the codes of bases 2r and 2r + 1, a dozen vector instructions per entry and one round trip -- was measured beside
            // this form in round 14 and is slower: 15.76 against 15.66 ms per 500 Mbase)
            // (the entries' numbers from a copy of the lane's number made here: the addresses of their staged words are five registers if
            // the compiler may carry them from pass to pass)
            uint32_t lq = lane;
            asm volatile("" : "+v"(lq));
            const uint32_t x[3] = {lq, 64u + lq, 128u + (lq & 31u)};
            uint32_t c16[3];
#pragma unroll
            for (int k = 0; k < 3; k++) c16[k] = __builtin_amdgcn_alignbit(stg[(x[k] >> 4) + 1], stg[x[k] >> 4], (x[k] & 15u) * 2u) & 0xFFFFu;
            i32x8 e[3];
#pragma unroll
            for (int k = 0; k < 3; k++) e[k] = onehot_f4(lut, c16[k]);
            if (any_n) {
#pragma unroll
                for (int k = 0; k < 3; k++) clear_n(e[k], __builtin_amdgcn_alignbit(stn[(x[k] >> 5) + 1], stn[x[k] >> 5], x[k] & 31u) & 0xFFu);
            }
            lds_i32x4 *hq = (lds_i32x4 *) (uintptr_t) hw_lds;
#pragma unroll
            for (int k = 0; k < 3; k++) hq[x[k]] = i32x4{e[k][0], e[k][1], e[k][2], e[k][3]};
        }
        if (any_n && A.skip_alln) {
            // a window whose bases are ALL non-ACGT (the tile's motifs span <= 32 bases) scores 0 on every motif and none reports that (plan:
            // every threshold > 0): such lanes queue nothing, and a pass made of them only -- the inside of an assembly gap -- is skipped whole
#pragma unroll
            for (int k = 0; k < 4; k++) lv[k] = lv[k] && __builtin_amdgcn_alignbit(stn[k + 1], stn[k], r) != 0xFFFFFFFFu;
            if (!__any(lv[0] || lv[1] || lv[2] || lv[3])) return;
        }
        const PfLive2 L{{PfLive{lv[0], lv[1], __builtin_amdgcn_ballot_w64(lv[0]), __builtin_amdgcn_ballot_w64(lv[1])},
                         PfLive{lv[2], lv[3], __builtin_amdgcn_ballot_w64(lv[2]), __builtin_amdgcn_ballot_w64(lv[3])}}};
        auto read_cd = [&](int i) { return *reinterpret_cast<const int4 *>(cls_lds + 8 * i); };      // {nk, n_row_tiles, base16, first_group}; paired: word 4
        int4 cd4 = read_cd(0);
        int cdp = cls_lds[4];
        for (int i = 0; i < n_classes; i++) {
            ClassDesc cd;                                                         // wave-uniform: into scalar registers
            cd.nk = __builtin_amdgcn_readfirstlane(cd4.x);
            cd.n_row_tiles = __builtin_amdgcn_readfirstlane(cd4.y);
            cd.base16 = (uint32_t) __builtin_amdgcn_readfirstlane(cd4.z);
            cd.first_group = __builtin_amdgcn_readfirstlane(cd4.w);
            cd.paired = __builtin_amdgcn_readfirstlane(cdp);
            if (i + 1 < n_classes) { cd4 = read_cd(i + 1); cdp = cls_lds[8 * (i + 1) + 4]; }      // the next class's, while this one runs
            const uint32_t off = cd.base16 * 16u;
            PfResume R{0, 0u, 0u, 0u};
            while (R.t < cd.n_row_tiles) {                                        // a class comes back early when the parking space runs low
                if (cd.paired) {
                    if (cd.nk == 1) f6_pair_class2<1, DENSE>(A, W, O, lds, off, cd.n_row_tiles, cd.first_group, hw_lds, pass0, L, R);
                    else f6_pair_class2<2, DENSE>(A, W, O, lds, off, cd.n_row_tiles, cd.first_group, hw_lds, pass0, L, R);
                } else if (cd.nk == 1) f6_class2<1, DENSE>(A, W, O, lds, off, cd.n_row_tiles, cd.first_group, hw_lds, any_n, pass0, L, R);
                else if (cd.nk == 2) f6_class2<2, DENSE>(A, W, O, lds, off, cd.n_row_tiles, cd.first_group, hw_lds, any_n, pass0, L, R);
                else R.t = cd.n_row_tiles;
                if (W.rq_n >= W.rq_flush) { pf_flush(em_lds, rq_lds, W.rq_n); W.rq_n = 0; }
            }
        }
    };
    {
        const uint32_t wave_passes = A.wave_passes < 1 ? 8u : (uint32_t) A.wave_passes;
        const uint32_t n_passes_total = (uint32_t) ((A.n_bases + PW - 1) / PW);       // <= 2^28: a set holds <= 2^34 bases
        const uint32_t n_units = (n_passes_total + wave_passes - 1) / wave_passes;
        constexpr uint32_t wpb = NT / 64;
        // A small input (A.use_counters == 0): one unit per wave, no atomic at all.  Else kPfCounters counter words per tile: a
        // wave's first unit in its word's group is its own number there; the words start at 0 and the waves add their group's
        // size themselves.
        const bool dyn = A.use_counters != 0;
        // (a uniform value INTO a scalar register: the divisions by K below are done by the vector unit, and what follows from them would stay
        // there -- the compiler knows it uniform and drops a readfirstlane as redundant.  Behind the empty statement it knows nothing of the
        // value, and the builtin stays; the instruction is still the compiler's own, with the wait states it wants around it)
        auto sgpr = [](uint32_t x) { asm volatile("" : "+v"(x)); return (uint32_t) __builtin_amdgcn_readfirstlane((int) x); };
        const uint32_t K = sgpr(!dyn ? 1u : (gridDim.x < (uint32_t) kPfCounters ? gridDim.x : (uint32_t) kPfCounters));     // every word needs a block
        const uint32_t g = sgpr(blockIdx.x % K);
        const uint32_t waves_g = sgpr(((gridDim.x - g + K - 1) / K) * wpb);
        const uint32_t units_g = sgpr(n_units > g ? (n_units - g + K - 1) / K : 0u);
        const uint32_t word_idx = sgpr(((uint32_t) blockIdx.y * (uint32_t) kPfCounters + g) * 16u);      // (<= 2^16 tiles: 32 bits hold it)
        unsigned int *word = A.chunk_counter + word_idx;
        uint32_t v = sgpr((blockIdx.x / K) * wpb + wv);                             // wave-uniform: everything derived from it lives in scalar registers
        PassWords words = v < units_g ? fetch((v * K + g) * wave_passes, lane) : PassWords{0u, 0u};
        while (v < units_g) {
            uint32_t next = 0xFFFFFFFFu;
            // the next unit: asked for before this one is scanned, looked at in its last pass
            unsigned int u = 0;
            const uint32_t uid = v * K + g;                                       // the unit: window starts [uid, uid + 1) * PW * wave_passes
            const uint32_t p0 = uid * wave_passes;
            for (uint32_t j = 0; j < wave_passes; j++) {                          // passes past the end scan dead lanes (last unit only)
                // The lane's number, made anew in every pass: what the set-up makes of it -- the staging's and the hand-out's lane conditions, the
                // two lane offsets of fetch() -- costs an instruction apiece, but carried through the pass (the compiler hoists all of it out of
                // the unit loop) a register or a pair of scalar registers apiece, which the scan has not got: the offsets came back from scratch
                // in front of either load, each behind a wait of its own
                uint32_t ln = lane;
                asm volatile("" : "+v"(ln));
                if (ln < 3u * CWP) stg[ln] = ln < 2u * CWP ? words.c : words.n;             // (the wave's LDS operations execute in order: no barrier)
                [[maybe_unused]] const bool pass_any_n = SH && __any((ln & (2u * NWP - 1u)) < 6u && words.n != 0u);        // (double pass: a non-ACGT base among the 192 staged)
                // (behind the staging, which waits for every vector-memory operation in flight)
                // (the counter word through a scalar base and a lane offset of 0 that the compiler cannot see through: of an atomic on an address it
                // knows uniform it makes a wave-wide reduction, whose result it reads -- and waits for -- on the spot)
                if (j == 0 && dyn && ln == 0) {
                    uint32_t zero = 0;
                    asm volatile("" : "+v"(zero));
                    u = atomicAdd(word + zero, 1u);
                }
                // the next pass's words -- of this unit, or the first of the wave's NEXT unit (its number arrived long ago) -- are in
                // flight while this pass is scanned
                if (j + 1 < wave_passes) words = fetch(p0 + j + 1, ln);
                else {
                    if (dyn) next = waves_g + sgpr(u);
                    if (next < units_g) words = fetch((next * K + g) * wave_passes, ln);
                }
                if constexpr (SH) scan_pass2((int64_t) (p0 + j) * 128, pass_any_n);
                else scan_pass((int64_t) (p0 + j) * 64);
            }
            v = next;
        }
    }
    if (W.rq_n) pf_flush(em_lds, rq_lds, W.rq_n);
    {                                                                             // the unused rest of the last block: empty records
        const unsigned long long base = DENSE ? O.base : em->base;
        const uint32_t left = DENSE ? O.left : em->left;
        // (parked form: the list and its size from the wave's PfEmit as well -- taken from the arguments they are four scalar registers kept
        // through the whole scan for this loop, which the scan has not got)
        uint64_t *const cand = DENSE ? A.cand : em->cand;
        const uint64_t cand_cap = DENSE ? A.cand_cap : em->cand_cap;
        for (uint32_t i = 0; i < left; i += 64) {
            const unsigned long long j = base + i + lane;
            if (i + lane < left && j < cand_cap) cand[j] = 0ULL;
        }
    }
}

typedef void (*PfKernel)(const PfArgs);
static PfKernel pf_kernel(bool wide, bool dense) {                  // (dense: only without wide classes)
    if (wide) return prefilter_f6_kernel<4, false>;
    return dense ? prefilter_f6_kernel<2, true> : prefilter_f6_kernel<2, false>;
}

int prefilter_set_lds(bool wide, bool dense, size_t bytes) {
    MS_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(pf_kernel(wide, dense)), hipFuncAttributeMaxDynamicSharedMemorySize, (int) bytes));
    return MS_OK;
}

// wide: the plan holds row tiles of 3 or 4 k-blocks; dense: the form that decodes candidates in place (many hits per row tile)
int launch_prefilter(const PfArgs &A, bool wide, bool dense, int blocks_per_tile, int n_tiles, size_t lds_bytes, hipStream_t st) {
    const int64_t n_chunks = (A.n_bases + kPfThreads - 1) / kPfThreads;
    if (blocks_per_tile > n_chunks) blocks_per_tile = (int) n_chunks;
    hipLaunchKernelGGL(pf_kernel(wide, dense), dim3((unsigned) blocks_per_tile, (unsigned) n_tiles), dim3(kPfThreads), lds_bytes, st, A);
    MS_HIP(hipGetLastError());
    return MS_OK;
}

}  // namespace ms
