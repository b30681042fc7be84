// ms_allelebest.hip -- the best-scoring window of every (motif, variant, haplotype) cell (ms_scan_alleles_best): the dense, cutoff-free
// form of ms_scan_alleles, as ms_scan_best is the dense form of ms_scan.
//
// For variant v = (chromosome, x, r, alt[0..a)) and motif m of width W the affected windows of either haplotype are ms_alleles.hip's
// (allele_windows: starts max(0, x - W + 1) .. min(x + len - 1, L_h - W) in that haplotype's coordinates), each scored as ms_scan scores
// it (columns 0 .. W - 1, forward M[b][c], reverse M[3 - b][W - 1 - c] at the same step, +0.0 for a base that adds nothing, raw / max_raw
// as one IEEE divide), and per haplotype they are walked in the reference's order -- start ascending, '+' before '-' -- from best = -inf,
// a window replacing the best iff its score is GREATER (ms_best.hip's rule).  26 bytes leave per cell: (score, offset, strand) twice.
//
// Mapping.  A block owns one motif and a tile of kAbTile variants; the motif's tab2 entries sit in LDS behind an all-zero entry
// (var_scan_kernel's layout), motifs wider than kAbTabMaxW read them from HBM.
//   Short cells (ab_cell_kernel): ONE THREAD per (variant) cell walks the windows of the ref and then of the alt haplotype one after
//   the other, in the reference's order, so that order holds by construction: no cross-lane reduction.  A single-base substitution
//   (r = a = 1) takes var_scan_kernel's walk: one pass over the columns gives the four raw sums of a window, the alt entry of column
//   k = x - s read once per window and selected.  For W <= 32 the 64 bases that hold all of a substitution's windows are read once and
//   window j's code / mask words are shifted out of those registers; wider motifs and the spliced walks read per window and step.
//   Long cells (ab_wave_kernel, a launch of its own so that the short path stays convergent): a cell that is not a substitution and has
//   more than kAbLongWindows affected windows on its two haplotypes together -- long insertions and deletions -- gets a wave per
//   (variant, haplotype); lanes stride over the windows and wave_best's total order decides (the greater q, equal q to the smaller
//   (start, strand) key).  The candidates are listed on the host (an upper bound that does not look at the motif); a wave whose cell is
//   short for its motif leaves at once, and ab_cell_kernel skips exactly the cells for which the same test says long.
//
// The divide is paid only by a window whose raw sum is strictly greater than the lane's best raw sum so far (ms_best.hip: with max_raw > 0
// a correctly rounded divide is monotone, so raw <= best_raw gives q <= best_q).  It stays exact per lane in the strided form because a
// lane's windows still ASCEND: a window with raw <= best_raw has q <= best_q and a greater (start, strand) key than the lane's best, so it
// loses under the total order as well as under the sequential rule; the lane's result is the first maximum of ITS windows, and the first
// maximum of the cell is, among the lanes' first maxima with the greatest q, the one of the smallest key -- what wave_best returns.
//
// No floating-point atomic, no sort, no data-dependent order; each of the six outputs of a cell is written exactly once: a scorable
// motif's short cells by their thread, its long cells by lane 0 of their two waves, every cell of an unscorable motif (ms_best.hip's
// definition) by ab_cell_kernel as the "no winner" triple (NaN, 0, 0).  Variants go in chunks (the grid's limits); the bytes do not depend
// on them (ms_debug_varscan_chunk sets the chunk here too).  The upload of the variants (al_upload) and the column step (tab_step) are
// ms_allele_dev.h's, shared with ms_alleles.hip, ms_personal.hip and ms_variants.hip.
#include <algorithm>
#include <memory>
#include <type_traits>

#include "ms_allele_dev.h"
#include "ms_best_dev.h"
#include "ms_device.h"
#include "ms_handles.h"

struct ms_allelebest {
    int device = 0;
    int32_t P = 0;
    int64_t V = 0;
    void *block = nullptr;                            // one pooled device block holding the six [P][V] arrays
    size_t block_bytes = 0;
    double *d_score[2] = {nullptr, nullptr};          // [0] ref haplotype, [1] alt; NaN: no winner
    int32_t *d_offset[2] = {nullptr, nullptr};        // winning start - x
    int8_t *d_strand[2] = {nullptr, nullptr};         // 1 '+', 2 '-', 0: no winner
    std::vector<uint8_t> mismatch;                    // [V]
    double device_ms = 0.0;                           // first launch -> last kernel done
};

namespace ms {

namespace {

constexpr int kAbThreads = 256;
constexpr int kAbTile = kAbThreads;             // variants per block: a thread each
constexpr int kAbLongWindows = 96;              // a cell (not a substitution) of more windows than this on both haplotypes together takes the wave path
constexpr int kAbTabMaxW = 896;                 // widest motif whose table (W x 4 entries, 56 KB) is staged in LDS; wider ones read it from HBM
constexpr int64_t kAbChunk = 1LL << 24;         // variants per launch (65536 tiles)
constexpr int kAbWaves = kAbThreads / 64;

struct AbOut {
    double *score[2];
    int32_t *offset[2];
    int8_t *strand[2];
};

struct AbArgs {
    const uint32_t *codes, *nmask, *acodes, *amask;
    int64_t n_bases;                             // bases of the packed genome
    DevPwm Pw;
    const uint8_t *scorable;                     // [P]
    const AlRec *rec;                            // [V]
    int64_t V;
    int strand_mask;
    AbOut O;
};

__device__ __forceinline__ bool ab_is_snv(const AlRec &q) { return q.r == 1 && q.a == 1; }

// the test both kernels make: this cell goes to the wave path
__device__ __forceinline__ bool ab_is_long(const AlRec &q, int W) {
    return !ab_is_snv(q) && allele_windows(q.lo, q.hi, q.r, W) + allele_windows(q.lo, q.hi, q.a, W) > (uint32_t) kAbLongWindows;
}

// window `rel` (its start, from x on) of haplotype hap (0 ref, 1 alt) of q: the two raw sums
template <bool LDS_TAB>
__device__ __forceinline__ void ab_window(const AbArgs &A, const double2 *lds, const double2 *__restrict__ tab_g, uint32_t zero, int W, const AlRec &q,
                                          int hap, int rel, double &fw, double &rv) {
    fw = 0.0;
    rv = 0.0;
    double u0 = 0.0, u1 = 0.0;
    for (int c0 = 0; c0 < W; c0 += 32) {
        const int n = (W - c0) < 32 ? (W - c0) : 32;
        uint64_t cw;
        uint32_t nw;
        if (hap) {
            alt_step(A.codes, A.nmask, A.acodes, A.amask, q, rel + c0, n, cw, nw);
        } else {
            cw = code_window(A.codes, q.g + rel + c0);
            nw = n_window(A.nmask, q.g + rel + c0);
        }
        tab_step<LDS_TAB, false>(lds, tab_g, zero, c0, n, cw, nw, -1, make_double2(0.0, 0.0), fw, rv, u0, u1);
    }
}

struct AbBest {                                  // a lane's best of one haplotype
    double raw, q;
    int32_t at;                                  // what the caller numbers its windows by
    int32_t strand;                              // 0: none yet
};

__device__ __forceinline__ AbBest ab_none() {
    AbBest b;
    b.raw = -std::numeric_limits<double>::infinity();
    b.q = b.raw;
    b.at = 0;
    b.strand = 0;
    return b;
}

// '+' then '-': the divide only where the raw sum improves (the header comment)
__device__ __forceinline__ void ab_take(AbBest &b, int strand_mask, double fw, double rv, double max_raw, int32_t at) {
    if ((strand_mask & 1) && fw > b.raw) {
        b.raw = fw;
        const double q = fw / max_raw;
        if (q > b.q) { b.q = q; b.at = at; b.strand = 1; }
    }
    if ((strand_mask & 2) && rv > b.raw) {
        b.raw = rv;
        const double q = rv / max_raw;
        if (q > b.q) { b.q = q; b.at = at; b.strand = 2; }
    }
}

__device__ __forceinline__ void ab_put(const AbOut &O, int hap, int64_t cell, double q, int32_t offset, int32_t strand) {
    O.score[hap][cell] = strand ? q : __builtin_nan("");
    O.offset[hap][cell] = strand ? offset : 0;
    O.strand[hap][cell] = (int8_t) strand;
}

// grid = (tiles of the chunk, motifs); a thread per variant of the tile.  LDS_TAB: the motif's table in LDS (W <= kAbTabMaxW) or read
// from HBM; a block of the other kind leaves at once.
template <bool LDS_TAB>
__global__ void __launch_bounds__(kAbThreads) ab_cell_kernel(const AbArgs A, int64_t v0, int64_t nv) {
    extern __shared__ double2 abtab_lds[];                     // [W * 4 + 1]: the motif's entries, and an all-zero one for the columns that add nothing
    const int32_t m = (int32_t) blockIdx.y;
    const int W = A.Pw.width[m];
    if ((W <= kAbTabMaxW) != LDS_TAB) return;
    const int64_t vl = (int64_t) blockIdx.x * kAbTile + threadIdx.x;
    const int64_t v = v0 + vl, cell = (int64_t) m * A.V + v;
    if (!A.scorable[m]) {                                      // (block-uniform) no cell of this motif has a winner
        if (vl < nv) {
            ab_put(A.O, 0, cell, 0.0, 0, 0);
            ab_put(A.O, 1, cell, 0.0, 0, 0);
        }
        return;
    }
    const double2 *__restrict__ tab_g = A.Pw.tab2 + A.Pw.tab_off[m];
    const uint32_t zero = (uint32_t) W * 4u;
    if (LDS_TAB) {
        tab_stage<kAbThreads>(abtab_lds, tab_g, W);
        __syncthreads();
    }
    if (vl >= nv) return;
    const AlRec q = A.rec[v];
    if (ab_is_long(q, W)) return;                              // ab_wave_kernel's
    const double max_raw = A.Pw.max_raw[m];
    const int base = q.lo < W - 1 ? q.lo : W - 1;              // bases in front of x that the first window starts at
    if (ab_is_snv(q)) {
        // windows s = x - k, k = base down to max(0, W - 1 - hi): the variant sits in column k
        const int k_last = W - 1 - q.hi > 0 ? W - 1 - q.hi : 0;
        const uint32_t a_code = (uint32_t) code_window(A.acodes, q.aoff) & 3u;
        const bool a_n = n_window(A.amask, q.aoff) & 1u;
        AbBest br = ab_none(), ba = ab_none();
        const int64_t g0 = q.g - base;
        // W <= 32 (block-uniform): all windows lie in the 64 bases from g0 on.  The second word pair is read only where the genome goes
        // on: a window needs it only if it reaches base g0 + 32, which is then inside the chromosome
        uint64_t c_lo = 0, c_hi = 0;
        uint32_t n_lo = 0, n_hi = 0;
        if (W <= 32) {
            c_lo = code_window(A.codes, g0);
            n_lo = n_window(A.nmask, g0);
            if (g0 + 32 < A.n_bases) {
                c_hi = code_window(A.codes, g0 + 32);
                n_hi = n_window(A.nmask, g0 + 32);
            }
        }
        for (int k = base; k >= k_last; k--) {
            const int j = base - k;
            double2 tk = make_double2(0.0, 0.0);               // what the alt allele adds at column k
            if (!a_n) {
                if constexpr (LDS_TAB) tk = abtab_lds[(uint32_t) k * 4u + a_code];
                else tk = tab_g[(uint32_t) k * 4u + a_code];
            }
            double rf = 0.0, rr = 0.0, af = 0.0, ar = 0.0;
            if (W <= 32) {
                const uint64_t cw = j ? (c_lo >> (2 * j)) | (c_hi << (64 - 2 * j)) : c_lo;
                const uint32_t nw = j ? (n_lo >> j) | (n_hi << (32 - j)) : n_lo;
                tab_step<LDS_TAB, true>(abtab_lds, tab_g, zero, 0, W, cw, nw, k, tk, rf, rr, af, ar);
            } else {
                for (int c0 = 0; c0 < W; c0 += 32) {
                    const int n = (W - c0) < 32 ? (W - c0) : 32;
                    const uint64_t cw = code_window(A.codes, g0 + j + c0);
                    const uint32_t nw = n_window(A.nmask, g0 + j + c0);
                    tab_step<LDS_TAB, true>(abtab_lds, tab_g, zero, c0, n, cw, nw, k - c0, tk, rf, rr, af, ar);
                }
            }
            ab_take(br, A.strand_mask, rf, rr, max_raw, -k);
            ab_take(ba, A.strand_mask, af, ar, max_raw, -k);
        }
        ab_put(A.O, 0, cell, br.q, br.at, br.strand);
        ab_put(A.O, 1, cell, ba.q, ba.at, ba.strand);
        return;
    }
#pragma unroll 1
    for (int hap = 0; hap < 2; hap++) {
        const int n_win = (int) allele_windows(q.lo, q.hi, hap ? q.a : q.r, W);
        AbBest b = ab_none();
#pragma unroll 1
        for (int i = 0; i < n_win; i++) {
            double fw, rv;
            ab_window<LDS_TAB>(A, abtab_lds, tab_g, zero, W, q, hap, i - base, fw, rv);
            ab_take(b, A.strand_mask, fw, rv, max_raw, i - base);
        }
        ab_put(A.O, hap, cell, b.q, b.at, b.strand);
    }
}

// grid = (ceil(2 x candidates of the chunk / kAbWaves), motifs): wave (2 c + hap) of the launch owns haplotype hap of candidate c
template <bool LDS_TAB>
__global__ void __launch_bounds__(kAbThreads) ab_wave_kernel(const AbArgs A, const int64_t *__restrict__ cand, int64_t n_cand) {
    extern __shared__ double2 abtab_lds[];
    const int32_t m = (int32_t) blockIdx.y;
    const int W = A.Pw.width[m];
    if ((W <= kAbTabMaxW) != LDS_TAB) return;
    if (!A.scorable[m]) return;                                // (ab_cell_kernel has filled the motif's row)
    const int wave = __builtin_amdgcn_readfirstlane((int) (threadIdx.x >> 6));
    const int lane = (int) (threadIdx.x & 63u);
    const int64_t item = (int64_t) blockIdx.x * kAbWaves + wave, ci = item >> 1;
    const int hap = (int) (item & 1);
    AlRec q = {};
    int64_t v = 0;
    bool is_long = false;
    if (ci < n_cand) {
        v = cand[ci];
        q = A.rec[v];
        is_long = ab_is_long(q, W);
    }
    if (!__syncthreads_or(is_long ? 1 : 0)) return;            // no long cell of this motif in the block: nothing to stage
    const double2 *__restrict__ tab_g = A.Pw.tab2 + A.Pw.tab_off[m];
    const uint32_t zero = (uint32_t) W * 4u;
    if (LDS_TAB) {
        tab_stage<kAbThreads>(abtab_lds, tab_g, W);
        __syncthreads();
    }
    if (!is_long) return;
    const double max_raw = A.Pw.max_raw[m];
    const int base = q.lo < W - 1 ? q.lo : W - 1;
    const int n_win = (int) allele_windows(q.lo, q.hi, hap ? q.a : q.r, W);
    AbBest b = ab_none();
#pragma unroll 1
    for (int i = lane; i < n_win; i += 64) {                   // ascending per lane: the divide argument holds lane by lane
        double fw, rv;
        ab_window<LDS_TAB>(A, abtab_lds, tab_g, zero, W, q, hap, i - base, fw, rv);
        ab_take(b, A.strand_mask, fw, rv, max_raw, i);
    }
    double bq = b.q;
    uint64_t key = b.strand ? (((uint64_t) (uint32_t) b.at << 2) | (uint32_t) b.strand) : kNoKey;
    wave_best(bq, key);
    if (lane == 0) {
        const bool won = key != kNoKey;
        ab_put(A.O, hap, (int64_t) m * A.V + v, bq, won ? (int32_t) (key >> 2) - base : 0, won ? (int32_t) (key & 3u) : 0);
    }
}

}  // namespace

}  // namespace ms

using namespace ms;

extern "C" {

int ms_debug_allelebest_dims(int32_t out[3]) {
    if (!out) { set_error("NULL argument"); return MS_ERR_INVALID; }
    out[0] = kAbTile;
    out[1] = kAbLongWindows;
    out[2] = kAbTabMaxW;
    return MS_OK;
}

void ms_allelebest_free(ms_allelebest *b) {
    if (!b) return;
    if (b->block) {
        (void) hipSetDevice(b->device);
        DeviceCtx *c = nullptr;
        if (get_ctx(b->device, &c) == MS_OK) pool_free(c, b->block, b->block_bytes); else (void) hipFree(b->block);
    }
    delete b;
}

int ms_scan_alleles_best(const ms_pwmset *pwms_c, const ms_genome *genome, const int32_t *chrom, const int64_t *pos, const int32_t *ref_len,
                         const char *alt_bases, const int64_t *alt_offsets, const char *ref_bases, int64_t n_variants, int strand_mask,
                         uint32_t flags, ms_allelebest **out) {
    if (!out) { set_error("out is NULL"); return MS_ERR_INVALID; }
    *out = nullptr;
    if (strand_mask < 1 || strand_mask > 3) { set_error("invalid strand mask %d (1 '+', 2 '-', 3 both)", strand_mask); return MS_ERR_INVALID; }
    if (flags != 0u) { set_error("unknown allele best-site scan flags 0x%x", flags); return MS_ERR_INVALID; }
    if (!require_device()) return MS_ERR_RUNTIME;
    if (!pwms_c || !genome) { set_error("NULL handle"); return MS_ERR_INVALID; }
    ms_pwmset *pwms = const_cast<ms_pwmset *>(pwms_c);
    const ms_seqset *G = reinterpret_cast<const ms_seqset *>(genome);
    const int64_t V = n_variants;
    const int32_t P = pwms->P;
    std::vector<int64_t> ref_off, cand;
    int64_t A = 0, Rn = 0;
    if (int vrc = validate_alleles(G, chrom, pos, ref_len, alt_bases, alt_offsets, ref_bases, V, ref_off, &A, &Rn)) return vrc;
    // the variants that can be long cells of SOME motif: no substitution, and r + a + 2 (W_max - 1) windows at most
    std::vector<uint8_t> ok;
    try {
        const int64_t slack = 2 * (int64_t) std::max(pwms->max_width - 1, 0);
        for (int64_t v = 0; v < V; v++) {
            const int64_t r = ref_len[v], a = alt_offsets[v + 1] - alt_offsets[v];
            if (!(r == 1 && a == 1) && r + a + slack > kAbLongWindows) cand.push_back(v);
        }
        ok.assign((size_t) std::max<int32_t>(P, 1), 0);
        for (int32_t m = 0; m < P; m++) ok[(size_t) m] = scorable(pwms, m) ? 1 : 0;
    } catch (const std::bad_alloc &) { set_error("out of host memory"); return MS_ERR_NOMEM; }
    DeviceCtx *c;
    int rc = get_ctx(G->device, &c);
    if (rc) return rc;
    std::unique_ptr<ms_allelebest> res(new (std::nothrow) ms_allelebest());
    if (!res) { set_error("out of host memory"); return MS_ERR_NOMEM; }
    try { res->mismatch.assign((size_t) V, 0); } catch (const std::bad_alloc &) { set_error("out of host memory"); return MS_ERR_NOMEM; }
    res->device = c->device;
    res->P = P;
    res->V = V;
    // ---- 26 bytes per cell, allocated before anything is launched: a failure there is the MS_ERR_NOMEM of the header (the test here only
    // keeps the byte counts below inside size_t)
    if (26.0 * (double) P * (double) V >= 0.5 * (double) std::numeric_limits<size_t>::max()) {
        set_error("%d x %lld cells do not fit the device", P, (long long) V);
        return MS_ERR_NOMEM;
    }
    const size_t cells = (size_t) P * (size_t) V, cz = std::max<size_t>(cells, 1);
    std::lock_guard<std::mutex> lk_dev(c->mu);
    std::lock_guard<std::mutex> lk_pwm(pwms->mu);
    MS_HIP(hipSetDevice(c->device));
    {
        Carve rv;
        Carve::Slot<double> s_score[2];
        Carve::Slot<int32_t> s_offset[2];
        Carve::Slot<int8_t> s_strand[2];
        for (int h = 0; h < 2; h++) s_score[h] = rv.add<double>(cz);
        for (int h = 0; h < 2; h++) s_offset[h] = rv.add<int32_t>(cz);
        for (int h = 0; h < 2; h++) s_strand[h] = rv.add<int8_t>(cz);
        void *blk = nullptr;
        size_t got = 0;
        if ((rc = pool_alloc(c, rv.bytes(), &blk, &got))) return rc;
        res->block = blk;
        res->block_bytes = got;
        for (int h = 0; h < 2; h++) {
            res->d_score[h] = Carve::at(blk, s_score[h]);
            res->d_offset[h] = Carve::at(blk, s_offset[h]);
            res->d_strand[h] = Carve::at(blk, s_strand[h]);
        }
    }
    ms_allelebest *raw = res.release();
    if (V == 0) { *out = raw; return MS_OK; }
    if ((rc = pwmset_upload(pwms, c->device, c->stream))) { ms_allelebest_free(raw); return rc; }
    const hipStream_t st = c->stream;

    int64_t chunk = varscan_chunk_setting();
    if (chunk <= 0) chunk = kAbChunk;
    chunk = std::min<int64_t>(chunk, V);
    const int64_t n_chunks = (V + chunk - 1) / chunk;

    Carve cv;
    const AlSlots us = al_upload_slots(cv, V, A, Rn);
    const auto s_ok = cv.add<uint8_t>((size_t) std::max<int32_t>(P, 1));
    const auto s_cand = cv.add<int64_t>(std::max<size_t>(cand.size(), 1));
    void *wblk = nullptr;
    size_t wgot = 0;
    if ((rc = pool_alloc(c, cv.bytes(), &wblk, &wgot))) {
        ms_allelebest_free(raw);
        return rc;
    }
    const AlDev U = al_upload_at(wblk, us);
    uint8_t *d_ok = Carve::at(wblk, s_ok);
    int64_t *d_cand = Carve::at(wblk, s_cand);
    auto fail = [&](int code) { (void) hipStreamSynchronize(st); pool_free(c, wblk, wgot); ms_allelebest_free(raw); return code; };   // (nothing queued may still read the blocks)
    auto hip_fail = [&](hipError_t e, const char *what) { set_error("%s failed: %s", what, hipGetErrorString(e)); return fail(e == hipErrorOutOfMemory ? MS_ERR_NOMEM : MS_ERR_RUNTIME); };

    AbArgs K;
    K.codes = G->d_codes; K.nmask = G->d_nmask; K.acodes = U.acode; K.amask = U.amask; K.n_bases = G->n_bases;
    K.Pw = dev_pwm(pwms); K.scorable = d_ok; K.rec = U.rec; K.V = V; K.strand_mask = strand_mask;
    for (int h = 0; h < 2; h++) { K.O.score[h] = raw->d_score[h]; K.O.offset[h] = raw->d_offset[h]; K.O.strand[h] = raw->d_strand[h]; }
    const int max_width = pwms->max_width;
    const int min_width = P > 0 ? *std::min_element(pwms->widths.begin(), pwms->widths.end()) : 0;
    int lds_width = 0;
    for (int32_t p = 0; p < P; p++) if (pwms->widths[p] <= kAbTabMaxW) lds_width = std::max(lds_width, (int) pwms->widths[p]);
    const size_t lds = ((size_t) lds_width * 4 + 1) * sizeof(double2);
    hipError_t he = hipSuccess;
    if (lds > 40 * 1024) {                                     // (wide motifs: rare enough to ask the driver every time; ab_wave_kernel has static LDS too)
        he = hipFuncSetAttribute(reinterpret_cast<const void *>(ab_cell_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds);
        if (he == hipSuccess) he = hipFuncSetAttribute(reinterpret_cast<const void *>(ab_wave_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds);
        if (he != hipSuccess) return hip_fail(he, "raising the LDS limit");
    }

    (void) hipEventRecord(c->ev[0], st);
    he = al_upload(G, U, chrom, pos, ref_len, alt_bases, alt_offsets, ref_bases, ref_off, V, A, Rn, raw->mismatch.data(), st);
    if (he == hipSuccess && P > 0) he = hipMemcpyAsync(d_ok, ok.data(), (size_t) P, hipMemcpyHostToDevice, st);
    if (he == hipSuccess && !cand.empty()) he = hipMemcpyAsync(d_cand, cand.data(), 8 * cand.size(), hipMemcpyHostToDevice, st);
    if (he != hipSuccess) return hip_fail(he, "variant upload");

    for (int64_t k = 0; P > 0 && k < n_chunks; k++) {
        const int64_t v0 = k * chunk, nv = std::min(chunk, V - v0);
        const dim3 grid((unsigned) ((nv + kAbTile - 1) / kAbTile), (unsigned) P);
        if (min_width <= kAbTabMaxW) {
            hipLaunchKernelGGL(ab_cell_kernel<true>, grid, dim3(kAbThreads), lds, st, K, v0, nv);
            if ((he = hipGetLastError()) != hipSuccess) return hip_fail(he, "allele best-site kernel");
        }
        if (max_width > kAbTabMaxW) {
            hipLaunchKernelGGL(ab_cell_kernel<false>, grid, dim3(kAbThreads), 0, st, K, v0, nv);
            if ((he = hipGetLastError()) != hipSuccess) return hip_fail(he, "allele best-site kernel (tables in HBM)");
        }
        // the chunk's candidates for the wave path: cand is ascending
        const int64_t c0 = std::lower_bound(cand.begin(), cand.end(), v0) - cand.begin();
        const int64_t c1 = std::lower_bound(cand.begin(), cand.end(), v0 + nv) - cand.begin();
        if (c1 > c0) {
            const dim3 wgrid((unsigned) ((2 * (c1 - c0) + kAbWaves - 1) / kAbWaves), (unsigned) P);
            if (min_width <= kAbTabMaxW) {
                hipLaunchKernelGGL(ab_wave_kernel<true>, wgrid, dim3(kAbThreads), lds, st, K, d_cand + c0, c1 - c0);
                if ((he = hipGetLastError()) != hipSuccess) return hip_fail(he, "allele best-site wave kernel");
            }
            if (max_width > kAbTabMaxW) {
                hipLaunchKernelGGL(ab_wave_kernel<false>, wgrid, dim3(kAbThreads), 0, st, K, d_cand + c0, c1 - c0);
                if ((he = hipGetLastError()) != hipSuccess) return hip_fail(he, "allele best-site wave kernel (tables in HBM)");
            }
        }
    }
    (void) hipEventRecord(c->ev[1], st);
    he = hipStreamSynchronize(st);
    if (he != hipSuccess) return hip_fail(he, "allele best-site scan");
    float ms01 = 0;
    (void) hipEventElapsedTime(&ms01, c->ev[0], c->ev[1]);
    raw->device_ms = ms01;
    pool_free(c, wblk, wgot);
    *out = raw;
    return MS_OK;
}

int ms_allelebest_shape(const ms_allelebest *b, int32_t *n_pwms, int64_t *n_variants) {
    if (!b) { set_error("NULL argument"); return MS_ERR_INVALID; }
    if (n_pwms) *n_pwms = b->P;
    if (n_variants) *n_variants = b->V;
    return MS_OK;
}

int ms_allelebest_sites(const ms_allelebest *b, int32_t m0, int32_t m1, double *score_ref, int32_t *offset_ref, int8_t *strand_ref,
                        double *score_alt, int32_t *offset_alt, int8_t *strand_alt) {
    if (!b) { set_error("NULL argument"); return MS_ERR_INVALID; }
    if (m0 < 0 || m1 > b->P || m0 > m1) { set_error("motif range [%d, %d) outside [0, %d)", m0, m1, b->P); return MS_ERR_INVALID; }
    const size_t at = (size_t) m0 * (size_t) b->V, n = (size_t) (m1 - m0) * (size_t) b->V;
    if (n == 0) return MS_OK;
    MS_HIP(hipSetDevice(b->device));
    double *score[2] = {score_ref, score_alt};
    int32_t *offset[2] = {offset_ref, offset_alt};
    int8_t *strand[2] = {strand_ref, strand_alt};
    for (int h = 0; h < 2; h++) {
        if (score[h]) MS_HIP(hipMemcpy(score[h], b->d_score[h] + at, 8 * n, hipMemcpyDeviceToHost));
        if (offset[h]) MS_HIP(hipMemcpy(offset[h], b->d_offset[h] + at, 4 * n, hipMemcpyDeviceToHost));
        if (strand[h]) MS_HIP(hipMemcpy(strand[h], b->d_strand[h] + at, n, hipMemcpyDeviceToHost));
    }
    return MS_OK;
}

int ms_allelebest_sites_device(const ms_allelebest *b, void **d_score_ref, void **d_offset_ref, void **d_strand_ref, void **d_score_alt,
                               void **d_offset_alt, void **d_strand_alt) {
    if (!b) { set_error("NULL argument"); return MS_ERR_INVALID; }
    if (d_score_ref) *d_score_ref = b->d_score[0];
    if (d_offset_ref) *d_offset_ref = b->d_offset[0];
    if (d_strand_ref) *d_strand_ref = b->d_strand[0];
    if (d_score_alt) *d_score_alt = b->d_score[1];
    if (d_offset_alt) *d_offset_alt = b->d_offset[1];
    if (d_strand_alt) *d_strand_alt = b->d_strand[1];
    return MS_OK;
}

int ms_allelebest_ref_mismatch(const ms_allelebest *b, uint8_t *out) {
    if (!b || (!out && b->V > 0)) { set_error("NULL argument"); return MS_ERR_INVALID; }
    std::copy(b->mismatch.begin(), b->mismatch.end(), out);
    return MS_OK;
}

int ms_allelebest_device_ms(const ms_allelebest *b, double *ms) {
    if (!b || !ms) { set_error("NULL argument"); return MS_ERR_INVALID; }
    *ms = b->device_ms;
    return MS_OK;
}

}  // extern "C"
