// ms_affinity.hip -- the summed likelihood ratio of every (motif, region) cell (ms_scan_affinity): total binding affinity, dense.
//
// For motif m of width W and region r of length L the TERMS of the cell are the (window start pos = 0 .. L - W, strand of the mask)
// pairs, with max_n >= 0 only the windows of at most max_n non-ACGT bases.  raw(term) is the raw sum exactly as ms_scan and ms_scan_best
// form it (columns 0 .. W - 1, forward M[b][c], reverse M[3 - b][W - 1 - c] at the same step, +0.0 for a base that adds nothing); max_raw
// is not read and nothing is divided: the PWMs are natural-log odds, so raw IS the window's log likelihood ratio.  Per cell
//     n_terms   the number of terms (a term of raw = -inf counts)
//     peak      the greatest raw over the terms                                       (bit-exact; NaN without a term; may be -inf)
//     sum       S = sum over the terms of exp(scale * (raw - peak)); raw = -inf adds 0
//     log_mean  scale * peak + log(S / n_terms), each operation rounded               (the plane ms_affinity_rank_sum ranks)
//
// Mapping: ms_best.hip's walk with another reduction at its end (ms_best_dev.h holds what the two share).  A wave owns a SEGMENT of
// kBestSegWindows window starts of a region, a block kBestWaves segments and one tile of motif tables in LDS; a lane keeps the words of
// its kBestStrips window starts in registers and walks the tile's motifs over them.
//
// The reducer is an ONLINE rescale: a lane's state is (peak, S, n) and a term x that is a number
//     x >  peak:   S = S * exp(scale * (peak - x)) + 1;   peak = x        (from peak = -inf: S = 0 * 0 + 1)
//     x <= peak:   S = S + exp(scale * (x - peak))
// -- ONE fp64 exp per term either way, its argument <= 0, no second pass over the strips and no 16 raw sums held in registers (the strip
// loop is not unrolled: ms_best_dev.h).  A term of raw = -inf only counts: it never meets the subtraction, so (-inf) - (-inf) is never
// formed.  A lane without a window in a strip, a strip past the region's last window and a window that max_n drops add neither a term
// nor a peak candidate.
//
// Order (the bytes are the same on every run, and a cell's bytes depend on nothing but its own motif, bases and arguments): a lane
// takes its terms in window order, '+' before '-'; then the wave's peak is the maximum over the lanes (exact, a butterfly of maxima),
// every lane rescales its S to it ONCE -- a lane that holds the wave's peak keeps its S untouched --, and S and n are added across the wave
// by a fixed xor butterfly (a + b == b + a: both partners of a step hold the same sum).  A region of one segment writes its cell; a
// longer one writes a partial (peak, S, n) per segment, and affinity_reduce_kernel folds a cell's partials: lane l takes segments
// l, l + 64, ... in ascending order by the same online rule -- S_a * exp(scale * (peak_a - peak)) + S_b * exp(scale * (peak_b - peak)),
// the factor of the greater peak being exactly 1 -- and the wave is reduced as above.  A partial of S = 0 (no term, or -inf terms only)
// adds its count and nothing else.  No atomics anywhere.
//
// Motifs wider than kBestTileMaxW read their table from HBM (score_window); a motif with a NaN or +inf entry is never scored and its
// row is filled with the "no term" cell (n_terms 0, peak NaN, sum 0, log_mean NaN).  A motif whose max_raw is <= 0 IS scored.
#include <algorithm>
#include <cmath>
#include <limits>
#include <memory>

#include "ms_best_dev.h"
#include "ms_device.h"
#include "ms_handles.h"

namespace ms {

namespace {

struct AffPart {                                         // a segment's share of one cell: 24 bytes
    double peak;                                         // -inf: no term that is a number
    double sum;
    int32_t n;
    int32_t reserved;
};

struct AffArgs {
    const uint32_t *codes, *nmask;
    const int64_t *offsets;                              // [R + 1]
    int64_t R;
    const int64_t *seg_first;                            // [R + 1] first segment of the region; nullptr: one segment per region
    const int64_t *part_first;                           // [R + 1] first partial of the region; nullptr: no partials
    int64_t n_seg, n_part;
    const int32_t *tile_first;                           // [tiles + 1] into mot
    const int32_t *mot;                                  // the scored motifs, tile after tile
    DevPwm Pw;
    int strand_mask;
    int32_t max_n;
    double scale;
    double *peak, *sum, *log_mean;                       // [P][R]
    int32_t *n_terms;
    AffPart *part;                                       // [P][n_part]
};

// one term of raw sum x into a lane's (peak, S, n); counted: the window is a term at all.  Wave-uniform control flow: exp is one call.
__device__ __forceinline__ void aff_term(bool counted, double x, double scale, double &peak, double &S, int32_t &n) {
    n += counted ? 1 : 0;
    const bool live = counted && x > -std::numeric_limits<double>::infinity();      // (x is never NaN or +inf: no such entry is scored)
    const bool up = live && x > peak;
    const double d = live ? (up ? peak - x : x - peak) : 0.0;                       // <= 0; -inf on a lane's first number
    const double e = exp(scale * d);
    S = live ? (up ? S * e + 1.0 : S + e) : S;
    peak = up ? x : peak;
}

// (pp, ps, pn) of an earlier reduction into (peak, S, n), by the same rule; ps > 0 implies a finite pp
__device__ __forceinline__ void aff_fold(double pp, double ps, int32_t pn, double scale, double &peak, double &S, int32_t &n) {
    n += pn;
    const bool live = ps > 0.0;
    const bool up = live && pp > peak;
    const double d = live ? (up ? peak - pp : pp - peak) : 0.0;
    const double e = d == 0.0 ? 1.0 : exp(scale * d);
    S = live ? (up ? S * e + ps : S + ps * e) : S;
    peak = up ? pp : peak;
}

// the lanes' (peak, S, n) -> the wave's, in every lane
__device__ __forceinline__ void aff_wave(double scale, double &peak, double &S, int32_t &n) {
    double wp = peak;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const double o = __shfl_xor(wp, d);
        wp = o > wp ? o : wp;
    }
    const bool shift = S > 0.0 && peak != wp;            // (S > 0: peak is a number, and so is wp)
    const double e = exp(scale * (shift ? peak - wp : 0.0));
    S = shift ? S * e : S;
    peak = wp;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        S += __shfl_xor(S, d);
        n += __shfl_xor(n, d);
    }
}

__device__ __forceinline__ void put_cell(const AffArgs &A, int64_t cell, double peak, double S, int32_t n) {
    const double ninf = -std::numeric_limits<double>::infinity(), nan = __builtin_nan("");
    const bool none = n == 0, dead = peak == ninf;
    A.n_terms[cell] = n;
    A.peak[cell] = none ? nan : peak;
    A.sum[cell] = (none || dead) ? 0.0 : S;
    const double ratio = S / (double) (none ? 1 : n);
    const double a = A.scale * peak, b = log(ratio);
    A.log_mean[cell] = none ? nan : (dead ? ninf : a + b);
}

// grid = (ceil(segments / kBestWaves), tiles).  LDS: the tile's tables in LDS; !LDS: one motif per tile, its table in HBM.
template <bool LDS>
__global__ void __launch_bounds__(kBestThreads, 4) affinity_kernel(const AffArgs A, int32_t tile0) {
    extern __shared__ double2 aff_lds[];                 // [1 + the tile's entries]
    const int32_t tile = tile0 + (int32_t) blockIdx.y;
    const int32_t k0 = A.tile_first[tile], k1 = A.tile_first[tile + 1];
    const int64_t tab0 = A.Pw.tab_off[A.mot[k0]];
    if (LDS) {
        const int32_t ml = A.mot[k1 - 1];
        const int32_t n = (int32_t) (A.Pw.tab_off[ml] - tab0) + A.Pw.width[ml] * 4;
        dense_stage_tile(aff_lds, A.Pw.tab2 + tab0, n);
    }
    const int wave = __builtin_amdgcn_readfirstlane((int) (threadIdx.x >> 6));
    const int lane = (int) (threadIdx.x & 63u);
    const int64_t seg = (int64_t) blockIdx.x * kBestWaves + wave;
    if (seg >= A.n_seg) return;
    const int64_t r = A.seg_first ? find_region_bsearch(A.seg_first, A.R, seg) : seg;
    const int64_t s_in = A.seg_first ? seg - A.seg_first[r] : 0;
    const bool whole = A.seg_first ? A.seg_first[r + 1] - A.seg_first[r] == 1 : true;
    const int64_t beg = A.offsets[r], L = A.offsets[r + 1] - beg;
    const int64_t p0 = s_in * kBestSegWindows;           // the segment's first window start

    uint64_t cw[kBestStrips];
    uint32_t nw[kBestStrips];
    dense_segment_words(A.codes, A.nmask, beg, L, p0, lane, cw, nw);

    for (int32_t k = k0; k < k1; k++) {
        const int32_t m = A.mot[k];
        const int W = A.Pw.width[m];
        const int64_t tab_m = A.Pw.tab_off[m];
        const uint32_t tb = 1u + (uint32_t) (tab_m - tab0);
        const int64_t last = L - W;                       // the region's last window start
        double peak = -std::numeric_limits<double>::infinity(), S = 0.0;
        int32_t n = 0;
#pragma unroll 1
        for (int s = 0; s < kBestStrips; s++) {
            if (p0 + s * 64 > last) break;                // (wave-uniform) no window of this strip, or of a later one, fits the region
            const int64_t pos = p0 + s * 64 + lane;
            const bool valid = pos <= last;
            double fwd = 0.0, rev = 0.0;
            int n_non = 0;
            dense_strip_sums<LDS, true>(aff_lds, tb, A.Pw.tab2 + tab_m, A.codes, A.nmask, W, beg + pos, valid, s, cw, nw, fwd, rev, n_non);
            const bool counted = valid && (A.max_n < 0 || n_non <= A.max_n);
            if (A.strand_mask & 1) aff_term(counted, fwd, A.scale, peak, S, n);      // '+' then '-'
            if (A.strand_mask & 2) aff_term(counted, rev, A.scale, peak, S, n);
        }
        aff_wave(A.scale, peak, S, n);
        if (lane == 0) {
            if (whole) put_cell(A, (int64_t) m * A.R + r, peak, S, n);
            else {
                AffPart p;
                p.peak = peak; p.sum = S; p.n = n; p.reserved = 0;
                A.part[(int64_t) m * A.n_part + A.part_first[r] + s_in] = p;
            }
        }
    }
}

// grid = (regions of more than one segment, ceil(scored motifs / 4)): a wave folds the partials of one (motif, region), lane l the
// segments l, l + 64, ... in ascending order
__global__ void __launch_bounds__(256) affinity_reduce_kernel(const AffArgs A, const int64_t *__restrict__ long_regions, int32_t k_first, int32_t n_mot) {
    const int32_t k = k_first + (int32_t) blockIdx.y * 4 + (int32_t) (threadIdx.x >> 6);
    if (k >= n_mot) return;
    const int lane = (int) (threadIdx.x & 63u);
    const int32_t m = A.mot[k];
    const int64_t r = long_regions[blockIdx.x];
    const int64_t n_seg = A.seg_first[r + 1] - A.seg_first[r];
    const AffPart *__restrict__ part = A.part + (int64_t) m * A.n_part + A.part_first[r];
    double peak = -std::numeric_limits<double>::infinity(), S = 0.0;
    int32_t n = 0;
    const int64_t trips = (n_seg + 63) / 64;              // (wave-uniform: exp is one call for the wave)
    for (int64_t t = 0; t < trips; t++) {
        const int64_t s = t * 64 + lane;
        const bool in = s < n_seg;
        AffPart p;
        p.peak = peak; p.sum = 0.0; p.n = 0; p.reserved = 0;
        if (in) p = part[s];
        aff_fold(p.peak, p.sum, p.n, A.scale, peak, S, n);
    }
    aff_wave(A.scale, peak, S, n);
    if (lane == 0) put_cell(A, (int64_t) m * A.R + r, peak, S, n);
}

// grid = (ceil(R / 256), motifs that are not scored): their rows hold no term
__global__ void __launch_bounds__(256) affinity_fill_kernel(const AffArgs A, const int32_t *__restrict__ motifs) {
    const int64_t r = (int64_t) blockIdx.x * 256 + threadIdx.x;
    if (r >= A.R) return;
    put_cell(A, (int64_t) motifs[blockIdx.y] * A.R + r, 0.0, 0.0, 0);
}

}  // namespace

}  // namespace ms

using namespace ms;

extern "C" {

int ms_debug_affinity_dims(int32_t out[8]) {
    if (!out) { set_error("NULL output"); return MS_ERR_INVALID; }
    out[0] = kBestSegWindows;
    out[1] = kBestTileMaxW;
    out[2] = kBestTileEntries;
    out[3] = kBestWaves;
    out[4] = kBestStrips;
    out[5] = (int32_t) sizeof(AffPart);
    out[6] = 0;
    out[7] = 0;
    return MS_OK;
}

void ms_affinity_free(ms_affinity *a) {
    dense_release(a);
    delete a;
}

int ms_scan_affinity(const ms_pwmset *pwms_c, const ms_seqset *seqs, int strand_mask, double scale, int32_t max_n, uint32_t flags, ms_affinity **out) {
    if (!out) { set_error("out is NULL"); return MS_ERR_INVALID; }
    *out = nullptr;
    int rc = dense_check(pwms_c, seqs, strand_mask);
    if (rc) return rc;
    if (flags != 0u) { set_error("unknown affinity scan flags 0x%x", flags); return MS_ERR_INVALID; }
    if (!(std::isfinite(scale) && scale > 0.0)) { set_error("scale must be a finite number > 0"); return MS_ERR_INVALID; }
    if (max_n < -1) { set_error("max_n must be >= -1 (-1: every window is a term)"); return MS_ERR_INVALID; }
    ms_pwmset *pwms = const_cast<ms_pwmset *>(pwms_c);
    const int32_t P = pwms->P;
    const int64_t R = seqs->R;
    std::unique_ptr<ms_affinity, void (*)(ms_affinity *)> res(nullptr, ms_affinity_free);      // (in front of the run: freed behind the run's wait for the stream)
    DenseRun run;
    // a motif whose max_raw is <= 0 is walked
    if ((rc = dense_open(&run, kBestGeom, pwms->widths.data(), P, &pwms->mu, seqs, "n_terms is", [&](int32_t m) { return entries_scorable(pwms, m); }))) return rc;
    const DensePlan &plan = run.plan;

    // ---- 28 bytes per cell, 24 per partial: both blocks are allocated before anything is launched, and a failure there is the MS_ERR_NOMEM
    // of the header (the test here only keeps the byte counts below inside size_t)
    if (28.0 * (double) P * (double) R + (double) sizeof(AffPart) * (double) P * (double) plan.n_part >= 0.5 * (double) std::numeric_limits<size_t>::max()) {
        set_error("%d x %lld cells do not fit the device", P, (long long) R);
        return MS_ERR_NOMEM;
    }
    res.reset(new (std::nothrow) ms_affinity());
    if (!res) { set_error("out of host memory"); return MS_ERR_NOMEM; }
    res->device = run.c->device;
    res->P = P;
    res->R = R;
    res->strand_mask = strand_mask;
    res->scale = scale;
    res->max_n = max_n;
    const size_t cells = (size_t) P * (size_t) R, cz = std::max<size_t>(cells, 1);
    Carve rv;
    const auto s_peak = rv.add<double>(cz), s_sum = rv.add<double>(cz), s_log_mean = rv.add<double>(cz);
    const auto s_n_terms = rv.add<int32_t>(cz);
    if ((rc = pool_alloc(run.c, rv.bytes(), &res->block, &res->block_bytes))) return rc;
    res->d_peak = Carve::at(res->block, s_peak);
    res->d_sum = Carve::at(res->block, s_sum);
    res->d_log_mean = Carve::at(res->block, s_log_mean);
    res->d_n_terms = Carve::at(res->block, s_n_terms);
    if (cells == 0) { *out = res.release(); return MS_OK; }

    const auto s_part = run.cv.add<AffPart>((size_t) P * (size_t) plan.n_part);
    if ((rc = dense_start(&run, pwms, seqs, reinterpret_cast<const void *>(affinity_kernel<true>)))) return rc;

    const DenseDev &d = run.d;
    AffArgs A;
    A.codes = seqs->d_codes; A.nmask = seqs->d_nmask; A.offsets = seqs->d_offsets; A.R = R;
    A.seg_first = d.seg_first; A.part_first = d.part_first;
    A.n_seg = plan.n_seg; A.n_part = plan.n_part;
    A.tile_first = d.tile_first; A.mot = d.mot;
    A.Pw = dev_pwm(pwms);
    A.strand_mask = strand_mask;
    A.max_n = max_n;
    A.scale = scale;
    A.peak = res->d_peak; A.sum = res->d_sum; A.log_mean = res->d_log_mean; A.n_terms = res->d_n_terms;
    A.part = Carve::at(run.work.p, s_part);
    AffArgs Aw = A;                                      // the wide motifs: one "tile" each
    Aw.tile_first = d.wide_first;

    const hipStream_t st = run.st;
    const int64_t n_mot = (int64_t) plan.mot.size();
    (void) hipEventRecord(run.c->ev[0], st);
    rc = dense_chunks((int64_t) plan.tile_first.size() - 1, "affinity kernel", [&](int64_t t0, unsigned ny) {
        hipLaunchKernelGGL(affinity_kernel<true>, dim3(run.gx, ny), dim3(kBestThreads), run.lds, st, A, (int32_t) t0);
    });
    if (!rc) rc = dense_chunks((int64_t) plan.wide_first.size() - 1, "affinity kernel (tables in HBM)", [&](int64_t t0, unsigned ny) {
        hipLaunchKernelGGL(affinity_kernel<false>, dim3(run.gx, ny), dim3(kBestThreads), 0, st, Aw, (int32_t) t0);
    });
    if (!rc && !plan.long_regions.empty()) rc = dense_chunks((n_mot + 3) / 4, "affinity reduction", [&](int64_t g0, unsigned ny) {       // four motifs a block
        hipLaunchKernelGGL(affinity_reduce_kernel, dim3((unsigned) plan.long_regions.size(), ny), dim3(256), 0, st, A, d.long_regions, (int32_t) (4 * g0), (int32_t) n_mot);
    });
    if (!rc) rc = dense_chunks((int64_t) plan.skipped.size(), "affinity fill", [&](int64_t u0, unsigned ny) {
        hipLaunchKernelGGL(affinity_fill_kernel, dim3((unsigned) ((R + 255) / 256), ny), dim3(256), 0, st, A, d.skipped + u0);
    });
    if (!rc) rc = dense_end(&run, "affinity scan", res.get());
    if (rc) return rc;
    *out = res.release();
    return MS_OK;
}

int ms_affinity_shape(const ms_affinity *a, int32_t *n_pwms, int64_t *n_seqs) { return dense_shape(a, n_pwms, n_seqs); }
int ms_affinity_device_ms(const ms_affinity *a, double *ms) { return dense_device_ms(a, ms); }

int ms_affinity_cells(const ms_affinity *a, int32_t m0, int32_t m1, double *peak, double *sum, int32_t *n_terms, double *log_mean) {
    size_t at = 0, n = 0;
    if (int rc = dense_rows(a, m0, m1, &at, &n)) return rc;
    if (peak && n) MS_HIP(hipMemcpy(peak, a->d_peak + at, 8 * n, hipMemcpyDeviceToHost));
    if (sum && n) MS_HIP(hipMemcpy(sum, a->d_sum + at, 8 * n, hipMemcpyDeviceToHost));
    if (n_terms && n) MS_HIP(hipMemcpy(n_terms, a->d_n_terms + at, 4 * n, hipMemcpyDeviceToHost));
    if (log_mean && n) MS_HIP(hipMemcpy(log_mean, a->d_log_mean + at, 8 * n, hipMemcpyDeviceToHost));
    return MS_OK;
}

int ms_affinity_cells_device(const ms_affinity *a, void **d_peak, void **d_sum, void **d_n_terms, void **d_log_mean) {
    if (!a) { set_error("NULL argument"); return MS_ERR_INVALID; }
    if (d_peak) *d_peak = a->d_peak;
    if (d_sum) *d_sum = a->d_sum;
    if (d_n_terms) *d_n_terms = a->d_n_terms;
    if (d_log_mean) *d_log_mean = a->d_log_mean;
    return MS_OK;
}

int ms_affinity_rank_sum(const ms_affinity *a, const uint8_t *sel_a, const ms_affinity *b, const uint8_t *sel_b, int32_t m0, int32_t m1, uint32_t flags, int64_t *u2,
                         uint64_t *ties, int64_t *n, double *device_ms) {
    if (!require_device()) return MS_ERR_RUNTIME;
    if (!a || !b) { set_error("NULL handle"); return MS_ERR_INVALID; }
    const RankPlane pa = {a->device, a->P, a->R, a->d_log_mean}, pb = {b->device, b->P, b->R, b->d_log_mean};
    return rank_sum_planes("affinity", pa, sel_a, pb, sel_b, m0, m1, flags, u2, ties, n, device_ms);
}

}  // extern "C"
