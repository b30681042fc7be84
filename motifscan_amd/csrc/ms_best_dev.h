// ms_best_dev.h -- the DEVICE helpers of the kernels that score every window of a cell, and the test for a motif the reference never
// reports a site of (scorable).  With ms_allelebest.hip (per variant haplotype) ms_best.hip shares the total-order wave reduction; the
// five dense walks (best_kernel, affinity_kernel, scorehist_kernel, expcounts_kernel of ms_expcounts.hip: the affinity walk taken a
// second time, and dimodel_best_kernel of ms_dimodel.hip: the best-site walk over first-order models) share the walk's kBest* sizes and
// the walk's steps as functions -- the staging of a tile, a segment's words into registers and, for the PWM walks, the column loop over
// an LDS tile of tables and the raw sums of one strip of window starts.  The two best-site walks also share what a cell ends in: a
// segment's partial (BestPart) and the write of a cell (put_best); the kernels behind them that fold the partials of long regions and
// fill the rows that are not scored are compiled once, in ms_best.hip (best_tail, ms_handles.h).
// best_kernel keeps the three steps written out in its own body: called through the functions, hipcc schedules its
// LDS form differently (its disassembly changes), and that kernel's code is to stay as measured.  A change to a step is made in both
// places -- the functions here, which affinity_kernel, scorehist_kernel and expcounts_kernel call, and best_kernel's body.
// The HOST side of the walks is not here: the plan (DenseGeom, dense_plan) and its layout in a work block are ms_dense_plan.h,
// plain C++; the driver of the three matrix walks (DenseRun), the owner of a work block (WorkBlock), the plan's upload, the chunked
// launches, the LDS limit and the head of the two result handles (DenseHead) are declared in ms_handles.h and implemented once, in
// ms_best.hip.
#pragma once
#include <algorithm>
#include <cmath>
#include <limits>

#include "ms_device.h"
#include "ms_handles.h"

namespace ms {

struct BestPart {                                        // a segment's best of one motif or model (declared in ms_handles.h)
    double q;
    int32_t pos;                                         // -1: no winner
    int32_t strand;
};

namespace {

constexpr uint64_t kNoKey = ~0ULL;

// the dense walk (best_kernel, affinity_kernel): a wave per segment of a region, a block per tile of motifs
constexpr int kBestThreads = 512;
constexpr int kBestWaves = kBestThreads / 64;            // segments per block
constexpr int kBestStrips = 8;                           // strips of 64 window starts whose words a lane keeps in registers
constexpr int kBestSegWindows = 64 * kBestStrips;
constexpr int kBestTileMaxW = 1024;                      // (= kExactTileMaxW, ms_fp64.hip) widest motif whose table fits a tile
constexpr int kBestTileEntries = kBestTileMaxW * 4;      // 64 KB of tab2 entries per tile (+ the zero entry): two blocks share a CU's 160 KB
constexpr DenseGeom kBestGeom = {kBestSegWindows, kBestTileMaxW, kBestTileEntries, true};      // what the host plans with: partials for long regions

// (q, key) of the wave's lanes -> the winner in every lane: the greater q, equal q to the smaller key = pos << 2 | strand
__device__ __forceinline__ void wave_best(double &q, uint64_t &key) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const double oq = __shfl_xor(q, d);
        const unsigned long long ok = __shfl_xor((unsigned long long) key, d);
        if (oq > q || (oq == q && ok < key)) { q = oq; key = ok; }
    }
}

// a cell of the three best-site planes: the winner (q, key = pos << 2 | strand), or the "no winner" triple for kNoKey
__device__ __forceinline__ void put_best(double *__restrict__ score, int32_t *__restrict__ pos, int8_t *__restrict__ strand, int64_t cell, double q, uint64_t key) {
    const bool won = key != kNoKey;
    score[cell] = won ? q : __builtin_nan("");
    pos[cell] = won ? (int32_t) (key >> 2) : -1;
    strand[cell] = won ? (int8_t) (key & 3u) : (int8_t) 0;
}

// (the dense walks over an LDS tile of tables: best_kernel, scorehist_kernel) up to 32 columns out of the registers: table entries tb + 4 c of the LDS tile, in column order; bit c of skip: the column adds entry 0
__device__ __forceinline__ void best_cols32(const double2 *__restrict__ lds, uint32_t tb, int n, uint64_t cw, uint32_t skip, double &fwd, double &rev) {
    for (int c1 = 0; c1 < n; c1 += 8) {
        const uint32_t bits = (uint32_t) (cw >> (2 * c1)), sk = skip >> c1;
        double2 t[8];
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const uint32_t idx = tb + (uint32_t) (c1 + k) * 4u + ((bits >> (2 * k)) & 3u);
            t[k] = lds[((sk >> k) & 1u) ? 0u : idx];
        }
#pragma unroll
        for (int k = 0; k < 8; k++) { fwd += t[k].x; rev += t[k].y; }
    }
}

// the tile's tables into LDS with one contiguous copy behind an all-zero entry 0 (n entries from src), the block's barrier included
__device__ __forceinline__ void dense_stage_tile(double2 *__restrict__ lds, const double2 *__restrict__ src, int32_t n) {
    if (threadIdx.x == 0) lds[0] = make_double2(0.0, 0.0);
    for (int32_t i = threadIdx.x; i < n; i += kBestThreads) lds[1 + i] = src[i];
    __syncthreads();
}

// the code / mask words of the lane's kBestStrips window starts p0 + 64 s + lane of the region [beg, beg + L), read once
__device__ __forceinline__ void dense_segment_words(const uint32_t *__restrict__ codes, const uint32_t *__restrict__ nmask, int64_t beg, int64_t L, int64_t p0, int lane,
                                                    uint64_t (&cw)[kBestStrips], uint32_t (&nw)[kBestStrips]) {
#pragma unroll
    for (int s = 0; s < kBestStrips; s++) {
        const int64_t pos = p0 + s * 64 + lane;
        const bool in = pos < L;                          // (a lane past the region reads nothing: the padding behind the planes is short)
        cw[s] = in ? code_window(codes, beg + pos) : 0ULL;
        nw[s] = in ? n_window(nmask, beg + pos) : ~0u;
    }
}

// The raw sums of the window that starts at base g (= beg + pos; valid: it lies inside its region) for strip s of the segment's words.
// LDS: the motif's table at entry tb of the tile; !LDS: in HBM at tab.  COUNT_N: n_non = the window's non-ACGT bases (the mask bits of
// its own W bases: from the register for the first 32 columns, from the further words a wider motif loads anyway).
template <bool LDS, bool COUNT_N>
__device__ __forceinline__ void dense_strip_sums(const double2 *__restrict__ lds, uint32_t tb, const double2 *__restrict__ tab, const uint32_t *__restrict__ codes,
                                                 const uint32_t *__restrict__ nmask, int W, int64_t g, bool valid, int s, const uint64_t (&cw)[kBestStrips],
                                                 const uint32_t (&nw)[kBestStrips], double &fwd, double &rev, int &n_non) {
    if (LDS) {
        // the strip's words out of the register arrays: a chain of selects on the wave-uniform s (the loop is NOT unrolled: eight
        // copies of the column loops spill; indexing the arrays with s would put them into scratch)
        uint64_t cws = cw[0];
        uint32_t nws = nw[0];
#pragma unroll
        for (int j = 1; j < kBestStrips; j++) { cws = s == j ? cw[j] : cws; nws = s == j ? nw[j] : nws; }
        const int n0 = W < 32 ? W : 32;
        best_cols32(lds, tb, n0, cws, nws | ~low_mask(n0), fwd, rev);
        if (COUNT_N) n_non = __popc(nws & low_mask(n0));
        for (int c0 = 32; c0 < W; c0 += 32) {             // wider motifs: the further words are read per motif (a lane without a window reads nothing)
            const int n = (W - c0) < 32 ? (W - c0) : 32;
            const uint64_t cwx = valid ? code_window(codes, g + c0) : 0ULL;
            const uint32_t nwx = valid ? n_window(nmask, g + c0) : ~0u;
            best_cols32(lds, tb + (uint32_t) c0 * 4u, n, cwx, nwx | ~low_mask(n), fwd, rev);
            if (COUNT_N) n_non += __popc(nwx & low_mask(n));
        }
    } else if (valid) {
        DevSeq S;
        S.codes = codes; S.nmask = nmask;
        score_window(S, tab, W, g, fwd, rev);
        if (COUNT_N)
            for (int c0 = 0; c0 < W; c0 += 32) n_non += __popc(n_window(nmask, g + c0) & low_mask((W - c0) < 32 ? (W - c0) : 32));
    }
}

// no entry of the motif is NaN or +inf (ms_scan_affinity scores every such motif; one that fails has an empty row)
inline bool entries_scorable(const ms_pwmset *p, int32_t m) {
    const double *v = p->values.data() + p->val_off[(size_t) m];
    const int64_t n = 4 * (int64_t) p->widths[(size_t) m];
    for (int64_t i = 0; i < n; i++)
        if (std::isnan(v[i]) || v[i] == std::numeric_limits<double>::infinity()) return false;
    return true;
}

// the reference never reports a site of a motif that fails this: max_raw is not a finite number > 0, or an entry is NaN or +inf
inline bool scorable(const ms_pwmset *p, int32_t m) {
    const double mr = p->max_raw[(size_t) m];
    return std::isfinite(mr) && mr > 0.0 && entries_scorable(p, m);
}

}  // namespace

}  // namespace ms
