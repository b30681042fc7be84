// ms_dimodel.hip -- the best-scoring window of every (first-order model, region) cell (ms_scan_best_dimodels): ms_scan_best's dense
// walk for models whose columns depend on their left neighbour, exact, into the same ms_best handle.
//
// A model of W columns is start[4] and trans[1 .. W - 1][16] (include/motifscan_amd.h has the definition, operation by operation).  The
// forward sum of a window is start[x_0], then trans[c][4 x_{c-1} + x_c] for c = 1 .. W - 1; the reverse sum reads the window on the other
// strand and adds its terms in GENOME order -- trans[W - c][4 (3 - x_c) + (3 - x_{c-1})] at step c, start[3 - x_{W-1}] last -- which is the
// order of the PWM scorer's reverse terms.  So one table entry {forward term, reverse term} per genome step serves both strands
// (di_build_table, ms_dimodel_plan.h): 4 end entries by a base, then 16 per step by the pair.  The pair's index is four consecutive bits
// of the packed code word, x_{c-1} | x_c << 2, and the table is laid out by those bits: the extract costs what the PWM walk's two bits do.
//
// Mapping: ms_scan_best's (ms_best.hip).  A wave owns a segment of kBestSegWindows window starts of a region, a block kBestWaves segments
// and one TILE of consecutive scorable models, staged in LDS with one contiguous copy behind an all-zero entry 0; a lane keeps the code
// and mask words of its kBestStrips window starts in registers and walks the tile's models over them.  A model has 4 (4 W - 3) entries, so
// the host plans with dense_plan and the pseudo-width 4 W - 3; the width cap kDiMaxWidth is the widest model that fits a tile alone, so
// every model is walked from LDS.  A packed word holds 32 bases, that is the pairs of 31 steps: the steps are taken in chunks of 31, chunk
// k from the word that starts at base 31 k of the window (its first base is the previous chunk's last, so the pair across a word edge is
// whole).  Chunk 0 is the register word; a model of more than 32 columns fetches the further words per window.  A step past the chunk's
// end reads entry 0: x + 0.0 == x for every x a sum can hold (a sum that starts at +0.0 never becomes -0.0).
//
// A window that holds a non-ACGT base has no score (one test of the mask word per chunk) and never wins -- unlike the PWM walks, where
// such a base adds +0.0.  The divide, the tie rule, the total-order wave reduction, the partials of long regions and the "no winner"
// triple are ms_scan_best's, argued in ms_best.hip's header; best_kernel itself is not touched.  Only the walk's kernel is here: the host
// driver (DenseRun), the allocation of the ms_best and the kernels that fold the partials and fill the unscorable rows (best_alloc,
// best_tail) are ms_best.hip's, through ms_handles.h.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <memory>
#include <new>
#include <vector>

#include "ms_best_dev.h"
#include "ms_device.h"
#include "ms_dimodel_plan.h"
#include "ms_handles.h"

struct ms_dimodelset {
    int32_t P = 0;
    std::vector<int32_t> widths, pseudo;                 // pseudo[m] = 4 W - 3: what dense_plan tiles by
    std::vector<double> max_raw;
    std::vector<uint8_t> ok;                             // di_scorable
    std::vector<ms::DiEntry> tab;                        // the models' tables one after the other
    std::vector<int64_t> tab_off;                        // [P] in entries
};

namespace ms {

namespace {

static_assert(sizeof(DiEntry) == sizeof(double2), "the host's entry is the device's double2");
constexpr DenseGeom kDiGeom = {kBestSegWindows, kDiTileEntries / 4, kDiTileEntries, true};

struct DiArgs {
    const uint32_t *codes, *nmask;
    const int64_t *offsets;                              // [R + 1]
    int64_t R;
    const int64_t *seg_first;                            // [R + 1]; nullptr: one segment per region
    const int64_t *part_first;                           // [R + 1]; nullptr: no partials
    int64_t n_seg, n_part;
    const int32_t *tile_first;                           // [tiles + 1] into mot
    const int32_t *mot;                                  // the scorable models, tile after tile
    const double2 *tab;                                  // the set's tables
    const int64_t *tab_off;                              // [P]
    const int32_t *width;                                // [P]
    const double *max_raw;                               // [P]
    int strand_mask;
    double *score;                                       // [P][R]
    int32_t *pos;
    int8_t *strand;
    BestPart *part;                                      // [P][n_part]
};

// n <= 31 steps of one chunk: the entries pb + 16 i + (four bits of the pair) of the LDS tile, added in step order; a step from n on adds entry 0
__device__ __forceinline__ void di_steps31(const double2 *__restrict__ lds, uint32_t pb, int n, uint64_t cw, double &fwd, double &rev) {
    for (int c1 = 0; c1 < n; c1 += 8) {
        const uint32_t bits = (uint32_t) (cw >> (2 * c1));                       // (18 bits of it are read: the pairs of eight steps)
        double2 t[8];
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const uint32_t idx = pb + (uint32_t) (c1 + k) * 16u + ((bits >> (2 * k)) & 15u);
            t[k] = lds[c1 + k < n ? idx : 0u];
        }
#pragma unroll
        for (int k = 0; k < 8; k++) { fwd += t[k].x; rev += t[k].y; }
    }
}

// grid = (ceil(segments / kBestWaves), tiles)
__global__ void __launch_bounds__(kBestThreads, 4) dimodel_best_kernel(const DiArgs A, int32_t tile0) {
    extern __shared__ double2 di_lds[];                  // [1 + the tile's entries]
    const int32_t tile = tile0 + (int32_t) blockIdx.y;
    const int32_t k0 = A.tile_first[tile], k1 = A.tile_first[tile + 1];
    const int64_t tab0 = A.tab_off[A.mot[k0]];
    {
        const int32_t ml = A.mot[k1 - 1];
        const int32_t n = (int32_t) (A.tab_off[ml] - tab0) + 4 * (4 * A.width[ml] - 3);
        dense_stage_tile(di_lds, A.tab + tab0, n);
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

    const double ninf = -std::numeric_limits<double>::infinity();
    for (int32_t k = k0; k < k1; k++) {
        const int32_t m = A.mot[k];
        const int W = A.width[m];
        const double max_raw = A.max_raw[m];
        const uint32_t tb = 1u + (uint32_t) (A.tab_off[m] - tab0);
        const int64_t last = L - W;                       // the region's last window start
        const int n0 = W - 1 < 31 ? W - 1 : 31;           // steps of chunk 0
        double best_raw = ninf, best_q = ninf;
        uint64_t best_key = kNoKey;
#pragma unroll 1
        for (int s = 0; s < kBestStrips; s++) {
            if (p0 + s * 64 > last) break;                // (wave-uniform) no window of this strip, or of a later one, fits the region
            const int64_t pos = p0 + s * 64 + lane;
            const bool inside = pos <= last;
            // the strip's words out of the register arrays: a chain of selects on the wave-uniform s (as in ms_best_dev.h)
            uint64_t cws = cw[0];
            uint32_t nws = nw[0];
#pragma unroll
            for (int j = 1; j < kBestStrips; j++) { cws = s == j ? cw[j] : cws; nws = s == j ? nw[j] : nws; }
            uint32_t non = nws & low_mask(n0 + 1);        // the window's non-ACGT bases, chunk by chunk
            double fwd = 0.0, rev = 0.0;
            fwd += di_lds[tb + ((uint32_t) cws & 3u)].x;  // start[x_0]
            di_steps31(di_lds, tb + 4u, n0, cws, fwd, rev);
            uint32_t x_last = (uint32_t) (cws >> (2 * n0)) & 3u;
            for (int c0 = 31; c0 < W - 1; c0 += 31) {     // wider models: the further words are read per model (a lane without a window reads nothing)
                const int n = (W - 1 - c0) < 31 ? (W - 1 - c0) : 31;
                const uint64_t cwx = inside ? code_window(A.codes, beg + pos + c0) : 0ULL;
                const uint32_t nwx = inside ? n_window(A.nmask, beg + pos + c0) : ~0u;
                non |= nwx & low_mask(n + 1);
                di_steps31(di_lds, tb + 4u + (uint32_t) c0 * 16u, n, cwx, fwd, rev);
                x_last = (uint32_t) (cwx >> (2 * n)) & 3u;
            }
            rev += di_lds[tb + x_last].y;                 // start[3 - x_{W-1}], last
            const bool valid = inside && non == 0u;
            // '+' then '-': the divide only where the raw sum improves (ms_best.hip's header: exact, quotient collisions included)
            if (valid && (A.strand_mask & 1) && fwd > best_raw) {
                best_raw = fwd;
                const double q = fwd / max_raw;
                if (q > best_q) { best_q = q; best_key = ((uint64_t) pos << 2) | 1u; }
            }
            if (valid && (A.strand_mask & 2) && rev > best_raw) {
                best_raw = rev;
                const double q = rev / max_raw;
                if (q > best_q) { best_q = q; best_key = ((uint64_t) pos << 2) | 2u; }
            }
        }
        wave_best(best_q, best_key);
        if (lane == 0) {
            if (whole) put_best(A.score, A.pos, A.strand, (int64_t) m * A.R + r, best_q, best_key);
            else {
                BestPart p;
                p.q = best_q;
                p.pos = best_key != kNoKey ? (int32_t) (best_key >> 2) : -1;
                p.strand = best_key != kNoKey ? (int32_t) (best_key & 3u) : 0;
                A.part[(int64_t) m * A.n_part + A.part_first[r] + s_in] = p;
            }
        }
    }
}

}  // namespace

}  // namespace ms

using namespace ms;

extern "C" {

int ms_debug_dimodel_dims(int32_t out[8]) {
    if (!out) { set_error("NULL output"); return MS_ERR_INVALID; }
    out[0] = kBestThreads;
    out[1] = kBestSegWindows;
    out[2] = kDiTileEntries;
    out[3] = kDiMaxWidth;
    out[4] = kBestStrips;
    out[5] = 31;                                         // steps per packed word: a model of more than out[5] + 1 columns reads further words
    out[6] = out[7] = 0;
    return MS_OK;
}

int ms_dimodelset_create(const double *values, const int32_t *widths, int32_t n_models, ms_dimodelset **out) {
    if (!out) { set_error("out is NULL"); return MS_ERR_INVALID; }
    *out = nullptr;
    int32_t bad = -1;
    switch (di_validate(values, widths, n_models, &bad)) {
    case kDiOk: break;
    case kDiNull: set_error("values / widths is NULL"); return MS_ERR_INVALID;
    case kDiCount: set_error("n_models must be >= 0, got %d", n_models); return MS_ERR_INVALID;
    case kDiWidth: set_error("model %d has width %d (need >= 1 column)", bad, widths[bad]); return MS_ERR_INVALID;
    case kDiTooWide: set_error("model %d has width %d: a first-order model has at most %d columns", bad, widths[bad], kDiMaxWidth); return MS_ERR_INVALID;
    }
    std::unique_ptr<ms_dimodelset> p(new (std::nothrow) ms_dimodelset());
    if (!p) { set_error("out of host memory"); return MS_ERR_NOMEM; }
    p->P = n_models;
    try {
        p->widths.assign(widths, widths + n_models);
        p->pseudo.resize((size_t) n_models);
        p->max_raw.resize((size_t) n_models);
        p->ok.resize((size_t) n_models);
        p->tab_off.resize((size_t) n_models);
        int64_t entries = 0;
        for (int32_t m = 0; m < n_models; m++) { p->tab_off[(size_t) m] = entries; entries += di_entries(widths[m]); }
        p->tab.resize((size_t) entries);
    } catch (const std::bad_alloc &) { set_error("out of host memory"); return MS_ERR_NOMEM; }
    const double *v = values;
    for (int32_t m = 0; m < n_models; m++) {
        const int32_t W = widths[m];
        p->pseudo[(size_t) m] = di_pseudo_width(W);
        p->max_raw[(size_t) m] = di_max_raw(v, W);
        p->ok[(size_t) m] = di_scorable(v, W, p->max_raw[(size_t) m]) ? 1 : 0;
        di_build_table(v, W, p->tab.data() + p->tab_off[(size_t) m]);
        v += (size_t) W * 16;
    }
    *out = p.release();
    return MS_OK;
}

int ms_dimodelset_size(const ms_dimodelset *p, int32_t *n_models) {
    if (!p || !n_models) { set_error("NULL argument"); return MS_ERR_INVALID; }
    *n_models = p->P;
    return MS_OK;
}

int ms_dimodelset_max_raw(const ms_dimodelset *p, double *out) {
    if (!p || (!out && p->P > 0)) { set_error("NULL argument"); return MS_ERR_INVALID; }
    if (p->P > 0) std::memcpy(out, p->max_raw.data(), (size_t) p->P * sizeof(double));
    return MS_OK;
}

void ms_dimodelset_free(ms_dimodelset *p) { delete p; }

int ms_scan_best_dimodels(const ms_dimodelset *models, const ms_seqset *seqs, int strand_mask, uint32_t flags, ms_best **out) {
    if (!out) { set_error("out is NULL"); return MS_ERR_INVALID; }
    *out = nullptr;
    int rc = dense_check(models, seqs, strand_mask);
    if (rc) return rc;
    if (flags != 0u) { set_error("unknown first-order best-site scan flags 0x%x", flags); return MS_ERR_INVALID; }
    const int32_t P = models->P;
    const int64_t R = seqs->R;
    BestPtr res(nullptr, ms_best_free);                  // (in front of the run: freed behind the run's wait for the stream)
    DenseRun run;
    // the tiles of the models go by their pseudo-widths (ms_dense_plan.h)
    if ((rc = dense_open(&run, kDiGeom, models->pseudo.data(), P, nullptr, seqs, "positions are", [&](int32_t m) { return models->ok[(size_t) m] != 0; }))) return rc;
    if ((rc = best_alloc(run, P, R, &res))) return rc;
    if (P == 0 || R == 0) { *out = res.release(); return MS_OK; }
    const DensePlan &plan = run.plan;

    // ---- the work block: the plan, the set's tables and per-model arrays (a model set keeps no device copy: a few KB per model, uploaded
    // per call in front of the timed launches), the partials
    Carve &cv = run.cv;
    const auto s_tab = cv.add<double2>(models->tab.size());
    const auto s_tab_off = cv.add<int64_t>((size_t) P);
    const auto s_width = cv.add<int32_t>((size_t) P);
    const auto s_max_raw = cv.add<double>((size_t) P);
    const auto s_part = cv.add<BestPart>((size_t) P * (size_t) plan.n_part);
    if ((rc = dense_start(&run, nullptr, seqs, reinterpret_cast<const void *>(dimodel_best_kernel)))) return rc;
    const hipStream_t st = run.st;
    hipError_t he = hipSuccess;
    auto up = [&](const auto &v, auto slot) {
        auto *p = Carve::at(run.work.p, slot);
        if (he == hipSuccess) he = hipMemcpyAsync(p, v.data(), sizeof(v[0]) * v.size(), hipMemcpyHostToDevice, st);
        return p;
    };
    const DenseDev &d = run.d;
    DiArgs A;
    A.tab = reinterpret_cast<const double2 *>(up(models->tab, s_tab));
    A.tab_off = up(models->tab_off, s_tab_off);
    A.width = up(models->widths, s_width);
    A.max_raw = up(models->max_raw, s_max_raw);
    if (he != hipSuccess) return hip_rc(he, "upload of the models");
    A.codes = seqs->d_codes; A.nmask = seqs->d_nmask; A.offsets = seqs->d_offsets; A.R = R;
    A.seg_first = d.seg_first; A.part_first = d.part_first;
    A.n_seg = plan.n_seg; A.n_part = plan.n_part;
    A.tile_first = d.tile_first; A.mot = d.mot;
    A.strand_mask = strand_mask;
    A.score = res->d_score; A.pos = res->d_pos; A.strand = res->d_strand;
    A.part = Carve::at(run.work.p, s_part);

    (void) hipEventRecord(run.c->ev[0], st);
    rc = dense_chunks((int64_t) plan.tile_first.size() - 1, "first-order best-site kernel", [&](int64_t t0, unsigned ny) {
        hipLaunchKernelGGL(dimodel_best_kernel, dim3(run.gx, ny), dim3(kBestThreads), run.lds, st, A, (int32_t) t0);
    });
    if (!rc) rc = best_tail(run, "first-order best-site", A.part, res.get());
    if (!rc) rc = dense_end(&run, "first-order best-site scan", res.get());
    if (rc) return rc;
    *out = res.release();
    return MS_OK;
}

}  // extern "C"
