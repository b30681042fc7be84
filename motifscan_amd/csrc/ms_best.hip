// ms_best.hip -- the best-scoring window of every (motif, region) cell (ms_scan_best): the dense motif x region matrix, exact.
//
// For motif m of width W and region r of length L the windows pos = 0 .. L - W are walked in the reference's order (pos ascending, '+'
// before '-'), each scored as ms_scan scores it (cscore.c:336-390; the scorer of ms_fp64.hip: columns 0 .. W - 1, forward M[b][c], reverse
// M[3 - b][W - 1 - c] at the same step, +0.0 for a base that adds nothing, raw / max_raw), and a window replaces the best iff its score is
// GREATER: NaN and -inf never win, ties keep the earlier window.  Nothing is emitted and nothing is sorted: 13 bytes leave per cell.
//
// Mapping.  A region is cut into SEGMENTS of kBestSegWindows window starts; a wave owns one segment, a block kBestWaves of them and one
// TILE of motifs: consecutive scorable motifs whose tab2 entries are consecutive in HBM and fit 64 KB, staged in LDS with ONE contiguous
// copy behind an all-zero entry 0 (exact_tiled_kernel's trick: a column that adds nothing ADDS +0.0).  A lane reads the code / mask words
// of its kBestStrips window starts ONCE, keeps them in registers, and walks the tile's motifs over them: the sequence reads and the
// region look-up are shared by the whole tile, a column is one 16-byte LDS read (<= 5 distinct addresses per wave) and two fp64 adds.
//
// The divide.  Per lane and motif the state is (best_raw, best_q, pos, strand).  The IEEE divide is paid only by a window whose raw sum is
// strictly GREATER than best_raw: with max_raw > 0 a correctly rounded divide is monotone, so raw <= best_raw gives q <= best_q, and such a
// window comes later in the walk -- it can never replace the best.  After a divide the window wins iff q > best_q (best_raw moves up either
// way: a later window that does not beat the NEW raw sum cannot beat a quotient that is >= its own).  This is exact under the semantics
// above, two different raw sums whose quotients round to the same double included: the earlier one keeps the cell.
//
// Order without an atomic: a lane's windows ascend; at the end of a motif the wave is reduced with a total order -- the greater q wins, equal
// q goes to the smaller (pos, strand) -- so the bytes are the same on every run.  A region of one segment writes its cell; a longer one writes
// a partial per segment, and best_reduce_kernel folds them in segment order by the same rule.
// Motifs wider than kBestTileMaxW read their table from HBM (score_window); unscorable motifs (max_raw not a finite number > 0, a NaN or
// +inf entry: the reference never reports a site for them) are filled with the "no winner" triple and never scored.
//
// Behind ms_scan_best this file also holds the host side that the five dense walks share (declared in ms_handles.h; ms_affinity.hip,
// ms_scorehist.hip, ms_expcounts.hip and ms_dimodel.hip call it): a plan's upload, the LDS limit, the accessors of a DenseHead, the
// driver of the three walks that fill a matrix (dense_check, dense_open, dense_start, dense_end), and the tail of the two best-site
// walks -- the allocation of an ms_best and the reduce and fill kernels, which ms_scan_best_dimodels ends in as well.
#include <algorithm>
#include <cmath>
#include <limits>
#include <memory>

#include "ms_best_dev.h"
#include "ms_device.h"
#include "ms_handles.h"

namespace ms {

namespace {

// (the sizes of the walk -- kBestThreads ... kBestTileEntries --, BestPart and put_best are in ms_best_dev.h: the other walks use them)
struct BestArgs {
    const uint32_t *codes, *nmask;
    const int64_t *offsets;                              // [R + 1]
    int64_t R;
    const int64_t *seg_first;                            // [R + 1] first segment of the region (every region has at least one); nullptr: one segment per region
    const int64_t *part_first;                           // [R + 1] first partial of the region (regions of one segment have none); nullptr: no partials
    int64_t n_seg, n_part;
    const int32_t *tile_first;                           // [tiles + 1] into mot
    const int32_t *mot;                                  // the scorable motifs, tile after tile
    DevPwm Pw;
    int strand_mask;
    double *score;                                       // [P][R]
    int32_t *pos;
    int8_t *strand;
    BestPart *part;                                      // [P][n_part]
};

struct BestTail {                                        // what the reduce and fill kernels read, whichever walk wrote the partials
    const int64_t *seg_first, *part_first;               // [R + 1]
    int64_t n_part;
    const int32_t *mot;                                  // the scorable motifs (or models)
    int64_t R;
    double *score;                                       // [P][R]
    int32_t *pos;
    int8_t *strand;
    const BestPart *part;                                // [P][n_part]
};

// grid = (ceil(segments / kBestWaves), tiles).  LDS: the tile's tables in LDS; !LDS: one motif per tile, its table in HBM.
template <bool LDS>
__global__ void __launch_bounds__(kBestThreads, 4) best_kernel(const BestArgs A, int32_t tile0) {
    extern __shared__ double2 best_lds[];                // [1 + the tile's entries]
    const int32_t tile = tile0 + (int32_t) blockIdx.y;
    const int32_t k0 = A.tile_first[tile], k1 = A.tile_first[tile + 1];
    const int64_t tab0 = A.Pw.tab_off[A.mot[k0]];
    if (LDS) {
        const int32_t ml = A.mot[k1 - 1];
        const int32_t n = (int32_t) (A.Pw.tab_off[ml] - tab0) + A.Pw.width[ml] * 4;
        const double2 *__restrict__ src = A.Pw.tab2 + tab0;
        if (threadIdx.x == 0) best_lds[0] = make_double2(0.0, 0.0);
        for (int32_t i = threadIdx.x; i < n; i += kBestThreads) best_lds[1 + i] = src[i];
        __syncthreads();
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
#pragma unroll
    for (int s = 0; s < kBestStrips; s++) {
        const int64_t pos = p0 + s * 64 + lane;
        const bool in = pos < L;                          // (a lane past the region reads nothing: the padding behind the planes is short)
        cw[s] = in ? code_window(A.codes, beg + pos) : 0ULL;
        nw[s] = in ? n_window(A.nmask, beg + pos) : ~0u;
    }

    const double ninf = -std::numeric_limits<double>::infinity();
    for (int32_t k = k0; k < k1; k++) {
        const int32_t m = A.mot[k];
        const int W = A.Pw.width[m];
        const double max_raw = A.Pw.max_raw[m];
        const int64_t tab_m = A.Pw.tab_off[m];
        const uint32_t tb = 1u + (uint32_t) (tab_m - tab0);
        const int64_t last = L - W;                       // the region's last window start
        double best_raw = ninf, best_q = ninf;
        uint64_t best_key = kNoKey;
#pragma unroll 1
        for (int s = 0; s < kBestStrips; s++) {
            if (p0 + s * 64 > last) break;                // (wave-uniform) no window of this strip, or of a later one, fits the region
            const int64_t pos = p0 + s * 64 + lane;
            const bool valid = pos <= last;
            double fwd = 0.0, rev = 0.0;
            if (LDS) {
                // the strip's words out of the register arrays: a chain of selects on the wave-uniform s (the loop is NOT unrolled: eight
                // copies of the column loops spill; indexing the arrays with s would put them into scratch)
                uint64_t cws = cw[0];
                uint32_t nws = nw[0];
#pragma unroll
                for (int j = 1; j < kBestStrips; j++) { cws = s == j ? cw[j] : cws; nws = s == j ? nw[j] : nws; }
                const int n0 = W < 32 ? W : 32;
                best_cols32(best_lds, tb, n0, cws, nws | ~low_mask(n0), fwd, rev);
                for (int c0 = 32; c0 < W; c0 += 32) {     // wider motifs: the further words are read per motif (a lane without a window reads nothing)
                    const int n = (W - c0) < 32 ? (W - c0) : 32;
                    const uint64_t cwx = valid ? code_window(A.codes, beg + pos + c0) : 0ULL;
                    const uint32_t nwx = valid ? n_window(A.nmask, beg + pos + c0) : ~0u;
                    best_cols32(best_lds, tb + (uint32_t) c0 * 4u, n, cwx, nwx | ~low_mask(n), fwd, rev);
                }
            } else if (valid) {
                DevSeq S;
                S.codes = A.codes; S.nmask = A.nmask;
                score_window(S, A.Pw.tab2 + tab_m, W, beg + pos, fwd, rev);
            }
            // '+' then '-': the divide only where the raw sum improves (the header comment: exact, quotient collisions included)
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

// grid = (regions of more than one segment, ceil(scorable motifs / 4)): a wave folds the partials of one (motif, region) in segment order
__global__ void __launch_bounds__(256) best_reduce_kernel(const BestTail A, const int64_t *__restrict__ long_regions, int32_t k_first, int32_t n_mot) {
    const int32_t k = k_first + (int32_t) blockIdx.y * 4 + (int32_t) (threadIdx.x >> 6);
    if (k >= n_mot) return;
    const int lane = (int) (threadIdx.x & 63u);
    const int32_t m = A.mot[k];
    const int64_t r = long_regions[blockIdx.x];
    const int64_t n = A.seg_first[r + 1] - A.seg_first[r];
    const BestPart *__restrict__ part = A.part + (int64_t) m * A.n_part + A.part_first[r];
    double best_q = -std::numeric_limits<double>::infinity();
    uint64_t best_key = kNoKey;
    for (int64_t s = lane; s < n; s += 64) {              // ascending: an equal q keeps the earlier segment
        const BestPart p = part[s];
        if (p.pos >= 0 && p.q > best_q) { best_q = p.q; best_key = ((uint64_t) (uint32_t) p.pos << 2) | (uint32_t) p.strand; }
    }
    wave_best(best_q, best_key);
    if (lane == 0) put_best(A.score, A.pos, A.strand, (int64_t) m * A.R + r, best_q, best_key);
}

// grid = (ceil(R / 256), unscorable motifs): their rows hold no winner
__global__ void __launch_bounds__(256) best_fill_kernel(const BestTail A, const int32_t *__restrict__ motifs) {
    const int64_t r = (int64_t) blockIdx.x * 256 + threadIdx.x;
    if (r >= A.R) return;
    put_best(A.score, A.pos, A.strand, (int64_t) motifs[blockIdx.y] * A.R + r, 0.0, kNoKey);
}

}  // namespace

// ---- the host side of the dense walks (ms_handles.h)

int dense_regions_fit(const ms_seqset *seqs, const char *what) {
    const int64_t *off = seqs->offsets.data();
    for (int64_t r = 0; r < seqs->R; r++)
        if (off[r + 1] - off[r] >= (1LL << 31)) {
            set_error("region %lld has %lld bases: %s 32-bit, cut it into regions of fewer than 2^31", (long long) r, (long long) (off[r + 1] - off[r]), what);
            return MS_ERR_INVALID;
        }
    return MS_OK;
}

int dense_upload(const DensePlan &pl, const DenseSlots &s, void *work, hipStream_t st, DenseDev *d) {
    hipError_t he = hipSuccess;
    auto up = [&](const auto &v, auto slot) -> decltype(v.data()) {
        if (v.empty()) return nullptr;
        auto *p = Carve::at(work, slot);
        if (he == hipSuccess) he = hipMemcpyAsync(p, v.data(), sizeof(v[0]) * v.size(), hipMemcpyHostToDevice, st);
        return p;
    };
    d->seg_first = up(pl.seg_first, s.seg_first);
    d->part_first = up(pl.part_first, s.part_first);
    d->long_regions = up(pl.long_regions, s.long_regions);
    d->mot = up(pl.mot, s.mot);
    d->tile_first = up(pl.tile_first, s.tile_first);
    d->wide_first = up(pl.wide_first, s.wide_first);
    d->skipped = up(pl.skipped, s.skipped);
    return he == hipSuccess ? MS_OK : hip_rc(he, "upload of the plan");
}

int dense_raise_lds(DeviceCtx *c, const void *kernel, size_t need, size_t most) {
    if (need <= 48 * 1024 || std::find(c->lds_raised.begin(), c->lds_raised.end(), kernel) != c->lds_raised.end()) return MS_OK;
    const hipError_t he = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int) most);
    if (he != hipSuccess) return hip_rc(he, "raising the LDS limit");
    c->lds_raised.push_back(kernel);
    return MS_OK;
}

int dense_check(const void *set, const ms_seqset *seqs, int strand_mask) {
    if (!require_device()) return MS_ERR_RUNTIME;
    if (!set || !seqs) { set_error("NULL handle"); return MS_ERR_INVALID; }
    if (strand_mask < 1 || strand_mask > 3) { set_error("invalid strand mask %d (1 '+', 2 '-', 3 both)", strand_mask); return MS_ERR_INVALID; }
    return MS_OK;
}

int dense_open(DenseRun *run, const DenseGeom &g, const int32_t *widths, int32_t P, std::mutex *set_mu, const ms_seqset *seqs, const char *fit_what,
               const std::function<bool(int32_t)> &walked) {
    int rc = dense_regions_fit(seqs, fit_what);
    if (rc) return rc;
    if ((rc = get_ctx(seqs->device, &run->c))) return rc;
    // ---- the plan, on the host: segments of the regions, tiles of the motifs (ms_dense_plan.h)
    if ((rc = dense_plan_for(g, widths, P, seqs, kBestWaves, walked, &run->plan))) return rc;
    run->gx = (unsigned) ((run->plan.n_seg + kBestWaves - 1) / kBestWaves);
    run->ds = dense_slots(run->cv, run->plan);
    run->lds = (run->plan.max_tile + 1) * sizeof(double2);
    run->lds_most = ((size_t) g.tile_entries + 1) * sizeof(double2);
    DeviceCtx *c = run->c;
    run->lk_dev = std::unique_lock<std::mutex>(c->mu);
    if (set_mu) run->lk_set = std::unique_lock<std::mutex>(*set_mu);
    MS_HIP(hipSetDevice(c->device));
    run->st = c->stream;
    return MS_OK;
}

int dense_start(DenseRun *run, ms_pwmset *pwms, const ms_seqset *seqs, const void *kernel) {
    int rc = run->work.alloc(run->c, run->st, run->cv.bytes());
    if (rc) return rc;
    if (pwms && (rc = pwmset_upload(pwms, run->c->device, run->st))) return rc;
    if ((rc = seqset_pack_pending(seqs, run->st))) return rc;
    if ((rc = dense_raise_lds(run->c, kernel, run->lds, run->lds_most))) return rc;
    return dense_upload(run->plan, run->ds, run->work.p, run->st, &run->d);
}

int dense_end(DenseRun *run, const char *what, DenseHead *h) {
    (void) hipEventRecord(run->c->ev[1], run->st);
    if (const int rc = run->work.wait(what)) return rc;
    float ms01 = 0;
    (void) hipEventElapsedTime(&ms01, run->c->ev[0], run->c->ev[1]);
    h->device_ms = ms01;
    run->work.release();
    return MS_OK;
}

int best_alloc(const DenseRun &run, int32_t P, int64_t R, BestPtr *res, bool gaps) {
    // ---- 13 bytes per cell (15 with the gap plane), 16 per partial (18): both blocks are allocated before anything is launched, and a failure
    // there is the MS_ERR_NOMEM of the header (the test here only keeps the byte counts below inside size_t)
    if ((gaps ? 15.0 : 13.0) * (double) P * (double) R + (gaps ? 18.0 : 16.0) * (double) P * (double) run.plan.n_part >= 0.5 * (double) std::numeric_limits<size_t>::max()) {
        set_error("%d x %lld cells do not fit the device", P, (long long) R);
        return MS_ERR_NOMEM;
    }
    ms_best *b = new (std::nothrow) ms_best();
    if (!b) { set_error("out of host memory"); return MS_ERR_NOMEM; }
    res->reset(b);
    b->device = run.c->device;
    b->P = P;
    b->R = R;
    const size_t cz = std::max<size_t>((size_t) P * (size_t) R, 1);
    Carve rv;
    const auto s_score = rv.add<double>(cz);
    const auto s_pos = rv.add<int32_t>(cz);
    const auto s_strand = rv.add<int8_t>(cz);
    const auto s_gap = rv.add<int16_t>(gaps ? cz : 0);
    if (const int rc = pool_alloc(run.c, rv.bytes(), &b->block, &b->block_bytes)) return rc;
    b->d_score = Carve::at(b->block, s_score);
    b->d_pos = Carve::at(b->block, s_pos);
    b->d_strand = Carve::at(b->block, s_strand);
    if (gaps) b->d_gap = Carve::at(b->block, s_gap);
    return MS_OK;
}

int best_tail(const DenseRun &run, const char *what, const BestPart *part, ms_best *b) {
    const DensePlan &plan = run.plan;
    const int64_t n_mot = (int64_t) plan.mot.size();
    const hipStream_t st = run.st;
    const BestTail A = {run.d.seg_first, run.d.part_first, plan.n_part, run.d.mot, b->R, b->d_score, b->d_pos, b->d_strand, part};
    const std::string reduce = std::string(what) + " reduction", fill = std::string(what) + " fill";
    int rc = MS_OK;
    if (!plan.long_regions.empty()) rc = dense_chunks((n_mot + 3) / 4, reduce.c_str(), [&](int64_t g0, unsigned ny) {                  // four motifs a block
        hipLaunchKernelGGL(best_reduce_kernel, dim3((unsigned) plan.long_regions.size(), ny), dim3(256), 0, st, A, run.d.long_regions, (int32_t) (4 * g0), (int32_t) n_mot);
    });
    if (!rc) rc = dense_chunks((int64_t) plan.skipped.size(), fill.c_str(), [&](int64_t u0, unsigned ny) {
        hipLaunchKernelGGL(best_fill_kernel, dim3((unsigned) ((b->R + 255) / 256), ny), dim3(256), 0, st, A, run.d.skipped + u0);
    });
    return rc;
}

void dense_release(DenseHead *h) {
    if (!h || !h->block) return;
    (void) hipSetDevice(h->device);
    DeviceCtx *c = nullptr;
    if (get_ctx(h->device, &c) == MS_OK) pool_free(c, h->block, h->block_bytes); else (void) hipFree(h->block);
    h->block = nullptr;
}

int dense_shape(const DenseHead *h, int32_t *n_pwms, int64_t *n_seqs) {
    if (!h) { set_error("NULL argument"); return MS_ERR_INVALID; }
    if (n_pwms) *n_pwms = h->P;
    if (n_seqs) *n_seqs = h->R;
    return MS_OK;
}

int dense_device_ms(const DenseHead *h, double *ms) {
    if (!h || !ms) { set_error("NULL argument"); return MS_ERR_INVALID; }
    *ms = h->device_ms;
    return MS_OK;
}

int dense_rows(const DenseHead *h, int32_t m0, int32_t m1, size_t *at, size_t *n) {
    if (!h) { set_error("NULL argument"); return MS_ERR_INVALID; }
    if (m0 < 0 || m1 > h->P || m0 > m1) { set_error("motif range [%d, %d) outside [0, %d)", m0, m1, h->P); return MS_ERR_INVALID; }
    *at = (size_t) m0 * (size_t) h->R;
    *n = (size_t) (m1 - m0) * (size_t) h->R;
    if (*n > 0) MS_HIP(hipSetDevice(h->device));
    return MS_OK;
}

}  // namespace ms

using namespace ms;

extern "C" {

int ms_debug_best_segment_windows(void) { return kBestSegWindows; }

void ms_best_free(ms_best *b) {
    dense_release(b);
    delete b;
}

int ms_scan_best(const ms_pwmset *pwms_c, const ms_seqset *seqs, int strand_mask, uint32_t flags, ms_best **out) {
    if (!out) { set_error("out is NULL"); return MS_ERR_INVALID; }
    *out = nullptr;
    int rc = dense_check(pwms_c, seqs, strand_mask);
    if (rc) return rc;
    if (flags != 0u) { set_error("unknown best-site scan flags 0x%x", flags); return MS_ERR_INVALID; }
    ms_pwmset *pwms = const_cast<ms_pwmset *>(pwms_c);
    const int32_t P = pwms->P;
    const int64_t R = seqs->R;
    BestPtr res(nullptr, ms_best_free);                  // (in front of the run: freed behind the run's wait for the stream)
    DenseRun run;
    if ((rc = dense_open(&run, kBestGeom, pwms->widths.data(), P, &pwms->mu, seqs, "positions are", [&](int32_t m) { return scorable(pwms, m); }))) return rc;
    if ((rc = best_alloc(run, P, R, &res))) return rc;
    if (P == 0 || R == 0) { *out = res.release(); return MS_OK; }
    const auto s_part = run.cv.add<BestPart>((size_t) P * (size_t) run.plan.n_part);
    if ((rc = dense_start(&run, pwms, seqs, reinterpret_cast<const void *>(best_kernel<true>)))) return rc;

    const DensePlan &plan = run.plan;
    const DenseDev &d = run.d;
    BestArgs A;
    A.codes = seqs->d_codes; A.nmask = seqs->d_nmask; A.offsets = seqs->d_offsets; A.R = R;
    A.seg_first = d.seg_first; A.part_first = d.part_first;
    A.n_seg = plan.n_seg; A.n_part = plan.n_part;
    A.tile_first = d.tile_first; A.mot = d.mot;
    A.Pw = dev_pwm(pwms);
    A.strand_mask = strand_mask;
    A.score = res->d_score; A.pos = res->d_pos; A.strand = res->d_strand;
    A.part = Carve::at(run.work.p, s_part);
    BestArgs Aw = A;                                     // the wide motifs: one "tile" each
    Aw.tile_first = d.wide_first;

    const hipStream_t st = run.st;
    (void) hipEventRecord(run.c->ev[0], st);
    rc = dense_chunks((int64_t) plan.tile_first.size() - 1, "best-site kernel", [&](int64_t t0, unsigned ny) {
        hipLaunchKernelGGL(best_kernel<true>, dim3(run.gx, ny), dim3(kBestThreads), run.lds, st, A, (int32_t) t0);
    });
    if (!rc) rc = dense_chunks((int64_t) plan.wide_first.size() - 1, "best-site kernel (tables in HBM)", [&](int64_t t0, unsigned ny) {
        hipLaunchKernelGGL(best_kernel<false>, dim3(run.gx, ny), dim3(kBestThreads), 0, st, Aw, (int32_t) t0);
    });
    if (!rc) rc = best_tail(run, "best-site", A.part, res.get());
    if (!rc) rc = dense_end(&run, "best-site scan", res.get());
    if (rc) return rc;
    *out = res.release();
    return MS_OK;
}

int ms_best_shape(const ms_best *b, int32_t *n_pwms, int64_t *n_seqs) { return dense_shape(b, n_pwms, n_seqs); }
int ms_best_device_ms(const ms_best *b, double *ms) { return dense_device_ms(b, ms); }

int ms_best_sites(const ms_best *b, int32_t m0, int32_t m1, double *score, int32_t *pos, int8_t *strand) {
    size_t at = 0, n = 0;
    if (int rc = dense_rows(b, m0, m1, &at, &n)) return rc;
    if (score && n) MS_HIP(hipMemcpy(score, b->d_score + at, 8 * n, hipMemcpyDeviceToHost));
    if (pos && n) MS_HIP(hipMemcpy(pos, b->d_pos + at, 4 * n, hipMemcpyDeviceToHost));
    if (strand && n) MS_HIP(hipMemcpy(strand, b->d_strand + at, n, hipMemcpyDeviceToHost));
    return MS_OK;
}

int ms_best_sites_device(const ms_best *b, void **d_score, void **d_pos, void **d_strand) {
    if (!b) { set_error("NULL argument"); return MS_ERR_INVALID; }
    if (d_score) *d_score = b->d_score;
    if (d_pos) *d_pos = b->d_pos;
    if (d_strand) *d_strand = b->d_strand;
    return MS_OK;
}

}  // extern "C"
