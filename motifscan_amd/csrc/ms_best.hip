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
#include <algorithm>
#include <cmath>
#include <limits>
#include <memory>

#include "ms_best_dev.h"
#include "ms_device.h"
#include "ms_handles.h"

namespace ms {

namespace {

// (the sizes of the walk -- kBestThreads ... kBestGridY -- are in ms_best_dev.h: ms_affinity.hip walks the same way)
struct BestPart {                                        // a segment's best of one motif
    double q;
    int32_t pos;                                         // -1: no winner
    int32_t strand;
};

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

__device__ __forceinline__ void put_best(double *__restrict__ score, int32_t *__restrict__ pos, int8_t *__restrict__ strand, int64_t cell, double q, uint64_t key) {
    const bool won = key != kNoKey;
    score[cell] = won ? q : __builtin_nan("");
    pos[cell] = won ? (int32_t) (key >> 2) : -1;
    strand[cell] = won ? (int8_t) (key & 3u) : (int8_t) 0;
}

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
__global__ void __launch_bounds__(256) best_reduce_kernel(const BestArgs A, const int64_t *__restrict__ long_regions, int32_t k_first, int32_t n_mot) {
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
__global__ void __launch_bounds__(256) best_fill_kernel(const int32_t *__restrict__ motifs, int64_t R, double *__restrict__ score, int32_t *__restrict__ pos,
                                                        int8_t *__restrict__ strand) {
    const int64_t r = (int64_t) blockIdx.x * 256 + threadIdx.x;
    if (r >= R) return;
    put_best(score, pos, strand, (int64_t) motifs[blockIdx.y] * R + r, 0.0, kNoKey);
}


}  // namespace

}  // namespace ms

using namespace ms;

extern "C" {

int ms_debug_best_segment_windows(void) { return kBestSegWindows; }

void ms_best_free(ms_best *b) {
    if (!b) return;
    if (b->block) {
        (void) hipSetDevice(b->device);
        DeviceCtx *c = nullptr;
        if (get_ctx(b->device, &c) == MS_OK) pool_free(c, b->block, b->block_bytes); else (void) hipFree(b->block);
    }
    delete b;
}

int ms_scan_best(const ms_pwmset *pwms_c, const ms_seqset *seqs, int strand_mask, uint32_t flags, ms_best **out) {
    if (!out) { set_error("out is NULL"); return MS_ERR_INVALID; }
    *out = nullptr;
    if (!require_device()) return MS_ERR_RUNTIME;
    if (!pwms_c || !seqs) { set_error("NULL handle"); return MS_ERR_INVALID; }
    if (strand_mask < 1 || strand_mask > 3) { set_error("invalid strand mask %d (1 '+', 2 '-', 3 both)", strand_mask); return MS_ERR_INVALID; }
    if (flags != 0u) { set_error("unknown best-site scan flags 0x%x", flags); return MS_ERR_INVALID; }
    ms_pwmset *pwms = const_cast<ms_pwmset *>(pwms_c);
    const int32_t P = pwms->P;
    const int64_t R = seqs->R;
    const int64_t *off = seqs->offsets.data();
    for (int64_t r = 0; r < R; r++)
        if (off[r + 1] - off[r] >= (1LL << 31)) {
            set_error("region %lld has %lld bases: positions are 32-bit, cut it into regions of fewer than 2^31", (long long) r, (long long) (off[r + 1] - off[r]));
            return MS_ERR_INVALID;
        }
    DeviceCtx *c;
    int rc = get_ctx(seqs->device, &c);
    if (rc) return rc;
    std::unique_ptr<ms_best> res(new (std::nothrow) ms_best());
    if (!res) { set_error("out of host memory"); return MS_ERR_NOMEM; }
    res->device = c->device;
    res->P = P;
    res->R = R;

    // ---- the plan, on the host: segments of the regions, tiles of the motifs (dense_plan, ms_best_dev.h)
    DensePlan plan;
    try {
        dense_plan(pwms, off, R, [&](int32_t m) { return scorable(pwms, m); }, &plan);
    } catch (const std::bad_alloc &) { set_error("out of host memory"); return MS_ERR_NOMEM; }
    const std::vector<int64_t> &seg_first = plan.seg_first, &part_first = plan.part_first, &long_regions = plan.long_regions;
    const std::vector<int32_t> &mot = plan.mot, &tile_first = plan.tile_first, &wide_first = plan.wide_first, &uns = plan.skipped;
    const int64_t n_seg = plan.n_seg, n_part = plan.n_part;
    const size_t max_tile = plan.max_tile;
    const int32_t n_lds_tiles = (int32_t) tile_first.size() - 1, n_wide = (int32_t) wide_first.size() - 1, n_mot = (int32_t) mot.size();
    const int64_t n_long = (int64_t) long_regions.size();
    if (n_long > 0x7FFFFFFFLL || (n_seg + kBestWaves - 1) / kBestWaves > 0x7FFFFFFFLL) { set_error("too many segments for one launch"); return MS_ERR_INVALID; }

    // ---- 13 bytes per cell, 16 per partial: both blocks are allocated before anything is launched, and a failure there is the MS_ERR_NOMEM
    // of the header (the test here only keeps the byte counts below inside size_t)
    if (13.0 * (double) P * (double) R + 16.0 * (double) P * (double) n_part >= 0.5 * (double) std::numeric_limits<size_t>::max()) {
        set_error("%d x %lld cells do not fit the device", P, (long long) R);
        return MS_ERR_NOMEM;
    }
    const size_t cells = (size_t) P * (size_t) R, cz = std::max<size_t>(cells, 1);
    std::lock_guard<std::mutex> lk_dev(c->mu);
    std::lock_guard<std::mutex> lk_pwm(pwms->mu);
    MS_HIP(hipSetDevice(c->device));
    {
        void *blk = nullptr;
        size_t got = 0;
        if ((rc = pool_alloc(c, up256(8 * cz) + up256(4 * cz) + up256(cz), &blk, &got))) return rc;
        res->block = blk;
        res->block_bytes = got;
        char *p = static_cast<char *>(blk);
        res->d_score = reinterpret_cast<double *>(p); p += up256(8 * cz);
        res->d_pos = reinterpret_cast<int32_t *>(p); p += up256(4 * cz);
        res->d_strand = reinterpret_cast<int8_t *>(p);
    }
    ms_best *raw = res.release();
    if (cells == 0) { *out = raw; return MS_OK; }

    const size_t b_seg = seg_first.empty() ? 0 : up256(8 * seg_first.size()), b_long = up256(8 * std::max<size_t>(long_regions.size(), 1)),
                 b_mot = up256(4 * std::max<size_t>(mot.size(), 1)), b_tile = up256(4 * tile_first.size()), b_wide = up256(4 * wide_first.size()),
                 b_uns = up256(4 * std::max<size_t>(uns.size(), 1)), b_part = up256(sizeof(BestPart) * std::max<size_t>((size_t) P * (size_t) n_part, 1));
    void *wblk = nullptr;
    size_t wgot = 0;
    if ((rc = pool_alloc(c, 2 * b_seg + b_long + b_mot + b_tile + b_wide + b_uns + b_part, &wblk, &wgot))) { ms_best_free(raw); return rc; }
    auto fail = [&](int code) { pool_free(c, wblk, wgot); ms_best_free(raw); return code; };
    auto hip_fail = [&](hipError_t e, const char *what) { set_error("%s failed: %s", what, hipGetErrorString(e)); return fail(e == hipErrorOutOfMemory ? MS_ERR_NOMEM : MS_ERR_RUNTIME); };
    char *b = static_cast<char *>(wblk);
    int64_t *d_seg = reinterpret_cast<int64_t *>(b); b += b_seg;
    int64_t *d_pfirst = reinterpret_cast<int64_t *>(b); b += b_seg;
    int64_t *d_long = reinterpret_cast<int64_t *>(b); b += b_long;
    int32_t *d_mot = reinterpret_cast<int32_t *>(b); b += b_mot;
    int32_t *d_tile = reinterpret_cast<int32_t *>(b); b += b_tile;
    int32_t *d_wide = reinterpret_cast<int32_t *>(b); b += b_wide;
    int32_t *d_uns = reinterpret_cast<int32_t *>(b); b += b_uns;
    BestPart *d_part = reinterpret_cast<BestPart *>(b);

    const hipStream_t st = c->stream;
    if ((rc = pwmset_upload(pwms, c->device, st))) return fail(rc);
    if ((rc = seqset_pack_pending(seqs, st))) return fail(rc);
    const size_t lds = (max_tile + 1) * sizeof(double2);
    hipError_t he = hipSuccess;
    if (lds > 48 * 1024 && !c->best_lds_set) {
        he = hipFuncSetAttribute(reinterpret_cast<const void *>(best_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int) ((kBestTileEntries + 1) * sizeof(double2)));
        if (he != hipSuccess) return hip_fail(he, "raising the LDS limit");
        c->best_lds_set = true;
    }
    if (!seg_first.empty()) {
        he = hipMemcpyAsync(d_seg, seg_first.data(), 8 * seg_first.size(), hipMemcpyHostToDevice, st);
        if (he == hipSuccess) he = hipMemcpyAsync(d_pfirst, part_first.data(), 8 * part_first.size(), hipMemcpyHostToDevice, st);
        if (he == hipSuccess && n_long > 0) he = hipMemcpyAsync(d_long, long_regions.data(), 8 * long_regions.size(), hipMemcpyHostToDevice, st);
    }
    if (he == hipSuccess && n_mot > 0) he = hipMemcpyAsync(d_mot, mot.data(), 4 * mot.size(), hipMemcpyHostToDevice, st);
    if (he == hipSuccess) he = hipMemcpyAsync(d_tile, tile_first.data(), 4 * tile_first.size(), hipMemcpyHostToDevice, st);
    if (he == hipSuccess) he = hipMemcpyAsync(d_wide, wide_first.data(), 4 * wide_first.size(), hipMemcpyHostToDevice, st);
    if (he == hipSuccess && !uns.empty()) he = hipMemcpyAsync(d_uns, uns.data(), 4 * uns.size(), hipMemcpyHostToDevice, st);
    if (he != hipSuccess) return hip_fail(he, "upload of the plan");

    BestArgs A;
    A.codes = seqs->d_codes; A.nmask = seqs->d_nmask; A.offsets = seqs->d_offsets; A.R = R;
    A.seg_first = seg_first.empty() ? nullptr : d_seg;
    A.part_first = seg_first.empty() ? nullptr : d_pfirst;
    A.n_seg = n_seg; A.n_part = n_part;
    A.tile_first = d_tile; A.mot = d_mot;
    A.Pw = dev_pwm(pwms);
    A.strand_mask = strand_mask;
    A.score = raw->d_score; A.pos = raw->d_pos; A.strand = raw->d_strand;
    A.part = d_part;

    (void) hipEventRecord(c->ev[0], st);
    const unsigned gx = (unsigned) ((n_seg + kBestWaves - 1) / kBestWaves);
    for (int32_t t0 = 0; t0 < n_lds_tiles; t0 += kBestGridY) {
        hipLaunchKernelGGL(best_kernel<true>, dim3(gx, (unsigned) std::min(kBestGridY, n_lds_tiles - t0)), dim3(kBestThreads), lds, st, A, t0);
        if ((he = hipGetLastError()) != hipSuccess) return hip_fail(he, "best-site kernel");
    }
    if (n_wide > 0) {
        BestArgs Aw = A;
        Aw.tile_first = d_wide;
        for (int32_t t0 = 0; t0 < n_wide; t0 += kBestGridY) {
            hipLaunchKernelGGL(best_kernel<false>, dim3(gx, (unsigned) std::min(kBestGridY, n_wide - t0)), dim3(kBestThreads), 0, st, Aw, t0);
            if ((he = hipGetLastError()) != hipSuccess) return hip_fail(he, "best-site kernel (tables in HBM)");
        }
    }
    for (int32_t kf = 0; n_long > 0 && kf < n_mot; kf += 4 * kBestGridY) {
        hipLaunchKernelGGL(best_reduce_kernel, dim3((unsigned) n_long, (unsigned) std::min(kBestGridY, (n_mot - kf + 3) / 4)), dim3(256), 0, st, A, d_long, kf, n_mot);
        if ((he = hipGetLastError()) != hipSuccess) return hip_fail(he, "best-site reduction");
    }
    for (size_t u0 = 0; u0 < uns.size(); u0 += kBestGridY) {
        hipLaunchKernelGGL(best_fill_kernel, dim3((unsigned) ((R + 255) / 256), (unsigned) std::min<size_t>(kBestGridY, uns.size() - u0)), dim3(256), 0, st,
                           d_uns + u0, R, raw->d_score, raw->d_pos, raw->d_strand);
        if ((he = hipGetLastError()) != hipSuccess) return hip_fail(he, "best-site fill");
    }
    (void) hipEventRecord(c->ev[1], st);
    he = hipStreamSynchronize(st);
    if (he != hipSuccess) return hip_fail(he, "best-site scan");
    float ms01 = 0;
    (void) hipEventElapsedTime(&ms01, c->ev[0], c->ev[1]);
    raw->device_ms = ms01;
    pool_free(c, wblk, wgot);
    *out = raw;
    return MS_OK;
}

int ms_best_shape(const ms_best *b, int32_t *n_pwms, int64_t *n_seqs) {
    if (!b) { set_error("NULL argument"); return MS_ERR_INVALID; }
    if (n_pwms) *n_pwms = b->P;
    if (n_seqs) *n_seqs = b->R;
    return MS_OK;
}

int ms_best_sites(const ms_best *b, int32_t m0, int32_t m1, double *score, int32_t *pos, int8_t *strand) {
    if (!b) { set_error("NULL argument"); return MS_ERR_INVALID; }
    if (m0 < 0 || m1 > b->P || m0 > m1) { set_error("motif range [%d, %d) outside [0, %d)", m0, m1, b->P); return MS_ERR_INVALID; }
    const size_t at = (size_t) m0 * (size_t) b->R, n = (size_t) (m1 - m0) * (size_t) b->R;
    if (n == 0) return MS_OK;
    MS_HIP(hipSetDevice(b->device));
    if (score) MS_HIP(hipMemcpy(score, b->d_score + at, 8 * n, hipMemcpyDeviceToHost));
    if (pos) MS_HIP(hipMemcpy(pos, b->d_pos + at, 4 * n, hipMemcpyDeviceToHost));
    if (strand) MS_HIP(hipMemcpy(strand, b->d_strand + at, n, hipMemcpyDeviceToHost));
    return MS_OK;
}

int ms_best_sites_device(const ms_best *b, void **d_score, void **d_pos, void **d_strand) {
    if (!b) { set_error("NULL argument"); return MS_ERR_INVALID; }
    if (d_score) *d_score = b->d_score;
    if (d_pos) *d_pos = b->d_pos;
    if (d_strand) *d_strand = b->d_strand;
    return MS_OK;
}

int ms_best_device_ms(const ms_best *b, double *ms) {
    if (!b || !ms) { set_error("NULL argument"); return MS_ERR_INVALID; }
    *ms = b->device_ms;
    return MS_OK;
}

}  // extern "C"
