// ms_expcounts.hip -- the E-step of a motif refinement (ms_affinity_expected_counts): per motif column, how much A, C, G, T weight stands
// under it over ALL windows of all regions, every window weighted by its posterior probability of being the site.  No reference
// counterpart; the posterior-weighted counterpart of ms_result_site_base_counts, and the derivative of the log affinity with respect to
// the matrix entries.  include/motifscan_amd.h holds the definition; in short, with U = 2^-32:
//     pi(m, r)   the cell's responsibility: 1 (prior_logit = +inf), 0 (no term, log_mean = -inf, prior_logit = -inf), else
//                1 / (1 + exp(-(log_mean + prior_logit)))
//     w(term)    min(pi * exp(scale * (x - peak)) / sum, 1) for a term of raw sum x > -inf; q = (int64) rint(w * 2^32); q = 0 for x = -inf
//     counts     q added under every motif column c, to the slot of the base there in the motif's orientation (4: a non-ACGT base)
//
// Mapping: ms_affinity.hip's walk taken a second time (ms_best_dev.h holds what the walks share: a wave per SEGMENT of kBestSegWindows
// window starts, a lane keeps the words of its kBestStrips window starts in registers, the tile's tables in LDS), with another ending and
// another grid.  The affinity kernel's grid -- one block per (8 segments, tile) -- would end in blocks x columns x 5 global atomics onto
// the few addresses of a motif.  Here the grid is BOUNDED in x (kExpGridCapX blocks per tile; y = tile): a block takes groups of
// kBestWaves segments in a grid-stride loop and keeps an accumulator uint64 [tile columns][5] in LDS, beside the tile's tables, over the
// whole loop; at its end it adds the accumulator's non-zero cells to the output with 64-bit integer atomics, once.  kExpTileEntries is
// sized so that tables (16 B an entry) and accumulator (10 B an entry) of a full tile take 52 KB: the 128 registers a lane may have
// allow two blocks a CU, and their LDS fits the CU's 160 KB three times.
//
// The adds: after a strip's raw sums a lane forms q for its one or two terms from the cell's (peak, sum, pi) -- wave-uniform values,
// read once per (motif, segment).  A strip in which no lane holds a q != 0 (a ballot) skips the column loop: with a sharp matrix almost
// every window rounds to 0.  A cell whose pi is 0, or whose pi * 2^32 is <= 1/2 while sum >= 1 (every w <= pi then, every q = 0), is not
// scored at all.  In the column loop the lanes do NOT walk the columns together: at a fixed column the 64 lanes of a wave would meet in at
// most 5 LDS addresses.  The columns are taken in steps of up to 32 (the code word of the first step is in registers, a wider motif
// reads the further words as dense_strip_sums does), and within a step of n columns lane l starts at column l mod n
// and wraps.  The LDS adds are 64-bit integer atomics (ds_add_u64); there is no floating-point atomic anywhere, and because integer
// addition commutes the bytes are the same on every run, for every grid and every split of the motifs into tiles or of the regions
// into shards.
//
// total[row] is the sum of the five slots of the row's column 0 (every term adds its q to exactly one slot of every column) and
// n_regions[row] the number of n_terms > 0 in the row of the affinity's plane: expcounts_finish_kernel, one block per row.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <limits>

#include "ms_best_dev.h"
#include "ms_device.h"
#include "ms_handles.h"

namespace ms {

namespace {

constexpr int kExpTileEntries = 2048;                    // 512 motif columns per tile: 32 KB of tables + 20 KB of accumulators
constexpr int kExpAccBytesPerColumn = 5 * (int) sizeof(unsigned long long);
constexpr int kExpGridCapX = 1024;                       // the grid's x, blocks PER TILE (y = tiles: a call launches up to tiles x 1024 blocks)
constexpr DenseGeom kExpGeom = {kBestSegWindows, MS_EXPECTED_MAX_WIDTH, kExpTileEntries, false};

static_assert(kExpTileEntries >= 4 * MS_EXPECTED_MAX_WIDTH, "the widest motif of the walk fits a tile");
static_assert((kExpTileEntries + 1) * 16 + (kExpTileEntries / 4) * kExpAccBytesPerColumn <= 80 * 1024, "two blocks share a CU's 160 KB");

std::atomic<int32_t> g_exp_grid_cap{0};                  // ms_debug_expected_grid_cap: 0 = kExpGridCapX

struct ExpArgs {
    const uint32_t *codes, *nmask;
    const int64_t *offsets;                              // [R + 1]
    int64_t R;
    const int64_t *seg_first;                            // [R + 1] first segment of the region; nullptr: one segment per region
    int64_t n_seg, n_groups;                             // groups of kBestWaves segments
    const int32_t *tile_first;                           // [tiles + 1] into mot
    const int32_t *mot;                                  // the walked motifs, tile after tile
    DevPwm Pw;
    int strand_mask;
    int32_t max_n;
    double scale, prior;
    const double *peak, *sum, *log_mean;                 // [P][R] the affinity's planes
    const int32_t *n_terms;
    int32_t m0, C;                                       // row = m - m0; C = the column pitch of a row
    uint32_t lds_tab;                                    // double2 entries in front of the accumulator: 1 + the largest tile's
    unsigned long long *counts;                          // [rows][C][5], zeroed by the caller
};

// q of a term of raw sum x (live: the term exists and x > -inf): subtract, multiply, exp, multiply, divide, clamp, scale, round -- each
// rounded once (-ffp-contract=off).  A NaN weight (a handle that does not belong to these inputs) is clamped to 1.
__device__ __forceinline__ unsigned long long exp_quant(bool live, double x, double peak, double scale, double pi, double sum) {
    const double d = x - peak;
    const double t = scale * d;
    const double e = exp(t);
    const double a = pi * e;
    const double v = a / sum;
    const double w = !(v < 1.0) ? 1.0 : (v > 0.0 ? v : 0.0);
    const long long q = (long long) rint(w * 4294967296.0);
    return live ? (unsigned long long) q : 0ULL;
}

// q0 ('+') and q1 ('-') of the lane's window under the n <= 32 columns c0 .. c0 + n - 1 of the window (cwx / nwx: their codes and mask
// bits): window column cc is motif column cc on '+' and W - 1 - cc, complemented, on '-'.  Lane l starts at column l mod n.
__device__ __forceinline__ void exp_add_columns(unsigned long long *__restrict__ acc, int W, int c0, int n, uint64_t cwx, uint32_t nwx, int lane, unsigned long long q0,
                                                unsigned long long q1) {
    // lane mod n without the integer division sequence: lane < 64 and n <= 32, so (lane + 1/2) / n is at least 1/64 away from an
    // integer and the single-precision product with the reciprocal truncates to the exact quotient.  (Lanes that share a start
    // column are n apart; the other even spread, lane * n / 64, puts them side by side and was measured slower: DESIGN.md.)
    int i = lane - n * (int) (((float) lane + 0.5f) * __builtin_amdgcn_rcpf((float) n));
    for (int j = 0; j < n; j++) {
        const uint32_t b = (uint32_t) (cwx >> (2 * i)) & 3u;
        const bool non = (nwx >> i) & 1u;
        const int cc = c0 + i;
        if (q0) atomicAdd(&acc[cc * 5 + (non ? 4 : (int) b)], q0);
        if (q1) atomicAdd(&acc[(W - 1 - cc) * 5 + (non ? 4 : 3 - (int) b)], q1);
        i = i + 1 == n ? 0 : i + 1;
    }
}

// grid = (min(groups of kBestWaves segments, the cap), tiles).  Dynamic LDS: [lds_tab] double2 of tables, then the accumulator.
__global__ void __launch_bounds__(kBestThreads, 4) expcounts_kernel(const ExpArgs A, int32_t tile0) {
    extern __shared__ double2 exp_lds[];
    const int32_t tile = tile0 + (int32_t) blockIdx.y;
    const int32_t k0 = A.tile_first[tile], k1 = A.tile_first[tile + 1];
    const int64_t tab0 = A.Pw.tab_off[A.mot[k0]];
    const int32_t ml = A.mot[k1 - 1];
    const int32_t n_ent = (int32_t) (A.Pw.tab_off[ml] - tab0) + A.Pw.width[ml] * 4;      // <= kExpTileEntries: the plan's tile
    unsigned long long *const acc = reinterpret_cast<unsigned long long *>(exp_lds + A.lds_tab);
    const int32_t n_acc = (n_ent / 4) * 5;
    for (int32_t i = threadIdx.x; i < n_acc; i += kBestThreads) acc[i] = 0ULL;
    dense_stage_tile(exp_lds, A.Pw.tab2 + tab0, n_ent);                                  // (its barrier covers the zeroing)
    const int wave = __builtin_amdgcn_readfirstlane((int) (threadIdx.x >> 6));
    const int lane = (int) (threadIdx.x & 63u);
    const double ninf = -std::numeric_limits<double>::infinity();

    // no thread leaves the loop's body by a return: the barrier behind it is the block's
    for (int64_t grp = blockIdx.x; grp < A.n_groups; grp += gridDim.x) {
        const int64_t seg = grp * kBestWaves + wave;
        if (seg >= A.n_seg) continue;
        const int64_t r = A.seg_first ? find_region_bsearch(A.seg_first, A.R, seg) : seg;
        const int64_t s_in = A.seg_first ? seg - A.seg_first[r] : 0;
        const int64_t beg = A.offsets[r], L = A.offsets[r + 1] - beg;
        const int64_t p0 = s_in * kBestSegWindows;       // the segment's first window start

        uint64_t cw[kBestStrips];
        uint32_t nw[kBestStrips];
        dense_segment_words(A.codes, A.nmask, beg, L, p0, lane, cw, nw);

        for (int32_t k = k0; k < k1; k++) {
            const int32_t m = A.mot[k];
            const int W = A.Pw.width[m];
            const int64_t tab_m = A.Pw.tab_off[m];
            const uint32_t tb = 1u + (uint32_t) (tab_m - tab0);
            const int64_t last = L - W;                   // the region's last window start
            if (p0 > last) continue;                      // (wave-uniform) no window of this segment fits the region
            const int64_t cell = (int64_t) m * A.R + r;
            if (A.n_terms[cell] == 0) continue;           // max_n dropped every window
            const double peak = A.peak[cell], sum = A.sum[cell], lm = A.log_mean[cell];
            double pi = 1.0;
            if (!(A.prior == std::numeric_limits<double>::infinity())) {
                const double t = lm + A.prior;
                const double e = exp(-t);
                const double den = 1.0 + e;
                pi = 1.0 / den;
                if (lm == ninf || A.prior == ninf) pi = 0.0;
            }
            if (pi == 0.0 || (pi * 4294967296.0 <= 0.5 && sum >= 1.0)) continue;         // every q of the cell is 0
            unsigned long long *const acc_m = acc + (uint32_t) (tab_m - tab0) / 4u * 5u;
#pragma unroll 1
            for (int s = 0; s < kBestStrips; s++) {
                if (p0 + s * 64 > last) break;            // (wave-uniform) no window of this strip, or of a later one, fits the region
                const int64_t pos = p0 + s * 64 + lane;
                const bool valid = pos <= last;
                double fwd = 0.0, rev = 0.0;
                int n_non = 0;
                dense_strip_sums<true, true>(exp_lds, tb, A.Pw.tab2 + tab_m, A.codes, A.nmask, W, beg + pos, valid, s, cw, nw, fwd, rev, n_non);
                const bool counted = valid && (A.max_n < 0 || n_non <= A.max_n);
                const unsigned long long q0 = exp_quant(counted && (A.strand_mask & 1) && fwd > ninf, fwd, peak, A.scale, pi, sum);
                const unsigned long long q1 = exp_quant(counted && (A.strand_mask & 2) && rev > ninf, rev, peak, A.scale, pi, sum);
                const bool any = (q0 | q1) != 0ULL;
                if (__ballot(any) == 0) continue;
                uint64_t cws = cw[0];
                uint32_t nws = nw[0];
#pragma unroll
                for (int j = 1; j < kBestStrips; j++) { cws = s == j ? cw[j] : cws; nws = s == j ? nw[j] : nws; }
                exp_add_columns(acc_m, W, 0, W < 32 ? W : 32, cws, nws, lane, q0, q1);
                for (int c0 = 32; c0 < W; c0 += 32) {     // (a lane without a weight reads nothing)
                    const uint64_t cwx = any ? code_window(A.codes, beg + pos + c0) : 0ULL;
                    const uint32_t nwx = any ? n_window(A.nmask, beg + pos + c0) : 0u;
                    exp_add_columns(acc_m, W, c0, (W - c0) < 32 ? (W - c0) : 32, cwx, nwx, lane, q0, q1);
                }
            }
        }
    }
    __syncthreads();
    for (int32_t k = k0; k < k1; k++) {
        const int32_t m = A.mot[k];
        const int32_t n = A.Pw.width[m] * 5;
        const unsigned long long *const src = acc + (uint32_t) (A.Pw.tab_off[m] - tab0) / 4u * 5u;
        unsigned long long *const dst = A.counts + (size_t) (m - A.m0) * (size_t) A.C * 5;
        for (int32_t i = threadIdx.x; i < n; i += kBestThreads) {
            const unsigned long long v = src[i];
            if (v) atomicAdd(&dst[i], v);
        }
    }
}

// grid = rows: total = the five slots of the row's column 0; n_regions = the cells of the row that hold a term
__global__ void __launch_bounds__(256) expcounts_finish_kernel(const int32_t *__restrict__ n_terms, int64_t R, int32_t m0, const unsigned long long *__restrict__ counts,
                                                                int32_t C, unsigned long long *__restrict__ total, unsigned long long *__restrict__ n_regions) {
    __shared__ unsigned long long part[256];
    const int32_t row = (int32_t) blockIdx.x;
    const int32_t *__restrict__ src = n_terms + (size_t) (m0 + row) * (size_t) R;
    unsigned long long n = 0;
    for (int64_t r = threadIdx.x; r < R; r += 256) n += src[r] > 0 ? 1u : 0u;
    part[threadIdx.x] = n;
    __syncthreads();
    for (int d = 128; d >= 1; d >>= 1) {
        if ((int) threadIdx.x < d) part[threadIdx.x] += part[threadIdx.x + d];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        n_regions[row] = part[0];
        const unsigned long long *c0 = counts + (size_t) row * (size_t) C * 5;
        total[row] = c0[0] + c0[1] + c0[2] + c0[3] + c0[4];
    }
}

}  // namespace

}  // namespace ms

using namespace ms;

extern "C" {

int ms_debug_expected_dims(int32_t out[8]) {
    if (!out) { set_error("NULL output"); return MS_ERR_INVALID; }
    out[0] = kBestSegWindows;
    out[1] = MS_EXPECTED_MAX_WIDTH;
    out[2] = kExpTileEntries;
    out[3] = kBestWaves;
    out[4] = kBestStrips;
    out[5] = kExpAccBytesPerColumn;
    out[6] = kExpGridCapX;
    out[7] = 0;
    return MS_OK;
}

int ms_debug_expected_grid_cap(int32_t blocks) {
    if (blocks < 0) { set_error("the grid cap must be >= 0 (0 = the library's own)"); return MS_ERR_INVALID; }
    g_exp_grid_cap.store(blocks);
    return MS_OK;
}

int ms_affinity_expected_counts(const ms_affinity *aff, const ms_pwmset *pwms_c, const ms_seqset *seqs, double prior_logit, int32_t m0, int32_t m1, uint32_t flags,
                                int64_t *counts, int64_t *total, int64_t *n_regions, double *device_ms) {
    if (!require_device()) return MS_ERR_RUNTIME;
    if (device_ms) *device_ms = 0.0;
    if (!aff || !pwms_c || !seqs) { set_error("NULL handle"); return MS_ERR_INVALID; }
    if (flags != 0u) { set_error("unknown expected-counts flags 0x%x", flags); return MS_ERR_INVALID; }
    if (std::isnan(prior_logit)) { set_error("prior_logit is NaN"); return MS_ERR_INVALID; }
    ms_pwmset *pwms = const_cast<ms_pwmset *>(pwms_c);
    if (pwms->P != aff->P) { set_error("the affinity result holds %d motifs, the PWM set %d", aff->P, pwms->P); return MS_ERR_INVALID; }
    if (seqs->R != aff->R) { set_error("the affinity result was made over %lld regions, the sequence set holds %lld", (long long) aff->R, (long long) seqs->R); return MS_ERR_INVALID; }
    if (seqs->device != aff->device) { set_error("the sequence set lives on device %d, the affinity result on device %d", seqs->device, aff->device); return MS_ERR_INVALID; }
    if (m0 < 0 || m1 < m0 || m1 > aff->P) { set_error("motif range [%d, %d) outside [0, %d)", m0, m1, aff->P); return MS_ERR_INVALID; }
    const int32_t rows = m1 - m0;
    if (rows == 0) return MS_OK;
    if (!counts) { set_error("NULL output"); return MS_ERR_INVALID; }
    for (int32_t m = m0; m < m1; m++)
        if (pwms->widths[(size_t) m] > MS_EXPECTED_MAX_WIDTH) {
            set_error("motif %d has %d columns: ms_affinity_expected_counts takes at most %d", m, pwms->widths[(size_t) m], MS_EXPECTED_MAX_WIDTH);
            return MS_ERR_INVALID;
        }
    const int32_t C = pwms->max_width;
    void *outs[3] = {counts, total, n_regions};
    const size_t out_bytes[3] = {8 * (size_t) rows * 5 * (size_t) C, 8 * (size_t) rows, 8 * (size_t) rows};
    bool on_dev[3] = {false, false, false};
    for (int i = 0; i < 3; ++i) {
        if (!outs[i]) continue;
        int other = -1;
        const int place = pointer_place(outs[i], aff->device, &other);
        if (place < 0) { set_error("output lives on device %d, the affinity result on device %d", other, aff->device); return MS_ERR_INVALID; }
        on_dev[i] = place > 0;
    }
    const int64_t R = seqs->R;
    DeviceCtx *c;
    int rc = get_ctx(aff->device, &c);
    if (rc) return rc;

    // ---- the plan, on the host: the affinity's segments (no partials), tiles of the range's scorable motifs
    DensePlan plan;
    if ((rc = dense_plan_for(kExpGeom, pwms, seqs, kBestWaves, [&](int32_t m) { return m >= m0 && m < m1 && entries_scorable(pwms, m); }, &plan))) return rc;
    const int64_t n_tiles = (int64_t) plan.tile_first.size() - 1;
    const int64_t n_groups = (plan.n_seg + kBestWaves - 1) / kBestWaves;

    std::lock_guard<std::mutex> lk_dev(c->mu);
    std::lock_guard<std::mutex> lk_pwm(pwms->mu);
    MS_HIP(hipSetDevice(c->device));
    Carve cv;
    const DenseSlots ds = dense_slots(cv, plan);
    const auto s_counts = cv.add<unsigned long long>(on_dev[0] ? 0 : out_bytes[0] / 8);
    const auto s_total = cv.add<unsigned long long>((size_t) rows), s_nreg = cv.add<unsigned long long>((size_t) rows);
    const hipStream_t st = c->stream;
    WorkBlock work;                                    // (behind the locks: it goes back behind a wait for the stream, whichever way this returns)
    if ((rc = work.alloc(c, st, cv.bytes() + 256))) return rc;
    void *const wblk = work.p;
    unsigned long long *d_counts = on_dev[0] ? reinterpret_cast<unsigned long long *>(counts) : Carve::at(wblk, s_counts);
    unsigned long long *d_total = Carve::at(wblk, s_total), *d_nreg = Carve::at(wblk, s_nreg);

    hipError_t he = hipMemsetAsync(d_counts, 0, out_bytes[0], st);
    if (he != hipSuccess) return hip_rc(he, "clearing the expected counts");
    (void) hipEventRecord(c->ev[0], st);
    if (n_tiles > 0 && n_groups > 0) {
        if ((rc = pwmset_upload(pwms, c->device, st))) return rc;
        if ((rc = seqset_pack_pending(seqs, st))) return rc;
        const size_t lds_tab = plan.max_tile + 1;
        const size_t lds = lds_tab * sizeof(double2) + (plan.max_tile / 4) * (size_t) kExpAccBytesPerColumn;
        const size_t lds_most = (size_t) (kExpTileEntries + 1) * sizeof(double2) + (size_t) (kExpTileEntries / 4) * (size_t) kExpAccBytesPerColumn;
        if ((rc = dense_raise_lds(c, reinterpret_cast<const void *>(expcounts_kernel), lds, lds_most))) return rc;
        DenseDev d;
        if ((rc = dense_upload(plan, ds, wblk, st, &d))) return rc;
        ExpArgs A;
        A.codes = seqs->d_codes; A.nmask = seqs->d_nmask; A.offsets = seqs->d_offsets; A.R = R;
        A.seg_first = d.seg_first;
        A.n_seg = plan.n_seg; A.n_groups = n_groups;
        A.tile_first = d.tile_first; A.mot = d.mot;
        A.Pw = dev_pwm(pwms);
        A.strand_mask = aff->strand_mask;
        A.max_n = aff->max_n;
        A.scale = aff->scale;
        A.prior = prior_logit;
        A.peak = aff->d_peak; A.sum = aff->d_sum; A.log_mean = aff->d_log_mean; A.n_terms = aff->d_n_terms;
        A.m0 = m0; A.C = C;
        A.lds_tab = (uint32_t) lds_tab;
        A.counts = d_counts;
        const int32_t cap_set = g_exp_grid_cap.load();
        const unsigned gx = (unsigned) std::min<int64_t>(n_groups, cap_set > 0 ? cap_set : kExpGridCapX);
        rc = dense_chunks(n_tiles, "expected-counts kernel", [&](int64_t t0, unsigned ny) {
            hipLaunchKernelGGL(expcounts_kernel, dim3(gx, ny), dim3(kBestThreads), lds, st, A, (int32_t) t0);
        });
        if (rc) return rc;
    }
    hipLaunchKernelGGL(expcounts_finish_kernel, dim3((unsigned) rows), dim3(256), 0, st, aff->d_n_terms, R, m0, d_counts, C, d_total, d_nreg);
    if ((he = hipGetLastError()) != hipSuccess) return hip_rc(he, "expected-counts finish kernel");
    (void) hipEventRecord(c->ev[1], st);
    if (!on_dev[0]) he = hipMemcpyAsync(counts, d_counts, out_bytes[0], hipMemcpyDeviceToHost, st);
    if (he == hipSuccess && total) he = hipMemcpyAsync(total, d_total, out_bytes[1], on_dev[1] ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st);
    if (he == hipSuccess && n_regions) he = hipMemcpyAsync(n_regions, d_nreg, out_bytes[2], on_dev[2] ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st);
    if (he != hipSuccess) return hip_rc(he, "expected counts");
    if ((rc = work.wait("expected counts"))) return rc;
    float ms01 = 0;
    (void) hipEventElapsedTime(&ms01, c->ev[0], c->ev[1]);
    if (device_ms) *device_ms = ms01;
    return MS_OK;
}

}  // extern "C"
