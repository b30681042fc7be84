// ms_sweep.hip -- the window sweep (N3): ms_scan_sweep and the hand-out of a span's hits to its windows, kernels and host code
// (the sibling hand-out for overlapping regions is ms_regions.hip).
//
// A sweep scans one chromosome span as ONE region and hands every hit to each window that holds it whole:
// window k = [k * stride, k * stride + window) of the span; a hit of a width-W motif at span position g lies in
// windows ceil((g + W - window) / stride) .. floor(g / stride)  (cscore.c:340: the window must contain all W bases).
#include <algorithm>

#include "ms_device.h"
#include "ms_handles.h"

namespace ms {

__device__ __forceinline__ void sweep_window_range(int64_t g, int W, int32_t window, int32_t stride, int64_t n_windows,
                                                   int64_t &lo, int64_t &hi) {
    hi = g / stride;
    if (hi > n_windows - 1) hi = n_windows - 1;
    const int64_t need = g + W - window;                       // smallest window start that still holds the site
    lo = need <= 0 ? 0 : (need + stride - 1) / stride;
}

__global__ void __launch_bounds__(256) sweep_count_kernel(int64_t n, const int64_t *__restrict__ motif_off, int32_t P,
                                                          const int32_t *__restrict__ width, const int64_t *__restrict__ pos,
                                                          int32_t window, int32_t stride, int64_t n_windows,
                                                          uint32_t *__restrict__ cnt) {
    const int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int32_t m = motif_of_hit(motif_off, P, i);
    int64_t lo, hi;
    sweep_window_range(pos[i], width[m], window, stride, n_windows, lo, hi);
    cnt[i] = hi >= lo ? (uint32_t) (hi - lo + 1) : 0u;
}

// Hand-out without a sort.  Within a motif the hits are ordered by span position g (then strand), and both ends of
// a hit's window range are non-decreasing in g, so the number of sites that precede site (hit i, window w) in the
// reference's order (motif, window, position, strand) is
//     dst[i]                                   all windows of all earlier hits (exclusive prefix sum of the counts)
//   + (w - lo_i)                               the hit's own earlier windows
//   - sum_{i' < i} max(0, hi_i' - w)           earlier hits' windows that come AFTER w
//   + sum_{i' > i} max(0, min(w, hi_i' + 1) - lo_i')   later hits' windows that come BEFORE w
// where only hits of the same motif within one window length of g contribute to the two sums (a few at most, except
// in low-complexity floods where the walk is bounded by window * 2 strands).  A site is the first of its
// (motif, window) iff the previous hit of the motif does not reach window w.
__global__ void __launch_bounds__(256) sweep_scatter_kernel(int64_t n, const int64_t *__restrict__ motif_off, int32_t P,
                                                            const int32_t *__restrict__ width, const int64_t *__restrict__ pos,
                                                            const double *__restrict__ score, const int8_t *__restrict__ strand,
                                                            const uint64_t *__restrict__ dst, int32_t window, int32_t stride,
                                                            int64_t n_windows, int64_t *__restrict__ seq_idx_out,
                                                            int64_t *__restrict__ pos_out, double *__restrict__ score_out,
                                                            int8_t *__restrict__ strand_out,
                                                            unsigned long long *__restrict__ region_counts) {
    const int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i < n;
    int32_t m = -1;
    int n_first = 0;
    if (live) {
        m = motif_of_hit(motif_off, P, i);
        const int W = width[m];
        const int64_t first = motif_off[m], last = motif_off[m + 1];
        const int64_t g = pos[i];
        int64_t lo, hi;
        sweep_window_range(g, W, window, stride, n_windows, lo, hi);
        if (hi >= lo) {
            const double sc = score[i];
            const int8_t sd = strand[i];
            const int64_t base = (int64_t) dst[i];
            int64_t prev_hi = -1;                                    // window range end of the previous hit of this motif
            if (i > first) { int64_t l2; sweep_window_range(pos[i - 1], W, window, stride, n_windows, l2, prev_hi); if (prev_hi < l2) prev_hi = -1; }
            for (int64_t w = lo; w <= hi; w++) {
                int64_t idx = base + (w - lo);
                for (int64_t j = i - 1; j >= first; j--) {           // earlier hits still reaching past w
                    int64_t l2, h2;
                    sweep_window_range(pos[j], W, window, stride, n_windows, l2, h2);
                    if (h2 <= lo) break;                             // monotone: nothing further back reaches past lo <= w
                    if (h2 >= l2 && h2 > w) idx -= h2 - w;
                }
                for (int64_t j = i + 1; j < last; j++) {             // later hits that already started before w
                    int64_t l2, h2;
                    sweep_window_range(pos[j], W, window, stride, n_windows, l2, h2);
                    if (l2 >= hi) break;                             // monotone: nothing further on starts before hi >= w
                    if (h2 >= l2 && l2 < w) idx += (w < h2 + 1 ? w : h2 + 1) - l2;
                }
                seq_idx_out[idx] = w;
                pos_out[idx] = g - w * stride;
                score_out[idx] = sc;
                strand_out[idx] = sd;
                if (prev_hi < w) n_first++;
            }
        }
    }
    // windows with >= 1 site per motif (stats.py:29-31): one atomic per (wave, motif)
    unsigned long long todo = __ballot(live && n_first > 0);
    while (todo) {
        const int leader = __ffsll((long long) todo) - 1;
        const int32_t mm = __shfl(m, leader);
        const unsigned long long same = __ballot(live && n_first > 0 && m == mm);
        int v = (live && m == mm) ? n_first : 0;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
        if ((int) (threadIdx.x & 63) == leader) atomicAdd(&region_counts[mm], (unsigned long long) v);
        todo &= ~same;
    }
}

// The hand-out of a COUNTS-ONLY sweep (MS_STREAM_NO_HITS; round 5): what the enrichment statistics read of a sweep is, per motif, the number
// of windows that hold >= 1 site (stats.py:29-31) -- plus, here, the number of sites.  Within a motif the hits are ordered by span
// position and both ends of a hit's window range are non-decreasing, so hit i is the FIRST site of exactly the windows of its range that
// the previous hit of the motif does not reach: max(0, hi_i - max(lo_i, prev_hi + 1) + 1).  One read per hit, no site is written
// (the full hand-out writes 25 bytes per (site, window): 36 GB per pass of a 3 Gbp genome).
__global__ void __launch_bounds__(kSweepCountThreads) sweep_countonly_kernel(int64_t n, const int64_t *__restrict__ motif_off, int32_t P,
                                                              const int32_t *__restrict__ width, const int64_t *__restrict__ pos,
                                                              int32_t window, int32_t stride, int64_t n_windows,
                                                              unsigned long long *__restrict__ region_counts, unsigned long long *__restrict__ n_sites /* [P] */) {
    const int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i < n;
    int32_t m = -1;
    int n_first = 0;
    unsigned long long mine = 0;
    if (live) {
        m = motif_of_hit(motif_off, P, i);
        const int W = width[m];
        int64_t lo, hi;
        sweep_window_range(pos[i], W, window, stride, n_windows, lo, hi);
        if (hi >= lo) {
            mine = (unsigned long long) (hi - lo + 1);
            int64_t prev_hi = -1;
            if (i > motif_off[m]) { int64_t l2; sweep_window_range(pos[i - 1], W, window, stride, n_windows, l2, prev_hi); if (prev_hi < l2) prev_hi = -1; }
            const int64_t from = lo > prev_hi + 1 ? lo : prev_hi + 1;
            n_first = hi >= from ? (int) (hi - from + 1) : 0;
        }
    }
    // per motif: windows with >= 1 site and sites -- one pair of atomics per (wave, motif), spread over the motifs' words (ONE counter for
    // the sites was tried first: 234 k atomics per span on one address, 2.6 ms per span at the ~90 M/s a single word sustains)
    unsigned long long todo = __ballot(live && mine > 0);
    while (todo) {
        const int leader = __ffsll((long long) todo) - 1;
        const int32_t mm = __shfl(m, leader);
        const unsigned long long same = __ballot(live && mine > 0 && m == mm);
        int v = (live && m == mm) ? n_first : 0;
        unsigned long long s64 = (live && m == mm) ? mine : 0ULL;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) { v += __shfl_xor(v, o); s64 += __shfl_xor(s64, o); }
        if ((int) (threadIdx.x & 63) == leader) {
            if (v) atomicAdd(&region_counts[mm], (unsigned long long) v);
            atomicAdd(&n_sites[mm], s64);
        }
        todo &= ~same;
    }
}

// per-motif offsets of the handed-out sites: where the motif's first hit went
__global__ void sweep_offsets_kernel(const int64_t *__restrict__ motif_off, int32_t P, int64_t n, const uint64_t *__restrict__ dst,
                                     int64_t total, int64_t *__restrict__ out) {
    const int32_t m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m > P) return;
    const int64_t f = m < P ? motif_off[m] : n;
    out[m] = f < n ? (int64_t) dst[f] : total;
}

static int launch_sweep_count(int64_t n, const int64_t *motif_off, int32_t P, const int32_t *width, const int64_t *pos,
                              int32_t window, int32_t stride, int64_t n_windows, uint32_t *cnt, hipStream_t st) {
    if (n == 0) return MS_OK;
    hipLaunchKernelGGL(sweep_count_kernel, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, st, n, motif_off, P, width, pos,
                       window, stride, n_windows, cnt);
    MS_HIP(hipGetLastError());
    return MS_OK;
}

static int launch_sweep_countonly(int64_t n, const int64_t *motif_off, int32_t P, const int32_t *width, const int64_t *pos,
                                  int32_t window, int32_t stride, int64_t n_windows, unsigned long long *region_counts, unsigned long long *n_sites, hipStream_t st) {
    if (n == 0) return MS_OK;
    hipLaunchKernelGGL(sweep_countonly_kernel, dim3((unsigned) ((n + kSweepCountThreads - 1) / kSweepCountThreads)), dim3(kSweepCountThreads), 0, st, n, motif_off, P, width, pos,
                       window, stride, n_windows, region_counts, n_sites);
    MS_HIP(hipGetLastError());
    return MS_OK;
}

static int launch_sweep_scatter(int64_t n, const int64_t *motif_off, int32_t P, const int32_t *width, const int64_t *pos,
                                const double *score, const int8_t *strand, const uint64_t *dst, int32_t window, int32_t stride,
                                int64_t n_windows, int64_t total, int64_t *seq_idx_out, int64_t *pos_out, double *score_out,
                                int8_t *strand_out, int64_t *motif_off_out, unsigned long long *region_counts, hipStream_t st) {
    hipLaunchKernelGGL(sweep_offsets_kernel, dim3((unsigned) ((P + 1 + 255) / 256)), dim3(256), 0, st, motif_off, P, n, dst, total,
                       motif_off_out);
    MS_HIP(hipGetLastError());
    if (n == 0) return MS_OK;
    hipLaunchKernelGGL(sweep_scatter_kernel, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, st, n, motif_off, P, width, pos,
                       score, strand, dst, window, stride, n_windows, seq_idx_out, pos_out, score_out, strand_out, region_counts);
    MS_HIP(hipGetLastError());
    return MS_OK;
}

// The counts-only form of the hand-out: consumes r1 and raw on failure, r1 on success (ev[0] is recorded by the caller).
static int sweep_counts_only(DeviceCtx *c, ms_pwmset *pwms, ms_result *r1, ms_result *raw, int64_t span_bases, int32_t window, int32_t stride,
                             int64_t n_windows, ms_result **out) {
    int rc;
    hipError_t he;
    const size_t n1 = (size_t) r1->n_hits;
    auto fail = [&](int code) { ms_result_free(raw); ms_result_free(r1); return code; };
    // what a counts-only sweep reads of a span: per motif the windows with >= 1 site, and the number of sites -- one pass over the
    // span's hit positions, nothing handed out (sweep_countonly_kernel)
    if ((size_t) pwms->P > (size_t) kSweepCountMaxMotifs) { set_error("internal: counts-only hand-out with more than %d motifs", kSweepCountMaxMotifs); return fail(MS_ERR_RUNTIME); }
    if ((rc = result_block_alloc(c, raw, 1))) return fail(rc);        // (room for >= kSweepCountMaxMotifs words behind the counts)
    raw->counts_only = true;
    const size_t P1 = (size_t) pwms->P + 1;
    unsigned long long *d_sites = reinterpret_cast<unsigned long long *>(raw->d_seq_idx);           // per-motif sites, summed on the host
    he = hipMemsetAsync(raw->d_region_counts, 0, 8 * P1, c->stream);
    if (he == hipSuccess) he = hipMemsetAsync(raw->d_motif_first, 0, 8 * P1, c->stream);
    if (he == hipSuccess) he = hipMemsetAsync(d_sites, 0, 8 * P1, c->stream);
    if (he != hipSuccess) { set_error("memset failed: %s", hipGetErrorString(he)); return fail(MS_ERR_RUNTIME); }
    rc = launch_sweep_countonly((int64_t) n1, r1->d_motif_first, r1->P, pwms->d_width, r1->d_pos, window, stride, n_windows,
                                raw->d_region_counts, d_sites, c->stream);
    if (rc) return fail(rc);
    (void) hipEventRecord(c->ev[1], c->stream);
    std::vector<unsigned long long> per_motif((size_t) pwms->P, 0ULL);
    if (pwms->P > 0) he = hipMemcpyAsync(per_motif.data(), d_sites, 8 * (size_t) pwms->P, hipMemcpyDeviceToHost, c->stream);
    if (he == hipSuccess) he = hipStreamSynchronize(c->stream);
    if (he != hipSuccess) { set_error("sweep count failed: %s", hipGetErrorString(he)); return fail(MS_ERR_RUNTIME); }
    unsigned long long n_sites = 0;
    for (size_t p = 0; p < per_motif.size(); p++) {      // the offsets a caller slices by: consistent with n_hits although no site array exists
        n_sites += per_motif[p];
        raw->motif_offsets[p + 1] = (int64_t) n_sites;
    }
    raw->n_hits = (int64_t) n_sites;
    float ms01 = 0;
    (void) hipEventElapsedTime(&ms01, c->ev[0], c->ev[1]);
    ms_scan_stats &stt = raw->stats;
    stt.ms_finalize += ms01;
    stt.ms_total += ms01;
    stt.n_hits = (int64_t) n_sites;
    stt.n_bases = span_bases;
    stt.n_windows = 0;
    for (int32_t p = 0; p < pwms->P; p++) stt.n_windows += n_windows * std::max<int64_t>(window - pwms->widths[p] + 1, 0);
    ms_result_free(r1);
    *out = raw;
    return MS_OK;
}

// r1: the scan of the span as ONE region.  Consumes r1 (also on failure).
int sweep_handout_locked(DeviceCtx *c, ms_pwmset *pwms, ms_result *r1, int64_t span_bases, int32_t window, int32_t stride,
                         int64_t n_windows, ms_result **out, bool counts_only) {
    int rc;
    auto fail = [&](int code) { ms_result_free(r1); return code; };
    // the device copies of the widths may have moved since the scan if the set was used on another device in between
    if ((rc = pwmset_upload(pwms, c->device, c->stream))) return fail(rc);
    const size_t n1 = (size_t) r1->n_hits;

    std::unique_ptr<ms_result> res(new (std::nothrow) ms_result());
    if (!res) { set_error("out of host memory"); return fail(MS_ERR_NOMEM); }
    res->device = r1->device;
    res->P = pwms->P;
    res->R = n_windows;
    res->stats = r1->stats;
    res->motif_offsets.assign((size_t) pwms->P + 1, 0);
    ms_result *raw = res.release();
    auto fail2 = [&](int code) { ms_result_free(raw); return fail(code); };

    // counts, destinations and the prefix sum's work space in ONE pooled block (no hipMalloc / hipFree per span: ADVICE r2)
    uint32_t *d_cnt = nullptr;
    uint64_t *d_dst = nullptr;
    void *wblk = nullptr;
    size_t wgot = 0;
    auto cleanup = [&]() { if (wblk) pool_free(c, wblk, wgot); wblk = nullptr; };
    uint64_t total = 0;
    hipError_t he = hipSuccess;
    (void) hipEventRecord(c->ev[0], c->stream);
    if (counts_only) return sweep_counts_only(c, pwms, r1, raw, span_bases, window, stride, n_windows, out);
    if (n1 > 0) {
        size_t tmp_bytes = 0;
        const size_t n8 = (n1 + 31) & ~(size_t) 31;
        if ((rc = exclusive_sum_u32(nullptr, &tmp_bytes, nullptr, nullptr, n1, c->stream))) return fail2(rc);
        if ((rc = pool_alloc(c, 12 * n8 + tmp_bytes + 256, &wblk, &wgot))) return fail2(rc);
        d_dst = static_cast<uint64_t *>(wblk);
        d_cnt = reinterpret_cast<uint32_t *>(d_dst + n8);
        void *d_tmp = d_cnt + n8;
        rc = launch_sweep_count((int64_t) n1, r1->d_motif_first, r1->P, pwms->d_width, r1->d_pos, window, stride, n_windows,
                                d_cnt, c->stream);
        if (!rc) rc = exclusive_sum_u32(d_tmp, &tmp_bytes, d_cnt, d_dst, n1, c->stream);
        uint32_t last_cnt = 0;
        uint64_t last_dst = 0;
        if (!rc) {
            he = hipMemcpyAsync(&last_cnt, d_cnt + (n1 - 1), 4, hipMemcpyDeviceToHost, c->stream);
            if (he == hipSuccess) he = hipMemcpyAsync(&last_dst, d_dst + (n1 - 1), 8, hipMemcpyDeviceToHost, c->stream);
            if (he == hipSuccess) he = hipStreamSynchronize(c->stream);
            if (he != hipSuccess) { set_error("sweep count failed: %s", hipGetErrorString(he)); rc = MS_ERR_RUNTIME; }
        }
        if (rc) { cleanup(); return fail2(rc); }
        total = last_dst + last_cnt;                          // 64-bit prefix sums: > 2^32 sites per call are fine
    }
    raw->n_hits = (int64_t) total;
    {
        if ((rc = result_block_alloc(c, raw, (size_t) total))) { cleanup(); return fail2(rc); }
        const size_t P1 = (size_t) pwms->P + 1;
        he = hipMemsetAsync(raw->d_region_counts, 0, 8 * P1, c->stream);
        if (he == hipSuccess) he = hipMemsetAsync(raw->d_motif_first, 0xFF, 8 * P1, c->stream);
        if (he != hipSuccess) { cleanup(); set_error("memset failed: %s", hipGetErrorString(he)); return fail2(MS_ERR_RUNTIME); }
    }
    (void) hipEventRecord(c->ev[1], c->stream);
    rc = launch_sweep_scatter((int64_t) n1, r1->d_motif_first, r1->P, pwms->d_width, r1->d_pos, r1->d_score, r1->d_strand, d_dst,
                              window, stride, n_windows, (int64_t) total, raw->d_seq_idx, raw->d_pos, raw->d_score, raw->d_strand,
                              raw->d_motif_first, raw->d_region_counts, c->stream);
    if (rc) { cleanup(); return fail2(rc); }
    (void) hipEventRecord(c->ev[2], c->stream);
    he = hipMemcpyAsync(raw->motif_offsets.data(), raw->d_motif_first, raw->motif_offsets.size() * sizeof(int64_t),
                        hipMemcpyDeviceToHost, c->stream);
    if (he == hipSuccess) he = hipStreamSynchronize(c->stream);
    cleanup();
    if (he != hipSuccess) { set_error("sweep hand-out failed: %s", hipGetErrorString(he)); return fail2(MS_ERR_RUNTIME); }

    // statistics: the span scan's stage times plus the hand-out (counts + prefix sum + scatter, booked under ms_finalize)
    float ms01 = 0, ms12 = 0;
    (void) hipEventElapsedTime(&ms01, c->ev[0], c->ev[1]);
    (void) hipEventElapsedTime(&ms12, c->ev[1], c->ev[2]);
    ms_scan_stats &stt = raw->stats;
    stt.ms_finalize += ms01 + ms12;
    stt.ms_total += ms01 + ms12;
    stt.n_hits = (int64_t) total;
    stt.n_bases = span_bases;                                   // bases scanned (each once)
    stt.n_windows = 0;                                          // unit count of the sweep as the reference sees it
    for (int32_t p = 0; p < pwms->P; p++) stt.n_windows += n_windows * std::max<int64_t>(window - pwms->widths[p] + 1, 0);
    stt.hbm_bytes_algorithmic += 16 * ((int64_t) total - (int64_t) n1);
    ms_result_free(r1);
    *out = raw;
    return MS_OK;
}

}  // namespace ms

using namespace ms;

// configs[4]-style sweep (N3): the windows [begin + k*stride, begin + k*stride + window), k = 0..n_windows-1, of one
// chromosome, with the result the reference gives when every window is a region of its own (scanner.py:71-87 cuts them,
// cscore.c:336-390 scans each) -- but every base is scored ONCE: the span is scanned as one region and each hit is
// handed to all windows that contain it whole (window / stride of them), written straight to its place in the
// reference's order (motif, window, position, strand) -- sweep_scatter_kernel, no second sort.
extern "C" int ms_scan_sweep(const ms_pwmset *pwms_c, const ms_genome *g, int32_t chrom, int64_t begin, int64_t end, int32_t window,
                             int32_t stride, int strand_mask, uint32_t flags, ms_result **out) {
    if (!out) { set_error("out is NULL"); return MS_ERR_INVALID; }
    *out = nullptr;
    if (!pwms_c || !g) { set_error("NULL handle"); return MS_ERR_INVALID; }
    if (strand_mask < 1 || strand_mask > 3) { set_error("invalid strand mask %d (1 '+', 2 '-', 3 both)", strand_mask); return MS_ERR_INVALID; }
    if (flags & ~(uint32_t) MS_SCAN_EXACT_ONLY) { set_error("unknown scan flags 0x%x", flags); return MS_ERR_INVALID; }
    if (window < 1 || stride < 1) { set_error("window and stride must be positive"); return MS_ERR_INVALID; }
    if (begin < 0 || end < begin) { set_error("bad span [%lld, %lld)", (long long) begin, (long long) end); return MS_ERR_INVALID; }
    const int64_t n_windows = end - begin >= window ? (end - begin - window) / stride + 1 : 0;
    const int64_t span_end = n_windows > 0 ? begin + (n_windows - 1) * stride + window : begin;
    ms_pwmset *pwms = const_cast<ms_pwmset *>(pwms_c);
    ms_seqset *span = nullptr;
    int rc = ms_seqset_from_genome(g, &chrom, &begin, &span_end, 1, &span);       // validates chrom / coordinates
    if (rc) return rc;
    DeviceCtx *c;
    if ((rc = get_ctx(span->device, &c))) { ms_seqset_free(span); return rc; }
    // both locks are held across the span scan AND the hand-out: nothing can move the PWM set's device copies in between
    std::lock_guard<std::mutex> lk_dev(c->mu);
    std::lock_guard<std::mutex> lk_pwm(pwms->mu);
    ms_result *r1 = nullptr;
    rc = scan_locked(c, pwms, span, strand_mask, flags, &r1);
    const int64_t span_bases = span->n_bases;
    ms_seqset_free(span);
    if (rc) return rc;
    return sweep_handout_locked(c, pwms, r1, span_bases, window, stride, n_windows, out);
}
