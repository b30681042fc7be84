// ms_plotdata.hip -- the numbers under `motifscan scan --plot-dist` (motifscan/plot.py:43-153), computed next to the hits.
//
// plot_motif_sites_dist (plot.py:43-92) histograms, per motif, the distance of every site centre to its region's summit in bins
// of 10 bp; plot_motif_sites_enrich (plot.py:95-153) ranks the regions by score and, for every rank, takes the fraction of the
// 2 * (R / 100) neighbouring ranks whose region holds a site -- a Python slice sum per rank, O(P x R^2 / 50) element visits.
// Here both are reductions over the de-duplicated hit arrays a result already holds in HBM:
//
//   site_hist_kernel     one LDS histogram per block over a slice of one motif's hits, then one global add per non-empty bin.
//                        The bin comes from 2 * d = 2 * (pos - summit_rel) + W in integers: no floating point, exact by construction.
//   rank_mark_kernel     has-site bits per (motif, RANK): hit -> region -> its rank (the inverse of the caller's order) -> one bit.
//   rank_prefix_kernel   per motif row, the exclusive prefix count of those bits per 64-bit word, so that the number of ranks with a
//                        site in [0, k) is prefix[k >> 6] + popcount(bits[k >> 6] below bit k & 63).
//   rank_profile_kernel  per rank: ratio_input = count / (tail - head), then / ratio_control -- two IEEE fp64 divisions in the
//                        reference's order -- staged in LDS with a 5-rank halo each side, reflected at the ends (plot.py:34-40's
//                        r_[...] padding done by index arithmetic), and smoothed with the 11 weights the caller passes.
// The profile is write-bound: (m1 - m0) x R doubles out, everything it reads (bits and prefix words: 12 B per 64 ranks) sits in L2.
#include <algorithm>
#include <cstring>
#include <mutex>
#include <vector>

#include "ms_handles.h"

namespace ms {
namespace {

constexpr int kHistThreads = 256;
constexpr int kHistLdsBins = 4096;                 // 16 KB of LDS counters; wider histograms add to global memory directly
constexpr int kScanThreads = 1024;                 // rank_prefix_kernel: one block per motif row
constexpr int kProfThreads = 256;
constexpr int kProfPerThread = 4;
constexpr int kProfTile = kProfThreads * kProfPerThread;
constexpr int kHalf = 5;                           // smoothing window 11 = 2 * kHalf + 1
constexpr int kHistHitsPerBlock = 8 * kHistThreads;  // hist_blocks_per_motif: one block per this many hits of the fullest motif (8 trips of its loop) ...
constexpr int kHistMaxBlocks = 64;                 // ... up to this many; beyond them the grid stays and the grid-stride loops run longer

// grid: x = blocks over one motif's hit slice, y = motif row (motif m0 + y).  counts [rows][n_bins], zeroed by the caller.
__global__ __launch_bounds__(kHistThreads) void site_hist_kernel(const int64_t *__restrict__ motif_first, int32_t m0,
                                                                 const int64_t *__restrict__ seq_idx, const int64_t *__restrict__ pos,
                                                                 const int32_t *__restrict__ width, const int64_t *__restrict__ summit_rel,
                                                                 int64_t edge0_x2, int32_t n_bins, unsigned long long *__restrict__ counts) {
    __shared__ unsigned int h[kHistLdsBins];
    const int row = blockIdx.y;
    const int64_t a = motif_first[m0 + row], b = motif_first[m0 + row + 1];
    const bool in_lds = n_bins <= kHistLdsBins;
    if (in_lds)
        for (int i = threadIdx.x; i < n_bins; i += blockDim.x) h[i] = 0;
    __syncthreads();
    const int64_t W = width[row];
    unsigned long long *out = counts + (size_t) row * n_bins;
    for (int64_t k = a + (int64_t) blockIdx.x * blockDim.x + threadIdx.x; k < b; k += (int64_t) gridDim.x * blockDim.x) {
        // 2 * (d - edge0); the edges are 10 apart, 20 in these units.  np.histogram: edge[i] <= d < edge[i + 1], the last bin closed.
        const int64_t t = 2 * (pos[k] - summit_rel[seq_idx[k]]) + W - edge0_x2;
        if (t < 0) continue;
        int64_t bin = t / 20;
        if (bin >= n_bins) {
            if (bin != n_bins || t % 20 != 0) continue;
            bin = n_bins - 1;
        }
        if (in_lds) atomicAdd(&h[bin], 1u);
        else atomicAdd(&out[bin], 1ull);
    }
    if (!in_lds) return;
    __syncthreads();
    for (int i = threadIdx.x; i < n_bins; i += blockDim.x)
        if (h[i]) atomicAdd(&out[i], (unsigned long long) h[i]);
}

// grid: x = blocks over one motif's hit slice, y = motif row.  bits [rows][nw + 1], zeroed by the caller; inv_rank [R]: region -> rank.
__global__ __launch_bounds__(kHistThreads) void rank_mark_kernel(const int64_t *__restrict__ motif_first, int32_t m0,
                                                                 const int64_t *__restrict__ seq_idx, const int32_t *__restrict__ inv_rank,
                                                                 int64_t nw1, unsigned long long *__restrict__ bits) {
    const int row = blockIdx.y;
    const int64_t a = motif_first[m0 + row], b = motif_first[m0 + row + 1];
    unsigned long long *rb = bits + (size_t) row * nw1;
    for (int64_t k = a + (int64_t) blockIdx.x * blockDim.x + threadIdx.x; k < b; k += (int64_t) gridDim.x * blockDim.x) {
        const int32_t r = inv_rank[seq_idx[k]];
        atomicOr(&rb[r >> 6], 1ull << (r & 63));
    }
}

// One block per motif row: prefix[w] = set bits in words [0, w), for w = 0 .. nw (prefix[nw] = the row's total).
__global__ __launch_bounds__(kScanThreads) void rank_prefix_kernel(const unsigned long long *__restrict__ bits, int64_t nw,
                                                                   uint32_t *__restrict__ prefix) {
    __shared__ uint32_t wave_sum[kScanThreads / 64];
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned long long *rb = bits + (size_t) row * (nw + 1);
    uint32_t *rp = prefix + (size_t) row * (nw + 1);
    const int64_t per = (nw + kScanThreads - 1) / kScanThreads;
    const int64_t lo = std::min<int64_t>(nw, tid * per), hi = std::min<int64_t>(nw, lo + per);
    uint32_t own = 0;
    for (int64_t w = lo; w < hi; ++w) own += (uint32_t) __popcll(rb[w]);
    // exclusive scan of `own` over the block: within the wave by shuffles, then over the 16 wave totals
    uint32_t incl = own;
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t v = __shfl_up(incl, d, 64);
        if (lane >= d) incl += v;
    }
    if (lane == 63) wave_sum[wave] = incl;
    __syncthreads();
    uint32_t base = 0;
    for (int i = 0; i < wave; ++i) base += wave_sum[i];
    uint32_t run = base + incl - own;
    for (int64_t w = lo; w < hi; ++w) {
        rp[w] = run;
        run += (uint32_t) __popcll(rb[w]);
    }
    if (tid == kScanThreads - 1) rp[nw] = run;          // the last thread's range ends at nw (or is empty and starts there)
}

__device__ __forceinline__ uint32_t ranks_with_site_below(const unsigned long long *rb, const uint32_t *rp, int64_t k) {
    const int64_t w = k >> 6;
    const int s = (int) (k & 63);
    return rp[w] + (s ? (uint32_t) __popcll(rb[w] & ((1ull << s) - 1ull)) : 0u);
}

// plot.py:135-140 for rank t (reflected into [0, R) first: plot.py:36's padding), one row
__device__ __forceinline__ double rank_ratio(const unsigned long long *rb, const uint32_t *rp, int64_t R, int64_t f, double ratio_control,
                                             int64_t t) {
    if (t < 0) t = -t;
    else if (t >= R) t = 2 * R - 2 - t;
    const int64_t head = t - f > 0 ? t - f : 0;
    const int64_t tail = t + f < R ? t + f : R;
    const uint32_t n = ranks_with_site_below(rb, rp, tail) - ranks_with_site_below(rb, rp, head);
    const double ratio_input = (double) n / (double) (tail - head);
    return ratio_input / ratio_control;
}

// grid: x = tiles of kProfTile ranks, y = motif row.  out [rows][R].  smooth: 11 weights, out[i] = sum_j kernel[j] * ratio[i - 5 + j].
__global__ __launch_bounds__(kProfThreads) void rank_profile_kernel(const unsigned long long *__restrict__ bits, const uint32_t *__restrict__ prefix,
                                                                    int64_t nw1, int64_t R, int64_t f, const double *__restrict__ ratio_control,
                                                                    const double *__restrict__ kernel, int smooth, double *__restrict__ out) {
    __shared__ double raw[kProfTile + 2 * kHalf];
    __shared__ double kw[2 * kHalf + 1];
    const int row = blockIdx.y;
    const unsigned long long *rb = bits + (size_t) row * nw1;
    const uint32_t *rp = prefix + (size_t) row * nw1;
    const double rc = ratio_control[row];
    const int64_t i0 = (int64_t) blockIdx.x * kProfTile;
    double *orow = out + (size_t) row * R;
    if (!smooth) {
        for (int j = threadIdx.x; j < kProfTile; j += kProfThreads) {
            const int64_t i = i0 + j;
            if (i < R) orow[i] = rank_ratio(rb, rp, R, f, rc, i);
        }
        return;
    }
    if (threadIdx.x < 2 * kHalf + 1) kw[threadIdx.x] = kernel[threadIdx.x];
    const int64_t n_here = std::min<int64_t>(kProfTile, R - i0);
    for (int j = threadIdx.x; j < n_here + 2 * kHalf; j += kProfThreads) raw[j] = rank_ratio(rb, rp, R, f, rc, i0 - kHalf + j);
    __syncthreads();
    for (int j = threadIdx.x; j < n_here; j += kProfThreads) {
        double y = 0.0;
        for (int q = 0; q < 2 * kHalf + 1; ++q) y += kw[q] * raw[j + q];
        orow[i0 + j] = y;
    }
}

int hist_blocks_per_motif(const std::vector<int64_t> &off, int32_t m0, int32_t m1) {
    int64_t most = 0;
    for (int32_t m = m0; m < m1; ++m) most = std::max<int64_t>(most, off[m + 1] - off[m]);
    return (int) std::max<int64_t>(1, std::min<int64_t>(kHistMaxBlocks, (most + kHistHitsPerBlock - 1) / kHistHitsPerBlock));
}

const char *kCountsOnly = "a counts-only result (MS_SCAN_COUNTS_ONLY, a counts-only batch or sweep span of a stream) holds the per-motif region counts and site numbers, no site arrays";

}  // namespace
}  // namespace ms

using namespace ms;

extern "C" {

int ms_debug_plot_dims(int32_t out[6]) {
    if (!out) { set_error("NULL output"); return MS_ERR_INVALID; }
    const int32_t dims[6] = {kHistLdsBins, kHistHitsPerBlock, kHistMaxBlocks, kScanThreads, kProfTile, kHalf};
    std::memcpy(out, dims, sizeof(dims));
    return MS_OK;
}

int ms_result_from_hits(int32_t n_pwms, int64_t n_regions, const int64_t *motif_offsets, const int64_t *seq_idx, const int64_t *pos,
                        const double *score, const int8_t *strand, ms_result **out) {
    if (!out || !motif_offsets || n_pwms < 0 || n_regions < 0) { set_error("NULL or negative argument"); return MS_ERR_INVALID; }
    *out = nullptr;
    if (motif_offsets[0] != 0) { set_error("motif_offsets[0] must be 0"); return MS_ERR_INVALID; }
    for (int32_t m = 0; m < n_pwms; ++m)
        if (motif_offsets[m + 1] < motif_offsets[m]) { set_error("motif_offsets must not decrease"); return MS_ERR_INVALID; }
    const int64_t n = motif_offsets[n_pwms];
    if (n > 0 && (!seq_idx || !pos || !score || !strand)) { set_error("NULL hit array"); return MS_ERR_INVALID; }
    // every region index is checked here: the plot kernels index per-region arrays with it
    std::vector<int64_t> counts((size_t) n_pwms, 0), seen((size_t) n_regions, -1);
    for (int32_t m = 0; m < n_pwms; ++m)
        for (int64_t k = motif_offsets[m]; k < motif_offsets[m + 1]; ++k) {
            if (seq_idx[k] < 0 || seq_idx[k] >= n_regions) { set_error("hit %lld: region %lld outside [0, %lld)", (long long) k, (long long) seq_idx[k], (long long) n_regions); return MS_ERR_INVALID; }
            if (strand[k] != 1 && strand[k] != 2) { set_error("hit %lld: strand must be 1 or 2", (long long) k); return MS_ERR_INVALID; }
            if (seen[seq_idx[k]] != m) { seen[seq_idx[k]] = m; ++counts[m]; }
        }
    DeviceCtx *c;
    int rc = get_ctx(current_device(), &c);
    if (rc) return rc;
    ms_result *r = new (std::nothrow) ms_result();
    if (!r) { set_error("out of host memory"); return MS_ERR_NOMEM; }
    r->device = c->device;
    r->P = n_pwms;
    r->R = n_regions;
    r->n_hits = n;
    r->motif_offsets.assign(motif_offsets, motif_offsets + n_pwms + 1);
    size_t got = 0;
    if ((rc = pool_alloc(c, result_block_bytes(n_pwms, (size_t) n), &r->block, &got))) { delete r; return rc; }
    r->block_bytes = got;
    result_carve(r, r->block, (size_t) n);
    const size_t P1 = (size_t) n_pwms + 1;
    hipError_t he = hipMemcpy(r->d_region_counts, counts.data(), 8 * (size_t) n_pwms, hipMemcpyHostToDevice);
    if (he == hipSuccess) he = hipMemcpy(r->d_motif_first, motif_offsets, 8 * P1, hipMemcpyHostToDevice);
    if (n > 0) {
        if (he == hipSuccess) he = hipMemcpy(r->d_seq_idx, seq_idx, 8 * (size_t) n, hipMemcpyHostToDevice);
        if (he == hipSuccess) he = hipMemcpy(r->d_pos, pos, 8 * (size_t) n, hipMemcpyHostToDevice);
        if (he == hipSuccess) he = hipMemcpy(r->d_score, score, 8 * (size_t) n, hipMemcpyHostToDevice);
        if (he == hipSuccess) he = hipMemcpy(r->d_strand, strand, (size_t) n, hipMemcpyHostToDevice);
    }
    if (he != hipSuccess) { set_error("upload of the hit arrays failed: %s", hipGetErrorString(he)); ms_result_free(r); return MS_ERR_RUNTIME; }
    r->stats.n_hits = n;
    r->stats.n_pwms = n_pwms;
    *out = r;
    return MS_OK;
}

int ms_result_site_histogram(const ms_result *r, const ms_pwmset *pwms, const int64_t *summit_rel, int64_t extend, int32_t m0, int32_t m1,
                             int64_t *counts, int64_t *n_sites) {
    if (!r || !pwms) { set_error("NULL handle"); return MS_ERR_INVALID; }
    if (r->counts_only) { set_error("%s", kCountsOnly); return MS_ERR_INVALID; }
    if (pwms->P != r->P) { set_error("result and PWM set disagree on the number of PWMs"); return MS_ERR_INVALID; }
    if (m0 < 0 || m1 < m0 || m1 > r->P) { set_error("motif range [%d, %d) outside [0, %d)", m0, m1, r->P); return MS_ERR_INVALID; }
    if (extend < 0 || extend > (1LL << 40)) { set_error("extend must be in [0, 2^40]"); return MS_ERR_INVALID; }
    if (r->R > 0 && !summit_rel) { set_error("NULL summit_rel"); return MS_ERR_INVALID; }
    const int64_t n_bins = (2 * extend + 11 + 9) / 10 - 1;      // len(np.arange(-extend - 5, extend + 6, 10)) - 1
    const int32_t rows = m1 - m0;
    if (rows == 0) return MS_OK;
    if (!counts || !n_sites) { set_error("NULL output"); return MS_ERR_INVALID; }
    if (n_bins > (1LL << 24) || (int64_t) rows * n_bins > (1LL << 31)) { set_error("%lld bins x %d motifs is too large", (long long) n_bins, rows); return MS_ERR_INVALID; }
    for (int32_t m = m0; m < m1; ++m) n_sites[m - m0] = r->motif_offsets[m + 1] - r->motif_offsets[m];
    DeviceCtx *c;
    int rc = get_ctx(r->device, &c);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk_dev(c->mu);
    const size_t cnt_bytes = 8 * (size_t) rows * n_bins, sum_bytes = 8 * (size_t) r->R, w_bytes = 4 * (size_t) rows;
    const size_t o_sum = (cnt_bytes + 255) & ~(size_t) 255, o_w = o_sum + ((sum_bytes + 255) & ~(size_t) 255);
    void *blk = nullptr;
    size_t got = 0;
    if ((rc = pool_alloc(c, o_w + w_bytes, &blk, &got))) return rc;
    char *b = static_cast<char *>(blk);
    unsigned long long *d_counts = reinterpret_cast<unsigned long long *>(b);
    int64_t *d_summit = reinterpret_cast<int64_t *>(b + o_sum);
    int32_t *d_width = reinterpret_cast<int32_t *>(b + o_w);
    const hipStream_t st = c->stream;
    hipError_t he = hipMemsetAsync(d_counts, 0, cnt_bytes, st);
    if (he == hipSuccess && sum_bytes) he = hipMemcpyAsync(d_summit, summit_rel, sum_bytes, hipMemcpyHostToDevice, st);
    if (he == hipSuccess) he = hipMemcpyAsync(d_width, pwms->widths.data() + m0, w_bytes, hipMemcpyHostToDevice, st);
    if (he == hipSuccess && r->n_hits > 0) {
        dim3 grid(hist_blocks_per_motif(r->motif_offsets, m0, m1), rows);
        hipLaunchKernelGGL(site_hist_kernel, grid, dim3(kHistThreads), 0, st, r->d_motif_first, m0, r->d_seq_idx, r->d_pos, d_width, d_summit,
                           2 * (-extend - 5), (int32_t) n_bins, d_counts);
        he = hipGetLastError();
    }
    if (he == hipSuccess) he = hipMemcpyAsync(counts, d_counts, cnt_bytes, hipMemcpyDeviceToHost, st);
    if (he == hipSuccess) he = hipStreamSynchronize(st);
    pool_free(c, blk, got);
    if (he != hipSuccess) { set_error("site histogram failed: %s", hipGetErrorString(he)); return MS_ERR_RUNTIME; }
    return MS_OK;
}

int ms_result_rank_profile(const ms_result *r, const int64_t *rank_order, const double *ratio_control, const double *kernel, int32_t m0,
                           int32_t m1, int flags, double *out) {
    if (!r) { set_error("NULL handle"); return MS_ERR_INVALID; }
    if (r->counts_only) { set_error("%s", kCountsOnly); return MS_ERR_INVALID; }
    if (m0 < 0 || m1 < m0 || m1 > r->P) { set_error("motif range [%d, %d) outside [0, %d)", m0, m1, r->P); return MS_ERR_INVALID; }
    if (flags & ~MS_PROFILE_UNSMOOTHED) { set_error("unknown flags 0x%x", flags); return MS_ERR_INVALID; }
    const int64_t R = r->R, f = R / 100;
    if (f == 0) { set_error("%lld regions: the window 2 * (R / 100) is empty (plot.py:138 divides by zero for R < 100)", (long long) R); return MS_ERR_INVALID; }
    if (R >= (1LL << 31)) { set_error("at most 2^31 - 1 regions"); return MS_ERR_INVALID; }
    const bool smooth = !(flags & MS_PROFILE_UNSMOOTHED) && R > 2 * kHalf + 1;       // plot.py:35: len(x) <= 11 is returned as it is
    const int32_t rows = m1 - m0;
    if (!rank_order || !ratio_control || (smooth && !kernel)) { set_error("NULL argument"); return MS_ERR_INVALID; }
    if (rows == 0) return MS_OK;
    if (!out) { set_error("NULL output"); return MS_ERR_INVALID; }
    for (int32_t i = 0; i < rows; ++i)
        if (!(ratio_control[i] > 0.0)) { set_error("ratio_control[%d] must be > 0 (plot.py:130-132 replaces 0 by 1)", i); return MS_ERR_INVALID; }
    // the order must be a permutation of [0, R): its inverse addresses the bit rows
    std::vector<int32_t> inv((size_t) R, -1);
    for (int64_t k = 0; k < R; ++k) {
        const int64_t g = rank_order[k];
        if (g < 0 || g >= R || inv[g] >= 0) { set_error("rank_order is not a permutation of [0, %lld) (entry %lld)", (long long) R, (long long) k); return MS_ERR_INVALID; }
        inv[g] = (int32_t) k;
    }
    hipPointerAttribute_t attr;
    std::memset(&attr, 0, sizeof(attr));
    const bool out_on_device = hipPointerGetAttributes(&attr, out) == hipSuccess && attr.type == hipMemoryTypeDevice;
    (void) hipGetLastError();                          // a pageable host pointer is "not found" here, which is no error
    if (out_on_device && attr.device != r->device) { set_error("output lives on device %d, the result on device %d", attr.device, r->device); return MS_ERR_INVALID; }
    DeviceCtx *c;
    int rc = get_ctx(r->device, &c);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk_dev(c->mu);
    const int64_t nw = (R + 63) / 64, nw1 = nw + 1;
    auto up = [](size_t x) { return (x + 255) & ~(size_t) 255; };
    const size_t b_bits = up(8 * (size_t) rows * nw1), b_pre = up(4 * (size_t) rows * nw1), b_inv = up(4 * (size_t) R), b_rc = up(8 * (size_t) rows),
                 b_k = up(8 * 11), b_out = out_on_device ? 0 : 8 * (size_t) rows * (size_t) R;
    void *blk = nullptr;
    size_t got = 0;
    if ((rc = pool_alloc(c, b_bits + b_pre + b_inv + b_rc + b_k + b_out, &blk, &got))) return rc;
    char *b = static_cast<char *>(blk);
    unsigned long long *d_bits = reinterpret_cast<unsigned long long *>(b);
    uint32_t *d_pre = reinterpret_cast<uint32_t *>(b + b_bits);
    int32_t *d_inv = reinterpret_cast<int32_t *>(b + b_bits + b_pre);
    double *d_rc = reinterpret_cast<double *>(b + b_bits + b_pre + b_inv);
    double *d_k = reinterpret_cast<double *>(b + b_bits + b_pre + b_inv + b_rc);
    double *d_out = out_on_device ? out : reinterpret_cast<double *>(b + b_bits + b_pre + b_inv + b_rc + b_k);
    const hipStream_t st = c->stream;
    hipError_t he = hipMemsetAsync(d_bits, 0, 8 * (size_t) rows * nw1, st);
    if (he == hipSuccess) he = hipMemcpyAsync(d_inv, inv.data(), 4 * (size_t) R, hipMemcpyHostToDevice, st);
    if (he == hipSuccess) he = hipMemcpyAsync(d_rc, ratio_control, 8 * (size_t) rows, hipMemcpyHostToDevice, st);
    if (he == hipSuccess && smooth) he = hipMemcpyAsync(d_k, kernel, 8 * 11, hipMemcpyHostToDevice, st);
    if (he == hipSuccess && r->n_hits > 0) {
        hipLaunchKernelGGL(rank_mark_kernel, dim3(hist_blocks_per_motif(r->motif_offsets, m0, m1), rows), dim3(kHistThreads), 0, st,
                           r->d_motif_first, m0, r->d_seq_idx, d_inv, nw1, d_bits);
        he = hipGetLastError();
    }
    if (he == hipSuccess) {
        hipLaunchKernelGGL(rank_prefix_kernel, dim3(rows), dim3(kScanThreads), 0, st, d_bits, nw, d_pre);
        he = hipGetLastError();
    }
    if (he == hipSuccess) {
        hipLaunchKernelGGL(rank_profile_kernel, dim3((unsigned) ((R + kProfTile - 1) / kProfTile), rows), dim3(kProfThreads), 0, st, d_bits, d_pre,
                           nw1, R, f, d_rc, d_k, smooth ? 1 : 0, d_out);
        he = hipGetLastError();
    }
    if (he == hipSuccess && !out_on_device) he = hipMemcpyAsync(out, d_out, 8 * (size_t) rows * (size_t) R, hipMemcpyDeviceToHost, st);
    if (he == hipSuccess) he = hipStreamSynchronize(st);
    pool_free(c, blk, got);
    if (he != hipSuccess) { set_error("rank profile failed: %s", hipGetErrorString(he)); return MS_ERR_RUNTIME; }
    return MS_OK;
}

}  // extern "C"
