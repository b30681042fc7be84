// ms_pairs.hip -- motif PAIRS over the ordered hit arrays a result already holds in HBM: which motifs have sites in the same regions
// (ms_result_cooccurrence) and at what centre-to-centre distance and relative orientation the sites of an anchor motif and of every
// partner motif lie (ms_result_pair_spacing).  No reference counterpart: the reference hands its hit lists to the caller, and at the
// benchmark's size (10^6 regions x 579 motifs, ~10^8 sites) a motif x motif matrix or a join of one motif's hits with every other
// motif's per region is hours of Python.  Both quantities are exact integer reductions, additive over shards of the regions.
//
//   pair_mark_kernel     has-site bits per (motif, REGION): bits[P][ceil(R / 64)], one atomicOr per hit (rank_mark_kernel of
//                        ms_plotdata.hip without the rank indirection).
//   cooc_kernel          out[a][j] = sum_w popcount(bits[m0 + a][w] & bits[j][w]) as a tiled popcount product: a block owns
//                        kCoTile anchor rows x kCoTile partner rows and walks chunks of kCoWords words staged in LDS; a lane keeps
//                        a 4 x 4 register tile of 32-bit sums (<= R < 2^31), so a staged word is used 4 times per read and the
//                        loop is bound by v_and / v_bcnt, not by LDS or L2.  The word range is cut across blockIdx.z to fill the
//                        device; the partial sums are added with 64-bit integer atomics (integer addition commutes: same bytes
//                        on every run).
//   pair_spacing_kernel  grid y = partner row, x = blocks over chunks of kPairChunk hits of the anchor's slice.  Both slices are
//                        sorted by (region, position), so a block first brackets the partner hits of the REGIONS its chunk covers
//                        (two block-level binary searches); each lane then finds its hit's region inside that bracket (two short
//                        searches: their difference is the hit's term of n_pairs), the first partner position in reach inside the
//                        region (a third), and walks forward while the position is in reach.  Bins go to an LDS histogram of
//                        4 x (2 max_dist + 1) 32-bit counters when that fits kPairLdsBins and the block cannot overflow them
//                        (partner hits x anchor hits of the block < 2^32), flushed once per block with 64-bit global adds; to
//                        global memory directly otherwise.  The bin index is range-checked where it is used.
//   pair_order_kernel    a result made of caller-supplied arrays (ms_result_from_hits) need not be in scan order: one pass over the
//                        slices the call reads sets a flag when (region, position) decreases, and the call then fails.
#include <algorithm>
#include <atomic>
#include <cstring>
#include <mutex>
#include <vector>

#include "ms_handles.h"

namespace ms {
namespace {

constexpr int kMarkThreads = 256;
constexpr int kCoThreads = 256;
constexpr int kCoTile = 64;                        // rows of either operand per block: 16 x 16 lanes, 4 x 4 sums each
constexpr int kCoWords = 32;                       // 64-bit words (2048 regions) staged per step
constexpr int kCoPitch = kCoWords + 1;             // 264 B row pitch: the 16 partner rows of a read fall on 16 distinct bank pairs
constexpr int kPairThreads = 256;
constexpr int kPairChunk = 1024;                   // anchor hits per chunk (4 per lane)
constexpr int kPairMaxBlocksX = 1024;
constexpr int kPairLdsBins = 4093;                 // 2 * max_dist + 1 at most for the LDS histogram: 4 x 4093 counters = 65 488 B, inside the 64 KB a launch gets without asking

// grid: x = blocks over one motif's hit slice, y = motif.  bits [P][nw], zeroed by the caller.
__global__ __launch_bounds__(kMarkThreads) void pair_mark_kernel(const int64_t *__restrict__ motif_first, const int64_t *__restrict__ seq_idx,
                                                                 int64_t nw, unsigned long long *__restrict__ bits) {
    const int m = blockIdx.y;
    const int64_t a = motif_first[m], b = motif_first[m + 1];
    unsigned long long *rb = bits + (size_t) m * nw;
    for (int64_t k = a + (int64_t) blockIdx.x * blockDim.x + threadIdx.x; k < b; k += (int64_t) gridDim.x * blockDim.x) {
        const int64_t r = seq_idx[k];
        atomicOr(&rb[r >> 6], 1ull << (r & 63));
    }
}

// grid: x = partner tiles, y = anchor tiles, z = cuts of the word range (chunks_per_block steps of kCoWords words each).
// out [rows][P], zeroed by the caller.
__global__ __launch_bounds__(kCoThreads) void cooc_kernel(const unsigned long long *__restrict__ bits, int64_t nw, int32_t P, int32_t m0,
                                                          int32_t rows, int64_t chunks_per_block, unsigned long long *__restrict__ out) {
    __shared__ unsigned long long sa[kCoTile * kCoPitch], sb[kCoTile * kCoPitch];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int a_base = blockIdx.y * kCoTile, b_base = blockIdx.x * kCoTile;
    const int64_t n_chunks = (nw + kCoWords - 1) / kCoWords;
    const int64_t ch0 = (int64_t) blockIdx.z * chunks_per_block, ch1 = std::min<int64_t>(ch0 + chunks_per_block, n_chunks);
    uint32_t acc[4][4] = {};
    for (int64_t ch = ch0; ch < ch1; ++ch) {
        const int64_t w0 = ch * kCoWords;
        for (int i = tid; i < kCoTile * kCoWords; i += kCoThreads) {
            const int row = i / kCoWords, w = i % kCoWords;
            const bool in_w = w0 + w < nw;
            const int ar = a_base + row, br = b_base + row;
            sa[row * kCoPitch + w] = in_w && ar < rows ? bits[(size_t) (m0 + ar) * nw + w0 + w] : 0ull;
            sb[row * kCoPitch + w] = in_w && br < P ? bits[(size_t) br * nw + w0 + w] : 0ull;
        }
        __syncthreads();
#pragma unroll 4
        for (int w = 0; w < kCoWords; ++w) {
            unsigned long long a[4], b[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                a[i] = sa[(ty + 16 * i) * kCoPitch + w];
                b[i] = sb[(tx + 16 * i) * kCoPitch + w];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] += (uint32_t) __popcll(a[i] & b[j]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int ar = a_base + ty + 16 * i, bc = b_base + tx + 16 * j;
            if (ar < rows && bc < P && acc[i][j]) atomicAdd(&out[(size_t) ar * P + bc], (unsigned long long) acc[i][j]);
        }
}

// first k in [lo, hi) with key[k] >= v  (key ascending)
__device__ __forceinline__ int64_t lower_bound_i64(const int64_t *__restrict__ key, int64_t lo, int64_t hi, int64_t v) {
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (key[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// first k in [lo, hi) with key[k] > v
__device__ __forceinline__ int64_t upper_bound_i64(const int64_t *__restrict__ key, int64_t lo, int64_t hi, int64_t v) {
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (key[mid] <= v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// grid: x = blocks over the chunks of the anchor's hit slice, y = partner row (motif m0 + y).  dw [rows] = W_partner - W_anchor.
// counts [rows][4][n_bins] (n_bins = 2 * max_dist + 1) and n_pairs [rows], zeroed by the caller.  Dynamic LDS: 16 * n_bins bytes when
// lds_hist, none otherwise.
__global__ __launch_bounds__(kPairThreads) void pair_spacing_kernel(const int64_t *__restrict__ motif_first, const int64_t *__restrict__ seq_idx,
                                                                    const int64_t *__restrict__ pos, const int8_t *__restrict__ strand,
                                                                    int32_t anchor, int32_t m0, const int32_t *__restrict__ dw, int32_t max_dist,
                                                                    int lds_hist, unsigned long long lds_pair_limit,
                                                                    unsigned long long *__restrict__ counts,
                                                                    unsigned long long *__restrict__ n_pairs) {
    extern __shared__ unsigned int h[];
    __shared__ int64_t bracket[2];
    const int row = blockIdx.y, tid = threadIdx.x;
    const int32_t j = m0 + row;
    const int64_t a0 = motif_first[anchor], a1 = motif_first[anchor + 1], j0 = motif_first[j], j1 = motif_first[j + 1];
    const int64_t n_chunks = (a1 - a0 + kPairChunk - 1) / kPairChunk;
    if (j1 == j0 || (int64_t) blockIdx.x >= n_chunks) return;                 // uniform over the block
    const int64_t my_chunks = (n_chunks - blockIdx.x + gridDim.x - 1) / gridDim.x;
    const int n_bins = 2 * max_dist + 1, n_cells = 4 * n_bins;
    // an LDS counter takes at most (partner hits) x (anchor hits of this block) increments
    const bool in_lds = lds_hist && (unsigned long long) (j1 - j0) <= lds_pair_limit / (unsigned long long) (my_chunks * kPairChunk);
    if (in_lds)
        for (int i = tid; i < n_cells; i += kPairThreads) h[i] = 0;
    const int64_t d = dw[row], D2 = 2 * (int64_t) max_dist;
    // |2 * (q - p) + d| <= D2  <=>  lo_off <= q - p <= hi_off
    const int64_t lo_off = -((D2 + d) >> 1), hi_off = (D2 - d) >> 1;
    const bool self = j == anchor;
    unsigned long long *out = counts + (size_t) row * n_cells;
    unsigned long long np = 0;
    for (int64_t ch = blockIdx.x; ch < n_chunks; ch += gridDim.x) {
        const int64_t c0 = a0 + ch * kPairChunk, c1 = std::min<int64_t>(c0 + kPairChunk, a1);
        __syncthreads();                                                      // the LDS zeroing; the previous chunk's readers of bracket[]
        if (tid == 0) bracket[0] = lower_bound_i64(seq_idx, j0, j1, seq_idx[c0]);
        if (tid == 64) bracket[1] = upper_bound_i64(seq_idx, j0, j1, seq_idx[c1 - 1]);
        __syncthreads();
        const int64_t blo = bracket[0], bhi = bracket[1];
        for (int64_t k = c0 + tid; k < c1; k += kPairThreads) {
            const int64_t r = seq_idx[k], p = pos[k];
            const int so = 2 * (strand[k] - 1);
            const int64_t lb = lower_bound_i64(seq_idx, blo, bhi, r), ub = upper_bound_i64(seq_idx, lb, bhi, r);
            np += (unsigned long long) (ub - lb) - (self && ub > lb ? 1ull : 0ull);   // self: [lb, ub) holds hit k itself (in an ordered slice)
            const int64_t q_max = p + hi_off;
            for (int64_t t = lower_bound_i64(pos, lb, ub, p + lo_off); t < ub; ++t) {
                const int64_t q = pos[t];
                if (q > q_max) break;
                if (self && t == k) continue;
                // the bin is checked itself, not inferred from the slice's order: slices that are not in (region, position) order (which
                // pair_order_kernel reports, and the call then fails) must still never address outside the histogram
                const int64_t bin = (2 * (q - p) + d + D2) >> 1;
                if (bin < 0 || bin > D2) continue;
                const int cell = (so + strand[t] - 1) * n_bins + (int) bin;
                if (in_lds) atomicAdd(&h[cell], 1u);
                else atomicAdd(&out[cell], 1ull);
            }
        }
    }
    for (int s = 32; s > 0; s >>= 1) np += __shfl_down(np, s, 64);
    if ((tid & 63) == 0 && np) atomicAdd(&n_pairs[row], np);
    if (!in_lds) return;
    __syncthreads();
    for (int i = tid; i < n_cells; i += kPairThreads)
        if (h[i]) atomicAdd(&out[i], (unsigned long long) h[i]);
}

// grid: x = blocks over one motif's hit slice, y = partner row, the last y the anchor.  *unordered is set when a slice is not in
// (region, position) order -- what a scan writes, and what pair_spacing_kernel's searches rest on.
__global__ __launch_bounds__(kMarkThreads) void pair_order_kernel(const int64_t *__restrict__ motif_first, const int64_t *__restrict__ seq_idx,
                                                                  const int64_t *__restrict__ pos, int32_t anchor, int32_t m0, int32_t rows,
                                                                  unsigned int *__restrict__ unordered) {
    const int32_t m = (int32_t) blockIdx.y < rows ? m0 + (int32_t) blockIdx.y : anchor;
    const int64_t a = motif_first[m], b = motif_first[m + 1];
    for (int64_t k = a + 1 + (int64_t) blockIdx.x * blockDim.x + threadIdx.x; k < b; k += (int64_t) gridDim.x * blockDim.x)
        if (seq_idx[k - 1] > seq_idx[k] || (seq_idx[k - 1] == seq_idx[k] && pos[k - 1] > pos[k])) *unordered = 1u;
}

std::atomic<unsigned long long> g_lds_pair_limit{0xFFFFFFFFull};     // ms_debug_pair_lds_pair_limit

int mark_blocks_per_motif(const std::vector<int64_t> &off, int32_t m0, int32_t m1) {
    int64_t most = 0;
    for (int32_t m = m0; m < m1; ++m) most = std::max<int64_t>(most, off[m + 1] - off[m]);
    return (int) std::max<int64_t>(1, std::min<int64_t>(64, (most + 8 * kMarkThreads - 1) / (8 * kMarkThreads)));
}

const char *kCountsOnly = "a counts-only result (MS_SCAN_COUNTS_ONLY, a counts-only batch or sweep span of a stream) holds the per-motif region counts and site numbers, no site arrays";


}  // namespace
}  // namespace ms

using namespace ms;

extern "C" {

int ms_debug_pair_lds_bins(void) { return kPairLdsBins; }
int ms_debug_cooc_chunk_regions(void) { return 64 * kCoWords; }

int ms_debug_pair_lds_pair_limit(int64_t limit, int64_t *previous) {
    if (limit < 0 || limit > 0xFFFFFFFFLL) { set_error("the limit must be in [0, 2^32 - 1] (0 = the library's own, 2^32 - 1)"); return MS_ERR_INVALID; }
    const unsigned long long old = g_lds_pair_limit.exchange(limit ? (unsigned long long) limit : 0xFFFFFFFFull);
    if (previous) *previous = (int64_t) old;
    return MS_OK;
}

int ms_result_cooccurrence(const ms_result *r, int32_t m0, int32_t m1, int64_t *out) {
    if (!r) { set_error("NULL handle"); return MS_ERR_INVALID; }
    if (r->counts_only) { set_error("%s", kCountsOnly); return MS_ERR_INVALID; }
    if (m0 < 0 || m1 < m0 || m1 > r->P) { set_error("motif range [%d, %d) outside [0, %d)", m0, m1, r->P); return MS_ERR_INVALID; }
    const int64_t R = r->R;
    if (R >= (1LL << 31)) { set_error("at most 2^31 - 1 regions"); return MS_ERR_INVALID; }
    const int32_t rows = m1 - m0, P = r->P;
    if (rows == 0) return MS_OK;
    if (!out) { set_error("NULL output"); return MS_ERR_INVALID; }
    hipPointerAttribute_t attr;
    std::memset(&attr, 0, sizeof(attr));
    const bool out_on_device = hipPointerGetAttributes(&attr, out) == hipSuccess && attr.type == hipMemoryTypeDevice;
    (void) hipGetLastError();                          // a pageable host pointer is "not found" here, which is no error
    if (out_on_device && attr.device != r->device) { set_error("output lives on device %d, the result on device %d", attr.device, r->device); return MS_ERR_INVALID; }
    DeviceCtx *c;
    int rc = get_ctx(r->device, &c);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk_dev(c->mu);
    const int64_t nw = (R + 63) / 64;
    const size_t bits_bytes = 8 * (size_t) P * (size_t) nw, out_bytes = 8 * (size_t) rows * (size_t) P;
    const size_t b_bits = up256(bits_bytes), b_out = out_on_device ? 0 : up256(out_bytes);
    void *blk = nullptr;
    size_t got = 0;
    if ((rc = pool_alloc(c, std::max<size_t>(256, b_bits + b_out), &blk, &got))) return rc;
    char *b = static_cast<char *>(blk);
    unsigned long long *d_bits = reinterpret_cast<unsigned long long *>(b);
    unsigned long long *d_out = out_on_device ? reinterpret_cast<unsigned long long *>(out) : reinterpret_cast<unsigned long long *>(b + b_bits);
    const hipStream_t st = c->stream;
    hipError_t he = hipMemsetAsync(d_out, 0, out_bytes, st);
    if (he == hipSuccess && r->n_hits > 0 && nw > 0) {
        he = hipMemsetAsync(d_bits, 0, bits_bytes, st);
        if (he == hipSuccess) {
            hipLaunchKernelGGL(pair_mark_kernel, dim3(mark_blocks_per_motif(r->motif_offsets, 0, P), P), dim3(kMarkThreads), 0, st, r->d_motif_first,
                               r->d_seq_idx, nw, d_bits);
            he = hipGetLastError();
        }
        if (he == hipSuccess) {
            // enough blocks to fill the device four times over, none with less than one step of kCoWords words
            const int64_t gx = (P + kCoTile - 1) / kCoTile, gy = (rows + kCoTile - 1) / kCoTile, n_chunks = (nw + kCoWords - 1) / kCoWords;
            const int64_t want_z = std::max<int64_t>(1, std::min<int64_t>(n_chunks, (4 * (int64_t) std::max(c->n_cu, 1) + gx * gy - 1) / (gx * gy)));
            const int64_t per = (n_chunks + want_z - 1) / want_z, gz = (n_chunks + per - 1) / per;
            hipLaunchKernelGGL(cooc_kernel, dim3((unsigned) gx, (unsigned) gy, (unsigned) gz), dim3(kCoThreads), 0, st, d_bits, nw, P, m0, rows, per, d_out);
            he = hipGetLastError();
        }
    }
    if (he == hipSuccess && !out_on_device) he = hipMemcpyAsync(out, d_out, out_bytes, hipMemcpyDeviceToHost, st);
    if (he == hipSuccess) he = hipStreamSynchronize(st);
    pool_free(c, blk, got);
    if (he != hipSuccess) { set_error("co-occurrence failed: %s", hipGetErrorString(he)); return MS_ERR_RUNTIME; }
    return MS_OK;
}

int ms_result_pair_spacing(const ms_result *r, const ms_pwmset *pwms, int32_t anchor, int32_t m0, int32_t m1, int32_t max_dist, int64_t *counts,
                           int64_t *n_pairs) {
    if (!r || !pwms) { set_error("NULL handle"); return MS_ERR_INVALID; }
    if (r->counts_only) { set_error("%s", kCountsOnly); return MS_ERR_INVALID; }
    if (pwms->P != r->P) { set_error("result and PWM set disagree on the number of PWMs"); return MS_ERR_INVALID; }
    if (anchor < 0 || anchor >= r->P) { set_error("anchor motif %d outside [0, %d)", anchor, r->P); return MS_ERR_INVALID; }
    if (m0 < 0 || m1 < m0 || m1 > r->P) { set_error("motif range [%d, %d) outside [0, %d)", m0, m1, r->P); return MS_ERR_INVALID; }
    if (max_dist < 0 || max_dist > (1 << 20)) { set_error("max_dist must be in [0, 2^20]"); return MS_ERR_INVALID; }
    const int32_t rows = m1 - m0;
    if (rows == 0) return MS_OK;
    if (!counts || !n_pairs) { set_error("NULL output"); return MS_ERR_INVALID; }
    const int64_t n_bins = 2 * (int64_t) max_dist + 1;
    if ((int64_t) rows * 4 * n_bins > (1LL << 31)) { set_error("%d motifs x 4 x %lld bins is too large", rows, (long long) n_bins); return MS_ERR_INVALID; }
    DeviceCtx *c;
    int rc = get_ctx(r->device, &c);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk_dev(c->mu);
    std::vector<int32_t> dw((size_t) rows);
    for (int32_t i = 0; i < rows; ++i) dw[i] = pwms->widths[m0 + i] - pwms->widths[anchor];
    const size_t cnt_bytes = 8 * (size_t) rows * 4 * (size_t) n_bins, np_bytes = 8 * (size_t) rows, dw_bytes = 4 * (size_t) rows;
    const size_t o_np = up256(cnt_bytes), o_flag = o_np + up256(np_bytes), o_dw = o_flag + 256;
    void *blk = nullptr;
    size_t got = 0;
    if ((rc = pool_alloc(c, o_dw + up256(dw_bytes), &blk, &got))) return rc;
    char *b = static_cast<char *>(blk);
    unsigned long long *d_counts = reinterpret_cast<unsigned long long *>(b);
    unsigned long long *d_np = reinterpret_cast<unsigned long long *>(b + o_np);
    unsigned int *d_unordered = reinterpret_cast<unsigned int *>(b + o_flag);
    int32_t *d_dw = reinterpret_cast<int32_t *>(b + o_dw);
    unsigned int unordered = 0;
    const hipStream_t st = c->stream;
    hipError_t he = hipMemsetAsync(d_counts, 0, o_dw, st);                     // the counts and, behind their padding, n_pairs and the order flag
    if (he == hipSuccess) he = hipMemcpyAsync(d_dw, dw.data(), dw_bytes, hipMemcpyHostToDevice, st);
    const int64_t n_anchor = r->motif_offsets[anchor + 1] - r->motif_offsets[anchor];
    if (he == hipSuccess && n_anchor > 0) {
        hipLaunchKernelGGL(pair_order_kernel, dim3(mark_blocks_per_motif(r->motif_offsets, 0, r->P), rows + 1), dim3(kMarkThreads), 0, st,
                           r->d_motif_first, r->d_seq_idx, r->d_pos, anchor, m0, rows, d_unordered);
        he = hipGetLastError();
    }
    if (he == hipSuccess && n_anchor > 0) {                                    // safe whatever the order check finds: its verdict is read with the outputs
        const bool lds_hist = n_bins <= kPairLdsBins;
        const int64_t gx = std::min<int64_t>(kPairMaxBlocksX, (n_anchor + kPairChunk - 1) / kPairChunk);
        hipLaunchKernelGGL(pair_spacing_kernel, dim3((unsigned) gx, rows), dim3(kPairThreads), lds_hist ? 16 * (size_t) n_bins : 0, st, r->d_motif_first,
                           r->d_seq_idx, r->d_pos, r->d_strand, anchor, m0, d_dw, max_dist, lds_hist ? 1 : 0, g_lds_pair_limit.load(), d_counts, d_np);
        he = hipGetLastError();
    }
    if (he == hipSuccess) he = hipMemcpyAsync(counts, d_counts, cnt_bytes, hipMemcpyDeviceToHost, st);
    if (he == hipSuccess) he = hipMemcpyAsync(n_pairs, d_np, np_bytes, hipMemcpyDeviceToHost, st);
    if (he == hipSuccess) he = hipMemcpyAsync(&unordered, d_unordered, sizeof(unordered), hipMemcpyDeviceToHost, st);
    if (he == hipSuccess) he = hipStreamSynchronize(st);
    pool_free(c, blk, got);
    if (he != hipSuccess) { set_error("pair spacing failed: %s", hipGetErrorString(he)); return MS_ERR_RUNTIME; }
    if (unordered) {
        std::memset(counts, 0, cnt_bytes);
        std::memset(n_pairs, 0, np_bytes);
        set_error("the sites of the anchor or of a partner motif are not in (region, position) order: pair spacing needs a result in scan order");
        return MS_ERR_INVALID;
    }
    return MS_OK;
}

}  // extern "C"
