// ms_ranksum.hip -- cutoff-free enrichment over best-site matrices that stay on the device (ms_best_rank_sum, ms_best_count_passing): the
// consumer of ms_scan_best's [P][R] score matrix.  Both results are exact integers; z and P-values are host arithmetic on them (enrich.py).
// The rank sums read nothing of a handle but one [P][R] plane of doubles per group: rank_sum_planes is their body, and ms_affinity_rank_sum
// (ms_affinity.hip) calls it with the log_mean planes of two affinity results.
//
// Order of cell values (both calls): a cell without a winner (score NaN) ranks below every number and ties with every other such cell;
// numbers compare as IEEE doubles (-0.0 == +0.0).  rs_gather_kernel turns a cell into an order-preserving 64-bit key: 0 for NaN (by
// isnan, not by bit pattern), else the sign flip of the bits with -0.0 made +0.0 first -- every number, -inf included, maps above 0.
//
// ms_best_rank_sum, per motif row, x over group A (na cells), y over group B (nb cells):
//     u2   = 2 #{x > y} + #{x == y}                    (twice the Mann-Whitney U of A; < 2^63 because na, nb < 2^31)
//     ties = sum over the tie groups of the pooled sample of t^3 - t        (128 bits)
// Motif rows go in batches of max(1, budget / (na + nb)).  Per batch: gather both groups' keys (coalesced along the region axis; a
// selection is an index list made once per call on the host), sort every row of either group (rocPRIM, ms_sort.hip: one segmented radix
// sort per batch for a group of up to kRsSegmentedMax cells, one device radix sort per row for a larger one), then rs_rank_kernel:
// one thread per element e of either sorted row finds the run of keys equal to e's in its own row and in the other group's row -- bounded
// binary searches of exactly ceil(log2(n + 1)) steps, every index inside [0, n]; an element whose neighbours differ skips the search of
// its own row, one whose key is absent from the other row the second search there -- and adds, from A's elements, 2 lower + (upper - lower)
// to u2 and, from all elements, t^2 - 1 (t = the pooled run) to ties: over a run that is t^3 - t.  t^2 - 1 < 2^64 is carried as two sums,
// of its low and of its high 32 bits: neither can overflow 64 bits over fewer than 2^32 elements.  Wave reduction (64 lanes), block
// reduction through LDS, one slot per (row, block); rs_fold_kernel adds a row's slots, the host puts the two tie sums together in 128 bits.
// Integer adds in fixed slots: the same bytes on every run and for every batch size.  No atomics, no floating point after the gather.
//
// ms_best_count_passing: counts[row][k] = #{selected r: score - cutoff[row][k] >= -1e-10}, ms_scan's hit rule (ms_fp64.hip) applied to
// the best score.  One pass over the cells, per cutoff a ballot + popcount per wave, one 64-bit integer add per block and cutoff.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "ms_handles.h"

namespace ms {

namespace {

constexpr int kRsThreads = 256;
constexpr int kRsWaves = kRsThreads / 64;
constexpr int kRsGatherElems = 4 * kRsThreads;          // cells per block of rs_gather_kernel
constexpr int kRsRankElems = 2 * kRsThreads;            // sorted elements per block of rs_rank_kernel
constexpr int kRsCountItems = 8;
constexpr int kRsCountElems = kRsCountItems * kRsThreads;   // cells per block of rs_count_kernel
constexpr int kRsCutChunk = 64;                         // cutoffs counted between two flushes of a block's LDS counters
constexpr int kRsGridY = 32768;
// A group of up to this many cells is sorted with ONE segmented radix sort per batch, a larger one with one device radix sort per row.
// Measured with 579 rows and na = nb = n (profiles/r12_ranksum_time*.json, the whole call, per row / segmented): n = 10 000: 38.1 / 1.3 ms;
// 100 000: 72.9 / 14.4; 250 000: 134.4 / 69.1; 500 000: 184.9 / 196.8; 1 000 000: 274.4 / 658.2.  A device sort costs launches -- below
// ~10^5 keys nothing else --, a segment is sorted by one block: the forms cross near 480 000; the switch sits at the last size measured
// at which the segmented form wins clearly.
constexpr uint32_t kRsSegmentedMax = 1u << 18;
constexpr int64_t kRsBudget = 1LL << 27;                // keys of both groups held at once (16 bytes each: unsorted + sorted), as ms_score_ranks
std::atomic<int64_t> g_rs_budget{0};                    // ms_debug_ranksum_budget: 0 = kRsBudget

__device__ __forceinline__ uint64_t order_key(double s) {
    if (isnan(s)) return 0ull;
    if (s == 0.0) s = 0.0;                               // -0.0 -> +0.0
    const uint64_t b = (uint64_t) __double_as_longlong(s);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

// grid = (ceil(n / kRsGatherElems), rows): keys[row][i] = key of score[m_first + row][idx ? idx[i] : i]
__global__ void __launch_bounds__(kRsThreads) rs_gather_kernel(const double *__restrict__ score, int64_t R, int32_t m_first, const int32_t *__restrict__ idx, uint32_t n,
                                                               uint64_t *__restrict__ keys, int32_t row0) {
    const int64_t row = (int64_t) row0 + blockIdx.y;
    const double *__restrict__ src = score + ((int64_t) m_first + row) * R;
    uint64_t *__restrict__ dst = keys + row * (int64_t) n;
    const uint32_t base = blockIdx.x * (uint32_t) kRsGatherElems + threadIdx.x;
#pragma unroll
    for (int j = 0; j < kRsGatherElems / kRsThreads; j++) {
        const uint32_t i = base + (uint32_t) j * kRsThreads;
        if (i < n) dst[i] = order_key(src[idx ? (uint32_t) idx[i] : i]);
    }
}

// first index in [0, n] whose key is >= k (UPPER: > k); exactly `steps` >= ceil(log2(n + 1)) steps, mid < n whenever it is read
template <bool UPPER>
__device__ __forceinline__ uint32_t rs_bound(const uint64_t *__restrict__ v, uint32_t n, int steps, uint64_t k) {
    uint32_t lo = 0, hi = n;
    for (int s = 0; s < steps; s++) {
        if (lo < hi) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            const uint64_t x = v[mid];
            const bool right = UPPER ? x <= k : x < k;
            lo = right ? mid + 1 : lo;
            hi = right ? hi : mid;
        }
    }
    return lo;
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

struct RankArgs {
    const uint64_t *a, *b;                               // sorted keys [rows][na], [rows][nb]
    uint32_t na, nb;
    int steps_a, steps_b;
    uint32_t blocks_a, blocks;                           // blocks over A's elements; over both groups'
    unsigned long long *part;                            // [rows][blocks][3]: u2, low and high 32-bit halves of t^2 - 1 summed
};

// grid = (blocks, rows)
__global__ void __launch_bounds__(kRsThreads) rs_rank_kernel(const RankArgs A, int32_t row0) {
    __shared__ unsigned long long red[kRsWaves][3];
    const int64_t row = (int64_t) row0 + blockIdx.y;
    const bool is_a = blockIdx.x < A.blocks_a;
    const uint32_t blk = is_a ? blockIdx.x : blockIdx.x - A.blocks_a;
    const uint64_t *__restrict__ own = is_a ? A.a + row * (int64_t) A.na : A.b + row * (int64_t) A.nb;
    const uint64_t *__restrict__ oth = is_a ? A.b + row * (int64_t) A.nb : A.a + row * (int64_t) A.na;
    const uint32_t n_own = is_a ? A.na : A.nb, n_oth = is_a ? A.nb : A.na;
    const int st_own = is_a ? A.steps_a : A.steps_b, st_oth = is_a ? A.steps_b : A.steps_a;
    unsigned long long u2 = 0, t_lo = 0, t_hi = 0;
#pragma unroll
    for (int j = 0; j < kRsRankElems / kRsThreads; j++) {
        const uint32_t i = blk * (uint32_t) kRsRankElems + (uint32_t) j * kRsThreads + threadIdx.x;
        if (i >= n_own) continue;
        const uint64_t k = own[i];
        const uint32_t lo_o = rs_bound<false>(oth, n_oth, st_oth, k);
        const uint32_t up_o = (lo_o < n_oth && oth[lo_o] == k) ? rs_bound<true>(oth, n_oth, st_oth, k) : lo_o;
        const uint32_t lo_s = (i > 0 && own[i - 1] == k) ? rs_bound<false>(own, n_own, st_own, k) : i;
        const uint32_t up_s = (i + 1 < n_own && own[i + 1] == k) ? rs_bound<true>(own, n_own, st_own, k) : i + 1;
        if (is_a) u2 += 2ull * lo_o + (up_o - lo_o);
        const unsigned long long t = (unsigned long long) (up_o - lo_o) + (up_s - lo_s);       // >= 1, < 2^32
        const unsigned long long v = t * t - 1ull;
        t_lo += v & 0xFFFFFFFFull;
        t_hi += v >> 32;
    }
    u2 = wave_sum(u2); t_lo = wave_sum(t_lo); t_hi = wave_sum(t_hi);
    const int wave = (int) (threadIdx.x >> 6);
    if ((threadIdx.x & 63u) == 0) { red[wave][0] = u2; red[wave][1] = t_lo; red[wave][2] = t_hi; }
    __syncthreads();
    if (threadIdx.x < 3) {
        unsigned long long s = 0;
#pragma unroll
        for (int w = 0; w < kRsWaves; w++) s += red[w][threadIdx.x];
        A.part[(row * (int64_t) A.blocks + blockIdx.x) * 3 + threadIdx.x] = s;
    }
}

// grid = (rows of the batch): out[row][3] = the row's slots added up
__global__ void __launch_bounds__(kRsThreads) rs_fold_kernel(const unsigned long long *__restrict__ part, uint32_t blocks, unsigned long long *__restrict__ out) {
    __shared__ unsigned long long red[kRsWaves][3];
    const unsigned long long *__restrict__ p = part + (int64_t) blockIdx.x * blocks * 3;
    unsigned long long s[3] = {0, 0, 0};
    for (uint32_t b = threadIdx.x; b < blocks; b += kRsThreads) { s[0] += p[(int64_t) b * 3]; s[1] += p[(int64_t) b * 3 + 1]; s[2] += p[(int64_t) b * 3 + 2]; }
#pragma unroll
    for (int q = 0; q < 3; q++) s[q] = wave_sum(s[q]);
    const int wave = (int) (threadIdx.x >> 6);
    if ((threadIdx.x & 63u) == 0) { red[wave][0] = s[0]; red[wave][1] = s[1]; red[wave][2] = s[2]; }
    __syncthreads();
    if (threadIdx.x < 3) {
        unsigned long long t = 0;
#pragma unroll
        for (int w = 0; w < kRsWaves; w++) t += red[w][threadIdx.x];
        out[(int64_t) blockIdx.x * 3 + threadIdx.x] = t;
    }
}

// grid = (ceil(n / kRsCountElems), rows): counts[row][k] += the block's selected cells that pass cutoff k
__global__ void __launch_bounds__(kRsThreads) rs_count_kernel(const double *__restrict__ score, int64_t R, int32_t m_first, const int32_t *__restrict__ idx, uint32_t n,
                                                              const double *__restrict__ cut, int32_t n_cut, int32_t row0, unsigned long long *__restrict__ counts) {
    __shared__ unsigned int s_cnt[kRsWaves][kRsCutChunk];
    const int64_t row = (int64_t) row0 + blockIdx.y;
    const double *__restrict__ src = score + ((int64_t) m_first + row) * R;
    const int wave = (int) (threadIdx.x >> 6), lane = (int) (threadIdx.x & 63u);
    double s[kRsCountItems];
#pragma unroll
    for (int j = 0; j < kRsCountItems; j++) {
        const uint32_t i = blockIdx.x * (uint32_t) kRsCountElems + (uint32_t) j * kRsThreads + threadIdx.x;
        s[j] = i < n ? src[idx ? (uint32_t) idx[i] : i] : __builtin_nan("");        // a NaN never passes
    }
    for (int32_t k0 = 0; k0 < n_cut; k0 += kRsCutChunk) {
        const int kc = n_cut - k0 < kRsCutChunk ? n_cut - k0 : kRsCutChunk;
        for (int k = 0; k < kc; k++) {
            const double c = cut[row * n_cut + k0 + k];
            unsigned int cnt = 0;
#pragma unroll
            for (int j = 0; j < kRsCountItems; j++) cnt += (unsigned int) __popcll(__ballot(s[j] - c >= -1e-10));
            if (lane == 0) s_cnt[wave][k] = cnt;
        }
        __syncthreads();
        if ((int) threadIdx.x < kc) {
            unsigned int t = 0;
#pragma unroll
            for (int w = 0; w < kRsWaves; w++) t += s_cnt[w][threadIdx.x];
            if (t) atomicAdd(&counts[row * n_cut + k0 + threadIdx.x], (unsigned long long) t);
        }
        __syncthreads();
    }
}


int ceil_log2_plus1(uint32_t n) {                        // the least s with 2^s >= n + 1
    int s = 0;
    while ((1ull << s) < (unsigned long long) n + 1ull) s++;
    return s;
}

// the selected regions of a handle as an index list (empty with *all = true for a NULL selection)
int selection(const uint8_t *sel, int64_t R, std::vector<int32_t> *idx, uint32_t *n, bool *all) {
    *all = sel == nullptr;
    if (*all) { *n = (uint32_t) R; return MS_OK; }
    try {
        for (int64_t r = 0; r < R; r++)
            if (sel[r]) idx->push_back((int32_t) r);
    } catch (const std::bad_alloc &) { set_error("out of host memory"); return MS_ERR_NOMEM; }
    *n = (uint32_t) idx->size();
    return MS_OK;
}

// the sort form of a group of n cells; MS_MEASURE=1 MS_RANKSUM_SORT=row | segmented forces one (tools/ranksum_time.py)
bool sort_segmented(uint32_t n) {
    const char *e = measure_env("MS_RANKSUM_SORT");
    if (e && std::strcmp(e, "segmented") == 0) return true;
    if (e && std::strcmp(e, "row") == 0) return false;
    return n <= kRsSegmentedMax;
}

}  // namespace

// The rank sums of two [P][R] planes of doubles that lie on one device: the body of ms_best_rank_sum, which ms_affinity_rank_sum shares.
// The caller has checked for a device and for NULL handles; `what` names its handles in the error texts.
int rank_sum_planes(const char *what, const RankPlane &pa, const uint8_t *sel_a, const RankPlane &pb, const uint8_t *sel_b, int32_t m0, int32_t m1, uint32_t flags,
                    int64_t *u2, uint64_t *ties, int64_t *n, double *device_ms) {
    const RankPlane *a = &pa, *b = &pb;
    if (flags != 0u) { set_error("unknown rank-sum flags 0x%x", flags); return MS_ERR_INVALID; }
    if (a->P != b->P) { set_error("the two %s results disagree on the number of PWMs (%d and %d)", what, a->P, b->P); return MS_ERR_INVALID; }
    if (m0 < 0 || m1 < m0 || m1 > a->P) { set_error("motif range [%d, %d) outside [0, %d)", m0, m1, a->P); return MS_ERR_INVALID; }
    if (a->device != b->device) { set_error("the %s results live on devices %d and %d", what, a->device, b->device); return MS_ERR_INVALID; }
    if (a->R >= (1LL << 31) || b->R >= (1LL << 31)) { set_error("a group of 2^31 regions or more: u2 would not fit 64 bits"); return MS_ERR_INVALID; }
    const int32_t rows = m1 - m0;
    if (rows == 0) return MS_OK;
    if (!u2 || !ties) { set_error("NULL output"); return MS_ERR_INVALID; }
    if (device_ms) *device_ms = 0.0;
    std::vector<int32_t> idx_a, idx_b;
    uint32_t na = 0, nb = 0;
    bool all_a = true, all_b = true;
    int rc;
    if ((rc = selection(sel_a, a->R, &idx_a, &na, &all_a)) || (rc = selection(sel_b, b->R, &idx_b, &nb, &all_b))) return rc;
    if (n) { n[0] = na; n[1] = nb; }
    const size_t N = (size_t) na + nb;
    if (N == 0) {
        std::memset(u2, 0, 8 * (size_t) rows);
        std::memset(ties, 0, 16 * (size_t) rows);
        return MS_OK;
    }
    DeviceCtx *c;
    if ((rc = get_ctx(a->device, &c))) return rc;
    const bool seg_a = sort_segmented(na), seg_b = sort_segmented(nb);
    const int64_t set_budget = g_rs_budget.load();
    const size_t budget = std::min<size_t>((size_t) (set_budget > 0 ? set_budget : kRsBudget), (size_t) 1 << 31);      // (the segmented sort's offsets are 32-bit)
    const int32_t batch = (int32_t) std::max<size_t>(1, std::min<size_t>((size_t) rows, budget / N));
    const uint32_t blocks_a = (uint32_t) (((size_t) na + kRsRankElems - 1) / kRsRankElems), blocks_b = (uint32_t) (((size_t) nb + kRsRankElems - 1) / kRsRankElems);
    const uint32_t blocks = blocks_a + blocks_b;

    std::lock_guard<std::mutex> lk_dev(c->mu);
    MS_HIP(hipSetDevice(c->device));
    const hipStream_t st = c->stream;
    size_t tmp_a = 0, tmp_b = 0;
    if (na && (rc = sort_key_rows(nullptr, &tmp_a, nullptr, nullptr, (size_t) batch, na, seg_a, st))) return rc;
    if (nb && (rc = sort_key_rows(nullptr, &tmp_b, nullptr, nullptr, (size_t) batch, nb, seg_b, st))) return rc;
    const size_t b_ia = all_a ? 0 : up256(4 * (size_t) std::max<uint32_t>(na, 1)), b_ib = all_b ? 0 : up256(4 * (size_t) std::max<uint32_t>(nb, 1)),
                 b_keys = up256(8 * (size_t) batch * N), b_tmp = up256(std::max(tmp_a, tmp_b) + 256), b_part = up256(24 * (size_t) batch * blocks),
                 b_out = up256(24 * (size_t) rows);
    void *blk = nullptr;
    size_t got = 0;
    if ((rc = pool_alloc(c, b_ia + b_ib + 2 * b_keys + b_tmp + b_part + b_out, &blk, &got))) return rc;      // MS_ERR_NOMEM: nothing has been launched
    auto hip_fail = [&](hipError_t e, const char *what) {
        (void) hipStreamSynchronize(st);
        pool_free(c, blk, got);
        set_error("%s failed: %s", what, hipGetErrorString(e));
        return e == hipErrorOutOfMemory ? MS_ERR_NOMEM : MS_ERR_RUNTIME;
    };
    char *p = static_cast<char *>(blk);
    int32_t *d_ia = all_a ? nullptr : reinterpret_cast<int32_t *>(p); p += b_ia;
    int32_t *d_ib = all_b ? nullptr : reinterpret_cast<int32_t *>(p); p += b_ib;
    uint64_t *d_raw = reinterpret_cast<uint64_t *>(p); p += b_keys;          // [batch][na] then [batch][nb]
    uint64_t *d_sorted = reinterpret_cast<uint64_t *>(p); p += b_keys;
    void *d_tmp = p; p += b_tmp;
    unsigned long long *d_part = reinterpret_cast<unsigned long long *>(p); p += b_part;
    unsigned long long *d_out = reinterpret_cast<unsigned long long *>(p);

    hipError_t he = hipSuccess;
    if (d_ia && na) he = hipMemcpyAsync(d_ia, idx_a.data(), 4 * (size_t) na, hipMemcpyHostToDevice, st);
    if (he == hipSuccess && d_ib && nb) he = hipMemcpyAsync(d_ib, idx_b.data(), 4 * (size_t) nb, hipMemcpyHostToDevice, st);
    if (he != hipSuccess) return hip_fail(he, "upload of the selections");
    (void) hipEventRecord(c->ev[0], st);
    for (int32_t r0 = 0; r0 < rows; r0 += batch) {
        const int32_t nr = std::min(batch, rows - r0);
        uint64_t *raw_a = d_raw, *raw_b = d_raw + (size_t) nr * na, *srt_a = d_sorted, *srt_b = d_sorted + (size_t) nr * na;
        for (int32_t y0 = 0; y0 < nr; y0 += kRsGridY) {
            const unsigned gy = (unsigned) std::min(kRsGridY, nr - y0);
            if (na) hipLaunchKernelGGL(rs_gather_kernel, dim3((na + kRsGatherElems - 1) / kRsGatherElems, gy), dim3(kRsThreads), 0, st, a->plane, a->R, m0 + r0, d_ia, na, raw_a, y0);
            if (nb) hipLaunchKernelGGL(rs_gather_kernel, dim3((nb + kRsGatherElems - 1) / kRsGatherElems, gy), dim3(kRsThreads), 0, st, b->plane, b->R, m0 + r0, d_ib, nb, raw_b, y0);
        }
        if ((he = hipGetLastError()) != hipSuccess) return hip_fail(he, "rank-sum gather kernel");
        size_t tb = b_tmp;
        if (na && (rc = sort_key_rows(d_tmp, &tb, raw_a, srt_a, (size_t) nr, na, seg_a, st))) { (void) hipStreamSynchronize(st); pool_free(c, blk, got); return rc; }
        tb = b_tmp;
        if (nb && (rc = sort_key_rows(d_tmp, &tb, raw_b, srt_b, (size_t) nr, nb, seg_b, st))) { (void) hipStreamSynchronize(st); pool_free(c, blk, got); return rc; }
        RankArgs A;
        A.a = srt_a; A.b = srt_b; A.na = na; A.nb = nb;
        A.steps_a = ceil_log2_plus1(na); A.steps_b = ceil_log2_plus1(nb);
        A.blocks_a = blocks_a; A.blocks = blocks; A.part = d_part;
        for (int32_t y0 = 0; y0 < nr; y0 += kRsGridY)
            hipLaunchKernelGGL(rs_rank_kernel, dim3(blocks, (unsigned) std::min(kRsGridY, nr - y0)), dim3(kRsThreads), 0, st, A, y0);
        if ((he = hipGetLastError()) != hipSuccess) return hip_fail(he, "rank kernel");
        hipLaunchKernelGGL(rs_fold_kernel, dim3((unsigned) nr), dim3(kRsThreads), 0, st, d_part, blocks, d_out + (size_t) r0 * 3);
        if ((he = hipGetLastError()) != hipSuccess) return hip_fail(he, "rank-sum fold kernel");
    }
    (void) hipEventRecord(c->ev[1], st);
    std::vector<unsigned long long> h_out;
    try { h_out.resize(3 * (size_t) rows); } catch (const std::bad_alloc &) { (void) hipStreamSynchronize(st); pool_free(c, blk, got); set_error("out of host memory"); return MS_ERR_NOMEM; }
    he = hipMemcpyAsync(h_out.data(), d_out, 24 * (size_t) rows, hipMemcpyDeviceToHost, st);
    if (he == hipSuccess) he = hipStreamSynchronize(st);
    if (he != hipSuccess) return hip_fail(he, "rank sums");
    float ms01 = 0;
    (void) hipEventElapsedTime(&ms01, c->ev[0], c->ev[1]);
    if (device_ms) *device_ms = ms01;
    pool_free(c, blk, got);
    for (int32_t i = 0; i < rows; i++) {
        u2[i] = (int64_t) h_out[3 * (size_t) i];
        const unsigned __int128 t = (unsigned __int128) h_out[3 * (size_t) i + 1] + ((unsigned __int128) h_out[3 * (size_t) i + 2] << 32);
        ties[2 * (size_t) i] = (uint64_t) t;
        ties[2 * (size_t) i + 1] = (uint64_t) (t >> 64);
    }
    return MS_OK;
}

}  // namespace ms

using namespace ms;

extern "C" {

int ms_debug_ranksum_dims(int32_t out[8]) {
    if (!out) { set_error("NULL output"); return MS_ERR_INVALID; }
    out[0] = kRsThreads;
    out[1] = kRsGatherElems;
    out[2] = kRsRankElems;
    out[3] = kRsCountElems;
    out[4] = (int32_t) kRsBudget;
    out[5] = kRsCutChunk;
    out[6] = (int32_t) kRsSegmentedMax;
    out[7] = 0;
    return MS_OK;
}

int ms_debug_ranksum_budget(int64_t elems, int64_t *previous) {
    if (elems < 0) { set_error("budget must be >= 0 (0 = the library's own)"); return MS_ERR_INVALID; }
    const int64_t old = g_rs_budget.exchange(elems);
    if (previous) *previous = old;
    return MS_OK;
}

int ms_best_rank_sum(const ms_best *a, const uint8_t *sel_a, const ms_best *b, const uint8_t *sel_b, int32_t m0, int32_t m1, uint32_t flags, int64_t *u2, uint64_t *ties,
                     int64_t *n, double *device_ms) {
    if (!require_device()) return MS_ERR_RUNTIME;
    if (!a || !b) { set_error("NULL handle"); return MS_ERR_INVALID; }
    const RankPlane pa = {a->device, a->P, a->R, a->d_score}, pb = {b->device, b->P, b->R, b->d_score};
    return rank_sum_planes("best-site", pa, sel_a, pb, sel_b, m0, m1, flags, u2, ties, n, device_ms);
}

int ms_best_count_passing(const ms_best *b, const uint8_t *sel, const double *cutoffs, int32_t n_cut, int32_t m0, int32_t m1, int64_t *counts, double *device_ms) {
    if (!require_device()) return MS_ERR_RUNTIME;
    if (!b) { set_error("NULL handle"); return MS_ERR_INVALID; }
    if (m0 < 0 || m1 < m0 || m1 > b->P) { set_error("motif range [%d, %d) outside [0, %d)", m0, m1, b->P); return MS_ERR_INVALID; }
    if (n_cut < 0 || (n_cut > 0 && (!cutoffs || !counts))) { set_error("bad cutoffs / counts"); return MS_ERR_INVALID; }
    if (b->R >= (1LL << 31)) { set_error("2^31 regions or more"); return MS_ERR_INVALID; }
    const int32_t rows = m1 - m0;
    const size_t cells = (size_t) rows * (size_t) n_cut;
    for (size_t i = 0; i < cells; i++)
        if (!std::isfinite(cutoffs[i])) { set_error("cutoff %zu of motif %zu is not finite", i % (size_t) n_cut, (size_t) m0 + i / (size_t) n_cut); return MS_ERR_INVALID; }
    if (device_ms) *device_ms = 0.0;
    if (cells == 0) return MS_OK;
    std::vector<int32_t> idx;
    uint32_t n = 0;
    bool all = true;
    int rc;
    if ((rc = selection(sel, b->R, &idx, &n, &all))) return rc;
    std::memset(counts, 0, 8 * cells);
    if (n == 0) return MS_OK;
    DeviceCtx *c;
    if ((rc = get_ctx(b->device, &c))) return rc;
    std::lock_guard<std::mutex> lk_dev(c->mu);
    MS_HIP(hipSetDevice(c->device));
    const hipStream_t st = c->stream;
    const size_t b_idx = all ? 0 : up256(4 * (size_t) n), b_cut = up256(8 * cells);
    void *blk = nullptr;
    size_t got = 0;
    if ((rc = pool_alloc(c, b_idx + 2 * b_cut, &blk, &got))) return rc;
    auto hip_fail = [&](hipError_t e, const char *what) {
        (void) hipStreamSynchronize(st);
        pool_free(c, blk, got);
        set_error("%s failed: %s", what, hipGetErrorString(e));
        return e == hipErrorOutOfMemory ? MS_ERR_NOMEM : MS_ERR_RUNTIME;
    };
    char *p = static_cast<char *>(blk);
    int32_t *d_idx = all ? nullptr : reinterpret_cast<int32_t *>(p); p += b_idx;
    double *d_cut = reinterpret_cast<double *>(p); p += b_cut;
    unsigned long long *d_counts = reinterpret_cast<unsigned long long *>(p);
    hipError_t he = hipMemcpyAsync(d_cut, cutoffs, 8 * cells, hipMemcpyHostToDevice, st);
    if (he == hipSuccess && d_idx) he = hipMemcpyAsync(d_idx, idx.data(), 4 * (size_t) n, hipMemcpyHostToDevice, st);
    if (he == hipSuccess) he = hipMemsetAsync(d_counts, 0, 8 * cells, st);
    if (he != hipSuccess) return hip_fail(he, "upload of the cutoffs");
    (void) hipEventRecord(c->ev[0], st);
    for (int32_t y0 = 0; y0 < rows; y0 += kRsGridY) {
        hipLaunchKernelGGL(rs_count_kernel, dim3((n + kRsCountElems - 1) / kRsCountElems, (unsigned) std::min(kRsGridY, rows - y0)), dim3(kRsThreads), 0, st, b->d_score, b->R, m0,
                           d_idx, n, d_cut, n_cut, y0, d_counts);
        if ((he = hipGetLastError()) != hipSuccess) return hip_fail(he, "count kernel");
    }
    (void) hipEventRecord(c->ev[1], st);
    he = hipMemcpyAsync(counts, d_counts, 8 * cells, hipMemcpyDeviceToHost, st);
    if (he == hipSuccess) he = hipStreamSynchronize(st);
    if (he != hipSuccess) return hip_fail(he, "counts of passing regions");
    float ms01 = 0;
    (void) hipEventElapsedTime(&ms01, c->ev[0], c->ev[1]);
    if (device_ms) *device_ms = ms01;
    pool_free(c, blk, got);
    return MS_OK;
}

}  // extern "C"
