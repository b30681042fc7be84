// ms_compare.hip -- motif sets compared with each other (ms_motifs_compare): for every (query, target) pair the best ungapped alignment
// of the two matrices, column against column in both orientations, and its P-value under a null made of the target set's own columns.
// The procedure is Tomtom's (Gupta et al. 2007); the reference project has no counterpart.  include/motifscan_amd.h holds the definition;
// in short, with the columns prepared on the host (ms_compare_plan.h):
//     k(i, c)        the integer score of query column i against target column c: floor((g - lo) * scale), clamped -- cmp_score below,
//                    the only place a column score is formed
//     H_i[k]         the number of target columns (and of their reversed forms) that score k against query column i: exact uint32
//     pm_{a,1} = f_a = H_a * invN;  pm_{a,L}[s] = sum_k pm_{a,L-1}[s - k] * f_{a+L-1}[k], ascending k from +0.0
//     tail_{a,L}[s]  the sum of pm_{a,L} from the top down to s, sequentially
//     per pair       over the admissible (orientation, offset): S = the sum of the overlap's column scores, p = tail_{a,L}[S]; the least
//                    key (p, -L, orientation, offset) is kept
// Three kernels per batch of queries, in stream order (no grid-wide barrier: the stream is the barrier):
//   histogram   block = (query column, tiles of kCmpHistTile target columns).  Consecutive lanes take consecutive target columns, one
//               32-byte read each; every wave counts into an LDS histogram of its own (scores bunch in a few bins), the block merges the
//               four and adds the non-zero bins to H.  Integers: the order changes nothing.
//   tables      block = (start a, query) walks L = 1 .. W - a: step L reads table (a, L - 1) and f_{a+L-1} (LDS) and stores table (a, L),
//               one thread per output score, a block barrier between steps.  pm stays in the tables; afterwards thread L - 1 turns table
//               (a, L) into its tail in place, top down.  One path for every W x bins.
//   alignment   block = (tile of kCmpAlignTile targets, query), one thread per pair, the query's vectors in LDS.  Every (i, j) cell of a
//               pair lies on one diagonal per orientation, so the column scores are formed again -- as many as the histogram formed -- and
//               no Q x T x W x W score array exists; one 8-byte gather from `tail` per admissible alignment.
// Every byte read was written by an earlier launch or copy of the same call (H is cleared per batch: it is added to).
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <new>

#include "ms_handles.h"
#include "ms_compare_plan.h"

namespace ms {

namespace {

constexpr int kCmpThreads = 256;                         // a block of all three kernels: four waves
constexpr int kCmpWaves = kCmpThreads / 64;
constexpr int kCmpHistTile = 2048;                       // target columns per tile of the histogram: 8 per thread, kCmpThreads apart
constexpr int kCmpHistGridY = 32768;                     // tiles side by side; a block takes further tiles gridDim.y apart
constexpr int kCmpAlignTile = kCmpThreads;               // targets per block of the alignment: one per thread
constexpr int64_t kCmpBudgetMiB = 256;
constexpr int32_t kCmpBatchCap = 4096;                   // queries of a batch: the y of a grid, and the rows of the staged planes

std::atomic<int64_t> g_cmp_budget{0};                    // ms_debug_compare_budget: 0 = kCmpBudgetMiB

struct CmpArgs {
    const double *tv;                                    // [target columns][4] prepared
    const int32_t *t_first;                              // [n_t + 1]
    const double *qv;                                    // [query columns][4] prepared, the queries of the call's range
    const int32_t *q_first;                              // [n + 1]
    const int64_t *q_tab;                                // [n] into tab, per batch
    const int64_t *col_off;                              // [query columns]
    uint32_t *H;                                         // [columns of a batch][bins]
    double *tab;                                         // the tables of a batch
    double *p_min;                                       // the planes of a batch: [queries of the batch][n_t]
    int32_t *offset, *overlap, *score, *n_offsets;
    int8_t *orient;
    int32_t n_t, nt_cols, metric, bins, min_overlap, both;
    double lo, scale, invN;
};

// The integer score of query vector u against target vector v.  Each product, sum, difference and the square root is one rounded
// operation (-ffp-contract=off, no fast-math: the f64 sqrt is the correctly rounded expansion).
__device__ __forceinline__ int32_t cmp_score(int metric, const double u[4], const double v[4], double lo, double scale, int32_t bins) {
    double g;
    if (metric == MS_COMPARE_PEARSON) {
        g = ((u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]) + u[3] * v[3];
    } else {
        const double d0 = u[0] - v[0], d1 = u[1] - v[1], d2 = u[2] - v[2], d3 = u[3] - v[3];
        const double ssd = ((d0 * d0 + d1 * d1) + d2 * d2) + d3 * d3;
        g = metric == MS_COMPARE_SW ? 2.0 - ssd : -sqrt(ssd);
    }
    const double t = floor((g - lo) * scale);
    return !(t >= 0.0) ? 0 : (t > (double) (bins - 1) ? bins - 1 : (int32_t) t);
}

// target column c as one 32-byte read; REV: its reversed form (the four entries in reverse order)
template <bool REV>
__device__ __forceinline__ void cmp_load(const double *__restrict__ tv, int64_t c, double v[4]) {
    const double2 lo = reinterpret_cast<const double2 *>(tv)[2 * c], hi = reinterpret_cast<const double2 *>(tv)[2 * c + 1];
    if (REV) { v[0] = hi.y; v[1] = hi.x; v[2] = lo.y; v[3] = lo.x; }
    else { v[0] = lo.x; v[1] = lo.y; v[2] = hi.x; v[3] = hi.y; }
}

// ---- histogram: grid = (the batch's query columns, tiles side by side); c0: the batch's first column in qv
__global__ void __launch_bounds__(kCmpThreads) compare_hist_kernel(const CmpArgs A, int32_t c0) {
    __shared__ uint32_t h[kCmpWaves][kCmpMaxBins];
    const int tid = (int) threadIdx.x;
    for (int i = tid; i < kCmpWaves * kCmpMaxBins; i += kCmpThreads) (&h[0][0])[i] = 0u;
    __syncthreads();
    const double *const qu = A.qv + ((size_t) c0 + blockIdx.x) * 4;
    const double u[4] = {qu[0], qu[1], qu[2], qu[3]};
    uint32_t *const mine = h[tid >> 6];
    for (int64_t first = (int64_t) blockIdx.y * kCmpHistTile; first < (int64_t) A.nt_cols; first += (int64_t) gridDim.y * kCmpHistTile) {
#pragma unroll
        for (int r = 0; r < kCmpHistTile / kCmpThreads; r++) {
            const int64_t c = first + r * kCmpThreads + tid;
            if (c >= (int64_t) A.nt_cols) continue;
            double v[4];
            cmp_load<false>(A.tv, c, v);
            atomicAdd(&mine[cmp_score(A.metric, u, v, A.lo, A.scale, A.bins)], 1u);
            if (A.both) {
                const double w[4] = {v[3], v[2], v[1], v[0]};
                atomicAdd(&mine[cmp_score(A.metric, u, w, A.lo, A.scale, A.bins)], 1u);
            }
        }
    }
    __syncthreads();
    uint32_t *const row = A.H + (size_t) blockIdx.x * (size_t) A.bins;
    for (int k = tid; k < A.bins; k += kCmpThreads) {
        uint32_t s = 0;
#pragma unroll
        for (int w = 0; w < kCmpWaves; w++) s += h[w][k];
        if (s) atomicAdd(&row[k], s);
    }
}

// ---- tables: grid = (the widest query of the batch, the batch's queries); k0: the batch's first query
__global__ void __launch_bounds__(kCmpThreads) compare_tables_kernel(const CmpArgs A, int32_t k0) {
    __shared__ double f[kCmpMaxBins];
    const int32_t q = k0 + (int32_t) blockIdx.y;
    const int32_t qc = A.q_first[q], W = A.q_first[q + 1] - qc, a = (int32_t) blockIdx.x;
    if (a >= W) return;                                  // (block-uniform: every thread of a block that stays meets every barrier)
    const int tid = (int) threadIdx.x;
    const int32_t bins = A.bins;
    const uint32_t *const Hq = A.H + (size_t) (qc - A.q_first[k0]) * (size_t) bins;
    double *const base = A.tab + A.q_tab[q] + A.col_off[qc + a];
    for (int32_t L = 1; L <= W - a; L++) {
        __syncthreads();                                 // the step before has read f and stored its table
        for (int k = tid; k < bins; k += kCmpThreads) f[k] = (double) Hq[(size_t) (a + L - 1) * (size_t) bins + k] * A.invN;
        __syncthreads();
        double *const cur = base + cmp_tables_upto(L - 1, bins);
        const int32_t len = (int32_t) cmp_table_len(L, bins);
        if (L == 1) {
            for (int32_t s = tid; s < len; s += kCmpThreads) cur[s] = f[s];
            continue;
        }
        const double *const prev = base + cmp_tables_upto(L - 2, bins);
        const int32_t top = (int32_t) cmp_table_len(L - 1, bins) - 1;
        for (int32_t s = tid; s < len; s += kCmpThreads) {
            const int32_t k_lo = s > top ? s - top : 0, k_hi = s < bins - 1 ? s : bins - 1;
            double acc = 0.0;
            for (int32_t k = k_lo; k <= k_hi; k++) acc = acc + prev[s - k] * f[k];
            cur[s] = acc;
        }
    }
    __syncthreads();
    if (tid < W - a) {                                   // table (a, tid + 1): pm to tail in place, top down -- the definition's order
        const int32_t L = tid + 1;
        double *const tb = base + cmp_tables_upto(L - 1, bins);
        int32_t s = (int32_t) cmp_table_len(L, bins) - 1;
        double acc = tb[s];
        for (s--; s >= 0; s--) {
            acc = acc + tb[s];
            tb[s] = acc;
        }
    }
}

// S of one alignment: the overlap's columns i in [a, e), target column j = i - o
template <bool REV>
__device__ __forceinline__ int32_t cmp_diagonal(const CmpArgs &A, const double *qs, int32_t tf, int32_t Wt, int32_t o, int32_t a, int32_t e) {
    int32_t S = 0;
    for (int32_t i = a; i < e; i++) {
        const int32_t j = i - o;
        double v[4];
        cmp_load<REV>(A.tv, (int64_t) tf + (REV ? Wt - 1 - j : j), v);
        S += cmp_score(A.metric, qs + 4 * i, v, A.lo, A.scale, A.bins);
    }
    return S;
}

// ---- alignment: grid = (tiles of kCmpAlignTile targets, the batch's queries)
__global__ void __launch_bounds__(kCmpThreads) compare_align_kernel(const CmpArgs A, int32_t k0) {
    __shared__ double qs[kCmpMaxWidth * 4];
    const int32_t q = k0 + (int32_t) blockIdx.y;
    const int32_t qc = A.q_first[q], Wq = A.q_first[q + 1] - qc;
    for (int i = (int) threadIdx.x; i < 4 * Wq; i += kCmpThreads) qs[i] = A.qv[(size_t) qc * 4 + i];
    __syncthreads();
    const int64_t t = (int64_t) blockIdx.x * kCmpAlignTile + (int64_t) threadIdx.x;
    if (t >= (int64_t) A.n_t) return;
    const int32_t tf = A.t_first[t], Wt = A.t_first[t + 1] - tf;
    const int32_t need = min(A.min_overlap, min(Wq, Wt));
    const double *const tabq = A.tab + A.q_tab[q];
    const int64_t *const co = A.col_off + qc;
    double bp = 0.0;
    int32_t bo = 0, bL = 0, bS = 0, n = 0, bor = 0;
    for (int32_t rev = 0; rev <= (A.both ? 1 : 0); rev++)
        for (int32_t o = -(Wt - 1); o < Wq; o++) {
            const int32_t a = o > 0 ? o : 0, e = min(Wq, Wt + o), L = e - a;
            if (L < need) continue;
            const int32_t S = rev ? cmp_diagonal<true>(A, qs, tf, Wt, o, a, e) : cmp_diagonal<false>(A, qs, tf, Wt, o, a, e);
            const double p = tabq[co[a] + cmp_tables_upto(L - 1, A.bins) + S];
            // the least (p, -L, orientation, o): the walk is in (orientation, o) order, so only a strictly better (p, -L) replaces
            if (n == 0 || p < bp || (p == bp && L > bL)) { bp = p; bo = o; bL = L; bS = S; bor = rev; }
            n++;
        }
    const size_t at = (size_t) blockIdx.y * (size_t) A.n_t + (size_t) t;
    A.p_min[at] = bp;
    A.offset[at] = bo;
    A.overlap[at] = bL;
    A.score[at] = bS;
    A.n_offsets[at] = n;
    A.orient[at] = (int8_t) bor;
}

struct CmpOut {                                          // where a call's results go: the six planes, or (query >= 0) one query's null
    double *p_min = nullptr;
    int32_t *offset = nullptr, *overlap = nullptr, *score = nullptr, *n_offsets = nullptr;
    int8_t *orient = nullptr;
    uint32_t *H = nullptr;
    double *tail = nullptr;
    bool null_only = false;
};

// widths first, then the column count against `most`, then the entries: a set refused for its size is not read
int check_set(const char *what, const double *values, const int32_t *widths, int32_t n, int64_t most) {
    if (n < 0) { set_error("a negative number of %s", what); return MS_ERR_INVALID; }
    if (n == 0) return MS_OK;
    if (!values || !widths) { set_error("NULL array (%s)", what); return MS_ERR_INVALID; }
    int64_t cols = 0;
    for (int32_t m = 0; m < n; m++) {
        if (widths[m] < 1 || widths[m] > MS_COMPARE_MAX_WIDTH) { set_error("%s %d: width %d outside [1, %d]", what, m, widths[m], MS_COMPARE_MAX_WIDTH); return MS_ERR_INVALID; }
        cols += widths[m];
    }
    if (cols > most) { set_error("the %s have more than 2^30 columns", what); return MS_ERR_INVALID; }
    for (int64_t i = 0; i < 4 * cols; i++)
        if (!std::isfinite(values[i])) { set_error("%s: entry %lld is not finite", what, (long long) i); return MS_ERR_INVALID; }
    return MS_OK;
}

// what ms_motifs_compare and ms_debug_compare_null share: everything but the device check and the outputs' NULL check
int compare_run(const double *q_values, const int32_t *q_widths, int32_t n_q, const double *t_values, const int32_t *t_widths, int32_t n_t, int metric, int32_t bins,
                int32_t min_overlap, int orientations, int32_t q0, int32_t q1, const CmpOut &out, double *device_ms) {
    int64_t nt_cols = 0;
    for (int32_t t = 0; t < n_t; t++) nt_cols += t_widths[t];
    const bool both = orientations == 3;

    // ---- the plan, on the host: the prepared vectors, the layout of the tables, the batches
    const int64_t set = g_cmp_budget.load();
    CmpPlan plan;
    std::vector<double> tv;
    std::vector<int32_t> t_first;
    try {
        if (cmp_plan(q_values, q_widths, q0, q1, metric, bins, set > 0 ? set : kCmpBudgetMiB << 20, kCmpBatchCap, &plan) == kCmpNoRoom) {
            set_error("the tables of query %d (%lld bytes at %d bins) do not fit the work budget", plan.bad, (long long) plan.bad_bytes, bins);
            return MS_ERR_NOMEM;
        }
        if ((int64_t) plan.q_first.back() > kCmpMaxColumns) { set_error("more than 2^30 query columns in one call: narrow [q0, q1)"); return MS_ERR_INVALID; }
        tv.resize(4 * (size_t) nt_cols);
        t_first.assign((size_t) n_t + 1, 0);
        size_t at = 0;
        for (int32_t t = 0; t < n_t; t++) {
            cmp_prepare(t_values + at, t_widths[t], metric, tv.data() + at);
            at += 4 * (size_t) t_widths[t];
            t_first[(size_t) t + 1] = t_first[(size_t) t] + t_widths[t];
        }
    } catch (const std::bad_alloc &) { set_error("out of host memory"); return MS_ERR_NOMEM; }
    double lo, scale;
    cmp_grid(metric, bins, &lo, &scale);
    const int64_t N = both ? 2 * nt_cols : nt_cols;

    DeviceCtx *c;
    int rc = get_ctx(current_device(), &c);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk_dev(c->mu);
    MS_HIP(hipSetDevice(c->device));
    const hipStream_t st = c->stream;

    const size_t q_cols = (size_t) plan.q_first.back(), cells = out.null_only ? 0 : (size_t) plan.max_queries * (size_t) n_t;
    Carve cv;
    const auto s_tv = cv.add<double>(tv.size()), s_qv = cv.add<double>(plan.qv.size());
    const auto s_tf = cv.add<int32_t>(t_first.size()), s_qf = cv.add<int32_t>(plan.q_first.size());
    const auto s_qt = cv.add<int64_t>(plan.q_tab.size()), s_co = cv.add<int64_t>(q_cols);
    const auto s_H = cv.add<uint32_t>((size_t) plan.max_cols * (size_t) bins);
    const auto s_tab = cv.add<double>((size_t) plan.max_doubles);
    const auto s_p = cv.add<double>(cells);
    const auto s_off = cv.add<int32_t>(cells), s_ovl = cv.add<int32_t>(cells), s_sc = cv.add<int32_t>(cells), s_n = cv.add<int32_t>(cells);
    const auto s_or = cv.add<int8_t>(cells);
    void *wblk = nullptr;
    size_t wgot = 0;
    if ((rc = pool_alloc(c, cv.bytes() + 256, &wblk, &wgot))) return rc;
    auto fail = [&](int code) { (void) hipStreamSynchronize(st); pool_free(c, wblk, wgot); return code; };

    hipError_t he = hipMemcpyAsync(Carve::at(wblk, s_tv), tv.data(), 8 * tv.size(), hipMemcpyHostToDevice, st);
    if (he == hipSuccess) he = hipMemcpyAsync(Carve::at(wblk, s_qv), plan.qv.data(), 8 * plan.qv.size(), hipMemcpyHostToDevice, st);
    if (he == hipSuccess) he = hipMemcpyAsync(Carve::at(wblk, s_tf), t_first.data(), 4 * t_first.size(), hipMemcpyHostToDevice, st);
    if (he == hipSuccess) he = hipMemcpyAsync(Carve::at(wblk, s_qf), plan.q_first.data(), 4 * plan.q_first.size(), hipMemcpyHostToDevice, st);
    if (he == hipSuccess) he = hipMemcpyAsync(Carve::at(wblk, s_qt), plan.q_tab.data(), 8 * plan.q_tab.size(), hipMemcpyHostToDevice, st);
    if (he == hipSuccess) he = hipMemcpyAsync(Carve::at(wblk, s_co), plan.col_off.data(), 8 * q_cols, hipMemcpyHostToDevice, st);
    if (he != hipSuccess) return fail(hip_rc(he, "upload of the plan"));

    CmpArgs A;
    A.tv = Carve::at(wblk, s_tv); A.t_first = Carve::at(wblk, s_tf); A.qv = Carve::at(wblk, s_qv); A.q_first = Carve::at(wblk, s_qf);
    A.q_tab = Carve::at(wblk, s_qt); A.col_off = Carve::at(wblk, s_co); A.H = Carve::at(wblk, s_H); A.tab = Carve::at(wblk, s_tab);
    A.p_min = Carve::at(wblk, s_p); A.offset = Carve::at(wblk, s_off); A.overlap = Carve::at(wblk, s_ovl); A.score = Carve::at(wblk, s_sc);
    A.n_offsets = Carve::at(wblk, s_n); A.orient = Carve::at(wblk, s_or);
    A.n_t = n_t; A.nt_cols = (int32_t) nt_cols; A.metric = metric; A.bins = bins; A.min_overlap = min_overlap; A.both = both ? 1 : 0;
    A.lo = lo; A.scale = scale; A.invN = 1.0 / (double) N;

    const int64_t tiles = (nt_cols + kCmpHistTile - 1) / kCmpHistTile;
    (void) hipEventRecord(c->ev[0], st);
    for (size_t b = 0; b + 1 < plan.batch_first.size(); b++) {
        const int32_t k0 = plan.batch_first[b], nb = plan.batch_first[b + 1] - k0;
        const int32_t c0 = plan.q_first[(size_t) k0], nc = plan.q_first[(size_t) k0 + (size_t) nb] - c0;
        int32_t wmax = 0;
        for (int32_t k = k0; k < k0 + nb; k++) wmax = std::max(wmax, plan.q_first[(size_t) k + 1] - plan.q_first[(size_t) k]);
        if ((he = hipMemsetAsync(A.H, 0, 4 * (size_t) nc * (size_t) bins, st)) != hipSuccess) return fail(hip_rc(he, "clear of the histograms"));
        hipLaunchKernelGGL(compare_hist_kernel, dim3((unsigned) nc, (unsigned) std::min<int64_t>(tiles, kCmpHistGridY)), dim3(kCmpThreads), 0, st, A, c0);
        if ((he = hipGetLastError()) != hipSuccess) return fail(hip_rc(he, "comparison histogram kernel"));
        hipLaunchKernelGGL(compare_tables_kernel, dim3((unsigned) wmax, (unsigned) nb), dim3(kCmpThreads), 0, st, A, k0);
        if ((he = hipGetLastError()) != hipSuccess) return fail(hip_rc(he, "comparison tables kernel"));
        if (out.null_only) {                               // one query, one batch
            (void) hipEventRecord(c->ev[1], st);
            he = hipMemcpyAsync(out.H, A.H, 4 * (size_t) nc * (size_t) bins, hipMemcpyDeviceToHost, st);
            if (he == hipSuccess) he = hipMemcpyAsync(out.tail, A.tab, 8 * (size_t) plan.max_doubles, hipMemcpyDeviceToHost, st);
            if (he != hipSuccess) return fail(hip_rc(he, "copy of the null"));
            continue;
        }
        hipLaunchKernelGGL(compare_align_kernel, dim3((unsigned) ((n_t + kCmpAlignTile - 1) / kCmpAlignTile), (unsigned) nb), dim3(kCmpThreads), 0, st, A, k0);
        if ((he = hipGetLastError()) != hipSuccess) return fail(hip_rc(he, "comparison alignment kernel"));
        if (b + 2 == plan.batch_first.size()) (void) hipEventRecord(c->ev[1], st);
        const size_t row0 = (size_t) k0 * (size_t) n_t, nbc = (size_t) nb * (size_t) n_t;   // the batch's rows of the caller's planes; the next batch reuses the staged ones in stream order
        he = hipMemcpyAsync(out.p_min + row0, A.p_min, 8 * nbc, hipMemcpyDeviceToHost, st);
        if (he == hipSuccess) he = hipMemcpyAsync(out.offset + row0, A.offset, 4 * nbc, hipMemcpyDeviceToHost, st);
        if (he == hipSuccess) he = hipMemcpyAsync(out.overlap + row0, A.overlap, 4 * nbc, hipMemcpyDeviceToHost, st);
        if (he == hipSuccess) he = hipMemcpyAsync(out.score + row0, A.score, 4 * nbc, hipMemcpyDeviceToHost, st);
        if (he == hipSuccess) he = hipMemcpyAsync(out.n_offsets + row0, A.n_offsets, 4 * nbc, hipMemcpyDeviceToHost, st);
        if (he == hipSuccess) he = hipMemcpyAsync(out.orient + row0, A.orient, nbc, hipMemcpyDeviceToHost, st);
        if (he != hipSuccess) return fail(hip_rc(he, "copy of the planes"));
    }
    if ((he = hipStreamSynchronize(st)) != hipSuccess) return fail(hip_rc(he, "motif comparison"));
    float ms01 = 0;
    (void) hipEventElapsedTime(&ms01, c->ev[0], c->ev[1]);
    if (device_ms) *device_ms = ms01;
    pool_free(c, wblk, wgot);
    return MS_OK;
}

int check_args(const double *q_values, const int32_t *q_widths, int32_t n_q, const double *t_values, const int32_t *t_widths, int32_t n_t, int metric, int32_t bins,
               int32_t min_overlap, int orientations) {
    if (metric < MS_COMPARE_PEARSON || metric > MS_COMPARE_ED) { set_error("invalid metric %d (0 pearson, 1 sw, 2 ed)", metric); return MS_ERR_INVALID; }
    if (bins < 2 || bins > MS_COMPARE_MAX_BINS) { set_error("bins must be in [2, %d]", MS_COMPARE_MAX_BINS); return MS_ERR_INVALID; }
    if (min_overlap < 1) { set_error("min_overlap must be >= 1"); return MS_ERR_INVALID; }
    if (orientations != 1 && orientations != 3) { set_error("invalid orientations %d (1 forward, 3 both)", orientations); return MS_ERR_INVALID; }
    const int rc = check_set("targets", t_values, t_widths, n_t, kCmpMaxColumns);
    return rc ? rc : check_set("queries", q_values, q_widths, n_q, INT64_MAX);
}

}  // namespace

}  // namespace ms

using namespace ms;

extern "C" {

int ms_debug_compare_dims(int32_t out[8]) {
    if (!out) { set_error("NULL output"); return MS_ERR_INVALID; }
    out[0] = kCmpThreads;
    out[1] = kCmpHistTile;
    out[2] = kCmpAlignTile;
    out[3] = (int32_t) kCmpBudgetMiB;
    out[4] = kCmpBatchCap;
    out[5] = kCmpHistGridY;
    out[6] = 0;                                          // no LDS-resident variant of the tables: one path for every W x bins
    out[7] = 0;
    return MS_OK;
}

int ms_debug_compare_budget(int64_t bytes, int64_t *previous) {
    if (bytes < 0) { set_error("budget must be >= 0 (0 = the library's own)"); return MS_ERR_INVALID; }
    const int64_t old = g_cmp_budget.exchange(bytes);
    if (previous) *previous = old;
    return MS_OK;
}

int ms_debug_compare_null(const double *q_values, const int32_t *q_widths, int32_t n_q, const double *t_values, const int32_t *t_widths, int32_t n_t, int metric,
                          int32_t bins, int orientations, int32_t query, uint32_t *H, double *tail) {
    if (!require_device()) return MS_ERR_RUNTIME;
    const int rc = check_args(q_values, q_widths, n_q, t_values, t_widths, n_t, metric, bins, 1, orientations);
    if (rc) return rc;
    if (query < 0 || query >= n_q) { set_error("query %d outside [0, %d)", query, n_q); return MS_ERR_INVALID; }
    if (n_t < 1) { set_error("a null needs at least one target"); return MS_ERR_INVALID; }
    if (!H || !tail) { set_error("NULL output"); return MS_ERR_INVALID; }
    CmpOut out;
    out.H = H; out.tail = tail; out.null_only = true;
    return compare_run(q_values, q_widths, n_q, t_values, t_widths, n_t, metric, bins, 1, orientations, query, query + 1, out, nullptr);
}

int ms_motifs_compare(const double *q_values, const int32_t *q_widths, int32_t n_q, const double *t_values, const int32_t *t_widths, int32_t n_t, int metric, int32_t bins,
                      int32_t min_overlap, int orientations, int32_t q0, int32_t q1, double *p_min, int32_t *offset, int32_t *overlap, int32_t *score,
                      int32_t *n_offsets, int8_t *orient, double *device_ms) {
    if (!require_device()) return MS_ERR_RUNTIME;
    if (device_ms) *device_ms = 0.0;
    const int rc = check_args(q_values, q_widths, n_q, t_values, t_widths, n_t, metric, bins, min_overlap, orientations);
    if (rc) return rc;
    if (q0 < 0 || q1 > n_q || q0 > q1) { set_error("invalid query range [%d, %d) of %d queries", q0, q1, n_q); return MS_ERR_INVALID; }
    if (q0 == q1 || n_t == 0) return MS_OK;
    if (!p_min || !offset || !overlap || !score || !n_offsets || !orient) { set_error("NULL output"); return MS_ERR_INVALID; }
    CmpOut out;
    out.p_min = p_min; out.offset = offset; out.overlap = overlap; out.score = score; out.n_offsets = n_offsets; out.orient = orient;
    return compare_run(q_values, q_widths, n_q, t_values, t_widths, n_t, metric, bins, min_overlap, orientations, q0, q1, out, device_ms);
}

}  // extern "C"
