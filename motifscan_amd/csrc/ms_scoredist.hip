// ms_scoredist.hip -- the analytic score distribution of a window under a Markov background (ms_pwmset_score_distribution): from a matrix
// and a conditional table alone, the probability of every integer score.  No reference counterpart (FIMO, MOODS, HOMER and TFM-Pvalue
// compute the same thing for an order-0 background).  include/motifscan_amd.h holds the definition; in short, per motif, over arrays
// [C = 4^order contexts][n_bins] of doubles:
//     old[ctx][0] = init[ctx], +0.0 elsewhere
//     per column c:  new[x][i] = ((t_A + t_C) + t_G) + t_T,  t_a = old[p_a][i - d[b][c]] * cond[p_a][b],  b = x & 3,
//                    p_a = a * 4^(order - 1) + (x >> 2)     (order 0: one context, t_b = old[0][i - d[b][c]] * cond[0][b])
//     mass[i] = new[0][i] + new[1][i] + ... left to right, after the last column
// The grid (step, s0, the shifts d) is made on the host: ms_scoredist_plan.h.
//
// Every element is ONE expression -- sd_element below, the only place that forms a term -- whatever computes it, so path, tile, batch
// and budget change no byte.  Two paths:
//   LDS     2 C n_bins 8 bytes fit the CU's LDS: one block per motif holds both buffers there and walks all W columns inside one launch,
//           a block barrier between columns; the context sum goes from LDS straight to mass.  Column 0 reads `init` instead of a buffer,
//           so nothing is cleared.
//   global  the two buffers of every motif of a batch lie in pooled device scratch.  ONE LAUNCH PER COLUMN over the batch: grid = (bin
//           tiles, contexts, motifs), a motif of W <= c returns at once; consecutive lanes take consecutive bins, so each of the four
//           shifted reads of a wave is one contiguous run.  Column c writes buffer c & 1 and reads the other (column 0: `init`), so every
//           byte read was written by the launch before -- recycled memory is never seen.  Then one launch for the context sum.  There is
//           no grid-wide barrier anywhere: the stream's order is the barrier, at most max_width + 1 launches a batch.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <new>

#include "ms_handles.h"
#include "ms_scoredist_plan.h"

namespace ms {

namespace {

constexpr int kSdThreads = 256;                          // a block of the global path's kernels
constexpr int kSdTileBins = 1024;                        // bins per block of the global path: 4 per thread, kSdThreads apart
constexpr int kSdLdsThreads = 1024;                      // the LDS path's block: one per motif and CU, 16 waves to hide the LDS latency
constexpr size_t kSdLdsBytes = 160 * 1024;               // the LDS of a gfx950 CU
constexpr int32_t kSdLdsElems = (int32_t) (kSdLdsBytes / 16);   // the largest C x n_bins of the LDS path
constexpr int64_t kSdBudgetMiB = 256;
constexpr int32_t kSdBatchCap = 32768;                   // motifs of a batch: the z of a grid

std::atomic<int64_t> g_sd_budget{0};                     // ms_debug_scoredist_budget: 0 = kSdBudgetMiB
std::atomic<int32_t> g_sd_force_global{0};               // ms_debug_scoredist_force_global

struct SdArgs {
    const int32_t *mot;                                  // [n] the motifs the device computes
    const int32_t *width;                                // [n]
    const int32_t *col_first;                            // [n + 1] into shift / 4
    const int32_t *shift;                                // [columns][4]; kSdAbsent: the entry is -inf
    const double *cond;                                  // [C][4]
    const double *init;                                  // [C]
    double *buf;                                         // global path: [motifs of a batch][2][C][n_bins]
    double *out;                                         // rows of n_bins doubles
    int32_t out_by_motif;                                // != 0: row mot[k] (the caller's device array); 0: row k - k0 (the batch's staging rows)
    int32_t order, C, n_bins;
};

// new[x][i] of one column: `old` is the previous column's [C][n_bins] (FIRST: column 0, whose "old" is init at bin 0 and +0.0 elsewhere),
// sh the column's four shifts.  Each product and each sum is one rounded operation (-ffp-contract=off).
template <bool FIRST>
__device__ __forceinline__ double sd_element(const double *old, const double *__restrict__ init, const double *__restrict__ cond, int order, int32_t C, int32_t n_bins,
                                             int32_t x, int32_t i, const int32_t sh[4]) {
    double t[4];
#pragma unroll
    for (int a = 0; a < 4; a++) {
        const int32_t p = order == 0 ? 0 : a * (C >> 2) + (x >> 2);
        const int b = order == 0 ? a : (x & 3);
        const int32_t s = sh[b];
        const int32_t j = i - s;
        const bool live = s >= 0 && j >= 0;              // (s <= the motif's span < n_bins, i < n_bins: j < n_bins)
        double o = 0.0;
        if (live) o = FIRST ? (j == 0 ? init[p] : 0.0) : old[(size_t) p * (size_t) n_bins + (size_t) j];
        const double prod = o * cond[p * 4 + b];
        t[a] = live ? prod : 0.0;
    }
    return ((t[0] + t[1]) + t[2]) + t[3];
}

// mass[i]: the contexts of the last column, left to right
__device__ __forceinline__ double sd_context_sum(const double *last, int32_t C, int32_t n_bins, int32_t i) {
    double s = last[i];
    for (int32_t x = 1; x < C; x++) s = s + last[(size_t) x * (size_t) n_bins + (size_t) i];
    return s;
}

// ---- LDS path: grid = the batch's motifs, kSdLdsThreads threads, dynamic LDS = 2 C n_bins doubles
__global__ void __launch_bounds__(kSdLdsThreads) scoredist_lds_kernel(const SdArgs A, int32_t k0) {
    extern __shared__ double sd_lds[];
    const int32_t k = k0 + (int32_t) blockIdx.x;
    const int32_t W = A.width[k];
    const int32_t *__restrict__ shift = A.shift + (size_t) A.col_first[k] * 4;
    const int32_t n = A.C * A.n_bins;                    // <= kSdLdsElems
    for (int32_t c = 0; c < W; c++) {                    // (W and the trip counts are block-uniform: every thread meets every barrier)
        const int32_t sh[4] = {shift[c * 4], shift[c * 4 + 1], shift[c * 4 + 2], shift[c * 4 + 3]};
        double *const cur = sd_lds + (size_t) (c & 1) * (size_t) n;
        const double *const old = sd_lds + (size_t) ((c & 1) ^ 1) * (size_t) n;
        for (int32_t e = (int32_t) threadIdx.x; e < n; e += kSdLdsThreads) {
            const int32_t x = e / A.n_bins, i = e - x * A.n_bins;
            cur[e] = c == 0 ? sd_element<true>(old, A.init, A.cond, A.order, A.C, A.n_bins, x, i, sh)
                            : sd_element<false>(old, A.init, A.cond, A.order, A.C, A.n_bins, x, i, sh);
        }
        __syncthreads();
    }
    const double *const last = sd_lds + (size_t) ((W - 1) & 1) * (size_t) n;
    double *const row = A.out + (size_t) (A.out_by_motif ? A.mot[k] : (int32_t) blockIdx.x) * (size_t) A.n_bins;
    for (int32_t i = (int32_t) threadIdx.x; i < A.n_bins; i += kSdLdsThreads) row[i] = sd_context_sum(last, A.C, A.n_bins, i);
}

// ---- global path, column c: grid = (bin tiles, contexts, the batch's motifs)
template <bool FIRST>
__global__ void __launch_bounds__(kSdThreads) scoredist_column_kernel(const SdArgs A, int32_t k0, int32_t c) {
    const int32_t k = k0 + (int32_t) blockIdx.z;
    if (A.width[k] <= c) return;
    const int32_t *__restrict__ shift = A.shift + ((size_t) A.col_first[k] + (size_t) c) * 4;
    const int32_t sh[4] = {shift[0], shift[1], shift[2], shift[3]};
    const size_t n = (size_t) A.C * (size_t) A.n_bins;
    double *const base = A.buf + (size_t) blockIdx.z * 2 * n;
    double *const cur = base + (size_t) (c & 1) * n;
    const double *const old = base + (size_t) ((c & 1) ^ 1) * n;
    const int32_t x = (int32_t) blockIdx.y;
    const int32_t i0 = (int32_t) blockIdx.x * kSdTileBins + (int32_t) threadIdx.x;
#pragma unroll
    for (int r = 0; r < kSdTileBins / kSdThreads; r++) {
        const int32_t i = i0 + r * kSdThreads;
        if (i < A.n_bins) cur[(size_t) x * (size_t) A.n_bins + (size_t) i] = sd_element<FIRST>(old, A.init, A.cond, A.order, A.C, A.n_bins, x, i, sh);
    }
}

// ---- global path, the context sum: grid = (bin tiles, the batch's motifs)
__global__ void __launch_bounds__(kSdThreads) scoredist_reduce_kernel(const SdArgs A, int32_t k0) {
    const int32_t k = k0 + (int32_t) blockIdx.y;
    const size_t n = (size_t) A.C * (size_t) A.n_bins;
    const double *const last = A.buf + (size_t) blockIdx.y * 2 * n + (size_t) ((A.width[k] - 1) & 1) * n;
    double *const row = A.out + (size_t) (A.out_by_motif ? A.mot[k] : (int32_t) blockIdx.y) * (size_t) A.n_bins;
    const int32_t i0 = (int32_t) blockIdx.x * kSdTileBins + (int32_t) threadIdx.x;
#pragma unroll
    for (int r = 0; r < kSdTileBins / kSdThreads; r++) {
        const int32_t i = i0 + r * kSdThreads;
        if (i < A.n_bins) row[i] = sd_context_sum(last, A.C, A.n_bins, i);
    }
}

}  // namespace

}  // namespace ms

using namespace ms;

extern "C" {

int ms_debug_scoredist_dims(int32_t out[4]) {
    if (!out) { set_error("NULL output"); return MS_ERR_INVALID; }
    out[0] = kSdThreads;
    out[1] = kSdTileBins;
    out[2] = kSdLdsElems;
    out[3] = (int32_t) kSdBudgetMiB;
    return MS_OK;
}

int ms_debug_scoredist_budget(int64_t bytes, int64_t *previous) {
    if (bytes < 0) { set_error("budget must be >= 0 (0 = the library's own)"); return MS_ERR_INVALID; }
    const int64_t old = g_sd_budget.exchange(bytes);
    if (previous) *previous = old;
    return MS_OK;
}

int ms_debug_scoredist_force_global(int32_t on, int32_t *previous) {
    const int32_t old = g_sd_force_global.exchange(on != 0 ? 1 : 0);
    if (previous) *previous = old;
    return MS_OK;
}

int ms_pwmset_score_distribution(const ms_pwmset *pwms, int strand, int32_t order, const double *cond, const double *init, int32_t n_bins, double *step, int64_t *s0,
                                 double *mass, double *device_ms) {
    if (!require_device()) return MS_ERR_RUNTIME;
    if (device_ms) *device_ms = 0.0;
    if (!pwms) { set_error("NULL handle"); return MS_ERR_INVALID; }
    if (strand != 1 && strand != 2) { set_error("invalid strand %d (1 forward, 2 reverse)", strand); return MS_ERR_INVALID; }
    if (order < 0 || order > MS_SCOREDIST_MAX_ORDER) { set_error("order must be in [0, %d]", MS_SCOREDIST_MAX_ORDER); return MS_ERR_INVALID; }
    if (n_bins < pwms->max_width + 3 || n_bins > MS_SCOREDIST_MAX_BINS) {
        set_error("n_bins must be in [the widest motif + 3 = %d, %d]", pwms->max_width + 3, MS_SCOREDIST_MAX_BINS);
        return MS_ERR_INVALID;
    }
    if (!cond || !init) { set_error("NULL array"); return MS_ERR_INVALID; }
    const int32_t P = pwms->P;
    const int32_t C = 1 << (2 * order);
    for (int32_t i = 0; i < 4 * C; i++)
        if (!(std::isfinite(cond[i]) && cond[i] >= 0.0)) { set_error("cond[%d][%d] is negative or not finite", i / 4, i % 4); return MS_ERR_INVALID; }
    for (int32_t i = 0; i < C; i++)
        if (!(std::isfinite(init[i]) && init[i] >= 0.0)) { set_error("init[%d] is negative or not finite", i); return MS_ERR_INVALID; }
    if (P == 0) return MS_OK;
    if (!step || !s0 || !mass) { set_error("NULL array"); return MS_ERR_INVALID; }
    const int device = current_device();
    int other = -1;
    const int place = pointer_place(mass, device, &other);
    if (place < 0) { set_error("mass lives on device %d, the calling thread is on device %d", other, device); return MS_ERR_INVALID; }
    const bool on_dev = place > 0;

    // ---- the plan, on the host: the grid of every motif and the batches
    const int64_t set = g_sd_budget.load();
    SdPlan plan;
    SdStatus ps;
    try {
        ps = sd_plan(pwms->values.data(), pwms->val_off.data(), pwms->widths.data(), P, strand, order, n_bins, set > 0 ? set : kSdBudgetMiB << 20, kSdBatchCap, &plan);
    } catch (const std::bad_alloc &) { set_error("out of host memory"); return MS_ERR_NOMEM; }
    if (ps == kSdNoRoom) {
        set_error("the two buffers of one motif (%lld bytes at order %d with %d bins) do not fit the work budget", (long long) plan.motif_bytes, order, n_bins);
        return MS_ERR_NOMEM;
    }
    if (ps == kSdNoFit) { set_error("motif %d: the quantised scores do not fit %d bins (entries too large against their range)", plan.bad, n_bins); return MS_ERR_INTERNAL; }
    std::memcpy(step, plan.step.data(), 8 * (size_t) P);
    std::memcpy(s0, plan.s0.data(), 8 * (size_t) P);
    const int32_t n_mot = (int32_t) plan.mot.size();
    const size_t row_bytes = 8 * (size_t) n_bins;

    DeviceCtx *c;
    int rc = get_ctx(device, &c);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk_dev(c->mu);
    MS_HIP(hipSetDevice(c->device));
    const hipStream_t st = c->stream;

    // the rows of the motifs the device does not compute: all +0.0
    {
        int32_t k = 0;
        for (int32_t m = 0; m < P; m++) {
            if (k < n_mot && plan.mot[(size_t) k] == m) { k++; continue; }
            if (!on_dev) std::memset(mass + (size_t) m * (size_t) n_bins, 0, row_bytes);
            else MS_HIP(hipMemsetAsync(mass + (size_t) m * (size_t) n_bins, 0, row_bytes, st));
        }
    }
    if (n_mot == 0) {
        MS_HIP(hipStreamSynchronize(st));
        return MS_OK;
    }

    const size_t elems = (size_t) C * (size_t) n_bins;
    const bool lds_path = !g_sd_force_global.load() && 16 * elems <= std::min(c->lds_max, kSdLdsBytes);
    int32_t per = 0;                                       // the motifs of the largest batch
    for (size_t b = 0; b + 1 < plan.batch_first.size(); b++) per = std::max(per, plan.batch_first[b + 1] - plan.batch_first[b]);
    Carve cv;
    const auto s_mot = cv.add<int32_t>((size_t) n_mot), s_width = cv.add<int32_t>((size_t) n_mot), s_first = cv.add<int32_t>((size_t) n_mot + 1);
    const auto s_shift = cv.add<int32_t>(plan.shift.size());
    const auto s_cond = cv.add<double>(4 * (size_t) C), s_init = cv.add<double>((size_t) C);
    const auto s_stage = cv.add<double>(on_dev ? 0 : (size_t) per * (size_t) n_bins);
    const auto s_buf = cv.add<double>(lds_path ? 0 : (size_t) per * 2 * elems);
    void *wblk = nullptr;
    size_t wgot = 0;
    if ((rc = pool_alloc(c, cv.bytes() + 256, &wblk, &wgot))) return rc;
    auto fail = [&](int code) { (void) hipStreamSynchronize(st); pool_free(c, wblk, wgot); return code; };

    hipError_t he = hipMemcpyAsync(Carve::at(wblk, s_mot), plan.mot.data(), 4 * (size_t) n_mot, hipMemcpyHostToDevice, st);
    if (he == hipSuccess) he = hipMemcpyAsync(Carve::at(wblk, s_width), plan.width.data(), 4 * (size_t) n_mot, hipMemcpyHostToDevice, st);
    if (he == hipSuccess) he = hipMemcpyAsync(Carve::at(wblk, s_first), plan.col_first.data(), 4 * ((size_t) n_mot + 1), hipMemcpyHostToDevice, st);
    if (he == hipSuccess) he = hipMemcpyAsync(Carve::at(wblk, s_shift), plan.shift.data(), 4 * plan.shift.size(), hipMemcpyHostToDevice, st);
    if (he == hipSuccess) he = hipMemcpyAsync(Carve::at(wblk, s_cond), cond, 32 * (size_t) C, hipMemcpyHostToDevice, st);
    if (he == hipSuccess) he = hipMemcpyAsync(Carve::at(wblk, s_init), init, 8 * (size_t) C, hipMemcpyHostToDevice, st);
    if (he != hipSuccess) return fail(hip_rc(he, "upload of the plan"));

    SdArgs A;
    A.mot = Carve::at(wblk, s_mot); A.width = Carve::at(wblk, s_width); A.col_first = Carve::at(wblk, s_first); A.shift = Carve::at(wblk, s_shift);
    A.cond = Carve::at(wblk, s_cond); A.init = Carve::at(wblk, s_init);
    A.buf = lds_path ? nullptr : Carve::at(wblk, s_buf);
    A.out = on_dev ? mass : Carve::at(wblk, s_stage);
    A.out_by_motif = on_dev ? 1 : 0;
    A.order = order; A.C = C; A.n_bins = n_bins;
    if (lds_path && (rc = dense_raise_lds(c, reinterpret_cast<const void *>(scoredist_lds_kernel), 16 * elems, std::min(c->lds_max, kSdLdsBytes)))) return fail(rc);

    const unsigned tiles = (unsigned) ((n_bins + kSdTileBins - 1) / kSdTileBins);
    (void) hipEventRecord(c->ev[0], st);
    for (size_t b = 0; b + 1 < plan.batch_first.size(); b++) {
        const int32_t k0 = plan.batch_first[b], nb = plan.batch_first[b + 1] - k0;
        if (lds_path) {
            hipLaunchKernelGGL(scoredist_lds_kernel, dim3((unsigned) nb), dim3(kSdLdsThreads), 16 * elems, st, A, k0);
            if ((he = hipGetLastError()) != hipSuccess) return fail(hip_rc(he, "score-distribution kernel (LDS)"));
        } else {
            int32_t wmax = 0;
            for (int32_t k = k0; k < k0 + nb; k++) wmax = std::max(wmax, plan.width[(size_t) k]);
            const dim3 grid(tiles, (unsigned) C, (unsigned) nb);
            for (int32_t col = 0; col < wmax; col++) {
                if (col == 0) hipLaunchKernelGGL(scoredist_column_kernel<true>, grid, dim3(kSdThreads), 0, st, A, k0, col);
                else hipLaunchKernelGGL(scoredist_column_kernel<false>, grid, dim3(kSdThreads), 0, st, A, k0, col);
                if ((he = hipGetLastError()) != hipSuccess) return fail(hip_rc(he, "score-distribution column kernel"));
            }
            hipLaunchKernelGGL(scoredist_reduce_kernel, dim3(tiles, (unsigned) nb), dim3(kSdThreads), 0, st, A, k0);
            if ((he = hipGetLastError()) != hipSuccess) return fail(hip_rc(he, "score-distribution reduce kernel"));
        }
        if (b + 2 == plan.batch_first.size()) (void) hipEventRecord(c->ev[1], st);
        if (!on_dev) {                                     // the batch's staging rows to the caller's rows; the next batch reuses them in stream order
            for (int32_t k = k0; k < k0 + nb && he == hipSuccess; k++)
                he = hipMemcpyAsync(mass + (size_t) plan.mot[(size_t) k] * (size_t) n_bins, A.out + (size_t) (k - k0) * (size_t) n_bins, row_bytes, hipMemcpyDeviceToHost, st);
            if (he != hipSuccess) return fail(hip_rc(he, "copy of the distribution"));
        }
    }
    if ((he = hipStreamSynchronize(st)) != hipSuccess) return fail(hip_rc(he, "score distribution"));
    float ms01 = 0;
    (void) hipEventElapsedTime(&ms01, c->ev[0], c->ev[1]);
    if (device_ms) *device_ms = ms01;
    pool_free(c, wblk, wgot);
    return MS_OK;
}

}  // extern "C"
