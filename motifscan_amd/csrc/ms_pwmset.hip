// ms_pwmset.hip -- the PWM set handle: creation and cutoffs, its lazily cached device copies and pre-filter plan, the two scoring entry
// points that need nothing else (ms_score, ms_score_ranks) and the host-only plan views of include/motifscan_amd_debug.h.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <climits>
#include <cstring>
#include <memory>
#include <mutex>
#include <thread>

#include "ms_device.h"
#include "ms_handles.h"

namespace ms {

// -------------------------------------------------------------------------- score --

constexpr int64_t kRankBudget = 1LL << 27;       // scores held at once by ms_score_ranks: its motifs go in batches of kRankBudget / R
static std::atomic<int64_t> g_rank_budget{0};    // ms_debug_score_rank_budget: 0 = kRankBudget
int64_t score_rank_budget_default() { return kRankBudget; }

// c_score (cscore.c:191-224): one thread per (sequence, motif); first W bases only.
__global__ void __launch_bounds__(256) score_kernel(const DevSeq S, const DevPwm Pw, int strand_mask,
                                                    double *__restrict__ out) {
    const int64_t r = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    const int32_t p = blockIdx.y;
    if (r >= S.R) return;
    const int W = Pw.width[p];
    const int64_t start = S.offsets[r];
    const int64_t len = S.offsets[r + 1] - start;
    const double2 *__restrict__ tab = Pw.tab2 + Pw.tab_off[p];
    double fwd = 0.0, rev = 0.0;
    const int n = (int) (len < W ? len : W);          // bases past the sequence end add nothing
    for (int c0 = 0; c0 < n; c0 += 32) {
        const uint64_t cw = code_window(S.codes, start + c0);
        const uint32_t nw = n_window(S.nmask, start + c0);
        const int m = (n - c0) < 32 ? (n - c0) : 32;
        for (int c = 0; c < m; c++) {
            if ((nw >> c) & 1u) continue;
            const uint32_t b = (uint32_t) (cw >> (2 * c)) & 3u;
            const double2 t = tab[(c0 + c) * 4 + b];
            fwd += t.x;
            rev += t.y;
        }
    }
    double s = 0.0;
    switch (strand_mask) {                               // cscore.c:208-222
        case 1: s = fwd; break;
        case 2: s = rev; break;
        case 3: s = fwd > rev ? fwd : rev; break;
    }
    out[(int64_t) p * S.R + r] = s / Pw.max_raw[p];
}

// out[k] = sorted[ranks[k]]  (ranks beyond the row give NaN)
__global__ void gather_ranks_kernel(const double *__restrict__ sorted, int64_t n, const int64_t *__restrict__ ranks,
                                    int32_t n_ranks, double *__restrict__ out) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_ranks) return;
    const int64_t r = ranks[k];
    out[k] = (r >= 0 && r < n) ? sorted[r] : __longlong_as_double(0x7FF8000000000000LL);
}

static int launch_gather_ranks(const double *sorted, int64_t n, const int64_t *ranks, int32_t n_ranks, double *out, hipStream_t st) {
    if (n_ranks <= 0) return MS_OK;
    hipLaunchKernelGGL(gather_ranks_kernel, dim3((unsigned) ((n_ranks + 63) / 64)), dim3(64), 0, st, sorted, n, ranks, n_ranks, out);
    MS_HIP(hipGetLastError());
    return MS_OK;
}

static int launch_score(const DevSeq &S, const DevPwm &Pw, int strand_mask, double *out, hipStream_t st) {
    if (S.R == 0 || Pw.P == 0) return MS_OK;
    for (int32_t p0 = 0; p0 < Pw.P; p0 += 32768) {
        const int32_t n = Pw.P - p0 < 32768 ? Pw.P - p0 : 32768;
        DevPwm sub = Pw;
        sub.tab_off += p0; sub.width += p0; sub.max_raw += p0; sub.cutoff += p0; sub.raw_floor += p0; sub.P = n;
        dim3 grid((unsigned) ((S.R + 255) / 256), (unsigned) n);
        hipLaunchKernelGGL(score_kernel, grid, dim3(256), 0, st, S, sub, strand_mask, out + (int64_t) p0 * S.R);
        MS_HIP(hipGetLastError());
    }
    return MS_OK;
}

// C-style max_raw: column maxima start at 0 (cscore.c:36-48)
static double c_max_raw(const double *m, int W) {
    double total = 0;
    for (int c = 0; c < W; c++) {
        double best = 0;
        for (int b = 0; b < 4; b++)
            if (m[(int64_t) b * W + c] > best) best = m[(int64_t) b * W + c];
        total += best;
    }
    return total;
}

static void pwmset_free_device(ms_pwmset *p) {
    if (p->device >= 0 || p->plan_device >= 0) (void) hipSetDevice(p->device >= 0 ? p->device : p->plan_device);
    dev_free(p->d_tab2); dev_free(p->d_tab_off); dev_free(p->d_width); dev_free(p->d_max_raw); dev_free(p->d_cutoff); dev_free(p->d_raw_floor); dev_free(p->d_thresh);
    dev_free(p->d_tables); dev_free(p->d_tiles); dev_free(p->d_group_fields); dev_free(p->d_exact_motifs); dev_free(p->d_field_meta);
    p->device = -1;
    p->plan_device = -1;
    p->dev_cutoff_version = 0;
}

int pwmset_upload(ms_pwmset *p, int device, hipStream_t st) {
    if (p->device != device) {
        pwmset_free_device(p);
        MS_HIP(hipSetDevice(device));
        size_t total_w = 0;
        for (int32_t i = 0; i < p->P; i++) total_w += (size_t) p->widths[i];
        std::vector<double2> tab(total_w * 4 + 1);       // (+ one all-zero entry at the end: what a column that adds nothing reads, DevPwm::zero_bytes)
        tab[total_w * 4].x = 0.0;
        tab[total_w * 4].y = 0.0;
        std::vector<int64_t> off(p->P);
        size_t o = 0;
        for (int32_t i = 0; i < p->P; i++) {
            const int W = p->widths[i];
            const double *m = p->values.data() + p->val_off[i];
            off[i] = (int64_t) o;
            for (int c = 0; c < W; c++)
                for (int b = 0; b < 4; b++) {
                    double2 t;
                    t.x = m[(int64_t) b * W + c];
                    t.y = m[(int64_t) (3 - b) * W + (W - 1 - c)];       // cscore.c:351
                    tab[o + (size_t) c * 4 + b] = t;
                }
            o += (size_t) W * 4;
        }
        p->tab2_entries = (int64_t) total_w * 4;
        p->tab_off_host = off;
        int rc;
        if ((rc = dev_alloc(&p->d_tab2, tab.size()))) return rc;
        if ((rc = dev_alloc(&p->d_tab_off, (size_t) p->P))) return rc;
        if ((rc = dev_alloc(&p->d_width, (size_t) p->P))) return rc;
        if ((rc = dev_alloc(&p->d_max_raw, (size_t) p->P))) return rc;
        if ((rc = dev_alloc(&p->d_cutoff, (size_t) p->P))) return rc;
        if ((rc = dev_alloc(&p->d_raw_floor, (size_t) p->P))) return rc;
        if ((rc = dev_alloc(&p->d_thresh, (size_t) p->P * 4 + 4))) return rc;
        if (p->P > 0) {
            MS_HIP(hipMemcpy(p->d_tab2, tab.data(), tab.size() * sizeof(double2), hipMemcpyHostToDevice));
            MS_HIP(hipMemcpy(p->d_tab_off, off.data(), off.size() * sizeof(int64_t), hipMemcpyHostToDevice));
            MS_HIP(hipMemcpy(p->d_width, p->widths.data(), (size_t) p->P * sizeof(int32_t), hipMemcpyHostToDevice));
            MS_HIP(hipMemcpy(p->d_max_raw, p->max_raw.data(), (size_t) p->P * sizeof(double), hipMemcpyHostToDevice));
        }
        p->device = device;
        p->dev_cutoff_version = 0;
    }
    if (p->dev_cutoff_version != p->cutoff_version) {
        if (p->P > 0) {
            MS_HIP(hipMemcpy(p->d_cutoff, p->cutoffs.data(), (size_t) p->P * sizeof(double), hipMemcpyHostToDevice));
            // raw-sum floor of the hit test (same bound as ms_plan.cpp's T, with twice its slack): a window whose
            // fp64 column sum is below it fails `sum / max_raw - cutoff >= -1e-10` for sure
            std::vector<double> fl((size_t) p->P);
            for (int32_t i = 0; i < p->P; i++) {
                const int W = p->widths[i];
                const double *m = p->values.data() + p->val_off[i];
                double abs_sum = 0;
                bool finite = std::isfinite(p->max_raw[i]) && p->max_raw[i] > 0 && std::isfinite(p->cutoffs[i]);
                for (int c = 0; c < W && finite; c++) {
                    double colmax = 0;
                    for (int b = 0; b < 4; b++) {
                        const double v = m[(int64_t) b * W + c];
                        if (!std::isfinite(v)) { finite = false; break; }
                        colmax = std::max(colmax, std::fabs(v));
                    }
                    abs_sum += colmax;
                }
                fl[(size_t) i] = finite ? (p->cutoffs[i] - 1e-10) * p->max_raw[i] - 2e-9 * (1.0 + abs_sum) : -INFINITY;
            }
            MS_HIP(hipMemcpy(p->d_raw_floor, fl.data(), (size_t) p->P * sizeof(double), hipMemcpyHostToDevice));
            std::vector<double> th((size_t) p->P * 4, 0.0);              // the hit test's three numbers side by side (rescore_kernel: one 16-byte + one 8-byte read)
            for (int32_t i = 0; i < p->P; i++) { th[4 * (size_t) i] = p->max_raw[i]; th[4 * (size_t) i + 1] = p->cutoffs[i]; th[4 * (size_t) i + 2] = fl[(size_t) i]; }
            p->raw_floor_host = fl;
            MS_HIP(hipMemcpy(p->d_thresh, th.data(), th.size() * sizeof(double), hipMemcpyHostToDevice));
        }
        p->dev_cutoff_version = p->cutoff_version;
    }
    (void) st;
    return MS_OK;
}

int pwmset_plan(ms_pwmset *p, int strand_mask, size_t lds_budget, bool exact_only, bool need_device,
                       int device) {
    const char *pe = measure_env("MS_PF_PAIR");                          // measurement only: "0" = no paired rows
    const bool pair_rows = !(pe && pe[0] == '0');
    const bool stale = p->plan_strand != strand_mask || p->plan_cutoff_version != p->cutoff_version ||
                       p->plan_lds != lds_budget || p->plan_exact_only != exact_only || p->plan_pair != pair_rows;
    if (stale) {
        if (exact_only) {
            p->plan = PrefilterPlan();
            p->plan.strand_mask = strand_mask;
            for (int32_t i = 0; i < p->P; i++) p->plan.exact_motifs.push_back(i);
        } else {
            int rc = build_plan(p->values.data(), p->val_off.data(), p->widths.data(), p->cutoffs.data(), p->max_raw.data(),
                                p->P, strand_mask, lds_budget, pair_rows, &p->plan);
            if (rc) return rc;
        }
        p->plan_strand = strand_mask;
        p->plan_pair = pair_rows;
        p->plan_cutoff_version = p->cutoff_version;
        p->plan_lds = lds_budget;
        p->plan_exact_only = exact_only;
        if (p->plan_device >= 0) {
            (void) hipSetDevice(p->plan_device);
            dev_free(p->d_tables); dev_free(p->d_tiles); dev_free(p->d_group_fields); dev_free(p->d_exact_motifs); dev_free(p->d_field_meta);
            p->plan_device = -1;
        }
    }
    if (need_device && p->plan_device != device) {
        MS_HIP(hipSetDevice(device));
        const PrefilterPlan &pl = p->plan;
        int rc;
        if ((rc = dev_alloc(&p->d_tables, pl.tables.size() / 4))) return rc;
        if ((rc = dev_alloc(&p->d_tiles, pl.tiles.size()))) return rc;
        if ((rc = dev_alloc(&p->d_group_fields, pl.group_fields.size()))) return rc;
        if ((rc = dev_alloc(&p->d_exact_motifs, pl.exact_motifs.size()))) return rc;
        if (!pl.tables.empty())
            MS_HIP(hipMemcpy(p->d_tables, pl.tables.data(), pl.tables.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        if (!pl.tiles.empty())
            MS_HIP(hipMemcpy(p->d_tiles, pl.tiles.data(), pl.tiles.size() * sizeof(TileDesc), hipMemcpyHostToDevice));
        if (!pl.group_fields.empty())
            MS_HIP(hipMemcpy(p->d_group_fields, pl.group_fields.data(), pl.group_fields.size() * sizeof(int32_t),
                             hipMemcpyHostToDevice));
        if (!pl.exact_motifs.empty())
            MS_HIP(hipMemcpy(p->d_exact_motifs, pl.exact_motifs.data(), pl.exact_motifs.size() * sizeof(int32_t),
                             hipMemcpyHostToDevice));
        {   // per field of every table group: motif, width, table offset (pwmset_upload has run: scan_locked's order)
            std::vector<FieldMeta> fmv(pl.group_fields.size());
            for (size_t i = 0; i < fmv.size(); i++) {
                const int32_t m = pl.group_fields[i];
                fmv[i].motif = m;
                fmv[i].width = m >= 0 ? p->widths[m] : 0;
                fmv[i].tab_bytes = m >= 0 && (size_t) m < p->tab_off_host.size() ? (uint32_t) ((uint64_t) p->tab_off_host[m] * sizeof(double2)) : 0u;
                float f32 = -INFINITY;                          // rounded DOWN: never above the fp64 floor
                if (m >= 0 && (size_t) m < p->raw_floor_host.size() && std::isfinite(p->raw_floor_host[m])) {
                    f32 = (float) p->raw_floor_host[m];
                    if ((double) f32 > p->raw_floor_host[m] || !std::isfinite(f32)) f32 = std::isfinite(f32) ? std::nextafterf(f32, -INFINITY) : -INFINITY;
                }
                fmv[i].floor32 = f32;
            }
            if ((rc = dev_alloc(&p->d_field_meta, fmv.size() + 1))) return rc;
            if (!fmv.empty()) MS_HIP(hipMemcpy(p->d_field_meta, fmv.data(), fmv.size() * sizeof(FieldMeta), hipMemcpyHostToDevice));
        }
        p->plan_device = device;
    }
    return MS_OK;
}

DevPwm dev_pwm(const ms_pwmset *p) {
    DevPwm d;
    d.tab2 = p->d_tab2; d.tab_off = p->d_tab_off; d.width = p->d_width; d.max_raw = p->d_max_raw;
    d.thresh = p->d_thresh;
    d.zero_bytes = (uint32_t) ((uint64_t) p->tab2_entries * sizeof(double2));
    d.tab32 = (uint64_t) (p->tab2_entries + 1) * sizeof(double2) <= 0xFFFFFFFFull ? 1 : 0;
    d.cutoff = p->d_cutoff; d.raw_floor = p->d_raw_floor; d.P = p->P;
    return d;
}

}  // namespace ms

using namespace ms;

extern "C" {

// ------------------------------------------------------------------------- PWM set --

int ms_pwmset_create(const double *values, const int32_t *widths, const double *cutoffs, int32_t n_pwms,
                     ms_pwmset **out) {
    if (!out) { set_error("out is NULL"); return MS_ERR_INVALID; }
    *out = nullptr;
    if (n_pwms < 0 || n_pwms > kMaxMotifs) { set_error("n_pwms must be in [0, %d]", kMaxMotifs); return MS_ERR_INVALID; }
    if (n_pwms > 0 && (!values || !widths)) { set_error("values / widths is NULL"); return MS_ERR_INVALID; }
    std::unique_ptr<ms_pwmset> p(new (std::nothrow) ms_pwmset());
    if (!p) { set_error("out of host memory"); return MS_ERR_NOMEM; }
    p->P = n_pwms;
    p->val_off.assign((size_t) n_pwms + 1, 0);
    for (int32_t i = 0; i < n_pwms; i++) {
        if (widths[i] < 1) { set_error("PWM %d has width %d (need >= 1 position per row)", i, widths[i]); return MS_ERR_INVALID; }
        p->val_off[i + 1] = p->val_off[i] + 4 * (int64_t) widths[i];
        p->max_width = std::max(p->max_width, (int) widths[i]);
    }
    try {
        p->values.assign(values, values + p->val_off[n_pwms]);
        p->widths.assign(widths, widths + n_pwms);
        p->cutoffs.assign((size_t) n_pwms, 1.0);                       // cscore.c:70-74
        if (cutoffs) p->cutoffs.assign(cutoffs, cutoffs + n_pwms);
        p->max_raw.resize((size_t) n_pwms);
    } catch (const std::bad_alloc &) { set_error("out of host memory"); return MS_ERR_NOMEM; }
    for (int32_t i = 0; i < n_pwms; i++) p->max_raw[i] = c_max_raw(p->values.data() + p->val_off[i], widths[i]);
    *out = p.release();
    return MS_OK;
}

int ms_pwmset_set_cutoffs(ms_pwmset *p, const double *cutoffs) {
    if (!p || (!cutoffs && p->P > 0)) { set_error("NULL argument"); return MS_ERR_INVALID; }
    std::lock_guard<std::mutex> lk(p->mu);
    if (p->P > 0) p->cutoffs.assign(cutoffs, cutoffs + p->P);
    p->cutoff_version++;
    return MS_OK;
}

int ms_pwmset_size(const ms_pwmset *p, int32_t *n_pwms) {
    if (!p || !n_pwms) { set_error("NULL argument"); return MS_ERR_INVALID; }
    *n_pwms = p->P;
    return MS_OK;
}

int ms_pwmset_max_raw(const ms_pwmset *p, double *out) {
    if (!p || (!out && p->P > 0)) { set_error("NULL argument"); return MS_ERR_INVALID; }
    if (p->P > 0) std::memcpy(out, p->max_raw.data(), (size_t) p->P * sizeof(double));
    return MS_OK;
}

void ms_pwmset_free(ms_pwmset *p) {
    if (!p) return;
    pwmset_free_device(p);
    delete p;
}

// --------------------------------------------------------------------------- score --

int ms_score(const ms_pwmset *pwms_c, const ms_seqset *seqs, int strand_mask, double *out) {
    if (!pwms_c || !seqs) { set_error("NULL handle"); return MS_ERR_INVALID; }
    if (strand_mask < 1 || strand_mask > 3) { set_error("invalid strand mask %d", strand_mask); return MS_ERR_INVALID; }
    ms_pwmset *pwms = const_cast<ms_pwmset *>(pwms_c);
    if (pwms->P == 0 || seqs->R == 0) return MS_OK;
    if (!out) { set_error("out is NULL"); return MS_ERR_INVALID; }
    DeviceCtx *c;
    int rc = get_ctx(seqs->device, &c);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk_dev(c->mu);
    std::lock_guard<std::mutex> lk_pwm(pwms->mu);
    if ((rc = pwmset_upload(pwms, c->device, c->stream))) return rc;
    double *d_out = nullptr;
    const size_t n = (size_t) pwms->P * (size_t) seqs->R;
    if ((rc = dev_alloc(&d_out, n))) return rc;
    rc = launch_score(dev_seq(seqs), dev_pwm(pwms), strand_mask, d_out, c->stream);
    hipError_t he = hipSuccess;
    if (!rc) he = hipMemcpyAsync(out, d_out, n * sizeof(double), hipMemcpyDeviceToHost, c->stream);
    if (!rc && he == hipSuccess) he = hipStreamSynchronize(c->stream);
    dev_free(d_out);
    if (rc) return rc;
    if (he != hipSuccess) { set_error("score kernel failed: %s", hipGetErrorString(he)); return MS_ERR_RUNTIME; }
    return MS_OK;
}

// The cutoff builder's device half (cli/motif.py:134-137, motif/__init__.py:378-401): score R
// sampled sequences with every PWM (c_score), sort each PWM's scores in descending order and read
// the scores at the requested 0-based ranks (the reference takes rank int(n * 0.1**e) - 1).
int ms_score_ranks(const ms_pwmset *pwms_c, const ms_seqset *seqs, int strand_mask, const int64_t *ranks,
                   int32_t n_ranks, double *out) {
    if (!pwms_c || !seqs) { set_error("NULL handle"); return MS_ERR_INVALID; }
    if (strand_mask < 1 || strand_mask > 3) { set_error("invalid strand mask %d", strand_mask); return MS_ERR_INVALID; }
    if (n_ranks < 0 || (n_ranks > 0 && (!ranks || !out))) { set_error("bad ranks / out"); return MS_ERR_INVALID; }
    ms_pwmset *pwms = const_cast<ms_pwmset *>(pwms_c);
    if (pwms->P == 0 || n_ranks == 0) return MS_OK;
    if (seqs->R == 0) { set_error("no sequences to rank"); return MS_ERR_INVALID; }
    DeviceCtx *c;
    int rc = get_ctx(seqs->device, &c);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk_dev(c->mu);
    std::lock_guard<std::mutex> lk_pwm(pwms->mu);
    if ((rc = pwmset_upload(pwms, c->device, c->stream))) return rc;
    const size_t R = (size_t) seqs->R;
    const int64_t set_budget = g_rank_budget.load();
    const size_t budget = (size_t) (set_budget > 0 ? set_budget : kRankBudget);
    const int32_t batch = (int32_t) std::max<size_t>(1, std::min<size_t>((size_t) pwms->P, budget / R));
    double *d_scores = nullptr, *d_sorted = nullptr, *d_out = nullptr;
    int64_t *d_ranks = nullptr;
    unsigned char *d_tmp = nullptr;
    size_t tmp_bytes = 0;
    auto cleanup = [&]() { dev_free(d_scores); dev_free(d_sorted); dev_free(d_out); dev_free(d_ranks); dev_free(d_tmp); };
    if ((rc = dev_alloc(&d_scores, (size_t) batch * R)) || (rc = dev_alloc(&d_sorted, R)) ||
        (rc = dev_alloc(&d_out, (size_t) pwms->P * (size_t) n_ranks)) || (rc = dev_alloc(&d_ranks, (size_t) n_ranks))) { cleanup(); return rc; }
    hipError_t he = hipMemcpyAsync(d_ranks, ranks, (size_t) n_ranks * sizeof(int64_t), hipMemcpyHostToDevice, c->stream);
    if (he == hipSuccess && (rc = sort_doubles_desc(nullptr, &tmp_bytes, d_scores, d_sorted, R, c->stream)) == MS_OK)
        rc = dev_alloc(&d_tmp, tmp_bytes);
    const DevSeq S = dev_seq(seqs);
    for (int32_t p0 = 0; rc == MS_OK && he == hipSuccess && p0 < pwms->P; p0 += batch) {
        const int32_t n = std::min(batch, pwms->P - p0);
        DevPwm sub = dev_pwm(pwms);
        sub.tab_off += p0; sub.width += p0; sub.max_raw += p0; sub.cutoff += p0; sub.raw_floor += p0; sub.P = n;
        rc = launch_score(S, sub, strand_mask, d_scores, c->stream);
        for (int32_t i = 0; rc == MS_OK && i < n; i++) {
            size_t tb = tmp_bytes;
            rc = sort_doubles_desc(d_tmp, &tb, d_scores + (size_t) i * R, d_sorted, R, c->stream);
            if (rc == MS_OK) rc = launch_gather_ranks(d_sorted, (int64_t) R, d_ranks, n_ranks, d_out + (size_t) (p0 + i) * n_ranks, c->stream);
        }
    }
    if (rc == MS_OK && he == hipSuccess)
        he = hipMemcpyAsync(out, d_out, (size_t) pwms->P * (size_t) n_ranks * sizeof(double), hipMemcpyDeviceToHost, c->stream);
    if (rc == MS_OK && he == hipSuccess) he = hipStreamSynchronize(c->stream);
    else (void) hipStreamSynchronize(c->stream);
    cleanup();
    if (rc) return rc;
    if (he != hipSuccess) { set_error("score/rank kernels failed: %s", hipGetErrorString(he)); return MS_ERR_RUNTIME; }
    return MS_OK;
}

int ms_debug_score_rank_budget(int64_t elems, int64_t *previous) {
    if (elems < 0) { set_error("budget must be >= 0 (0 = the library's own)"); return MS_ERR_INVALID; }
    const int64_t old = g_rank_budget.exchange(elems);
    if (previous) *previous = old;
    return MS_OK;
}

// ------------------------------------------------------------------ test inspection --
// Host-only views of the pre-filter plan, so CPU tests can prove the quantiser never drops a
// window the reference reports (tests/test_host_cabi.py).  Not part of the drop-in surface.

int ms_debug_plan_dims(const ms_pwmset *pwms_c, int strand_mask, int64_t lds_budget, int32_t *n_fast,
                       int32_t *n_exact, int32_t *n_groups, int32_t *n_tiles) {
    if (!pwms_c) { set_error("NULL handle"); return MS_ERR_INVALID; }
    if (strand_mask < 1 || strand_mask > 3) { set_error("invalid strand mask %d", strand_mask); return MS_ERR_INVALID; }
    ms_pwmset *pwms = const_cast<ms_pwmset *>(pwms_c);
    std::lock_guard<std::mutex> lk(pwms->mu);
    int rc = pwmset_plan(pwms, strand_mask, (size_t) lds_budget, false, false, -1);
    if (rc) return rc;
    if (n_fast) *n_fast = (int32_t) pwms->plan.fast_motifs.size();
    if (n_exact) *n_exact = (int32_t) pwms->plan.exact_motifs.size();
    if (n_groups) *n_groups = (int32_t) pwms->plan.group_kb.size();
    if (n_tiles) *n_tiles = (int32_t) pwms->plan.tiles.size();
    return MS_OK;
}

// The plan built by the last ms_debug_plan_dims call, decoded from the PHYSICAL operand image the kernel reads (any pointer
// may be NULL): group_fields [n_groups][16] motif of the field (-1 = empty), rows [n_groups][16 fields][64 columns][4 bases]
// int16 = what the product adds for that base at that column, units of 1/8 (the bias column reads 0 here), bias [n_groups][16]
// = the entry of the field's last column (MS_ERR_RUNTIME if its four bases disagree), group_kb [n_groups] matrix instructions
// per row tile, group_cols [n_groups] columns of the group's fields incl. the bias column (16 per instruction, paired rows: 8),
// group_paired [n_groups] 0 = plain row, 1 / 2 = field X / Y of a paired row, exact_motifs [n_exact], tile_first_group [n_tiles + 1].
int ms_debug_plan_rows(const ms_pwmset *pwms_c, int32_t *group_fields, int16_t *rows, int32_t *bias, int32_t *group_kb,
                       int32_t *group_cols, int32_t *group_paired, int32_t *exact_motifs, int32_t *tile_first_group) {
    if (!pwms_c) { set_error("NULL handle"); return MS_ERR_INVALID; }
    ms_pwmset *pwms = const_cast<ms_pwmset *>(pwms_c);
    std::lock_guard<std::mutex> lk(pwms->mu);
    const PrefilterPlan &pl = pwms->plan;
    if (pwms->plan_strand < 0) { set_error("call ms_debug_plan_dims first"); return MS_ERR_INVALID; }
    const size_t nq = pl.group_kb.size();
    if (group_fields && nq) std::memcpy(group_fields, pl.group_fields.data(), pl.group_fields.size() * sizeof(int32_t));
    if (exact_motifs && !pl.exact_motifs.empty())
        std::memcpy(exact_motifs, pl.exact_motifs.data(), pl.exact_motifs.size() * sizeof(int32_t));
    if (tile_first_group) {
        for (size_t t = 0; t < pl.tiles.size(); t++) tile_first_group[t] = pl.tiles[t].first_group;
        tile_first_group[pl.tiles.size()] = (int32_t) nq;
    }
    const uint8_t *bytes = reinterpret_cast<const uint8_t *>(pl.tables.data());
    for (size_t q = 0; q < nq; q++) {
        const GroupInfo &gi = pl.group_info[q];
        const int n_cols = pl.group_cols[q];
        const uint8_t *tab = bytes + gi.tab_off;
        // column c of the field: plain rows -- column c % 16 of k-block c / 16; paired rows -- column c % 8 of half-block c / 8 in k-half `sel`
        auto entry = [&](int row, int c, int b) {
            return gi.paired ? f6_value(f6_get(tab, gi.nk, c / kPairCols, row, kPairCols * gi.sel + c % kPairCols, b))
                             : f6_value(f6_get(tab, gi.nk, c / kF6Cols, row, c % kF6Cols, b));
        };
        if (group_kb) group_kb[q] = gi.nk;
        if (group_cols) group_cols[q] = n_cols;
        if (group_paired) group_paired[q] = gi.paired ? 1 + gi.sel : 0;
        for (int f = 0; f < kGroupFields; f++) {
            const int row = mfma_row_of(gi.h, f);
            int b0 = entry(row, n_cols - 1, 0);
            if (gi.paired) {                                    // what the kernel's constant B slots make of the four entries, less the field offset
                b0 = -kPairOffset;
                for (int b = 0; b < 4; b++) b0 += kPairBiasW[b] * entry(row, n_cols - 1, b);
            } else {
                for (int b = 1; b < 4; b++)
                    if (entry(row, n_cols - 1, b) != b0) {
                        set_error("bias column of group %zu field %d differs between bases", q, f);
                        return MS_ERR_RUNTIME;
                    }
            }
            if (bias) bias[q * kGroupFields + f] = b0;
            if (rows)
                for (int c = 0; c < kF6Cols * kF6MaxKb; c++)
                    for (int b = 0; b < 4; b++)
                        rows[((q * kGroupFields + f) * (kF6Cols * kF6MaxKb) + c) * 4 + b] = (int16_t) (c < n_cols - 1 ? entry(row, c, b) : 0);       // units of 1/8
        }
    }
    return MS_OK;
}

}  // extern "C"
