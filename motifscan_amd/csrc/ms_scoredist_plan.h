// ms_scoredist_plan.h -- the host's plan of the analytic score distribution (ms_pwmset_score_distribution, ms_scoredist.hip): the score
// grid of every motif (step, s0, the shifts d[c][b] of its quantised entries), the fit assertion, and the batches of motifs whose ping-pong
// buffers share a work budget.  Plain C++, no HIP call, so that it is checked on the CPU (tests/sanitize/scoredist_plan_asan.cpp), as
// ms_place.h and ms_dense_plan.h are.  include/motifscan_amd.h holds the definition this restates; every operation on a double below is
// one rounded IEEE operation (the library and the sanitizer program are built with -ffp-contract=off).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <limits>
#include <vector>

namespace ms {

constexpr int32_t kSdAbsent = -1;                     // the shift of an entry of -inf: the mass that would pass through it is dropped
constexpr double kSdMaxQuant = 4503599627370496.0;    // 2^52: a quantised entry beyond it is refused (the fit assertion fails)

enum SdStatus { kSdOk = 0, kSdUnscorable = 1, kSdNoFit = 2, kSdNoRoom = 3 };

// bytes of one motif's two buffers [2][C][n_bins] of doubles (C = 4^order <= 1024, n_bins <= 2^20: at most 2^34)
inline int64_t sd_motif_bytes(int32_t order, int32_t n_bins) { return 2 * ((int64_t) 1 << (2 * order)) * (int64_t) n_bins * 8; }

// The grid of one motif M[4][W] (row-major, rows A C G T) for n_bins >= W + 3: *step, *s0 and d[W][4] -- the shifts in the order the
// recurrence walks the columns under `strand` (1: d[c][b] of M; 2: of M'[b][c] = M[3 - b][W - 1 - c]); kSdAbsent for an entry of -inf.
// kSdUnscorable: *step = 0, *s0 = 0, d untouched.  kSdNoFit: the fit assertion failed (outputs undefined).
inline SdStatus sd_quantise(const double *M, int32_t W, int32_t n_bins, int strand, double *step, int64_t *s0, int32_t *d) {
    const double inf = std::numeric_limits<double>::infinity();
    *step = 0.0;
    *s0 = 0;
    double max_raw = 0.0, hi = 0.0, lo = 0.0;
    for (int32_t c = 0; c < W; c++) {
        double col = 0.0, mx = -inf, mn = inf;
        for (int b = 0; b < 4; b++) {
            const double v = M[(size_t) b * W + c];
            if (std::isnan(v) || v == inf) return kSdUnscorable;
            if (v > col) col = v;
            if (v == -inf) continue;
            if (v > mx) mx = v;
            if (v < mn) mn = v;
        }
        if (mx == -inf) return kSdUnscorable;          // a column without a finite entry
        max_raw += col;
        hi = hi + mx;
        lo = lo + mn;
    }
    if (!(std::isfinite(max_raw) && max_raw > 0.0)) return kSdUnscorable;
    const double range = hi - lo;
    const double st = hi == lo ? 1.0 : range / (double) (n_bins - W - 2);
    if (!(std::isfinite(st) && st > 0.0)) return kSdNoFit;
    int64_t sum_min = 0, sum_span = 0;
    for (int32_t c = 0; c < W; c++) {
        int64_t q[4], qmin = 0, qmax = 0;
        bool have = false;
        for (int b = 0; b < 4; b++) {
            const double v = M[(size_t) b * W + c];
            q[b] = 0;
            if (v == -inf) continue;
            const double t = std::floor(v / st);
            if (!(std::fabs(t) < kSdMaxQuant)) return kSdNoFit;
            q[b] = (int64_t) t;
            if (!have || q[b] < qmin) qmin = q[b];
            if (!have || q[b] > qmax) qmax = q[b];
            have = true;
        }
        if (__builtin_add_overflow(sum_min, qmin, &sum_min)) return kSdNoFit;
        sum_span += qmax - qmin;                        // (each below 2^53, W of them: no overflow for any width a set takes)
        if (sum_span >= (int64_t) n_bins) return kSdNoFit;
        for (int b = 0; b < 4; b++) {
            const bool absent = M[(size_t) b * W + c] == -inf;
            const int32_t v = absent ? kSdAbsent : (int32_t) (q[b] - qmin);
            if (strand == 2) d[(size_t) (W - 1 - c) * 4 + (size_t) (3 - b)] = v;
            else d[(size_t) c * 4 + (size_t) b] = v;
        }
    }
    *step = st;
    *s0 = sum_min;
    return kSdOk;
}

struct SdPlan {
    std::vector<double> step;            // [P]
    std::vector<int64_t> s0;             // [P]
    std::vector<int32_t> mot;            // the scorable motifs, ascending: the rows the device computes
    std::vector<int32_t> width;          // [mot.size()]
    std::vector<int32_t> col_first;      // [mot.size() + 1] first column of the motif in `shift`
    std::vector<int32_t> shift;          // [columns][4]
    std::vector<int32_t> batch_first;    // [batches + 1] into mot
    int32_t max_w = 0;                   // the widest scorable motif
    int64_t motif_bytes = 0;             // one motif's two buffers
    int32_t bad = -1;                    // kSdNoFit: the motif
};

// The motifs of one batch: as many as the budget holds, at most `cap` (the z of a grid); 0: one motif's buffers do not fit.
inline int32_t sd_batch_motifs(int64_t motif_bytes, int64_t budget, int32_t cap) {
    const int64_t n = budget / motif_bytes;
    return (int32_t) (n < (int64_t) cap ? n : (int64_t) cap);
}

// values / val_off / widths: the set's matrices as ms_pwmset holds them ([4][W] row-major at val_off[m]); n_bins >= the widest motif + 3.
// kSdOk, kSdNoFit (pl->bad) or kSdNoRoom (with P > 0 only; nothing is planned).
inline SdStatus sd_plan(const double *values, const int64_t *val_off, const int32_t *widths, int32_t P, int strand, int32_t order, int32_t n_bins,
                        int64_t budget, int32_t cap, SdPlan *pl) {
    *pl = SdPlan();
    pl->motif_bytes = sd_motif_bytes(order, n_bins);
    pl->step.assign((size_t) P, 0.0);
    pl->s0.assign((size_t) P, 0);
    pl->col_first.push_back(0);
    pl->batch_first.push_back(0);
    if (P == 0) return kSdOk;
    const int32_t per = sd_batch_motifs(pl->motif_bytes, budget, cap);
    if (per < 1) return kSdNoRoom;
    std::vector<int32_t> d;
    for (int32_t m = 0; m < P; m++) {
        const int32_t W = widths[m];
        d.assign((size_t) W * 4, 0);
        const SdStatus s = sd_quantise(values + val_off[m], W, n_bins, strand, &pl->step[(size_t) m], &pl->s0[(size_t) m], d.data());
        if (s == kSdUnscorable) continue;
        if (s != kSdOk) { pl->bad = m; return kSdNoFit; }
        pl->mot.push_back(m);
        pl->width.push_back(W);
        pl->shift.insert(pl->shift.end(), d.begin(), d.end());
        pl->col_first.push_back((int32_t) (pl->shift.size() / 4));
        if (W > pl->max_w) pl->max_w = W;
    }
    const int32_t n = (int32_t) pl->mot.size();
    for (int32_t k = per; k < n; k += per) pl->batch_first.push_back(k);
    if (n > 0) pl->batch_first.push_back(n);
    return kSdOk;
}

}  // namespace ms
