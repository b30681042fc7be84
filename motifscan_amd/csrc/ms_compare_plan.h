// ms_compare_plan.h -- the host's half of the motif comparison (ms_motifs_compare, ms_compare.hip): the columns as the device sees them
// (the prepared vectors of a matrix under a metric), the score grid (lo, scale), the layout of one query's tables -- where the table of
// every (start a, length L) lies -- and the batches of queries whose tables share a work budget.  Plain C++, no HIP call, so that it is
// checked on the CPU (tests/sanitize/compare_plan_asan.cpp), as ms_scoredist_plan.h is.  include/motifscan_amd.h holds the definition
// this restates; every operation on a double below is one rounded IEEE operation (the library and the sanitizer program are built with
// -ffp-contract=off).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define MS_CMP_HD __host__ __device__
#else
#define MS_CMP_HD
#endif

namespace ms {

constexpr int32_t kCmpMaxWidth = 64;                  // MS_COMPARE_MAX_WIDTH
constexpr int32_t kCmpMaxBins = 256;                  // MS_COMPARE_MAX_BINS
constexpr int64_t kCmpMaxColumns = (int64_t) 1 << 30; // the most columns of a target set (and of the queries of one call's range)

enum CmpStatus { kCmpOk = 0, kCmpNoRoom = 1 };

// The prepared vectors of one matrix M[4][W] (row-major, rows A C G T): out[W][4].  metric 0 (pearson): the centred column over its norm,
// all +0.0 where the norm is not > 0; metrics 1, 2 (sw, ed): the column itself.
inline void cmp_prepare(const double *M, int32_t W, int metric, double *out) {
    for (int32_t c = 0; c < W; c++) {
        const double x0 = M[c], x1 = M[(size_t) W + c], x2 = M[2 * (size_t) W + c], x3 = M[3 * (size_t) W + c];
        double *u = out + (size_t) c * 4;
        if (metric != 0) { u[0] = x0; u[1] = x1; u[2] = x2; u[3] = x3; continue; }
        const double mean = (((x0 + x1) + x2) + x3) * 0.25;
        const double c0 = x0 - mean, c1 = x1 - mean, c2 = x2 - mean, c3 = x3 - mean;
        const double n = std::sqrt(((c0 * c0 + c1 * c1) + c2 * c2) + c3 * c3);
        const bool ok = n > 0.0;
        u[0] = ok ? c0 / n : 0.0; u[1] = ok ? c1 / n : 0.0; u[2] = ok ? c2 / n : 0.0; u[3] = ok ? c3 / n : 0.0;
    }
}

// the score grid of a metric: the integer score of a column pair is floor((g - lo) * scale), clamped to [0, bins - 1]
inline void cmp_grid(int metric, int32_t bins, double *lo, double *scale) {
    if (metric == 2) { *lo = -std::sqrt(2.0); *scale = (double) bins / std::sqrt(2.0); return; }
    *lo = metric == 0 ? -1.0 : 0.0;
    *scale = (double) bins * 0.5;
}

// entries of the table of an overlap of L columns: the scores 0 .. L (bins - 1)
MS_CMP_HD inline int64_t cmp_table_len(int32_t L, int32_t bins) { return (int64_t) L * (bins - 1) + 1; }
// entries of the tables of the lengths 1 .. n of one start: where the table of length n + 1 begins behind the start's first table
MS_CMP_HD inline int64_t cmp_tables_upto(int32_t n, int32_t bins) { return (int64_t) (bins - 1) * n * (n + 1) / 2 + n; }
// where the tables of start a begin in a query of width W: behind those of the starts before it (a = W: the query's whole size)
inline int64_t cmp_start_offset(int32_t W, int32_t bins, int32_t a) {
    int64_t at = 0;
    for (int32_t b = 0; b < a; b++) at += cmp_tables_upto(W - b, bins);
    return at;
}
// doubles of all tables of a query of width W (at the caps, 64 columns and 256 bins: 11 670 880, 89 MiB)
inline int64_t cmp_query_doubles(int32_t W, int32_t bins) { return cmp_start_offset(W, bins, W); }

struct CmpPlan {
    std::vector<double> qv;              // [columns][4] the prepared vectors of the queries [q0, q1)
    std::vector<int32_t> q_first;        // [n + 1] first column of query q0 + k
    std::vector<int64_t> q_tab;          // [n] where the query's tables begin in its batch's table block (doubles)
    std::vector<int64_t> col_off;        // [columns] where the tables of start a of the query begin behind q_tab
    std::vector<int32_t> batch_first;    // [batches + 1] into the n queries
    int64_t max_doubles = 0;             // the table block of the largest batch
    int32_t max_cols = 0, max_queries = 0, max_width = 0;   // of the largest batch each
    int32_t bad = -1;                    // kCmpNoRoom: the query (index into all queries) ...
    int64_t bad_bytes = 0;               // ... and the bytes of its tables
};

// values / widths: the matrices concatenated ([4][W] row-major each), all n_q of them; the plan covers the queries [q0, q1).  A batch
// takes queries while their tables fit `budget` bytes, at most `cap` of them.  kCmpNoRoom: the tables of one query do not fit alone.
inline CmpStatus cmp_plan(const double *values, const int32_t *widths, int32_t q0, int32_t q1, int metric, int32_t bins, int64_t budget, int32_t cap,
                          CmpPlan *pl) {
    *pl = CmpPlan();
    pl->q_first.push_back(0);
    pl->batch_first.push_back(0);
    size_t at = 0;
    for (int32_t q = 0; q < q0; q++) at += 4 * (size_t) widths[q];
    int64_t used = 0;
    int32_t cols = 0, wmax = 0;
    auto close = [&](int32_t k) {
        const int32_t n = k - pl->batch_first.back();
        if (used > pl->max_doubles) pl->max_doubles = used;
        if (cols > pl->max_cols) pl->max_cols = cols;
        if (n > pl->max_queries) pl->max_queries = n;
        if (wmax > pl->max_width) pl->max_width = wmax;
        pl->batch_first.push_back(k);
        used = 0; cols = 0; wmax = 0;
    };
    for (int32_t q = q0; q < q1; q++) {
        const int32_t W = widths[q], k = q - q0;
        const int64_t need = cmp_query_doubles(W, bins);
        if (need * 8 > budget) { pl->bad = q; pl->bad_bytes = need * 8; return kCmpNoRoom; }
        if (k > pl->batch_first.back() && ((used + need) * 8 > budget || k - pl->batch_first.back() >= cap)) close(k);
        pl->q_tab.push_back(used);
        used += need;
        cols += W;
        if (W > wmax) wmax = W;
        const size_t c0 = pl->qv.size();
        pl->qv.resize(c0 + 4 * (size_t) W);
        cmp_prepare(values + at, W, metric, pl->qv.data() + c0);
        at += 4 * (size_t) W;
        for (int32_t a = 0; a < W; a++) pl->col_off.push_back(cmp_start_offset(W, bins, a));
        pl->q_first.push_back(pl->q_first.back() + W);
    }
    if (q1 > q0) close(q1 - q0);
    return kCmpOk;
}

}  // namespace ms
