// tests/sanitize/compare_plan_asan.cpp -- the host's half of the motif comparison (motifscan_amd/csrc/ms_compare_plan.h: the prepared
// columns, the score grid, the offsets of every (a, L) table of a query, the batches) under AddressSanitizer +
// UndefinedBehaviorSanitizer, compiled by plain g++ from the header the library is built from, against a brute-force restatement: the
// columns prepared entry by entry, the tables laid one behind the other and their places counted, the batches filled one query at a
// time.  Every array is allocated at exactly the size the plan promises.  CPU build container only
// (`make -C motifscan_amd/csrc compare_plan_asan`).
#include "ms_compare_plan.h"

#include <cstdio>
#include <cstdlib>
#include <random>

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } } while (0)

static int n_checks = 0;

static std::vector<double> random_matrix(int32_t W, std::mt19937_64 &rng, int kind) {
    std::uniform_real_distribution<double> u(0.0, 1.0);
    std::vector<double> m((size_t) 4 * W);
    for (int32_t c = 0; c < W; c++) {
        double x[4], sum = 0.0;
        for (int b = 0; b < 4; b++) { x[b] = kind == 1 && c == W / 2 ? 0.25 : u(rng); sum += x[b]; }      // kind 1: a flat column, norm 0
        if (kind == 2) { for (int b = 0; b < 4; b++) x[b] = 0.0; x[rng() % 4] = 1.0; sum = 1.0; }          // kind 2: one-hot columns
        for (int b = 0; b < 4; b++) m[(size_t) b * W + c] = x[b] / sum;
    }
    return m;
}

// the prepared columns of one matrix, entry by entry
static void check_prepare(const std::vector<double> &m, int32_t W, int metric) {
    std::vector<double> out((size_t) 4 * W);                        // exactly its size: a store past it stops the run
    ms::cmp_prepare(m.data(), W, metric, out.data());
    for (int32_t c = 0; c < W; c++) {
        double x[4];
        for (int b = 0; b < 4; b++) x[b] = m[(size_t) b * W + c];
        if (metric != 0) { for (int b = 0; b < 4; b++) CHECK(out[(size_t) c * 4 + b] == x[b]); continue; }
        double s = x[0];
        for (int b = 1; b < 4; b++) s = s + x[b];
        const double mean = s * 0.25;
        double q = 0.0, cc[4];
        for (int b = 0; b < 4; b++) { cc[b] = x[b] - mean; q = b == 0 ? cc[0] * cc[0] : q + cc[b] * cc[b]; }
        const double n = std::sqrt(q);
        double norm2 = 0.0;
        for (int b = 0; b < 4; b++) {
            const double want = n > 0.0 ? cc[b] / n : 0.0;
            CHECK(out[(size_t) c * 4 + b] == want);
            if (!(n > 0.0)) CHECK(!std::signbit(out[(size_t) c * 4 + b]));
            norm2 += want * want;
        }
        CHECK(n > 0.0 ? std::fabs(norm2 - 1.0) < 1e-12 : norm2 == 0.0);
    }
    n_checks++;
}

// the places of a query's tables: laid one behind the other in (a ascending, L ascending) order
static void check_layout(int32_t W, int32_t bins) {
    int64_t at = 0;
    for (int32_t a = 0; a < W; a++) {
        CHECK(ms::cmp_start_offset(W, bins, a) == at);
        for (int32_t L = 1; L <= W - a; L++) {
            CHECK(ms::cmp_start_offset(W, bins, a) + ms::cmp_tables_upto(L - 1, bins) == at);
            CHECK(ms::cmp_table_len(L, bins) == (int64_t) L * (bins - 1) + 1);
            at += ms::cmp_table_len(L, bins);
        }
    }
    CHECK(ms::cmp_query_doubles(W, bins) == at && ms::cmp_start_offset(W, bins, W) == at);
    n_checks++;
}

struct Set {
    std::vector<double> values;
    std::vector<int32_t> widths;
    void add(const std::vector<double> &m, int32_t W) { values.insert(values.end(), m.begin(), m.end()); widths.push_back(W); }
};

static void check_plan(const Set &S, int32_t q0, int32_t q1, int metric, int32_t bins, int64_t budget, int32_t cap) {
    ms::CmpPlan pl;
    const ms::CmpStatus st = ms::cmp_plan(S.values.data(), S.widths.data(), q0, q1, metric, bins, budget, cap, &pl);
    for (int32_t q = q0; q < q1; q++)
        if (ms::cmp_query_doubles(S.widths[(size_t) q], bins) * 8 > budget) {          // the first query that does not fit alone
            CHECK(st == ms::kCmpNoRoom && pl.bad == q && pl.bad_bytes == ms::cmp_query_doubles(S.widths[(size_t) q], bins) * 8);
            n_checks++;
            return;
        }
    CHECK(st == ms::kCmpOk);
    const int32_t n = q1 - q0;
    CHECK((int32_t) pl.q_first.size() == n + 1 && (int32_t) pl.q_tab.size() == n && pl.q_first[0] == 0);
    size_t at = 0;
    for (int32_t q = 0; q < q0; q++) at += 4 * (size_t) S.widths[(size_t) q];
    for (int32_t k = 0; k < n; k++) {
        const int32_t W = S.widths[(size_t) (q0 + k)];
        CHECK(pl.q_first[(size_t) k + 1] - pl.q_first[(size_t) k] == W);
        std::vector<double> want((size_t) 4 * W);
        ms::cmp_prepare(S.values.data() + at, W, metric, want.data());
        for (size_t i = 0; i < want.size(); i++) CHECK(pl.qv[(size_t) pl.q_first[(size_t) k] * 4 + i] == want[i]);
        for (int32_t a = 0; a < W; a++) CHECK(pl.col_off[(size_t) pl.q_first[(size_t) k] + (size_t) a] == ms::cmp_start_offset(W, bins, a));
        at += 4 * (size_t) W;
    }
    CHECK(pl.qv.size() == 4 * (size_t) pl.q_first[(size_t) n] && pl.col_off.size() == (size_t) pl.q_first[(size_t) n]);
    // the batches, filled one query at a time: a query opens a new batch when it does not fit the rest of the budget or the cap is met
    std::vector<int32_t> first{0};
    std::vector<int64_t> tab;
    int64_t used = 0, max_doubles = 0;
    int32_t max_cols = 0, max_queries = 0, max_width = 0, cols = 0, cnt = 0;
    for (int32_t k = 0; k < n; k++) {
        const int32_t W = S.widths[(size_t) (q0 + k)];
        const int64_t need = ms::cmp_query_doubles(W, bins);
        if (cnt > 0 && ((used + need) * 8 > budget || cnt >= cap)) { first.push_back(k); used = 0; cols = 0; cnt = 0; }
        tab.push_back(used);
        used += need; cols += W; cnt++;
        max_doubles = used > max_doubles ? used : max_doubles;
        max_cols = cols > max_cols ? cols : max_cols;
        max_queries = cnt > max_queries ? cnt : max_queries;
        max_width = W > max_width ? W : max_width;
    }
    if (n > 0) first.push_back(n);
    CHECK(pl.batch_first == first && pl.q_tab == tab);
    CHECK(pl.max_doubles == max_doubles && pl.max_cols == max_cols && pl.max_queries == max_queries && pl.max_width == max_width);
    for (size_t b = 0; b + 1 < pl.batch_first.size(); b++) {                            // every batch: not empty, within budget and cap
        const int32_t k0 = pl.batch_first[b], k1 = pl.batch_first[b + 1];
        CHECK(k1 > k0 && k1 - k0 <= cap);
        int64_t sum = 0;
        for (int32_t k = k0; k < k1; k++) { CHECK(pl.q_tab[(size_t) k] == sum); sum += ms::cmp_query_doubles(S.widths[(size_t) (q0 + k)], bins); }
        CHECK(sum * 8 <= budget && sum <= pl.max_doubles);
    }
    n_checks++;
}

int main() {
    std::mt19937_64 rng(29);
    const int32_t widths[] = {1, 2, 5, 9, 31, 63, 64};
    Set S;
    for (int kind = 0; kind < 3; kind++)
        for (int32_t W : widths) {
            const std::vector<double> m = random_matrix(W, rng, kind);
            for (int metric = 0; metric < 3; metric++) check_prepare(m, W, metric);
            S.add(m, W);
        }
    {   // a flat column under pearson: +0.0 four times, not a NaN
        const std::vector<double> flat(4, 0.25);
        double out[4];
        ms::cmp_prepare(flat.data(), 1, 0, out);
        for (double v : out) CHECK(v == 0.0 && !std::signbit(v));
        n_checks++;
    }
    for (int32_t bins : {2, 3, 7, 100, 256})
        for (int32_t W : {1, 2, 3, 17, 64}) check_layout(W, bins);
    CHECK(ms::cmp_query_doubles(ms::kCmpMaxWidth, ms::kCmpMaxBins) == 11670880);          // the caps: 89 MiB, inside the default budget
    for (int metric = 0; metric < 3; metric++) {
        double lo, scale;
        ms::cmp_grid(metric, 100, &lo, &scale);
        CHECK(metric == 0 ? (lo == -1.0 && scale == 50.0) : metric == 1 ? (lo == 0.0 && scale == 50.0) : (lo == -std::sqrt(2.0) && scale == 100.0 / std::sqrt(2.0)));
        n_checks++;
    }
    const int32_t n = (int32_t) S.widths.size();
    for (int32_t bins : {2, 8, 100}) {
        const int64_t widest = ms::cmp_query_doubles(64, bins) * 8;
        for (int64_t budget : {widest - 8, widest, 2 * widest + 8, 1000 * widest, (int64_t) 256 << 20})
            for (int32_t cap : {1, 3, 4096})
                for (int metric : {0, 2}) {
                    check_plan(S, 0, n, metric, bins, budget, cap);
                    check_plan(S, 3, n - 2, metric, bins, budget, cap);
                    check_plan(S, 5, 6, metric, bins, budget, cap);
                    check_plan(S, 4, 4, metric, bins, budget, cap);                     // an empty range: valid whatever the budget
                }
    }
    std::printf("compare_plan_asan: ok (%d checks)\n", n_checks);
    return 0;
}
