// tests/sanitize/scoredist_plan_asan.cpp -- the host's plan of the analytic score distribution (motifscan_amd/csrc/ms_scoredist_plan.h: the
// score grid, the shifts, the fit assertion, the batches) under AddressSanitizer + UndefinedBehaviorSanitizer, compiled by plain g++ from
// the header the library is built from, against a brute-force restatement: the grid recomputed entry by entry, every W-mer of a narrow
// motif walked through the shifts, the batches counted one motif at a time.  Every array is allocated at exactly the size the plan
// promises.  CPU build container only (`make -C motifscan_amd/csrc scoredist_plan_asan`).
#include "ms_scoredist_plan.h"

#include <cstdio>
#include <cstdlib>
#include <random>

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } } while (0)

static int n_checks = 0;
static const double kInf = std::numeric_limits<double>::infinity();

struct Set {
    std::vector<double> values;
    std::vector<int64_t> val_off{0};
    std::vector<int32_t> widths;
    void add(const std::vector<double> &m, int32_t W) {
        values.insert(values.end(), m.begin(), m.end());
        val_off.push_back((int64_t) values.size());
        widths.push_back(W);
    }
};

static std::vector<double> random_matrix(int32_t W, std::mt19937_64 &rng, int kind) {
    std::uniform_real_distribution<double> u(-6.0, 2.0);
    std::vector<double> m((size_t) 4 * W);
    for (double &v : m) v = kind == 3 ? std::floor(u(rng)) : u(rng);
    if (kind == 1) { m[(size_t) (rng() % 4) * W + rng() % W] = -kInf; m[(size_t) (rng() % 4) * W] = -kInf; }
    if (kind == 2) for (int b = 0; b < 4; b++) m[(size_t) b * W + W / 2] = 1.25;       // a column of four equal entries: shift 0
    if (kind == 4) for (double &v : m) v = 0.5;                                        // hi == lo: step 1
    return m;
}

// the grid of one motif, entry by entry, and the plan's row against it
static void check_motif(const double *M, int32_t W, int32_t n_bins, int strand, double step, int64_t s0, const int32_t *d) {
    double hi = 0.0, lo = 0.0;
    for (int32_t c = 0; c < W; c++) {
        double mx = -kInf, mn = kInf;
        for (int b = 0; b < 4; b++) {
            const double v = M[(size_t) b * W + c];
            if (v == -kInf) continue;
            mx = v > mx ? v : mx;
            mn = v < mn ? v : mn;
        }
        hi = hi + mx;
        lo = lo + mn;
    }
    const double want = hi == lo ? 1.0 : (hi - lo) / (double) (n_bins - W - 2);
    CHECK(step == want && step > 0.0);
    int64_t sum_min = 0, sum_max = 0;
    for (int32_t c = 0; c < W; c++) {
        int64_t qmin = INT64_MAX, q[4];
        for (int b = 0; b < 4; b++) {
            const double v = M[(size_t) b * W + c];
            q[b] = v == -kInf ? INT64_MAX : (int64_t) std::floor(v / step);
            qmin = q[b] < qmin ? q[b] : qmin;
        }
        sum_min += qmin;
        int32_t dmax = 0;
        for (int b = 0; b < 4; b++) {
            const int32_t got = strand == 2 ? d[(size_t) (W - 1 - c) * 4 + (size_t) (3 - b)] : d[(size_t) c * 4 + (size_t) b];
            if (M[(size_t) b * W + c] == -kInf) { CHECK(got == ms::kSdAbsent); continue; }
            CHECK(got >= 0 && (int64_t) got == q[b] - qmin);
            dmax = got > dmax ? got : dmax;
        }
        sum_max += dmax;
    }
    CHECK(s0 == sum_min);
    CHECK(sum_max < n_bins);                                                           // the fit
    if (W <= 6) {                                                                      // every W-mer lands on the grid, the best one on sum_max
        int64_t best = -1;
        for (int64_t w = 0; w < ((int64_t) 1 << (2 * W)); w++) {
            int64_t s = 0;
            bool live = true;
            for (int32_t c = 0; c < W; c++) {
                const int32_t v = d[(size_t) c * 4 + (size_t) ((w >> (2 * (W - 1 - c))) & 3)];
                if (v < 0) { live = false; break; }
                s += v;
            }
            if (!live) continue;
            CHECK(s >= 0 && s < n_bins);
            best = s > best ? s : best;
        }
        CHECK(best <= sum_max);
    }
    n_checks++;
}

static void check_set(const Set &S, int strand, int32_t order, int32_t n_bins, int64_t budget, int32_t cap, const std::vector<bool> &scorable) {
    const int32_t P = (int32_t) S.widths.size();
    ms::SdPlan pl;
    const ms::SdStatus st = ms::sd_plan(S.values.data(), S.val_off.data(), S.widths.data(), P, strand, order, n_bins, budget, cap, &pl);
    const int64_t bytes = 2 * ((int64_t) 1 << (2 * order)) * (int64_t) n_bins * 8;
    CHECK(pl.motif_bytes == bytes);
    int32_t per = 0;                                                                   // motifs of a batch, counted one at a time
    while (per < cap && (int64_t) (per + 1) * bytes <= budget) per++;
    CHECK(ms::sd_batch_motifs(bytes, budget, cap) == per);
    if (P > 0 && per == 0) { CHECK(st == ms::kSdNoRoom); n_checks++; return; }
    CHECK(st == ms::kSdOk);
    CHECK((int32_t) pl.step.size() == P && (int32_t) pl.s0.size() == P);
    size_t k = 0;
    for (int32_t m = 0; m < P; m++) {
        if (!scorable[(size_t) m]) { CHECK(pl.step[(size_t) m] == 0.0 && pl.s0[(size_t) m] == 0); CHECK(k >= pl.mot.size() || pl.mot[k] != m); continue; }
        CHECK(k < pl.mot.size() && pl.mot[k] == m && pl.width[k] == S.widths[(size_t) m]);
        CHECK(pl.col_first[k + 1] - pl.col_first[k] == S.widths[(size_t) m]);
        // the motif's shifts in a block of exactly their size: a read past it stops the run
        std::vector<int32_t> d(pl.shift.begin() + (size_t) pl.col_first[k] * 4, pl.shift.begin() + (size_t) pl.col_first[k + 1] * 4);
        check_motif(S.values.data() + S.val_off[(size_t) m], S.widths[(size_t) m], n_bins, strand, pl.step[(size_t) m], pl.s0[(size_t) m], d.data());
        CHECK(pl.max_w >= S.widths[(size_t) m]);
        k++;
    }
    CHECK(k == pl.mot.size() && pl.col_first.size() == k + 1 && pl.shift.size() == (size_t) pl.col_first[k] * 4);
    // the batches: in order, none empty, none over the budget or the cap, all but the last full, together every computed motif once
    CHECK(pl.batch_first.front() == 0 && pl.batch_first.back() == (int32_t) k);
    CHECK(pl.batch_first.size() == (k == 0 ? 1 : (k + (size_t) per - 1) / (size_t) per + 1));
    for (size_t b = 0; b + 1 < pl.batch_first.size(); b++) {
        const int32_t nb = pl.batch_first[b + 1] - pl.batch_first[b];
        CHECK(nb >= 1 && nb <= per && (int64_t) nb * bytes <= budget);
        if (b + 2 < pl.batch_first.size()) CHECK(nb == per);
    }
    n_checks++;
}

int main() {
    std::mt19937_64 rng(23);
    const int32_t widths[] = {1, 2, 5, 6, 9, 31};
    Set S;
    std::vector<bool> scorable;
    for (int kind = 0; kind < 5; kind++)
        for (int32_t W : widths) {
            S.add(random_matrix(W, rng, kind), W);
            bool ok = true;                                                            // max_raw > 0, and a finite entry in every column
            const double *M = S.values.data() + S.val_off[S.widths.size() - 1];
            double mr = 0.0;
            for (int32_t c = 0; c < W; c++) {
                double col = 0.0;
                int fin = 0;
                for (int b = 0; b < 4; b++) { const double v = M[(size_t) b * W + c]; col = v > col ? v : col; fin += v != -kInf; }
                mr += col;
                ok = ok && fin > 0;
            }
            scorable.push_back(ok && mr > 0.0);
        }
    {   // the unscorable kinds: NaN, +inf, a column of -inf, max_raw = 0 -- between scorable motifs
        std::vector<double> m = random_matrix(4, rng, 0);
        m[5] = std::nan("");
        S.add(m, 4); scorable.push_back(false);
        m = random_matrix(4, rng, 0); m[2] = kInf;
        S.add(m, 4); scorable.push_back(false);
        m = random_matrix(4, rng, 0); for (int b = 0; b < 4; b++) m[(size_t) b * 4 + 1] = -kInf;
        S.add(m, 4); scorable.push_back(false);
        m = random_matrix(4, rng, 0); for (double &v : m) v = -std::fabs(v);
        S.add(m, 4); scorable.push_back(false);
        m = random_matrix(3, rng, 0); m[0] = 3.0;
        S.add(m, 3); scorable.push_back(true);
    }
    const int32_t bins[] = {34, 35, 64, 1000, 1 << 20};
    for (int strand = 1; strand <= 2; strand++)
        for (int32_t n_bins : bins)
            for (int32_t order : {0, 2, 5}) {
                const int64_t bytes = ms::sd_motif_bytes(order, n_bins);
                for (int64_t budget : {bytes - 1, bytes, 3 * bytes + 5, 1000 * bytes})
                    for (int32_t cap : {2, 32768}) check_set(S, strand, order, n_bins, budget, cap, scorable);
            }
    Set none;
    check_set(none, 1, 0, 16, 1, 4, {});                                               // P = 0: valid whatever the budget

    {   // entries far too large against their range: the fit assertion refuses, it does not convert out of range
        std::vector<double> m = {1e300, 1e300 + 1e285, 1e300, 1e300};
        double step;
        int64_t s0;
        int32_t d[4];
        CHECK(ms::sd_quantise(m.data(), 1, 8, 1, &step, &s0, d) == ms::kSdNoFit);
        m = {1e308, -1e308, 0.0, 0.0};                                                  // hi - lo overflows
        CHECK(ms::sd_quantise(m.data(), 1, 8, 1, &step, &s0, d) == ms::kSdNoFit);
        n_checks += 2;
    }
    std::printf("scoredist_plan_asan: ok (%d checks)\n", n_checks);
    return 0;
}
