// tests/sanitize/dimodel_plan_asan.cpp -- the host's half of the first-order best-site walk (motifscan_amd/csrc/ms_dimodel_plan.h: the
// argument checks, the table the device reads, the Viterbi maximum, the scorable test) under AddressSanitizer +
// UndefinedBehaviorSanitizer, compiled by plain g++ from the header the library is built from.  The table is built into an array of
// exactly the promised size and then WALKED as the kernel walks it -- end entry by the first base, one entry per genome step by the four
// bits of the pair, end entry by the last base -- and both sums are compared, bit for bit, with a restatement that follows the
// definition's own indices (trans[j][4 a + b], the window read on the other strand); the Viterbi maximum is compared with the maximum
// over all 4^W sequences.  CPU build container only (`make -C motifscan_amd/csrc dimodel_plan_asan`).
#include "ms_dimodel_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } } while (0)

static int n_cases = 0;
static const double kInf = std::numeric_limits<double>::infinity();

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

// ---- the restatement: the definition's indices, one addition at a time
static double def_forward(const std::vector<double> &v, int W, const int *x) {
    double s = 0.0;
    s += v[(size_t) x[0]];
    for (int j = 1; j < W; j++) s += v[(size_t) j * 16 + 4 * x[j - 1] + x[j]];
    return s;
}
static double def_reverse(const std::vector<double> &v, int W, const int *x) {
    std::vector<int> y((size_t) W);
    for (int j = 0; j < W; j++) y[(size_t) j] = 3 - x[W - 1 - j];
    double s = 0.0;
    for (int j = W - 1; j >= 1; j--) s += v[(size_t) j * 16 + 4 * y[(size_t) j - 1] + y[(size_t) j]];
    s += v[(size_t) y[0]];
    return s;
}

// ---- the kernel's walk over the table (an exact-size copy: a step past it stops the run)
static void walk_table(const ms::DiEntry *tab, int W, const int *x, double *fwd, double *rev) {
    double f = 0.0, r = 0.0;
    f += tab[x[0]].fwd;
    for (int c = 1; c < W; c++) {
        const int q = x[c - 1] | (x[c] << 2);
        const ms::DiEntry e = tab[4 + 16 * (c - 1) + q];
        f += e.fwd;
        r += e.rev;
    }
    r += tab[x[W - 1]].rev;
    *fwd = f;
    *rev = r;
}

static std::vector<double> random_values(std::mt19937_64 &rng, int W, int holes, bool junk_row0) {
    std::uniform_real_distribution<double> u(-3.0, 2.0);
    std::vector<double> v((size_t) W * 16);
    for (double &d : v) d = std::round(u(rng) * 1e5) / 1e5;
    if (junk_row0)
        for (int i = 4; i < 16; i++) v[(size_t) i] = std::numeric_limits<double>::quiet_NaN();      // never read
    for (int h = 0; h < holes; h++) {
        const size_t i = (size_t) (rng() % (uint64_t) (W * 16));
        if (i >= 4 && i < 16) continue;
        v[i] = -kInf;
    }
    return v;
}

static void one_model(std::mt19937_64 &rng, int W, int holes) {
    const std::vector<double> v = random_values(rng, W, holes, (rng() & 1) != 0);
    CHECK(ms::di_entries(W) == 4 + 16 * (int64_t) (W - 1) && ms::di_pseudo_width(W) * 4 == ms::di_entries(W));
    std::vector<ms::DiEntry> tab((size_t) ms::di_entries(W));
    ms::di_build_table(v.data(), W, tab.data());
    std::vector<int> x((size_t) W);
    double brute = -kInf;
    const bool all = W <= 6;
    const uint64_t n_seq = all ? (uint64_t) 1 << (2 * W) : 200;
    for (uint64_t s = 0; s < n_seq; s++) {
        for (int j = 0; j < W; j++) x[(size_t) j] = (int) ((all ? s >> (2 * j) : rng()) & 3u);       // every sequence, or 200 drawn ones
        double f, r;
        walk_table(tab.data(), W, x.data(), &f, &r);
        const double df = def_forward(v, W, x.data()), dr = def_reverse(v, W, x.data());
        CHECK(same_bits(f, df) && same_bits(r, dr));
        if (df > brute) brute = df;
        // the reverse sum is the forward sum's terms of the other strand, in the opposite order: equal as a set of terms, so the two
        // agree exactly wherever no rounding happens -- a window of one or two columns
        if (W <= 2) {
            std::vector<int> y((size_t) W);
            for (int j = 0; j < W; j++) y[(size_t) j] = 3 - x[(size_t) (W - 1 - j)];
            CHECK(same_bits(dr, def_forward(v, W, y.data())));
        }
    }
    const double mr = ms::di_max_raw(v.data(), W);
    if (all) CHECK(same_bits(mr, brute));
    else CHECK(mr >= brute);
    bool bad = !(std::isfinite(mr) && mr > 0.0);
    for (size_t i = 0; i < v.size(); i++)
        if (!(i >= 4 && i < 16) && (std::isnan(v[i]) || v[i] == kInf)) bad = true;
    CHECK(ms::di_scorable(v.data(), W, mr) == !bad);
    n_cases++;
}

static void scorable_cases() {
    std::mt19937_64 rng(5);
    for (int W = 1; W <= 5; W++) {
        std::vector<double> v = random_values(rng, W, 0, false);
        for (double &d : v) d = std::fabs(d) + 0.25;
        const double mr = ms::di_max_raw(v.data(), W);
        CHECK(ms::di_scorable(v.data(), W, mr));
        for (size_t i = 0; i < v.size(); i++) {
            const bool read = !(i >= 4 && i < 16);
            for (double badv : {std::numeric_limits<double>::quiet_NaN(), kInf}) {
                std::vector<double> w = v;
                w[i] = badv;
                CHECK(ms::di_scorable(w.data(), W, ms::di_max_raw(w.data(), W)) == !read);
            }
            std::vector<double> w = v;
            w[i] = -kInf;                                 // a forbidden transition is allowed (other paths remain)
            CHECK(ms::di_scorable(w.data(), W, ms::di_max_raw(w.data(), W)));
        }
        std::vector<double> neg = v;
        for (double &d : neg) d = -d;
        CHECK(!ms::di_scorable(neg.data(), W, ms::di_max_raw(neg.data(), W)));
        std::vector<double> none = v;
        for (int b = 0; b < 4; b++) none[(size_t) b] = -kInf;
        CHECK(ms::di_max_raw(none.data(), W) == -kInf && !ms::di_scorable(none.data(), W, -kInf));
        n_cases++;
    }
}

static void validation_cases() {
    int32_t bad = 7;
    const double vals[16] = {};
    int32_t w1[3] = {1, ms::kDiMaxWidth, 64};
    CHECK(ms::di_validate(nullptr, nullptr, 0, &bad) == ms::kDiOk && bad == -1);
    CHECK(ms::di_validate(nullptr, nullptr, -1, &bad) == ms::kDiCount);
    CHECK(ms::di_validate(nullptr, w1, 3, &bad) == ms::kDiNull);
    CHECK(ms::di_validate(vals, nullptr, 3, &bad) == ms::kDiNull);
    CHECK(ms::di_validate(vals, w1, 3, &bad) == ms::kDiOk && bad == -1);          // (the widths alone are read)
    int32_t w2[3] = {4, 0, ms::kDiMaxWidth + 1};
    CHECK(ms::di_validate(vals, w2, 3, &bad) == ms::kDiWidth && bad == 1);
    w2[1] = -5;
    CHECK(ms::di_validate(vals, w2, 3, &bad) == ms::kDiWidth && bad == 1);
    w2[1] = 9;
    CHECK(ms::di_validate(vals, w2, 3, &bad) == ms::kDiTooWide && bad == 2);
    CHECK(ms::di_validate(vals, w2, 2, &bad) == ms::kDiOk);
    CHECK(ms::kDiMaxWidth >= 64 && ms::di_entries(ms::kDiMaxWidth) <= ms::kDiTileEntries && ms::di_entries(ms::kDiMaxWidth + 1) > ms::kDiTileEntries);
    n_cases++;
}

int main() {
    std::mt19937_64 rng(20260102);
    for (int W = 1; W <= 6; W++)
        for (int rep = 0; rep < 12; rep++) one_model(rng, W, rep % 4);
    for (int W : {7, 31, 32, 33, 34, 63, 64, 65, 128, ms::kDiMaxWidth})
        for (int rep = 0; rep < 4; rep++) one_model(rng, W, rep);
    scorable_cases();
    validation_cases();
    std::printf("dimodel_plan_asan: ok (%d cases)\n", n_cases);
    return 0;
}
