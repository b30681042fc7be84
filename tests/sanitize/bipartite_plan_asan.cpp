// tests/sanitize/bipartite_plan_asan.cpp -- the host's half of the bipartite best-site walk (motifscan_amd/csrc/ms_bipartite_plan.h: the
// checks of the spec arrays, the scorable rule, the table layout, the pseudo-widths, the reduction key) under AddressSanitizer +
// UndefinedBehaviorSanitizer, compiled by plain g++ from the header the library is built from.  A spec's table is built into an array of
// exactly the promised size and then WALKED as the kernel walks it -- entry 4 c + x per column of either element -- and the element sums
// are compared, bit for bit, with a restatement that follows the definition's own indices (M[x][c], M[3 - x][W - 1 - c]); the checks are
// compared with a brute-force restatement over random and hand-made spec arrays; the key is compared with a sort of the walk's order.
// CPU build container only (`make -C motifscan_amd/csrc bipartite_plan_asan`).
#include "ms_bipartite_plan.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } } while (0)

static int n_cases = 0;
static const double kInf = std::numeric_limits<double>::infinity();
static const double kNaN = std::numeric_limits<double>::quiet_NaN();

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

static std::vector<double> random_matrix(std::mt19937_64 &rng, int W) {
    std::uniform_real_distribution<double> u(-3.0, 2.0);
    std::vector<double> m((size_t) 4 * W);
    for (double &d : m) d = std::round(u(rng) * 1e5) / 1e5;
    return m;
}

// ---- the restatement of the element sums: the definition's indices, one addition at a time (x < 0: a base that adds nothing)
static void def_sums(const std::vector<double> &m, int W, const int *x, double *fwd, double *rev) {
    double f = 0.0, r = 0.0;
    for (int c = 0; c < W; c++) {
        if (x[c] < 0) continue;
        f += m[(size_t) x[c] * W + c];
        r += m[(size_t) (3 - x[c]) * W + (W - 1 - c)];
    }
    *fwd = f;
    *rev = r;
}

// ---- the kernel's walk over a table of exactly 4 W entries
static void walk_table(const ms::BpEntry *tab, int W, const int *x, double *fwd, double *rev) {
    double f = 0.0, r = 0.0;
    for (int c = 0; c < W; c++) {
        if (x[c] < 0) continue;                          // (the kernel adds its all-zero entry 0)
        f += tab[4 * c + x[c]].fwd;
        r += tab[4 * c + x[c]].rev;
    }
    *fwd = f;
    *rev = r;
}

static double def_max_raw(const std::vector<double> &m, int W) {
    double total = 0;
    for (int c = 0; c < W; c++) {
        double best = 0;
        for (int b = 0; b < 4; b++) best = std::max(best, m[(size_t) b * W + c]);
        total += best;
    }
    return total;
}

static void one_table(std::mt19937_64 &rng, int Wa, int Wb) {
    const std::vector<double> ma = random_matrix(rng, Wa), mb = random_matrix(rng, Wb);
    CHECK(ms::bp_pseudo_width(Wa, Wb) == Wa + Wb && ms::bp_entries(Wa, Wb) == 4 * (int64_t) (Wa + Wb));
    std::vector<ms::BpEntry> tab((size_t) ms::bp_entries(Wa, Wb));        // exactly: a write past it stops the run
    ms::bp_spec_table(ma.data(), Wa, mb.data(), Wb, tab.data());
    std::vector<int> x((size_t) std::max(Wa, Wb));
    for (int rep = 0; rep < 8; rep++) {
        for (int &b : x) b = (rng() % 9 == 0) ? -1 : (int) (rng() & 3);
        double f0, r0, f1, r1;
        def_sums(ma, Wa, x.data(), &f0, &r0);
        walk_table(tab.data(), Wa, x.data(), &f1, &r1);
        CHECK(same_bits(f0, f1) && same_bits(r0, r1));
        def_sums(mb, Wb, x.data(), &f0, &r0);
        walk_table(tab.data() + 4 * (size_t) Wa, Wb, x.data(), &f1, &r1);
        CHECK(same_bits(f0, f1) && same_bits(r0, r1));
    }
    n_cases++;
}

// ---- the scorable rule against its restatement
static bool def_scorable(const std::vector<double> &ma, int Wa, const std::vector<double> &mb, int Wb) {
    for (const std::vector<double> *m : {&ma, &mb})
        for (double v : *m)
            if (v != v || v == kInf) return false;
    const double d = def_max_raw(ma, Wa) + def_max_raw(mb, Wb);
    return d == d && d != kInf && d != -kInf && d > 0.0;
}

static void one_scorable(std::mt19937_64 &rng, int Wa, int Wb, int kind) {
    std::vector<double> ma = random_matrix(rng, Wa), mb = random_matrix(rng, Wb);
    bool want = true;
    switch (kind) {
    case 1: ma[rng() % ma.size()] = kNaN; want = false; break;
    case 2: mb[rng() % mb.size()] = kInf; want = false; break;
    case 3: mb[rng() % mb.size()] = -kInf; break;                                              // ordinary (the other entries keep max_raw > 0 with near certainty; checked below)
    case 4: for (double &v : ma) v = -std::fabs(v) - 0.5; for (double &v : mb) v = -std::fabs(v) - 0.5; want = false; break;       // the sum is 0
    case 5: for (double &v : mb) v = 0.0; break;                                               // an all-zero partner is legal
    case 6: for (double &v : ma) v = 0.0; for (double &v : mb) v = 0.0; want = false; break;
    default: break;
    }
    const double ra = def_max_raw(ma, Wa), rb = def_max_raw(mb, Wb);
    CHECK(same_bits(ms::bp_denominator(ra, rb), ra + rb));
    const bool got = ms::bp_scorable(ma.data(), Wa, ra, mb.data(), Wb, rb);
    CHECK(got == def_scorable(ma, Wa, mb, Wb));
    if (kind != 0 && kind != 3 && kind != 5) CHECK(got == want);
    CHECK(ms::bp_entries_ok(ma.data(), Wa) == (kind != 1));
    n_cases++;
}

// ---- the checks against their restatement: the first failing spec and its reason, in the header's order
static ms::BpStatus def_validate(const std::vector<int32_t> &a, const std::vector<int32_t> &b, const std::vector<uint8_t> &flip, const std::vector<int32_t> &g0,
                                 const std::vector<int32_t> &g1, const std::vector<int32_t> &widths, int32_t *bad) {
    const int32_t P = (int32_t) widths.size();
    *bad = -1;
    for (size_t k = 0; k < a.size(); k++) {
        ms::BpStatus s = ms::kBpOk;
        if (a[k] < 0 || a[k] >= P || b[k] < 0 || b[k] >= P) s = ms::kBpIndex;
        else if (flip[k] != 0 && flip[k] != 1) s = ms::kBpFlip;
        else if (g0[k] < 0 || g0[k] > g1[k] || g1[k] > ms::kBpMaxGap) s = ms::kBpGap;
        else if (widths[(size_t) a[k]] > ms::kBpMaxWidth || widths[(size_t) b[k]] > ms::kBpMaxWidth) s = ms::kBpTooWide;
        if (s != ms::kBpOk) { *bad = (int32_t) k; return s; }
    }
    return ms::kBpOk;
}

static void one_validate(std::mt19937_64 &rng, int n, int faults) {
    std::vector<int32_t> widths = {1, 6, ms::kBpMaxWidth, ms::kBpMaxWidth + 1, 33};
    std::vector<int32_t> a((size_t) n), b((size_t) n), g0((size_t) n), g1((size_t) n);
    std::vector<uint8_t> flip((size_t) n);
    for (int k = 0; k < n; k++) {
        a[(size_t) k] = (int32_t) (rng() % 3);
        b[(size_t) k] = (rng() & 1) ? 4 : (int32_t) (rng() % 3);
        flip[(size_t) k] = (uint8_t) (rng() & 1);
        g0[(size_t) k] = (int32_t) (rng() % (uint64_t) (ms::kBpMaxGap + 1));
        g1[(size_t) k] = g0[(size_t) k] + (int32_t) (rng() % (uint64_t) (ms::kBpMaxGap + 1 - g0[(size_t) k]));
    }
    for (int f = 0; f < faults && n > 0; f++) {
        const size_t k = (size_t) (rng() % (uint64_t) n);
        switch (rng() % 8) {
        case 0: a[k] = -1; break;
        case 1: b[k] = (int32_t) widths.size(); break;
        case 2: flip[k] = 2; break;
        case 3: g0[k] = -1; break;
        case 4: g1[k] = g0[k] - 1; break;
        case 5: g1[k] = ms::kBpMaxGap + 1; break;
        case 6: a[k] = 3; break;                         // the element above the cap
        default: flip[k] = 255; break;
        }
    }
    int32_t bad = -7, want_bad = -7;
    const ms::BpStatus got = ms::bp_validate(a.data(), b.data(), flip.data(), g0.data(), g1.data(), n, widths.data(), (int32_t) widths.size(), &bad);
    const ms::BpStatus want = def_validate(a, b, flip, g0, g1, widths, &want_bad);
    CHECK(got == want && bad == want_bad);
    if (faults == 0) CHECK(got == ms::kBpOk);
    n_cases++;
}

static void by_hand() {
    int32_t bad = 0;
    const int32_t w[2] = {3, 5}, a[1] = {0}, b[1] = {1}, g[1] = {ms::kBpMaxGap};
    const uint8_t f[1] = {1};
    CHECK(ms::bp_validate(nullptr, nullptr, nullptr, nullptr, nullptr, 0, w, 2, &bad) == ms::kBpOk && bad == -1);
    CHECK(ms::bp_validate(nullptr, nullptr, nullptr, nullptr, nullptr, -1, w, 2, &bad) == ms::kBpCount);
    CHECK(ms::bp_validate(nullptr, b, f, g, g, 1, w, 2, &bad) == ms::kBpNull);
    CHECK(ms::bp_validate(a, b, f, g, nullptr, 1, w, 2, &bad) == ms::kBpNull);
    CHECK(ms::bp_validate(a, b, f, g, g, 1, w, 2, &bad) == ms::kBpOk);
    CHECK(ms::bp_validate(a, b, f, g, g, 1, w, 1, &bad) == ms::kBpIndex && bad == 0);
    CHECK(ms::bp_validate(a, b, f, g, g, 1, w, 0, &bad) == ms::kBpIndex);
    CHECK(64 * ms::kBpHaloStrips >= ms::kBpMaxWidth + ms::kBpMaxGap && 4 * 2 * ms::kBpMaxWidth <= ms::kBpTileEntries);
    n_cases++;
}

// ---- the key: sorting by it is sorting by (pos, strand, g - g_min), and its fields come back
static void keys(std::mt19937_64 &rng) {
    struct Pl { int64_t pos; int strand; int32_t dg; };
    std::vector<Pl> pl;
    for (int i = 0; i < 400; i++) {
        const int64_t pos = (i % 7 == 0) ? (int64_t) ((1LL << 31) - 1 - (int64_t) (rng() % 3)) : (int64_t) (rng() % 1000);
        pl.push_back({pos, 1 + (int) (rng() & 1), (int32_t) (rng() % (uint64_t) (ms::kBpMaxGap + 1))});
    }
    for (const Pl &p : pl) {
        const uint64_t k = ms::bp_key(p.pos, p.strand, p.dg);
        CHECK(k != ~0ULL && ms::bp_key_pos(k) == p.pos && ms::bp_key_strand(k) == p.strand && ms::bp_key_dg(k) == p.dg);
    }
    for (size_t i = 0; i + 1 < pl.size(); i++) {
        const Pl &p = pl[i], &q = pl[i + 1];
        const bool before = p.pos != q.pos ? p.pos < q.pos : p.strand != q.strand ? p.strand < q.strand : p.dg < q.dg;
        CHECK(before == (ms::bp_key(p.pos, p.strand, p.dg) < ms::bp_key(q.pos, q.strand, q.dg)));
    }
    n_cases++;
}

int main() {
    std::mt19937_64 rng(20261021);
    by_hand();
    const int widths[] = {1, 2, 3, 6, 31, 32, 33, 34, 63, ms::kBpMaxWidth};
    for (int Wa : widths)
        for (int Wb : widths) one_table(rng, Wa, Wb);
    for (int kind = 0; kind <= 6; kind++)
        for (int rep = 0; rep < 6; rep++) one_scorable(rng, 1 + (int) (rng() % 12), 1 + (int) (rng() % 12), kind);
    for (int rep = 0; rep < 40; rep++) one_validate(rng, (int) (rng() % 9), rep % 4);
    keys(rng);
    std::printf("bipartite_plan_asan: ok (%d cases)\n", n_cases);
    return 0;
}
