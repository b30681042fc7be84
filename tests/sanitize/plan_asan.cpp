// tests/sanitize/plan_asan.cpp -- the host side of the pre-filter (motifscan_amd/csrc/ms_plan.cpp: thresholds, the e2m3
// quantiser, paired rows, the row-tile DP, the operand image) under AddressSanitizer + UndefinedBehaviorSanitizer, compiled
// by plain g++ from the SAME source file the library is built from -- and, on plans built the way a scan builds them, the scan's
// geometry (ms_scan_geom.cpp: key layout, LDS layout, launch shape) over a small grid of set shapes and devices, against the
// invariants the kernels rely on.  CPU build container only (`make -C motifscan_amd/csrc
// sanitize`; tests/test_sanitizers.py runs it, once with the benchmark motif set dumped to a raw file).
//
//     plan_asan [motifs.bin]      motifs.bin: int32 n, int32 widths[n], double cutoffs[n][n_sets], int32 n_sets, double values[...]
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../motifscan_amd/csrc/ms_scan_geom.h"

namespace ms {
void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    std::vfprintf(stderr, fmt, ap);
    va_end(ap);
    std::fputc('\n', stderr);
}
}  // namespace ms

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } \
    } while (0)

namespace {

double c_max_raw(const double *m, int W) {          // cscore.c:36-48: column maxima start at 0
    double s = 0;
    for (int c = 0; c < W; c++) {
        double mx = 0;
        for (int b = 0; b < 4; b++) if (m[(size_t) b * W + c] > mx) mx = m[(size_t) b * W + c];
        s += mx;
    }
    return s;
}

long n_plans = 0, n_geoms = 0;

bool pow2(int64_t v) { return v > 0 && (v & (v - 1)) == 0; }

// what the pre-filter (ms_kernels.hip) and ms_order.hip take for granted about a scan's geometry (the comments of ms_kernels.h and ms_scan_geom.cpp)
void check_geometry(const ms::ScanShape &sh, const ms::ScanOverrides &ov) {
    const ms::ScanGeom g = ms::scan_geometry(sh, ov);
    n_geoms++;
    CHECK(g.lds_bytes <= sh.lds_max / (size_t) ms::kPfBlocksPerCu);
    CHECK(g.lds_fixed == (g.wide ? ms::kPfLdsFixedWide : ms::kPfLdsFixedNarrow) && (size_t) g.rare_off16 * 16 + ms::kPfRareBytesMin <= g.lds_bytes);
    CHECK(g.rare_cap >= (uint32_t) ms::kRareCapMin && g.rare_cap <= (uint32_t) ms::kRareCapMax);
    CHECK(g.bpt >= 1);
    CHECK(g.wave_passes >= 1 && (!g.counter_used || pow2(g.wave_passes)));
    CHECK(pow2(g.cand_block) && g.cand_block >= 64 && g.cand_block <= 2048);
    CHECK(g.end_bit <= 64 && g.end_bit == g.gbits + 1 + g.mbits);
    int gbits_global = 1;
    while ((1LL << gbits_global) <= sh.n_bases) gbits_global++;
    CHECK(g.pbits == 0 ? g.gbits == gbits_global : (g.gbits == g.rbits + g.pbits && g.rbits + g.pbits <= gbits_global + 2));
    CHECK(g.wide == sh.plan->wide && !(g.wide && g.dense));
}

// the plan as scan_plan (ms_scan.hip) builds it for a device of lds_max bytes of LDS per block, then the geometry over the grid
void geometry_all(const std::vector<double> &values, const std::vector<int64_t> &off, const std::vector<int32_t> &widths,
                  const std::vector<double> &cutoffs, const std::vector<double> &max_raw, int strand) {
    const int32_t n = (int32_t) widths.size();
    ms::ScanOverrides test_ov;                                  // the switches tests/test_gpu_parity.py drives, at their harshest
    test_ov.lds_budget = 4096; test_ov.rare_cap_max = ms::kRareCapMin; test_ov.max_blocks = 2; test_ov.pf_dense = 1; test_ov.sort_low_bits = 24;
    for (const ms::ScanOverrides &ov : {ms::ScanOverrides(), test_ov})
        for (size_t lds_max : {(size_t) 64 * 1024, (size_t) 160 * 1024}) {
            ms::PrefilterPlan plan;
            int rc = ms::build_plan(values.data(), off.data(), widths.data(), cutoffs.data(), max_raw.data(), n, strand,
                                    ms::scan_lds_budget(lds_max, true, ov), true, &plan);
            if (rc != MS_OK) continue;
            const bool wide = plan.wide;
            rc = ms::build_plan(values.data(), off.data(), widths.data(), cutoffs.data(), max_raw.data(), n, strand,
                                ms::scan_lds_budget(lds_max, wide, ov), true, &plan);
            CHECK(rc == MS_OK && plan.wide == wide);             // the kernel family does not depend on the budget
            const int64_t shapes[4][2] = {{1, 3000000000LL}, {1000000, 50}, {1, 1}, {0, 0}};       // (regions, bases of each)
            for (const auto &shape : shapes)
                for (int n_cu : {1, 256})
                    for (double density : {-1.0, 0.05}) {
                        ms::ScanShape sh;
                        sh.plan = &plan; sh.P = n;
                        sh.R = shape[0]; sh.max_len = shape[1]; sh.n_bases = shape[0] * shape[1];
                        for (int32_t p : plan.fast_motifs) sh.fast_windows += shape[0] * std::max<int64_t>(shape[1] - widths[(size_t) p] + 1, 0);
                        sh.n_cu = n_cu; sh.lds_max = lds_max; sh.cu_reserved = n_cu / 32;
                        sh.density_known = density >= 0; sh.pred_density = density;
                        check_geometry(sh, ov);
                    }
        }
}

void plan_all(const std::vector<double> &values, const std::vector<int32_t> &widths, const std::vector<double> &cutoffs) {
    const int32_t n = (int32_t) widths.size();
    std::vector<int64_t> off((size_t) n + 1, 0);
    for (int32_t p = 0; p < n; p++) off[(size_t) p + 1] = off[(size_t) p] + 4 * (int64_t) widths[(size_t) p];
    CHECK((size_t) off[(size_t) n] == values.size());
    std::vector<double> max_raw((size_t) n);
    for (int32_t p = 0; p < n; p++) max_raw[(size_t) p] = c_max_raw(values.data() + off[(size_t) p], widths[(size_t) p]);
    for (int strand = 1; strand <= 3; strand++) {
        geometry_all(values, off, widths, cutoffs, max_raw, strand);
        for (int pair = 0; pair < 2; pair++)
            for (size_t lds : {(size_t) 8 * 1024, (size_t) 24 * 1024, (size_t) 70 * 1024, (size_t) 139 * 1024}) {
                ms::PrefilterPlan plan;
                const int rc = ms::build_plan(values.data(), off.data(), widths.data(), cutoffs.data(), max_raw.data(), n, strand, lds,
                                              pair != 0, &plan);
                CHECK(rc == MS_OK || rc == MS_ERR_INVALID || rc == MS_ERR_NOMEM);
                if (rc != MS_OK) continue;
                n_plans++;
                CHECK(plan.fast_motifs.size() + plan.exact_motifs.size() == (size_t) n);
                CHECK(plan.group_fields.size() == plan.group_kb.size() * ms::kGroupFields);
                for (int32_t f : plan.group_fields) CHECK(f >= -1 && f < n);
                for (const auto &t : plan.tiles)                          // every tile's operand image lies inside the table buffer
                    CHECK(((size_t) t.table_off16 + t.table_len16) * 16 <= plan.tables.size() * sizeof(uint32_t) && t.n_classes <= ms::kMaxClasses);
            }
    }
}

}  // namespace

int main(int argc, char **argv) {
    std::mt19937_64 rng(20250310);
    std::uniform_real_distribution<double> uni(0.0, 1.0);
    // (1) random log-odds-like sets over every width the plan distinguishes (1 ... 70: > 63 goes to the exact kernel), cutoffs
    //     from far below to above the attainable range, plus the degenerate matrices of SURVEY.md Q4 (max_raw = 0, -inf, huge)
    for (int round = 0; round < 12; round++) {
        std::vector<double> values;
        std::vector<int32_t> widths;
        std::vector<double> cutoffs;
        const int n = round == 0 ? 0 : (round == 1 ? 1 : 40 + 37 * round);
        for (int p = 0; p < n; p++) {
            const int W = 1 + (int) (rng() % 70);
            widths.push_back(W);
            const int kind = (int) (rng() % 16);
            for (int b = 0; b < 4; b++)
                for (int c = 0; c < W; c++) {
                    double v = std::round(1e5 * std::log((0.002 + uni(rng)) / 0.25)) / 1e5;
                    if (kind == 0) v = -std::fabs(v) - 0.1;                         // max_raw = 0
                    if (kind == 1 && (b + c) % 5 == 0) v = -INFINITY;
                    if (kind == 2) v *= 1e6;
                    if (kind == 3) v *= 1e-8;
                    if (kind == 4) v = 0.0;
                    values.push_back(v);
                }
            const double cuts[] = {0.35 + 0.5 * uni(rng), -0.3, 0.0, 1.0, 1.0 + 1e-10, 2.0, 1e-300, NAN};
            cutoffs.push_back(kind >= 8 ? cuts[0] : cuts[rng() % 8]);
        }
        plan_all(values, widths, cutoffs);
    }
    // (2) the benchmark motif set at each of its cutoff columns, when the test hands it over
    if (argc > 1) {
        FILE *f = std::fopen(argv[1], "rb");
        CHECK(f);
        int32_t n = 0, n_sets = 0;
        CHECK(std::fread(&n, 4, 1, f) == 1 && std::fread(&n_sets, 4, 1, f) == 1 && n > 0 && n_sets > 0);
        std::vector<int32_t> widths((size_t) n);
        CHECK(std::fread(widths.data(), 4, (size_t) n, f) == (size_t) n);
        std::vector<double> cuts((size_t) n * (size_t) n_sets);
        CHECK(std::fread(cuts.data(), 8, cuts.size(), f) == cuts.size());
        size_t nv = 0;
        for (int32_t w : widths) nv += 4 * (size_t) w;
        std::vector<double> values(nv);
        CHECK(std::fread(values.data(), 8, nv, f) == nv);
        std::fclose(f);
        for (int s = 0; s < n_sets; s++) {
            std::vector<double> c((size_t) n);
            for (int32_t p = 0; p < n; p++) c[(size_t) p] = cuts[(size_t) p * (size_t) n_sets + (size_t) s];
            plan_all(values, widths, c);
        }
    }
    std::printf("plan_asan: ok (%ld plans, %ld scan geometries)\n", n_plans, n_geoms);
    return 0;
}
