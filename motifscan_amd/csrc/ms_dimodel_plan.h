// ms_dimodel_plan.h -- the host's half of the first-order best-site walk (ms_scan_best_dimodels, ms_dimodel.hip): the checks of a model
// set's arguments, the table the device reads, the Viterbi maximum and the test for a model that is never scored.  Plain C++, no HIP
// include, so that it is checked on the CPU (tests/sanitize/dimodel_plan_asan.cpp), as ms_dense_plan.h is.  include/motifscan_amd.h holds
// the definition this restates; every operation on a double below is one rounded IEEE operation (the library and the sanitizer program
// are built with -ffp-contract=off).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <limits>

namespace ms {

// The walk's LDS tile holds kDiTileEntries table entries of 16 bytes (64 KB, as the PWM walk's); a model of W columns has
// 4 + 16 (W - 1) = 4 (4 W - 3) of them, so every model of up to kDiMaxWidth columns fits one tile and there is no table-in-HBM path.
constexpr int32_t kDiTileEntries = 4096;
constexpr int32_t kDiMaxWidth = (kDiTileEntries / 4 + 3) / 4;         // 256: 4 (4 * 256 - 3) = 4084 entries
static_assert(4 * (4 * kDiMaxWidth - 3) <= kDiTileEntries && 4 * (4 * (kDiMaxWidth + 1) - 3) > kDiTileEntries, "the cap is the widest model of one tile");
static_assert(kDiMaxWidth >= 64, "the cap must be at least 64");

struct DiEntry {                                         // one table entry: what a genome step adds to the forward and to the reverse sum
    double fwd, rev;
};
static_assert(sizeof(DiEntry) == 16, "an entry is one 16-byte LDS read");

// the "width" the dense plan sees: a model takes 4 * di_pseudo_width(W) entries, as a PWM of that many columns would
inline int32_t di_pseudo_width(int32_t W) { return 4 * W - 3; }
inline int64_t di_entries(int32_t W) { return 4 * (int64_t) di_pseudo_width(W); }

enum DiStatus { kDiOk = 0, kDiNull = 1, kDiCount = 2, kDiWidth = 3, kDiTooWide = 4 };

// values: the models' [W][16] rows one after the other; widths [n].  *bad: the model a width status names.
inline DiStatus di_validate(const double *values, const int32_t *widths, int32_t n, int32_t *bad) {
    *bad = -1;
    if (n < 0) return kDiCount;
    if (n > 0 && (!values || !widths)) return kDiNull;
    for (int32_t m = 0; m < n; m++) {
        if (widths[m] < 1) { *bad = m; return kDiWidth; }
        if (widths[m] > kDiMaxWidth) { *bad = m; return kDiTooWide; }
    }
    return kDiOk;
}

// v [W][16]: v_0[b] = start[b], v_j[b] = max_a (v_{j-1}[a] + trans[j][4 a + b]), max_raw = max_b v_{W-1}[b].  A comparison with a NaN
// is false, so a NaN candidate never replaces a number; di_scorable turns such a model away by its entries.
inline double di_max_raw(const double *v, int32_t W) {
    const double ninf = -std::numeric_limits<double>::infinity();
    double cur[4] = {v[0], v[1], v[2], v[3]};
    for (int32_t j = 1; j < W; j++) {
        const double *t = v + (size_t) j * 16;
        double nxt[4];
        for (int b = 0; b < 4; b++) {
            double best = ninf;
            for (int a = 0; a < 4; a++) {
                const double s = cur[a] + t[4 * a + b];
                if (s > best) best = s;
            }
            nxt[b] = best;
        }
        for (int b = 0; b < 4; b++) cur[b] = nxt[b];
    }
    double best = ninf;
    for (int b = 0; b < 4; b++)
        if (cur[b] > best) best = cur[b];
    return best;
}

// max_raw is a finite number > 0 and no entry that is read -- row 0's first four, every later row's sixteen -- is NaN or +inf
inline bool di_scorable(const double *v, int32_t W, double max_raw) {
    if (!(std::isfinite(max_raw) && max_raw > 0.0)) return false;
    const double pinf = std::numeric_limits<double>::infinity();
    for (int b = 0; b < 4; b++)
        if (std::isnan(v[b]) || v[b] == pinf) return false;
    for (size_t i = 16; i < (size_t) W * 16; i++)
        if (std::isnan(v[i]) || v[i] == pinf) return false;
    return true;
}

// The table of one model, out[di_entries(W)]:
//   entries 0 .. 3, by a base code x: {start[x], start[3 - x]} -- .fwd is read with the window's first base, .rev with its last;
//   entries 4 + 16 (c - 1) + q for the genome step c = 1 .. W - 1, by the four code bits q = x_{c-1} | x_c << 2 of the pair as they stand
//   in a packed word: {trans[c][4 x_{c-1} + x_c], trans[W - c][4 (3 - x_c) + (3 - x_{c-1})]}.
inline void di_build_table(const double *v, int32_t W, DiEntry *out) {
    for (int x = 0; x < 4; x++) { out[x].fwd = v[x]; out[x].rev = v[3 - x]; }
    for (int32_t c = 1; c < W; c++) {
        DiEntry *e = out + 4 + 16 * (size_t) (c - 1);
        const double *tf = v + (size_t) c * 16, *tr = v + (size_t) (W - c) * 16;
        for (int q = 0; q < 16; q++) {
            const int x0 = q & 3, x1 = q >> 2;
            e[q].fwd = tf[4 * x0 + x1];
            e[q].rev = tr[4 * (3 - x1) + (3 - x0)];
        }
    }
}

}  // namespace ms
