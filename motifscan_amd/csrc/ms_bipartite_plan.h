// ms_bipartite_plan.h -- the host's half of the bipartite best-site walk (ms_scan_best_bipartite, ms_bipartite.hip): the checks of the
// spec arrays, the test for a spec that is never scored, the denominator, the pseudo-widths the dense plan tiles by and the table the
// device reads.  Plain C++, no HIP include, so that it is checked on the CPU (tests/sanitize/bipartite_plan_asan.cpp), as
// ms_dimodel_plan.h is.  include/motifscan_amd.h holds the definition this restates; every operation on a double below is one rounded
// IEEE operation (the library and the sanitizer program are built with -ffp-contract=off).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <limits>

namespace ms {

// The caps of the walk.  An element of up to kBpMaxWidth columns and a gap of up to kBpMaxGap bases put the second half at most
// kBpMaxWidth + kBpMaxGap = 128 window starts behind the first: kBpHaloStrips strips of 64.  A spec's two tables take 4 (W_a + W_b)
// entries of 16 bytes, at most 8 KB, so every spec fits a tile of kBpTileEntries entries (32 KB) many times over.
constexpr int32_t kBpMaxWidth = 64;
constexpr int32_t kBpMaxGap = 64;
constexpr int32_t kBpHaloStrips = 2;
constexpr int32_t kBpTileEntries = 2048;
static_assert(kBpMaxWidth + kBpMaxGap <= 64 * kBpHaloStrips, "the second half lies inside the halo");
static_assert(4 * 2 * kBpMaxWidth <= kBpTileEntries, "every spec fits a tile");
static_assert(kBpMaxGap < 128, "g - g_min takes seven bits of the reduction key");

struct BpEntry {                                         // one table entry: what a base adds to the forward and to the reverse sum (the PWM walk's tab2 entry)
    double fwd, rev;
};
static_assert(sizeof(BpEntry) == 16, "an entry is one 16-byte LDS read");

// the "width" the dense plan sees: a spec takes 4 * bp_pseudo_width entries, as a PWM of that many columns would
inline int32_t bp_pseudo_width(int32_t Wa, int32_t Wb) { return Wa + Wb; }
inline int64_t bp_entries(int32_t Wa, int32_t Wb) { return 4 * (int64_t) bp_pseudo_width(Wa, Wb); }

enum BpStatus { kBpOk = 0, kBpNull = 1, kBpCount = 2, kBpIndex = 3, kBpFlip = 4, kBpGap = 5, kBpTooWide = 6 };

// a, b, flip, gap_min, gap_max [n]; widths [P] of the PWM set.  *bad: the spec a status from kBpIndex on names.
inline BpStatus bp_validate(const int32_t *a, const int32_t *b, const uint8_t *flip, const int32_t *gap_min, const int32_t *gap_max, int32_t n, const int32_t *widths,
                            int32_t P, int32_t *bad) {
    *bad = -1;
    if (n < 0) return kBpCount;
    if (n > 0 && (!a || !b || !flip || !gap_min || !gap_max)) return kBpNull;
    for (int32_t k = 0; k < n; k++) {
        *bad = k;
        if (a[k] < 0 || a[k] >= P || b[k] < 0 || b[k] >= P) return kBpIndex;
        if (flip[k] > 1) return kBpFlip;
        if (gap_min[k] < 0 || gap_min[k] > gap_max[k] || gap_max[k] > kBpMaxGap) return kBpGap;
        if (widths[a[k]] > kBpMaxWidth || widths[b[k]] > kBpMaxWidth) return kBpTooWide;
    }
    *bad = -1;
    return kBpOk;
}

// no entry of the [4][W] matrix is NaN or +inf (entries_scorable of ms_best_dev.h, on the values alone)
inline bool bp_entries_ok(const double *m, int32_t W) {
    for (int64_t i = 0; i < 4 * (int64_t) W; i++)
        if (std::isnan(m[i]) || m[i] == std::numeric_limits<double>::infinity()) return false;
    return true;
}

// the denominator of a spec's scores: one rounded addition of the two elements' max_raw
inline double bp_denominator(double max_raw_a, double max_raw_b) { return max_raw_a + max_raw_b; }

// both elements pass the entry test and the SUM of their max_raw is a finite number > 0 (an element whose columns are all zero is legal)
inline bool bp_scorable(const double *ma, int32_t Wa, double max_raw_a, const double *mb, int32_t Wb, double max_raw_b) {
    const double d = bp_denominator(max_raw_a, max_raw_b);
    return std::isfinite(d) && d > 0.0 && bp_entries_ok(ma, Wa) && bp_entries_ok(mb, Wb);
}

// The table of one element, out[4 W]: entry 4 c + x for column c and base code x holds {M[x][c], M[3 - x][W - 1 - c]} -- what the PWM
// walks read (ms_pwmset.hip lays tab2 out the same way), so the element sums are ms_scan_best's.  m: [4][W] row-major.
inline void bp_element_table(const double *m, int32_t W, BpEntry *out) {
    for (int32_t c = 0; c < W; c++)
        for (int x = 0; x < 4; x++) {
            out[(size_t) c * 4 + x].fwd = m[(size_t) x * W + c];
            out[(size_t) c * 4 + x].rev = m[(size_t) (3 - x) * W + (W - 1 - c)];
        }
}

// The table of spec k: the entries of a, then those of b, at out[bp_entries(Wa, Wb)].
inline void bp_spec_table(const double *ma, int32_t Wa, const double *mb, int32_t Wb, BpEntry *out) {
    bp_element_table(ma, Wa, out);
    bp_element_table(mb, Wb, out + 4 * (size_t) Wa);
}

// (constexpr: the kernel calls them too)
// the key of the total-order reduction: the walk's order within a cell -- pos, then strand ('+' = 1 before '-' = 2), then g - g_min
constexpr uint64_t bp_key(int64_t pos, int strand, int32_t dg) { return ((uint64_t) pos << 9) | ((uint64_t) strand << 7) | (uint64_t) dg; }
constexpr int64_t bp_key_pos(uint64_t key) { return (int64_t) (key >> 9); }
constexpr int bp_key_strand(uint64_t key) { return (int) ((key >> 7) & 3u); }
constexpr int32_t bp_key_dg(uint64_t key) { return (int32_t) (key & 127u); }

}  // namespace ms
