// ms_scan_geom.h -- every decision a scan makes before its first launch (key layout, kernel family, LDS layout, launch geometry, buffer
// sizes, how the hits are ordered), as plain integer arithmetic on sizes: ms_scan_geom.cpp, pure host code with no HIP call, so that it
// also runs under the sanitizers without a device (tests/sanitize/plan_asan.cpp).  ms_scan.hip is its only user in the library.
#pragma once
#include <climits>
#include <cmath>

#include "ms_kernels.h"

namespace ms {

// The scan pipeline's MS_MEASURE test switches (ms_internal.h: measure_env), each holding the product's value unless its variable is set.
// Read once per scan and never kept across scans: the tests change the environment between two scans of one process.
struct ScanOverrides {
    size_t lds_budget = (size_t) -1;      // MS_PF_LDS_BUDGET: at most this many bytes of tables per LDS tile (several tiles, as a very large motif set would have)
    int pf_dense = -1;                    // MS_PF_DENSE: 0 / 1 = the parked / the dense pre-filter at any density (never for a wide plan); -1: by density
    int rare_cap_max = kRareCapMax;       // MS_PF_RARE_CAP: at most this many parking entries per wave (kRareCapMin at least)
    int max_blocks = INT_MAX;             // MS_PF_MAX_BLOCKS: few blocks per tile, as a very large motif set would have
    bool coord_global = false;            // MS_HIT_COORD=global: hit keys carry the global base position, never (region, position)
    double rescore_sorted_min = 2.0e6;    // MS_RESCORE_SORTED_MIN: expected candidates from which the fp64 stage takes the carried form (0 = always, 1e30 = never)
    bool sort_full = false;               // MS_SORT_FULL: every key bit by radix passes
    int sort_low_bits = -1;               // MS_SORT_LOW_BITS: force L of order_low_bits (the motif bits stay above it); -1: by run length
    int order_run_cap = 1 << 30;          // MS_ORDER_RUN_CAP: longer runs take order_finalize_kernel's overflow path
    size_t fixup_min = (size_t) 1 << 20;  // MS_SORT_FIXUP_MIN: the fix-up form from this many hits (0: on short lists too)
    bool no_predict = false;              // MS_NO_PREDICT: never the predicted-size form
    int order_buckets = -1;               // MS_ORDER_BUCKETS: 0 / 1 = the fp64 stage never / at any list size emits its hits in low-digit buckets; -1: by size (bucket_gate)
    uint64_t bucket_cap_max = ~0ULL;      // MS_ORDER_BUCKET_CAP: no bucket holds more than this many hits (a test's way to the overflow path)
};
MS_HIDDEN ScanOverrides read_scan_overrides();

// the B-operand table, the waves' sequence staging, their PfEmit and (at least) kRareCapMin parking entries follow the tables -- and the
// waves' one-hot arrays (40 KB) in the double-pass kernels ONLY: a plan with a wide tile (a motif of 32 ... 63 columns on the pre-filter)
// runs the single-pass kernels, which never touch that array, and keeps the room for its tables
constexpr size_t kPfLdsFixedWide = kF6LutBytes + kPfStageBytes + kPfEmitBytes + kPfRareBytesMin;
constexpr size_t kPfLdsFixedNarrow = kPfLdsFixedWide + kPfOnehotBytes;
// what a block's LDS leaves for one tile's tables: the budget the plan is built with
MS_HIDDEN size_t scan_lds_budget(size_t lds_max, bool wide, const ScanOverrides &ov);

struct ScanShape {                       // the sizes a scan's geometry follows from
    const PrefilterPlan *plan = nullptr; // tiles, kb_total, the fast and exact motif lists, wide
    int32_t P = 0;                       // motifs of the set
    int64_t n_bases = 0, R = 0, max_len = 0;   // the sequence set: bases, regions, the longest region
    int64_t fast_windows = 0;            // windows of the motifs on the pre-filter
    int n_cu = 0;                        // the device: CUs, LDS bytes per block, CUs the copy streams own while a batch stream is live
    size_t lds_max = 0;
    int cu_reserved = 0;
    bool density_known = false;          // the PWM set's prediction state: the previous scan at these cutoffs and strands found ...
    double pred_density = -1.0;          // ... this many hits per (motif, window)
};

struct ScanGeom {
    // hit keys: motif << (gbits + 1) | coordinate << 1 | strand bit (HitOut)
    int gbits = 1, rbits = 1, pbits = 0, mbits = 1, end_bit = 0;
    int coord_shift12 = 0;               // the 4-byte compact coordinate (MS_SCAN_PACK12_INTERNAL): position bits + 1 when the set fits, else 0
    // pre-filter: kernel family and LDS layout (PfArgs, 16-byte units)
    bool wide = false, dense = false;
    size_t lds_fixed = 0, lds_bytes = 0;
    uint32_t lut_off16 = 0, stage_off16 = 0, emit_off16 = 0, onehot_off16 = 0, rare_off16 = 0, rare_cap = kRareCapMin;
    // pre-filter: launch geometry
    int n_tiles = 0, bpt = 1, wave_passes = 1;
    bool counter_used = true;
    uint32_t cand_block = 64;
    uint64_t cand_static = 0;            // the waves' own first candidate blocks (PfArgs::cand_static)
    // scratch sizes of the first pass
    size_t want_cand = 0, want_hits = 0;
    bool rescore_carry = false;          // fp64 stage: the carried form for long candidate lists
    // ordering
    int sort_begin_large = 0, sort_low_bits = -1, order_run_cap = 1 << 30;
    size_t fixup_min = (size_t) 1 << 20;
};
MS_HIDDEN ScanGeom scan_geometry(const ScanShape &s, const ScanOverrides &ov);
// the key fields alone (gbits, rbits, pbits, mbits, end_bit, coord_shift12) of a set of these sizes: what scan_geometry() puts there
MS_HIDDEN ScanGeom scan_key_layout(int64_t n_bases, int64_t R, int64_t max_len, int32_t P, bool coord_global);

// the first key bit the radix passes cover when n_sort slots are ordered (the kernels behind them order the bits below)
MS_HIDDEN int scan_sort_begin(const ScanGeom &g, int32_t P, size_t n_sort);
// ---- hits emitted in buckets of the lowest radix digit d0 = (key >> L) & 255 (ms_fp64.hip, "the bucketed flush"): the pass over that digit
// is the identity on such a list, so the radix passes start at L + 8.  Bucket b owns cap_b slots of the predicted-size list, in digit order.
// offsets [R + 1], widths [P] as the scan sees them; the hit density of a scan is taken as uniform over these pairs (the prediction's own model)
MS_HIDDEN void bucket_weights(const int64_t *offsets, int64_t R, const int32_t *widths, int32_t P, int gbits, int pbits, int L, BucketWeights *out);
// a bucket's share of mu expected hits, and the slots it needs at least: that share + 6 sigma of a Poisson count + 1 (0 for a bucket no key can fall
// into).  The same expressions, operation for operation, in bucket_plan_kernel (ms_order.hip).
inline double bucket_expected(double mu, unsigned long long w, unsigned long long total) { return total ? mu * (double) w / (double) total : 0.0; }
inline unsigned long long bucket_need_one(double mu, unsigned long long w, unsigned long long total) {
    if (!w) return 0;
    const double e = bucket_expected(mu, w, total);
    return (unsigned long long) std::ceil(e + 6.0 * std::sqrt(e + 1.0)) + 1ULL;
}
MS_HIDDEN unsigned long long bucket_need(const BucketWeights &bw, double mu);         // the sum over the buckets
// cap_b = need_b + the bucket's share (rounded down) of what n_pred leaves above the sum of the needs, at most cap_max, and cut off where the
// running sum would pass n_pred: sum cap_b <= n_pred always; cap_b >= need_b for every b when bucket_need() <= n_pred and cap_max allows it
MS_HIDDEN void bucket_caps(const BucketWeights &bw, double mu, unsigned long long n_pred, unsigned long long cap_max, unsigned long long *base, unsigned long long *cap);
struct BucketShape {                     // what the gate looks at besides the sizes
    bool predicted = false, counts_only = false, carry_only = false, sticky_off = false;   // carry_only: the fp64 stage is rescore_carry_kernel alone
    int pbits = 0, gbits = 0, end_bit = 0, L = 0;
    int64_t P = 0, R = 0;                // motifs and regions: the largest key of the scan
};
// whether the key layout can be bucketed at all (any forced or unforced scan): d0 must lie inside the coordinate bits, and no hit key may
// be all ones in the bits they sort -- the padding keys stand IN FRONT of later buckets' hits, and a stable sort would leave them there on a tie
MS_HIDDEN bool bucket_layout_ok(const BucketShape &s);
// the product's gate: every condition of the form, then the size -- the per-bucket slack must fit inside the prediction's own margin, that is
// need <= n_pred.  MS_ORDER_BUCKETS=1 passes any size of a layout bucket_layout_ok() takes (the caller raises n_pred to the need); =0 never.
MS_HIDDEN bool bucket_gate(const BucketShape &s, const ScanOverrides &ov, unsigned long long need, unsigned long long n_pred);

// a buffer was too small: the counters hold the exact need -- the sizes of the next pass
MS_HIDDEN void scan_grow(size_t cand_cap, size_t hit_cap, unsigned long long n_cand, unsigned long long n_hits, size_t *want_cand, size_t *want_hits);

}  // namespace ms
