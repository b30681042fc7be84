// ms_scan_geom.h -- every decision a scan makes before its first launch (key layout, kernel family, LDS layout, launch geometry, buffer
// sizes, how the hits are ordered), as plain integer arithmetic on sizes: ms_scan_geom.cpp, pure host code with no HIP call, so that it
// also runs under the sanitizers without a device (tests/sanitize/plan_asan.cpp).  ms_scan.hip is its only user in the library.
#pragma once
#include <climits>

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

// the first key bit the radix passes cover when n_sort slots are ordered (the kernels behind them order the bits below)
MS_HIDDEN int scan_sort_begin(const ScanGeom &g, int32_t P, size_t n_sort);
// a buffer was too small: the counters hold the exact need -- the sizes of the next pass
MS_HIDDEN void scan_grow(size_t cand_cap, size_t hit_cap, unsigned long long n_cand, unsigned long long n_hits, size_t *want_cand, size_t *want_hits);

}  // namespace ms
