// ms_scan_geom.cpp -- a scan's geometry from its sizes (ms_scan_geom.h).  Pure host code: no HIP call, no handle.
#include <algorithm>
#include <cmath>
#include <vector>

#include "ms_scan_geom.h"

namespace ms {

ScanOverrides read_scan_overrides() {
    ScanOverrides o;
    if (const char *e = measure_env("MS_PF_LDS_BUDGET")) o.lds_budget = (size_t) std::max(1, atoi(e));
    if (const char *e = measure_env("MS_PF_DENSE")) o.pf_dense = atoi(e) != 0 ? 1 : 0;          // test aid / A-B: either form at any density
    if (const char *e = measure_env("MS_PF_RARE_CAP")) o.rare_cap_max = std::max(kRareCapMin, atoi(e));
    if (const char *e = measure_env("MS_PF_MAX_BLOCKS")) o.max_blocks = std::max(1, atoi(e));
    if (const char *e = measure_env("MS_HIT_COORD")) o.coord_global = e[0] == 'g';
    if (const char *e = measure_env("MS_RESCORE_SORTED_MIN")) o.rescore_sorted_min = atof(e);   // test aid / A-B: 0 = always, 1e30 = never
    o.sort_full = measure_env("MS_SORT_FULL") != nullptr;
    if (const char *e = measure_env("MS_SORT_LOW_BITS")) o.sort_low_bits = std::max(0, atoi(e));
    if (const char *e = measure_env("MS_ORDER_RUN_CAP")) o.order_run_cap = std::max(1, atoi(e));
    if (const char *e = measure_env("MS_SORT_FIXUP_MIN")) o.fixup_min = (size_t) std::max(0, atoi(e));
    o.no_predict = measure_env("MS_NO_PREDICT") != nullptr;
    if (const char *e = measure_env("MS_ORDER_BUCKETS")) o.order_buckets = atoi(e) != 0 ? 1 : 0;   // test aid / A-B: the bucketed hit list at any size, or never
    if (const char *e = measure_env("MS_ORDER_BUCKET_CAP")) o.bucket_cap_max = (uint64_t) std::max(0LL, atoll(e));
    return o;
}

size_t scan_lds_budget(size_t lds_max, bool wide, const ScanOverrides &ov) {
    return std::min(lds_max / (size_t) kPfBlocksPerCu - (wide ? kPfLdsFixedWide : kPfLdsFixedNarrow), ov.lds_budget);
}

static int bits_for(int64_t n) {                  // the least b >= 1 with 2^b >= n
    int b = 1;
    while ((1LL << b) < std::max<int64_t>(n, 1)) b++;
    return b;
}

static void key_layout(const ScanShape &s, const ScanOverrides &ov, ScanGeom &g) {
    while ((1LL << g.gbits) <= s.n_bases) g.gbits++;
    // hit coordinate = (region, position in the region) when that costs at most 2 more key bits than the global base
    // position: finalize_rp_kernel then needs no position -> region look-ups.  MS_HIT_COORD=global forces the other form.
    const int pb = bits_for(s.max_len);
    g.rbits = bits_for(s.R);
    if (g.rbits + pb <= g.gbits + 2 && !ov.coord_global) { g.pbits = pb; g.gbits = g.rbits + pb; }
    g.mbits = bits_for(s.P);
    g.end_bit = g.gbits + 1 + g.mbits;
    // the 4-byte compact coordinate when the set's largest region index and position fit 31 bits beside the strand bit
    g.coord_shift12 = g.rbits + pb + 1 <= 32 ? pb + 1 : 0;
}

ScanGeom scan_key_layout(int64_t n_bases, int64_t R, int64_t max_len, int32_t P, bool coord_global) {
    ScanShape s;
    s.n_bases = n_bases; s.R = R; s.max_len = max_len; s.P = P;
    ScanOverrides ov;
    ov.coord_global = coord_global;
    ScanGeom g;
    key_layout(s, ov, g);
    return g;
}

static void lds_layout(const ScanShape &s, const ScanOverrides &ov, ScanGeom &g) {
    g.lds_fixed = g.wide ? kPfLdsFixedWide : kPfLdsFixedNarrow;
    size_t tables = 0;
    for (const TileDesc &t : s.plan->tiles) tables = std::max(tables, (size_t) t.table_len16 * 16);
    g.lut_off16 = (uint32_t) (tables / 16);
    g.stage_off16 = g.lut_off16 + (uint32_t) (kF6LutBytes / 16);
    g.emit_off16 = g.stage_off16 + (uint32_t) (kPfStageBytes / 16);
    g.onehot_off16 = g.emit_off16 + (uint32_t) (kPfEmitBytes / 16);
    g.rare_off16 = g.onehot_off16 + (uint32_t) ((g.wide ? 0 : kPfOnehotBytes) / 16);      // (a wide plan's kernels have no one-hot array)
    g.lds_bytes = tables + g.lds_fixed;
    // the waves' candidate parking space takes what the tables leave of the block's LDS: kRareCapMin ... kRareCapMax entries per wave
    const size_t per_entry = (size_t) (kPfThreads / 64) * kRareEntryWords * sizeof(uint32_t);
    const size_t avail = s.lds_max / (size_t) kPfBlocksPerCu;
    if (avail > g.lds_bytes) g.rare_cap = (uint32_t) std::min<size_t>((size_t) kRareCapMax, (size_t) kRareCapMin + (avail - g.lds_bytes) / per_entry);
    g.rare_cap = std::min(g.rare_cap, (uint32_t) ov.rare_cap_max);                          // test aid
    g.lds_bytes += (size_t) (g.rare_cap - (uint32_t) kRareCapMin) * per_entry;
}

// blocks per tile and the unit of the per-wave hand-out
static void launch_shape(const ScanShape &s, const ScanOverrides &ov, ScanGeom &g) {
    if (g.n_tiles == 0) return;
    // While a batch stream is live and the device is partitioned (StreamSel): the scan owns n_cu - cu_reserved CUs (the
    // units are handed out dynamically: fewer blocks just take more each)
    const int64_t pf_chunks = (s.n_bases + kPfThreads - 1) / kPfThreads;
    g.bpt = (int) std::max<int64_t>(1, std::min<int64_t>(pf_chunks, (s.n_cu - s.cu_reserved) * kPfBlocksPerCu / g.n_tiles));
    g.bpt = std::min(g.bpt, ov.max_blocks);
    // unit of the per-wave hand-out: a pass (64 window starts against a tile's k-blocks; 128 in a double pass) takes ~0.25 us per k-block and 64 windows with 16
    // waves per CU, and the launch's waves should not exceed ~47 atomics per microsecond on a tile's counter word
    const int64_t kb_tile = std::max<int64_t>(1, s.plan->kb_total / g.n_tiles);
    const double waves = (double) g.bpt * (kPfThreads / 64);                          // per tile
    const double waves_word = waves / std::min(kPfCounters, g.bpt);                   // ... and per counter word
    const int64_t pass_windows = g.wide ? 64 : 128;                                   // the kernels without wide classes scan double passes (ms_kernels.hip)
    const int64_t need = (int64_t) std::ceil(waves_word / (47.0 * 0.25 * (double) (pass_windows / 64) * (double) kb_tile));
    const int64_t passes_total = (s.n_bases + pass_windows - 1) / pass_windows, n_waves = (int64_t) waves;
    int64_t wp = 2;                                               // a power of two: units start on 128-position boundaries at least
    while (wp < 256 && (double) wp < 0.9 * (double) need) wp *= 2;            // the words' rate limit
    while (wp < 8 && 128 * wp <= passes_total / n_waves) wp *= 2;             // a long launch: the tail (one unit) stays below 1 % anyway, fewer atomics
    if (passes_total <= 8 * std::max<int64_t>(wp, 8) * n_waves) {
        // fewer than 8 units (of 8 passes at least) per wave: one even unit each and no atomics (a second round of a few
        // units would leave most waves idle); the kernel then never touches the counter words
        wp = std::max<int64_t>(1, (passes_total + n_waves - 1) / n_waves);
        g.counter_used = false;
    }
    g.wave_passes = (int) wp;
    g.cand_static = (uint64_t) std::min<int64_t>(g.bpt, pf_chunks) * g.n_tiles * (kPfThreads / 64) * g.cand_block;
}

ScanGeom scan_geometry(const ScanShape &s, const ScanOverrides &ov) {
    const PrefilterPlan &plan = *s.plan;
    ScanGeom g;
    key_layout(s, ov, g);
    g.wide = plan.wide;
    g.n_tiles = (int) plan.tiles.size();

    // expected density at the CLI default p = 1e-4 is ~1.5e-4 candidates per window and strand; 4x head room
    g.want_cand = (size_t) std::min<double>(std::max<double>(1 << 20, 6e-4 * (double) s.fast_windows), 3.0e9);
    g.want_hits = g.want_cand;
    if (!plan.exact_motifs.empty()) g.want_hits = std::max<size_t>(g.want_hits, 1 << 22);
    // a wave reserves candidate slots in blocks (ms_kernels.hip, "candidate hand-off"): about a quarter of what it is expected to
    // need, 64 ... 2048 (its first block is its own, without an atomic); the slots a wave leaves unused in its last block are head
    // room on top
    const int64_t pf_waves_max = (int64_t) s.n_cu * kPfBlocksPerCu * (kPfThreads / 64);
    // what the previous scan of this set at these cutoffs and strands found, per (motif, window): sizes the blocks, and picks the kernel form
    const double cand_density = s.density_known ? std::max(1.5e-4, 1.3 * s.pred_density) : 1.5e-4;
    while (g.cand_block < 2048 && (double) g.cand_block * 4.0 * (double) pf_waves_max < cand_density * (double) s.fast_windows) g.cand_block *= 2;
    g.want_cand += (size_t) 2 * pf_waves_max * g.cand_block;          // the waves' own first blocks + the unused rest of their last ones

    // the dense-candidate form of the pre-filter (ms_kernels.hip): expected hits per row tile and 64 window starts above kDenseHitsPerHalfTile
    int64_t n_row_tiles = 0;
    for (const TileDesc &t : plan.tiles)
        for (int i = 0; i < t.n_classes; i++) n_row_tiles += t.cls[i].n_row_tiles;
    if (s.density_known && !g.wide && n_row_tiles > 0)
        g.dense = s.pred_density * 64.0 * (double) plan.fast_motifs.size() / (double) n_row_tiles > kDenseHitsPerHalfTile;
    if (ov.pf_dense >= 0) g.dense = !g.wide && ov.pf_dense != 0;

    lds_layout(s, ov, g);
    launch_shape(s, ov, g);
    // long candidate lists: chunks of 4096 candidates in motif order with their windows carried along (fewer cache lines per read); short ones: list order, many small blocks
    g.rescore_carry = 1.5e-4 * (double) s.fast_windows >= ov.rescore_sorted_min;

    // the radix passes cover the key bits above kSortLowBits, sort_fixup_kernel the rest (MS_SORT_FULL: all bits by radix passes;
    // a short hit list is ordered by launch latencies, not passes: one kernel fewer matters more there).  With region coordinates
    // (pbits > 0) order_finalize_kernel sorts the runs below L = order_low_bits(n) bits instead, and writes the result arrays (L > 0).
    g.sort_begin_large = (g.end_bit > 2 * kSortLowBits && !ov.sort_full) ? kSortLowBits : 0;
    g.sort_low_bits = ov.sort_low_bits;
    g.order_run_cap = ov.order_run_cap;
    g.fixup_min = ov.fixup_min;
    return g;
}

static int order_low_bits(const ScanGeom &g, int32_t P, size_t n) {
    if (g.sort_low_bits >= 0) return std::min(g.sort_low_bits, g.gbits + 1);
    if (g.sort_begin_large == 0) return 0;
    // one radix pass fewer per eight bits, as long as the expected run n / (P x 2^(gbits + 1 - L)) stays short enough for the
    // rank sort in LDS (the motif bits stay above L: each run's first hit is then decided on any hit of the run before it)
    int L = 0;
    for (int b = kSortLowBits; b <= kOrderMaxLowBits && b <= g.gbits + 1; b += 8)
        if (b == kSortLowBits || std::ldexp((double) n / (double) std::max(P, 1), b - g.gbits - 1) <= kOrderMeanRun) L = b;
    return L;
}

int scan_sort_begin(const ScanGeom &g, int32_t P, size_t n_sort) {
    if (g.pbits > 0) return n_sort >= g.fixup_min || g.sort_low_bits >= 0 ? order_low_bits(g, P, n_sort) : 0;
    return n_sort >= g.fixup_min ? g.sort_begin_large : 0;
}

// ---- the bucketed hit list

// d0 of key = motif << (gbits + 1) | coord << 1 | strand is (coord >> c) & 255 with c = L - 1, as long as the digit stays inside the coordinate
// (L + 8 <= gbits + 1: bucket_layout_ok).  A region's positions fall into chunks of 2^c coordinates; a chunk [a, b) of a region of length
// len holds F(len - a) - F(len - b) window starts, F(x) = sum over the motif widths W of max(x - W + 1, 0).
void bucket_weights(const int64_t *offsets, int64_t R, const int32_t *widths, int32_t P, int gbits, int pbits, int L, BucketWeights *out) {
    for (auto &w : out->w) w = 0;
    out->total = 0;
    if (L < 1 || L + 8 > gbits + 1 || pbits < 1 || P < 1) return;
    const int c = L - 1;
    int max_w = 0;
    unsigned long long sum_w = 0;
    for (int32_t p = 0; p < P; p++) { max_w = std::max(max_w, (int) widths[p]); sum_w += (unsigned long long) widths[p]; }
    std::vector<unsigned long long> tab((size_t) max_w + 1, 0);        // F up to the widest motif; linear beyond it
    for (int32_t p = 0; p < P; p++)
        for (int x = std::max((int) widths[p], 1); x <= max_w; x++) tab[(size_t) x] += (unsigned long long) (x - widths[p] + 1);
    auto F = [&](int64_t x) -> unsigned long long {
        if (x <= 0) return 0;
        if (x <= max_w) return tab[(size_t) x];
        return (unsigned long long) P * (unsigned long long) (x + 1) - sum_w;
    };
    for (int64_t r = 0; r < R; r++) {
        const int64_t len = offsets[r + 1] - offsets[r];
        if (len <= 0) continue;
        const uint64_t c0 = (uint64_t) r << pbits;
        for (uint64_t u = c0 >> c; u <= (c0 + (uint64_t) len - 1) >> c; u++) {
            const int64_t a = (u << c) > c0 ? (int64_t) ((u << c) - c0) : 0;
            const int64_t b = std::min<int64_t>(len, (int64_t) (((u + 1) << c) - c0));
            const unsigned long long n = F(len - a) - F(len - b);
            out->w[u & 255u] += n;
            out->total += n;
        }
    }
}

unsigned long long bucket_need(const BucketWeights &bw, double mu) {
    unsigned long long need = 0;
    for (int b = 0; b < kOrderBuckets; b++) need += bucket_need_one(mu, bw.w[b], bw.total);
    return need;
}

void bucket_caps(const BucketWeights &bw, double mu, unsigned long long n_pred, unsigned long long cap_max, unsigned long long *base, unsigned long long *cap) {
    const unsigned long long need = bucket_need(bw, mu);
    const unsigned long long extra = n_pred > need ? n_pred - need : 0;
    unsigned long long at = 0;                      // the running sum of the uncut capacities
    for (int b = 0; b < kOrderBuckets; b++) {
        unsigned long long cb = bucket_need_one(mu, bw.w[b], bw.total);
        if (bw.w[b]) cb += (unsigned long long) std::floor((double) extra * (double) bw.w[b] / (double) bw.total);
        cb = std::min(cb, cap_max);
        base[b] = std::min(at, n_pred);
        cap[b] = std::min(cb, n_pred - base[b]);
        at += cb;
    }
}

bool bucket_layout_ok(const BucketShape &s) {
    // (the digit inside the coordinate: with a motif bit in it every bucket would hold one class of motifs, and motifs differ tenfold in how often they hit)
    if (!(s.pbits > 0 && s.L > 0 && s.L + 8 <= s.gbits + 1 && s.end_bit <= 63 && s.P > 0 && s.R > 0)) return false;
    // the largest key a hit can have (last motif, last region, any position), in the bits [L + 8, end_bit)
    const uint64_t top = ((((uint64_t) (s.P - 1) << s.gbits) | ((uint64_t) (s.R - 1) << s.pbits) | ((1ULL << s.pbits) - 1ULL)) << 1) >> (s.L + 8);
    return top != (1ULL << (s.end_bit - s.L - 8)) - 1ULL;
}

bool bucket_gate(const BucketShape &s, const ScanOverrides &ov, unsigned long long need, unsigned long long n_pred) {
    if (!s.predicted || s.counts_only || !s.carry_only || s.sticky_off || ov.order_buckets == 0 || !bucket_layout_ok(s)) return false;
    if (ov.order_buckets == 1) return true;
    // a full digit left for the passes above d0, and the needs inside the prediction
    return s.end_bit - (s.L + 8) >= 8 && need <= n_pred;
}

void scan_grow(size_t cand_cap, size_t hit_cap, unsigned long long n_cand, unsigned long long n_hits, size_t *want_cand, size_t *want_hits) {
    // (a truncated candidate list under-reports hits, so leave head room there)
    *want_cand = std::max<size_t>(cand_cap, (size_t) (n_cand + n_cand / 16 + 1024));
    const unsigned long long hit_need = n_cand > cand_cap ? std::max<unsigned long long>(n_hits, 2 * n_cand) : n_hits;
    *want_hits = std::max<size_t>(hit_cap, (size_t) (hit_need + hit_need / 16 + 1024));
}

}  // namespace ms
