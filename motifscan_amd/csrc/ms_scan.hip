// ms_scan.hip -- the scan pipeline: pre-filter -> fp64 re-score of the candidates (+ motifs the filter cannot take) -> order ->
// coordinates.  scan_locked is a driver over named stages (scan_plan, scan_front, scan_back, ...) that share one ScanCtx; what a scan
// decides before its first launch is ScanGeom (ms_scan_geom.cpp: host arithmetic on sizes).  Also the scans that are queued and
// finished later (PendingScan), and ms_scan.  (The window sweep and its hand-out: ms_sweep.hip.)
#include <algorithm>
#include <cmath>
#include <climits>
#include <cstring>
#include <memory>
#include <mutex>

#include "ms_handles.h"
#include "ms_scan_geom.h"

namespace ms {

constexpr int kScanDebugGeomWords = 16;          // ms_debug_scan_candidates' geom
constexpr int64_t kRescoreCarryChunk = 4096;     // records per chunk of rescore_carry_kernel (kRwChunk, ms_fp64.hip: a test compares the two)

static int scratch_reserve(Scratch &sc, size_t cand_cap, size_t hit_cap) {
    int rc;
    if (cand_cap > sc.cand_cap) {
        dev_free(sc.cand);
        sc.cand_cap = 0;
        if ((rc = dev_alloc(&sc.cand, cand_cap))) return rc;
        sc.cand_cap = cand_cap;
    }
    if (hit_cap > sc.hit_cap) {
        dev_free(sc.keys); dev_free(sc.vals); dev_free(sc.keys_sorted);
        sc.hit_cap = 0;
        if ((rc = dev_alloc(&sc.keys, hit_cap))) return rc;
        if ((rc = dev_alloc(&sc.vals, hit_cap))) return rc;
        if ((rc = dev_alloc(&sc.keys_sorted, hit_cap))) return rc;
        sc.hit_cap = hit_cap;
    }
    return MS_OK;
}

// ------------------------------------------------------------------- pending scans --

int pending_scan_init(PendingScan *p) {
    for (auto &e : p->ev) MS_HIP(hipEventCreate(&e));
    MS_HIP(hipEventCreateWithFlags(&p->done, hipEventDisableTiming));
    MS_HIP(hipHostMalloc(&p->h_counters, 8 * sizeof(unsigned long long)));
    return MS_OK;
}

PendingScan *pending_scan_acquire(DeviceCtx *c) {
    {
        std::lock_guard<std::mutex> lk(c->pend_mu);
        if (!c->pend_cache.empty()) { PendingScan *p = c->pend_cache.back(); c->pend_cache.pop_back(); return p; }
    }
    PendingScan *p = new (std::nothrow) PendingScan();
    if (!p) { set_error("out of host memory"); return nullptr; }
    if (pending_scan_init(p) != MS_OK) { pending_scan_destroy(p); delete p; return nullptr; }
    return p;
}

void pending_scan_release(DeviceCtx *c, PendingScan *p) {
    if (!p) return;
    if (p->raw) { ms_result_free(p->raw); p->raw = nullptr; }
    p->active = false;
    std::lock_guard<std::mutex> lk(c->pend_mu);
    if (c->pend_cache.size() < 8) { c->pend_cache.push_back(p); return; }
    pending_scan_destroy(p);
    delete p;
}

void pending_scan_destroy(PendingScan *p) {
    for (auto &e : p->ev) if (e) (void) hipEventDestroy(e);
    if (p->done) (void) hipEventDestroy(p->done);
    if (p->h_counters) (void) hipHostFree(p->h_counters);
    if (p->h_offsets) (void) hipHostFree(p->h_offsets);
    *p = PendingScan();
}

// stage times, counts and the next scan's prediction, once a scan's kernels are known to be done
static void finish_scan(ms_result *raw, hipEvent_t *ev, ms_pwmset *pwms, int64_t n_bases, int64_t R, const ScanKey &key,
                        unsigned long long n_cand, unsigned long long n_hits, bool with_back, unsigned long long n_overflow) {
    ms_scan_stats &stt = raw->stats;
    stt.order_overflow_runs = (int32_t) std::min<unsigned long long>(n_overflow, INT32_MAX);
    stt.n_candidates = (int64_t) n_cand;
    stt.n_hits = (int64_t) n_hits;
    raw->n_hits = (int64_t) n_hits;
    int64_t pwm_bytes = 0;
    for (int32_t p = 0; p < pwms->P; p++) pwm_bytes += 32LL * pwms->widths[p];
    // compulsory HBM bytes of one call
    stt.hbm_bytes_algorithmic = (n_bases + 3) / 4 + (n_bases + 7) / 8 + 8 * (R + 1) + pwm_bytes + 16 * (int64_t) n_hits + 8LL * pwms->P;
    float ms01 = 0, ms12 = 0, ms34 = 0, ms45 = 0, ms05 = 0;
    (void) hipEventElapsedTime(&ms01, ev[0], ev[1]);
    (void) hipEventElapsedTime(&ms12, ev[1], ev[2]);
    stt.ms_prefilter = ms01; stt.ms_exact = ms12; stt.ms_total = ms01 + ms12;
    if (with_back) {
        (void) hipEventElapsedTime(&ms34, ev[3], ev[4]);
        (void) hipEventElapsedTime(&ms45, ev[4], ev[5]);
        (void) hipEventElapsedTime(&ms05, ev[0], ev[5]);
        stt.ms_sort = ms34; stt.ms_finalize = ms45; stt.ms_total = ms05;
    }
    if (stt.n_windows > 0) {            // what the next scan of this set of PWMs may expect (scan_locked)
        pwms->pred_density = (double) n_hits / (double) stt.n_windows;
        pwms->pred_key = key;
    }
}

// The end of a scan whose sizes were predicted: did the scratch buffers and the predicted hit count hold?  A prediction that held
// narrows the margin of the next scans; one that failed doubles it, and the density is learnt again through the exactly-sized form.
// bucket_overflow: a hit of a bucketed list did not fit its bucket (counters[3]).  That is a failed prediction too -- of how the hits spread
// over the regions -- and such data (hits crowded into few regions) would fail again: the set's scans emit plain lists from then on.
static bool prediction_held(ms_pwmset *pwms, unsigned long long n_cand, size_t cand_cap, unsigned long long n_hits, size_t hit_cap, size_t n_pred,
                            bool bucket_overflow) {
    if (bucket_overflow) pwms->bucket_off = true;
    if (n_cand <= cand_cap && n_hits <= hit_cap && n_hits <= n_pred && !bucket_overflow) {
        pwms->pred_margin = std::max(0.04, pwms->pred_margin * 0.9);
        return true;
    }
    pwms->pred_margin = std::min(1.0, pwms->pred_margin * 2.0);
    pwms->pred_density = -1.0;
    return false;
}

int scan_complete(DeviceCtx *c, ms_pwmset *pwms, PendingScan *p, ms_result **out) {
    *out = nullptr;
    if (!p || !p->active) { set_error("no pending scan"); return MS_ERR_INVALID; }
    p->active = false;
    ms_result *raw = p->raw;
    p->raw = nullptr;
    hipError_t he = hipEventSynchronize(p->done);
    if (he != hipSuccess) { set_error("scan kernels failed: %s", hipGetErrorString(he)); ms_result_free(raw); return MS_ERR_RUNTIME; }
    const unsigned long long n_cand = p->cand_static + p->h_counters[0], n_hits = p->h_counters[1];
    (void) c;
    if (!prediction_held(pwms, n_cand, p->cand_cap, n_hits, p->hit_cap, p->n_pred, p->h_counters[3] != 0)) { ms_result_free(raw); return MS_SCAN_RETRY; }
    const size_t n_off = raw->motif_offsets.size();      // (copied in stream order, in front of `done`: pending_fill)
    std::memcpy(raw->motif_offsets.data(), p->h_offsets, n_off * sizeof(int64_t));
    try { raw->h_region_counts.assign(p->h_offsets + n_off, p->h_offsets + n_off + raw->P); } catch (const std::bad_alloc &) { raw->h_region_counts.clear(); }
    finish_scan(raw, p->ev, pwms, p->n_bases, p->R, ScanKey{p->strand_mask, pwms->cutoff_version, p->exact_only}, n_cand, n_hits, true, p->h_counters[2]);
    *out = raw;
    return MS_OK;
}

// ------------------------------------------------------------------ the scan's stages --

// What the stages of one scan share.  The caller of scan_locked holds c->mu (one scan at a time per device: shared scratch) and
// pwms->mu (lazily cached device copies / plan).
struct ScanCtx {
    DeviceCtx *c = nullptr;
    ms_pwmset *pwms = nullptr;
    const ms_seqset *seqs = nullptr;
    ms_result *raw = nullptr;
    int strand_mask = 3;
    uint32_t flags = 0;
    ScanKey key;
    ScanGeom g;
    hipEvent_t *ev = nullptr;            // stage events of this scan: the device's, or a pending scan's own set
    DevSeq S;
    DevPwm Pw;
    bool counts_ok = false;              // a counts-only scan whose set the bitmap form takes (scan_counts_fast)
    // the bucketed hit list (scan_bucket_decide): the fp64 stage emits in buckets of the digit at bk_L, the radix passes start at bk_L + 8
    bool bucketed = false;
    int bk_L = 0;
    double bk_mu = 0.0;                  // expected hits, and the sum of the buckets' needs at that expectation (bucket_need)
    unsigned long long bk_need = 0, bk_cap_max = ~0ULL;
    BucketWeights bk_w;                  // the sequence set's bucket weights for this key layout, L and these motif widths
    const ScanDebug *dbg = nullptr;      // a debug entry's stop / start point (ms_handles.h)
};

// The plan of this scan, with its device copies.  Which kernel family it runs (PrefilterPlan::wide) decides the LDS budget it is built
// with, so a set that may plan wide is planned under the wide budget first.
static int scan_plan(DeviceCtx *c, ms_pwmset *pwms, const ScanKey &key, const ScanOverrides &ov) {
    int rc;
    // only a motif of 32 ... kMaxFastWidth columns can make a wide tile; whether one does (it may fall to the all-fp64 path) the plan says.
    // The outcome is remembered per (strand, cutoffs, exact-only): a set whose wide motifs all left the pre-filter plans once, not twice per scan
    bool may_be_wide = false, wide = false;
    for (int32_t w : pwms->widths) may_be_wide = may_be_wide || (w >= 2 * kF6Cols && w <= kMaxFastWidth);
    if (may_be_wide && !key.exact_only && !(pwms->narrow_key == key)) {
        if ((rc = pwmset_plan(pwms, key.strand, scan_lds_budget(c->lds_max, true, ov), key.exact_only, false, c->device))) return rc;
        wide = pwms->plan.wide;
        if (!wide) pwms->narrow_key = key;
    }
    return pwmset_plan(pwms, key.strand, scan_lds_budget(c->lds_max, wide, ov), key.exact_only, true, c->device);
}

// the result handle, with the statistics that follow from the sizes alone; *fast_windows: the windows of the motifs on the pre-filter
static ms_result *scan_result_new(DeviceCtx *c, const ms_pwmset *pwms, const ms_seqset *seqs, int strand_mask, int64_t *fast_windows) {
    const PrefilterPlan &plan = pwms->plan;
    std::unique_ptr<ms_result> res(new (std::nothrow) ms_result());
    if (!res) { set_error("out of host memory"); return nullptr; }
    res->device = c->device;
    res->P = pwms->P;
    res->R = seqs->R;
    res->motif_offsets.assign((size_t) pwms->P + 1, 0);
    ms_scan_stats &stt = res->stats;
    std::memset(&stt, 0, sizeof(stt));
    stt.n_bases = seqs->n_bases;
    stt.n_pwms = pwms->P;
    stt.n_pwms_exact = (int32_t) plan.exact_motifs.size();
    stt.n_tiles = (int32_t) plan.tiles.size();
    int64_t cells = 0;                                                          // (window, column) pairs of one strand
    *fast_windows = 0;
    for (int32_t p = 0; p < pwms->P; p++) stt.n_windows += windows_for_width(seqs, pwms->widths[p]);
    for (int32_t p : plan.fast_motifs) {
        *fast_windows += windows_for_width(seqs, pwms->widths[p]);
        cells += windows_for_width(seqs, pwms->widths[p]) * pwms->widths[p];
    }
    const int64_t padded = ((seqs->n_bases + 63) / 64) * 64;
    stt.lds_bytes_read = plan.lds_bytes_per_position * padded / (plan.wide ? 1 : 2);      // (the double pass reads a row tile's operand once for 128 window starts)
    stt.pf_engine = 3;
    stt.mfma_ops_algorithmic = 2 * (strand_mask == 3 ? 2 : 1) * cells;           // one multiply-add per cell and strand
    stt.mfma_ops = padded / 32 * plan.kb_total * (2LL * 32 * 32 * 64);           // one 32x32x64 instruction per (32 windows, row tile, k-block)
    return res.release();
}

// nothing to scan: [] / [[]...]  (cscore.c:443-445)
static int scan_empty(ScanCtx &x) {
    int rc;
    if ((rc = result_block_alloc(x.c, x.raw, 0))) return rc;
    hipError_t he = hipMemsetAsync(x.raw->block, 0, 16 * ((size_t) x.pwms->P + 1), x.c->stream);       // counts and offsets: all zero
    if (he == hipSuccess) he = hipStreamSynchronize(x.c->stream);
    if (he != hipSuccess) { set_error("memset failed: %s", hipGetErrorString(he)); return MS_ERR_RUNTIME; }
    return MS_OK;
}

static HitOut scan_hit_out(const ScanCtx &x) {
    const Scratch &sc = x.c->sc;
    HitOut H;
    H.keys = sc.keys; H.vals = sc.vals; H.n_hits = sc.counters + 1; H.cap = sc.hit_cap; H.gbits = x.g.gbits; H.pbits = x.g.pbits;
    return H;
}

static BucketOut scan_bucket_out(const ScanCtx &x) {
    const Scratch &sc = x.c->sc;
    BucketOut B;
    B.base = sc.bucket_tab; B.cap = sc.bucket_tab + kOrderBuckets; B.fill = sc.bucket_tab + 2 * kOrderBuckets; B.overflow = sc.counters + 3;
    B.shift = x.bk_L;
    // the digit counts of the radix passes that are left, [bk_L + 8, end_bit): taken in the fp64 stage where they fit its LDS words
    const int places = (x.g.end_bit - (x.bk_L + 8) + 7) / 8;
    const bool counted = places >= 1 && places <= kBucketHistPlaces;
    B.hist = counted ? sc.bucket_tab + kBucketHistAt : nullptr;
    B.hist_places = counted ? places : 0;
    return B;
}

// "fetch the eight counters and wait": counters [0] candidate record slots, [1] hits, [2] runs ordered by order_overflow_kernel
static int fetch_counters(DeviceCtx *c, const char *what) {
    hipError_t he = hipMemcpyAsync(c->sc.h_counters, c->sc.counters, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream);
    if (he == hipSuccess) he = hipStreamSynchronize(c->stream);
    if (he != hipSuccess) { set_error("%s failed: %s", what, hipGetErrorString(he)); return MS_ERR_RUNTIME; }
    return MS_OK;
}

// the pre-filter's launch, in the geometry ScanGeom holds
static int scan_prefilter(ScanCtx &x) {
    DeviceCtx *c = x.c;
    Scratch &sc = c->sc;
    const ScanGeom &g = x.g;
    int rc;
    PfArgs A;
    A.codes = x.S.codes; A.nmask = x.S.nmask; A.n_bases = x.S.n_bases; A.skip_alln = x.pwms->plan.alln_can_hit ? 0 : 1;
    A.tables = x.pwms->d_tables; A.tiles = x.pwms->d_tiles;
    A.lut_off16 = g.lut_off16; A.stage_off16 = g.stage_off16; A.emit_off16 = g.emit_off16; A.onehot_off16 = g.onehot_off16; A.rare_off16 = g.rare_off16;
    A.rare_cap = g.rare_cap;
    A.cand = sc.cand; A.n_cand = sc.counters; A.cand_cap = sc.cand_cap; A.cand_block = g.cand_block; A.cand_static = g.cand_static;
    const size_t counter_words = (size_t) g.n_tiles * kPfCounters * 16;            // kPfCounters words per tile, 64 bytes apart
    if (counter_words > sc.chunk_counters_cap) {
        dev_free(sc.chunk_counters);
        sc.chunk_counters_cap = 0;
        if ((rc = dev_alloc(&sc.chunk_counters, counter_words + 16))) return rc;
        sc.chunk_counters_cap = counter_words + 16;
    }
    A.chunk_counter = sc.chunk_counters;
    A.wave_passes = g.wave_passes;
    A.use_counters = g.counter_used ? 1 : 0;
    if (g.counter_used) {
        hipError_t he = hipMemsetAsync(A.chunk_counter, 0, sizeof(unsigned int) * counter_words, c->stream);
        if (he != hipSuccess) { set_error("memset failed: %s", hipGetErrorString(he)); return MS_ERR_RUNTIME; }
    }
    const int li = g.wide ? 2 : g.dense ? 1 : 0;
    if (g.lds_bytes > c->lds_set[li]) {
        if ((rc = prefilter_set_lds(g.wide, g.dense, g.lds_bytes))) return rc;
        c->lds_set[li] = g.lds_bytes;
    }
    return launch_prefilter(A, g.wide, g.dense, g.bpt, g.n_tiles, g.lds_bytes, c->stream);
}

// ms_debug_scan_from_candidates: the caller's record slots in place of the pre-filter's launch.  Empty records fill the list up to the
// waves' own first blocks, and counters[0] says that the fp64 stage sees exactly the given slots.  A list longer than the scratch is cut
// where the pre-filter's own stores would be cut: scan_exact reads the full count, grows the scratch and runs the pass again.
static int scan_upload_candidates(ScanCtx &x) {
    DeviceCtx *c = x.c;
    Scratch &sc = c->sc;
    const ScanDebug &d = *x.dbg;
    const uint64_t n_static = std::min<uint64_t>(x.g.cand_static, sc.cand_cap), n_copy = std::min<uint64_t>(d.n, sc.cand_cap);
    hipError_t he = hipSuccess;
    if (n_copy) he = hipMemcpyAsync(sc.cand, d.records, n_copy * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream);
    if (he == hipSuccess && n_copy < n_static) he = hipMemsetAsync(sc.cand + n_copy, 0, (n_static - n_copy) * sizeof(uint64_t), c->stream);
    sc.h_counters[0] = d.n > x.g.cand_static ? d.n - x.g.cand_static : 0ULL;        // (pinned, and next written by fetch_counters behind this copy)
    if (he == hipSuccess) he = hipMemcpyAsync(sc.counters, sc.h_counters, sizeof(unsigned long long), hipMemcpyHostToDevice, c->stream);
    if (he != hipSuccess) { set_error("candidate upload failed: %s", hipGetErrorString(he)); return MS_ERR_RUNTIME; }
    return MS_OK;
}

// pre-filter + fp64 stage of one pass, queued on the scan stream (events 0, 1, 2 around the two stages)
static int scan_front(ScanCtx &x, const HitOut &H, const BucketOut *B = nullptr) {
    DeviceCtx *c = x.c;
    Scratch &sc = c->sc;
    const PrefilterPlan &plan = x.pwms->plan;
    int rc;
    hipError_t he = hipMemsetAsync(sc.counters, 0, 8 * sizeof(unsigned long long), c->stream);
    if (he != hipSuccess) { set_error("memset failed: %s", hipGetErrorString(he)); return MS_ERR_RUNTIME; }
    (void) hipEventRecord(x.ev[0], c->stream);
    const bool given = x.dbg && !x.dbg->stop;         // the candidate list comes from the caller
    if (x.g.n_tiles > 0 && (rc = given ? scan_upload_candidates(x) : scan_prefilter(x))) return rc;
    (void) hipEventRecord(x.ev[1], c->stream);
    if (x.dbg && x.dbg->stop) {                       // ms_debug_scan_candidates: the list is all that is wanted
        (void) hipEventRecord(x.ev[2], c->stream);
        return MS_OK;
    }
    if (!plan.fast_motifs.empty()) {                 // (few blocks for a small scan measured slower: the kernel is a chain of dependent gathers and wants every record in flight at once)
        if (x.g.rescore_carry) {
            if (!c->rc_lds_set) { if ((rc = rescore_carry_set_lds())) return rc; c->rc_lds_set = true; }
            if (B) rc = launch_rescore_carry_bucketed(x.S, x.Pw, sc.cand, sc.counters, x.g.cand_static, sc.cand_cap, x.pwms->d_field_meta, x.strand_mask, H, *B, c->n_cu, c->stream);
            else rc = launch_rescore_carry(x.S, x.Pw, sc.cand, sc.counters, x.g.cand_static, sc.cand_cap, x.pwms->d_field_meta, x.strand_mask, H, c->n_cu, c->stream);
            if (rc) return rc;
        } else if ((rc = launch_rescore(x.S, x.Pw, sc.cand, sc.counters, x.g.cand_static, sc.cand_cap, x.pwms->d_field_meta, x.strand_mask, H, c->n_cu * 8, c->stream))) return rc;
    }
    if (!plan.exact_motifs.empty()) {
        int max_w = 0;
        for (int32_t m : plan.exact_motifs) max_w = std::max(max_w, (int) x.pwms->widths[m]);
        if ((rc = launch_exact_all(x.S, x.Pw, x.pwms->d_exact_motifs, (int32_t) plan.exact_motifs.size(), x.strand_mask, H, c->stream, max_w))) return rc;
    }
    (void) hipEventRecord(x.ev[2], c->stream);
    return MS_OK;
}

// counts only: the flag map costs ~2 x P x R bytes of traffic (clear + count), the ordering it replaces ~200 bytes per hit -- so the map is
// taken where the set holds at least one hit per ~50 (motif, region) cells (configs[3]: one per 9; a million 50-bp regions: one per 100,
// where the sort is the cheaper way to the same counts).  Decided before the result block is sized (a second, exactly-sized run after a
// failed prediction decides again).
static bool scan_counts_fast(const ScanCtx &x, size_t n_expected) {
    return x.counts_ok && (double) x.pwms->P * (double) x.seqs->R <= (double) kCountsGateRatio * (double) std::max<size_t>(n_expected, 1);
}

// the complete per-motif offsets are on the device; one copy brings them to the host.  (Not for a scan that is only being
// QUEUED: the destination is pageable memory, for which the "async" copy makes the host wait for everything queued before
// it -- scan_complete fetches the offsets once the scan is done.)
static int fetch_offsets(ScanCtx &x, bool queue_only) {
    if (queue_only) return MS_OK;
    ms_result *raw = x.raw;
    hipError_t he = hipMemcpyAsync(raw->motif_offsets.data(), raw->d_motif_first, raw->motif_offsets.size() * sizeof(int64_t), hipMemcpyDeviceToHost, x.c->stream);
    if (he != hipSuccess) { set_error("copy failed: %s", hipGetErrorString(he)); return MS_ERR_RUNTIME; }
    return MS_OK;
}

// the counts-only form of scan_back: the hits are counted where the fp64 stage left them (events 4, 5 with nothing between them)
static int back_count_only(ScanCtx &x, size_t n_sort, const unsigned long long *n_dev, bool queue_only) {
    DeviceCtx *c = x.c;
    ms_result *raw = x.raw;
    const int32_t P = x.pwms->P;
    int rc;
    // the bitmap + the per-motif site counters in one pooled block the result owns (a queued scan's kernels outlive this call)
    const size_t words = count_only_bitmap_words(P, x.seqs->R);
    if ((rc = pool_alloc(c, words * 4 + 256 + 8 * (size_t) P, &raw->coord_blk, &raw->coord_bytes))) return rc;
    uint32_t *bitmap = static_cast<uint32_t *>(raw->coord_blk);
    unsigned long long *motif_hits = reinterpret_cast<unsigned long long *>(static_cast<char *>(raw->coord_blk) + ((words * 4 + 255) & ~(size_t) 255));
    if ((rc = launch_count_only(c->sc.keys, (int64_t) n_sort, n_dev, x.g.gbits, x.g.pbits, x.seqs->R, P, bitmap, raw->d_region_counts, motif_hits, raw->d_motif_first, c->stream))) return rc;
    raw->counts_only = true;
    (void) hipEventRecord(x.ev[4], c->stream);
    (void) hipEventRecord(x.ev[5], c->stream);
    return fetch_offsets(x, queue_only);
}

// the radix passes over the key bits [sort_begin, end_bit) of the first n_sort slots, and the fix-up behind them for global-position keys
// (a bucketed list: sort_begin = L + 8, the digit at L is in order as the list stands)
static int back_sort(ScanCtx &x, size_t n_sort, const unsigned long long *n_dev, int sort_begin, size_t ovf_bytes) {
    DeviceCtx *c = x.c;
    Scratch &sc = c->sc;
    int rc;
    size_t need = 0;
    if ((rc = sort_hit_pairs(nullptr, &need, sc.keys, sc.keys_sorted, sc.vals, x.raw->d_score, n_sort, sort_begin, x.g.end_bit, c->stream))) return rc;
    // a bucketed list comes with its digit counts (BucketOut::hist): the passes then run without rocPRIM's histogram pass over the list
    const unsigned long long *counts = x.bucketed && sort_begin == x.bk_L + 8 ? scan_bucket_out(x).hist : nullptr;
    if (counts) {
        size_t need_counted = 0;
        bool can = false;
        if ((rc = sort_hit_pairs_counted(nullptr, &need_counted, sc.keys, sc.keys_sorted, sc.vals, x.raw->d_score, n_sort, sort_begin, x.g.end_bit, nullptr,
                                         &can, c->stream))) return rc;
        if (can) need = std::max(need, need_counted);
        else counts = nullptr;
    }
    need = std::max(need, ovf_bytes);             // (the radix temp storage is free once the passes are done: order_finalize_kernel's overflow list goes there)
    if (need > sc.sort_tmp_bytes) {
        if (sc.sort_tmp) (void) hipFree(sc.sort_tmp);
        sc.sort_tmp = nullptr; sc.sort_tmp_bytes = 0;
        unsigned char *tmp = nullptr;
        if ((rc = dev_alloc(&tmp, need))) return rc;
        sc.sort_tmp = tmp;
        sc.sort_tmp_bytes = need;
    }
    size_t have = sc.sort_tmp_bytes;
    bool done = false;
    if (counts && (rc = sort_hit_pairs_counted(sc.sort_tmp, &have, sc.keys, sc.keys_sorted, sc.vals, x.raw->d_score, n_sort, sort_begin, x.g.end_bit, counts,
                                               &done, c->stream))) return rc;
    if (!done && (rc = sort_hit_pairs(sc.sort_tmp, &have, sc.keys, sc.keys_sorted, sc.vals, x.raw->d_score, n_sort, sort_begin, x.g.end_bit, c->stream))) return rc;
    if (x.g.pbits == 0 && sort_begin) return launch_sort_fixup(sc.keys_sorted, x.raw->d_score, (int64_t) n_sort, n_dev, c->stream);
    return MS_OK;
}

// the compact coordinate words of MS_SCAN_PACK_INTERNAL / MS_SCAN_PACK12_INTERNAL, in a pooled block the result owns
static int back_pack_coords(ScanCtx &x, size_t n_sort, const unsigned long long *n_dev) {
    DeviceCtx *c = x.c;
    ms_result *raw = x.raw;
    int rc;
    const size_t n_round = (n_sort + 65535) & ~(size_t) 65535;
    if ((rc = pool_alloc(c, 8 * n_round + 256, &raw->coord_blk, &raw->coord_bytes))) return rc;
    raw->d_coord = static_cast<uint64_t *>(raw->coord_blk);
    raw->d_coord_bad = reinterpret_cast<unsigned int *>(raw->d_coord + n_round);
    hipError_t he = hipMemsetAsync(raw->d_coord_bad, 0, sizeof(unsigned int), c->stream);
    if (he != hipSuccess) { set_error("memset failed: %s", hipGetErrorString(he)); return MS_ERR_RUNTIME; }
    // the 4-byte form when asked for and the set's largest region index and position fit 31 bits beside the strand bit
    raw->coord_shift = (x.flags & MS_SCAN_PACK12_INTERNAL) ? x.g.coord_shift12 : 0;
    return launch_pack_hits((int64_t) n_sort, n_dev, raw->d_seq_idx, raw->d_pos, raw->d_strand, raw->d_coord, raw->d_coord_bad, c->stream, raw->coord_shift);
}

// ordering + coordinates of the first n_sort slots of the hit list into the result block (events 3, 4, 5); n_dev != nullptr:
// only the device knows how many of them are hits (the rest are all-ones keys, which sort behind every hit).  queue_only: this
// back belongs to a scan that is only queued (scan_complete finishes it).
static int scan_back(ScanCtx &x, size_t n_sort, const unsigned long long *n_dev, bool counts_fast, bool queue_only) {
    DeviceCtx *c = x.c;
    Scratch &sc = c->sc;
    ms_result *raw = x.raw;
    const ScanGeom &g = x.g;
    const int32_t P = x.pwms->P;
    int rc;
    hipError_t he = hipMemsetAsync(raw->d_region_counts, 0, 8 * ((size_t) P + 1), c->stream);
    if (he != hipSuccess) { set_error("memset failed: %s", hipGetErrorString(he)); return MS_ERR_RUNTIME; }
    (void) hipEventRecord(x.ev[3], c->stream);
    raw->counts_only = false;
    if (counts_fast) return back_count_only(x, n_sort, n_dev, queue_only);
    const int sort_begin = scan_sort_begin(g, P, n_sort);
    const size_t ovf_bytes = g.pbits > 0 && sort_begin > 0 ? order_overflow_bytes(n_sort, g.order_run_cap) : 0;
    if (n_sort > 0 && (rc = back_sort(x, n_sort, n_dev, x.bucketed ? sort_begin + 8 : sort_begin, ovf_bytes))) return rc;
    (void) hipEventRecord(x.ev[4], c->stream);
    if (g.pbits > 0 && sort_begin > 0) {
        // counters[2]: the runs order_finalize_kernel leaves to its overflow launch (zeroed with the others in front of the pre-filter).
        // (A list sorted over every bit -- a short one: launch latencies, not bytes -- keeps the lighter finalize_rp_kernel.)
        if ((rc = launch_order_finalize(sc.keys_sorted, raw->d_score, (int64_t) n_sort, n_dev, sort_begin, g.rbits, g.pbits, P, raw->d_seq_idx,
                                        raw->d_pos, raw->d_strand, raw->d_motif_first, raw->d_region_counts, sc.keys, sc.vals, sc.sort_tmp,
                                        ovf_bytes, sc.counters + 2, g.order_run_cap, c->stream))) return rc;
    } else if ((rc = launch_finalize(sc.keys_sorted, (int64_t) n_sort, n_dev, g.gbits, g.rbits, g.pbits, P, x.S, raw->d_seq_idx, raw->d_pos,
                                     raw->d_strand, raw->d_motif_first, raw->d_region_counts, c->stream))) return rc;
    if ((x.flags & (MS_SCAN_PACK_INTERNAL | MS_SCAN_PACK12_INTERNAL)) && n_sort > 0 && (rc = back_pack_coords(x, n_sort, n_dev))) return rc;
    (void) hipEventRecord(x.ev[5], c->stream);
    return fetch_offsets(x, queue_only);
}

// Whether this predicted-size scan emits its hits in buckets (bucket_gate, ms_scan_geom.h), with what it takes: the set's bucket weights for this
// key layout and L (made once per sequence set, on the host, from its offsets), and the sum of the buckets' needs.  Forced on by a test
// (MS_ORDER_BUCKETS=1), *n_pred grows to that sum: a short list's 6-sigma slacks do not fit a few per cent of it.
static void scan_bucket_decide(ScanCtx &x, const ScanOverrides &ov, double mu, size_t *n_pred) {
    const PrefilterPlan &plan = x.pwms->plan;
    ms_seqset *seqs = const_cast<ms_seqset *>(x.seqs);           // (the cached weights; the caller holds the device's lock)
    BucketShape bs;
    bs.predicted = true;
    bs.counts_only = x.counts_ok;                                // (any counts-only scan: whether it takes the bitmap form is decided on the final n_pred)
    bs.carry_only = x.g.rescore_carry && x.g.n_tiles > 0 && !plan.fast_motifs.empty() && plan.exact_motifs.empty();
    bs.sticky_off = x.pwms->bucket_off;
    bs.pbits = x.g.pbits; bs.gbits = x.g.gbits; bs.end_bit = x.g.end_bit; bs.P = x.pwms->P; bs.R = x.seqs->R;
    bs.L = scan_sort_begin(x.g, x.pwms->P, *n_pred);
    if (!bucket_gate(bs, ov, 0, *n_pred) || seqs->offsets.size() != (size_t) seqs->R + 1) return;      // (need 0: everything but the size, before the weights are looked at)
    uint64_t wh = 1469598103934665603ULL;                         // FNV-1a of the widths
    for (int32_t w : x.pwms->widths) wh = (wh ^ (uint64_t) (uint32_t) w) * 1099511628211ULL;
    auto &cache = seqs->bk_weights;
    size_t at = 0;
    while (at < cache.size() && !(cache[at].L == bs.L && cache[at].gbits == bs.gbits && cache[at].pbits == bs.pbits && cache[at].widths == wh)) at++;
    try {
        if (at == cache.size()) {
            if (cache.size() >= 4) cache.pop_back();
            cache.insert(cache.begin(), ms_seqset::BkWeights{bs.gbits, bs.pbits, bs.L, wh, {}});
            bucket_weights(seqs->offsets.data(), seqs->R, x.pwms->widths.data(), x.pwms->P, bs.gbits, bs.pbits, bs.L, &cache[0].w);
        } else if (at > 0) std::rotate(cache.begin(), cache.begin() + at, cache.begin() + at + 1);
    } catch (const std::bad_alloc &) { return; }
    x.bk_w = cache[0].w;
    if (x.bk_w.total == 0) return;
    const unsigned long long need = bucket_need(x.bk_w, mu);
    if (!bucket_gate(bs, ov, need, *n_pred)) return;
    if (need > *n_pred) {                                        // forced
        if (need > 3000000000ULL || scan_sort_begin(x.g, x.pwms->P, (size_t) need) != bs.L) return;
        *n_pred = (size_t) need;
    }
    x.bucketed = true;
    x.bk_L = bs.L; x.bk_mu = mu; x.bk_need = need; x.bk_cap_max = ov.bucket_cap_max;
}

// Every launch of a scan whose sizes are PREDICTED, queued at once: the result block, the sort and the coordinate kernel are sized
// for n_pred hits (the fp64 stage's real count stays on the device: the unused slots are filled with all-ones keys that sort last,
// finalize reads the count there).
static int scan_queue_predicted(ScanCtx &x, size_t n_pred, bool queue_only) {
    Scratch &sc = x.c->sc;
    int rc;
    if ((rc = scratch_reserve(sc, x.g.want_cand, std::max(x.g.want_hits, n_pred)))) return rc;
    const bool counts_fast = scan_counts_fast(x, n_pred);
    if ((rc = result_block_alloc(x.c, x.raw, counts_fast ? 1 : n_pred))) return rc;
    x.raw->stats.n_passes = 1;
    x.raw->stats.order_bucketed = x.bucketed ? 1 : 0;
    if (x.bucketed) {
        // the buckets' places for this scan, then the front with the bucketed fp64 stage; the tail fill also makes counters[1] out of the fills
        const BucketOut B = scan_bucket_out(x);
        if ((rc = launch_bucket_plan(x.bk_w, x.bk_mu, n_pred, x.bk_need, x.bk_cap_max, sc.bucket_tab, x.c->stream))) return rc;
        if ((rc = scan_front(x, scan_hit_out(x), &B))) return rc;
        if ((rc = launch_fill_tail_buckets(sc.keys, sc.bucket_tab, n_pred, sc.counters + 1, sc.counters + 3, B.hist, B.hist_places,
                                           x.g.end_bit - (x.bk_L + 8) - 8 * (B.hist_places - 1), x.c->stream))) return rc;
    } else {
        if ((rc = scan_front(x, scan_hit_out(x)))) return rc;
        if ((rc = launch_fill_tail(sc.keys, sc.counters + 1, n_pred, x.c->stream))) return rc;
    }
    return scan_back(x, n_pred, sc.counters + 1, counts_fast, queue_only);
}

// A predicted scan that is queued, not waited for: the owner queues its next scan behind this one first (everything is in order on one
// stream: the next scan's kernels only touch the shared scratch after this scan's are done; a scratch buffer that has to grow
// is freed by hipFree, which waits for the device).  What scan_complete needs goes into the slot.
static int pending_fill(ScanCtx &x, PendingScan *pend, size_t n_pred) {
    DeviceCtx *c = x.c;
    const Scratch &sc = c->sc;
    ms_result *raw = x.raw;
    // the per-motif offsets too, in stream order, into the slot's own pinned words: scan_complete used to fetch them with a blocking hipMemcpy
    // into pageable memory once the scan was done -- one more synchronous driver call per batch on the scan stage's thread (same pass time
    // either way, profiles/r06z_offsets_ab.log; kept because nothing on that thread should block that need not).  The per-motif region counts
    // ride along: the stream's copy-out stage brings them to the host with every batch, and its own small copy is one more blit kernel that
    // has to find a CU beside the running pre-filter
    const size_t n_off = raw->motif_offsets.size(), n_words = n_off + (size_t) x.pwms->P;
    hipError_t he;
    if (pend->h_offsets_cap < n_words) {
        if (pend->h_offsets) (void) hipHostFree(pend->h_offsets);
        pend->h_offsets = nullptr; pend->h_offsets_cap = 0;
        he = hipHostMalloc(&pend->h_offsets, (n_words + 64) * sizeof(int64_t));
        if (he != hipSuccess) { set_error("out of pinned host memory"); return MS_ERR_NOMEM; }
        pend->h_offsets_cap = n_words + 64;
    }
    he = hipMemcpyAsync(pend->h_offsets, raw->d_motif_first, n_off * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream);
    if (he == hipSuccess && x.pwms->P > 0)
        he = hipMemcpyAsync(pend->h_offsets + n_off, raw->d_region_counts, (size_t) x.pwms->P * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream);
    if (he == hipSuccess) he = hipMemcpyAsync(pend->h_counters, sc.counters, 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream);
    if (he == hipSuccess) he = hipEventRecord(pend->done, c->stream);
    if (he != hipSuccess) { set_error("scan kernels failed: %s", hipGetErrorString(he)); return MS_ERR_RUNTIME; }
    pend->cand_cap = sc.cand_cap;
    pend->hit_cap = sc.hit_cap;
    pend->active = true;
    pend->raw = raw;
    pend->n_pred = n_pred;
    pend->cand_static = x.g.cand_static;
    pend->n_bases = x.seqs->n_bases;
    pend->R = x.seqs->R;
    pend->strand_mask = x.strand_mask;
    pend->exact_only = x.key.exact_only;
    return MS_OK;
}

// ms_debug_scan_candidates: the candidate list as the pre-filter left it, and the geometry it was launched in
static int scan_candidates_out(ScanCtx &x, unsigned long long n_cand) {
    DeviceCtx *c = x.c;
    const Scratch &sc = c->sc;
    const ScanDebug &d = *x.dbg;
    const ScanGeom &g = x.g;
    const uint64_t n_slots = x.g.n_tiles > 0 ? std::min<uint64_t>(n_cand, sc.cand_cap) : 0, n_copy = d.out ? std::min<uint64_t>(n_slots, d.cap) : 0;
    *d.n_slots = n_slots;
    if (n_copy) {
        hipError_t he = hipMemcpyAsync(d.out, sc.cand, n_copy * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream);
        if (he == hipSuccess) he = hipStreamSynchronize(c->stream);
        if (he != hipSuccess) { set_error("candidate copy failed: %s", hipGetErrorString(he)); return MS_ERR_RUNTIME; }
    }
    const int64_t geom[kScanDebugGeomWords] = {g.wide, g.dense, g.counter_used, g.wave_passes, g.bpt, g.n_tiles, (int64_t) g.rare_cap, (int64_t) g.cand_block,
                                               (int64_t) g.cand_static, x.pwms->plan.alln_can_hit ? 0 : 1, g.wide ? 64 : 128, kRescoreCarryChunk};
    std::memcpy(d.geom, geom, sizeof(geom));
    return MS_OK;
}

// The exactly-sized form: the front runs (again, with larger buffers, while one overflows), the host reads the counts, and the result
// block, the sort and the coordinate kernel are sized by them.
static int scan_exact(ScanCtx &x, size_t want_cand, size_t want_hits) {
    DeviceCtx *c = x.c;
    Scratch &sc = c->sc;
    ms_result *raw = x.raw;
    int rc;
    unsigned long long n_cand = 0, n_hits = 0;
    for (int pass = 1;; pass++) {
        if ((rc = scratch_reserve(sc, want_cand, want_hits))) return rc;
        raw->stats.n_passes += 1;
        if ((rc = scan_front(x, scan_hit_out(x)))) return rc;
        if ((rc = fetch_counters(c, "scan kernels"))) return rc;
        n_cand = x.g.cand_static + sc.h_counters[0];
        n_hits = sc.h_counters[1];
        if (n_cand <= sc.cand_cap && n_hits <= sc.hit_cap) break;
        if (pass >= 8) { set_error("scan buffers kept overflowing (%llu candidates, %llu hits)", n_cand, n_hits); return MS_ERR_RUNTIME; }
        scan_grow(sc.cand_cap, sc.hit_cap, n_cand, n_hits, &want_cand, &want_hits);       // ... and run the pass again
    }
    if (x.dbg && x.dbg->stop) return scan_candidates_out(x, n_cand);
    if (x.flags & MS_SCAN_RAW_INTERNAL) {                      // the caller takes the unordered hits from the scratch
        finish_scan(raw, x.ev, x.pwms, x.seqs->n_bases, x.seqs->R, x.key, n_cand, n_hits, false, 0);
        raw->raw_gbits = x.g.gbits;
        raw->raw_pbits = x.g.pbits;
        return MS_OK;
    }
    // one pooled block for everything the result owns
    const bool counts_fast = scan_counts_fast(x, (size_t) n_hits);
    if ((rc = result_block_alloc(c, raw, counts_fast ? 1 : (size_t) n_hits))) return rc;
    if ((rc = scan_back(x, (size_t) n_hits, nullptr, counts_fast, false))) return rc;
    if ((rc = fetch_counters(c, "finalize"))) return rc;
    finish_scan(raw, x.ev, x.pwms, x.seqs->n_bases, x.seqs->R, x.key, n_cand, n_hits, true, sc.h_counters[2]);
    return MS_OK;
}

// The scan pipeline.  Three forms:
//   predicted, synchronous -- sizes PREDICTED from the previous scan of these PWMs.  The hit density of a motif set at its cutoffs is a
//       property of the set (p-value x windows x strands): consecutive scans -- the batches of a stream, the input and control sets of
//       a run, a benchmark's steps -- repeat it within a fraction of a percent.  Everything is sized for the predicted count plus a
//       margin, every launch is queued at once (scan_queue_predicted), and ONE synchronisation at the very end validates the
//       prediction.  A wrong prediction (count above the margin, or a scratch buffer too small) costs a second, exactly-sized run
//       and doubles the margin of the next scans.
//   predicted, queued (pend != nullptr) -- the same launches, not waited for: MS_SCAN_PENDING, scan_complete validates.
//   exactly sized (scan_exact) -- no prediction for this key yet, the caller forbids one, or the prediction just failed.  It always runs
//       to the end, with or without a PendingScan slot (the first batch of a stream, whose PWM set has no prediction yet, came back
//       with all-zero offsets when it did not).
int scan_locked(DeviceCtx *c, ms_pwmset *pwms, const ms_seqset *seqs, int strand_mask, uint32_t flags, ms_result **out, PendingScan *pend,
                const ScanDebug *dbg) {
    int rc;
    const ScanOverrides ov = read_scan_overrides();
    ScanCtx x;
    x.c = c; x.pwms = pwms; x.seqs = seqs; x.strand_mask = strand_mask; x.flags = flags; x.ev = c->ev; x.dbg = dbg;
    if ((rc = seqset_pack_pending(seqs, c->stream))) return rc;       // a batch stream's set: its pack / hint kernels run here, in front of its pre-filter
    if ((rc = pwmset_upload(pwms, c->device, c->stream))) return rc;
    x.key = ScanKey{strand_mask, pwms->cutoff_version, (flags & MS_SCAN_EXACT_ONLY) != 0};
    if ((rc = scan_plan(c, pwms, x.key, ov))) return rc;

    ScanShape sh;
    std::unique_ptr<ms_result, void (*)(ms_result *)> res(scan_result_new(c, pwms, seqs, strand_mask, &sh.fast_windows), ms_result_free);
    if (!res) return MS_ERR_NOMEM;
    x.raw = res.get();
    if (dbg && dbg->stop) { *dbg->n_slots = 0; std::memset(dbg->geom, 0, kScanDebugGeomWords * sizeof(int64_t)); }
    if (dbg && !dbg->stop) {
        // the kernels behind the list trust a record as they trust the pre-filter: a flagged one must name a base and a table group of this scan
        const uint64_t n_groups = pwms->plan.group_kb.size();
        for (uint64_t i = 0; i < dbg->n; i++) {
            const uint64_t rec = dbg->records[i];
            if ((rec & 0xFFFFu) && ((int64_t) (rec >> 30) >= seqs->n_bases || ((rec >> 16) & 0x3FFFu) >= n_groups)) {
                set_error("record %llu names base %llu, table group %llu (the set has %lld bases, the plan %llu groups)", (unsigned long long) i,
                          (unsigned long long) (rec >> 30), (unsigned long long) ((rec >> 16) & 0x3FFFu), (long long) seqs->n_bases, (unsigned long long) n_groups);
                return MS_ERR_INVALID;
            }
        }
    }
    if (pwms->P == 0 || seqs->n_bases == 0) {
        if (dbg && dbg->stop) { *out = nullptr; return MS_OK; }
        if ((rc = scan_empty(x))) return rc;
        *out = res.release();
        return MS_OK;
    }

    // what the previous scan of this set at these cutoffs and strands found, per (motif, window), if there was one
    const bool density_known = pwms->pred_density >= 0 && pwms->pred_key == x.key;
    sh.plan = &pwms->plan; sh.P = pwms->P;
    sh.n_bases = seqs->n_bases; sh.R = seqs->R; sh.max_len = seqs->len_sorted.empty() ? 0 : seqs->len_sorted.back();
    sh.n_cu = c->n_cu; sh.lds_max = c->lds_max; sh.cu_reserved = c->n_streams.load() > 0 ? c->n_cu_copy : 0;
    sh.density_known = density_known; sh.pred_density = pwms->pred_density;
    x.g = scan_geometry(sh, ov);
    x.S = dev_seq(seqs);
    x.Pw = dev_pwm(pwms);
    x.counts_ok = (flags & MS_SCAN_COUNTS_ONLY_INTERNAL) && !(flags & MS_SCAN_RAW_INTERNAL) && count_only_supported(pwms->P, seqs->R, x.g.pbits);
    ms_scan_stats &stt = x.raw->stats;
    if (x.g.n_tiles > 0 && x.g.dense) stt.pf_engine = 4;

    Scratch &sc = c->sc;
    size_t want_cand = x.g.want_cand, want_hits = x.g.want_hits;
    if (density_known && !(flags & (MS_SCAN_RAW_INTERNAL | MS_SCAN_NO_PREDICT_INTERNAL)) && !ov.no_predict && !dbg) {
        if (pend) x.ev = pend->ev;
        const double mu = pwms->pred_density * (double) stt.n_windows;
        size_t n_pred = (size_t) std::min<double>(mu * (1.0 + pwms->pred_margin) + 6.0 * std::sqrt(mu + 1.0) + 256.0, 3.0e9);
        scan_bucket_decide(x, ov, mu, &n_pred);
        if ((rc = scan_queue_predicted(x, n_pred, pend != nullptr))) return rc;
        if (pend) {
            if ((rc = pending_fill(x, pend, n_pred))) return rc;
            res.release();                           // (the slot owns the result now)
            *out = nullptr;
            return MS_SCAN_PENDING;
        }
        if ((rc = fetch_counters(c, "scan kernels"))) return rc;
        const unsigned long long n_cand = x.g.cand_static + sc.h_counters[0], n_hits = sc.h_counters[1];
        if (prediction_held(pwms, n_cand, sc.cand_cap, n_hits, sc.hit_cap, n_pred, sc.h_counters[3] != 0)) {
            finish_scan(x.raw, x.ev, pwms, seqs->n_bases, seqs->R, x.key, n_cand, n_hits, true, sc.h_counters[2]);
            *out = res.release();
            return MS_OK;
        }
        // the prediction failed: give the blocks back and run again with exact sizes
        pool_free(c, x.raw->block, x.raw->block_bytes);
        x.raw->block = nullptr;
        x.raw->block_bytes = 0;
        if (x.raw->coord_blk) { pool_free(c, x.raw->coord_blk, x.raw->coord_bytes); x.raw->coord_blk = nullptr; x.raw->d_coord = nullptr; x.raw->d_coord_bad = nullptr; }
        stt.n_passes = 1;
        stt.order_bucketed = 0;
        x.bucketed = false;
        scan_grow(sc.cand_cap, sc.hit_cap, n_cand, n_hits, &want_cand, &want_hits);
    }
    if ((rc = scan_exact(x, want_cand, want_hits))) return rc;
    *out = dbg && dbg->stop ? nullptr : res.release();
    return MS_OK;
}

}  // namespace ms

using namespace ms;

extern "C" {

int ms_scan(const ms_pwmset *pwms_c, const ms_seqset *seqs, int strand_mask, uint32_t flags, ms_result **out) {
    if (!out) { set_error("out is NULL"); return MS_ERR_INVALID; }
    *out = nullptr;
    if (!pwms_c || !seqs) { set_error("NULL handle"); return MS_ERR_INVALID; }
    if (strand_mask < 1 || strand_mask > 3) { set_error("invalid strand mask %d (1 '+', 2 '-', 3 both)", strand_mask); return MS_ERR_INVALID; }
    if (flags & ~(uint32_t) (MS_SCAN_EXACT_ONLY | MS_SCAN_COUNTS_ONLY)) { set_error("unknown scan flags 0x%x", flags); return MS_ERR_INVALID; }
    ms_pwmset *pwms = const_cast<ms_pwmset *>(pwms_c);       // lazily cached device copies / plan
    DeviceCtx *c;
    int rc = get_ctx(seqs->device, &c);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk_dev(c->mu);
    std::lock_guard<std::mutex> lk_pwm(pwms->mu);
    const uint32_t internal = (flags & MS_SCAN_EXACT_ONLY) | ((flags & MS_SCAN_COUNTS_ONLY) ? MS_SCAN_COUNTS_ONLY_INTERNAL : 0u);
    return scan_locked(c, pwms, seqs, strand_mask, internal, out);
}

// The two debug entries around the candidate list (include/motifscan_amd_debug.h): ms_scan's own driver with a stop or a start point
// (ScanDebug).  What the set remembers of its last scan -- the prediction of the next one's sizes -- is put back: a list of the caller's
// choosing says nothing about the set's hit density.
static int scan_debug(const ms_pwmset *pwms_c, const ms_seqset *seqs, int strand_mask, uint32_t flags, const ScanDebug &dbg, ms_result **out) {
    if (!pwms_c || !seqs) { set_error("NULL handle"); return MS_ERR_INVALID; }
    if (strand_mask < 1 || strand_mask > 3) { set_error("invalid strand mask %d (1 '+', 2 '-', 3 both)", strand_mask); return MS_ERR_INVALID; }
    if (flags & ~(uint32_t) (MS_SCAN_EXACT_ONLY | MS_SCAN_COUNTS_ONLY)) { set_error("unknown scan flags 0x%x", flags); return MS_ERR_INVALID; }
    ms_pwmset *pwms = const_cast<ms_pwmset *>(pwms_c);
    DeviceCtx *c;
    int rc = get_ctx(seqs->device, &c);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk_dev(c->mu);
    std::lock_guard<std::mutex> lk_pwm(pwms->mu);
    const double density = pwms->pred_density, margin = pwms->pred_margin;
    const ScanKey key = pwms->pred_key;
    const uint32_t internal = (flags & MS_SCAN_EXACT_ONLY) | ((flags & MS_SCAN_COUNTS_ONLY) ? MS_SCAN_COUNTS_ONLY_INTERNAL : 0u) | MS_SCAN_NO_PREDICT_INTERNAL;
    rc = scan_locked(c, pwms, seqs, strand_mask, internal, out, nullptr, &dbg);
    pwms->pred_density = density; pwms->pred_margin = margin; pwms->pred_key = key;
    return rc;
}

int ms_debug_scan_candidates(const ms_pwmset *pwms, const ms_seqset *seqs, int strand_mask, uint32_t flags, uint64_t *records, uint64_t cap,
                             uint64_t *n_slots, int64_t geom[16]) {
    if (!n_slots || !geom) { set_error("NULL argument"); return MS_ERR_INVALID; }
    ScanDebug dbg;
    dbg.stop = true; dbg.out = records; dbg.cap = records ? cap : 0; dbg.n_slots = n_slots; dbg.geom = geom;
    ms_result *none = nullptr;
    return scan_debug(pwms, seqs, strand_mask, flags, dbg, &none);
}

int ms_debug_scan_from_candidates(const ms_pwmset *pwms, const ms_seqset *seqs, int strand_mask, uint32_t flags, const uint64_t *records, uint64_t n,
                                  ms_result **result) {
    if (!result) { set_error("out is NULL"); return MS_ERR_INVALID; }
    *result = nullptr;
    if (n > 0 && !records) { set_error("records is NULL"); return MS_ERR_INVALID; }
    ScanDebug dbg;
    dbg.records = records; dbg.n = n;
    return scan_debug(pwms, seqs, strand_mask, flags, dbg, result);
}

// the bucketed hit list's host arithmetic alone, for CPU tests (include/motifscan_amd_debug.h)
int ms_debug_bucket_plan(const int64_t *offsets, int64_t n_seqs, const int32_t *widths, int32_t n_pwms, int32_t gbits, int32_t pbits, int32_t end_bit,
                         int32_t low_bits, int64_t n_regions, uint64_t *weights, double mu, uint64_t n_pred, uint64_t cap_max, uint32_t form, int32_t force,
                         uint64_t *need, int32_t *gate, uint64_t *base, uint64_t *cap) {
    if (!weights || !need || !gate || !base || !cap) { set_error("NULL argument"); return MS_ERR_INVALID; }
    BucketWeights bw;
    if (offsets) {
        if (!widths || n_seqs < 0 || n_pwms < 0) { set_error("invalid set"); return MS_ERR_INVALID; }
        bucket_weights(offsets, n_seqs, widths, n_pwms, gbits, pbits, low_bits, &bw);
        for (int b = 0; b < kOrderBuckets; b++) weights[b] = bw.w[b];
    } else {
        bw.total = 0;
        for (int b = 0; b < kOrderBuckets; b++) { bw.w[b] = weights[b]; bw.total += weights[b]; }
    }
    BucketShape bs;
    bs.predicted = (form & 1u) != 0; bs.counts_only = (form & 2u) != 0; bs.carry_only = (form & 4u) != 0; bs.sticky_off = (form & 8u) != 0;
    bs.pbits = pbits; bs.gbits = gbits; bs.end_bit = end_bit; bs.L = low_bits; bs.P = n_pwms; bs.R = offsets ? n_seqs : n_regions;
    ScanOverrides ov;
    ov.order_buckets = force < 0 ? -1 : (force ? 1 : 0);
    *need = bucket_need(bw, mu);
    *gate = bw.total > 0 && bucket_gate(bs, ov, *need, n_pred) ? 1 : 0;
    unsigned long long b64[kOrderBuckets], c64[kOrderBuckets];
    bucket_caps(bw, mu, n_pred, cap_max, b64, c64);
    for (int b = 0; b < kOrderBuckets; b++) { base[b] = b64[b]; cap[b] = c64[b]; }
    return MS_OK;
}

// the hit keys' layout for a set of these sizes, as scan_locked would choose it (include/motifscan_amd_debug.h)
int ms_debug_key_layout(int64_t n_bases, int64_t n_seqs, int64_t max_len, int32_t n_pwms, int32_t coord_global, int32_t *gbits, int32_t *pbits) {
    if (!gbits || !pbits) { set_error("NULL argument"); return MS_ERR_INVALID; }
    if (n_bases < 0 || n_seqs < 0 || max_len < 0 || max_len > n_bases || n_pwms < 0) { set_error("invalid sizes"); return MS_ERR_INVALID; }
    const ScanGeom g = scan_key_layout(n_bases, n_seqs, max_len, n_pwms, coord_global != 0);
    *gbits = g.gbits;
    *pbits = g.pbits;
    return MS_OK;
}

}  // extern "C"
