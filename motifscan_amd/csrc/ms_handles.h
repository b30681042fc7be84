// ms_handles.h -- private to libmotifscan_amd: per-device state and the structs behind the opaque handles of
// include/motifscan_amd.h, shared by the library's translation units: ms_context.hip (device contexts, pools), ms_pwmset.hip, ms_seqset.hip,
// ms_result.hip (one per handle), ms_scan.hip (scan pipeline), ms_sweep.hip (window sweep), ms_regions.hip and ms_stream.hip (batch streams,
// host-streamed sweeps), ms_best.hip (best window per cell), ms_allelebest.hip (best window per variant haplotype), ms_pairs.hip (motif pairs over a result's hits), ms_scorehist.hip (score histogram of every window),
// ms_personal.hip (a variant set spliced into a new resident genome, and the lift map between the two), ms_sitestack.hip (base counts per
// motif column over a result's sites), ms_ranksum.hip (rank sums and passing-region counts over best-site matrices), ms_affinity.hip (the
// summed likelihood ratio of every cell), ms_expcounts.hip (the expected base counts per motif column on an affinity's terms), ms_shuffle.hip (a sequence set shuffled into a new one: mono- and dinucleotide controls),
// ms_kmers.hip (the k-mer counts of a sequence set or a genome), ms_sitesignal.hip (a resident per-base track and its sums over a result's sites),
// ms_variants.hip and ms_alleles.hip (the record scans over variants: one placement driver, place_records, and one handle head, RecHead).
// The five dense walks -- ms_best.hip, ms_affinity.hip, ms_scorehist.hip, ms_expcounts.hip, ms_dimodel.hip (the best window per first-order
// model) -- plan on the host with ms_dense_plan.h and share the dense_* helpers below (the plan's upload, the chunked launches, the LDS limit;
// DenseHead, what ms_best and ms_affinity begin with) and WorkBlock, the one place a work block goes back to the pool from.  The three that
// fill a [P][R] matrix (ms_scan_best, ms_scan_affinity, ms_scan_best_dimodels) run through one driver, DenseRun, and the two best-site walks
// end in one tail (best_alloc, best_tail).  ms_best.hip implements all of it.  ms_bipartite.hip (the best site of two half-sites with a
// variable spacer) is a sixth walk on the same driver and tail; it adds the gap plane to ms_best.
#pragma once
#include <sched.h>
#include <atomic>
#include <condition_variable>
#include <deque>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "ms_dense_plan.h"
#include "ms_kernels.h"
#include "ms_place.h"

namespace ms {

// sizes of the arrays carved out of one pooled block: 256-byte slots (Carve, ms_place.h)
inline size_t up256(size_t x) { return Carve::up(x); }

// false, with the error text set, where there is no device: a handle cannot exist without one, and an entry point says so before it
// asks for a handle
inline bool require_device() {
    int n_dev = 0;
    if (ms_device_count(&n_dev) == MS_OK && n_dev > 0) return true;
    set_error("no usable HIP device; libmotifscan_amd has no CPU fallback");
    return false;
}

struct Scratch {                 // grow-only work buffers of the scan pipeline
    uint64_t *cand = nullptr;     size_t cand_cap = 0;
    uint64_t *keys = nullptr;     double *vals = nullptr;   uint64_t *keys_sorted = nullptr;  size_t hit_cap = 0;
    void *sort_tmp = nullptr;     size_t sort_tmp_bytes = 0;
    unsigned int *chunk_counters = nullptr;    size_t chunk_counters_cap = 0;   // per LDS tile: the pre-filter's chunk dispenser
    unsigned long long *counters = nullptr;      // 8 words: [0] candidate record slots, [1] hits, [2] runs ordered by order_overflow_kernel, [3] != 0: a hit did not fit its bucket (ms_scan.hip)
    unsigned long long *bucket_tab = nullptr;    // kBucketTabWords: base, capacity and fill of the 256 buckets of a bucketed hit list (BucketOut)
    unsigned long long *h_counters = nullptr;    // pinned
};

// Free list of result blocks (ms_result keeps its arrays in HBM until freed; a scan loop would
// otherwise pay a hipMalloc + hipFree of ~200 MB per call).
struct BlockPool {
    std::mutex mu;
    std::vector<std::pair<void *, size_t>> free_;
    size_t bytes = 0;
    // Blocks are handed out in size classes (pool_class: eight per octave), so that batches of similar but unequal size -- the
    // chromosomes of a sweep, the batches of a region stream -- reuse each other's blocks instead of going to the driver:
    // hipMalloc maps pages for milliseconds and hipFree waits for the whole device, either stalls every stage of a stream.
    size_t max_bytes = 96ull << 30;                        // cached at most: a third of the device's memory (set in get_ctx from hipMemGetInfo)
    static constexpr size_t kMaxBlocks = 512;
    uint64_t n_hit = 0, n_miss = 0, n_driver_free = 0, ns_driver = 0;
};

// A stream in two editions: `whole` may use every CU; `part` is confined by a CU mask (hipExtStreamCreateWithCUMask).
// With MS_MEASURE=1 MS_CU_PARTITION=1 the CUs are partitioned while a batch stream is live (DeviceCtx::n_streams > 0): the
// scan's stream keeps all but 1 of every 32 CUs, the upload / copy-out streams get those.  What it is for
// (tools/ubench/cu_share_probe.hip): the pre-filter's blocks are persistent and each fills a CU, and a second kernel's
// workgroups are handed to the shader engines in order -- one full engine stalls the whole hand-out, so a pack or copy kernel
// launched beside the pre-filter ends only when the pre-filter does, even when whole CUs elsewhere are idle (248 or 240 hog
// blocks still hold a side kernel back for their whole run; 224, one free CU per engine, do not).  With the masks the 62 MB
// upload + pack takes 2.4 ms beside a scan, not 4.  It is OFF by default because it buys nothing end to end
// (profiles/r02_cu_partition_ab.log): the pre-filter runs power-limited, and copy kernels that really run beside it lower its
// clock (2236 vs 2343 MHz) on top of the 3 % of CUs they take -- 76.5 vs 75.2 ms per configs[3] pass, and the sweep's
// copy-out of every site drops to 41 GB/s on 8 CUs.  Starved copies that wait for the pre-filter cost less than concurrent ones.
struct StreamSel {
    hipStream_t whole = nullptr, part = nullptr;
    const std::atomic<int> *n_streams = nullptr;
    operator hipStream_t() const { return (part && n_streams && n_streams->load(std::memory_order_relaxed) > 0) ? part : whole; }
};

struct DeviceCtx {
    int device = -1;
    BlockPool pool;
    // stream is only used under `mu`, and n_streams only changes under `mu`: one scan sees one edition throughout.
    // stream_up / stream_down are used without `mu`: every function reads them ONCE into a local hipStream_t.
    StreamSel stream;
    StreamSel stream_up;                     // sequence upload + packing (runs beside a scan of the previous batch)
    StreamSel stream_down;                   // copy-out of hit arrays (runs beside a scan of the next batch)
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    hipEvent_t ev[8] = {};
    int n_cu = 0;
    int n_cu_copy = 0;                       // CUs the copy streams own while the device is partitioned (0: masks unavailable)
    std::atomic<int> n_streams{0};           // live batch streams on this device
    size_t lds_max = 0;
    bool rc_lds_set = false;                // rescore_carry_kernel's dynamic-LDS attribute raised
    std::vector<const void *> lds_raised;   // the dense walks' kernels whose attribute dense_raise_lds has raised
    size_t lds_set[3] = {};                 // dynamic-LDS attribute already raised to this, per pre-filter kernel (parked, dense, wide)
    Scratch sc;
    std::mutex mu;               // one scan at a time per device (shared scratch)
    // the pending-scan slots (events + pinned counter words) of batch streams that have ended, for the next stream on this device: a pass that
    // opens and drains its own stream (bench.py 'pipelined') otherwise pays 14 hipEventCreate + 2 hipHostMalloc at its start and their release --
    // hipHostFree waits for the whole device -- at its end (round 6)
    std::mutex pend_mu;
    std::vector<struct PendingScan *> pend_cache;
};

int get_ctx(int device, DeviceCtx **out);
int current_device();                 // the calling thread's device (ms_set_device)
void set_current_device(int device);  // thread-local only; no HIP call

// Give every cached block of the calling thread's device back to the driver (ms_context.hip); returns the bytes released.
size_t pool_trim_current_device();
// ms_hostpack.cpp: convert_seq and the region hints on host threads (units of 32 bases / blocks of 64 positions [u0, u1) / [b0, b1))
void host_pack_units(const uint8_t *bases, int64_t n_bases, int64_t u0, int64_t u1, uint32_t *codes, uint32_t *nmask);
void host_region_hints(const int64_t *offsets, int64_t R, int64_t b0, int64_t b1, int32_t *blk2reg, int32_t *info, bool all_far);
// ms_numa.cpp: NUMA placement of a device's host side (sysfs + sched_setaffinity; no device code)
int parse_cpulist(const char *text, cpu_set_t *set);
int numa_node_of_bdf(const char *bdf, const char *root);
int numa_cpus_of_node(int node, const char *root, cpu_set_t *set);
int numa_node_count(const char *root);
int numa_bind_calling_thread(int node);
// the policy (MS_NUMA_BIND, ms_numa.cpp) applied to the calling thread for `device`: returns the node bound to, -1 if none
int numa_bind_for_device(int device, bool force);
void pinned_pool_stats(uint64_t out[4]);
int result_fetch_region_counts(ms_result *r);
int seqset_create_upload_only(const char *bases, const int64_t *offsets, int64_t n_seqs, ms_seqset **out);
int seqset_pack_pending(const ms_seqset *s, hipStream_t st);
int seqset_create_hostpacked(const char *bases, const int64_t *offsets, int64_t n_seqs, int n_threads, void **stage_io, size_t *stage_bytes_io, ms_seqset **out);

// ms_debug_alloc_fill (ms_context.hip; tests only): -1 = off, 0..255 = every block handed out -- by dev_alloc, by pool_alloc on a hit and on
// a miss, by pinned_alloc on a hit and on a miss -- is filled with that byte over its whole granted size before the caller sees it, so
// that a test decides what "recycled memory" holds.  Off, it costs the one relaxed load below and no HIP call.
extern std::atomic<int> g_alloc_fill;
inline int alloc_fill_setting() { return g_alloc_fill.load(std::memory_order_relaxed); }
// `bytes` of device memory at p, on `device` (-1: the calling thread's current one), set to `byte`: hipDeviceSynchronize, hipMemset,
// hipDeviceSynchronize -- the library's streams are non-blocking, and the fill has to be complete on every one of them
MS_HIDDEN int alloc_fill_device(void *p, size_t bytes, int byte, int device);

template <typename T>
inline int dev_alloc(T **p, size_t n) {
    *p = nullptr;
    if (n == 0) n = 1;
    hipError_t e = hipMalloc(reinterpret_cast<void **>(p), n * sizeof(T));
    if (e == hipErrorOutOfMemory && pool_trim_current_device() > 0) {       // the block cache may be what fills the device: drop it, once
        (void) hipGetLastError();
        e = hipMalloc(reinterpret_cast<void **>(p), n * sizeof(T));
    }
    if (e != hipSuccess) {
        set_error("hipMalloc of %zu bytes failed: %s", n * sizeof(T), hipGetErrorString(e));
        return e == hipErrorOutOfMemory ? MS_ERR_NOMEM : MS_ERR_RUNTIME;
    }
    if (const int fill = alloc_fill_setting(); fill >= 0) {
        if (const int rc = alloc_fill_device(*p, n * sizeof(T), fill, -1)) { (void) hipFree(*p); *p = nullptr; return rc; }
    }
    return MS_OK;
}

template <typename T>
inline void dev_free(T *&p) {
    if (p) (void) hipFree(p);
    p = nullptr;
}

int pool_alloc(DeviceCtx *c, size_t bytes, void **out, size_t *got);
void pool_free(DeviceCtx *c, void *p, size_t bytes);
void *pinned_alloc(size_t bytes, size_t *got);
void pinned_free(void *p, size_t bytes);

// (strand mask, cutoffs, exact-only): what a PWM set's memos about its scans -- the hit density, "plans without a wide tile" -- are keyed by
struct ScanKey {
    int strand = -1;
    uint64_t cutoff_version = 0;
    bool exact_only = false;
    bool operator==(const ScanKey &o) const { return strand == o.strand && cutoff_version == o.cutoff_version && exact_only == o.exact_only; }
};

}  // namespace ms

// ------------------------------------------------------------------------- handles --

struct ms_pwmset {
    int32_t P = 0;
    std::vector<double> values;       // concatenated [4][W] row-major, as given
    std::vector<int64_t> val_off;     // [P+1] in doubles
    std::vector<int32_t> widths;
    std::vector<double> cutoffs;
    std::vector<double> max_raw;
    int max_width = 0;
    uint64_t cutoff_version = 1;
    // device copies (lazy)
    int device = -1;
    uint64_t dev_cutoff_version = 0;
    double2 *d_tab2 = nullptr;
    int64_t *d_tab_off = nullptr;
    int32_t *d_width = nullptr;
    int64_t tab2_entries = 0;                     // entries of d_tab2 before its closing all-zero entry
    std::vector<int64_t> tab_off_host;            // the motifs' offsets in d_tab2 (entries)
    double *d_thresh = nullptr;                   // [P][4] {max_raw, cutoff, raw_floor, 0} (DevPwm::thresh)
    std::vector<double> raw_floor_host;           // [P] (FieldMeta::floor32 is made of it)
    ms::FieldMeta *d_field_meta = nullptr;        // [table groups][16] of the plan (rescore_kernel)
    double *d_max_raw = nullptr;
    double *d_cutoff = nullptr;
    double *d_raw_floor = nullptr;
    // what the last scan with these PWMs (the one pred_key names) found, for the one-sync form of the next (ms_scan.hip, scan_locked):
    // hits per window, and how far above it the next count may be before the prediction counts as failed
    double pred_density = -1.0, pred_margin = 0.06;
    bool bucket_off = false;                      // a bucket of a bucketed hit list overflowed once (skewed data): this set's scans emit plain lists from then on
    ms::ScanKey pred_key;
    // pre-filter plan (lazy, keyed by strand mask / cutoffs / LDS budget / exact-only)
    ms::PrefilterPlan plan;
    int plan_strand = -1;
    uint64_t plan_cutoff_version = 0;
    size_t plan_lds = 0;
    bool plan_exact_only = false;
    bool plan_pair = true;                        // paired rows in the plan (always, but for MS_MEASURE=1 MS_PF_PAIR=0)
    int plan_device = -1;
    // (strand, cutoffs, exact-only) for which a set WITH motifs of >= 32 columns is known to plan without a wide tile (ms_scan.hip, scan_plan)
    ms::ScanKey narrow_key;
    uint4 *d_tables = nullptr;
    ms::TileDesc *d_tiles = nullptr;
    int32_t *d_group_fields = nullptr;            // [table groups][kGroupFields] motif of the field, -1 = empty
    int32_t *d_exact_motifs = nullptr;
    std::mutex mu;
};

struct ms_seqset {
    int device = 0;
    int64_t R = 0;
    int64_t n_bases = 0;
    std::vector<int64_t> offsets;         // host copy [R+1]
    std::vector<int64_t> len_sorted;      // DISTINCT region lengths ascending
    std::vector<int64_t> len_cnt_ge;      // [i]: number of regions with length >= len_sorted[i]   (+ trailing 0)
    std::vector<int64_t> len_sum_ge;      // [i]: their total length                              (+ trailing 0)
    void *block = nullptr;                // one pooled device block holding codes / nmask / offsets / blk2reg
    size_t block_bytes = 0;
    uint8_t *d_ascii = nullptr;           // pooled block; kept only when asked to
    size_t ascii_bytes = 0;
    uint32_t *d_codes = nullptr;
    uint32_t *d_nmask = nullptr;
    int64_t *d_offsets = nullptr;
    int32_t *d_blk2reg = nullptr;         // region of position 64*b
    int4 *d_blkinfo = nullptr;            // ... with the region's and the next two regions' starts relative to 64*b (DevSeq::blkinfo)
    hipStream_t up = nullptr;             // the upload stream this set is being built on (DeviceCtx::stream_up, read once)
    void *h_off_pin = nullptr;            // the offsets' way to the device: a pinned copy (from pageable memory the runtime copies with a KERNEL, which waits for a CU the pre-filter holds)
    size_t h_off_pin_bytes = 0;
    // the weights of a bucketed hit list's 256 buckets (bucket_weights, ms_scan_geom.h), made by the first scan that wants them and kept: the offsets
    // of a live set never change.  Keyed by the key layout, L and the motif widths (bk_widths: a hash).  Touched under the device's lock.
    // Up to four are kept (the last used first): PWM sets of different widths that take turns on one sequence set each find theirs.
    struct BkWeights { int gbits, pbits, L; uint64_t widths; ms::BucketWeights w; };
    std::vector<BkWeights> bk_weights;
    bool built = false;                   // construction finished (its work on `up` is done)
    bool pack_pending = false;            // a batch stream's upload-only set: ASCII and offsets are in HBM, pack_kernel / blk2reg_kernel still to run (seqset_pack_pending, on the scan stream)
};

struct ms_result {
    int device = 0;
    int32_t P = 0;
    int64_t R = 0;                                    // sequences of the scanned set
    int64_t n_hits = 0;
    bool deduped = false;
    int raw_gbits = 0, raw_pbits = 0;                 // MS_SCAN_RAW_INTERNAL: layout of the unordered hit keys left in the device scratch
    bool counts_only = false;                         // a sweep span of a counts-only stream: per-motif window counts and the number of sites, NO site arrays
    void *block = nullptr;                            // one device block holding everything below
    size_t block_bytes = 0;
    int64_t *d_seq_idx = nullptr;
    int64_t *d_pos = nullptr;
    double *d_score = nullptr;
    int8_t *d_strand = nullptr;
    unsigned long long *d_region_counts = nullptr;   // [P]
    int64_t *d_motif_first = nullptr;                 // [P+1]: after ms_scan returns, the per-motif offsets
    std::vector<int64_t> motif_offsets;               // [P+1]
    void *coord_blk = nullptr;                        // MS_SCAN_PACK_INTERNAL: the compact coordinate words, made by the scan itself ...
    size_t coord_bytes = 0;
    uint64_t *d_coord = nullptr;                      // ... [n slots] + a "does not fit" flag word behind them
    unsigned int *d_coord_bad = nullptr;
    int coord_shift = 0;                              // 0: 8-byte words; > 0: 4-byte words seq_idx << coord_shift | pos << 1 | strand bit (MS_SCAN_PACK12_INTERNAL, when the set fits)
    int h_coord_shift = 0;                            // ... the form of the host copy
    void *h_pinned = nullptr;                         // host copy of the hit arrays (pinned), made on demand
    bool h_packed = false;                            // ... in the compact form (coord | score)
    size_t h_pinned_bytes = 0;
    int64_t h_pinned_hits = -1;
    std::vector<int64_t> h_region_counts;             // a batch stream's copy-out stage brings the per-motif region counts along (ms_result_region_counts then copies host to host)
    ms_scan_stats stats;
};

namespace ms {

// What the handles of the two dense [P][R] results begin with (ms_best, ms_affinity), and the one implementation of what only reads it
// (ms_best.hip).
struct DenseHead {
    int device = 0;
    int32_t P = 0;
    int64_t R = 0;
    void *block = nullptr;                            // one pooled device block holding the [P][R] planes
    size_t block_bytes = 0;
    double device_ms = 0.0;                           // first launch -> last kernel done
};
MS_HIDDEN void dense_release(DenseHead *h);           // the block back to its device's pool
MS_HIDDEN int dense_shape(const DenseHead *h, int32_t *n_pwms, int64_t *n_seqs);
MS_HIDDEN int dense_device_ms(const DenseHead *h, double *ms);
// the motif rows [m0, m1) of a plane, checked: they are the *n cells from cell *at on; with *n > 0 the calling thread is on the handle's device
MS_HIDDEN int dense_rows(const DenseHead *h, int32_t m0, int32_t m1, size_t *at, size_t *n);

}  // namespace ms

struct ms_best : ms::DenseHead {                      // ms_scan_best: the best window of every (motif, region) cell; three planes
    double *d_score = nullptr;                        // NaN: no winner
    int32_t *d_pos = nullptr;                         // relative to the region start, -1: no winner
    int8_t *d_strand = nullptr;                       // 1 '+', 2 '-', 0: no winner
    int16_t *d_gap = nullptr;                         // ms_scan_best_bipartite only (nullptr from every other scan): the winner's gap, -1: no winner
};

struct ms_affinity : ms::DenseHead {                  // ms_scan_affinity: the summed likelihood ratio of every (motif, region) cell; four planes
    double *d_peak = nullptr;                         // the greatest raw sum over the terms; NaN: no term
    double *d_sum = nullptr;                          // sum of exp(scale * (raw - peak))
    double *d_log_mean = nullptr;                     // scale * peak + log(sum / n_terms): the plane ms_affinity_rank_sum ranks
    int32_t *d_n_terms = nullptr;
    int strand_mask = 0;                              // the scan's arguments, for ms_affinity_expected_counts (ms_expcounts.hip): the second walk
    double scale = 0.0;                               // over the same terms reads them here, so they cannot disagree with the planes
    int32_t max_n = -1;
};

struct ms_track {                                     // ms_track_create: one int32 per base of a sequence set
    int device = 0;
    int64_t R = 0;
    int64_t n_values = 0;
    std::vector<int64_t> offsets;                     // host copy [R+1]
    void *block = nullptr;                            // one pooled device block: [pad][values][pad] | offsets
    size_t block_bytes = 0;
    int32_t *d_values = nullptr;                      // the first value, kTrackPad zeroed values behind the block's start (ms_sitesignal.hip)
    int64_t *d_offsets = nullptr;                     // [R+1]
};

namespace ms {

// 1: device memory of `device`; 0: host memory; -1: device memory of another device (*other) -- where an output or an input array of the
// caller's lies (ms_sitestack.hip)
MS_HIDDEN int pointer_place(const void *p, int device, int *other);

// What the handles of the two record scans begin with (ms_varscan, ms_allelescan): the placement's output (place_records) and the one
// implementation of the accessors that only read it.
struct RecHead {
    int device = 0;
    int32_t P = 0;
    int64_t V = 0;
    int64_t n = 0;                                    // records
    void *block = nullptr;                            // one pooled device block holding the record arrays
    size_t block_bytes = 0;
    std::vector<int64_t> motif_offsets;               // [P+1]
    std::vector<int64_t> gained, lost;                // [P], counted on the device
    double device_ms = 0.0;                           // first launch -> last kernel done
};
MS_HIDDEN void rec_release(RecHead *h);               // the block back to its device's pool
MS_HIDDEN int rec_num_sites(const RecHead *h, int64_t *n);
MS_HIDDEN int rec_motif_offsets(const RecHead *h, int64_t *out);
MS_HIDDEN int rec_motif_counts(const RecHead *h, int64_t *gained, int64_t *lost);
MS_HIDDEN int rec_device_ms(const RecHead *h, double *ms);

// The scratch of place_records in the caller's work block: place_slots adds it to the block's layout (it asks the prefix sum for its
// temporary size, hence the stream and the return code).
struct PlaceSlots {
    Carve::Slot<uint32_t> cnt;                        // [n_cells] records of every (motif, tile) of a chunk
    Carve::Slot<uint64_t> excl;                       // [n_cells] their exclusive prefix sums
    Carve::Slot<uint64_t> tot, base;                  // [chunks][P] records of the motif in the chunk, and where they go
    Carve::Slot<unsigned long long> gl;               // [2][max(P, 1)] gained, lost
    Carve::Slot<char> tmp;
    size_t tmp_bytes = 0;
};
MS_HIDDEN int place_slots(Carve &cv, const PlaceChunks &ch, int32_t P, hipStream_t st, PlaceSlots *out);

// The two launches of a chunk [v0, v0 + nv) of variants, and the allocation of the record block once their number is known.
struct PlaceCalls {
    std::function<int(int64_t v0, int64_t nv, uint32_t *tile_cnt, unsigned long long *gained, unsigned long long *lost)> count;
    std::function<int(int64_t v0, int64_t nv, const uint64_t *tile_excl, const uint64_t *row_base)> fill;
    std::function<int(size_t n)> alloc;
};
// Records in output order without a sort or an atomic (ms_variants.hip's header has the scheme): every chunk counted, the counts summed
// into h->motif_offsets and h->n, the records allocated, every chunk filled; then h->gained / lost / device_ms (from c->ev[0], which the
// caller has recorded in front of its upload).  `tile`: variants per block of the caller's kernel; `what` names the scan in the error
// texts.  The caller holds c->mu; on an error it synchronises the stream before it gives `work` back.
MS_HIDDEN int place_records(DeviceCtx *c, const PlaceChunks &ch, int tile, void *work, const PlaceSlots &s, const char *what, const PlaceCalls &calls, RecHead *h);

// ---- the host side of a dense walk (ms_best.hip; the plan itself is ms_dense_plan.h)
// the code of a failed HIP call, with the error text "<what> failed: <HIP's text>" set
inline int hip_rc(hipError_t e, const char *what) {
    set_error("%s failed: %s", what, hipGetErrorString(e));
    return e == hipErrorOutOfMemory ? MS_ERR_NOMEM : MS_ERR_RUNTIME;
}
// MS_ERR_INVALID for a region of 2^31 bases or more: `what` ("positions are", "n_terms is") is 32-bit in the result
MS_HIDDEN int dense_regions_fit(const ms_seqset *seqs, const char *what);
// dense_plan of widths[P] over a sequence set, with the two ways it fails: out of host memory, and more long regions or blocks of
// segs_per_block segments than the x of one grid holds.  The widths are a PWM set's, or the pseudo-widths of a first-order model set
// (ms_dimodel.hip).
template <typename Walked>
inline int dense_plan_for(const DenseGeom &g, const int32_t *widths, int32_t P, const ms_seqset *seqs, int segs_per_block, Walked walked, DensePlan *pl) {
    try { dense_plan(g, widths, P, seqs->offsets.data(), seqs->R, walked, pl); }
    catch (const std::bad_alloc &) { set_error("out of host memory"); return MS_ERR_NOMEM; }
    if (pl->long_regions.size() > 0x7FFFFFFFull || (pl->n_seg + segs_per_block - 1) / segs_per_block > 0x7FFFFFFFLL) { set_error("too many segments for one launch"); return MS_ERR_INVALID; }
    return MS_OK;
}
template <typename Walked>
inline int dense_plan_for(const DenseGeom &g, const ms_pwmset *pwms, const ms_seqset *seqs, int segs_per_block, Walked walked, DensePlan *pl) {
    return dense_plan_for(g, pwms->widths.data(), pwms->P, seqs, segs_per_block, walked, pl);
}
// A plan's arrays on the device, in the work block they were given slots in (dense_slots): nullptr where the plan has none.
struct DenseDev {
    const int64_t *seg_first = nullptr, *part_first = nullptr, *long_regions = nullptr;
    const int32_t *mot = nullptr, *tile_first = nullptr, *wide_first = nullptr, *skipped = nullptr;
};
MS_HIDDEN int dense_upload(const DensePlan &pl, const DenseSlots &s, void *work, hipStream_t st, DenseDev *d);
// The dynamic-LDS limit of a dense walk's kernel raised to `most` bytes, the first time a launch on this device needs more than the
// 48 KB every kernel may have: once per device and kernel (DeviceCtx::lds_raised), as ms_scan_best always did.
MS_HIDDEN int dense_raise_lds(DeviceCtx *c, const void *kernel, size_t need, size_t most);
// Rows [0, n) of a grid's y -- tiles, groups of motifs -- in chunks of at most kDenseGridY: launch(first, count) queues one chunk, and
// `what` names the kernel in the error text of a launch that fails.
constexpr int64_t kDenseGridY = 32768;
template <typename Launch>
inline int dense_chunks(int64_t n, const char *what, Launch launch) {
    for (int64_t y0 = 0; y0 < n; y0 += kDenseGridY) {
        launch(y0, (unsigned) std::min(kDenseGridY, n - y0));
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return hip_rc(e, what);
    }
    return MS_OK;
}
// A work block from the device's pool and the stream its readers and writers are queued on: the ONE place such a block goes back from.
// The pool is not stream-ordered (pool_free hands the block on at once, pool_alloc may fill it from elsewhere), so release() waits for the
// stream first unless wait() has succeeded: on every early return nothing queued may still touch the block.  Its owner declares it
// BEHIND its lock guards (the wait runs under them) and behind the result handle the queued work fills (freed after it).
struct WorkBlock {
    DeviceCtx *c = nullptr;
    hipStream_t st = nullptr;
    void *p = nullptr;
    size_t bytes = 0;
    bool idle = false;                                // wait() has succeeded: nothing queued is left
    WorkBlock() = default;
    WorkBlock(const WorkBlock &) = delete;
    ~WorkBlock() { release(); }
    int alloc(DeviceCtx *ctx, hipStream_t stream, size_t n) { c = ctx; st = stream; return pool_alloc(c, n, &p, &bytes); }
    int wait(const char *what) {                      // the owner's last synchronisation; `what` names it in the error text
        const hipError_t e = hipStreamSynchronize(st);
        idle = e == hipSuccess;
        return idle ? MS_OK : hip_rc(e, what);
    }
    void release() {
        if (p && !idle) (void) hipStreamSynchronize(st);
        pool_free(c, p, bytes);
        p = nullptr;
    }
};
// The driver of the three walks that fill a [P][R] matrix (ms_scan_best, ms_scan_affinity, ms_scan_best_dimodels): what one keeps from its
// checks to its last launch.  An entry point runs dense_check, its own checks, dense_open, allocates its result, adds its slots to cv,
// runs dense_start, launches, and dense_end.  Whichever way it returns the work block goes back first, the locks are released last.
struct DenseRun {
    DeviceCtx *c = nullptr;
    hipStream_t st = nullptr;
    DensePlan plan;
    Carve cv;                                         // the work block's layout: the plan's slots, then the caller's
    DenseSlots ds;
    DenseDev d;                                       // the plan's arrays in the work block
    unsigned gx = 0;                                  // blocks of kBestWaves segments: the x of the walk's grid
    size_t lds = 0, lds_most = 0;                     // bytes of the plan's largest tile behind its zero entry, and of a full tile
    std::unique_lock<std::mutex> lk_dev, lk_set;      // the device's lock, and the PWM set's where there is one
    WorkBlock work;
};
// require_device, then the checks the three share, with their texts: a NULL handle (`set`: the PWM or model set), the strand mask
MS_HIDDEN int dense_check(const void *set, const ms_seqset *seqs, int strand_mask);
// dense_regions_fit(fit_what), the device's context, the plan of widths[P] by the walk's geometry, the locks, the thread on the device
MS_HIDDEN int dense_open(DenseRun *run, const DenseGeom &g, const int32_t *widths, int32_t P, std::mutex *set_mu, const ms_seqset *seqs, const char *fit_what,
                         const std::function<bool(int32_t)> &walked);
// the work block of layout cv, then on the stream: the PWM set's device copies (pwms may be nullptr), a pending pack of the sequence
// set, `kernel`'s LDS limit (dense_raise_lds), the plan into run->d
MS_HIDDEN int dense_start(DenseRun *run, ms_pwmset *pwms, const ms_seqset *seqs, const void *kernel);
// c->ev[1] behind the last launch, the wait for the stream, h->device_ms since c->ev[0], the work block back to the pool
MS_HIDDEN int dense_end(DenseRun *run, const char *what, DenseHead *h);

// The tail of the three best-site walks (ms_scan_best, ms_scan_best_dimodels, ms_scan_best_bipartite), which fill the same handle.
struct BestPart;                                      // a segment's best of one motif (ms_best_dev.h)
using BestPtr = std::unique_ptr<ms_best, void (*)(ms_best *)>;
// an ms_best of P x R cells on the run's device, three planes carved from one pooled block (a cell's worth for an empty matrix); gaps:
// with the fourth plane d_gap (ms_scan_best_bipartite), 15 bytes per cell
MS_HIDDEN int best_alloc(const DenseRun &run, int32_t P, int64_t R, BestPtr *res, bool gaps = false);
// queues "reduce the long regions, fill the skipped rows" behind the walk's kernels; part[P][n_part]: the segments' partials; `what`
// ("best-site") names the walk in the error text of a launch that fails
MS_HIDDEN int best_tail(const DenseRun &run, const char *what, const BestPart *part, ms_best *b);

// One [P][R] plane of doubles per group, ranked per motif row (ms_ranksum.hip): what ms_best_rank_sum (the score plane of two ms_best) and
// ms_affinity_rank_sum (the log_mean plane of two ms_affinity) both are.  `what` names the handles in the error texts.
struct RankPlane {
    int device;
    int32_t P;
    int64_t R;
    const double *plane;
};
MS_HIDDEN int rank_sum_planes(const char *what, const RankPlane &a, const uint8_t *sel_a, const RankPlane &b, const uint8_t *sel_b, int32_t m0, int32_t m1, uint32_t flags,
                              int64_t *u2, uint64_t *ties, int64_t *n, double *device_ms);

// Internal scan flag: stop after the fp64 stage -- the hits stay UNORDERED in the device scratch (c->sc.keys / vals, key =
// motif << (gbits + 1) | coordinate << 1 | strand bit, coordinate = sequence << pbits | position when pbits > 0, else the
// global base position); the result holds only the count, the key layout and the stage times.  For callers that re-key the
// hits anyway (ms_scan_regions_once) and keep holding c->mu until they are done with the scratch.
#define MS_SCAN_RAW_INTERNAL 0x80000000u

// Internal scan flag: also produce the compact coordinate words (ms_result_hits_packed_host) at the end of the scan, on the scan
// stream -- a batch stream's copy-out then consists of copies only (a pack kernel launched on the copy-out stream would wait for
// the next batch's pre-filter, whose persistent blocks fill every CU).
#define MS_SCAN_PACK_INTERNAL 0x20000000u
// ... in the 4-byte form (ms_result_hits_packed12_host) when every (region, position) of the set fits 31 bits; the 8-byte form otherwise.
#define MS_SCAN_PACK12_INTERNAL 0x10000000u
// Internal scan flag: COUNTS ONLY -- the result holds n_hits, the per-motif site numbers (motif_offsets) and the per-motif region counts, NO site
// arrays (ms_result::counts_only: the hit accessors refuse it): the hits are counted where the fp64 stage left them, unordered
// (count_only_kernel), and the radix sort + finalize are skipped.  Falls back to the ordered path by itself where the bitmap form does not
// apply (global-position keys, more than 4096 motifs, an absurd P x R).
#define MS_SCAN_COUNTS_ONLY_INTERNAL 0x08000000u
// Internal scan flag: never use the predicted-size form (the exactly-sized re-run after a failed prediction).
#define MS_SCAN_NO_PREDICT_INTERNAL 0x40000000u

// A scan whose launches are all queued but whose completion has not been waited for (the predicted-size form, scan_locked with
// pend != nullptr): the owner -- a batch stream's scanner thread -- queues the NEXT batch's scan behind it before it waits, so
// the device never idles between batches.  The slot's events and pinned counter words belong to one scan at a time.
struct PendingScan {
    hipEvent_t ev[6] = {};                   // around the stages, as DeviceCtx::ev
    hipEvent_t done = nullptr;
    unsigned long long *h_counters = nullptr;   // pinned, 8 words
    int64_t *h_offsets = nullptr;               // pinned: the queued scan's per-motif offsets land here, in stream order, in front of `done`
    size_t h_offsets_cap = 0;                   // (words; grown to P + 1)
    size_t cand_cap = 0, hit_cap = 0;           // the scratch capacities at queue time
    bool active = false;
    ms_result *raw = nullptr;
    size_t n_pred = 0;
    uint64_t cand_static = 0;
    int64_t n_bases = 0, R = 0;
    int strand_mask = 3;
    bool exact_only = false;
};
constexpr int MS_SCAN_PENDING = 1000;        // scan_locked: queued, call scan_complete
constexpr int MS_SCAN_RETRY = 1001;          // scan_complete: the prediction failed, run scan_locked(..., MS_SCAN_NO_PREDICT_INTERNAL) again
int pending_scan_init(PendingScan *p);
// a slot from the device's cache (or a new one), and back (ms_scan.hip); a slot that holds an unfinished scan must not be released
PendingScan *pending_scan_acquire(DeviceCtx *c);
void pending_scan_release(DeviceCtx *c, PendingScan *p);
void pending_scan_destroy(PendingScan *p);
// waits for a pending scan; MS_OK: *out is the result; MS_SCAN_RETRY: nothing was produced.  The caller holds pwms->mu.
int scan_complete(DeviceCtx *c, ms_pwmset *pwms, PendingScan *p, ms_result **out);

// A stop or a start point in the exactly-sized scan, for the two debug entries of include/motifscan_amd_debug.h (tests only; a scan that
// carries one is never predicted or queued):
//   stop  -- the front ends behind the pre-filter: the candidate list goes to the host (out / cap / n_slots / geom), no fp64 stage, no result;
//   start -- the pre-filter's launch is replaced by an upload of `records` into the candidate list; everything behind it runs as usual.
struct ScanDebug {
    bool stop = false;
    uint64_t *out = nullptr;                 // stop: the first min(*n_slots, cap) record slots land here (nullptr: only the count)
    uint64_t cap = 0;
    uint64_t *n_slots = nullptr;             // stop: min(cand_static + counters[0], the list's capacity)
    int64_t *geom = nullptr;                 // stop: [16] the launch's geometry (ms_debug_scan_candidates)
    const uint64_t *records = nullptr;       // start: n record slots (0 = empty)
    uint64_t n = 0;
};

// The scan pipeline proper (ms_scan.hip); the caller holds c->mu and pwms->mu.  pend != nullptr: if the sizes can be predicted the
// scan is only QUEUED (returns MS_SCAN_PENDING, finish with scan_complete); otherwise it runs to the end as usual.
int scan_locked(DeviceCtx *c, ms_pwmset *pwms, const ms_seqset *seqs, int strand_mask, uint32_t flags, ms_result **out, PendingScan *pend = nullptr,
                const ScanDebug *dbg = nullptr);
// Hand the hits of a span scan (one region) to the windows of a fixed-stride sweep, in place of *span_res (ms_sweep.hip);
// the caller holds c->mu and pwms->mu.
// counts_only: only the per-motif window counts and the number of sites are made (ms_result::counts_only: the hit accessors refuse it)
int sweep_handout_locked(DeviceCtx *c, ms_pwmset *pwms, ms_result *span_res, int64_t span_bases, int32_t window, int32_t stride,
                         int64_t n_windows, ms_result **out, bool counts_only = false);
int pwmset_upload(ms_pwmset *p, int device, hipStream_t st);
// One pooled device block holds everything a result owns: [counts P+1][offsets P+1][seq_idx n][pos n][score n][strand n]
size_t result_block_bytes(int32_t P, size_t n);
void result_carve(ms_result *r, void *blk, size_t n);

// Helpers of one handle's translation unit that another unit needs (MS_HIDDEN: not exported from the shared object)
// a block for n hits from the device's pool, carved: r->block, r->block_bytes and the array pointers (ms_result.hip; r->P is set)
MS_HIDDEN int result_block_alloc(DeviceCtx *c, ms_result *r, size_t n);
// the pre-filter plan for (strand mask, cutoffs, LDS budget, exact-only), cached in the set; need_device: with its device copies (ms_pwmset.hip)
MS_HIDDEN int pwmset_plan(ms_pwmset *p, int strand_mask, size_t lds_budget, bool exact_only, bool need_device, int device);
MS_HIDDEN DevPwm dev_pwm(const ms_pwmset *p);
MS_HIDDEN DevSeq dev_seq(const ms_seqset *s);
// sum_r max(L_r - W + 1, 0) from the set's sorted lengths (ms_seqset.hip)
MS_HIDDEN int64_t windows_for_width(const ms_seqset *s, int W);
// what ms_debug_varscan_chunk set: variants per chunk of the variant scans, 0 = their own size (ms_variants.hip; read by ms_alleles.hip and ms_allelebest.hip)
MS_HIDDEN int64_t varscan_chunk_setting();
// the allele scan's half of ms_debug_varscan_dims (ms_alleles.hip): kAlTile, kAlThreads, kAlTabMaxW
MS_HIDDEN void allelescan_dims(int32_t out[3]);
// the path constants of the kernels around the scan, for ms_debug_genome_dims (ms_background.hip): the pack / extract block in bases
// (ms_seqset.hip), kNearThreads / kGeneTile / kOverlapThreads (ms_annotation.hip), the element budget of a score-rank batch (ms_pwmset.hip)
MS_HIDDEN int32_t seqset_block_bases();
// a set of these offsets on `device` with its planes and hints unwritten, and blk2reg_kernel for it on `st` (ms_seqset.hip; ms_personal.hip writes the planes)
MS_HIDDEN int seqset_create_unpacked(const int64_t *offsets, int64_t n_seqs, int device, ms_seqset **out);
MS_HIDDEN int seqset_launch_hints(const ms_seqset *s, hipStream_t st);MS_HIDDEN void annotation_dims(int32_t out[3]);
MS_HIDDEN int64_t score_rank_budget_default();

}  // namespace ms
