// ms_kernels.h -- the pre-filter's constants, the kernels' argument structs, and the launchers that cross a translation unit (a kernel
// whose only caller is one handle's file sits in that file, its launcher file-local).
#pragma once
#include "ms_internal.h"

namespace ms {

constexpr int kPfThreads = 1024;      // pre-filter block: 16 waves, one block per CU (4 waves per SIMD: <= 128 VGPRs) -- its waves never meet at a barrier
constexpr int kPfBlocksPerCu = 1;     // after the tables are loaded, so the block shape only decides how many copies of the tables a CU's LDS holds
constexpr int kPfCounters = 8;        // counter words per LDS tile of the per-wave hand-out (64 bytes apart)
constexpr size_t kPfClsBytes = (size_t) kMaxClasses * 32;   // the tile's class descriptors, 32 bytes apiece, behind the B-operand table (prefilter_f6_kernel)
constexpr size_t kF6LutBytes = 256 * 8 + kPfClsBytes;       // byte of four 2-bit codes -> 16 fp4 one-hot k-slots (8 bytes), after the tile's tables; + the class descriptors
constexpr int kPfStageWords = 24;            // per wave: the current pass's code words, then its non-ACGT words -- 8 + 4 (64 window starts), or 16 + 8 (the double pass: 128), after the B-operand table
constexpr size_t kPfStageBytes = (size_t) (kPfThreads / 64) * kPfStageWords * sizeof(uint32_t);
// per wave: the lanes that hold a candidate park their 16 result registers here; the flag words are decoded later, one parked entry
// per lane (ms_kernels.hip, "candidate hand-off")
constexpr int kRareCapMin = 16;              // entries per wave: whatever LDS the tile's tables leave, between these two (PfArgs::rare_cap)
constexpr int kRareCapMax = 64;              // (a wave has 64 lanes: an event never needs more)
constexpr int kRareEntryWords = 12;          // the flag bytes of the 16 result registers (8 words for paired rows, 4 for plain ones) + {position low word, position high bits | group << 8 | paired << 31} at byte 32 + 2 spare: 48 bytes (ms_kernels.hip, park_store)
constexpr size_t kPfRareBytesMin = (size_t) (kPfThreads / 64) * kRareCapMin * kRareEntryWords * sizeof(uint32_t);
constexpr size_t kPfOnehotBytes = (size_t) (kPfThreads / 64) * 160 * 16;  // per wave: the double pass's one-hot array, 160 entries of 16 bytes (ms_kernels.hip, kOnehotEntries)
constexpr double kDenseHitsPerHalfTile = 12.0; // the dense-candidate kernel (ms_kernels.hip) above this many expected hits per row tile and 64 windows: measured 4.4 (p = 1e-3) 34.9 against
                                               // 31.9 ms parked, 44 (p = 1e-2, 1/8 shard) 5.7 against 9.5 ms (profiles/r05_dense_form.log)
constexpr int kPfEmitWords = 16;             // per wave: its place in the global candidate list and the launch's constants (PfEmit, ms_kernels.hip)
constexpr size_t kPfEmitBytes = (size_t) (kPfThreads / 64) * kPfEmitWords * sizeof(uint32_t);

struct DevSeq {
    const uint32_t *codes;
    const uint32_t *nmask;
    const int64_t *offsets;   // [R+1]
    const int32_t *blk2reg;   // [n_bases/64 + 2] region of position 64*b
    const int4 *blkinfo;      // [n_bases/64 + 2] {that region, its start, the next region's, the one after's: relative to 64*b} (blk2reg_kernel)
    int64_t R;
    int64_t n_bases;
};

struct DevPwm {
    const double2 *tab2;      // see ms_fp64.hip header
    const int64_t *tab_off;   // [P] offset of motif p in tab2 (double2 units)
    const int32_t *width;     // [P]
    const double *max_raw;    // [P]
    const double *cutoff;     // [P]
    const double *raw_floor;  // [P] a raw (un-normalised) sum below this can never pass the hit test (-inf if unknown)
    int32_t P;
    uint32_t zero_bytes;      // byte offset of tab2's closing all-zero entry (what a column that adds nothing reads: score_window32)
    int32_t tab32;            // != 0: every entry of tab2 lies below 4 GB, byte offsets fit 32 bits
    const double *thresh;     // [P][4] {max_raw, cutoff, raw_floor, 0}: what the hit test reads, side by side
};

// What rescore_kernel needs to know about a field of a table group, in one 16-byte read (plan-specific: ms_pwmset::d_field_meta)
struct FieldMeta {
    int32_t motif;            // -1: empty field
    int32_t width;
    uint32_t tab_bytes;       // byte offset of the motif's table in DevPwm::tab2 (DevPwm::tab32)
    float floor32;            // the motif's raw-sum floor (DevPwm::raw_floor) rounded DOWN to a float: a sum below it is no hit
};

struct HitOut {
    uint64_t *keys;           // motif << (gbits+1) | coordinate << 1 | strand bit; coordinate = (region << pbits | position in
                              // the region) when pbits > 0 (gbits = rbits + pbits), else the global base position
    double *vals;             // normalised fp64 score
    unsigned long long *n_hits;
    uint64_t cap;
    int gbits;                // bits of the coordinate field
    int pbits;                // > 0: bits of the position inside a region (see keys)
};

// A hit list in BUCKETS of the lowest radix digit d0 = (key >> shift) & 255 (a predicted-size scan whose geometry passes bucket_gate,
// ms_scan_geom.h): bucket b owns the slots [base[b], base[b] + cap[b]) of HitOut::keys / vals, fill[b] counts the hits sent to it (beyond
// cap[b]: dropped, *overflow set -- the scan is run again with a plain list).  One table of kBucketTabWords words: base, cap, fill (256
// each), then [768] the end of the last bucket, then from kBucketHistAt on the digit counts of the radix passes that are left: place p counts
// the list's keys -- the hits the buckets hold and the all-ones keys that pad them -- by (key >> (shift + 8 + 8 p)) & 255 (BucketOut::hist;
// bucket_plan_kernel zeroes them, the bucketed fp64 stage adds the hits, fill_tail_buckets_kernel the padding keys, sort_hit_pairs_counted
// reads them in place of a histogram pass over the list).
constexpr int kOrderBuckets = 256;
constexpr int kBucketHistPlaces = 3;             // places counted at most: a scan whose passes cover more takes the histogram pass
constexpr size_t kBucketHistAt = 3 * kOrderBuckets + 8;
constexpr size_t kBucketTabWords = kBucketHistAt + (size_t) kBucketHistPlaces * 256;
struct BucketWeights {                   // per (sequence set, motif widths, key layout, L): the (motif, window start) pairs whose key falls into each bucket (bucket_weights, ms_scan_geom.h)
    unsigned long long w[kOrderBuckets];
    unsigned long long total;
};
struct BucketOut {
    const unsigned long long *base;
    const unsigned long long *cap;
    unsigned long long *fill;
    unsigned long long *overflow;
    int shift;
    unsigned long long *hist;            // [hist_places][256], or nullptr: not counted
    int hist_places;
};
struct BucketHitOut : HitOut {
    BucketOut B;
};

struct PfArgs {
    const uint32_t *codes;
    const uint32_t *nmask;
    int64_t n_bases;
    const uint4 *tables;
    const TileDesc *tiles;
    uint32_t lut_off16;       // start of the B-operand table in dynamic LDS (16-byte units)
    uint32_t stage_off16;     // start of the per-wave sequence staging
    uint32_t rare_off16;      // start of the per-wave parking space for candidate lanes' result registers
    uint32_t emit_off16;      // start of the per-wave PfEmit
    uint32_t onehot_off16;    // start of the per-wave one-hot arrays
    uint32_t rare_cap;        // entries of a wave's parking space; decoded when fewer than 8 (above 32 entries: a quarter) are free
    uint64_t *cand;           // candidate records; a wave reserves blocks of cand_block slots (unused slots are written as 0 = empty)
    unsigned long long *n_cand;   // slots reserved so far
    uint64_t cand_cap;
    uint32_t cand_block;      // >= 64
    uint64_t cand_static;     // slots [0, cand_static) are the launch's waves' own first blocks (wave w: [w, w + 1) * cand_block)
    int skip_alln;            // != 0: no motif of the plan reports a window made of non-ACGT bases only: such windows are dropped unseen
    unsigned int *chunk_counter;   // [LDS tiles][kPfCounters] words 64 bytes apart, zeroed: the units behind the waves' own first ones
    int use_counters;              // 0: a small input, one even unit per wave and no atomics
    int wave_passes;               // per-wave hand-out: passes of 64 window starts a wave takes per atomic (sized on the host: ms_scan_geom.cpp)
};

// ms_kernels.hip: the pre-filter
int prefilter_set_lds(bool wide, bool dense, size_t bytes);
int launch_prefilter(const PfArgs &A, bool wide, bool dense, int blocks_per_tile, int n_tiles, size_t lds_bytes, hipStream_t st);
// ms_fp64.hip: every window of the motifs the pre-filter cannot take; the pre-filter's candidates, short lists and long ones
// (rescore_carry_kernel: chunks of the list in motif order, the window carried along; one 1024-thread block per CU)
int launch_exact_all(const DevSeq &S, const DevPwm &Pw, const int32_t *motifs, int32_t n_motifs, int strand_mask,
                     const HitOut &H, hipStream_t st, int max_width);
int launch_rescore(const DevSeq &S, const DevPwm &Pw, const uint64_t *cand, const unsigned long long *n_cand, uint64_t n_static,
                   uint64_t cand_cap, const FieldMeta *field_meta, int strand_mask, const HitOut &H, int n_blocks, hipStream_t st);
int rescore_carry_set_lds();
int launch_rescore_carry(const DevSeq &S, const DevPwm &Pw, const uint64_t *cand, const unsigned long long *n_cand, uint64_t n_static,
                         uint64_t cand_cap, const FieldMeta *field_meta, int strand_mask, const HitOut &H, int n_blocks, hipStream_t st);
// ... the same with the hits flushed into the buckets of B
int launch_rescore_carry_bucketed(const DevSeq &S, const DevPwm &Pw, const uint64_t *cand, const unsigned long long *n_cand, uint64_t n_static,
                                  uint64_t cand_cap, const FieldMeta *field_meta, int strand_mask, const HitOut &H, const BucketOut &B, int n_blocks,
                                  hipStream_t st);
// ms_order.hip (its header says which key layout takes which of these).  launch_sort_fixup: after a sort over the key bits above
// kSortLowBits, runs of hits equal in those bits into full key order (in place)
int launch_fill_tail(uint64_t *keys, const unsigned long long *n_dev, uint64_t cap, hipStream_t st);
// the bucketed hit list's table for this scan (base, cap from the weights and n_pred; fill zeroed), queued in front of the fp64 stage, and its
// tail fill behind it: all-ones keys into the unused slots of every bucket and behind the last one, *n_hits = the hits the buckets hold
int launch_bucket_plan(const BucketWeights &bw, double mu, unsigned long long n_pred, unsigned long long need, unsigned long long cap_max,
                       unsigned long long *tab, hipStream_t st);
// (hist != nullptr: the all-ones keys are added to the digit counts of hist_places places, the last of them hist_last_bits wide)
int launch_fill_tail_buckets(uint64_t *keys, const unsigned long long *tab, uint64_t n_pred, unsigned long long *n_hits, unsigned long long *overflow,
                             unsigned long long *hist, int hist_places, int hist_last_bits, hipStream_t st);
// sort_hit_pairs (ms_internal.h) for a list whose digit counts are known: counts[p * 256 + d] keys have the digit d at the bits
// [begin_bit + 8 p, + 8) (cut at end_bit), for every place of [begin_bit, end_bit).  The radix passes run without the histogram pass over the
// list; *done = false and nothing queued where that cannot be had (another rocPRIM than the one this was written against, a configuration
// that does not sort eight bits a pass, too little temporary storage): the caller then takes sort_hit_pairs.  temp == nullptr: the bytes
// of temporary storage it takes into *temp_bytes (*done: whether it can run at all).
int sort_hit_pairs_counted(void *temp, size_t *temp_bytes, const uint64_t *keys_in, uint64_t *keys_out, const double *vals_in, double *vals_out,
                           size_t n, int begin_bit, int end_bit, const unsigned long long *counts, bool *done, hipStream_t stream);
int launch_sort_fixup(uint64_t *keys, double *vals, int64_t n, const unsigned long long *n_dev, hipStream_t st);
int launch_finalize(const uint64_t *keys, int64_t n, const unsigned long long *n_dev, int gbits, int rbits, int pbits, int32_t P, const DevSeq &S,
                    int64_t *seq_idx, int64_t *pos, int8_t *strand, int64_t *motif_first, unsigned long long *region_counts,
                    hipStream_t st);
// keys sorted over the bits [L, end_bit) -> every run of equal key >> L into full key order, decoded like launch_finalize's
// region form (pbits > 0), scores moved within d_score.  Runs the kernel cannot sort in LDS are listed in ovf_buf (order_overflow_bytes(n,
// run_cap) bytes; *ovf_n zero on entry, the number listed on exit) and sorted by a second launch, through tmp_keys / tmp_vals ([n] each).
size_t order_overflow_bytes(size_t n, int run_cap);
int launch_order_finalize(uint64_t *keys, double *score, int64_t n, const unsigned long long *n_dev, int L, int rbits, int pbits, int32_t P,
                          int64_t *seq_idx, int64_t *pos, int8_t *strand, int64_t *motif_first, unsigned long long *region_counts,
                          uint64_t *tmp_keys, double *tmp_vals, void *ovf_buf, size_t ovf_bytes, unsigned long long *ovf_n, int run_cap,
                          hipStream_t st);
// ms_regions.hip: counts only, from the unordered hit keys
constexpr int kCountsGateRatio = 50;            // the flag map is taken while P x R <= this x the hits expected (scan_counts_fast, ms_scan.hip)
constexpr int kSweepCountThreads = 256;         // threads (= hits) of a block of sweep_countonly_kernel (ms_sweep.hip)
constexpr int kSweepCountMaxMotifs = 65536;     // motifs whose site counters fit behind a counts-only sweep result's own counts
bool count_only_supported(int32_t P, int64_t R, int pbits);
size_t count_only_bitmap_words(int32_t P, int64_t R);
int launch_count_only(const uint64_t *keys, int64_t n, const unsigned long long *n_dev, int gbits, int pbits, int64_t R, int32_t P, uint32_t *bitmap,
                      unsigned long long *region_counts, unsigned long long *motif_hits, int64_t *motif_first, hipStream_t st);
// ms_result.hip: the compact copy-out of a result, which a scan that was asked for it queues itself (ms_scan.hip)
int launch_pack_hits(int64_t n, const unsigned long long *n_dev, const int64_t *seq_idx, const int64_t *pos, const int8_t *strand, uint64_t *coord,
                     unsigned int *bad, hipStream_t st, int shift = 0);

}  // namespace ms
