/*
 * motifscan_amd_debug.h -- host-only inspection of the integer pre-filter plan of
 * libmotifscan_amd.so.  NOT part of the drop-in surface (nothing in the reference corresponds
 * to it): it lets CPU tests prove that the quantised operand rows can never drop a window the
 * reference scorer (cscore.c:340-390) reports.  Needs no GPU.
 */
#ifndef MOTIFSCAN_AMD_DEBUG_H
#define MOTIFSCAN_AMD_DEBUG_H

#include "motifscan_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Build (and cache) the plan for a strand mask and an LDS budget in bytes; report its shape. */
int ms_debug_plan_dims(const ms_pwmset *pwms, int strand_mask, int64_t lds_budget, int32_t *n_fast,
                       int32_t *n_exact, int32_t *n_groups, int32_t *n_tiles);

/* The plan built by the last ms_debug_plan_dims call, decoded from the PHYSICAL fp6 operand image the kernel reads
 * (any pointer may be NULL).  A table group has 16 fields = the 16 result registers of a lane: with both strands scanned
 * field n = motif slot n >> 1, even n forward, odd n reverse; with one strand field n = motif slot n.
 *   group_fields [n_groups][16]  motif of the field, -1 = empty
 *   rows [n_groups][16][64 motif columns][4 bases] int16: what the product adds for that base at that column, in units
 *        of 1/8; a non-ACGT base adds nothing (its one-hot column is all zero)
 *   bias [n_groups][16]: the row's constant (stored in the last column of the row tile, which the kernel never clears)
 *   group_kb [n_groups]: k-blocks of 16 columns evaluated for the group's row tile
 *   exact_motifs [n_exact], tile_first_group [n_tiles + 1]
 * A window is a candidate for a field iff bias + the sum over its ACGT columns of rows[..][column][base] is >= 0. */
int ms_debug_plan_rows(const ms_pwmset *pwms, int32_t *group_fields, int16_t *rows, int32_t *bias, int32_t *group_kb,
                       int32_t *exact_motifs, int32_t *tile_first_group);

/* The host packer of ms_seqset_create_hostpacked alone (no device): codes [2 x ceil(n / 32)], nmask [ceil(n / 32)], blk2reg [(n + 63) / 64 + 1],
 * blkinfo [4 x that], n = offsets[n_seqs] -- the layout pack_kernel / blk2reg_kernel write on the device. */
int ms_debug_host_pack(const char *bases, const int64_t *offsets, int64_t n_seqs, uint32_t *codes, uint32_t *nmask, int32_t *blk2reg, int32_t *blkinfo);

/* The NUMA look-ups of ms_numa_bind_thread against a sysfs tree under `root` ("" = the machine's own; no device, no binding): the node of
 * PCI device `bdf` (-1 unknown), the number of CPUs of that node (0 unknown), the number of online nodes. */
int ms_debug_numa_probe(const char *root, const char *bdf, int32_t *node, int32_t *n_cpus, int32_t *n_nodes);

/* The host arithmetic behind a scan's bucketed hit list (the fp64 stage writes the hits of a long, predicted-size list in 256 buckets of the
 * radix digit at key bit low_bits, and the hit sort runs one pass fewer); no device.
 *   weights [256]: offsets != NULL -- computed from the set (offsets [n_seqs + 1], widths [n_pwms]) for the key layout (gbits coordinate bits,
 *       pbits of them the position in a region) and returned: the (motif, window start) pairs whose key falls into each bucket;
 *       offsets == NULL -- taken as given (n_pwms and n_regions then say how many motifs and regions the set has: the gate looks at the largest key).
 *   mu: expected hits; n_pred: slots of the list; cap_max: no bucket larger than this (UINT64_MAX: no limit).
 *   form: bit 0 predicted-size scan, bit 1 counts-only form, bit 2 the fp64 stage is rescore_carry_kernel alone, bit 3 the PWM set's sticky
 *       "a bucket overflowed once" flag; force: -1 the product's gate, 0 / 1 as MS_ORDER_BUCKETS; end_bit: key bits in all.
 *   *need: the sum over the buckets of (expected count + 6 sigma of a Poisson count + 1, rounded up); *gate: 1 if such a scan is bucketed;
 *   base, cap [256]: the buckets' places in the list (sum of cap <= n_pred). */
int ms_debug_bucket_plan(const int64_t *offsets, int64_t n_seqs, const int32_t *widths, int32_t n_pwms, int32_t gbits, int32_t pbits, int32_t end_bit,
                         int32_t low_bits, int64_t n_regions, uint64_t *weights, double mu, uint64_t n_pred, uint64_t cap_max, uint32_t form, int32_t force,
                         uint64_t *need, int32_t *gate, uint64_t *base, uint64_t *cap);

/* The layout of a scan's hit keys (motif << (gbits + 1) | coordinate << 1 | strand bit) for a sequence set of n_bases bases in n_seqs
 * regions, the longest of max_len bases, and n_pwms motifs -- the same arithmetic a scan runs before its first launch; no device.
 * coord_global != 0: as under MS_MEASURE=1 MS_HIT_COORD=global.  *gbits: coordinate bits.  *pbits > 0: the coordinate is
 * region << pbits | position in the region; *pbits == 0: it is the global base position (ms_scan_regions_once then looks the span up
 * by binary search).  A test learns from it which of the two forms a set takes by itself. */
int ms_debug_key_layout(int64_t n_bases, int64_t n_seqs, int64_t max_len, int32_t n_pwms, int32_t coord_global, int32_t *gbits, int32_t *pbits);

/* Free the current device's grow-only work buffers (candidate list, hit list, sort space), so a
 * test can force the "buffer too small -> grow -> run the pass again" path.  Needs a GPU. */
int ms_debug_release_scratch(void);

/* The candidate list between the two stages of a scan: one 64-bit record per window start and table group, g << 30 | group << 16 | flags,
 * bit n of the flags = field n of the group is a candidate at window start g (global base position); 0 = an empty slot.  Groups and fields
 * are numbered as ms_debug_plan_rows numbers them.  Both entries run ms_scan's exactly-sized form -- the same overrides, geometry, scratch
 * and its grow-and-run-again loop -- with a stop or a start point, and leave the set's size prediction as it was.  flags: as ms_scan's.
 * Need a GPU.
 *
 * ms_debug_scan_candidates queues the counter clear and the pre-filter of a scan of (pwms, seqs, strand_mask), waits, and copies the
 * first min(*n_slots, cap) slots to records (NULL: only the count); *n_slots = the slots the launch used: the waves' own first blocks and
 * the blocks they reserved after them (which wave reserves how many depends on the hand-out: the number may differ between two calls).
 * No fp64 stage runs and no result is built.  geom: the launch's geometry -- [0] the wide kernel, [1] the dense-candidate form,
 * [2] the hand-out's counters are used, [3] passes per unit, [4] blocks per LDS tile, [5] LDS tiles, [6] parking entries per wave,
 * [7] slots per candidate block, [8] slots of the waves' own first blocks, [9] windows of non-ACGT bases only are dropped unseen,
 * [10] window starts per pass (128 / 64), [11] records per chunk of the carried fp64 stage; [12..15] reserved, 0.
 *
 * ms_debug_scan_from_candidates is the same scan with the pre-filter's launch replaced by an upload of records[0 .. n) into the candidate
 * list (padded with empty slots up to the waves' own first blocks); the fp64 stage -- rescore_kernel or rescore_carry_kernel, as the
 * geometry has it --, the motifs on the all-fp64 path, ordering and finalize run as in any scan; *result is an ordinary ms_result.  A
 * flagged record must name a base of the set and a group of the plan (MS_ERR_INVALID otherwise); the same (g, group) twice, or a flag on
 * an empty field, is outside the contract. */
int ms_debug_scan_candidates(const ms_pwmset *pwms, const ms_seqset *seqs, int strand_mask, uint32_t flags, uint64_t *records, uint64_t cap,
                             uint64_t *n_slots, int64_t geom[16]);
int ms_debug_scan_from_candidates(const ms_pwmset *pwms, const ms_seqset *seqs, int strand_mask, uint32_t flags, const uint64_t *records, uint64_t n,
                                  ms_result **result);

/* ms_scan_variants (and ms_scan_alleles and ms_scan_alleles_best: the same knob) takes its variants in chunks (the per-(motif, tile) record counts of one chunk are bounded,
 * ms_scan_alleles_best's chunks bound its grids); n_variants > 0 sets the
 * chunk size for the calls that follow in this process, 0 gives it back to the library.  *previous (may be NULL) = the value before.
 * The result of a scan does not depend on it: a test proves that with a chunk of a few variants.  Needs no GPU. */
int ms_debug_varscan_chunk(int64_t n_variants, int64_t *previous);

/* The sizes at which ms_scan_variants and ms_scan_alleles change path, as constants of the build: out[0] the variants of one block's tile
 * of ms_scan_variants, out[1] the threads of that block (= the items of one round), out[2] the widest motif whose table it stages in LDS
 * (wider ones read it from HBM, in a second launch over the same grid); out[3], out[4], out[5] the same three of ms_scan_alleles.  Tests
 * size their boundary cases from here.  Needs no GPU. */
int ms_debug_varscan_dims(int32_t out[6]);

/* The sizes at which ms_scan_alleles_best changes path, as constants of the build: out[0] the variants of one block's tile (a thread per
 * variant); out[1] the window count -- both haplotypes of a cell together -- above which a cell that is not a single-base substitution
 * takes the wave path (a wave per haplotype); out[2] the widest motif whose table is staged in LDS (wider ones read it from HBM).  Tests
 * size their boundary cases from here.  Needs no GPU. */
int ms_debug_allelebest_dims(int32_t out[3]);

/* ms_scan_best cuts a region into segments of this many window starts (one wave each); a region of more than one segment goes through the
 * per-segment partials and their reduction.  A constant of the build: a test sizes a region of more than two segments with it.  Needs no GPU. */
int ms_debug_best_segment_windows(void);

/* ms_result_pair_spacing bins into an LDS histogram while 2 * max_dist + 1 is at most this, and adds to global memory directly above it.
 * A constant of the build: a test sits on both sides of it.  Needs no GPU. */
int ms_debug_pair_lds_bins(void);
/* ms_result_cooccurrence walks the regions in steps of this many (one LDS stage of bit words); a result of more regions than one step
 * may have its word range cut across blocks, whose partial sums are added atomically.  A constant of the build.  Needs no GPU. */
int ms_debug_cooc_chunk_regions(void);
/* A block of ms_result_pair_spacing uses its LDS histogram only while (partner hits) x (anchor hits of the block) <= this limit, so that
 * no 32-bit counter can overflow; above it the block adds to global memory.  The library's own limit is 2^32 - 1 (more than 4M partner
 * hits); limit > 0 sets it for the calls that follow in this process, so that a small case reaches the fallback, 0 gives it back to the
 * library.  *previous (may be NULL) = the value before.  The result does not depend on it.  Needs no GPU. */
int ms_debug_pair_lds_pair_limit(int64_t limit, int64_t *previous);

/* The sizes at which the plot-data kernels (ms_result_site_histogram, ms_result_rank_profile) change path, as constants of the build:
 * out[0] the widest histogram (bins) counted in LDS -- wider ones add to global memory directly; out[1] the hits of the fullest motif
 * per block of the histogram and rank-mark grids (several trips of a block's grid-stride loop); out[2] the most such blocks per motif, beyond
 * which the grid stays as it is and the loops run longer; out[3] the threads of the one block that prefix-counts a motif's rank words (more than 64 * out[3] regions: several words per
 * thread); out[4] the ranks per block of the profile; out[5] the smoothing halo either side (window 2 * out[5] + 1).  Tests take every
 * boundary size from here.  Needs no GPU. */
int ms_debug_plot_dims(int32_t out[6]);

/* The sizes at which the kernels either side of the scan change path (ms_seqset.hip, ms_background.hip, ms_pwmset.hip,
 * ms_annotation.hip), as constants of the build: out[0] the bases of one block's tile of the base count; out[1] the chromosomes of a
 * tile counted in LDS (later ones add to global memory); out[2] the candidates per block of the window filter; out[3] the bases per
 * block of the pack and extract kernels; out[4] the regions per block of ms_genes_nearest_tss; out[5] the genes per LDS tile of it;
 * out[6] the regions per block of ms_genes_promoter_overlap; out[7] the scores ms_score_ranks holds at once (its motifs go in batches
 * of out[7] / n_seqs, at least one).  Tests take every boundary size from here.  Needs no GPU. */
int ms_debug_genome_dims(int32_t out[8]);

/* The four device arrays of a built sequence set on the host, in the layout of ms_debug_host_pack (codes [2 x ceil(n / 32)], nmask
 * [ceil(n / 32)], blk2reg [(n + 63) / 64 + 1], blkinfo [4 x that]); any pointer may be NULL.  MS_ERR_INVALID for a set whose planes are
 * not on the device yet (a batch stream's upload-only set before its scan).  Needs a GPU. */
int ms_debug_seqset_planes(const ms_seqset *seqs, uint32_t *codes, uint32_t *nmask, int32_t *blk2reg, int32_t *blkinfo);

/* ms_score_ranks scores its motifs in batches of (budget / n_seqs, at least one): elems > 0 sets the budget for the calls that follow
 * in this process, so that a small case runs several batches, 0 gives it back to the library.  *previous (may be NULL) = the value
 * before.  The result does not depend on it: a test proves that with batches of one and of three motifs.  Needs no GPU. */
int ms_debug_score_rank_budget(int64_t elems, int64_t *previous);

/* The sizes at which ms_scan_score_histogram changes path, as constants of the build: out[0] the window starts per segment (a region of
 * more takes several); out[1] the widest motif whose table is staged in an LDS tile (wider ones read it from HBM); out[2] the LDS counter
 * slots per block (MS_SCOREHIST_MAX_BINS + 2); out[3] the window starts a block counts between two flushes of its LDS counters (a region
 * of more is counted by several blocks, or in several flushes).  Tests size their boundary cases from here.  Needs no GPU. */
int ms_debug_scorehist_dims(int32_t out[4]);

/* The path constants of ms_genome_apply_alleles and ms_liftmap_lift, as constants of the build: out[0] the output bases of one block of the
 * splice kernel; out[1] the applied variants (= alt pieces, each followed by a genome piece) a block stages in LDS -- a block whose bases
 * touch more searches them in global memory; out[2] the queries per block of the lift kernel; out[3] reserved, 0.  Tests size their boundary
 * cases from here.  Needs no GPU. */
int ms_debug_personal_dims(int32_t out[4]);
/* The stage times of the ms_genome_apply_alleles call that made the map, in ms: out[0] upload, alt packing and prep; out[1] order, status and
 * layout up to the copy of the new offsets; out[2] the host's part (the output genome's tables and block); out[3] the splice and the region hints. */
int ms_debug_liftmap_stage_ms(const ms_liftmap *m, double out[4]);

/* The path constants of ms_result_site_base_counts, as constants of the build: out[0] the threads of a block; out[1] the hits of one
 * block chunk (a motif of more hits takes several chunks, and beyond a fixed number of blocks several chunks per block); out[2] the
 * largest column pitch C = max_width + 2 * flank counted in LDS -- above it the counts go to global memory directly; out[3] the same
 * when dinuc is not asked for (equal to out[2]: one limit).  Tests size their boundary cases from here.  Needs no GPU. */
int ms_debug_sitestack_dims(int32_t out[4]);

/* The path constants of ms_result_site_signal, as constants of the build: out[0] the threads of a block; out[1] the sites of one block
 * chunk (a wave takes them 64 at a time; a motif of more sites takes several chunks); out[2] the columns of one panel -- a block holds
 * the sums of one panel in registers, 4 columns per lane, and a row of more columns (W + 2 * flank) takes several panels in the grid's z,
 * whose per-site sums are then added with 64-bit atomics instead of stored: the largest row of the one-panel form; out[3] the most blocks
 * in x, beyond which a block takes several chunks.  Tests size their boundary cases from here.  Needs no GPU. */
int ms_debug_sitesignal_dims(int32_t out[4]);

/* The path constants of ms_best_rank_sum and ms_best_count_passing, as constants of the build: out[0] the threads of a block; out[1] the
 * cells per block of the gather kernel; out[2] the sorted elements per block of the rank kernel (a group of more takes several blocks, each
 * with its own partial slot); out[3] the cells per block of the count kernel; out[4] the default element budget of a batch of motif rows;
 * out[5] the cutoffs a block counts between two flushes of its LDS counters; out[6] the largest group (cells per motif row) whose rows are
 * sorted by one segmented radix sort per batch -- a larger group takes one device radix sort per row; out[7] reserved, 0.  Tests size their
 * boundary cases from here.  Needs no GPU. */
int ms_debug_ranksum_dims(int32_t out[8]);
/* ms_best_rank_sum ranks its motif rows in batches of (budget / (na + nb), at least one): elems > 0 sets the budget for the calls that follow
 * in this process, 0 gives it back to the library.  *previous (may be NULL) = the value before.  The result does not depend on it.  Needs no GPU. */
int ms_debug_ranksum_budget(int64_t elems, int64_t *previous);

/* The sizes at which ms_scan_affinity changes path, as constants of the build (it walks as ms_scan_best does): out[0] the window starts per
 * segment (a region of more takes several, folded from partials); out[1] the widest motif whose table rides an LDS tile (wider ones read it
 * from HBM); out[2] the table entries (motif columns x 4) of one LDS tile -- a motif set of more starts a second tile; out[3] the waves
 * (= segments) per block; out[4] the strips of 64 window starts per segment; out[5] the bytes of a segment's partial; out[6], out[7]
 * reserved, 0.  Tests size their boundary cases from here.  Needs no GPU. */
int ms_debug_affinity_dims(int32_t out[8]);

/* The sizes of ms_affinity_expected_counts' walk, as constants of the build: out[0] the window starts per segment; out[1] the widest motif
 * it takes (MS_EXPECTED_MAX_WIDTH); out[2] the table entries (motif columns x 4) of one LDS tile -- a motif range of more starts a second
 * tile; out[3] the waves (= segments) per block; out[4] the strips of 64 window starts per segment; out[5] the bytes of LDS accumulator
 * per motif column; out[6] the default cap of the grid's x (blocks per tile: a block takes further groups of out[3] segments in a
 * grid-stride loop); out[7] reserved, 0.  Needs no GPU. */
int ms_debug_expected_dims(int32_t out[8]);

/* The cap of the grid's x for the ms_affinity_expected_counts calls that follow in this process; 0 gives it back to the library.  With a
 * cap of 1 or 2 a small case makes the grid-stride loop take several trips.  The result does not depend on it.  Needs no GPU. */
int ms_debug_expected_grid_cap(int32_t blocks);

/* The sizes at which ms_seqset_shuffle changes path, as constants of the build: out[0] the longest run handled by one lane and out[1] the
 * longest run handled by one wave in LDS -- equal, the mapping has no lane tier: every run of up to out[1] bases takes one wave, a longer
 * one takes one block with its keys in pooled global scratch; out[2] the bases per block of the stage that writes the mask plane, clears
 * the code words and finds the runs (the runs then set their code bits word by word); out[3] reserved, 0.  Tests size their boundary
 * cases from here.  Needs no GPU. */
int ms_debug_shuffle_dims(int32_t out[4]);
/* The stage times of the last ms_seqset_shuffle call on the calling thread's device, in ms: out[0] the mask plane, the cleared code words
 * and the run count, up to the host's read of it; out[1] the run list and the long runs' scratch layout; out[2] the shuffle kernels;
 * out[3] the region hints.  MS_ERR_INVALID before the first call. */
int ms_debug_shuffle_stage_ms(double out[4]);

/* The path constants of ms_seqset_kmer_counts / ms_genome_kmer_counts, as constants of the build: out[0] the threads of a block; out[1] the
 * bases of one block tile of the count pass; out[2] the largest k counted in a block table of LDS counters (lds_k) -- above it the counts go
 * to global memory directly; out[3] the most windows of a sequence whose codes are sorted in LDS for nseq (sort_windows) -- a longer
 * sequence sets bits in a bitmap in device scratch; out[4] the sequences per block of that sort tier (1: one block per sequence); out[5] the
 * default budget of a batch of bitmaps in MiB; out[6], out[7] reserved, 0.  Tests size their boundary cases from here.  Needs no GPU. */
int ms_debug_kmer_dims(int32_t out[8]);
/* The bitmaps of the long sequences of a k-mer count are taken in batches of (budget / bitmap bytes, at least one) sequences: bytes > 0 sets
 * the budget for the calls that follow in this process, 0 gives it back to the library.  *previous (may be NULL) = the value before.  The
 * result does not depend on it.  Needs no GPU. */
int ms_debug_kmer_bitmap_budget(int64_t bytes, int64_t *previous);
/* The path constants of the counts-only forms (MS_SCAN_COUNTS_ONLY's flag map, ms_regions.hip; a MS_STREAM_NO_HITS sweep span, ms_sweep.hip),
 * as constants of the build: out[0] the motifs the flag map's LDS histogram holds -- a set of more takes the ordered path; out[1] the threads
 * of a block of its three kernels (the per-motif prefix cuts the motifs into out[1] ranges of ceil(P / out[1])); out[2] the hit keys per block
 * while the grid may grow; out[3] the largest grid -- more than out[2] * out[3] keys take further trips of the blocks' loop; out[4] the gate:
 * the flag map is taken while motifs x regions <= out[4] x the hits expected (the true number on a set's first scan, the predicted one later);
 * out[5] the threads (= hits) of a block of the sweep's counting kernel; out[6] the most motifs a counts-only span takes; out[7] reserved, 0.
 * Tests size their boundary cases from here.  Needs no GPU. */
int ms_debug_counts_dims(int32_t out[8]);

/* The path constants of ms_pwmset_score_distribution, as constants of the build: out[0] the threads of a block of the global path's
 * kernels; out[1] the bins of one block tile of the global path; out[2] the largest C x n_bins (contexts x bins) the LDS path takes -- both
 * buffers of such a motif fit the 160 KiB of LDS of a gfx950 CU; out[3] the default work budget in MiB.  Tests size their boundary cases
 * from here.  Needs no GPU. */
int ms_debug_scoredist_dims(int32_t out[4]);
/* The motifs of a score distribution are taken in batches of (budget / (2 C n_bins 8), none: MS_ERR_NOMEM) motifs: bytes > 0 sets the
 * budget for the calls that follow in this process, 0 gives it back to the library.  *previous (may be NULL) = the value before.  The
 * result does not depend on it.  Needs no GPU. */
int ms_debug_scoredist_budget(int64_t bytes, int64_t *previous);
/* on != 0: the calls that follow in this process take the global path even where the LDS path applies; 0 gives the choice back to the
 * library.  *previous (may be NULL) = the value before.  The result does not depend on it.  Needs no GPU. */
int ms_debug_scoredist_force_global(int32_t on, int32_t *previous);

/* The path constants of ms_motifs_compare, as constants of the build: out[0] the threads of a block of its three kernels; out[1] the target
 * columns of one tile of the histogram kernel; out[2] the targets of one block of the alignment kernel; out[3] the default work budget
 * in MiB; out[4] the most queries of one batch; out[5] the most histogram tiles side by side in a grid (a block takes further tiles that
 * far apart); out[6] the largest W x bins of an LDS-resident tables variant: 0, there is none; out[7] reserved, 0.  Tests size their
 * boundary cases from here.  Needs no GPU. */
int ms_debug_compare_dims(int32_t out[8]);
/* The queries of a comparison are taken in batches whose tables fit a budget (a query whose tables do not fit alone: MS_ERR_NOMEM):
 * bytes > 0 sets the budget for the calls that follow in this process, 0 gives it back to the library.  *previous (may be NULL) = the
 * value before.  The result does not depend on it.  Needs no GPU. */
int ms_debug_compare_budget(int64_t bytes, int64_t *previous);
/* The null of one query as ms_motifs_compare builds it from the same inputs: H uint32 [Wq][bins], and tail, all tables of the query flat
 * in (start a ascending, length L ascending) order, L (bins - 1) + 1 doubles each.  Statuses as ms_motifs_compare's; also
 * MS_ERR_INVALID for a query outside [0, n_q), for n_t < 1 and for NULL outputs.  Needs a GPU. */
int ms_debug_compare_null(const double *q_values, const int32_t *q_widths, int32_t n_q, const double *t_values, const int32_t *t_widths,
                          int32_t n_t, int metric, int32_t bins, int orientations, int32_t query, uint32_t *H, double *tail);

/* The path constants of ms_scan_best_dimodels, as constants of the build: out[0] the threads of a block of its walk; out[1] the window
 * starts per segment of a region (one wave each; a region of more than one segment goes through the partials and their reduction);
 * out[2] the table entries of one LDS tile (a model of W columns takes 4 (4 W - 3): a run of consecutive scorable models shares a tile
 * while their entries fit); out[3] the width cap, the widest model whose table fits a tile alone (wider: MS_ERR_INVALID from
 * ms_dimodelset_create); out[4] the strips of 64 window starts a lane keeps in registers; out[5] the steps one packed word serves (a model
 * of more than out[5] + 1 columns reads further words per window); out[6], out[7] reserved, 0.  Tests size their boundary cases from
 * here.  Needs no GPU. */
int ms_debug_dimodel_dims(int32_t out[8]);

/* The path constants of ms_scan_best_bipartite, as constants of the build: out[0] the threads of a block of its walk; out[1] the window
 * starts per segment of a region (one wave each; a region of more than one segment goes through the partials, their reduction and the
 * gather of the winner's gap); out[2] the table entries of one LDS tile (a spec takes 4 (W_a + W_b): a run of consecutive scorable specs
 * shares a tile while their entries fit); out[3] the width cap of an element and out[4] the gap cap G (above either: MS_ERR_INVALID);
 * out[5] the halo strips of 64 window starts a wave sums behind its segment (64 out[5] >= out[3] + out[4]); out[6] the LDS bytes of a
 * block, the tile and the waves' rings; out[7] reserved, 0.  Tests size their boundary cases from here.  Needs no GPU. */
int ms_debug_bipartite_dims(int32_t out[8]);

/* A set as a batch stream's upload stage leaves it: ASCII and offsets in HBM, the planes still to be packed by its first scan.  The entry
 * points that read the planes directly (ms_seqset_kmer_counts, ms_seqset_shuffle, ms_seqset_packed_host) refuse it with MS_ERR_INVALID: this
 * is how a test gets one.  Every scan entry point takes it and packs it; free it with ms_seqset_free.  Needs a GPU. */
int ms_debug_seqset_upload_only(const char *bases, const int64_t *offsets, int64_t n_seqs, ms_seqset **out);

/* The 16 words that follow the code plane and the 16 that follow the mask plane of a built sequence set (a genome handle is one: cast it):
 * the kernels' window reads run into them, and every way of making a set leaves them zero.  MS_ERR_INVALID for a set whose planes are not
 * on the device yet.  Needs a GPU. */
int ms_debug_seqset_pad_words(const ms_seqset *seqs, uint32_t codes_pad[16], uint32_t nmask_pad[16]);

/* What a block holds when the library hands it out. Device working memory, result blocks and pinned host blocks are recycled, and a
 * recycled block still holds what the previous call left in it; a fresh one holds whatever the driver gives.  byte = 0..255: from now on
 * every block handed out in this process -- a device allocation, a block of the device cache on a hit and on a miss, a block of the pinned
 * host cache on a hit and on a miss -- is filled with that byte over its whole granted size before its caller sees it (device blocks: the
 * device is synchronised, filled and synchronised again, so the fill is complete on every stream).  byte = -1 (the default) turns it off:
 * the allocation paths then make no call they did not make before.  Anything else is MS_ERR_INVALID.  *previous (may be NULL) = the value
 * before.  No result depends on it: tests/test_gpu_recycled_memory.py proves that, entry point by entry point, with 0x00, 0xFF and 0xA5.
 * Set by this call only, never from the environment.  The call itself needs no GPU. */
int ms_debug_alloc_fill(int32_t byte, int32_t *previous);

/* Give every block of the calling thread's device cache (ms_device_pool_stats) back to the driver, so that the allocations that follow are
 * misses: a test that wants fresh memory AND recycled memory under ms_debug_alloc_fill gets both in a chosen order.  *bytes (may be
 * NULL) = the bytes released.  Blocks that handles own are not touched.  Needs a GPU. */
int ms_debug_pool_trim(uint64_t *bytes);

#ifdef __cplusplus
}
#endif
#endif
