/*
 * motifscan_amd.h -- C-ABI of the MI355X-native PWM scan path (libmotifscan_amd.so).
 *
 * Drop-in boundary for ONE hot path of shao-lab/MotifScan: the native scorer
 * motifscan/motif/cscore.c (module motifscan.motif.cscore) as used by
 * motifscan/scanner.py:125 (c_scan_motif) and motifscan/cli/motif.py:134 (c_score).
 * Plain C, plain pointers and sizes, no Python.h, no torch types.  Every entry point
 * returns an int status (MS_OK = 0) and never calls exit(); the message of the last
 * failure on the calling thread is ms_last_error().  All handles are re-entrant and
 * device-bound (no file-scope state like cscore.c:26-34).
 *
 * There is NO CPU fallback behind this interface: without a gfx950 device every
 * compute entry point fails with MS_ERR_RUNTIME.
 *
 * Reference interface each entry point replaces (paths relative to /root/reference):
 *
 *   ms_pwmset_create      convert_pwm + get_max_raw_score          cscore.c:36-79
 *                         (PWM list -> double[4][W], max_raw clamped at 0 per column,
 *                          cutoff defaults to 1 when no cutoffs are given, cscore.c:70-74)
 *   ms_seqset_create      convert_seq                              cscore.c:81-114
 *                         (ASCII -> base codes: A/a C/c G/g T/t, anything else "no
 *                          contribution"); here 2-bit codes + a 1-bit non-ACGT plane in HBM
 *   ms_seqset_from_device same, for ASCII that is already resident in device memory
 *   ms_genome_create /    Scanner._extract_seq -> Genome.fetch_sequence (pysam)   scanner.py:71-87,
 *   ms_seqset_from_genome   genome/__init__.py:117-135: packed genome resident in HBM, regions cut on device
 *   ms_genome_create_packed / ms_genome_packed_host / ms_pack_bases_host
 *                         Genome.__init__ -> pysam.FastaFile (genome/__init__.py:61-83): the FASTA is packed ONCE into a genome
 *                         file (motifscan_amd/genome.py) whose planes are uploaded as they are
 *   ms_genome_base_counts cal_bg_freq's per-chromosome A / C / G / T counts     genome/__init__.py:179-220
 *   ms_genome_window_filter / ms_randint_replay_host
 *                         Genome.random_sequences (genome/__init__.py:137-176): the seeded start draws replayed on the host, the
 *                         N filter + first-n_times compaction of the candidate windows on the device (motif --build's background)
 *   ms_genes_create / ms_genes_nearest_tss / ms_genes_promoter_overlap / ms_control_regions_replay_host
 *                         Genes (genome/annotation.py:32-54) as arrays; dis_to_nearest_gene, subset_by_location's overlap test and
 *                         generate_control_regions (region/utils.py:16-180): the walks over a chromosome's genes on the device,
 *                         the seeded randint / choice draws replayed on the host (cli/scan.py:60-79)
 *   ms_scan_sweep         the same extraction + scan for the windows of a fixed-stride sweep of one chromosome
 *                         (BASELINE configs[4]); every base is scored once instead of window / stride times
 *   ms_scan_regions_once  the same extraction + scan for region lists that overlap (peaks +- window/2, random controls:
 *                         cli/scan.py:43-48,76-86, region/utils.py:89-145): the union of the regions is scored once
 *   ms_scan               scan_motif / scan_motif_thread           cscore.c:317-476
 *                         (Python name c_scan_motif; "OOOII" = pwms, cutoffs, seqs, strand,
 *                          n_threads; n_threads has no meaning on the GPU and is not taken)
 *   ms_result_*           the list-of-lists result building         cscore.c:443-471
 *                         (per PWM: [seq_idx, pos, score, strand], order = seq asc, pos asc,
 *                          '+' (1) before '-' (2)), delivered as flat arrays + offsets
 *   ms_result_region_counts   the per-motif "number of regions with >= 1 site" that
 *                         motifscan/stats.py:29-31 derives from the nested site lists
 *                         (the only quantity the multi-GPU all-reduce needs)
 *   ms_result_dedup       _deduplicate_sites / deduplicate_motif_sites  scanner.py:156-193 (device)
 *   ms_result_site_tables the per-(motif, region) count / max score of write_sites_table  io/__init__.py:23-33
 *   ms_score              motif_score / motif_score_thread         cscore.c:174-302
 *                         (Python name c_score; "OOII")
 *   ms_score_ranks        c_score + the sort / rank pick of get_score_cutoffs   motif/__init__.py:378-401
 *   ms_dedup_hits         _deduplicate_sites / deduplicate_motif_sites  scanner.py:156-193
 *                         (host-side, on the sparse hit arrays)
 *   ms_stream_*           the same scan_motifs path (scanner.py:89-132) for region lists handed over in batches: host ASCII
 *                         in -> hit arrays in pinned host memory out, with the upload of batch i+2, the packing + scan of
 *                         batch i+1 and the copy-out of batch i overlapped per device (SURVEY.md 8(d) "pack + H2D + kernel +
 *                         D2H", 8(e) "double-buffered chunks"); ms_stream_submit_span does the same for the spans of a
 *                         host-streamed window sweep (BASELINE configs[4]: cli/scan.py:43-48 over a whole genome)
 *   ms_sweep_spans        the windows of a fixed-stride sweep over all chromosomes (Scanner._extract_seq per window,
 *                         scanner.py:71-87) cut into spans of bounded size, each with the global index of its first window
 *   ms_result_site_histogram  the distance histogram of plot_motif_sites_dist     plot.py:43-92 (the loop at :65-70)
 *                         (site centre - summit in bins of 10 bp; the counts only: the / n and the smoothing stay on the host)
 *   ms_result_rank_profile    the ranked fold-change profile of plot_motif_sites_enrich   plot.py:95-153 (the loop at :133-141)
 *                         and its smoothing, smooth() plot.py:34-40
 *   ms_result_from_hits   a result made of hit arrays that are on the host (the sites of a view that no longer owns its result)
 *   ms_scan_variants / ms_varscan_*
 *                         no reference counterpart: the windows of a resident genome that cover a single-base substitution, scored for
 *                         both alleles with the scan's own lines (cscore.c:336-390) -- the motif sites a variant creates or destroys
 *   ms_scan_alleles / ms_allelescan_*
 *                         the same for alleles of any length (multi-base, insertions, deletions): the windows of the ref and of the
 *                         spliced alt haplotype that the allele touches, each scored on its own haplotype
 *   ms_scan_alleles_best / ms_allelebest_*
 *                         no reference counterpart: the maximum of cscore.c:336-390 over the windows an allele touches, per haplotype --
 *                         the best-scoring window of every (motif, variant, haplotype) cell, the dense form of ms_scan_alleles
 *   ms_genome_apply_alleles / ms_liftmap_*
 *                         no reference counterpart: a whole variant set spliced into a NEW resident genome (a personal haplotype) that
 *                         every region-based entry point takes as it is, and the coordinate map between the two genomes
 *   ms_scan_best / ms_best_*
 *                         no reference counterpart: the maximum of cscore.c:336-390 over a region -- the best-scoring window of every
 *                         (motif, region) cell, the dense score matrix behind "max motif score per peak"
 *   ms_dimodelset_* / ms_scan_best_dimodels
 *                         no reference counterpart: the same best-site matrix for FIRST-ORDER models, whose column scores depend on the
 *                         base of the column before (dinucleotide weight matrices, first-order BaMMs, TFFMs) -- into the same ms_best handle
 *   ms_scan_best_bipartite / ms_best_gaps*
 *                         no reference counterpart: the best site of two half-sites of the set with a spacer of variable length in a
 *                         fixed relative orientation (nuclear-receptor repeats, p53, composite elements) -- into the same ms_best handle,
 *                         with the winner's gap as a fourth plane
 *   ms_result_cooccurrence   no reference counterpart: the motif x motif matrix of "regions that hold a site of both", reduced on the
 *                         device from the hit arrays a result holds (has-site bit rows, a tiled popcount product)
 *   ms_result_pair_spacing    no reference counterpart: for one anchor motif against every partner motif, the histogram of the
 *                         centre-to-centre distances of their sites in the same region by relative orientation (SpaMo-style spacing)
 *   ms_scan_score_histogram   c_score at EVERY window of a sequence set, counted per score bin: the exhaustive form of what
 *                         get_score_cutoffs samples (motif_score_thread, cscore.c:174-229; the sort and the rank reads of
 *                         motif/__init__.py:378-401) -- the score distribution behind exact cutoffs and empirical P-values
 *   ms_result_site_base_counts   no reference counterpart: how often A, C, G and T stand under each motif column (and the flanks) over a
 *                         result's sites, in the motif's orientation, with the adjacent-column dinucleotide counts -- the observed
 *                         count matrix of the sites found, reduced on the device from the hit arrays and the packed sequence
 *   ms_track_* / ms_result_site_signal
 *                         no reference counterpart: a per-base int32 track (cut counts, coverage, conservation in fixed point) resident
 *                         beside a sequence set, and its sums under each motif column and flank over a result's sites, per strand and
 *                         in the motif's orientation -- the footprint profile -- with per-site upstream / core / downstream sums
 *   ms_best_rank_sum      no reference counterpart: the rank-sum (Mann-Whitney / AUROC) comparison of two groups of regions by their best
 *                         score per motif, without a cutoff -- the exact integers 2U and the tie sum, from the matrices ms_scan_best left
 *                         on the device
 *   ms_best_count_passing no reference counterpart: the number of regions whose best score passes each of several cutoffs per motif --
 *                         what ms_result_region_counts gives for one ms_scan per cutoff, from ONE best-site scan
 *   ms_scan_affinity / ms_affinity_*
 *                         no reference counterpart: the sum of exp(raw window score) over ALL windows of a region -- total binding
 *                         affinity (TRAP, AME's avg / sum scoring) per (motif, region) cell, dense, without a hit per window;
 *                         ms_affinity_rank_sum ranks it as ms_best_rank_sum ranks the best score
 *   ms_affinity_expected_counts
 *                         no reference counterpart: the E-step of MEME-style expectation maximisation -- per motif column the A, C, G, T
 *                         weight under it over ALL windows, each weighted by its posterior probability of being the site (ZOOPS / OOPS);
 *                         the posterior-weighted counterpart of ms_result_site_base_counts, without a cutoff
 *   ms_seqset_shuffle / ms_seqset_packed_host
 *                         no reference counterpart: the input sequences shuffled on the device, keeping base composition or exact
 *                         dinucleotide counts per run of ACGT -- the composition-matched control set of AME / HOMER, as another sequence set
 *   ms_genome_kmer_counts / ms_seqset_kmer_counts
 *                         cal_bg_freq (genome/__init__.py:179-220) generalised from single bases to k-mers of up to 12 bases, over the
 *                         whole genome or a region set: the counts behind a Markov background of order k - 1 (FIMO's --bgfile, HOMER's
 *                         background).  nseq -- the sequences that hold a k-mer at least once, HOMER's way of counting a k-mer's
 *                         enrichment -- has no reference counterpart
 *   ms_pwmset_score_distribution
 *                         no reference counterpart: the ANALYTIC distribution of a window's score under a Markov background of order
 *                         0 .. 5 (FIMO / MOODS / TFM-Pvalue style P-values): from a matrix and a conditional table alone, without a
 *                         sequence -- the column-by-column convolution of the discretised score over the background's contexts
 *   ms_motifs_compare     no reference counterpart: two motif sets compared with each other, matrix against matrix (Tomtom) -- per pair
 *                         the best ungapped alignment in both orientations and its P-value under a null of the target set's own columns
 */
#ifndef MOTIFSCAN_AMD_H
#define MOTIFSCAN_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MS_OK            0
#define MS_ERR_INVALID   1   /* bad argument / shape           -> ValueError   */
#define MS_ERR_NOMEM     2   /* host or device allocation      -> MemoryError  */
#define MS_ERR_RUNTIME   3   /* HIP failure, no usable device  -> RuntimeError */
#define MS_ERR_INTERNAL  4   /* an invariant of the library's own plan does not hold -> RuntimeError */

#define MS_STRAND_FWD    1   /* same bit mask as cscore.c:319 */
#define MS_STRAND_REV    2
#define MS_STRAND_BOTH   3

/* ms_scan flags */
#define MS_SCAN_DEFAULT      0u
#define MS_SCAN_EXACT_ONLY   1u   /* skip the integer pre-filter: score every window in fp64 (validation) */
#define MS_SCAN_COUNTS_ONLY  2u   /* only what the enrichment statistics read of a region set (stats.py:27-31): n_hits, the per-motif site numbers
                                     (ms_result_motif_offsets) and the per-motif region counts -- the hits are counted unordered, no site array is
                                     made (the hit accessors of the result fail with MS_ERR_INVALID).  What cli/scan.py:81-89 needs of the control regions. */

typedef struct ms_pwmset ms_pwmset;
typedef struct ms_seqset ms_seqset;
typedef struct ms_result ms_result;
typedef struct ms_genome ms_genome;

/* Per-call measurements, filled by ms_scan (HIP events on the library's own stream). */
typedef struct ms_scan_stats {
    int64_t n_bases;            /* total bases in the sequence set                                   */
    int64_t n_windows;          /* sum_p sum_r max(L_r - W_p + 1, 0): exact unit count               */
    int64_t n_candidates;       /* windows x strands that passed the integer pre-filter              */
    int64_t n_hits;
    int32_t n_pwms;
    int32_t n_pwms_exact;       /* PWMs routed to the all-fp64 path (W > 63, max_raw <= 0, non-finite entries, a cutoff below the quantiser's floor) */
    int32_t n_tiles;            /* LDS tiles of pre-filter operand tables                            */
    int32_t n_passes;           /* 1, or 2 when a buffer had to grow and the scan was re-run         */
    double  ms_prefilter;       /* device time of the pre-filter kernel (dominant kernel)            */
    double  ms_exact;           /* fp64 kernels: candidate re-scoring + the motifs of the all-fp64 path */
    double  ms_sort;            /* ordering of the hit list                                          */
    double  ms_finalize;        /* coordinates, per-motif offsets, region counts                     */
    double  ms_total;           /* first launch -> last kernel done                                  */
    int64_t lds_bytes_read;     /* bytes the pre-filter reads from LDS (operand tables)              */
    int64_t hbm_bytes_algorithmic; /* codes + mask + offsets + PWMs + 16 B/hit + 8 B/PWM */
    double  pf_clock_mhz;       /* always 0 (reserved) */
    int64_t mfma_ops;           /* multiply-adds x 2 the pre-filter issues on the matrix cores (one-hot zeros and width padding included) */
    int64_t mfma_ops_algorithmic; /* 2 x windows x strands x W: the adds the reference performs */
    int32_t pf_engine;          /* 3: the fp6 x fp4 one-hot product on the matrix cores, candidates parked and decoded later; 4: the same with the flags decoded in place (chosen when the previous scan of the PWM set found many hits per row tile: p >= ~5e-4) */
    int32_t order_overflow_runs; /* runs of hits too long for the ordering's LDS sort, ordered by its global-memory form instead (0 on i.i.d. sequence) */
    int32_t order_bucketed;     /* 1: the fp64 stage wrote the hits in buckets of the lowest sorted radix digit and the hit sort ran one pass fewer (long hit lists of a PWM set's second and later scans); 0: the plain list */
    int32_t reserved0;          /* always 0 */
} ms_scan_stats;

const char *ms_last_error(void);
int ms_version(void);

/* Device selection is per calling thread (like hipSetDevice).  Handles remember their device. */
int ms_device_count(int *count);
int ms_set_device(int device);
int ms_device_name(char *buf, int buflen);
/* NUMA placement of the host side (no reference counterpart: the reference has one process and no device): binds the CALLING thread to the
 * CPUs of the NUMA node the calling thread's device hangs off (sysfs numa_node of its PCI address; sched_setaffinity), so that memory the
 * thread allocates afterwards -- pinned buffers included -- is node-local.  The batch stream's three threads do this by themselves where the
 * policy says so: MS_NUMA_BIND=0 never, =1 always, unset = on machines with more than one NUMA node and more than one visible GPU.
 * force != 0 overrides the policy.  *node = the node bound to, or -1 if nothing was done. */
int ms_numa_bind_thread(int force, int *node);
/* The calling thread's device keeps freed HBM blocks for reuse (hipMalloc / hipFree stall every stream of the device).
 * out[0] requests served from the cache, out[1] requests that went to the driver, out[2] blocks returned to the driver,
 * out[3] nanoseconds spent inside the driver for [1] and [2], out[4] bytes cached now, out[5] blocks cached now.
 * No reference counterpart (numpy owns the reference's memory). */
int ms_device_pool_stats(uint64_t out[6]);

/* ---- PWM set -------------------------------------------------------------------------- */
/* values: the P matrices concatenated, each row-major [4][width] (rows A,C,G,T).
 * cutoffs: P doubles or NULL (then every cutoff is 1, cscore.c:70-74). */
int ms_pwmset_create(const double *values, const int32_t *widths, const double *cutoffs,
                     int32_t n_pwms, ms_pwmset **out);
int ms_pwmset_set_cutoffs(ms_pwmset *pwms, const double *cutoffs);
int ms_pwmset_size(const ms_pwmset *pwms, int32_t *n_pwms);
int ms_pwmset_max_raw(const ms_pwmset *pwms, double *out /* [P] */);
void ms_pwmset_free(ms_pwmset *pwms);

/* ---- sequence set ---------------------------------------------------------------------- */
/* bases: the R sequences concatenated as ASCII; offsets[R+1] (offsets[0] = 0). Copies to the
 * device and packs there.  keep_ascii != 0 keeps the ASCII resident so ms_seqset_repack can
 * re-run the extraction/packing kernel (bench.py times it inside the step). */
int ms_seqset_create(const char *bases, const int64_t *offsets, int64_t n_seqs, int keep_ascii,
                     ms_seqset **out);
/* The same set with convert_seq done by n_threads HOST threads: the 2-bit codes, the non-ACGT mask and the region hints are made in pinned
 * staging memory and copied over -- no kernel runs, so building the set never waits for CUs a running scan holds (what the batch stream's
 * upload stage does under MS_STREAM_HOST_PACK).  bases is borrowed for the duration of the call. */
int ms_seqset_create_hostpacked(const char *bases, const int64_t *offsets, int64_t n_seqs, int n_threads, ms_seqset **out);
/* d_bases: device pointer to the concatenated ASCII (borrowed for the call); offsets on host. */
int ms_seqset_from_device(const void *d_bases, const int64_t *offsets, int64_t n_seqs,
                          ms_seqset **out);
int ms_seqset_repack(ms_seqset *seqs);
int ms_seqset_size(const ms_seqset *seqs, int64_t *n_seqs, int64_t *n_bases);
/* The two planes of a sequence set copied back to host buffers, in ms_genome_create_packed's layout (codes[2 * ceil(n / 32)],
 * nmask[ceil(n / 32)]): the counterpart of ms_genome_packed_host for a set -- how the bases of a set that was made on the device
 * (ms_seqset_shuffle, ms_seqset_from_genome) reach the host.  MS_ERR_INVALID for a set whose planes are not on the device yet (a batch
 * stream's upload-only set before its scan). */
int ms_seqset_packed_host(const ms_seqset *seqs, uint32_t *codes, uint32_t *nmask);
void ms_seqset_free(ms_seqset *seqs);

/* ---- shuffled control sequences -------------------------------------------------------------- */
/* A new set on the same device with the same offsets whose sequences are the input's, shuffled on the device: the composition-matched
 * control of AME / HOMER / the TRAP null, for sets that have no genomic control (FASTA input, personal genomes).  Every scan entry point
 * takes the result as it is.  A sequence is cut into its maximal runs of ACGT bases; a non-ACGT position stays where it is and every run
 * is shuffled on its own, so the count of valid windows of any width is unchanged.
 *   MS_SHUFFLE_MONO   the base composition of every run is kept
 *   MS_SHUFFLE_DINUC  every dinucleotide count and the first and last base of every run are kept
 * Sequence k of the set is shuffled as sequence r = seq_index_base + k: a shard of a set gets exactly the bytes the whole set would.
 *
 * THE RESULT IS SPECIFIED AS A FUNCTION and does not depend on the device mapping (motifscan_amd/shuffle.py restates it sequentially;
 * the device output equals it bit for bit).  All arithmetic is unsigned 64-bit with wrap-around.
 *   mix(x): x ^= x >> 30; x *= 0xbf58476d1ce4e5b9; x ^= x >> 27; x *= 0x94d049bb133111eb; x ^= x >> 31
 *   h(seed, r, x, y) = mix(mix(mix(mix(seed + 0x9e3779b97f4a7c15) + r) + x) + y)
 * With b the run's start, e its end and p a position, all relative to the sequence's first base, and s[p] the 2-bit code:
 *   mono   the output run is the run's bases ordered by the key (h(seed, r, b, p), p), ascending.
 *   dinuc  Altschul-Erickson with the arborescence drawn by Wilson's loop-erased walk (rejection takes ~n tries on poly-A and
 *          microsatellite runs).  Runs of fewer than 3 bases are copied.  Otherwise
 *          1. m[u][w] = the number of p in [b, e - 1) with s[p] = u, s[p + 1] = w;  f = s[e - 1].
 *          2. in_tree = {f}, draw counter d = 0.  For v = 0, 1, 2, 3 in order, unless v is in the tree or row m[v] is all zero: walk u = v;
 *             while u is not in the tree: tot = sum over w != u of m[u][w]; x = (h(seed, r, b, 2^62 | d) * tot) >> 64 (the high half of the
 *             128-bit product); d += 1; w = the first w != u in ascending order whose running sum of m[u][w] exceeds x; next[u] = w
 *             (overwriting); u = w.  Then walk again from v along next, marking vertices in the tree until one already is.
 *          3. For every u != f with a non-zero row the reserved edge is the largest p with s[p] = u, s[p + 1] = next[u].
 *          4. Order the edges p in [b, e - 1) by the key (s[p], reserved(p) ? 1 : 0, h(seed, r, b, p), p): the successors s[p + 1] in that
 *             order, grouped by s[p], are the four lists L_u -- each shuffled, its reserved successor last.
 *          5. out[b] = s[b]; then repeatedly cur = L_cur[ptr[cur]++], written out.  The walk uses every edge and ends on f.
 * The draw (h * tot) >> 64 is biased by less than tot / 2^64; that is part of the specification.  The loop-erased walk has no cap (a cap
 * would change the distribution); its expected length is at most the run's hitting time, a few hundred draws on (AC) x 100 G.
 *
 * MS_ERR_RUNTIME ("no CPU fallback") without a device, before anything else.  MS_ERR_INVALID: NULL handle or out, kind outside {1, 2},
 * flags != 0, seq_index_base < 0, a set whose planes are not on the device yet (a batch stream's upload-only set).  n_seqs = 0 and empty
 * sequences are valid.  Runs of more than ms_debug_shuffle_dims()[1] bases are sorted by one block each in pooled device scratch
 * (about 34 bytes per base of such runs for the call's duration; a chromosome-long run is correct but slow). */
#define MS_SHUFFLE_MONO  1   /* base composition of every ACGT run kept */
#define MS_SHUFFLE_DINUC 2   /* every dinucleotide count, first and last base of every ACGT run kept */
int ms_seqset_shuffle(const ms_seqset *seqs, int kind, uint64_t seed, int64_t seq_index_base, uint32_t flags /* 0 */, ms_seqset **out);

/* ---- resident genome + on-device region extraction ------------------------------------------ */
/* Replaces the per-region Genome.fetch_sequence (pysam) calls of Scanner._extract_seq
 * (scanner.py:71-87, genome/__init__.py:117-135): the genome is packed ONCE into HBM (2-bit codes +
 * non-ACGT plane), and a region list (chromosome index, 0-based half-open [start, end) already
 * clipped to the chromosome as scanner.py:81-83 does) is cut into a sequence set on the device. */
int ms_genome_create(const char *bases, const int64_t *chrom_offsets, int32_t n_chroms, ms_genome **out);
/* The genome from its packed form -- the two planes of the HBM layout: codes[2 * ceil(n / 32)] (2 bits per base, base i of a 32-base unit at
 * bits [2i, 2i + 2) of the unit's two words; a/A 0, c/C 1, g/G 2, t/T 3, anything else 0) and nmask[ceil(n / 32)] (bit i: base i is none of
 * those), the chromosomes back to back.  "Pack the FASTA once" (SURVEY.md N3): a genome file made by motifscan_amd/genome.py is uploaded as it
 * is, 0.375 B per base, with no ASCII and no pack kernel -- what replaces Genome.__init__ / pysam.FastaFile (genome/__init__.py:61-83) on the
 * measured path.  The planes are validated (MS_ERR_INVALID for a non-ACGT base with a non-zero code, or bits past the last base). */
int ms_genome_create_packed(const uint32_t *codes, const uint32_t *nmask, const int64_t *chrom_offsets, int32_t n_chroms, ms_genome **out);
/* The two planes of a resident genome copied back to host buffers of those sizes (to write the genome file). */
int ms_genome_packed_host(const ms_genome *genome, uint32_t *codes, uint32_t *nmask);
/* convert_seq (cscore.c:81-114) into the same two planes on n_threads HOST threads -- no device is touched: the genome-file builder.
 * (Marshalling only: there is still no CPU scan path.) */
int ms_pack_bases_host(const char *bases, int64_t n_bases, int n_threads, uint32_t *codes, uint32_t *nmask);
int ms_genome_size(const ms_genome *genome, int32_t *n_chroms, int64_t *n_bases);
void ms_genome_free(ms_genome *genome);
int ms_seqset_from_genome(const ms_genome *genome, const int32_t *chrom, const int64_t *start,
                          const int64_t *end, int64_t n_regions, ms_seqset **out);

/* ---- the genome-wide jobs of `motif --build` / `genome --install` (ms_background.hip) ------ */
/* cal_bg_freq (genome/__init__.py:179-220) per chromosome: counts[c][0..3] = the numbers of A, C, G, T of chromosome c in either
 * case (the reference's .upper() + count); N and every other non-ACGT byte count for nothing.  counts: host [n_chroms][4]. */
int ms_genome_base_counts(const ms_genome *genome, int64_t *counts);
/* The N filter of Genome.random_sequences (genome/__init__.py:137-176) over candidate windows [gstart[k], gstart[k] + length) in
 * GENOME coordinates (chromosome offset + start; each window must lie inside the genome), taken in attempt order k = 0, 1, ...:
 * a window is accepted when its count of N / n bytes is <= max_n.  That count is the window's non-ACGT bases (the nmask plane)
 * minus the entries of exc_pos (host, ascending genome positions of the non-ACGT bytes that are NOT N / n -- the IUPAC letters a
 * genome file keeps; PackedGenome.exc_pos) inside the window: a window holding an R but no N passes at max_n = 0.
 * taken_idx (host, >= n_want entries) receives the candidate indices of the FIRST n_want accepted windows in attempt order (a stable
 * compaction); *n_taken = min(n_want, accepted windows). */
int ms_genome_window_filter(const ms_genome *genome, const int64_t *gstart, int64_t n_cand, int32_t length, int32_t max_n,
                            const int64_t *exc_pos, int64_t n_exc, int64_t n_want, int64_t *taken_idx, int64_t *n_taken);
/* Host only, no device: n_att sequential calls of numpy's legacy RandomState.randint(high[k]) replayed from the raw 32-bit words
 * that the same state would give (np.random.randint(0, 2**32, dtype=np.uint32)), for 1 <= high[k] <= 2^32: with rng = high - 1,
 * rng == 0 consumes no word and returns 0; otherwise words w are taken in order until (w & mask) <= rng, mask = 2^bitlen(rng) - 1.
 * start[k] = the value drawn, words_used[k] = words consumed by calls 0 .. k.  Stops when the words run out: *n_done = calls
 * completed.  MS_ERR_INVALID for a high outside [1, 2^32] (numpy raises for high <= 0 and draws 64-bit words above 2^32). */
int ms_randint_replay_host(const uint32_t *words, int64_t n_words, const int64_t *high, int64_t n_att, int64_t *start,
                           int64_t *words_used, int64_t *n_done);

/* ---- gene annotation: control regions and promoter / distal subsets (ms_annotation.hip) ---- */
/* A gene table in the reference's order (genome/annotation.py:32-54, Genes._genes): chromosome c (indexed by first appearance in the
 * file) owns genes [chrom_offsets[c], chrom_offsets[c + 1]) of tss / strand (MS_STRAND_FWD '+', MS_STRAND_REV '-'), in FILE order.
 * Creating one touches no device; its device copy is made by the first call below, on the calling thread's device. */
typedef struct ms_genes ms_genes;
int ms_genes_create(const int64_t *chrom_offsets, int32_t n_chroms, const int64_t *tss, const int8_t *strand, ms_genes **out);
void ms_genes_free(ms_genes *genes);
/* dis_to_nearest_gene (region/utils.py:148-180) for n regions (chromosome index of the gene table, start): the reference's recurrence
 * over the chromosome's genes in file order -- m = cutoff; d = start - tss; |d| < m: m = d (SIGNED), target = gene -- so the first
 * accepted d <= 0 ends the walk, ties and |d| == cutoff are not accepted.  found[r] = 0 where the reference returns None (also for
 * chrom < 0, a chromosome index past the table and a chromosome without genes; distance[r] = 0 then); otherwise distance[r] = m, negated
 * for a target on the '-' strand (0 is a distance, not None).  Host arrays in the caller's order, regions in any chromosome order. */
int ms_genes_nearest_tss(const ms_genes *genes, const int32_t *chrom, const int64_t *start, int64_t n, int64_t cutoff,
                         int64_t *distance, uint8_t *found);
/* The overlap test of subset_by_location (region/utils.py:51-86): the promoters [tss - upstream, tss + downstream] ('+') /
 * [tss - downstream, tss + upstream] ('-') of the region's chromosome (Gene.promoter, genome/annotation.py:25-29), sorted as Python
 * sorts lists of pairs, searched with the literal binary search of overlap_with (region/utils.py:16-48).  overlap[r] = 1 / 0 (0 for a
 * chromosome without genes).  The sorted table of one (upstream, downstream) pair is kept in the handle until another is asked for. */
int ms_genes_promoter_overlap(const ms_genes *genes, int64_t upstream, int64_t downstream, const int32_t *chrom,
                              const int64_t *start, const int64_t *end, int64_t n, uint8_t *overlap);
/* Host only, no device: the draws of generate_control_regions (region/utils.py:112-145) for n_regions regions in order, replayed from
 * the raw 32-bit words Python's generator would give next (random.getrandbits(32 * n), least significant word first).  randint(a, b)
 * is a + _randbelow(b - a + 1), choice(seq) is seq[_randbelow(len(seq))], and _randbelow(n) takes words w until w >> (32 - bitlen(n))
 * is < n (n == 1 consumes words too).
 *   tss == NULL  the no-annotation path: n_random times randint(0, chrom_size[r] - length[r]) per region.
 *   otherwise    tss / strand are the gene table's arrays and region r's chromosome owns genes [gene_lo[r], gene_hi[r]): an empty
 *                range skips the region (nothing drawn, nothing written); distance[r] / found[r] are ms_genes_nearest_tss's, and
 *                !found[r] draws randint(10000, 100000) once, in front of the first choice; every attempt draws a gene and keeps
 *                start = tss + distance ('+') / tss - distance ('-') iff start >= 0 and start + length[r] <= chrom_size[r].
 * start_out[r * n_random + j] = the j-th start kept for region r; words_used[r] = words consumed by regions 0 .. r; attempts[r]
 * (may be NULL) = draws of a start / a gene made for region r.  *n_done = regions completed; *stop says why the replay ended and
 * *stop_words how many words the reference would have consumed by then:
 *   MS_REPLAY_DONE         every region is complete
 *   MS_REPLAY_WORDS        the words ran out inside region *n_done: call again for the regions from there with more words
 *                          (*stop_words = words_used of the last complete region)
 *   MS_REPLAY_ATTEMPTS     region *n_done made max_attempts attempts without keeping n_random starts (the reference never ends)
 *   MS_REPLAY_NO_SIZE      region *n_done has chrom_size == MS_REPLAY_SIZE_MISSING where the reference looks it up (KeyError)
 *   MS_REPLAY_EMPTY_RANGE  chrom_size - length < 0 (randint raises ValueError)      MS_REPLAY_WIDE  a width >= 2^32 (not replayed) */
#define MS_REPLAY_DONE         0
#define MS_REPLAY_WORDS        1
#define MS_REPLAY_ATTEMPTS     2
#define MS_REPLAY_NO_SIZE      3
#define MS_REPLAY_EMPTY_RANGE  4
#define MS_REPLAY_WIDE         5
#define MS_REPLAY_SIZE_MISSING INT64_MIN
int ms_control_regions_replay_host(const uint32_t *words, int64_t n_words, int64_t n_regions, const int64_t *chrom_size,
                                   const int64_t *length, const int64_t *gene_lo, const int64_t *gene_hi, const int64_t *distance,
                                   const uint8_t *found, const int64_t *tss, const int8_t *strand, int32_t n_random, int64_t max_attempts,
                                   int64_t *start_out, int64_t *words_used, int64_t *attempts, int64_t *n_done, int32_t *stop,
                                   int64_t *stop_words);

/* ---- scan (c_scan_motif) ---------------------------------------------------------------- */
int ms_scan(const ms_pwmset *pwms, const ms_seqset *seqs, int strand_mask, uint32_t flags,
            ms_result **out);
/* Window sweep: windows k = 0 .. n-1 = [begin + k*stride, begin + k*stride + window) of chromosome `chrom`, all inside
 * [begin, end) (n = (end - begin - window) / stride + 1).  The result is what ms_scan gives for those n windows as n
 * regions (seq_idx = k, pos relative to the window start, same order, same fp64 scores, region counts = windows with
 * a site) -- scanner.py:71-87 + cscore.c:336-390 per window -- but the span is scanned ONCE and every hit is handed to
 * the windows that contain all of its bases. */
int ms_scan_sweep(const ms_pwmset *pwms, const ms_genome *genome, int32_t chrom, int64_t begin, int64_t end,
                  int32_t window, int32_t stride, int strand_mask, uint32_t flags, ms_result **out);
/* Region lists that OVERLAP (peaks +- window/2 closer than the window; the random control set drawn around them:
 * cli/scan.py:43-48, 76-86): the same result as ms_seqset_from_genome + ms_scan over the n_regions regions (seq_idx =
 * index in the caller's list, any order, any overlap, empty regions allowed) -- but the union of the regions is scanned
 * ONCE and every hit is handed to each region that holds all of its bases.  stats.n_bases = bases actually scanned. */
int ms_scan_regions_once(const ms_pwmset *pwms, const ms_genome *genome, const int32_t *chrom, const int64_t *start,
                         const int64_t *end, int64_t n_regions, int strand_mask, uint32_t flags, ms_result **out);
int ms_result_num_hits(const ms_result *res, int64_t *n_hits);
int ms_result_motif_offsets(const ms_result *res, int64_t *out /* [P+1] */);
/* Copy the hit arrays to host buffers of length n_hits (any pointer may be NULL). */
int ms_result_hits(const ms_result *res, int64_t *seq_idx, int64_t *pos, double *score, int8_t *strand);
/* The same arrays in library-owned pinned host memory (one device-to-host copy at PCIe rate).  A result has ONE pinned buffer,
 * which this call shares with ms_result_hits_packed_host and ms_result_hits_packed12_host and which holds one form at a time: the
 * pointers stay valid until the result is freed, de-duplicated, or asked for a DIFFERENT form -- such a request overwrites the
 * buffer even when it is refused (MS_ERR_INVALID: a hit does not fit the form).  Call again to get the arrays back. */
int ms_result_hits_host(ms_result *res, const int64_t **seq_idx, const int64_t **pos, const double **score,
                        const int8_t **strand);
int ms_result_region_counts(const ms_result *res, int64_t *out /* [P] */);
/* Device pointer (int64[P]) of the same counts, for a device-side all-reduce; valid until free. */
int ms_result_region_counts_device(const ms_result *res, void **d_counts);
int ms_result_stats(const ms_result *res, ms_scan_stats *out);
/* De-duplicate overlapping sites on the device, in place (scanner.py:156-193: per motif, region and
 * strand, greedy left to right, the lower-scoring of two sites closer than the motif width is
 * dropped, a tie keeps the earlier one).  Order and per-motif region counts are unaffected. */
int ms_result_dedup(ms_result *res, const ms_pwmset *pwms);
/* Per (motif, region): number of sites and maximum score (NaN where there is none) -- the two
 * aggregates the reference's site tables are made of (io/__init__.py:23-33).  Host buffers [P][R]. */
int ms_result_site_tables(const ms_result *res, int32_t *n_sites, double *max_score);
void ms_result_free(ms_result *res);

/* ---- single-base substitutions on a resident genome: motif sites gained and lost (ms_variants.hip) ---------- */
/* Variant v = (chromosome index chrom[v], 0-based position pos[v] on it, alt byte alt[v]); duplicates and any order are allowed, an alt
 * equal to the reference base is scored like any other.  For motif m of width W the windows that matter start at
 * s in [max(0, x - W + 1), min(x, L_c - W)] (none when L_c < W; a window never crosses a chromosome boundary).  For each of them and each
 * strand of strand_mask two normalised scores are computed exactly as ms_scan computes them (cscore.c:336-390: columns in order, forward
 * M[b][c], reverse M[3 - b][W - 1 - c], a non-ACGT base adds nothing, raw / max_raw, hit iff score - cutoff >= -1e-10): score_ref on the
 * genome as it is, score_alt with base x replaced by the alt byte converted as convert_seq converts it (AaCcGgTt, anything else "no
 * contribution": cscore.c:81-114).  A RECORD exists for every (motif, variant, s, strand) of which at least one allele passes: variant =
 * index in the caller's arrays, start = s, strand 1 / 2, both scores whatever their value, state bit 0 = ref passes, bit 1 = alt passes
 * (1 lost, 2 gained, 3 kept).  Order: motif, variant index, start ascending, '+' before '-'; the same bytes on every run.  No record is
 * ever dropped, however many there are.  The handle is device-bound (the genome's device).
 * MS_ERR_INVALID: a chromosome index outside the genome, pos outside [0, L_c), a strand mask outside 1..3, flags != 0.  n_variants = 0 is
 * valid and gives an empty result. */
typedef struct ms_varscan ms_varscan;
int  ms_scan_variants(const ms_pwmset *pwms, const ms_genome *genome, const int32_t *chrom, const int64_t *pos, const char *alt,
                      int64_t n_variants, int strand_mask, uint32_t flags /* 0 */, ms_varscan **out);
int  ms_varscan_num_sites(const ms_varscan *vs, int64_t *n);
int  ms_varscan_motif_offsets(const ms_varscan *vs, int64_t *out /* [P+1] */);
/* Copy the record arrays to host buffers of length n (any pointer may be NULL). */
int  ms_varscan_sites(const ms_varscan *vs, int64_t *variant, int64_t *start, int8_t *strand, double *score_ref, double *score_alt,
                      uint8_t *state);
/* The base the genome holds at every variant: 0..3 = A C G T, -1 = non-ACGT (to check a VCF's REF column against). */
int  ms_varscan_ref_codes(const ms_varscan *vs, int8_t *out /* [V] */);
/* gained[m] / lost[m] = input variants (duplicates count apiece) with at least one record of motif m whose state is 2 / 1; counted on
 * the device, like ms_result_region_counts.  Either pointer may be NULL. */
int  ms_varscan_motif_counts(const ms_varscan *vs, int64_t *gained /* [P] */, int64_t *lost /* [P] */);
/* Device time of the call that made the result: upload of the variants -> last kernel done (HIP events on the library's stream). */
int  ms_varscan_device_ms(const ms_varscan *vs, double *ms);
void ms_varscan_free(ms_varscan *vs);

/* ---- alleles of any length on a resident genome: substitutions, multi-base alleles, insertions, deletions (ms_alleles.hip) ---------- */
/* Variant v = (chromosome index chrom[v], 0-based x = pos[v], r = ref_len[v], alt = alt_bases[alt_offsets[v] .. alt_offsets[v + 1]) of
 * a bytes): the r >= 0 reference bases [x, x + r) of the chromosome (length L) are replaced by the a >= 0 alt bytes.  The REF haplotype is
 * the chromosome as it is; the ALT haplotype is chrom[0:x] + alt + chrom[x + r:], of length L' = L - r + a.  Alt bytes are converted as
 * convert_seq converts them (AaCcGgTt, anything else "no contribution": cscore.c:81-114), as in ms_scan_variants.
 * Affected windows of a motif of width W: on the ref haplotype the starts s in [max(0, x - W + 1), min(x + r - 1, L - W)]; on the alt
 * haplotype, in ALT-HAPLOTYPE coordinates, the starts t in [max(0, x - W + 1), min(x + a - 1, L' - W)].  ONE formula covers an empty
 * allele: with r = 0 (a = 0) the range is exactly the windows that straddle the junction between x - 1 and x, and it is empty for W = 1.
 * A haplotype shorter than W has no windows.  Every affected window is scored as ms_scan scores it (cscore.c:336-390: columns in order,
 * forward M[b][c], reverse M[3 - b][W - 1 - c] at the same step, +0.0 for a base that adds nothing, raw / max_raw, hit iff
 * score - cutoff >= -1e-10).  A RECORD (variant, allele, start, strand, score) exists for every affected window and strand of strand_mask
 * that passes: variant = index in the caller's arrays, allele 0 = ref / 1 = alt, start in THAT haplotype's coordinates (for allele 1 and
 * start >= x + a the reference coordinate is start - a + r), strand 1 / 2.  Order: motif, variant index, allele (ref first), start
 * ascending, '+' before '-'; the same bytes on every run; no record is ever dropped; duplicates and any input order are allowed.
 * gained[m] / lost[m] (counted on the device in the count pass) = input variants with at least one alt record and no ref record /
 * at least one ref record and no alt record of motif m.  This classifies VARIANTS, not positions: windows of two haplotypes of different
 * lengths have no canonical pairing, so -- unlike ms_varscan_motif_counts, which counts variants with a gained / lost WINDOW -- a variant
 * that destroys one site of a motif and creates another of the same motif counts as neither here.
 * With ref_bases (the REF strings concatenated, sum of ref_len bytes) every REF is compared with the genome at [x, x + r), ignoring case;
 * a non-ACGT genome base matches any letter that is not A, C, G or T.  ms_allelescan_ref_mismatch gives 1 per variant that differs, and
 * 0 for every variant when ref_bases was NULL.
 * MS_ERR_INVALID: a chromosome index outside the genome; x outside [0, L], r < 0 or x + r > L; r + a = 0; alt_offsets that do not start at
 * 0 or decrease; an allele (r or a) longer than MS_ALLELE_MAX_LEN; a strand mask outside 1..3; flags != 0; NULL handles.  n_variants = 0
 * is valid and gives an empty result.  Without a device: MS_ERR_RUNTIME ("no CPU fallback") before anything else. */
#define MS_ALLELE_MAX_LEN 65536
typedef struct ms_allelescan ms_allelescan;
int  ms_scan_alleles(const ms_pwmset *pwms, const ms_genome *genome, const int32_t *chrom, const int64_t *pos, const int32_t *ref_len,
                     const char *alt_bases, const int64_t *alt_offsets /* [V+1] */, const char *ref_bases /* or NULL */,
                     int64_t n_variants, int strand_mask, uint32_t flags /* 0 */, ms_allelescan **out);
int  ms_allelescan_num_sites(const ms_allelescan *as, int64_t *n);
int  ms_allelescan_motif_offsets(const ms_allelescan *as, int64_t *out /* [P+1] */);
/* Copy the record arrays to host buffers of length n (any pointer may be NULL). */
int  ms_allelescan_sites(const ms_allelescan *as, int64_t *variant, uint8_t *allele, int64_t *start, int8_t *strand, double *score);
int  ms_allelescan_motif_counts(const ms_allelescan *as, int64_t *gained /* [P] */, int64_t *lost /* [P] */);
int  ms_allelescan_ref_mismatch(const ms_allelescan *as, uint8_t *out /* [V] */);
/* Device time of the call that made the result: upload of the variants -> last kernel done. */
int  ms_allelescan_device_ms(const ms_allelescan *as, double *ms);
void ms_allelescan_free(ms_allelescan *as);

/* ---- the best-scoring window of every (motif, variant, haplotype) cell: ms_scan_alleles without a cutoff, dense (ms_allelebest.hip) ---------- */
/* The variant arguments, their validation, the alt-byte conversion, the REF check and the MS_ERR_* cases are ms_scan_alleles's, word for word;
 * so are the affected windows of motif m (width W): ref-haplotype starts s in [max(0, x - W + 1), min(x + r - 1, L - W)] and alt-haplotype
 * starts t in [max(0, x - W + 1), min(x + a - 1, L' - W)], the empty-allele and W = 1 cases included.  Every window is scored as ms_scan scores
 * it (columns in order, forward M[b][c], reverse M[3 - b][W - 1 - c] at the same step, +0.0 for a base that adds nothing, raw / max_raw as one
 * IEEE fp64 divide).  The cutoffs of the PWM set are not read.
 * The BEST SITE of (m, v, haplotype) follows ms_scan_best's rule over that haplotype's affected windows: start ascending, '+' before '-',
 * from best = -inf, a window replacing the best iff score > best -- NaN and -inf never win, ties keep the earlier window.  Per cell and
 * haplotype: score (double), offset (int32) = winning start - x in that haplotype's own coordinates, in [-(W - 1), max(r, a) - 1], and strand
 * (int8, 1 or 2).  A cell without a winner -- no affected window, a haplotype shorter than W, -inf in every window -- holds (NaN, 0, 0):
 * strand == 0 is the marker.  So does every cell of an UNSCORABLE motif (ms_scan_best's definition: max_raw not a finite number > 0, or a
 * NaN or +inf entry).  The bytes of all six arrays are the same on every run and do not depend on the variant chunking
 * (ms_debug_varscan_chunk).  MS_ERR_NOMEM, with nothing launched, when the 26 bytes x n_pwms x n_variants do not fit the device.
 * n_variants = 0 is valid and gives an empty result.  Without a device: MS_ERR_RUNTIME ("no CPU fallback") before anything else. */
typedef struct ms_allelebest ms_allelebest;
int  ms_scan_alleles_best(const ms_pwmset *pwms, const ms_genome *genome, const int32_t *chrom, const int64_t *pos, const int32_t *ref_len,
                          const char *alt_bases, const int64_t *alt_offsets /* [V+1] */, const char *ref_bases /* or NULL */,
                          int64_t n_variants, int strand_mask, uint32_t flags /* 0 */, ms_allelebest **out);
int  ms_allelebest_shape(const ms_allelebest *b, int32_t *n_pwms, int64_t *n_variants);
/* Motifs m0 <= m < m1 into host buffers [(m1 - m0)][V] row-major; any pointer may be NULL.  MS_ERR_INVALID for m0 < 0, m1 > n_pwms, m0 > m1. */
int  ms_allelebest_sites(const ms_allelebest *b, int32_t m0, int32_t m1, double *score_ref, int32_t *offset_ref, int8_t *strand_ref,
                         double *score_alt, int32_t *offset_alt, int8_t *strand_alt);
/* Device pointers of the full [n_pwms][V] arrays, valid until free; any pointer may be NULL. */
int  ms_allelebest_sites_device(const ms_allelebest *b, void **d_score_ref, void **d_offset_ref, void **d_strand_ref, void **d_score_alt,
                                void **d_offset_alt, void **d_strand_alt);
/* 1 per variant whose REF differs from the genome (ms_allelescan_ref_mismatch's rule), 0 for every variant when ref_bases was NULL. */
int  ms_allelebest_ref_mismatch(const ms_allelebest *b, uint8_t *out /* [V] */);
/* Device time of the call that made the result: upload of the variants -> last kernel done. */
int  ms_allelebest_device_ms(const ms_allelebest *b, double *ms);
void ms_allelebest_free(ms_allelebest *b);

/* ---- a personal haplotype: a variant set applied to a resident genome, and the map between the two (ms_personal.hip) ---------- */
/* The variant arguments, their validation, the alt-byte conversion, the REF check and the MS_ERR_INVALID cases are ms_scan_alleles's, word
 * for word (x in [0, L], r + a > 0, MS_ALLELE_MAX_LEN, the REF rule); flags other than MS_APPLY_SKIP_MISMATCH are MS_ERR_INVALID.  Without
 * a device: MS_ERR_RUNTIME ("no CPU fallback") before anything else.  MS_ERR_NOMEM when the new planes do not fit the device (the splice is
 * not launched then).
 * WHICH VARIANTS ARE APPLIED.  With MS_APPLY_SKIP_MISMATCH and ref_bases a variant whose REF differs from the genome gets status 2 and
 * takes no further part (without the flag it is applied like any other; ms_liftmap_ref_mismatch names it either way).  The rest are ordered by
 * (chromosome, x, index in the caller's arrays).  Variant v is skipped for overlap (status 0) iff some variant u of its chromosome EARLIER
 * in that order has x_u + r_u > x_v -- whether u is itself applied or not: the running maximum of the ends in front of v exceeds x_v.  Every
 * other variant is applied (status 1).  So: a duplicate of a substitution is skipped; an insertion (r = 0) at x does not block a later
 * variant at x; several insertions at one point are all applied, in input-index order; and, the rule being a max-scan (parallel) and NOT
 * the sequential greedy rule of consensus tools, a variant that overlaps a skipped one is skipped too.  The input order does not matter
 * beyond the index tie-break.
 * THE OUTPUT GENOME has the same number of chromosomes; chromosome c is the reference chromosome with [x, x + r) of every applied variant
 * replaced by its alt bases, of length L'_c = L_c + sum(a - r) (0 is allowed).  It is a complete ms_genome, independent of the input genome
 * and of the map: its planes are exactly what ms_pack_bases_host makes of the spliced ASCII (a non-ACGT alt byte is a mask bit with code
 * 0, bits past the last base are zero), with the region hints and host tables of any other genome, the same bytes on every run.
 * n_variants = 0 gives a copy.  Positions and length sums are 64-bit throughout.
 * THE LIFT MAP.  Per chromosome, with its applied variants in order (x_i, r_i, a_i) and x'_i = x_i + sum_{j < i} (a_j - r_j):
 *   MS_LIFT_REF_TO_ALT, p in [0, L_c]:  x_i <= p < x_i + r_i for some i -> x'_i + min(p - x_i, a_i), inside = 1; otherwise
 *       p + sum(a_j - r_j) over the applied j with x_j + r_j <= p, inside = 0 (a reference base at an insertion point lies BEHIND the
 *       inserted bases);
 *   MS_LIFT_ALT_TO_REF, q in [0, L'_c]: x'_i <= q < x'_i + a_i -> x_i + min(q - x'_i, r_i), inside = 1 (AlleleSites.ref_start's convention);
 *       otherwise q - sum(a_j - r_j) over the applied j with x'_j + a_j <= q.
 * Both are non-decreasing and map the chromosome's end to the chromosome's end.  A chromosome index or a position outside those ranges is
 * MS_ERR_INVALID.  Host arrays in and out; the queries run on the device.  The map owns its device arrays and outlives both genomes. */
#define MS_APPLY_SKIP_MISMATCH 1u
#define MS_LIFT_REF_TO_ALT 0
#define MS_LIFT_ALT_TO_REF 1
typedef struct ms_liftmap ms_liftmap;
int  ms_genome_apply_alleles(const ms_genome *genome, const int32_t *chrom, const int64_t *pos, const int32_t *ref_len,
                             const char *alt_bases, const int64_t *alt_offsets /* [V+1] */, const char *ref_bases /* or NULL */,
                             int64_t n_variants, uint32_t flags, ms_genome **out, ms_liftmap **map /* may be NULL */);
int  ms_liftmap_shape(const ms_liftmap *m, int32_t *n_chroms, int64_t *n_variants, int64_t *n_applied);
int  ms_liftmap_status(const ms_liftmap *m, uint8_t *status /* [V] */);          /* 1 applied, 0 skipped: overlap, 2 skipped: REF mismatch */
int  ms_liftmap_ref_mismatch(const ms_liftmap *m, uint8_t *out /* [V] */);
int  ms_liftmap_chrom_sizes(const ms_liftmap *m, int64_t *ref_len /* [C] */, int64_t *alt_len /* [C] */);
int  ms_liftmap_lift(const ms_liftmap *m, int direction, const int32_t *chrom, const int64_t *pos, int64_t n,
                     int64_t *out_pos, uint8_t *inside /* may be NULL */);
/* Device time of the call that made the map: first launch -> last kernel done (the host's sizing of the output in between included). */
int  ms_liftmap_device_ms(const ms_liftmap *m, double *ms);
void ms_liftmap_free(ms_liftmap *m);

/* ---- the best-scoring window of every (motif, region) cell: the dense motif x region matrix (ms_best.hip) ---------- */
/* For motif m of width W and region r of length L, over the window starts pos = 0 .. L - W and the strands of strand_mask: score(pos, strand)
 * is the normalised score exactly as ms_scan computes it (cscore.c:336-390: columns in order, forward M[b][c], reverse M[3 - b][W - 1 - c]
 * at the same step, a non-ACGT base adds nothing, raw / max_raw as an IEEE fp64 divide).  The BEST SITE of the cell is found by walking the
 * windows in the reference's order -- pos ascending, '+' before '-' -- from best = -inf, a window replacing the best iff score > best: NaN
 * and -inf never win, ties keep the earlier window.  Per cell: score (double), pos (int32, relative to the region start), strand (int8,
 * 1 or 2).  A cell without a winner -- L < W, an -inf entry in every window -- holds score = NaN, pos = -1, strand = 0, and so does every
 * cell of an UNSCORABLE motif: max_raw not a finite number > 0, or an entry that is NaN or +inf (the reference never reports a site of such
 * a motif either).  Entries of -inf are ordinary: the window's raw sum is -inf and it never wins.  This is what ms_scan with a cutoff
 * of -1e30 gives as the first hit of the greatest score per cell -- without making a hit per window.  The cutoffs of the PWM set are not read.
 * The bytes of all three arrays are the same on every run.  The handle is bound to the sequence set's device.  There is no "handles on
 * different devices" error: a PWM set is not bound to a device -- its device copies are made on, or moved to, the sequence set's device by
 * the call, exactly as in ms_scan -- so no pair of handles can disagree.  Sets cut from a resident genome (ms_seqset_from_genome) are
 * sequence sets like any other.  Work memory: a region of more than ms_debug_best_segment_windows() bases costs 16 bytes per (motif, segment)
 * for the duration of the call (a 250 Mbase chromosome handed in as ONE region x 579 motifs: 4.5 GB), regions of one segment nothing.
 * MS_ERR_INVALID: NULL handles, a strand mask outside 1..3, flags != 0, a region of 2^31 bases or more (pos is 32-bit).  MS_ERR_NOMEM: the
 * 13 bytes per cell do not fit the device (nothing has been launched then).  n_seqs = 0 is valid and gives an empty result.  Without a
 * device: MS_ERR_RUNTIME ("no CPU fallback") before anything else. */
typedef struct ms_best ms_best;
int  ms_scan_best(const ms_pwmset *pwms, const ms_seqset *seqs, int strand_mask, uint32_t flags /* 0 */, ms_best **out);
int  ms_best_shape(const ms_best *b, int32_t *n_pwms, int64_t *n_seqs);
/* Motifs m0 <= m < m1 into host buffers [(m1 - m0)][n_seqs] row-major; any pointer may be NULL.  MS_ERR_INVALID for m0 < 0, m1 > n_pwms, m0 > m1. */
int  ms_best_sites(const ms_best *b, int32_t m0, int32_t m1, double *score, int32_t *pos, int8_t *strand);
/* Device pointers of the full [n_pwms][n_seqs] arrays, valid until free (for a consumer that stays on the device); any pointer may be NULL. */
int  ms_best_sites_device(const ms_best *b, void **d_score, void **d_pos, void **d_strand);
/* Device time of the call that made the result: first launch -> last kernel done (HIP events on the library's stream). */
int  ms_best_device_ms(const ms_best *b, double *ms);
void ms_best_free(ms_best *b);

/* ---- first-order models: the best-scoring window of every (model, region) cell (ms_dimodel.hip) ---------------------- */
/* A FIRST-ORDER MODEL of width W >= 1 is values[W][16] of fp64, bases coded A, C, G, T = 0 .. 3.  Row 0 holds start[b] = values[0][b] for
 * b = 0 .. 3 (its entries 4 .. 15 are never read); row j >= 1 holds trans[j][4 a + b], the score of base b at column j given base a at
 * column j - 1.  For a window with the bases x_0 .. x_{W-1}, all of them ACGT (lower case included, as everywhere):
 *     forward raw sum   S+ = 0.0; S+ += start[x_0]; then S+ += trans[j][4 x_{j-1} + x_j] for j = 1, .., W - 1 in that order;
 *     reverse raw sum   with y_j = 3 - x_{W-1-j}, the window read on the other strand: S- = 0.0; S- += trans[j][4 y_{j-1} + y_j] for
 *                       j = W - 1 down to 1 in that order; S- += start[y_0] last.
 * The reverse order is model columns descending, that is genome columns ascending: the order in which ms_scan adds its reverse terms
 * (M[3 - b][W - 1 - c] at step c).  A model with trans[j][4 a + b] = M[b][j] and start[b] = M[b][0] therefore gives ms_scan_best's raw
 * sums of M on both strands, bit for bit, on a window without a non-ACGT base.  Every "+=" is one rounded IEEE fp64 addition.
 * A window that holds ANY non-ACGT base has no score and never wins.  This departs from the PWM walks, where such a base adds +0.0, on
 * purpose: a pair term with an unknown neighbour has no sensible value.
 *     max_raw   the Viterbi maximum in the same arithmetic: v_0[b] = start[b]; v_j[b] = max over a of (v_{j-1}[a] + trans[j][4 a + b]);
 *               max_raw = max over b of v_{W-1}[b].  A rounded addition is monotone, so this IS the greatest forward raw sum over all
 *               4^W windows, and the best possible site scores exactly 1.0.
 *     score     raw / max_raw, one IEEE fp64 divide.
 * The BEST SITE of a cell is ms_scan_best's: the windows pos = 0 .. L - W are walked pos ascending, '+' before '-', over the strands of
 * strand_mask, from best = -inf, a window replacing the best iff its score is GREATER -- ties keep the earlier window, -inf never wins.  A
 * cell without a winner (L < W, a non-ACGT base or a forbidden transition in every window) holds score = NaN, pos = -1, strand = 0.
 * A model is SCORABLE iff max_raw is a finite number > 0 and no entry that is read is NaN or +inf; entries of -inf are allowed and mean a
 * forbidden transition (the window's raw sum is -inf).  Every cell of an unscorable model holds the no-winner triple.
 *
 * ms_dimodelset_create copies values (the models' [W][16] rows one after the other) and widths[n_models]; it needs no device, and a model
 * set is not bound to one: the scan uploads the set's tables to the sequence set's device per call (4 (4 W - 3) entries of 16 bytes per
 * model), so there is no "handles on different devices" error, as in ms_scan_best.  MS_ERR_INVALID: out NULL, n_models < 0, NULL arrays
 * with n_models > 0, a width < 1, a width above the cap ms_debug_dimodel_dims reports (256: the widest model whose table fits one LDS
 * tile).  ms_dimodelset_max_raw writes max_raw[n_models], whether a model is scorable or not.
 *
 * ms_scan_best_dimodels returns an ordinary ms_best with n_pwms = the number of models: ms_best_shape, ms_best_sites,
 * ms_best_sites_device, ms_best_device_ms, ms_best_rank_sum, ms_best_count_passing and ms_best_free take it as they take ms_scan_best's.
 * The bytes of all three planes are the same on every run, and a cell does not depend on which other models and regions share the call.
 * Work memory: the set's tables, and ms_scan_best's 16 bytes per (model, segment) of the regions of more than one segment.
 * MS_ERR_INVALID: out NULL, NULL handles, a strand mask outside 1..3, flags != 0, a region of 2^31 bases or more.  MS_ERR_NOMEM: the 13 bytes
 * per cell do not fit the device (nothing has been launched then).  n_models = 0 and n_seqs = 0 are valid and give empty results.  Without a
 * device: MS_ERR_RUNTIME ("no CPU fallback") before anything else. */
typedef struct ms_dimodelset ms_dimodelset;
int  ms_dimodelset_create(const double *values /* [sum of W][16] */, const int32_t *widths /* [n_models] */, int32_t n_models, ms_dimodelset **out);
int  ms_dimodelset_size(const ms_dimodelset *models, int32_t *n_models);
int  ms_dimodelset_max_raw(const ms_dimodelset *models, double *out /* [n_models] */);
void ms_dimodelset_free(ms_dimodelset *models);
int  ms_scan_best_dimodels(const ms_dimodelset *models, const ms_seqset *seqs, int strand_mask, uint32_t flags /* 0 */, ms_best **out);

/* ---- bipartite motifs: the best site of two half-sites with a variable spacer (ms_bipartite.hip) ---------------------- */
/* A BIPARTITE SPEC over a PWM set is (a, b, flip, g_min, g_max): a and b are motif indices of the set (a == b is allowed), flip is 0 or 1,
 * and 0 <= g_min <= g_max <= G (G = 64; both elements have at most 64 columns; ms_debug_bipartite_dims reports the caps).  For motif m of
 * width W_m and window start p of a region:
 *     F_m(p), R_m(p)   the forward and the reverse raw sum of the window exactly as ms_scan_best forms them: S = 0.0, then for the columns
 *                      c = 0 .. W_m - 1 in that order F += M[x][c] and R += M[3 - x][W_m - 1 - c] for the base x at p + c; a non-ACGT base
 *                      adds nothing.  Every "+=" is one rounded IEEE fp64 addition.
 * For a gap g the site spans S = W_a + g + W_b bases and is placed at p, 0 <= p <= L - S, on either strand:
 *     '+'  raw = F_a(p) + Y(p + W_a + g)      with Y  = F_b for flip == 0 and R_b for flip == 1;
 *     '-'  raw = Y'(p) + R_a(p + W_b + g)     with Y' = R_b for flip == 0 and F_b for flip == 1: the same composite read on the other strand,
 *                                             so on the forward strand b's half comes first.
 * Each raw is ONE rounded fp64 addition of the two element sums, left operand first as written.  The bases of the spacer are never read.
 *     denominator   D = max_raw_a + max_raw_b, one rounded addition of the set's two max_raw values (ms_pwmset_max_raw);
 *     score         raw / D, one IEEE fp64 divide.
 * The BEST SITE of a cell (spec, region): p is walked ascending; at each p '+' comes before '-' over the strands of strand_mask; within a
 * strand g ascends from g_min to g_max; from best = -inf a placement replaces the best iff its score is GREATER -- ties keep the earlier
 * placement, -inf never wins.  Per cell the result holds score (fp64), pos (int32: the leftmost base of the whole site, relative to the
 * region), strand (int8: 1 or 2) and gap (int16); a cell without a winner holds NaN, -1, 0, -1.
 * A spec is SCORABLE iff no entry of either element is NaN or +inf and D is a finite number > 0 -- the rule is on the sum, so a partner
 * whose columns are all zero is legal.  Every cell of an unscorable spec holds the no-winner values.  An entry of -inf is ordinary: the
 * placement's raw sum is -inf.
 *
 * ms_scan_best_bipartite returns an ordinary ms_best with n_pwms = n_specs: ms_best_shape, ms_best_sites, ms_best_sites_device,
 * ms_best_device_ms, ms_best_rank_sum, ms_best_count_passing and ms_best_free take it as they take ms_scan_best's.  The handle carries a
 * fourth plane, the gaps: ms_best_gaps copies the rows m0 <= m < m1 of it to host memory, ms_best_gaps_device gives its device address
 * (valid until ms_best_free); on a handle from any other scan both return MS_ERR_INVALID.  The bytes of all four planes are the same on
 * every run, and a cell does not depend on which other specs and regions share the call.  The PWM set's cutoffs are not read, and the set
 * is not bound to a device by this call: the specs' tables (4 (W_a + W_b) entries of 16 bytes each) are uploaded per call.
 * Work memory: those tables, and 18 bytes per (spec, segment) of the regions of more than one segment.
 * MS_ERR_RUNTIME ("no CPU fallback") without a device, before anything else.  MS_ERR_INVALID: out NULL, NULL handles, NULL arrays with
 * n_specs > 0, n_specs < 0, an index outside the set, flip > 1, g_min < 0, g_min > g_max, g_max > G, an element wider than the cap, a strand
 * mask outside 1..3, flags != 0, a region of 2^31 bases or more.  MS_ERR_NOMEM: the 15 bytes per cell or the work block do not fit the device
 * (nothing has been launched then).  n_specs = 0 and n_seqs = 0 are valid and give empty results. */
int  ms_scan_best_bipartite(const ms_pwmset *pwms, const int32_t *a, const int32_t *b, const uint8_t *flip, const int32_t *gap_min, const int32_t *gap_max,
                            int32_t n_specs, const ms_seqset *seqs, int strand_mask, uint32_t flags /* 0 */, ms_best **out);
int  ms_best_gaps(const ms_best *b, int32_t m0, int32_t m1, int16_t *gap /* [m1 - m0][n_seqs] */);
int  ms_best_gaps_device(const ms_best *b, void **d_gap);

/* ---- cutoff-free enrichment over best-site matrices that stay on the device (ms_ranksum.hip) ------------------------- */
/* ORDER OF CELL VALUES, for both calls: a cell without a winner (score NaN, strand 0) ranks below every number; all cells without a winner
 * tie with one another; numbers compare as IEEE doubles, so -0.0 equals +0.0.  Nothing is special-cased for unscorable motifs: their rows
 * are all NaN and follow the rule (u2 = na * nb, ties = N^3 - N).
 *
 * ms_best_rank_sum.  Group A = the cells a.score[m][i] with sel_a == NULL or sel_a[i] != 0 (na of them); group B likewise from b (nb).  a and b
 * may be the same handle; the selections may overlap.  Per motif row m0 <= m < m1, with x over group A, y over group B and N = na + nb:
 *     u2[m - m0]   = 2 #{(x, y): x > y} + #{(x, y): x == y}      twice the Mann-Whitney U of group A, an integer; AUROC = u2 / (2 na nb); it
 *                                                                 fits int64 because a group holds fewer than 2^31 regions
 *     ties[m - m0] = sum over the tie groups of the pooled sample of (t^3 - t), an unsigned 128-bit integer as {low word, high word}
 *                    (it passes 2^63 at N = 2 097 152)
 * n (may be NULL) receives {na, nb}.  na = 0 or nb = 0 is valid and gives u2 = 0.  m0 == m1 does nothing and returns MS_OK.  The outputs are
 * HOST memory.  Rank sums are NOT additive over region shards: a multi-GPU caller shards the motifs, not the regions.  The call is
 * synchronous.  It is an exact integer reduction: the same bytes on every run and for every internal batching (motif rows are ranked in
 * batches of max(1, budget / N) rows, budget = 2^27 elements; work memory 16 bytes per element of a batch plus the sort's own).
 * z and P-values are host arithmetic on these integers (motifscan_amd/enrich.py).
 *
 * ms_best_count_passing.  counts[row][k] = the number of selected regions whose best score s satisfies s - cutoffs[row][k] >= -1e-10: ms_scan's
 * hit rule, one rounded subtraction; a NaN cell never passes.  The rounded subtraction is monotone in s, so this is exactly the number of
 * regions that hold at least one site at that cutoff: it equals what ms_result_region_counts gives for an ms_scan of the same sequence set
 * and strand mask at that cutoff.  The counts are additive over region shards.  The outputs are HOST memory.  n_cut = 0 is valid.
 *
 * Errors, both calls: MS_ERR_RUNTIME ("no CPU fallback") without a usable device, before the handles are looked at.  MS_ERR_INVALID: NULL
 * handles or NULL required outputs, flags != 0, a motif range outside [0, n_pwms], a->P != b->P, handles on different devices, n_cut < 0 or
 * n_cut > 0 with NULL arrays, a cutoff that is not finite.  MS_ERR_NOMEM: the work memory does not fit (nothing has been launched). */
int ms_best_rank_sum(const ms_best *a, const uint8_t *sel_a /* [Ra] or NULL */,
                     const ms_best *b, const uint8_t *sel_b /* [Rb] or NULL */,
                     int32_t m0, int32_t m1, uint32_t flags /* 0 */,
                     int64_t *u2 /* [m1 - m0] */, uint64_t *ties /* [m1 - m0][2]: low word, high word */,
                     int64_t *n /* [2]: na, nb; may be NULL */, double *device_ms /* or NULL */);
int ms_best_count_passing(const ms_best *b, const uint8_t *sel /* [R] or NULL */,
                          const double *cutoffs /* [m1 - m0][n_cut] */, int32_t n_cut, int32_t m0, int32_t m1,
                          int64_t *counts /* [m1 - m0][n_cut] */, double *device_ms /* or NULL */);

/* ---- total binding affinity: the summed likelihood ratio of every (motif, region) cell, dense (ms_affinity.hip) ---------- */
/* The PWMs are natural-log odds, so a window's raw sum is its log likelihood ratio.  For motif m of width W and region r of length L the
 * TERMS of the cell are the pairs (window start pos = 0 .. L - W, strand of strand_mask).  With max_n >= 0 only the windows that hold at
 * most max_n non-ACGT bases among their own W bases are terms (the bits of the non-ACGT mask, IUPAC letters included, as in
 * ms_scan_score_histogram); max_n = -1 takes every window, as the scan does.  raw(term) is the raw sum exactly as ms_scan / ms_scan_best
 * form it: columns in order, forward M[b][c], reverse M[3 - b][W - 1 - c] at the same step, +0.0 for a base that adds nothing.  max_raw is
 * NOT read and nothing is divided.  Per cell, four planes [n_pwms][n_seqs]:
 *     n_terms   int32    the number of terms; a term of raw = -inf counts.  0 for L < W or when max_n removes every window.
 *     peak      double   the greatest raw over the terms, bit-exact.  NaN if n_terms == 0.  May be -inf.
 *     sum       double   S = sum over the terms of exp(scale * (raw - peak)); a term of raw = -inf adds 0.  S = 0 if peak is -inf or
 *                        n_terms == 0; otherwise 1 <= S <= n_terms up to rounding.
 *     log_mean  double   scale * peak + log(sum / n_terms), each operation rounded once: the log of the region's MEAN likelihood ratio
 *                        (+ log(n_terms): of its total binding affinity).  -inf if peak == -inf, NaN if n_terms == 0.  The plane
 *                        ms_affinity_rank_sum ranks.
 * A motif with an entry that is NaN or +inf has an EMPTY ROW everywhere: n_terms = 0, peak = NaN, sum = 0, log_mean = NaN.  A motif whose
 * max_raw is <= 0 (an all-negative matrix) IS scored, unlike in ms_scan_best: its likelihood ratios are well defined.  scale must be
 * finite and > 0: the lambda of TRAP-like models; 1.0 for natural-log odds, ln 2 for a log2 matrix.  The cutoffs of the PWM set are not read.
 * ACCURACY of sum against the exact sum of the exact exponentials of the float64 raw sums: within 16 (n_terms + 8) 2^-53 of it, relative
 * (DESIGN.md has the derivation; n_terms and peak are exact).
 * DETERMINISM: all four planes are the same bytes on every run, and a cell's bytes depend only on its motif, its region's bases,
 * strand_mask, scale and max_n -- not on which other regions or motifs share the call.  The reduction order is fixed: a lane takes its
 * windows in order, the wave is folded by a fixed butterfly, the segments of a long region in a fixed order; no floating-point atomics.
 * Work memory: a region of more than ms_debug_affinity_dims()[0] bases costs 24 bytes per (motif, segment) for the duration of the call.
 * MS_ERR_RUNTIME ("no CPU fallback") without a device, before anything else.  MS_ERR_INVALID: NULL handles, a strand mask outside 1..3,
 * flags != 0, scale not finite or <= 0, max_n < -1, a region of 2^31 bases or more.  MS_ERR_NOMEM: the 28 bytes per cell plus the partials
 * do not fit (nothing has been launched then).  n_seqs = 0 and n_pwms = 0 are valid and give an empty result. */
typedef struct ms_affinity ms_affinity;
int  ms_scan_affinity(const ms_pwmset *pwms, const ms_seqset *seqs, int strand_mask, double scale, int32_t max_n, uint32_t flags /* 0 */,
                      ms_affinity **out);
int  ms_affinity_shape(const ms_affinity *a, int32_t *n_pwms, int64_t *n_seqs);
/* Motifs m0 <= m < m1 into host buffers [(m1 - m0)][n_seqs] row-major; any pointer may be NULL.  MS_ERR_INVALID for m0 < 0, m1 > n_pwms, m0 > m1. */
int  ms_affinity_cells(const ms_affinity *a, int32_t m0, int32_t m1, double *peak, double *sum, int32_t *n_terms, double *log_mean);
/* Device pointers of the full [n_pwms][n_seqs] planes, valid until free; any pointer may be NULL. */
int  ms_affinity_cells_device(const ms_affinity *a, void **d_peak, void **d_sum, void **d_n_terms, void **d_log_mean);
/* Device time of the call that made the result: first launch -> last kernel done. */
int  ms_affinity_device_ms(const ms_affinity *a, double *ms);
void ms_affinity_free(ms_affinity *a);
/* ms_best_rank_sum's semantics, outputs and errors exactly, applied to the log_mean planes of two affinity results (they may be the same
 * handle): a NaN cell (no term) ranks below every number and ties with every other NaN cell; -inf is an ordinary number. */
int  ms_affinity_rank_sum(const ms_affinity *a, const uint8_t *sel_a /* [Ra] or NULL */,
                          const ms_affinity *b, const uint8_t *sel_b /* [Rb] or NULL */,
                          int32_t m0, int32_t m1, uint32_t flags /* 0 */,
                          int64_t *u2 /* [m1 - m0] */, uint64_t *ties /* [m1 - m0][2]: low word, high word */,
                          int64_t *n /* [2]: na, nb; may be NULL */, double *device_ms /* or NULL */);

/* ---- expected base counts per motif column: the E-step of a motif refinement, on the affinity's terms (ms_expcounts.hip) ---------- */
#define MS_EXPECTED_MAX_WIDTH 256
/* For motifs m0 <= m < m1 (row = m - m0): how much A, C, G, T weight stands under every motif column over ALL windows of all regions,
 * every window weighted by its posterior probability of being the site.  aff must be the result of ms_scan_affinity(pwms, seqs, ...):
 * strand_mask, scale and max_n are read from the handle.  The unit of every output is U = 2^-32.
 *   TERMS     of cell (m, r): exactly ms_scan_affinity's -- window start 0 .. L - W, the strands of the mask, the max_n filter -- and
 *             their raw sums x formed exactly as there (the same column order, +0.0 for a non-ACGT base).
 *   pi(m, r)  the cell's responsibility: 1 if prior_logit is +inf (OOPS, "one site per region"; no arithmetic is done); 0 if
 *             n_terms == 0, if log_mean is -inf or if prior_logit is -inf; otherwise 1 / (1 + exp(-(log_mean + prior_logit))), each
 *             operation rounded once.  This is the ZOOPS posterior that region r holds a site of m when a fraction g of the regions
 *             does, prior_logit = log(g / (1 - g)): g A / (1 - g + g A) with A = exp(log_mean), the mean likelihood ratio.
 *   w(term)   for x > -inf: v = pi * exp(scale * (x - peak)) / sum with peak and sum of the cell's planes -- subtract, multiply, exp,
 *             multiply, divide, each rounded once -- clamped: w = 1 unless v < 1, 0 unless v > 0 (the clamp never acts on planes that
 *             belong to these inputs, where 0 <= v <= 1; with any other it keeps the conversion defined, and the result is meaningless).
 *             q = (int64) rint(w * 2^32), round half to even.  A term of x = -inf has q = 0.
 *   SLOTS     the term adds q to ONE slot of EVERY motif column c = 0 .. W - 1: on '+' that of the base at pos + c, on '-' that of the
 *             base at pos + W - 1 - c, complemented; slots 0 .. 3 are A, C, G, T in the motif's orientation, slot 4 a non-ACGT base
 *             (a bit of the non-ACGT plane).  ms_result_site_base_counts' orientation rule, without flanks.
 *   counts[row][c][s]  the sum of those q; the column pitch of a row is pwms->max_width, the columns behind W are zero.
 *   total[row]         (may be NULL) the sum of q over all terms: every used column of counts sums to it exactly.
 *   n_regions[row]     (may be NULL) the regions with n_terms > 0.
 * A motif with an empty row in aff (a NaN or +inf entry) has all three zero.
 * Why 2^-32: a weight is in [0, 1], so a region adds at most 2^32 in OOPS and an int64 holds 2^31 regions per motif; rounding a term
 * costs at most 2^-33; and integer sums do not depend on the order of summation.  PROMISES: the same bytes on every run; a row's bytes
 * depend only on its motif, the regions and the affinity call's arguments -- not on the motif range, on the other motifs of the set or on
 * how the work is split; counts, total and n_regions over a sequence set equal the sums over any partition of it into shards (each with
 * its own ms_scan_affinity), exactly.  No floating-point atomics.
 * MS_EXPECTED_MAX_WIDTH is not a measured limit: the accumulators and tables of a tile of motifs are kept in LDS together, real
 * matrices have under 40 columns, and this walk has no path for tables in HBM.
 * Synchronous.  An empty motif range (m0 == m1) does nothing and returns MS_OK.  Every output is host memory or device memory of the
 * handle's device; the stream rule is ms_result_site_base_counts': the library writes a device output on its own stream, work the caller
 * has queued on that memory must have finished before the call, and the call returns after its own writes are done.  *device_ms (may be
 * NULL): first launch -> last kernel done.
 * MS_ERR_RUNTIME ("no CPU fallback") without a usable device, before anything else.  MS_ERR_INVALID, before anything is launched: NULL
 * handles or a NULL counts, flags != 0, prior_logit NaN, a motif range outside [0, P], pwms->P != the handle's P, seqs->R != the handle's
 * R or seqs on another device, a motif of more than MS_EXPECTED_MAX_WIDTH columns INSIDE the range, an output on another device. */
int ms_affinity_expected_counts(const ms_affinity *aff, const ms_pwmset *pwms, const ms_seqset *seqs, double prior_logit, int32_t m0,
                                int32_t m1, uint32_t flags /* 0 */, int64_t *counts /* [(m1 - m0)][pwms->max_width][5] */,
                                int64_t *total /* [m1 - m0], or NULL */, int64_t *n_regions /* [m1 - m0], or NULL */,
                                double *device_ms /* or NULL */);

/* The hit arrays in COMPACT form in library-owned pinned host memory: coord[i] = seq_idx << 32 | pos << 1 | (strand - 1),
 * score[i] -- 16 bytes per hit on the host link instead of 25.  Needs seq_idx < 2^32 and pos < 2^31 (MS_ERR_INVALID
 * otherwise).  Valid until the result is freed or de-duplicated, or a different form is asked for (ms_result_hits_host,
 * ms_result_hits_packed12_host; a refused request included): the three accessors share one pinned buffer. */
int ms_result_hits_packed_host(ms_result *res, const uint64_t **coord, const double **score);
/* ... and in 12 bytes per hit: coord32[i] = seq_idx << *shift | pos << 1 | (strand - 1), score[i] -- for results whose region indices and
 * positions fit 31 bits together (a batch of 250 000 regions of 500 bp: 18 + 9), i.e. every batch of a batch stream; MS_ERR_INVALID (and the
 * 16-byte form stays available) when they do not.  Same list building (cscore.c:443-471), a quarter less on the host link.  The
 * pointers are valid until the result is freed or de-duplicated, or a different form is asked for (ms_result_hits_host,
 * ms_result_hits_packed_host): the three accessors share one pinned buffer.  A refused call leaves no form in the buffer. */
int ms_result_hits_packed12_host(ms_result *res, const uint32_t **coord, const double **score, int32_t *shift);
/* Which compact form a result holds after a batch stream's copy-out: *bytes_per_hit = 12, 16, or 0 (the plain arrays). */
int ms_result_packed_form(const ms_result *res, int32_t *bytes_per_hit);

/* ---- pinned host memory -------------------------------------------------------------------- */
/* Page-locked host memory for sequence input: uploads from it run at the full link rate and overlap with scans. */
int ms_host_alloc(size_t bytes, void **out);
/* The library's cache of pinned result blocks (size classes, like the device block cache): out[0] requests served from it, out[1] requests that
 * went to the driver, out[2] blocks returned to the driver, out[3] nanoseconds inside the driver.  Steady-state batches show no [1] / [2]. */
int ms_host_pool_stats(uint64_t out[4]);
void ms_host_free(void *p);

/* ---- batch streams: upload | pack + scan | copy-out overlapped ------------------------------- */
#define MS_STREAM_DEDUP       1u   /* de-duplicate every batch on the device (scanner.py:156-193) before the copy-out      */
#define MS_STREAM_NO_HITS     2u   /* counts only (control regions: stats.py:29-31): a batch is scanned with MS_SCAN_COUNTS_ONLY, a sweep span
                                      makes ONLY the per-motif window counts and the number of sites (no site array exists: the hit
                                      accessors of such a result fail with MS_ERR_INVALID; ms_result_motif_offsets then gives the running
                                      per-motif site numbers, consistent with n_hits; with MS_STREAM_DEDUP such a span is NOT de-duplicated --
                                      de-duplication never empties a window, the counts are the same)                           */
#define MS_STREAM_EXACT_ONLY  4u   /* MS_SCAN_EXACT_ONLY for every batch (validation)                                      */
#define MS_STREAM_PACKED      8u   /* copy the hits out in the compact form of ms_result_hits_packed_host                  */
#define MS_STREAM_PACKED12   32u   /* ... in the 12-byte form of ms_result_hits_packed12_host for every batch that fits it, the 16-byte form for
                                      the others (ms_result_packed_form tells which)                                        */
#define MS_STREAM_HOST_PACK  16u   /* the upload stage packs on host threads (ms_seqset_create_hostpacked): no kernel beside the scan */
typedef struct ms_stream ms_stream;
/* depth: batches that may wait between two stages (>= 1; 2 overlaps all three stages).  The stream is bound to the
 * calling thread's device (ms_set_device).  The PWM set must outlive the stream. */
int ms_stream_create(const ms_pwmset *pwms, int strand_mask, uint32_t flags, int depth, ms_stream **out);
/* Queue one batch of regions (same arguments as ms_seqset_create).  offsets is copied; bases is BORROWED until
 * ms_stream_next has returned this batch.  Fails with MS_ERR_INVALID when ms_stream_capacity batches are in flight. */
int ms_stream_submit(ms_stream *st, const char *bases, const int64_t *offsets, int64_t n_seqs);
/* The same for a batch of which only the per-motif region counts will be read (MS_STREAM_NO_HITS for this batch alone): what the
 * reference does with the control regions -- cli/scan.py:81-89 scans them, stats.py:29-31 counts the regions with >= 1 site, no
 * writer ever sees their sites -- while the input regions' batches of the same stream carry their hits out. */
int ms_stream_submit_counts_only(ms_stream *st, const char *bases, const int64_t *offsets, int64_t n_seqs);
/* Queue one span of a window sweep: n_bases of ONE chromosome starting at a window start; the result is what
 * ms_scan_sweep gives for it (seq_idx = window index inside the span: add ms_span.first_window). */
int ms_stream_submit_span(ms_stream *st, const char *bases, int64_t n_bases, int32_t window, int32_t stride);
/* A batch of regions of a genome that is resident in HBM (ms_genome_create): what ms_seqset_from_genome + ms_scan give for them,
 * with the cut of batch i + 1 out of the 2-bit genome overlapping the scan of batch i and the copy-out of batch i - 1
 * (scanner.py:71-87 + 125 per batch; the genome must outlive the batch's result).  The arrays are copied. */
int ms_stream_submit_regions(ms_stream *st, const ms_genome *genome, const int32_t *chrom, const int64_t *start, const int64_t *end,
                             int64_t n_regions);
/* The oldest batch's result (submission order), its hit arrays already in pinned host memory (ms_result_hits_host /
 * ms_result_hits_packed_host return at once).  *out = NULL when nothing is in flight.  The caller frees the result. */
int ms_stream_next(ms_stream *st, ms_result **out);
int ms_stream_in_flight(const ms_stream *st, int *n);
/* Where the stream's three stages spent their time so far, for stage k = 0 uploader, 1 scanner, 2 downloader:
 * out[4k] batches done, out[4k+1] ms working, out[4k+2] ms waiting for input, out[4k+3] ms waiting for room downstream.
 * The stage with the least waiting is the one that bounds the stream. */
int ms_stream_stats(const ms_stream *stream, double out[12]);
int ms_stream_capacity(const ms_stream *st, int *n);
void ms_stream_free(ms_stream *st);          /* drains and discards whatever is still in flight */

/* ---- sweep planning ------------------------------------------------------------------------ */
typedef struct ms_span {
    int32_t chrom;            /* chromosome index                                                       */
    int32_t reserved;
    int64_t begin, end;       /* bases [begin, end) of the chromosome; begin is a window start          */
    int64_t first_window;     /* global index (over all chromosomes, in order) of the span's first window */
    int64_t n_windows;
} ms_span;
/* Cut the sweep "windows [k*stride, k*stride + window) of every chromosome" (chromosomes shorter than a window have
 * none) into spans of at most max_span_bases bases; neighbouring spans of a chromosome overlap by window - stride bases.
 * spans may be NULL (count only); at most cap entries are written; *n_spans is the number needed. */
int ms_sweep_spans(const int64_t *chrom_len, int32_t n_chroms, int32_t window, int32_t stride, int64_t max_span_bases,
                   ms_span *spans, int64_t cap, int64_t *n_spans);

/* ---- score (c_score) -------------------------------------------------------------------- */
/* out: host, [P][R] row-major.  A sequence shorter than a PWM scores its missing bases as
 * non-ACGT (the reference reads out of bounds there, cscore.c:195-196). */
int ms_score(const ms_pwmset *pwms, const ms_seqset *seqs, int strand_mask, double *out);

/* The device half of the cutoff builder (`motifscan motif --build`: cli/motif.py:134-137 and
 * get_score_cutoffs, motif/__init__.py:378-401): c_score of all R sequences for every PWM, each
 * PWM's scores sorted in DESCENDING order, out[p][k] = score at 0-based rank ranks[k]
 * (the reference reads rank int(R * 0.1**e) - 1 for e = 2 .. min(len(str(R)), 7) - 1). */
int ms_score_ranks(const ms_pwmset *pwms, const ms_seqset *seqs, int strand_mask, const int64_t *ranks,
                   int32_t n_ranks, double *out /* [P][n_ranks] */);

/* ---- de-duplication of overlapping sites (scanner.py:156-193), host side ---------------- */
/* In: hits in ms_result order.  Out: keep[n_hits] (1 = kept).  Kept hits are already in the
 * order Scanner.scan_motifs returns them (start ascending, '+' before '-' on ties). */
int ms_dedup_hits(const int64_t *motif_offsets, int32_t n_pwms, const int32_t *widths,
                  const int64_t *seq_idx, const int64_t *pos, const double *score,
                  const int8_t *strand, uint8_t *keep);

/* ---- plot data (motifscan scan --plot-dist: plot.py:43-153) -------------------------------- */
/* A result made of hit arrays in ms_result order (per motif: region, position, '+' (1) before '-' (2)), uploaded to the calling
 * thread's device: what the plot data below read when the hits are no longer on the device.  motif_offsets[P+1]; every seq_idx must
 * lie in [0, n_regions) (MS_ERR_INVALID otherwise).  The per-motif region counts are made on the host. */
int ms_result_from_hits(int32_t n_pwms, int64_t n_regions, const int64_t *motif_offsets, const int64_t *seq_idx, const int64_t *pos,
                        const double *score, const int8_t *strand, ms_result **out);
/* plot.py:60-70: for motifs m0 <= m < m1, the histogram of d = pos + W/2 - summit_rel[seq_idx] over the result's sites (which are counted as
 * they are: a scan with remove_dup de-duplicates first, ms_result_dedup) in the bins of np.arange(-extend - 5, extend + 6, 10) --
 * edge[i] <= d < edge[i + 1], the last bin closed, everything else dropped; n_bins = ceil((2 * extend + 11) / 10) - 1.  The bin is taken
 * from 2d = 2 * (pos - summit_rel) + W in integers, so the counts are exact.  summit_rel[R] = summit - sequence start, host.
 * counts: host [(m1 - m0) x n_bins]; n_sites: host [m1 - m0], all sites of the motif (len(distances), in range or not).
 * MS_ERR_INVALID on a counts-only result, as the other hit accessors. */
int ms_result_site_histogram(const ms_result *res, const ms_pwmset *pwms, const int64_t *summit_rel, int64_t extend, int32_t m0, int32_t m1,
                             int64_t *counts, int64_t *n_sites);
#define MS_PROFILE_UNSMOOTHED 1   /* ms_result_rank_profile: the fold changes as plot.py:141 appends them, without smooth() */
/* plot.py:120-142 for motifs m0 <= m < m1 of a result over R regions: rank_order[R] (host) = the region at each rank (a permutation of
 * [0, R): plot.py:121-122's stable descending sort, made by the caller); f = R / 100; for every rank idx, head = max(0, idx - f),
 * tail = min(idx + f, R), ratio_input = (ranks in [head, tail) whose region holds >= 1 site) / (tail - head), and
 * out = ratio_input / ratio_control[m - m0] -- two IEEE fp64 divisions in this order.  ratio_control [m1 - m0] must be > 0 (the caller
 * applies plot.py:130-132's 0 -> 1).  Unless MS_PROFILE_UNSMOOTHED, each row is then smoothed as plot.py:34-40 does for R > 11: reflected
 * at both ends, out[i] = sum_j kernel[j] * ratio[i - 5 + j], kernel = (w / w.sum()) reversed, w = np.hanning(11) (host, 11 doubles).
 * out: [(m1 - m0) x R] doubles, host or device memory of the result's device.  MS_ERR_INVALID for R < 100 (plot.py:138 divides by zero
 * there) and on a counts-only result. */
int ms_result_rank_profile(const ms_result *res, const int64_t *rank_order, const double *ratio_control, const double *kernel, int32_t m0,
                           int32_t m1, int flags, double *out);

/* ---- motif pairs: co-occurrence and anchor spacing over a result's hit arrays (ms_pairs.hip) -------------- */
/* Both read the result's sites as they are (de-duplicated or not, like ms_result_site_histogram), are synchronous, exact integer
 * reductions -- the same bytes on every run -- and additive over shards of the regions (one all-reduce(sum) across ranks).  Both do
 * nothing and return MS_OK for an empty motif range (m0 == m1), and fail with MS_ERR_INVALID on a counts-only result, as the other hit
 * accessors.
 *
 * out[a][j], a = 0 .. m1 - m0 - 1, j = 0 .. P - 1: the number of regions of the result that hold at least one site of motif m0 + a AND at
 * least one site of motif j.  out[a][m0 + a] is motif m0 + a's ms_result_region_counts value; the full matrix (m0 = 0, m1 = P) is
 * symmetric; a motif without sites has a zero row and a zero column.  out: [(m1 - m0) x P] int64, host memory or device memory of the
 * result's device (then a consumer can all-reduce it where it is).  The library writes a device `out` on its own stream: work the caller
 * has queued on that memory on another stream (a fill, a collective) must have finished before the call; the call returns after its own
 * writes are done.
 * MS_ERR_INVALID: NULL handle or output, a motif range outside [0, P], R >= 2^31, output on another device. */
int ms_result_cooccurrence(const ms_result *res, int32_t m0, int32_t m1, int64_t *out /* [(m1 - m0)][P] */);
/* Anchor motif a = `anchor` (width Wa) against the partner motifs j = m0 + row (width Wj), row = 0 .. m1 - m0 - 1.  An ordered PAIR is a
 * site s of a and a site t of j in the same region.  For j == a a site is not paired with itself, but with every other site of a -- its
 * other-strand twin at the same position included -- so both (s, t) and (t, s) are pairs.  Per pair, in half base pairs,
 * t2 = 2 * (pos_t - pos_s) + Wj - Wa is the distance from the anchor site's centre to the partner site's (its parity is that of Wj - Wa);
 * the pair is counted iff |t2| <= 2 * max_dist, in bin (t2 + 2 * max_dist) >> 1 of 2 * max_dist + 1 (for an odd Wj - Wa the last bin stays
 * 0) and orientation o = 2 * (strand_s - 1) + (strand_t - 1): 0 '+/+', 1 '+/-', 2 '-/+', 3 '-/-' (anchor first).  Nothing is
 * reflected for an anchor on the '-' strand: the caller folds (t2 -> -t2, both strands flipped; motifscan_amd/pairs.py).
 * counts[row][o][bin] = the number of such pairs; n_pairs[row] = ALL ordered pairs of the row in the same region, whatever their
 * distance: sum over the regions of n_a(region) * n_j(region), minus n_a for j == a.  Both host memory.
 * The sites of the anchor and of the partner motifs must be in scan order -- per motif by region, then position -- which every scan
 * result is; a result made by ms_result_from_hits of arrays that are not is refused (checked on the device, outputs zeroed).
 * MS_ERR_INVALID: NULL handles or outputs, pwms->P != the result's P, anchor outside [0, P), a motif range outside [0, P], max_dist < 0 or
 * > 2^20, (m1 - m0) * 4 * (2 * max_dist + 1) > 2^31, sites out of order. */
int ms_result_pair_spacing(const ms_result *res, const ms_pwmset *pwms, int32_t anchor, int32_t m0, int32_t m1, int32_t max_dist,
                           int64_t *counts /* [(m1 - m0)][4][2 * max_dist + 1] */, int64_t *n_pairs /* [m1 - m0] */);

/* ---- site stacks: base counts per motif column over a result's sites (ms_sitestack.hip) ------------------------- */
#define MS_SITESTACK_MAX_FLANK 64
/* For motifs m0 <= m < m1 (row = m - m0) of a result and the sequence set it was made over: what the motif's sites look like, column
 * by column, in the MOTIF's orientation.  C = pwms->max_width + 2 * flank is the column pitch of every row.  Motif m of width W uses
 * columns j = 0 .. W + 2 * flank - 1 (column flank + c is motif column c); the columns behind them stay zero.  For a site (region r of
 * length L, pos, strand), column j reads region base q = pos - flank + j as it is on '+', and q = pos + W - 1 + flank - j complemented
 * (code 3 - b) on '-': the columns follow the motif, exactly as the scan's reverse strand reads M[3 - b][W - 1 - c].
 *   counts[row][j][s]: s = 0 .. 3 the sites with A, C, G, T there after orientation (either case); s = 4 a non-ACGT base (a bit of the
 *       packed "non-ACGT" plane: IUPAC letters count as well as N); s = 5 q < 0 or q >= L, outside the region -- decided by the
 *       region's bounds, never by what lies beside it in the packed planes.
 *   dinuc[row][j][4 * a + b], j = 0 .. W + 2 * flank - 2 (may be NULL): the sites whose oriented base is a at column j and b at column
 *       j + 1, counted only when both columns fall in slots 0 .. 3.
 *   n_sites[row] (may be NULL): the motif's sites in the result; every used column of counts sums to it.
 * The sites are read as they are (de-duplicated or not).  Synchronous; an exact integer reduction -- the same bytes on every run --
 * and additive over shards of the regions.  An empty motif range (m0 == m1) does nothing and returns MS_OK.  Every output is host
 * memory or device memory of the result's device (then a consumer can all-reduce it where it is).  The library writes a device output
 * on its own stream: work the caller has queued on that memory on another stream (a fill, a collective) must have finished before the
 * call; the call returns after its own writes are done.  *device_ms (may be NULL): first launch -> last kernel done.
 * MS_ERR_RUNTIME without a usable device, before anything else.  MS_ERR_INVALID: NULL handles or a NULL counts, flags != 0, flank
 * outside [0, MS_SITESTACK_MAX_FLANK], a motif range outside [0, P], pwms->P != the result's P, seqs->R != the result's R or seqs on
 * another device, a counts-only result, an output on another device, and a site with a region index outside [0, R), pos < 0 or
 * pos + W > L (a result of ms_result_from_hits, or the wrong sequence set: checked on the device while counting, outputs zeroed). */
int ms_result_site_base_counts(const ms_result *res, const ms_pwmset *pwms, const ms_seqset *seqs, int32_t flank, int32_t m0, int32_t m1,
                               uint32_t flags /* 0 */, int64_t *counts /* [(m1 - m0)][C][6] */, int64_t *dinuc /* [(m1 - m0)][C][16], or NULL */,
                               int64_t *n_sites /* [m1 - m0], or NULL */, double *device_ms /* or NULL */);

/* ---- signal tracks over sites: footprint profiles and per-site sums (ms_sitesignal.hip) ------------------------- */
typedef struct ms_track ms_track;
/* A resident track: one int32 per base of a sequence set, laid out by the same offsets (offsets[n_seqs] values).  Any int32 is a value;
 * there is no "missing" sentinel.  values: host memory or device memory of the calling thread's device; offsets: host memory, starts at
 * 0 and does not decrease.  The block comes from the device pool, like a sequence set's, and carries a few zeroed values at either end so
 * that the 16-byte loads of ms_result_site_signal form no address outside it.  Synchronous.  MS_ERR_RUNTIME without a usable device,
 * before anything else.  MS_ERR_INVALID: NULL pointers, n_seqs < 0, offsets that do not start at 0 or decrease, values on another device. */
int  ms_track_create(const int32_t *values, const int64_t *offsets, int64_t n_seqs, ms_track **out);
int  ms_track_size(const ms_track *t, int64_t *n_seqs, int64_t *n_values);
/* values [first, first + n) of the track, read back to host memory (tests). */
int  ms_track_values_host(const ms_track *t, int64_t first, int64_t n, int32_t *out);
void ms_track_free(ms_track *t);

#define MS_SITESIGNAL_MAX_FLANK 512
/* For motifs m0 <= m < m1 (row = m - m0) of a result and a track over the sequence set it was made of: the track summed over the motif's
 * sites, column by column, in the MOTIF's orientation.  C = pwms->max_width + 2 * flank is the column pitch of every row.  The strand index
 * s is 0 for '+' (result strand 1) and 1 for '-' (result strand 2).  A site (region r of length L, pos, strand) of a motif of width W uses
 * columns j = 0 .. W + 2 * flank - 1 (column flank + c is motif column c); the columns behind them stay zero.  Column j reads track
 * position q = pos - flank + j on '+' and q = pos + W - 1 + flank - j on '-': the values are not complemented, only their order is
 * reversed -- exactly the site stack's column rule (ms_result_site_base_counts).  A column is INSIDE iff 0 <= q < L of its own region,
 * decided by the region's bounds alone.
 *   sum[row][s][j]      the sum of value[offsets[r] + q] over the motif's sites of strand s whose column j is inside
 *   cover[row][s][j]    the number of those sites (may be NULL)
 *   n_sites[row][s]     the motif's sites of strand s (may be NULL); every column has cover <= n_sites.  The strands are kept apart so
 *                       that a caller with strand-specific tracks (Tn5 '+' cuts and '-' cuts) can swap tracks for the '-' sites
 *                       afterwards; the folded profile is sum[row][0] + sum[row][1]
 *   per_site[k - motif_offsets[m0]][0 .. 2]   for hit k of the selected slice (n_sel = motif_offsets[m1] - motif_offsets[m0] rows, in the
 *                       result's hit order), over its inside columns only: the upstream sum, columns [0, flank); the core sum, columns
 *                       [flank, flank + W); the downstream sum, columns [flank + W, W + 2 * flank) -- upstream and downstream in the
 *                       motif's orientation.  How many of a site's columns are inside is a closed form of (pos, W, L, flank) and is
 *                       left to the caller.
 * At least one of sum and per_site must be non-NULL.  The sites are read as they are (de-duplicated or not).  Synchronous; exact int64
 * sums -- |value| < 2^31 and fewer than 2^32 sites cannot overflow -- the same bytes on every run, additive over shards of the regions.
 * An empty motif range (m0 == m1) does nothing and returns MS_OK.  Every output is host memory or device memory of the result's device
 * (then a consumer can all-reduce it where it is).  The library writes a device output on its own stream: work the caller has queued on
 * that memory on another stream (a fill, a collective) must have finished before the call; the call returns after its own writes are
 * done.  *device_ms (may be NULL): first launch -> last kernel done.
 * MS_ERR_RUNTIME without a usable device, before anything else.  MS_ERR_INVALID: NULL handles, sum and per_site both NULL, flags != 0,
 * flank outside [0, MS_SITESIGNAL_MAX_FLANK], a motif range outside [0, P], pwms->P != the result's P, the track's R != the result's R, a
 * track or an output on another device, a counts-only result, and a site with a region index outside [0, R), pos < 0 or pos + W > L (a
 * result of ms_result_from_hits, or the wrong track: checked on the device while reducing, outputs zeroed). */
int ms_result_site_signal(const ms_result *res, const ms_pwmset *pwms, const ms_track *track, int32_t flank, int32_t m0, int32_t m1,
                          uint32_t flags /* 0 */, int64_t *sum /* [(m1 - m0)][2][C], or NULL */, int64_t *cover /* [(m1 - m0)][2][C], or NULL */,
                          int64_t *n_sites /* [(m1 - m0)][2], or NULL */, int64_t *per_site /* [n_sel][3], or NULL */,
                          double *device_ms /* or NULL */);

/* ---- the score distribution of every window (ms_scorehist.hip) ------------------------------------------------ */
#define MS_SCOREHIST_MAX_BINS   4096
#define MS_HIST_PER_POSITION    1u   /* one count per window start: (fwd > rev ? fwd : rev) / max_raw, i.e. c_score (cscore.c:207-223) at every
                                        position; with a one-strand mask it is that strand's score.  Without the flag: one count per
                                        (window, strand of strand_mask), the scores ms_scan compares with the cutoff. */
/* Counts, per motif, the scores of ALL windows of the sequence set in n_bins equal bins: what get_score_cutoffs (motif/__init__.py:378-401)
 * estimates from 10^6 sampled windows scored by c_score (cscore.c:174-229), done exhaustively.  The windows are ms_scan_best's: motif m of
 * width W, region of length L, starts 0 .. L - W, each scored exactly as ms_scan scores it (columns in order, forward M[b][c], reverse
 * M[3 - b][W - 1 - c] at the same step, a non-ACGT base adds +0.0, raw / max_raw as one IEEE fp64 divide).  The set's cutoffs are not read.
 *
 * The bin rule, with d = score - lo[m] as one rounded subtraction and t = d * inv_width[m] as one rounded multiply: t < 0 goes to
 * out[m][0] ("below"; a score of -inf too), t >= n_bins to out[m][n_bins + 1] ("above"), anything else to out[m][1 + (int) floor(t)].
 * A motif that is unscorable -- max_raw is not a finite number > 0, or an entry is NaN or +inf: the reference never reports a site of it --
 * gets an all-zero row; for every other motif no score is NaN and every counted window lands in exactly one slot, so a row sums to the
 * number of counted windows (x the strands of the mask without MS_HIST_PER_POSITION).
 *
 * max_n >= 0: a window with more than max_n non-ACGT bases among its own W bases is not counted at all; max_n < 0: every window counts.
 * This counts bits of the packed "non-ACGT" plane, so IUPAC letters count as well as N / n.  It is NOT the reference's filter
 * (motif/__init__.py:378-401 draws windows of the widest motif's width and rejects on N / n only, for all motifs alike).
 *
 * out: [P x (n_bins + 2)] int64, host memory or device memory of the sequence set's device (then a consumer can all-reduce it where it
 * is).  The library writes a device `out` on its own stream: work the caller has queued on that memory on another stream (a fill, a
 * collective) must have finished before the call; the call returns after its own writes are done.  An exact integer reduction: the same
 * bytes on every run, additive over shards of the regions.  device_ms (may be NULL): first launch -> last kernel done.
 * n_seqs = 0 or P = 0 is valid and gives zeros.  Without a device: MS_ERR_RUNTIME (no CPU fallback), before anything else is looked at.
 * MS_ERR_INVALID: NULL handles or arrays, a strand mask outside 1..3, unknown flags, n_bins outside [1, MS_SCOREHIST_MAX_BINS], a lo that
 * is not finite, an inv_width that is not finite and > 0, an output on another device. */
int ms_scan_score_histogram(const ms_pwmset *pwms, const ms_seqset *seqs, int strand_mask, uint32_t flags,
                            const double *lo /* [P] */, const double *inv_width /* [P] */, int32_t n_bins, int32_t max_n,
                            int64_t *out /* [P][n_bins + 2] */, double *device_ms /* or NULL */);

/* ---- k-mer counts of a sequence set or a resident genome (ms_kmers.hip) ------------------------------------------ */
#define MS_KMER_MAX_K      12
#define MS_KMER_CANONICAL  1u   /* a window counts under min(code, code of its reverse complement) */
/* The k-mer spectrum of the selected sequences, without a motif: what a Markov background of order k - 1, a k-mer enrichment of one region
 * set against another and a check of a shuffled or spliced set's composition are made of.  sel: R flags on the host (0 = leave the
 * sequence out), or NULL for all.
 *
 * The windows of sequence r of length L are the starts p = 0 .. L - k; a window never crosses a sequence end.  A window is COUNTED iff r
 * is selected and none of its k bases has its bit set in the non-ACGT plane (IUPAC letters count as non-ACGT as well as N, as in
 * ms_scan_score_histogram).  The CODE of a counted window puts base j, 0-based from the left, at bits [2(k - 1 - j), 2(k - j)), with
 * A 0, C 1, G 2, T 3 in either case: the first base is most significant, so numeric order is lexicographic order.  Its reverse complement
 * has the code sum_j (3 - b_j) << 2j.  With MS_KMER_CANONICAL the window counts under the smaller of the two (a palindrome, code == rc,
 * even k only, counts once per window); without the flag only the forward code is used.
 *   occ[c]     the number of counted windows of code c; the entries sum to totals[1]
 *   nseq[c]    the number of selected sequences with at least one counted window of code c (NULL: not made)
 *   totals[0]  the selected sequences               totals[1]  the counted windows
 *   totals[2]  the windows of selected sequences that were left out for a non-ACGT base
 *   totals[3]  the selected sequences with L < k    (totals: host, or NULL)
 *
 * occ, nseq: [4^k] int64 each, host memory or device memory of the set's device (then a consumer can all-reduce it where it
 * is).  The library writes a device output on its own stream: work the caller has queued on that memory on another stream (a fill, a
 * collective) must have finished before the call; the call returns after its own writes are done.  The library zeroes both outputs.
 * Exact integer reductions: the same bytes on every run, additive over shards of the sequences -- nseq included, because a sequence lies
 * wholly in one shard -- and independent of every internal tiling, batching and scratch budget.  device_ms (may be NULL): first launch
 * -> last kernel done.
 *
 * nseq is made per sequence: a sequence of up to ms_debug_kmer_dims()[3] windows is sorted by one block in LDS; a longer one gets a bitmap
 * of 4^k bits in pooled device scratch (2 MiB at k = 12), in batches of sequences whose bitmaps fit a budget (64 MiB), cleared per batch.
 * A set of many sequences just above that length at k = 12 is correct but pays the clearing of 2 MiB for each of them: measured, 256
 * sequences of 4207 bases take 0.77 ms with nseq against 0.31 ms without, 1.8 us per sequence; a genome's chromosomes are
 * one batch.
 *
 * MS_ERR_RUNTIME ("no CPU fallback") without a device, before anything else.  MS_ERR_INVALID: a NULL handle or NULL occ, k outside
 * [1, MS_KMER_MAX_K], unknown flags, a set whose planes are not on the device yet (a batch stream's upload-only set, as in
 * ms_seqset_shuffle), an output on another device.  MS_ERR_NOMEM, with nothing launched, when the work memory does not fit.  n_seqs = 0,
 * empty sequences and an all-zero sel are valid and give zeros. */
int ms_seqset_kmer_counts(const ms_seqset *seqs, int32_t k, uint32_t flags, const uint8_t *sel /* [R] host, or NULL: all */,
                          int64_t *occ /* [4^k] */, int64_t *nseq /* [4^k], or NULL */, int64_t *totals /* [4] host, or NULL */,
                          double *device_ms /* or NULL */);
/* The same over a resident genome, whose sequences are its chromosomes (sel_chrom: n_chroms flags): cal_bg_freq (genome/__init__.py:179-220)
 * is k = 1 without the flag, summed over the chromosomes. */
int ms_genome_kmer_counts(const ms_genome *genome, int32_t k, uint32_t flags, const uint8_t *sel_chrom /* [n_chroms] or NULL */,
                          int64_t *occ, int64_t *nseq, int64_t *totals, double *device_ms);

/* ---- the analytic score distribution under a Markov background (ms_scoredist.hip) ------------------------------- */
#define MS_SCOREDIST_MAX_ORDER 5
#define MS_SCOREDIST_MAX_BINS  (1 << 20)
/* The distribution of a window's score from the matrix and a background model alone, no sequence: for every motif the probability of
 * each INTEGER score of a window of W ACGT bases whose `order` preceding bases are distributed as init and whose every base is drawn by
 * cond.  cond [4^order][4] is the conditional table of the background (row = the code of the last `order` bases, oldest base most
 * significant: the k-mer code rule of ms_seqset_kmer_counts, so cond is KmerCounts.markov() of the (order + 1)-mer counts); init
 * [4^order] the distribution of the context in front of the window.  C = 4^order contexts.  Neither is normalised or checked to sum to 1.
 *
 * THE SCORE GRID, made on the host in plain fp64, per motif m of width W with entries M[b][c]:
 *   unscorable   max_raw (get_max_raw_score, cscore.c:36-48) is not a finite number > 0, an entry is NaN or +inf, or a column has no
 *                finite entry: step[m] = 0, s0[m] = 0 and the row of mass is all +0.0.
 *   range        over the finite entries only: hi = sum_c max_b M[b][c], lo = sum_c min_b M[b][c], columns in order, one rounded add
 *                each.  step = (hi - lo) / (n_bins - W - 2) (one subtraction, one divide), or 1.0 when hi == lo.
 *   entries      q[b][c] = (int64) floor(M[b][c] / step): one rounded divide, then floor.  An entry of -inf is ABSENT: the mass that
 *                would pass through it is dropped.  s0 = sum_c min_b q[b][c] and d[b][c] = q[b][c] - min_b' q[b'][c] >= 0 (the minima
 *                over the column's present entries).
 *   fit          sum_c max_b d[b][c] < n_bins follows from the choice of step; the plan asserts it and the call returns
 *                MS_ERR_INTERNAL where it does not hold (entries so large against their range that q leaves the int64 range).
 *   strand 2     the same q, d, step and s0, run through the columns of M'[b][c] = M[3 - b][W - 1 - c].
 *
 * THE RECURRENCE, over arrays [C][n_bins] of doubles: old[ctx][0] = init[ctx], every other entry +0.0.  For each column c = 0 .. W - 1,
 * each new context x and each i in [0, n_bins), with b = x & 3 and the predecessors p_a = a * 4^(order - 1) + (x >> 2), a = A, C, G, T:
 *     new[x][i] = ((t_A + t_C) + t_G) + t_T,     t_a = old[p_a][i - d[b][c]] * cond[p_a][b],
 * t_a = +0.0 where i - d[b][c] < 0 or the entry (b, c) is absent.  At order 0 there is one context and the four terms run over
 * b = A, C, G, T, each with its own shift: t_b = old[0][i - d[b][c]] * cond[0][b].  Every product and every sum is ONE IEEE fp64
 * operation (no FMA).  mass[m][i] = the sum of the last column's new[x][i] over x = 0 .. C - 1, left to right: the probability that the
 * window's integer score sum_c q[b_c][c] is s0[m] + i.  1 - the row's sum is the probability of a score of -inf.  Every element is this
 * expression whatever path, tile, batch or budget computes it: the same bytes on every run, and the bytes of the Python restatement
 * (motifscan_amd.pvalues.restate_distribution).
 *
 * How a raw sum R of the scan (fp64, columns in order) relates to the integer score S of the same window: step (S - 1) <= R <=
 * step (S + W + 1) for every n_bins up to MS_SCOREDIST_MAX_BINS (DESIGN.md 4 has the proof), which is what P-value bounds and
 * conservative cutoffs are made of (motifscan_amd/pvalues.py).
 *
 * Two paths, the same bytes: a motif whose two buffers (2 C n_bins 8 bytes) fit the LDS of a CU runs all its columns in ONE launch,
 * one block per motif; otherwise the buffers lie in pooled device scratch and every column is one launch over all motifs of a batch,
 * followed by one launch for the context sum.  The motifs are taken in batches whose buffers fit a work budget (256 MiB; on either
 * path, so that the status does not depend on the path).
 *
 * step, s0: [P] host.  mass: [P][n_bins] doubles, host memory or device memory of the calling thread's device (ms_set_device), written
 * under the stream rule ms_scan_score_histogram documents.  device_ms (may be NULL): first launch -> last kernel done.  P = 0 is valid.
 * MS_ERR_RUNTIME ("no CPU fallback") without a device, before anything else is looked at.  MS_ERR_INVALID: NULL handles or arrays, strand
 * outside {1, 2}, order outside [0, MS_SCOREDIST_MAX_ORDER], n_bins outside [max_width + 3, MS_SCOREDIST_MAX_BINS], a cond or init entry
 * that is negative or not finite, a device mass on another device.  MS_ERR_NOMEM, with nothing launched, when one motif's two buffers do
 * not fit the work budget. */
int ms_pwmset_score_distribution(const ms_pwmset *pwms, int strand /* 1 forward, 2 reverse */, int32_t order,
                                 const double *cond /* [4^order][4] host */, const double *init /* [4^order] host */,
                                 int32_t n_bins, double *step /* [P] host */, int64_t *s0 /* [P] host */,
                                 double *mass /* [P][n_bins], host or device */, double *device_ms /* or NULL */);

/* ---- motif sets compared with each other: best alignment and P-value per pair (ms_compare.hip) ------------------- */
#define MS_COMPARE_PEARSON 0
#define MS_COMPARE_SW      1      /* Sandelin-Wasserman: 2 - sum of squared differences */
#define MS_COMPARE_ED      2      /* minus the Euclidean distance */
#define MS_COMPARE_MAX_WIDTH 64
#define MS_COMPARE_MAX_BINS  256
/* Which target motif does a query motif resemble, at which offset and in which orientation, and how likely is so good a match by
 * chance: the Tomtom procedure (Gupta et al., Genome Biology 2007).  Every ungapped alignment of the two matrices is scored column
 * against column, each alignment score becomes a P-value under a null built from the target set's own columns, the best alignment is
 * kept.  q_values / t_values are the matrices concatenated, each row-major [4][width] with rows A, C, G, T (ms_pwmset_create's layout):
 * probability columns, but nothing is checked beyond "finite".
 *
 * THE COLUMNS AS THE DEVICE SEES THEM, prepared on the host in plain fp64, one rounded operation per step.  For a column x:
 *   pearson   mean = (((x0 + x1) + x2) + x3) * 0.25;  c_b = x_b - mean;  n = sqrt(((c0 c0 + c1 c1) + c2 c2) + c3 c3);  u_b = c_b / n, or all
 *             +0.0 where n > 0 does not hold
 *   sw, ed    u = x
 * The REVERSE orientation of a target is made from the prepared vectors: column j of the reversed target is prepared column Wt - 1 - j
 * with its four entries in reverse order.  (Not "prepare the reverse complement": the order of the mean's additions would differ.)
 *
 * THE COLUMN SCORE, on the device, every product, sum, difference and square root one IEEE fp64 operation (no FMA), for a query vector u
 * and a target vector v:
 *   pearson   g = ((u0 v0 + u1 v1) + u2 v2) + u3 v3
 *   sw, ed    d_b = u_b - v_b;  ssd = ((d0 d0 + d1 d1) + d2 d2) + d3 d3;  sw: g = 2.0 - ssd;  ed: g = -sqrt(ssd), correctly rounded
 * and the integer score k = (int) floor((g - lo) * scale), clamped to [0, bins - 1] (a NaN gives 0), with the host doubles
 *   pearson lo = -1.0, scale = bins * 0.5;   sw lo = 0.0, scale = bins * 0.5;   ed lo = -sqrt(2.0), scale = bins / sqrt(2.0).
 *
 * THE NULL OF ONE QUERY COLUMN i: H_i[k] = the number of target columns c with score(i, c) = k, over all sum Wt forward columns of the
 * whole target set, and over their reversed forms as well when orientations == 3; N is that number of columns (sum Wt <= 2^30), H exact
 * uint32.  f_i[k] = (double) H_i[k] * invN with invN = 1.0 / (double) N made on the host: one multiply.
 *
 * THE TABLES OF ONE QUERY of width W: for every start a and length L with a + L <= W, over the scores s in [0, L (bins - 1)],
 *   pm_{a,1} = f_a
 *   pm_{a,L}[s] = the sum over k = 0 .. bins - 1 with 0 <= s - k <= (L - 1)(bins - 1) of pm_{a,L-1}[s - k] * f_{a+L-1}[k], the terms in
 *                 ascending k, each product and each sum one rounded operation, starting from +0.0
 *   tail_{a,L}[top] = pm_{a,L}[top],  tail_{a,L}[s] = tail_{a,L}[s + 1] + pm_{a,L}[s]: summed from the top down, sequentially.
 * They depend on the query and on the whole target set, not on q0, q1, batches or paths.
 *
 * THE ALIGNMENT of query q (width Wq) and target t (width Wt): offset o runs over [-(Wt - 1), Wq - 1]; target column j lies under query
 * column i = j + o; the overlap is a = max(0, o) to e = min(Wq, Wt + o), L = e - a; an alignment is admissible when
 * L >= min(min_overlap, Wq, Wt).  S = the sum of the L integer column scores, p = tail_{a,L}[S].  Over all admissible (orientation, o)
 * the least key (p, -L, orientation [forward first], o) is kept.  Per pair: p_min the kept p (the table's bytes), offset the kept o,
 * overlap the kept L, score the kept S, orient 0 forward / 1 reverse, n_offsets the number of admissible alignments (always >= 1).  The
 * correction 1 - (1 - p_min)^n_offsets, E-values and q-values are host arithmetic (motifscan_amd/compare.py).
 *
 * The six outputs are host planes [(q1 - q0)][n_t] for the queries [q0, q1).  Every element is the expressions above whatever tile or
 * batch computes it: the same bytes on every run, and the bytes of the Python restatement (motifscan_amd.compare.restate_compare).  The
 * queries are taken in batches whose tables fit a work budget (256 MiB); a query of width W holds sum over n = 1 .. W of
 * ((bins - 1) n (n + 1) / 2 + n) doubles, 89 MiB at the caps.  device_ms (may be NULL): first launch -> last kernel done.
 *
 * MS_ERR_RUNTIME ("no CPU fallback") without a device, before anything else is looked at.  MS_ERR_INVALID: NULL arrays where a count is
 * non-zero, a negative count, a width outside [1, MS_COMPARE_MAX_WIDTH], an entry that is not finite, a metric outside 0..2, bins outside
 * [2, MS_COMPARE_MAX_BINS], min_overlap < 1, orientations not 1 or 3, q0 < 0, q1 > n_q or q0 > q1, sum Wt > 2^30 (or more than 2^30 query
 * columns in [q0, q1)).  n_q == 0, n_t == 0 and q0 == q1 are valid and write nothing.  MS_ERR_NOMEM, with nothing launched, if one
 * query's tables do not fit the work budget.  No status writes to the outputs. */
int ms_motifs_compare(const double *q_values, const int32_t *q_widths, int32_t n_q,
                      const double *t_values, const int32_t *t_widths, int32_t n_t,
                      int metric, int32_t bins, int32_t min_overlap, int orientations /* 1 forward, 3 both */,
                      int32_t q0, int32_t q1,
                      double *p_min, int32_t *offset, int32_t *overlap, int32_t *score, int32_t *n_offsets, int8_t *orient,
                      double *device_ms /* or NULL */);

#ifdef __cplusplus
}
#endif
#endif /* MOTIFSCAN_AMD_H */
