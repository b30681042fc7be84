"""
motifscan_amd -- MI355X-native drop-in for ONE hot path of shao-lab/MotifScan: the PWM scan
(`motifscan.scanner.Scanner.scan_motifs` -> `motifscan.motif.cscore.c_scan_motif`) and its sibling
`c_score`, behind the C-ABI in include/motifscan_amd.h.

    motifscan_amd.cscore    c_scan_motif / c_score with the reference's signatures
    motifscan_amd.scanner   Scanner / MotifSite / make_motif_sites / deduplicate_motif_sites
    motifscan_amd.matrix    PFM -> PPM -> PWM log-odds definitions
    motifscan_amd.annotation  Gene / Genes / RefGeneTxtParser / read_gene_annotation (genome/annotation.py)
    motifscan_amd.regions   GenomicRegion / RegionArray / subset_by_location / generate_control_regions / dis_to_nearest_gene
    motifscan_amd.dist      region sharding over the GPUs of a node + the one all-reduce
    motifscan_amd.synth     seeded synthetic workloads (bench.py, tests)
    motifscan_amd.shuffle   the sequential restatement of ms_seqset_shuffle (mono- and dinucleotide shuffled controls), numpy only
    motifscan_amd.kmers     k-mer codes, the restatement of ms_seqset_kmer_counts, Markov backgrounds, k-mer enrichment, seed matrices
    motifscan_amd.footprint signal tracks over sites: host Track constructors, footprint profiles and per-site flank / core sums
                            (ms_result_site_signal), and their sequential restatement
    motifscan_amd.em        motif refinement without a cutoff: expected base counts per motif column over all windows
                            (ms_affinity_expected_counts, the E-step), their numpy restatement and mpmath reference, the M-step, the loop
    motifscan_amd.dimodel   first-order motif models (a column's score depends on the base before it): DiModel and its constructors from a
                            PWM, from counts and from a site stack, and the numpy restatement of ms_scan_best_dimodels
    motifscan_amd.bipartite bipartite motifs (two half-sites of a PWM set, a spacer of variable length, a fixed relative orientation): the
                            Bipartite spec, specs from a pair-spacing histogram, and the numpy restatement of ms_scan_best_bipartite

There is no CPU fallback anywhere in this package.
"""
__version__ = "0.1.0"
