"""
Randomised parity fuzzer: HIP path (through the C-ABI) vs the oracle on seeded random cases built
to sit ON the decision boundary of cscore.c:360-389 (`score / max_raw - cutoff >= -1e-10`):

  * matrices with few distinct values (integers, halves, one repeated value) so many windows tie;
  * cutoffs placed exactly on attainable scores (k / max_raw), one ulp either side of them, and
    1e-10 either side (the reference's own slack);
  * widths 1..66 (every k-block class of the pre-filter, and the all-fp64 kernel past 63 columns), all-negative matrices (max_raw == 0),
    huge / tiny magnitudes, cutoffs <= 0 (everything hits) and > 1 (nothing can);
  * sequences with N runs, lower case, other IUPAC letters, empty and shorter-than-W regions;
  * (round 6) every case also through MS_SCAN_COUNTS_ONLY and through a two-batch stream with the 12-byte copy-out.

The same matrices, sequences and cutoffs feed five more families, one per entry point that judges windows with a decision of its own
or hands them out by one; a seventh family has no scan in it:

  * --sweep     ms_scan_sweep: one chromosome, random window / stride, against the oracle over the windows as separate regions;
  * --sweep-counts  the same cases as spans of a MS_STREAM_NO_HITS stream: the counts-only hand-out, its per-motif site and window numbers;
  * --variants  ms_scan_variants: single-base substitutions (duplicates, any order, alt letters that add nothing) on a resident genome,
                against the oracle over the ref and alt flank of every variant -- all-pass for the scores, the real cutoff for the states;
  * --alleles   ms_scan_alleles: alleles of 0..40 bases incl. insertions behind the last base, REF strings on even seeds;
  * --best      ms_scan_best: the first window of the greatest score per (motif, region), regions of up to three segments, run twice;
  * --once      ms_scan_regions_once: overlapping, nested, touching, duplicate and empty regions of a resident genome in five layouts
                (summit windows, tiny regions beside chromosome-long ones, jittered tilings, shared starts, uniform), against the oracle
                over the regions cut as strings: as is, run twice, with the span hits keyed by global positions, every third seed under
                MS_SCAN_EXACT_ONLY, odd seeds de-duplicated; the tally counts the windows that end flush with a region, stick out of one
                by a base or start a base in front of one, and which form of hit key the spans take by themselves.

  * --plot      ms_result_site_histogram and ms_result_rank_profile over synthetic hit arrays (ms_result_from_hits; no oracle): centres on a
                bin edge and half a base pair or one either side, on and around the first and the closed last edge and far outside the
                window; region counts on the rank words' and the profile tile's edges, windows both sides of the LDS histogram's limit;
                rows without a site and with one in every region, ranks with tied scores; counts and unsmoothed profiles exact, smoothed
                profiles within 16 * 2^-53 of the exact sum.

  * --genome    the kernels in front of and behind the scan on a resident genome (no scan): pack_kernel / blk2reg_kernel / extract_kernel
                read back plane for plane (ms_debug_seqset_planes) against the host packer -- set sizes on the unit and block edges, ASCII
                at unaligned device addresses, every source phase against every output phase, empty and one-base regions, more than 32
                regions in one unit; ms_genome_base_counts against numpy counts over genomes of a tile - 1 .. 2 tiles + 1 bases whose
                chromosomes end on every bit of a unit, on and across the tile edges, past the LDS counters by number and by empty
                neighbours; ms_genome_window_filter against N / n counts of the byte slices with exceptions on both window ends, counts
                on max_n and one above, n_want either side of the accepted count, candidate counts on the wave and block edges;
                ResidentGenome.random_windows against the restated sampler, the global RandomState included; ms_score by bits against the
                oracle and ms_score_ranks against the sorted oracle row, in one batch, in batches of one motif and of three.
  * --annot     ms_genes_nearest_tss against the reference's recurrence restated (chromosomes of 0 .. 2 tiles + 1 genes; one lane, one wave
                or nothing of a block live behind the first LDS tile; distances equal to the running minimum and one either side; five
                cutoffs) and ms_genes_promoter_overlap against the literal binary search (regions on and one base off an interval's ends,
                empty and inverted regions, extents that sum to 0 and below, one table switched between two extent pairs and back).

Each of --variants, --alleles, --best and --once is make_<x>_case(seed) (inputs), expected_<x>(oracle, case) (expected arrays and a tally; neither needs a GPU) and
run_<x>_case(seed, oracle, _lib) (the device call, compared exactly: integers by value, scores by their bits).  Odd seeds of the variant
and allele families run in chunks of 7 variants.  The plot family is split the same way, but its expected_plot(case) needs no oracle; so are the genome and annot families, whose cases take
every boundary size from the library's own constants (ms_debug_genome_dims).
CONDITIONS holds what the seeds of a family must put on the boundary.

It lives under tests/ because it uses the oracle (test infrastructure).  Run on the GPU box:
    python tests/fuzz_parity.py --cases 200 --seed 0
    python tests/fuzz_parity.py --variants --cases 30        (likewise --alleles, --best, --sweep, --sweep-counts, --once, --plot, --genome, --annot; each prints its tallies)
`tests/test_gpu_parity.py::test_fuzz_decision_boundary` runs a few cases of ms_scan's family in the GPU suite,
tests/test_gpu_fuzz_entry_points.py the next four and the plot, genome and annot families, tests/test_gpu_scan_once.py the scan-once family; tests/test_fuzz_cases_host.py checks the cases
themselves without a GPU.
"""
import argparse
import contextlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def random_matrix(rng, w):
    kind = rng.integers(0, 8)
    if kind == 0:                                   # small integers: masses of exact ties
        m = rng.integers(-3, 4, size=(4, w)).astype(np.float64)
    elif kind == 1:                                 # halves / quarters (exact in binary)
        m = rng.integers(-8, 9, size=(4, w)) / 4.0
    elif kind == 2:                                 # log-odds-like, rounded as the reference's files are
        p = rng.dirichlet(np.full(4, rng.choice([0.2, 1.0, 5.0])), size=w).T
        m = np.round(np.log2(np.maximum(p, 1e-4) / 0.25), 6)
    elif kind == 3:                                 # huge magnitudes
        m = rng.normal(0, 1, size=(4, w)) * 10.0 ** rng.integers(2, 7)
    elif kind == 4:                                 # tiny magnitudes
        m = rng.normal(0, 1, size=(4, w)) * 10.0 ** -rng.integers(3, 9)
    elif kind == 5:                                 # all negative: max_raw == 0
        m = -np.abs(rng.normal(0, 1, size=(4, w))) - 0.01
    elif kind == 6:                                 # one informative column, the rest flat
        m = np.zeros((4, w))
        m[:, rng.integers(0, w)] = rng.normal(0, 2, size=4)
    else:                                           # one strong base per column, mixed penalties
        m = np.full((4, w), -float(rng.integers(1, 6)))
        m[rng.integers(0, 4, size=w), np.arange(w)] = float(rng.integers(1, 3))
    return np.ascontiguousarray(m, dtype=np.float64)


def max_raw_of(m):
    return float(np.sum(np.maximum(m.max(axis=0), 0.0)))


def random_sequences(rng, n, max_len):
    out = []
    for _ in range(n):
        kind = rng.integers(0, 10)
        L = int(rng.integers(0, max_len + 1))
        if kind == 0:
            s = ""
        elif kind == 1:
            s = "ACGT"[rng.integers(0, 4)] * L
        elif kind == 2:
            unit = "".join(rng.choice(list("ACGT"), size=int(rng.integers(1, 5))))
            s = (unit * (L // len(unit) + 1))[:L]
        else:
            p = np.array([.24, .24, .24, .24, .03, .01])
            s = "".join(rng.choice(list("ACGTNR"), p=p, size=L))
            if kind == 3 and L > 10:
                a = int(rng.integers(0, L - 5))
                s = s[:a] + "N" * int(rng.integers(1, 40)) + s[a:]
            if kind == 4:
                s = s.lower()
            elif kind == 5:
                s = "".join(c.lower() if rng.random() < 0.3 else c for c in s)
        out.append(s)
    return out


def attainable_cutoff(rng, m, seqs):
    """A cutoff sitting on (or a hair beside) the ratio of a window that really occurs."""
    w = m.shape[1]
    mr = max_raw_of(m)
    cands = [s for s in seqs if len(s) >= w and set(s.upper()) <= set("ACGT")]
    if mr <= 0 or not cands or rng.random() < 0.15:
        return float(rng.choice([-0.2, 0.0, 0.3, 0.8, 1.0, 1.0 + 1e-12, 1.3]))
    s = cands[rng.integers(0, len(cands))].upper()
    a = int(rng.integers(0, len(s) - w + 1))
    score = 0.0
    for c in range(w):                              # same summation order as cscore.c:352-358
        score += m["ACGT".index(s[a + c]), c]
    ratio = score / mr
    nudge = rng.integers(0, 7)
    if nudge == 0:
        return ratio
    if nudge == 1:
        return float(np.nextafter(ratio, np.inf))
    if nudge == 2:
        return float(np.nextafter(ratio, -np.inf))
    if nudge == 3:
        return ratio + 1e-10
    if nudge == 4:
        return ratio + 1.0000001e-10
    if nudge == 5:
        return ratio + 0.9999999e-10
    return float(np.round(ratio, 8))                # what `motif --build` writes (np.around(, 8))


def make_case(seed):
    rng = np.random.default_rng(seed)
    n_motifs = int(rng.choice([1, 2, 5, 13, 40, 97, 200]))
    wmax = int(rng.choice([8, 16, 32, 40, 66]))            # 66: row tiles of 3 and 4 k-blocks, and the all-fp64 kernel past 63 columns
    mats = [random_matrix(rng, int(rng.integers(1, wmax + 1))) for _ in range(n_motifs)]
    seqs = random_sequences(rng, int(rng.choice([1, 7, 60, 300])), int(rng.choice([20, 150, 700])))
    cutoffs = np.array([attainable_cutoff(rng, m, seqs) for m in mats], dtype=np.float64)
    strand = int(rng.integers(1, 4))
    return mats, cutoffs, seqs, strand


def check_dedup_and_score(seed, oracle, _lib, mats, widths, seqs, strand, want, pw, res):
    """Device de-dup (ms_result_dedup) vs the oracle's restatement of scanner.py:156-193 on the nested
    lists (cases small enough for Python lists), and ms_score vs oracle_score on the regions long
    enough for every motif (shorter ones read out of bounds in the reference, cscore.c:196-204)."""
    if len(want["pos"]) <= 150_000:
        off = want["motif_offsets"]
        cols = [want[k].tolist() for k in ("seq_idx", "pos", "score", "strand")]
        nested = [[[cols[0][k], cols[1][k], cols[2][k], cols[3][k]] for k in range(off[p], off[p + 1])]
                  for p in range(len(widths))]
        dd = oracle.deduplicate_motif_sites(oracle.make_motif_sites(nested, [0] * len(seqs)), widths.tolist())
        flat = [(p, r, s.start, s.score, 1 if s.strand == "+" else 2)
                for p, per in enumerate(dd) for r, sites in enumerate(per) for s in sites]
        res.dedup(pw)
        d = res.hits()
        motif = np.repeat(np.arange(len(widths)), np.diff(d["motif_offsets"]))
        mine = list(zip(motif.tolist(), d["seq_idx"].tolist(), d["pos"].tolist(), d["score"].tolist(),
                        d["strand"].astype(np.int32).tolist()))
        if mine != flat:
            return f"seed {seed}: de-duplicated sites differ ({len(mine)} vs {len(flat)})"
    wmax = int(widths.max())
    long_seqs = [s for s in seqs if len(s) >= wmax]
    if long_seqs:
        raw = "".join(long_seqs).encode()
        offsets = np.concatenate([[0], np.cumsum([len(s) for s in long_seqs])]).astype(np.int64)
        vals = np.concatenate([m.ravel() for m in mats])
        sq = _lib.SeqSet(raw, offsets)
        try:
            got = _lib.score(pw, sq, strand)
        finally:
            sq.close()
        ref = oracle.score_arrays(vals, widths, raw, offsets, strand, 4)
        if not np.array_equal(got, ref, equal_nan=True):
            return f"seed {seed}: c_score differs"
    return None


def check_round6_paths(seed, _lib, raw, offsets, strand, want, pw, sq):
    """Round 6's paths on the same case: MS_SCAN_COUNTS_ONLY (n_hits, per-motif site numbers, per-motif region counts from the UNORDERED hits,
    or from the ordered path where the flag map does not apply) and the batch stream with the 12-byte copy-out (two batches cut at a random
    region; packing on the scan stage; the second batch counts-only every other seed)."""
    n_motifs = len(want["motif_offsets"]) - 1
    want_regions = expected_counts(want, n_motifs)[2]
    co = _lib.scan(pw, sq, strand, _lib.MS_SCAN_COUNTS_ONLY)
    try:
        if co.n_hits != len(want["pos"]) or not np.array_equal(co.motif_offsets, want["motif_offsets"]) or not np.array_equal(co.region_counts(), want_regions):
            return f"seed {seed}: counts-only scan differs"
    finally:
        co.close()
    R = len(offsets) - 1
    if R < 2:
        return None
    cut = 1 + seed % (R - 1)
    second_counts_only = seed % 2 == 1
    b = np.frombuffer(raw, dtype=np.uint8)
    batches = [(b[:int(offsets[cut])], offsets[:cut + 1].copy(), False), (b[int(offsets[cut]):], offsets[cut:] - offsets[cut], second_counts_only)]
    parts, counts = [], np.zeros(n_motifs, dtype=np.int64)
    for (bb, oo, co_), start, res in zip(batches, (0, cut), _lib.scan_stream(pw, iter(batches), strand, packed=12)):
        counts += res.region_counts()
        if not co_:
            parts.append((res.hits(packed=True), start))
        res.close()
    if not np.array_equal(counts, want_regions):
        return f"seed {seed}: the stream's region counts differ"
    merged = _lib.merge_hits(parts, n_motifs)
    sel = np.ones(len(want["pos"]), dtype=bool) if not second_counts_only else want["seq_idx"] < cut
    for k in ("seq_idx", "pos", "score"):
        if not np.array_equal(merged[k], want[k][sel]):
            return f"seed {seed}: the 12-byte stream's {k} differ"
    if not np.array_equal(merged["strand"].astype(np.int32), want["strand"].astype(np.int32)[sel]):
        return f"seed {seed}: the 12-byte stream's strands differ"
    return None


def run_case(seed, oracle, _lib):
    mats, cutoffs, seqs, strand = make_case(seed)
    vals = np.concatenate([m.ravel() for m in mats])
    widths = np.array([m.shape[1] for m in mats], dtype=np.int32)
    raw = "".join(seqs).encode()
    offsets = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64)
    want = oracle.scan_arrays(vals, widths, cutoffs, raw, offsets, strand, 4)
    pw, sq = _lib.PwmSet(vals, widths, cutoffs), _lib.SeqSet(raw, offsets)
    res = _lib.scan(pw, sq, strand)
    try:
        got = {k: v.copy() for k, v in res.hits().items()}
        st = res.stats()
        extra = check_round6_paths(seed, _lib, raw, offsets, strand, want, pw, sq)
        extra = extra or check_dedup_and_score(seed, oracle, _lib, mats, widths, seqs, strand, want, pw, res)
    finally:
        res.close()
        sq.close()
        pw.close()
    if extra:
        return False, extra, st
    for k in ("motif_offsets", "seq_idx", "pos"):
        if not np.array_equal(got[k], want[k]):
            return False, f"seed {seed}: {k} differs ({len(got['pos'])} vs {len(want['pos'])} hits)", st
    if not np.array_equal(got["strand"].astype(np.int32), want["strand"].astype(np.int32)):
        return False, f"seed {seed}: strand differs", st
    if not np.array_equal(got["score"], want["score"]):
        return False, f"seed {seed}: scores differ (max abs {np.max(np.abs(got['score'] - want['score']))})", st
    return True, len(want["pos"]), st


def make_sweep_case(seed):
    """The sweep family's inputs (no GPU): motifs, cutoffs on attainable scores, one chromosome, a span of it and window / stride
    incl. stride > window and windows narrower than motifs; `seqs` are the windows as separate regions."""
    rng = np.random.default_rng(1_000_003 * 7 + seed)
    n_motifs = int(rng.choice([1, 3, 20, 60]))
    mats = [random_matrix(rng, int(rng.integers(1, 34))) for _ in range(n_motifs)]
    L = int(rng.choice([50, 400, 3000]))
    kind = rng.integers(0, 4)
    if kind == 0:
        unit = "".join(rng.choice(list("ACGT"), size=int(rng.integers(1, 4))))
        chrom = (unit * (L // len(unit) + 1))[:L]                       # low complexity: dense neighbourhoods
    else:
        chrom = "".join(rng.choice(list("ACGTNacgt"), p=[.22, .22, .22, .22, .04, .02, .02, .02, .02], size=L))
    window = int(rng.choice([5, 12, 30, 64, 200]))
    stride = int(rng.choice([1, 3, 7, 25, 50, 300]))
    begin = int(rng.integers(0, max(1, L // 4)))
    end = int(rng.integers(begin, L + 1))
    n_win = (end - begin - window) // stride + 1 if end - begin >= window else 0
    if n_win > 20000:
        stride = max(stride, (end - begin) // 20000 + 1)
        n_win = (end - begin - window) // stride + 1
    seqs = [chrom[begin + k * stride: begin + k * stride + window] for k in range(n_win)]
    cutoffs = np.array([attainable_cutoff(rng, m, seqs[:50] + [chrom]) for m in mats], dtype=np.float64)
    strand = int(rng.integers(1, 4))
    return {"mats": mats, "cutoffs": cutoffs, "chrom": chrom, "begin": begin, "end": end, "window": window, "stride": stride,
            "n_win": n_win, "seqs": seqs, "strand": strand}


def expected_sweep(oracle, case):
    """(flat matrix values, widths, the oracle's hits over the windows as separate regions); no GPU."""
    vals = np.concatenate([m.ravel() for m in case["mats"]])
    widths = np.array([m.shape[1] for m in case["mats"]], dtype=np.int32)
    raw = "".join(case["seqs"]).encode()
    offsets = np.arange(case["n_win"] + 1, dtype=np.int64) * case["window"]
    return vals, widths, oracle.scan_arrays(vals, widths, case["cutoffs"], raw, offsets, case["strand"], 4)


def sweep_tally(seed, oracle):
    """What a sweep case holds, from the oracle alone: its number of windows, the sites to compare and its kinds of motif."""
    case = make_sweep_case(seed)
    want = expected_sweep(oracle, case)[2]
    return {"n_win": case["n_win"], "sites": len(want["pos"]), "cases_without_windows": int(case["n_win"] == 0), **motif_kinds(case["mats"])}


def run_sweep_case(seed, oracle, _lib):
    """ms_scan_sweep (every base scored once, hits handed to the windows that hold them) vs the oracle over the same
    windows as separate regions."""
    case = make_sweep_case(seed)
    mats, cutoffs, chrom, strand = case["mats"], case["cutoffs"], case["chrom"], case["strand"]
    begin, end, window, stride, n_motifs = case["begin"], case["end"], case["window"], case["stride"], len(mats)
    vals, widths, want = expected_sweep(oracle, case)
    genome = _lib.ResidentGenome({"x": "ACGT" * 3, "chr": chrom})
    pw = _lib.PwmSet(vals, widths, cutoffs)
    res = _lib.scan_sweep(pw, genome, "chr", begin, end, window, stride, strand)
    try:
        got = {k: v.copy() for k, v in res.hits().items()}
        counts = res.region_counts()
    finally:
        res.close()
        pw.close()
        genome.close()
    for k in ("motif_offsets", "seq_idx", "pos", "score"):
        if not np.array_equal(got[k], want[k]):
            return False, f"sweep seed {seed}: {k} differs ({len(got['pos'])} vs {len(want['pos'])} sites)"
    if not np.array_equal(got["strand"].astype(np.int32), want["strand"].astype(np.int32)):
        return False, f"sweep seed {seed}: strand differs"
    if not np.array_equal(counts, expected_counts(want, n_motifs)[2]):
        return False, f"sweep seed {seed}: window counts differ"
    return True, len(want["pos"])


def span_counts(_lib, pw, span, window, stride, strand, flags):
    """(n_hits, motif_offsets, region_counts, hits() refused as a counts-only result) of one span through a stream of these flags."""
    st = _lib.Stream(pw, strand, flags, depth=1)
    try:
        st.submit_span(np.frombuffer(span.encode(), dtype=np.uint8), window, stride)
        res = st.next()
        try:
            refused = False
            try:
                res.hits()
            except ValueError as e:
                refused = "counts-only" in str(e)
            return res.n_hits, res.motif_offsets.copy(), res.region_counts(), refused
        finally:
            res.close()
    finally:
        st.close()


def run_sweep_counts_case(seed, oracle, _lib, case=None):
    """The counts-only hand-out of a sweep span (sweep_countonly_kernel, behind MS_STREAM_NO_HITS) on the sweep family's cases: the span
    chrom[begin:end] through a stream, its n_hits, per-motif site numbers and per-motif window counts against the oracle over the windows
    as separate regions; all zero where the span holds no window; no site arrays; and the same numbers under MS_STREAM_DEDUP, which
    leaves a counts-only span as it is.  case: a dict like make_sweep_case's in place of the seed's own."""
    case = case or make_sweep_case(seed)
    n_motifs = len(case["mats"])
    vals, widths, want = expected_sweep(oracle, case)
    n_hits, offsets, counts = expected_counts(want, n_motifs)
    span = case["chrom"][case["begin"]:case["end"]]
    pw = _lib.PwmSet(vals, widths, case["cutoffs"])
    try:
        for flags in (_lib.MS_STREAM_NO_HITS, _lib.MS_STREAM_NO_HITS | _lib.MS_STREAM_DEDUP):
            got = span_counts(_lib, pw, span, case["window"], case["stride"], case["strand"], flags)
            what = f"sweep-counts seed {seed} (stream flags {flags})"
            if got[0] != n_hits or not np.array_equal(got[1], offsets):
                return False, f"{what}: site numbers differ ({got[0]} vs {n_hits} sites)"
            if not np.array_equal(got[2], counts):
                return False, f"{what}: window counts differ"
            if case["n_win"] == 0 and (got[0] or got[1].any() or got[2].any()):
                return False, f"{what}: counts of a span without a window"
            if not got[3]:
                return False, f"{what}: hits() did not refuse a counts-only span"
    finally:
        pw.close()
    return True, n_hits


# ------------------------------------------------------------------------------------------------ variants, alleles, best sites
#
# Each family: make_<x>_case(seed) builds the inputs, expected_<x>(oracle, case) the expected arrays and a tally dict (neither uses a
# GPU), run_<x>_case(seed, oracle, _lib) makes the device call.  Every comparison is exact: integers by value, scores by their bits.

def expected_counts(want, P):
    """counts_cases.expected_counts (imported late: that module reads this one's constants)."""
    from counts_cases import expected_counts as f
    return f(want, P)


ALL_PASS = -1e30
NEAR = 2e-10                                            # a scored window is "near" when its score is within this of the motif's cutoff
ALT_LETTERS = "ACGTACGTNacgtR"
VARIANT_STREAM, ALLELE_STREAM, BEST_STREAM, ONCE_STREAM, PLOT_STREAM = 2_000_003 * 11, 3_000_017 * 13, 5_000_011 * 17, 7_000_003 * 23, 11_000_027 * 29
GENOME_STREAM, ANNOT_STREAM = 13_000_027 * 31, 17_000_023 * 37


def motif_kinds(mats):
    """How many of the motifs are of the kinds every family has to meet: max_raw == 0, 64 columns or more, one column."""
    return {"max_raw_zero": sum(max_raw_of(m) == 0 for m in mats), "wide": sum(m.shape[1] >= 64 for m in mats),
            "width_one": sum(m.shape[1] == 1 for m in mats)}


def add_tally(total, tally):
    """Sum a case's tally into a running one: numbers are added, sets (what was seen) united."""
    for k, v in tally.items():
        if isinstance(v, (set, frozenset)):
            total[k] = total.get(k, set()) | v
        elif isinstance(v, np.ndarray):                 # a table of counters
            total[k] = total.get(k, 0) + v
        else:
            total[k] = total.get(k, 0) + int(v)
    return total


def shown(total):
    """A tally for printing: a set as its size, a table of counters as its least cell."""
    return {k: len(v) if isinstance(v, (set, frozenset)) else f"least cell {int(v.min())}" if isinstance(v, np.ndarray) else v for k, v in total.items()}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def random_motifs(rng, counts):
    n_motifs = int(rng.choice(counts))
    wmax = int(rng.choice([8, 16, 32, 40, 66]))
    return [random_matrix(rng, int(rng.integers(1, wmax + 1))) for _ in range(n_motifs)]


def random_chromosomes(rng):
    chroms = [s for s in random_sequences(rng, int(rng.choice([2, 4, 8])), int(rng.choice([40, 150, 300]))) if s]
    return chroms or ["ACGTTGCANacgtACGGT"]


def score_tables(oracle, mat, cutoff, seqs, strand):
    """The oracle twice over `seqs` for one motif: its scan at the all-pass cutoff gives score[N, 2] of every window x strand it reports
    (NaN elsewhere), its scan at the real cutoff gives hit[N, 2] -- the reference's own line decides.  Windows are numbered sequence
    after sequence, start ascending: woff[i] is the first window of sequence i."""
    W = mat.shape[1]
    nwin = np.maximum(np.array([len(s) for s in seqs], dtype=np.int64) - W + 1, 0)
    woff = np.concatenate([[0], np.cumsum(nwin)])
    vals, widths = oracle.flatten_pwms([mat])
    bases, off = oracle.flatten_seqs(seqs)
    score, hit = np.full((int(woff[-1]), 2), np.nan), np.zeros((int(woff[-1]), 2), dtype=bool)
    r = oracle.scan_arrays(vals, widths, [ALL_PASS], bases, off, strand)
    score[woff[r["seq_idx"]] + r["pos"], r["strand"] - 1] = r["score"]
    r = oracle.scan_arrays(vals, widths, [cutoff], bases, off, strand)
    hit[woff[r["seq_idx"]] + r["pos"], r["strand"] - 1] = True
    assert not np.any(hit & np.isnan(score))
    return nwin, woff, score, hit


def near_tally(score, hit, cutoff):
    near = np.abs(score - cutoff) <= NEAR                # (NaN compares false: a window the oracle does not score is not counted)
    return {"near_pass": int((near & hit).sum()), "near_fail": int((near & ~hit).sum()), "pairs": int((~np.isnan(score)).sum())}


# ---- ms_scan_variants

def make_variants_case(seed):
    rng = np.random.default_rng(VARIANT_STREAM + seed)
    mats = random_motifs(rng, [1, 2, 5, 13, 40])
    chroms = random_chromosomes(rng)
    V = int(rng.choice([1, 30, 200, 400]))
    chrom_idx = rng.integers(0, len(chroms), V).astype(np.int32)
    lens = np.array([len(c) for c in chroms], dtype=np.int64)
    pos = (rng.random(V) * lens[chrom_idx]).astype(np.int64)            # uniform on the chromosome: duplicates and any order occur
    alt = "".join(rng.choice(list(ALT_LETTERS), size=V)).encode()
    cutoffs = np.array([attainable_cutoff(rng, m, chroms) for m in mats], dtype=np.float64)
    return {"mats": mats, "cutoffs": cutoffs, "chroms": chroms, "chrom_idx": chrom_idx, "pos": pos, "alt": alt,
            "strand": int(rng.integers(1, 4))}


def expected_variants(oracle, case):
    """The records include/motifscan_amd.h describes for ms_scan_variants, from the oracle over Python-built flank strings
    [max(0, x - W + 1), min(L, x + W)) of the ref and the alt allele."""
    chroms, chrom_idx, pos, alt = case["chroms"], case["chrom_idx"], case["pos"], case["alt"].decode()
    V = len(pos)
    out = {k: [] for k in ("variant", "start", "strand", "score_ref", "score_alt", "state")}
    offsets, gained, lost = [0], [], []
    tally = {"records": 0, "near_pass": 0, "near_fail": 0, "pairs": 0, **motif_kinds(case["mats"])}
    by_width = {}
    for mat, cutoff in zip(case["mats"], case["cutoffs"]):
        W = mat.shape[1]
        if W not in by_width:
            ref_seqs, alt_seqs, los = [], [], []
            for v in range(V):
                seq, x = chroms[chrom_idx[v]], int(pos[v])
                lo, hi = max(0, x - W + 1), min(len(seq), x + W)
                ref_seqs.append(seq[lo:hi])
                alt_seqs.append(seq[lo:x] + alt[v] + seq[x + 1:hi])
                los.append(lo)
            by_width[W] = (ref_seqs + alt_seqs, np.array(los, dtype=np.int64))
        seqs, los = by_width[W]
        nwin, woff, score, hit = score_tables(oracle, mat, cutoff, seqs, case["strand"])
        n = int(woff[V])
        assert int(woff[-1]) == 2 * n
        add_tally(tally, near_tally(score, hit, cutoff))
        state = hit[:n].astype(np.uint8) | (hit[n:].astype(np.uint8) << 1)
        keep = state.ravel() != 0                                        # window-major, '+' before '-'
        variant = np.repeat(np.arange(V, dtype=np.int64), nwin[:V])
        start = np.repeat(los, nwin[:V]) + (np.arange(n) - np.repeat(woff[:V], nwin[:V]))
        out["variant"].append(np.repeat(variant, 2)[keep])
        out["start"].append(np.repeat(start, 2)[keep])
        out["strand"].append(np.tile(np.array([1, 2], dtype=np.int8), n)[keep])
        out["score_ref"].append(score[:n].ravel()[keep])
        out["score_alt"].append(score[n:].ravel()[keep])
        out["state"].append(state.ravel()[keep])
        offsets.append(offsets[-1] + int(keep.sum()))
        gained.append(np.unique(out["variant"][-1][out["state"][-1] == 2]).size)
        lost.append(np.unique(out["variant"][-1][out["state"][-1] == 1]).size)
    want = {k: np.concatenate(v) for k, v in out.items()}
    want["motif_offsets"] = np.array(offsets, dtype=np.int64)
    want["gained"], want["lost"] = np.array(gained, dtype=np.int64), np.array(lost, dtype=np.int64)
    want["ref_codes"] = np.array([oracle.convert_seq(chroms[c][int(x)].encode())[0] for c, x in zip(chrom_idx, pos)], dtype=np.int8)
    tally["records"] = offsets[-1]
    for s in (1, 2, 3):
        tally[f"state_{s}"] = int((want["state"] == s).sum())
    return want, tally


def chunked(seed, _lib, call):
    """Odd seeds run with 7 variants per chunk (ms_debug_varscan_chunk): the result must not depend on the chunk size."""
    if seed % 2 == 0:
        return call()
    prev = _lib.varscan_chunk(7)
    try:
        return call()
    finally:
        _lib.varscan_chunk(prev)


def run_variants_case(seed, oracle, _lib):
    case = make_variants_case(seed)
    want, tally = expected_variants(oracle, case)
    genome = _lib.ResidentGenome({f"c{i}": c for i, c in enumerate(case["chroms"])})
    pw = _lib.PwmSet.from_matrices(case["mats"], case["cutoffs"])
    try:
        res = chunked(seed, _lib, lambda: _lib.scan_variants(pw, genome, case["chrom_idx"], case["pos"], case["alt"], case["strand"]))
        try:
            got = res.sites()
            got["gained"], got["lost"] = res.motif_counts()
            got["ref_codes"] = res.ref_codes()
        finally:
            res.close()
    finally:
        pw.close()
        genome.close()
    for k in ("motif_offsets", "variant", "start", "strand", "state", "gained", "lost", "ref_codes"):
        if not np.array_equal(got[k], want[k]):
            return False, f"variants seed {seed}: {k} differs ({len(got['state'])} vs {len(want['state'])} records)"
    for k in ("score_ref", "score_alt"):
        if not same_bits(got[k], want[k]):
            return False, f"variants seed {seed}: the bits of {k} differ"
    return True, tally


# ---- ms_scan_alleles

def allele_flanks(seq, x, r, alt, W):
    """(lo, ref flank, alt flank): the pieces of the two haplotypes whose windows of width W are exactly the affected ones."""
    lo, hi = max(0, x - W + 1), min(len(seq), x + r + W - 1)
    return lo, seq[lo:hi], seq[lo:x] + alt + seq[x + r:hi]


def make_alleles_case(seed):
    rng = np.random.default_rng(ALLELE_STREAM + seed)
    mats = random_motifs(rng, [1, 2, 5, 13, 40])
    chroms = random_chromosomes(rng)
    V = int(rng.choice([1, 30, 200]))
    chrom_idx = rng.integers(0, len(chroms), V).astype(np.int32)
    pos, ref_len, alts = np.zeros(V, dtype=np.int64), np.zeros(V, dtype=np.int32), []
    for v in range(V):
        L = len(chroms[chrom_idx[v]])
        hi = 41 if rng.random() < 0.1 else 4
        r, a = int(rng.integers(0, hi)), int(rng.integers(0, hi))
        r = min(r, L)
        if r + a == 0:
            a = 1
        pos[v], ref_len[v] = int(rng.integers(0, L - r + 1)), r            # x = L occurs for pure insertions
        alts.append("".join(rng.choice(list(ALT_LETTERS), size=a)))
    cutoffs = np.array([attainable_cutoff(rng, m, chroms) for m in mats], dtype=np.float64)
    strand = int(rng.integers(1, 4))
    refs = None
    if seed % 2 == 0:                                   # REF strings: half as the genome has them, half with one letter changed
        refs = []
        for v in range(V):
            x, r = int(pos[v]), int(ref_len[v])
            ref = chroms[chrom_idx[v]][x:x + r]
            if r and rng.random() < 0.5:
                k = int(rng.integers(0, r))
                other = [c for c in "ACGTN" if "ACGT".find(c) != "ACGT".find(ref[k].upper())]
                ref = ref[:k] + other[int(rng.integers(0, len(other)))] + ref[k + 1:]
            refs.append(ref)
    return {"mats": mats, "cutoffs": cutoffs, "chroms": chroms, "chrom_idx": chrom_idx, "pos": pos, "ref_len": ref_len, "alts": alts,
            "refs": refs, "strand": strand}


def expected_alleles(oracle, case):
    """The records include/motifscan_amd.h describes for ms_scan_alleles, from the oracle over the Python-built flanks of the two
    haplotypes; gained / lost classify variants (records on one haplotype only)."""
    chroms, chrom_idx, pos, ref_len, alts = case["chroms"], case["chrom_idx"], case["pos"], case["ref_len"], case["alts"]
    V = len(pos)
    out = {k: [] for k in ("variant", "allele", "start", "strand", "score")}
    offsets, gained, lost = [0], [], []
    tally = {"records": 0, "near_pass": 0, "near_fail": 0, "pairs": 0, **motif_kinds(case["mats"])}
    by_width = {}
    for mat, cutoff in zip(case["mats"], case["cutoffs"]):
        W = mat.shape[1]
        if W not in by_width:
            seqs, los = [], []
            for v in range(V):
                lo, fr, fa = allele_flanks(chroms[chrom_idx[v]], int(pos[v]), int(ref_len[v]), alts[v], W)
                seqs += [fr, fa]                                             # variant, then allele (ref first): the order of the records
                los += [lo, lo]
            by_width[W] = (seqs, np.array(los, dtype=np.int64))
        seqs, los = by_width[W]
        nwin, woff, score, hit = score_tables(oracle, mat, cutoff, seqs, case["strand"])
        add_tally(tally, near_tally(score, hit, cutoff))
        n = int(woff[-1])
        keep = hit.ravel()                                                   # window-major, '+' before '-'
        seq_of = np.repeat(np.arange(2 * V, dtype=np.int64), nwin)
        start = np.repeat(los, nwin) + (np.arange(n) - np.repeat(woff[:-1], nwin))
        out["variant"].append(np.repeat(seq_of // 2, 2)[keep])
        out["allele"].append(np.repeat(seq_of % 2, 2)[keep].astype(np.uint8))
        out["start"].append(np.repeat(start, 2)[keep])
        out["strand"].append(np.tile(np.array([1, 2], dtype=np.int8), n)[keep])
        out["score"].append(score.ravel()[keep])
        offsets.append(offsets[-1] + int(keep.sum()))
        has = np.zeros((V, 2), dtype=bool)
        has[out["variant"][-1], out["allele"][-1]] = True
        gained.append(int((has[:, 1] & ~has[:, 0]).sum()))
        lost.append(int((has[:, 0] & ~has[:, 1]).sum()))
    want = {k: np.concatenate(v) for k, v in out.items()}
    want["motif_offsets"] = np.array(offsets, dtype=np.int64)
    want["gained"], want["lost"] = np.array(gained, dtype=np.int64), np.array(lost, dtype=np.int64)
    mismatch = np.zeros(V, dtype=bool)
    if case["refs"] is not None:                        # case is ignored; a non-ACGT genome base matches any letter that is not ACGT
        for v in range(V):
            x, r = int(pos[v]), int(ref_len[v])
            mismatch[v] = not np.array_equal(oracle.convert_seq(chroms[chrom_idx[v]][x:x + r].encode()), oracle.convert_seq(case["refs"][v].encode()))
    want["ref_mismatch"] = mismatch
    tally.update(records=offsets[-1], gained=int(sum(gained)), lost=int(sum(lost)), ref_mismatches=int(mismatch.sum()),
                 at_chrom_end=int(sum(int(pos[v]) == len(chroms[chrom_idx[v]]) for v in range(V))))
    return want, tally


def run_alleles_case(seed, oracle, _lib):
    case = make_alleles_case(seed)
    want, tally = expected_alleles(oracle, case)
    genome = _lib.ResidentGenome({f"c{i}": c for i, c in enumerate(case["chroms"])})
    pw = _lib.PwmSet.from_matrices(case["mats"], case["cutoffs"])
    try:
        res = chunked(seed, _lib, lambda: _lib.scan_alleles(pw, genome, case["chrom_idx"], case["pos"], case["ref_len"], case["alts"],
                                                            refs=case["refs"], strand_mask=case["strand"]))
        try:
            got = res.sites()
            got["gained"], got["lost"] = res.motif_counts()
            got["ref_mismatch"] = res.ref_mismatch()
        finally:
            res.close()
    finally:
        pw.close()
        genome.close()
    for k in ("motif_offsets", "variant", "allele", "start", "strand", "gained", "lost", "ref_mismatch"):
        if not np.array_equal(got[k], want[k]):
            return False, f"alleles seed {seed}: {k} differs ({len(got['score'])} vs {len(want['score'])} records)"
    if not same_bits(got["score"], want["score"]):
        return False, f"alleles seed {seed}: the bits of score differ"
    return True, tally


# ---- ms_scan_best

def oracle_best(oracle, mats, seqs, strand_mask, segment_windows=None, tally=None):
    """Per cell the greatest score of the oracle's all-pass scan and the FIRST hit that reaches it (the oracle lists a cell's hits pos
    ascending, '+' before '-'); NaN / -1 / 0 where the oracle reports nothing.  With a dict as `tally`, the cells whose greatest score
    more than one (window, strand) reaches are counted into it, and those whose tied windows start in different segments of
    `segment_windows` window starts."""
    vals, widths = oracle.flatten_pwms(mats)
    bases, off = oracle.flatten_seqs(seqs)
    P, R = len(mats), len(seqs)
    r = oracle.scan_arrays(vals, widths, np.full(P, ALL_PASS), bases, off, strand_mask)
    score = np.full((P, R), np.nan)
    pos = np.full((P, R), -1, dtype=np.int32)
    strand = np.zeros((P, R), dtype=np.int8)
    for m in range(P):
        a, b = int(r["motif_offsets"][m]), int(r["motif_offsets"][m + 1])
        if a == b:
            continue
        seq, sc = r["seq_idx"][a:b], r["score"][a:b]
        assert np.all(np.diff(seq) >= 0)
        first = np.concatenate([[0], np.flatnonzero(np.diff(seq)) + 1])
        counts = np.diff(np.concatenate([first, [b - a]]))
        best = np.maximum.reduceat(sc, first)
        at_best = sc == np.repeat(best, counts)
        at = np.minimum.reduceat(np.where(at_best, np.arange(b - a), b - a), first)
        cells = seq[first]
        score[m, cells], pos[m, cells], strand[m, cells] = sc[at], r["pos"][a:b][at], r["strand"][a:b][at]
        if tally is not None:
            tied = np.add.reduceat(at_best.astype(np.int64), first) > 1
            tally["tied_cells"] = tally.get("tied_cells", 0) + int(tied.sum())
            if segment_windows:
                last = np.maximum.reduceat(np.where(at_best, r["pos"][a:b], -1), first)
                across = tied & (last // segment_windows != r["pos"][a:b][at] // segment_windows)
                tally["tied_across_segments"] = tally.get("tied_across_segments", 0) + int(across.sum())
    return score, pos, strand


def make_best_case(seed):
    rng = np.random.default_rng(BEST_STREAM + seed)
    mats = random_motifs(rng, [1, 2, 5, 13, 40, 97])
    seqs = random_sequences(rng, int(rng.choice([1, 7, 60])), int(rng.choice([20, 150, 700, 1300])))     # 1300: regions of three segments
    return {"mats": mats, "seqs": seqs, "strand": int(rng.integers(1, 4))}


def expected_best(oracle, case, segment_windows):
    tally = {"cells": len(case["mats"]) * len(case["seqs"]), "tied_cells": 0, "tied_across_segments": 0, **motif_kinds(case["mats"])}
    want = oracle_best(oracle, case["mats"], case["seqs"], case["strand"], segment_windows, tally)
    tally["winners"] = int((want[1] >= 0).sum())
    tally["pairs"] = sum(max(len(s) - m.shape[1] + 1, 0) for m in case["mats"] for s in case["seqs"]) * bin(case["strand"]).count("1")
    return want, tally


def same_best(got, want):
    """None, or what differs: positions and strands by value, scores by their bits with the NaN cells compared apart."""
    (gs, gp, gd), (ws, wp, wd) = got, want
    if gs.dtype != np.float64 or gp.dtype != np.int32 or gd.dtype != np.int8 or gs.shape != ws.shape:
        return "dtypes or shapes"
    if not np.array_equal(gp, wp):
        return "pos"
    if not np.array_equal(gd, wd):
        return "strand"
    if not np.array_equal(np.isnan(gs), np.isnan(ws)):
        return "the cells without a winner"
    if not np.array_equal(gs.view(np.int64)[~np.isnan(ws)], ws.view(np.int64)[~np.isnan(ws)]):
        return "the bits of score"
    if not (np.all(gp[np.isnan(gs)] == -1) and np.all(gd[np.isnan(gs)] == 0)):
        return "pos / strand of the cells without a winner"
    return None


def run_best_case(seed, oracle, _lib):
    case = make_best_case(seed)
    want, tally = expected_best(oracle, case, _lib.best_segment_windows())
    pw, sq = _lib.PwmSet.from_matrices(case["mats"]), _lib.SeqSet.from_strings(case["seqs"])
    try:
        runs = []
        for _ in range(2):                              # twice: the bytes are the same on every run
            res = _lib.scan_best(pw, sq, case["strand"])
            try:
                runs.append(res.sites())
            finally:
                res.close()
    finally:
        sq.close()
        pw.close()
    if runs[0][0].shape != (len(case["mats"]), len(case["seqs"])):
        return False, f"best seed {seed}: shape {runs[0][0].shape}"
    bad = same_best(runs[0], want)
    if bad:
        return False, f"best seed {seed}: {bad} differ"
    if any(a.tobytes() != b.tobytes() for a, b in zip(*runs)):
        return False, f"best seed {seed}: two runs give different bytes"
    return True, tally


# ---- ms_scan_regions_once

ONCE_LAYOUTS = ("summits", "mixed", "tilings", "shared_starts", "uniform")


def once_regions(rng, kind, lens, n):
    """n regions (chromosome, start, end) of one layout kind on chromosomes of these lengths, all inside their chromosome."""
    out = []

    def clipped(c, a, b):
        a = min(max(int(a), 0), lens[c])
        out.append((c, a, min(max(int(b), a), lens[c])))

    if kind == "summits":                               # summit +- w / 2, summits uniform: spacing much smaller than w
        w = int(rng.choice([20, 100, 500]))
        for _ in range(n):
            c = int(rng.integers(0, len(lens)))
            s = int(rng.integers(0, lens[c] + 1))
            clipped(c, s - w // 2, s + w // 2)
    elif kind == "mixed":                               # tiny regions beside one or two that cover a chromosome: the span_maxlen bound
        for _ in range(min(n, int(rng.integers(1, 3)))):
            c = int(rng.integers(0, len(lens)))
            clipped(c, rng.integers(0, 3), lens[c] - int(rng.integers(0, 3)))
        while len(out) < n:
            c = int(rng.integers(0, len(lens)))
            a = int(rng.integers(0, lens[c] + 1))
            clipped(c, a, a + int(rng.choice([0, 1, 3, 17, 120])))
    elif kind == "tilings":                             # touching tiles, one-base overlaps and one-base gaps
        w = int(rng.choice([8, 33, 64]))
        at = [int(rng.integers(0, w)) for _ in lens]
        for _ in range(n):
            room = [c for c in range(len(lens)) if at[c] + w <= lens[c]]
            c = room[int(rng.integers(0, len(room)))] if room else int(rng.integers(0, len(lens)))
            if not room:
                at[c] = int(rng.integers(0, w))          # every chromosome is tiled: the next row over one of them, at another phase
            clipped(c, at[c] + int(rng.integers(-1, 2)), at[c] + w + int(rng.integers(-1, 2)))
            at[c] += w
    elif kind == "shared_starts":                       # equal starts, nesting, duplicates
        starts = []
        for _ in range(int(rng.integers(1, 5))):
            c = int(rng.integers(0, len(lens)))
            starts.append((c, int(rng.integers(0, lens[c] + 1))))
        for _ in range(n):
            c, a = starts[int(rng.integers(0, len(starts)))]
            clipped(c, a, a + int(rng.choice([0, 5, 40, 41, 300])))
    else:
        for _ in range(n):
            c = int(rng.integers(0, len(lens)))
            a = int(rng.integers(0, lens[c] + 1))
            clipped(c, a, a + int(rng.integers(0, 400)))
    return out


def make_once_case(seed):
    """The scan-once family's inputs (no GPU): motifs, 1 / 2 / 5 chromosomes, a region list of one of ONCE_LAYOUTS with an eighth of it
    repeated as exact duplicates, shuffled; cutoffs on attainable scores of the cut regions."""
    rng = np.random.default_rng(ONCE_STREAM + seed)
    mats = random_motifs(rng, [1, 2, 5, 13, 40])
    chroms = [random_sequences(rng, 1, int(rng.choice([60, 400, 1500, 6000])))[0] or "ACGTTGCANacgtACGGT" for _ in range(int(rng.choice([1, 2, 5])))]
    n = int(rng.choice([1, 8, 60, 300]))
    kind = ONCE_LAYOUTS[int(rng.integers(0, len(ONCE_LAYOUTS)))]
    regions = once_regions(rng, kind, [len(c) for c in chroms], n - n // 8)
    regions += [regions[int(k)] for k in rng.integers(0, len(regions), n // 8)]
    regions = [regions[int(k)] for k in rng.permutation(len(regions))]
    seqs = [chroms[c][a:b] for c, a, b in regions]
    cutoffs = np.array([attainable_cutoff(rng, m, seqs) for m in mats], dtype=np.float64)
    chrom_idx, start, end = (np.array([r[k] for r in regions], dtype=t) for k, t in enumerate((np.int32, np.int64, np.int64)))
    return {"mats": mats, "cutoffs": cutoffs, "chroms": chroms, "chrom_idx": chrom_idx, "start": start, "end": end, "seqs": seqs,
            "strand": int(rng.integers(1, 4)), "layout": kind}


def merge_spans(chrom_idx, start, end):
    """The regions ordered by (chromosome, start, index) and merged into spans the way ms_scan_regions_once does: a region joins the
    span in front of it iff it starts before that span's end (touching regions do not join; an empty region can be a span of its own).
    Returns (order [R], span of every ORDERED region [R], span chromosome / start / end [S])."""
    ci, st, en = np.asarray(chrom_idx, dtype=np.int64), np.asarray(start, dtype=np.int64), np.asarray(end, dtype=np.int64)
    order = np.lexsort((np.arange(len(ci)), st, ci))
    span_of, sp = [], []
    for r in order.tolist():
        if sp and sp[-1][0] == ci[r] and st[r] < sp[-1][2]:
            sp[-1][2] = max(sp[-1][2], int(en[r]))
        else:
            sp.append([int(ci[r]), int(st[r]), int(en[r])])
        span_of.append(len(sp) - 1)
    sp = np.array(sp, dtype=np.int64).reshape(-1, 3)
    return order, np.array(span_of, dtype=np.int64), sp[:, 0], sp[:, 1], sp[:, 2]


def bits_for(n):
    b = 1
    while (1 << b) < max(int(n), 1):
        b += 1
    return b


def default_key_form(n_bases, n_seqs, max_len):
    """"local" / "global": the form of the hit coordinate a scan of a set of these sizes chooses by itself (ms_scan_geom.cpp, key_layout:
    (region, position) when that costs at most two bits more than the global base position).  tests/test_fuzz_cases_host.py holds this
    against the library's own answer (ms_debug_key_layout)."""
    gbits = 1
    while (1 << gbits) <= n_bases:
        gbits += 1
    return "local" if bits_for(n_seqs) + bits_for(max_len) <= gbits + 2 else "global"


def once_span_shape(case):
    """(bases, spans, longest span) of the case's merged regions: the sequence set ms_scan_regions_once scans."""
    _, _, _, sp_start, sp_end = merge_spans(case["chrom_idx"], case["start"], case["end"])
    lens = sp_end - sp_start
    return int(lens.sum()), len(lens), int(lens.max()) if len(lens) else 0


def once_tally(case, want):
    """What a scan-once case puts on the hand-out's boundaries, from the regions and the oracle's hits alone."""
    ci, st, en = case["chrom_idx"].astype(np.int64), case["start"], case["end"]
    widths = np.array([m.shape[1] for m in case["mats"]], dtype=np.int64)
    R, n = len(ci), len(want["pos"])
    order, span_sorted, sp_chrom, sp_start, sp_end = merge_spans(ci, st, en)
    span = np.zeros(R, dtype=np.int64)
    span[order] = span_sorted
    lens = en - st
    tally = {"sites": n, "cases_without_sites": int(n == 0), "empty_regions": int((lens == 0).sum()), **motif_kinds(case["mats"]),
             "strand_masks": {case["strand"]}, "layouts": {case["layout"]}}
    tally["pairs"] = int(sum(np.maximum(lens - w + 1, 0).sum() for w in widths.tolist())) * bin(case["strand"]).count("1")
    # the merge: touching non-empty neighbours that stay apart, equal starts with different ends, spans of very different regions
    so_c, so_s, so_e = ci[order], st[order], en[order]
    new_span = np.concatenate([[True], np.diff(span_sorted) > 0]) if R else np.zeros(0, dtype=bool)
    prev_end = np.concatenate([[0], sp_end[span_sorted[:-1]]]) if R else np.zeros(0, dtype=np.int64)
    prev_len = np.concatenate([[0], (sp_end - sp_start)[span_sorted[:-1]]]) if R else np.zeros(0, dtype=np.int64)
    same_chrom = np.concatenate([[False], so_c[1:] == so_c[:-1]]) if R else np.zeros(0, dtype=bool)
    tally["touching"] = int((new_span & same_chrom & (so_s == prev_end) & (prev_len > 0) & (so_e > so_s)).sum())
    tally["equal_starts"] = int((same_chrom & (so_s == np.concatenate([[-1], so_s[:-1]])) & (so_e != np.concatenate([[-1], so_e[:-1]]))).sum()) if R else 0
    mixed = 0
    for s in range(len(sp_chrom)):
        ls = lens[order][span_sorted == s]
        mixed += int(ls[ls > 0].size > 0 and ls.max() >= 50 * ls[ls > 0].min())
    tally["mixed_spans"] = mixed
    goff = np.concatenate([[0], np.cumsum([len(c) for c in case["chroms"]])])
    tally["span_start_residues"] = {int(x) for x in ((goff[sp_chrom] + sp_start)[sp_end > sp_start] % 32).tolist()}
    form = default_key_form(*once_span_shape(case))
    tally["cases_local"], tally["cases_global"] = int(n > 0 and form == "local"), int(n > 0 and form == "global")
    for k in ("shared_sites", "shared_by_8", "flush_end", "flush_start", "one_base_out", "one_base_before"):
        tally[k] = 0
    if n == 0:
        return tally
    # the sites: shared between regions, flush with a region's ends
    m = np.repeat(np.arange(len(widths)), np.diff(want["motif_offsets"]))
    r, p, W = want["seq_idx"], want["pos"], widths[m]
    g = st[r] + p
    big = int(max(len(c) for c in case["chroms"])) + 2
    site = ((m * len(case["chroms"]) + ci[r]) * big + g) * 2 + (want["strand"].astype(np.int64) - 1)
    uniq, first, inverse, count = np.unique(site, return_index=True, return_inverse=True, return_counts=True)
    tally["shared_sites"], tally["shared_by_8"] = int((count[inverse] >= 2).sum()), int((count[inverse] >= 8).sum())
    tally["flush_end"], tally["flush_start"] = int((p + W == lens[r]).sum()), int((p == 0).sum())
    # per distinct span site, the regions of its span the inclusion test has to turn down by one base
    ug, uW, usp = g[first], W[first], span[r[first]]
    by_end = np.sort((span * big + en) * big + st)                          # (span, end, start)
    lo = np.searchsorted(by_end, (usp * big + ug + uW - 1) * big, side="left")
    hi = np.searchsorted(by_end, (usp * big + ug + uW - 1) * big + ug, side="right")
    tally["one_base_out"] = int((hi - lo).sum())                            # start <= g and g + W == end + 1
    by_start = np.sort((span * big + st) * big + en)                        # (span, start, end)
    lo = np.searchsorted(by_start, (usp * big + ug + 1) * big + ug + uW, side="left")
    hi = np.searchsorted(by_start, (usp * big + ug + 1) * big + big - 1, side="right")
    tally["one_base_before"] = int((hi - lo).sum())                         # g == start - 1 and g + W <= end
    return tally


def expected_once(oracle, case):
    """(the oracle's hits over the regions cut as Python strings, in the caller's order; the tally); no GPU."""
    vals, widths = oracle.flatten_pwms(case["mats"])
    bases, off = oracle.flatten_seqs(case["seqs"])
    want = oracle.scan_arrays(vals, widths, case["cutoffs"], bases, off, case["strand"], 4)
    return want, once_tally(case, want)


def once_differs(got, want):
    """None, or what differs between two hit lists: integers by value, scores by their bits."""
    for k in ("motif_offsets", "seq_idx", "pos"):
        if not np.array_equal(got[k], want[k]):
            return f"{k} differs ({len(got['pos'])} vs {len(want['pos'])} sites)"
    if not np.array_equal(got["strand"].astype(np.int32), want["strand"].astype(np.int32)):
        return "strand differs"
    if not same_bits(got["score"], want["score"]):
        return "the bits of score differ"
    return None


@contextlib.contextmanager
def forced_global_keys():
    """Scans inside the block key their hits by the global base position (MS_MEASURE=1 MS_HIT_COORD=global; a scan reads the switches
    when it starts).  The environment is as before afterwards."""
    before = {k: os.environ.get(k) for k in ("MS_MEASURE", "MS_HIT_COORD")}
    os.environ.update(MS_MEASURE="1", MS_HIT_COORD="global")
    try:
        yield
    finally:
        for k, v in before.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def check_once(case, want, _lib, dedup=False, exact_only=False):
    """ms_scan_regions_once over a ResidentGenome of the case's chromosomes against `want` (expected_once): as is (hits, region counts,
    site tables), again on the same PwmSet (the same bytes), with the span hits keyed by global positions, optionally under
    MS_SCAN_EXACT_ONLY, and optionally de-duplicated against ms_dedup_hits over the expected arrays.  None, or what differs."""
    P, R = len(case["mats"]), len(case["chrom_idx"])
    widths = np.array([m.shape[1] for m in case["mats"]], dtype=np.int32)
    motif = np.repeat(np.arange(P, dtype=np.int64), np.diff(want["motif_offsets"]))
    want_regions = np.bincount(np.unique(motif << 32 | want["seq_idx"]) >> 32, minlength=P)
    genome = _lib.ResidentGenome({f"c{i}": c for i, c in enumerate(case["chroms"])})
    pw = _lib.PwmSet.from_matrices(case["mats"], case["cutoffs"])

    def scan(flags=0):
        return _lib.scan_regions_once(pw, genome, case["chrom_idx"], case["start"], case["end"], case["strand"], flags)

    def differs(res, what):
        bad = once_differs(res.hits(), want)
        if bad is None and not np.array_equal(res.region_counts(), want_regions):
            bad = "region counts differ"
        return f"{what}: {bad}" if bad else None

    res = scan()
    try:
        bad = differs(res, "as is")
        if bad:
            return bad
        first = {k: v.tobytes() for k, v in res.hits().items()}
        n_sites, max_score = res.site_tables(R)
        want_n, want_max = np.zeros((P, R), dtype=np.int32), np.full((P, R), -np.inf)
        np.add.at(want_n, (motif, want["seq_idx"]), 1)
        np.maximum.at(want_max, (motif, want["seq_idx"]), want["score"])
        want_max[want_n == 0] = np.nan
        if not np.array_equal(n_sites, want_n) or not np.array_equal(np.isnan(max_score), np.isnan(want_max)) or \
                not same_bits(max_score[want_n > 0], want_max[want_n > 0]):
            return "site tables differ"
        again = scan()
        try:
            if {k: v.tobytes() for k, v in again.hits().items()} != first:
                return "a second run on the same PWM set gives different bytes"
        finally:
            again.close()
        with forced_global_keys():
            glob = scan()
        try:
            bad = differs(glob, "global positions")
        finally:
            glob.close()
        if bad:
            return bad
        if exact_only:
            ex = scan(_lib.MS_SCAN_EXACT_ONLY)
            try:
                bad = differs(ex, "exact only")
            finally:
                ex.close()
            if bad:
                return bad
        if dedup:
            keep = _lib.dedup_keep(want["motif_offsets"], widths, want["seq_idx"], want["pos"], want["score"], want["strand"])
            kept = {k: want[k][keep] for k in ("seq_idx", "pos", "score", "strand")}
            kept["motif_offsets"] = np.concatenate([[0], np.cumsum(np.bincount(motif[keep], minlength=P))]).astype(np.int64)
            res.dedup(pw)
            bad = once_differs(res.hits(), kept)
            if bad is None and not np.array_equal(res.region_counts(), want_regions):
                bad = "region counts differ"                                  # (de-duplication never empties a region)
            if bad:
                return f"de-duplicated: {bad}"
    finally:
        res.close()
        pw.close()
        genome.close()
    return None


def run_once_case(seed, oracle, _lib):
    """Odd seeds are also de-duplicated, every third seed also runs under MS_SCAN_EXACT_ONLY."""
    case = make_once_case(seed)
    want, tally = expected_once(oracle, case)
    bad = check_once(case, want, _lib, dedup=seed % 2 == 1, exact_only=seed % 3 == 0)
    return (False, f"once seed {seed}: {bad}") if bad else (True, tally)


# ---- ms_result_site_histogram / ms_result_rank_profile (the plot data; no scan and no oracle: synthetic hit arrays)

def plot_n_bins(extend):
    return len(np.arange(-extend - 5, extend + 6, 10)) - 1


def plot_boundary_sizes(dims):
    """(region counts, extends) on the plot kernels' boundaries, from the library's own constants (_lib.plot_dims): the word and window
    edges, the profile tile and its halo; the usual windows, and the widest histogram counted in LDS with the first one that is not."""
    tile, half, lds = dims["prof_tile"], dims["half"], dims["hist_lds_bins"]
    ext_lds = max(e for e in range(5 * lds - 10, 5 * lds + 10) if plot_n_bins(e) <= lds)
    return ([100, 101, 127, 128, 129, 199, 200, tile - 1, tile, tile + 1, tile + half, tile + half + 1, 2 * tile],
            [0, 4, 5, 17, 250, ext_lds, ext_lds + 1])


def make_plot_case(seed, dims=None):
    """The plot family's inputs (no GPU): 1 .. 9 motifs of 1 .. 64 columns (some without a hit), R regions from the boundary list or
    uniform in [100, 3000] with summits of their own (some outside any region), a window from the ladder or uniform in [0, 600]; hits
    whose centres sit on a bin edge or within a base pair of one, on and around the first and the last edge, far outside, or anywhere
    in the window, several per region; region scores with ties, ranked by plot.rank_order; ratio_control of every magnitude."""
    from motifscan_amd import plot
    if dims is None:
        from motifscan_amd import _lib
        dims = _lib.plot_dims()
    rng = np.random.default_rng(PLOT_STREAM + seed)
    sizes, ladder = plot_boundary_sizes(dims)
    P = int(rng.integers(1, 10))
    widths = rng.integers(1, 65, size=P).astype(np.int32)
    R = int(rng.choice(sizes)) if rng.random() < 0.6 else int(rng.integers(100, 3001))
    extend = int(rng.choice(ladder)) if rng.random() < 0.5 else int(rng.integers(0, 601))
    summit_rel = rng.integers(-50, 2 * extend + 50, size=R).astype(np.int64)
    edges = np.arange(-extend - 5, extend + 6, 10)
    no_hits = rng.random() < 0.05
    off, region, pos = [0], [], []
    for m in range(P):
        W = int(widths[m])
        kind = 0 if no_hits else int(rng.integers(0, 7))     # 0: empty; 1: every region; 2: one rank end; 3: edges; 4 - 6: mixed
        if kind == 0:
            n = 0
        elif kind == 1:
            n = R + int(rng.integers(0, R))
        elif kind == 2:
            n = int(rng.integers(1, 4))
        else:
            n = int(rng.integers(1, 3 * R))
        r = rng.integers(0, R, size=n)
        if kind == 1:
            r[:R] = np.arange(R)                                # a site in every region, some regions several times
        # twice the distance centre - summit: on an edge, half a base pair and one base pair either side of one (as W's parity allows),
        # anywhere in the window, or far outside it
        e = edges[rng.integers(0, len(edges), size=n)]
        end = rng.random(n) < 0.3
        e[end] = np.where(rng.random(int(end.sum())) < 0.5, edges[0], edges[-1])
        near = 2 * e + rng.integers(-2, 3, size=n)
        spread = rng.integers(2 * edges[0] - 30, 2 * edges[-1] + 31, size=n)
        far = rng.choice([-1, 1], size=n) * ((1 << 41) + rng.integers(0, 1000, size=n))
        how = rng.random(n)
        d2 = np.where(how < (0.9 if kind == 3 else 0.45), near, np.where(how < 0.97, spread, far))
        d2 += (d2 - W) % 2                                      # 2 * pos = d2 - W + 2 * summit must be even
        region.append(r)
        pos.append((d2 - W) // 2 + summit_rel[r])
        off.append(off[-1] + n)
    off = np.array(off, dtype=np.int64)
    region = np.concatenate(region).astype(np.int64) if region else np.zeros(0, dtype=np.int64)
    pos = np.concatenate(pos).astype(np.int64) if pos else np.zeros(0, dtype=np.int64)
    scores = np.round(rng.normal(0, 3, size=R), 0)              # integral: many ties, both zeros
    scores[rng.random(R) < 0.05] = -0.0
    order = plot.rank_order(scores)
    for m in range(P):                                          # the hits of a "one rank end" motif go to rank 0 or rank R - 1
        if 0 < off[m + 1] - off[m] < 4:
            region[off[m]:off[m + 1]] = order[0 if rng.random() < 0.5 else R - 1]
    for m in range(P):                                          # ms_result order: by region, then position
        sl = slice(off[m], off[m + 1])
        o = np.lexsort((pos[sl], region[sl]))
        region[sl], pos[sl] = region[sl][o], pos[sl][o]
    ratio = np.array([(1.0, 1 / 3, 7 / 13, 1e-300)[(m + seed) % 4] for m in range(P)])
    return {"P": P, "R": R, "widths": widths, "extend": extend, "summit_rel": summit_rel, "motif_offsets": off, "region": region, "pos": pos,
            "scores": scores, "order": order, "ratio": ratio, "dims": dims}


def plot_smoothed_reference(y, k):
    """sum_j k[j] * y[i - 5 + j] over y reflected at both ends, summed wider than double: np.longdouble where that is wider (x86), else
    math.fsum on a strided sample of the ranks (both ends and every 37th).  Returns (the ranks, their reference values)."""
    import math
    half = len(k) // 2
    R = len(y)
    if np.finfo(np.longdouble).nmant > np.finfo(np.float64).nmant:
        s = np.pad(y, half, mode="reflect").astype(np.longdouble)
        ref = np.zeros(R, dtype=np.longdouble)
        for j in range(len(k)):
            ref += np.longdouble(k[j]) * s[j:j + R]
        return np.arange(R), ref
    s = np.pad(y, half, mode="reflect")
    idx = np.unique(np.concatenate([np.arange(min(R, 2 * half + 2)), np.arange(0, R, 37), np.arange(max(0, R - 2 * half - 2), R)]))
    return idx, np.array([math.fsum(float(k[j]) * float(s[i + j]) for j in range(len(k))) for i in idx])


def plot_smoothed_differs(got, raw, k):
    """None, or where a smoothed profile row leaves the exact sum of its 11 non-negative products k[j] * raw[..] by more than
    16 * 2^-53 of it: gamma_11 of any summation order, fused or not, with room for the reference's own rounding."""
    idx, ref = plot_smoothed_reference(raw, k)
    err = np.abs(got[idx].astype(ref.dtype) - ref)
    bad = np.flatnonzero(~(err <= 16 * 2.0 ** -53 * ref))
    if len(bad):
        i = int(bad[0])
        return f"rank {int(idx[i])}: got {got[idx[i]]!r}, exact {ref[i]!r}"
    return None


def expected_plot(case):
    """(dict(counts, n_sites, raw, smooth_k), tally) of a plot case: numpy alone -- np.histogram over the centres, the window ratio from
    prefix counts over the ranked has-site flags; no GPU.  The tally counts what the case puts on the kernels' edges."""
    from motifscan_amd import plot
    from test_plot_host import flat_histogram, flat_profiles
    P, R, ext, off, dims = case["P"], case["R"], case["extend"], case["motif_offsets"], case["dims"]
    counts, n_sites = flat_histogram(off, case["region"], case["pos"], case["widths"], case["summit_rel"], ext)
    raw = flat_profiles(off, case["region"], case["order"], case["ratio"], np.arange(P), False)
    n = int(off[-1])
    m = np.repeat(np.arange(P), np.diff(off))
    d2 = 2 * (case["pos"] - case["summit_rel"][case["region"]]) + case["widths"][m].astype(np.int64)      # twice centre - summit
    first, last = 2 * (-ext - 5), 2 * (-ext - 5) + 20 * counts.shape[1]
    with_site = np.array([len(np.unique(case["region"][off[i]:off[i + 1]])) for i in range(P)], dtype=np.int64)
    f, tile, half = R // 100, dims["prof_tile"], dims["half"]
    tally = {"sites": n, "cases_without_sites": int(n == 0), "in_range": int(counts.sum()),
             "on_edge": int(((d2 - first) % 20 == 0)[(d2 >= first) & (d2 <= last)].sum()), "on_last_edge": int((d2 == last).sum()),
             "below_first": int((d2 < first).sum()), "beyond_last": int((d2 > last).sum()), "half_bp": int((d2 % 2 != 0).sum()),
             "empty_rows": int((with_site == 0).sum()), "full_rows": int((with_site == R).sum()),
             "cases_r_mult_64": int(R % 64 == 0), "cases_multi_tile": int(R > tile), "cases_short_last_tile": int(0 < R % tile < half),
             "cases_global_bins": int(counts.shape[1] > dims["hist_lds_bins"]),
             "clipped_head": P * f, "clipped_tail": P * (f - 1), "width_one": int((case["widths"] == 1).sum()),
             "wide": int((case["widths"] >= 64).sum())}
    return {"counts": counts, "n_sites": n_sites, "raw": raw, "smooth_k": plot.smoothing_weights()}, tally


def run_plot_case(seed, oracle, _lib):
    """The device's histogram and profiles of a case against expected_plot: counts and unsmoothed profiles exactly, the smoothed
    profiles within the derived bound, a range of motifs against the rows of the whole call.  `oracle` is not used."""
    case = make_plot_case(seed, _lib.plot_dims())
    want, tally = expected_plot(case)
    P, R = case["P"], case["R"]
    n = int(case["motif_offsets"][-1])
    res = _lib.result_from_hits(P, R, case["motif_offsets"], case["region"], case["pos"], np.zeros(n), np.ones(n, dtype=np.int8))
    pw = _lib.PwmSet.from_matrices([np.full((4, int(w)), 0.25) for w in case["widths"]])
    try:
        counts, n_sites = res.site_histogram(pw, case["summit_rel"], case["extend"])
        if not np.array_equal(counts, want["counts"]) or not np.array_equal(n_sites, want["n_sites"]):
            bad = np.argwhere(counts != want["counts"])
            return False, f"plot seed {seed}: histogram differs ({len(bad)} bins, first (motif, bin) {bad[:1].tolist()})"
        m0 = seed % P
        m1 = min(P, m0 + 1 + seed % 3)
        part, part_n = res.site_histogram(pw, case["summit_rel"], case["extend"], m0, m1)
        if not np.array_equal(part, counts[m0:m1]) or not np.array_equal(part_n, n_sites[m0:m1]):
            return False, f"plot seed {seed}: histogram of motifs [{m0}, {m1}) differs from those rows of the whole call"
        raw = res.rank_profile(case["order"], case["ratio"], smoothed=False)
        if not same_bits(raw, want["raw"]):
            return False, f"plot seed {seed}: the bits of the unsmoothed profile differ"
        sm = res.rank_profile(case["order"], case["ratio"], want["smooth_k"])
        for m in range(P):
            bad = plot_smoothed_differs(sm[m], want["raw"][m], want["smooth_k"])
            if bad:
                return False, f"plot seed {seed}: smoothed profile of motif {m}, {bad}"
        part = res.rank_profile(case["order"], case["ratio"][m0:m1], want["smooth_k"], m0, m1)
        if not same_bits(part, sm[m0:m1]):
            return False, f"plot seed {seed}: profile of motifs [{m0}, {m1}) differs from those rows of the whole call"
    finally:
        res.close()
        pw.close()
    return True, tally

# ---- the genome-build kernels (ms_seqset.hip, ms_background.hip, ms_pwmset.hip's ms_score / ms_score_ranks); no scan

GENOME_LETTERS = np.frombuffer(b"ACGTacgtNn" + b"RYKMSWBDHVrykmswbdhv", dtype=np.uint8)
GENOME_P = np.array([0.19] * 4 + [0.03] * 4 + [0.05, 0.02] + [0.0025] * 20)
FILTER_LENGTHS = (1, 31, 32, 33, 64, 100)
RANK_WIDTHS = (1, 31, 32, 33, 63, 64, 65, 66)
GENOME_NAN_SEEDS = (3, 11, 19, 27, 35)                  # the seeds that hold ONE motif with max_raw == 0 (its rank row has NaN: not compared)
EXTRACT_MAX_LEN = 70


def ref_random_sequences(chroms, n_times, length, max_n=0, random_seed=None, log=None):
    """Genome.random_sequences (genome/__init__.py:137-176) restated over a dict of strings, step by step.  With a dict as `log`, the
    accepted (chromosome name, start) pairs and the number of attempts are left in it."""
    if random_seed is not None:
        np.random.seed(random_seed)
    sizes = {c: len(s) for c, s in chroms.items()}
    names = sorted(chroms)
    total = sum(sizes.values())
    random_chroms = np.random.choice(names, size=n_times, p=[sizes[c] / total for c in names])
    out, n_loop, windows = [], 0, []
    while len(out) < n_times:
        chrom = random_chroms[n_loop % n_times]
        start = np.random.randint(sizes[chrom] - length)
        seq = chroms[chrom][start:start + length]
        if seq.count("N") + seq.count("n") <= max_n:
            out.append(seq)
            windows.append((str(chrom), int(start)))
        n_loop += 1
    if log is not None:
        log.update(windows=windows, n_loop=n_loop)
    return out


def same_random_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and tuple(a[2:]) == tuple(b[2:])


def genome_dims_of(dims):
    if dims is None:
        from motifscan_amd import _lib
        dims = _lib.genome_dims()
    return dims


def genome_bytes(rng, n, all_bytes=False):
    """n bytes over ACGTacgtNn and the IUPAC letters of both cases, with N / n runs; all_bytes: every byte value 0 .. 255 once."""
    a = GENOME_LETTERS[rng.choice(GENOME_LETTERS.size, size=n, p=GENOME_P)]
    for _ in range(min(n // 400, 100)):
        k = int(rng.integers(0, n))
        a[k:k + int(rng.integers(1, 60))] = ord("N") if rng.random() < 0.8 else ord("n")
    if all_bytes and n >= 256:
        k = int(rng.integers(0, n - 255))
        a[k:k + 256] = rng.permutation(256).astype(np.uint8)
    return a


def pack_totals(dims):
    blk = dims["pack_block_bases"]
    return [0, 1, 31, 32, 33, 63, 64, 65, blk - 1, blk, blk + 1]


def random_offsets(rng, total, n_seqs):
    """offsets [n_seqs + 1] of a set of `total` bases: cuts anywhere, equal cuts (empty sequences) included."""
    cuts = np.sort(rng.integers(0, total + 1, size=n_seqs - 1))
    return np.concatenate([[0], cuts, [total]]).astype(np.int64)


def count_layout(rng, N, tile, lds, clustered):
    """Chromosome lengths summing to N for the base count: empty chromosomes in front and behind; `clustered`: lds + 1 or more
    chromosomes of 33 bases in the first tile (their ends walk through every bit of a unit; those past the lds-th take global atomics),
    else three short chromosomes each behind lds or more empty ones (pushed past index lds by empties alone); at the tile edges inside
    the genome in turn a chromosome that ends on the edge and one that straddles it (`clustered` starts with the end, else with the
    straddler); the rest in chromosomes of 2 000 .. 30 000 bases (a thread's stride of 256 units leaves them)."""
    lens = [0] * int(rng.integers(1, 3))
    lens.append(int(rng.integers(40, 400)))
    if clustered:
        lens += [33] * (lds + 1 + int(rng.integers(0, 8)))
    else:
        for _ in range(3):
            lens += [0] * (lds + int(rng.integers(0, 4)))
            lens.append(int(rng.integers(1, 70)))

    def fill(to):
        used = sum(lens)
        while used < to:
            L = min(int(rng.integers(2000, 30000)), to - used)
            lens.append(L)
            used += L

    for k, edge in enumerate(range(tile, N, tile)):
        if (k % 2 == 0) == clustered:
            fill(edge)                                      # a chromosome ends on the tile edge
        else:
            fill(edge - int(rng.integers(1, 30)))
            lens.append(min(int(rng.integers(31, 90)), N - sum(lens)))      # ... straddles it
    fill(N)
    assert sum(lens) == N
    return lens + [0] * int(rng.integers(1, 3))


def count_genome(rng, N, tile, lds, clustered, all_bytes):
    """(lengths, bytes) of one genome of the base count: count_layout's chromosomes, one of the long ones all N / n, one lower case."""
    lens = count_layout(rng, N, tile, lds, clustered)
    off = np.concatenate([[0], np.cumsum(lens)])
    a = genome_bytes(rng, N, all_bytes)
    long_ones = [c for c, L in enumerate(lens) if L >= 2000]
    c = long_ones[int(rng.integers(0, len(long_ones)))]
    a[off[c]:off[c + 1]] = np.where(rng.random(lens[c]) < 0.7, ord("N"), ord("n"))
    c = long_ones[int(rng.integers(0, len(long_ones)))]
    a[off[c]:off[c + 1]] |= 0x20
    return lens, a


def extract_regions(rng, lens, blk, seed):
    """The extraction's region list [(chromosome, start, end)] over chromosomes of these lengths: regions of 0 .. 70 bases whose source
    phase (genome position mod 32) is one their output phase has not met yet, until all 32 x 32 pairs occurred; region boundaries on
    every multiple of blk in the output and a base either side; a region that ends on the last base of every chromosome; twice 40 or more empty
    regions in a row (at chromosome ends and on an empty chromosome too); 32 one-base regions and 8 empty ones inside one output unit;
    the output ends on a multiple of blk - 1, + 0 or + 1 by seed."""
    goff = np.concatenate([[0], np.cumsum(lens)])
    real = [c for c, L in enumerate(lens) if L >= 200]
    regs, dst, seen, queue = [], [0], np.zeros((32, 32), dtype=bool), []

    def add(c, a, b):
        assert 0 <= a <= b <= lens[c]
        regs.append((c, int(a), int(b)))
        dst[0] += b - a

    def phased(length):
        c = real[int(rng.integers(0, len(real)))]
        d = dst[0] % 32
        want = np.flatnonzero(~seen[:, d])
        s = int(want[rng.integers(0, len(want))]) if len(want) else int(rng.integers(0, 32))
        lo = int((s - goff[c]) % 32)
        a = lo + 32 * int(rng.integers(0, (lens[c] - length - lo) // 32 + 1))
        if length:
            seen[s, d] = True
        add(c, a, a + length)

    def walk(until):
        while not until():
            gap = (dst[0] // blk + 1) * blk - 1 - dst[0]
            if not queue and 0 < gap <= EXTRACT_MAX_LEN:
                queue.extend([gap, 1, 1])                   # boundaries on blk - 1, blk and blk + 1
            phased(queue.pop(0) if queue else int(rng.integers(0, EXTRACT_MAX_LEN + 1)))

    walk(lambda: seen.all() and not queue)
    for c, L in enumerate(lens):
        if L:
            add(c, max(0, L - int(rng.integers(1, EXTRACT_MAX_LEN + 1))), L)
    last = max(c for c, L in enumerate(lens) if L)
    add(last, lens[last] - 1, lens[last])                   # the genome's last base alone
    empties = [(c, L) for c, L in enumerate(lens)] + [(c, 0) for c in real]
    for k in range(40):
        c, a = empties[k % len(empties)]
        add(c, a, a)
    phased(int(rng.integers(1, EXTRACT_MAX_LEN + 1)))
    for k in range(40 + int(rng.integers(0, 30))):
        c, a = empties[int(rng.integers(0, len(empties)))]
        add(c, a, a)
    c = real[0]
    add(c, 5, 5 + (-dst[0]) % 32)
    for k in range(32):
        c = real[k % len(real)]
        a = int(rng.integers(0, lens[c]))
        add(c, a, a + 1)
        if k % 4 == 3:
            add(c, a, a)
    while (dst[0] + 1) % blk:                               # ... up to one base short of the next multiple of blk
        gap = (dst[0] // blk + 1) * blk - 1 - dst[0]
        phased(gap if gap <= EXTRACT_MAX_LEN else int(rng.integers(1, EXTRACT_MAX_LEN + 1)))
    for _ in range(seed % 3):
        phased(1)
    return regs


def filter_calls(rng, bases, seed, dims, run0, run_len):
    """The window filter's calls over the genome `bases`: per call dict(gstart, length, max_n, n_want).  Candidate counts on the wave and
    block edges; starts anywhere, beside an exception byte (the exception at g0 - 1, g0, g1 - 1 and g1) and on the genome's last window;
    max_n 0, at least the length, below every window's count inside the N run [run0, run0 + run_len) (all rejected), or a count v that
    occurs beside v + 1; n_want 1, the accepted count and one either side of it, or more than the candidates."""
    N, ft = len(bases), dims["filter_threads"]
    fold = bases | 0x20
    is_n = fold == ord("n")
    acgt = (fold == ord("a")) | (fold == ord("c")) | (fold == ord("g")) | (fold == ord("t"))
    exc = np.flatnonzero(~acgt & ~is_n)
    cn = np.concatenate([[0], np.cumsum(is_n)])
    calls = []
    for j, n_cand in enumerate([1, 63, 64, 65, ft - 1, ft, ft + 1, ft * int(rng.integers(2, 5)) + 1, 2, 129, 3 * ft, ft * int(rng.integers(2, 5)) + 1]):
        length = FILTER_LENGTHS[(seed + j) % len(FILTER_LENGTHS)]
        kind = (2 * seed + j) % 6
        g0 = rng.integers(0, N - length + 1, size=n_cand)
        if kind == 2:
            g0 = rng.integers(run0 - length + 1, run0 + run_len, size=n_cand)
        else:
            near = rng.random(n_cand) < 0.5
            e = exc[rng.integers(0, len(exc), size=n_cand)] + rng.choice([1, 0, 1 - length, -length], size=n_cand)
            g0 = np.where(near, e, g0)
            g0[int(rng.integers(0, n_cand))] = N - length
        g0 = np.clip(g0, 0, N - length).astype(np.int64)
        nn = cn[g0 + length] - cn[g0]
        if kind in (0, 2):
            max_n = 0
        elif kind == 1:
            max_n = length + int(rng.choice([0, 5]))
        else:
            both = np.intersect1d(nn, nn - 1)
            max_n = int(both[rng.integers(0, len(both))]) if len(both) else int(np.median(nn))
        acc = int((nn <= max_n).sum())
        n_want = (1, max(1, acc - 1), max(1, acc), acc + 1, n_cand + 5)[(seed + j) % 5]
        calls.append({"gstart": g0, "length": length, "max_n": max_n, "n_want": n_want})
    return calls


def make_genome_case(seed, dims=None):
    """The genome family's inputs (no GPU; every boundary size from _lib.genome_dims): sets to pack of 0 .. 65 bases and of the pack
    block - 1, + 0 and + 1, a set of empty sequences and one of none; a genome of eleven chromosomes (empty, 1, 31, 33 and 64 bases
    among them) with extract_regions' list and filter_calls' windows; two samples of random_windows, the first rejecting more than a
    fifth of its attempts; eight genomes for the base count, of tile - 1, tile, tile + 1 and 2 tiles + 1 bases in both of count_layout's forms; motifs of
    RANK_WIDTHS' widths and up to three more (P no multiple of 3), tie-rich; odd seeds hold every byte value."""
    dims = genome_dims_of(dims)
    rng = np.random.default_rng(GENOME_STREAM + seed)
    tile, lds, blk = dims["count_tile_bases"], dims["lds_chroms"], dims["pack_block_bases"]
    all_bytes = seed % 2 == 1
    packs = [(genome_bytes(rng, T, all_bytes), random_offsets(rng, T, int(rng.integers(1, 6)))) for T in pack_totals(dims)]
    packs.append((np.zeros(0, dtype=np.uint8), np.zeros(5, dtype=np.int64)))
    packs.append((np.zeros(0, dtype=np.uint8), np.zeros(1, dtype=np.int64)))
    big = [int(x) for x in rng.integers(400, 9000, size=4)]
    lens = [0, big[0], 1, 33, 64, big[1], 0, big[2], 31, big[3], 0]
    goff = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    bases = genome_bytes(rng, int(goff[-1]), all_bytes)
    run_len = 300
    run0 = int(goff[1] + rng.integers(0, big[0] - run_len))
    bases[run0:run0 + run_len] = np.where(rng.random(run_len) < 0.8, ord("N"), ord("n"))
    regions = extract_regions(rng, lens, blk, seed)
    calls = filter_calls(rng, bases, seed, dims, run0, run_len)
    samples = [{"n_times": 100, "length": 9, "max_n": 0, "seed": 1000 + seed}, {"n_times": 60, "length": 100, "max_n": 5, "seed": None}]
    counts = [count_genome(rng, N, tile, lds, clustered, all_bytes) for N in (tile - 1, tile, tile + 1, 2 * tile + 1) for clustered in (True, False)]
    n_extra = (0, 2, 3)[seed % 3]
    nan_motif = seed in GENOME_NAN_SEEDS
    if nan_motif and n_extra == 0:
        n_extra = 2
    mats = []
    for w in list(RANK_WIDTHS) + [int(x) for x in rng.integers(1, 67, size=n_extra)]:
        m = random_matrix(rng, w)
        while max_raw_of(m) == 0:
            m = random_matrix(rng, w)
        mats.append(m)
    if nan_motif:
        mats[-1] = -np.abs(rng.integers(1, 4, size=mats[-1].shape)).astype(np.float64)
    return {"dims": dims, "packs": packs, "lens": lens, "goff": goff, "bases": bases, "regions": regions, "calls": calls, "samples": samples,
            "counts": counts, "mats": mats, "strand": 1 + seed % 3, "all_bytes": all_bytes}


def sampling_chroms(case):
    """The chromosomes of the case's genome long enough to be sampled, under names whose sorted order is not the file order:
    (names, uint8 arrays)."""
    keep = [c for c, L in enumerate(case["lens"]) if L >= 200]
    return [f"c{(7 * c) % 11}_{c}" for c in keep], [case["bases"][case["goff"][c]:case["goff"][c + 1]] for c in keep]


def packed_cut(bases, goff, regions):
    """(bytes, offsets) of the regions cut out of the genome as byte strings."""
    parts = [bases[goff[c] + a:goff[c] + b] for c, a, b in regions]
    offsets = np.concatenate([[0], np.cumsum([len(x) for x in parts])]).astype(np.int64)
    return (np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)), offsets


def count_tally(lens, dims):
    """What a genome of these chromosome lengths puts on base_count_kernel's paths, from the offsets alone."""
    tile, lds = dims["count_tile_bases"], dims["lds_chroms"]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    N, lens = int(off[-1]), np.asarray(lens, dtype=np.int64)
    nonempty = np.flatnonzero(lens > 0)
    ends = off[nonempty + 1]
    t = {"end_bits": np.bincount((ends - 1) % 32, minlength=32), "end_bit0": int(((ends - 1) % 32 == 0).sum()), "end_bit31": int((ends % 32 == 0).sum()),
         "end_on_tile_edge": int(((ends % tile == 0) & (ends < N)).sum()),
         "straddles_tile_edge": int(((off[nonempty] // tile != (ends - 1) // tile) & (off[nonempty] % tile != 0)).sum()),
         "leading_empty": int(nonempty[0]), "trailing_empty": int(len(lens) - 1 - nonempty[-1]),
         "last_unit_1": int(N % 32 == 1), "last_unit_31": int(N % 32 == 31), "lds_path": 0, "global_by_nonempty": 0, "global_by_empty": 0,
         "size_tile_minus_1": int(N == tile - 1), "size_tile": int(N == tile), "size_tile_plus_1": int(N == tile + 1), "size_2_tiles_plus_1": int(N == 2 * tile + 1)}
    for t0 in range(0, N, tile):
        cb = int(np.searchsorted(off, t0, side="right")) - 1
        for c in nonempty[(off[nonempty] < min(t0 + tile, N)) & (ends > t0)].tolist():
            if c - cb < lds:
                t["lds_path"] += 1
            elif int((lens[cb:c] > 0).sum()) >= lds:
                t["global_by_nonempty"] += 1
            else:
                t["global_by_empty"] += 1
    # a thread's next unit (256 units on) starts past the chromosome its last unit ended in: it looks its chromosome up again
    units = np.arange((N + 31) // 32, dtype=np.int64)
    units = units[units % (tile // 32) >= 256]
    last = np.minimum(32 * (units - 256) + 32, N) - 1
    t["stride_leaves_chrom"] = int((32 * units >= off[np.searchsorted(off, last, side="right")]).sum())
    return t


def expected_genome(oracle, case):
    """(expected arrays, tally) of a genome case from the library's host packer (held against the oracle's convert_seq by
    tests/test_genome.py), numpy counts of the bytes, the restated sampler and the oracle's c_score; no GPU."""
    from motifscan_amd import _lib
    dims, bases, goff, lens = case["dims"], case["bases"], case["goff"], case["lens"]
    blk, N = dims["pack_block_bases"], len(bases)
    want, tally = {}, {"phase_table": np.zeros((32, 32), dtype=np.int64), "end_bits": np.zeros(32, dtype=np.int64)}
    # 1. pack
    want["packs"] = [_lib.host_pack(b, o) for b, o in case["packs"]]
    totals = [len(b) for b, _ in case["packs"]]
    tally.update(pack_sets=len(totals), pack_block_edge=sum(T in (blk - 1, blk, blk + 1) for T in totals),
                 pack_unit_edge=sum(T in (31, 32, 33, 63, 64, 65) for T in totals), pack_empty_sets=sum(T == 0 for T in totals),
                 pack_empty_seqs=int(sum((np.diff(o) == 0).sum() for _, o in case["packs"])), cases_all_bytes=int(case["all_bytes"]))
    # 2. extract
    cut, offsets = packed_cut(bases, goff, case["regions"])
    want["extract"] = _lib.host_pack(cut, offsets)
    want["extract_offsets"], want["genome"] = offsets, _lib.host_pack(bases, goff)
    reg = np.array(case["regions"], dtype=np.int64)
    rl, ds = reg[:, 2] - reg[:, 1], offsets[:-1]
    ne = rl > 0
    np.add.at(tally["phase_table"], ((goff[reg[:, 0]] + reg[:, 1])[ne] % 32, ds[ne] % 32), 1)
    empty_runs = np.diff(np.flatnonzero(np.concatenate([[True], ne, [True]]))) - 1
    on_edge = (ds >= blk - 1) & (((ds + 1) % blk) <= 2)
    tally.update(regions=len(reg), empty_regions=int((~ne).sum()), empty_runs_of_40=int((empty_runs >= 40).sum()),
                 units_of_more_than_32_regions=int((np.bincount(ds // 32) > 32).sum()), one_base_regions=int((rl == 1).sum()),
                 ends_on_chrom_last_base=int((ne & (reg[:, 2] == np.asarray(lens)[reg[:, 0]])).sum()),
                 ends_on_genome_last_base=int((ne & (goff[reg[:, 0]] + reg[:, 2] == N)).sum()),
                 chrom_changes=int((np.diff(reg[ne, 0]) != 0).sum()), starts_on_block_edge=int(on_edge.sum()),
                 extract_lengths={int(x) for x in rl.tolist()}, out_mod_block={int((offsets[-1] + 1) % blk)})
    # 3. base counts
    want["counts"] = []
    for cl, a in case["counts"]:
        off = np.concatenate([[0], np.cumsum(cl)])
        want["counts"].append(np.array([[np.count_nonzero((a[off[c]:off[c + 1]] | 0x20) == ord(b)) for b in "acgt"] for c in range(len(cl))],
                                       dtype=np.int64).reshape(len(cl), 4))
        ct = count_tally(cl, dims)
        tally["end_bits"] += ct.pop("end_bits")
        add_tally(tally, ct)
        fold = [a[off[c]:off[c + 1]] | 0x20 for c in range(len(cl)) if cl[c] >= 2000]
        tally["all_n_chroms"] = tally.get("all_n_chroms", 0) + sum(bool(np.all(f == ord("n"))) for f in fold)
        tally["lower_case_chroms"] = tally.get("lower_case_chroms", 0) + sum(bool(np.all(a[off[c]:off[c + 1]] & 0x20)) for c in range(len(cl)) if cl[c] >= 2000)
    # 4. the window filter
    fold = bases | 0x20
    is_n = fold == ord("n")
    other = ~((fold == ord("a")) | (fold == ord("c")) | (fold == ord("g")) | (fold == ord("t")))
    is_exc = np.concatenate([other & ~is_n, [False]])
    cn, co = np.concatenate([[0], np.cumsum(is_n)]), np.concatenate([[0], np.cumsum(other)])
    want["exc_pos"] = np.flatnonzero(is_exc).astype(np.int64)
    want["taken"] = []
    ft = dims["filter_threads"]
    for k in ("n_equal_max", "n_equal_max_plus_1", "exc_at_g0_minus_1", "exc_at_g0", "exc_at_g1_minus_1", "exc_at_g1", "pass_by_exceptions",
              "window_on_last_base", "n_want_below_accepted", "n_want_equal_accepted", "n_want_above_accepted", "n_want_above_candidates",
              "n_want_one", "all_rejected", "all_accepted", "max_n_zero", "max_n_at_least_length", "n_cand_wave_edge", "n_cand_block_edge",
              "n_cand_blocks_plus_1", "filter_lengths_on_unit_edge"):
        tally[k] = 0
    tally["filter_phases"] = set()
    for call in case["calls"]:
        g0, L, max_n, n_want = call["gstart"], call["length"], call["max_n"], call["n_want"]
        nn, no = cn[g0 + L] - cn[g0], co[g0 + L] - co[g0]
        ok = nn <= max_n
        acc, n_cand = int(ok.sum()), len(g0)
        want["taken"].append(np.flatnonzero(ok)[:n_want].astype(np.int64))
        tally["n_equal_max"] += int((nn == max_n).sum())
        tally["n_equal_max_plus_1"] += int((nn == max_n + 1).sum())
        tally["exc_at_g0_minus_1"] += int(is_exc[g0 - 1][g0 > 0].sum())
        tally["exc_at_g0"] += int(is_exc[g0].sum())
        tally["exc_at_g1_minus_1"] += int(is_exc[g0 + L - 1].sum())
        tally["exc_at_g1"] += int(is_exc[g0 + L].sum())
        tally["pass_by_exceptions"] += int((ok & (no > max_n)).sum())
        tally["window_on_last_base"] += int((g0 + L == N).sum())
        tally["n_want_below_accepted"] += int(n_want < acc)
        tally["n_want_equal_accepted"] += int(n_want == acc)
        tally["n_want_above_accepted"] += int(acc < n_want <= n_cand)
        tally["n_want_above_candidates"] += int(n_want > n_cand)
        tally["n_want_one"] += int(n_want == 1)
        tally["all_rejected"] += int(acc == 0)
        tally["all_accepted"] += int(acc == n_cand)
        tally["max_n_zero"] += int(max_n == 0)
        tally["max_n_at_least_length"] += int(max_n >= L)
        tally["n_cand_wave_edge"] += int(n_cand in (63, 64, 65))
        tally["n_cand_block_edge"] += int(n_cand in (ft - 1, ft, ft + 1))
        tally["n_cand_blocks_plus_1"] += int(n_cand > ft + 1 and n_cand % ft == 1)
        tally["filter_lengths_on_unit_edge"] += int(L in (31, 32, 33, 64))
        tally["filter_phases"] |= {int(x) for x in (g0 % 32).tolist()}
    # ... and its front end: the restated sampler over strings, the global RandomState saved and put back
    names, arrs = sampling_chroms(case)
    strings = {n: a.tobytes().decode("latin-1") for n, a in zip(names, arrs)}
    file_idx = {n: i for i, n in enumerate(names)}
    before = np.random.get_state()
    want["samples"], windows = [], []
    tally["samples_with_second_batch"] = 0
    try:
        for sm in case["samples"]:
            log = {}
            ref_random_sequences(strings, sm["n_times"], sm["length"], sm["max_n"], sm["seed"], log)
            ci = np.array([file_idx[n] for n, _ in log["windows"]], dtype=np.int32)
            st = np.array([s for _, s in log["windows"]], dtype=np.int64)
            want["samples"].append((ci, st, np.random.get_state()))
            tally["samples_with_second_batch"] += int(log["n_loop"] > max(sm["n_times"] + sm["n_times"] // 4, 64))
            windows += [(names[c], s, s + sm["length"]) for c, s in zip(ci.tolist(), st.tolist())]
    finally:
        np.random.set_state(before)
    # 5. scores and ranks over windows of the genome: the samples', the filter's accepted ones that lie inside a chromosome, empty
    # and one-base ones
    orig = {n: int(n.split("_")[1]) for n in names}
    sregs = [(orig[n], a, b) for n, a, b in windows]
    for call, taken in zip(case["calls"], want["taken"]):
        if call["length"] >= 64:
            for g in call["gstart"][taken][:40].tolist():
                c = int(np.searchsorted(goff, g, side="right")) - 1
                if g + call["length"] <= goff[c + 1]:
                    sregs.append((c, g - int(goff[c]), g - int(goff[c]) + call["length"]))
    sregs += [(1, 7, 7), (0, 0, 0), (2, 0, 1), (3, 0, 33), (8, 0, 31), (1, lens[1] - 66, lens[1])]
    want["score_regions"] = sregs
    raw, soff = packed_cut(bases, goff, sregs)
    vals, widths = oracle.flatten_pwms(case["mats"])
    R, P = len(sregs), len(case["mats"])
    want["score"] = {s: oracle.score_arrays(vals, widths, raw.tobytes(), soff, s) for s in (1, 2, 3)}
    ranks = np.array([0, int(R * 0.1 ** 1) - 1, int(R * 0.1 ** 2) - 1, int(R * 0.1 ** 4) - 1, R - 1, -1, R], dtype=np.int64)
    row_of = want["score"][case["strand"]]
    want["ranks"], want["rank_rows"] = ranks, np.full((P, len(ranks)), np.nan)
    want["rank_compared"] = np.ones(P, dtype=bool)
    tally.update(score_regions=R, shorter_than_motif=int(sum((np.diff(soff) < w).sum() for w in widths.tolist())), empty_score_regions=int((np.diff(soff) == 0).sum()),
                 rank_rows_compared=0, rank_rows_with_nan=0, ranks_outside=0, tied_rank_values=0, **motif_kinds(case["mats"]))
    for p in range(P):
        row = row_of[p].tolist()
        if np.isnan(row_of[p]).any():
            want["rank_compared"][p] = False
            tally["rank_rows_with_nan"] += 1
            continue
        srt = sorted(row, reverse=True)
        for k, r in enumerate(ranks.tolist()):
            if 0 <= r < R:
                want["rank_rows"][p, k] = srt[r]
                tally["tied_rank_values"] += int(row.count(srt[r]) > 1)
            else:
                tally["ranks_outside"] += 1
        tally["rank_rows_compared"] += 1
    return want, tally


def planes_differ(got, want):
    """None, or the first of (codes, nmask, blk2reg, blkinfo) that differs between two quadruples of planes."""
    for name, g, w in zip(("codes", "nmask", "blk2reg", "blkinfo"), got, want):
        if g.shape != w.shape or g.dtype != w.dtype or not np.array_equal(g, w):
            return name
    return None


def plane_invariants_broken(codes, nmask, n):
    """None, or which of the planes' invariants does not hold: code 0 under every mask bit, nothing set past base n."""
    cw = codes[0::2].astype(np.uint64) | (codes[1::2].astype(np.uint64) << np.uint64(32))
    m, spread = nmask.astype(np.uint64), np.zeros(len(nmask), dtype=np.uint64)
    for i in range(32):
        spread |= ((m >> np.uint64(i)) & np.uint64(1)) * (np.uint64(3) << np.uint64(2 * i))
    if np.any(cw & spread):
        return "a code under a mask bit"
    if len(nmask) != (n + 31) // 32:
        return "the number of units"
    if n % 32 and (int(cw[-1]) >> (2 * (n % 32)) or int(nmask[-1]) >> (n % 32)):
        return "bits past the last base"
    return None


def same_score_bits(got, want):
    """Scores by their bits; NaN cells (0 / 0 of a motif with max_raw == 0: the sign of the NaN is the divider's own) by their place."""
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.int64)[~nan], want.view(np.int64)[~nan])


def check_genome_ranks(case, want, _lib, pw, sq):
    """ms_score_ranks with the library's budget, with batches of one motif and of three: None, or what differs."""
    R, P = len(want["score_regions"]), len(case["mats"])
    assert P % 3 and case["dims"]["rank_budget"] // R >= P
    runs = []
    for budget in (0, R, 3 * R + 1):
        prev = _lib.score_rank_budget(budget)
        try:
            runs.append(_lib.score_ranks(pw, sq, want["ranks"], case["strand"]))
        finally:
            _lib.score_rank_budget(prev)
    for name, r in zip(("one motif per batch", "three motifs per batch"), runs[1:]):
        if r.tobytes() != runs[0].tobytes():
            return f"score_ranks in batches of {name} differs from one batch (motifs {np.flatnonzero((r.view(np.int64) != runs[0].view(np.int64)).any(axis=1)).tolist()})"
    keep = want["rank_compared"]
    if not same_score_bits(runs[0][keep], want["rank_rows"][keep]):
        bad = np.argwhere(runs[0][keep].view(np.int64) != want["rank_rows"][keep].view(np.int64))
        return f"score_ranks differs from the sorted oracle row at (compared motif, rank slot) {bad[:3].tolist()}"
    outside = (want["ranks"] < 0) | (want["ranks"] >= R)
    if not np.isnan(runs[0][:, outside]).all():
        return "a rank outside the row does not give NaN"
    return None


def run_genome_case(seed, oracle, _lib):
    """The device's planes, region hints, base counts, accepted windows, sampled windows, scores and ranks of a case against
    expected_genome, all exactly."""
    import torch
    case = make_genome_case(seed, _lib.genome_dims())
    want, tally = expected_genome(oracle, case)
    where = f"genome seed {seed}"
    # 1. pack: ms_genome_create, and ms_seqset_from_device at a byte offset of 1 .. 15
    shift = 1 + seed % 15
    for (b, o), w in zip(case["packs"], want["packs"]):
        g = _lib.ResidentGenome({f"s{i}": b[o[i]:o[i + 1]] for i in range(len(o) - 1)})
        try:
            bad = planes_differ(_lib.seqset_planes(g), w)
        finally:
            g.close()
        if bad:
            return False, f"{where}: pack of {len(b)} bases in {len(o) - 1} sequences: {bad} differ from the host packer"
        t = torch.zeros(len(b) + 32, dtype=torch.uint8, device="cuda:0")
        t[shift:shift + len(b)] = torch.from_numpy(b).to("cuda:0")
        torch.cuda.synchronize()
        sq = _lib.SeqSet.from_device(t.data_ptr() + shift, o)
        try:
            bad = planes_differ(_lib.seqset_planes(sq), w)
        finally:
            sq.close()
        if bad:
            return False, f"{where}: pack of {len(b)} device bytes at offset {shift}: {bad} differ from the host packer"
    names, arrs = sampling_chroms(case)
    genome = _lib.ResidentGenome({f"c{i}": case["bases"][case["goff"][i]:case["goff"][i + 1]] for i in range(len(case["lens"]))})
    sampler = _lib.ResidentGenome(dict(zip(names, arrs)), keep_host=True)
    pw = _lib.PwmSet.from_matrices(case["mats"])
    try:
        bad = planes_differ(_lib.seqset_planes(genome), want["genome"])
        if bad:
            return False, f"{where}: the genome's {bad} differ from the host packer"
        # 2. extract
        reg = np.array(case["regions"], dtype=np.int64)
        sq = genome.extract(reg[:, 0], reg[:, 1], reg[:, 2])
        try:
            got = _lib.seqset_planes(sq)
        finally:
            sq.close()
        bad = planes_differ(got, want["extract"]) or plane_invariants_broken(got[0], got[1], int(want["extract_offsets"][-1]))
        if bad:
            return False, f"{where}: extraction of {len(reg)} regions: {bad}"
        # 3. base counts
        for (cl, a), w in zip(case["counts"], want["counts"]):
            off = np.concatenate([[0], np.cumsum(cl)])
            g = _lib.ResidentGenome({f"c{i}": a[off[i]:off[i + 1]] for i in range(len(cl))})
            try:
                got = g.base_counts()
            finally:
                g.close()
            if not np.array_equal(got, w):
                return False, f"{where}: base counts of {len(a)} bases differ at chromosomes {np.flatnonzero((got != w).any(axis=1))[:5].tolist()}"
        # 4. the window filter and the sampler
        for k, (call, w) in enumerate(zip(case["calls"], want["taken"])):
            got = _lib.window_filter(genome, call["gstart"], call["length"], call["max_n"], want["exc_pos"], call["n_want"])
            if not np.array_equal(got, w):
                return False, f"{where}: window filter call {k} ({len(call['gstart'])} candidates of {call['length']}, max_n {call['max_n']}, n_want {call['n_want']}): {len(got)} taken, {len(w)} expected"
        before = np.random.get_state()
        try:
            for sm, (ci, st, state) in zip(case["samples"], want["samples"]):
                got_c, got_s = sampler.random_windows(sm["n_times"], sm["length"], sm["max_n"], sm["seed"])
                if not (np.array_equal(got_c, ci) and np.array_equal(got_s, st)):
                    return False, f"{where}: random_windows({sm}) differs from the restated sampler"
                if not same_random_state(np.random.get_state(), state):
                    return False, f"{where}: numpy's global RandomState after random_windows({sm}) is not the reference's"
        finally:
            np.random.set_state(before)
        # 5. scores and ranks over windows extracted on the device
        sreg = np.array(want["score_regions"], dtype=np.int64)
        sq = genome.extract(sreg[:, 0], sreg[:, 1], sreg[:, 2])
        try:
            for s in (1, 2, 3):
                if not same_score_bits(_lib.score(pw, sq, s), want["score"][s]):
                    return False, f"{where}: the bits of ms_score differ for strand mask {s}"
            bad = check_genome_ranks(case, want, _lib, pw, sq)
        finally:
            sq.close()
        if bad:
            return False, f"{where}: {bad}"
    finally:
        pw.close()
        sampler.close()
        genome.close()
    return True, tally

# ---- the gene-annotation kernels (ms_annotation.hip: ms_genes_nearest_tss, ms_genes_promoter_overlap); no scan and no oracle

ANNOT_CUTOFFS = (10000, 0, 1, -5, 1 << 59)              # the first one is the reference's own: the scenarios are built for it
ANNOT_EXTENTS = ((2000, 2000), (3000, 1000), (0, 0), (500, -500), (100, -300), (-200, 1000), (1000, 3000))
OVERLAP_KINDS = ("end_on_lo", "end_on_lo_plus_1", "start_on_hi", "start_on_hi_minus_1", "empty_inside", "empty_on_lo", "empty_on_hi",
                 "start_behind_end", "overlapping", "far")


def annot_gene_counts(dims):
    """The genes per chromosome of an annot case: 0 .. 3, every power of two up to the LDS tile with one either side, two tiles and
    two tiles + 1."""
    tile = dims["gene_tile"]
    sizes = {0, 1, 2, 3, tile - 1, tile, tile + 1, 2 * tile, 2 * tile + 1}
    k = 4
    while k <= tile:
        sizes |= {k - 1, k, k + 1}
        k *= 2
    return sorted(sizes)


def interleave(rng, lists):
    """The lists' items in one list, chosen list by list in a random order that keeps every list's own order."""
    labels = np.repeat(np.arange(len(lists)), [len(x) for x in lists])
    at = [0] * len(lists)
    out = []
    for c in rng.permutation(labels).tolist():
        out.append(lists[c][at[c]])
        at[c] += 1
    return out


def make_annot_case(seed, dims=None):
    """The annot family's inputs (no GPU): a gene table whose chromosomes hold annot_gene_counts' numbers of genes in a shuffled order,
    duplicate genes and equal TSS on opposite strands among them, and
      * regions for nearest_tss, 1, 2 blocks + 1, block + 1, block - 1 and block of them on the chromosomes of 0, 1, 2, 3 and tile - 1
        genes, a few elsewhere and on chromosomes -1 and n_chroms, their chromosomes interleaved.  On tile + 1 genes a block and two
        waves: all regions freeze on the first gene (a negative or zero distance, closer genes behind it) but lane `lone` of the block
        and wave `wave` of the two, which stay live to the last gene of the last tile and accept it alone; on two tiles 70 regions that
        all freeze in the first tile; on two tiles + 1 the genes approach the
        regions from one side in steps of -3 .. +1 (accepted in every tile; distances equal to the running minimum and one either
        side of it); elsewhere regions within 10 001 of a gene, negative coordinates on the chromosome of `tile` genes;
      * five calls of promoter_overlap with extents A, B, A (two of ANNOT_EXTENTS), a pair that sums to 0 and one that sums to less,
        over block - 1, block, block + 1, block and 2 blocks + 1 regions of
        OVERLAP_KINDS relative to a gene's interval under the call's extents, chromosomes out of range among them."""
    dims = genome_dims_of(dims)
    rng = np.random.default_rng(ANNOT_STREAM + seed)
    tile, block, oblock = dims["gene_tile"], dims["near_threads"], dims["overlap_threads"]
    C = ANNOT_CUTOFFS[0]
    sizes = [int(x) for x in rng.permutation(annot_gene_counts(dims))]
    n_chroms = len(sizes)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    tss = rng.integers(0, 5_000_000, size=int(off[-1])).astype(np.int64)
    strand = rng.integers(1, 3, size=int(off[-1])).astype(np.int8)
    chrom_of_size = {g: c for c, g in enumerate(sizes)}
    near = [[] for _ in range(n_chroms)]                    # per chromosome, the starts of its regions in their order

    def around(c, n):
        g = rng.integers(off[c], off[c + 1], size=n)
        return (tss[g] + np.where(rng.random(n) < 0.05, 0, rng.integers(-10001, 10002, size=n))).tolist()

    # tile genes: negative coordinates
    c = chrom_of_size[tile]
    tss[off[c]:off[c + 1]] = rng.integers(-60_000, 60_000, size=tile)
    near[c] = around(c, 100)
    near[chrom_of_size[0]] = [int(rng.integers(-100, 100000))]
    near[chrom_of_size[1]] = around(chrom_of_size[1], 2 * block + 1)
    near[chrom_of_size[2]] = around(chrom_of_size[2], block + 1)
    near[chrom_of_size[3]] = around(chrom_of_size[3], block - 1)
    near[chrom_of_size[tile - 1]] = around(chrom_of_size[tile - 1], block)
    # tile + 1 genes: one live lane, one live wave, one frozen lane
    c = chrom_of_size[tile + 1]
    T = int(rng.integers(1_000_000, 2_000_000))
    far = T + 60_000
    tss[off[c]:off[c + 1]] = T + rng.integers(-4000, 4001, size=tile + 1)
    tss[off[c]] = T
    tss[off[c + 1] - 1] = far - 7 if seed % 2 else far + 7
    lone, wave = int(rng.integers(0, block)), int(rng.integers(0, 2))
    starts = (T - rng.integers(0, 3000, size=block + 128)).tolist()
    starts[lone] = far
    for k in range(64):
        starts[block + 64 * wave + k] = far + int(rng.integers(-3, 4))
    near[c] = starts
    # two tiles: frozen in the first tile
    c = chrom_of_size[2 * tile]
    T = int(rng.integers(1_000_000, 2_000_000))
    tss[off[c]:off[c + 1]] = T + rng.integers(-4000, 4001, size=2 * tile)
    tss[off[c]:off[c] + 4] = T + rng.integers(3000, 9000, size=4)      # far enough to be accepted by some and not by others
    tss[off[c] + 4] = T
    near[c] = (T - rng.integers(0, 3000, size=70)).tolist()
    # two tiles + 1: the genes come closer in steps of -3 .. +1
    c = chrom_of_size[2 * tile + 1]
    T = int(rng.integers(1_000_000, 2_000_000))
    D = 9900 + np.cumsum(rng.choice([-3, -2, -1, -1, 0, 0, 1], size=2 * tile + 1))
    assert D.min() > 500
    tss[off[c]:off[c + 1]] = T - D
    twin = np.flatnonzero(np.diff(D) == 0) + 1
    strand[off[c] + twin] = 3 - strand[off[c] + twin - 1]                 # equal TSS on opposite strands: the first in file order wins
    near[c] = (T + rng.integers(0, 400, size=70)).tolist()
    for c in rng.choice([c for c in range(n_chroms) if not near[c] and sizes[c]], size=6, replace=False).tolist():
        near[c] = around(c, int(rng.integers(1, 5)))
    # duplicate genes for the sorted promoter lists
    for c in range(n_chroms):
        if sizes[c] >= 4 and not near[c]:
            k = rng.integers(off[c], off[c + 1] - 1, size=max(1, sizes[c] // 16))
            tss[k + 1], strand[k + 1] = tss[k], strand[k]
    pairs = interleave(rng, [[(c, x) for x in near[c]] for c in range(n_chroms)] + [[(-1, 5), (n_chroms, 7), (-1, int(tss[0])), (n_chroms, 0)]])
    near_chrom, near_start = np.array([p[0] for p in pairs], dtype=np.int32), np.array([p[1] for p in pairs], dtype=np.int64)
    # promoter overlap: extents A, B, A
    A = ANNOT_EXTENTS[seed % len(ANNOT_EXTENTS)]
    B = ANNOT_EXTENTS[(seed + 1 + seed // len(ANNOT_EXTENTS) % (len(ANNOT_EXTENTS) - 1)) % len(ANNOT_EXTENTS)]
    if seed % 2:
        B = (A[0], A[1] + 700)                              # only `downstream` changes: the cached table's key has two parts
    calls, n_genes = [], np.asarray(sizes, dtype=np.int64)
    for (up, down), n in zip((A, B, A, ANNOT_EXTENTS[2 + seed % 2], ANNOT_EXTENTS[4]), (oblock - 1, oblock, oblock + 1, oblock, 2 * oblock + 1)):
        ci = rng.integers(0, n_chroms, size=n)
        outside = rng.random(n) < 0.05
        ci[outside] = rng.choice([-1, n_chroms], size=int(outside.sum()))
        kind = rng.integers(0, len(OVERLAP_KINDS), size=n)
        cc = np.where(outside, 0, ci)
        real = ~outside & (n_genes[cc] > 0)
        g = np.minimum(off[cc] + (rng.random(n) * n_genes[cc]).astype(np.int64), len(tss) - 1)      # a gene of the chromosome, where it has one
        lo, hi = np.where(strand[g] == 1, tss[g] - up, tss[g] - down), np.where(strand[g] == 1, tss[g] + down, tss[g] + up)
        w, mid = rng.integers(1, 500, size=n), (lo + hi) // 2
        forms = np.array([(lo - w, lo), (lo - w, lo + 1), (hi, hi + w), (hi - 1, hi + w), (mid, mid), (lo, lo), (hi, hi), (mid + w, mid - w),
                          (mid - w, mid + w), (hi + 10_000_000, hi + 10_000_000 + w)])                  # [kind][start / end][region]
        st, en = forms[kind, 0, np.arange(n)], forms[kind, 1, np.arange(n)]
        plain = rng.integers(0, 1000, size=n)
        st, en = np.where(real, st, plain).astype(np.int64), np.where(real, en, plain + 100).astype(np.int64)
        calls.append({"upstream": up, "downstream": down, "chrom": ci.astype(np.int32), "start": st, "end": en, "kind": kind})
    return {"dims": dims, "sizes": sizes, "off": off, "tss": tss, "strand": strand, "near_chrom": near_chrom, "near_start": near_start,
            "lone": lone, "wave": wave, "calls": calls}


def nearest_stepwise(off, tss, strand, chrom, start, cutoff):
    """dis_to_nearest_gene (region/utils.py:148-180) for every region at once: the reference's recurrence over the genes of the region's
    chromosome in file order -- m = cutoff; per gene d = start - tss; |d| < m: m = d, target = the gene -- one numpy step per gene
    index, every chromosome that has such a gene taking it together.  (distance, found)."""
    n_chroms, n = len(off) - 1, len(chrom)
    dist, found = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=bool)
    idx = np.flatnonzero((chrom >= 0) & (chrom < n_chroms))
    c = chrom[idx].astype(np.int64)
    s, base, n_g = start[idx].astype(np.int64), off[c], off[c + 1] - off[c]
    m = np.full(len(idx), cutoff, dtype=np.int64)
    minus, hit = np.zeros(len(idx), dtype=bool), np.zeros(len(idx), dtype=bool)
    for i in range(int(n_g.max()) if len(idx) else 0):
        live = i < n_g
        g = np.where(live, base + i, 0)
        d = s - tss[g]
        acc = live & (np.abs(d) < m)
        m = np.where(acc, d, m)
        minus = np.where(acc, strand[g] == 2, minus)
        hit |= acc
    dist[idx], found[idx] = np.where(hit, np.where(minus, -m, m), 0), hit
    return dist, found


def nearest_restated(off, tss, strand, chrom, start, cutoff, tile, trace=None, chunk=256):
    """The same recurrence, a chromosome at a time and `chunk` genes at a time (a tile is cut into whole chunks), for the regions that
    can still accept (m > 0): while a region has accepted only positive distances its m is the least |d| so far (or the cutoff), so
    gene k of a chunk is accepted iff |d_k| < min(m, |d| of the chunk's genes before k) and no gene before k was accepted with
    d <= 0 -- the first such gene freezes the region for good.  (distance, found).  tests/test_fuzz_cases_host.py holds it against
    nearest_stepwise and against the plain loop nearest_plain.  With a dict as `trace`, what the walk met is left in it, per region
    that has a chromosome: how often |d| was the running minimum, one less and one more, accepts with d == 0 and of the first of two
    equal TSS on opposite strands, the tiles with an accept, the last accepted gene, whether the region could still accept after the
    first tile and at the last gene, and whether a gene behind the one that froze it at a negative distance was closer."""
    n_chroms, n = len(off) - 1, len(chrom)
    dist, found = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=bool)
    keys = ("ties", "min_minus_1", "min_plus_1", "zero_accepts", "twin_wins", "accepts", "tiles_hit", "closer_later")
    tr = {k: np.zeros(n, dtype=np.int64) for k in keys}
    tr["last_accept"], tr["live_after_tile_1"], tr["live_at_last_gene"] = np.full(n, -1, dtype=np.int64), np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
    for ch in range(n_chroms):
        rows = np.flatnonzero(chrom == ch)
        G = int(off[ch + 1] - off[ch])
        if not len(rows) or not G:
            continue
        t, sd = tss[off[ch]:off[ch + 1]], strand[off[ch]:off[ch + 1]]
        twin = np.concatenate([(t[1:] == t[:-1]) & (sd[1:] != sd[:-1]), [False]])
        s = start[rows].astype(np.int64)
        m = np.full(len(rows), cutoff, dtype=np.int64)
        target = np.full(len(rows), -1, dtype=np.int64)
        for k0 in [k for t0 in range(0, G, tile) for k in range(t0, min(t0 + tile, G), chunk)]:
            k1 = min(k0 + chunk, G, (k0 // tile + 1) * tile)
            if trace is not None and k0 == tile:
                tr["live_after_tile_1"][rows] = m > 0
            live = np.flatnonzero(m > 0)
            if not len(live):
                break
            d = s[live, None] - t[None, k0:k1]
            a = np.abs(d)
            before_min = np.minimum.accumulate(np.concatenate([m[live, None], a[:, :-1]], axis=1), axis=1)
            record = a < before_min
            stop = record & (d <= 0)
            stops_before = np.cumsum(stop, axis=1) - stop
            acc = record & (stops_before == 0)
            any_acc = acc.any(axis=1)
            last = acc.shape[1] - 1 - np.argmax(acc[:, ::-1], axis=1)
            hit_rows = live[any_acc]
            m[hit_rows] = d[any_acc, last[any_acc]]
            target[hit_rows] = k0 + last[any_acc]
            if trace is not None:
                pos = stops_before == 0
                r = rows[live]
                tr["ties"][r] += (pos & (a == before_min)).sum(axis=1)
                tr["min_minus_1"][r] += (pos & (a == before_min - 1)).sum(axis=1)
                tr["min_plus_1"][r] += (pos & (a == before_min + 1)).sum(axis=1)
                tr["zero_accepts"][r] += (acc & (d == 0)).sum(axis=1)
                tr["twin_wins"][r] += (acc & twin[None, k0:k1]).sum(axis=1)
                tr["accepts"][r] += acc.sum(axis=1)
                tr["tiles_hit"][r] |= any_acc.astype(np.int64) << (k0 // tile)
                if k1 == G:
                    tr["live_at_last_gene"][r] = pos[:, -1]
        hit = target >= 0
        dist[rows] = np.where(hit, np.where(sd[np.maximum(target, 0)] == 2, -m, m), 0)
        found[rows] = hit
        if trace is not None:
            tr["last_accept"][rows] = target
            frozen = np.flatnonzero(hit & (m < 0))
            if len(frozen):
                behind = np.arange(G)[None, :] > target[frozen, None]
                tr["closer_later"][rows[frozen]] = (behind & (np.abs(s[frozen, None] - t[None, :]) < -m[frozen, None])).any(axis=1)
    if trace is not None:
        trace.update(tr)
    return dist, found


def nearest_plain(off, tss, strand, chrom, start, cutoff):
    """The same for ONE region as the reference writes it: a plain Python loop over the chromosome's genes."""
    if not (0 <= chrom < len(off) - 1):
        return 0, False
    m, target = cutoff, None
    for g in range(int(off[chrom]), int(off[chrom + 1])):
        d = start - int(tss[g])
        if abs(d) < m:
            m, target = d, g
    if target is None:
        return 0, False
    return (-m if strand[target] == 2 else m), True


def overlap_literal(intervals, start, end):
    """overlap_with (region/utils.py:16-48) as subset_by_location calls it: the literal binary search over a sorted list of [lo, hi]."""
    left, right = 0, len(intervals) - 1
    while left <= right:
        mid = (left + right) // 2
        lo, hi = intervals[mid]
        if not (end <= lo or start >= hi):
            return True
        if start >= hi:
            left = mid + 1
        else:
            right = mid - 1
    return False


def promoter_lists(case, up, down):
    """Per chromosome the promoter intervals [lo, hi] of (up, down), sorted as Python sorts lists."""
    off, fwd = case["off"], case["strand"] == 1
    lo, hi = np.where(fwd, case["tss"] - up, case["tss"] - down).tolist(), np.where(fwd, case["tss"] + down, case["tss"] + up).tolist()
    return [sorted(zip(lo[off[c]:off[c + 1]], hi[off[c]:off[c + 1]])) for c in range(len(off) - 1)]        # (pairs order as lists of two do)


def expected_annot(oracle, case):
    """(expected arrays, tally) of an annot case from the restated recurrence and the literal binary search; no GPU, and `oracle` is
    not used (the reference's walks are Python: they are restated here and held against plain loops by tests/test_fuzz_cases_host.py)."""
    dims, off, tss, strand, sizes = case["dims"], case["off"], case["tss"], case["strand"], np.asarray(case["sizes"])
    tile, block, oblock = dims["gene_tile"], dims["near_threads"], dims["overlap_threads"]
    chrom, start = case["near_chrom"], case["near_start"]
    n_chroms = len(sizes)
    want, tr = {"nearest": {}, "overlap": []}, {}
    for cutoff in ANNOT_CUTOFFS:
        want["nearest"][cutoff] = nearest_restated(off, tss, strand, chrom, start, cutoff, tile, tr if cutoff == ANNOT_CUTOFFS[0] else None)
    in_range = (chrom >= 0) & (chrom < n_chroms)
    c = np.where(in_range, chrom, 0).astype(np.int64)
    n_g = np.where(in_range, sizes[c], 0)
    tiles = (n_g + tile - 1) // tile
    multi = tiles >= 2
    per_chrom = np.bincount(c[n_g > 0], minlength=n_chroms)                # the regions that reach the device, per chromosome
    tally = {"regions": len(chrom), "chrom_below_range": int((chrom < 0).sum()), "chrom_above_range": int((chrom >= n_chroms).sum()),
             "regions_without_genes": int((n_g == 0).sum()), "found": int(want["nearest"][ANNOT_CUTOFFS[0]][1].sum()),
             "strict_tie_rejections": int(tr["ties"].sum()), "min_minus_1_accepts": int(tr["min_minus_1"].sum()),
             "min_plus_1_rejections": int(tr["min_plus_1"].sum()), "zero_distance_accepts": int(tr["zero_accepts"].sum()),
             "first_of_equal_tss_wins": int(tr["twin_wins"].sum()), "negative_accept_closer_later": int(tr["closer_later"].sum()),
             "accepts_in_every_tile": int((multi & (tr["tiles_hit"] == (1 << tiles) - 1)).sum()),
             "only_last_gene_accepts": int((multi & (tr["accepts"] == 1) & (tr["last_accept"] == n_g - 1)).sum()),
             "negative_tss": int((tss < 0).sum()), "negative_starts": int((start < 0).sum()),
             "lone_live_lane_blocks": 0, "lone_live_wave_blocks": 0, "blocks_frozen_in_tile_1": 0, "cutoffs": len(ANNOT_CUTOFFS),
             "cutoff_zero": int(0 in ANNOT_CUTOFFS), "cutoff_negative": sum(x < 0 for x in ANNOT_CUTOFFS), "cutoff_huge": int(1 << 59 in ANNOT_CUTOFFS)}
    for name, g in (("no", 0), ("one", 1), ("tile_minus_1", tile - 1), ("tile", tile), ("tile_plus_1", tile + 1), ("two_tiles", 2 * tile),
                    ("two_tiles_plus_1", 2 * tile + 1)):
        tally[f"walked_chroms_of_{name}_genes"] = int(((sizes == g) & ((per_chrom > 0) | (g == 0))).sum())
    for name, r in (("one", 1), ("block_minus_1", block - 1), ("block", block), ("block_plus_1", block + 1), ("two_blocks_plus_1", 2 * block + 1)):
        tally[f"chroms_of_{name}_regions"] = int((np.bincount(c[in_range], minlength=n_chroms) == r).sum())
    # the blocks as the entry cuts them: a chromosome's regions in their order, near_threads at a time
    for ch in np.flatnonzero((per_chrom > 0) & (sizes > tile)).tolist():
        mine = np.flatnonzero(in_range & (c == ch))
        live1, to_end = tr["live_after_tile_1"][mine], tr["live_at_last_gene"][mine]
        for b0 in range(0, len(mine), block):
            l1, le = live1[b0:b0 + block], to_end[b0:b0 + block]
            waves = [bool(l1[w:w + 64].any()) for w in range(0, len(l1), 64)]
            tally["blocks_frozen_in_tile_1"] += int(not l1.any())
            tally["lone_live_lane_blocks"] += int(l1.sum() == 1 and len(l1) == block and bool(le[l1].all()))
            tally["lone_live_wave_blocks"] += int(sum(waves) == 1 and len(waves) > 1 and l1.sum() > 1 and bool(le[l1].all()))
    # promoter overlap
    for k in OVERLAP_KINDS:
        tally[k] = 0
    tally.update(extent_switches=0, extents_sum_zero=0, extents_sum_negative=0, extents_asymmetric=0, downstream_alone_switches=0, overlaps=0, duplicate_intervals=0,
                 overlap_n_block_minus_1=0, overlap_n_block=0, overlap_n_block_plus_1=0, overlap_chrom_out_of_range=0,
                 probed_chroms_of_0_to_3_genes=0, probed_chroms_of_pow2_minus_1_genes=0, probed_chroms_of_pow2_genes=0, probed_chroms_of_pow2_plus_1_genes=0)
    prev, lists = None, {}
    for call in case["calls"]:
        ext = (call["upstream"], call["downstream"])
        if ext not in lists:
            lists[ext] = promoter_lists(case, *ext)
        iv = lists[ext]
        ok = (call["chrom"] >= 0) & (call["chrom"] < n_chroms)
        want["overlap"].append(np.array([bool(o) and overlap_literal(iv[ch], s_, e_) for o, ch, s_, e_ in
                                         zip(ok.tolist(), call["chrom"].tolist(), call["start"].tolist(), call["end"].tolist())], dtype=bool))
        real = ok & (sizes[np.where(ok, call["chrom"], 0)] > 0)
        for k, name in enumerate(OVERLAP_KINDS):
            tally[name] += int((real & (call["kind"] == k)).sum())
        g = sizes[call["chrom"][real]]
        pow2 = lambda x: (x >= 4) & ((x & (x - 1)) == 0)
        tally["probed_chroms_of_0_to_3_genes"] += int((sizes[call["chrom"][ok]] <= 3).sum())
        tally["probed_chroms_of_pow2_minus_1_genes"] += int(pow2(g + 1).sum())
        tally["probed_chroms_of_pow2_genes"] += int(pow2(g).sum())
        tally["probed_chroms_of_pow2_plus_1_genes"] += int(pow2(g - 1).sum())
        tally["extent_switches"] += int(prev is not None and prev != ext)
        tally["downstream_alone_switches"] += int(prev is not None and prev[0] == ext[0] and prev[1] != ext[1])
        tally["extents_sum_zero"] += int(sum(ext) == 0)
        tally["extents_sum_negative"] += int(sum(ext) < 0)
        tally["extents_asymmetric"] += int(ext[0] != ext[1])
        tally["overlaps"] += int(want["overlap"][-1].sum())
        if prev is None:
            tally["duplicate_intervals"] = sum(sum(a == b for a, b in zip(x, x[1:])) for x in iv)
        tally["overlap_chrom_out_of_range"] += int((~ok).sum())
        n = len(call["chrom"])
        for name, v in (("overlap_n_block_minus_1", oblock - 1), ("overlap_n_block", oblock), ("overlap_n_block_plus_1", oblock + 1)):
            tally[name] += int(n == v)
        prev = ext
    return want, tally


def run_annot_case(seed, oracle, _lib):
    """One GeneTable: nearest_tss at every cutoff of ANNOT_CUTOFFS, then promoter_overlap with extents A, B and A again with nearest_tss
    between them, against expected_annot; all exactly."""
    case = make_annot_case(seed, _lib.genome_dims())
    want, tally = expected_annot(oracle, case)
    table = _lib.GeneTable(case["off"], case["tss"], case["strand"])
    try:
        def nearest(cutoff):
            dist, found = table.nearest_tss(case["near_chrom"], case["near_start"], cutoff)
            wd, wf = want["nearest"][cutoff]
            if not np.array_equal(found, wf):
                return f"annot seed {seed}: nearest_tss at cutoff {cutoff}: found differs at regions {np.flatnonzero(found != wf)[:5].tolist()}"
            if not np.array_equal(dist, wd):
                return f"annot seed {seed}: nearest_tss at cutoff {cutoff}: distance differs at regions {np.flatnonzero(dist != wd)[:5].tolist()}"
            return None

        for cutoff in ANNOT_CUTOFFS:
            bad = nearest(cutoff)
            if bad:
                return False, bad
        for k, (call, w) in enumerate(zip(case["calls"], want["overlap"])):
            got = table.promoter_overlap(call["chrom"], call["start"], call["end"], call["upstream"], call["downstream"])
            if not np.array_equal(got, w):
                r = int(np.flatnonzero(got != w)[0])
                return False, (f"annot seed {seed}: promoter_overlap call {k} (extents {call['upstream']}, {call['downstream']}) differs at region {r} "
                               f"({OVERLAP_KINDS[call['kind'][r]]}, chromosome {call['chrom'][r]})")
            bad = nearest(ANNOT_CUTOFFS[0])
            if bad:
                return False, bad + " (between promoter_overlap calls)"
    finally:
        table.close()
    return True, tally


FAMILIES = {"variants": run_variants_case, "alleles": run_alleles_case, "best": run_best_case, "once": run_once_case, "plot": run_plot_case,
            "genome": run_genome_case, "annot": run_annot_case}

# What the seeds of a family must put on the boundary, summed over SEEDS[family] from the oracle's output alone: conditions, not
# measurements.  If a change to a generator misses one, the seed range changes -- not the threshold, not the mix of matrix kinds.
SEEDS = {"variants": range(30), "alleles": range(30), "best": range(30), "sweep": range(40), "once": range(40), "plot": range(40),
         "genome": range(40), "annot": range(40)}
CONDITIONS = {"variants": {"near_fail": 10_000, "near_pass": 10_000, "records": 100_000},
              "alleles": {"near_fail": 5_000, "near_pass": 5_000, "gained": 500, "lost": 500},
              "best": {"tied_cells": 1_000, "tied_across_segments": 300},
              "sweep": {"sites": 100_000},
              "once": {"sites": 500_000, "shared_sites": 500_000, "shared_by_8": 100_000, "flush_end": 5_000, "flush_start": 5_000,
                       "one_base_out": 2_000, "one_base_before": 2_000, "touching": 20, "equal_starts": 200, "empty_regions": 100,
                       "mixed_spans": 10, "cases_local": 10, "cases_global": 3},
              "plot": {"sites": 200_000, "in_range": 150_000, "on_edge": 20_000, "on_last_edge": 3_000, "below_first": 10_000, "beyond_last": 10_000,
                       "half_bp": 100_000, "empty_rows": 20, "full_rows": 20, "cases_r_mult_64": 5, "cases_multi_tile": 15,
                       "cases_short_last_tile": 3, "cases_global_bins": 2, "clipped_head": 1_000, "clipped_tail": 1_000},
              # genome, annot: one counter per boundary; over the 40 seeds each was at least 40 when these floors were set, at half (or less) of what was counted
              "genome": {"pack_sets": 260, "pack_block_edge": 60, "pack_unit_edge": 120, "pack_empty_sets": 60, "pack_empty_seqs": 198,
                         "regions": 33_000, "empty_regions": 2300, "empty_runs_of_40": 40, "units_of_more_than_32_regions": 55,
                         "one_base_regions": 1300, "ends_on_chrom_last_base": 192, "ends_on_genome_last_base": 42, "chrom_changes": 23_000,
                         "starts_on_block_edge": 359, "end_bit0": 232, "end_bit31": 252, "end_on_tile_edge": 60, "straddles_tile_edge": 60,
                         "leading_empty": 234, "trailing_empty": 245, "last_unit_1": 80, "last_unit_31": 40, "lds_path": 3100,
                         "global_by_nonempty": 1100, "global_by_empty": 998, "size_tile_minus_1": 40, "size_tile": 40, "size_tile_plus_1": 40,
                         "size_2_tiles_plus_1": 40, "stride_leaves_chrom": 350_000, "all_n_chroms": 160, "lower_case_chroms": 160, "n_equal_max": 6300,
                         "n_equal_max_plus_1": 6400, "exc_at_g0_minus_1": 11_000, "exc_at_g0": 12_000, "exc_at_g1_minus_1": 12_000,
                         "exc_at_g1": 11_000, "pass_by_exceptions": 6700, "window_on_last_base": 240, "n_want_below_accepted": 67,
                         "n_want_equal_accepted": 45, "n_want_above_accepted": 69, "n_want_above_candidates": 58, "n_want_one": 88, "all_rejected": 52,
                         "all_accepted": 52, "max_n_zero": 103, "max_n_at_least_length": 40, "n_cand_wave_edge": 60, "n_cand_block_edge": 60,
                         "n_cand_blocks_plus_1": 40, "filter_lengths_on_unit_edge": 160, "samples_with_second_batch": 40, "score_regions": 4700,
                         "shorter_than_motif": 19_000, "empty_score_regions": 40, "rank_rows_compared": 192, "ranks_outside": 576,
                         "tied_rank_values": 316},
              "annot": {"regions": 38_000, "chrom_below_range": 40, "chrom_above_range": 40, "regions_without_genes": 100, "found": 38_000,
                        "strict_tie_rejections": 1_500_000, "min_minus_1_accepts": 1_300_000, "min_plus_1_rejections": 960_000,
                        "zero_distance_accepts": 1100, "first_of_equal_tss_wins": 780_000, "negative_accept_closer_later": 12_000,
                        "accepts_in_every_tile": 560, "only_last_gene_accepts": 1300, "negative_tss": 20_000, "negative_starts": 1000,
                        "lone_live_lane_blocks": 20, "lone_live_wave_blocks": 20, "blocks_frozen_in_tile_1": 20, "cutoffs": 100, "cutoff_zero": 20,
                        "cutoff_negative": 20, "cutoff_huge": 20, "walked_chroms_of_no_genes": 20, "walked_chroms_of_one_genes": 20,
                        "walked_chroms_of_tile_minus_1_genes": 20, "walked_chroms_of_tile_genes": 20, "walked_chroms_of_tile_plus_1_genes": 20,
                        "walked_chroms_of_two_tiles_genes": 20, "walked_chroms_of_two_tiles_plus_1_genes": 20, "chroms_of_one_regions": 52,
                        "chroms_of_block_minus_1_regions": 20, "chroms_of_block_regions": 20, "chroms_of_block_plus_1_regions": 20,
                        "chroms_of_two_blocks_plus_1_regions": 20, "end_on_lo": 2800, "end_on_lo_plus_1": 2800, "start_on_hi": 2800,
                        "start_on_hi_minus_1": 2800, "empty_inside": 2800, "empty_on_lo": 2700, "empty_on_hi": 2700, "start_behind_end": 2800,
                        "overlapping": 2800, "far": 2800, "extent_switches": 77, "extents_sum_zero": 35, "extents_sum_negative": 26,
                        "extents_asymmetric": 72, "downstream_alone_switches": 20, "overlaps": 9900, "duplicate_intervals": 56_000, "overlap_n_block_minus_1": 20,
                        "overlap_n_block": 40, "overlap_n_block_plus_1": 20, "overlap_chrom_out_of_range": 1500,
                        "probed_chroms_of_0_to_3_genes": 3300, "probed_chroms_of_pow2_minus_1_genes": 8200, "probed_chroms_of_pow2_genes": 9200,
                        "probed_chroms_of_pow2_plus_1_genes": 9100}}
SWEEP_MAX_EMPTY = 10                                    # at most this many of the sweep cases may have no window at all
PLOT_MAX_EMPTY = 4                                      # at most this many of the plot cases may have no hit at all
ONCE_MAX_EMPTY = 12                                     # at most this many of the scan-once cases may have no site at all
ONCE_SEEN = {"span_start_residues": 32, "strand_masks": 3, "layouts": len(ONCE_LAYOUTS)}      # every one of them must occur
GENOME_SEEN = {"extract_lengths": EXTRACT_MAX_LEN + 1, "out_mod_block": 3, "filter_phases": 32}   # ... of the genome family's sets
GENOME_TABLES = ("phase_table", "end_bits")             # no cell of these may be empty: extraction's source phase x output phase, the bit of a unit a chromosome ends on
GENOME_MAX_NAN_ROWS = 5                                 # motifs whose oracle row holds NaN (left out of the rank comparison), over all seeds; one per seed at most


def unmet_conditions(family, total):
    """The conditions a family's summed tally misses, as text (empty: all met).  Every family with motifs must also meet one with
    max_raw == 0 (but for the plot family, which has widths and no matrices) and one of a single column, and -- but for the sweep, whose
    generator draws 1 .. 33 columns -- one of 64 columns or more."""
    need = dict(CONDITIONS[family])
    if family != "annot":                               # (the annot family has no motifs)
        need["width_one"] = 1
    if family not in ("plot", "annot"):
        need["max_raw_zero"] = 1
    if family not in ("sweep", "annot"):
        need["wide"] = 1
    bad = [f"{k}: {total.get(k, 0)} < {n}" for k, n in need.items() if total.get(k, 0) < n]
    if family == "sweep" and total.get("cases_without_windows", 0) > SWEEP_MAX_EMPTY:
        bad.append(f"cases_without_windows: {total['cases_without_windows']} > {SWEEP_MAX_EMPTY}")
    if family == "plot" and total.get("cases_without_sites", 0) > PLOT_MAX_EMPTY:
        bad.append(f"cases_without_sites: {total['cases_without_sites']} > {PLOT_MAX_EMPTY}")
    if family == "genome":
        bad += [f"{k}: {len(total.get(k, ()))} of {n} seen" for k, n in GENOME_SEEN.items() if len(total.get(k, ())) != n]
        bad += [f"{k}: {int((np.asarray(total.get(k, 0)) == 0).sum())} empty cells" for k in GENOME_TABLES if not np.all(np.asarray(total.get(k, 0)) > 0)]
        if total.get("rank_rows_with_nan", 0) > GENOME_MAX_NAN_ROWS:
            bad.append(f"rank_rows_with_nan: {total['rank_rows_with_nan']} > {GENOME_MAX_NAN_ROWS}")
    if family == "once":
        bad += [f"{k}: {len(total.get(k, ()))} of {n} seen" for k, n in ONCE_SEEN.items() if len(total.get(k, ())) != n]
        if total.get("cases_without_sites", 0) > ONCE_MAX_EMPTY:
            bad.append(f"cases_without_sites: {total['cases_without_sites']} > {ONCE_MAX_EMPTY}")
    return bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=100)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--sweep", action="store_true", help="fuzz ms_scan_sweep instead of ms_scan")
    ap.add_argument("--sweep-counts", action="store_true", help="fuzz the counts-only hand-out of a sweep span (MS_STREAM_NO_HITS) instead of ms_scan")
    ap.add_argument("--variants", action="store_true", help="fuzz ms_scan_variants instead of ms_scan")
    ap.add_argument("--alleles", action="store_true", help="fuzz ms_scan_alleles instead of ms_scan")
    ap.add_argument("--best", action="store_true", help="fuzz ms_scan_best instead of ms_scan")
    ap.add_argument("--once", action="store_true", help="fuzz ms_scan_regions_once instead of ms_scan")
    ap.add_argument("--plot", action="store_true", help="fuzz ms_result_site_histogram and ms_result_rank_profile instead of ms_scan")
    ap.add_argument("--genome", action="store_true", help="fuzz the pack / extract / base-count / window-filter / score-rank kernels instead of ms_scan")
    ap.add_argument("--annot", action="store_true", help="fuzz ms_genes_nearest_tss and ms_genes_promoter_overlap instead of ms_scan")
    a = ap.parse_args()
    from oracle import oracle
    oracle.build()
    from motifscan_amd import _lib
    _lib.set_device(0)
    if a.sweep or a.sweep_counts:
        bad, total, tally = 0, 0, {}
        for k in range(a.cases):
            ok, info = (run_sweep_counts_case if a.sweep_counts else run_sweep_case)(a.seed + k, oracle, _lib)
            if not ok:
                bad += 1
                print("MISMATCH", info, flush=True)
            else:
                total += info
            add_tally(tally, sweep_tally(a.seed + k, oracle))
        print(f"{'sweep-counts' if a.sweep_counts else 'sweep'} fuzz: {a.cases} cases from seed {a.seed}: {bad} mismatches, {total} sites compared; tallies {tally}")
        return 1 if bad else 0
    for name, run in FAMILIES.items():
        if getattr(a, name):
            bad, tally = 0, {}
            for k in range(a.cases):
                ok, info = run(a.seed + k, oracle, _lib)
                if not ok:
                    bad += 1
                    print("MISMATCH", info, flush=True)
                else:
                    add_tally(tally, info)
            print(f"{name} fuzz: {a.cases} cases from seed {a.seed}: {bad} mismatches; tallies {shown(tally)}")
            if name in ("genome", "annot") and not bad and a.seed == 0 and a.cases >= len(SEEDS[name]):
                unmet = unmet_conditions(name, tally)
                print(f"{name} fuzz: CONDITIONS {'met' if not unmet else 'NOT met: ' + '; '.join(unmet)}")
                return 1 if unmet else 0
            return 1 if bad else 0
    bad, total_hits, fast, exact = 0, 0, 0, 0
    for k in range(a.cases):
        ok, info, st = run_case(a.seed + k, oracle, _lib)
        if not ok:
            bad += 1
            print("MISMATCH", info, flush=True)
        else:
            total_hits += info
        fast += st["n_pwms"] - st["n_pwms_exact"]
        exact += st["n_pwms_exact"]
    print(f"fuzz: {a.cases} cases from seed {a.seed}: {bad} mismatches, {total_hits} hits compared, "
          f"{fast} motifs through the pre-filter, {exact} through the exact-only kernel")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
