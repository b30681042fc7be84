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

Each of --variants, --alleles, --best and --once is make_<x>_case(seed) (inputs), expected_<x>(oracle, case) (expected arrays and a tally; neither needs a GPU) and
run_<x>_case(seed, oracle, _lib) (the device call, compared exactly: integers by value, scores by their bits).  Odd seeds of the variant
and allele families run in chunks of 7 variants.  The plot family is split the same way, but its expected_plot(case) needs no oracle.
CONDITIONS holds what the seeds of a family must put on the boundary.

It lives under tests/ because it uses the oracle (test infrastructure).  Run on the GPU box:
    python tests/fuzz_parity.py --cases 200 --seed 0
    python tests/fuzz_parity.py --variants --cases 30        (likewise --alleles, --best, --sweep, --once, --plot; each prints its tallies)
`tests/test_gpu_parity.py::test_fuzz_decision_boundary` runs a few cases of ms_scan's family in the GPU suite,
tests/test_gpu_fuzz_entry_points.py the next four and the plot family, tests/test_gpu_scan_once.py the scan-once family; tests/test_fuzz_cases_host.py checks the cases
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
    pair = np.unique((np.repeat(np.arange(n_motifs), np.diff(want["motif_offsets"])).astype(np.int64) << 32) | want["seq_idx"])
    want_regions = np.bincount(pair >> 32, minlength=n_motifs)
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
    pair = np.unique((np.repeat(np.arange(n_motifs), np.diff(want["motif_offsets"])).astype(np.int64) << 32) | want["seq_idx"])
    if not np.array_equal(counts, np.bincount(pair >> 32, minlength=n_motifs)):
        return False, f"sweep seed {seed}: window counts differ"
    return True, len(want["pos"])


# ------------------------------------------------------------------------------------------------ variants, alleles, best sites
#
# Each family: make_<x>_case(seed) builds the inputs, expected_<x>(oracle, case) the expected arrays and a tally dict (neither uses a
# GPU), run_<x>_case(seed, oracle, _lib) makes the device call.  Every comparison is exact: integers by value, scores by their bits.

ALL_PASS = -1e30
NEAR = 2e-10                                            # a scored window is "near" when its score is within this of the motif's cutoff
ALT_LETTERS = "ACGTACGTNacgtR"
VARIANT_STREAM, ALLELE_STREAM, BEST_STREAM, ONCE_STREAM, PLOT_STREAM = 2_000_003 * 11, 3_000_017 * 13, 5_000_011 * 17, 7_000_003 * 23, 11_000_027 * 29


def motif_kinds(mats):
    """How many of the motifs are of the kinds every family has to meet: max_raw == 0, 64 columns or more, one column."""
    return {"max_raw_zero": sum(max_raw_of(m) == 0 for m in mats), "wide": sum(m.shape[1] >= 64 for m in mats),
            "width_one": sum(m.shape[1] == 1 for m in mats)}


def add_tally(total, tally):
    """Sum a case's tally into a running one: numbers are added, sets (what was seen) united."""
    for k, v in tally.items():
        if isinstance(v, (set, frozenset)):
            total[k] = total.get(k, set()) | v
        else:
            total[k] = total.get(k, 0) + int(v)
    return total


def shown(total):
    """A tally for printing: a set as its size."""
    return {k: len(v) if isinstance(v, (set, frozenset)) else v for k, v in total.items()}


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


FAMILIES = {"variants": run_variants_case, "alleles": run_alleles_case, "best": run_best_case, "once": run_once_case, "plot": run_plot_case}

# What the seeds of a family must put on the boundary, summed over SEEDS[family] from the oracle's output alone: conditions, not
# measurements.  If a change to a generator misses one, the seed range changes -- not the threshold, not the mix of matrix kinds.
SEEDS = {"variants": range(30), "alleles": range(30), "best": range(30), "sweep": range(40), "once": range(40), "plot": range(40)}
CONDITIONS = {"variants": {"near_fail": 10_000, "near_pass": 10_000, "records": 100_000},
              "alleles": {"near_fail": 5_000, "near_pass": 5_000, "gained": 500, "lost": 500},
              "best": {"tied_cells": 1_000, "tied_across_segments": 300},
              "sweep": {"sites": 100_000},
              "once": {"sites": 500_000, "shared_sites": 500_000, "shared_by_8": 100_000, "flush_end": 5_000, "flush_start": 5_000,
                       "one_base_out": 2_000, "one_base_before": 2_000, "touching": 20, "equal_starts": 200, "empty_regions": 100,
                       "mixed_spans": 10, "cases_local": 10, "cases_global": 3},
              "plot": {"sites": 200_000, "in_range": 150_000, "on_edge": 20_000, "on_last_edge": 3_000, "below_first": 10_000, "beyond_last": 10_000,
                       "half_bp": 100_000, "empty_rows": 20, "full_rows": 20, "cases_r_mult_64": 5, "cases_multi_tile": 15,
                       "cases_short_last_tile": 3, "cases_global_bins": 2, "clipped_head": 1_000, "clipped_tail": 1_000}}
SWEEP_MAX_EMPTY = 10                                    # at most this many of the sweep cases may have no window at all
PLOT_MAX_EMPTY = 4                                      # at most this many of the plot cases may have no hit at all
ONCE_MAX_EMPTY = 12                                     # at most this many of the scan-once cases may have no site at all
ONCE_SEEN = {"span_start_residues": 32, "strand_masks": 3, "layouts": len(ONCE_LAYOUTS)}      # every one of them must occur


def unmet_conditions(family, total):
    """The conditions a family's summed tally misses, as text (empty: all met).  Every family must also meet a motif with max_raw == 0
    (but for the plot family, which has widths and no matrices) and one of a single column, and -- but for the sweep, whose generator
    draws 1 .. 33 columns -- one of 64 columns or more."""
    need = dict(CONDITIONS[family], width_one=1)
    if family != "plot":
        need["max_raw_zero"] = 1
    if family != "sweep":
        need["wide"] = 1
    bad = [f"{k}: {total.get(k, 0)} < {n}" for k, n in need.items() if total.get(k, 0) < n]
    if family == "sweep" and total.get("cases_without_windows", 0) > SWEEP_MAX_EMPTY:
        bad.append(f"cases_without_windows: {total['cases_without_windows']} > {SWEEP_MAX_EMPTY}")
    if family == "plot" and total.get("cases_without_sites", 0) > PLOT_MAX_EMPTY:
        bad.append(f"cases_without_sites: {total['cases_without_sites']} > {PLOT_MAX_EMPTY}")
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
    ap.add_argument("--variants", action="store_true", help="fuzz ms_scan_variants instead of ms_scan")
    ap.add_argument("--alleles", action="store_true", help="fuzz ms_scan_alleles instead of ms_scan")
    ap.add_argument("--best", action="store_true", help="fuzz ms_scan_best instead of ms_scan")
    ap.add_argument("--once", action="store_true", help="fuzz ms_scan_regions_once instead of ms_scan")
    ap.add_argument("--plot", action="store_true", help="fuzz ms_result_site_histogram and ms_result_rank_profile instead of ms_scan")
    a = ap.parse_args()
    from oracle import oracle
    oracle.build()
    from motifscan_amd import _lib
    _lib.set_device(0)
    if a.sweep:
        bad, total, tally = 0, 0, {}
        for k in range(a.cases):
            ok, info = run_sweep_case(a.seed + k, oracle, _lib)
            if not ok:
                bad += 1
                print("MISMATCH", info, flush=True)
            else:
                total += info
            add_tally(tally, sweep_tally(a.seed + k, oracle))
        print(f"sweep fuzz: {a.cases} cases from seed {a.seed}: {bad} mismatches, {total} sites compared; tallies {tally}")
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
