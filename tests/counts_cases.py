"""
Cases and restatements for the counts-only forms: MS_SCAN_COUNTS_ONLY's flag map (count_only_kernel, count_rows_kernel,
motif_prefix_kernel in ms_regions.hip, behind scan_counts_fast in ms_scan.hip) and the counts-only hand-out of a sweep span
(sweep_countonly_kernel in ms_sweep.hip, behind MS_STREAM_NO_HITS).  No GPU is needed to build them.

  * expected_counts(want, P): what a counts-only result holds -- (n_hits, motif_offsets, region_counts) -- from an oracle hit dict;
  * closed_form_counts(widths, lengths, passes, strands): the same three for N-free regions whose motifs pass every window or none;
  * flag_map_cases(dims): named sets (mats, cutoffs, seqs, strand, must_take_flag_map) on the edges of the three kernels, every size
    taken from _lib.counts_dims(); is_closed_form(name): its expectation is the closed form (the oracle need not run);
  * sweep_count_cases(dims): named (mats, cutoffs, span, window, stride, strand) on the edges of the window arithmetic;
  * hit_windows(pos, W, window, stride, n_win): the windows of a hit, restated by the definition.

tests/test_counts_cases_host.py holds every case to what it claims, from the oracle alone; tests/test_gpu_counts_boundaries.py runs
them on the device.  All expected values are integers: every comparison is exact.
"""
import numpy as np

import fuzz_parity

ALL_PASS = fuzz_parity.ALL_PASS
NEVER = 1.3                                             # a ratio score / max_raw never exceeds 1
COUNTS_STREAM = 19_000_013 * 41                         # the random stream of these cases (fuzz_parity's families have their own)


# ------------------------------------------------------------------------------------------------ restatements

def expected_counts(want, P):
    """(n_hits, motif_offsets [P + 1], region_counts [P]) of an oracle hit dict: per motif the number of sites and the number of
    regions (or windows) with at least one (stats.py:29-31) -- the distinct (motif, region) pairs."""
    offsets = np.asarray(want["motif_offsets"], dtype=np.int64)
    pair = np.unique((np.repeat(np.arange(P), np.diff(offsets)).astype(np.int64) << 32) | np.asarray(want["seq_idx"], dtype=np.int64))
    return len(want["pos"]), offsets, np.bincount(pair >> 32, minlength=P).astype(np.int64)


def n_strands(strand_mask):
    return 2 if strand_mask == 3 else 1


def closed_form_counts(widths, lengths, passes, strands):
    """(n_hits, motif_offsets, region_counts) of N-free regions of these lengths under motifs of these widths, of which passes[m] says
    whether motif m passes EVERY window (cutoff ALL_PASS, max_raw > 0) or none (cutoff NEVER); strands = how many strands are scanned.
    Sites of a passing motif = strands * sum over the regions of max(L - W + 1, 0); its regions = the number of L >= W."""
    widths, lengths = np.asarray(widths, dtype=np.int64), np.asarray(lengths, dtype=np.int64)
    passes = np.asarray(passes, dtype=bool)
    windows = np.maximum(lengths[None, :] - widths[:, None] + 1, 0)
    sites = np.where(passes, int(strands) * windows.sum(axis=1), 0)
    regions = np.where(passes, (windows > 0).sum(axis=1), 0).astype(np.int64)
    offsets = np.concatenate([[0], np.cumsum(sites)]).astype(np.int64)
    return int(offsets[-1]), offsets, regions


def flat(mats, seqs):
    """(matrix values, widths, bases, offsets) as the library and the oracle take them."""
    vals = np.concatenate([m.ravel() for m in mats])
    widths = np.array([m.shape[1] for m in mats], dtype=np.int32)
    offsets = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64)
    return vals, widths, "".join(seqs).encode(), offsets


def hit_windows(pos, W, window, stride, n_win):
    """The windows k (start k * stride, `window` bases) that hold the site [pos, pos + W) whole, by the definition."""
    return [k for k in range(n_win) if k * stride <= pos and pos + W <= k * stride + window]


# ------------------------------------------------------------------------------------------------ builders

def small_int_matrix(rng, w):
    """A tie-rich matrix of small integers with a positive entry (max_raw > 0: an all-pass cutoff then passes every window)."""
    m = rng.integers(-3, 4, size=(4, w)).astype(np.float64)
    if m.max() <= 0:
        m[rng.integers(0, 4), rng.integers(0, w)] = float(rng.integers(1, 4))
    return np.ascontiguousarray(m)


def word_matrix(word):
    """The motif that only its own word reaches at cutoff 1.0: 1 on the word's base, -1 elsewhere."""
    m = np.full((4, len(word)), -1.0)
    m[["ACGT".index(c) for c in word], np.arange(len(word))] = 1.0
    return np.ascontiguousarray(m)


def random_dna(rng, n):
    return "".join(rng.choice(list("ACGT"), size=n)) if n else ""


def prefix_ranges(P, threads):
    """The motif ranges of motif_prefix_kernel: thread t sums [t * per, min((t + 1) * per, P)), per = ceil(P / threads).  Returns
    (per, the range edges strictly inside (0, P))."""
    per = -(-P // threads)
    return per, list(range(per, P, per))


def empty_motif_mask(rng, P, threads):
    """Which of P motifs never pass, roughly a third: index 0 and P - 1 (P > 2), the left side of every sixth thread-range edge of the
    prefix kernel, the right side of every sixth, both sides of every sixth -- where a range holds two motifs or more -- and runs of
    2..5 neighbours until a third are empty (equal neighbours in motif_first)."""
    empty = np.zeros(P, dtype=bool)
    if P == 1:
        return empty
    empty[0] = True
    if P > 2:
        empty[P - 1] = True
    per, edges = prefix_ranges(P, threads)
    for t, e in enumerate(edges, 1):
        if t % 6 == 0:
            empty[e - 1] = True
        elif t % 6 == 3:
            empty[e] = True
        elif t % 6 == 1 and per >= 2:
            empty[e - 1] = empty[e] = True
    while P > 6 and empty.sum() * 3 < P:
        a = int(rng.integers(1, P - 1))
        empty[a:min(a + int(rng.integers(2, 6)), P - 1)] = True
    assert not empty.all()
    return empty


def p_edge_case(rng, P, threads, strand):
    mats = [small_int_matrix(rng, int(rng.integers(1, 4))) for _ in range(P)]
    empty = empty_motif_mask(rng, P, threads)
    kinds = rng.integers(0, 3, size=P)                   # of the passing motifs: every window, ratio >= 0.5, the best windows alone
    cutoffs = np.where(empty, NEVER, np.choose(kinds, [ALL_PASS, 0.5, 1.0]))
    seqs = [random_dna(rng, int(rng.integers(10, 17))) for _ in range(int(rng.integers(5, 10)))]
    return mats, cutoffs.astype(np.float64), seqs, strand


BASE_MOTIFS = ("C", "G", "T")                            # three width-1 motifs: motif m passes exactly where the base is BASE_MOTIFS[m]


def r_edge_cases(rng, R):
    """P = 3 over R regions: random tie-rich motifs over regions of 10..16 bases; the same with empty regions at both ends; motif 0
    hitting only region R - 1 and motif 1 only region 0 (the last flag byte of row 0 beside the first of row 1), nothing else anywhere;
    every hit in the last region."""
    out = {}
    mats = [small_int_matrix(rng, int(rng.integers(1, 4))) for _ in range(3)]
    cutoffs = np.array([ALL_PASS, 0.5, 0.0])
    seqs = [random_dna(rng, int(rng.integers(10, 17))) for _ in range(R)]
    out["random"] = (mats, cutoffs, seqs, 3, True)
    if R >= 3:
        out["empty_ends"] = (mats, cutoffs, [""] + seqs[1:-1] + [""], 3, True)
    base = [word_matrix(c) for c in BASE_MOTIFS]
    ones = np.ones(3)
    L = 16
    if R >= 2:
        out["cross"] = (base, ones, ["G" * L] + ["A" * L] * (R - 2) + ["C" * L], 1, True)
    out["last_region"] = (base, ones, ["A" * L] * (R - 1) + ["CGT" * 5 + "C"], 1, True)
    return out


def many_motifs_case(rng, R, P=300):
    """P exact-match motifs (cutoff 1.0, 6..8 columns, one strand) of which each occurs 0, 1 or 2 times: the words are planted between
    N's (a window with an N cannot reach ratio 1), so a wave of 64 hit keys holds many distinct motifs."""
    words = []
    while len(words) < P:                                # no word inside another: a word occurs where it was planted, nowhere else
        w = random_dna(rng, int(rng.integers(6, 9)))
        if not any(w in v or v in w for v in words):
            words.append(w)
    times = rng.integers(0, 3, size=P)
    planted = [w for w, t in zip(words, times) for _ in range(t)]
    rng.shuffle(planted)
    per = -(-len(planted) // R)
    seqs = ["N".join(planted[r * per:(r + 1) * per]) for r in range(R)]
    width = max(len(s) for s in seqs)
    seqs = [s + "N" * (width - len(s)) for s in seqs]    # (equal lengths: the hit keys stay region-local)
    return [word_matrix(w) for w in words], np.ones(P), seqs, 1, True


def all_pass_case(n):
    """n hits in closed form: motif 0 never passes, motif 1 (one column) passes every window; both strands where n is even.  Up to five
    regions of equal length, give or take a base."""
    strand = 3 if n % 2 == 0 else 1
    bases = n // n_strands(strand)
    R = min(5, bases)
    lens = [bases // R + (1 if r < bases % R else 0) for r in range(R)]
    mats = [np.ascontiguousarray(np.array([[1.0], [2.0], [0.0], [-1.0]])), np.ascontiguousarray(np.array([[-1.0], [0.0], [1.0], [1.0]]))]
    seqs = [("ACGTTGCA" * (L // 8 + 1))[:L] for L in lens]
    return mats, np.array([NEVER, ALL_PASS]), seqs, strand, True


def second_trip_case(dims, P=128):
    """max_blocks * keys_per_block + 65 hits: the grid of count_only_kernel has stopped growing, every thread has taken its
    keys_per_block / threads whole trips, and 65 keys take one more, padded with dead lanes up to whole waves.  P - 1 one-column motifs
    and one of two columns, all-pass, one strand: n = P * bases - R, over R = -n mod P (+ P while under 40) regions."""
    n = dims["max_blocks"] * dims["keys_per_block"] + 65
    R = (-n) % P
    while R < 40:
        R += P
    bases = (n + R) // P
    assert P * bases - R == n
    lens = [bases // R + (1 if r < bases % R else 0) for r in range(R)]
    col = np.array([[1.0], [0.0], [-1.0], [2.0]])
    mats = [np.ascontiguousarray(col)] * (P - 1) + [np.ascontiguousarray(np.hstack([col, col]))]
    unit = "ACGGTCATTGCA"
    seqs = [(unit * (L // len(unit) + 1))[:L] for L in lens]
    return mats, np.full(P, ALL_PASS), seqs, 2, True


def gate_cases(dims):
    """Two sets that differ in one base, on the gate P x R <= ratio x n: P = ratio exact-match motifs (8 columns of C / G / T, one strand)
    over R = 8 regions of 20 A's with one word planted in each: n = R hits, P x R == ratio x n -- the flag map.  With one planted base
    turned into an A the set holds n - 1 hits: P x R == ratio x (n - 1) + ratio -- the ordered path, on the first scan of a fresh PWM
    set (later scans gate on the predicted size, which is above the true one)."""
    rng = np.random.default_rng(COUNTS_STREAM + 7)
    P, R = dims["gate_ratio"], 8
    words = set()
    while len(words) < P:
        words.add("".join(rng.choice(list("CGT"), size=8)))
    words = sorted(words)
    mats, cutoffs = [word_matrix(w) for w in words], np.ones(P)
    seqs = ["A" * 6 + words[(7 * r) % P] + "A" * 6 for r in range(R)]
    broken = list(seqs)
    broken[3] = seqs[3][:9] + "A" + seqs[3][10:]
    return {"gate_on": (mats, cutoffs, seqs, 1, True), "gate_off": (mats, cutoffs, broken, 1, False)}


def is_closed_form(name):
    """The flag-map cases whose expectation is closed_form_counts: the oracle need not run (second_trip holds 8.4 M hits)."""
    return name.startswith("n_") or name == "second_trip"


def flag_map_cases(dims):
    """name -> (mats, cutoffs, seqs, strand, must_take_flag_map), every size from _lib.counts_dims()."""
    bins, T, kpb = dims["bins"], dims["threads"], dims["keys_per_block"]
    rng = np.random.default_rng(COUNTS_STREAM)
    out = {}
    for k, P in enumerate((1, 2, T - 1, T, T + 1, 2 * T - 1, 2 * T + 1, bins - 1, bins, bins + 1)):
        out[f"P_{P}"] = (*p_edge_case(rng, P, T, 1 + k % 3), P <= bins)
    out["P_1_no_hit"] = ([small_int_matrix(rng, 2)], np.array([NEVER]), [random_dna(rng, 12) for _ in range(5)], 3, True)
    for R in (1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 257):
        for kind, case in r_edge_cases(rng, R).items():
            out[f"R_{R}_{kind}"] = case
    for R in (1, 4):
        out[f"many_motifs_R_{R}"] = many_motifs_case(rng, R)
    for n in (1, 63, 64, 65, 255, 256, 257, kpb - 1, kpb, kpb + 1, 2 * kpb + 1):
        out[f"n_{n}"] = all_pass_case(n)
    out["second_trip"] = second_trip_case(dims)
    out.update(gate_cases(dims))
    return out


def closed_form_of(case):
    """closed_form_counts of a case whose cutoffs are ALL_PASS or NEVER and whose regions hold no N."""
    mats, cutoffs, seqs, strand, _ = case
    assert all(c in (ALL_PASS, NEVER) for c in cutoffs.tolist()) and all(set(s) <= set("ACGT") for s in {*seqs})
    return closed_form_counts([m.shape[1] for m in mats], [len(s) for s in seqs], cutoffs == ALL_PASS, n_strands(strand))


# ------------------------------------------------------------------------------------------------ the sweep's counts-only hand-out

def sweep_case_dict(case):
    """A named sweep-count case as the dict fuzz_parity.expected_sweep takes (the span is the whole chromosome)."""
    mats, cutoffs, span, window, stride, strand = case
    n_win = (len(span) - window) // stride + 1 if len(span) >= window else 0
    return {"mats": mats, "cutoffs": np.asarray(cutoffs, dtype=np.float64), "chrom": span, "begin": 0, "end": len(span), "window": window,
            "stride": stride, "n_win": n_win, "seqs": [span[k * stride:k * stride + window] for k in range(n_win)], "strand": strand}


def sweep_count_cases(dims):
    """name -> (mats, cutoffs, span, window, stride, strand): the edges of n_first = hi - max(lo, prev_hi + 1) + 1."""
    rng = np.random.default_rng(COUNTS_STREAM + 1)
    T = dims["sweep_threads"]
    tie = lambda w: small_int_matrix(rng, w)
    one = np.ascontiguousarray(np.array([[1.0], [1.0], [2.0], [1.0]]))       # one column, every base scores: all-pass, a hit per base
    out = {}
    out["window_equals_W"] = ([tie(8), tie(3)], [0.4, 0.6], random_dna(rng, 200), 8, 3, 3)
    out["W_above_window"] = ([tie(12), tie(5), tie(9)], [ALL_PASS, 0.3, ALL_PASS], random_dna(rng, 150), 8, 2, 3)
    out["stride_equals_window"] = ([tie(4), tie(1)], [0.5, ALL_PASS], random_dna(rng, 205), 20, 20, 3)
    out["stride_above_window"] = ([tie(3), tie(1), tie(10)], [0.2, ALL_PASS, 0.1], random_dna(rng, 300), 10, 25, 3)
    out["stride_one_wide_window"] = ([tie(3), tie(2)], [0.7, 0.9], random_dna(rng, 400), 100, 1, 3)
    out["bases_past_last_window"] = ([tie(5), tie(1)], [0.3, ALL_PASS], random_dna(rng, 30 + 7 * 12 + 6), 30, 7, 2)
    out["span_below_window"] = ([tie(3), tie(1)], [ALL_PASS, ALL_PASS], random_dna(rng, 15), 20, 5, 3)
    out["span_is_one_window"] = ([tie(3), tie(1)], [ALL_PASS, 0.5], random_dna(rng, 20), 20, 5, 3)
    pal = "GAATTC"
    span = "".join(random_dna(rng, int(rng.integers(0, 9))) + (pal if rng.random() < 0.7 else "ACGT") for _ in range(40))
    out["palindromes"] = ([word_matrix(pal), word_matrix("ACGT"), word_matrix("GGCC")], [1.0, 1.0, 1.0], span, 24, 5, 3)
    out["low_complexity_A"] = ([tie(4), tie(2), tie(7)], [0.0, 0.5, ALL_PASS], "A" * 300, 16, 3, 3)
    out["low_complexity_AC"] = ([tie(4), tie(3), tie(1)], [0.25, 0.5, ALL_PASS], "AC" * 170 + "A", 12, 5, 3)
    words = set()
    while len(words) < 220:
        words.add(random_dna(rng, 5))
    span = random_dna(rng, 3000)
    out["many_motifs"] = ([word_matrix(w) for w in sorted(words)], [1.0] * 220, span, 64, 16, 3)
    tied = [tie(int(rng.integers(2, 5))) for _ in range(200)]
    out["many_tied_motifs"] = (tied, [1.0] * 200, random_dna(rng, 600), 40, 9, 3)
    for n in (T - 1, T, T + 1):                          # the span's hits (the kernel's threads) on a block's edge: a hit per base, one strand
        out[f"hits_{n}"] = ([one], [ALL_PASS], random_dna(rng, n), 16, 1, 1)     # (stride 1: no base lies past the last whole window)
    return out


# ------------------------------------------------------------------------------------------------ predictions and streams

def prediction_case():
    """(mats, cutoffs, sparse seqs, dense seqs, strand): two sets of the same region lengths -- so the same number of windows -- under
    one PWM set at cutoff 1.  The sparse one has an N at six bases in ten (a window with an N cannot reach ratio 1), the dense one
    none, and holds several times the hits: scanned behind the sparse set, the size predicted from it is too small; the sparse one
    scanned behind the dense one is predicted far too large, and most slots of its hit list are padding."""
    rng = np.random.default_rng(COUNTS_STREAM + 2)
    mats = [small_int_matrix(rng, int(rng.integers(2, 5))) for _ in range(40)]
    dense = [random_dna(rng, 30) for _ in range(60)]
    sparse = ["".join("N" if rng.random() < 0.6 else c for c in random_dna(rng, 30)) for _ in range(60)]
    return mats, np.ones(40), sparse, dense, 3


def stream_case():
    """(mats, cutoffs, seqs, strand) for the stream tests: tie-rich motifs over low-complexity and random regions, so that sites overlap
    (de-duplication removes some) and every region holds sites (the flag map is taken)."""
    rng = np.random.default_rng(COUNTS_STREAM + 3)
    mats = [small_int_matrix(rng, int(rng.integers(2, 7))) for _ in range(12)]
    cutoffs = np.array([0.6, 0.8, 1.0, ALL_PASS] * 3)
    seqs = []
    for r in range(37):
        L = int(rng.integers(20, 41))
        unit = random_dna(rng, int(rng.integers(1, 4)))
        seqs.append((unit * L)[:L] if r % 3 == 0 else random_dna(rng, L))
    return mats, cutoffs, seqs, 3
