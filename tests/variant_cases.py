"""
The cases of tests/test_gpu_variant_boundaries.py -- ms_scan_variants (ms_variants.hip) and ms_scan_alleles (ms_alleles.hip) at the motif
widths, allele lengths and variant counts at which their kernels change path -- and the helpers tests/test_gpu_variants.py and
tests/test_gpu_alleles.py share with it: the seeded matrices, the window counts, the haplotype flanks, the oracle's table of every window
an allele touches, and the records a scan must return for a table.  tests/test_variant_cases_host.py asserts without a GPU that every
case sits where it claims.  Needs no GPU to import or to build: the expected scores are the pinned oracle's (oracle/), run on Python-built
flank strings of the two haplotypes.  Everything is seeded: a case is the same bytes wherever it is built.

Every size comes from _lib.varscan_dims() (T = variants per block tile, R = threads = items per round, M = the widest motif whose table
is staged in LDS, per scan).  The cases:

    snv_steps      widths R/2 - 1, R/2, R/2 + 1, R - 1, R, R + 1 (the item stepping of var_scan_kernel: R // W = 2, 1, 0 and R % W = 0);
                   chromosomes of 100, R and 700 bases; 2T + 1 variants
    snv_lds_edge   widths [M + 1, 11, M, 768, 767] (the HBM-table kernel in a second launch; the dynamic-LDS raise); one chromosome of
                   2 (M + 1) + 50 bases; 40 variants
    snv_only_wide  widths [M + 1, M + 77]: no LDS launch at all; 20 variants
    al_lds_edge    widths [M + 1, 11, M, 640, 639] with the allele kernel's M; eight allele shapes at five places each
    al_long        widths 1, 8, 33, 70 on 70 000 bases: an insertion and a deletion of MS_ALLELE_MAX_LEN bases, insertions and deletions
                   around 32, 64 and 256 bases; two variant lists (`lists`) that differ in the last allele, so that the alt bytes end one
                   short of and one past a multiple of 32
    al_tiles       widths 5, 33, 129 on 900 bases; 2T + 1 variants, a 300-base insertion last in tile 0 and a 300-base deletion first in tile 1
    al_only_wide   width [M + 1]; 12 variants

A case is a dict: kind ("snv" / "allele"), chroms (name -> bytes), names, lens, mats, chrom_idx, pos, alt (snv: uint8 [V]) or ref_len / alts
(allele), V, table (per motif, see snv_flank_table / allele_flank_table), cutoffs ("all": every window's bits are compared; "q90": the
motif's 0.9 quantile of its finite ref-haplotype scores; "none": 2.0, nothing passes), lists (name -> ascending variant indices: the
variant lists the case is scanned with) and what its builder placed on purpose (`marks`).
"""
import numpy as np

ALL_PASS = -1e30
MS_ALLELE_MAX_LEN = 65536
ALTS = "ACGTNt"
ALT_LETTERS = b"ACGTACGTNacgtn"
SHAPES = ((1, 1), (0, 1), (1, 0), (0, 3), (3, 0), (2, 2), (2, 5), (5, 2), (0, 40), (35, 0), (1, 33))
CASES = ("snv_steps", "snv_lds_edge", "snv_only_wide", "al_lds_edge", "al_long", "al_tiles", "al_only_wide")
ALL_STRANDS = ("snv_steps", "snv_lds_edge", "al_lds_edge")          # run at strand masks 1, 2 and 3; the others at 3


# ------------------------------------------------------------------------------------------------ shared with the two older test files

def passes(score, cutoff):
    return score - cutoff >= -1e-10                     # cscore.c:358 / 375


def n_windows(x, L, W):
    """Windows of width W that cover position x of a chromosome of L bases: starts max(0, x - W + 1) .. min(x, L - W)."""
    return np.maximum(np.minimum(x, L - W) - np.maximum(0, x - W + 1) + 1, 0)


def n_affected(x, length, L_hap, W):
    """The header's formula: starts max(0, x - W + 1) .. min(x + length - 1, L_hap - W) on a haplotype of L_hap bases."""
    return np.maximum(np.minimum(x + length - 1, L_hap - W) - np.maximum(0, x - W + 1) + 1, 0)


def flanks(seq, x, r, alt, W):
    """(lo, ref flank, alt flank): the pieces of the two haplotypes whose windows of width W are exactly the affected ones."""
    lo, hi = max(0, x - W + 1), min(len(seq), x + r + W - 1)
    return lo, seq[lo:hi], seq[lo:x] + alt + seq[x + r:hi]


def seeded_matrix(width, seed):
    """A log-odds-like matrix: Dirichlet columns against a flat background, five decimals as the reference keeps them."""
    rng = np.random.default_rng(seed)
    ppm = rng.dirichlet(np.full(4, 0.4), size=width).T
    return np.round(np.log2((ppm + 0.01) / 1.04 / 0.25), 5)


def all_pass_scores(oracle, mat, seqs, n_threads=1):
    """(nwin, woff, sc): the windows of width W of every string, their prefix, and the oracle's score of every window x strand
    [windows, 2]; a window the all-pass scan does not report holds a -inf entry."""
    W = mat.shape[1]
    nwin = np.maximum(np.array([len(s) for s in seqs]) - W + 1, 0)
    woff = np.concatenate([[0], np.cumsum(nwin)])
    vals, widths = oracle.flatten_pwms([mat])
    bases, off = oracle.flatten_seqs(seqs)
    r = oracle.scan_arrays(vals, widths, [ALL_PASS], bases, off, 3, n_threads)
    sc = np.full((int(woff[-1]), 2), -np.inf)
    sc[woff[r["seq_idx"]] + r["pos"], r["strand"] - 1] = r["score"]
    return nwin, woff, sc


def snv_flank_table(oracle, chroms, names, mats, chrom_idx, pos, alt, n_threads=1):
    """Per motif, every window that covers a variant, scored by the oracle on the ref and on the alt flank [x - W + 1, x + W) clipped to
    the chromosome: dict(variant, start, ref [windows, 2 strands], alt [windows, 2])."""
    V = len(pos)
    lens = np.array([len(chroms[n]) for n in names])
    table = []
    for mat in mats:
        W = mat.shape[1]
        ref_seqs, alt_seqs, starts = [], [], []
        for v in range(V):
            seq, x = chroms[names[chrom_idx[v]]], int(pos[v])
            lo, hi = max(0, x - W + 1), min(len(seq), x + W)
            ref_seqs.append(seq[lo:hi])
            alt_seqs.append(seq[lo:x] + bytes([alt[v]]) + seq[x + 1:hi])
            starts.append(lo)
        score = []
        for seqs in (ref_seqs, alt_seqs):
            nwin, woff, sc = all_pass_scores(oracle, mat, seqs, n_threads)
            assert np.array_equal(nwin, n_windows(pos, lens[chrom_idx], W))
            score.append(sc)
        variant = np.repeat(np.arange(V), nwin)
        start = np.repeat(np.array(starts), nwin) + (np.arange(int(woff[-1])) - np.repeat(woff[:-1], nwin))
        table.append({"variant": variant, "start": start, "ref": score[0], "alt": score[1]})
    return table


def allele_flank_table(oracle, chroms, names, mats, chrom_idx, pos, ref_len, alts, n_threads=1):
    """Per motif, every affected window of either haplotype, scored by the oracle on Python-built flank strings (ref, alt per variant):
    dict(variant, allele, start, score [windows, 2 strands])."""
    V = len(pos)
    lens = np.array([len(chroms[n]) for n in names])
    alt_len = np.array([len(a) for a in alts], dtype=np.int64)
    table = []
    for mat in mats:
        W = mat.shape[1]
        seqs, los = [], []
        for v in range(V):
            lo, fr, fa = flanks(chroms[names[chrom_idx[v]]], int(pos[v]), int(ref_len[v]), alts[v], W)
            seqs += [fr, fa]
            los += [lo, lo]
        nwin, woff, sc = all_pass_scores(oracle, mat, seqs, n_threads)
        L = lens[chrom_idx]
        assert np.array_equal(nwin[0::2], n_affected(pos, ref_len, L, W))
        assert np.array_equal(nwin[1::2], n_affected(pos, alt_len, L - ref_len + alt_len, W))
        seq_of = np.repeat(np.arange(2 * V), nwin)
        start = np.repeat(np.array(los), nwin) + (np.arange(int(woff[-1])) - np.repeat(woff[:-1], nwin))
        table.append({"variant": seq_of // 2, "allele": (seq_of % 2).astype(np.uint8), "start": start, "score": sc})
    return table


def expected_snv_records(table, cutoffs, strand_mask):
    out = {k: [] for k in ("variant", "start", "strand", "score_ref", "score_alt", "state")}
    offsets = [0]
    for t, cut in zip(table, cutoffs):
        state = (passes(t["ref"], cut).astype(np.uint8) | (passes(t["alt"], cut).astype(np.uint8) << 1))
        for s in (0, 1):
            if not strand_mask & (1 << s):
                state[:, s] = 0
        keep = state.ravel() != 0                       # window-major, '+' before '-'
        out["variant"].append(np.repeat(t["variant"], 2)[keep])
        out["start"].append(np.repeat(t["start"], 2)[keep])
        out["strand"].append(np.tile(np.array([1, 2], dtype=np.int8), len(t["variant"]))[keep])
        out["score_ref"].append(t["ref"].ravel()[keep])
        out["score_alt"].append(t["alt"].ravel()[keep])
        out["state"].append(state.ravel()[keep])
        offsets.append(offsets[-1] + int(keep.sum()))
    return {k: np.concatenate(v) for k, v in out.items()}, np.array(offsets, dtype=np.int64)


def expected_allele_records(table, cutoffs, strand_mask, V):
    out = {k: [] for k in ("variant", "allele", "start", "strand", "score")}
    offsets, gained, lost = [0], [], []
    for t, cut in zip(table, cutoffs):
        hit = passes(t["score"], cut)
        for s in (0, 1):
            if not strand_mask & (1 << s):
                hit[:, s] = False
        keep = hit.ravel()                              # window-major, '+' before '-'
        out["variant"].append(np.repeat(t["variant"], 2)[keep])
        out["allele"].append(np.repeat(t["allele"], 2)[keep])
        out["start"].append(np.repeat(t["start"], 2)[keep])
        out["strand"].append(np.tile(np.array([1, 2], dtype=np.int8), len(t["variant"]))[keep])
        out["score"].append(t["score"].ravel()[keep])
        offsets.append(offsets[-1] + int(keep.sum()))
        has = np.zeros((V, 2), dtype=bool)
        has[out["variant"][-1], out["allele"][-1]] = True
        gained.append(int((has[:, 1] & ~has[:, 0]).sum()))
        lost.append(int((has[:, 0] & ~has[:, 1]).sum()))
    return {k: np.concatenate(v) for k, v in out.items()}, np.array(offsets, dtype=np.int64), np.array(gained), np.array(lost)


def snv_gained_lost(records, offsets, V):
    """(gained, lost) per motif out of SNV records: the variants with a record of state 2 / of state 1 (as test_gpu_variants.py counts them)."""
    motif = np.repeat(np.arange(len(offsets) - 1), np.diff(offsets))
    out = []
    for state in (2, 1):
        sel = records["state"] == state
        pairs = np.unique(motif[sel].astype(np.int64) * V + records["variant"][sel])
        out.append(np.bincount(pairs // V, minlength=len(offsets) - 1))
    return out[0], out[1]


# ------------------------------------------------------------------------------------------------ the boundary cases

def subset_table(table, sel, V):
    """The table of the variant list sel (ascending indices into the case's V variants), renumbered 0 .. len(sel) - 1.  A variant's
    records do not depend on its neighbours."""
    sel = np.asarray(sel, dtype=np.int64)
    assert np.all(np.diff(sel) > 0)
    new = np.full(V, -1, dtype=np.int64)
    new[sel] = np.arange(len(sel))
    out = []
    for t in table:
        keep = new[t["variant"]] >= 0
        out.append({k: (new[v[keep]] if k == "variant" else v[keep]) for k, v in t.items()})
    return out


def tile_counts(T):
    return (T - 1, T, T + 1, 2 * T, 2 * T + 1)


def chunk_sizes(T):
    """a few variants, exactly one tile, one tile and one variant"""
    return (7, T, T + 1)


def allele_windows(lo, hi, length, W):
    """allele_windows of ms_allele_dev.h, restated: windows of a haplotype whose allele has `length` bases, lo bases in front, hi behind."""
    n = length + min(hi - W + 1, 0) + min(lo, W - 1)
    return max(n, 0)


def _dna(rng, n):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)].copy()


def _lower(a, lo, hi):
    a[lo:hi] = np.frombuffer(bytes(a[lo:hi]).lower(), dtype=np.uint8)


def _alt_bytes(rng, a):
    return np.frombuffer(ALT_LETTERS, dtype=np.uint8)[rng.integers(0, len(ALT_LETTERS), a)].tobytes()


def _finish(case, oracle):
    names = case["names"]
    case["lens"] = np.array([len(case["chroms"][n]) for n in names])
    case["chrom_idx"] = np.asarray(case["chrom_idx"], dtype=np.int32)
    case["pos"] = np.asarray(case["pos"], dtype=np.int64)
    case["V"] = V = len(case["pos"])
    if case["kind"] == "snv":
        case["alt"] = np.asarray(case["alt"], dtype=np.uint8)
        assert len(case["alt"]) == V
        case["table"] = snv_flank_table(oracle, case["chroms"], names, case["mats"], case["chrom_idx"], case["pos"], case["alt"], 4)
        ref_scores = [t["ref"] for t in case["table"]]
    else:
        case["ref_len"] = np.asarray(case["ref_len"], dtype=np.int32)
        assert len(case["alts"]) == V and len(case["ref_len"]) == V
        case["alt_len"] = np.array([len(a) for a in case["alts"]], dtype=np.int64)
        case["table"] = allele_flank_table(oracle, case["chroms"], names, case["mats"], case["chrom_idx"], case["pos"], case["ref_len"],
                                           case["alts"], 4)
        ref_scores = [t["score"][t["allele"] == 0] for t in case["table"]]
    P = len(case["mats"])
    case["cutoffs"] = {"q90": np.array([float(np.quantile(s[np.isfinite(s)], 0.9)) for s in ref_scores]),
                       "all": np.full(P, ALL_PASS), "none": np.full(P, 2.0)}
    case.setdefault("lists", {"all": np.arange(V)})
    return case


def _snv_steps(oracle, dims):
    T, R = dims["variants"]["tile"], dims["variants"]["threads"]
    widths = (R // 2 - 1, R // 2, R // 2 + 1, R - 1, R, R + 1)
    rng = np.random.default_rng(20250301)
    lens = (100, R, 700)
    seqs = [_dna(rng, n) for n in lens]
    n_run = (300, 330)                                  # bases 100 + R + 300 ... of the packed genome: across a 32-base word edge
    seqs[2][n_run[0]:n_run[1]] = ord("N")
    _lower(seqs[2], 400, 450)
    seqs[2][500] = ord("R")                             # one IUPAC letter
    names = ["c100", "cR", "c700"]
    chrom_idx, pos = [], []
    for ci, L in enumerate(lens):                       # both ends of every chromosome
        chrom_idx += [ci, ci]
        pos += [0, L - 1]
    for W in widths:                                    # the last position whose first window is clipped, the first whose last one is
        for ci in (1, 2):
            if W <= lens[ci]:
                chrom_idx += [ci, ci]
                pos += [W - 1, lens[ci] - W]
    for x in (n_run[0] - 1, n_run[0], (n_run[0] + n_run[1]) // 2, n_run[1] - 1, n_run[1]):
        chrom_idx.append(2)
        pos.append(x)
    n_seeded = 2 * T + 1 - len(pos)
    ci = rng.choice(3, n_seeded, p=[0.04, 0.16, 0.8])
    chrom_idx += ci.tolist()
    pos += [int(rng.integers(0, lens[c])) for c in ci]
    alt = np.frombuffer(ALTS.encode(), dtype=np.uint8)[rng.integers(0, len(ALTS), len(pos))]
    return _finish({"kind": "snv", "chroms": {n: s.tobytes() for n, s in zip(names, seqs)}, "names": names,
                    "mats": [seeded_matrix(w, 300 + w) for w in widths], "chrom_idx": chrom_idx, "pos": pos, "alt": alt,
                    "marks": {"n_run": n_run, "n_run_chrom": 2}}, oracle)


def _edge_chromosome(rng, M):
    """2 (M + 1) + 50 bases with a run of N from W - 20 to W + 5, W = M + 1"""
    W = M + 1
    s = _dna(rng, 2 * W + 50)
    s[W - 20:W + 5] = ord("N")
    _lower(s, 100, 160)
    return s, (W - 20, W + 5)


def _snv_lds_edge(oracle, dims):
    M = dims["variants"]["lds_max_width"]
    widths = (M + 1, 11, M, 768, 767)
    rng = np.random.default_rng(20250302)
    s, n_run = _edge_chromosome(rng, M)
    L, W = len(s), M + 1
    pos = [0, L - 1, W - 1, L - W] + np.linspace(n_run[0] - 2, n_run[1] + 1, 12).astype(int).tolist() + rng.integers(0, L, 24).tolist()
    alt = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, len(pos))].copy()
    alt[5], alt[20] = ord("N"), ord("g")
    return _finish({"kind": "snv", "chroms": {"edge": s.tobytes()}, "names": ["edge"], "mats": [seeded_matrix(w, 400 + w) for w in widths],
                    "chrom_idx": [0] * len(pos), "pos": pos, "alt": alt, "marks": {"n_run": n_run, "n_run_chrom": 0}}, oracle)


def _snv_only_wide(oracle, dims):
    M = dims["variants"]["lds_max_width"]
    widths = (M + 1, M + 77)
    rng = np.random.default_rng(20250302)               # (the chromosome of snv_lds_edge: the same seed, drawn first)
    s, n_run = _edge_chromosome(rng, M)
    L = len(s)
    rng = np.random.default_rng(20250303)
    pos = [0, L - 1] + [x for W in widths for x in (W - 1, L - W)] + [n_run[0] - 1, n_run[0], n_run[1] - 1, n_run[1]] + rng.integers(0, L, 10).tolist()
    alt = np.frombuffer(ALTS.encode(), dtype=np.uint8)[rng.integers(0, len(ALTS), len(pos))]
    return _finish({"kind": "snv", "chroms": {"edge": s.tobytes()}, "names": ["edge"], "mats": [seeded_matrix(w, 500 + w) for w in widths],
                    "chrom_idx": [0] * len(pos), "pos": pos, "alt": alt, "marks": {"n_run": n_run, "n_run_chrom": 0}}, oracle)


def _al_lds_edge(oracle, dims):
    M = dims["alleles"]["lds_max_width"]
    widths = (M + 1, 11, M, 640, 639)
    rng = np.random.default_rng(20250304)
    s, n_run = _edge_chromosome(rng, M)
    L = len(s)
    shapes = ((1, 1), (0, 1), (1, 0), (0, 300), (300, 0), (40, 33), (2, 700))
    pos, ref_len, alts = [], [], []
    for r, a in shapes:                                 # at 0, at the far end, across the N run, and at two seeded places
        for x in (0, L - r, n_run[0] + 1 if r + a <= 2 else n_run[0] - 3, int(rng.integers(1, L - r)), int(rng.integers(1, L - r))):
            pos.append(x), ref_len.append(r), alts.append(_alt_bytes(rng, a))
    pos.append(L), ref_len.append(0), alts.append(_alt_bytes(rng, 5))          # (0, 5) behind the last base
    return _finish({"kind": "allele", "chroms": {"edge": s.tobytes()}, "names": ["edge"], "mats": [seeded_matrix(w, 600 + w) for w in widths],
                    "chrom_idx": [0] * len(pos), "pos": pos, "ref_len": ref_len, "alts": alts, "marks": {"n_run": n_run}}, oracle)


LONG_LENGTHS = (31, 32, 33, 63, 64, 65, 255, 256, 257)


def _al_long(oracle, dims):
    widths = (1, 8, 33, 70)
    rng = np.random.default_rng(20250305)
    L = 70_000
    s = _dna(rng, L)
    n_runs = ((10_000, 10_100), (69_000, 69_040))
    for lo, hi in n_runs:
        s[lo:hi] = ord("N")
    _lower(s, 40_000, 40_500)
    big = _dna(rng, MS_ALLELE_MAX_LEN)                  # the longest insertion: N runs and lower case inside it
    big[100:140] = ord("N")
    big[30_000:30_033] = ord("n")
    _lower(big, 5_000, 6_000)
    pos, ref_len, alts = [], [], []

    def add(x, r, alt):
        pos.append(int(x)), ref_len.append(r), alts.append(alt)
    add(777, 0, _alt_bytes(rng, 5))                     # listed first: no later allele starts on a 32-base edge of the alt plane
    add(35_000, 0, big.tobytes())
    add(2_000, MS_ALLELE_MAX_LEN, b"")                  # the longest deletion: bases 2 000 .. 67 535, the first N run inside it
    for n in LONG_LENGTHS:
        add(rng.integers(100, L - 400), 0, _alt_bytes(rng, n))
        add(rng.integers(100, L - 400), n, b"")
    add(n_runs[1][0] - 10, 0, _alt_bytes(rng, 64))      # an insertion in front of, and a deletion across, the second N run
    add(n_runs[1][0] - 20, 65, b"")
    A0 = sum(len(a) for a in alts)
    tail = (31 - A0) % 32 or 32                         # the alt bytes end at 32 k - 1 with this last allele, at 32 k + 1 with two more
    x_tail = int(rng.integers(100, L - 400))
    add(x_tail, 0, _alt_bytes(rng, tail))
    add(x_tail, 0, _alt_bytes(rng, tail + 2))
    V = len(pos)
    lists = {"tail_32k_minus_1": np.concatenate([np.arange(V - 2), [V - 2]]), "tail_32k_plus_1": np.concatenate([np.arange(V - 2), [V - 1]])}
    return _finish({"kind": "allele", "chroms": {"long": s.tobytes()}, "names": ["long"], "mats": [seeded_matrix(w, 700 + w) for w in widths],
                    "chrom_idx": [0] * V, "pos": pos, "ref_len": ref_len, "alts": alts, "lists": lists, "marks": {"n_runs": n_runs}}, oracle)


def _mixed(rng, n, L):
    pos, ref_len, alts = [], [], []
    for i in range(n):
        r, a = SHAPES[int(rng.integers(0, len(SHAPES)))]
        x = (0, L - r)[i % 2] if i % 16 < 2 else int(rng.integers(0, L - r + 1))
        pos.append(x), ref_len.append(r), alts.append(_alt_bytes(rng, a))
    return pos, ref_len, alts


def _al_tiles(oracle, dims):
    T = dims["alleles"]["tile"]
    widths = (5, 33, 129)
    rng = np.random.default_rng(20250306)
    L = 900
    s = _dna(rng, L)
    s[440:470] = ord("N")
    _lower(s, 600, 640)
    pos, ref_len, alts = _mixed(rng, 2 * T + 1, L)
    pos[T - 1], ref_len[T - 1], alts[T - 1] = 450, 0, _alt_bytes(rng, 300)     # the last variant of tile 0
    pos[T], ref_len[T], alts[T] = 200, 300, b""                                 # the first of tile 1
    return _finish({"kind": "allele", "chroms": {"c900": s.tobytes()}, "names": ["c900"], "mats": [seeded_matrix(w, 800 + w) for w in widths],
                    "chrom_idx": [0] * len(pos), "pos": pos, "ref_len": ref_len, "alts": alts, "marks": {}}, oracle)


def _al_only_wide(oracle, dims):
    M = dims["alleles"]["lds_max_width"]
    rng = np.random.default_rng(20250304)               # (the chromosome of al_lds_edge)
    s, n_run = _edge_chromosome(rng, M)
    L = len(s)
    rng = np.random.default_rng(20250307)
    shapes = ((0, 20), (20, 0), (1, 1), (0, 20), (20, 0), (1, 1), (0, 300), (300, 0), (40, 33), (2, 700), (1, 1), (0, 1))
    pos, ref_len, alts = [], [], []
    for i, (r, a) in enumerate(shapes):                 # three at x = 0, three at the far end, one across the N run, the others seeded
        x = 0 if i < 3 else L - r if i < 6 else n_run[0] - 3 if i == 6 else int(rng.integers(1, L - r))
        pos.append(x), ref_len.append(r), alts.append(_alt_bytes(rng, a))
    return _finish({"kind": "allele", "chroms": {"edge": s.tobytes()}, "names": ["edge"], "mats": [seeded_matrix(M + 1, 900)],
                    "chrom_idx": [0] * len(pos), "pos": pos, "ref_len": ref_len, "alts": alts, "marks": {"n_run": n_run}}, oracle)


_BUILDERS = {"snv_steps": _snv_steps, "snv_lds_edge": _snv_lds_edge, "snv_only_wide": _snv_only_wide, "al_lds_edge": _al_lds_edge,
             "al_long": _al_long, "al_tiles": _al_tiles, "al_only_wide": _al_only_wide}
_BUILT = {}


def build(name, oracle, dims=None):
    """The case `name`, built once per process (the oracle's tables are the cost) and never changed by its users."""
    if name not in _BUILT:
        if dims is None:
            from motifscan_amd import _lib
            dims = _lib.varscan_dims()
        _BUILT[name] = _BUILDERS[name](oracle, dims)
    return _BUILT[name]


def expected(case, which, strand_mask, sel=None):
    """What a scan of the case's variant list sel (default: all of them) must return at cutoff set `which`: (records, motif_offsets, gained, lost)."""
    V = case["V"]
    table = case["table"]
    n = V
    if sel is not None:
        table, n = subset_table(table, sel, V), len(sel)
    cutoffs = case["cutoffs"][which]
    if case["kind"] == "snv":
        rec, offsets = expected_snv_records(table, cutoffs, strand_mask)
        gained, lost = snv_gained_lost(rec, offsets, n)
        return rec, offsets, gained, lost
    return expected_allele_records(table, cutoffs, strand_mask, n)
