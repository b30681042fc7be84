"""Cases shared by tests/test_result_cases_host.py and tests/test_gpu_result_boundaries.py: synthetic hit lists in ms_result order for what
ms_result.hip does to a scan's hits after they are ordered -- dedup_kernel, the prefix sum with remap_offsets_kernel and
compact_hits_kernel, site_tables_kernel with fill_nan_kernel, pack_hits_kernel in both forms and the three pinned-host accessors.
Building a case needs neither a GPU nor the library; a device result is made of one with ms_result_from_hits.  (The two batches of
regions for the stream test at the end are the only scanned input: synth.make_regions with tandem repeats written over every third region.)

Order: per motif by region, then position, '+' (1) before '-' (2); (region, pos, strand) is unique within a motif.  Scores are small
integers, halves and a few negative values: ties are plentiful and every comparison is exact.  -0.0 is never used, so no cell holds
both zeros and a maximum is the same bits whichever of two equal scores gave it.

Expected values: the reference's recurrence in its literal form -- every (motif, region) as a list of MotifSite through
oracle.deduplicate_motif_sites (plain Python), the survivors mapped back to keep flags through the unique (pos, strand); the site
tables are len(x) and max(s.score for s in x) per cell.

CONDITIONS: what the cases together must put in front of the kernels, tallied from the arrays and the literal keep flags (the 18 gap
cells alone are counted where they are built).

Not covered: a result whose region index needs 31 bits, which ms_result_hits_packed12_host refuses before it packs anything.
ms_result_from_hits checks every region index against a host table of 8 * R bytes, 16 GiB at R = 2^31, so such a result cannot be
built here.
"""
import functools

import numpy as np

# The kernels of ms_result.hip are __launch_bounds__(256), launched with (n + 255) / 256 blocks of 256 threads, one hit per thread.
BLOCK = 256
# result_carve / result_block_bytes (ms_result.hip) and the three pinned layouts of the accessors round the hit count up to this.
ROUND = 65536

WIDTHS = (1, 2, 8, 33, 64)
SCORES = (-2.0, -0.5, 0.0, 0.5, 1.0, 1.5, 2.0, 3.0)

GAPS = ("W-1", "W", "W+1")
STRANDS = ("same", "opposite")
SECOND = ("below", "equal", "above")
GAP_CELLS = tuple(f"gap:{g}:{s}:{c}" for g in GAPS for s in STRANDS for c in SECOND)

TWELVE_R = (1, 2, 3, 4, 5, 2 ** 8, 2 ** 8 + 1, 2 ** 16, 2 ** 16 + 1, 2 ** 20, 2 ** 20 + 1)


def twelve_shift(R):
    """The shift of the 12-byte form made on demand for a result of R regions: the position and the strand bit get what R - 1 leaves."""
    return 32 - max(1, int(R - 1).bit_length())


CONDITIONS = dict({c: 1 for c in GAP_CELLS},
                  replaced_chain_sites=300, segments_across_block_edge=3, head_at_255=1, head_at_0=1, head_at_1=1,
                  trailing_empty_motifs=1, shared_region_across_motif_edge=1,
                  survivors_below_round=1, survivors_equal_round=1, survivors_above_round=1,
                  **{f"shift{twelve_shift(R)}_{what}": 1 for R in TWELVE_R for what in ("accepted", "refused")})


class Builder:
    """Sites per motif, in any order -> a case in ms_result order."""

    def __init__(self, name, widths, n_regions=None):
        self.name, self.widths, self.n_regions = name, [int(w) for w in widths], n_regions
        self.rows = [[] for _ in widths]                 # per motif: arrays (region, pos, strand, score) [4][k]
        self.next_region = [0] * len(widths)
        self.tally = {}

    def region(self, m, n=1):
        """the next n unused region indices of motif m (the first of them)"""
        r = self.next_region[m]
        self.next_region[m] += n
        return r

    def add(self, m, region, pos, strand, score):
        a = np.broadcast_arrays(np.asarray(region, dtype=np.float64), np.asarray(pos, dtype=np.float64), np.asarray(strand, dtype=np.float64),
                                np.asarray(score, dtype=np.float64))
        self.rows[m].append(np.stack([x.ravel() for x in a]))          # (positions below 2^53: exact in a double)
        self.next_region[m] = max(self.next_region[m], int(np.max(a[0], initial=-1)) + 1)

    def count(self, key, n=1):
        self.tally[key] = self.tally.get(key, 0) + n

    def case(self):
        off, cols = [0], []
        for rows in self.rows:
            a = np.concatenate(rows, axis=1) if rows else np.zeros((4, 0))
            a = a[:, np.lexsort((a[2], a[1], a[0]))]
            cols.append(a)
            off.append(off[-1] + a.shape[1])
        a = np.concatenate(cols, axis=1)
        R = self.n_regions if self.n_regions is not None else max(self.next_region + [0])
        case = {"name": self.name, "widths": np.array(self.widths, dtype=np.int32), "n_regions": int(R),
                "motif_offsets": np.array(off, dtype=np.int64), "seq_idx": a[0].astype(np.int64), "pos": a[1].astype(np.int64),
                "strand": a[2].astype(np.int8), "score": a[3].copy(), "tally": dict(self.tally)}
        return case


def order_problems(case):
    """What keeps a case from being a result of ms_scan: [] if it is in ms_result order with unique keys and valid values."""
    bad = []
    off, seq, pos, strand = case["motif_offsets"], case["seq_idx"], case["pos"], case["strand"]
    n = len(seq)
    if off[0] != 0 or off[-1] != n or (np.diff(off) < 0).any() or len(off) != len(case["widths"]) + 1:
        bad.append("motif_offsets")
    if not len(pos) == len(strand) == len(case["score"]) == n:
        bad.append("array lengths")
    if n and (seq.min() < 0 or seq.max() >= case["n_regions"] or pos.min() < 0 or not np.isin(strand, (1, 2)).all()):
        bad.append("values out of range")
    if np.isnan(case["score"]).any() or (np.signbit(case["score"]) & (case["score"] == 0)).any():
        bad.append("NaN or -0.0 score")
    for p in range(len(off) - 1):
        a, b = int(off[p]), int(off[p + 1])
        key = list(zip(seq[a:b].tolist(), pos[a:b].tolist(), strand[a:b].tolist()))
        if any(not x < y for x, y in zip(key, key[1:])):
            bad.append(f"motif {p}: keys not strictly increasing")
    return bad


def segments(case):
    """[(motif, first, end)] of the (motif, region) segments, in list order."""
    off, seq = case["motif_offsets"], case["seq_idx"]
    out = []
    for p in range(len(off) - 1):
        a, b = int(off[p]), int(off[p + 1])
        if a == b:
            continue
        cuts = [a] + (a + 1 + np.flatnonzero(np.diff(seq[a:b]))).tolist() + [b]
        out += [(p, s, e) for s, e in zip(cuts, cuts[1:])]
    return out


def motif_sites(case, keep=None):
    """{(motif, region): [MotifSite]} of the hits (of those with a keep flag): the reference's shape, without the empty cells"""
    from oracle.oracle import MotifSite
    seq, pos, score, strand = case["seq_idx"], case["pos"].tolist(), case["score"].tolist(), case["strand"].tolist()
    out = {}
    for p, s, e in segments(case):
        x = [MotifSite(pos[i], score[i], "+" if strand[i] == 1 else "-") for i in range(s, e) if keep is None or keep[i]]
        if x:
            out[(p, int(seq[s]))] = x
    return out


def literal_keep(case):
    """Keep flags by oracle.deduplicate_motif_sites (scanner.py:156-193 in plain Python) on every (motif, region)."""
    from oracle import oracle
    pos, strand = case["pos"].tolist(), case["strand"].tolist()
    keep = np.zeros(len(pos), dtype=bool)
    sites = motif_sites(case)
    for p, s, e in segments(case):
        r = int(case["seq_idx"][s])
        kept = oracle.deduplicate_motif_sites([[sites[(p, r)]]], [int(case["widths"][p])])[0][0]
        index = {(pos[i], strand[i]): i for i in range(s, e)}
        assert len(index) == e - s
        for site in kept:
            keep[index[(site.start, 1 if site.strand == "+" else 2)]] = True
    return keep


def filtered(case, keep):
    """The case's arrays after de-duplication with these keep flags."""
    off = case["motif_offsets"]
    kept_before = np.concatenate([[0], np.cumsum(keep)]).astype(np.int64)
    return {"motif_offsets": kept_before[off], "seq_idx": case["seq_idx"][keep], "pos": case["pos"][keep], "score": case["score"][keep],
            "strand": case["strand"][keep]}


def site_tables_expected(case, keep=None):
    """io/__init__.py:23-33 as it stands: (n_sites int32 [P][R], max_score float64 [P][R]) = len(x) and max(s.score for s in x) of
    every cell's site list x, 0 and NaN where there is none."""
    P, R = len(case["widths"]), case["n_regions"]
    n_sites = np.zeros((P, R), dtype=np.int32)
    max_score = np.full((P, R), np.nan)
    for (p, r), x in motif_sites(case, keep).items():
        n_sites[p, r] = len(x)
        max_score[p, r] = max(s.score for s in x)
    return n_sites, max_score


def tally_of(case, keep):
    """The case's own counts (the gap cells) + what the arrays and the literal keep flags show."""
    t = dict(case["tally"])
    off, strand = case["motif_offsets"], case["strand"]
    n = len(strand)
    for p, s, e in segments(case):
        if (s // BLOCK) != ((e - 1) // BLOCK):
            t["segments_across_block_edge"] = t.get("segments_across_block_edge", 0) + 1
        if e - s >= 2 and s > 0 and s % BLOCK in (BLOCK - 1, 0, 1):              # a head whose walk has something to decide
            k = f"head_at_{s % BLOCK}"
            t[k] = t.get(k, 0) + 1
        if e - s >= 2 and (strand[s:e] == strand[s]).all() and keep[s:e].sum() == 1 and keep[e - 1] \
                and (np.diff(case["score"][s:e]) > 0).all():                      # every site replaced the one before it
            t["replaced_chain_sites"] = max(t.get("replaced_chain_sites", 0), e - s)
    if n:
        t["trailing_empty_motifs"] = int((off[1:-1] == n).sum()) if off[-2] == n else 0
    for p in range(len(off) - 2):
        a, b, c = int(off[p]), int(off[p + 1]), int(off[p + 2])
        if a < b < c and case["seq_idx"][b - 1] == case["seq_idx"][b] and abs(int(case["pos"][b]) - int(case["pos"][b - 1])) < min(case["widths"][p:p + 2]):
            t["shared_region_across_motif_edge"] = t.get("shared_region_across_motif_edge", 0) + 1
    if n > ROUND:
        kept = int(keep.sum())
        k = "survivors_below_round" if kept < ROUND else "survivors_equal_round" if kept == ROUND else "survivors_above_round"
        t[k] = t.get(k, 0) + 1
    return t


def add_tally(total, t):
    for k, v in t.items():
        total[k] = max(total.get(k, 0), v) if k == "replaced_chain_sites" else total.get(k, 0) + v
    return total


def unmet_conditions(total):
    return [f"{k}: {total.get(k, 0)} < {v}" for k, v in CONDITIONS.items() if total.get(k, 0) < v]


# ------------------------------------------------------------------------------------------------------- de-dup families --

def _add_gaps(b, base_pos=(0, 5000)):
    """Pairs of sites W - 1, W and W + 1 apart, on one strand and on both, the second scoring below, like and above the first: each
    cell in a region of its own, at the region's start and further in."""
    for m, W in enumerate(b.widths):
        for g, d in zip(GAPS, (W - 1, W, W + 1)):
            for st in STRANDS:
                if d == 0 and st == "same":
                    continue                                   # (W = 1: the same site twice)
                for c, second in zip(SECOND, (0.5, 1.0, 1.5)):
                    for k, p0 in enumerate(base_pos):
                        s0 = 1 + (k + m) % 2
                        s1 = s0 if st == "same" else 3 - s0
                        if d == 0 and s0 == 2:
                            s0, s1 = 1, 2
                        b.add(m, b.region(m), [p0, p0 + d], [s0, s1], [1.0, second])
                        b.count(f"gap:{g}:{st}:{c}")


def _chain_scores(kind, n, rng):
    k = np.arange(n)
    if kind == "ascending":
        return -2.0 + 0.5 * k
    if kind == "descending":
        return 200.0 - 0.5 * k
    if kind == "constant":
        return np.full(n, 1.5)
    if kind == "sawtooth":
        return np.array([0.0, 1.0, 2.0, 0.5])[k % 4]
    return rng.choice([-0.5, 0.0, 1.0, 1.0, 2.0], size=n)       # four values


CHAIN_LENGTHS = (2, 3, 17, 300)
CHAIN_KINDS = ("ascending", "descending", "constant", "sawtooth", "random")


def _add_chains(b, rng):
    """Runs of sites at spacing 1 and at spacing W - 1 on one strand (W >= 2): every site overlaps the one before it."""
    for m, W in enumerate(b.widths):
        if W < 2:
            continue
        for spacing in sorted({1, W - 1}):
            for n in CHAIN_LENGTHS:
                for j, kind in enumerate(CHAIN_KINDS):
                    b.add(m, b.region(m), 7 + spacing * np.arange(n), 1 + (j + n) % 2, _chain_scores(kind, n, rng))


def _add_interleaved(b, rng):
    """'+' and '-' sites on the same positions and on alternating ones: the site a strand keeps lies several list entries back."""
    for m, W in enumerate(b.widths):
        for n in (4, 11, 60):
            p = 3 + np.arange(n)
            r = b.region(m)                                      # both strands on every position
            b.add(m, r, p, 1, rng.choice(SCORES, size=n))
            b.add(m, r, p, 2, rng.choice(SCORES, size=n))
            r = b.region(m)                                      # '+' on the even positions, '-' on the odd ones
            b.add(m, r, p, 1 + (p % 2), rng.choice(SCORES, size=n))
            r = b.region(m)                                      # runs of one strand between sites of the other, random steps
            p = np.cumsum(rng.choice([1, 1, 2, 3, W, W + 1], size=n))
            b.add(m, r, p, 1 + (rng.random(n) < 0.3), rng.choice(SCORES, size=n))


def _add_region_edges(b):
    """Equal and near positions in neighbouring regions: the walk ends at the region change, whatever the scores are."""
    for m, W in enumerate(b.widths):
        for first, second in ((1.0, 2.0), (2.0, 1.0), (1.0, 1.0)):
            r = b.region(m, 2)
            b.add(m, r, [100, 100 + W], 1, [0.5, first])
            q = sorted({100 + W - W // 2, 100 + W, 100 + W + max(W - 1, 1)})
            b.add(m, r + 1, q, 1, [second] * (len(q) - 1) + [0.0])


def _build_families():
    rng = np.random.default_rng(20241)
    b = Builder("families", WIDTHS)
    _add_gaps(b)
    _add_chains(b, rng)
    _add_interleaved(b, rng)
    _add_region_edges(b)
    return b.case()


def _random_segment(rng, n, W):
    """n sites of one region: steps of 0 ('+' then '-' on one position), 1, 2, W - 1, W and W + 5, strands mixed."""
    pos, strand = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int8)
    p, s = 11, 1
    steps = [0, 1, 1, 2, max(W - 1, 1), W, W + 5]
    for k in range(n):
        if k:
            step = int(rng.choice(steps))
            s2 = 1 + int(rng.random() < 0.4)
            if step == 0 and not (s == 1 and s2 == 2):
                step = 1
            p, s = p + step, s2
        else:
            s = 1 + int(rng.random() < 0.4)
        pos[k], strand[k] = p, s
    return pos, strand, rng.choice([0.0, 0.5, 1.0, 2.0], size=n)


def _build_seams():
    """Segments of 1, 255, 256, 257 and 513 hits, single-hit regions in front of them so that their heads fall on the last thread of a
    block, the first and the second; 513 hits from a block's last thread on span three blocks.  Two motifs: the second starts
    wherever the first ends."""
    rng = np.random.default_rng(20242)
    widths = (8, 33)
    b = Builder("seams", widths)
    at = 0                                                       # flat index of the next hit

    def filler_to(m, residue):
        nonlocal at
        while at % BLOCK != residue:
            b.add(m, b.region(m), int(rng.integers(0, 50)), 1 + at % 2, 1.0)
            at += 1

    def segment(m, n):
        nonlocal at
        pos, strand, score = _random_segment(rng, n, widths[m])
        b.add(m, b.region(m), pos, strand, score)
        at += n

    for m, plan in enumerate((((255, 257), (0, 256), (1, 255), (0, 513), (None, 1), (255, 513), (None, 1), (1, 257)),
                              ((255, 513), (None, 255), (1, 256), (0, 257), (None, 1)))):
        for residue, n in plan:
            if residue is not None:
                filler_to(m, residue)
            segment(m, n)
    return b.case()


def _build_motif_edges():
    """Empty motifs first, in the middle, two in a row and last; neighbouring motifs whose last and first region are the same index,
    with positions closer than either width."""
    widths = (8, 33, 33, 2, 64, 64, 8, 1, 5)
    b = Builder("motif_edges", widths, n_regions=12)
    # motif 0 empty; 1 and 2 share region 7 across their edge: the first site of motif 2 would replace / lose to the last of motif 1
    b.add(1, 2, [5, 9], 1, [1.0, 2.0])
    b.add(1, 7, [90, 100], [1, 1], [0.5, 1.0])
    b.add(2, 7, [101, 110, 200], [1, 1, 2], [2.0, 3.0, 1.0])
    b.add(2, 11, [0, 1], 2, [1.0, 1.0])
    # motif 3 empty; 4 holds the last region alone; 5 starts in the same region with a lower score
    b.add(4, 11, [40, 50], 2, [0.5, 2.0])
    b.add(5, 11, [51, 52], 2, [1.0, 0.5])
    # 6 and 7: two empty motifs in a row; 8 ends the list with hits in regions 0 and 11
    b.add(8, 0, [0, 4, 5, 9], 1, [1.0, 0.5, 1.0, 1.0])
    b.add(8, 11, [3, 3, 7], [1, 2, 1], [0.0, -0.5, 2.0])
    first = b.case()
    # the same with empty motifs at the end, the last hit one that is dropped / kept
    widths2 = (8, 33, 5, 5)
    out = [first]
    for name, last in (("motif_edges_last_dropped", 0.5), ("motif_edges_last_kept", 3.0)):
        b = Builder(name, widths2, n_regions=4)
        b.add(0, 3, [10, 12], 1, [1.0, 1.0])
        b.add(1, 3, [11, 20, 40], 1, [2.0, 1.0, last])
        out.append(b.case())
    return out


def _build_single_motif():
    b = Builder("single_motif", (8,))
    _add_gaps(b, base_pos=(3,))
    b.add(0, b.region(0), 2 * np.arange(40), 1 + np.arange(40) % 2, np.array([1.0, 0.5, 2.0, 2.0, -0.5])[np.arange(40) % 5])
    return b.case()


def _build_rounding(name, n_hits, n_dropped):
    """n_hits hits of which exactly n_dropped are dropped: single-site regions, regions of four sites W apart, and n_dropped regions
    that hold one overlapping pair -- in two motifs, positions small enough for the 12-byte form."""
    rng = np.random.default_rng(n_hits * 7 + n_dropped)
    widths = (8, 33)
    b = Builder(name, widths)
    quads = 25
    singles = n_hits - 2 * n_dropped - 4 * quads
    share = (singles * 3 // 5, singles - singles * 3 // 5)
    for m, W in enumerate(widths):
        for k in range(n_dropped // 2 + (m == 0) * (n_dropped % 2)):
            b.add(m, 1000 * (k + 1) + m, [200 + k, 200 + k + W - 1], 1 + k % 2, [1.0, 1.0 + 0.5 * (k % 3 - 1)])
        for k in range(quads // 2 + (m == 0) * (quads % 2)):
            b.add(m, 37 + 1500 * k + m, 60 + W * np.arange(4), 2 - k % 2, [2.0, 2.0, 1.0, 3.0])
        taken = np.unique(np.concatenate([x[0] for x in b.rows[m]])).astype(np.int64) if b.rows[m] else np.zeros(0, dtype=np.int64)
        free = np.setdiff1d(np.arange(n_hits), taken)[:share[m]]
        b.add(m, free, rng.integers(0, 1 << 13, size=share[m]), 1 + (rng.random(share[m]) < 0.5), rng.choice(SCORES, size=share[m]))
    b.n_regions = n_hits
    return b.case()


def _build_noops():
    b = Builder("nothing_dropped", WIDTHS)
    for m, W in enumerate(WIDTHS):
        for k in range(6):
            r = b.region(m)
            b.add(m, r, 10 + W * np.arange(20), 1, 1.0 + 0.5 * (np.arange(20) % 3))
            b.add(m, r, 10 + W * np.arange(20) + (k % 2), 2, 2.0)
    return [b.case(), Builder("empty", (8, 33, 2), n_regions=5).case()]


@functools.lru_cache(maxsize=None)
def dedup_cases():
    """{name: case}; every case also holds "keep", its literal keep flags.  Built once per process; nothing may write to the arrays."""
    cases = [_build_families(), _build_seams()] + _build_motif_edges() + [_build_single_motif()] + _build_noops()
    cases += [_build_rounding("round_below", ROUND + 4, 5), _build_rounding("round_equal", ROUND + 4, 4),
              _build_rounding("round_above", ROUND + 4, 3), _build_rounding("round_all_survive", ROUND, 0)]
    out = {}
    for c in cases:
        c["keep"] = literal_keep(c)
        for k in ("motif_offsets", "seq_idx", "pos", "strand", "score", "keep", "widths"):
            c[k].setflags(write=False)
        out[c["name"]] = c
    return out


SMALL_DEDUP = ("families", "seams", "motif_edges", "motif_edges_last_dropped", "motif_edges_last_kept", "single_motif", "nothing_dropped", "empty")
ROUNDING = ("round_below", "round_equal", "round_above", "round_all_survive")


# --------------------------------------------------------------------------------------------------------- compact forms --

def encode16(case):
    """coord = seq_idx << 32 | pos << 1 | (strand - 1), as include/motifscan_amd.h states it"""
    return (case["seq_idx"].astype(np.uint64) << np.uint64(32)) | (case["pos"].astype(np.uint64) << np.uint64(1)) | (case["strand"] == 2).astype(np.uint64)


def encode12(case, shift):
    """coord32 = seq_idx << shift | pos << 1 | (strand - 1)"""
    w = (case["seq_idx"].astype(np.uint64) << np.uint64(shift)) | (case["pos"].astype(np.uint64) << np.uint64(1)) | (case["strand"] == 2).astype(np.uint64)
    assert (w >> np.uint64(32) == 0).all()
    return w.astype(np.uint32)


def decode16(coord):
    coord = np.asarray(coord, dtype=np.uint64)
    return ((coord >> np.uint64(32)).astype(np.int64), ((coord & np.uint64(0xFFFFFFFF)) >> np.uint64(1)).astype(np.int64),
            ((coord & np.uint64(1)) + np.uint64(1)).astype(np.int8))


def decode12(coord, shift):
    coord = np.asarray(coord, dtype=np.uint32)
    return ((coord >> np.uint32(shift)).astype(np.int64), ((coord & np.uint32((1 << shift) - 1)) >> np.uint32(1)).astype(np.int64),
            ((coord & np.uint32(1)) + np.uint32(1)).astype(np.int8))


def fits16(case):
    return bool((case["pos"] < 2 ** 31).all())


def fits12(case):
    """whether ms_result_hits_packed12_host can pack the case on demand: the regions leave the positions enough bits"""
    return bool((case["pos"] < 2 ** (twelve_shift(case["n_regions"]) - 1)).all())


def _spread(b, rng, n, R, pos_limit, motifs):
    """n hits per motif, regions 0 ... R - 1, positions 10, 11, ... (below pos_limit)"""
    assert 10 + n <= pos_limit
    for m in motifs:
        region = np.sort(rng.integers(0, R, size=n))
        b.add(m, region, 10 + np.arange(n), 1 + (rng.random(n) < 0.5), rng.choice(SCORES, size=n))


@functools.lru_cache(maxsize=None)
def compact_cases():
    """{name: case} with "accept16", "accept12" and "shift" (the 12-byte form's, whether it is accepted or not)."""
    out = {}
    rng = np.random.default_rng(20243)
    # 16-byte form: the four corner positions on both strands among 257 hits; then one hit one past the last position that fits
    b = Builder("sixteen_corners", (8, 33), n_regions=300)
    for m in (0, 1):
        for r in (0, 150 + m, 299):
            for s in (1, 2):
                b.add(m, r, [0, 1, 2 ** 31 - 2, 2 ** 31 - 1], s, [1.0, 0.5, -0.5, 2.0])
    _spread(b, rng, (257 - 48 + 1) // 2, 300, 2 ** 31, (0,))
    b.add(1, np.arange(20, 20 + 257 - 48 - 105), 2 ** 31 - 1 - np.arange(257 - 48 - 105), 2, 1.5)
    out[b.name] = b.case()
    for at in (0, 128, 256):                                     # 257 hits, each in a region of its own; the hit at index `at` does not fit
        b = Builder(f"sixteen_refused_at_{at}", (8,), n_regions=257)
        pos = rng.integers(0, 1 << 20, size=257)
        pos[at] = 2 ** 31
        b.add(0, np.arange(257), pos, 1 + np.arange(257) % 2, rng.choice(SCORES, size=257))
        out[b.name] = b.case()
    # 12-byte form on demand: per R the word with every bit set (region R - 1, the last position that fits, '-'), then one position more
    for R in TWELVE_R:
        shift = twelve_shift(R)
        for what in ("accepted", "refused"):
            b = Builder(f"twelve_{what}_R{R}", (8, 33), n_regions=R)
            _spread(b, rng, 20, R, 2 ** (shift - 1), (0, 1))
            b.add(1, R - 1, 2 ** (shift - 1) - 1, 2, 3.0)
            if what == "refused":
                b.add(0, 0, 2 ** (shift - 1), 1, 3.0)
            b.count(f"shift{shift}_{what}")
            out[b.name] = b.case()
    for name in ("empty", "one_hit"):
        b = Builder(name, (8, 33, 2), n_regions=5)
        if name == "one_hit":
            b.add(1, 4, 77, 2, 1.5)
        out[b.name] = b.case()
    for c in out.values():
        c["shift"] = twelve_shift(c["n_regions"])
        c["accept16"], c["accept12"] = fits16(c), fits12(c)
        for k in ("motif_offsets", "seq_idx", "pos", "strand", "score", "widths"):
            c[k].setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------------ de-dup under a stream --

STREAM_MOTIFS = 40            # of synth.load_motif_set
STREAM_MIN_DROPPED = 50       # sites the two batches must lose to de-duplication (the oracle's scan of them loses 100)


def low_complexity_batch(n_regions, length, seed):
    """Regions of `length` bp; every third one a tandem repeat of a unit of 1 ... 6 bases, where a motif's sites recur at the period and
    overlap each other."""
    from motifscan_amd import synth
    bases, offsets = synth.make_regions(n_regions, length, seed=seed, frac_n=0.02)
    bases = bases.copy()
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    for r in range(0, n_regions, 3):
        unit = acgt[rng.integers(0, 4, size=int(rng.integers(1, 7)))]
        a, b = int(offsets[r]), int(offsets[r + 1])
        bases[a:b] = np.resize(unit, b - a)
    return bases, offsets


def stream_batches():
    """two batches of about 200 regions of 300 bp"""
    return [low_complexity_batch(200, 300, 31), low_complexity_batch(193, 300, 32)]
