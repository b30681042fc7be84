"""
motifscan_amd.bipartite -- bipartite motifs: two half-sites of a PWM set with a spacer of VARIABLE length between them, in a fixed
relative orientation (nuclear-receptor DR / IR repeats, p53, bZIP / bHLH composite sites, the SOX-OCT element).  A single PWM cannot
express such a site -- it has one fixed width -- and `pairs.pair_spacing` only says which spacings two motifs prefer; this scores the
model that histogram suggests.  include/motifscan_amd.h has the definition the device follows (ms_scan_best_bipartite,
ms_bipartite.hip); this module holds the spec, the way from a spacing histogram to specs, and the definition restated in numpy.

    Bipartite(a, b, flip, gap_min, gap_max)
                                      a, b: motif indices of the PWM list (a == b is allowed); flip 0: b is read on a's strand, 1: on the
                                      opposite one; the spacer holds gap_min .. gap_max bases.  On '+' the site is a's half, the spacer,
                                      b's half; on '-' the same composite read on the other strand.
    best_bipartite_host(matrices, specs, sequences, strand=3)
                                      (score, pos, strand, gap) planes [n_specs][R] as ms_scan_best_bipartite defines them: the same
                                      additions in the same order, so the device's planes equal these byte for byte
    element_sums_host(matrix, seq)    (forward, reverse) raw sums of every window start of one PWM, as ms_scan_best forms them
    scorable_host(matrices, spec)     the header's test for a spec that is scored at all
    specs_from_spacing(spacing, anchor, partners, widths, min_count=1, max_gap=64)
                                      the non-overlapping bins of a pairs.PairSpacing as specs, one per relative arrangement with counts
    BipartiteSites(score, start, strand, gap)
                                      what Scanner.best_sites_bipartite returns: (n_specs, n_regions) arrays, start in genome coordinates

The device side is _lib.scan_best_bipartite and Scanner.best_sites_bipartite / rank_sum_bipartite; there is no CPU path behind those.
"""
from collections import namedtuple

import numpy as np

_STRAND_FLAG = {"+": 1, "-": 2, "both": 3}

# ASCII -> 0 .. 3 for A, C, G, T in either case, -1 for every other byte (as the library's packer reads a base)
_CODE = np.full(256, -1, dtype=np.int8)
for _i, _ch in enumerate("ACGT"):
    _CODE[ord(_ch)] = _CODE[ord(_ch.lower())] = _i

Bipartite = namedtuple("Bipartite", ["a", "b", "flip", "gap_min", "gap_max"])
Bipartite.__doc__ = """One bipartite spec over a PWM list: motif indices a and b, flip (0: b on a's strand, 1: b reverse-complemented), and the
spacer lengths gap_min .. gap_max (0 <= gap_min <= gap_max <= the cap ms_debug_bipartite_dims reports)."""

BipartiteSites = namedtuple("BipartiteSites", ["score", "start", "strand", "gap"])
BipartiteSites.__doc__ = """Scanner.best_sites_bipartite: (n_specs, n_regions) arrays -- score (float64, NaN where no placement wins), start (int64,
the leftmost base of the whole site in genome coordinates, -1 where none), strand (int8: 1 '+', 2 '-', 0 where none) and gap (int16: the
winner's spacer length, -1 where none)."""


def spec_arrays(specs):
    """(a, b int32, flip uint8, gap_min, gap_max int32) [n]: the arrays ms_scan_best_bipartite reads, from Bipartite objects or 5-tuples."""
    rows = [tuple(int(v) for v in s) for s in specs]
    if any(len(r) != 5 for r in rows):
        raise ValueError("a bipartite spec is (a, b, flip, gap_min, gap_max)")
    if any(not 0 <= r[2] <= 255 for r in rows):
        raise ValueError("flip must be 0 or 1")
    cols = list(zip(*rows)) if rows else [()] * 5
    return (np.array(cols[0], dtype=np.int32), np.array(cols[1], dtype=np.int32), np.array(cols[2], dtype=np.uint8),
            np.array(cols[3], dtype=np.int32), np.array(cols[4], dtype=np.int32))


def _codes(seq):
    raw = seq.encode("latin-1", "replace") if isinstance(seq, str) else bytes(seq)
    return _CODE[np.frombuffer(raw, dtype=np.uint8)].astype(np.int64)


def max_raw_host(matrix):
    """The PWM scan's max_raw: the column maxima, none below 0, added in column order."""
    m = np.asarray(matrix, dtype=np.float64)
    total = 0.0
    for c in range(m.shape[1]):
        best = 0.0
        for b in range(4):
            if m[b, c] > best:
                best = float(m[b, c])
        total += best
    return total


def element_sums_host(matrix, seq):
    """(fwd, rev) float64 [max(L - W + 1, 0)]: F(p) and R(p) of every window start -- columns in order, forward M[x][c], reverse
    M[3 - x][W - 1 - c], a non-ACGT base adds nothing."""
    m = np.asarray(matrix, dtype=np.float64)
    x = seq if isinstance(seq, np.ndarray) else _codes(seq)
    W, n = m.shape[1], len(x) - m.shape[1] + 1
    if n <= 0:
        return np.zeros(0), np.zeros(0)
    fwd, rev = np.zeros(n), np.zeros(n)
    for c in range(W):
        xc = x[c:c + n]
        known, xs = xc >= 0, np.where(xc < 0, 0, xc)
        fwd = np.where(known, fwd + m[xs, c], fwd)
        rev = np.where(known, rev + m[3 - xs, W - 1 - c], rev)
    return fwd, rev


def _entries_ok(m):
    return not np.isnan(m).any() and not (m == np.inf).any()


def scorable_host(matrices, spec):
    """No entry of either element is NaN or +inf, and max_raw_a + max_raw_b is a finite number > 0."""
    ma, mb = np.asarray(matrices[spec[0]], dtype=np.float64), np.asarray(matrices[spec[1]], dtype=np.float64)
    d = max_raw_host(ma) + max_raw_host(mb)
    return bool(np.isfinite(d) and d > 0.0 and _entries_ok(ma) and _entries_ok(mb))


def best_bipartite_host(matrices, specs, sequences, strand=3):
    """ms_scan_best_bipartite restated: (score float64, pos int32, strand int8, gap int16) [n_specs][R].  matrices: the PWMs [4][W];
    strand: 1, 2, 3 or '+', '-', 'both'."""
    mask = _STRAND_FLAG.get(strand, strand)
    if mask not in (1, 2, 3):
        raise ValueError(f"invalid strand mask {strand!r} (1 '+', 2 '-', 3 both)")
    mats = [np.asarray(m, dtype=np.float64) for m in matrices]
    specs, codes = [Bipartite(*s) for s in specs], [_codes(s) for s in sequences]
    shape = (len(specs), len(codes))
    score, pos = np.full(shape, np.nan), np.full(shape, -1, dtype=np.int32)
    strd, gap = np.zeros(shape, dtype=np.int8), np.full(shape, -1, dtype=np.int16)
    sums = {}                                              # (motif, region) -> (F, R): the specs share their elements' sums

    def sums_of(m, r):
        if (m, r) not in sums:
            sums[(m, r)] = element_sums_host(mats[m], codes[r])
        return sums[(m, r)]
    for k, sp in enumerate(specs):
        if not scorable_host(mats, sp):
            continue
        Wa, Wb = mats[sp.a].shape[1], mats[sp.b].shape[1]
        denom = max_raw_host(mats[sp.a]) + max_raw_host(mats[sp.b])
        n_gaps = sp.gap_max - sp.gap_min + 1
        for r, x in enumerate(codes):
            n_pos = len(x) - (Wa + sp.gap_min + Wb) + 1    # placement starts at the smallest gap
            if n_pos <= 0:
                continue
            (fa, ra), (fb, rb) = sums_of(sp.a, r), sums_of(sp.b, r)
            second, first = (rb, fb) if sp.flip else (fb, rb)          # Y, read shifted on '+'; Y', read in place on '-'
            raw = np.full((n_pos, 2, n_gaps), -np.inf)     # [p]['+', '-'][g - g_min]: the walk's order when flattened
            for j in range(n_gaps):
                g = sp.gap_min + j
                n = len(x) - (Wa + g + Wb) + 1
                if n <= 0:
                    break
                if mask & 1:
                    raw[:n, 0, j] = fa[:n] + second[Wa + g:Wa + g + n]
                if mask & 2:
                    raw[:n, 1, j] = first[:n] + ra[Wb + g:Wb + g + n]
            q = (raw / denom).ravel()
            w = int(np.argmax(q))                          # the first maximum is the walk's winner
            if q[w] > -np.inf:
                score[k, r], pos[k, r] = q[w], w // (2 * n_gaps)
                strd[k, r], gap[k, r] = 1 + (w // n_gaps) % 2, sp.gap_min + w % n_gaps
    return score, pos, strd, gap


def specs_from_spacing(spacing, anchor, partners, widths, min_count=1, max_gap=64):
    """The specs a pairs.PairSpacing (made with oriented=True) suggests: per partner row and per relative arrangement that holds a bin of
    at least min_count pairs whose two sites do NOT overlap, one Bipartite over the gaps of those bins (gap_min .. gap_max = the
    smallest and the greatest of them; bins of a gap above max_gap are left out).  partners: the motif index of every row (the `motifs`
    the histogram was made with); widths: the width of every motif.  The centre distance x of a bin gives the gap,
    |x| - (W_anchor + W_partner) / 2, and its sign which motif comes first:

        partner on the anchor's strand, downstream (x > 0)      Bipartite(anchor, partner, 0, ..)
        partner on the anchor's strand, upstream (x < 0)        Bipartite(partner, anchor, 0, ..)
        partner on the opposite strand, downstream              Bipartite(anchor, partner, 1, ..)    the two halves face each other

    A partner on the opposite strand UPSTREAM of the anchor (the halves point away from each other) has no spec: a spec's first half is
    read forward on one of the two strands, and neither reading of that arrangement begins so.  Its bins are left out.
    Returns the specs in row order, arrangements in the order above."""
    if spacing.oriented is None:
        raise ValueError("specs_from_spacing needs a PairSpacing made with oriented=True")
    widths = np.asarray(widths, dtype=np.int64)
    anchor, min_count, max_gap = int(anchor), int(min_count), int(max_gap)
    partners = [int(p) for p in partners]
    oriented, xs = np.asarray(spacing.oriented), np.asarray(spacing.x)
    if len(partners) != oriented.shape[0]:
        raise ValueError(f"partners must name the motif of each of the {oriented.shape[0]} rows")
    out = []
    for i, partner in enumerate(partners):
        diff, both = int(widths[partner] - widths[anchor]), int(widths[partner] + widths[anchor])
        n_bins = oriented.shape[2] - (diff & 1)            # an odd width difference leaves the last bin unused
        x2 = np.rint(2 * xs[i, :n_bins]).astype(np.int64)  # twice the distance: whole numbers
        gaps = (np.abs(x2) - both) // 2                    # |x| - (W_a + W_p) / 2 (2 |x| and W_a + W_p have the same parity)
        for o, side, first, second, flip in ((0, 1, anchor, partner, 0), (0, -1, partner, anchor, 0), (1, 1, anchor, partner, 1)):
            use = (np.sign(x2) == side) & (gaps >= 0) & (gaps <= max_gap) & (oriented[i, o, :n_bins] >= max(min_count, 1))
            if use.any():
                out.append(Bipartite(first, second, flip, int(gaps[use].min()), int(gaps[use].max())))
    return out
