"""
motifscan_amd.pairs -- questions about PAIRS of motifs, answered on the device from the hit arrays of a scan (ms_pairs.hip).  The
reference has no counterpart: it hands back nested site lists, and at 10^6 regions x 579 motifs a motif x motif matrix or a per-region
join of one motif's sites with every other motif's is hours of Python.

    cooccurrence(motif_sites, motifs=slice(None)) -> int64 [len(motifs), P]
        out[a][j] = regions that hold at least one site of motif motifs[a] and at least one of motif j (ms_result_cooccurrence).
        The diagonal is the per-motif "regions with a site" count; the full matrix is symmetric.
    pair_spacing(motif_sites, pwms, anchor, max_dist=100, motifs=slice(None), oriented=True) -> PairSpacing
        for the anchor motif against each partner motif: the histogram of the centre-to-centre distances of their sites in the same
        region, by relative orientation (ms_result_pair_spacing), with the x axis in bp and -- oriented=True -- the counts folded onto
        the anchor's strand.

`motif_sites` is what `plot` accepts: a `MotifSites` (while it still owns its device result that result is read in place, otherwise its
flat arrays are uploaded) or the reference's nested lists.  Both quantities are sums over regions: the matrices of region shards add up
(one all-reduce across ranks; `ScanResult.cooccurrence(out=<device pointer>)` writes where a collective can read).  The significance of
a cell or of a spacing peak is host arithmetic over these small arrays and is not done here.  There is no CPU path: without a device
these functions raise.
"""
from collections import namedtuple

import numpy as np

from . import _lib
from .plot import _device_sites

PairSpacing = namedtuple("PairSpacing", ["counts", "n_pairs", "x", "oriented"])
PairSpacing.__doc__ = """counts int64 [rows][4][2 * max_dist + 1]: pairs by orientation o = 2 * (anchor on '-') + (partner on '-') and bin;
n_pairs int64 [rows]: all ordered pairs in the same region, at any distance; x float64 [rows][2 * max_dist + 1]: the bins' distances
partner centre - anchor centre in bp (whole numbers for an even W_partner - W_anchor, halves for an odd one, whose last bin is unused);
oriented int64 [rows][2][2 * max_dist + 1] (None with oriented=False): [0] partner on the anchor's strand, [1] on the opposite one, x
measured along the anchor's strand."""


def _rows(motifs, P):
    rows = np.arange(P)[motifs] if isinstance(motifs, slice) else np.asarray(motifs, dtype=np.int64).reshape(-1)
    if len(rows) and (rows.min() < 0 or rows.max() >= P):
        raise IndexError("motif index out of range")
    return rows


def _runs(rows):
    """(i, j) for every maximal run rows[i:j] of consecutive motif indices: one library call each."""
    i = 0
    while i < len(rows):
        j = i + 1
        while j < len(rows) and rows[j] == rows[j - 1] + 1:
            j += 1
        yield i, j
        i = j


def spacing_axis(max_dist, width_diff):
    """float64 [2 * max_dist + 1]: x[i] = (2 * i - 2 * max_dist + (width_diff & 1)) / 2, the distance partner centre - anchor centre of
    bin i in bp, for a partner width_diff = W_partner - W_anchor wider than the anchor."""
    return (2 * np.arange(2 * max_dist + 1) - 2 * max_dist + (int(width_diff) & 1)) / 2


def fold_orientations(counts, width_diff):
    """int64 [..., 2, n_bins] from the raw counts [..., 4, n_bins] of partners width_diff [...] wider than the anchor: the pairs of an
    anchor on '+' as they are ([0] '+/+', [1] '+/-'); those of an anchor on '-' seen from its own strand -- reflected, which negates the
    distance (the bin order is reversed within the bins in use: all n_bins for an even width_diff, n_bins - 1 for an odd one) and flips
    both strands ('-/-' joins [0], '-/+' joins [1])."""
    counts = np.asarray(counts)
    lead, n_bins = counts.shape[:-2], counts.shape[-1]
    odd = np.broadcast_to(np.asarray(width_diff, dtype=np.int64) & 1, lead).astype(bool).reshape(-1)
    flat = counts.reshape(-1, 4, n_bins)
    out = flat[:, :2, :].copy()
    minus = flat[:, :1:-1, :]                                    # orientations 3, 2
    out[~odd] += minus[~odd][:, :, ::-1]
    out[odd, :, :n_bins - 1] += minus[odd][:, :, :n_bins - 1][:, :, ::-1]
    return out.reshape(lead + (2, n_bins))


def cooccurrence(motif_sites, motifs=slice(None)):
    """int64 [len(motifs), P]: regions with a site of motif motifs[a] and a site of motif j (`motifs`: a slice or motif indices)."""
    res, _, owned = _device_sites(motif_sites)
    try:
        rows = _rows(motifs, res.n_pwms)
        out = np.zeros((len(rows), res.n_pwms), dtype=np.int64)
        for i, j in _runs(rows):
            res.cooccurrence(int(rows[i]), int(rows[j - 1]) + 1, out=out[i:j])
        return out
    finally:
        if owned:
            res.close()


def _pwmset(pwms):
    """(PwmSet, ours to close): a _lib.PwmSet as it is, else one made of the matrices (or of objects with a .matrix)."""
    if isinstance(pwms, _lib.PwmSet):
        return pwms, False
    return _lib.PwmSet.from_matrices([getattr(p, "matrix", p) for p in pwms]), True


def pair_spacing(motif_sites, pwms, anchor, max_dist=100, motifs=slice(None), oriented=True):
    """PairSpacing of the anchor motif against the partner motifs selected by `motifs` (a slice or motif indices); pwms: the scan's
    PWMs (their widths place the site centres) -- a _lib.PwmSet, matrices [4][W] or objects with a .matrix."""
    res, _, owned = _device_sites(motif_sites)
    pw, pw_owned = None, False
    try:
        pw, pw_owned = _pwmset(pwms)
        rows = _rows(motifs, res.n_pwms)
        anchor, max_dist = int(anchor), int(max_dist)
        if not len(rows):                                        # the library still checks the other arguments
            res.pair_spacing(pw, anchor, max_dist, 0, 0)
        parts = [res.pair_spacing(pw, anchor, max_dist, int(rows[i]), int(rows[j - 1]) + 1) for i, j in _runs(rows)]
        n_bins = 2 * max_dist + 1
        counts = np.concatenate([c for c, _ in parts]) if parts else np.zeros((0, 4, n_bins), dtype=np.int64)
        n_pairs = np.concatenate([n for _, n in parts]) if parts else np.zeros(0, dtype=np.int64)
        widths = np.asarray(pw.widths, dtype=np.int64)
        diff = widths[rows] - widths[anchor]
        x = np.stack([spacing_axis(max_dist, d) for d in diff]) if len(rows) else np.zeros((0, n_bins))
        return PairSpacing(counts, n_pairs, x, fold_orientations(counts, diff) if oriented else None)
    finally:
        if pw_owned:
            pw.close()
        if owned:
            res.close()
