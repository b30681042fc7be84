"""
motifscan_amd.sitestack -- what the sites of a scan LOOK like, counted on the device from the hit arrays of a result and the packed
sequences they were found in (ms_sitestack.hip).  The reference has no counterpart: it hands back nested site lists, and the observed
count matrix of a motif's sites is then some 50 string slices per site in Python.

    site_base_counts(motif_sites, pwms, seqs, flank=0, motifs=slice(None), dinuc=False) -> SiteStack
        per motif and per column of the motif (with `flank` columns either side), in the MOTIF's orientation: how many sites have A, C,
        G, T there, a non-ACGT base, or nothing (the column lies outside the region); with dinuc=True also the counts of the 16 base
        pairs of adjacent columns (ms_result_site_base_counts).
    SiteStack.pfm(i)                  int64 [4][W], ready for matrix.PositionFrequencyMatrix -- the logo of the sites actually found,
                                      and the counting step of a matrix refinement (scan, count, to_ppm().to_pwm(), scan again)
    SiteStack.columns(i)              int64 [W + 2 * flank][6], the row trimmed to the motif's own columns
    SiteStack.information_content(i)  bits per column
    site_base_counts_host(...)        the same counts from ASCII strings in sequential Python: the definition, restated (tests)

`motif_sites` is what `plot` accepts: a `MotifSites` (while it still owns its device result that result is read in place, otherwise its
flat arrays are uploaded) or the reference's nested lists, whose sites carry genome coordinates: pass the regions' starts as
`seq_starts` then.  `seqs` holds the regions the sites were found in, in the same order: a `_lib.SeqSet` or a list of strings.  The
counts are sums over regions: the arrays of region shards add up.  There is no CPU path behind site_base_counts: without a device it
raises.
"""
from collections import namedtuple
from types import SimpleNamespace

import numpy as np

from . import _lib
from .pairs import _pwmset, _rows, _runs
from .plot import _device_sites
from .sites import MotifSites

_SiteStack = namedtuple("SiteStack", ["counts", "dinuc", "n_sites", "widths", "flank"])

_CODE = {"A": 0, "C": 1, "G": 2, "T": 3, "a": 0, "c": 1, "g": 2, "t": 3}


class SiteStack(_SiteStack):
    """counts int64 [rows][C][6], C = the scan's widest motif + 2 * flank: per column j of row i's motif (column flank + c is motif
    column c; columns from widths[i] + 2 * flank on are unused and zero) the sites with A, C, G, T there in the motif's orientation
    (slots 0 .. 3), with a non-ACGT base (4), and whose column lies outside the region (5); dinuc int64 [rows][C][16] or None:
    [j][4 * a + b] the sites with a at column j and b at column j + 1, both in slots 0 .. 3; n_sites int64 [rows]: the motif's sites
    -- every used column of counts sums to it; widths int64 [rows]; flank."""
    __slots__ = ()

    def columns(self, i):
        """int64 [W + 2 * flank][6]: row i trimmed to its motif's columns."""
        return self.counts[i, :int(self.widths[i]) + 2 * self.flank]

    def pfm(self, i):
        """int64 [4][W]: the observed count matrix of motif i's sites (A, C, G, T by motif column; sites with a non-ACGT base at a
        column are left out of that column)."""
        W = int(self.widths[i])
        return np.ascontiguousarray(self.counts[i, self.flank:self.flank + W, :4].T)

    def information_content(self, i, bg=None):
        """float64 [W + 2 * flank]: sum_b f_b * log2(f_b / bg_b) per column, f the frequencies of slots 0 .. 3 (a column without such a
        base: 0.0); bg: four background frequencies, uniform by default."""
        n = self.columns(i)[:, :4].astype(np.float64)
        bg = np.full(4, 0.25) if bg is None else np.asarray(bg, dtype=np.float64)
        tot = n.sum(axis=1, keepdims=True)
        f = np.divide(n, tot, out=np.zeros_like(n), where=tot > 0)
        term = np.zeros_like(f)
        np.log2(f / bg, out=term, where=f > 0)
        return (f * term).sum(axis=1)


def site_base_counts_host(motif_offsets, seq_idx, pos, strand, widths, sequences, flank, dinuc=False):
    """The definition of ms_result_site_base_counts restated over ASCII strings, one site and one column at a time: hit arrays in
    ms_result order (strand 1 '+', 2 '-'), widths [P], sequences [R] of str or bytes.  Returns a SiteStack over all P motifs."""
    widths = np.asarray(widths, dtype=np.int64)
    P, flank = len(widths), int(flank)
    if len(motif_offsets) != P + 1:
        raise ValueError("need motif_offsets[P + 1]")
    if not 0 <= flank <= 64:
        raise ValueError("flank must be in [0, 64]")
    C = (int(widths.max()) if P else 0) + 2 * flank
    counts = np.zeros((P, C, 6), dtype=np.int64)
    di = np.zeros((P, C, 16), dtype=np.int64) if dinuc else None
    n_sites = np.diff(np.asarray(motif_offsets, dtype=np.int64))
    seqs = [s.decode("latin-1") if isinstance(s, (bytes, bytearray)) else s for s in sequences]
    for m in range(P):
        W = int(widths[m])
        for k in range(int(motif_offsets[m]), int(motif_offsets[m + 1])):
            r, p, minus = int(seq_idx[k]), int(pos[k]), int(strand[k]) == 2
            if not 0 <= r < len(seqs):
                raise ValueError(f"hit {k}: region {r} outside [0, {len(seqs)})")
            s = seqs[r]
            if p < 0 or p + W > len(s):
                raise ValueError(f"hit {k}: the site does not lie inside its region")
            prev = 5
            for j in range(W + 2 * flank):
                q = p + W - 1 + flank - j if minus else p - flank + j
                if q < 0 or q >= len(s):
                    slot = 5
                else:
                    b = _CODE.get(s[q])
                    slot = 4 if b is None else 3 - b if minus else b
                counts[m, j, slot] += 1
                if dinuc and j and prev < 4 and slot < 4:
                    di[m, j - 1, 4 * prev + slot] += 1
                prev = slot
    return SiteStack(counts, di, n_sites, widths, flank)


def _shifted(motif_sites, seq_starts):
    """The reference's nested lists with the sites' starts made relative to their regions."""
    starts = np.asarray(seq_starts, dtype=np.int64)
    return [[[SimpleNamespace(start=s.start - int(starts[r]), score=s.score, strand=s.strand) for s in sites] for r, sites in enumerate(per)]
            for per in motif_sites]


def site_base_counts(motif_sites, pwms, seqs, flank=0, motifs=slice(None), dinuc=False, seq_starts=None):
    """SiteStack of the motifs selected by `motifs` (a slice or motif indices).  pwms: the scan's PWMs (their widths lay out the
    columns) -- a _lib.PwmSet, matrices [4][W] or objects with a .matrix; seqs: the scanned regions, a _lib.SeqSet or a list of strings;
    seq_starts: for nested lists only, the regions' starts in the coordinates the sites carry (default 0)."""
    if seq_starts is not None and not isinstance(motif_sites, MotifSites):
        motif_sites = _shifted(motif_sites, seq_starts)
    res, _, owned = _device_sites(motif_sites)
    pw, pw_owned, sq, sq_owned = None, False, None, False
    try:
        pw, pw_owned = _pwmset(pwms)
        if isinstance(seqs, _lib.SeqSet):
            sq = seqs
        else:
            sq, sq_owned = _lib.SeqSet.from_strings(seqs), True
        rows = _rows(motifs, res.n_pwms)
        flank = int(flank)
        if not len(rows):                                        # the library still checks the other arguments
            res.site_base_counts(pw, sq, flank, 0, 0, dinuc)
        parts = [res.site_base_counts(pw, sq, flank, int(rows[i]), int(rows[j - 1]) + 1, dinuc) for i, j in _runs(rows)]
        widths = np.asarray(pw.widths, dtype=np.int64)
        C = (int(widths.max()) if len(widths) else 0) + 2 * flank
        counts = np.concatenate([p[0] for p in parts]) if parts else np.zeros((0, C, 6), dtype=np.int64)
        di = None
        if dinuc:
            di = np.concatenate([p[1] for p in parts]) if parts else np.zeros((0, C, 16), dtype=np.int64)
        n_sites = np.concatenate([p[2] for p in parts]) if parts else np.zeros(0, dtype=np.int64)
        return SiteStack(counts, di, n_sites, widths[rows], flank)
    finally:
        if sq_owned:
            sq.close()
        if pw_owned:
            pw.close()
        if owned:
            res.close()
