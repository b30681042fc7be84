"""
motifscan_amd.scoredist -- the score distribution of every window of a region set or a genome (ms_scan_score_histogram), and what follows
from it: exhaustive score cutoffs, empirical P-values, the number of sites at any cutoff.

The reference builds its cutoffs from a SAMPLE (`motif --build`: 10^6 random windows scored by c_score, cscore.c:174-229, sorted and read
at the ranks int(n * 0.1**e) - 1, motif/__init__.py:378-401; motifscan_amd.build reproduces that).  Here every window is scored and
counted on the device, so a P-value reaches down to one over the number of windows and no seed is involved.

The bin rule (the library's definition, restated here with numpy's correctly rounded float64 operations):
    d = score - lo[m]            one rounded subtraction
    t = d * inv_width[m]         one rounded multiply
    t < 0        -> bin -1       ("below", a score of -inf included)        slot 0 of a counts row
    t >= n_bins  -> bin n_bins   ("above")                                  slot n_bins + 1
    otherwise    -> bin floor(t)                                            slot 1 + floor(t)
A counts row has n_bins + 2 slots; slot = bin + 1.

Everything in ScoreHistogram and restate_histogram is numpy / plain Python floats and needs no GPU; genome_histogram and
exhaustive_cutoffs run the device.
"""
from decimal import Decimal
from fractions import Fraction

import numpy as np

from . import _lib

_CODE = np.full(256, -1, dtype=np.int8)
for _i, _ch in enumerate("ACGT"):
    _CODE[ord(_ch)] = _CODE[ord(_ch.lower())] = _i


def _fraction(p):
    """A P-value given as a string ('1e-4') or a number, as the exact fraction its decimal text names."""
    return Fraction(Decimal(p if isinstance(p, str) else repr(float(p))))


def _keys(x):
    """float64 -> uint64 whose order is the doubles' order (-0.0 just below +0.0; no NaN)."""
    u = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
    return np.where(u >> np.uint64(63) != 0, ~u, u | np.uint64(1 << 63))


def _values(k):
    k = np.ascontiguousarray(k, dtype=np.uint64)
    return np.where(k >> np.uint64(63) != 0, k & np.uint64((1 << 63) - 1), ~k).view(np.float64)


def bin_rule(scores, lo, inv_width, n_bins):
    """The bin (-1 below, 0 .. n_bins - 1, n_bins above) of every score; lo / inv_width broadcast against scores."""
    with np.errstate(all="ignore"):
        d = np.asarray(scores, dtype=np.float64) - lo
        t = d * inv_width
        inside = np.floor(np.where((t >= 0) & (t < n_bins), t, 0.0)).astype(np.int64)
    return np.where(t < 0, -1, np.where(t >= n_bins, n_bins, inside))


def default_hi(lo=0.0, n_bins=1024):
    """The upper edge for scores in [lo, 1]: the least double above 1.0, widened (its distance to 1.0 doubled) until a score of exactly
    1.0 falls in the last bin, n_bins - 1, under the bin rule."""
    lo = float(lo)
    step = float(np.spacing(1.0))
    while True:
        hi = 1.0 + step
        inv = np.float64(n_bins) / np.float64(hi - lo)
        if int(bin_rule(1.0, lo, inv, n_bins)) == n_bins - 1:
            return hi
        step *= 2.0


class ScoreHistogram:
    """counts int64 [P][n_bins + 2] with its binning (lo [P], inv_width [P], n_bins).  Pure numpy."""

    def __init__(self, counts, lo, inv_width, n_bins):
        self.n_bins = int(n_bins)
        self.counts = np.asarray(counts, dtype=np.int64)
        P = self.counts.shape[0]
        self.lo = np.ascontiguousarray(np.broadcast_to(np.asarray(lo, dtype=np.float64), (P,)))
        self.inv_width = np.ascontiguousarray(np.broadcast_to(np.asarray(inv_width, dtype=np.float64), (P,)))
        if self.counts.ndim != 2 or self.counts.shape[1] != self.n_bins + 2:
            raise ValueError("counts must be (P, n_bins + 2)")

    @classmethod
    def from_range(cls, counts, lo, hi, n_bins):
        """With inv_width = n_bins / (hi - lo), as _lib.score_histogram computes it."""
        lo, inv_width = _lib.histogram_binning(np.asarray(counts).shape[0], lo, hi, n_bins)
        return cls(counts, lo, inv_width, n_bins)

    def same_binning(self, other):
        return (self.n_bins == other.n_bins and self.counts.shape == other.counts.shape and self.lo.tobytes() == other.lo.tobytes()
                and self.inv_width.tobytes() == other.inv_width.tobytes())

    def __add__(self, other):
        if not isinstance(other, ScoreHistogram):
            return NotImplemented
        if not self.same_binning(other):
            raise ValueError("histograms with different binning cannot be added")
        return ScoreHistogram(self.counts + other.counts, self.lo, self.inv_width, self.n_bins)

    @property
    def n_windows(self):
        """int64 [P]: the windows counted per motif (x the strands of the mask for a per-strand histogram)."""
        return self.counts.sum(axis=1)

    def bin_of(self, m, scores):
        """The bin of every score under motif m's binning: -1 below, 0 .. n_bins - 1, n_bins above (slot of the counts row = bin + 1)."""
        return bin_rule(scores, self.lo[m], self.inv_width[m], self.n_bins)

    def bin_floor(self, m, i):
        """The least double whose bin under motif m's binning is >= i (-inf for i <= -1; i <= n_bins), by bisection on the ordered bit
        patterns of the doubles with bin_of: bin_of(nextafter(c, -inf)) < i <= bin_of(c)."""
        scalar = np.ndim(i) == 0
        i = np.atleast_1d(np.asarray(i, dtype=np.int64))
        if np.any(i > self.n_bins):
            raise ValueError("no score has a bin above n_bins")
        a = np.broadcast_to(_keys(-np.inf), i.shape).copy()          # bin_of(a) < i unless i <= -1
        b = np.broadcast_to(_keys(np.inf), i.shape).copy()           # bin_of(b) = n_bins >= i
        while np.any(b - a > 1):
            mid = a + (b - a) // np.uint64(2)
            up = self.bin_of(m, _values(mid)) >= i
            b = np.where(up, mid, b)
            a = np.where(up, a, mid)
        out = np.where(i <= -1, -np.inf, _values(b))
        return float(out[0]) if scalar else out

    def tail(self, m):
        """int64 [n_bins + 2]: tail[s] = the windows of motif m counted in slot s and above (tail[0] = all of them)."""
        return np.cumsum(self.counts[m][::-1])[::-1]

    def p_value(self, m, scores):
        """(windows counted in the score's bin and above) / (windows counted): never below the true empirical P-value of the score (the
        share of windows that score at least as high), and equal to it where the score is its bin's floor.  NaN where no window was
        counted."""
        tail = self.tail(m)
        n = int(tail[0])
        slots = self.bin_of(m, scores) + 1
        with np.errstate(all="ignore"):
            out = tail[slots] / np.float64(n)
        return out

    def cutoff_slots(self, p_values):
        """int64 [P][len(p_values)]: the lowest slot whose tail / n is <= p (exact integer arithmetic on the P-value's decimal text);
        -1 where even the top slot exceeds p or no window was counted."""
        fr = [_fraction(p) for p in p_values]
        out = np.full((self.counts.shape[0], len(fr)), -1, dtype=np.int64)
        for m in range(self.counts.shape[0]):
            tail = self.tail(m)
            n = int(tail[0])
            if n == 0:
                continue
            for k, f in enumerate(fr):
                bound = (f.numerator * n) // f.denominator           # tail <= p n  <=>  tail <= floor(p n)
                ok = np.flatnonzero(tail <= bound)
                if len(ok):
                    out[m, k] = ok[0]                                 # (tail is non-increasing: the first is the lowest)
        return out

    def cutoffs(self, p_values):
        """Per motif a dict {p: cutoff}: bin_floor of the lowest bin whose tail / n is <= p -- the scores >= that cutoff are exactly the
        windows of that bin and above, so the empirical P-value of the cutoff is <= p.  None where even the top slot exceeds p (or no
        window was counted)."""
        p_values = list(p_values)
        slots = self.cutoff_slots(p_values)
        out = []
        for m in range(self.counts.shape[0]):
            have = slots[m] >= 0
            floors = self.bin_floor(m, np.where(have, slots[m] - 1, 0)) if len(p_values) else []
            out.append({p: (float(floors[k]) if have[k] else None) for k, p in enumerate(p_values)})
        return out


def scorable(mat):
    """The library's rule: max_raw (cscore.c:36-48) is a finite number > 0 and no entry is NaN or +inf."""
    mat = np.asarray(mat, dtype=np.float64)
    mr = max_raw_of(mat)
    return bool(np.isfinite(mr) and mr > 0 and not np.any(np.isnan(mat)) and not np.any(mat == np.inf))


def max_raw_of(mat):
    """get_max_raw_score (cscore.c:36-48) in Python floats, columns in order."""
    mr = 0.0
    for c in range(mat.shape[1]):
        col = 0.0
        for b in range(4):
            if mat[b, c] > col:
                col = float(mat[b, c])
        mr += col
    return mr


def least_score(mat):
    """A lower bound of every finite score of a scorable motif, a notch below the least one: the sum over the columns of
    min(0, the least finite entry) -- a non-ACGT base adds nothing -- over max_raw.  Where a full-range histogram starts."""
    mat = np.asarray(mat, dtype=np.float64)
    finite = np.where(np.isfinite(mat), mat, 0.0)
    low = float(np.minimum(finite.min(axis=0), 0.0).sum()) / max_raw_of(mat)
    return low * (1.0 + 1e-9) - 1e-300


def window_raw_sums(mat, seq):
    """(fwd, rev, n_non) of every window of one sequence (str / bytes): the raw sums in the scan's order of operations -- columns
    0 .. W - 1, forward M[b][c], reverse M[3 - b][W - 1 - c] at the same step, +0.0 for a non-ACGT base -- one float64 add per column,
    vectorised over the windows; n_non = the non-ACGT bases (anything but ACGTacgt) of the window."""
    mat = np.asarray(mat, dtype=np.float64)
    W = mat.shape[1]
    raw = np.frombuffer(seq.encode() if isinstance(seq, str) else bytes(seq), dtype=np.uint8)
    n = len(raw) - W + 1
    if n <= 0:
        return np.zeros(0), np.zeros(0), np.zeros(0, dtype=np.int64)
    code = _CODE[raw]
    fwd, rev, n_non = np.zeros(n), np.zeros(n), np.zeros(n, dtype=np.int64)
    with np.errstate(all="ignore"):
        for c in range(W):
            b = code[c:c + n]
            ok = b >= 0
            bb = np.where(ok, b, 0)
            fwd = fwd + np.where(ok, mat[bb, c], 0.0)
            rev = rev + np.where(ok, mat[3 - bb, W - 1 - c], 0.0)
            n_non += ~ok
    return fwd, rev, n_non


def raw_sums(mats, seqs):
    """window_raw_sums of every (motif, sequence), [P][R] nested lists: what restate_histogram takes as `sums` when several histograms
    of the same inputs are wanted (the sums do not depend on the strand mask, the binning or max_n)."""
    return [[window_raw_sums(mat, seq) for seq in seqs] for mat in mats]


def restate_histogram(mats, seqs, strand, lo, hi, n_bins, per_position=False, max_n=-1, sums=None):
    """ms_scan_score_histogram's definition in numpy / Python floats, for host tests and small inputs: int64 [P][n_bins + 2].
    sums: raw_sums(mats, seqs) made earlier, or None."""
    if strand not in (1, 2, 3):
        raise ValueError("invalid strand mask")
    mats = [np.asarray(m, dtype=np.float64) for m in mats]
    lo, inv_width = _lib.histogram_binning(len(mats), lo, hi, n_bins)
    out = np.zeros((len(mats), n_bins + 2), dtype=np.int64)
    for m, mat in enumerate(mats):
        if not scorable(mat):
            continue
        mr = np.float64(max_raw_of(mat))
        for r, seq in enumerate(seqs):
            fwd, rev, n_non = window_raw_sums(mat, seq) if sums is None else sums[m][r]
            keep = np.ones(len(fwd), dtype=bool) if max_n < 0 else n_non <= max_n
            if per_position:
                raws = [np.where(fwd > rev, fwd, rev) if strand == 3 else (fwd if strand == 1 else rev)]
            else:
                raws = [r for s, r in ((1, fwd), (2, rev)) if strand & s]
            for raw in raws:
                with np.errstate(all="ignore"):
                    score = raw[keep] / mr
                out[m] += np.bincount(bin_rule(score, lo[m], inv_width[m], n_bins) + 1, minlength=n_bins + 2)
    return out


def _matrices(matrices):
    """(PwmSet, list of 4 x W arrays) of a list of matrices or a matrix.MotifSet."""
    if hasattr(matrices, "flat") and hasattr(matrices, "widths"):
        vals, widths = matrices.flat()
        mats, o = [], 0
        for w in np.asarray(widths).tolist():
            mats.append(np.asarray(vals[o:o + 4 * w], dtype=np.float64).reshape(4, w))
            o += 4 * w
        return _lib.PwmSet(vals, widths, None), mats
    mats = [np.asarray(m, dtype=np.float64) for m in matrices]
    return _lib.PwmSet.from_matrices(mats), mats


def genome_histogram(resident, matrices, lo=0.0, hi=None, n_bins=1024, per_position=True, max_n=0, strand=3):
    """The score histogram of every window of a ResidentGenome: one region per chromosome (ResidentGenome.extract) and ONE device call.
    matrices: 4 x W arrays or a MotifSet.  hi=None: default_hi(lo, n_bins) for a scalar lo.  Returns a ScoreHistogram."""
    if hi is None:
        hi = default_hi(lo, n_bins)
    pw, _ = _matrices(matrices)
    try:
        sizes = [resident.chrom_sizes[n] for n in resident.names]
        sq = resident.extract(np.arange(len(sizes)), np.zeros(len(sizes), dtype=np.int64), sizes)
        try:
            counts = _lib.score_histogram(pw, sq, strand, lo, hi, n_bins, per_position, max_n)
        finally:
            sq.close()
        return ScoreHistogram.from_range(counts, lo, hi, n_bins)
    finally:
        pw.close()


def exhaustive_cutoffs(matrices, resident, p_values=("1e-2", "1e-3", "1e-4", "1e-5", "1e-6", "1e-7", "1e-8"), strand=3, max_n=0, passes=2,
                       n_bins=_lib.MS_SCOREHIST_MAX_BINS, details=None):
    """Score cutoffs from EVERY window of a resident genome: per motif a dict {p: cutoff}, in build.build_motif's format (a MotifSet's
    `cutoffs[m]` takes it as it is).

    This is NOT the reference's sampled cutoff (motif/__init__.py:378-401: the score at rank int(n * 0.1**e) - 1 of 10^6 random windows
    of the widest motif's length, averaged over repeats and rounded): it is the exhaustive form.  P-values are per POSITION, as c_score
    defines a position's score -- the greater of the two strands' raw sums over max_raw for strand=3 -- and a cutoff c has the defining
    property (windows scoring >= c) / (windows counted) <= p.  max_n drops windows by their OWN non-ACGT bases (every motif's own width,
    IUPAC letters included), not by the widest motif's window as the reference's sampler does.  The cutoffs are not rounded.

    Pass 1 counts every window into n_bins bins over [0, 1 + eps).  Pass 2 (one device call per P-value) zooms each (motif, P-value)
    into the bin that held the answer, n_bins bins again: the cutoff is then within (1 / n_bins^2) of the least score whose empirical
    P-value is <= p.  (A cutoff under 0 -- a motif most of whose windows score below 0 -- is zoomed into [the least possible score, 0).)  None for a motif without counted windows (an unscorable one, or a genome shorter than the motif).
    details: a dict that receives the histograms the cutoffs were read from, 'first' and 'second' ({p: ScoreHistogram})."""
    p_values = list(p_values)
    if passes not in (1, 2):
        raise ValueError("passes must be 1 or 2")
    pw, mats = _matrices(matrices)
    try:
        sizes = [resident.chrom_sizes[n] for n in resident.names]
        sq = resident.extract(np.arange(len(sizes)), np.zeros(len(sizes), dtype=np.int64), sizes)
        try:
            hi = default_hi(0.0, n_bins)
            first = ScoreHistogram.from_range(_lib.score_histogram(pw, sq, strand, 0.0, hi, n_bins, True, max_n), 0.0, hi, n_bins)
            out = first.cutoffs(p_values)
            if details is not None:
                details["first"], details["second"] = first, {}
            if passes == 1:
                return out
            slots = first.cutoff_slots(p_values)
            P = pw.n
            for k, p in enumerate(p_values):
                # the answer lies in slot s - 1 (its tail exceeds p n, slot s's does not): zoom into [floor(s - 1), floor(s)) where that
                # slot is a bin, and into [the least possible score, 0) where it is "below" (a motif most of whose windows score under 0);
                # a motif without counted windows keeps pass 1's None and is binned anywhere
                zoom = slots[:, k] >= 1
                lo2, hi2 = np.zeros(P), np.full(P, hi)
                for m in np.flatnonzero(zoom):
                    if slots[m, k] >= 2:
                        lo2[m], hi2[m] = first.bin_floor(m, np.array([slots[m, k] - 2, slots[m, k] - 1]))
                    else:
                        lo2[m], hi2[m] = least_score(mats[m]), first.bin_floor(m, 0)
                second = ScoreHistogram.from_range(_lib.score_histogram(pw, sq, strand, lo2, hi2, n_bins, True, max_n), lo2, hi2, n_bins)
                if details is not None:
                    details["second"][p] = second
                fine = second.cutoffs([p])
                for m in np.flatnonzero(zoom):
                    if fine[m][p] is not None:
                        out[m][p] = fine[m][p]
            return out
        finally:
            sq.close()
    finally:
        pw.close()
