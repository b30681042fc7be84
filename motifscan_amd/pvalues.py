"""
motifscan_amd.pvalues -- analytic P-values: the distribution of a window's score from the matrix and a Markov background alone
(ms_pwmset_score_distribution, ms_scoredist.hip), and what follows from it: P-value bounds of a score and conservative score cutoffs,
without a genome to count.  build.py samples 10^6 windows and scoredist.exhaustive_cutoffs bins every window of a resident genome; both
answer "how often does this score occur in THIS sequence".  This module answers what FIMO, MOODS, HOMER and TFM-Pvalue answer: given a
matrix and a background model, the probability of every score.

    background_from_counts(kc, pseudocount=1.0) -> (cond, init)    the background of order k - 1 of a non-canonical kmers.KmerCounts
    restate_distribution(mats, cond, init, n_bins, strand)         the library's definition in numpy, byte for byte (tests, small inputs)
    score_distribution(matrices, cond, init, n_bins, strand)       the device call -> ScoreDistribution
    analytic_cutoffs(matrices, background, p_values)               per motif {p: cutoff}, in build.build_motif's format

The score grid (include/motifscan_amd.h has the definition): per motif a step; the entries quantised to q = floor(M / step); the integer
score S of a window is the sum of its q; mass[m][i] is the probability of S = s0[m] + i.  An entry of -inf drops the mass that would
pass through it: 1 - the row's sum is the probability of a score of -inf.

THE BRACKET between the scan's raw sum R of a window (fp64, the scan's order of adds) and its integer score S:
    step (S - 1) <= R <= step (S + W + 1)
(the real-number statement is step S <= R < step (S + W); the extra bin on each side absorbs the roundings; DESIGN.md section 4 has the
proof and its premise, ScoreDistribution.bracket_ok).  For a normalised score x = R / max_raw and j = floor(x max_raw / step):
    tail(j + 2) <= P(score >= x) <= tail(j - W - 1)
and a cutoff made from the lowest integer score i* whose tail is <= p, step (i* + W + 1) / max_raw rounded up, lets only windows of
S >= i* pass: the cutoffs are conservative.

Everything but score_distribution / analytic_cutoffs is numpy / plain Python floats and needs no GPU.
"""
from fractions import Fraction

import numpy as np

from . import _lib
from .scoredist import _fraction, _matrices, max_raw_of, scorable

MAX_ORDER, MAX_BINS = _lib.MS_SCOREDIST_MAX_ORDER, _lib.MS_SCOREDIST_MAX_BINS
_MAX_QUANT = 2.0 ** 52


def background_from_counts(kc, pseudocount=1.0):
    """(cond float64 [4^(k-1)][4], init float64 [4^(k-1)]) of a non-canonical kmers.KmerCounts of k = order + 1: cond is
    kc.markov(pseudocount), init each context's share of the pseudo-counted row sums (uniform where they are all zero).  k = 1 gives
    order 0: one context, init = [1.0]."""
    cond = kc.markov(pseudocount)
    if kc.k - 1 > MAX_ORDER:
        raise ValueError(f"a background of order {kc.k - 1}: the score distribution takes at most order {MAX_ORDER}")
    if kc.k == 1:
        return cond, np.ones(1, dtype=np.float64)
    rows = (kc.occ.reshape(-1, 4).astype(np.float64) + float(pseudocount)).sum(axis=1)
    tot = rows.sum()
    init = rows / tot if tot > 0 else np.full(rows.shape, 1.0 / rows.size)
    return cond, init


def quantise(mat, n_bins, strand=1):
    """The score grid of one motif: (step, s0, d) with d int64 [4][W] the shifts in the order the recurrence walks the columns under
    `strand` (-1: an absent entry), or None for an unscorable motif -- scoredist.scorable's rule, or a column without a finite entry.
    Python floats: one rounded operation each, columns in order.  ValueError where the fit assertion fails (the library:
    MS_ERR_INTERNAL)."""
    mat = np.asarray(mat, dtype=np.float64)
    W = mat.shape[1]
    if n_bins < W + 3:
        raise ValueError("n_bins must be at least the motif's width + 3")
    if not scorable(mat):
        return None
    hi = lo = 0.0
    for c in range(W):
        fin = [float(v) for v in mat[:, c] if v != -np.inf]
        if not fin:
            return None
        hi = hi + max(fin)
        lo = lo + min(fin)
    step = 1.0 if hi == lo else (hi - lo) / float(n_bins - W - 2)
    if not (np.isfinite(step) and step > 0.0):
        raise ValueError("the quantised scores do not fit (a range that is not a finite number > 0)")
    absent = mat == -np.inf
    with np.errstate(all="ignore"):
        t = np.floor(np.where(absent, 0.0, mat) / np.float64(step))
    if not np.all(np.abs(t) < _MAX_QUANT):
        raise ValueError("the quantised scores do not fit (entries too large against their range)")
    q = t.astype(np.int64)
    big = np.iinfo(np.int64).max
    qmin = np.where(absent, big, q).min(axis=0)
    qmax = np.where(absent, -big, q).max(axis=0)
    if int((qmax - qmin).sum()) >= n_bins:
        raise ValueError("the quantised scores do not fit n_bins")
    d = np.where(absent, -1, q - qmin[None, :])
    if strand == 2:
        d = d[::-1, ::-1]
    return float(step), int(sum(int(v) for v in qmin)), np.ascontiguousarray(d)


def _shifted(rows, s, n_bins):
    """rows [k][n_bins] moved up by s bins, +0.0 shifted in; all +0.0 for s < 0 (an absent entry)."""
    out = np.zeros_like(rows)
    if 0 <= s < n_bins:
        out[:, s:] = rows[:, :n_bins - s]
    return out


def restate_distribution(mats, cond, init, n_bins, strand=1):
    """ms_pwmset_score_distribution's definition in numpy: (mass float64 [P][n_bins], step float64 [P], s0 int64 [P]).  Every product and
    every sum is one elementwise float64 operation in the library's order -- ((t_A + t_C) + t_G) + t_T per element, the contexts of the
    last column added left to right in a loop, never numpy's own (pairwise) summation -- so the bytes equal the device's."""
    if strand not in (1, 2):
        raise ValueError("strand must be 1 (forward) or 2 (reverse)")
    cond = np.ascontiguousarray(cond, dtype=np.float64).reshape(-1, 4)
    init = np.ascontiguousarray(init, dtype=np.float64).reshape(-1)
    C = init.size
    order = {4 ** k: k for k in range(MAX_ORDER + 1)}.get(C)
    if order is None or cond.shape[0] != C:
        raise ValueError("init must hold 4^order entries, order <= MS_SCOREDIST_MAX_ORDER, and cond 4 per entry of init")
    if np.any(~np.isfinite(cond)) or np.any(cond < 0) or np.any(~np.isfinite(init)) or np.any(init < 0):
        raise ValueError("cond and init must be finite and >= 0")
    n_bins = int(n_bins)
    mats = [np.asarray(m, dtype=np.float64) for m in mats]
    if n_bins < max([m.shape[1] for m in mats], default=0) + 3 or n_bins > MAX_BINS:
        raise ValueError("n_bins outside [the widest motif + 3, MS_SCOREDIST_MAX_BINS]")
    mass = np.zeros((len(mats), n_bins), dtype=np.float64)
    step, s0 = np.zeros(len(mats), dtype=np.float64), np.zeros(len(mats), dtype=np.int64)
    quarter = C // 4
    for m, mat in enumerate(mats):
        g = quantise(mat, n_bins, strand)
        if g is None:
            continue
        step[m], s0[m], d = g
        old = np.zeros((C, n_bins), dtype=np.float64)
        old[:, 0] = init
        for c in range(mat.shape[1]):
            new = np.empty_like(old)
            if order == 0:
                t = [_shifted(old, int(d[b, c]), n_bins) * cond[0, b] for b in range(4)]
                new[:] = ((t[0] + t[1]) + t[2]) + t[3]
            else:
                for b in range(4):                       # the contexts x = 4 (x >> 2) + b: predecessors a * 4^(order - 1) + (x >> 2)
                    t = [_shifted(old[a * quarter:(a + 1) * quarter], int(d[b, c]), n_bins) * cond[a * quarter:(a + 1) * quarter, b][:, None]
                         for a in range(4)]
                    new[b::4] = ((t[0] + t[1]) + t[2]) + t[3]
            old = new
        row = old[0].copy()
        for x in range(1, C):
            row = row + old[x]
        mass[m] = row
    return mass, step, s0


class ScoreDistribution:
    """mass float64 [P][n_bins] (the probability of the integer score s0[m] + i), step [P], s0 [P], widths [P], max_raw [P].  step = 0
    marks an unscorable motif (an all-zero row).  Pure numpy."""

    def __init__(self, mass, step, s0, widths, max_raw, abs_sum=None):
        self.mass = np.asarray(mass, dtype=np.float64)
        self.n_bins = self.mass.shape[1]
        self.step = np.asarray(step, dtype=np.float64)
        self.s0 = np.asarray(s0, dtype=np.int64)
        self.widths = np.asarray(widths, dtype=np.int64)
        self.max_raw = np.asarray(max_raw, dtype=np.float64)
        # the premise of the bracket's proof: (W + 5) 2^-53 sum_c max_b |M[b][c]| < step
        self.abs_sum = None if abs_sum is None else np.asarray(abs_sum, dtype=np.float64)

    @classmethod
    def from_matrices(cls, mats, mass, step, s0):
        mats = [np.asarray(m, dtype=np.float64) for m in mats]
        abs_sum = [float(np.where(np.isfinite(m), np.abs(m), 0.0).max(axis=0).sum()) for m in mats]
        return cls(mass, step, s0, [m.shape[1] for m in mats], [max_raw_of(m) for m in mats], abs_sum)

    @property
    def bracket_ok(self):
        """bool [P]: the motif is scorable and the roundings the bracket absorbs are smaller than one step -- the premise of the proof."""
        if self.abs_sum is None:
            raise ValueError("made without the matrices (abs_sum): use ScoreDistribution.from_matrices")
        with np.errstate(all="ignore"):
            return (self.step > 0) & ((self.widths + 5) * 2.0 ** -53 * self.abs_sum < self.step)

    def lost(self, m):
        """1 - the row's sum: the probability that a window scores -inf (it passes through an entry of -inf)."""
        import math
        return 1.0 - math.fsum(self.mass[m].tolist())

    def tail(self, m):
        """float64 [n_bins + 1]: tail[i] = the probability of an integer score >= s0[m] + i, summed from the top (the small terms first);
        tail[n_bins] = 0."""
        out = np.zeros(self.n_bins + 1, dtype=np.float64)
        out[:self.n_bins] = np.cumsum(self.mass[m][::-1])[::-1]
        return out

    def _tail_at(self, m, scores_int):
        """tail of ABSOLUTE integer scores (any int64): everything at or below s0 gives tail[0], everything above the grid 0."""
        idx = np.clip(np.asarray(scores_int, dtype=np.int64) - self.s0[m], 0, self.n_bins)
        return self.tail(m)[idx]

    def p_value_bounds(self, m, scores):
        """(lower, upper) of P(score >= x) for normalised scores x (raw / max_raw, what the scan compares with a cutoff): with
        j = floor(x max_raw / step), tail(j + 2) <= P <= tail(j - W - 1).  NaN for an unscorable motif."""
        x = np.asarray(scores, dtype=np.float64)
        if not self.step[m] > 0:
            return np.full(x.shape, np.nan), np.full(x.shape, np.nan)
        j = np.floor(x * self.max_raw[m] / self.step[m]).astype(np.int64)
        return self._tail_at(m, j + 2), self._tail_at(m, j - int(self.widths[m]) - 1)

    def cutoff_index(self, m, p):
        """i*: the lowest grid index whose tail is <= p (exact comparison of the doubles with the P-value's decimal text); None where
        no score of positive probability has it."""
        f = _fraction(p)
        tail = self.tail(m)
        i = int(np.searchsorted(-tail, -float(f), side="left"))          # tail is non-increasing
        i = min(max(i, 0), self.n_bins)
        while i > 0 and Fraction(float(tail[i - 1])) <= f:
            i -= 1
        while i < self.n_bins and Fraction(float(tail[i])) > f:
            i += 1
        if i >= self.n_bins or tail[i] <= 0.0:
            return None
        return i

    def cutoffs(self, p_values):
        """Per motif a dict {p: cutoff}, in build.build_motif's format: step (s0 + i* + W + 1) / max_raw, one ulp up -- every window
        whose normalised score passes it has an integer score >= s0 + i*, so its P-value is <= p.  None for an unscorable motif and
        where no score of positive probability has a tail <= p."""
        p_values = list(p_values)
        out = []
        for m in range(self.mass.shape[0]):
            row = {}
            for p in p_values:
                i = self.cutoff_index(m, p) if self.step[m] > 0 else None
                if i is None:
                    row[p] = None
                    continue
                c = self.step[m] * float(int(self.s0[m]) + i + int(self.widths[m]) + 1) / self.max_raw[m]
                row[p] = float(np.nextafter(c, np.inf))
            out.append(row)
        return out


def score_distribution(matrices, cond, init, n_bins=65536, strand=3, timing=None):
    """The device call: a ScoreDistribution of the matrices (4 x W arrays or a MotifSet) under the background (cond, init).  strand: 1
    forward, 2 reverse, 3 the elementwise (forward + reverse) * 0.5 of two calls -- the distribution of a (window, strand) pair with
    the strand drawn evenly, which is what a two-strand scan compares with its cutoff.  step and s0 do not depend on the strand."""
    if strand not in (1, 2, 3):
        raise ValueError("invalid strand mask")
    init = np.ascontiguousarray(init, dtype=np.float64).reshape(-1)
    order = {4 ** k: k for k in range(MAX_ORDER + 1)}.get(init.size)
    if order is None:
        raise ValueError("init must hold 4^order entries, order <= MS_SCOREDIST_MAX_ORDER")
    pw, mats = _matrices(matrices)
    try:
        ms = 0.0
        parts = []
        for s in ((1, 2) if strand == 3 else (strand,)):
            t = {}
            parts.append(_lib.score_distribution(pw, s, order, cond, init, n_bins, timing=t))
            ms += t["device_ms"]
        if timing is not None:
            timing["device_ms"] = ms
        mass, step, s0 = parts[0]
        if strand == 3:
            mass = (mass + parts[1][0]) * 0.5
        return ScoreDistribution.from_matrices(mats, mass, step, s0)
    finally:
        pw.close()


def analytic_cutoffs(matrices, background, p_values=("1e-2", "1e-3", "1e-4", "1e-5", "1e-6"), n_bins=65536, strand=3):
    """Conservative score cutoffs without a genome: per motif {p: cutoff}, in build.build_motif's format (a MotifSet's `cutoffs[m]` takes
    it as exhaustive_cutoffs' output is taken).  background: (cond, init), or a non-canonical kmers.KmerCounts of k = order + 1."""
    cond, init = background_from_counts(background) if hasattr(background, "markov") else background
    return score_distribution(matrices, cond, init, n_bins, strand).cutoffs(p_values)
