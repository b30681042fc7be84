"""
motifscan_amd.affinity -- total binding affinity per (motif, region): the summed likelihood ratio over ALL windows (ms_scan_affinity).

The PWMs are natural-log odds (matrix.py), so a window's raw sum is its log likelihood ratio and exp(raw) its likelihood ratio.  TRAP,
Clover and PWMEnrich call the sum over a region's windows its total binding affinity or occupancy; it is AME's `avg` / `sum` scoring,
where the best window (ms_scan_best) is AME's `max` and the region counts are its `totalhits`.  It still sees a weak site repeated
five times, which the best window cannot.

The definition (include/motifscan_amd.h): the TERMS of a cell are the (window start, strand of the mask) pairs of the region, with
max_n >= 0 only the windows of at most max_n non-ACGT bases; raw(term) is the scan's raw window sum (scoredist.window_raw_sums);
    n_terms     the number of terms (raw = -inf terms count)
    peak        the greatest raw over the terms                                  NaN if n_terms == 0; may be -inf
    sum         S = sum of exp(scale * (raw - peak)); a raw of -inf adds 0       0 if peak is -inf or n_terms == 0
    log_mean    scale * peak + log(S / n_terms)                                  -inf if peak is -inf, NaN if n_terms == 0
A motif with a NaN or +inf entry has an empty row everywhere.  An all-negative matrix IS scored (ms_scan_best does not score it).

    AffinityArrays                        the four (P, R) planes; .log_sum(), .mean_odds()
    affinity_host(mats, seqs, ...)        the numpy restatement, two passes in float64 -- needs no GPU
    affinity_reference(mats, seqs, ...)   the same S with mpmath at >= 120 bits from the exact float64 raw sums
    check_args(scale, max_n)              what the bindings refuse before any library call
Scanner.affinity / Scanner.affinity_rank_sum run the device.
"""
import math

import numpy as np

from . import scoredist


class AffinityArrays:
    """(n_pwms, n_regions) arrays: peak (float64), sum (float64), n_terms (int32), log_mean (float64) -- the module's docstring."""
    __slots__ = ("peak", "sum", "n_terms", "log_mean")

    def __init__(self, peak, sum, n_terms, log_mean):
        self.peak, self.sum, self.n_terms, self.log_mean = peak, sum, n_terms, log_mean

    def log_sum(self):
        """log of the region's SUMMED likelihood ratio (the total binding affinity): log_mean + log(n_terms); NaN where no term."""
        with np.errstate(all="ignore"):
            return self.log_mean + np.log(np.where(self.n_terms > 0, self.n_terms, 1).astype(np.float64))

    def mean_odds(self):
        """The region's mean likelihood ratio exp(log_mean) (it overflows to inf where log_mean passes 709.78)."""
        with np.errstate(all="ignore"):
            return np.exp(self.log_mean)


def check_args(scale, max_n):
    """(scale as float, max_n as int), or ValueError: scale must be finite and > 0, max_n an integer >= -1."""
    try:
        s = float(scale)
    except (TypeError, ValueError):
        raise ValueError(f"scale must be a finite number > 0, got {scale!r}")
    if not (math.isfinite(s) and s > 0.0):
        raise ValueError(f"scale must be a finite number > 0, got {scale!r}")
    if isinstance(max_n, bool) or not isinstance(max_n, (int, np.integer)) or int(max_n) < -1 or int(max_n) >= 2 ** 31:
        raise ValueError(f"max_n must be an integer >= -1 (-1: every window), got {max_n!r}")
    return s, int(max_n)


def empty_row(mat):
    """The library's rule: a motif with an entry that is NaN or +inf has no term anywhere."""
    mat = np.asarray(mat, dtype=np.float64)
    return bool(np.any(np.isnan(mat)) or np.any(mat == np.inf))


def cell_terms(mat, seq, strand, max_n=-1, sums=None):
    """The raw sums of a cell's terms as one float64 array ('+' terms, then '-' terms; the order carries no meaning).
    sums: scoredist.window_raw_sums(mat, seq) made earlier, or None."""
    if strand not in (1, 2, 3):
        raise ValueError("invalid strand mask")
    fwd, rev, n_non = scoredist.window_raw_sums(mat, seq) if sums is None else sums
    keep = np.ones(len(fwd), dtype=bool) if max_n < 0 else n_non <= max_n
    parts = [r[keep] for s, r in ((1, fwd), (2, rev)) if strand & s]
    return np.concatenate(parts) if parts else np.zeros(0)


def _finish(peak, total, n_terms, scale):
    """log_mean from the three other planes, each operation rounded once."""
    with np.errstate(all="ignore"):
        lm = np.float64(scale) * peak + np.log(total / np.where(n_terms > 0, n_terms, 1).astype(np.float64))
    lm = np.where(np.isneginf(peak), -np.inf, lm)
    return np.where(n_terms == 0, np.nan, lm)


def _walk(mats, seqs, strand, scale, max_n, cell_sum):
    scale, max_n = check_args(scale, max_n)
    mats = [np.asarray(m, dtype=np.float64) for m in mats]
    P, R = len(mats), len(seqs)
    peak, n_terms = np.full((P, R), np.nan), np.zeros((P, R), dtype=np.int32)
    total = np.zeros((P, R), dtype=object)
    for m, mat in enumerate(mats):
        if empty_row(mat):
            continue
        for r, seq in enumerate(seqs):
            raw = cell_terms(mat, seq, strand, max_n)
            n_terms[m, r] = len(raw)
            if len(raw) == 0:
                continue
            peak[m, r] = raw.max()
            if peak[m, r] > -np.inf:
                total[m, r] = cell_sum(raw, peak[m, r], scale)
    return peak, total, n_terms, scale


def affinity_host(mats, seqs, strand, scale=1.0, max_n=-1):
    """ms_scan_affinity restated in numpy, for host tests and small inputs: mats a list of 4 x W matrices, seqs a list of str / bytes,
    strand the mask 1 / 2 / 3.  Two passes per cell: the peak, then the sum of exp(scale * (raw - peak)) in float64."""
    def cell_sum(raw, peak, scale):
        live = raw[raw > -np.inf]
        return float(np.exp(np.float64(scale) * (live - peak)).sum())
    peak, total, n_terms, scale = _walk(mats, seqs, strand, scale, max_n, cell_sum)
    total = total.astype(np.float64)
    return AffinityArrays(peak, total, n_terms, _finish(peak, total, n_terms, scale))


def affinity_reference(mats, seqs, strand, scale=1.0, max_n=-1, prec=160, as_mpf=False):
    """The same planes with S summed by mpmath at `prec` >= 120 bits from the exact float64 raw sums: scale * (raw - peak) is formed
    without rounding, a term below 2^-(prec + 16) of the peak's is below the working precision and left out.  `sum` is rounded to
    float64 once at the end, or with as_mpf an object array of mpmath numbers (0 where there is nothing to add)."""
    import mpmath
    if prec < 120:
        raise ValueError("prec must be >= 120 bits")
    ctx = mpmath.mp.clone()
    ctx.prec = int(prec)
    floor = -(prec + 16) * math.log(2.0)

    def cell_sum(raw, peak, scale):
        live = raw[raw > -np.inf]
        values, counts = np.unique(live, return_counts=True)
        s, pk, sc = ctx.mpf(0), ctx.mpf(float(peak)), ctx.mpf(scale)
        for v, k in zip(values.tolist(), counts.tolist()):
            if scale * (v - peak) < floor - 1.0:
                continue
            s += int(k) * ctx.exp(sc * (ctx.mpf(v) - pk))
        return s
    peak, total, n_terms, scale = _walk(mats, seqs, strand, scale, max_n, cell_sum)
    rounded = np.array([[float(x) for x in row] for row in total], dtype=np.float64).reshape(total.shape)
    out = AffinityArrays(peak, rounded, n_terms, _finish(peak, rounded, n_terms, scale))
    if as_mpf:
        out.sum = np.array([[ctx.mpf(x) for x in row] for row in total], dtype=object).reshape(total.shape)
    return out
