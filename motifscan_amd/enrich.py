"""
motifscan_amd.enrich -- cutoff-free motif enrichment from best-site matrices (ms_best_rank_sum, ms_best_count_passing).

The device reduces two groups of regions to exact integers per motif; everything statistical is host arithmetic on them:

    RankSum(u2, ties, na, nb)       u2 = 2 #{x > y} + #{x == y} over x in group A, y in group B (twice the Mann-Whitney U of A),
                                    ties = sum over the pooled sample's tie groups of t^3 - t (Python ints: it passes 2^64)
        .auroc()                    u2 / (2 na nb)
        .z()                        (U - na nb / 2) / sqrt(na nb / 12 * (N + 1 - T / (N (N - 1)))), no continuity correction
        .p_value(alternative)       the normal approximation's tail, through math.erfc
    rank_sum_host(xa, xb)           the numpy restatement of ms_best_rank_sum's contract (include/motifscan_amd.h)
    count_passing_host(x, cutoffs)  ... and of ms_best_count_passing's
    rank_sum(best_a, best_b, ...)   the device calls on _lib.BestSites handles
    count_passing(best, cutoffs, ...)

Order of cell values: a cell without a winner (NaN) ranks below every number and ties with every other such cell; numbers compare as
IEEE doubles (-0.0 == +0.0, -inf is an ordinary number).
"""
import math

import numpy as np

_ALTERNATIVES = ("greater", "less", "two-sided")


def tie_sum(counts):
    """sum of t^3 - t over tie-group sizes, as an exact Python int (a group of 3 000 000 alone passes 2^64)."""
    return sum(int(t) ** 3 - int(t) for t in counts)


class RankSum:
    """The integers of one rank-sum comparison per motif: u2 (int64 array), ties (list of Python ints), na, nb."""
    __slots__ = ("u2", "ties", "na", "nb")

    def __init__(self, u2, ties, na, nb):
        self.u2 = np.atleast_1d(np.asarray(u2, dtype=np.int64))
        self.ties = [int(t) for t in (ties if np.ndim(ties) else [ties])]
        self.na, self.nb = int(na), int(nb)
        if len(self.ties) != len(self.u2):
            raise ValueError("u2 and ties must hold one entry per motif")

    def __len__(self):
        return len(self.u2)

    def auroc(self):
        """P(x > y) + P(x == y) / 2 per motif; NaN when a group is empty."""
        pairs = self.na * self.nb
        if pairs == 0:
            return np.full(len(self.u2), np.nan)
        return np.array([int(u) / (2 * pairs) for u in self.u2.tolist()], dtype=np.float64)

    def z(self):
        """The normal approximation's z of U = u2 / 2 with the tie-corrected variance, no continuity correction; NaN where the
        variance is 0 (an empty group, or every pooled value tied).  The difference U - mean and the variance's numerator are taken in
        integers, so nothing cancels in floating point."""
        na, nb = self.na, self.nb
        N = na + nb
        out = np.full(len(self.u2), np.nan)
        if na == 0 or nb == 0 or N < 2:
            return out
        den = 12 * N * (N - 1)
        for i, (u2, T) in enumerate(zip(self.u2.tolist(), self.ties)):
            num = na * nb * ((N + 1) * N * (N - 1) - T)          # variance = num / den, exactly
            if num > 0:
                out[i] = ((u2 - na * nb) / 2) / math.sqrt(num / den)
        return out

    def p_value(self, alternative="greater"):
        """'greater': group A scores higher than group B; 'less'; 'two-sided'.  NaN where z is."""
        if alternative not in _ALTERNATIVES:
            raise ValueError(f"alternative must be one of {_ALTERNATIVES}, got {alternative!r}")
        out = np.full(len(self.u2), np.nan)
        for i, z in enumerate(self.z().tolist()):
            if z != z:
                continue
            if alternative == "greater":
                out[i] = 0.5 * math.erfc(z / math.sqrt(2.0))
            elif alternative == "less":
                out[i] = 0.5 * math.erfc(-z / math.sqrt(2.0))
            else:
                out[i] = math.erfc(abs(z) / math.sqrt(2.0))
        return out


def _rows(x):
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 1:
        x = x.reshape(1, -1)
    if x.ndim != 2:
        raise ValueError("scores must be [n] or [rows][n]")
    return x


def rank_sum_host(xa, xb):
    """ms_best_rank_sum restated in numpy: xa [rows][na] and xb [rows][nb] best scores (NaN = no winner; 1-D = one row) -> RankSum.
    The numbers of each row are sorted and counted with searchsorted; the cells without a winner are counted apart: they lie below every
    number and tie with one another."""
    xa, xb = _rows(xa), _rows(xb)
    if xa.shape[0] != xb.shape[0]:
        raise ValueError("the two groups must hold the same motif rows")
    na, nb = xa.shape[1], xb.shape[1]
    u2, ties = [], []
    for a, b in zip(xa, xb):
        a_num, b_num = np.sort(a[~np.isnan(a)]), np.sort(b[~np.isnan(b)])
        a_nan, b_nan = na - len(a_num), nb - len(b_num)
        below = np.searchsorted(b_num, a_num, side="left")
        upto = np.searchsorted(b_num, a_num, side="right")
        greater = int(below.sum()) + len(a_num) * b_nan       # a number beats every smaller number and every cell without a winner
        equal = int((upto - below).sum()) + a_nan * b_nan
        u2.append(2 * greater + equal)
        _, groups = np.unique(np.concatenate([a_num, b_num]) + 0.0, return_counts=True)      # (+ 0.0: -0.0 and +0.0 are one value)
        ties.append(tie_sum(groups.tolist() + [a_nan + b_nan]))
    return RankSum(np.asarray(u2, dtype=np.int64), ties, na, nb)


def count_passing_host(x, cutoffs):
    """ms_best_count_passing restated in numpy: x [rows][n] best scores, cutoffs [rows][K] -> int64 [rows][K], the cells with
    score - cutoff >= -1e-10 (one rounded subtraction; a NaN never passes)."""
    x = _rows(x)
    cutoffs = np.asarray(cutoffs, dtype=np.float64)
    if cutoffs.ndim == 1:
        cutoffs = cutoffs.reshape(-1, 1)
    if cutoffs.ndim != 2 or cutoffs.shape[0] != x.shape[0]:
        raise ValueError("cutoffs must be [rows][K]")
    if not np.isfinite(cutoffs).all():
        raise ValueError("a cutoff is not finite")
    with np.errstate(invalid="ignore"):
        return (x[:, :, None] - cutoffs[:, None, :] >= -1e-10).sum(axis=1).astype(np.int64)


def rank_sum(best_a, best_b, sel_a=None, sel_b=None, m0=0, m1=None):
    """ms_best_rank_sum on two _lib.BestSites handles (they may be the same one) -> RankSum.  No matrix leaves the device."""
    return RankSum(*best_a.rank_sum(best_b, sel_a, sel_b, m0, m1))


def count_passing(best, cutoffs, sel=None, m0=0, m1=None):
    """ms_best_count_passing on a _lib.BestSites handle -> int64 [m1 - m0][K]."""
    return best.count_passing(cutoffs, sel, m0, m1)
