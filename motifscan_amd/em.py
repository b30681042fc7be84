"""
motifscan_amd.em -- motif refinement without a cutoff: the E-step of expectation maximisation on the device
(ms_affinity_expected_counts), the M-step and the loop around them.

sitestack.py refines a matrix from the sites ABOVE A CUTOFF ("scan, count, to_ppm().to_pwm(), scan again"); a weak seed has no sensible
cutoff.  What MEME-style tools do instead: every window of every region adds to the counts with its posterior probability of being the
site.  That is also the derivative of the log affinity with respect to the matrix entries.

The definition (include/motifscan_amd.h holds it as the contract; the unit is U = 2^-32):
    terms      of cell (m, r): exactly ms_scan_affinity's -- window start 0 .. L - W, the strands of the mask, the max_n filter; raw sums
               x as scoredist.window_raw_sums forms them
    pi(m, r)   1 if prior_logit is +inf (OOPS: one site per region); 0 if n_terms == 0, log_mean == -inf or prior_logit == -inf;
               otherwise 1 / (1 + exp(-(log_mean + prior_logit))) -- the ZOOPS posterior that the region holds a site when a fraction
               gamma of the regions does, prior_logit = log(gamma / (1 - gamma))
    w(term)    for x > -inf: pi * exp(scale * (x - peak)) / sum, clamped to [0, 1] (a NaN to 1); q = (int64) rint(w * 2^32), half to
               even; q = 0 for x = -inf
    slots      the term adds q to one slot of every motif column c: '+' the base at pos + c, '-' the base at pos + W - 1 - c
               complemented; slots 0 .. 3 = A, C, G, T in the motif's orientation, slot 4 = a non-ACGT base
    counts[m][c][s], total[m] (the sum of q over all terms; every used column sums to it), n_regions[m] (regions with a term)

    ExpectedCounts                       counts, total, n_regions, widths; .pfm(i), .occupancy(i), .n_weight(i)
    expected_counts_host(...)            the numpy restatement over scoredist.window_raw_sums, with the `slack` of its rounding
    expected_counts_reference(...)       the same weights with mpmath at >= 120 bits, quantised the same way, and the real sums
    log_likelihood(aff_arrays, prior)    per motif, the ZOOPS log likelihood ratio of the regions from the affinity's planes
    m_step(expected, bg, pseudo)         the pfm -> the next natural-log-odds matrices
    refine(mats, seqs, ...)              the loop: scan_affinity, expected_counts, m_step, gamma <- occupancy
Scanner.expected_counts / Scanner.refine_motifs run it over a scanner's regions.

SLACK.  Device and numpy form w * 2^32 in float64 with the same operations, but their exp may differ: the argument of exp is <= 0 and
rounded twice (the subtraction, the multiplication), exp is within 1 ulp on both sides, pi and the divide add a few 2^-53 relative.
Together that is below 16 * 2^-53 * w, times 2^32 below 2^-17 units.  So the two can round a term differently only where w * 2^32 lies
within 2^-16 of an integer + 1/2, and then by one unit.  `slack` counts those terms per cell of `counts`; it is derived, not measured.
"""
import math

import numpy as np

from . import affinity, matrix, scoredist

UNIT = 2.0 ** -32
_TWO32 = 2.0 ** 32
BAND = 2.0 ** -16

_SLOT = np.full(256, 4, dtype=np.int64)
for _i, _b in enumerate("ACGT"):
    _SLOT[ord(_b)] = _SLOT[ord(_b.lower())] = _i


class ExpectedCounts:
    """counts int64 (P, C, 5), total int64 (P,), n_regions int64 (P,) in units of 2^-32, and the motifs' widths (P,): C is the column
    pitch (the widest motif of the set), the columns behind a motif's width are zero."""
    __slots__ = ("counts", "total", "n_regions", "widths")

    def __init__(self, counts, total, n_regions, widths):
        self.counts, self.total, self.n_regions = counts, total, n_regions
        self.widths = np.asarray(widths, dtype=np.int64)

    def __len__(self):
        return len(self.widths)

    def pfm(self, i):
        """float64 [4][W]: the expected number of sites with A, C, G, T under each column of motif i (counts[..., :4] * 2^-32)."""
        W = int(self.widths[i])
        return self.counts[i, :W, :4].T.astype(np.float64) * UNIT

    def n_weight(self, i):
        """float64 [W]: the weight under each column that stands on a non-ACGT base (slot 4)."""
        return self.counts[i, :int(self.widths[i]), 4].astype(np.float64) * UNIT

    def occupancy(self, i):
        """The expected number of sites per region that has a term: total * 2^-32 / n_regions (NaN without such a region)."""
        n = int(self.n_regions[i])
        return float(self.total[i]) * UNIT / n if n else math.nan


def prior_logit_of(gamma):
    """log(gamma / (1 - gamma)); gamma None or 1 gives +inf (OOPS), 0 gives -inf."""
    if gamma is None:
        return math.inf
    g = float(gamma)
    if not 0.0 <= g <= 1.0:
        raise ValueError(f"gamma must be in [0, 1], got {gamma!r}")
    if g == 1.0:
        return math.inf
    if g == 0.0:
        return -math.inf
    return math.log(g / (1.0 - g))


def _check_prior(prior_logit):
    p = float(prior_logit)
    if math.isnan(p):
        raise ValueError("prior_logit is NaN")
    return p


def responsibility(log_mean, n_terms, prior_logit):
    """pi of every cell (the module's docstring), float64 of the planes' shape."""
    prior = _check_prior(prior_logit)
    lm = np.asarray(log_mean, dtype=np.float64)
    if prior == math.inf:
        return np.ones(lm.shape)
    with np.errstate(all="ignore"):
        pi = 1.0 / (1.0 + np.exp(-(lm + np.float64(prior))))
    dead = (np.asarray(n_terms) == 0) | np.isneginf(lm)
    if prior == -math.inf:
        dead = np.ones(lm.shape, dtype=bool)
    return np.where(dead, 0.0, pi)


def _planes_of(planes, mats, seqs, strand, scale, max_n):
    if planes is None:
        a = affinity.affinity_host(mats, seqs, strand, scale, max_n)
        planes = (a.peak, a.sum, a.log_mean, a.n_terms)
    peak, total, log_mean, n_terms = (np.asarray(x) for x in planes)
    if not (peak.shape == total.shape == log_mean.shape == n_terms.shape == (len(mats), len(seqs))):
        raise ValueError("planes must be (peak, sum, log_mean, n_terms), each of shape (n_pwms, n_regions)")
    return peak, total, log_mean, n_terms


def _cell_terms(mat, seq, strand, max_n):
    """[(minus, pos int64 [n], x float64 [n])] of the strands of the mask: the cell's terms, and the slot of every base of seq."""
    fwd, rev, n_non = scoredist.window_raw_sums(mat, seq)
    keep = np.ones(len(fwd), dtype=bool) if max_n < 0 else n_non <= max_n
    pos = np.nonzero(keep)[0]
    raw = np.frombuffer(seq.encode() if isinstance(seq, str) else bytes(seq), dtype=np.uint8)
    return [(s == 2, pos, x[keep]) for s, x in ((1, fwd), (2, rev)) if strand & s], _SLOT[raw]


def _scatter(dst, W, minus, pos, slots, values):
    """values[i] under every motif column of the window at pos[i] into dst [C][5] (the orientation rule of the docstring)."""
    for c in range(W):
        s = slots[pos + (W - 1 - c if minus else c)]
        if minus:
            s = np.where(s < 4, 3 - s, 4)
        np.add.at(dst[c], s, values)


def _walk(mats, seqs, strand, scale, max_n, prior_logit, planes, cell):
    if strand not in (1, 2, 3):
        raise ValueError("invalid strand mask")
    scale, max_n = affinity.check_args(scale, max_n)
    prior = _check_prior(prior_logit)
    mats = [np.asarray(m, dtype=np.float64) for m in mats]
    seqs = list(seqs)
    peak, total, log_mean, n_terms = _planes_of(planes, mats, seqs, strand, scale, max_n)
    pi = responsibility(log_mean, n_terms, prior)
    for m, mat in enumerate(mats):
        if affinity.empty_row(mat):
            continue
        W = mat.shape[1]
        for r, seq in enumerate(seqs):
            if n_terms[m, r] == 0:
                continue
            terms, slots = _cell_terms(mat, seq, strand, max_n)
            for minus, pos, x in terms:
                live = x > -np.inf
                if live.any():
                    cell(m, W, minus, pos[live], slots, x[live], float(peak[m, r]), float(total[m, r]), float(log_mean[m, r]), float(pi[m, r]), scale, prior)
    widths = [m.shape[1] for m in mats]
    n_regions = (n_terms > 0).sum(axis=1).astype(np.int64)
    for m, mat in enumerate(mats):
        if affinity.empty_row(mat):
            n_regions[m] = 0
    return widths, n_regions


def _pitch(mats):
    return max([np.asarray(m).shape[1] for m in mats], default=0)


def expected_counts_host(mats, seqs, strand, scale=1.0, max_n=-1, prior_logit=math.inf, planes=None):
    """ms_affinity_expected_counts restated in numpy: (ExpectedCounts, slack).  mats: a list of 4 x W matrices; seqs: a list of str /
    bytes; planes: (peak, sum, log_mean, n_terms) of the cells, each (P, R) -- the device's own, so that only the second pass is
    compared -- or None for affinity.affinity_host's.  slack int64 (P, C, 5): the terms under that cell of `counts` whose w * 2^32,
    formed in float64, lies within 2^-16 of an integer + 1/2 (the module's docstring: only there may device and numpy differ, by 1)."""
    P, C = len(mats), _pitch(mats)
    counts, slack = np.zeros((P, C, 5), dtype=np.int64), np.zeros((P, C, 5), dtype=np.int64)
    total = np.zeros(P, dtype=np.int64)

    def cell(m, W, minus, pos, slots, x, peak, total_cell, log_mean, pi, scale, prior):
        with np.errstate(all="ignore"):
            v = np.float64(pi) * np.exp(np.float64(scale) * (x - np.float64(peak))) / np.float64(total_cell)
        w = np.where(v < 1.0, np.where(v > 0.0, v, 0.0), 1.0)
        y = w * _TWO32
        q = np.rint(y).astype(np.int64)
        near = (np.abs(y - np.floor(y) - 0.5) <= BAND).astype(np.int64)
        total[m] += int(q.sum())
        _scatter(counts[m], W, minus, pos, slots, q)
        _scatter(slack[m], W, minus, pos, slots, near)

    widths, n_regions = _walk(mats, seqs, strand, scale, max_n, prior_logit, planes, cell)
    return ExpectedCounts(counts, total, n_regions, widths), slack


def expected_counts_reference(mats, seqs, strand, scale=1.0, max_n=-1, prior_logit=math.inf, planes=None, prec=160):
    """The same weights with mpmath at `prec` >= 120 bits from the float64 raw sums and planes -- pi, the exponential and the division
    without float64 rounding -- quantised the same way: (ExpectedCounts, real, n_contrib).  real (P, C, 5), an object array of mpmath
    numbers: the UNQUANTISED sums of w * 2^32; n_contrib int64 (P, C, 5): the terms of x > -inf and pi > 0 that add under the cell, so
    that |counts - real| <= n_contrib / 2 here, and n_contrib * (1/2 + 2^-16) bounds a float64 implementation."""
    import mpmath
    if prec < 120:
        raise ValueError("prec must be >= 120 bits")
    ctx = mpmath.mp.clone()
    ctx.prec = int(prec)
    P, C = len(mats), _pitch(mats)
    counts, n_contrib = np.zeros((P, C, 5), dtype=np.int64), np.zeros((P, C, 5), dtype=np.int64)
    real = np.empty((P, C, 5), dtype=object)
    real.fill(ctx.mpf(0))
    total = np.zeros(P, dtype=np.int64)
    two32, half = ctx.mpf(2) ** 32, ctx.mpf(1) / 2

    def quantise(y):
        f = ctx.floor(y)
        d = y - f
        n = int(f)
        return n + 1 if d > half else n if d < half else n + (n & 1)

    def cell(m, W, minus, pos, slots, x, peak, total_cell, log_mean, pi, scale, prior):
        if pi == 0.0:
            return
        pi_mp = ctx.mpf(1) if prior == math.inf else 1 / (1 + ctx.exp(-(ctx.mpf(log_mean) + ctx.mpf(prior))))
        values, inverse = np.unique(x, return_inverse=True)
        ys = []
        for v in values.tolist():
            w = pi_mp * ctx.exp(ctx.mpf(scale) * (ctx.mpf(v) - ctx.mpf(peak))) / ctx.mpf(total_cell)
            ys.append(min(max(w, ctx.mpf(0)), ctx.mpf(1)) * two32)
        q = np.array([quantise(y) for y in ys], dtype=np.int64)[inverse]
        total[m] += int(q.sum())
        _scatter(counts[m], W, minus, pos, slots, q)
        _scatter(n_contrib[m], W, minus, pos, slots, np.ones(len(pos), dtype=np.int64))
        y_obj = np.array(ys + [None], dtype=object)[:-1][inverse]
        _scatter(real[m], W, minus, pos, slots, y_obj)

    widths, n_regions = _walk(mats, seqs, strand, scale, max_n, prior_logit, planes, cell)
    return ExpectedCounts(counts, total, n_regions, widths), real, n_contrib


def log_likelihood(aff_arrays, prior_logit):
    """float64 [P]: per motif the sum over the regions with a term of logaddexp(log(1 - gamma), log(gamma) + log_mean), the ZOOPS log
    likelihood ratio of the regions against background, from the planes of an affinity.AffinityArrays (or anything with .log_mean and
    .n_terms).  On the host: a device-side reduction is not part of the library."""
    prior = _check_prior(prior_logit)
    lm = np.asarray(aff_arrays.log_mean, dtype=np.float64)
    has = np.asarray(aff_arrays.n_terms) > 0
    with np.errstate(all="ignore"):
        log_g = -np.logaddexp(0.0, -prior) if prior != math.inf else 0.0              # log gamma
        log_1g = -np.logaddexp(0.0, prior) if prior != math.inf else -math.inf         # log (1 - gamma)
        cell = np.logaddexp(log_1g, log_g + np.where(has, lm, -np.inf))
    return np.where(has, cell, 0.0).sum(axis=1)


def _bg_vector(bg):
    if bg is None:
        return np.full(4, 0.25)
    v = np.array([bg[b] for b in matrix.BASES] if isinstance(bg, dict) else bg, dtype=np.float64)
    if v.shape != (4,) or not np.all(v > 0) or not np.all(np.isfinite(v)):
        raise ValueError("bg must hold four positive frequencies (A, C, G, T)")
    return v / v.sum()


def m_step(expected, bg=None, pseudo=0.01, scale=1.0):
    """The next matrices from an ExpectedCounts: a list of float64 4 x W log-odds matrices, natural log divided by `scale` (so that
    scale * raw stays the log likelihood ratio).  Per column: the pfm goes through matrix.columns_to_ppm(normalize=False) -- a plain
    division by the column's sum, which fits -- then every column is smoothed with the background, (ppm + pseudo * bg) / (1 + pseudo),
    and the log-odds are log(ppm / bg).  matrix.py's other rules do NOT fit here and are not used: pseudo_normalize lifts only columns
    that hold an exact 0 (a posterior-weighted count is almost never exactly 0, so a base of weight 1e-9 would keep a log-odds of -20),
    and columns_to_pwm rounds to 5 decimals as the reference does for its files, which would make the loop's likelihood trace jitter.
    The weight on non-ACGT bases (slot 4) is left out.  A motif without any weight gets the background (all zeros)."""
    if not 0.0 < float(pseudo) < 1.0:
        raise ValueError("pseudo must be in (0, 1)")
    b = _bg_vector(bg)
    out = []
    for i in range(len(expected)):
        pfm = expected.pfm(i)
        col = pfm.sum(axis=0)
        with np.errstate(all="ignore"):
            ppm = np.where(col > 0, matrix.columns_to_ppm(pfm, normalize=False), b[:, None])
        ppm = (ppm + float(pseudo) * b[:, None]) / (1.0 + float(pseudo))
        out.append(np.log(ppm / b[:, None]) / float(scale))
    return out


class Refinement:
    """What refine returns: mats (the final matrices), gammas float64 [iters + 1][P] (the value each iteration ran with, and the last
    update), log_likelihood float64 [iters][P] (of the matrices each iteration STARTED with), and with keep=True `steps`: per
    iteration dict(mats, gamma, planes, expected) -- planes is a list of P tuples (peak, sum, log_mean, n_terms), each (1, R)."""
    __slots__ = ("mats", "gammas", "log_likelihood", "steps")

    def __init__(self, mats, gammas, log_likelihood, steps):
        self.mats, self.gammas, self.log_likelihood, self.steps = mats, gammas, log_likelihood, steps


def check_gamma(gamma, n_pwms):
    """refine's starting gamma as float64 [n_pwms] (a scalar is broadcast; None, OOPS, gives ones), or ValueError."""
    if gamma is None:
        return np.ones(n_pwms)
    g = np.broadcast_to(np.asarray(gamma, dtype=np.float64), (n_pwms,)).copy()
    if not np.all((g > 0) & (g < 1)):
        raise ValueError("gamma must lie strictly between 0 and 1 (None: one site per region)")
    return g


def refine(mats, seqs, iters=10, gamma=0.5, update_gamma=True, strand=3, scale=1.0, max_n=-1, bg=None, pseudo=0.01, device=True, keep=False):
    """Expectation maximisation of every matrix of `mats` on its own (ZOOPS; gamma=None: OOPS) over the regions `seqs` (a list of str,
    or with device=True a _lib.SeqSet): per iteration scan_affinity, expected_counts, m_step, and with update_gamma gamma <- the
    occupancy clipped to [1e-4, 1 - 1e-4].  Every motif runs with its own gamma, so the expected counts are asked for one motif row at
    a time (a row's bytes do not depend on the range).  device=False runs the same loop over affinity_host and expected_counts_host.
    Which known motif a refined matrix resembles: compare.compare (the matrices as a 'ppm' MotifSet against a library)."""
    if strand not in (1, 2, 3):
        raise ValueError("invalid strand mask")
    scale, max_n = affinity.check_args(scale, max_n)
    iters = int(iters)
    if iters < 1:
        raise ValueError("iters must be >= 1")
    mats = [np.array(m, dtype=np.float64) for m in mats]
    P = len(mats)
    oops = gamma is None
    g = check_gamma(gamma, P)
    gammas, trace, steps = [g.copy()], [], []
    sq = own = None
    if device:
        from . import _lib
        sq = seqs if isinstance(seqs, _lib.SeqSet) else _lib.SeqSet.from_strings(list(seqs))
        own = None if sq is seqs else sq
    else:
        seqs = list(seqs)
    try:
        for _ in range(iters):
            priors = [math.inf if oops else prior_logit_of(x) for x in g.tolist()]
            if device:
                pw = _lib.PwmSet.from_matrices(mats)
                try:
                    res = _lib.scan_affinity(pw, sq, strand, scale, max_n)
                    try:
                        peak, total, n_terms, log_mean = res.cells()
                        rows = [res.expected_counts(pw, sq, priors[i], slice(i, i + 1)) for i in range(P)]
                    finally:
                        res.close()
                finally:
                    pw.close()
                C = _pitch(mats)
                exp = ExpectedCounts(np.concatenate([r[0] for r in rows]).reshape(P, C, 5), np.concatenate([r[1] for r in rows]),
                                     np.concatenate([r[2] for r in rows]), [m.shape[1] for m in mats])
            else:
                a = affinity.affinity_host(mats, seqs, strand, scale, max_n)
                peak, total, n_terms, log_mean = a.peak, a.sum, a.n_terms, a.log_mean
                rows = [expected_counts_host([mats[i]], seqs, strand, scale, max_n, priors[i],
                                             planes=(peak[i:i + 1], total[i:i + 1], log_mean[i:i + 1], n_terms[i:i + 1]))[0] for i in range(P)]
                C = _pitch(mats)
                counts = np.zeros((P, C, 5), dtype=np.int64)
                for i, e in enumerate(rows):
                    counts[i, :e.counts.shape[1]] = e.counts[0]
                exp = ExpectedCounts(counts, np.array([e.total[0] for e in rows], dtype=np.int64),
                                     np.array([e.n_regions[0] for e in rows], dtype=np.int64), [m.shape[1] for m in mats])
            trace.append(np.array([log_likelihood(affinity.AffinityArrays(peak[i:i + 1], total[i:i + 1], n_terms[i:i + 1], log_mean[i:i + 1]), priors[i])[0]
                                   for i in range(P)]))
            if keep:
                steps.append(dict(mats=[m.copy() for m in mats], gamma=g.copy(), expected=exp,
                                  planes=[(peak[i:i + 1], total[i:i + 1], log_mean[i:i + 1], n_terms[i:i + 1]) for i in range(P)]))
            mats = m_step(exp, bg, pseudo, scale)
            if update_gamma and not oops:
                occ = np.array([exp.occupancy(i) for i in range(P)])
                g = np.where(np.isnan(occ), g, np.clip(occ, 1e-4, 1.0 - 1e-4))
            gammas.append(g.copy())
    finally:
        if own is not None:
            own.close()
    return Refinement(mats, np.array(gammas), np.array(trace).reshape(iters, P), steps if keep else None)
