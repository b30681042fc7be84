"""
motifscan_amd.compare -- motif sets compared with each other on the device (ms_motifs_compare, ms_compare.hip): which known motif does a
matrix resemble, at which offset and in which orientation, and which motifs of a library are near-duplicates of each other.  The procedure
is Tomtom's (Gupta, Stamatoyannopoulos, Bailey, Noble: Quantifying similarity between motifs, Genome Biology 2007): every ungapped
alignment of two matrices is scored column against column, the alignment score becomes a P-value under a null built from the target
set's own columns, the best alignment is kept and corrected for the number of alignments tried.  include/motifscan_amd.h fixes the
definition operation by operation; the device call returns, per (query, target) pair, the least table P-value `p_min` with its
`offset`, `overlap`, `score` and `orient`, and the number of alignments tried, `n_offsets`.  Everything behind that is host arithmetic.

    compare(queries, targets, metric, bins, min_overlap, both, q_block)    the device call -> Comparison
    Comparison.p_value() / e_value() / q_value()                           1 - (1 - p_min)^n_offsets; x targets; Benjamini-Hochberg per query
    Comparison.best(k)                                                     per query the k best targets with offset, orientation, overlap
    Comparison.groups(threshold)                                           redundancy classes of a set compared with itself
    restate_null / restate_compare                                         the definition in numpy, in the definition's order of operations
    prepare / grid / column_scores / table_doubles / table_offset          its parts, as the tests use them

An offset o puts target column j under query column j + o: o > 0, the target begins o columns into the query; o < 0, the query begins -o
columns into the target.  orient 1: the target is reverse-complemented.

Everything but `compare` is numpy / plain Python and needs no GPU.
"""
import numpy as np

from . import _lib

METRICS = {"pearson": _lib.MS_COMPARE_PEARSON, "sw": _lib.MS_COMPARE_SW, "ed": _lib.MS_COMPARE_ED}


def _metric(metric):
    if metric in METRICS:
        return METRICS[metric]
    if metric in METRICS.values():
        return int(metric)
    raise ValueError(f"metric must be one of {sorted(METRICS)}")


# ------------------------------------------------------------------------------------------------ the definition, in numpy

def prepare(matrix, metric):
    """float64 [W][4]: the columns of one [4][W] matrix as the device sees them.  pearson: the centred column over its norm (all +0.0
    where the norm is not > 0), each step one rounded operation in the header's order; sw, ed: the column itself."""
    x = np.ascontiguousarray(np.asarray(matrix, dtype=np.float64).T)
    if _metric(metric) != _lib.MS_COMPARE_PEARSON:
        return x
    mean = (((x[:, 0] + x[:, 1]) + x[:, 2]) + x[:, 3]) * 0.25
    c = x - mean[:, None]
    n = np.sqrt(((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2]) + c[:, 3] * c[:, 3])
    ok = n > 0.0
    with np.errstate(all="ignore"):
        u = c / n[:, None]
    return np.where(ok[:, None], u, 0.0)


def grid(metric, bins):
    """(lo, scale) of the integer score k = floor((g - lo) * scale) of a metric."""
    m = _metric(metric)
    if m == _lib.MS_COMPARE_ED:
        return -np.sqrt(2.0), np.float64(bins) / np.sqrt(2.0)
    return (-1.0 if m == _lib.MS_COMPARE_PEARSON else 0.0), np.float64(bins) * 0.5


def column_scores(U, V, metric, bins):
    """int32 [n][m]: the integer score of every prepared vector of U [n][4] against every one of V [m][4]."""
    m = _metric(metric)
    u = [U[:, b][:, None] for b in range(4)]
    v = [V[:, b][None, :] for b in range(4)]
    with np.errstate(all="ignore"):
        if m == _lib.MS_COMPARE_PEARSON:
            g = ((u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]) + u[3] * v[3]
        else:
            d = [u[b] - v[b] for b in range(4)]
            ssd = ((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) + d[3] * d[3]
            g = 2.0 - ssd if m == _lib.MS_COMPARE_SW else -np.sqrt(ssd)
        lo, scale = grid(m, bins)
        t = np.floor((g - lo) * scale)
        k = np.where(t >= 0.0, np.minimum(t, bins - 1), 0.0)             # a NaN gives 0, as on the device
    return k.astype(np.int32)


def tables_upto(n, bins):
    """Entries of the tables of the lengths 1 .. n of one start: (bins - 1) n (n + 1) / 2 + n."""
    return (bins - 1) * n * (n + 1) // 2 + n


def table_offset(W, bins, a, L):
    """Where table (a, L) of a query of width W begins in its flat tables ((a ascending, L ascending) order)."""
    return sum(tables_upto(W - b, bins) for b in range(a)) + tables_upto(L - 1, bins)


def table_doubles(W, bins):
    """Doubles of all tables of a query of width W: 8 of these bytes is what a query takes of the work budget."""
    return table_offset(W, bins, W, 1)


def _check(bins, min_overlap=1):
    if not 2 <= int(bins) <= _lib.MS_COMPARE_MAX_BINS:
        raise ValueError(f"bins must be in [2, {_lib.MS_COMPARE_MAX_BINS}]")
    if int(min_overlap) < 1:
        raise ValueError("min_overlap must be >= 1")


def _matrices(mats):
    out = [np.asarray(m, dtype=np.float64) for m in mats]
    for m in out:
        if m.ndim != 2 or m.shape[0] != 4 or not 1 <= m.shape[1] <= _lib.MS_COMPARE_MAX_WIDTH:
            raise ValueError(f"each matrix must be [4][W] with W in [1, {_lib.MS_COMPARE_MAX_WIDTH}]")
        if not np.isfinite(m).all():
            raise ValueError("a matrix entry is not finite")
    return out


class _Targets:
    """The prepared target set: all vectors side by side, and the first column of every target."""

    def __init__(self, mats, metric):
        self.widths = np.array([m.shape[1] for m in mats], dtype=np.int64)
        self.first = np.concatenate([[0], np.cumsum(self.widths)])
        self.vectors = np.concatenate([prepare(m, metric) for m in mats]) if mats else np.zeros((0, 4))


def _null(U, tg, metric, bins, both):
    """Of one prepared query U [W][4] against the target set: (H uint32 [W][bins], tail float64 flat, Kf, Kr) -- Kf / Kr int32
    [W][target columns], the scores against every forward column and against its reversed form."""
    W = len(U)
    Kf = column_scores(U, tg.vectors, metric, bins)
    Kr = column_scores(U, tg.vectors[:, ::-1], metric, bins) if both else None
    H = np.zeros((W, bins), dtype=np.int64)
    for i in range(W):
        H[i] = np.bincount(Kf[i], minlength=bins)
        if both:
            H[i] += np.bincount(Kr[i], minlength=bins)
    N = (2 if both else 1) * len(tg.vectors)
    f = H.astype(np.float64) * (1.0 / np.float64(N))
    # pm of every length: pm[L] is [W - L + 1][L (bins - 1) + 1], one row per start a.  The k-loop runs over all starts of one L at a
    # time: at step k every element that has a term for this k gets it added -- per element the terms arrive in ascending k from +0.0,
    # and an element without a term for a k is not touched.
    pm = {1: f.copy()}
    for L in range(2, W + 1):
        prev = pm[L - 1][:W - L + 1]
        last = f[L - 1:]                                                 # f of column a + L - 1, per start a
        plen = prev.shape[1]
        acc = np.zeros((W - L + 1, L * (bins - 1) + 1))
        for k in range(bins):
            acc[:, k:k + plen] = acc[:, k:k + plen] + prev * last[:, k:k + 1]
        pm[L] = acc
    # tail: from the top down, sequentially (an accumulate is sequential; a pairwise sum would not be the definition)
    tails = {L: np.add.accumulate(p[:, ::-1], axis=1)[:, ::-1] for L, p in pm.items()}
    flat = np.concatenate([tails[L][a] for a in range(W) for L in range(1, W - a + 1)])
    return H.astype(np.uint32), flat, Kf, Kr


def restate_null(query, targets, metric="pearson", bins=100, both=True):
    """The null of one query matrix against a target set, in the definition's order: (H uint32 [Wq][bins], tail float64 flat -- every
    table in (a ascending, L ascending) order, table_offset gives their places)."""
    _check(bins)
    (q,), t = _matrices([query]), _matrices(targets)
    if not t:
        raise ValueError("a null needs at least one target")
    H, flat, _, _ = _null(prepare(q, metric), _Targets(t, metric), _metric(metric), int(bins), bool(both))
    return H, flat


_DIAG = {}


def _diagonals(Wq, Wt):
    """Per (Wq, Wt): the cell -> diagonal index (i - j + Wt - 1, i.e. o + Wt - 1) and per offset o its a, L."""
    key = (Wq, Wt)
    if key not in _DIAG:
        i, j = np.meshgrid(np.arange(Wq), np.arange(Wt), indexing="ij")
        o = np.arange(-(Wt - 1), Wq)
        a = np.maximum(o, 0)
        L = np.minimum(Wq, Wt + o) - a
        _DIAG[key] = ((i - j + Wt - 1).ravel(), o, a, L)
    return _DIAG[key]


def restate_compare(queries, targets, metric="pearson", bins=100, min_overlap=5, both=True):
    """ms_motifs_compare's definition in numpy: dict of the six planes [n_q][n_t], the bytes the device gives."""
    _check(bins, min_overlap)
    m, bins, both = _metric(metric), int(bins), bool(both)
    qs, ts = _matrices(queries), _matrices(targets)
    out = {name: np.zeros((len(qs), len(ts)), dtype=dt) for name, dt in _lib.COMPARE_PLANES}
    if not qs or not ts:
        return out
    tg = _Targets(ts, m)
    for qi, q in enumerate(qs):
        Wq = q.shape[1]
        _, flat, Kf, Kr = _null(prepare(q, m), tg, m, bins, both)
        start = np.array([table_offset(Wq, bins, a, 1) for a in range(Wq)], dtype=np.int64)
        for ti in range(len(ts)):
            Wt, tf = int(tg.widths[ti]), int(tg.first[ti])
            cell, o, a, L = _diagonals(Wq, Wt)
            adm = L >= min(int(min_overlap), Wq, Wt)
            cand = []
            for rev in range(2 if both else 1):
                sub = Kr[:, tf:tf + Wt][:, ::-1] if rev else Kf[:, tf:tf + Wt]      # reversed target: column j is column Wt - 1 - j, entries reversed
                S = np.bincount(cell, weights=sub.ravel(), minlength=Wq + Wt - 1).astype(np.int64)     # (small integers: exact in a double)
                p = flat[(start[a] + tables_upto(L - 1, bins) + S)[adm]]
                cand.append((p, L[adm], np.full(adm.sum(), rev), o[adm], S[adm]))
            p, Lc, rv, oc, Sc = (np.concatenate(x) for x in zip(*cand))
            w = np.lexsort((oc, rv, -Lc, p))[0]                          # the least (p, -L, orientation, o)
            out["p_min"][qi, ti], out["offset"][qi, ti], out["overlap"][qi, ti] = p[w], oc[w], Lc[w]
            out["score"][qi, ti], out["orient"][qi, ti], out["n_offsets"][qi, ti] = Sc[w], rv[w], len(p)
    return out


def n_offsets_closed_form(Wq, Wt, min_overlap, both=True):
    """The number of admissible alignments of widths Wq, Wt: the offsets whose overlap is at least m = min(min_overlap, Wq, Wt), per
    orientation Wq + Wt - 1 - 2 (m - 1)."""
    m = min(int(min_overlap), Wq, Wt)
    return (2 if both else 1) * (Wq + Wt + 1 - 2 * m)


# ------------------------------------------------------------------------------------------------ the result

class Comparison:
    """The six planes [n_q][n_t] of a comparison and the host arithmetic on them."""

    def __init__(self, planes, query_names=None, target_names=None, metric="pearson", bins=100, min_overlap=5, both=True):
        for name, dt in _lib.COMPARE_PLANES:
            setattr(self, name, np.asarray(planes[name], dtype=dt))
        self.n_queries, self.n_targets = self.p_min.shape
        self.query_names = list(query_names) if query_names is not None else [None] * self.n_queries
        self.target_names = list(target_names) if target_names is not None else [None] * self.n_targets
        self.metric, self.bins, self.min_overlap, self.both = metric, bins, min_overlap, both

    def planes(self):
        return {name: getattr(self, name) for name, _ in _lib.COMPARE_PLANES}

    def p_value(self):
        """1 - (1 - p_min)^n_offsets, as -expm1(n_offsets * log1p(-p_min)): the best of n_offsets alignments, corrected."""
        with np.errstate(divide="ignore"):
            return -np.expm1(self.n_offsets * np.log1p(-np.minimum(self.p_min, 1.0)))

    def e_value(self):
        return self.p_value() * float(self.n_targets)

    def q_value(self):
        """Benjamini-Hochberg per query row: q of the i-th smallest of m P-values = min over j >= i of p_(j) m / j, at most 1."""
        p = self.p_value()
        m = self.n_targets
        out = np.ones_like(p)
        if m == 0:
            return out
        order = np.argsort(p, axis=1, kind="stable")
        ranked = np.take_along_axis(p, order, axis=1) * float(m) / np.arange(1, m + 1)
        q = np.minimum(np.minimum.accumulate(ranked[:, ::-1], axis=1)[:, ::-1], 1.0)
        np.put_along_axis(out, order, q, axis=1)
        return out

    def best(self, k=1):
        """Per query a list of its k best targets, by (p_value, target index): dicts of target, name, p_value, e_value, offset, orient,
        overlap."""
        p = self.p_value()
        rows = []
        for qi in range(self.n_queries):
            order = np.argsort(p[qi], kind="stable")[:k]
            rows.append([dict(target=int(t), name=self.target_names[t], p_value=float(p[qi, t]), e_value=float(p[qi, t]) * self.n_targets,
                              offset=int(self.offset[qi, t]), orient=int(self.orient[qi, t]), overlap=int(self.overlap[qi, t])) for t in order])
        return rows

    def groups(self, threshold):
        """The connected components of a set compared with itself, two motifs joined where either's p_value against the other is
        <= threshold: a list of ascending index lists, ordered by their first members -- the redundancy classes to collapse an
        enrichment table by."""
        if self.n_queries != self.n_targets:
            raise ValueError("groups needs a set compared with itself")
        parent = list(range(self.n_queries))

        def find(x):
            while parent[x] != x:
                parent[x] = parent[parent[x]]
                x = parent[x]
            return x

        for i, j in zip(*np.nonzero(self.p_value() <= threshold)):
            ri, rj = find(int(i)), find(int(j))
            if ri != rj:
                parent[max(ri, rj)] = min(ri, rj)
        classes = {}
        for i in range(self.n_queries):
            classes.setdefault(find(i), []).append(i)
        return sorted(classes.values())


def _ppm_set(mset, what):
    kind = getattr(mset, "kind", None)
    if kind == "pfm":
        return mset.to_ppm()
    if kind == "ppm":
        return mset
    if kind == "pwm":
        raise ValueError(f"{what}: log-odds matrices without their background are not comparable; pass the 'ppm' or 'pfm' set")
    raise ValueError(f"{what} must be a MotifSet of kind 'ppm' or 'pfm'")


def compare(queries, targets, metric="pearson", bins=100, min_overlap=5, both=True, q_block=None, timing=None):
    """Every motif of `queries` against every motif of `targets` (MotifSets of kind 'ppm' or 'pfm'; counts go through to_ppm()) on the
    device: a Comparison.  metric 'pearson', 'sw' (Sandelin-Wasserman) or 'ed' (Euclidean); bins: score levels per column; min_overlap:
    the fewest columns of an alignment (motifs narrower than that align in full); both: also against the reverse complement of each
    target.  q_block: queries per device call (None: all at once), so that a large library never holds its Q x T planes on the device
    at once.  timing: a dict that receives the summed 'device_ms'."""
    qs, ts = _ppm_set(queries, "queries"), _ppm_set(targets, "targets")
    (qv, qw), (tv, tw) = qs.flat(), ts.flat()
    n_q = len(qw)
    step = n_q if q_block is None else int(q_block)
    if q_block is not None and step < 1:
        raise ValueError("q_block must be >= 1")
    m = _metric(metric)
    parts = [_lib.compare_motifs(qv, qw, tv, tw, m, bins, min_overlap, 3 if both else 1, q0, min(q0 + step, n_q), timing=timing)
             for q0 in range(0, n_q, max(step, 1))]
    if not parts:
        parts = [_lib.compare_motifs(qv, qw, tv, tw, m, bins, min_overlap, 3 if both else 1, 0, 0, timing=timing)]
    planes = {name: np.concatenate([p[name] for p in parts]) for name, _ in _lib.COMPARE_PLANES}
    return Comparison(planes, qs.names, ts.names, metric, bins, min_overlap, both)
