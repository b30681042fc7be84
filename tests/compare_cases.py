"""
Case makers shared by tests/test_compare_host.py and tests/test_gpu_compare.py (ms_motifs_compare; motifscan_amd.compare): seeded motif
sets, the hand-written alignment cases with the answers they pin, a scalar brute-force restatement that shares no code with
compare.restate_compare, and byte comparison of plane dicts.  Not a test module.
"""
import math

import numpy as np

from motifscan_amd import _lib, compare

PLANES = tuple(name for name, _ in _lib.COMPARE_PLANES)
METRIC_NAMES = ("pearson", "sw", "ed")


def dirichlet_set(n, seed, wmin=4, wmax=14, alpha=0.3):
    """n probability matrices [4][W], W uniform in [wmin, wmax], Dirichlet(alpha) columns."""
    rng = np.random.default_rng(seed)
    return [np.ascontiguousarray(rng.dirichlet(np.full(4, alpha), size=int(rng.integers(wmin, wmax + 1))).T) for _ in range(n)]


def matrix_of(width, seed, alpha=0.3):
    return np.ascontiguousarray(np.random.default_rng(seed).dirichlet(np.full(4, alpha), size=width).T)


def revcomp(m):
    return np.ascontiguousarray(np.asarray(m)[::-1, ::-1])


def flat(mats):
    """(values, widths) as the C call takes them."""
    values = np.concatenate([np.ascontiguousarray(m, dtype=np.float64).ravel() for m in mats]) if len(mats) else np.zeros(0)
    return values, np.array([np.asarray(m).shape[1] for m in mats], dtype=np.int32)


def same_planes(got, want):
    return all(np.asarray(got[k]).dtype == np.asarray(want[k]).dtype and np.asarray(got[k]).tobytes() == np.asarray(want[k]).tobytes() for k in PLANES)


def rows_of(planes, q0, q1):
    return {k: planes[k][q0:q1] for k in PLANES}


def inverse_is_exact(n):
    """n * fl(1 / n) == 1.0: a histogram with all its n counts in one bin then gives f = 1.0 exactly."""
    return float(n) * (1.0 / float(n)) == 1.0


def alignment_cases():
    """The hand-written cases: a list of dicts(name, queries, targets, kw, expect) with expect a list of (query, target, offset, orient,
    overlap, n_offsets or None).  24 Dirichlet(0.3) targets of width 4-14 at default_rng(7) are the database of all of them."""
    db = dirichlet_set(24, 7)
    wide = next(i for i, m in enumerate(db) if m.shape[1] >= 10)
    rng = np.random.default_rng(70)
    cases = []
    W = db[3].shape[1]
    cases.append(dict(name="a target equal to the query", queries=[db[3]], targets=db, kw={}, expect=[(0, 3, 0, 0, W, None)]))
    cases.append(dict(name="the reverse complement of a target as the query", queries=[revcomp(db[3])], targets=db, kw={}, expect=[(0, 3, 0, 1, W, None)]))
    cases.append(dict(name="the query is columns 2..8 of a target", queries=[db[wide][:, 2:9]], targets=db, kw={}, expect=[(0, wide, -2, 0, 7, None)]))
    extra = rng.dirichlet(np.full(4, 0.3), size=3).T
    cases.append(dict(name="a target embedded in the query behind 3 extra columns", queries=[np.concatenate([extra, db[wide]], axis=1)], targets=db, kw={},
                      expect=[(0, wide, 3, 0, db[wide].shape[1], None)]))
    half = rng.dirichlet(np.full(4, 0.3), size=4).T
    pal = np.concatenate([half, revcomp(half)], axis=1)
    assert np.array_equal(pal, revcomp(pal))
    cases.append(dict(name="a palindromic motif: forward wins the tie", queries=[pal], targets=db + [pal], kw={}, expect=[(0, len(db), 0, 0, 8, None)]))
    same = np.repeat(np.array([[0.7], [0.1], [0.15], [0.05]]), 6, axis=1)
    cases.append(dict(name="identical columns: the full overlap wins", queries=[same], targets=db + [same], kw=dict(min_overlap=1),
                      expect=[(0, len(db), 0, 0, 6, 2 * (2 * 6 - 1))]))
    return cases


def uniform_query_case():
    """An all-0.25 query under pearson: every prepared vector is +0.0, every column score the same bin, every p exactly 1.0 -- so the
    largest overlap, forward, least offset wins.  (queries, targets, expect) with targets narrower and wider than the query; the
    database's column count N has N * fl(1 / N) == 1.0, asserted."""
    db = dirichlet_set(9, 11, 3, 12)
    while not inverse_is_exact(2 * sum(m.shape[1] for m in db)):
        db.append(matrix_of(5, 100 + len(db)))
    q = np.full((4, 7), 0.25)
    expect = []
    for t, m in enumerate(db):
        Wt = m.shape[1]
        expect.append((0, t, 0 if Wt <= 7 else -(Wt - 7), 0, min(7, Wt), None))
    assert any(m.shape[1] > 7 for m in db) and any(m.shape[1] < 7 for m in db)
    return [q], db, expect


# ------------------------------------------------------------------------------------------------ a scalar restatement

def scalar_prepare(column, metric):
    x = [float(v) for v in column]
    if metric != "pearson":
        return x
    mean = (((x[0] + x[1]) + x[2]) + x[3]) * 0.25
    c = [v - mean for v in x]
    n = math.sqrt(((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]) + c[3] * c[3])
    return [v / n for v in c] if n > 0.0 else [0.0] * 4


def scalar_score(u, v, metric, bins):
    """The integer column score in plain Python floats (each operation one rounded fp64 operation)."""
    if metric == "pearson":
        g, lo, scale = ((u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]) + u[3] * v[3], -1.0, bins * 0.5
    else:
        d = [a - b for a, b in zip(u, v)]
        ssd = ((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) + d[3] * d[3]
        g, lo, scale = (2.0 - ssd, 0.0, bins * 0.5) if metric == "sw" else (-math.sqrt(ssd), -math.sqrt(2.0), bins / math.sqrt(2.0))
    return min(max(int(math.floor((g - lo) * scale)), 0), bins - 1)


def scalar_columns(mats, metric, reverse=False):
    """Per matrix the list of its prepared columns; reverse: the reversed target (column j = prepared column W - 1 - j, entries reversed)."""
    out = []
    for m in mats:
        cols = [scalar_prepare(np.asarray(m)[:, c], metric) for c in range(np.asarray(m).shape[1])]
        out.append([list(reversed(c)) for c in reversed(cols)] if reverse else cols)
    return out


def brute_compare(queries, targets, metric, bins, min_overlap, both):
    """The planes by plain loops over pairs, orientations, offsets and columns; the tables come from compare.restate_null (whose bytes
    tests/test_compare_host.py pins to exact rationals), everything else is scalar Python."""
    out = {name: np.zeros((len(queries), len(targets)), dtype=dt) for name, dt in _lib.COMPARE_PLANES}
    fwd, rev = scalar_columns(targets, metric), scalar_columns(targets, metric, True)
    for qi, q in enumerate(queries):
        Wq = np.asarray(q).shape[1]
        qcols = scalar_columns([q], metric)[0]
        tail = compare.restate_null(q, targets, metric, bins, both)[1]
        for ti in range(len(targets)):
            Wt = len(fwd[ti])
            need = min(min_overlap, Wq, Wt)
            best, n = None, 0
            for orient, cols in enumerate((fwd[ti], rev[ti]) if both else (fwd[ti],)):
                for o in range(-(Wt - 1), Wq):
                    a, e = max(0, o), min(Wq, Wt + o)
                    L = e - a
                    if L < need:
                        continue
                    S = sum(scalar_score(qcols[i], cols[i - o], metric, bins) for i in range(a, e))
                    p = float(tail[compare.table_offset(Wq, bins, a, L) + S])
                    n += 1
                    key = (p, -L, orient, o)
                    if best is None or key < best[0]:
                        best = (key, S)
            (p, negL, orient, o), S = best
            out["p_min"][qi, ti], out["offset"][qi, ti], out["overlap"][qi, ti] = p, o, -negL
            out["score"][qi, ti], out["orient"][qi, ti], out["n_offsets"][qi, ti] = S, orient, n
    return out


def library_ppm(n=579):
    """The synthetic JASPAR-like library as probability matrices: its log-odds entries exponentiated against its background and every
    column rescaled to sum 1 (the entries were rounded to 5 decimals)."""
    from motifscan_amd import synth
    values, widths, _ = synth.load_motif_set(n)
    out = []
    for m in synth.matrices_of(values, widths):
        p = np.exp(m) * synth.BG[:, None]
        out.append(np.ascontiguousarray(p / p.sum(axis=0)))
    return out


def columns_set(n_cols, seed, width=64):
    """Dirichlet targets of `width` columns each (the last one narrower) with n_cols columns in all."""
    rng = np.random.default_rng(seed)
    widths = [width] * (n_cols // width) + ([n_cols % width] if n_cols % width else [])
    return [np.ascontiguousarray(rng.dirichlet(np.full(4, 0.3), size=w).T) for w in widths]
