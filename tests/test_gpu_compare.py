"""
ms_motifs_compare (ms_compare.hip) on the GPU: motif sets compared with each other, the six planes held byte for byte to the numpy
restatement (`compare.restate_compare`) and the null of a query (`ms_debug_compare_null`: every histogram count and every table byte) to
`compare.restate_null`; tests/test_compare_host.py pins both to exact arithmetic.  The sizes come from ms_debug_compare_dims: the
histogram's tile of target columns and the alignment's tile of targets, each with its neighbours.  Query range, batch size
(ms_debug_compare_budget) and what recycled memory holds change no byte.
"""
import ctypes

import numpy as np
import pytest

from compare_cases import (METRIC_NAMES, PLANES, alignment_cases, columns_set, dirichlet_set, flat, library_ppm, matrix_of, revcomp, rows_of, same_planes,
                           uniform_query_case)
from motifscan_amd import _lib, compare
from motifscan_amd.matrix import MotifSet

pytestmark = pytest.mark.gpu

MAXW = _lib.MS_COMPARE_MAX_WIDTH


def device_compare(queries, targets, metric="pearson", bins=100, min_overlap=5, both=True, q0=0, q1=None, timing=None):
    return _lib.compare_motifs(*flat(queries), *flat(targets), compare.METRICS[metric], bins, min_overlap, 3 if both else 1, q0, q1, timing=timing)


def device_null(queries, targets, metric, bins, both, query):
    return _lib.compare_null(*flat(queries), *flat(targets), compare.METRICS[metric], bins, 3 if both else 1, query)


def null_matches(queries, targets, metric, bins, both, query):
    H, tail = device_null(queries, targets, metric, bins, both, query)
    wantH, want_tail = compare.restate_null(queries[query], targets, metric, bins, both)
    N = (2 if both else 1) * sum(t.shape[1] for t in targets)
    return H.dtype == np.uint32 and H.tobytes() == wantH.tobytes() and tail.tobytes() == want_tail.tobytes() and H.sum(axis=1).tolist() == [N] * len(H)


@pytest.fixture(scope="module")
def dims():
    return _lib.compare_dims()


# ------------------------------------------------------------------------------------------------ 1. widths, bins, metrics, orientations

@pytest.mark.parametrize("both", [False, True])
@pytest.mark.parametrize("metric", METRIC_NAMES)
def test_widths_from_one_to_the_cap(metric, both):
    mats = [matrix_of(w, 500 + w) for w in (1, 2, 63, MAXW, 5, 9)]
    mats.append(revcomp(mats[3]))
    want = {m: compare.restate_compare(mats, mats, metric, 8, m, both) for m in (1, 5, 100)}
    for min_overlap, w in want.items():
        assert same_planes(device_compare(mats, mats, metric, 8, min_overlap, both), w), min_overlap
    full = want[100]                                                 # above every width: only the full overlaps of the narrower motif
    assert full["overlap"][3, 2] == 63 and full["n_offsets"][3, 2] == (2 if both else 1) * 2 and full["overlap"][0, 3] == 1
    assert want[5]["offset"][3, 3] == 0 and want[5]["overlap"][3, 3] == MAXW and want[5]["orient"][3, 6] == (1 if both else 0)
    for query in (0, 2, 3):
        assert null_matches(mats, mats, metric, 8, both, query), query


@pytest.mark.parametrize("bins", [2, 100, _lib.MS_COMPARE_MAX_BINS])
def test_bin_counts_at_narrow_widths(bins):
    mats = dirichlet_set(9, 31 + bins, 1, 6)
    for metric in METRIC_NAMES:
        for both in (False, True):
            for min_overlap in (1, 5):
                want = compare.restate_compare(mats, mats, metric, bins, min_overlap, both)
                assert same_planes(device_compare(mats, mats, metric, bins, min_overlap, both), want), (metric, both, min_overlap)
        widest = max(range(len(mats)), key=lambda i: mats[i].shape[1])
        assert null_matches(mats, mats, metric, bins, True, widest)


# ------------------------------------------------------------------------------------------------ 2. tiles

def test_target_columns_around_the_histogram_tile(dims):
    tile = dims["hist_tile"]
    queries = [matrix_of(5, 61), matrix_of(1, 62), matrix_of(3, 63)]
    for n_cols in (tile - 1, tile, tile + 1, 2 * tile + 1):
        targets = columns_set(n_cols, 70 + n_cols % 7)
        assert sum(t.shape[1] for t in targets) == n_cols
        for both, metric in ((True, "pearson"), (False, "ed")):
            assert same_planes(device_compare(queries, targets, metric, 50, 5, both), compare.restate_compare(queries, targets, metric, 50, 5, both)), n_cols
            assert null_matches(queries, targets, metric, 50, both, 0), n_cols
    lone = [matrix_of(1, 64)]                                            # a single target of width 1
    for metric in METRIC_NAMES:
        assert same_planes(device_compare(queries, lone, metric, 50, 5, True), compare.restate_compare(queries, lone, metric, 50, 5, True))
        assert null_matches(queries, lone, metric, 50, True, 0) and null_matches(queries, lone, metric, 50, False, 2)


def test_target_counts_around_the_alignment_tile(dims):
    tile = dims["align_tile"]
    queries = [matrix_of(4, 81), matrix_of(2, 82)]
    pool = dirichlet_set(2 * tile + 1, 83, 1, 3)
    for n_t in (tile - 1, tile, tile + 1, 2 * tile + 1):
        got = device_compare(queries, pool[:n_t], "sw", 20, 2, True)
        assert got["p_min"].shape == (2, n_t) and same_planes(got, compare.restate_compare(queries, pool[:n_t], "sw", 20, 2, True)), n_t


# ------------------------------------------------------------------------------------------------ 3. bin edges

def test_scores_on_bin_edges_and_the_clamp():
    """Under sw, columns whose squared distance is a dyadic rational put g on a bin edge lo + k / scale exactly: one-hot against one-hot
    (ssd 0: g = 2, k = bins, clamped to bins - 1; ssd 2: k = 0), one-hot against a half-half column (ssd 0.5: k = 0.75 bins), two
    disjoint half-half columns (ssd 1: k = bins / 2)."""
    e = np.eye(4)
    hh = [np.array([0.5, 0.5, 0.0, 0.0]), np.array([0.0, 0.0, 0.5, 0.5]), np.array([0.5, 0.0, 0.5, 0.0])]
    cols = [e[0], e[1], e[2], e[3]] + hh
    singles = [np.ascontiguousarray(c.reshape(4, 1)) for c in cols]
    wide = [np.ascontiguousarray(np.stack([cols[i] for i in idx], axis=1)) for idx in ((0, 4, 1, 5), (3, 6, 6, 2, 0), (4, 4, 4))]
    mats = singles + wide
    for bins in (4, 100, 256):
        for metric in METRIC_NAMES:
            want = compare.restate_compare(mats, mats, metric, bins, 1, True)
            assert same_planes(device_compare(mats, mats, metric, bins, 1, True), want), (bins, metric)
            assert null_matches(mats, mats, metric, bins, True, len(singles))
        got = device_compare(singles, singles, "sw", bins, 1, False)          # width 1 against width 1: `score` is the column score
        assert got["score"][0, 0] == bins - 1 and got["score"][0, 1] == 0           # identical columns: the clamp; ssd 2: the lowest bin
        assert got["score"][0, 4] == (3 * bins) // 4 and got["score"][4, 5] == bins // 2 and got["score"][4, 4] == bins - 1
    ident = device_compare(singles, singles, "pearson", 100, 1, False)
    assert all(ident["score"][i, i] == 99 for i in range(len(singles)))             # g = 1: (1 + 1) * 50 = 100, clamped


# ------------------------------------------------------------------------------------------------ 4. ties

@pytest.mark.parametrize("metric", METRIC_NAMES)
def test_hand_written_alignment_cases_on_the_device(metric):
    for case in alignment_cases():
        got = device_compare(case["queries"], case["targets"], metric, 100, both=True, **case["kw"])
        assert same_planes(got, compare.restate_compare(case["queries"], case["targets"], metric, 100, both=True, **case["kw"])), case["name"]
        for q, t, offset, orient, overlap, n_offsets in case["expect"]:
            assert (got["offset"][q, t], got["orient"][q, t], got["overlap"][q, t]) == (offset, orient, overlap), (case["name"], metric)
            assert n_offsets is None or got["n_offsets"][q, t] == n_offsets


def test_an_all_quarter_query_on_the_device():
    queries, targets, expect = uniform_query_case()
    got = device_compare(queries, targets, "pearson", 100, 5, True)
    assert same_planes(got, compare.restate_compare(queries, targets, "pearson", 100, 5, True))
    assert got["p_min"].tobytes() == np.ones_like(got["p_min"]).tobytes()
    for q, t, offset, orient, overlap, _ in expect:
        assert (got["offset"][q, t], got["orient"][q, t], got["overlap"][q, t]) == (offset, orient, overlap), t


# ------------------------------------------------------------------------------------------------ 5. batches and query ranges

@pytest.fixture(scope="module")
def batch_case():
    queries = [matrix_of(5, 90 + i) for i in range(5)]
    targets = dirichlet_set(11, 95, 2, 9)
    return dict(queries=queries, targets=targets, want=compare.restate_compare(queries, targets, "ed", 10, 3, True), per=8 * compare.table_doubles(5, 10))


def test_batches_change_no_byte_and_a_query_that_does_not_fit_is_refused(batch_case):
    queries, targets, want, per = (batch_case[k] for k in ("queries", "targets", "want", "per"))
    for budget in (0, 5 * per, 4 * per + 8, 2 * per, per):                # one batch; 4 + 1; 2 + 2 + 1; five batches of one
        before = _lib.compare_budget(budget)
        try:
            assert same_planes(device_compare(queries, targets, "ed", 10, 3, True), want), budget
            for q0, q1 in ((1, 4), (3, 5), (1, 2), (0, 3)):              # ranges that start and end inside a batch
                assert same_planes(device_compare(queries, targets, "ed", 10, 3, True, q0, q1), rows_of(want, q0, q1)), (budget, q0, q1)
            assert null_matches(queries, targets, "ed", 10, True, 4)
        finally:
            _lib.compare_budget(before)
    mixed = [matrix_of(w, 110 + w) for w in (3, 9, 1, 9, 2, 4)]
    want_mixed = compare.restate_compare(mixed, targets, "pearson", 10, 3, True)
    before = _lib.compare_budget(8 * compare.table_doubles(9, 10))       # the widest query alone fills a batch
    try:
        assert same_planes(device_compare(mixed, targets, "pearson", 10, 3, True), want_mixed)
    finally:
        _lib.compare_budget(before)
    before = _lib.compare_budget(per - 1)
    try:
        sentinel = {k: np.full_like(v, 77) for k, v in want.items()}
        with pytest.raises(MemoryError, match="work budget"):
            device_compare(queries, targets, "ed", 10, 3, True)
        assert raw_call(queries, targets, out=sentinel) == _lib.MS_ERR_NOMEM and all((sentinel[k] == 77).all() for k in PLANES)
        narrow = [matrix_of(4, 120)]                                     # a narrower query still fits
        assert same_planes(device_compare(narrow, targets, "ed", 10, 3, True), compare.restate_compare(narrow, targets, "ed", 10, 3, True))
    finally:
        _lib.compare_budget(before)


# ------------------------------------------------------------------------------------------------ 6. recycled memory

@pytest.mark.parametrize("fill", [0x00, 0xFF, 0xA5])
def test_recycled_memory_changes_no_byte(batch_case, fill):
    queries, targets, want = (batch_case[k] for k in ("queries", "targets", "want"))
    other_q, other_t = dirichlet_set(3, 130, 1, 12), dirichlet_set(40, 131, 1, 12)
    other_want = compare.restate_compare(other_q, other_t, "sw", 64, 5, False)
    plain = device_compare(queries, targets, "ed", 10, 3, True)
    with _lib.alloc_fill(fill):
        first = device_compare(queries, targets, "ed", 10, 3, True)
        assert same_planes(device_compare(other_q, other_t, "sw", 64, 5, False), other_want)      # another call through the same pool
        again = device_compare(queries, targets, "ed", 10, 3, True)
        assert null_matches(queries, targets, "ed", 10, True, 2)
    assert same_planes(plain, want) and same_planes(first, want) and same_planes(again, want)


# ------------------------------------------------------------------------------------------------ 7. statuses

def raw_call(queries, targets, out, metric=0, bins=10, min_overlap=3, orientations=3, q0=0, q1=None, q_values="set", q_widths="set", t_values="set",
             t_widths="set", n_q=None, n_t=None, null=()):
    """The C call itself; `out`: dict of the six planes (a name in `null`: NULL).  Arrays given as "set" come from the matrices."""
    qv, qw = flat(queries)
    tv, tw = flat(targets)
    qv, qw = (qv if isinstance(q_values, str) else q_values), (qw if isinstance(q_widths, str) else q_widths)
    tv, tw = (tv if isinstance(t_values, str) else t_values), (tw if isinstance(t_widths, str) else t_widths)
    p = lambda a, t: None if a is None else _lib.ptr(a, t)
    o = lambda k, t: None if k in null else _lib.ptr(out[k], t)
    n_q = len(queries) if n_q is None else n_q
    return _lib.lib().ms_motifs_compare(p(qv, ctypes.c_double), p(qw, ctypes.c_int32), n_q, p(tv, ctypes.c_double), p(tw, ctypes.c_int32),
                                        len(targets) if n_t is None else n_t, metric, bins, min_overlap, orientations, q0, n_q if q1 is None else q1,
                                        o("p_min", ctypes.c_double), o("offset", ctypes.c_int32), o("overlap", ctypes.c_int32), o("score", ctypes.c_int32),
                                        o("n_offsets", ctypes.c_int32), o("orient", ctypes.c_int8), None)


def test_statuses_write_nothing(batch_case):
    queries, targets, want = (batch_case[k] for k in ("queries", "targets", "want"))
    out = {k: np.full_like(v, 77) for k, v in want.items()}
    untouched = lambda: all((out[k] == 77).all() for k in PLANES)
    INV, OK = _lib.MS_ERR_INVALID, _lib.MS_OK
    qv, qw = flat(queries)
    tv, tw = flat(targets)

    def bad_width(w, v):
        ww = w.copy()
        ww[1] = v
        return ww

    def bad_value(vals, v):
        vv = vals.copy()
        vv[7] = v
        return vv

    cases = [dict(q_values=None), dict(q_widths=None), dict(t_values=None), dict(t_widths=None), dict(n_q=-1, q1=0), dict(n_t=-1)]
    cases += [dict(null=(k,)) for k in PLANES]
    cases += [dict(q_widths=bad_width(qw, v)) for v in (0, -3, MAXW + 1)] + [dict(t_widths=bad_width(tw, v)) for v in (0, MAXW + 1)]
    cases += [dict(q_values=bad_value(qv, v)) for v in (np.nan, np.inf)] + [dict(t_values=bad_value(tv, v)) for v in (np.nan, -np.inf)]
    cases += [dict(metric=-1), dict(metric=3), dict(bins=1), dict(bins=_lib.MS_COMPARE_MAX_BINS + 1), dict(min_overlap=0), dict(min_overlap=-5)]
    cases += [dict(orientations=v) for v in (0, 2, 4)] + [dict(q0=-1), dict(q1=len(queries) + 1), dict(q0=3, q1=2)]
    for kw in cases:
        assert raw_call(queries, targets, out, **kw) == INV and untouched(), kw
    with pytest.raises(ValueError):
        _lib.check(raw_call(queries, targets, out, metric=3))
    # more than 2^30 target columns: refused on the widths alone, before a value is read
    many = np.full((1 << 30) // MAXW + 1, MAXW, dtype=np.int32)
    assert raw_call(queries, targets, out, t_widths=many, n_t=len(many)) == INV and untouched()
    del many
    # the three empty cases
    assert raw_call(queries, targets, out, n_q=0, q_values=None, q_widths=None) == OK and untouched()
    assert raw_call(queries, targets, out, n_t=0, t_values=None, t_widths=None) == OK and untouched()
    assert raw_call(queries, targets, out, q0=2, q1=2, null=PLANES) == OK and untouched()
    empty = device_compare([], targets)
    assert empty["p_min"].shape == (0, len(targets)) and device_compare(queries, [])["orient"].shape == (len(queries), 0)
    # and the call itself, into the same planes
    assert raw_call(queries, targets, out, metric=2) == OK and same_planes(out, want)
    L = _lib.lib()
    H, tail = np.zeros((5, 10), dtype=np.uint32), np.zeros(compare.table_doubles(5, 10))
    null_args = lambda query, n_t=len(targets), H=H, tail=tail: (
        _lib.ptr(qv, ctypes.c_double), _lib.ptr(qw, ctypes.c_int32), len(queries), _lib.ptr(tv, ctypes.c_double), _lib.ptr(tw, ctypes.c_int32), n_t, 2, 10, 3, query,
        None if H is None else _lib.ptr(H, ctypes.c_uint32), None if tail is None else _lib.ptr(tail, ctypes.c_double))
    for args in (null_args(-1), null_args(len(queries)), null_args(0, n_t=0), null_args(0, H=None), null_args(0, tail=None)):
        assert L.ms_debug_compare_null(*args) == INV and not H.any() and not tail.any()
    assert L.ms_debug_compare_null(*null_args(0)) == OK and H.sum() == 5 * 2 * int(tw.sum())


# ------------------------------------------------------------------------------------------------ through Python

def test_python_front_tiles_the_queries_and_takes_count_matrices():
    mats = dirichlet_set(7, 140, 3, 10)
    names = [f"m{i}" for i in range(len(mats))]
    ppm = MotifSet.from_matrices("ppm", mats, names=names)
    want = compare.restate_compare(mats, mats, "pearson", 100, 5, True)
    timing = {}
    whole = compare.compare(ppm, ppm, timing=timing)
    assert same_planes(whole.planes(), want) and timing["device_ms"] > 0
    for q_block in (1, 3, 7, 50):
        assert same_planes(ppm.compare(ppm, q_block=q_block).planes(), want), q_block
    assert [row[0]["name"] for row in whole.best(1)] == names and all(row[0]["offset"] == 0 and row[0]["orient"] == 0 for row in whole.best(1))
    counts = MotifSet.from_matrices("pfm", [np.rint(m * 200).astype(np.int64) + 1 for m in mats])
    via = compare.compare(counts, ppm, metric="sw", bins=50, both=False)
    assert same_planes(via.planes(), compare.restate_compare([m.matrix for m in counts.to_ppm()], mats, "sw", 50, 5, False))
    with pytest.raises(ValueError):
        compare.compare(ppm.to_pwm(), ppm)


# ------------------------------------------------------------------------------------------------ 8. the synthetic library against itself

def test_the_synthetic_library_against_itself():
    mats = library_ppm()
    n = len(mats)
    assert n == 579 and max(m.shape[1] for m in mats) <= MAXW
    lib_set = MotifSet.from_matrices("ppm", mats)
    timing = {}
    c = compare.compare(lib_set, lib_set, metric="pearson", bins=100, both=True, timing=timing)
    print(f"ms_motifs_compare, {n} x {n} motifs, {sum(m.shape[1] for m in mats)} columns, pearson, 100 bins, both orientations: device_ms = {timing['device_ms']:.3f}")
    assert timing["device_ms"] > 0
    p = c.p_value()
    duplicates = {}
    for i, m in enumerate(mats):
        duplicates.setdefault(m.tobytes(), []).append(i)
    for i in range(n):
        same = duplicates[mats[i].tobytes()]
        best = int(np.argmin(p[i]))                                      # (the first of equal minima: the least index of an exact duplicate)
        assert best == same[0], i
        assert (c.offset[i, i], c.orient[i, i], c.overlap[i, i]) == (0, 0, mats[i].shape[1]) and p[i, i] == p[i, best], i
    groups = c.groups(1e-6)
    assert sorted(i for g in groups for i in g) == list(range(n)) and all(g == sorted(g) for g in groups)        # a partition
    rows = sorted(np.random.default_rng(8).choice(n, size=6, replace=False).tolist())
    want = compare.restate_compare([mats[i] for i in rows], mats, "pearson", 100, 5, True)
    got = {k: c.planes()[k][rows] for k in PLANES}
    assert same_planes(got, want)
