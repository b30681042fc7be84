"""
The host side of the motif comparison (ms_motifs_compare; motifscan_amd.compare), no GPU: the numpy restatement of the contract
(`compare.restate_null`, `compare.restate_compare`) pinned to exact arithmetic -- histograms against a scalar brute-force count, every
tail table against the exact rational over all column tuples --, hand-written alignment cases that pin the sign of `offset`, the
reverse orientation and the tie rule, the properties of the planes (query tiling, forward-only, the closed form of n_offsets, the range
of p_min), the host arithmetic of `Comparison` against hand-written answers, the "no device" answer, and the plan's stand-alone
program under ASan + UBSan (motifscan_amd/csrc/ms_compare_plan.h, tests/sanitize/compare_plan_asan.cpp).
tests/test_gpu_compare.py holds the device to the same restatement byte for byte.
"""
import itertools
import os
import re
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from compare_cases import (METRIC_NAMES, alignment_cases, brute_compare, dirichlet_set, matrix_of, revcomp, rows_of, same_planes, scalar_columns,
                           scalar_score, uniform_query_case)
from motifscan_amd import _lib, compare
from motifscan_amd.matrix import MotifSet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "motifscan_amd", "csrc")
BIN = os.path.join(ROOT, "tests", "sanitize", "compare_plan_asan.bin")


# ------------------------------------------------------------------------------------------------ the symbols, no device

def test_header_declares_the_entry_point_and_the_library_has_it():
    with open(os.path.join(ROOT, "include", "motifscan_amd.h")) as fh:
        text = fh.read()
    assert re.search(r"\bint\s+ms_motifs_compare\s*\(", text)
    for name, value in (("MS_COMPARE_PEARSON", 0), ("MS_COMPARE_SW", 1), ("MS_COMPARE_ED", 2), ("MS_COMPARE_MAX_WIDTH", 64), ("MS_COMPARE_MAX_BINS", 256)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), text) and getattr(_lib, name) == value
    with open(os.path.join(ROOT, "include", "motifscan_amd_debug.h")) as fh:
        dbg = fh.read()
    for name in ("ms_debug_compare_dims", "ms_debug_compare_budget", "ms_debug_compare_null"):
        assert re.search(r"\bint\s+%s\s*\(" % name, dbg) and hasattr(_lib.lib(), name)
    assert hasattr(_lib.lib(), "ms_motifs_compare")


def test_dims_and_budget_need_no_device():
    d = _lib.compare_dims()
    assert d["threads"] >= 64 and d["hist_tile"] % d["threads"] == 0 and d["align_tile"] >= 1
    assert d["budget_mib"] << 20 >= 8 * compare.table_doubles(_lib.MS_COMPARE_MAX_WIDTH, _lib.MS_COMPARE_MAX_BINS)    # the caps fit the default budget
    assert d["batch_cap"] >= 1 and d["lds_limit"] == 0
    assert _lib.lib().ms_debug_compare_dims(None) == _lib.MS_ERR_INVALID
    assert _lib.lib().ms_debug_compare_budget(-1, None) == _lib.MS_ERR_INVALID
    before = _lib.compare_budget(12345)
    assert _lib.compare_budget(before) == 12345 and _lib.compare_budget(before) == before


def test_no_gpu_means_loud_failure_before_any_validation():
    L = _lib.lib()
    args = (None, None, -1, None, None, -1, 9, 0, 0, 2, 5, 1) + (None,) * 7                      # every one of them invalid
    have_device = _lib.device_count() > 0
    rc_null = L.ms_debug_compare_null(None, None, -1, None, None, -1, 9, 0, 2, 0, None, None)
    rc = L.ms_motifs_compare(*args)
    if have_device:
        assert rc == _lib.MS_ERR_INVALID and rc_null == _lib.MS_ERR_INVALID
        return
    assert rc == _lib.MS_ERR_RUNTIME and rc_null == _lib.MS_ERR_RUNTIME
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _lib.check(rc)


# ------------------------------------------------------------------------------------------------ the exact null

@pytest.mark.parametrize("metric", METRIC_NAMES)
@pytest.mark.parametrize("both, widths, bins", [(True, (1, 3), 7), (True, (2, 2), 2), (False, (3, 4, 1), 5), (False, (8,), 7), (True, (4,), 3),
                                                (True, (1, 2), 7), (False, (3, 2, 2), 6), (False, (5,), 4), (True, (3,), 5)])
def test_null_against_a_brute_force_count_and_exact_rationals(metric, both, widths, bins):
    targets = [matrix_of(w, 300 + 10 * i + w) for i, w in enumerate(widths)]
    query = matrix_of(3, 41)
    query[:, 1] = targets[0][:, 0]                               # a query column that is in the database: the clamp at bins - 1 is met
    columns = [c for t in scalar_columns(targets, metric) for c in t]
    if both:
        columns += [c for t in scalar_columns(targets, metric, True) for c in t]
    N = len(columns)
    assert N <= 8 and N == (2 if both else 1) * sum(widths)
    H, tail = compare.restate_null(query, targets, metric, bins, both)
    q = scalar_columns([query], metric)[0]
    K = [[scalar_score(u, v, metric, bins) for v in columns] for u in q]          # [query column][database column]
    for i in range(3):
        assert H[i].tolist() == np.bincount(K[i], minlength=bins).tolist()
    assert H.dtype == np.uint32 and H.sum(axis=1).tolist() == [N] * 3 and H[1, bins - 1] >= 1
    assert len(tail) == compare.table_doubles(3, bins)
    # The bound, in units of 2^-53 (u), counted along the longest path of rounded operations to one tail entry as the issue states it,
    # L bins + L + 1: the tail sum makes at most L (bins - 1) additions, each of the L columns' f is one conversion-free multiply H * invN
    # on top of invN's own division (L + 1), and the L - 1 convolution steps add one product each (L - 1); their inner sums have at most
    # min(N, bins) - 1 non-zero terms each and are covered by the +1 and the slack of the tail's count, which no s reaches in full.  A
    # worst-case analysis of sums of non-negative terms (Higham, lemma 3.1) would allow 2 L bins + L - bins roundings; the stated,
    # smaller figure is what is held here, and the worst error seen is printed.
    u = Fraction(1, 2 ** 53)
    worst = Fraction(0)
    for a in range(3):
        for L in range(1, 3 - a + 1):
            top = L * (bins - 1)
            sums = [sum(K[a + l][c] for l, c in enumerate(tup)) for tup in itertools.product(range(N), repeat=L)]
            at = compare.table_offset(3, bins, a, L)
            for s in range(top + 1):
                want = Fraction(sum(1 for v in sums if v >= s), N ** L)
                got = float(tail[at + s])
                if want == 0:
                    assert got == 0.0
                    continue
                assert got > 0.0
                err = abs(Fraction(got) - want) / want
                worst = max(worst, err)
                assert err <= (L * bins + L + 1) * u, (a, L, s, float(err / u))
    print(f"{metric} both={both} widths={widths} bins={bins}: worst relative error {float(worst / u):.2f} u")


def test_table_layout_is_a_ascending_then_l_ascending():
    for W, bins in ((1, 2), (3, 7), (6, 100), (64, 256)):
        at = 0
        for a in range(W):
            for L in range(1, W - a + 1):
                assert compare.table_offset(W, bins, a, L) == at
                at += L * (bins - 1) + 1
        assert compare.table_doubles(W, bins) == at
    assert compare.table_doubles(64, 256) == 11670880


# ------------------------------------------------------------------------------------------------ hand-written alignments

@pytest.mark.parametrize("metric", METRIC_NAMES)
def test_hand_written_alignment_cases(metric):
    for case in alignment_cases():
        got = compare.restate_compare(case["queries"], case["targets"], metric, 100, both=True, **case["kw"])
        for q, t, offset, orient, overlap, n_offsets in case["expect"]:
            assert (got["offset"][q, t], got["orient"][q, t], got["overlap"][q, t]) == (offset, orient, overlap), (case["name"], metric)
            assert n_offsets is None or got["n_offsets"][q, t] == n_offsets, case["name"]
            p = compare.Comparison(got).p_value()
            assert p[q].argmin() == t, (case["name"], metric)                # and it is the query's best target of the database


def test_an_all_quarter_query_under_pearson_has_every_p_exactly_one():
    queries, targets, expect = uniform_query_case()
    got = compare.restate_compare(queries, targets, "pearson", 100, min_overlap=5)
    assert got["p_min"].tobytes() == np.ones_like(got["p_min"]).tobytes()
    for q, t, offset, orient, overlap, _ in expect:
        assert (got["offset"][q, t], got["orient"][q, t], got["overlap"][q, t]) == (offset, orient, overlap), t
    assert np.all(compare.Comparison(got).p_value() == 1.0)


# ------------------------------------------------------------------------------------------------ properties

@pytest.fixture(scope="module")
def small():
    queries, targets = dirichlet_set(5, 21, 1, 9), dirichlet_set(7, 22, 1, 11)
    targets[2] = revcomp(queries[1])
    return dict(queries=queries, targets=targets, full={m: compare.restate_compare(queries, targets, m, 20, 3, True) for m in METRIC_NAMES})


@pytest.mark.parametrize("metric", METRIC_NAMES)
def test_the_vectorised_restatement_is_the_scalar_one(small, metric):
    want = brute_compare(small["queries"], small["targets"], metric, 20, 3, True)
    assert same_planes(small["full"][metric], want)
    assert small["full"][metric]["orient"][1, 2] == 1 and small["full"][metric]["offset"][1, 2] == 0


def test_any_tiling_of_the_queries_gives_the_rows_of_the_full_result(small):
    q, t, full = small["queries"], small["targets"], small["full"]["pearson"]
    for q0, q1 in ((0, 1), (1, 4), (4, 5), (2, 2), (0, 5)):
        assert same_planes(compare.restate_compare(q[q0:q1], t, "pearson", 20, 3, True), rows_of(full, q0, q1))


@pytest.mark.parametrize("metric", METRIC_NAMES)
def test_forward_only_is_the_forward_half_with_its_own_null(small, metric):
    got = compare.restate_compare(small["queries"], small["targets"], metric, 20, 3, False)
    assert same_planes(got, brute_compare(small["queries"], small["targets"], metric, 20, 3, False))
    assert not got["orient"].any() and np.array_equal(2 * got["n_offsets"], small["full"][metric]["n_offsets"])
    H1 = compare.restate_null(small["queries"][0], small["targets"], metric, 20, False)[0]
    H3 = compare.restate_null(small["queries"][0], small["targets"], metric, 20, True)[0]
    assert np.array_equal(2 * H1.sum(axis=1), H3.sum(axis=1)) and np.all(H1 <= H3)


def test_n_offsets_has_a_closed_form_and_p_min_lies_in_the_unit_interval(small):
    q, t = small["queries"], small["targets"]
    for min_overlap in (1, 3, 5, 100):
        for both in (False, True):
            got = compare.restate_compare(q, t, "sw", 20, min_overlap, both)
            for qi, ti in itertools.product(range(len(q)), range(len(t))):
                Wq, Wt = q[qi].shape[1], t[ti].shape[1]
                m = min(min_overlap, Wq, Wt)
                assert got["n_offsets"][qi, ti] == (2 if both else 1) * (Wq + Wt + 1 - 2 * m) == compare.n_offsets_closed_form(Wq, Wt, min_overlap, both)
                assert got["overlap"][qi, ti] >= m and -(Wt - 1) <= got["offset"][qi, ti] <= Wq - 1
            assert np.all(got["p_min"] > 0.0) and np.all(got["p_min"] <= 1.0)           # > 0: every aligned column is in its own null
    for metric in METRIC_NAMES:
        assert np.all(small["full"][metric]["p_min"] > 0.0) and np.all(small["full"][metric]["p_min"] <= 1.0)


def test_restatement_refuses_what_the_library_refuses():
    m = matrix_of(4, 1)
    for bad in (dict(bins=1), dict(bins=257), dict(min_overlap=0), dict(metric="cosine")):
        kw = dict(metric="pearson", bins=10, min_overlap=2)
        kw.update(bad)
        with pytest.raises(ValueError):
            compare.restate_compare([m], [m], **kw)
    for mats in ([np.zeros((4, 65))], [np.zeros((3, 4))], [np.full((4, 2), np.nan)]):
        with pytest.raises(ValueError):
            compare.restate_compare(mats, [m])
    with pytest.raises(ValueError):
        compare.restate_null(m, [])
    empty = compare.restate_compare([], [m])
    assert empty["p_min"].shape == (0, 1) and compare.restate_compare([m], [])["orient"].shape == (1, 0)


# ------------------------------------------------------------------------------------------------ host arithmetic

def hand_comparison():
    planes = dict(p_min=np.array([[0.5, 1e-3, 1.0], [1e-20, 0.25, 0.25], [0.1, 0.1, 1e-9]]),
                  n_offsets=np.array([[2, 10, 3], [4, 1, 2], [1, 1, 5]], dtype=np.int32),
                  offset=np.array([[0, -2, 1], [3, 0, 0], [0, 0, 0]], dtype=np.int32), overlap=np.array([[5, 7, 4], [6, 5, 5], [4, 4, 8]], dtype=np.int32),
                  score=np.zeros((3, 3), dtype=np.int32), orient=np.array([[0, 1, 0], [0, 0, 1], [0, 0, 0]], dtype=np.int8))
    return compare.Comparison(planes, ["q0", "q1", "q2"], ["t0", "t1", "t2"])


def test_p_e_and_q_values_against_hand_written_answers():
    c = hand_comparison()
    p = c.p_value()
    want = np.array([[0.75, 1 - 0.999 ** 10, 1.0], [4e-20, 0.25, 1 - 0.75 ** 2], [0.1, 0.1, 5e-9 - 1e-17]])      # (1 - (1 - x)^5 = 5 x - 10 x^2 + ...)
    assert np.allclose(p, want, rtol=1e-12, atol=0) and p[0, 2] == 1.0
    assert abs(p[1, 0] / 4e-20 - 1) < 1e-12                      # no cancellation where 1 - (1 - p)^n would round to 0
    assert np.allclose(c.e_value(), 3 * want, rtol=1e-12)
    q = c.q_value()
    # row 0: sorted p = (0.00995.., 0.75, 1.0) -> p m / rank = (0.02985.., 1.125, 1.0) -> running minimum from the right, capped at 1
    assert np.allclose(q[0], [1.0, 3 * want[0, 1], 1.0], rtol=1e-12)
    # row 1: (4e-20, 0.25, 0.4375) -> (1.2e-19, 0.375, 0.4375)
    assert np.allclose(q[1], [1.2e-19, 0.375, 0.4375], rtol=1e-12)
    # row 2: (5e-9, 0.1, 0.1) -> (1.5e-8, 0.15, 0.1) -> (1.5e-8, 0.1, 0.1): the tie takes the smaller value
    assert np.allclose(q[2], [0.1, 0.1, 3 * want[2, 2]], rtol=1e-12)
    over = compare.Comparison(dict(c.planes(), p_min=np.full((3, 3), 1.0 + 2.0 ** -52)))
    assert np.all(over.p_value() == 1.0)                         # a tail that rounds above 1 is a P-value of 1


def test_best_lists_targets_by_p_value_with_their_alignment():
    best = hand_comparison().best(2)
    assert [[b["target"] for b in row] for row in best] == [[1, 0], [0, 1], [2, 0]]
    first = best[0][0]
    assert (first["name"], first["offset"], first["orient"], first["overlap"]) == ("t1", -2, 1, 7) and abs(first["e_value"] - 3 * first["p_value"]) < 1e-18
    assert len(hand_comparison().best(9)[0]) == 3


def test_groups_are_the_connected_components_under_the_threshold():
    n = 6
    p = np.ones((n, n))
    for i, j in ((0, 3), (3, 5), (4, 1)):                        # one direction is enough; 0-3-5 chain, 1-4 pair, 2 alone
        p[i, j] = 1e-6
    np.fill_diagonal(p, 1e-12)
    planes = dict(p_min=p, n_offsets=np.ones((n, n), dtype=np.int32), offset=np.zeros((n, n), dtype=np.int32), overlap=np.ones((n, n), dtype=np.int32),
                  score=np.zeros((n, n), dtype=np.int32), orient=np.zeros((n, n), dtype=np.int8))
    c = compare.Comparison(planes)
    assert c.groups(1e-5) == [[0, 3, 5], [1, 4], [2]]
    assert c.groups(1e-13) == [[i] for i in range(n)] and c.groups(1.0) == [list(range(n))]
    with pytest.raises(ValueError):
        compare.Comparison({k: v[:2] for k, v in planes.items()}).groups(0.1)


def test_compare_takes_probability_and_count_sets_and_refuses_log_odds():
    counts = MotifSet.from_matrices("pfm", [np.array([[8, 0, 1], [1, 9, 1], [1, 1, 7], [0, 0, 1]])])
    assert compare._ppm_set(counts, "queries").kind == "ppm"
    with pytest.raises(ValueError, match="log-odds"):
        compare.compare(counts.to_ppm().to_pwm(), counts)
    with pytest.raises(ValueError):
        compare.compare([np.zeros((4, 3))], counts)
    assert callable(MotifSet.compare)


# ------------------------------------------------------------------------------------------------ the plan under the sanitizers

@pytest.mark.skipif(shutil.which("g++") is None or shutil.which("make") is None, reason="needs g++ and make")
def test_plan_under_address_and_ub_sanitizers():
    asan = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    if not (os.path.isabs(asan) and os.path.exists(asan)):
        pytest.skip("the sanitizer runtimes are not installed on this box")
    subprocess.run(["make", "-s", "-C", CSRC, "compare_plan_asan"], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([BIN], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "compare_plan_asan: ok" in out.stdout, (out.stdout + out.stderr)[-4000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-4000:]
    assert int(out.stdout.split("(")[1].split()[0]) >= 100
