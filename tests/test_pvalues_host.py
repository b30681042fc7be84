"""
The host side of the analytic score distribution (ms_pwmset_score_distribution; motifscan_amd.pvalues), no GPU: the numpy restatement
of the contract (`pvalues.restate_distribution`) pinned to exact arithmetic -- integer counts of W-mers under a uniform background,
exact rationals under a non-uniform Markov background --, the bracket between the scan's raw sum and the integer score by enumeration
of every W-mer, P-value bounds and conservative cutoffs against enumeration, the background of a k-mer count, the "no device" answer,
and the plan's stand-alone program under ASan + UBSan (motifscan_amd/csrc/ms_scoredist_plan.h, tests/sanitize/scoredist_plan_asan.cpp).
tests/test_gpu_pvalues.py holds the device to the same restatement byte for byte.
"""
import itertools
import os
import re
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from motifscan_amd import _lib, pvalues, scoredist
from motifscan_amd.kmers import KmerCounts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "motifscan_amd", "csrc")
BIN = os.path.join(ROOT, "tests", "sanitize", "scoredist_plan_asan.bin")
UNIFORM = (np.full((1, 4), 0.25), np.ones(1))


def seeded_matrix(width, seed):
    """A log-odds-like matrix: Dirichlet columns against a flat background, five decimals as the reference keeps them."""
    rng = np.random.default_rng(seed)
    ppm = rng.dirichlet(np.full(4, 0.4), size=width).T
    return np.round(np.log2((ppm + 0.01) / 1.04 / 0.25), 5)


def holed_matrix(width, seed):
    """seeded_matrix with two entries of -inf (never a whole column)."""
    mat = seeded_matrix(width, seed)
    mat[0, width // 2] = -np.inf
    mat[3, 0] = -np.inf
    return mat


def background(order, seed):
    """A non-uniform (cond, init) of the order: every probability >= 0.05, so that no product of a few columns comes near underflow."""
    rng = np.random.default_rng(seed)
    C = 4 ** order
    cond = rng.dirichlet(np.full(4, 2.0), size=C) * 0.8 + 0.05
    init = rng.dirichlet(np.full(C, 2.0)) * 0.5 + 0.5 / C
    return cond, init


def all_words(W):
    """uint8 [4^W][W]: the base codes of every W-mer, in code order (first base most significant)."""
    return np.array(list(itertools.product(range(4), repeat=W)), dtype=np.uint8).reshape(4 ** W, W)


def word_scores(mat, n_bins, strand=1):
    """(S int64 [4^W] the integer score of every W-mer, -1 where it passes an absent entry -- relative to s0 --, step, s0) for the
    forward walk: plain enumeration over pvalues.quantise's grid."""
    step, s0, d = pvalues.quantise(mat, n_bins, strand)
    words = all_words(mat.shape[1])
    per = d[words, np.arange(mat.shape[1])[None, :]]
    return np.where((per < 0).any(axis=1), -1, per.sum(axis=1)), step, s0


def word_raw_sums(mat):
    """float64 [4^W]: the scan's forward raw sum of every W-mer (scoredist.window_raw_sums over the W-mers laid end to end: the windows
    at multiples of W)."""
    W = mat.shape[1]
    text = np.frombuffer(b"ACGT", dtype=np.uint8)[all_words(W)].tobytes()
    return scoredist.window_raw_sums(mat, text)[0][::W]


# ------------------------------------------------------------------------------------------------ the symbols, no device

def test_header_declares_the_entry_point_and_the_library_has_it():
    with open(os.path.join(ROOT, "include", "motifscan_amd.h")) as fh:
        text = fh.read()
    assert re.search(r"\bint\s+ms_pwmset_score_distribution\s*\(", text)
    assert re.search(r"#define\s+MS_SCOREDIST_MAX_ORDER\s+5\b", text) and re.search(r"#define\s+MS_SCOREDIST_MAX_BINS\s+\(1 << 20\)", text)
    assert (_lib.MS_SCOREDIST_MAX_ORDER, _lib.MS_SCOREDIST_MAX_BINS) == (5, 1 << 20)
    with open(os.path.join(ROOT, "include", "motifscan_amd_debug.h")) as fh:
        dbg = fh.read()
    for name in ("ms_debug_scoredist_dims", "ms_debug_scoredist_budget", "ms_debug_scoredist_force_global"):
        assert re.search(r"\bint\s+%s\s*\(" % name, dbg) and hasattr(_lib.lib(), name)


def test_dims_and_knobs_need_no_device():
    d = _lib.scoredist_dims()
    assert d["threads"] >= 64 and d["tile_bins"] % d["threads"] == 0
    assert 16 * d["lds_elems"] == 160 * 1024                     # both buffers of the largest LDS case fill a CU's LDS
    assert d["budget_mib"] >= 64
    assert _lib.lib().ms_debug_scoredist_dims(None) == _lib.MS_ERR_INVALID
    assert _lib.lib().ms_debug_scoredist_budget(-1, None) == _lib.MS_ERR_INVALID
    before = _lib.scoredist_budget(12345)
    assert _lib.scoredist_budget(before) == 12345 and _lib.scoredist_budget(before) == before
    was = _lib.scoredist_force_global(True)
    assert _lib.scoredist_force_global(was) is True and _lib.scoredist_force_global(was) is was


def test_no_gpu_means_loud_failure_before_any_validation():
    L = _lib.lib()
    args = (None, 7, 99, None, None, 0, None, None, None, None)  # every one of them invalid
    have_device = _lib.device_count() > 0
    rc = L.ms_pwmset_score_distribution(*args)
    if have_device:
        assert rc == _lib.MS_ERR_INVALID
        return
    assert rc == _lib.MS_ERR_RUNTIME
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _lib.check(rc)


# ------------------------------------------------------------------------------------------------ exact integers

@pytest.mark.parametrize("W, holes", [(1, False), (2, False), (6, False), (6, True), (8, False)])
def test_uniform_background_counts_the_words_of_every_integer_score_exactly(W, holes):
    mat = holed_matrix(W, 40 + W) if holes else seeded_matrix(W, 40 + W)
    n_bins = 256
    mass, step, s0 = pvalues.restate_distribution([mat], *UNIFORM, n_bins)
    S, st, z = word_scores(mat, n_bins)
    assert (step[0], s0[0]) == (st, z)
    counts = np.bincount(S[S >= 0], minlength=n_bins)
    assert len(counts) == n_bins                                  # the fit: no W-mer scores past the grid
    assert counts.sum() == (4 ** W if not holes else np.count_nonzero(S >= 0)) and (not holes or counts.sum() < 4 ** W)
    # 0.25 is a power of two and a count below 2^53 an exact double: every operation of the recurrence is exact
    assert (mass[0] * float(4 ** W)).tobytes() == counts.astype(np.float64).tobytes()


# ------------------------------------------------------------------------------------------------ exact rationals

def exact_distribution(mat, cond, init, n_bins, strand=1):
    """The definition in Fractions, from the doubles given: a list of n_bins Fractions."""
    _, _, d = pvalues.quantise(mat, n_bins, strand)
    C = len(init)
    order = {4 ** k: k for k in range(6)}[C]
    fc = [[Fraction(float(v)) for v in row] for row in np.asarray(cond).reshape(C, 4)]
    old = [{0: Fraction(float(v))} for v in init]
    for c in range(mat.shape[1]):
        new = [dict() for _ in range(C)]
        for x in range(C):
            for a in range(4):
                p, b = (0, a) if order == 0 else (a * (C // 4) + (x >> 2), x & 3)
                s = int(d[b, c])
                if s < 0 or fc[p][b] == 0:
                    continue
                for j, v in old[p].items():
                    if v != 0 and j + s < n_bins:
                        new[x][j + s] = new[x].get(j + s, 0) + v * fc[p][b]
        old = new
    out = [Fraction(0)] * n_bins
    for x in range(C):
        for i, v in old[x].items():
            out[i] += v
    return out


@pytest.mark.parametrize("order, W, n_bins, holes", [(0, 6, 64, False), (1, 5, 40, True), (2, 6, 48, False), (_lib.MS_SCOREDIST_MAX_ORDER, 3, 12, False),
                                                     (_lib.MS_SCOREDIST_MAX_ORDER, 4, 20, True)])
def test_markov_background_against_exact_rational_arithmetic(order, W, n_bins, holes):
    mat = holed_matrix(W, 60 + W + order) if holes else seeded_matrix(W, 60 + W + order)
    cond, init = background(order, 7 + order)
    assert cond.min() >= 0.05 and init.min() > 0 and 0.05 ** (W + 1) > 2.0 ** -900
    for strand in (1, 2):
        mass = pvalues.restate_distribution([mat], cond, init, n_bins, strand)[0][0]
        exact = exact_distribution(mat, cond, init, n_bins, strand)
        # derived, not measured: per column a value passes one product and at most three sums, four roundings; the context sum adds
        # 4^order - 1 more.  All terms are >= 0, so n roundings give a relative error of at most n u / (1 - n u) (Higham, Accuracy and
        # Stability of Numerical Algorithms, lemma 3.1)
        n = 4 * W + 4 ** order - 1
        u = Fraction(1, 2 ** 53)
        bound = n * u / (1 - n * u)
        worst = Fraction(0)
        for got, want in zip(mass.tolist(), exact):
            if want == 0:
                assert got == 0.0
                continue
            assert got > 0.0
            err = abs(Fraction(got) - want) / want
            worst = max(worst, err)
        print(f"order {order} W {W} strand {strand}: worst relative error {float(worst / u):.2f} u, bound {float(bound / u):.1f} u")
        assert worst <= bound
        assert abs(sum(exact) - 1) < Fraction(1, 10 ** 9) or holes


# ------------------------------------------------------------------------------------------------ the bracket, P-value bounds, cutoffs

@pytest.mark.parametrize("W, holes", [(1, False), (4, True), (8, False)])
def test_every_word_satisfies_the_bracket(W, holes):
    mat = holed_matrix(W, 80 + W) if holes else seeded_matrix(W, 80 + W)
    R = word_raw_sums(mat)
    for n_bins in (W + 3, 256, 1 << 20):
        S, step, s0 = word_scores(mat, n_bins)
        live = S >= 0
        assert np.array_equal(live, R > -np.inf)
        # exact: a double is a dyadic rational, so the comparison is made on integers -- R 2^k against step 2^k (S -+ ...)
        fs = Fraction(step)
        for r, s in zip(R[live].tolist(), (S[live] + s0).tolist()):
            assert fs * (s - 1) <= Fraction(r) <= fs * (s + W + 1), (n_bins, r, s)


@pytest.mark.parametrize("W, holes", [(5, False), (6, True)])
def test_p_value_bounds_enclose_the_enumerated_p_value_at_every_distinct_score(W, holes):
    mat = holed_matrix(W, 90 + W) if holes else seeded_matrix(W, 90 + W)
    R = word_raw_sums(mat)
    score = R / scoredist.max_raw_of(mat)
    for n_bins in (W + 3, 256, 1 << 14):
        dist = pvalues.ScoreDistribution.from_matrices([mat], *pvalues.restate_distribution([mat], *UNIFORM, n_bins))
        assert dist.bracket_ok[0]
        xs = np.unique(score[score > -np.inf])
        emp = (len(score) - np.searchsorted(np.sort(score), xs, side="left")) / float(4 ** W)     # exact: a count over a power of two
        lower, upper = dist.p_value_bounds(0, xs)
        assert np.all(lower <= emp) and np.all(emp <= upper)
        assert abs(dist.lost(0) - np.count_nonzero(score == -np.inf) / 4.0 ** W) < 1e-12


@pytest.mark.parametrize("W, holes", [(5, False), (6, True)])
def test_cutoffs_are_conservative_against_enumeration(W, holes):
    mat = holed_matrix(W, 90 + W) if holes else seeded_matrix(W, 90 + W)
    score = word_raw_sums(mat) / scoredist.max_raw_of(mat)
    p_values = ["0.25", "0.0625", "1e-2", "1e-3", "1e-9"]
    for n_bins in (W + 3, 256, 1 << 14):
        S, step, s0 = word_scores(mat, n_bins)
        dist = pvalues.ScoreDistribution.from_matrices([mat], *pvalues.restate_distribution([mat], *UNIFORM, n_bins))
        cut = dist.cutoffs(p_values)[0]
        assert cut["1e-9"] is None                               # no score of positive probability is that rare among 4^W words
        for p in p_values[:-1]:
            i = dist.cutoff_index(0, p)
            if cut[p] is None:
                assert i is None
                continue
            tail = dist.tail(0)
            assert tail[i] <= float(p) and (i == 0 or tail[i - 1] > float(p))
            passing = score >= cut[p]
            assert np.all(S[passing] >= i)                       # every word that passes has an integer score >= s0 + i*
            assert np.count_nonzero(passing) / 4.0 ** W <= float(p)


def test_unscorable_motifs_get_an_empty_row_and_no_cutoff():
    good = seeded_matrix(4, 5)
    column = good.copy()
    column[:, 1] = -np.inf                                       # a column without a finite entry
    mats = [good, -np.abs(good), column, np.where(np.arange(16).reshape(4, 4) == 5, np.nan, good)]
    mass, step, s0 = pvalues.restate_distribution(mats, *UNIFORM, 32)
    assert step[0] > 0 and not mass[1:].any() and not step[1:].any() and not s0[1:].any()
    dist = pvalues.ScoreDistribution.from_matrices(mats, mass, step, s0)
    assert dist.cutoffs(["1e-1"])[1] == {"1e-1": None} and np.isnan(dist.p_value_bounds(2, [0.5])[0]).all()
    assert list(dist.bracket_ok) == [True, False, False, False]


def test_strand_two_is_the_forward_walk_of_the_reverse_complement():
    # entries on a grid of 1/8: the column sums behind `step` are exact, so they do not depend on the order of the columns
    mat = np.round(holed_matrix(6, 17) * 8) / 8
    cond, init = background(2, 3)
    for n_bins in (9, 100):
        rev = pvalues.restate_distribution([mat], cond, init, n_bins, 2)
        fwd = pvalues.restate_distribution([np.ascontiguousarray(mat[::-1, ::-1])], cond, init, n_bins, 1)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(rev, fwd))
        assert rev[0].tobytes() != pvalues.restate_distribution([mat], cond, init, n_bins, 1)[0].tobytes()


def test_background_from_counts_against_hand_written_counts():
    occ = np.array([3, 0, 1, 0, 0, 0, 0, 0, 5, 5, 5, 5, 1, 2, 3, 4], dtype=np.int64)
    kc = KmerCounts(2, False, occ, None, 1, int(occ.sum()), 0, 0)
    cond, init = pvalues.background_from_counts(kc, pseudocount=1.0)
    assert cond.tolist() == [[4 / 8, 1 / 8, 2 / 8, 1 / 8], [0.25] * 4, [6 / 24] * 4, [2 / 14, 3 / 14, 4 / 14, 5 / 14]]
    assert init.tolist() == [8 / 50, 4 / 50, 24 / 50, 14 / 50]
    cond0, init0 = pvalues.background_from_counts(kc, pseudocount=0.0)
    assert cond0[1].tolist() == [0.25] * 4 and init0.tolist() == [4 / 34, 0.0, 20 / 34, 10 / 34]
    mono = KmerCounts(1, False, np.array([1, 2, 3, 2], dtype=np.int64), None, 1, 8, 0, 0)
    cond1, init1 = pvalues.background_from_counts(mono, pseudocount=0.5)
    assert cond1.tolist() == [[1.5 / 10, 2.5 / 10, 3.5 / 10, 2.5 / 10]] and init1.tolist() == [1.0]
    with pytest.raises(ValueError):
        pvalues.background_from_counts(KmerCounts(2, True, occ, None, 1, 0, 0, 0))
    with pytest.raises(ValueError):
        pvalues.background_from_counts(KmerCounts(7, False, np.zeros(4 ** 7, dtype=np.int64), None, 0, 0, 0, 0))


def test_restatement_refuses_what_the_library_refuses():
    mat = seeded_matrix(4, 1)
    for bad in (dict(n_bins=6), dict(n_bins=(1 << 20) + 1), dict(strand=3), dict(cond=np.full((1, 4), -0.25)), dict(init=np.array([np.inf])),
                dict(init=np.ones(2)), dict(cond=np.full((4, 4), 0.25))):
        kw = dict(cond=UNIFORM[0], init=UNIFORM[1], n_bins=16, strand=1)
        kw.update(bad)
        with pytest.raises(ValueError):
            pvalues.restate_distribution([mat], **kw)


# ------------------------------------------------------------------------------------------------ the plan under the sanitizers

@pytest.mark.skipif(shutil.which("g++") is None or shutil.which("make") is None, reason="needs g++ and make")
def test_plan_under_address_and_ub_sanitizers():
    asan = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    if not (os.path.isabs(asan) and os.path.exists(asan)):
        pytest.skip("the sanitizer runtimes are not installed on this box")
    subprocess.run(["make", "-s", "-C", CSRC, "scoredist_plan_asan"], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([BIN], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "scoredist_plan_asan: ok" in out.stdout, (out.stdout + out.stderr)[-4000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-4000:]
    assert int(out.stdout.split("(")[1].split()[0]) >= 100
