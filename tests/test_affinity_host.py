"""
The host side of the affinity scan (ms_scan_affinity; motifscan_amd.affinity, _lib.scan_affinity / Affinity, Scanner.affinity /
Scanner.affinity_rank_sum): the numpy restatement against the mpmath reference on hand-written and seeded random cases, what must fail
loudly without a GPU, and the argument checks that come before any library call.  No GPU.

The bound on `sum` is the one the device test uses (DESIGN.md has the derivation): |S - S_ref| <= 16 (n_terms + 8) 2^-53 S_ref.
"""
import ctypes
import math

import numpy as np
import pytest

from motifscan_amd import _lib, affinity, scanner, scoredist

LN2 = math.log(2.0)


def bound(n_terms, s_ref):
    return 16.0 * (n_terms + 8.0) * 2.0 ** -53 * s_ref


def check_against_reference(mats, seqs, strand, scale=1.0, max_n=-1):
    got = affinity.affinity_host(mats, seqs, strand, scale, max_n)
    ref = affinity.affinity_reference(mats, seqs, strand, scale, max_n, as_mpf=True)
    assert np.array_equal(got.n_terms, ref.n_terms) and got.n_terms.dtype == np.int32
    assert np.array_equal(got.peak, ref.peak, equal_nan=True)
    worst = 0.0
    for m in range(len(mats)):
        for r in range(len(seqs)):
            s_ref = ref.sum[m, r]
            if s_ref == 0:
                assert got.sum[m, r] == 0.0
                continue
            err = abs(got.sum[m, r] - s_ref)
            assert err <= bound(int(got.n_terms[m, r]), s_ref), (m, r, float(err), float(s_ref))
            worst = max(worst, float(err / bound(int(got.n_terms[m, r]), s_ref)))
            assert 1.0 - 1e-12 <= got.sum[m, r] <= got.n_terms[m, r] * (1.0 + 1e-12)
    # log_mean from the planes, one ulp each for the divide, the log, the multiply and the add
    with np.errstate(all="ignore"):
        want = scale * got.peak + np.log(got.sum / np.maximum(got.n_terms, 1))
        tol = 8.0 * 2.0 ** -53 * (np.abs(scale * got.peak) + np.abs(np.log(got.sum / np.maximum(got.n_terms, 1))) + 1.0)
        diff = np.abs(got.log_mean - want)
    special = (got.n_terms == 0) | np.isneginf(got.peak)
    assert np.all(np.isnan(got.log_mean[got.n_terms == 0]))
    assert np.all(np.isneginf(got.log_mean[(got.n_terms > 0) & np.isneginf(got.peak)]))
    assert np.all(diff[~special] <= tol[~special])
    return got, worst


def random_case(seed):
    rng = np.random.default_rng(seed)
    mats = []
    for _ in range(int(rng.integers(1, 5))):
        W = int(rng.integers(1, 40))
        m = rng.normal(0.0, 1.5, size=(4, W))
        kind = rng.integers(0, 8)
        if kind == 0:
            m[rng.integers(0, 4), rng.integers(0, W)] = -np.inf
        elif kind == 1:
            m = -np.abs(m) - 0.1                                      # all-negative: scored here
        elif kind == 2:
            m[rng.integers(0, 4), rng.integers(0, W)] = np.nan if rng.integers(0, 2) else np.inf
        mats.append(m)
    seqs = []
    for _ in range(int(rng.integers(1, 5))):
        L = int(rng.integers(0, 90))
        s = rng.choice(list("ACGTacgtNnR"), p=[.2, .2, .2, .2, .03, .03, .03, .03, .04, .02, .02], size=L)
        seqs.append("".join(s))
    strand = int(rng.integers(1, 4))
    scale = [0.5, 1.0, LN2, 3.0][int(rng.integers(0, 4))]
    max_n = [-1, -1, 0, 1, 3][int(rng.integers(0, 5))]
    return mats, seqs, strand, scale, max_n


def test_restatement_matches_the_reference_on_seeded_random_cases():
    worst, cells = 0.0, 0
    for seed in range(40):
        mats, seqs, strand, scale, max_n = random_case(1000 + seed)
        got, w = check_against_reference(mats, seqs, strand, scale, max_n)
        worst = max(worst, w)
        cells += got.peak.size
        for m, mat in enumerate(mats):                                # peak = the maximum of window_raw_sums, bit for bit
            for r, seq in enumerate(seqs):
                fwd, rev, n_non = scoredist.window_raw_sums(mat, seq)
                keep = np.ones(len(fwd), dtype=bool) if max_n < 0 else n_non <= max_n
                terms = np.concatenate([x[keep] for s, x in ((1, fwd), (2, rev)) if strand & s])
                if affinity.empty_row(mat) or len(terms) == 0:
                    assert got.n_terms[m, r] == 0 and np.isnan(got.peak[m, r]) and got.sum[m, r] == 0.0
                else:
                    assert got.n_terms[m, r] == len(terms)
                    assert got.peak[m, r].tobytes() == terms.max().tobytes()
    print(f"{cells} cells, largest error / bound = {worst:.4f}")
    assert cells > 150


def test_two_windows_give_one_plus_exp_minus_d():
    d = 1.75
    mat = np.array([[0.0], [-d], [-9.0], [-9.0]])                       # one column: A scores 0, C scores -d
    for scale in (0.5, 1.0, LN2):
        got, _ = check_against_reference([mat], ["AC"], 1, scale)
        assert got.n_terms[0, 0] == 2 and got.peak[0, 0] == 0.0
        assert got.sum[0, 0] == pytest.approx(1.0 + math.exp(-scale * d), rel=4e-16)
        assert got.log_mean[0, 0] == pytest.approx(math.log((1.0 + math.exp(-scale * d)) / 2.0), rel=1e-15)
        arr = affinity.AffinityArrays(got.peak, got.sum, got.n_terms, got.log_mean)
        assert arr.log_sum()[0, 0] == pytest.approx(math.log(1.0 + math.exp(-scale * d)), rel=1e-15)
        assert arr.mean_odds()[0, 0] == pytest.approx((1.0 + math.exp(-scale * d)) / 2.0, rel=1e-15)


def test_palindromic_motif_on_both_strands_doubles_the_sum():
    half = np.array([[1.0, -0.5], [-1.0, 0.25], [0.5, -2.0], [-0.75, 0.125]])
    pal = np.concatenate([half, half[::-1, ::-1]], axis=1)              # M[3 - b][W - 1 - c] == M[b][c]
    assert np.array_equal(pal[::-1, ::-1], pal)
    seq = "ACGTTGCAAGGTCCATnACGT"
    one, _ = check_against_reference([pal], [seq], 1)
    rev, _ = check_against_reference([pal], [seq], 2)
    both, _ = check_against_reference([pal], [seq], 3)
    assert np.array_equal(one.peak, rev.peak) and np.array_equal(one.peak, both.peak)
    assert both.n_terms[0, 0] == 2 * one.n_terms[0, 0]
    assert both.sum[0, 0] == pytest.approx(2.0 * one.sum[0, 0], rel=1e-14)
    assert both.log_mean[0, 0] == pytest.approx(one.log_mean[0, 0], abs=1e-14)


def test_short_regions_minus_infinity_and_the_all_negative_matrix():
    mat = np.array([[-np.inf, 0.5, 0.1], [0.2, -0.3, 0.4], [0.3, 0.1, -0.2], [0.1, 0.2, 0.3]])      # an A in column 0 kills the '+' window
    got, _ = check_against_reference([mat], ["AC", "", "AAAAAA", "ACAGTC", "CCGG"], 1)
    assert got.n_terms[0].tolist() == [0, 0, 4, 4, 2]
    assert np.isnan(got.peak[0, 0]) and got.sum[0, 0] == 0.0 and np.isnan(got.log_mean[0, 0])          # L < W
    assert np.isneginf(got.peak[0, 2]) and got.sum[0, 2] == 0.0 and np.isneginf(got.log_mean[0, 2])     # every term -inf
    assert np.isfinite(got.peak[0, 3]) and 1.0 <= got.sum[0, 3] <= 2.0 + 1e-12                          # windows 0 and 2 are -inf: two numbers left
    assert got.sum[0, 4] > 1.0
    neg = -np.array([[0.5, 1.0], [0.25, 2.0], [1.5, 0.125], [3.0, 0.75]])
    assert not scoredist.scorable(neg) and not affinity.empty_row(neg)           # NaN everywhere in ms_scan_best, scored here
    got, _ = check_against_reference([neg], ["ACGTAC"], 3)
    assert got.n_terms[0, 0] == 10 and got.peak[0, 0] < 0 and got.sum[0, 0] > 1.0 and np.isfinite(got.log_mean[0, 0])
    for bad in (np.nan, np.inf):
        m = np.ones((4, 2))
        m[1, 1] = bad
        got, _ = check_against_reference([m, neg], ["ACGTAC"], 3)
        assert got.n_terms[0, 0] == 0 and np.isnan(got.peak[0, 0]) and got.sum[0, 0] == 0.0 and np.isnan(got.log_mean[0, 0])
        assert got.n_terms[1, 0] == 10


def test_max_n_lower_case_and_n_bases():
    mat = np.array([[1.0, -1.0, 0.5, 0.25], [0.5, 0.75, -0.5, 1.0], [-1.0, 0.25, 1.5, -0.75], [0.125, -2.0, 0.375, 0.5]])
    seq = "ACGNNTACGTAC"                                                  # the windows at 0 .. 4 hold 1, 2, 2, 2, 1 non-ACGT bases
    n_non = scoredist.window_raw_sums(mat, seq)[2]
    assert n_non.tolist() == [1, 2, 2, 2, 1, 0, 0, 0, 0]
    counts = {}
    for max_n in (-1, 0, 1, 2, 3):
        got, _ = check_against_reference([mat], [seq], 3, 1.0, max_n)
        counts[max_n] = int(got.n_terms[0, 0])
    assert counts == {-1: 18, 0: 8, 1: 12, 2: 18, 3: 18}                  # on the count (2) every window is a term, one below (1) three are dropped
    upper, _ = check_against_reference([mat], [seq], 3)
    lower, _ = check_against_reference([mat], [seq.lower()], 3)
    mixed, _ = check_against_reference([mat], ["acGnNtACgtAc"], 3)
    for other in (lower, mixed):
        assert all(np.array_equal(getattr(upper, k), getattr(other, k)) for k in ("peak", "sum", "n_terms", "log_mean"))
    alln, _ = check_against_reference([mat], ["NNNNNN"], 3)
    assert alln.n_terms[0, 0] == 6 and alln.peak[0, 0] == 0.0 and alln.sum[0, 0] == 6.0 and alln.log_mean[0, 0] == 0.0     # a base that adds nothing: raw = 0
    none, _ = check_against_reference([mat], ["NNNNNN"], 3, 1.0, 0)
    assert none.n_terms[0, 0] == 0 and np.isnan(none.peak[0, 0])


def test_scale_is_the_exponent_s_factor():
    mat = np.array([[1.0, -1.0, 0.5], [0.5, 0.75, -0.5], [-1.0, 0.25, 1.5], [0.125, -2.0, 0.375]])
    seq = "ACGTTGCATGCAAGCT"
    fwd = scoredist.window_raw_sums(mat, seq)[0]
    for scale in (0.5, 1.0, LN2):
        got, _ = check_against_reference([mat], [seq], 1, scale)
        want = sum(math.exp(scale * (x - fwd.max())) for x in fwd.tolist())
        assert got.sum[0, 0] == pytest.approx(want, rel=1e-14)
    log2mat = mat / LN2                                                  # the same motif as a log2 matrix, read with scale = ln 2
    a, _ = check_against_reference([mat], [seq], 3, 1.0)
    b, _ = check_against_reference([log2mat], [seq], 3, LN2)
    assert b.log_mean[0, 0] == pytest.approx(a.log_mean[0, 0], rel=1e-13)
    for bad in (0.0, -1.0, math.inf, math.nan, "x", None):
        with pytest.raises(ValueError, match="scale"):
            affinity.affinity_host([mat], [seq], 3, bad)
    for bad in (-2, 1.5, None, True):
        with pytest.raises(ValueError, match="max_n"):
            affinity.affinity_host([mat], [seq], 3, 1.0, bad)
    with pytest.raises(ValueError, match="strand"):
        affinity.affinity_host([mat], [seq], 0)
    with pytest.raises(ValueError, match="prec"):
        affinity.affinity_reference([mat], [seq], 3, prec=64)


def test_no_gpu_means_loud_failure_not_fallback():
    L = _lib.lib()
    dims = _lib.affinity_dims()                                          # the symbols exist, with or without a device
    assert dims["segment_windows"] == 64 * dims["strips"] >= 64 and dims["tile_entries"] == 4 * dims["tile_max_width"] and dims["waves"] >= 1
    assert dims["part_bytes"] == 24
    if _lib.device_count() > 0:
        pytest.skip("a GPU is visible")
    pw = _lib.PwmSet.from_matrices([np.ones((4, 3))])
    h = ctypes.c_void_p()
    rc = L.ms_scan_affinity(pw.h, None, 3, 1.0, -1, 0, ctypes.byref(h))     # no device: said before the handles are looked at
    assert rc == _lib.MS_ERR_RUNTIME and not h.value
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _lib.check(rc)
    rc = L.ms_affinity_rank_sum(None, None, None, None, 0, 0, 0, None, None, None, None)
    assert rc == _lib.MS_ERR_RUNTIME
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _lib.check(rc)

    class Handle:
        h = None
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _lib.scan_affinity(pw, Handle(), 3)
    pw.close()
    sc = _scanner()
    with pytest.raises(RuntimeError):
        sc.affinity([_Pwm()])
    with pytest.raises(RuntimeError):
        sc.affinity_rank_sum([_Pwm()], _scanner())


class _Pwm:
    matrix, length, cutoffs = np.ones((4, 3)), 3, None


def _scanner():
    class Region:
        chrom, start, end, summit = "chr1", 2, 12, 7

    class Genome:
        chrom_sizes = {"chr1": 20}

        def fetch_sequence(self, chrom, start, end):
            return "ACGTACGTACGTACGTACGT"[start:end]
    return scanner.Scanner(Genome(), [Region()])


def test_arguments_are_checked_before_any_library_call(monkeypatch):
    class Handle:
        h, n = None, 0
    for mask in (0, 4, -1):
        with pytest.raises(ValueError, match="strand mask"):
            _lib.scan_affinity(Handle(), Handle(), mask)
    with pytest.raises(ValueError, match="flags"):
        _lib.scan_affinity(Handle(), Handle(), 3, flags=1)
    for bad in (0.0, -2.0, math.inf, math.nan):
        with pytest.raises(ValueError, match="scale"):
            _lib.scan_affinity(Handle(), Handle(), 3, scale=bad)
    with pytest.raises(ValueError, match="max_n"):
        _lib.scan_affinity(Handle(), Handle(), 3, max_n=-2)

    def no_library_call(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib.PwmSet, "from_matrices", staticmethod(no_library_call))
    monkeypatch.setattr(_lib, "scan_affinity", no_library_call)
    sc, ctl = _scanner(), _scanner()
    for kw in ({"scale": 0.0}, {"scale": math.nan}, {"scale": -1.0}, {"scale": math.inf}, {"max_n": -2}, {"max_n": 0.5}):
        with pytest.raises(ValueError):
            sc.affinity([_Pwm()], **kw)
        with pytest.raises(ValueError):
            sc.affinity_rank_sum([_Pwm()], ctl, **kw)
    with pytest.raises(ValueError, match="Scanner"):
        sc.affinity_rank_sum([_Pwm()], object())
    with pytest.raises(ValueError, match="one flag per region"):
        sc.affinity_rank_sum([_Pwm()], ctl, sel=[1, 0])
    with pytest.raises(ValueError, match="one flag per region"):
        sc.affinity_rank_sum([_Pwm()], ctl, sel_control=[[1]])
