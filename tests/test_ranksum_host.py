"""
The host side of cutoff-free enrichment (ms_best_rank_sum, ms_best_count_passing; motifscan_amd.enrich): the numpy restatements pinned by
a brute-force pair count written here, the 128-bit tie sum, RankSum.z against exact rational arithmetic, the P-value against scipy where
it is installed, the exported symbols and what must fail loudly without a GPU.  No GPU.  tests/test_gpu_ranksum.py runs the device
against the same restatements.
"""
import ctypes
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from motifscan_amd import _lib, enrich

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VALUES = [float("nan"), float("-inf"), -0.0, 0.0, 0.25, 0.5, 1.0, -0.5]


def brute_force(xa, xb):
    """(u2, ties) by the definition: an O(na * nb) double loop with the NaN rule spelled out."""
    def cmp(x, y):                                        # -1, 0, 1; a NaN lies below every number and equals every other NaN
        xn, yn = x != x, y != y
        if xn or yn:
            return 0 if (xn and yn) else (-1 if xn else 1)
        return (x > y) - (x < y)
    u2 = 0
    for x in xa:
        for y in xb:
            c = cmp(x, y)
            u2 += 2 if c > 0 else (1 if c == 0 else 0)
    pooled, ties = list(xa) + list(xb), 0
    for x in pooled:                                      # every element adds t^2 - 1, t = the size of its tie group: t^3 - t per group
        t = sum(1 for y in pooled if cmp(x, y) == 0)
        ties += t * t - 1
    return u2, ties


def test_symbols_header_and_constants():
    with open(os.path.join(ROOT, "include", "motifscan_amd.h")) as fh:
        text = fh.read()
    table = text[:text.index("#ifndef MOTIFSCAN_AMD_H")]
    for name in ("ms_best_rank_sum", "ms_best_count_passing"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", text) and re.search(name + r"\s+no reference counterpart", table)
        assert hasattr(_lib.lib(), name)
    with open(os.path.join(ROOT, "include", "motifscan_amd_debug.h")) as fh:
        dbg = fh.read()
    assert re.search(r"\bint\s+ms_debug_ranksum_dims\s*\(\s*int32_t\s+out\[8\]\s*\)", dbg)
    assert re.search(r"\bint\s+ms_debug_ranksum_budget\s*\(\s*int64_t\s+elems\s*,\s*int64_t\s*\*\s*previous\s*\)", dbg)
    assert hasattr(_lib.lib(), "ms_debug_ranksum_dims") and hasattr(_lib.lib(), "ms_debug_ranksum_budget")
    d = _lib.ranksum_dims()                               # no device needed
    assert d["threads"] % 64 == 0
    for k in ("gather_elems", "rank_elems", "count_elems"):
        assert d[k] > 0 and d[k] % d["threads"] == 0
    assert d["budget"] == 1 << 27 and d["cut_chunk"] >= 1 and 1 <= d["segmented_max"] < d["budget"]
    prev = _lib.ranksum_budget(12345)
    try:
        assert _lib.ranksum_budget(777) == 12345
    finally:
        assert _lib.ranksum_budget(prev) == 777
    with pytest.raises(ValueError):
        _lib.ranksum_budget(-1)


def test_no_gpu_means_loud_failure_not_fallback():
    have_device = _lib.device_count() > 0
    u2, ties, counts, cut = np.zeros(1, dtype=np.int64), np.zeros(2, dtype=np.uint64), np.zeros(1, dtype=np.int64), np.zeros(1)
    rc_rank = _lib.lib().ms_best_rank_sum(None, None, None, None, 0, 1, 0, _lib.ptr(u2, ctypes.c_int64), _lib.ptr(ties, ctypes.c_uint64), None, None)
    rc_count = _lib.lib().ms_best_count_passing(None, None, _lib.ptr(cut, ctypes.c_double), 1, 0, 1, _lib.ptr(counts, ctypes.c_int64), None)
    if have_device:
        assert rc_rank == _lib.MS_ERR_INVALID and rc_count == _lib.MS_ERR_INVALID           # NULL handles
        return
    for rc in (rc_rank, rc_count):
        assert rc == _lib.MS_ERR_RUNTIME                  # no device: said before the handles are looked at
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _lib.check(_lib.lib().ms_best_rank_sum(None, None, None, None, 0, 1, 0, _lib.ptr(u2, ctypes.c_int64), _lib.ptr(ties, ctypes.c_uint64), None, None))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _lib.check(_lib.lib().ms_best_count_passing(None, None, _lib.ptr(cut, ctypes.c_double), 1, 0, 1, _lib.ptr(counts, ctypes.c_int64), None))

    from motifscan_amd import scanner

    class Genome:
        chrom_sizes = {"c": 12}

        def fetch_sequence(self, chrom, start, end):
            return "ACGTACGTACGT"[start:end]

    class Region:
        chrom, start, end, summit = "c", 0, 12, 6

    class Pwm:
        matrix, length, cutoffs = np.ones((4, 3)), 3, {"1e-4": 0.5}

    a, b = scanner.Scanner(Genome(), [Region()]), scanner.Scanner(Genome(), [Region()])
    with pytest.raises(RuntimeError):
        a.rank_sum([Pwm()], b)
    with pytest.raises(RuntimeError):
        a.count_regions_passing([Pwm()], [[0.5]])


def test_restatement_against_a_brute_force_pair_count():
    rng = np.random.default_rng(7)
    seen_empty = set()
    for _ in range(300):
        na, nb = int(rng.integers(0, 12)), int(rng.integers(0, 12))
        xa, xb = rng.choice(VALUES, size=na), rng.choice(VALUES, size=nb)
        got = enrich.rank_sum_host(xa, xb)
        want_u2, want_ties = brute_force(xa.tolist(), xb.tolist())
        assert (int(got.u2[0]), got.ties[0], got.na, got.nb) == (want_u2, want_ties, na, nb), (xa, xb)
        back = enrich.rank_sum_host(xb, xa)
        assert int(got.u2[0]) + int(back.u2[0]) == 2 * na * nb and back.ties == got.ties
        if na == 0 or nb == 0:
            assert int(got.u2[0]) == 0
            seen_empty.add((na == 0, nb == 0))
    assert len(seen_empty) >= 2                           # (empty groups were among the cases)


def test_restatement_takes_motif_rows():
    rng = np.random.default_rng(8)
    xa, xb = rng.choice(VALUES, size=(5, 9)), rng.choice(VALUES, size=(5, 4))
    got = enrich.rank_sum_host(xa, xb)
    assert len(got) == 5 and got.u2.dtype == np.int64
    for i in range(5):
        assert (int(got.u2[i]), got.ties[i]) == brute_force(xa[i].tolist(), xb[i].tolist())
    all_nan = enrich.rank_sum_host(np.full((1, 6), np.nan), np.full((1, 5), np.nan))         # an unscorable motif's row
    assert int(all_nan.u2[0]) == 6 * 5 and all_nan.ties[0] == 11 ** 3 - 11
    with pytest.raises(ValueError):
        enrich.rank_sum_host(np.zeros((2, 3)), np.zeros((3, 3)))


def test_tie_sum_beyond_64_bits():
    t = enrich.tie_sum([3_000_000])                       # one tie group of 3 000 000 cells without a winner
    assert t == 3_000_000 ** 3 - 3_000_000 == 26_999_999_999_997_000_000 and t > 1 << 64
    assert enrich.tie_sum([1, 1, 1]) == 0 and enrich.tie_sum([2, 3]) == 6 + 24 and enrich.tie_sum([]) == 0
    rs = enrich.RankSum([2_000_000 * 1_000_000], [t], 2_000_000, 1_000_000)                 # every pooled value tied: no variance
    assert rs.ties[0] == t and isinstance(rs.ties[0], int)
    assert rs.auroc()[0] == 0.5 and math.isnan(rs.z()[0]) and math.isnan(rs.p_value()[0])


def z_exact(u2, ties, na, nb):
    """z from the integers with rational arithmetic and ONE square root."""
    N = na + nb
    var = Fraction(na * nb, 12) * (N + 1 - Fraction(ties, N * (N - 1)))
    diff = Fraction(u2, 2) - Fraction(na * nb, 2)
    if diff == 0:
        return 0.0
    return math.copysign(math.sqrt(diff * diff / var), diff)


def test_z_against_exact_rational_arithmetic():
    rng = np.random.default_rng(9)
    checked = 0
    for _ in range(200):
        na, nb = int(rng.integers(1, 40)), int(rng.integers(1, 40))
        xa, xb = rng.choice(VALUES + [0.75, 2.0], size=na), rng.choice(VALUES, size=nb)
        rs = enrich.rank_sum_host(xa, xb)
        N = na + nb
        if rs.ties[0] == N ** 3 - N:
            assert math.isnan(rs.z()[0])
            continue
        want, got = z_exact(int(rs.u2[0]), rs.ties[0], na, nb), float(rs.z()[0])
        assert abs(got - want) <= 1e-12 * abs(want), (got, want)      # under ten roundings of 2^-53 each
        checked += 1
    assert checked > 150
    # the benchmark's size, ties beyond 2^64 in play
    na = nb = 1_000_000
    ties = enrich.tie_sum([1_500_000] + [1] * 500_000)
    u2 = na * nb + 123_456_789_012
    got, want = float(enrich.RankSum([u2], [ties], na, nb).z()[0]), z_exact(u2, ties, na, nb)
    assert want > 0 and abs(got - want) <= 1e-12 * want
    assert math.isnan(enrich.RankSum([0], [0], 0, 5).z()[0]) and math.isnan(enrich.RankSum([0], [0], 0, 5).auroc()[0])


def test_p_value_alternatives():
    rs = enrich.rank_sum_host(np.array([[0.9, 0.8, 0.7, 0.95, 0.4]]), np.array([[0.1, 0.2, 0.85, 0.3]]))
    z = float(rs.z()[0])
    assert z > 0
    g, l, t = (float(rs.p_value(a)[0]) for a in ("greater", "less", "two-sided"))
    assert abs(g + l - 1.0) < 1e-15 and abs(t - 2 * g) < 1e-15 and g < 0.5
    assert abs(g - 0.5 * math.erfc(z / math.sqrt(2))) == 0
    with pytest.raises(ValueError):
        rs.p_value("different")


def test_against_scipy_on_nan_free_input():
    stats = pytest.importorskip("scipy.stats")
    rng = np.random.default_rng(10)
    numbers = [v for v in VALUES if v == v and v != float("-inf")] + [0.125, 0.75]
    checked = 0
    for _ in range(60):
        na, nb = int(rng.integers(2, 60)), int(rng.integers(2, 60))
        xa, xb = rng.choice(numbers, size=na) + rng.choice([0.0, 0.3], size=na), rng.choice(numbers, size=nb)
        rs = enrich.rank_sum_host(xa, xb)
        if math.isnan(rs.z()[0]) or abs(rs.z()[0]) > 6:
            continue
        ref = stats.mannwhitneyu(xa, xb, alternative="greater", method="asymptotic", use_continuity=False)
        assert int(rs.u2[0]) == 2 * ref.statistic
        assert abs(float(rs.p_value("greater")[0]) - ref.pvalue) <= 1e-9 * ref.pvalue
        checked += 1
    assert checked > 30


def test_count_passing_host_at_the_rule_s_edges():
    s = 0.8125
    above = np.nextafter(s + 1e-10, np.inf)
    x = np.array([[s, np.nan, -np.inf, 0.2, s]])
    # a cutoff on the score passes; so does score + 1e-10 when the rounded subtraction gives >= -1e-10; the next double may not
    cut = np.array([[s, s + 1e-10, above, 0.2, 0.9, -5.0]])
    want = [[int(sum(1 for v in x[0] if v == v and (v - c) >= -1e-10)) for c in cut[0]]]
    got = enrich.count_passing_host(x, cut)
    assert got.dtype == np.int64 and got.tolist() == want
    assert got[0, 0] == 2 and got[0, 3] == 3 and got[0, 4] == 0 and got[0, 5] == 3          # -inf and NaN never pass
    assert got[0, 1] == (2 if s - (s + 1e-10) >= -1e-10 else 0) and got[0, 2] == (2 if s - above >= -1e-10 else 0)
    assert got[0, 1] >= got[0, 2]
    far = np.nextafter(s + 2e-10, np.inf)
    assert enrich.count_passing_host(x, [[far]])[0, 0] == 0
    assert enrich.count_passing_host(np.zeros((2, 0)), np.zeros((2, 3))).tolist() == [[0, 0, 0], [0, 0, 0]]
    assert enrich.count_passing_host([0.5, 0.1], [0.3]).tolist() == [[1]]                    # 1-D: one row, one cutoff
    for bad in ([[np.nan]], [[np.inf]]):
        with pytest.raises(ValueError):
            enrich.count_passing_host(x, bad)
    with pytest.raises(ValueError):
        enrich.count_passing_host(x, np.zeros((2, 1)))
