"""
ms_affinity_expected_counts (ms_expcounts.hip) on the GPU, against motifscan_amd.em: every case of tests/test_em_host.py (make_cases,
sized by ms_debug_expected_dims) is scanned once (ms_scan_affinity), counted once, and restated once on the host FROM THE DEVICE'S OWN
PLANES, so that only the second pass is compared:  |device - host| <= slack  cell by cell, slack being the number of terms under the
cell whose w * 2^32 lies within 2^-16 of an integer + 1/2 (em's docstring derives the band; tests/test_em_host.py asserts on the CPU
that at most 1 % of the non-zero cells of these cases have any).  n_regions is exact.

Against the mpmath reference the bound is |device - real sum| <= (terms under the cell) * (1/2 + 2^-16): rounding a term costs at most
1/2, and the float64 weight is within 2^-17 units of the real one.  test_device_is_within_the_derived_bound_of_the_real_sums prints the
largest ratio seen.
"""
import ctypes
import math

import numpy as np
import pytest

from motifscan_amd import _lib, em, scanner
from test_em_host import CASES, CLOSED_SEQS, INF, assert_invariants, assert_within_slack, check_refinement, closed_expected, consensus_matrix, planted_case, random_mat, random_seq

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _device():
    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible")
    _lib.set_device(0)


class Run:
    """One ms_scan_affinity over (mats, seqs) and its handles, for the expected-counts calls of a test."""

    def __init__(self, mats, seqs, strand=3, scale=1.0, max_n=-1):
        self.mats, self.seqs = [np.asarray(m, dtype=np.float64) for m in mats], list(seqs)
        self.pw, self.sq = _lib.PwmSet.from_matrices(self.mats), _lib.SeqSet.from_strings(self.seqs)
        self.res = _lib.scan_affinity(self.pw, self.sq, strand, scale, max_n)
        peak, total, n_terms, log_mean = self.res.cells()
        self.planes = (peak, total, log_mean, n_terms)

    def counts(self, prior=INF, motifs=slice(None), out=None):
        c, t, n = self.res.expected_counts(self.pw, self.sq, prior, motifs, out)
        m0, m1, _ = motifs.indices(len(self.mats))
        return em.ExpectedCounts(c, t, n, [m.shape[1] for m in self.mats[m0:m1]])

    def close(self):
        self.res.close()
        self.sq.close()
        self.pw.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def same_bytes(a, b):
    return all(getattr(a, k).tobytes() == getattr(b, k).tobytes() and getattr(a, k).shape == getattr(b, k).shape for k in ("counts", "total", "n_regions"))


_DEV, _HOST = {}, {}


def dev(name):
    """(ExpectedCounts of the device, the device's planes) of a case, made once."""
    if name not in _DEV:
        mats, seqs, strand, scale, max_n, prior = CASES[name]
        with Run(mats, seqs, strand, scale, max_n) as run:
            _DEV[name] = (run.counts(prior), run.planes)
    return _DEV[name]


def host(name):
    """(ExpectedCounts, slack) of the restatement over the device's planes, made once."""
    if name not in _HOST:
        mats, seqs, strand, scale, max_n, prior = CASES[name]
        _HOST[name] = em.expected_counts_host(mats, seqs, strand, scale, max_n, prior, planes=dev(name)[1])
    return _HOST[name]


@pytest.mark.parametrize("name", sorted(CASES))
def test_device_matches_the_restatement_over_its_own_planes(name):
    got, _ = dev(name)
    want, slack = host(name)
    assert got.counts.shape == want.counts.shape
    assert_invariants(got)
    assert_within_slack(got, want, slack)
    if name != "never":
        assert got.counts.any()
    print(f"{name}: {int((got.counts != 0).sum())} non-zero cells, {int((got.counts != want.counts).sum())} differ from the restatement")


def test_a_prior_of_minus_infinity_gives_nothing_but_the_region_count():
    got, planes = dev("never")
    assert not got.counts.any() and not got.total.any()
    assert np.array_equal(got.n_regions, (planes[3] > 0).sum(axis=1)) and got.n_regions.any()


def test_tiles_ranges_and_rows_alone():
    mats, seqs, strand, scale, max_n, prior = CASES["tiles"]
    full, _ = dev("tiles")
    want, slack = host("tiles")
    with Run(mats, seqs, strand, scale, max_n) as run:
        inside = run.counts(prior, slice(3, 6))                                # the range starts inside the second tile
        assert inside.counts.tobytes() == full.counts[3:6].tobytes() and inside.total.tobytes() == full.total[3:6].tobytes()
        assert inside.n_regions.tobytes() == full.n_regions[3:6].tobytes()
        assert_within_slack(inside, em.ExpectedCounts(want.counts[3:6], want.total[3:6], want.n_regions[3:6], want.widths[3:6]), slack[3:6])
        for i in range(len(mats)):                                             # a row computed alone: the same bytes
            alone = run.counts(prior, slice(i, i + 1))
            assert alone.counts.tobytes() == full.counts[i:i + 1].tobytes() and alone.total[0] == full.total[i] and alone.n_regions[0] == full.n_regions[i]
        assert same_bytes(run.counts(prior, slice(0, 0)), em.ExpectedCounts(full.counts[:0], full.total[:0], full.n_regions[:0], []))
    # the narrow motif behind the wide ones, in a set of its own: the row does not depend on the other motifs of the set
    with Run([mats[3]], seqs, strand, scale, max_n) as run:
        alone = run.counts(prior)
        assert alone.counts[0].tobytes() == full.counts[3, :3].tobytes() and alone.total[0] == full.total[3]


def test_the_grid_stride_loop_gives_the_same_bytes():
    dims = _lib.expected_dims()
    mats, seqs, strand, scale, max_n, prior = CASES["loop"]
    assert sum(max(1, -(-len(s) // dims["segment_windows"])) for s in seqs) > 2 * dims["waves"]
    full, _ = dev("loop")
    with Run(mats, seqs, strand, scale, max_n) as run:
        for cap in (1, 2):
            with _lib.expected_grid_cap(cap):
                assert same_bytes(run.counts(prior), full)
        assert same_bytes(run.counts(prior), full)                             # ... and two runs give the same bytes


def test_two_runs_give_the_same_bytes_and_shards_add_up_exactly():
    for name in ("segments", "minus_inf", "w65"):
        mats, seqs, strand, scale, max_n, prior = CASES[name]
        full, _ = dev(name)
        with Run(mats, seqs, strand, scale, max_n) as run:
            assert same_bytes(run.counts(prior), full)
        cut = len(seqs) // 3
        with Run(mats, seqs[:cut], strand, scale, max_n) as a, Run(mats, seqs[cut:], strand, scale, max_n) as b:
            ea, eb = a.counts(prior), b.counts(prior)
        assert np.array_equal(ea.counts + eb.counts, full.counts)
        assert np.array_equal(ea.total + eb.total, full.total) and np.array_equal(ea.n_regions + eb.n_regions, full.n_regions)


def test_minus_infinity_and_empty_rows():
    for name in ("minus_inf", "minus_inf_oops"):
        got, planes = dev(name)
        n_terms = planes[3]
        some, every, nan_row, half, inf_row, neg = range(6)
        assert got.total[some] > 0 and got.total[half] > 0 and got.total[neg] > 0               # the all-negative matrix is counted
        assert np.isneginf(planes[0][every][n_terms[every] > 0]).all()                          # every term of its cells is -inf:
        assert got.n_regions[every] == (n_terms[every] > 0).sum() > 0                           # ... they count as regions
        assert got.total[every] == 0 and not got.counts[every].any()                            # ... and add no weight
        for row in (nan_row, inf_row):
            assert got.n_regions[row] == 0 and got.total[row] == 0 and not got.counts[row].any()
        assert got.n_regions[neg] == (n_terms[neg] > 0).sum()


def test_closed_forms_are_exact_integers_on_the_device():
    counts, total = closed_expected()
    with Run([consensus_matrix()], CLOSED_SEQS) as run:
        got = run.counts(INF)
    assert np.array_equal(got.counts, counts) and got.total[0] == total and got.n_regions[0] == 3
    mat = np.round(np.random.default_rng(3).normal(size=(4, 5)), 2)
    with Run([mat], ["NNNNNN"]) as run:
        alln = run.counts(INF)
    assert np.array_equal(alln.counts[0, :, 4], np.full(5, 1 << 32)) and not alln.counts[0, :, :4].any() and alln.total[0] == 1 << 32
    with Run([np.zeros((4, 3))], ["ACGTACGTAC"]) as run:                        # 16 terms of raw 0: log_mean = 0
        assert [int(run.counts(p).total[0]) for p in (INF, -INF, 0.0)] == [1 << 32, 0, 1 << 31]


@pytest.mark.parametrize("name", ("w33", "w65", "segments_plus", "max_n_2", "minus_inf", "loop"))
def test_device_is_within_the_derived_bound_of_the_real_sums(name):
    mats, seqs, strand, scale, max_n, prior = CASES[name]
    got, planes = dev(name)
    _, real, n_contrib = em.expected_counts_reference(mats, seqs, strand, scale, max_n, prior, planes=planes)
    worst = 0.0
    for idx in np.argwhere(n_contrib > 0):
        i = tuple(idx)
        bound = int(n_contrib[i]) * (0.5 + 2.0 ** -16)
        err = abs(int(got.counts[i]) - real[i])
        assert err <= bound, (i, float(err), bound)
        worst = max(worst, float(err / bound))
    assert not got.counts[n_contrib == 0].any()
    print(f"{name}: {int((n_contrib > 0).sum())} cells, largest |device - real| / bound = {worst:.4f}")
    assert (n_contrib > 0).any()


def test_every_invalid_argument_of_the_header():
    L = _lib.lib()
    rng = np.random.default_rng(11)
    max_w = _lib.expected_dims()["max_width"]
    mats = [random_mat(rng, 4), random_mat(rng, max_w + 1), random_mat(rng, 6)]
    seqs = [random_seq(rng, max_w + 20), random_seq(rng, 30)]
    with Run(mats, seqs) as run, Run(mats[:2], seqs) as fewer_motifs, Run(mats, seqs[:1]) as fewer_regions:
        counts = np.zeros((3, max_w + 1, 5), dtype=np.int64)
        out = counts.ctypes.data_as(ctypes.c_void_p)

        def call(aff=run.res.h, pw=run.pw.h, sq=run.sq.h, prior=0.0, m0=0, m1=1, flags=0, dst=out):
            return L.ms_affinity_expected_counts(aff, pw, sq, prior, m0, m1, flags, dst, None, None, None)
        assert call() == _lib.MS_OK and counts[0].any()
        for kw in ({"aff": None}, {"pw": None}, {"sq": None}, {"dst": None}, {"flags": 1}, {"prior": math.nan}, {"m0": -1}, {"m0": 2, "m1": 1}, {"m1": 4},
                   {"pw": fewer_motifs.pw.h}, {"sq": fewer_regions.sq.h}, {"aff": fewer_motifs.res.h}, {"aff": fewer_regions.res.h},
                   {"m0": 0, "m1": 3}, {"m0": 1, "m1": 2}):                     # the motif of max_width + 1 columns inside the range
            assert call(**kw) == _lib.MS_ERR_INVALID, kw
            assert _lib.lib().ms_last_error()
        with pytest.raises(ValueError, match="columns"):
            run.counts(0.0, slice(1, 3))
        assert call(m0=2, m1=3) == _lib.MS_OK                                  # the same motif outside the range is fine
        assert call(m0=1, m1=1, dst=None) == _lib.MS_OK and call(m0=3, m1=3) == _lib.MS_OK      # m0 == m1 does nothing
        third = run.counts(0.0, slice(2, 3))
        want, slack = em.expected_counts_host([mats[2]], seqs, 3, 1.0, -1, 0.0, planes=tuple(p[2:3] for p in run.planes))
        assert third.counts.shape == (1, max_w + 1, 5) and np.all(np.abs(third.counts[:, :6] - want.counts) <= slack) and not third.counts[:, 6:].any()
        with pytest.raises(ValueError, match="NaN"):
            run.counts(math.nan)
        with pytest.raises(ValueError, match="slice"):
            run.res.expected_counts(run.pw, run.sq, 0.0, slice(0, 3, 2))
        with pytest.raises(ValueError, match="out"):
            run.res.expected_counts(run.pw, run.sq, 0.0, slice(0, 1), out=(np.zeros((1, 3, 5), dtype=np.int64), None, None))


def test_outputs_in_device_memory_equal_the_host_ones():
    import torch
    mats, seqs, strand, scale, max_n, prior = CASES["loop"]
    full, _ = dev("loop")
    C = full.counts.shape[1]
    with Run(mats, seqs, strand, scale, max_n) as run:
        bufs = [torch.full(shape, -1, dtype=torch.int64, device="cuda") for shape in ((2, C, 5), (2,), (2,))]
        torch.cuda.synchronize()                                  # the fills run on torch's stream, the library writes on its own
        ptrs = tuple(int(t.data_ptr()) for t in bufs)
        back = run.res.expected_counts(run.pw, run.sq, prior, slice(1, 3), out=ptrs)
        assert back == ptrs
        torch.cuda.synchronize()
        for h, t in zip((full.counts[1:3], full.total[1:3], full.n_regions[1:3]), bufs):
            assert np.ascontiguousarray(h).tobytes() == t.cpu().numpy().tobytes() and h.any()
        mixed = run.res.expected_counts(run.pw, run.sq, prior, slice(1, 3), out=(None, ptrs[1], None))      # host counts, device total
        assert mixed[0].tobytes() == np.ascontiguousarray(full.counts[1:3]).tobytes() and mixed[1] == ptrs[1]


def test_refine_recovers_the_planted_motif_on_the_device():
    seed, seqs, planted, bg = planted_case()
    res = em.refine([seed], seqs, iters=4, gamma=0.5, strand=3, bg=bg, pseudo=0.01, device=True, keep=True)
    check_refinement(res, planted, bg)
    for it, step in enumerate(res.steps):                          # the device's counts for the device's current matrix and planes
        prior = em.prior_logit_of(step["gamma"][0])
        want, slack = em.expected_counts_host(step["mats"], seqs, 3, 1.0, -1, prior, planes=step["planes"][0])
        assert_invariants(step["expected"])
        assert_within_slack(step["expected"], want, slack)
        assert step["expected"].total[0] > 0, it
    assert res.log_likelihood.shape == (4, 1) and np.all(np.isfinite(res.log_likelihood))


def test_through_a_scanner_on_one_strand():
    rng = np.random.default_rng(5)
    chrom = random_seq(rng, 700, 0.01)

    class Genome:
        chrom_sizes = {"chr1": len(chrom)}

        def fetch_sequence(self, name, start, end):
            return chrom[start:end]

    class Region:
        def __init__(self, start, end):
            self.chrom, self.start, self.end, self.summit = "chr1", start, end, (start + end) // 2

    class Pwm:
        def __init__(self, mat):
            self.matrix, self.length, self.cutoffs = mat, mat.shape[1], None
    mats = [random_mat(rng, 6, 6.0), random_mat(rng, 11, 6.0)]
    pwms = [Pwm(m) for m in mats]
    sc = scanner.Scanner(Genome(), [Region(s, s + n) for s, n in ((0, 90), (100, 5), (150, 200), (400, 11), (420, 280))], strand="+")
    seqs = list(sc.sequences)
    assert [len(s) for s in seqs] == [90, 5, 200, 11, 280]
    for gamma, prior in ((None, INF), (0.3, math.log(0.3 / 0.7))):
        got = sc.expected_counts(pwms, gamma=gamma, scale=1.0, max_n=1)
        with Run(mats, seqs, 1, 1.0, 1) as plus, Run(mats, seqs, 3, 1.0, 1) as both:
            want, other = plus.counts(prior), both.counts(prior)
        assert isinstance(got, em.ExpectedCounts) and same_bytes(got, want) and got.widths.tolist() == [6, 11] and got.counts.any()
        assert not np.array_equal(got.counts, other.counts)                     # the scanner's strand is honoured
    mine = sc.refine_motifs(pwms, iters=2, gamma=0.4, max_n=1, pseudo=0.02)
    direct = em.refine(mats, seqs, iters=2, gamma=0.4, strand=1, max_n=1, pseudo=0.02, device=True)
    both = em.refine(mats, seqs, iters=2, gamma=0.4, strand=3, max_n=1, pseudo=0.02, device=True)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(mine.mats, direct.mats)) and mine.gammas.tobytes() == direct.gammas.tobytes()
    assert mine.log_likelihood.tobytes() == direct.log_likelihood.tobytes() and mine.log_likelihood.shape == (2, 2)
    assert not all(np.array_equal(a, b) for a, b in zip(mine.mats, both.mats))
    sc.close()
