"""
ms_pwmset_score_distribution (ms_scoredist.hip) on the GPU: the analytic score distribution under a Markov background, held byte for
byte (mass, step, s0) to the numpy restatement (`pvalues.restate_distribution`, which tests/test_pvalues_host.py pins to exact
arithmetic).  The sizes come from ms_debug_scoredist_dims: the bin tile of the global path and its neighbours, the largest contexts x
bins the LDS path takes and one above it.  Path (ms_debug_scoredist_force_global), batch size (ms_debug_scoredist_budget), the place of
the output and what recycled memory holds change no byte.  One test ties the distribution to the scan's own arithmetic on all 4^5
pentamers.
"""
import ctypes

import numpy as np
import pytest

from motifscan_amd import _lib, pvalues, scoredist
from test_pvalues_host import UNIFORM, all_words, background, holed_matrix, seeded_matrix, word_scores

pytestmark = pytest.mark.gpu

WIDE = 257            # a set takes any width; one past the widest motif the other dense entry points take


def device_run(mats, cond, init, n_bins, strand=1, out=None, timing=None):
    order = {4 ** k: k for k in range(6)}[np.asarray(init).size]
    pw = _lib.PwmSet.from_matrices(mats)
    try:
        return _lib.score_distribution(pw, strand, order, cond, init, n_bins, out=out, timing=timing)
    finally:
        pw.close()


def same_bytes(got, want):
    return all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip(got, want))


def edge_matrices():
    """W = 1, a wide motif, a column of four equal entries (shift 0), a column whose shift is the whole range, entries of -inf, and an
    unscorable motif between scorable ones."""
    flat = seeded_matrix(5, 11)
    flat[:, 2] = 0.75
    one_column = np.full((4, 3), 0.5)
    one_column[:, 1] = [-3.0, 1.0, 0.25, -1.5]
    return [seeded_matrix(1, 1), seeded_matrix(WIDE, 2), flat, -np.abs(seeded_matrix(6, 3)), one_column, holed_matrix(7, 4), seeded_matrix(9, 5)]


@pytest.fixture(scope="module")
def dims():
    return _lib.scoredist_dims()


@pytest.fixture(scope="module")
def small():
    """Five narrow motifs (one unscorable, one with holes) under an order-1 background, and their restatement at the LDS path's size."""
    mats = [seeded_matrix(4, 21), holed_matrix(6, 22), -np.abs(seeded_matrix(3, 23)), seeded_matrix(9, 24), seeded_matrix(2, 25)]
    cond, init = background(1, 5)
    return dict(mats=mats, cond=cond, init=init, n_bins=200, want=pvalues.restate_distribution(mats, cond, init, 200, 1))


# ------------------------------------------------------------------------------------------------ 1. widths and columns

@pytest.mark.parametrize("strand", [1, 2])
def test_widths_and_columns(strand):
    mats = edge_matrices()
    for (cond, init), n_bins in ((UNIFORM, WIDE + 3), (background(0, 2), 1500), (background(1, 3), 700)):
        want = pvalues.restate_distribution(mats, cond, init, n_bins, strand)
        assert want[1][3] == 0 and not want[0][3].any() and np.count_nonzero(want[1]) == len(mats) - 1
        got = device_run(mats, cond, init, n_bins, strand)
        assert same_bytes(got, want)
        d = pvalues.quantise(mats[4], n_bins, strand)[2]
        assert d.max() == n_bins - 3 - 2 and sorted(d[:, 0].tolist()) == [0, 0, 0, 0]      # the whole range in one column's shift
    step, s0 = got[1], got[2]
    assert step[0] > 0 and s0.dtype == np.int64


def test_an_empty_set_is_valid():
    mass, step, s0 = device_run([], *UNIFORM, 16)
    assert mass.shape == (0, 16) and step.shape == (0,) and s0.shape == (0,)


# ------------------------------------------------------------------------------------------------ 2. bin counts, orders, strand

def test_bin_counts_around_the_tile_and_the_lds_limit(dims):
    mats = [seeded_matrix(9, 31), holed_matrix(4, 32), seeded_matrix(1, 33)]
    tile, lds = dims["tile_bins"], dims["lds_elems"]
    b0, b1 = background(0, 8), background(1, 9)
    cases = [(b0, 12), (b0, tile - 1), (b0, tile), (b0, tile + 1), (b0, 2 * tile + 1), (b0, lds), (b0, lds + 1), (b1, lds // 4), (b1, lds // 4 + 1)]
    assert lds % 4 == 0 and lds > 2 * tile + 1
    for (cond, init), n_bins in cases:
        want = pvalues.restate_distribution(mats, cond, init, n_bins, 1)
        assert same_bytes(device_run(mats, cond, init, n_bins, 1), want), n_bins
        before = _lib.scoredist_force_global(True)
        try:
            assert same_bytes(device_run(mats, cond, init, n_bins, 1), want), n_bins
        finally:
            _lib.scoredist_force_global(before)


@pytest.mark.parametrize("order, n_bins", [(0, 300), (1, 200), (2, 100), (3, 161), (4, 64), (_lib.MS_SCOREDIST_MAX_ORDER, 64)])
def test_every_order_both_strands(order, n_bins, dims):
    mats = [seeded_matrix(5, 41), holed_matrix(8, 42), seeded_matrix(3, 43)]
    cond, init = background(order, 50 + order)
    assert order < 3 or 4 ** order * n_bins > dims["lds_elems"]          # the high orders take the global path, the low ones LDS
    for strand in (1, 2):
        want = pvalues.restate_distribution(mats, cond, init, n_bins, strand)
        assert same_bytes(device_run(mats, cond, init, n_bins, strand), want)
    assert abs(want[0][0].sum() - init.sum()) < 1e-12                    # no hole: all the mass arrives


# ------------------------------------------------------------------------------------------------ 3. paths, batches, output memory

def test_path_and_batch_size_change_no_byte(small, dims):
    mats, cond, init, n_bins, want = (small[k] for k in ("mats", "cond", "init", "n_bins", "want"))
    assert 4 * n_bins <= dims["lds_elems"]
    assert same_bytes(device_run(mats, cond, init, n_bins), want)
    per_motif = 2 * 4 * n_bins * 8
    for force in (False, True):
        was = _lib.scoredist_force_global(force)
        try:
            for budget in (per_motif, 3 * per_motif + 8, 0):             # batches of one motif, of three, the library's own
                before = _lib.scoredist_budget(budget)
                try:
                    assert same_bytes(device_run(mats, cond, init, n_bins), want), (force, budget)
                finally:
                    _lib.scoredist_budget(before)
        finally:
            _lib.scoredist_force_global(was)


def test_device_output(small):
    import torch
    mats, cond, init, n_bins, want = (small[k] for k in ("mats", "cond", "init", "n_bins", "want"))
    for force in (False, True):
        was = _lib.scoredist_force_global(force)
        try:
            dev = torch.full((len(mats), n_bins), -1.0, dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()                              # the fill runs on torch's stream, the library writes on its own
            timing = {}
            out, step, s0 = device_run(mats, cond, init, n_bins, out=int(dev.data_ptr()), timing=timing)
            torch.cuda.synchronize()
            assert out == int(dev.data_ptr()) and timing["device_ms"] > 0
            assert same_bytes((dev.cpu().numpy(), step, s0), want)
        finally:
            _lib.scoredist_force_global(was)
    into = np.full((len(mats), n_bins), -1.0)
    assert device_run(mats, cond, init, n_bins, out=into)[0] is into and into.tobytes() == want[0].tobytes()


@pytest.mark.parametrize("fill", [0xFF, 0xA5])
def test_recycled_memory_changes_no_byte(small, fill):
    mats, cond, init, n_bins, want = (small[k] for k in ("mats", "cond", "init", "n_bins", "want"))
    other = [seeded_matrix(7, 61)]
    other_want = pvalues.restate_distribution(other, *UNIFORM, 3000, 2)
    for force in (False, True):
        was = _lib.scoredist_force_global(force)
        try:
            plain = device_run(mats, cond, init, n_bins)
            with _lib.alloc_fill(fill):
                first = device_run(mats, cond, init, n_bins)
                assert same_bytes(device_run(other, *UNIFORM, 3000, 2), other_want)      # another call through the same pool
                again = device_run(mats, cond, init, n_bins)
            assert same_bytes(plain, want) and same_bytes(first, want) and same_bytes(again, want)
        finally:
            _lib.scoredist_force_global(was)


# ------------------------------------------------------------------------------------------------ 4. statuses

def test_statuses(small):
    L = _lib.lib()
    mats = small["mats"]
    pw = _lib.PwmSet.from_matrices(mats)
    d, i64 = ctypes.c_double, ctypes.c_int64
    try:
        n_bins = 32
        cond, init = (np.ascontiguousarray(a) for a in background(1, 1))
        mass, step, s0 = np.zeros((len(mats), n_bins)), np.zeros(len(mats)), np.zeros(len(mats), dtype=np.int64)

        def call(h=pw.h, strand=1, order=1, cond=cond, init=init, n_bins=n_bins, step=step, s0=s0, mass=mass):
            p = lambda a, t: None if a is None else _lib.ptr(a, t)
            return L.ms_pwmset_score_distribution(h, strand, order, p(cond, d), p(init, d), n_bins, p(step, d), p(s0, i64),
                                                  None if mass is None else ctypes.c_void_p(mass.ctypes.data), None)

        assert call() == _lib.MS_OK
        assert call(h=None) == _lib.MS_ERR_INVALID
        for name in ("cond", "init", "step", "s0", "mass"):
            assert call(**{name: None}) == _lib.MS_ERR_INVALID, name
        for strand in (0, 3, -1):
            assert call(strand=strand) == _lib.MS_ERR_INVALID
        for order in (-1, _lib.MS_SCOREDIST_MAX_ORDER + 1):
            assert call(order=order) == _lib.MS_ERR_INVALID
        widest = max(m.shape[1] for m in mats)
        assert call(n_bins=widest + 2) == _lib.MS_ERR_INVALID and call(n_bins=_lib.MS_SCOREDIST_MAX_BINS + 1) == _lib.MS_ERR_INVALID
        assert call(n_bins=widest + 3, mass=np.zeros((len(mats), widest + 3))) == _lib.MS_OK
        for bad in (-0.25, np.nan, np.inf):
            c2, i2 = cond.copy(), init.copy()
            c2[2, 1], i2[3] = bad, bad
            assert call(cond=c2) == _lib.MS_ERR_INVALID and call(init=i2) == _lib.MS_ERR_INVALID
        with pytest.raises(ValueError):
            _lib.check(call(strand=3))

        per_motif = 2 * 4 * n_bins * 8
        before = _lib.scoredist_budget(per_motif - 1)
        try:
            rc = call()
            assert rc == _lib.MS_ERR_NOMEM
            with pytest.raises(MemoryError, match="work budget"):
                _lib.check(rc)
            _lib.scoredist_budget(per_motif)
            assert call() == _lib.MS_OK
        finally:
            _lib.scoredist_budget(before)
        # the largest request the arguments allow does not fit the library's own budget: refused, nothing launched
        big_cond, big_init = background(_lib.MS_SCOREDIST_MAX_ORDER, 1)
        assert call(order=_lib.MS_SCOREDIST_MAX_ORDER, cond=big_cond, init=big_init, n_bins=_lib.MS_SCOREDIST_MAX_BINS) == _lib.MS_ERR_NOMEM

        import torch
        if torch.cuda.device_count() > 1:
            far = torch.zeros((len(mats), n_bins), dtype=torch.float64, device="cuda:1")
            torch.cuda.synchronize()
            rc = L.ms_pwmset_score_distribution(pw.h, 1, 1, _lib.ptr(cond, d), _lib.ptr(init, d), n_bins, _lib.ptr(step, d), _lib.ptr(s0, i64),
                                                ctypes.c_void_p(int(far.data_ptr())), None)
            assert rc == _lib.MS_ERR_INVALID
    finally:
        pw.close()


# ------------------------------------------------------------------------------------------------ 5. through Python

class Pwm:
    def __init__(self, matrix):
        self.matrix, self.length, self.cutoffs = matrix, matrix.shape[1], None


class Region:
    def __init__(self, chrom, start, end):
        self.chrom, self.start, self.end, self.summit = chrom, start, end, (start + end) // 2


def test_python_fronts_both_strands_and_the_scanner(small):
    from motifscan_amd import kmers, scanner
    mats, cond, init, n_bins = (small[k] for k in ("mats", "cond", "init", "n_bins"))
    fwd, step, s0 = pvalues.restate_distribution(mats, cond, init, n_bins, 1)
    rev = pvalues.restate_distribution(mats, cond, init, n_bins, 2)[0]
    timing = {}
    dist = pvalues.score_distribution(mats, cond, init, n_bins, strand=3, timing=timing)
    assert same_bytes((dist.mass, dist.step, dist.s0), ((fwd + rev) * 0.5, step, s0)) and timing["device_ms"] > 0
    assert dist.max_raw.tolist() == [scoredist.max_raw_of(m) for m in mats]
    want = pvalues.ScoreDistribution.from_matrices(mats, (fwd + rev) * 0.5, step, s0).cutoffs(["1e-1", "1e-3"])
    assert pvalues.analytic_cutoffs(mats, (cond, init), ["1e-1", "1e-3"], n_bins=n_bins) == want
    assert want[2] == {"1e-1": None, "1e-3": None} and want[3]["1e-3"] > want[3]["1e-1"] > 0
    assert want[0]["1e-3"] is None                               # 4 columns: no score of that motif is as rare as 1e-3

    rng = np.random.default_rng(3)
    chrom = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.choice(4, 3000, p=[0.35, 0.15, 0.15, 0.35])].tobytes()
    regions = [("c1", 0, 1200), ("c1", 1500, 3000)]
    seqs = [chrom[a:b].decode() for _, a, b in regions]
    genome = _lib.ResidentGenome({"c1": chrom})
    try:
        sc = scanner.Scanner(genome, [Region(*r) for r in regions], strand="+", p_value="no such key")
        try:
            got = sc.score_distribution([Pwm(m) for m in mats], order=2, n_bins=150)
        finally:
            sc.close()
    finally:
        genome.close()
    bg = pvalues.background_from_counts(kmers.kmer_counts_host(seqs, 3))
    assert bg[0].shape == (16, 4) and abs(bg[1].sum() - 1.0) < 1e-12
    assert same_bytes((got.mass, got.step, got.s0), pvalues.restate_distribution(mats, *bg, 150, 1))


# ------------------------------------------------------------------------------------------------ 6. the scan's own arithmetic

def test_the_distribution_brackets_the_scan_on_every_pentamer():
    W = 5
    mat = seeded_matrix(W, 71)
    words = ["".join("ACGT"[b] for b in w) for w in all_words(W).tolist()]
    n_bins = 4096
    pw, sq = _lib.PwmSet.from_matrices([mat]), _lib.SeqSet.from_strings(words)
    try:
        score = _lib.score(pw, sq, 1)[0]                          # the forward score of every pentamer: its only window
        mass, step, s0 = _lib.score_distribution(pw, 1, 0, *UNIFORM, n_bins)
        dist = pvalues.ScoreDistribution.from_matrices([mat], mass, step, s0)
        assert dist.bracket_ok[0] and abs(dist.lost(0)) < 1e-12

        xs = np.unique(score)
        emp = (len(score) - np.searchsorted(np.sort(score), xs, side="left")) / float(4 ** W)
        lower, upper = dist.p_value_bounds(0, xs)
        assert np.all(lower <= emp) and np.all(emp <= upper)

        p = "0.0625"
        cut = dist.cutoffs([p])[0][p]
        i = dist.cutoff_index(0, p)
        assert cut is not None and i is not None
        pw.set_cutoffs(np.array([cut]))
        res = _lib.scan(pw, sq, 1)
        try:
            n_hits = res.n_hits
        finally:
            res.close()
        S = word_scores(mat, n_bins)[0]                           # relative to s0, as i is
        assert np.count_nonzero(S >= i + W + 3) <= n_hits <= 64
    finally:
        sq.close()
        pw.close()
