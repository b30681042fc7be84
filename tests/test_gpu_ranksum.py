"""
ms_best_rank_sum and ms_best_count_passing (ms_ranksum.hip) on the GPU.  The inputs are best-site matrices made by ms_scan_best over tiny
sets (tests/test_gpu_best.py pins that call to the oracle); the expected integers come from the numpy restatements of
motifscan_amd.enrich applied to the host copy of the same matrices (tests/test_ranksum_host.py pins those to a brute-force pair count).
Small integer PWMs and short regions make ties the rule; an unscorable motif, a motif with a -inf entry, regions shorter than the motif
and all-N regions make cells without a winner.  Group sizes straddle a wave, and every per-block element count of ms_debug_ranksum_dims.

"Handles on different devices" needs two devices and is not exercised here.
"""
import ctypes

import numpy as np
import pytest

from motifscan_amd import _lib, enrich, scanner

pytestmark = pytest.mark.gpu

WIDTHS = (1, 5, 12)


@pytest.fixture(scope="module", autouse=True)
def _device():
    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible")
    _lib.set_device(0)


def make_mats():
    rng = np.random.default_rng(31)
    mats = []
    for w in WIDTHS:
        m = rng.integers(-3, 4, size=(4, w)).astype(np.float64)
        m[0, 0] = 2.0                                     # scorable whatever was drawn
        mats.append(m)
    mats.append(-np.abs(rng.integers(0, 4, size=(4, 5)).astype(np.float64)))        # every entry <= 0: max_raw = 0, unscorable
    holes = rng.integers(-2, 3, size=(4, 5)).astype(np.float64)
    holes[1, 1] = 3.0
    holes[0, 2] = -np.inf                                 # an A at column 2 ('+') never is part of a site
    mats.append(holes)
    return mats


def make_regions(n, seed):
    """n short regions: per motif width W the lengths W - 1 (no window), W, W + 3, and an all-N region, over a two-letter-heavy alphabet."""
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b"AACCAGTN", dtype=np.uint8)
    out = []
    for i in range(n):
        w = WIDTHS[i % 3]
        kind = (i // 3) % 4
        length = max(1, (w - 1, w, w + 3, w + 3)[kind])
        out.append("N" * length if kind == 3 else letters[rng.integers(0, len(letters), length)].tobytes().decode())
    return out


class World:
    """Best-site matrices by (pool, number of regions, strand mask), made once and kept on the device for the module."""

    def __init__(self):
        self.mats = make_mats()
        self.pw = _lib.PwmSet.from_matrices(self.mats)
        self.dims = _lib.ranksum_dims()
        self.most = 2 * max(self.dims["gather_elems"], self.dims["rank_elems"], self.dims["count_elems"]) + 77
        self.pools = {"a": make_regions(self.most, 41), "b": make_regions(self.most, 42)}
        self.cache = {}

    def best(self, pool, n, strand_mask=3):
        """(BestSites handle, host copy of its scores [P][n])"""
        key = (pool, n, strand_mask)
        if key not in self.cache:
            sq = _lib.SeqSet.from_strings(self.pools[pool][:n])
            try:
                res = _lib.scan_best(self.pw, sq, strand_mask)
            finally:
                sq.close()
            self.cache[key] = (res, res.sites()[0])
        return self.cache[key]

    def close(self):
        for res, _ in self.cache.values():
            res.close()
        self.pw.close()


@pytest.fixture(scope="module")
def world():
    w = World()
    yield w
    w.close()


def same(got, want):
    """(u2, ties, na, nb) of the device against an enrich.RankSum"""
    u2, ties, na, nb = got
    assert u2.dtype == np.int64 and np.array_equal(u2, want.u2)
    assert ties == want.ties and (na, nb) == (want.na, want.nb)


def group_sizes(dims):
    edges = sorted({dims[k] + d for k in ("gather_elems", "rank_elems") for d in (-1, 0, 1)})
    small = [0, 1, 2, 63, 64, 65]
    pairs = [(0, 5), (5, 0), (0, 0), (1, 1), (1, 2), (2, 63), (63, 64), (64, 65), (65, 1)]
    pairs += list(zip(edges, reversed(edges))) + [(edges[0], 1), (2, edges[-1]), (edges[-1], edges[-1])]
    assert {n for p in pairs for n in p} >= set(small) | set(edges)
    return pairs


@pytest.mark.parametrize("strand_mask", (1, 2, 3))
def test_ties_and_cells_without_a_winner(world, strand_mask):
    n_nan = n_tied = 0
    for na, nb in group_sizes(world.dims):
        (ha, xa), (hb, xb) = world.best("a", na, strand_mask), world.best("b", nb, strand_mask)
        want = enrich.rank_sum_host(xa, xb)
        same(ha.rank_sum(hb), want)
        N, u = na + nb, len(WIDTHS)                       # the unscorable motif's row: all NaN
        assert int(want.u2[u]) == na * nb and want.ties[u] == N ** 3 - N
        n_nan += int(np.isnan(xa[len(WIDTHS) + 1]).sum())
        n_tied += sum(1 for t in want.ties[:len(WIDTHS)] if t > 0)
    assert n_nan > 100 and n_tied > 10                    # (the cases hold what they are meant to hold)
    xs = world.best("a", 65, strand_mask)[1]
    assert np.isnan(xs[:len(WIDTHS)]).any() and not np.isnan(xs[:len(WIDTHS)]).all() and np.isneginf(xs).sum() == 0


def test_selections(world):
    h, x = world.best("a", world.most)
    R = world.most
    rng = np.random.default_rng(5)
    ones = np.ones(R, dtype=np.uint8)
    h2, x2 = world.best("b", 300)
    base = h.rank_sum(h2)
    same(base, enrich.rank_sum_host(x, x2))
    for sel_a, sel_b in ((ones, None), (None, np.ones(300, dtype=np.uint8)), (ones, np.ones(300, dtype=np.uint8))):
        got = h.rank_sum(h2, sel_a, sel_b)                # NULL against all-ones: the same bytes
        assert got[0].tobytes() == base[0].tobytes() and got[1:] == base[1:]
    half = rng.random(R) < 0.5
    third = rng.random(R) < 0.3
    one = np.zeros(R, dtype=bool)
    one[R - 1] = True
    none = np.zeros(R, dtype=bool)
    edge = np.zeros(R, dtype=bool)
    edge[rng.permutation(R)[:world.dims["rank_elems"] + 1]] = True
    for sel_a, sel_b in ((half, ~half), (half, third), (half, half), (none, half), (half, none), (none, none), (one, half), (half, one), (one, one),
                         (edge, ~edge), (200 * half.astype(np.uint8), third)):          # (any non-zero flag selects)
        a, b = np.asarray(sel_a) != 0, np.asarray(sel_b) != 0
        same(h.rank_sum(h, sel_a, sel_b), enrich.rank_sum_host(x[:, a], x[:, b]))
    same(h2.rank_sum(h, None, third), enrich.rank_sum_host(x2, x[:, third]))
    with pytest.raises(ValueError):
        h.rank_sum(h, np.ones(R - 1, dtype=np.uint8))


def test_batching_gives_the_same_bytes(world):
    (ha, xa), (hb, xb) = world.best("a", 130), world.best("b", 77)
    want = enrich.rank_sum_host(xa, xb)
    base = ha.rank_sum(hb)
    same(base, want)
    N, P = 130 + 77, len(world.mats)
    assert P >= 5
    prev = _lib.ranksum_budget(0)
    try:
        for budget in (N, 3 * N, 3 * N + N // 2, N - 1, 1):          # one row per batch, three (5 = 3 + 2), three again, "less than one row" twice
            _lib.ranksum_budget(budget)
            got = ha.rank_sum(hb)
            assert got[0].tobytes() == base[0].tobytes() and got[1:] == base[1:], budget
            sub = ha.rank_sum(hb, m0=1, m1=P)
            assert np.array_equal(sub[0], base[0][1:]) and sub[1] == base[1][1:]
    finally:
        _lib.ranksum_budget(prev)


def test_either_side_of_the_sort_forms(world):
    """A group of up to dims['segmented_max'] cells takes the segmented sort, a larger one a device sort per row: one group on either
    side in one call, then the other way round, and selections that bring both groups to the segmented side."""
    edge = world.dims["segmented_max"]
    pool = world.pools["a"]
    many = (pool * (edge // len(pool) + 2))[:edge + 1]    # (the pool repeated: ties everywhere)
    sq = _lib.SeqSet.from_strings(many)
    try:
        big = _lib.scan_best(world.pw, sq)
    finally:
        sq.close()
    try:
        x = big.sites()[0]
        at = np.ones(edge + 1, dtype=np.uint8)
        at[7] = 0                                         # exactly `edge` cells
        want = enrich.rank_sum_host(x, x[:, at != 0])
        same(big.rank_sum(big, None, at), want)           # per row against segmented
        back = big.rank_sum(big, at, None)
        assert np.array_equal(back[0] + want.u2, np.full(len(want), 2 * (edge + 1) * edge)) and back[1] == want.ties
        prev = _lib.ranksum_budget(2 * edge + 1)          # ... and one row per batch
        try:
            same(big.rank_sum(big, None, at), want)
        finally:
            _lib.ranksum_budget(prev)
        few = np.zeros(edge + 1, dtype=np.uint8)
        few[::1000] = 1
        same(big.rank_sum(big, at, few), enrich.rank_sum_host(x[:, at != 0], x[:, few != 0]))
    finally:
        big.close()


def raw_rank_sum(ha, hb, m0, m1, rows, flags=0, u2_null=False, fill=-7):
    u2, ties, n = np.full(rows, fill, dtype=np.int64), np.full((rows, 2), 9, dtype=np.uint64), np.full(2, fill, dtype=np.int64)
    rc = _lib.lib().ms_best_rank_sum(ha.h if ha else None, None, hb.h if hb else None, None, m0, m1, flags, None if u2_null else _lib.ptr(u2, ctypes.c_int64),
                                     _lib.ptr(ties, ctypes.c_uint64), _lib.ptr(n, ctypes.c_int64), None)
    return rc, u2, ties, n


def test_motif_ranges_and_determinism(world):
    (ha, xa), (hb, xb) = world.best("a", 515), world.best("b", 64)
    P = len(world.mats)
    full = ha.rank_sum(hb)
    same(full, enrich.rank_sum_host(xa, xb))
    again = ha.rank_sum(hb)
    assert again[0].tobytes() == full[0].tobytes() and again[1:] == full[1:]
    for m0, m1 in ((0, 1), (1, 3), (2, P), (P - 1, P), (0, P)):
        sub = ha.rank_sum(hb, m0=m0, m1=m1)
        assert np.array_equal(sub[0], full[0][m0:m1]) and sub[1] == full[1][m0:m1] and sub[2:] == full[2:]
    for m in (0, 2, P):                                   # an empty range: MS_OK, nothing written
        rc, u2, ties, n = raw_rank_sum(ha, hb, m, m, 2)
        assert rc == _lib.MS_OK and (u2 == -7).all() and (ties == 9).all() and (n == -7).all()
    assert ha.rank_sum(hb, m0=2, m1=2)[2:] == (515, 64)


def last_error():
    return _lib.lib().ms_last_error().decode()


def test_rank_sum_refusals(world):
    (ha, _), (hb, _) = world.best("a", 5), world.best("b", 5)
    P = len(world.mats)
    pw1 = _lib.PwmSet.from_matrices(world.mats[:2])
    sq = _lib.SeqSet.from_strings(["ACGTACGTACGTAC"])
    other = _lib.scan_best(pw1, sq)
    try:
        rc = raw_rank_sum(ha, other, 0, 1, 1)[0]
        assert rc == _lib.MS_ERR_INVALID and "number of PWMs" in last_error()
        with pytest.raises(ValueError, match="number of PWMs"):
            ha.rank_sum(other, m0=0, m1=1)
    finally:
        other.close()
        sq.close()
        pw1.close()
    rc = raw_rank_sum(ha, hb, 0, 1, 1, flags=1)[0]
    assert rc == _lib.MS_ERR_INVALID and "flags" in last_error()
    for m0, m1 in ((-1, 1), (0, P + 1), (3, 2), (P + 1, P + 1)):
        rc = raw_rank_sum(ha, hb, m0, m1, P + 2)[0]
        assert rc == _lib.MS_ERR_INVALID and "motif range" in last_error(), (m0, m1)
    rc = raw_rank_sum(ha, hb, 0, 1, 1, u2_null=True)[0]
    assert rc == _lib.MS_ERR_INVALID and "NULL output" in last_error()
    assert raw_rank_sum(None, hb, 0, 1, 1)[0] == _lib.MS_ERR_INVALID and "NULL handle" in last_error()
    assert raw_rank_sum(ha, None, 0, 1, 1)[0] == _lib.MS_ERR_INVALID


def attained_cutoffs(x, rng, k_extra):
    """Per motif row: cutoffs on attained best scores, at score + 1e-10, one double above that, one double below the score, and
    k_extra drawn between the row's extremes."""
    rows = []
    for row in x:
        num = row[np.isfinite(row)]
        picks = rng.choice(num, size=3) if len(num) else np.array([0.25, 0.5, 0.75])
        cuts = []
        for s in picks:
            cuts += [s, s + 1e-10, np.nextafter(s + 1e-10, np.inf), np.nextafter(s, -np.inf), np.nextafter(s + 1e-10, -np.inf)]
        lo, hi = (num.min(), num.max()) if len(num) else (0.0, 1.0)
        cuts += rng.uniform(lo - 0.1, hi + 0.1, size=k_extra).tolist()
        rows.append(cuts)
    return np.asarray(rows, dtype=np.float64)


def test_count_passing_against_the_restatement(world):
    rng = np.random.default_rng(6)
    ce, chunk = world.dims["count_elems"], world.dims["cut_chunk"]
    P = len(world.mats)
    for n in (1, 63, 65, ce - 1, ce, ce + 1, world.most):
        h, x = world.best("a", n)
        cut = attained_cutoffs(x, rng, 2)
        want = enrich.count_passing_host(x, cut)
        got = h.count_passing(cut)
        assert got.dtype == np.int64 and got.shape == cut.shape and np.array_equal(got, want), n
        assert np.array_equal(h.count_passing(cut), got)
    h, x = world.best("a", world.most)
    cut = attained_cutoffs(x, rng, chunk + 1 - 15)        # one more cutoff than a block counts between two flushes
    assert cut.shape[1] == chunk + 1
    want = enrich.count_passing_host(x, cut)
    assert np.array_equal(h.count_passing(cut), want) and want.any() and (want < world.most).any()
    assert np.array_equal(h.count_passing(cut[:, :chunk]), want[:, :chunk])
    sel = rng.random(world.most) < 0.4
    assert np.array_equal(h.count_passing(cut, sel), enrich.count_passing_host(x[:, sel], cut))
    assert np.array_equal(h.count_passing(cut, np.ones(world.most, dtype=np.uint8)), want)
    assert not h.count_passing(cut, np.zeros(world.most, dtype=np.uint8)).any()
    assert np.array_equal(h.count_passing(cut[1:4], m0=1, m1=4), want[1:4])
    assert np.array_equal(h.count_passing(cut[2, :1], m0=2, m1=3), want[2:3, :1])           # 1-D: one cutoff per motif
    assert h.count_passing(np.zeros((P, 0))).shape == (P, 0)                                  # n_cut = 0 is MS_OK
    assert _lib.lib().ms_best_count_passing(h.h, None, None, 0, 0, P, None, None) == _lib.MS_OK
    assert h.count_passing(np.zeros((0, 3)), m0=2, m1=2).shape == (0, 3)
    # the counts are additive over region shards
    left = np.arange(world.most) < 700
    assert np.array_equal(h.count_passing(cut, left) + h.count_passing(cut, ~left), want)


@pytest.mark.parametrize("strand_mask", (1, 2, 3))
def test_count_passing_is_the_scans_region_count(rnd, strand_mask):
    keys = [str(k) for k in rnd["cutoff_keys"]]
    cut = np.stack([rnd["cutoff_by_key"][k] for k in keys], axis=1)                          # [P][K]
    sq = _lib.SeqSet.from_strings(rnd["seqs"])
    pw = _lib.PwmSet.from_matrices(rnd["mats"])
    try:
        best = _lib.scan_best(pw, sq, strand_mask)
        try:
            got = best.count_passing(cut)
        finally:
            best.close()
        for k, key in enumerate(keys):
            pw.set_cutoffs(rnd["cutoff_by_key"][key])
            res = _lib.scan(pw, sq, strand_mask)
            try:
                want = res.region_counts()
            finally:
                res.close()
            assert np.array_equal(got[:, k], want), key
        assert got.any() and (got[:, 0] >= got[:, -1]).all()
    finally:
        pw.close()
        sq.close()


def test_count_passing_refusals(world):
    h, _ = world.best("a", 5)
    P = len(world.mats)
    counts = np.zeros((P, 2), dtype=np.int64)

    def raw(cut, m0=0, m1=P, n_cut=2, counts_null=False):
        cut = np.ascontiguousarray(cut, dtype=np.float64)
        return _lib.lib().ms_best_count_passing(h.h, None, _lib.ptr(cut, ctypes.c_double), n_cut, m0, m1, None if counts_null else _lib.ptr(counts, ctypes.c_int64), None)

    good = np.full((P, 2), 0.5)
    assert raw(good) == _lib.MS_OK
    for bad in (np.nan, np.inf, -np.inf):
        cut = good.copy()
        cut[P - 1, 1] = bad
        assert raw(cut) == _lib.MS_ERR_INVALID and "not finite" in last_error()
        with pytest.raises(ValueError, match="not finite"):
            h.count_passing(cut)
    for m0, m1 in ((-1, 1), (0, P + 1), (3, 2)):
        assert raw(good, m0, m1) == _lib.MS_ERR_INVALID and "motif range" in last_error()
    assert raw(good, n_cut=-1) == _lib.MS_ERR_INVALID
    assert raw(good, counts_null=True) == _lib.MS_ERR_INVALID
    assert _lib.lib().ms_best_count_passing(h.h, None, None, 2, 0, P, _lib.ptr(counts, ctypes.c_int64), None) == _lib.MS_ERR_INVALID
    assert _lib.lib().ms_best_count_passing(None, None, _lib.ptr(good, ctypes.c_double), 2, 0, P, _lib.ptr(counts, ctypes.c_int64), None) == _lib.MS_ERR_INVALID


def test_scanner_end_to_end():
    rng = np.random.default_rng(12)
    chroms = {"chr1": "".join(rng.choice(list("ACGT"), size=3000)), "chr2": "".join(rng.choice(list("AACGTN"), size=2000))}

    class Genome:
        chrom_sizes = {k: len(v) for k, v in chroms.items()}

        def fetch_sequence(self, chrom, start, end):
            return chroms[chrom][start:end]

    class Region:
        def __init__(self, chrom, start, end):
            self.chrom, self.start, self.end, self.summit = chrom, start, end, (start + end) // 2

    class Pwm:
        def __init__(self, matrix):
            self.matrix, self.length, self.cutoffs = matrix, matrix.shape[1], {"1e-4": 0.8}

    pwms = [Pwm(m) for m in make_mats()]
    peaks = [Region("chr1", int(s), int(s) + int(n)) for s, n in zip(rng.integers(0, 2900, 70), rng.integers(3, 60, 70))]
    ctrl = [Region("chr2", int(s), int(s) + int(n)) for s, n in zip(rng.integers(0, 1900, 45), rng.integers(3, 60, 45))]
    for strand in ("both", "+"):
        a, b = scanner.Scanner(Genome(), peaks, strand=strand), scanner.Scanner(Genome(), ctrl, strand=strand)
        try:
            xa, xb = a.best_sites(pwms).score, b.best_sites(pwms).score
            got = a.rank_sum(pwms, b)
            want = enrich.rank_sum_host(xa, xb)
            assert isinstance(got, enrich.RankSum) and np.array_equal(got.u2, want.u2) and got.ties == want.ties and (got.na, got.nb) == (70, 45)
            assert np.array_equal(got.z(), want.z(), equal_nan=True) and np.isfinite(got.z()).sum() >= 3 and np.isnan(got.z()[len(WIDTHS)])
            sel, sel_c = rng.random(70) < 0.5, rng.random(45) < 0.5
            got = a.rank_sum(pwms, b, sel, sel_c)
            want = enrich.rank_sum_host(xa[:, sel], xb[:, sel_c])
            assert np.array_equal(got.u2, want.u2) and got.ties == want.ties and (got.na, got.nb) == (int(sel.sum()), int(sel_c.sum()))
            cut = np.tile([0.3, 0.6, 0.8, 1.0], (len(pwms), 1))
            counts = a.count_regions_passing(pwms, cut)
            assert counts.dtype == np.int64 and np.array_equal(counts, enrich.count_passing_host(xa, cut))
            assert np.array_equal(counts[:, 2], a.count_regions_with_sites(pwms))            # ... the scan's own count at that cutoff
        finally:
            a.close()
            b.close()
