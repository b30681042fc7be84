"""
Motif pairs on the device (ms_result_cooccurrence, ms_result_pair_spacing; motifscan_amd.pairs) against the numpy restatements of
tests/test_pairs_host.py.  Every comparison is exact: both quantities are integer reductions.  Most results are made of seeded
synthetic hit arrays (ms_result_from_hits), which places every boundary where the test wants it; the last tests scan.  Run with -m gpu.
"""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest

from motifscan_amd import _lib, pairs, synth
from motifscan_amd.scanner import Scanner
from test_pairs_host import HAND, HAND_WIDTHS, hit_arrays, np_cooccurrence, np_pair_spacing, random_hits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def device():
    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests need an MI355X (there is no CPU fallback)")
    _lib.set_device(0)


def result_of(hits, n_regions):
    offsets, seq_idx, pos, strand = hits
    return _lib.result_from_hits(len(offsets) - 1, n_regions, offsets, seq_idx, pos, np.zeros(len(pos)), strand)


def pwmset_of(widths):
    return _lib.PwmSet.from_matrices([np.ones((4, w)) for w in widths])


# ------------------------------------------------------------------------------------------------------- co-occurrence --

def check_cooccurrence(hits, P, R, ranges):
    res = result_of(hits, R)
    try:
        want = np_cooccurrence(hits[0], hits[1], P, R)
        got = res.cooccurrence()
        assert got.dtype == np.int64 and got.shape == (P, P) and np.array_equal(got, want)
        assert np.array_equal(got, got.T) and np.array_equal(np.diag(got), res.region_counts())
        for m0, m1 in ranges:
            assert np.array_equal(res.cooccurrence(m0, m1), want[m0:m1]), (m0, m1)
        return got
    finally:
        res.close()


def cooc_hits(rng, P, R):
    """Random sites of about a third of the regions per motif; of the last two motifs one has no site, one a site in every region."""
    per = [random_hits(rng, R, max(1, R // 3), 50) for _ in range(P)]
    if P >= 2:
        per[-2] = np.zeros((0, 3), dtype=np.int64)
        per[-1] = np.stack([np.arange(R), np.full(R, 7), np.full(R, 1)], axis=1)
    return hit_arrays(per)


@pytest.mark.parametrize("R", [1, 63, 64, 65, 129, 4097])
def test_cooccurrence_across_word_boundaries(R):
    P = 5
    got = check_cooccurrence(cooc_hits(np.random.default_rng(R), P, R), P, R, [(0, 1), (P - 1, P), (3, 3), (1, 4)])
    assert not got[3].any() and not got[:, 3].any() and got[4, 4] == R        # no site at all; a site in every region


@pytest.mark.parametrize("P", [1, 33, 67])
def test_cooccurrence_across_tile_tails(P):
    ranges = [(0, 1), (P - 1, P), (P // 2, P // 2)] + ([(P // 3, 2 * P // 3 + 1), (3, 3)] if P > 3 else [])
    check_cooccurrence(cooc_hits(np.random.default_rng(100 + P), P, 200), P, 200, ranges)


def test_cooccurrence_with_the_word_range_cut_across_blocks():
    """More regions than a few LDS stages and only four tiles of motifs: the library cuts the word range across blocks (it wants more
    blocks than the device has compute units), whose partial sums meet in 64-bit atomic adds."""
    P, R = 67, 3 * _lib.cooc_chunk_regions() + 5
    check_cooccurrence(cooc_hits(np.random.default_rng(9), P, R), P, R, [(60, 67)])


def test_cooccurrence_of_empty_results():
    for P, R in ((3, 10), (3, 0)):
        res = result_of(hit_arrays([[] for _ in range(P)]), R)
        try:
            got = res.cooccurrence()
            assert got.shape == (P, P) and not got.any()
        finally:
            res.close()


def test_cooccurrence_into_device_memory_gives_the_same_bytes():
    import torch
    P, R = 33, 1000
    hits = cooc_hits(np.random.default_rng(3), P, R)
    res = result_of(hits, R)
    try:
        host = res.cooccurrence(5, 30)
        dev = torch.full((25, P), -1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()                                  # the fill runs on torch's stream, the library writes on its own
        assert res.cooccurrence(5, 30, out=int(dev.data_ptr())) == int(dev.data_ptr())
        torch.cuda.synchronize()
        assert host.tobytes() == dev.cpu().numpy().tobytes() and host.any()
    finally:
        res.close()


# -------------------------------------------------------------------------------------------------------------- spacing --

def check_spacing(hits, R, widths, anchor, max_dist, ranges=()):
    res, pw = result_of(hits, R), pwmset_of(widths)
    try:
        want, want_n = np_pair_spacing(*hits, widths, anchor, max_dist)
        counts, n_pairs = res.pair_spacing(pw, anchor, max_dist)
        assert counts.dtype == np.int64 and counts.shape == want.shape
        assert np.array_equal(counts, want) and np.array_equal(n_pairs, want_n)
        for m0, m1 in ranges:
            c, n = res.pair_spacing(pw, anchor, max_dist, m0, m1)
            assert np.array_equal(c, want[m0:m1]) and np.array_equal(n, want_n[m0:m1]), (m0, m1)
        return counts, n_pairs
    finally:
        res.close()
        pw.close()


def test_spacing_of_the_hand_written_case():
    counts, n_pairs = check_spacing(HAND, 3, HAND_WIDTHS, 0, 2, [(0, 1), (2, 3), (1, 1)])
    assert n_pairs.tolist() == [6, 8, 3] and counts[2, 1].tolist() == [0, 1, 0, 1, 0]


@pytest.mark.parametrize("max_dist", [0, 1, 7])
def test_spacing_on_dense_random_sites(max_dist):
    rng = np.random.default_rng(20 + max_dist)
    widths = [8, 11, 8, 20, 5]
    hits = hit_arrays([random_hits(rng, 37, 300, 40) for _ in widths])
    for anchor in (0, 3):
        counts, _ = check_spacing(hits, 37, widths, anchor, max_dist, [(1, 4), (4, 5)])
        assert counts.sum() > 0
        # the anchor against itself: every pair is seen from both of its ends
        assert np.array_equal(counts[anchor, 1], counts[anchor, 2][::-1])
        assert np.array_equal(counts[anchor, 0], counts[anchor, 0][::-1]) and np.array_equal(counts[anchor, 3], counts[anchor, 3][::-1])


def test_spacing_counts_the_last_distance_in_range_and_not_the_next():
    D = 7
    # anchor of width 4 at 100; a partner of width 6 (even): t2 = 2 * (q - 100) + 2; one of width 5 (odd): t2 = 2 * (q - 100) + 1
    hits = hit_arrays([[(0, 100, 1)],
                       [(0, 91, 1), (0, 92, 1), (0, 106, 2), (0, 107, 2)],            # t2 = -16, -14, +14, +16
                       [(0, 92, 1), (0, 93, 1), (0, 106, 2), (0, 107, 2)]])           # t2 = -15, -13, +13, +15
    counts, n_pairs = check_spacing(hits, 1, [4, 6, 5], 0, D)
    assert n_pairs.tolist() == [0, 4, 4] and counts.sum() == 4
    assert counts[1, 0, 0] == 1 and counts[1, 1, 2 * D] == 1                          # |t2| = 2 * max_dist: the first and the last bin
    assert counts[2, 0, 0] == 1 and counts[2, 1, 2 * D - 1] == 1 and not counts[2, :, 2 * D].any()


def test_sites_of_adjacent_regions_never_pair():
    hits = hit_arrays([[(r, 10, 1) for r in range(0, 40, 2)],
                       [(r, 10, 1) for r in range(1, 40, 2)] + [(r, 10, 2) for r in range(1, 40, 2)],
                       [(r, 12, 2) for r in range(0, 40, 4)]])
    counts, n_pairs = check_spacing(hits, 40, [6, 6, 6], 0, 5)
    assert not counts[1].any() and n_pairs.tolist() == [0, 0, 10] and counts[2].sum() == 10


def test_spacing_without_anchor_hits_or_partner_hits():
    rng = np.random.default_rng(4)
    hits = hit_arrays([random_hits(rng, 9, 60, 30), [], random_hits(rng, 9, 60, 30)])
    counts, n_pairs = check_spacing(hits, 9, [5, 6, 7], 0, 4)
    assert not counts[1].any() and n_pairs[1] == 0 and counts[2].any()
    counts, n_pairs = check_spacing(hits, 9, [5, 6, 7], 1, 4)
    assert not counts.any() and not n_pairs.any()


def test_spacing_of_a_region_with_thousands_of_sites():
    """One region holds 3 000 sites of either motif, the others one or none: the forward walks cross the blocks' chunks of anchor hits and
    the partner bracket of a chunk is a small part of a long region; n_pairs of a row is near 10^7, summed in 64 bits."""
    rng = np.random.default_rng(8)
    crowd = np.stack([np.full(3000, 17), np.repeat(np.arange(1500), 2), np.tile([1, 2], 1500)], axis=1)
    per = []
    for _ in range(2):
        few = random_hits(rng, 40, 25, 1500)
        per.append(np.concatenate([few[few[:, 0] != 17], crowd]))
    per.append(random_hits(rng, 40, 200, 1500))
    counts, n_pairs = check_spacing(hit_arrays(per), 40, [10, 13, 6], 0, 7, [(1, 2)])
    assert n_pairs[0] >= 3000 * 2999 and n_pairs[1] >= 3000 * 3000 and counts[1].sum() > 3000 * 20


def test_spacing_on_both_sides_of_the_lds_bin_limit():
    rng = np.random.default_rng(12)
    D = (_lib.pair_lds_bins() - 1) // 2
    hits = hit_arrays([random_hits(rng, 3, 400, 3 * D) for _ in range(3)])
    for max_dist in (D, D + 1):                                   # 2 * max_dist + 1 == the limit: LDS; two more bins: global memory
        counts, _ = check_spacing(hits, 3, [9, 12, 6], 1, max_dist, [(2, 3)])
        assert counts[:, :, :50].any() and counts[:, :, -50:].any()


def test_spacing_when_a_block_may_overflow_its_lds_counters():
    """With the library's limit the fallback needs more than four million partner hits; with a limit of 1000 pairs per block every block
    of this case bins in global memory although the histogram would fit LDS.  The result is the same."""
    rng = np.random.default_rng(31)
    widths = [8, 11, 8, 20, 5]
    hits = hit_arrays([random_hits(rng, 37, 300, 40) for _ in widths])
    before = _lib.pair_lds_pair_limit(1000)
    try:
        assert before == 2 ** 32 - 1
        counts, _ = check_spacing(hits, 37, widths, 3, 7, [(1, 4)])
        assert counts.sum() > 0
    finally:
        assert _lib.pair_lds_pair_limit(0) == 1000
    check_spacing(hits, 37, widths, 3, 7)


def test_sites_out_of_scan_order_are_refused_by_the_spacing_and_fine_for_the_cooccurrence():
    """ms_result_from_hits takes arrays in any order (the plot data do not care).  The spacing kernel's searches do: a slice whose
    positions descend inside a region, or whose regions descend, is refused -- on the LDS path and on the global one -- and nothing is
    written outside the histogram on the way (the bin is range-checked where it is used)."""
    from motifscan_amd.sites import MotifSite
    offsets = np.array([0, 4, 8], dtype=np.int64)
    pw = pwmset_of([6, 9])
    for seq_idx, pos in (([0, 0, 0, 1, 0, 0, 1, 1], [500, 20, 300, 7, 10, 510, 3, 9]),          # positions descend in region 0 of motif 0
                         ([0, 0, 1, 1, 1, 0, 0, 1], [1, 2, 3, 4, 10000, 1, 5000, 6])):         # regions descend in motif 1
        seq_idx, pos = np.array(seq_idx, dtype=np.int64), np.array(pos, dtype=np.int64)
        strand = np.array([1, 2, 1, 2, 1, 1, 2, 2], dtype=np.int8)
        res = _lib.result_from_hits(2, 2, offsets, seq_idx, pos, np.zeros(8), strand)
        try:
            for max_dist in (600, _lib.pair_lds_bins()):
                for anchor in (0, 1):
                    with pytest.raises(ValueError, match="order"):
                        res.pair_spacing(pw, anchor, max_dist)
            assert np.array_equal(res.cooccurrence(), np_cooccurrence(offsets, seq_idx, 2, 2))
        finally:
            res.close()
    pw.close()
    lists = [[[MotifSite(500, 1.0, "+"), MotifSite(20, 1.0, "-")], [MotifSite(7, 1.0, "+")]],
             [[MotifSite(10, 1.0, "+")], []]]
    with pytest.raises(ValueError, match="order"):
        pairs.pair_spacing(lists, [np.ones((4, 6)), np.ones((4, 9))], 0, 50)
    assert pairs.cooccurrence(lists).tolist() == [[2, 1], [1, 1]]
    lists[0][0].reverse()                                         # in order: accepted
    sp = pairs.pair_spacing(lists, [np.ones((4, 6)), np.ones((4, 9))], 0, 50)
    assert sp.n_pairs.tolist() == [2, 2] and sp.counts.sum() == 1


# ----------------------------------------------------------------------------------------------------------- end to end --

class ChromGenome:
    """One synthetic chromosome, with what Scanner reads of a genome (scanner.py:81-87)."""

    def __init__(self, seq):
        self.seq = seq
        self.chrom_sizes = {"chr1": len(seq)}

    def fetch_sequence(self, chrom, start, end):
        return self.seq[start:end]


R_SCAN, L_SCAN, ANCHOR, DIST = 300, 200, 41, 50


@pytest.fixture(scope="module")
def scan_set():
    vals, widths, cutoffs = synth.load_motif_set(579, p_value="1e-3")
    bases, offsets = synth.make_regions(R_SCAN, L_SCAN, seed=23)
    return vals, widths, cutoffs, bases, offsets


def test_scan_result_before_and_after_dedup(scan_set):
    vals, widths, cutoffs, bases, offsets = scan_set
    pw, sq = _lib.PwmSet(vals, widths, cutoffs), _lib.SeqSet(bases, offsets)
    res = _lib.scan(pw, sq, 3)
    try:
        n_before = res.n_hits
        for deduped in (False, True):
            if deduped:
                res.dedup(pw)
            h = res.hits()
            assert np.array_equal(res.cooccurrence(), np_cooccurrence(h["motif_offsets"], h["seq_idx"], 579, R_SCAN))
            want, want_n = np_pair_spacing(h["motif_offsets"], h["seq_idx"], h["pos"], h["strand"], widths, ANCHOR, DIST)
            counts, n_pairs = res.pair_spacing(pw, ANCHOR, DIST)
            assert np.array_equal(counts, want) and np.array_equal(n_pairs, want_n)
            assert (counts.sum(axis=(1, 2)) > 0).sum() > 579 // 2                # the cells are well filled at 1e-3
        assert res.n_hits <= n_before
    finally:
        res.close()
        pw.close()
        sq.close()


def test_pairs_module_from_a_view_and_from_plain_lists(scan_set):
    vals, widths, cutoffs, bases, offsets = scan_set
    genome = ChromGenome(bases.tobytes().decode())
    regions = [SimpleNamespace(chrom="chr1", start=i * L_SCAN, end=(i + 1) * L_SCAN, summit=i * L_SCAN + 100, score=None) for i in range(R_SCAN)]
    pwms = [SimpleNamespace(matrix=m, length=m.shape[1], cutoffs={"1e-3": c}, matrix_id=f"M{i}", name=f"m{i}")
            for i, (m, c) in enumerate(zip(synth.matrices_of(vals, widths), cutoffs))]
    sc = Scanner(genome, regions, window_size=0, p_value="1e-3", remove_dup=True)
    sites = sc.scan_motifs(pwms)
    try:
        assert isinstance(sites._h.owner, _lib.ScanResult) and sites._h.owner.h        # read in place, not uploaded
        a = sites.arrays()
        want_co = np_cooccurrence(a["motif_offsets"], a["region"], 579, R_SCAN)
        want, want_n = np_pair_spacing(a["motif_offsets"], a["region"], a["start"], a["strand"], widths, ANCHOR, DIST)
        rows = [ANCHOR, 3, 4, 5, 578]
        diff = np.asarray(widths, dtype=np.int64) - widths[ANCHOR]
        for given in (sites, sites.to_lists()):
            assert np.array_equal(pairs.cooccurrence(given), want_co)
            assert np.array_equal(pairs.cooccurrence(given, motifs=rows), want_co[rows])
            sp = pairs.pair_spacing(given, pwms, ANCHOR, DIST)
            assert np.array_equal(sp.counts, want) and np.array_equal(sp.n_pairs, want_n)
            assert np.array_equal(sp.oriented, pairs.fold_orientations(want, diff)) and sp.oriented.sum() == want.sum()
            assert np.array_equal(sp.x, np.stack([pairs.spacing_axis(DIST, d) for d in diff]))
            sub = pairs.pair_spacing(given, pwms, ANCHOR, DIST, motifs=rows, oriented=False)
            assert np.array_equal(sub.counts, want[rows]) and np.array_equal(sub.n_pairs, want_n[rows]) and sub.oriented is None
    finally:
        sites.close()
        sc.close()


# ------------------------------------------------------------------------------------------------------------ validation --

def test_refused_calls():
    vals, widths, cutoffs = synth.load_motif_set(8)
    bases, offsets = synth.make_regions(200, 300, seed=3)
    pw, sq = _lib.PwmSet(vals, widths, cutoffs), _lib.SeqSet(bases, offsets)
    other = pwmset_of([5, 6, 7])
    counts_only = _lib.scan(pw, sq, 3, _lib.MS_SCAN_COUNTS_ONLY)
    res = _lib.scan(pw, sq, 3)
    try:
        with pytest.raises(ValueError, match="counts-only"):
            counts_only.cooccurrence()
        with pytest.raises(ValueError, match="counts-only"):
            counts_only.pair_spacing(pw, 0, 10)
        with pytest.raises(ValueError, match="anchor"):
            res.pair_spacing(pw, 8, 10)
        with pytest.raises(ValueError, match="max_dist"):
            res.pair_spacing(pw, 0, -1)
        with pytest.raises(ValueError, match="max_dist"):
            res.pair_spacing(pw, 0, (1 << 20) + 1)
        wide, wide_pw = result_of(hit_arrays([[] for _ in range(300)]), 4), pwmset_of([5] * 300)
        try:
            with pytest.raises(ValueError, match="too large"):
                wide.pair_spacing(wide_pw, 0, 1 << 20)            # 300 x 4 x (2^21 + 1) > 2^31
            c, n = wide.pair_spacing(wide_pw, 0, 1 << 20, 10, 12)
            assert c.shape == (2, 4, (1 << 21) + 1) and not c.any() and not n.any()
        finally:
            wide.close()
            wide_pw.close()
        with pytest.raises(ValueError, match="disagree"):
            res.pair_spacing(other, 0, 10)
        for m0, m1 in ((-1, 2), (3, 2), (0, 9)):
            with pytest.raises(ValueError, match="motif range"):
                res.cooccurrence(m0, m1, out=np.zeros((max(m1 - m0, 0), 8), dtype=np.int64))
            with pytest.raises(ValueError, match="motif range"):
                res.pair_spacing(pw, 0, 10, m0, m1)
        L = _lib.lib()
        assert L.ms_result_cooccurrence(res.h, 0, 8, None) == _lib.MS_ERR_INVALID
        one = np.zeros(1, dtype=np.int64)
        assert L.ms_result_pair_spacing(res.h, pw.h, 0, 0, 8, 10, None, _lib.ptr(one, ctypes.c_int64)) == _lib.MS_ERR_INVALID
        with pytest.raises(IndexError):
            pairs.cooccurrence([[[]] * 4] * 3, motifs=[3])
        # an empty motif range does nothing, whatever the outputs are
        assert L.ms_result_cooccurrence(res.h, 4, 4, None) == _lib.MS_OK
        c, n = res.pair_spacing(pw, 0, 10, 4, 4)
        assert c.shape == (0, 4, 21) and n.shape == (0,)
    finally:
        res.close()
        counts_only.close()
        other.close()
        pw.close()
        sq.close()
