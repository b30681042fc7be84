"""
Site stacks on the device (ms_result_site_base_counts; motifscan_amd.sitestack, Scanner.site_base_counts) against the hand-written
cases and the sequential restatement of tests/test_sitestack_host.py.  Every comparison is exact: the counts are integer reductions.
Most results are made of chosen hit arrays (ms_result_from_hits), which places every boundary where the test wants it -- the first
region's left flank (an address below the plane), the last region's right flank (the pad), the 32-column fetch steps, the chunk of a
block, the widest row counted in LDS -- with the sizes from ms_debug_sitestack_dims; the last tests scan.  Run with -m gpu.
"""
from types import SimpleNamespace

import numpy as np
import pytest

from motifscan_amd import _lib, sitestack, synth
from motifscan_amd.scanner import Scanner
from test_sitestack_host import HAND, hand_expected, hit_arrays, random_case

pytestmark = pytest.mark.gpu

DIMS = _lib.sitestack_dims()                       # constants of the build: no device
CHUNK, LDS_C = DIMS["chunk_hits"], DIMS["lds_columns"]


@pytest.fixture(scope="module", autouse=True)
def device():
    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests need an MI355X (there is no CPU fallback)")
    _lib.set_device(0)


class Case:
    """A result of chosen hits with the PWM set (widths only) and the sequence set it goes with."""

    def __init__(self, hits, widths, seqs, n_regions=None):
        self.hits, self.widths, self.seqs = hits, list(widths), list(seqs)
        offsets, seq_idx, pos, strand = hits
        self.res = _lib.result_from_hits(len(offsets) - 1, len(seqs) if n_regions is None else n_regions, offsets, seq_idx, pos,
                                         np.zeros(len(pos)), strand)
        self.pw = _lib.PwmSet.from_matrices([np.ones((4, w)) for w in widths])
        self.sq = _lib.SeqSet.from_strings(self.seqs)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.res.close()
        self.pw.close()
        self.sq.close()

    def device(self, flank, dinuc=True, **kw):
        return self.res.site_base_counts(self.pw, self.sq, flank, dinuc=dinuc, **kw)

    def host(self, flank):
        return sitestack.site_base_counts_host(*self.hits, self.widths, self.seqs, flank, dinuc=True)


def check(case, flank, ranges=(), want=None):
    """Device == restatement for counts, dinuc and n_sites; the call without dinuc gives the same counts; sub-ranges give the same rows."""
    want = case.host(flank) if want is None else want
    counts, dinuc, n_sites = case.device(flank)
    assert counts.dtype == np.int64 and counts.shape == want.counts.shape and dinuc.shape == want.dinuc.shape
    assert np.array_equal(counts, want.counts)
    assert np.array_equal(dinuc, want.dinuc)
    assert np.array_equal(n_sites, want.n_sites)
    plain, none, n2 = case.device(flank, dinuc=False)
    assert none is None and np.array_equal(plain, want.counts) and np.array_equal(n2, want.n_sites)
    for m0, m1 in ranges:
        c, d, n = case.device(flank, m0=m0, m1=m1)
        assert c.shape[0] == m1 - m0 and np.array_equal(c, want.counts[m0:m1]) and np.array_equal(d, want.dinuc[m0:m1]), (m0, m1)
        assert np.array_equal(n, want.n_sites[m0:m1]), (m0, m1)
    return want


def edge_sites(seqs, widths, rng=None, extra=0):
    """Per motif: both strands at pos 0 and L - W of every region that holds the motif, and `extra` random positions."""
    sites = []
    for W in widths:
        per = []
        for r, s in enumerate(seqs):
            if len(s) < W:
                continue
            ps = {0, len(s) - W}
            if extra and rng is not None:
                ps |= set(rng.integers(0, len(s) - W + 1, size=extra).tolist())
            per += [(r, int(p), st) for p in ps for st in (1, 2)]
        sites.append(per)
    return sites


def random_seqs(rng, lengths, letters="ACGT" * 5 + "acgtNnRYK"):
    return ["".join(rng.choice(list(letters), size=int(n))) for n in lengths]


# ------------------------------------------------------------------------------------------------------------- hand cases --

@pytest.mark.parametrize("case", HAND, ids=[c["name"] for c in HAND])
def test_hand_written_cases(case):
    want_counts, want_dinuc = hand_expected(case)
    with Case(hit_arrays(case["sites"]), case["widths"], case["seqs"]) as c:
        counts, dinuc, n_sites = c.device(case["flank"])
        assert np.array_equal(counts, want_counts)
        assert np.array_equal(dinuc, want_dinuc)
        assert n_sites.tolist() == [len(s) for s in case["sites"]]
        assert np.array_equal(c.device(case["flank"], dinuc=False)[0], want_counts)


# ------------------------------------------------------------------------------------------------------------ region edges --

@pytest.mark.parametrize("flank", [1, 15, 16, 17, 64])
def test_flanks_at_the_edges_of_back_to_back_regions(flank):
    """Region lengths that are no multiple of 16 or 32, a one-base region and regions shorter than the flank, back to back: sites at
    pos 0 and L - W of every region, so the first region's left flank lies below the planes' first word, the last region's right flank
    in the pad, and every other flank in a neighbour's bases -- all of them slot 5."""
    rng = np.random.default_rng(flank)
    seqs = random_seqs(rng, [1, 3, 17, 33, 47, 5, 100, 31, 1, 64, 9])
    widths = [1, 3, 9]
    with Case(hit_arrays(edge_sites(seqs, widths)), widths, seqs) as c:
        want = check(c, flank)
        W0 = want.columns(0)
        assert W0[:flank, 5].sum() > 0 and W0[flank + 1:, 5].sum() > 0 and want.counts[:, :, :4].sum() > 0
    first_only = [s for s in seqs[:1]] + seqs[3:4]                              # the one-base region first in the set, one region behind it
    with Case(hit_arrays(edge_sites(first_only, [1])), [1], first_only) as c:
        check(c, flank)


# ------------------------------------------------------------------------------------------------------------- fetch steps --

@pytest.mark.parametrize("W, flank", [(1, 0), (1, 15), (2, 15), (1, 16), (31, 16), (32, 16), (1, 32), (33, 0), (64, 32), (70, 64)])
def test_columns_across_the_32_column_fetch_steps(W, flank):
    """W + 2 * flank at 1, 31, 32, 33, 63, 64, 65, 33, 128 and 198 columns: the last fetch step of a site holds 1 .. 32 columns, and on
    '-' the steps run from the other end.  A second, narrower motif shares the pitch."""
    rng = np.random.default_rng(100 * W + flank)
    seqs = random_seqs(rng, [W, W + 1, W + 31, W + 40, 2 * W + 70, 3, W + 16])
    widths = [W, max(1, W // 2)]
    with Case(hit_arrays(edge_sites(seqs, widths, rng, extra=2)), widths, seqs) as c:
        want = check(c, flank, ranges=[(1, 2)])
        assert want.counts.shape[1] == W + 2 * flank and want.n_sites.min() > 0


@pytest.mark.parametrize("C", [LDS_C, LDS_C + 1])
def test_one_column_inside_and_one_past_the_lds_path(C):
    """C = max_width + 2 * flank at the widest pitch counted in LDS and one past it (global 64-bit adds), with and without dinuc."""
    rng = np.random.default_rng(C)
    flank = 2
    W = C - 2 * flank
    seqs = random_seqs(rng, [W + 5, W, W + 37])
    widths = [5, W]
    with Case(hit_arrays(edge_sites(seqs, widths, rng, extra=1)), widths, seqs) as c:
        want = check(c, flank, ranges=[(0, 1), (1, 2)])
        assert want.counts.shape[1] == C and want.counts[1, C - 1].sum() == want.n_sites[1] > 0


# -------------------------------------------------------------------------------------------------------- chunk boundaries --

def test_motifs_around_the_chunk_of_a_block():
    """CHUNK - 1, CHUNK, CHUNK + 1 and 3 CHUNK + 5 hits, an empty motif between two full ones, and sub-ranges equal to the rows of the
    full call."""
    rng = np.random.default_rng(7)
    seqs = random_seqs(rng, rng.integers(20, 60, size=40))
    widths = [3, 4, 2, 5, 3]
    n_hits = [CHUNK - 1, CHUNK, 0, CHUNK + 1, 3 * CHUNK + 5]
    sites = []
    for W, n in zip(widths, n_hits):
        r = rng.integers(0, len(seqs), size=n)
        sites.append([(int(x), int(rng.integers(0, len(seqs[x]) - W + 1)), int(rng.integers(1, 3))) for x in r])
    P = len(widths)
    with Case(hit_arrays(sites), widths, seqs) as c:
        want = check(c, 1, ranges=[(0, 1), (P - 1, P), (2, 2), (3, 3), (1, 4)])
        assert want.n_sites.tolist() == n_hits and not want.counts[2].any()


# ------------------------------------------------------------------------------------------------------------ hot counters --

@pytest.mark.parametrize("letter, slot", [("A", 0), ("N", 4)])
def test_every_lane_of_every_wave_in_one_slot(letter, slot):
    """Poly-A regions (then N only): all sites of more than two chunks land in the same counter of every column."""
    W, n, flank = 4, 2 * CHUNK + 10, 2
    seqs = [letter * 50] * 4
    sites = [[(k % 4, 2 + k % 40, 1) for k in range(n)]]
    with Case(hit_arrays(sites), [W], seqs) as c:
        counts, dinuc, n_sites = c.device(flank)
        want = np.zeros((1, W + 2 * flank, 6), dtype=np.int64)
        want[0, :, slot] = n
        assert np.array_equal(counts, want) and n_sites.tolist() == [n]
        want_d = np.zeros((1, W + 2 * flank, 16), dtype=np.int64)
        if slot == 0:
            want_d[0, :-1, 0] = n
        assert np.array_equal(dinuc, want_d)
        minus = [[(r, p, 2) for r, p, _ in sites[0]]]                          # '-': T under every column
    if slot == 0:
        with Case(hit_arrays(minus), [W], seqs) as c:
            counts, dinuc, _ = c.device(flank)
            assert counts[0, :, 3].tolist() == [n] * (W + 2 * flank) and counts.sum() == n * (W + 2 * flank)
            assert dinuc[0, :-1, 15].tolist() == [n] * (W + 2 * flank - 1) and dinuc.sum() == n * (W + 2 * flank - 1)


def test_every_flank_column_outside():
    W, n, flank = 4, 2 * CHUNK + 10, 3
    seqs = ["ACGT"] * 5
    sites = [[(k % 5, 0, 1 + k % 2) for k in range(n)]]
    with Case(hit_arrays(sites), [W], seqs) as c:
        want = check(c, flank)
        assert want.counts[0, :flank, 5].tolist() == [n] * flank and want.counts[0, flank + W:, 5].tolist() == [n] * flank
        assert want.counts[0, flank:flank + W, :4].sum() == n * W           # ACGT and its reverse complement ACGT


# ---------------------------------------------------------------------------------------------------------------- non-ACGT --

def test_runs_of_n_iupac_letters_and_lower_case():
    rng = np.random.default_rng(11)
    for seed in range(8):
        seqs, widths, sites = random_case(rng, max_len=int(rng.choice([6, 40, 90])))
        seqs[0] = seqs[0] + "N" * 37 + "acgtn" + "RYKMSWBDHV"
        with Case(hit_arrays(sites), widths, seqs) as c:
            check(c, int(rng.choice([0, 3, 20, 64])))
    seqs = ["ACGT" + "N" * 70 + "acgu", "nnnnnnnn", "RYKMacgtACGT"]
    with Case(hit_arrays(edge_sites(seqs, [4, 8], rng, extra=3)), [4, 8], seqs) as c:
        want = check(c, 5)
        assert want.counts[:, :, 4].sum() > 0


# ------------------------------------------------------------------------------------------------------------------- scans --

class ChromGenome:
    """One synthetic chromosome, with what Scanner reads of a genome (scanner.py:81-87)."""

    def __init__(self, seq):
        self.seq = seq
        self.chrom_sizes = {"chr1": len(seq)}

    def fetch_sequence(self, chrom, start, end):
        return self.seq[start:end]


@pytest.fixture(scope="module")
def rnd_scan(rnd):
    off = rnd["seq_offsets"]
    genome = ChromGenome("".join(rnd["seqs"]))
    regions = [SimpleNamespace(chrom="chr1", start=int(off[i]), end=int(off[i + 1]), summit=int(off[i]), score=None) for i in range(len(off) - 1)]
    pwms = [SimpleNamespace(matrix=m, length=m.shape[1], cutoffs={"1e-3": float(c)}, matrix_id=f"M{i}", name=f"m{i}")
            for i, (m, c) in enumerate(zip(rnd["mats"], rnd["cutoff_by_key"]["1e-3"]))]
    return genome, regions, pwms


@pytest.mark.parametrize("remove_dup", [False, True])
def test_scanner_site_base_counts_against_the_restatement(rnd, rnd_scan, remove_dup, oracle):
    genome, regions, pwms = rnd_scan
    widths = [p.length for p in pwms]
    flank = 8
    sc = Scanner(genome, regions, window_size=0, strand="both", p_value="1e-3", remove_dup=remove_dup)
    try:
        got = sc.site_base_counts(pwms, flank=flank, dinuc=True)
        a = sc.scan_motifs_arrays(pwms)
        pos = a["start"] - np.asarray(sc.seq_starts, dtype=np.int64)[a["region"]]
        want = sitestack.site_base_counts_host(a["motif_offsets"], a["region"], pos, a["strand"], widths, rnd["seqs"], flank, dinuc=True)
        a["_result"].close()
    finally:
        sc.close()
    assert isinstance(got, sitestack.SiteStack) and got.flank == flank and np.array_equal(got.widths, widths)
    assert np.array_equal(got.counts, want.counts) and np.array_equal(got.dinuc, want.dinuc) and np.array_equal(got.n_sites, want.n_sites)
    assert got.n_sites.sum() > 1000 and got.pfm(3).shape == (4, widths[3])
    if not remove_dup:                                                          # the restatement over the ORACLE's hits: the same arrays
        flat = oracle.c_scan_motif([p.matrix.tolist() for p in pwms], [p.cutoffs["1e-3"] for p in pwms], rnd["seqs"], 3, 1)
        hits = hit_arrays([[(int(s), int(p), int(d)) for s, p, _, d in per] for per in flat])
        ref = sitestack.site_base_counts_host(*hits, widths, rnd["seqs"], flank, dinuc=True)
        assert np.array_equal(got.counts, ref.counts) and np.array_equal(got.dinuc, ref.dinuc) and np.array_equal(got.n_sites, ref.n_sites)


def test_module_function_from_a_view_and_from_plain_lists(rnd, rnd_scan):
    genome, regions, pwms = rnd_scan
    sc = Scanner(genome, regions[:80], window_size=0, p_value="1e-3", remove_dup=True)
    sites = sc.scan_motifs(pwms)
    try:
        a = sites.arrays()
        starts = np.asarray(sc.seq_starts, dtype=np.int64)
        widths = [p.length for p in pwms]
        want = sitestack.site_base_counts_host(a["motif_offsets"], a["region"], a["start"] - starts[a["region"]], a["strand"], widths,
                                               rnd["seqs"][:80], 4, dinuc=True)
        rows = [7, 3, 4, 5, 47]
        got = sitestack.site_base_counts(sites, pwms, sc._seqset(), flank=4, dinuc=True)
        assert np.array_equal(got.counts, want.counts) and np.array_equal(got.dinuc, want.dinuc) and np.array_equal(got.n_sites, want.n_sites)
        sub = sitestack.site_base_counts(sites.to_lists(), pwms, rnd["seqs"][:80], flank=4, motifs=rows, seq_starts=starts)
        assert sub.dinuc is None and np.array_equal(sub.counts, want.counts[rows]) and np.array_equal(sub.widths, np.asarray(widths)[rows])
        assert np.array_equal(sub.pfm(1), want.pfm(3)) and np.array_equal(sub.columns(4), want.columns(47))
        none = sitestack.site_base_counts(sites, pwms, sc._seqset(), flank=4, motifs=[])
        assert none.counts.shape == (0, want.counts.shape[1], 6)
    finally:
        sites.close()
        sc.close()


def test_regions_scanned_once_with_a_set_cut_from_the_resident_genome(rnd):
    """ms_scan_regions_once over overlapping regions of a resident genome; the sequences come from ms_seqset_from_genome over the same
    regions."""
    chrom = "".join(rnd["seqs"][:40])
    g = _lib.ResidentGenome({"chr1": chrom})
    starts = np.arange(0, 6000, 130, dtype=np.int64)
    ends = starts + 301
    idx = np.zeros(len(starts), dtype=np.int32)
    pw = _lib.PwmSet.from_matrices(rnd["mats"], rnd["cutoff_by_key"]["1e-3"])
    sq = g.extract(idx, starts, ends)
    res = _lib.scan_regions_once(pw, g, idx, starts, ends, 3)
    try:
        h = res.hits()
        seqs = [chrom[s:e] for s, e in zip(starts, ends)]
        widths = [m.shape[1] for m in rnd["mats"]]
        want = sitestack.site_base_counts_host(h["motif_offsets"], h["seq_idx"], h["pos"], h["strand"], widths, seqs, 10, dinuc=True)
        counts, dinuc, n_sites = res.site_base_counts(pw, sq, 10, dinuc=True)
        assert np.array_equal(counts, want.counts) and np.array_equal(dinuc, want.dinuc) and np.array_equal(n_sites, want.n_sites)
        assert n_sites.sum() > 500
    finally:
        res.close()
        sq.close()
        pw.close()
        g.close()


# ---------------------------------------------------------------------------------------------- additivity and determinism --

def test_region_shards_add_up_and_two_runs_give_the_same_bytes():
    rng = np.random.default_rng(5)
    seqs, widths = random_seqs(rng, rng.integers(10, 80, size=30)), [6, 11, 2]
    sites = edge_sites(seqs, widths, rng, extra=4)
    cut = 13
    with Case(hit_arrays(sites), widths, seqs) as whole:
        a = whole.device(7)
        b = whole.device(7)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)) and a[0].any() and a[1].any()
    parts = []
    for lo, hi in ((0, cut), (cut, len(seqs))):
        shard = [[(r - lo, p, s) for r, p, s in per if lo <= r < hi] for per in sites]
        with Case(hit_arrays(shard), widths, seqs[lo:hi]) as c:
            parts.append(c.device(7))
    for whole_arr, x, y in zip(a, *parts):
        assert np.array_equal(whole_arr, x + y)


def test_outputs_in_device_memory_equal_the_host_ones():
    import torch
    rng = np.random.default_rng(6)
    seqs, widths = random_seqs(rng, rng.integers(10, 80, size=20)), [6, 11, 2, 9]
    with Case(hit_arrays(edge_sites(seqs, widths, rng, extra=3)), widths, seqs) as c:
        host = c.device(3, m0=1, m1=4)
        C = max(widths) + 6
        dev = [torch.full(shape, -1, dtype=torch.int64, device="cuda") for shape in ((3, C, 6), (3, C, 16), (3,))]
        torch.cuda.synchronize()                                  # the fills run on torch's stream, the library writes on its own
        ptrs = tuple(int(t.data_ptr()) for t in dev)
        assert c.device(3, m0=1, m1=4, out=ptrs) == ptrs
        torch.cuda.synchronize()
        for h, t in zip(host, dev):
            assert h.tobytes() == t.cpu().numpy().tobytes() and h.any()
        mixed = c.device(3, m0=1, m1=4, out=(None, ptrs[1], None))            # host counts, device dinuc
        assert np.array_equal(mixed[0], host[0]) and mixed[1] == ptrs[1] and np.array_equal(mixed[2], host[2])


def test_empty_results_and_empty_ranges():
    with Case(hit_arrays([[], []]), [3, 5], ["ACGT", "AC"]) as c:
        counts, dinuc, n_sites = c.device(2)
        assert counts.shape == (2, 9, 6) and not counts.any() and not dinuc.any() and n_sites.tolist() == [0, 0]
        counts, dinuc, n_sites = c.device(2, m0=1, m1=1)
        assert counts.shape == (0, 9, 6) and n_sites.shape == (0,)


# ---------------------------------------------------------------------------------------------------------------- refusals --

def test_refused_calls():
    seqs = ["ACGTACGTAC", "GGGTTTAAAC"]
    widths = [3, 4]
    hits = hit_arrays([[(0, 0, 1), (1, 7, 2)], [(1, 6, 1)]])
    with Case(hits, widths, seqs) as c:
        for kw in (dict(flank=-1), dict(flank=65), dict(flank=0, flags=1), dict(flank=0, m0=1, m1=3), dict(flank=0, m0=-1, m1=1), dict(flank=0, m0=2, m1=1)):
            with pytest.raises(ValueError):
                c.device(**kw)
        pw3 = _lib.PwmSet.from_matrices([np.ones((4, 3))] * 3)
        sq1, sq3 = _lib.SeqSet.from_strings(seqs[:1]), _lib.SeqSet.from_strings(seqs + ["ACGT"])
        try:
            with pytest.raises(ValueError, match="number of PWMs"):
                c.res.site_base_counts(pw3, c.sq, 0)
            for sq in (sq1, sq3):
                with pytest.raises(ValueError, match="regions"):
                    c.res.site_base_counts(c.pw, sq, 0)
            with pytest.raises(ValueError):
                c.res.site_base_counts(c.pw, c.sq, 0, out=(np.zeros((2, 4, 6), dtype=np.int32), None, None))
            with pytest.raises(ValueError):
                c.res.site_base_counts(c.pw, c.sq, 0, out=(None, np.zeros((2, 4, 16), dtype=np.int64), None))     # dinuc not asked for
            rc = _lib.lib().ms_result_site_base_counts(c.res.h, c.pw.h, c.sq.h, 0, 0, 2, 0, None, None, None, None)
            assert rc == _lib.MS_ERR_INVALID                                   # NULL counts
            vals, w8, cutoffs = synth.load_motif_set(8)
            bases, offsets = synth.make_regions(200, 300, seed=3)
            pw8, sq8 = _lib.PwmSet(vals, w8, cutoffs), _lib.SeqSet(bases, offsets)
            counts_only = _lib.scan(pw8, sq8, 3, _lib.MS_SCAN_COUNTS_ONLY)
            try:
                with pytest.raises(ValueError, match="counts-only"):
                    counts_only.site_base_counts(pw8, sq8, 0)
            finally:
                counts_only.close()
                pw8.close()
                sq8.close()
        finally:
            pw3.close()
            sq1.close()
            sq3.close()


@pytest.mark.parametrize("bad", ["pos + W = L + 1", "pos = -1", "the last region against a shorter set"])
@pytest.mark.parametrize("wide", [False, True])
def test_sites_outside_their_region_are_refused_with_the_outputs_zeroed(bad, wide):
    """Only ms_result_from_hits or the wrong sequence set can bring such a site: it is found on the device while counting -- on the LDS
    path and on the global one -- nothing is read for it, and the outputs are zero afterwards."""
    seqs = ["ACGTACGTAC", "GGGTTTAAAC", "ACGTTGCA"]
    W2 = LDS_C + 1 if wide else 4
    widths = [3, W2]
    good = [(0, 0, 1), (1, 7, 2), (2, 5, 1)]
    n_regions = len(seqs)
    if bad == "pos + W = L + 1":
        sites = [good + [(2, 6, 1)], []]
    elif bad == "pos = -1":
        sites = [good[:2] + [(2, -1, 2)], []]
    else:                                                                       # regions of the same number, but the last one too short for the site
        sites = [good, []]
        seqs = seqs[:2] + ["ACGTTGC"]
    hits = hit_arrays([sorted(s) for s in sites])
    with Case(hits, widths, seqs, n_regions) as c:
        C = max(widths) + 4
        out = (np.full((2, C, 6), -7, dtype=np.int64), np.full((2, C, 16), -7, dtype=np.int64), np.full(2, -7, dtype=np.int64))
        with pytest.raises(ValueError, match="inside its region"):
            c.device(2, out=out)
        assert not out[0].any() and not out[1].any() and not out[2].any()
    if bad.startswith("the last region"):                                      # seq_idx = R - 1 against a one-region-shorter set: refused by R
        with Case(hit_arrays([good, []]), widths, seqs[:2], 3) as c:
            with pytest.raises(ValueError, match="regions"):
                c.device(2)
