"""
The four plot-data kernels of ms_plotdata.hip (site_hist_kernel, rank_mark_kernel, rank_prefix_kernel, rank_profile_kernel) at the
sizes where they change path, over synthetic hit arrays (ms_result_from_hits): no scan, no oracle, no golden.  Every boundary size
comes from ms_debug_plot_dims (_lib.plot_dims), so the cases follow the constants if one moves.  Run with -m gpu.

Histogram (exact): centres on a bin edge and half a base pair / one base pair either side of it, below the first edge, on the closed
last edge, just past it and 2^40 away, at windows both sides of the LDS histogram's limit; a motif of exactly one block's hits, one
more (a second block, whose LDS counts merge with the first's), and more than the most blocks times a block's hits (the grid is capped
and the stride loops run on); ranges of motifs whose widths differ in parity; empty inputs.

Profile: region counts on the 64-rank word, the window (R / 100), the profile tile with its halo, and the prefix scan's one word per
thread; rows without a site, with a site everywhere, at one end only, on the word seams, random; three rank orders.  Unsmoothed: bit
for bit (two IEEE divisions).  Smoothed: every product k[j] * x is non-negative, so the sum in any order, fused or not, is within
gamma_11 of the exact sum y; |got - ref| <= 16 * 2^-53 * ref against a reference summed in np.longdouble (fuzz_parity.plot_smoothed_differs:
math.fsum on a sample where longdouble is no wider than double).  The bound is derived, not measured.

Expected values: flat_histogram / flat_profiles of tests/test_plot_host.py, which np_histogram / np_profiles there are made of and the
goldens and the reference's literal slice sum hold.
"""
import numpy as np
import pytest

import fuzz_parity as fp
from motifscan_amd import _lib, plot
from test_plot_host import flat_histogram, flat_profiles

pytestmark = pytest.mark.gpu

WIDTHS = (1, 2, 7, 8, 33, 64)
RATIOS = (1.0, 1 / 3, 7 / 13, 1e-300)
FAR = 1 << 40


@pytest.fixture(scope="module", autouse=True)
def device():
    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests need an MI355X (there is no CPU fallback)")
    _lib.set_device(0)


@pytest.fixture(scope="module")
def dims():
    return _lib.plot_dims()


class Hits:
    """Hit arrays per motif -> a device result (ms_result order: by region, then position) and a PWM set of the widths."""

    def __init__(self, widths, R):
        self.widths, self.R = [int(w) for w in widths], int(R)
        self.region, self.pos = [[] for _ in widths], [[] for _ in widths]

    def add(self, m, region, pos):
        self.region[m].append(np.asarray(region, dtype=np.int64).ravel())
        self.pos[m].append(np.asarray(pos, dtype=np.int64).ravel())

    def arrays(self):
        off, region, pos = [0], [], []
        for r, p in zip(self.region, self.pos):
            r = np.concatenate(r) if r else np.zeros(0, dtype=np.int64)
            p = np.concatenate(p) if p else np.zeros(0, dtype=np.int64)
            o = np.lexsort((p, r))
            region.append(r[o]), pos.append(p[o])
            off.append(off[-1] + len(r))
        return np.array(off, dtype=np.int64), np.concatenate(region), np.concatenate(pos)

    def result(self):
        off, region, pos = self.arrays()
        n = len(region)
        return _lib.result_from_hits(len(self.widths), self.R, off, region, pos, np.zeros(n), np.ones(n, dtype=np.int8))

    def pwms(self):
        return _lib.PwmSet.from_matrices([np.full((4, w), 0.25) for w in self.widths])


def lds_extends(dims):
    """(the largest extend whose histogram is counted in LDS, the first that adds to global memory)."""
    lds = dims["hist_lds_bins"]
    ext = max(e for e in range(5 * lds - 10, 5 * lds + 10) if fp.plot_n_bins(e) <= lds)
    assert fp.plot_n_bins(ext) == lds and fp.plot_n_bins(ext + 1) == lds + 1
    return ext, ext + 1


def summits(R, extend, seed):
    """summit - region start per region: all different from their neighbours, some in front of the region, some far behind it."""
    s = np.random.default_rng(seed).integers(0, 2 * extend + 1, size=R).astype(np.int64)
    s[::7] = -3 - np.arange(len(s[::7]))
    s[3::11] += 10 * extend + 1000
    return s


# ---------------------------------------------------------------------------------------------------------- histogram --

EXTENDS = ("0", "4", "5", "17", "250", "lds", "global")


def ladder_doubled_distances(edges, which, W):
    """Twice the distance centre - summit of every hit of the ladder of a W-column motif: each edge of `which` with 0, +-1/2, +-1 bp as
    W's parity allows (2 * d = W mod 2); below the first edge, on the last, half a base pair (a whole one for even W) past it, and
    2^40 bp away on both sides."""
    out = []
    for e in which:
        out += [2 * int(edges[e]) + q for q in (-2, -1, 0, 1, 2)]
    first, last = 2 * int(edges[0]), 2 * int(edges[-1])
    out += [first - 1, first - 2, first - 40, last, last + 1, last + 2, last - 1, last - 2, 2 * FAR + 1, 2 * FAR, -2 * FAR - 1, -2 * FAR]
    return np.array([d for d in out if (d - W) % 2 == 0], dtype=np.int64)


@pytest.mark.parametrize("which", EXTENDS)
def test_histogram_edge_ladder(dims, which):
    ext_lds, ext_global = lds_extends(dims)
    extend = {"lds": ext_lds, "global": ext_global}.get(which) or int(which)
    edges = plot.bin_edges(extend)
    n_edges, lds = len(edges), dims["hist_lds_bins"]
    if which in ("lds", "global"):              # the first three edges, the last three, and those either side of bin hist_lds_bins - 1
        assert (len(edges) - 1 > lds) == (which == "global")
        at = sorted({0, 1, 2, n_edges - 3, n_edges - 2, n_edges - 1, lds - 1, lds})
    else:
        at = list(range(n_edges))
    R = 23
    summit = summits(R, extend, 5)
    h = Hits(WIDTHS, R)
    on_edge = half = 0
    for m, W in enumerate(WIDTHS):
        d2 = ladder_doubled_distances(edges, at, W)
        d2 = np.repeat(d2, 3)                                                  # each of them in three regions, with three summits
        region = (np.arange(len(d2)) * 5 + m) % R
        h.add(m, region, (d2 - W) // 2 + summit[region])
        on_edge += int((np.isin(d2, 2 * edges)).sum())
        half += int((d2 % 2 != 0).sum())
    assert on_edge > 0 and half > 0
    off, region, pos = h.arrays()
    want, want_n = flat_histogram(off, region, pos, WIDTHS, summit, extend)
    # the integer rule the kernel uses agrees with np.histogram on this ladder (held here so that a failure below is the device's)
    W = np.repeat(np.array(WIDTHS, dtype=np.int64), np.diff(off))
    t = 2 * (pos - summit[region]) + W + 2 * (extend + 5)
    n_bins = want.shape[1]
    b = np.where(t == 20 * n_bins, n_bins - 1, t // 20)
    ok = (t >= 0) & (b < n_bins)
    rule = np.zeros_like(want)
    np.add.at(rule, (np.repeat(np.arange(len(WIDTHS)), np.diff(off))[ok], b[ok]), 1)
    assert np.array_equal(rule, want)
    assert want[:, -1].sum() > 0 and want[:, 0].sum() > 0 and want.sum() < off[-1]        # both end bins hold hits, some hits are outside
    res, pw = h.result(), h.pwms()
    try:
        got, got_n = res.site_histogram(pw, summit, extend)
    finally:
        res.close()
        pw.close()
    assert got.shape == want.shape
    assert np.array_equal(got, want), np.argwhere(got != want)[:8].tolist()
    assert np.array_equal(got_n, want_n)


@pytest.fixture(scope="module")
def block_case(dims):
    """Five motifs: exactly one block's hits, one more, more than the capped grid's blocks times a block's hits in ONE bin, as many
    spread over all bins (and beyond both ends), none.  Regions and draws are kept, the positions made per extend."""
    per, cap = dims["hist_hits_per_block"], dims["hist_max_blocks"]
    big = cap * per + 4 * per + 37
    rng = np.random.default_rng(17)
    R = 257
    return {"R": R, "n": [per, per + 1, big, big, 0], "region": [rng.integers(0, R, size=n) for n in (per, per + 1, big, big, 0)],
            "u": [rng.random(n) for n in (per, per + 1, big, big, 0)]}


@pytest.mark.parametrize("which", ["lds", "global"])
def test_histogram_block_merge_and_stride_loop(dims, block_case, which):
    extend = lds_extends(dims)[which == "global"]
    edges = plot.bin_edges(extend)
    n_bins = len(edges) - 1
    widths = (8, 7, 33, 64, 2)
    R = block_case["R"]
    summit = summits(R, extend, 9)
    h = Hits(widths, R)
    lo, hi = 2 * int(edges[0]) - 60, 2 * int(edges[-1]) + 60
    for m, W in enumerate(widths):
        region, u = block_case["region"][m], block_case["u"][m]
        if m == 2:                                                             # one bin, the one past the LDS limit where there is one
            d2 = 2 * int(edges[n_bins - 1]) + (u * 20).astype(np.int64)
        else:
            d2 = lo + (u * (hi - lo)).astype(np.int64)
        d2 += (d2 - W) % 2
        h.add(m, region, (d2 - W) // 2 + summit[region])
    off, region, pos = h.arrays()
    assert np.diff(off).tolist() == block_case["n"]
    assert off[3] - off[2] > dims["hist_max_blocks"] * dims["hist_hits_per_block"]
    want, want_n = flat_histogram(off, region, pos, widths, summit, extend)
    assert np.count_nonzero(want[2]) == 1 and want[2].sum() == block_case["n"][2] and np.count_nonzero(want[3]) > 0.9 * n_bins
    res, pw = h.result(), h.pwms()
    try:
        got, got_n = res.site_histogram(pw, summit, extend)
    finally:
        res.close()
        pw.close()
    assert np.array_equal(got, want), np.argwhere(got != want)[:8].tolist()
    assert np.array_equal(got.sum(axis=1), want.sum(axis=1)) and 0 < got[3].sum() < block_case["n"][3]
    assert np.array_equal(got_n, np.diff(off)) and np.array_equal(got_n, want_n)


def test_histogram_of_motif_ranges_with_widths_of_alternating_parity():
    widths = (7, 8, 33, 64, 1, 2)
    extend, R = 17, 40
    edges = plot.bin_edges(extend)
    summit = summits(R, extend, 3)
    rng = np.random.default_rng(23)
    h = Hits(widths, R)
    for m, W in enumerate(widths):
        n = 60 + 11 * m
        # within half a base pair and a base pair of an edge: the width of a neighbouring row (other parity) moves these across it
        d2 = 2 * edges[rng.integers(0, len(edges), size=n)] + rng.integers(-2, 3, size=n)
        d2 += (d2 - W) % 2
        region = rng.integers(0, R, size=n)
        h.add(m, region, (d2 - W) // 2 + summit[region])
    off, region, pos = h.arrays()
    want, want_n = flat_histogram(off, region, pos, widths, summit, extend)
    for m in range(len(widths) - 1):                                           # the neighbour's width would give another row
        sl = slice(off[m], off[m + 1])
        wrong = flat_histogram(np.array([0, off[m + 1] - off[m]]), region[sl], pos[sl], [widths[m + 1]], summit, extend)[0]
        assert not np.array_equal(wrong[0], want[m])
    res, pw = h.result(), h.pwms()
    try:
        whole, whole_n = res.site_histogram(pw, summit, extend)
        assert np.array_equal(whole, want) and np.array_equal(whole_n, want_n)
        for m0, m1 in ((0, 6), (0, 1), (1, 4), (5, 6), (3, 3)):
            part, part_n = res.site_histogram(pw, summit, extend, m0, m1)
            assert part.shape == (m1 - m0, want.shape[1]) and part_n.shape == (m1 - m0,)
            assert np.array_equal(part, want[m0:m1]) and np.array_equal(part_n, want_n[m0:m1]), (m0, m1)
    finally:
        res.close()
        pw.close()


def test_histogram_of_empty_inputs():
    # hits, but a window of one bin (extend 0: edges -5 and 5, both closed)
    widths = (1, 2, 7)
    R = 9
    summit = summits(R, 10, 1)
    h = Hits(widths, R)
    for m, W in enumerate(widths):
        d2 = np.array([d for d in range(-14, 15) if (d - W) % 2 == 0] * 2, dtype=np.int64)
        region = (np.arange(len(d2)) * 2 + m) % R
        h.add(m, region, (d2 - W) // 2 + summit[region])
    off, region, pos = h.arrays()
    want, want_n = flat_histogram(off, region, pos, widths, summit, 0)
    assert want.shape == (3, 1) and (want > 0).all() and (want[:, 0] < want_n).all()
    res, pw = h.result(), h.pwms()
    try:
        got, got_n = res.site_histogram(pw, summit, 0)
        assert np.array_equal(got, want) and np.array_equal(got_n, want_n)
    finally:
        res.close()
    # no hit at all; no region at all
    for R in (5, 0):
        res = Hits(widths, R).result()
        try:
            got, got_n = res.site_histogram(pw, np.arange(R), 250)
            assert got.shape == (3, 51) and not got.any() and not got_n.any()
            part, _ = res.site_histogram(pw, np.arange(R), 250, 1, 2)
            assert part.shape == (1, 51) and not part.any()
        finally:
            res.close()
    pw.close()


# ------------------------------------------------------------------------------------------------------------ profile --

REGION_COUNTS = {
    "100": lambda d: 100, "101": lambda d: 101, "127": lambda d: 127, "128": lambda d: 128, "129": lambda d: 129, "199": lambda d: 199,
    "200": lambda d: 200,
    "tile-1": lambda d: d["prof_tile"] - 1, "tile": lambda d: d["prof_tile"], "tile+1": lambda d: d["prof_tile"] + 1,
    "tile+half": lambda d: d["prof_tile"] + d["half"], "tile+half+1": lambda d: d["prof_tile"] + d["half"] + 1,
    "2tile": lambda d: 2 * d["prof_tile"],
    "scan": lambda d: 64 * d["scan_threads"], "scan+1": lambda d: 64 * d["scan_threads"] + 1, "scan+64": lambda d: 64 * d["scan_threads"] + 64,
    "scan+65": lambda d: 64 * d["scan_threads"] + 65, "2scan+1": lambda d: 128 * d["scan_threads"] + 1,
}
LARGEST = "2scan+1"


def rank_rows(R, seed, big=0):
    """The ranks that hold a site, per row (with repeats: a region hit twice): none, every rank, rank 0 only, rank R - 1 only, the
    ranks either side of every word seam, 30 % at random -- and, for big > 0, `big` draws over all ranks."""
    rng = np.random.default_rng(seed)
    every = np.concatenate([np.arange(R), rng.integers(0, R, size=R // 10 + 1)])
    k = np.arange(R)
    rows = [np.zeros(0, dtype=np.int64), every, np.array([0, 0]), np.array([R - 1]), k[(k % 64 == 63) | (k % 64 == 0)],
            np.flatnonzero(rng.random(R) < 0.3)]
    if big:
        rows.append(rng.integers(0, R, size=big))
    return rows


def orders(R, seed):
    return {"identity": np.arange(R), "reversed": np.arange(R)[::-1].copy(), "permuted": np.random.default_rng(seed).permutation(R)}


def ranked_hits(rows, order, R):
    """A Hits whose motif m has its sites in the regions at the ranks rows[m] of `order`."""
    h = Hits([10] * len(rows), R)
    for m, ranks in enumerate(rows):
        h.add(m, order[ranks], np.arange(len(ranks)) % 50)
    return h


def check_profiles(res, off, region, order, ratio, k):
    P = len(off) - 1
    want = flat_profiles(off, region, order, ratio, np.arange(P), False)
    raw = res.rank_profile(order, ratio, smoothed=False)
    assert raw.shape == want.shape
    assert fp.same_bits(raw, want), np.argwhere(raw != want)[:8].tolist()
    sm = res.rank_profile(order, ratio, k)
    for m in range(P):
        bad = fp.plot_smoothed_differs(sm[m], want[m], k)
        assert bad is None, f"row {m}: {bad}"
    return want, sm


@pytest.mark.parametrize("size", list(REGION_COUNTS))
def test_profile_rows_at_region_count(dims, size):
    R = REGION_COUNTS[size](dims)
    k = plot.smoothing_weights()
    assert (k >= 0).all()                                                        # what the smoothed bound rests on
    big = dims["hist_max_blocks"] * dims["hist_hits_per_block"] + 4 * dims["hist_hits_per_block"] + 37 if size == LARGEST else 0
    rows = rank_rows(R, 41, big)
    ratio = np.array([RATIOS[m % 4] for m in range(len(rows))])
    for name, order in orders(R, 43).items():
        h = ranked_hits(rows, order, R)
        off, region, _ = h.arrays()
        if big:
            assert off[-1] - off[-2] > dims["hist_max_blocks"] * dims["hist_hits_per_block"]
        res = h.result()
        try:
            want, _ = check_profiles(res, off, region, order, ratio, k)
        finally:
            res.close()
        f = R // 100
        assert not want[0].any() and np.all(want[1] == 1.0 / ratio[1]), name       # no site: 0; a site everywhere: 1 / ratio_control
        # rank 0 lies in the windows of ranks 0 .. f, rank R - 1 in those of ranks R - f .. R - 1 (the window is [i - f, i + f))
        assert np.flatnonzero(want[2]).tolist() == list(range(f + 1)) and np.flatnonzero(want[3]).tolist() == list(range(R - f, R)), name
    # a result without any hit (the mark kernel is not launched)
    res = Hits([10, 10], R).result()
    try:
        for smoothed in (False, True):
            assert not res.rank_profile(np.arange(R), np.ones(2), k, smoothed=smoothed).any()
    finally:
        res.close()


def test_profile_chunks_and_a_device_buffer_at_the_first_multi_word_size(dims):
    import torch
    R = 64 * dims["scan_threads"] + 1
    k = plot.smoothing_weights()
    rows = rank_rows(R, 47)
    order = orders(R, 53)["permuted"]
    ratio = np.array([RATIOS[m % 4] for m in range(len(rows))])
    P = len(rows)
    res = ranked_hits(rows, order, R).result()
    try:
        for smoothed in (True, False):
            whole = res.rank_profile(order, ratio, k, smoothed=smoothed)
            parts = [res.rank_profile(order, ratio[m0:m1], k, m0, m1, smoothed=smoothed) for m0, m1 in ((0, 1), (1, 4), (4, 4), (4, P))]
            assert fp.same_bits(np.concatenate(parts), whole)
            dev = torch.full((3, R), -1.0, dtype=torch.float64, device="cuda")
            res.rank_profile(order, ratio[2:5], k, 2, 5, smoothed=smoothed, out=int(dev.data_ptr()))
            torch.cuda.synchronize()
            assert fp.same_bits(dev.cpu().numpy(), whole[2:5])
    finally:
        res.close()
