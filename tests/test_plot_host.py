"""
motifscan_amd.plot on the host (no GPU): the pieces that stay in numpy (bin edges, x, the ranking, the smoothing weights and the host
smooth() of the histogram rows), argument validation and the drop-ins' early returns -- against the reference's own output
(tests/golden/ref_plot.npz, made by tests/golden/make_golden_plot.py).  The two device calls are replaced by numpy restatements of
the contract (`np_histogram`, `np_profiles` below; the GPU tests compare the device against the same restatements).
"""
import ctypes
import logging
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

from motifscan_amd import _lib, plot
from motifscan_amd.sites import MotifSite, MotifSites

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_plot.npz")
DIST = ("dist_w200", "dist_w0", "dist_w100", "dist_w35")
ENR = ("enr_100", "enr_101", "enr_2003")


@pytest.fixture(scope="module")
def gold():
    d = np.load(GOLDEN)
    return {k: d[k] for k in d.files}


# ------------------------------------------------------------------------------- the contract, restated in numpy --

def flat_sites(motif_sites):
    """(motif_offsets, region, genome start) of a MotifSites or of nested lists."""
    if isinstance(motif_sites, MotifSites):
        a = motif_sites.arrays()
        return a["motif_offsets"], a["region"], a["start"]
    off, region, start = [0], [], []
    for per in motif_sites:
        for r, sites in enumerate(per):
            for s in sites:
                region.append(r)
                start.append(s.start)
        off.append(len(region))
    return np.array(off, dtype=np.int64), np.array(region, dtype=np.int64), np.array(start, dtype=np.int64)


def flat_histogram(off, region, start, widths, summits, extend):
    """plot.py:65-68 over flat hit arrays: np.histogram of start + W / 2 - summit[region] per motif -> (counts, n_sites)."""
    off, region, start = np.asarray(off, dtype=np.int64), np.asarray(region, dtype=np.int64), np.asarray(start, dtype=np.int64)
    summits = np.asarray(summits, dtype=np.int64)
    edges = np.arange(-extend - 5, extend + 6, 10)
    counts = np.zeros((len(widths), len(edges) - 1), dtype=np.int64)
    for m, w in enumerate(widths):
        sl = slice(off[m], off[m + 1])
        d = start[sl] + int(w) / 2 - summits[region[sl]]
        counts[m] = np.histogram(d, bins=edges)[0]
    return counts, np.diff(off)


def flat_profiles(off, region, order, ratio, rows, smoothed):
    """plot.py:133-142 per motif of `rows` over flat hit arrays: prefix counts over the ranked has-site flags, the window ratio (two
    divisions), smooth().  ratio is indexed by motif."""
    R = len(order)
    f = R // 100
    idx = np.arange(R)
    head, tail = np.maximum(0, idx - f), np.minimum(idx + f, R)
    out = np.empty((len(rows), R))
    for i, m in enumerate(rows):
        has = np.zeros(R, dtype=bool)
        has[region[off[m]:off[m + 1]]] = True
        pre = np.concatenate([[0], np.cumsum(has[order])])
        y = ((pre[tail] - pre[head]) / (tail - head)) / ratio[m]
        out[i] = plot.smooth(y) if smoothed else y
    return out


def np_histogram(motif_sites, pwms, summits, extend):
    """plot.py:65-68: np.histogram of site.start + W / 2 - summit per motif -> (counts, n_sites)."""
    off, region, start = flat_sites(motif_sites)
    return flat_histogram(off, region, start, [pwm.length for pwm in pwms], summits, extend)


def np_profiles(motif_sites, order, ratio, rows, smoothed):
    """plot.py:133-142 per motif: prefix counts over the ranked has-site flags, the window ratio (two divisions), smooth()."""
    off, region, _ = flat_sites(motif_sites)
    return flat_profiles(off, region, order, ratio, rows, smoothed)


@pytest.fixture
def host_device(monkeypatch):
    monkeypatch.setattr(plot, "_device_histogram", np_histogram)
    monkeypatch.setattr(plot, "_device_profiles", np_profiles)


# ------------------------------------------------------------------------------------------------- golden inputs --

class Pwm:
    def __init__(self, i, width):
        self.matrix_id, self.name, self.length = f"MA{i:04d}.1", f"motif-{i}/w{width}", int(width)
        self.matrix = np.full((4, int(width)), 0.25)


def nested(P, R, off, region, start, score, strand):
    out = [[[] for _ in range(R)] for _ in range(P)]
    for m in range(P):
        for k in range(off[m], off[m + 1]):
            out[m][region[k]].append(MotifSite(int(start[k]), float(score[k]), "+" if strand[k] == 1 else "-"))
    return out


def dist_inputs(g, name, as_view=False):
    """(regions, pwms, motif_sites, window_size) of a golden case; as_view: a MotifSites over sequences that start at the regions."""
    starts, ends, summits = g[f"{name}_starts"], g[f"{name}_ends"], g[f"{name}_summits"]
    regions = [SimpleNamespace(chrom="chr1", start=int(s), end=int(e), summit=int(u), score=1.0) for s, e, u in zip(starts, ends, summits)]
    pwms = [Pwm(i, w) for i, w in enumerate(g[f"{name}_widths"])]
    off, region, start = g[f"{name}_motif_offsets"], g[f"{name}_region"], g[f"{name}_start"]
    if as_view:
        sites = MotifSites(off, region, start - starts[region], g[f"{name}_score"], g[f"{name}_strand"], starts)
    else:
        sites = nested(len(pwms), len(regions), off, region, start, g[f"{name}_score"], g[f"{name}_strand"])
    return regions, pwms, sites, int(g[f"{name}_window_size"])


def enr_inputs(g, name, as_view=False, control="lists"):
    scores = g[f"{name}_scores"]
    R, Rc = len(scores), int(g[f"{name}_n_control_regions"])
    regions = [SimpleNamespace(chrom="chr1", start=1000 * i, end=1000 * i + 500, summit=1000 * i + 250, score=float(s))
               for i, s in enumerate(scores)]
    ai = [g[f"{name}_in_{k}"] for k in ("motif_offsets", "region", "start", "score", "strand")]
    ac = [g[f"{name}_ctl_{k}"] for k in ("motif_offsets", "region", "start", "score", "strand")]
    P = len(ai[0]) - 1
    pwms = [Pwm(i, 10) for i in range(P)]
    sites = MotifSites(ai[0], ai[1], ai[2], ai[3], ai[4], np.zeros(R, dtype=np.int64)) if as_view else nested(P, R, *ai)
    if control == "counts":
        ctl = plot.RegionCounts(np.array([len(np.unique(ac[1][ac[0][m]:ac[0][m + 1]])) for m in range(P)]), Rc)
    else:
        ctl = nested(P, Rc, *ac)
    return regions, pwms, sites, ctl


# ------------------------------------------------------------------------------------------------------------ tests --

@pytest.mark.parametrize("name", DIST)
def test_bin_edges_and_x_match_the_reference(gold, name):
    ws = int(gold[f"{name}_window_size"])
    extend = (ws if ws > 0 else int(gold[f"{name}_ends"][0] - gold[f"{name}_starts"][0])) // 2
    edges = plot.bin_edges(extend)
    assert edges[0] == -extend - 5 and np.all(np.diff(edges) == 10) and edges[-1] <= extend + 5
    assert np.array_equal(plot.bin_centres(edges), gold[f"{name}_x"])
    # the device derives the bin count from extend alone (include/motifscan_amd.h)
    assert len(edges) - 1 == (2 * extend + 11 + 9) // 10 - 1


def test_smoothing_weights_are_numpys_hanning_reversed():
    k = plot.smoothing_weights()
    w = np.hanning(11)
    assert k.shape == (11,) and k.flags.c_contiguous
    assert np.array_equal(k, (w / w.sum())[::-1])
    # what np.convolve does with them: out[i] = sum_j k[j] * x[i - 5 + j] in the interior
    x = np.random.default_rng(1).random(40)
    y = plot.smooth(x)
    i = 20
    assert y[i] == pytest.approx(sum(k[j] * x[i - 5 + j] for j in range(11)), rel=1e-14)


def test_smooth_returns_short_input_as_it_is():
    x = [0.5] * 11
    assert plot.smooth(x) is x


@pytest.mark.parametrize("name", ENR + ("enr_50",))
def test_rank_order_is_pythons_stable_descending_sort(gold, name):
    scores = gold[f"{name}_scores"]
    assert (scores == 0).sum() > 2 and np.signbit(scores[scores == 0]).any() and (~np.signbit(scores[scores == 0])).any()
    want = sorted(range(len(scores)), key=lambda i: float(scores[i]), reverse=True)
    assert plot.rank_order(scores).tolist() == want


def test_rank_order_refuses_nan():
    with pytest.raises(ValueError, match="NaN"):
        plot.rank_order([1.0, float("nan"), 0.0])


@pytest.mark.parametrize("as_view", [False, True])
@pytest.mark.parametrize("name", DIST)
def test_site_distributions_with_numpy_counts_equal_the_reference(gold, host_device, name, as_view):
    regions, pwms, sites, ws = dist_inputs(gold, name, as_view)
    x, freq = plot.site_distributions(sites, regions, pwms, ws)
    assert np.array_equal(x, gold[f"{name}_x"])
    assert freq.shape == gold[f"{name}_freq"].shape
    assert np.array_equal(freq, gold[f"{name}_freq"])                # bit for bit: the same numpy calls on the same counts


@pytest.mark.parametrize("control", ["lists", "counts"])
@pytest.mark.parametrize("name", ENR)
def test_enrichment_profiles_with_numpy_stand_in_equal_the_reference(gold, host_device, name, control):
    regions, _, sites, ctl = enr_inputs(gold, name, control=control)
    raw = plot.enrichment_profiles(sites, ctl, regions, smoothed=False)
    assert np.array_equal(raw, gold[f"{name}_unsmoothed"])
    sm = plot.enrichment_profiles(sites, ctl, regions)
    assert np.array_equal(sm, gold[f"{name}_profile"])
    sub = plot.enrichment_profiles(sites, ctl, regions, motifs=[3, 1])
    assert np.array_equal(sub, gold[f"{name}_profile"][[3, 1]])


def test_ratio_control_falls_back_to_one_and_divides_like_python():
    r = plot.ratio_control([0, 1, 7], 3)
    assert r.tolist() == [1.0, 1 / 3, 7 / 3]
    with pytest.raises(ZeroDivisionError):
        plot.ratio_control([0], 0)


def test_enrichment_between_10_and_99_regions_divides_by_zero(gold, host_device):
    assert bool(gold["enr_50_zero_division"])
    regions, _, sites, ctl = enr_inputs(gold, "enr_50")
    with pytest.raises(ZeroDivisionError):
        plot.enrichment_profiles(sites, ctl, regions)


def test_enrichment_argument_validation(gold, host_device):
    regions, _, sites, ctl = enr_inputs(gold, "enr_100")
    with pytest.raises(ValueError, match="regions for sites"):
        plot.enrichment_profiles(sites, ctl, regions[:-1])
    bad = [SimpleNamespace(**{**vars(r), "score": None}) for r in regions]
    with pytest.raises(ValueError, match="no score"):
        plot.enrichment_profiles(sites, ctl, bad)
    nan = [SimpleNamespace(**{**vars(r), "score": float("nan") if i == 3 else r.score}) for i, r in enumerate(regions)]
    with pytest.raises(ValueError, match="NaN"):
        plot.enrichment_profiles(sites, ctl, nan)
    with pytest.raises(ValueError, match="control set"):
        plot.enrichment_profiles(sites, plot.RegionCounts([1, 2], 10), regions)
    with pytest.raises(IndexError):
        plot.enrichment_profiles(sites, ctl, regions, motifs=[4])
    few = [SimpleNamespace(score=1.0)] * 9
    with pytest.raises(ValueError, match="Too few"):
        plot.enrichment_profiles([[()] * 9], plot.RegionCounts([0], 9), few)


def test_distribution_argument_validation(gold, host_device):
    regions, pwms, sites, ws = dist_inputs(gold, "dist_w200")
    with pytest.raises(ValueError, match="one common length"):
        plot.site_distributions(sites, regions, pwms, 0)
    with pytest.raises(ValueError, match="PWMs for"):
        plot.site_distributions(sites, regions, pwms[:-1], ws)
    with pytest.raises(ValueError, match="regions for sites"):
        plot.site_distributions(sites, regions[:-1], pwms, ws)


def test_drop_in_dist_early_returns(gold, tmp_path, caplog):
    regions, pwms, sites, _ = dist_inputs(gold, "dist_w200")
    with caplog.at_level(logging.ERROR, logger="motifscan_amd.plot"):
        assert plot.plot_motif_sites_dist(str(tmp_path), [], pwms, sites, 0) is None
        assert plot.plot_motif_sites_dist(str(tmp_path), regions, pwms, sites, 0) is None
    assert [r.getMessage() for r in caplog.records] == ["No regions found for plotting",
                                                       "Unable to plot when the scanning length is different across regions"]
    assert not os.path.exists(tmp_path / "plots")


def test_drop_in_enrich_early_returns(gold, tmp_path, caplog):
    regions, pwms, sites, ctl = enr_inputs(gold, "enr_100")
    unscored = [SimpleNamespace(**{**vars(r), "score": None}) for r in regions]
    with caplog.at_level(logging.ERROR, logger="motifscan_amd.plot"):
        assert plot.plot_motif_sites_enrich(str(tmp_path), unscored, pwms, sites, ctl) is None
        assert plot.plot_motif_sites_enrich(str(tmp_path), regions[:9], pwms, [per[:9] for per in sites], ctl) is None
    assert [r.getMessage() for r in caplog.records] == ["Unable to plot when some regions have no scores set for sorting",
                                                       "Too few regions to plot: 9"]
    assert not os.path.exists(tmp_path / "plots")


def test_drop_ins_draw_the_reference_bars(gold, host_device, tmp_path, monkeypatch):
    import matplotlib.axes
    bars = []
    real = matplotlib.axes.Axes.bar

    def bar(self, x, height, *a, **k):
        bars.append((np.asarray(list(x)), np.asarray(height)))
        return real(self, x, height, *a, **k)

    monkeypatch.setattr(matplotlib.axes.Axes, "bar", bar)
    regions, pwms, sites, ws = dist_inputs(gold, "dist_w100")
    plot.plot_motif_sites_dist(str(tmp_path), regions, pwms, sites, ws)
    assert np.array_equal(np.stack([h for _, h in bars]), gold["dist_w100_freq"])
    assert [h.dtype.kind in "iu" for _, h in bars] == gold["dist_w100_int_rows"].tolist()
    names = sorted(os.listdir(tmp_path / "plots"))
    assert names == sorted(f"MA{i:04d}_1_motif_{i}_w{p.length}_sites_distributions.pdf" for i, p in enumerate(pwms))
    bars.clear()
    regions, pwms, sites, ctl = enr_inputs(gold, "enr_101")
    plot.plot_motif_sites_enrich(str(tmp_path), regions, pwms, sites, ctl)
    assert np.array_equal(np.stack([h for _, h in bars]), gold["enr_101_profile"])
    assert all(np.array_equal(x, np.arange(1, 102)) for x, _ in bars)
    assert len([n for n in os.listdir(tmp_path / "plots") if n.endswith("_sites_enrichment.pdf")]) == 4


# --------------------------------------------------------------- the restatement at sizes without a golden; the kernels' constants --

def literal_profile(flags, ratio_control):
    """plot.py:135-140 as ms_plotdata.hip's header describes it: per rank the slice sum of the ranked has-site flags over the
    2 * (R / 100) neighbouring ranks, over the slice's length, over ratio_control -- plain Python, one rank at a time."""
    R = len(flags)
    f = R // 100
    out = []
    for idx in range(R):
        head = max(0, idx - f)
        tail = min(idx + f, R)
        ratio_input = sum(flags[head:tail]) / (tail - head)
        out.append(ratio_input / ratio_control)
    return out


@pytest.mark.parametrize("size", ["128", "200", "tile-1", "tile+1", "tile+half"])
def test_profile_restatement_equals_the_literal_slice_sum(size):
    d = _lib.plot_dims()
    R = {"tile-1": d["prof_tile"] - 1, "tile+1": d["prof_tile"] + 1, "tile+half": d["prof_tile"] + d["half"]}.get(size) or int(size)
    rng = np.random.default_rng(R)
    k = np.arange(R)
    rows = [np.zeros(0, dtype=np.int64), np.concatenate([k, k[::9]]), np.array([0]), np.array([R - 1]), k[(k % 64 == 63) | (k % 64 == 0)],
            np.flatnonzero(rng.random(R) < 0.3)]
    ratio = np.array([1.0, 1 / 3, 7 / 13, 1e-300, 1.0, 1 / 3])
    for order in (np.arange(R), np.arange(R)[::-1].copy(), rng.permutation(R)):
        off = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
        region = np.concatenate([order[r] for r in rows])                       # row m has its sites at the ranks rows[m]
        raw = flat_profiles(off, region, order, ratio, np.arange(len(rows)), False)
        sm = flat_profiles(off, region, order, ratio, np.arange(len(rows)), True)
        for m, ranks in enumerate(rows):
            flags = np.zeros(R, dtype=bool)
            flags[ranks] = True
            want = literal_profile(flags.tolist(), float(ratio[m]))
            assert raw[m].tolist() == want, (size, m)
            assert np.array_equal(sm[m], plot.smooth(np.array(want))), (size, m)
        # a sub-set of rows indexes ratio by motif
        assert np.array_equal(flat_profiles(off, region, order, ratio, [5, 2], False), raw[[5, 2]])


def test_plot_dims_are_constants_of_the_build():
    L = _lib.lib()
    out = (ctypes.c_int32 * 6)()
    assert L.ms_debug_plot_dims(out) == _lib.MS_OK
    d = _lib.plot_dims()
    assert list(out) == [d[k] for k in ("hist_lds_bins", "hist_hits_per_block", "hist_max_blocks", "scan_threads", "prof_tile", "half")]
    assert all(v > 0 for v in out)
    assert 4 * d["hist_lds_bins"] <= 64 * 1024                                   # 32-bit counters in one block's static LDS
    assert d["scan_threads"] % 64 == 0 and d["scan_threads"] <= 1024              # whole waves, one block
    assert 2 * d["half"] + 1 == plot.SMOOTH_WINDOW == len(plot.smoothing_weights())
    assert d["prof_tile"] > 2 * d["half"]
    assert L.ms_debug_plot_dims(None) == _lib.MS_ERR_INVALID
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "motifscan_amd_debug.h")) as fh:
        assert re.search(r"\bint\s+ms_debug_plot_dims\s*\(\s*int32_t\s+out\s*\[\s*6\s*\]\s*\)", fh.read())


def test_bin_count_crosses_the_lds_limit_where_the_device_tests_assume():
    """include/motifscan_amd.h: n_bins = (2 * extend + 11 + 9) / 10 - 1.  It equals numpy's count around the limit, reaches
    hist_lds_bins at 5 extends, and is one more at the next: the two windows tests/test_gpu_plot_boundaries.py runs."""
    lds = _lib.plot_dims()["hist_lds_bins"]
    n_bins = {e: (2 * e + 11 + 9) // 10 - 1 for e in range(5 * lds - 12, 5 * lds + 12)}
    assert all(n == len(plot.bin_edges(e)) - 1 for e, n in n_bins.items())
    at_limit = [e for e, n in n_bins.items() if n == lds]
    assert at_limit == list(range(5 * lds - 5, 5 * lds)) and n_bins[5 * lds] == lds + 1
    for e in (0, 4, 5, 17, 250):
        assert (2 * e + 11 + 9) // 10 - 1 == len(plot.bin_edges(e)) - 1 <= lds
