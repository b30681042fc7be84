"""
The plot data of `motifscan scan --plot-dist` on the device (ms_result_site_histogram, ms_result_rank_profile; motifscan_amd.plot):
against the reference's own bars (tests/golden/ref_plot.npz) and, at BASELINE configs[1] size, against the numpy restatement of the
contract in tests/test_plot_host.py over the pinned oracle's hits.  Run with -m gpu.

Exact: histogram counts, freq (numpy normalises and smooths the device's counts), the unsmoothed profiles (two IEEE divisions).
Within rtol 1e-13 + atol 1e-13 * max|y| per motif: the smoothed profiles -- numpy sums its 11 products in the order of the BLAS it was
built with, the device in index order.
"""
import os
from types import SimpleNamespace

import numpy as np
import pytest

from motifscan_amd import _lib, plot, synth
from motifscan_amd.scanner import Scanner
from test_plot_host import DIST, ENR, dist_inputs, enr_inputs, np_histogram, np_profiles

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_plot.npz")


@pytest.fixture(scope="module", autouse=True)
def device():
    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests need an MI355X (there is no CPU fallback)")
    _lib.set_device(0)


@pytest.fixture(scope="module")
def gold():
    d = np.load(GOLDEN)
    return {k: d[k] for k in d.files}


def assert_smoothed_close(got, want):
    assert got.shape == want.shape
    for g, w in zip(got, want):
        np.testing.assert_allclose(g, w, rtol=1e-13, atol=1e-13 * max(np.abs(w).max(), 0.0))


@pytest.mark.parametrize("as_view", [False, True])
@pytest.mark.parametrize("name", DIST)
def test_golden_site_distributions(gold, name, as_view):
    regions, pwms, sites, ws = dist_inputs(gold, name, as_view)
    extend = (ws if ws > 0 else regions[0].end - regions[0].start) // 2
    counts, n_sites = plot._device_histogram(sites, pwms, [r.summit for r in regions], extend)
    want_counts, want_n = np_histogram(sites, pwms, [r.summit for r in regions], extend)
    assert np.array_equal(counts, want_counts) and np.array_equal(n_sites, want_n)
    x, freq = plot.site_distributions(sites, regions, pwms, ws)
    assert np.array_equal(x, gold[f"{name}_x"])
    assert np.array_equal(freq, gold[f"{name}_freq"])


@pytest.mark.parametrize("as_view,control", [(False, "lists"), (True, "counts")])
@pytest.mark.parametrize("name", ENR)
def test_golden_enrichment_profiles(gold, name, as_view, control):
    regions, _, sites, ctl = enr_inputs(gold, name, as_view, control)
    raw = plot.enrichment_profiles(sites, ctl, regions, smoothed=False)
    assert np.array_equal(raw, gold[f"{name}_unsmoothed"])
    assert_smoothed_close(plot.enrichment_profiles(sites, ctl, regions), gold[f"{name}_profile"])


def test_golden_enrichment_between_10_and_99_regions_divides_by_zero(gold):
    regions, _, sites, ctl = enr_inputs(gold, "enr_50")
    with pytest.raises(ZeroDivisionError):
        plot.enrichment_profiles(sites, ctl, regions)
    res = _lib.result_from_hits(4, 50, gold["enr_50_in_motif_offsets"], gold["enr_50_in_region"], gold["enr_50_in_start"],
                                gold["enr_50_in_score"], gold["enr_50_in_strand"])
    try:
        with pytest.raises(ValueError, match="divides by zero"):               # the C-ABI refuses it too
            res.rank_profile(np.arange(50), np.ones(4), plot.smoothing_weights())
    finally:
        res.close()


def test_drop_ins_write_pdfs_with_the_reference_bars(gold, tmp_path, monkeypatch):
    import matplotlib.axes
    bars = []
    real = matplotlib.axes.Axes.bar

    def bar(self, x, height, *a, **k):
        bars.append((np.asarray(list(x)), np.asarray(height)))
        return real(self, x, height, *a, **k)

    monkeypatch.setattr(matplotlib.axes.Axes, "bar", bar)
    regions, pwms, sites, ws = dist_inputs(gold, "dist_w0", as_view=True)
    plot.plot_motif_sites_dist(str(tmp_path), regions, pwms, sites, ws)
    assert np.array_equal(np.stack([h for _, h in bars]), gold["dist_w0_freq"])
    assert all(np.array_equal(x, gold["dist_w0_x"]) for x, _ in bars)
    bars.clear()
    regions, pwms, sites, ctl = enr_inputs(gold, "enr_2003")
    plot.plot_motif_sites_enrich(str(tmp_path), regions, pwms, sites, ctl)
    assert_smoothed_close(np.stack([h for _, h in bars]), gold["enr_2003_profile"])
    pdfs = sorted(os.listdir(tmp_path / "plots"))
    assert len(pdfs) == 8 and all(os.path.getsize(tmp_path / "plots" / p) > 0 for p in pdfs)


class ChromGenome:
    """One synthetic chromosome, with what Scanner reads of a genome (scanner.py:81-87)."""

    def __init__(self, seq):
        self.seq = seq
        self.chrom_sizes = {"chr1": len(seq)}

    def fetch_sequence(self, chrom, start, end):
        return self.seq[start:end]


def test_configs1_scanner_result_against_the_restatement_and_the_oracle(oracle):
    """BASELINE configs[1]: 10k x 500 bp, the 50-PWM set; seeded summits and scores.  The MotifSites of Scanner.scan_motifs owns its
    device result, which the plot data read in place; its hits are the pinned oracle's."""
    R, L = 10_000, 500
    vals, widths, cutoffs = synth.load_motif_set(50)
    bases, offsets = synth.make_regions(2 * R, L, seed=11, frac_n=0.01)
    genome = ChromGenome(bases.tobytes().decode())
    rng = np.random.default_rng(7)
    summits = rng.integers(100, 400, size=2 * R)
    scores = np.round(rng.normal(50, 20, size=R), 0)                     # integral: ties
    regions = [SimpleNamespace(chrom="chr1", start=i * L, end=(i + 1) * L, summit=i * L + int(summits[i]), score=float(scores[i]))
               for i in range(R)]
    control = [SimpleNamespace(chrom="chr1", start=i * L, end=(i + 1) * L, summit=i * L + 250, score=None) for i in range(R, 2 * R)]
    mats, o = [], 0
    for w in widths:
        mats.append(vals[o:o + 4 * w].reshape(4, w))
        o += 4 * w
    pwms = [SimpleNamespace(matrix=m, length=m.shape[1], cutoffs={"1e-4": c}, matrix_id=f"M{i}", name=f"m{i}")
            for i, (m, c) in enumerate(zip(mats, cutoffs))]
    sc = Scanner(genome, regions, window_size=0, p_value="1e-4", remove_dup=False)
    sites = sc.scan_motifs(pwms)
    want = oracle.scan_arrays(vals, widths, cutoffs, bases[:R * L].tobytes(), offsets[:R + 1], 3, 8)
    a = sites.arrays()
    assert np.array_equal(a["motif_offsets"], want["motif_offsets"]) and np.array_equal(a["region"], want["seq_idx"])
    assert np.array_equal(a["start"] - np.arange(R)[a["region"]] * L, want["pos"])
    res = sites._h.owner
    assert isinstance(res, _lib.ScanResult) and res.h                       # read in place, not uploaded
    n_ctl = Scanner(genome, control, window_size=0, p_value="1e-4").count_regions_with_sites(pwms)
    ctl = plot.RegionCounts(n_ctl, R)

    # site distributions: window 500 -> 51 bins
    counts, n_sites = plot._device_histogram(sites, pwms, [r.summit for r in regions], 250)
    want_counts, want_n = np_histogram(sites, pwms, [r.summit for r in regions], 250)
    assert np.array_equal(counts, want_counts) and np.array_equal(n_sites, want_n) and counts.sum() > 0
    # chunks of motifs give the same rows as one call
    pw = _lib.PwmSet(vals, widths, cutoffs)
    try:
        rel = np.array([r.summit - r.start for r in regions], dtype=np.int64)
        parts = [res.site_histogram(pw, rel, 250, m0, m1)[0] for m0, m1 in ((0, 17), (17, 18), (18, 50))]
        assert np.array_equal(np.concatenate(parts), counts)
    finally:
        pw.close()

    # ranked enrichment
    order = plot.rank_order(scores)
    ratio = plot.ratio_control(n_ctl, R)
    rows = np.arange(50)
    raw = plot.enrichment_profiles(sites, ctl, regions, smoothed=False)
    assert np.array_equal(raw, np_profiles(sites, order, ratio, rows, False))
    sm = plot.enrichment_profiles(sites, ctl, regions)
    assert_smoothed_close(sm, np_profiles(sites, order, ratio, rows, True))
    k = plot.smoothing_weights()
    chunked = np.concatenate([res.rank_profile(order, ratio[m0:m1], k, m0, m1) for m0, m1 in ((0, 1), (1, 33), (33, 50))])
    assert np.array_equal(chunked, sm)
    sub = plot.enrichment_profiles(sites, ctl, regions, motifs=slice(5, 40, 7))
    assert np.array_equal(sub, sm[5:40:7])

    # a device buffer as the output (torch owns it)
    import torch
    dev = torch.empty((10, R), dtype=torch.float64, device="cuda")
    res.rank_profile(order, ratio[20:30], k, 20, 30, out=int(dev.data_ptr()))
    torch.cuda.synchronize()
    assert np.array_equal(dev.cpu().numpy(), sm[20:30])
    sites.close()
    sc.close()


def test_counts_only_result_is_refused():
    vals, widths, cutoffs = synth.load_motif_set(8)
    bases, offsets = synth.make_regions(200, 300, seed=3)
    pw, sq = _lib.PwmSet(vals, widths, cutoffs), _lib.SeqSet(bases, offsets)
    res = _lib.scan(pw, sq, 3, _lib.MS_SCAN_COUNTS_ONLY)
    try:
        with pytest.raises(ValueError, match="counts-only"):
            res.site_histogram(pw, np.full(200, 150), 150)
        with pytest.raises(ValueError, match="counts-only"):
            res.rank_profile(np.arange(200), np.ones(8), plot.smoothing_weights())
    finally:
        res.close()
        pw.close()
        sq.close()
