"""
motifscan_amd.plot -- `motifscan.plot` (/root/reference/motifscan/plot.py:43-153, what `motifscan scan --plot-dist` draws) with the
numbers under the bars computed on the device.

The reference walks the nested site lists in Python: `plot_motif_sites_dist` makes one float per site and histograms them,
`plot_motif_sites_enrich` sums a slice of up to 2 * (R // 100) flags for every rank of every motif -- O(P x R^2 / 50) element visits,
far longer than the scan at the region counts this project is built for.  Here:

    site_distributions(motif_sites, regions, pwms, window_size) -> (x, freq [P, n_bins])
        the histogram counts come from ms_result_site_histogram (integer bins: exact); the `/ n` and smooth() of these small
        arrays run in numpy exactly as the reference runs them, so freq is the reference's array bit for bit.
    enrichment_profiles(motif_sites, motif_sites_control, regions, motifs=slice(None), smoothed=True) -> [len(motifs), R]
        the ranking is made here (a stable descending sort, plot.py:121-122), the fold changes and their smoothing on the device
        (ms_result_rank_profile), chunked by motif so that the output block stays bounded.
    plot_motif_sites_dist / plot_motif_sites_enrich
        the reference's two functions with the same signatures, early returns, log messages, file names and matplotlib calls:
        only the data come from the functions above.

`motif_sites` is what `Scanner.scan_motifs` returns (a `MotifSites`; while it still owns its device result that result is used as it
is, otherwise its flat arrays are uploaded) or the reference's nested lists (flattened and uploaded).  `motif_sites_control` may also
be a `RegionCounts` -- the per-motif region counts of a counts-only control scan (`Scanner.count_regions_with_sites`) with the number
of control regions.  There is no CPU path for the profile arithmetic: without a device these functions raise.
"""
import logging
import os
import re
from collections import namedtuple

import numpy as np

from . import _lib
from .sites import MotifSites

logger = logging.getLogger(__name__)

RegionCounts = namedtuple("RegionCounts", ["n_regions_with_site", "n_regions"])

SMOOTH_WINDOW = 11                   # plot.py:34: smooth(x, window_len=11)
PROFILE_BLOCK_BYTES = 256 << 20      # device output block per ms_result_rank_profile call (P x R doubles are 4.6 GB at 10^6 regions)
_UNSAFE_FILE_CHARS = re.compile(r"[-:./*]")     # motifscan.io.utils.replace_special_char: these become '_'


# ----------------------------------------------------------------------------------------------------- host-side pieces --

def bin_edges(extend):
    """plot.py:67: the histogram's bin edges, 10 bp apart, covering [-extend - 5, extend + 5]."""
    return np.arange(-extend - 5, extend + 6, 10)


def bin_centres(edges):
    """plot.py:71-73: x[i] = (edge[i] + edge[i + 1]) // 2."""
    return (edges[:-1] + edges[1:]) // 2


def smoothing_weights():
    """The 11 weights smooth() convolves with (w / w.sum(), w = np.hanning(11)), reversed as np.convolve applies them: the
    device computes out[i] = sum_j k[j] * x[i - 5 + j]."""
    w = np.hanning(SMOOTH_WINDOW)
    return np.ascontiguousarray((w / w.sum())[::-1])


def smooth(x):
    """plot.py:34-40 on the host, for the small histogram rows: x as it is when len(x) <= 11, else the convolution with the
    normalised Hanning window over x reflected by 10 at both ends, cut back to len(x)."""
    if len(x) <= SMOOTH_WINDOW:
        return x
    pad = SMOOTH_WINDOW - 1
    s = np.pad(np.asarray(x), pad, mode="reflect")
    w = np.hanning(SMOOTH_WINDOW)
    return np.convolve(w / w.sum(), s, mode="same")[pad:-pad]


def rank_order(scores):
    """plot.py:121-122: the regions by score, descending, ties in input order (Python's sort is stable also with reverse=True).
    NaN scores are refused: the reference's order is undefined for them."""
    s = np.asarray(scores, dtype=np.float64)
    if np.isnan(s).any():
        raise ValueError("region scores contain NaN: their rank order is undefined")
    return np.argsort(-s, kind="stable")


def region_scores(regions):
    scores = [r.score for r in regions]
    if any(s is None for s in scores):
        raise ValueError("some regions have no score set for sorting")
    return scores


def same_length(regions):
    """The common length of the regions, or None when they differ (plot.py:17-25)."""
    lengths = {r.end - r.start for r in regions}
    return lengths.pop() if len(lengths) == 1 else None


def control_counts(motif_sites_control):
    """(int64 [P] regions with >= 1 site, number of regions) of the control set, however it was scanned."""
    if isinstance(motif_sites_control, RegionCounts):
        return np.asarray(motif_sites_control.n_regions_with_site, dtype=np.int64), int(motif_sites_control.n_regions)
    if isinstance(motif_sites_control, MotifSites):
        return np.asarray(motif_sites_control.n_regions_with_site, dtype=np.int64), motif_sites_control.n_regions
    rows = list(motif_sites_control)
    n_regions = len(rows[0]) if rows else 0
    return np.array([sum(len(s) > 0 for s in per) for per in rows], dtype=np.int64), n_regions


def ratio_control(n_with_site, n_regions):
    """plot.py:127-132: n_control / n_regions_control per motif (int / int: one correctly rounded double), 0 replaced by 1."""
    if n_regions == 0:
        raise ZeroDivisionError("division by zero: the control set has no regions")
    r = np.asarray(n_with_site, dtype=np.int64) / np.int64(n_regions)
    r[r == 0] = 1.0
    return r


def _n_regions(motif_sites):
    if isinstance(motif_sites, MotifSites):
        return motif_sites.n_regions
    return len(motif_sites[0]) if len(motif_sites) else 0


# ---------------------------------------------------------------------------------------------------- device plumbing --

def _device_sites(motif_sites):
    """(ScanResult, seq_starts int64 [R], owned): the result the device reads.  A MotifSites that still owns its scan result hands
    that over (owned False: not ours to free); otherwise the flat arrays -- of the view or of the reference's nested lists, whose
    sites carry genome coordinates (then seq_starts = 0) -- are uploaded."""
    if isinstance(motif_sites, MotifSites):
        h = motif_sites._h
        if h.region is None:
            raise ValueError("the MotifSites has been closed")
        if isinstance(h.owner, _lib.ScanResult) and h.owner.h:
            return h.owner, h.seq_starts, False
        res = _lib.result_from_hits(motif_sites.n_pwms, motif_sites.n_regions, h.motif_offsets, h.region, h.pos, h.score, h.strand)
        return res, h.seq_starts, True
    rows = list(motif_sites)
    n_regions = len(rows[0]) if rows else 0
    region, start, score, strand, counts = [], [], [], [], []
    for per in rows:
        if len(per) != n_regions:
            raise ValueError("every motif needs one site list per region")
        k0 = len(region)
        for r, sites in enumerate(per):
            for s in sites:
                region.append(r)
                start.append(s.start)
                score.append(s.score)
                strand.append(1 if s.strand == "+" else 2)
        counts.append(len(region) - k0)
    offsets = np.concatenate([[0], np.cumsum(counts, dtype=np.int64)]).astype(np.int64)
    res = _lib.result_from_hits(len(rows), n_regions, offsets, np.array(region, dtype=np.int64), np.array(start, dtype=np.int64),
                                np.array(score, dtype=np.float64), np.array(strand, dtype=np.int8))
    return res, np.zeros(n_regions, dtype=np.int64), True


def _device_histogram(motif_sites, pwms, summits, extend):
    """counts int64 [P, n_bins], n_sites int64 [P] (ms_result_site_histogram)."""
    res, seq_starts, owned = _device_sites(motif_sites)
    pw = _lib.PwmSet.from_matrices([pwm.matrix for pwm in pwms])
    try:
        return res.site_histogram(pw, np.asarray(summits, dtype=np.int64) - seq_starts, extend)
    finally:
        pw.close()
        if owned:
            res.close()


def _device_profiles(motif_sites, order, ratio, rows, smoothed):
    """float64 [len(rows), R] (ms_result_rank_profile), one call per contiguous run of motifs, each cut to PROFILE_BLOCK_BYTES."""
    R = len(order)
    out = np.empty((len(rows), R), dtype=np.float64)
    if len(rows) == 0:
        return out
    res, _, owned = _device_sites(motif_sites)
    kernel = smoothing_weights()
    step = max(1, PROFILE_BLOCK_BYTES // (8 * max(R, 1)))
    try:
        i = 0
        while i < len(rows):
            j = i + 1
            while j < len(rows) and j - i < step and rows[j] == rows[j - 1] + 1:
                j += 1
            res.rank_profile(order, ratio[rows[i]:rows[j - 1] + 1], kernel, int(rows[i]), int(rows[j - 1]) + 1, smoothed, out=out[i:j])
            i = j
    finally:
        if owned:
            res.close()
    return out


# --------------------------------------------------------------------------------------------------------- the data --

def _distributions(motif_sites, regions, pwms, window_size):
    pwms = list(pwms)
    regions = list(regions)
    if len(pwms) != len(motif_sites):
        raise ValueError(f"{len(pwms)} PWMs for {len(motif_sites)} motifs of sites")
    if len(regions) != _n_regions(motif_sites):
        raise ValueError(f"{len(regions)} regions for sites of {_n_regions(motif_sites)} regions")
    if window_size <= 0:
        if not regions:
            raise ValueError("no regions: the window size cannot be taken from them")
        window_size = same_length(regions)
        if window_size is None:
            raise ValueError("window_size <= 0 needs regions of one common length")
    extend = window_size // 2
    edges = bin_edges(extend)
    counts, n_sites = _device_histogram(motif_sites, pwms, [r.summit for r in regions], extend)
    freq = np.zeros(counts.shape, dtype=np.float64)
    for m in range(len(pwms)):
        # plot.py:68-69: a motif with sites is normalised and smoothed; one without keeps its (zero) counts
        freq[m] = smooth(counts[m] / n_sites[m]) if n_sites[m] > 0 else counts[m]
    return bin_centres(edges), freq, n_sites


def site_distributions(motif_sites, regions, pwms, window_size):
    """(x int [n_bins], freq float64 [P, n_bins]): plot_motif_sites_dist's bars of every motif (plot.py:57-73).  window_size <= 0 takes
    the common length of the regions (ValueError when they differ, where the reference logs an error and draws nothing)."""
    x, freq, _ = _distributions(motif_sites, regions, pwms, window_size)
    return x, freq


def enrichment_profiles(motif_sites, motif_sites_control, regions, motifs=slice(None), smoothed=True):
    """float64 [len(motifs), R]: plot_motif_sites_enrich's bars (plot.py:119-142) for the motifs selected by `motifs` (a slice or a
    sequence of motif indices).  smoothed=False gives the fold changes before smooth().  Raises ValueError for regions without scores,
    NaN scores or fewer than 10 regions (where the reference logs an error and draws nothing) and ZeroDivisionError for 10 <= R < 100
    (where the reference divides by zero: its window 2 * (R // 100) is empty)."""
    regions = list(regions)
    R = len(regions)
    if R != _n_regions(motif_sites):
        raise ValueError(f"{R} regions for sites of {_n_regions(motif_sites)} regions")
    order = rank_order(region_scores(regions))
    if len(str(R)) < 2:
        raise ValueError(f"Too few regions to plot: {R}")
    n_with_site, n_control_regions = control_counts(motif_sites_control)
    P = len(motif_sites)
    if len(n_with_site) != P:
        raise ValueError(f"{len(n_with_site)} motifs in the control set, {P} in the input")
    rows = np.arange(P)[motifs] if isinstance(motifs, slice) else np.asarray(motifs, dtype=np.int64).reshape(-1)
    if len(rows) and (rows.min() < 0 or rows.max() >= P):
        raise IndexError("motif index out of range")
    if len(rows) == 0:
        return np.zeros((0, R), dtype=np.float64)
    if R // 100 == 0:
        raise ZeroDivisionError(f"division by zero: {R} regions give an empty window of 2 * ({R} // 100) ranks (plot.py:136-138)")
    ratio = ratio_control(n_with_site, n_control_regions)
    return _device_profiles(motif_sites, order, ratio, rows, smoothed)


# -------------------------------------------------------------------------------------------------------- the drop-ins --

def _pyplot():
    import matplotlib as mpl
    mpl.use("Agg")
    import matplotlib.pyplot as plt
    return plt


def _file_name(pwm):
    return _UNSAFE_FILE_CHARS.sub("_", pwm.matrix_id + "_" + pwm.name)


def plot_motif_sites_dist(output_dir, regions, pwms, motif_sites, window_size):
    """plot.py:43-92 with the bars from site_distributions."""
    if window_size <= 0:
        if len(regions) == 0:
            logger.error("No regions found for plotting")
            return
        if same_length(regions) is None:
            logger.error("Unable to plot when the scanning length is different across regions")
            return
    output_dir = os.path.join(output_dir, "plots")
    if not os.path.isdir(output_dir):
        os.makedirs(output_dir)
    if window_size <= 0:
        window_size = regions[0].end - regions[0].start
    extend = window_size // 2
    pwms = list(pwms)
    x, freq, n_sites = _distributions(motif_sites, regions, pwms, window_size)
    x = list(x)
    plt = _pyplot()
    for m, pwm in enumerate(pwms):
        logger.debug(f"Plotting for {pwm.matrix_id + ',' + pwm.name}")
        heights = freq[m] if n_sites[m] > 0 else freq[m].astype(np.int64)
        fig = plt.figure(figsize=(4, 3.5))
        ax = fig.gca()
        ax.bar(x, heights, width=10, color="#4169E1", label=pwm.matrix_id + "," + pwm.name)
        ax.legend(loc="upper right", fontsize=8, frameon=False)
        ax.set_xlabel("Distance to Center/Summit", fontsize=8)
        ax.set_ylabel("Fraction", fontsize=8)
        ax.set_xlim(-extend - 5, extend + 5)
        if n_sites[m] > 0:
            ax.set_ylim(0, 1.2 * max(heights))
        else:
            ax.set_ylim(0, 0.1)
        ax.tick_params(axis="both", which="major", labelsize=8)
        fig.subplots_adjust(left=0.15, right=0.98, bottom=0.15, top=0.95)
        fig.savefig(os.path.join(output_dir, f"{_file_name(pwm)}_sites_distributions.pdf"))
        plt.close()


def plot_motif_sites_enrich(output_dir, regions, pwms, motif_sites, motif_sites_control):
    """plot.py:95-153 with the bars from enrichment_profiles."""
    if any(r.score is None for r in regions):
        logger.error("Unable to plot when some regions have no scores set for sorting")
        return
    n_regions_input = len(regions)
    if len(str(n_regions_input)) < 2:
        logger.error(f"Too few regions to plot: {n_regions_input}")
        return
    output_dir = os.path.join(output_dir, "plots")
    if not os.path.isdir(output_dir):
        os.makedirs(output_dir)
    pwms = list(pwms)
    n = min(len(pwms), len(motif_sites), len(control_counts(motif_sites_control)[0]))     # the reference zips the three
    profiles = enrichment_profiles(motif_sites, motif_sites_control, regions, motifs=slice(0, n))
    plt = _pyplot()
    for m, pwm in enumerate(pwms[:n]):
        logger.debug(f"Plotting for {pwm.matrix_id + ',' + pwm.name}")
        fold_changes = profiles[m]
        fig = plt.figure(figsize=(4, 3.5))
        ax = fig.gca()
        ax.bar(range(1, n_regions_input + 1), fold_changes, width=1, color="#4169E1", label=pwm.matrix_id + "," + pwm.name)
        ax.legend(loc="upper right", fontsize=8, frameon=False)
        ax.set_xlabel("Regions Ranked by Score (Descending)", fontsize=8)
        ax.set_ylabel("Fold Change", fontsize=8)
        ax.set_xlim(0, n_regions_input)
        y_max = max(fold_changes)
        if y_max > 0:
            ax.set_ylim(0, 1.2 * y_max)
        else:
            ax.set_ylim(0, 0.1)
        ax.tick_params(axis="both", which="major", labelsize=8)
        fig.subplots_adjust(left=0.15, right=0.98, bottom=0.15, top=0.95)
        fig.savefig(os.path.join(output_dir, f"{_file_name(pwm)}_sites_enrichment.pdf"))
        plt.close()
