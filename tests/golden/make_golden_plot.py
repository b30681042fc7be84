#!/usr/bin/env python3
"""
tests/golden/make_golden_plot.py -- golden vectors of the reference's `motifscan.plot` (plot_motif_sites_dist and
plot_motif_sites_enrich, what `motifscan scan --plot-dist` draws), made by running the REAL reference on the CPU with the stubs of
make_golden.py (imported from it, not edited).  Nothing here runs on the GPU box and nothing here is product code.

What is captured: matplotlib's Axes.bar is patched to record (x, heights) of every bar chart the reference draws -- the numbers
motifscan_amd.plot computes on the device -- and the reference's smooth() is wrapped to record the fold changes it is handed by
plot_motif_sites_enrich (the profile before smoothing).  The PDFs go to a temporary directory.

One adaptation: plot.py:133 calls np.asarray on a motif's per-region site lists, which numpy >= 1.24 refuses for ragged lists
("inhomogeneous shape").  The site lists are therefore handed to the reference in `SiteList`, a container numpy treats as one
object; it offers exactly what plot.py reads of a region's sites (len, iteration).

Cases (inputs and outputs in ref_plot.npz, keys prefixed by the case name):
  dist_w200    window_size > 0, regions of different lengths, summits off centre, odd and even widths (half-integer distances),
               distances on a bin edge, on the last edge and outside the range, a motif without sites; 21 bins (smoothed)
  dist_w0      window_size == 0 over regions of one length (1000 bp: 101 bins)
  dist_w100    11 bins: smooth() returns its input
  dist_w35     4 bins whose last edge (18) lies inside extend + 5
  enr_100 / enr_101 / enr_2003   R = 100, 101 and 2003 regions with tied scores (-0.0 and 0.0 among them); a motif whose control set
               has no site (ratio_control falls back to 1), a motif without input sites
  enr_50       10 <= R < 100: the reference raises ZeroDivisionError

Usage:  python3 tests/golden/make_golden_plot.py
"""
import os
import sys
import tempfile
from unittest import mock

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import import_reference  # noqa: E402


class SiteList:
    """A region's sites as plot.py reads them (len, iteration), opaque to np.asarray."""
    __slots__ = ("_s",)

    def __init__(self, sites):
        self._s = list(sites)

    def __len__(self):
        return len(self._s)

    def __iter__(self):
        return iter(self._s)


class Pwm:
    """What plot.py reads of a PWM: matrix_id, name, length."""

    def __init__(self, i, width):
        self.matrix_id, self.name, self.length = f"MA{i:04d}.1", f"motif-{i}/w{width}", int(width)


def nested(P, R, motif_offsets, region, start, score, strand, MotifSite):
    out = [[[] for _ in range(R)] for _ in range(P)]
    for m in range(P):
        for k in range(motif_offsets[m], motif_offsets[m + 1]):
            out[m][region[k]].append(MotifSite(int(start[k]), float(score[k]), "+" if strand[k] == 1 else "-"))
    return [[SiteList(s) for s in per] for per in out]


def flat(per_motif):
    """[(region, start)] per motif -> flat arrays ordered by (motif, region, start, strand)."""
    rng = np.random.default_rng(len(per_motif))
    off, region, start, score, strand = [0], [], [], [], []
    for sites in per_motif:
        for r, s in sorted(sites):
            region.append(r)
            start.append(s)
            score.append(float(np.round(rng.uniform(5, 15), 6)))
            strand.append(int(rng.integers(1, 3)))
        off.append(len(region))
    return (np.array(off, dtype=np.int64), np.array(region, dtype=np.int64), np.array(start, dtype=np.int64),
            np.array(score, dtype=np.float64), np.array(strand, dtype=np.int8))


def dist_case(rng, name, window_size, starts, ends, summits, widths, n_random):
    R = len(starts)
    ext = (window_size if window_size > 0 else int(ends[0] - starts[0])) // 2
    edges = np.arange(-ext - 5, ext + 6, 10)
    per_motif = []
    for m, W in enumerate(widths):
        sites = []
        if m == len(widths) - 1:                       # the last motif has no site at all
            per_motif.append(sites)
            continue
        for _ in range(n_random):
            r = int(rng.integers(R))
            d2 = int(rng.integers(2 * (-ext - 30), 2 * (ext + 30)))       # 2 * distance, parity fixed by W below
            d2 += (d2 - W) % 2
            sites.append((r, int(summits[r]) + (d2 - W) // 2))
        for e in (edges[0], edges[1], edges[len(edges) // 2], edges[-1], edges[-1] + 1, edges[0] - 1):
            r = int(rng.integers(R))
            d2 = 2 * int(e) + (W % 2)                  # on the edge (even W) or half a base past it (odd W)
            sites.append((r, int(summits[r]) + (d2 - W) // 2))
            if W % 2:
                sites.append((r, int(summits[r]) + (2 * int(e) - 1 - W) // 2))   # half a base before it
        per_motif.append(sites)
    return {"window_size": np.int64(window_size), "starts": starts, "ends": ends, "summits": summits,
            "widths": np.asarray(widths, dtype=np.int32)}, flat(per_motif)


def main():
    REF = import_reference()
    import matplotlib.axes
    import motifscan.plot as rplot
    MotifSite = REF["scanner"].MotifSite
    GR = REF["GenomicRegion"]
    rng = np.random.default_rng(20261015)
    save = {}
    bars = []
    smooth_in = []
    real_bar, real_smooth = matplotlib.axes.Axes.bar, rplot.smooth

    def bar(self, x, height, *a, **k):
        bars.append((np.asarray(list(x)), np.asarray(height)))
        return real_bar(self, x, height, *a, **k)

    def smooth(x, window_len=11):
        smooth_in.append(np.asarray(x, dtype=np.float64).copy())
        return real_smooth(x, window_len)

    tmp = tempfile.mkdtemp()
    with mock.patch.object(matplotlib.axes.Axes, "bar", bar), mock.patch.object(rplot, "smooth", smooth):
        # ---- site distributions
        for name, ws, R, lens, widths, n_random in (("dist_w200", 200, 40, None, [7, 8, 12, 13, 5, 21, 10], 400),
                                                    ("dist_w0", 0, 30, 1000, [6, 11, 15, 9], 600),
                                                    ("dist_w100", 100, 25, None, [8, 9, 4], 150),
                                                    ("dist_w35", 35, 20, None, [7, 10, 6], 80)):
            starts = rng.integers(1_000, 1_000_000, size=R).astype(np.int64)
            L = np.full(R, lens, dtype=np.int64) if lens else rng.integers(150, 700, size=R).astype(np.int64)
            ends = starts + L
            summits = starts + (L // 2 + rng.integers(-L // 4, L // 4 + 1)).astype(np.int64)        # off centre
            inp, (off, region, start, score, strand) = dist_case(rng, name, ws, starts, ends, summits, widths, n_random)
            P = len(widths)
            regions = [GR("chr1", int(s), int(e), summit=int(u), score=1.0) for s, e, u in zip(starts, ends, summits)]
            pwms = [Pwm(i, w) for i, w in enumerate(widths)]
            bars.clear()
            smooth_in.clear()
            rplot.plot_motif_sites_dist(tmp, regions, pwms, nested(P, R, off, region, start, score, strand, MotifSite), ws)
            assert len(bars) == P
            for k, v in inp.items():
                save[f"{name}_{k}"] = v
            save[f"{name}_motif_offsets"], save[f"{name}_region"], save[f"{name}_start"] = off, region, start
            save[f"{name}_score"], save[f"{name}_strand"] = score, strand
            save[f"{name}_x"] = bars[0][0].astype(np.int64)
            save[f"{name}_freq"] = np.stack([h.astype(np.float64) for _, h in bars])
            save[f"{name}_int_rows"] = np.array([h.dtype.kind in "iu" for _, h in bars])
            print(f"{name}: {P} motifs, {len(region)} sites, {len(bars[0][0])} bins")

        # ---- ranked enrichment
        for name, R, Rc in (("enr_100", 100, 300), ("enr_101", 101, 250), ("enr_2003", 2003, 4000), ("enr_50", 50, 120)):
            scores = np.round(rng.normal(0.0, 1.0, size=R), 1)                  # one decimal: many ties
            scores[rng.choice(R, size=max(2, R // 20), replace=False)] = -0.0
            scores[rng.choice(R, size=max(2, R // 20), replace=False)] = 0.0
            regions = [GR("chr1", 1000 * i, 1000 * i + 500, score=float(s)) for i, s in enumerate(scores)]
            P = 4
            rank = np.argsort(-scores, kind="stable")
            per_in, per_ctl = [], []
            for m in range(P):
                if m == 2:
                    per_in.append([])                      # no input site
                else:
                    p = np.linspace(0.7, 0.1, R) if m != 1 else np.full(R, 0.3)
                    hit = rng.random(R) < p
                    per_in.append([(int(rank[i]), int(rng.integers(0, 480))) for i in np.flatnonzero(hit)
                                   for _ in range(int(rng.integers(1, 3)))])
                if m == 3:
                    per_ctl.append([])                     # ratio_control 0 -> 1
                else:
                    per_ctl.append([(int(r), int(rng.integers(0, 480))) for r in np.flatnonzero(rng.random(Rc) < 0.25)])
            fin, fct = flat(per_in), flat(per_ctl)
            pwms = [Pwm(i, 10) for i in range(P)]
            bars.clear()
            smooth_in.clear()
            raised = False
            try:
                rplot.plot_motif_sites_enrich(tmp, regions, pwms, nested(P, R, *fin, MotifSite), nested(P, Rc, *fct, MotifSite))
            except ZeroDivisionError:
                raised = True
            save[f"{name}_scores"] = scores
            for tag, arrs in (("in", fin), ("ctl", fct)):
                for k, v in zip(("motif_offsets", "region", "start", "score", "strand"), arrs):
                    save[f"{name}_{tag}_{k}"] = v
            save[f"{name}_n_control_regions"] = np.int64(Rc)
            save[f"{name}_zero_division"] = np.bool_(raised)
            if not raised:
                assert len(bars) == P and len(smooth_in) == P
                save[f"{name}_profile"] = np.stack([h.astype(np.float64) for _, h in bars])
                save[f"{name}_unsmoothed"] = np.stack(smooth_in)
            print(f"{name}: R={R}, control {Rc}, {'ZeroDivisionError' if raised else 'profiles captured'}")
    out = os.path.join(HERE, "ref_plot.npz")
    np.savez_compressed(out, **save)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
