#!/usr/bin/env python3
"""
tools/plotdata_time.py -- time the data behind `motifscan scan --plot-dist` (motifscan_amd.plot) at BASELINE configs[2] in full, next to
the reference's own loops (motifscan/plot.py:43-153) timed on the CPU at a reduced size and extrapolated.  Prints one JSON line.

  --part gpu    configs[2]: 100 000 regions x 1 kb, the 579-PWM set at p = 1e-4, scanned + de-duplicated on the device, with a
                100 000-region control set scanned counts-only.  For site_distributions and enrichment_profiles: the wall time of
                the call as a user makes it (output in host memory, D2H included), the median of --repeats after one warm-up, and
                for the profiles also the call with the output left in HBM (a torch buffer: no D2H).
  --part cpu    the reference's plot_motif_sites_dist / plot_motif_sites_enrich on the CPU, at --ref-motifs motifs and --ref-regions
                regions, with matplotlib's Axes.bar and Figure.savefig patched out (what is left is the data loops plus an empty
                figure per motif), extrapolated to 579 motifs x 100 000 regions: by R for the distances; for the enrichment a R + b R^2 is
                fitted through two sizes (R and 2R) and evaluated at 100 000.  Needs the reference on this host (tests/golden/make_golden.py's import), never the GPU.
  --merge A B   one JSON line of the two parts' outputs.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

P_FULL, R_FULL, L_FULL = 579, 100_000, 1000


def part_gpu(repeats):
    from motifscan_amd import _lib, plot, synth
    from motifscan_amd.sites import MotifSites
    _lib.set_device(0)
    vals, widths, cutoffs = synth.load_motif_set(P_FULL)
    bases, offsets = synth.make_regions(R_FULL, L_FULL, seed=2)
    cbases, coffsets = synth.make_regions(R_FULL, L_FULL, seed=3)
    pw, sq, sqc = _lib.PwmSet(vals, widths, cutoffs), _lib.SeqSet(bases, offsets), _lib.SeqSet(cbases, coffsets)
    res = _lib.scan(pw, sq, 3).dedup(pw)
    h = res.hits(copy=False, motif=False)
    starts = np.arange(R_FULL, dtype=np.int64) * L_FULL
    sites = MotifSites(h["motif_offsets"], h["seq_idx"], h["pos"], h["score"], h["strand"], starts, owner=res)
    ctl_res = _lib.scan(pw, sqc, 3, _lib.MS_SCAN_COUNTS_ONLY)
    ctl = plot.RegionCounts(ctl_res.region_counts(), R_FULL)
    ctl_res.close()
    rng = np.random.default_rng(5)
    summits = starts + rng.integers(250, 750, size=R_FULL)
    scores = np.round(rng.normal(100, 30, size=R_FULL), 1)
    regions = [SimpleNamespace(chrom="chr1", start=int(s), end=int(s) + L_FULL, summit=int(u), score=float(v))
               for s, u, v in zip(starts, summits, scores)]
    pwms = [SimpleNamespace(matrix=vals[o:o + 4 * w].reshape(4, w), length=int(w))
            for o, w in zip(np.concatenate([[0], np.cumsum(4 * widths)[:-1]]), widths)]

    def timed(fn):
        fn()
        t = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            fn()
            t.append(time.perf_counter() - t0)
        return statistics.median(t)

    t_dist = timed(lambda: plot.site_distributions(sites, regions, pwms, 0))
    t_enr = timed(lambda: plot.enrichment_profiles(sites, ctl, regions))
    import torch
    order = plot.rank_order(scores)
    ratio = plot.ratio_control(ctl.n_regions_with_site, ctl.n_regions)
    k = plot.smoothing_weights()
    dev = torch.empty((P_FULL, R_FULL), dtype=torch.float64, device="cuda")

    def resident():
        res.rank_profile(order, ratio, k, 0, P_FULL, out=int(dev.data_ptr()))
    t_res = timed(resident)
    out = {"part": "gpu", "device": _lib.device_name(), "config": "configs[2]: 100000 regions x 1000 bp, 579 PWMs p=1e-4, 100000 control regions",
           "n_sites_input": int(sites.n_sites), "repeats": repeats,
           "site_distributions_wall_s": t_dist, "enrichment_profiles_wall_s": t_enr,
           "enrichment_profiles_resident_s": t_res,
           "profile_bytes_written": 8 * P_FULL * R_FULL,
           "both_wall_s": t_dist + t_enr}
    sites.close()
    pw.close()
    sq.close()
    sqc.close()
    return out


def part_cpu(n_motifs, n_regions):
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    from make_golden import import_reference
    from make_golden_plot import Pwm, SiteList
    REF = import_reference()
    import matplotlib.axes
    import matplotlib.figure
    import motifscan.plot as rplot
    from unittest import mock
    MotifSite, GR = REF["scanner"].MotifSite, REF["GenomicRegion"]
    rng = np.random.default_rng(9)
    starts = np.arange(2 * n_regions) * L_FULL
    summits = starts + rng.integers(250, 750, size=2 * n_regions)
    regions = [GR("chr1", int(s), int(s) + L_FULL, summit=int(u), score=float(v))
               for s, u, v in zip(starts, summits, np.round(rng.normal(100, 30, size=2 * n_regions), 1))]
    pwms = [Pwm(i, 12) for i in range(n_motifs)]

    def sites_for(R):
        per = []
        for _ in range(n_motifs):
            k = rng.poisson(0.3, size=R)                  # sites per region
            per.append([SiteList(MotifSite(int(starts[r]) + int(rng.integers(0, 990)), 10.0, "+") for _ in range(k[r])) for r in range(R)])
        return per

    sites = sites_for(2 * n_regions)
    control = sites_for(2 * n_regions)
    t_enr = {}
    with mock.patch.object(matplotlib.axes.Axes, "bar", lambda *a, **k: None), \
            mock.patch.object(matplotlib.figure.Figure, "savefig", lambda *a, **k: None):
        out_dir = tempfile.mkdtemp()
        t0 = time.perf_counter()
        rplot.plot_motif_sites_dist(out_dir, regions[:n_regions], pwms, [per[:n_regions] for per in sites], 0)
        t_dist = time.perf_counter() - t0
        for R in (n_regions, 2 * n_regions):
            t0 = time.perf_counter()
            rplot.plot_motif_sites_enrich(out_dir, regions[:R], pwms, [per[:R] for per in sites], control)
            t_enr[R] = time.perf_counter() - t0
    # t(R) = a R + b R^2 through the two enrichment points: the quadratic term is the slice sums, the linear one everything else
    r1, r2 = n_regions, 2 * n_regions
    b = (t_enr[r2] / r2 - t_enr[r1] / r1) / (r2 - r1)
    a = t_enr[r1] / r1 - b * r1
    scale_m = P_FULL / n_motifs
    return {"part": "cpu", "cpu": os.uname().machine, "cpu_count": os.cpu_count(), "ref_motifs": n_motifs, "ref_regions": [r1, r2],
            "ref_sites_per_region_mean": 0.3, "patched_out": ["Axes.bar", "Figure.savefig"],
            "ref_dist_s": t_dist, "ref_enrich_s": [t_enr[r1], t_enr[r2]],
            "ref_dist_extrapolated_s": t_dist * scale_m * R_FULL / r1,
            "ref_enrich_extrapolated_s": scale_m * (a * R_FULL + b * R_FULL ** 2),
            "extrapolation": f"x {P_FULL}/{n_motifs} motifs; distances x R from {r1}; enrichment a R + b R^2 fitted at R = {r1}, {r2}, "
                             f"evaluated at R = {R_FULL}"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["gpu", "cpu"])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--ref-motifs", type=int, default=4)
    ap.add_argument("--ref-regions", type=int, default=10_000)
    ap.add_argument("--merge", nargs=2)
    a = ap.parse_args()
    if a.merge:
        parts = {}
        for p in a.merge:
            with open(p) as fh:
                d = json.loads(fh.read().strip().splitlines()[-1])
            parts[d.pop("part")] = d
        g, c = parts["gpu"], parts["cpu"]
        out = {"gpu": g, "reference_cpu": c,
               "speedup_dist": c["ref_dist_extrapolated_s"] / g["site_distributions_wall_s"],
               "speedup_enrich": c["ref_enrich_extrapolated_s"] / g["enrichment_profiles_wall_s"]}
    elif a.part == "gpu":
        out = part_gpu(a.repeats)
    elif a.part == "cpu":
        out = part_cpu(a.ref_motifs, a.ref_regions)
    else:
        ap.error("--part or --merge")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
