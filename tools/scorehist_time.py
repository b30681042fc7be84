#!/usr/bin/env python3
"""
tools/scorehist_time.py -- device time of ms_scan_score_histogram ("Score histogram") beside ms_scan_best on the
same inputs: the same dense fp64 walk over every window, once with the counting and once with the best-of-wave reduction.

    python tools/scorehist_time.py [--regions 100000] [--length 500] [--motifs 579] [--bins 1024] [--warmup 2] [--repeats 7]

One process, one device.  Three quantities, each --warmup calls and then --repeats measured ones, the calls of the three taking turns
(so that a drift of the device's clock hits all alike); the time is the library's own event time (`device_ms`: first launch -> last
kernel done), reported as median, minimum and maximum:
    tail   the histogram with lo = 0.7, hi = the default (a score of 1.0 in the last bin), per position
    full   the same with lo = each motif's least possible score (scoredist.least_score): every window pays the divide
    best   ms_scan_best (ms_best_device_ms)
and the row sums of both histograms are checked against the number of windows.  Prints one JSON line.  Needs an MI355X.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from motifscan_amd import _lib, scoredist, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=100000)
    ap.add_argument("--length", type=int, default=500)
    ap.add_argument("--motifs", type=int, default=579)
    ap.add_argument("--bins", type=int, default=1024)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()
    if _lib.device_count() < 1:
        raise SystemExit("scorehist_time needs an MI355X: no HIP device visible and there is no CPU fallback")
    _lib.set_device(0)
    vals, widths, _ = synth.load_motif_set(a.motifs)
    mats = synth.matrices_of(vals, widths)
    bases, offsets = synth.make_regions(a.regions, a.length, seed=1)
    pw, sq = _lib.PwmSet(vals, widths, None), _lib.SeqSet(bases, offsets)
    hi = scoredist.default_hi(0.7, a.bins)
    least = np.array([scoredist.least_score(np.asarray(m)) for m in mats])
    out = np.zeros((len(widths), a.bins + 2), dtype=np.int64)
    ms = {"tail": [], "full": [], "best": []}
    sums = {}
    for _ in range(a.warmup + a.repeats):
        t = {}
        _lib.score_histogram(pw, sq, 3, 0.7, hi, a.bins, True, -1, out=out, timing=t)
        ms["tail"].append(t["device_ms"])
        sums["tail"] = out.sum(axis=1)
        in_tail = int(out[:, 1:].sum())
        _lib.score_histogram(pw, sq, 3, least, hi, a.bins, True, -1, out=out, timing=t)
        ms["full"].append(t["device_ms"])
        sums["full"] = out.sum(axis=1)
        below_full = int(out[:, 0].sum())
        best = _lib.scan_best(pw, sq, 3)
        ms["best"].append(best.device_ms())
        best.close()
    n_windows = np.maximum(np.diff(offsets)[None, :] - np.asarray(widths, dtype=np.int64)[:, None] + 1, 0).sum(axis=1)
    same = bool(np.array_equal(sums["tail"], n_windows) and np.array_equal(sums["full"], n_windows) and below_full == 0)
    sq.close()
    pw.close()
    line = {"device": _lib.device_name(), "regions": a.regions, "length": a.length, "motifs": len(widths), "bins": a.bins, "per_position": True,
            "strands": 2, "windows": int(n_windows.sum()), "windows_at_or_above_0.7": in_tail, "row_sums_equal_window_counts": same,
            "warmup": a.warmup, "repeats": a.repeats}
    for k, v in ms.items():
        m = v[a.warmup:]
        line[k + "_ms"] = {"median": statistics.median(m), "min": min(m), "max": max(m), "all": v}
    print(json.dumps(line))
    if not same:
        raise SystemExit("a row of a histogram does not sum to the motif's window count")


if __name__ == "__main__":
    main()
