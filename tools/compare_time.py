#!/usr/bin/env python3
"""
tools/compare_time.py -- device time of ms_motifs_compare ("Motif comparison") for the shipped synth_jaspar579 set
against itself, beside what the call computes and the numpy restatement of one query row.

    python tools/compare_time.py [--motifs 579] [--metric pearson] [--bins 100] [--forward-only] [--warmup 2] [--repeats 7]

One process, one device.  --warmup calls, then --repeats measured ones; the time is the library's own event time (`device_ms`: first
launch -> last kernel done, the copies of the planes to the host not included), reported as median, minimum and maximum, and beside it
the host's wall time of the whole call (plan, upload, kernels, copy-out).  Counted from the shapes, not measured:
    hist_cells    column scores the histogram forms: query columns x target columns x orientations
    align_cells   column scores the alignment forms: per pair and orientation the cells of the admissible diagonals
    table_macs    multiply-adds of the convolved tables: per table (a, L >= 2) its entries x the terms of each
    table_mib     the tables of all queries
Prints one JSON line.  Needs an MI355X.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from motifscan_amd import _lib, compare, synth  # noqa: E402


def library_ppm(n):
    values, widths, _ = synth.load_motif_set(n)
    out = []
    for m in synth.matrices_of(values, widths):
        p = np.exp(m) * synth.BG[:, None]
        out.append(np.ascontiguousarray(p / p.sum(axis=0)))
    return out


def counts(widths, bins, min_overlap, orientations):
    w = np.asarray(widths, dtype=np.int64)
    cols = int(w.sum())
    align = 0
    for wq in np.unique(w):
        nq = int((w == wq).sum())
        for wt in np.unique(w):
            nt = int((w == wt).sum())
            need = min(min_overlap, wq, wt)
            o = np.arange(-(wt - 1), wq)
            L = np.minimum(wq, wt + o) - np.maximum(o, 0)
            align += nq * nt * int(L[L >= need].sum())
    macs = 0
    for W in w.tolist():
        for a in range(W):
            for L in range(2, W - a + 1):
                macs += ((L - 1) * (bins - 1) + 1) * bins                 # every entry of table (a, L - 1) meets every bin of the new column once
    doubles = sum(compare.table_doubles(W, bins) for W in w.tolist())
    return dict(hist_cells=cols * cols * orientations, align_cells=align * orientations, table_macs=macs, table_mib=doubles * 8 / 2 ** 20)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--motifs", type=int, default=579)
    ap.add_argument("--metric", default="pearson", choices=sorted(compare.METRICS))
    ap.add_argument("--bins", type=int, default=100)
    ap.add_argument("--min-overlap", type=int, default=5)
    ap.add_argument("--forward-only", action="store_true")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()
    if _lib.device_count() < 1:
        raise SystemExit("compare_time needs an MI355X: no HIP device visible and there is no CPU fallback")
    _lib.set_device(0)
    mats = library_ppm(a.motifs)
    values = np.concatenate([m.ravel() for m in mats])
    widths = np.array([m.shape[1] for m in mats], dtype=np.int32)
    orientations = 1 if a.forward_only else 3
    ms, wall = [], []
    for _ in range(a.warmup + a.repeats):
        t = {}
        t0 = time.perf_counter()
        planes = _lib.compare_motifs(values, widths, values, widths, compare.METRICS[a.metric], a.bins, a.min_overlap, orientations, timing=t)
        wall.append((time.perf_counter() - t0) * 1e3)
        ms.append(t["device_ms"])
    diag_ok = bool(np.all(np.diagonal(planes["offset"]) == 0) and np.all(np.diagonal(planes["overlap"]) == widths))
    t0 = time.perf_counter()
    compare.restate_compare(mats[:1], mats, a.metric, a.bins, a.min_overlap, not a.forward_only)
    restate_s = time.perf_counter() - t0
    m, w = ms[a.warmup:], wall[a.warmup:]
    out = {"device": _lib.device_name(), "motifs": len(mats), "columns": int(widths.sum()), "metric": a.metric, "bins": a.bins, "min_overlap": a.min_overlap,
           "orientations": orientations, "budget_mib": _lib.compare_dims()["budget_mib"],
           "device_ms": {"median": statistics.median(m), "min": min(m), "max": max(m), "all": ms},
           "wall_ms": {"median": statistics.median(w), "min": min(w), "max": max(w)}, "restate_one_row_s": restate_s,
           "self_at_offset_0_full_overlap": diag_ok, "warmup": a.warmup, "repeats": a.repeats}
    out.update(counts(widths, a.bins, a.min_overlap, 2 if orientations == 3 else 1))
    print(json.dumps(out))
    if not diag_ok:
        raise SystemExit("a motif's alignment with itself is not the full overlap at offset 0")


if __name__ == "__main__":
    main()
