#!/usr/bin/env python3
"""
tools/dimodel_time.py -- device time of ms_scan_best_dimodels beside ms_scan_best's on the same resident sequence set, in one process
("First-order models: best site per (model, region)").

    python tools/dimodel_time.py [--regions 100000] [--length 500] [--motifs 579] [--warmup 1] [--repeats 5] [--out FILE]

Default: 100 000 regions x 500 bp, without non-ACGT bases, x the 579 shipped motifs.  The first-order models are DiModel.from_pwm of
those PWMs, so both calls answer the same question and their three planes must be equal byte for byte: the tool checks that before it
reports a time.  Per repeat the set is scanned by ms_scan_best and by ms_scan_best_dimodels in turn; the figures are the medians of
ms_best_device_ms (HIP events on the library's stream: first launch -> last kernel done) over --repeats after --warmup.  Counted from
the shapes, not measured: the tiles of either walk (a model's table is 4 W - 3 PWM columns' worth of entries, so a tile holds about a
quarter as many models and the segments' words are read that many more times).  Prints one JSON line and writes it to --out if given.
Needs an MI355X.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from motifscan_amd import _lib, dimodel, synth  # noqa: E402


def tiles(entries, tile_entries):
    """Tiles of a run of consecutive scorable tables taken greedily, as the dense plan takes them."""
    n, used = 0, 0
    for e in entries:
        if used and used + e > tile_entries:
            n, used = n + 1, 0
        used += e
    return n + (1 if used else 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=100_000)
    ap.add_argument("--length", type=int, default=500)
    ap.add_argument("--motifs", type=int, default=579)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.repeats < 5:
        raise SystemExit("dimodel_time reports a median of at least 5 runs")
    if _lib.device_count() < 1:
        raise SystemExit("dimodel_time needs an MI355X: no HIP device visible and there is no CPU fallback")
    _lib.set_device(0)
    vals, widths, cutoffs = synth.load_motif_set(a.motifs)
    pw = _lib.PwmSet(vals, widths, cutoffs)
    ms = _lib.DiModelSet.from_models([dimodel.DiModel.from_pwm(m) for m in synth.matrices_of(vals, widths)])
    sq = _lib.SeqSet(*synth.make_regions(a.regions, a.length, seed=1, frac_n=0.0))

    b, d = _lib.scan_best(pw, sq, 3), _lib.scan_best_dimodels(ms, sq, 3)
    same = all(x.tobytes() == y.tobytes() for x, y in zip(b.sites(), d.sites()))
    b.close()
    d.close()

    def best_scan():
        r = _lib.scan_best(pw, sq, 3)
        t = r.device_ms()
        r.close()
        return t

    def dimodel_scan():
        r = _lib.scan_best_dimodels(ms, sq, 3)
        t = r.device_ms()
        r.close()
        return t

    both = [(best_scan(), dimodel_scan()) for _ in range(a.warmup + a.repeats)]          # in turn: a drift of the clock meets both alike
    best_all, di_all = [t[0] for t in both], [t[1] for t in both]
    best, di = statistics.median(best_all[a.warmup:]), statistics.median(di_all[a.warmup:])
    dims = _lib.dimodel_dims()
    out = {"device": _lib.device_name(), "regions": a.regions, "length": a.length, "motifs": len(widths), "mean_width": float(np.mean(widths)),
           "windows_both_strands": 2.0 * sum(a.regions * max(a.length - int(w) + 1, 0) for w in widths),
           "best_device_ms": best, "dimodel_device_ms": di, "ratio_dimodel_over_best": di / best,
           "best_tiles": tiles([4 * int(w) for w in widths], dims["tile_entries"]),
           "dimodel_tiles": tiles([4 * (4 * int(w) - 3) for w in widths], dims["tile_entries"]),
           "planes_equal": same, "warmup": a.warmup, "repeats": a.repeats, "best_ms_all": best_all, "dimodel_ms_all": di_all}
    sq.close()
    ms.close()
    pw.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if not same:
        raise SystemExit("the degenerate models' planes differ from ms_scan_best's")


if __name__ == "__main__":
    main()
