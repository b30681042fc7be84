#!/usr/bin/env python3
"""
tools/best_time.py -- device time of ms_scan_best on one shard of the benchmark's kind ("The best-scoring window of
every (motif, region) cell"), beside the fp64 stage of an exact-only ms_scan of the same input: the same fp64 work per window through
exact_tiled_kernel, one motif per block row, its hits emitted.

    python tools/best_time.py [--regions 20000] [--length 500] [--motifs 579] [--warmup 2] [--repeats 5]

One process; --warmup calls of each path first, then the median over --repeats calls of ms_best_device_ms and of ms_scan_stats.ms_exact
(HIP events on the library's stream).  Prints one JSON line: both figures, their ratio and the U/s (bp x motifs / s) the first implies.
Needs an MI355X.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from motifscan_amd import _lib, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=20000)
    ap.add_argument("--length", type=int, default=500)
    ap.add_argument("--motifs", type=int, default=579)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    if _lib.device_count() < 1:
        raise SystemExit("best_time needs an MI355X: no HIP device visible and there is no CPU fallback")
    _lib.set_device(0)
    vals, widths, cutoffs = synth.load_motif_set(a.motifs)
    bases, offsets = synth.make_regions(a.regions, a.length, seed=1)
    pw, sq = _lib.PwmSet(vals, widths, cutoffs), _lib.SeqSet(bases, offsets)
    best_ms, exact_ms = [], []
    for _ in range(a.warmup + a.repeats):
        b = _lib.scan_best(pw, sq, 3)
        best_ms.append(b.device_ms())
        b.close()
    for _ in range(a.warmup + a.repeats):
        r = _lib.scan(pw, sq, 3, _lib.MS_SCAN_EXACT_ONLY)
        exact_ms.append(r.stats()["ms_exact"])
        r.close()
    sq.close()
    pw.close()
    best, exact = statistics.median(best_ms[a.warmup:]), statistics.median(exact_ms[a.warmup:])
    bp_motifs = float(a.regions) * a.length * len(widths)
    print(json.dumps({"device": _lib.device_name(), "regions": a.regions, "length": a.length, "motifs": len(widths), "strands": 2,
                      "mean_width": float(np.mean(widths)), "best_device_ms": best, "exact_only_ms_exact": exact,
                      "ratio_best_over_exact": best / exact, "best_U_per_s": bp_motifs / (best * 1e-3),
                      "best_ms_all": best_ms, "exact_ms_all": exact_ms}))


if __name__ == "__main__":
    main()
