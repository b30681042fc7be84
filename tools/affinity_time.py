#!/usr/bin/env python3
"""
tools/affinity_time.py -- device time of ms_scan_affinity beside ms_scan_best's on the same handles, and of ms_affinity_rank_sum beside
ms_best_rank_sum, in one process ("Total binding affinity per (motif, region)").

    python tools/affinity_time.py [--regions 125000] [--length 500] [--motifs 579] [--warmup 1] [--repeats 3] [--out FILE]

Default: one GPU's share of BASELINE configs[3] -- 125 000 input and 125 000 control regions x 500 bp x the 579 motifs, both strands.
Per repeat the input set is scanned by ms_scan_best and by ms_scan_affinity in turn (the same PwmSet and SeqSet handles); the figures
are the medians of ms_best_device_ms and ms_affinity_device_ms (HIP events on the library's stream) over --repeats after --warmup.
Then the control set is scanned once by each, and the two rank sums are timed the same way (their own device_ms).  The affinity scan is
also timed on one strand (half the terms at the same column work: what a term's exp costs) and with max_n = 0.  Prints one JSON
line and writes it to --out if given.  Needs an MI355X.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from motifscan_amd import _lib, synth  # noqa: E402


def median_ms(fn, warmup, repeats):
    times = [fn() for _ in range(warmup + repeats)]
    return statistics.median(times[warmup:]), times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=125_000)
    ap.add_argument("--length", type=int, default=500)
    ap.add_argument("--motifs", type=int, default=579)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if _lib.device_count() < 1:
        raise SystemExit("affinity_time needs an MI355X: no HIP device visible and there is no CPU fallback")
    _lib.set_device(0)
    vals, widths, cutoffs = synth.load_motif_set(a.motifs)
    pw = _lib.PwmSet(vals, widths, cutoffs)
    sets = [_lib.SeqSet(*synth.make_regions(a.regions, a.length, seed=seed)) for seed in (1, 2)]

    def best_scan(strand=3):
        b = _lib.scan_best(pw, sets[0], strand)
        ms = b.device_ms()
        b.close()
        return ms

    def affinity_scan(strand=3, max_n=-1):
        r = _lib.scan_affinity(pw, sets[0], strand, 1.0, max_n)
        ms = r.device_ms()
        r.close()
        return ms

    best, best_all = median_ms(best_scan, a.warmup, a.repeats)
    aff, aff_all = median_ms(affinity_scan, a.warmup, a.repeats)
    best1, _ = median_ms(lambda: best_scan(1), a.warmup, a.repeats)
    aff1, _ = median_ms(lambda: affinity_scan(1), a.warmup, a.repeats)
    aff_n0, _ = median_ms(lambda: affinity_scan(3, 0), a.warmup, a.repeats)

    def ranked(x, y):
        t = {}
        x.rank_sum(y, timing=t)
        return t["device_ms"]
    b0, b1 = (_lib.scan_best(pw, s, 3) for s in sets)
    best_rs, best_rs_all = median_ms(lambda: ranked(b0, b1), a.warmup, a.repeats)
    b0.close()
    b1.close()
    a0, a1 = (_lib.scan_affinity(pw, s, 3) for s in sets)
    aff_rs, aff_rs_all = median_ms(lambda: ranked(a0, a1), a.warmup, a.repeats)
    u2, _, na, nb = a0.rank_sum(a1)
    a0.close()
    a1.close()
    for s in sets:
        s.close()
    pw.close()
    terms = 2.0 * sum(a.regions * max(a.length - int(w) + 1, 0) for w in widths)
    out = {"device": _lib.device_name(), "regions_input": a.regions, "regions_control": a.regions, "length": a.length, "motifs": len(widths),
           "mean_width": float(np.mean(widths)), "terms_both_strands": terms,
           "best_device_ms": best, "affinity_device_ms": aff, "ratio_affinity_over_best": aff / best,
           "best_one_strand_ms": best1, "affinity_one_strand_ms": aff1, "affinity_max_n0_ms": aff_n0,
           "ns_per_term_affinity_minus_best": (aff - best) * 1e6 / terms,
           "best_rank_sum_ms": best_rs, "affinity_rank_sum_ms": aff_rs, "ratio_rank_sum": aff_rs / best_rs,
           "median_auroc_input_vs_control": float(np.median(u2 / (2.0 * na * nb))),
           "best_ms_all": best_all, "affinity_ms_all": aff_all, "best_rank_sum_ms_all": best_rs_all, "affinity_rank_sum_ms_all": aff_rs_all}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
