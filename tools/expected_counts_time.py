#!/usr/bin/env python3
"""
tools/expected_counts_time.py -- device time of ms_affinity_expected_counts beside ms_scan_affinity's on the same handles, in one process
("Expected base counts per motif column").

    python tools/expected_counts_time.py [--regions 125000] [--length 500] [--motifs 579] [--warmup 1] [--repeats 3] [--out FILE]

Default: one GPU's share of BASELINE configs[3] -- 125 000 regions x 500 bp x the 579 motifs, both strands.  Three cases, each on its own
affinity handle: OOPS (prior_logit = +inf) and prior_logit = 0 with the library's matrices, and OOPS with the 579 matrices flattened
(x 0.25), so that few weights round to 0 and nearly every term adds under every column.  The yardstick is ms_scan_affinity of the same
handles: the walk the new call repeats.  The figures are the medians of ms_affinity_device_ms and of the call's own device_ms (HIP events
on the library's stream) over --repeats after --warmup.  Also reported: the share of counts cells that are non-zero and the occupancy
(total * 2^-32 / n_regions) of the median motif, as a check that the case is what it claims.  Prints one JSON line and writes it to
--out if given.  Needs an MI355X.
"""
import argparse
import json
import math
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
        raise SystemExit("expected_counts_time needs an MI355X: no HIP device visible and there is no CPU fallback")
    _lib.set_device(0)
    vals, widths, cutoffs = synth.load_motif_set(a.motifs)
    vals = np.asarray(vals, dtype=np.float64)
    sq = _lib.SeqSet(*synth.make_regions(a.regions, a.length, seed=1))
    terms = 2.0 * sum(a.regions * max(a.length - int(w) + 1, 0) for w in widths)
    out = {"device": _lib.device_name(), "regions": a.regions, "length": a.length, "motifs": len(widths), "mean_width": float(np.mean(widths)),
           "terms_both_strands": terms, "dims": _lib.expected_dims()}
    for name, factor, prior in (("oops", 1.0, math.inf), ("prior0", 1.0, 0.0), ("flat_oops", 0.25, math.inf)):
        pw = _lib.PwmSet(vals * factor, widths, cutoffs)

        def affinity_scan():
            r = _lib.scan_affinity(pw, sq, 3, 1.0, -1)
            ms = r.device_ms()
            r.close()
            return ms
        aff, aff_all = median_ms(affinity_scan, a.warmup, a.repeats)
        res = _lib.scan_affinity(pw, sq, 3, 1.0, -1)
        last = {}

        def counted():
            last["out"] = res.expected_counts(pw, sq, prior)
            return res.expected_counts_ms
        exp, exp_all = median_ms(counted, a.warmup, a.repeats)
        counts, total, n_regions = last["out"]
        used = sum(int(w) * 4 for w in widths)
        occ = total * 2.0 ** -32 / np.maximum(n_regions, 1)
        out[name] = {"matrix_factor": factor, "prior_logit": "inf" if prior == math.inf else prior, "affinity_device_ms": aff, "expected_counts_device_ms": exp,
                     "ratio_expected_over_affinity": exp / aff, "ns_per_term_expected": exp * 1e6 / terms, "nonzero_share_of_acgt_cells": float((counts[:, :, :4] != 0).sum() / used),
                     "median_occupancy": float(np.median(occ)), "affinity_ms_all": aff_all, "expected_counts_ms_all": exp_all}
        res.close()
        pw.close()
    sq.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
