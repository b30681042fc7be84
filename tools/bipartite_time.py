#!/usr/bin/env python3
"""
tools/bipartite_time.py -- device time of ms_scan_best_bipartite beside ms_scan_best's of the element motifs on the same resident
sequence set, in one process ("Bipartite motifs: best site of two half-sites with a variable spacer").

    python tools/bipartite_time.py [--regions 100000] [--length 500] [--specs 64] [--gap-max 10] [--warmup 1] [--repeats 5] [--out FILE]

Default: 100 000 regions x 500 bp, without non-ACGT bases; 64 specs drawn from the shipped set -- motif i with motif i + 64, gaps 0 .. 10,
flip = i & 1 -- and, beside it, ms_scan_best of the 128 element motifs: the work the bipartite walk repeats (it forms both elements' sums
per spec) before it places anything.  Before a time is reported the four planes of the first 64 regions are compared with the numpy
restatement (bipartite.best_bipartite_host), byte for byte.  Per repeat the set is scanned by both calls in turn; the figures are the
medians of ms_best_device_ms (HIP events on the library's stream: first launch -> last kernel done) over --repeats after --warmup.
Counted from the shapes, not measured: the placements (start, strand, gap) the walk scores, and the LDS reads of a placement's partner
per window start -- one 8-byte read per strand and gap.  Prints one JSON line and writes it to --out if given.  Needs an MI355X.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from motifscan_amd import _lib, bipartite, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=100_000)
    ap.add_argument("--length", type=int, default=500)
    ap.add_argument("--specs", type=int, default=64)
    ap.add_argument("--gap-max", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.repeats < 5:
        raise SystemExit("bipartite_time reports a median of at least 5 runs")
    if _lib.device_count() < 1:
        raise SystemExit("bipartite_time needs an MI355X: no HIP device visible and there is no CPU fallback")
    _lib.set_device(0)
    n = a.specs
    vals, widths, cutoffs = synth.load_motif_set(2 * n)
    mats = synth.matrices_of(vals, widths)
    specs = [bipartite.Bipartite(i, i + n, i & 1, 0, a.gap_max) for i in range(n)]
    pw = _lib.PwmSet(vals, widths, cutoffs)
    bases, offsets = synth.make_regions(a.regions, a.length, seed=1, frac_n=0.0)
    sq = _lib.SeqSet(bases, offsets)

    # ---- the planes of the first 64 regions against the restatement, before any time is reported
    n_check = min(64, a.regions)
    r = _lib.scan_best_bipartite(pw, specs, sq, 3)
    got = r.sites() + (r.gaps(),)
    r.close()
    subset = [bytes(bases[offsets[i]:offsets[i + 1]]).decode("latin-1") for i in range(n_check)]
    want = bipartite.best_bipartite_host(mats, specs, subset, 3)
    same = all(np.ascontiguousarray(g[:, :n_check]).tobytes() == w.tobytes() for g, w in zip(got, want))
    if not same:
        raise SystemExit("the planes of the first %d regions differ from the restatement" % n_check)

    def best_scan():
        r = _lib.scan_best(pw, sq, 3)
        t = r.device_ms()
        r.close()
        return t

    def bipartite_scan():
        r = _lib.scan_best_bipartite(pw, specs, sq, 3)
        t = r.device_ms()
        r.close()
        return t

    both = [(best_scan(), bipartite_scan()) for _ in range(a.warmup + a.repeats)]        # in turn: a drift of the clock meets both alike
    best_all, bp_all = [t[0] for t in both], [t[1] for t in both]
    best, bp = statistics.median(best_all[a.warmup:]), statistics.median(bp_all[a.warmup:])
    n_gaps = a.gap_max + 1
    placements = 2.0 * a.regions * sum(max(a.length - (int(widths[s.a]) + g + int(widths[s.b])) + 1, 0) for s in specs for g in range(n_gaps))
    dims = _lib.bipartite_dims()
    out = {"device": _lib.device_name(), "regions": a.regions, "length": a.length, "specs": n, "gaps": [0, a.gap_max], "elements": 2 * n,
           "mean_element_width": float(np.mean(widths)), "element_windows_both_strands": 2.0 * sum(a.regions * max(a.length - int(w) + 1, 0) for w in widths),
           "placements": placements, "lds_partner_reads_per_window_start": 2 * n_gaps,
           "best_device_ms": best, "bipartite_device_ms": bp, "ratio_bipartite_over_best": bp / best,
           "ns_per_placement": bp * 1e6 / placements, "lds_bytes_per_block": dims["lds_bytes"], "tile_entries": dims["tile_entries"],
           "planes_equal_on_first_regions": same, "checked_regions": n_check, "warmup": a.warmup, "repeats": a.repeats,
           "best_ms_all": best_all, "bipartite_ms_all": bp_all}
    sq.close()
    pw.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
