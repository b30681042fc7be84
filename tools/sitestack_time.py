#!/usr/bin/env python3
"""
tools/sitestack_time.py -- device time of ms_result_site_base_counts ("Site stacks") on the result of one
shard of the benchmark's kind, beside the time of ms_result_hits_host for the same result: the copy of the hit arrays that the host
route (slice the sequences in Python) has to pay before it can start.

    python tools/sitestack_time.py [--regions 125000] [--length 500] [--motifs 579] [--warmup 2] [--repeats 5]

One process, one scan (p = 1e-4, both strands, de-duplicated).  The count: --warmup calls first, then the median over --repeats calls
of the call's device_ms (HIP events on the library's stream) at flank 0 and 20, with and without dinuc, on one result whose hits
never leave the device.  The copy: --warmup + --repeats fresh results of the same scan, the wall-clock time of the first
ms_result_hits_host of each (it ends in a stream synchronise; later calls on one result return the cached copy), median of the last
--repeats.  Every used column of the counts is checked against n_sites.  Prints one JSON line.  Needs an MI355X.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from motifscan_amd import _lib, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=125000)
    ap.add_argument("--length", type=int, default=500)
    ap.add_argument("--motifs", type=int, default=579)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    if _lib.device_count() < 1:
        raise SystemExit("sitestack_time needs an MI355X: no HIP device visible and there is no CPU fallback")
    _lib.set_device(0)
    vals, widths, cutoffs = synth.load_motif_set(a.motifs, p_value="1e-4")
    bases, offsets = synth.make_regions(a.regions, a.length, seed=1)
    pw, sq = _lib.PwmSet(vals, widths, cutoffs), _lib.SeqSet(bases, offsets)

    copy_ms = []
    for _ in range(a.warmup + a.repeats):
        res = _lib.scan(pw, sq, 3).dedup(pw)
        t0 = time.perf_counter()
        res.hits(copy=False, motif=False)
        copy_ms.append((time.perf_counter() - t0) * 1e3)
        res.close()

    res = _lib.scan(pw, sq, 3).dedup(pw)
    n_hits = res.n_hits
    count_ms = {}
    for flank in (0, 20):
        for dinuc in (False, True):
            ms = []
            for _ in range(a.warmup + a.repeats):
                counts, di, n_sites = res.site_base_counts(pw, sq, flank, dinuc=dinuc)
                ms.append(res.site_base_counts_ms)
            for m, W in enumerate(widths):
                if not (counts[m, :W + 2 * flank].sum(axis=1) == n_sites[m]).all():
                    raise SystemExit(f"motif {m}: a column does not sum to the number of sites")
            if int(n_sites.sum()) != n_hits:
                raise SystemExit("n_sites does not sum to the number of hits")
            count_ms[f"flank{flank}" + ("_dinuc" if dinuc else "")] = ms
    res.close()
    sq.close()
    pw.close()
    copy = statistics.median(copy_ms[a.warmup:])
    med = {k: statistics.median(v[a.warmup:]) for k, v in count_ms.items()}
    print(json.dumps({"device": _lib.device_name(), "regions": a.regions, "length": a.length, "motifs": len(widths), "strands": 2,
                      "p_value": "1e-4", "deduped": True, "n_hits": n_hits, "mean_width": float(np.mean(widths)),
                      "site_base_counts_device_ms": med, "hits_host_ms": copy, "hits_host_bytes": 25 * n_hits,
                      "ratio_copy_over_count": {k: copy / v for k, v in med.items()},
                      "site_base_counts_ms_all": count_ms, "hits_host_ms_all": copy_ms}))


if __name__ == "__main__":
    main()
