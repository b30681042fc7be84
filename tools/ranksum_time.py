#!/usr/bin/env python3
"""
tools/ranksum_time.py -- cutoff-free enrichment on the device ("Cutoff-free enrichment over best-site matrices")
beside what a user does without it, on one GPU.

    python tools/ranksum_time.py [--regions 100000] [--length 500] [--motifs 579] [--cutoffs 4] [--warmup 1] [--repeats 3]
                                 [--host-motifs 0] [--sort-forms auto,row,segmented] [--out profiles/r12_ranksum_time.json]

Input + control regions of --regions each are scanned with ms_scan_best (its device time is reported); then, median over --repeats calls
after --warmup:
  * ms_best_rank_sum of the two matrices, wall clock and the library's event time, once per sort form of --sort-forms ("auto": the
    product, which picks a form per group by its size; "row": one device radix sort per motif row and group; "segmented": one
    segmented radix sort per batch and group -- the last two forced with MS_MEASURE=1 MS_RANKSUM_SORT=row | segmented);
  * ms_best_count_passing with --cutoffs cutoffs per motif on either matrix;
  * the host route: ms_best_sites to the host (the copy), then numpy sort / searchsorted per row (enrich.rank_sum_host) and the
    comparisons of enrich.count_passing_host.  --host-motifs K > 0 runs it for the first K motifs only (the 1 M + 1 M job: 9.3 GB of
    scores) and reports the time per motif as well.
Both routes must give the same integers (checked; the run fails otherwise).  Writes one JSON object to --out and prints it.
Needs an MI355X.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from motifscan_amd import _lib, enrich, synth  # noqa: E402


def timed(fn, warmup, repeats):
    """(median wall seconds, median device ms, last result)"""
    wall, dev, out = [], [], None
    for i in range(warmup + repeats):
        timing = {}
        t0 = time.perf_counter()
        out = fn(timing)
        if i >= warmup:
            wall.append(time.perf_counter() - t0)
            dev.append(timing.get("device_ms", float("nan")))
    return statistics.median(wall), statistics.median(dev), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=100_000)
    ap.add_argument("--length", type=int, default=500)
    ap.add_argument("--motifs", type=int, default=579)
    ap.add_argument("--cutoffs", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--host-motifs", type=int, default=0)
    ap.add_argument("--sort-forms", default="auto,row,segmented")
    ap.add_argument("--out", default=os.path.join("profiles", "r12_ranksum_time.json"))
    a = ap.parse_args()
    if _lib.device_count() < 1:
        raise SystemExit("ranksum_time needs an MI355X: no HIP device visible and there is no CPU fallback")
    _lib.set_device(0)
    vals, widths, cutoffs = synth.load_motif_set(a.motifs)
    P = len(widths)
    pw = _lib.PwmSet(vals, widths, cutoffs)
    best, scan_ms = [], []
    for seed in (1, 2):
        bases, offsets = synth.make_regions(a.regions, a.length, seed=seed)
        sq = _lib.SeqSet(bases, offsets)
        del bases
        _lib.scan_best(pw, sq, 3).close()                 # warm-up
        b = _lib.scan_best(pw, sq, 3)
        scan_ms.append(b.device_ms())
        best.append(b)
        sq.close()
    inp, ctl = best
    out = {"device": _lib.device_name(), "regions_input": a.regions, "regions_control": a.regions, "length": a.length, "motifs": P,
           "strands": 2, "warmup": a.warmup, "repeats": a.repeats, "scan_best_device_ms": scan_ms,
           "score_matrix_bytes": 2 * 8 * P * a.regions, "budget_elems": _lib.ranksum_dims()["budget"]}

    results = {}
    for form in [f for f in a.sort_forms.split(",") if f]:
        if form in ("row", "segmented"):
            os.environ["MS_MEASURE"], os.environ["MS_RANKSUM_SORT"] = "1", form
        else:
            os.environ.pop("MS_RANKSUM_SORT", None)
        wall, dev, res = timed(lambda t: inp.rank_sum(ctl, timing=t), a.warmup, a.repeats)
        results[form] = res
        out[f"rank_sum_{form}_wall_s"], out[f"rank_sum_{form}_device_ms"] = wall, dev
    os.environ.pop("MS_RANKSUM_SORT", None)
    forms = list(results)
    for f in forms[1:]:
        if not (np.array_equal(results[f][0], results[forms[0]][0]) and results[f][1:] == results[forms[0]][1:]):
            raise SystemExit(f"sort forms {forms[0]} and {f} disagree")
    u2, ties, na, nb = results[forms[0]]

    rng = np.random.default_rng(3)
    cut = np.sort(rng.uniform(0.6, 0.95, size=(P, a.cutoffs)), axis=1)
    wall, dev, counts_in = timed(lambda t: inp.count_passing(cut, timing=t), a.warmup, a.repeats)
    counts_ctl = ctl.count_passing(cut)
    out["count_passing_wall_s"], out["count_passing_device_ms"], out["cutoffs_per_motif"] = wall, dev, a.cutoffs

    # the host route, in slices of motif rows so that the host copy stays small
    K = P if a.host_motifs <= 0 else min(P, a.host_motifs)
    step = max(1, min(K, (1 << 24) // max(1, a.regions)))
    t_copy = t_rank = t_count = 0.0
    for m0 in range(0, K, step):
        m1 = min(K, m0 + step)
        t0 = time.perf_counter()
        xa, xb = inp.sites(m0, m1)[0], ctl.sites(m0, m1)[0]
        t1 = time.perf_counter()
        host = enrich.rank_sum_host(xa, xb)
        t2 = time.perf_counter()
        host_in, host_ctl = enrich.count_passing_host(xa, cut[m0:m1]), enrich.count_passing_host(xb, cut[m0:m1])
        t3 = time.perf_counter()
        t_copy, t_rank, t_count = t_copy + t1 - t0, t_rank + t2 - t1, t_count + t3 - t2
        if not (np.array_equal(host.u2, u2[m0:m1]) and host.ties == ties[m0:m1] and (host.na, host.nb) == (na, nb)):
            raise SystemExit(f"device and host rank sums disagree in motifs [{m0}, {m1})")
        if not (np.array_equal(host_in, counts_in[m0:m1]) and np.array_equal(host_ctl, counts_ctl[m0:m1])):
            raise SystemExit(f"device and host counts disagree in motifs [{m0}, {m1})")
    out.update({"host_motifs": K, "host_copy_s": t_copy, "host_rank_sum_s": t_rank, "host_count_passing_both_sets_s": t_count,
                "host_route_s_per_motif": (t_copy + t_rank) / K, "host_route_s_all_motifs_scaled": (t_copy + t_rank) * P / K,
                "same_integers": True, "ties_max_bits": max(t.bit_length() for t in ties), "auroc_range": [float(np.nanmin(enrich.RankSum(u2, ties, na, nb).auroc())),
                                                                                                      float(np.nanmax(enrich.RankSum(u2, ties, na, nb).auroc()))]})
    for b in best:
        b.close()
    pw.close()
    text = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
