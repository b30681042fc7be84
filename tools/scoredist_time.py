#!/usr/bin/env python3
"""
tools/scoredist_time.py -- device time of ms_pwmset_score_distribution ("Analytic score distribution") for the
shipped synth_jaspar579 set, beside the least time its bytes could take and the numpy restatement of one motif.

    python tools/scoredist_time.py [--motifs 579] [--warmup 2] [--repeats 7] [--cases 0:4096,0:65536,3:16384]

One process, one device.  Per case "order:bins": --warmup calls, then --repeats measured ones, the cases taking turns (so that a drift
of the device's clock hits all alike); the time is the library's own event time (`device_ms`: first launch -> last kernel done) with
the output left in device memory (a torch tensor), reported as median, minimum and maximum.  Beside it:
    floor_ms     the bytes the recurrence must move -- 5 x 8 x C x bins per motif column: four shifted reads and one write of every
                 element -- over 6 TB/s, what a streaming kernel reaches on this device.  The LDS path moves none of them through HBM:
                 there the figure is a yardstick, not a bound.
    restate_s    pvalues.restate_distribution of ONE motif (the widest) on the host, in seconds
and the row sums are checked against 1.  Prints one JSON line per case.  Needs an MI355X.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from motifscan_amd import _lib, pvalues, synth  # noqa: E402

STREAM_BYTES_PER_S = 6.0e12


def synthetic_background(order):
    """A fixed non-uniform background of the order: GC-poor, with a depleted CG step."""
    base = np.array([0.3, 0.2, 0.2, 0.3])
    C = 4 ** order
    cond = np.tile(base, (C, 1))
    if order >= 1:
        cond[1::4, 2] *= 0.25                                     # G after C
        cond /= cond.sum(axis=1, keepdims=True)
    return cond, np.full(C, 1.0 / C)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--motifs", type=int, default=579)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--cases", default="0:4096,0:65536,3:16384")
    a = ap.parse_args()
    cases = [tuple(int(v) for v in c.split(":")) for c in a.cases.split(",")]
    if _lib.device_count() < 1:
        raise SystemExit("scoredist_time needs an MI355X: no HIP device visible and there is no CPU fallback")
    import torch
    _lib.set_device(0)
    vals, widths, _ = synth.load_motif_set(a.motifs)
    mats = [np.asarray(m, dtype=np.float64) for m in synth.matrices_of(vals, widths)]
    widest = max(mats, key=lambda m: m.shape[1])
    pw = _lib.PwmSet(vals, widths, None)
    dims = _lib.scoredist_dims()
    ms = {c: [] for c in cases}
    sums = {}
    for _ in range(a.warmup + a.repeats):
        for order, bins in cases:
            cond, init = synthetic_background(order)
            dev = torch.empty((len(widths), bins), dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
            t = {}
            _, step, _ = _lib.score_distribution(pw, 1, order, cond, init, bins, out=int(dev.data_ptr()), timing=t)
            ms[(order, bins)].append(t["device_ms"])
            sums[(order, bins)] = (dev.sum(dim=1).cpu().numpy(), step)
            del dev
    pw.close()
    ok = True
    for order, bins in cases:
        cond, init = synthetic_background(order)
        t0 = time.perf_counter()
        pvalues.restate_distribution([widest], cond, init, bins, 1)
        restate_s = time.perf_counter() - t0
        row, step = sums[(order, bins)]
        scorable = step > 0
        same = bool(np.all(np.abs(row[scorable] - 1.0) < 1e-9) and not row[~scorable].any())
        ok = ok and same
        columns = int(np.asarray(widths, dtype=np.int64)[scorable].sum())
        floor_ms = 5 * 8 * 4 ** order * bins * columns / STREAM_BYTES_PER_S * 1e3
        m = ms[(order, bins)][a.warmup:]
        print(json.dumps({"device": _lib.device_name(), "motifs": len(widths), "scorable": int(scorable.sum()), "columns": columns, "order": order,
                          "bins": bins, "path": "lds" if 4 ** order * bins <= dims["lds_elems"] else "global", "budget_mib": dims["budget_mib"],
                          "device_ms": {"median": statistics.median(m), "min": min(m), "max": max(m), "all": ms[(order, bins)]},
                          "floor_ms": floor_ms, "restate_one_motif_s": restate_s, "widest": int(widest.shape[1]), "rows_sum_to_one": same,
                          "warmup": a.warmup, "repeats": a.repeats}))
    if not ok:
        raise SystemExit("a row of a distribution does not sum to 1")


if __name__ == "__main__":
    main()
