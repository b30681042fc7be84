#!/usr/bin/env python3
"""
tools/pairs_time.py -- wall-clock time of the motif-pair reductions (ms_result_cooccurrence, ms_result_pair_spacing; DESIGN.md section 4,
"Motif pairs") on one shard of the benchmark's kind, beside the same quantities computed in numpy from the same hit arrays on the host
(the only thing there is to compare with: the reference has no such function).

    python tools/pairs_time.py [--regions 20000] [--length 500] [--motifs 579] [--max-dist 100] [--warmup 2] [--repeats 5]

One process.  The shard is scanned once (1e-4 cutoffs, both strands, de-duplicated); then, per quantity, --warmup calls and the median
over --repeats wall-clock times of the synchronous call: the full motifs x motifs co-occurrence matrix, and the spacing of one
mid-frequency anchor (the motif with the median number of sites) against all motifs.  The numpy forms -- a bit matrix product for the
co-occurrence, a sorted join per partner for the spacing -- are timed once each and must give the same arrays.  Prints one JSON line.
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
from motifscan_amd import _lib, synth  # noqa: E402


def host_cooccurrence(h, P, R):
    has = np.zeros((P, R), dtype=np.float32)                    # exact in float32 up to 2^24 regions, and the product runs in BLAS
    has[np.repeat(np.arange(P), np.diff(h["motif_offsets"])), h["seq_idx"]] = 1
    return np.rint(has @ has.T).astype(np.int64)


def host_pair_spacing(h, widths, anchor, max_dist):
    """The join the device does, per partner: both slices are sorted by (region, position), so the partners in reach of every anchor
    site are a range found by two searchsorted calls over a combined key."""
    off, reg, pos, strand = h["motif_offsets"], h["seq_idx"], h["pos"], h["strand"].astype(np.int64)
    P, D2 = len(off) - 1, 2 * max_dist
    span = int(pos.max()) + 2 * max_dist + 256 if len(pos) else 1        # room for the reach on both sides (widths differ by < 128)
    key = reg * span + pos + max_dist + 64
    counts = np.zeros((P, 4, D2 + 1), dtype=np.int64)
    n_pairs = np.zeros(P, dtype=np.int64)
    a = slice(off[anchor], off[anchor + 1])
    for j in range(P):
        b = slice(off[j], off[j + 1])
        d = int(widths[j]) - int(widths[anchor])
        lo_off, hi_off = -((D2 + d) >> 1), (D2 - d) >> 1
        n_pairs[j] = (np.searchsorted(reg[b], reg[a], "right") - np.searchsorted(reg[b], reg[a], "left")).sum() - (a.stop - a.start if j == anchor else 0)
        lo = np.searchsorted(key[b], key[a] + lo_off, "left")
        hi = np.searchsorted(key[b], key[a] + hi_off, "right")
        n = hi - lo
        s = np.repeat(np.arange(a.start, a.stop), n)
        t = off[j] + np.repeat(lo - np.cumsum(n) + n, n) + np.arange(n.sum())
        keep = s != t
        s, t = s[keep], t[keep]
        cell = (2 * (strand[s] - 1) + strand[t] - 1) * (D2 + 1) + ((2 * (pos[t] - pos[s]) + d + D2) >> 1)
        counts[j] = np.bincount(cell, minlength=4 * (D2 + 1)).reshape(4, D2 + 1)
    return counts, n_pairs


def timed(fn, warmup, repeats):
    out, ms = None, []
    for _ in range(warmup + repeats):
        t0 = time.perf_counter()
        out = fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return out, statistics.median(ms[warmup:]), ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=20000)
    ap.add_argument("--length", type=int, default=500)
    ap.add_argument("--motifs", type=int, default=579)
    ap.add_argument("--max-dist", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    if _lib.device_count() < 1:
        raise SystemExit("pairs_time needs an MI355X: no HIP device visible and there is no CPU fallback")
    _lib.set_device(0)
    vals, widths, cutoffs = synth.load_motif_set(a.motifs)
    bases, offsets = synth.make_regions(a.regions, a.length, seed=1)
    pw, sq = _lib.PwmSet(vals, widths, cutoffs), _lib.SeqSet(bases, offsets)
    res = _lib.scan(pw, sq, 3).dedup(pw)
    P = len(widths)
    n_sites = np.diff(res.motif_offsets)
    anchor = int(np.argsort(n_sites, kind="stable")[P // 2])
    cooc, cooc_ms, cooc_all = timed(res.cooccurrence, a.warmup, a.repeats)
    (counts, n_pairs), sp_ms, sp_all = timed(lambda: res.pair_spacing(pw, anchor, a.max_dist), a.warmup, a.repeats)
    h = res.hits()
    t0 = time.perf_counter()
    want_cooc = host_cooccurrence(h, P, a.regions)
    t1 = time.perf_counter()
    want_counts, want_n = host_pair_spacing(h, widths, anchor, a.max_dist)
    t2 = time.perf_counter()
    same = bool(np.array_equal(cooc, want_cooc) and np.array_equal(counts, want_counts) and np.array_equal(n_pairs, want_n))
    res.close()
    sq.close()
    pw.close()
    print(json.dumps({"device": _lib.device_name(), "regions": a.regions, "length": a.length, "motifs": P, "strands": 2, "n_sites": int(n_sites.sum()),
                      "anchor": anchor, "anchor_sites": int(n_sites[anchor]), "max_dist": a.max_dist,
                      "cooccurrence_ms": cooc_ms, "cooccurrence_numpy_ms": (t1 - t0) * 1e3,
                      "pair_spacing_ms": sp_ms, "pair_spacing_numpy_ms": (t2 - t1) * 1e3, "pairs_in_range": int(counts.sum()),
                      "pairs_same_region": int(n_pairs.sum()), "device_equals_numpy": same,
                      "cooccurrence_ms_all": cooc_all, "pair_spacing_ms_all": sp_all}))
    if not same:
        raise SystemExit("the device and the numpy restatement disagree")


if __name__ == "__main__":
    main()
