#!/usr/bin/env python3
"""
tools/shuffle_time.py -- what a shuffled control set costs beside the scan it feeds ("Shuffled control sequences").

    python tools/shuffle_time.py [--regions 1000000] [--length 500] [--motifs 579] [--warmup 2] [--repeats 20] [--out FILE]

Default: the benchmark's set, 1 M regions x 500 bp from synth.  Timed in one process, each as the median of --repeats after --warmup:
  * ms_seqset_shuffle of the set for both kinds: the host clock around the call (it returns synchronised) and the sum and split of its
    four device stages (ms_debug_shuffle_stage_ms);
  * the creation of the same set by ms_seqset_from_genome from a resident genome that holds the regions back to back (host clock);
  * ms_scan_best of the motif set on it, both strands (ms_best_device_ms) -- on the input set and on its dinucleotide shuffle.
Prints one JSON line and writes it to --out if given.  Needs an MI355X.
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


def median_of(fn, warmup, repeats):
    vals = [fn() for _ in range(warmup + repeats)]
    return statistics.median(vals[warmup:]), vals[warmup:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=1_000_000)
    ap.add_argument("--length", type=int, default=500)
    ap.add_argument("--motifs", type=int, default=579)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if _lib.device_count() < 1:
        raise SystemExit("shuffle_time needs an MI355X: no HIP device visible and there is no CPU fallback")
    _lib.set_device(0)
    vals, widths, cutoffs = synth.load_motif_set(a.motifs)
    pw = _lib.PwmSet(vals, widths, cutoffs)
    bases, offsets = synth.make_regions(a.regions, a.length, seed=1)
    sq = _lib.SeqSet(bases, offsets)
    genome = _lib.ResidentGenome({"all": bases})
    starts = np.ascontiguousarray(offsets[:-1])
    ends = np.ascontiguousarray(offsets[1:])
    chrom = np.zeros(a.regions, dtype=np.int32)

    def shuffle_call(kind, stages):
        t0 = time.perf_counter()
        sh = sq.shuffled(kind, 1)
        ms = (time.perf_counter() - t0) * 1e3
        stages.append(_lib.shuffle_stage_ms())
        sh.close()
        return ms

    def extract_call():
        t0 = time.perf_counter()
        cut = genome.extract(chrom, starts, ends)
        ms = (time.perf_counter() - t0) * 1e3
        cut.close()
        return ms

    def best_call(s):
        b = _lib.scan_best(pw, s, 3)
        ms = b.device_ms()
        b.close()
        return ms

    out = {"device": _lib.device_name(), "regions": a.regions, "length": a.length, "motifs": len(widths), "repeats": a.repeats}
    for kind in ("mono", "dinuc"):
        stages = []
        wall, wall_all = median_of(lambda: shuffle_call(kind, stages), a.warmup, a.repeats)
        st = np.median(np.array(stages[a.warmup:]), axis=0)
        out[f"shuffle_{kind}_wall_ms"] = wall
        out[f"shuffle_{kind}_device_ms"] = float(st.sum())
        out[f"shuffle_{kind}_stage_ms"] = [float(x) for x in st]
        out[f"shuffle_{kind}_wall_ms_min_max"] = [min(wall_all), max(wall_all)]
    out["from_genome_wall_ms"], _ = median_of(extract_call, a.warmup, a.repeats)
    out["scan_best_device_ms"], best_all = median_of(lambda: best_call(sq), a.warmup, a.repeats)
    out["scan_best_device_ms_min_max"] = [min(best_all), max(best_all)]
    di = sq.shuffled("dinuc", 1)
    out["scan_best_on_dinuc_shuffle_device_ms"], _ = median_of(lambda: best_call(di), a.warmup, a.repeats)
    di.close()
    out["dinuc_shuffle_over_scan_best"] = out["shuffle_dinuc_wall_ms"] / out["scan_best_device_ms"]
    for h in (sq, genome, pw):
        h.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
