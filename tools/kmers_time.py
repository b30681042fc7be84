#!/usr/bin/env python3
"""
tools/kmers_time.py -- what the k-mer counts cost beside their two yardsticks ("K-mer counts").

    python tools/kmers_time.py [--regions 1000000] [--length 500] [--genome-mbp 250] [--hot-bases 100000000] [--motifs 579]
                               [--repeats 5] [--out FILE]

Timed in one process, each as the median device_ms of --repeats calls after one warm call:
  * ms_seqset_kmer_counts of the benchmark's set (1 M regions x 500 bp from synth) at k = 6, 8, 10, 12, canonical, with and without nseq;
  * ms_genome_kmer_counts of a synthetic single-chromosome genome at k = 8 and 12, with and without nseq, next to ms_genome_base_counts
    on the same genome (host clock around the call: it returns synchronised and reads the same planes once);
  * the hot-bin input: poly-A and (AC)n in the proportion 7 : 4, as two sequences, at k = lds_k and lds_k + 1 and at 12, occ only;
  * 256 sequences just above sort_windows at k = 12 with nseq: the clearing of one 2 MiB bitmap each;
  * ms_scan_best of the motif set on the 1 M x 500 bp set, both strands: what an enrichment by scanning costs.
Prints one JSON line per group as it goes, then the whole as one line, and writes that to --out if given.  Needs an MI355X.
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


def median_ms(fn, repeats):
    fn()
    vals = [fn() for _ in range(repeats)]
    return statistics.median(vals), [min(vals), max(vals)]


def kmer_call(handle, k, nseq, occ, nsq):
    t = {}
    handle.kmer_counts(k, canonical=True, nseq=nseq, out=(occ, nsq if nseq else None), timing=t)
    return t["device_ms"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=1_000_000)
    ap.add_argument("--length", type=int, default=500)
    ap.add_argument("--genome-mbp", type=int, default=250)
    ap.add_argument("--hot-bases", type=int, default=100_000_000)
    ap.add_argument("--motifs", type=int, default=579)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if _lib.device_count() < 1:
        raise SystemExit("kmers_time needs an MI355X: no HIP device visible and there is no CPU fallback")
    _lib.set_device(0)
    dims = _lib.kmer_dims()
    out = {"device": _lib.device_name(), "dims": dims, "repeats": a.repeats}
    bufs = {k: (np.zeros(4 ** k, dtype=np.int64), np.zeros(4 ** k, dtype=np.int64)) for k in (6, dims["lds_k"], dims["lds_k"] + 1, 8, 10, 12)}

    def group(name, handle, ks, nseqs=(False, True)):
        res = {}
        for k in ks:
            for nseq in nseqs:
                med, span = median_ms(lambda: kmer_call(handle, k, nseq, *bufs[k]), a.repeats)
                res[f"k{k}_{'occ_nseq' if nseq else 'occ'}_device_ms"] = med
                res[f"k{k}_{'occ_nseq' if nseq else 'occ'}_min_max"] = span
        out[name] = res
        print(json.dumps({name: res}), flush=True)
        return res

    # ---- the benchmark's region set
    bases, offsets = synth.make_regions(a.regions, a.length, seed=1)
    sq = _lib.SeqSet(bases, offsets)
    out["regions"] = {"n": a.regions, "length": a.length}
    group("regions_kmers", sq, (6, 8, 10, 12))
    vals, widths, cutoffs = synth.load_motif_set(a.motifs)
    pw = _lib.PwmSet(vals, widths, cutoffs)

    def best_call():
        b = _lib.scan_best(pw, sq, 3)
        ms = b.device_ms()
        b.close()
        return ms

    out["scan_best_device_ms"], out["scan_best_min_max"] = median_ms(best_call, 2)
    out["motifs"] = len(widths)
    print(json.dumps({"scan_best_device_ms": out["scan_best_device_ms"]}), flush=True)
    pw.close()
    sq.close()
    del bases

    # ---- a synthetic genome of one chromosome
    n = a.genome_mbp * 1_000_000
    g_bases = np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.RandomState(7).randint(0, 4, n, dtype=np.uint8)]
    genome = _lib.ResidentGenome({"chr1": g_bases})
    del g_bases

    def base_call():
        t0 = time.perf_counter()
        genome.base_counts()
        return (time.perf_counter() - t0) * 1e3

    out["genome_bases"] = n
    out["genome_base_counts_wall_ms"], out["genome_base_counts_min_max"] = median_ms(base_call, a.repeats)
    print(json.dumps({"genome_base_counts_wall_ms": out["genome_base_counts_wall_ms"]}), flush=True)
    group("genome_kmers", genome, (dims["lds_k"], 8, 12))
    genome.close()

    # ---- hot bins
    na = a.hot_bases * 7 // 11
    hot = _lib.SeqSet.from_strings(["A" * na, "AC" * ((a.hot_bases - na) // 2)])
    out["hot_bases"] = a.hot_bases
    group("hot_bins", hot, (dims["lds_k"], dims["lds_k"] + 1, 12), nseqs=(False,))
    hot.close()

    # ---- many sequences just above sort_windows at k = 12
    L = dims["sort_windows"] + 100 + 11
    rs = np.random.RandomState(9)
    many = _lib.SeqSet(np.frombuffer(b"ACGT", dtype=np.uint8)[rs.randint(0, 4, 256 * L)], np.arange(257, dtype=np.int64) * L)
    out["just_above_sort_windows"] = {"n": 256, "length": L}
    group("just_above_sort_windows_kmers", many, (12,))
    many.close()

    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
