#!/usr/bin/env python3
"""
tools/build_motif_time.py -- times motif --build's genome-wide jobs on the resident genome (needs an MI355X):

  base_counts      ms_genome_base_counts (cal_bg_freq's counting) over a seeded synthetic genome of --gbp x 10^9 bases (default 1.2),
                   per call: host clock around the call, which ends in a stream synchronise (memset + kernel + 8 * 4 * n_chroms bytes
                   back); the floor is 0.375 B/base over the HBM streaming rate
  cal_bg_freq      the Python call on the resident genome (counts + the skip rule + rounding)
  random_windows   Genome.random_sequences' draws, 10^6 windows of the 579-motif set's widest motif (30), max_n = 0: numpy's choice,
                   the host replay of the start draws, the device N filter, the rewind of the global state
  extract + score_ranks   the sampled windows cut on the device and scored by the 579 PWMs (both strands), the cutoff ranks picked
  python_randint_loop     10^6 sequential np.random.randint(high) calls in a Python loop: what the host replay replaces

The synthetic genome is built straight in the packed layout (codes + nmask, N runs with code 0), 24 chromosomes of unequal sizes that
are not multiples of 32.  One JSON line on stdout, and in the file --out names (profiles/build_motif_time.json is such a line).
Usage: timeout -k 10 600 python3 tools/build_motif_time.py [--gbp 1.2] [--reps 20] [--out PATH]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from motifscan_amd import _lib, build, genome  # noqa: E402


def synthetic_packed(n_bases, seed):
    rng = np.random.default_rng(seed)
    w = rng.random(24) + 0.5
    sizes = np.floor(w / w.sum() * n_bases).astype(np.int64) | 1
    offsets = np.concatenate([[0], np.cumsum(sizes)])
    n = int(offsets[-1])
    units = (n + 31) // 32
    codes = rng.integers(0, 1 << 32, size=2 * units, dtype=np.uint32)
    nmask = np.zeros(units, dtype=np.uint32)
    runs = rng.integers(0, units, size=units // 2000)                     # N runs of 1 ... 64 units
    for u, ln in zip(runs.tolist(), rng.integers(1, 65, size=runs.size).tolist()):
        nmask[u:u + ln] = 0xFFFFFFFF
    codes[0::2][nmask != 0] = 0
    codes[1::2][nmask != 0] = 0
    tail = n - 32 * (units - 1)                                           # nothing past the last base
    if tail < 32:
        cw = (int(codes[-1]) << 32 | int(codes[-2])) & ((1 << (2 * tail)) - 1)
        codes[-2], codes[-1] = cw & 0xFFFFFFFF, cw >> 32
        nmask[-1] &= (1 << tail) - 1
    return genome.PackedGenome([f"chr{i + 1}" for i in range(24)], offsets, codes, nmask)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gbp", type=float, default=1.2)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--n-random", type=int, default=1_000_000)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    if _lib.device_count() < 1:
        raise SystemExit("needs an MI355X")
    _lib.set_device(0)
    out = {"tool": "build_motif_time", "device": _lib.device_name(), "gbp": a.gbp}
    t = time.perf_counter()
    pg = synthetic_packed(int(a.gbp * 1e9), 5)
    out["genome_make_s"] = time.perf_counter() - t
    out["n_bases"] = pg.n_bases
    t = time.perf_counter()
    rg = pg.to_resident()
    out["upload_s"] = time.perf_counter() - t
    rg.base_counts()                                                      # warm-up
    ts = []
    for _ in range(a.reps):
        t = time.perf_counter()
        counts = rg.base_counts()
        ts.append(time.perf_counter() - t)
    ts.sort()
    out["base_counts_ms"] = {"min": 1e3 * ts[0], "median": 1e3 * ts[len(ts) // 2], "max": 1e3 * ts[-1]}
    out["base_counts_GBps_median"] = 0.375 * pg.n_bases / ts[len(ts) // 2] / 1e9
    out["base_counts_floor_ms_at_6TBps"] = 0.375 * pg.n_bases / 6.0e12 * 1e3
    # a cheap check that the timed call computed the right thing: ACGT counts + non-ACGT bases = every base
    out["base_counts_total_ok"] = int(counts.sum()) + int(np.bitwise_count(pg.nmask).sum()) == pg.n_bases
    t = time.perf_counter()
    out["cal_bg_freq"] = genome.cal_bg_freq(rg)
    out["cal_bg_freq_s"] = time.perf_counter() - t

    d = np.load(os.path.join(ROOT, "motifscan_amd", "data", "synth_jaspar579.npz"))
    widths, vals = d["widths"], d["pwm_values"]
    L = int(widths.max())
    ranks = build.cutoff_ranks(a.n_random)
    pw = _lib.PwmSet(vals, widths, None)
    rg.random_windows(1000, L, 0, 1)                                      # warm-up
    t = time.perf_counter()
    ci, st = rg.random_windows(a.n_random, L, 0, 11)
    out["random_windows_s"] = time.perf_counter() - t
    t = time.perf_counter()
    sq = rg.extract(ci, st, st + L)
    out["extract_s"] = time.perf_counter() - t
    _lib.score_ranks(pw, sq, list(ranks.values()), 3)                      # warm-up of the scoring path
    t = time.perf_counter()
    _lib.score_ranks(pw, sq, list(ranks.values()), 3)
    out["score_ranks_s"] = time.perf_counter() - t
    out["sample_extract_score_s"] = out["random_windows_s"] + out["extract_s"] + out["score_ranks_s"]
    sq.close()
    pw.close()
    rg.close()
    hs = (np.asarray(list(pg.chrom_sizes.values()), dtype=np.int64) - L)[np.random.default_rng(3).integers(0, 24, size=a.n_random)].tolist()
    np.random.seed(1)
    t = time.perf_counter()
    for h in hs:
        np.random.randint(h)
    out["python_randint_loop_s"] = time.perf_counter() - t
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
