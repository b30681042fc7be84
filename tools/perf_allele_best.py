#!/usr/bin/env python3
"""
tools/perf_allele_best.py -- times ms_scan_alleles_best (needs an MI355X).  One process: the synthetic 579-motif set, a seeded genome of
--genome-bp (200 000 000) bases in --chroms (8) chromosomes, --snvs (10^6) single-base substitutions and --indels (10^5) insertions and
deletions of up to --indel-len (50) bases.

  snv     ms_allelebest_device_ms of the substitutions against ms_varscan_device_ms of ms_scan_variants on the same input at p = 1e-4:
          the sparse scan is the yardstick -- it does the same column work and writes only the windows that pass.  What the dense scan
          has to pay beyond it is its output, 26 bytes per (motif, variant) cell: out_bytes / --hbm-write-tbs (6.0 TB/s: plain stores,
          MI355X) is reported as the byte floor, and ratio_to_yardstick_plus_floor = dense / (sparse + floor).
  indel   the same for the indels against ms_allelescan_device_ms of ms_scan_alleles at p = 1e-4.

One warm-up call of each path on the timed input, then the median of --reps (5) calls, the two paths alternating.  One JSON line on
stdout, and in the file --out names.
Usage: timeout -k 10 900 python3 tools/perf_allele_best.py [--snvs N] [--indels N] [--genome-bp N] [--motifs P] [--reps 5] [--out PATH]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from motifscan_amd import _lib, synth  # noqa: E402


def spread(x):
    return {"min": min(x), "median": sorted(x)[len(x) // 2], "max": max(x)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--snvs", type=int, default=1_000_000)
    ap.add_argument("--indels", type=int, default=100_000)
    ap.add_argument("--indel-len", type=int, default=50)
    ap.add_argument("--genome-bp", type=int, default=200_000_000)
    ap.add_argument("--chroms", type=int, default=8)
    ap.add_argument("--motifs", type=int, default=579)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--hbm-write-tbs", type=float, default=6.0)
    ap.add_argument("--out")
    args = ap.parse_args()
    if _lib.device_count() < 1:
        raise SystemExit("needs an MI355X: there is no CPU fallback")
    _lib.set_device(0)
    vals, widths, cutoffs = synth.load_motif_set(args.motifs)
    P = int(len(widths))
    chrom_bp = args.genome_bp // args.chroms
    bases, offsets = synth.make_regions(args.chroms, chrom_bp, seed=11, frac_n=0.002)
    names = [f"chr{i + 1}" for i in range(args.chroms)]
    genome = _lib.ResidentGenome({n: bases[offsets[i]:offsets[i + 1]] for i, n in enumerate(names)})
    del bases
    pw = _lib.PwmSet(vals, widths, cutoffs)
    rng = np.random.default_rng(17)

    # ---- the substitutions
    V = args.snvs
    s_chrom = rng.integers(0, args.chroms, V).astype(np.int32)
    s_pos = rng.integers(0, chrom_bp, V).astype(np.int64)
    s_alt = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, V)].tobytes()
    s_alts = [s_alt[i:i + 1] for i in range(V)]
    s_len = np.ones(V, dtype=np.int32)

    def dense(chrom, pos, ref_len, alts):
        res = _lib.scan_alleles_best(pw, genome, chrom, pos, ref_len, alts)
        ms = res.device_ms()
        res.close()
        return ms, None

    def sparse_snv():
        res = _lib.scan_variants(pw, genome, s_chrom, s_pos, s_alt)
        out = res.device_ms(), res.n_sites
        res.close()
        return out

    def timed(a, b, reps):
        ta, tb, extra = [], [], None
        a(), b()                                                            # warm-up: code objects, the PWM tables, the pools
        for _ in range(reps):
            ta.append(a()[0])
            ms, extra = b()
            tb.append(ms)
        return ta, tb, extra

    d_snv, y_snv, n_snv = timed(lambda: dense(s_chrom, s_pos, s_len, s_alts), sparse_snv, args.reps)

    # ---- the indels: half insertions, half deletions, 1 .. indel_len bases
    I = args.indels
    i_chrom = rng.integers(0, args.chroms, I).astype(np.int32)
    i_pos = rng.integers(0, chrom_bp - args.indel_len, I).astype(np.int64)
    length, is_ins = rng.integers(1, args.indel_len + 1, I), rng.random(I) < 0.5
    i_len = np.where(is_ins, 0, length).astype(np.int32)
    a_len = np.where(is_ins, length, 0)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, int(a_len.sum()))].tobytes()
    aoff = np.concatenate([[0], np.cumsum(a_len)])
    i_alts = [letters[aoff[v]:aoff[v + 1]] for v in range(I)]

    def sparse_indel():
        res = _lib.scan_alleles(pw, genome, i_chrom, i_pos, i_len, i_alts)
        out = res.device_ms(), res.n_sites
        res.close()
        return out

    d_ind, y_ind, n_ind = ([], [], 0) if I == 0 else timed(lambda: dense(i_chrom, i_pos, i_len, i_alts), sparse_indel, args.reps)

    def block(n_var, d, y, records):
        out_bytes = 26 * P * n_var
        floor_ms = out_bytes / (args.hbm_write_tbs * 1e12) * 1e3
        dm, ym = spread(d)["median"], spread(y)["median"]
        return {"variants": n_var, "cells": P * n_var, "dense_device_ms": spread(d), "yardstick_device_ms": spread(y), "yardstick_records": int(records),
                "out_bytes": out_bytes, "out_floor_ms": floor_ms, "ratio_to_yardstick": dm / ym, "ratio_to_yardstick_plus_floor": dm / (ym + floor_ms),
                "dense_cells_per_s": P * n_var / (dm * 1e-3), "calls": args.reps}

    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    except OSError:
        commit = None
    out = {"tool": "perf_allele_best", "device": _lib.device_name(), "commit": commit, "motifs": P, "genome_bp": int(offsets[-1]), "p_value": "1e-4",
           "hbm_write_tbs": args.hbm_write_tbs, "dims": _lib.allelebest_dims(),
           "snv": block(V, d_snv, y_snv, n_snv), "indel": None if I == 0 else block(I, d_ind, y_ind, n_ind)}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    genome.close()
    pw.close()


if __name__ == "__main__":
    main()
