#!/usr/bin/env python3
"""
tools/variants_time.py -- times ms_scan_variants against the detour that was the only way before it (needs an MI355X): --variants
(default 10^6) seeded single-base substitutions x the first --motifs (579) motifs of the benchmark set at p = 1e-4, on a synthetic genome
of --chroms (8) chromosomes of --chrom-bp (4 000 000) bases.  One process; a warm-up call of each path on 1000 variants comes first.

  variant_scan   _lib.scan_variants + the copy of every record array to the host, --reps (3) calls: wall_ms = host clock around the call,
                 device_ms = ms_varscan_device_ms (HIP events on the library's stream: upload of the variants -> last kernel done)
  detour         per allele one flank string [x - Wmax + 1, x + Wmax) per variant built in Python, SeqSet.from_strings, ms_scan, the hits
                 that do not cover the variant thrown away, the two hit lists joined on the host -- 1 call, its stages apiece
  same_records   the two paths give the same (motif, variant, start, strand, state) records

One JSON line on stdout, and in the file --out names.
Usage: timeout -k 10 600 python3 tools/variants_time.py [--variants N] [--motifs P] [--reps 3] [--out PATH]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from motifscan_amd import _lib, synth  # noqa: E402


def keys_of(motif, variant, start, strand, V, span):
    return ((motif.astype(np.int64) * V + variant) * span + start) * 2 + (strand.astype(np.int64) - 1)


def detour(pw, widths, chroms, names, chrom_idx, pos, alt, span):
    """(sorted record keys, states, stage times in s) by the route open without ms_scan_variants."""
    V, wmax = len(pos), int(widths.max())
    t0 = time.perf_counter()
    los = np.maximum(pos - wmax + 1, 0)
    ref_seqs, alt_seqs = [], []
    for v in range(V):
        seq, x, lo = chroms[names[chrom_idx[v]]], int(pos[v]), int(los[v])
        flank = seq[lo:x + wmax]
        ref_seqs.append(flank)
        alt_seqs.append(flank[:x - lo] + alt[v:v + 1] + flank[x - lo + 1:])
    t1 = time.perf_counter()
    found, t_pack, t_scan, t_join = [], 0.0, 0.0, 0.0
    xr = pos - los
    for seqs in (ref_seqs, alt_seqs):
        a = time.perf_counter()
        sq = _lib.SeqSet.from_strings(seqs)
        b = time.perf_counter()
        r = _lib.scan(pw, sq, 3)
        h = r.hits(copy=False)
        c = time.perf_counter()
        covers = (h["pos"] <= xr[h["seq_idx"]]) & (h["pos"] + widths[h["motif"]] > xr[h["seq_idx"]])
        found.append(keys_of(h["motif"][covers], h["seq_idx"][covers], h["pos"][covers] + los[h["seq_idx"][covers]], h["strand"][covers], V, span))
        del h
        r.close()
        sq.close()
        d = time.perf_counter()
        t_pack, t_scan, t_join = t_pack + b - a, t_scan + c - b, t_join + d - c
    a = time.perf_counter()
    keys = np.union1d(found[0], found[1])
    state = np.isin(keys, found[0]).astype(np.uint8) | (np.isin(keys, found[1]).astype(np.uint8) << 1)
    t_join += time.perf_counter() - a
    return keys, state, {"flank_strings_s": t1 - t0, "from_strings_s": t_pack, "two_scans_s": t_scan, "filter_and_join_s": t_join,
                         "total_s": time.perf_counter() - t0}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variants", type=int, default=1_000_000)
    ap.add_argument("--motifs", type=int, default=579)
    ap.add_argument("--chroms", type=int, default=8)
    ap.add_argument("--chrom-bp", type=int, default=4_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out")
    args = ap.parse_args()
    if _lib.device_count() < 1:
        raise SystemExit("needs an MI355X: there is no CPU fallback")
    _lib.set_device(0)
    vals, widths, cutoffs = synth.load_motif_set(args.motifs)
    bases, offsets = synth.make_regions(args.chroms, args.chrom_bp, seed=11, frac_n=0.002)
    raw = bases.tobytes()
    names = [f"chr{i + 1}" for i in range(args.chroms)]
    chroms = {n: raw[offsets[i]:offsets[i + 1]] for i, n in enumerate(names)}
    rng = np.random.default_rng(12)
    V = args.variants
    chrom_idx = rng.integers(0, args.chroms, V).astype(np.int32)
    pos = rng.integers(0, args.chrom_bp, V).astype(np.int64)
    alt = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, V)].tobytes()
    span = 1 << int(args.chrom_bp).bit_length()
    genome = _lib.ResidentGenome(chroms)
    pw = _lib.PwmSet(vals, widths, cutoffs)

    def run(n):
        res = _lib.scan_variants(pw, genome, chrom_idx[:n], pos[:n], alt[:n])
        s, dev = res.sites(), res.device_ms()
        res.close()
        return s, dev

    run(min(V, 1000))                                                       # warm-up: code objects, the PWM tables, the pools
    detour(pw, widths, chroms, names, chrom_idx[:1000], pos[:1000], alt[:1000], span)
    wall, dev = [], []
    for _ in range(args.reps):
        t = time.perf_counter()
        s, d = run(V)
        wall.append(1e3 * (time.perf_counter() - t))
        dev.append(d)
    keys, state, stages = detour(pw, widths, chroms, names, chrom_idx, pos, alt, span)
    same = bool(np.array_equal(keys_of(s["motif"], s["variant"], s["start"], s["strand"], V, span), keys) and np.array_equal(s["state"], state))
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    except OSError:
        commit = None
    out = {"tool": "variants_time", "device": _lib.device_name(), "commit": commit, "variants": V, "motifs": int(len(widths)),
           "genome_bp": int(offsets[-1]), "p_value": "1e-4", "records": int(len(s["state"])),
           "states": np.bincount(s["state"], minlength=4).tolist(),
           "variant_scan": {"wall_ms": {"min": min(wall), "median": sorted(wall)[len(wall) // 2], "max": max(wall)},
                            "device_ms": {"min": min(dev), "median": sorted(dev)[len(dev) // 2], "max": max(dev)}, "calls": args.reps},
           "detour": dict(stages, calls=1), "same_records": same}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    genome.close()
    pw.close()
    if not same:
        raise SystemExit("the two paths disagree")


if __name__ == "__main__":
    main()
