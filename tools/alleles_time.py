#!/usr/bin/env python3
"""
tools/alleles_time.py -- times ms_scan_alleles (needs an MI355X): --variants (default 10^6) seeded alleles -- 80 % single-base
substitutions, 10 % insertions and 10 % deletions of 1 .. 20 bases -- x the first --motifs (579) motifs of the benchmark set at p = 1e-4,
on a synthetic genome of --chroms (8) chromosomes of --chrom-bp (4 000 000) bases.  One process; a warm-up call of each path on 1000
variants comes first.

  allele_scan    _lib.scan_alleles + the copy of every record array to the host, --reps (3) calls: wall_ms = host clock around the call
                 (the flattening of the alt strings included), device_ms = ms_allelescan_device_ms (upload -> last kernel done)
  detour         the route without it: per haplotype one flank string per variant built in Python ([x - Wmax + 1, x + len + Wmax - 1) of
                 that haplotype), SeqSet.from_strings, ms_scan, the hits outside the affected windows thrown away, the two hit lists
                 sorted into the record order on the host -- 1 call, its stages apiece
  same_records   the two paths give the same (motif, variant, allele, start, strand, score) records
  snv_subset     the single-base substitutions alone through ms_scan_alleles and through ms_scan_variants: device_ms of each over --reps
                 calls (informational: which kernel is faster on the input both take)

One JSON line on stdout, and in the file --out names.
Usage: timeout -k 10 900 python3 tools/alleles_time.py [--variants N] [--motifs P] [--reps 3] [--out PATH]
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


def keys_of(motif, variant, allele, start, strand, V, span):
    return ((((motif.astype(np.int64) * V + variant) * 2 + allele) * span + start) * 2) + (strand.astype(np.int64) - 1)


def detour(pw, widths, chroms, names, chrom_idx, pos, ref_len, alts, span):
    """(sorted record keys, their scores, stage times in s) by the route open without ms_scan_alleles."""
    V, wmax = len(pos), int(widths.max())
    t0 = time.perf_counter()
    los = np.maximum(pos - wmax + 1, 0)
    seqs = ([], [])
    for v in range(V):
        seq, x, lo, r = chroms[names[chrom_idx[v]]], int(pos[v]), int(los[v]), int(ref_len[v])
        tail = seq[x + r:x + r + wmax - 1]
        seqs[0].append(seq[lo:x + r] + tail)
        seqs[1].append(seq[lo:x] + alts[v] + tail)
    t1 = time.perf_counter()
    lengths = (ref_len.astype(np.int64), np.array([len(a) for a in alts], dtype=np.int64))
    keys, scores, t_pack, t_scan, t_join = [], [], 0.0, 0.0, 0.0
    for allele in (0, 1):
        a = time.perf_counter()
        sq = _lib.SeqSet.from_strings(seqs[allele])
        b = time.perf_counter()
        r = _lib.scan(pw, sq, 3)
        h = r.hits(copy=False)
        c = time.perf_counter()
        v = h["seq_idx"]
        start, x = h["pos"] + los[v], pos[v]
        affected = (start >= x - widths[h["motif"]] + 1) & (start <= x + lengths[allele][v] - 1)
        keys.append(keys_of(h["motif"][affected], v[affected], allele, start[affected], h["strand"][affected], V, span))
        scores.append(np.array(h["score"][affected]))
        del h
        r.close()
        sq.close()
        d = time.perf_counter()
        t_pack, t_scan, t_join = t_pack + b - a, t_scan + c - b, t_join + d - c
    a = time.perf_counter()
    keys, scores = np.concatenate(keys), np.concatenate(scores)
    order = np.argsort(keys, kind="stable")
    keys, scores = keys[order], scores[order]
    t_join += time.perf_counter() - a
    return keys, scores, {"flank_strings_s": t1 - t0, "from_strings_s": t_pack, "two_scans_s": t_scan, "filter_and_join_s": t_join,
                          "total_s": time.perf_counter() - t0}


def spread(x):
    return {"min": min(x), "median": sorted(x)[len(x) // 2], "max": max(x)}


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
    rng = np.random.default_rng(13)
    V = args.variants
    chrom_idx = rng.integers(0, args.chroms, V).astype(np.int32)
    kind, length = rng.random(V), rng.integers(1, 21, V)
    ref_len = np.where(kind < 0.8, 1, np.where(kind < 0.9, 0, length)).astype(np.int32)
    alt_len = np.where(kind < 0.8, 1, np.where(kind < 0.9, length, 0))
    pos = rng.integers(0, args.chrom_bp - 20, V).astype(np.int64)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, int(alt_len.sum()))].tobytes()
    aoff = np.concatenate([[0], np.cumsum(alt_len)])
    alts = [letters[aoff[v]:aoff[v + 1]] for v in range(V)]
    span = 1 << (int(args.chrom_bp) + 64).bit_length()
    genome = _lib.ResidentGenome(chroms)
    pw = _lib.PwmSet(vals, widths, cutoffs)

    def run(sel):
        res = _lib.scan_alleles(pw, genome, chrom_idx[sel], pos[sel], ref_len[sel], alts[sel] if isinstance(sel, slice) else [alts[i] for i in sel])
        s, dev = res.sites(), res.device_ms()
        res.close()
        return s, dev

    def run_snv(sel, alt_bytes):
        res = _lib.scan_variants(pw, genome, chrom_idx[sel], pos[sel], alt_bytes)
        n, dev = res.n_sites, res.device_ms()
        res.close()
        return n, dev

    warm = slice(0, min(V, 1000))
    run(warm)                                                               # warm-up: code objects, the PWM tables, the pools
    detour(pw, widths, chroms, names, chrom_idx[warm], pos[warm], ref_len[warm], alts[warm], span)
    snv = np.flatnonzero(kind < 0.8)
    snv_alt = b"".join(alts[i] for i in snv)
    run_snv(snv[:1000], snv_alt[:1000])
    wall, dev = [], []
    for _ in range(args.reps):
        t = time.perf_counter()
        s, d = run(slice(0, V))
        wall.append(1e3 * (time.perf_counter() - t))
        dev.append(d)
    keys, scores, stages = detour(pw, widths, chroms, names, chrom_idx, pos, ref_len, alts, span)
    same = bool(np.array_equal(keys_of(s["motif"], s["variant"], s["allele"], s["start"], s["strand"], V, span), keys)
                and np.array_equal(s["score"], scores))
    records, per_allele = int(len(s["score"])), np.bincount(s["allele"], minlength=2).tolist()
    del s, keys, scores
    dev_al, dev_snv, n_al, n_snv = [], [], 0, 0
    for _ in range(args.reps):
        sa, d = run(snv)
        n_al = int(len(sa["score"]))
        del sa
        dev_al.append(d)
        n_snv, d = run_snv(snv, snv_alt)
        dev_snv.append(d)
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    except OSError:
        commit = None
    out = {"tool": "alleles_time", "device": _lib.device_name(), "commit": commit, "variants": V, "motifs": int(len(widths)),
           "genome_bp": int(offsets[-1]), "p_value": "1e-4", "records": records, "records_per_allele": per_allele,
           "mix": {"snv": int((kind < 0.8).sum()), "insertions": int(((kind >= 0.8) & (kind < 0.9)).sum()), "deletions": int((kind >= 0.9).sum())},
           "allele_scan": {"wall_ms": spread(wall), "device_ms": spread(dev), "calls": args.reps},
           "detour": dict(stages, calls=1), "same_records": same,
           "not_slower_than_detour": bool(max(wall) <= 1e3 * stages["total_s"]),
           "snv_subset": {"variants": int(len(snv)), "allele_scan_device_ms": spread(dev_al), "allele_scan_records": n_al,
                          "variant_scan_device_ms": spread(dev_snv), "variant_scan_records": int(n_snv), "calls": args.reps}}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    genome.close()
    pw.close()
    if not same:
        raise SystemExit("the two paths disagree")
    if not out["not_slower_than_detour"]:
        raise SystemExit("ms_scan_alleles was slower end to end than the flank-string detour")


if __name__ == "__main__":
    main()
