#!/usr/bin/env python3
"""
tools/personal_genome_time.py -- times ms_genome_apply_alleles and ms_liftmap_lift (needs an MI355X) on a synthetic genome of the size
bench.py's sweep uses (--genome-mbp, default 3000, the chromosome lengths of synth.c5_chrom_lengths) and --variants (4 500 000) seeded
variants sorted by (chromosome, position): about 90 % single-base substitutions, the rest insertions and deletions of 1 .. 20 bases in equal parts.
The genome is made as random packed planes (no ASCII) and uploaded with ms_genome_create_packed.

Three steps, each in a fresh child process under its own time limit (--step-timeout seconds); the run stops at the first that fails:
  apply   ms_genome_apply_alleles: device_ms (first launch -> last kernel done) and the stage times of --reps calls after one warm-up
          on 1000 variants, the wall time of the call, the number applied
  copy    a device-to-device copy of the two planes (0.375 B per base), the floor of the splice: --reps copies timed with events
  lift    --queries (10 000 000) random ref -> alt and alt -> ref queries through ms_liftmap_lift: wall time of the call, host arrays
          in and out

One JSON line on stdout, and in the file --out names.
Usage: python3 tools/personal_genome_time.py [--genome-mbp 3000] [--variants N] [--queries N] [--reps 3] [--out profiles/personal_genome_time.json]
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


def spread(x):
    return {"min": min(x), "median": sorted(x)[len(x) // 2], "max": max(x)}


def make_genome(_lib, lens):
    from motifscan_amd import genome as _genome
    n = int(lens.sum())
    units = (n + 31) // 32
    rng = np.random.default_rng(17)
    codes = rng.integers(0, 1 << 32, 2 * units, dtype=np.uint32)
    nmask = np.zeros(units, dtype=np.uint32)
    if n % 32:                                                   # nothing may be set past the last base
        valid = n % 32
        word = (int(codes[-1]) << 32) | int(codes[-2])
        word &= (1 << (2 * valid)) - 1
        codes[-2], codes[-1] = word & 0xFFFFFFFF, word >> 32
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    names = [f"chr{i + 1}" for i in range(len(lens))]
    return _lib.ResidentGenome.from_packed(_genome.PackedGenome(names, offsets, codes, nmask))


def make_variants(lens, V):
    rng = np.random.default_rng(19)
    n = int(lens.sum())
    g = np.sort(rng.integers(0, n - 64, V))
    offsets = np.concatenate([[0], np.cumsum(lens)])
    chrom = (np.searchsorted(offsets, g, side="right") - 1).astype(np.int32)
    pos = g - offsets[chrom]
    kind, length = rng.random(V), rng.integers(1, 21, V)
    ref_len = np.where(kind < 0.9, 1, np.where(kind < 0.95, 0, length)).astype(np.int32)
    alt_len = np.where(kind < 0.9, 1, np.where(kind < 0.95, length, 0))
    ref_len = np.minimum(ref_len, lens[chrom] - pos).astype(np.int32)       # (a deletion at the very end of a chromosome is cut short)
    alt_len = np.where(ref_len + alt_len == 0, 1, alt_len)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, int(alt_len.sum()))].tobytes()
    aoff = np.concatenate([[0], np.cumsum(alt_len)])
    alts = [letters[aoff[v]:aoff[v + 1]] for v in range(V)]
    mix = {"substitutions": int((kind < 0.9).sum()), "insertions": int(((kind >= 0.9) & (kind < 0.95)).sum()), "deletions": int((kind >= 0.95).sum())}
    return chrom, pos.astype(np.int64), ref_len, alts, mix


def step_apply(args, lens):
    from motifscan_amd import _lib
    _lib.set_device(0)
    genome = make_genome(_lib, lens)
    chrom, pos, ref_len, alts, mix = make_variants(lens, args.variants)
    out, lm = _lib.apply_alleles(genome, chrom[:1000], pos[:1000], ref_len[:1000], alts[:1000])          # warm-up: code objects, the pools
    out.close()
    lm.close()
    dev, wall, stages, applied, alt_bp = [], [], [], 0, 0
    for _ in range(args.reps):
        t = time.perf_counter()
        out, lm = _lib.apply_alleles(genome, chrom, pos, ref_len, alts)
        wall.append(1e3 * (time.perf_counter() - t))
        dev.append(lm.device_ms())
        stages.append(lm.stage_ms())
        applied, alt_bp = lm.n_applied, int(lm.alt_sizes.sum())
        out.close()
        lm.close()
    best = stages[int(np.argmin(dev))]
    return {"device": _lib.device_name(), "variants": args.variants, "mix": mix, "applied": applied, "genome_bp": int(lens.sum()), "personal_bp": alt_bp,
            "device_ms": spread(dev), "wall_ms": spread(wall), "stage_ms_of_fastest_call": best, "calls": args.reps}


def step_copy(args, lens):
    import torch
    n = int(lens.sum())
    nbytes = ((n + 31) // 32) * 12                               # code plane 8 bytes + mask plane 4 bytes per 32 bases
    src = torch.randint(0, 255, (nbytes,), dtype=torch.uint8, device="cuda:0")
    dst = torch.empty_like(src)
    dst.copy_(src)
    torch.cuda.synchronize()
    ms = []
    for _ in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        dst.copy_(src)
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return {"plane_bytes": nbytes, "d2d_copy_ms": spread(ms), "calls": args.reps}


def step_lift(args, lens):
    from motifscan_amd import _lib
    _lib.set_device(0)
    genome = make_genome(_lib, lens)
    chrom, pos, ref_len, alts, _ = make_variants(lens, args.variants)
    out, lm = _lib.apply_alleles(genome, chrom, pos, ref_len, alts)
    rng = np.random.default_rng(23)
    res = {"queries": args.queries}
    for name, lift, sizes in (("ref_to_alt", lm.to_alt, lm.ref_sizes), ("alt_to_ref", lm.to_ref, lm.alt_sizes)):
        qc = rng.integers(0, len(lens), args.queries).astype(np.int32)
        qp = (rng.random(args.queries) * (sizes[qc] + 1)).astype(np.int64)
        lift(qc[:1000], qp[:1000])
        ms = []
        for _ in range(args.reps):
            t = time.perf_counter()
            got, inside = lift(qc, qp)
            ms.append(1e3 * (time.perf_counter() - t))
        res[name] = {"wall_ms": spread(ms), "inside": int(inside.sum())}
    out.close()
    lm.close()
    genome.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome-mbp", type=int, default=3000)
    ap.add_argument("--variants", type=int, default=4_500_000)
    ap.add_argument("--queries", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--step", choices=("apply", "copy", "lift"))
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--out")
    args = ap.parse_args()
    from motifscan_amd import synth
    lens = synth.c5_chrom_lengths(args.genome_mbp * 1_000_000)
    if args.step:                                                # a child: one step, its result as the last line
        print(json.dumps({"apply": step_apply, "copy": step_copy, "lift": step_lift}[args.step](args, lens)))
        return
    out = {"tool": "personal_genome_time"}
    try:
        out["commit"] = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or None
    except OSError:
        out["commit"] = None
    for step in ("apply", "copy", "lift"):                       # a fresh process per step, each under its own limit; nothing follows a failure
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--genome-mbp", str(args.genome_mbp), "--variants", str(args.variants),
               "--queries", str(args.queries), "--reps", str(args.reps)]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_timeout)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"step {step} did not end within {args.step_timeout} s")
        if p.returncode != 0:
            sys.stderr.write(p.stderr[-4000:])
            raise SystemExit(f"step {step} failed with status {p.returncode}")
        out[step] = json.loads(p.stdout.strip().splitlines()[-1])
    out["apply_over_copy"] = out["apply"]["device_ms"]["median"] / out["copy"]["d2d_copy_ms"]["median"]
    out["splice_over_copy"] = out["apply"]["stage_ms_of_fastest_call"]["splice"] / out["copy"]["d2d_copy_ms"]["median"]
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
