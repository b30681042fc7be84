#!/usr/bin/env python3
"""
tools/control_regions_time.py -- times the gene-annotation work in front of `motifscan scan` (needs an MI355X), at the CLI job's size:
--regions (default 10^6) input regions x 500 bp over 24 chromosomes, a --genes (default 65 000) gene annotation in shuffled file
order, n_random = 5.  One run; every figure says how many calls it is made of.

  nearest_tss_ms / promoter_overlap_ms   ms_genes_nearest_tss / ms_genes_promoter_overlap: host clock around the call (grouping or
                      nothing on the host, upload, kernel, copy back, stream synchronise), min / median / max over --reps (20) calls
  kernel_trace        one `rocprofv3 --kernel-trace --stats` run of this tool's --kernels-only mode (3 calls of each entry) in a child
                      process, the tool's LAST step on the device: the device time per call of nearest_tss_kernel and
                      promoter_overlap_kernel.  null only where no rocprofv3 is installed; a child that faults, aborts or runs into
                      its time limit ends the tool with a failure
  yardstick           with --bench-line FILE --bench-commit ID: ms_per_step of the parent commit's plain `python bench.py` on the same
                      machine, and nearest_tss_kernel's share of it (under a tenth: the direct form of the kernel is good enough)
  replay_s            the host replay of the draws alone (ms_control_regions_replay_host + its Python driver), 1 call
  generate_control_regions_s   end to end with genes (distances on the device + replay + the RegionArray), 1 call
  scanner_from_region_array_s  Scanner(resident genome, the 5 x regions RegionArray, window 0): coordinates only, 1 call
  python_loop_s_scaled         the reference's per-region Python loop (every gene of the chromosome per region, then randint / choice
                      per control region), restated here, timed on every 1000th region and multiplied by 1000

One JSON line on stdout, and in the file --out names (profiles/control_regions_time.json is such a line).
Usage: timeout -k 10 900 python3 tools/control_regions_time.py [--regions N] [--genes G] [--reps 20] [--bench-line FILE --bench-commit ID] [--out PATH]
"""
import argparse
import csv
import glob
import json
import os
import random
import signal
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from motifscan_amd import _lib, annotation, regions  # noqa: E402
from motifscan_amd.scanner import Scanner  # noqa: E402

N_CHROMS, CHROM_SIZE, LENGTH, N_RANDOM = 24, 10_000_000, 500, 5


def workload(n_regions, n_genes, seed=1):
    rng = np.random.default_rng(seed)
    names = [f"chr{i + 1}" for i in range(N_CHROMS)]
    w = rng.random(N_CHROMS) + 0.5
    gchrom = rng.choice(N_CHROMS, size=n_genes, p=w / w.sum())           # unequal chromosomes, rows in shuffled order
    genes = annotation.Genes.from_arrays([names[c] for c in gchrom], rng.integers(0, CHROM_SIZE, n_genes), rng.integers(1, 3, n_genes))
    rchrom = rng.choice(N_CHROMS, size=n_regions, p=w / w.sum()).astype(np.int32)
    start = rng.integers(0, CHROM_SIZE - LENGTH, n_regions)
    return names, genes, regions.RegionArray(names, rchrom, start, start + LENGTH)


def spread(ts):
    ts = sorted(ts)
    return {"min": 1e3 * ts[0], "median": 1e3 * ts[len(ts) // 2], "max": 1e3 * ts[-1], "calls": len(ts)}


def timed(fn, reps):
    fn()                                                                  # warm-up (uploads the tables)
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t)
    return spread(ts)


def kernel_trace(a):
    """Device time per call of the two kernels from one profiled child run.  None ONLY where no rocprofv3 is installed.  The child
    runs in a process group of its own; a time limit ends the whole group, and a child that ends with any status but 0 -- a fault,
    an abort, the time limit -- ends this tool with a failure: nothing more is started on the device after it."""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "--output-format", "csv", "--", sys.executable, os.path.abspath(__file__),
               "--kernels-only", "--regions", str(a.regions), "--genes", str(a.genes)]
        try:
            child = subprocess.Popen(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, start_new_session=True)
        except FileNotFoundError:
            return None
        try:
            rc = child.wait(timeout=300)
        except subprocess.TimeoutExpired:
            os.killpg(child.pid, signal.SIGKILL)
            child.wait()
            raise SystemExit("the profiled child run did not end within 300 s: its process group was killed; stopping here")
        if rc != 0:
            raise SystemExit(f"the profiled child run ended with status {rc}; stopping here")
        out = {}
        for path in glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                for k in ("nearest_tss_kernel", "promoter_overlap_kernel"):
                    if k in row.get("Name", ""):
                        out[k] = {"calls": int(row["Calls"]), "mean_ms": float(row["AverageNs"]) / 1e6, "min_ms": float(row["MinNs"]) / 1e6,
                                  "max_ms": float(row["MaxNs"]) / 1e6}
        if len(out) != 2:
            raise SystemExit(f"the profiled child run left no statistics of the two kernels under {tmp} (found {sorted(out)})")
        return out


def python_loop(arr, genes, sizes, step):
    """The reference's loop (region/utils.py:112-180) restated, on every step-th region."""
    fetched = {c: genes.fetch(c) for c in arr.chroms}
    random.seed(1)
    t = time.perf_counter()
    n = 0
    for r in list(arr)[::step]:
        gs = fetched[r.chrom]
        m, target = 10000, None
        for g in gs:
            d = r.start - g.tss
            if abs(d) < m:
                m, target = d, g
        dist = None if target is None else (-m if target.strand == "-" else m)
        k = 0
        while k < N_RANDOM:
            if dist is None:
                dist = random.randint(10000, 100000)
            g = random.choice(gs)
            s = g.tss + dist if g.strand == "+" else g.tss - dist
            if s >= 0 and s + LENGTH <= sizes[r.chrom]:
                k += 1
        n += 1
    return time.perf_counter() - t, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=1_000_000)
    ap.add_argument("--genes", type=int, default=65_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--kernels-only", action="store_true", help="3 calls of each device entry and nothing else (the profiled child)")
    ap.add_argument("--bench-line", default=None, help="file holding the JSON line of the parent commit's plain `python bench.py` on this machine")
    ap.add_argument("--bench-commit", default=None, help="the commit that bench line was made from")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    if _lib.device_count() < 1:
        raise SystemExit("needs an MI355X")
    _lib.set_device(0)
    names, genes, arr = workload(a.regions, a.genes)
    table = genes.table()
    gidx = regions._gene_chrom_idx(arr, genes)
    if a.kernels_only:
        for _ in range(3):
            table.nearest_tss(gidx, arr.start, 10000)
            table.promoter_overlap(gidx, arr.start, arr.end, 2000, 2000)
        return
    sizes = {c: CHROM_SIZE for c in names}
    out = {"tool": "control_regions_time", "device": _lib.device_name(), "runs": 1, "n_regions": a.regions, "n_genes": a.genes,
           "n_chroms": N_CHROMS, "region_length": LENGTH, "n_random": N_RANDOM,
           "genes_per_chrom": {"min": int(np.diff(genes.chrom_offsets).min()), "max": int(np.diff(genes.chrom_offsets).max())}}
    out["nearest_tss_ms"] = timed(lambda: table.nearest_tss(gidx, arr.start, 10000), a.reps)
    out["promoter_overlap_ms"] = timed(lambda: table.promoter_overlap(gidx, arr.start, arr.end, 2000, 2000), a.reps)
    dist, found = table.nearest_tss(gidx, arr.start, 10000)
    out["found_fraction"] = float(found.mean())
    out["region_gene_pairs"] = int(np.diff(genes.chrom_offsets)[gidx].sum())
    off = genes.chrom_offsets
    size = np.full(len(arr), CHROM_SIZE, dtype=np.int64)
    random.seed(1)
    t = time.perf_counter()
    _, attempts = regions._replay_control_starts(size, arr.end - arr.start, N_RANDOM, 10 ** 6, lambda i: "", (off[gidx], off[gidx + 1], dist, found, genes.tss, genes.strand))
    out["replay_s"] = time.perf_counter() - t
    out["replay_draws"] = int(attempts.sum())
    t = time.perf_counter()
    ctl = regions.generate_control_regions(N_RANDOM, arr, sizes, genes=genes, random_seed=1)
    out["generate_control_regions_s"] = time.perf_counter() - t
    out["n_control_regions"] = len(ctl)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from build_motif_time import synthetic_packed
    pg = synthetic_packed(N_CHROMS * (CHROM_SIZE + 64), 5)
    pg.chrom_sizes = dict(pg.chrom_sizes)
    rg = pg.to_resident()
    small = min(pg.chrom_sizes.values())
    inside = regions.RegionArray(ctl.chroms, ctl.chrom_idx, np.minimum(ctl.start, small - LENGTH), np.minimum(ctl.start, small - LENGTH) + LENGTH)
    t = time.perf_counter()
    sc = Scanner(rg, inside, window_size=0)
    out["scanner_from_region_array_s"] = time.perf_counter() - t
    out["scanner_regions"] = len(sc.seq_starts)
    rg.close()
    table.close()
    # the last step that uses the device: the profiled child, after this process has closed everything it held there
    out["kernel_trace"] = kernel_trace(a)
    if a.bench_line:
        # the yardstick for nearest_tss_kernel: ms_per_step of a plain `python bench.py` of the PARENT commit (the tree without this
        # feature), taken on the same machine; a tenth of it is the bar below which the direct form of the kernel is kept
        with open(a.bench_line) as fh:
            bench = json.loads([ln for ln in fh if ln.startswith("{")][-1])
        out["yardstick"] = {"what": "ms_per_step of the parent commit's plain bench run, same machine", "commit": a.bench_commit,
                            "command": "python bench.py", "steps": bench["steps"], "warmup": bench["warmup"], "ms_per_step": bench["ms_per_step"]}
        if out["kernel_trace"]:
            out["nearest_tss_kernel_share_of_step"] = out["kernel_trace"]["nearest_tss_kernel"]["mean_ms"] / bench["ms_per_step"]
    step = 1000
    secs, n = python_loop(arr, genes, sizes, step)
    out["python_loop_sample"] = {"regions": n, "seconds": secs, "every": step}
    out["python_loop_s_scaled"] = secs * step
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
