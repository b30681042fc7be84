#!/usr/bin/env python3
"""
tests/golden/make_golden_regions.py -- goldens of the region utilities in front of `motifscan scan` (region/utils.py,
genome/annotation.py), made by running the REAL reference (MotifScan 1.3.0) where its source tree is present, the way
make_golden_build.py does.  Nothing here needs a GPU and nothing here is product code: make_golden.import_reference() puts the
reference tree on sys.path with an empty `pysam` placeholder, and its two modules are imported and called as they are.

Output:
  tests/golden/ref_gene_annotation.txt   the reference tests' five-row refGene file (data), copied
  tests/golden/ref_regions.npz
    toy_*       the reference tests' three regions on that file: dis_to_nearest_gene, subset sizes, seeded control regions
    gene_*      a synthetic annotation in FILE order (chromosome name, tss, strand per row): four chromosomes, rows shuffled over
                position and chromosome, both strands, clusters of identical TSS, TSS within 10 kb of both chromosome ends, one
                chromosome with a single gene
    reg_*       regions in mixed chromosome order: random ones, some on a chromosome without genes, starts exactly 10 000 from a TSS,
                exact ties between two TSS, starts on a TSS (d == 0), starts just upstream of one gene of a cluster
    near_*      dis_to_nearest_gene per region (dist, with found = 0 for None)
    sub_*       subset_by_location's kept indices for promoter / distal at (2000, 2000) and (4000, 500)
    ctl_*       generate_control_regions for {genes, no genes} x seeds {3, 11} x n_random {1, 5}: chromosome (index into reg_chroms),
                start, end, and the SHA-256 of repr(random.getstate()) after the call

Usage:  python3 tests/golden/make_golden_regions.py
"""
import hashlib
import os
import random
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402

SIZE = 2_000_000
SEEDS, N_RANDOM = (3, 11), (1, 5)
PAIRS = ((2000, 2000), (4000, 500))


def digest():
    return hashlib.sha256(repr(random.getstate()).encode()).hexdigest()


def make_annotation(rng):
    rows = []
    for chrom, n in (("chrA", 300), ("chrB", 250), ("chrC", 200)):
        tss = rng.integers(0, SIZE, size=n)
        tss[:6] = rng.integers(0, 10000, size=6)                        # within 10 kb of both ends
        tss[6:12] = SIZE - 1 - rng.integers(0, 10000, size=6)
        for k in range(12, 60, 4):                                       # clusters of identical TSS
            tss[k + 1:k + 4] = tss[k]
        rows += [(chrom, int(t), "+-"[int(rng.integers(0, 2))]) for t in tss]
    rows.append(("chrS", SIZE // 2, "-"))
    order = rng.permutation(len(rows))                                  # neither sorted by position nor grouped by chromosome
    return [rows[i] for i in order]


def write_refgene(path, rows):
    with open(path, "w") as fh:
        for i, (chrom, tss, strand) in enumerate(rows):
            tx = (tss, tss + 5000) if strand == "+" else (tss - 5000, tss)
            fh.write(f"585\tNM_{i:06d}\t{chrom}\t{strand}\t{tx[0]}\t{tx[1]}\t{tx[0]}\t{tx[1]}\t1\t{tx[0]},\t{tx[1]},\t0\tG{i}\tunk\tunk\t-1,\n")


def make_regions(rng, rows, GenomicRegion):
    by_chrom = {}
    for chrom, tss, _ in rows:
        by_chrom.setdefault(chrom, []).append(tss)
    regs = []

    def add(chrom, start):
        start = int(min(max(start, 0), SIZE - 1000))
        regs.append(GenomicRegion(chrom, start, start + int(rng.integers(200, 800))))

    for chrom in ("chrA", "chrB", "chrC", "chrS", "chrN"):
        for s in rng.integers(0, SIZE - 1000, size=40):
            add(chrom, s)
    for chrom in ("chrA", "chrB", "chrC"):
        t = np.array(by_chrom[chrom])
        for x in rng.choice(t, size=30):
            add(chrom, x + int(rng.integers(-12000, 12000)))             # near a gene, either side
        for x in rng.choice(t, size=10):
            add(chrom, x + 10000)                                       # |d| == cutoff: not accepted
            add(chrom, x - 10000)
            add(chrom, x)                                               # d == 0
            add(chrom, x - int(rng.integers(1, 50)))                     # just upstream: a negative d, accepted, ends the walk
        for _ in range(10):                                             # exact ties between two TSS
            a, b = rng.choice(t, size=2, replace=False)
            if abs(int(a) - int(b)) < 19000 and (int(a) + int(b)) % 2 == 0:
                add(chrom, (int(a) + int(b)) // 2)
        near = np.sort(t)
        for i in np.flatnonzero(np.diff(near) % 2 == 0)[:10]:
            if 0 < near[i + 1] - near[i] < 19000:
                add(chrom, (int(near[i]) + int(near[i + 1])) // 2)
    add("chrS", SIZE // 2 + 3)
    add("chrS", SIZE // 2 - 9999)
    order = rng.permutation(len(regs))
    return [regs[i] for i in order]


def main():
    R = make_golden.import_reference()
    from motifscan.genome.annotation import read_gene_annotation
    from motifscan.region.utils import dis_to_nearest_gene, generate_control_regions, subset_by_location
    GenomicRegion = R["GenomicRegion"]
    rng = np.random.default_rng(20261016)
    save = {"reference_version": np.array(R["version"])}

    toy_src = os.path.join(make_golden.REF, "tests", "data", "genomes", "test", "test_gene_annotation.txt")
    toy_dst = os.path.join(HERE, "ref_gene_annotation.txt")
    shutil.copyfile(toy_src, toy_dst)
    genes = read_gene_annotation(toy_dst)
    toy = [GenomicRegion("chr1", 9868, 13868), GenomicRegion("chr1", 50000, 51000), GenomicRegion("chr1", 17200, 17500)]
    near = [dis_to_nearest_gene(r, genes.fetch(r.chrom)) for r in toy]
    save["toy_near_dist"] = np.array([0 if d is None else d for d in near], dtype=np.int64)
    save["toy_near_found"] = np.array([d is not None for d in near])
    save["toy_subset_sizes"] = np.array([len(subset_by_location(toy[:1], genes, "promoter")), len(subset_by_location(toy[:1], genes, "distal")),
                                         len(subset_by_location([GenomicRegion("chr1", 9868, 10868)], genes, "promoter", upstream=1000))])
    ctl = generate_control_regions(2, toy, {"chr1": 1000000}, genes=genes, random_seed=1)
    save["toy_ctl_start"] = np.array([r.start for r in ctl], dtype=np.int64)
    save["toy_ctl_end"] = np.array([r.end for r in ctl], dtype=np.int64)
    save["toy_ctl_digest"] = np.array(digest())

    rows = make_annotation(rng)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "synth_refgene.txt")
        write_refgene(path, rows)
        genes = read_gene_annotation(path)
    save["gene_chrom"] = np.array([r[0] for r in rows])
    save["gene_tss"] = np.array([r[1] for r in rows], dtype=np.int64)
    save["gene_strand"] = np.array([r[2] for r in rows])
    regs = make_regions(rng, rows, GenomicRegion)
    chroms = sorted({r.chrom for r in regs})
    save["reg_chroms"] = np.array(chroms)
    save["reg_chrom"] = np.array([chroms.index(r.chrom) for r in regs], dtype=np.int32)
    save["reg_start"] = np.array([r.start for r in regs], dtype=np.int64)
    save["reg_end"] = np.array([r.end for r in regs], dtype=np.int64)
    save["chrom_size"] = np.array([SIZE] * len(chroms), dtype=np.int64)
    chrom_size = {c: SIZE for c in chroms}

    near = [dis_to_nearest_gene(r, genes.fetch(r.chrom)) for r in regs]
    save["near_dist"] = np.array([0 if d is None else d for d in near], dtype=np.int64)
    save["near_found"] = np.array([d is not None for d in near])
    where = {id(r): i for i, r in enumerate(regs)}
    for up, down in PAIRS:
        for loc in ("promoter", "distal"):
            kept = subset_by_location(regs, genes, loc, upstream=up, downstream=down)
            save[f"sub_{loc}_{up}_{down}"] = np.array([where[id(r)] for r in kept], dtype=np.int64)
    for with_genes in (0, 1):
        for seed in SEEDS:
            for n_random in N_RANDOM:
                random.seed(12345)                                       # overwritten by the call's own seeding
                ctl = generate_control_regions(n_random, regs, chrom_size, genes=genes if with_genes else None, random_seed=seed)
                key = f"ctl_{with_genes}_{seed}_{n_random}"
                save[key + "_chrom"] = np.array([chroms.index(r.chrom) for r in ctl], dtype=np.int32)
                save[key + "_start"] = np.array([r.start for r in ctl], dtype=np.int64)
                save[key + "_end"] = np.array([r.end for r in ctl], dtype=np.int64)
                save[key + "_digest"] = np.array(digest())
    out = os.path.join(HERE, "ref_regions.npz")
    np.savez_compressed(out, **save)
    n_none = int((~save["near_found"]).sum())
    n_neg = int((save["near_dist"] < 0).sum())
    print(f"wrote {out} ({os.path.getsize(out)} bytes): {len(rows)} genes, {len(regs)} regions, {n_none} without a gene in reach, "
          f"{n_neg} negative distances, kept {[int(save[k].size) for k in save if k.startswith('sub_')]}")


if __name__ == "__main__":
    main()
