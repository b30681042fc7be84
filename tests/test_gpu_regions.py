"""
Gene-annotation work on the device (ms_annotation.hip): dis_to_nearest_gene, subset_by_location and generate_control_regions against
the goldens made by the real reference (tests/golden/ref_regions.npz, make_golden_regions.py), the reference tests' own assertions on
its toy annotation, a full-size check against numpy restatements written here, and the RegionArray path of Scanner.
"""
import hashlib
import os
import random

import numpy as np
import pytest

from motifscan_amd import _lib, annotation, regions, synth
from motifscan_amd.regions import GenomicRegion
from motifscan_amd.scanner import Scanner

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOY = os.path.join(ROOT, "tests", "golden", "ref_gene_annotation.txt")


@pytest.fixture(scope="module", autouse=True)
def _device():
    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible")
    _lib.set_device(0)


@pytest.fixture(scope="module")
def gold():
    d = np.load(os.path.join(ROOT, "tests", "golden", "ref_regions.npz"))
    out = {k: d[k] for k in d.files}
    out["genes"] = annotation.Genes.from_arrays([str(c) for c in out["gene_chrom"]], out["gene_tss"], out["gene_strand"])
    chroms = [str(c) for c in out["reg_chroms"]]
    out["chroms"] = chroms
    out["regs"] = [GenomicRegion(chroms[c], s, e) for c, s, e in zip(out["reg_chrom"].tolist(), out["reg_start"].tolist(), out["reg_end"].tolist())]
    out["sizes"] = {c: int(s) for c, s in zip(chroms, out["chrom_size"])}
    return out


def digest():
    return hashlib.sha256(repr(random.getstate()).encode()).hexdigest()


def test_nearest_gene_distances_equal_the_reference(gold):
    dist, found = regions.nearest_gene_distances(gold["regs"], gold["genes"])
    assert np.array_equal(found, gold["near_found"])
    assert np.array_equal(dist[found], gold["near_dist"][gold["near_found"]])
    assert (~found).sum() > 0 and (dist[found] == 0).sum() > 0 and (dist < 0).sum() > 0
    arr = regions.RegionArray.from_regions(gold["regs"])
    d2, f2 = regions.nearest_gene_distances(arr, gold["genes"])
    assert np.array_equal(d2, dist) and np.array_equal(f2, found)


def test_single_region_equals_the_batch(gold):
    dist, found = regions.nearest_gene_distances(gold["regs"], gold["genes"])
    for i in list(range(0, len(gold["regs"]), 9)):
        r = gold["regs"][i]
        one = regions.dis_to_nearest_gene(r, gold["genes"].fetch(r.chrom))
        assert one == (int(dist[i]) if found[i] else None)
        assert one is None or isinstance(one, int)


@pytest.mark.parametrize("pair", [(2000, 2000), (4000, 500)])
def test_subset_by_location_equals_the_reference(gold, pair):
    up, down = pair
    regs = gold["regs"]
    for loc in ("promoter", "distal"):
        kept = regions.subset_by_location(regs, gold["genes"], loc, upstream=up, downstream=down)
        want = gold[f"sub_{loc}_{up}_{down}"].tolist()
        assert len(kept) == len(want) and all(k is regs[i] for k, i in zip(kept, want))          # the input's own objects, input order
        arr = regions.subset_by_location(regions.RegionArray.from_regions(regs), gold["genes"], loc, upstream=up, downstream=down)
        assert isinstance(arr, regions.RegionArray) and arr == kept
    other = regions.subset_by_location(regs, gold["genes"], "anything else", upstream=up, downstream=down)        # behaves as distal
    assert [id(r) for r in other] == [id(regs[i]) for i in gold[f"sub_distal_{up}_{down}"].tolist()]


@pytest.mark.parametrize("with_genes", [0, 1])
@pytest.mark.parametrize("seed", [3, 11])
@pytest.mark.parametrize("n_random", [1, 5])
def test_control_regions_equal_the_reference(gold, with_genes, seed, n_random):
    random.seed(12345)
    got = regions.generate_control_regions(n_random, gold["regs"], gold["sizes"], genes=gold["genes"] if with_genes else None, random_seed=seed)
    key = f"ctl_{with_genes}_{seed}_{n_random}"
    assert [got.chroms[c] for c in got.chrom_idx] == [gold["chroms"][c] for c in gold[key + "_chrom"]]
    assert np.array_equal(got.start, gold[key + "_start"]) and np.array_equal(got.end, gold[key + "_end"])
    assert digest() == str(gold[key + "_digest"])


def test_reference_tests_on_the_toy_annotation(gold):
    genes = annotation.read_gene_annotation(TOY)
    toy = [GenomicRegion("chr1", 9868, 13868), GenomicRegion("chr1", 50000, 51000), GenomicRegion("chr1", 17200, 17500)]
    sizes = [len(regions.subset_by_location(toy[:1], genes, "promoter")), len(regions.subset_by_location(toy[:1], genes, "distal")),
             len(regions.subset_by_location([GenomicRegion("chr1", 9868, 10868)], genes, "promoter", upstream=1000))]
    assert sizes == [1, 0, 0] == gold["toy_subset_sizes"].tolist()
    dist, found = regions.nearest_gene_distances(toy, genes)
    assert np.array_equal(found, gold["toy_near_found"]) and np.array_equal(dist[found], gold["toy_near_dist"][gold["toy_near_found"]])
    assert len(regions.generate_control_regions(n_random=2, regions=toy, chrom_size={"chr1": 1000000}, genes=genes)) == 6
    got = regions.generate_control_regions(n_random=2, regions=toy, chrom_size={"chr1": 1000000}, genes=genes, random_seed=1)
    assert len(got) == 6 and np.array_equal(got.start, gold["toy_ctl_start"]) and np.array_equal(got.end, gold["toy_ctl_end"])
    assert digest() == str(gold["toy_ctl_digest"])
    assert len(regions.generate_control_regions(n_random=2, regions=toy, chrom_size={"chr1": 1000000})) == 6


def test_scale_against_numpy_restatements():
    """200 000 regions over 24 chromosomes against 60 000 genes in shuffled file order: every distance, flag and overlap."""
    rng = np.random.default_rng(7)
    n_chroms, n_genes, n = 24, 60000, 200000
    size = 50_000_000
    names = [f"chr{i}" for i in range(n_chroms)]
    gchrom = rng.integers(0, n_chroms, n_genes)
    tss = rng.integers(0, size, n_genes)
    tss[1::50] = tss[0::50][:len(tss[1::50])]                       # identical TSS here and there
    strand = rng.integers(1, 3, n_genes)
    genes = annotation.Genes.from_arrays([names[c] for c in gchrom], tss, strand)
    rchrom = rng.integers(0, n_chroms, n).astype(np.int32)
    near = rng.random(n) < 0.7                                      # most regions near a gene of their chromosome
    start = rng.integers(0, size, n)
    for c in range(n_chroms):
        sel = np.flatnonzero((rchrom == c) & near)
        start[sel] = rng.choice(tss[gchrom == c], size=sel.size) + rng.integers(-10001, 10002, sel.size)
    start = np.maximum(start, 0)
    end = start + rng.integers(1, 3000, n)
    arr = regions.RegionArray(names, rchrom, start, end)
    dist, found = regions.nearest_gene_distances(arr, genes)
    overlap = genes.table().promoter_overlap(regions._gene_chrom_idx(arr, genes), start, end, 3000, 1000)     # the table's own chromosome order
    want_d, want_f, want_o = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
    for c in range(n_chroms):
        sel = np.flatnonzero(rchrom == c)
        s, e = start[sel], end[sel]
        m = np.full(sel.size, 10000, dtype=np.int64)
        minus, hit, ov = np.zeros(sel.size, dtype=bool), np.zeros(sel.size, dtype=bool), np.zeros(sel.size, dtype=bool)
        lo_g, hi_g = genes.chrom_range(names[c])
        for t, sd in zip(genes.tss[lo_g:hi_g].tolist(), genes.strand[lo_g:hi_g].tolist()):       # file order
            d = s - t
            acc = np.abs(d) < m
            m = np.where(acc, d, m)
            minus = np.where(acc, sd == 2, minus)
            hit |= acc
            lo, hi = (t - 3000, t + 1000) if sd == 1 else (t - 1000, t + 3000)
            ov |= ~((e <= lo) | (s >= hi))                              # brute-force any-overlap
        want_d[sel], want_f[sel], want_o[sel] = np.where(hit, np.where(minus, -m, m), 0), hit, ov
    assert np.array_equal(found, want_f) and np.array_equal(dist, want_d)
    assert np.array_equal(overlap, want_o)
    assert 0.2 < found.mean() < 0.9 and 0.05 < overlap.mean() < 0.9


def test_region_array_through_scanner_equals_the_object_list(gold):
    vals, widths, cutoffs = synth.load_motif_set(16)
    rng = np.random.default_rng(3)
    size = 300000                                                   # chrS's one gene sits mid-chromosome: every drawn distance (<= 100 kb) fits
    chroms = {c: np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size)].tobytes().decode() for c in ("chrA", "chrB", "chrS")}
    genome = _lib.ResidentGenome(chroms, keep_host=True)
    sizes = {c: size for c in chroms}
    genes = annotation.Genes.from_arrays(["chrA"] * 40 + ["chrB"] * 40 + ["chrS"], np.concatenate([rng.integers(0, size, 80), [size // 2]]),
                                         rng.integers(1, 3, 81))
    regs = [GenomicRegion(c, s, s + 300) for c, s in zip(rng.choice(["chrA", "chrB", "chrS"], size=200), rng.integers(0, size - 1000, 200).tolist())]
    ctl = regions.generate_control_regions(3, regs, sizes, genes=genes, random_seed=5)
    assert isinstance(ctl, regions.RegionArray) and len(ctl) == 600

    class Pwm:
        def __init__(self, m, c):
            self.matrix, self.cutoffs, self.length = m, {"1e-4": c}, m.shape[1]

    off = np.concatenate([[0], np.cumsum(4 * widths)])
    pwms = [Pwm(vals[off[i]:off[i + 1]].reshape(4, -1), cutoffs[i]) for i in range(len(widths))]
    try:
        for window in (0, 200, 1000000):
            a, b = Scanner(genome, ctl, window_size=window), Scanner(genome, list(ctl), window_size=window)
            assert a.seq_starts == b.seq_starts and a.seq_ends == b.seq_ends and len(a.seq_starts) == 600
            assert np.array_equal(a.count_regions_with_sites(pwms), b.count_regions_with_sites(pwms))
            a.close()
            b.close()
    finally:
        genome.close()


def test_annotation_without_genes_and_unused_chromosome_names():
    """An empty annotation gives no control regions, as the reference's `continue` does for every region; a RegionArray that carries a
    chromosome name no region uses goes through Scanner as the list of its regions does, though the genome does not know the name."""
    empty = annotation.Genes.from_arrays([], [], [])
    regs = [GenomicRegion("chrA", 10, 300), GenomicRegion("chrB", 5, 100)]
    state = random.getstate()
    got = regions.generate_control_regions(3, regs, {"chrA": 1000, "chrB": 1000}, genes=empty)
    assert isinstance(got, regions.RegionArray) and len(got) == 0 and random.getstate() == state
    assert regions.subset_by_location(regs, empty, "promoter") == [] and regions.subset_by_location(regs, empty, "distal") == regs
    dist, found = regions.nearest_gene_distances(regs, empty)
    assert not found.any()
    genome = _lib.ResidentGenome({"chrA": "ACGT" * 100, "chrB": "TTGCA" * 50}, keep_host=True)
    try:
        arr = regions.RegionArray(["chrZ", "chrB", "chrA"], [2, 1, 2], [10, 5, 200], [300, 100, 390])
        for window in (0, 100):
            a, b = Scanner(genome, arr, window_size=window), Scanner(genome, list(arr), window_size=window)
            assert a.seq_starts == b.seq_starts and a.seq_ends == b.seq_ends and a.sequences == b.sequences
    finally:
        genome.close()
