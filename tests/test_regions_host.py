"""
Gene annotations and region utilities, the host side (no device): the parser and Genes against the reference tests' literal answers,
overlap_with, the replay of Python's randint / choice from raw generator words (ms_control_regions_replay_host + its driver) against
the standard library itself, generate_control_regions(genes=None) against the goldens of the real reference
(tests/golden/ref_regions.npz, make_golden_regions.py), and the errors with the generator state the reference leaves.
"""
import ctypes
import hashlib
import os
import random

import numpy as np
import pytest

from motifscan_amd import _lib, annotation, regions
from motifscan_amd.regions import GenomicRegion

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOY = os.path.join(ROOT, "tests", "golden", "ref_gene_annotation.txt")


@pytest.fixture(scope="module")
def gold():
    d = np.load(os.path.join(ROOT, "tests", "golden", "ref_regions.npz"))
    return {k: d[k] for k in d.files}


def digest():
    return hashlib.sha256(repr(random.getstate()).encode()).hexdigest()


def gold_regions(gold):
    chroms = [str(c) for c in gold["reg_chroms"]]
    regs = [GenomicRegion(chroms[c], s, e) for c, s, e in zip(gold["reg_chrom"].tolist(), gold["reg_start"].tolist(), gold["reg_end"].tolist())]
    return chroms, regs, {c: int(s) for c, s in zip(chroms, gold["chrom_size"])}


# ---------------------------------------------------------------- annotation: the literals of the reference's test_genome_annotation.py

def test_gene():
    gene = annotation.Gene(chrom="chr1", tss=10000, strand="+", name="gene1")
    assert (gene.chrom, gene.tss, gene.strand, gene.name) == ("chr1", 10000, "+", "gene1")
    assert gene.promoter(upstream=4000, downstream=2000) == [6000, 12000]
    assert annotation.Gene(chrom="chr1", tss=10000, strand="-", name="gene2").promoter(upstream=4000, downstream=2000) == [8000, 14000]
    with pytest.raises(ValueError):
        annotation.Gene(chrom="chr1", tss=10000, strand=".", name="bad")


def test_parser_and_genes(tmp_path):
    parser = annotation.RefGeneTxtParser(TOY)
    assert parser.path == TOY
    got = [(g.chrom, g.tss, g.strand, g.name) for g in parser.parse()]
    assert got == [("chr1", 11868, "+", "NR_148357"), ("chr1", 11873, "+", "NR_046018"), ("chr22", 24666798, "+", "NM_015330"),
                   ("chr1", 17436, "-", "NR_106918"), ("chr1", 17436, "-", "NR_107062")]
    for genes in (annotation.Genes(TOY), annotation.read_gene_annotation(TOY)):
        assert genes.path == TOY and len(genes) == 5
        assert len(genes.fetch("chr1")) == 4 and genes.fetch("chrX") == []
        assert [g.tss for g in genes.fetch("chr1")] == [11868, 11873, 17436, 17436]          # file order
        assert genes.chrom_names == ["chr1", "chr22"]                                       # first appearance
    bad = tmp_path / "bad.txt"
    bad.write_text(open(TOY).read().replace("\tchr22\t+\t", "\tchr22\t.\t"))
    with pytest.raises(ValueError, match="Invalid strand"):
        list(annotation.RefGeneTxtParser(str(bad)).parse())


def test_genes_from_arrays_keeps_file_order_per_chromosome():
    g = annotation.Genes.from_arrays(["b", "a", "b", "a", "b"], [5, 4, 3, 2, 1], ["+", "-", "-", "+", "+"])
    assert g.chrom_names == ["b", "a"] and g.chrom_offsets.tolist() == [0, 3, 5]
    assert g.tss.tolist() == [5, 3, 1, 4, 2] and g.strand.tolist() == [1, 2, 1, 2, 1]
    assert [(x.tss, x.strand) for x in g.fetch("a")] == [(4, "-"), (2, "+")]
    with pytest.raises(ValueError):
        annotation.Genes.from_arrays(["a"], [1], ["."])


def test_overlap_with():
    assert not regions.overlap_with([], 1, 100)
    intervals = [[1, 5], [3, 8], [10, 12]]
    assert regions.overlap_with(intervals, 1, 3)
    assert regions.overlap_with(intervals, 3, 6)
    assert not regions.overlap_with(intervals, 0, 1)
    assert not regions.overlap_with(intervals, 8, 10)
    assert not regions.overlap_with(intervals, 15, 20)


def test_region_classes():
    with pytest.raises(ValueError):
        GenomicRegion("chr1", 10, 10)
    r = GenomicRegion("chr1", 10, 21)
    assert r.summit == 15 and r.score is None
    regs = [GenomicRegion("b", 1, 5), GenomicRegion("a", 2, 9, summit=3), GenomicRegion("b", 7, 8)]
    arr = regions.RegionArray.from_regions(regs)
    assert len(arr) == 3 and arr.chroms == ["b", "a"] and arr.chrom_idx.tolist() == [0, 1, 0]
    assert arr == regs and arr == list(arr) and not arr == regs[:2] and not arr == [regs[0], regs[2], regs[1]]
    assert (arr[1].chrom, arr[1].start, arr[1].end, arr[1].summit) == ("a", 2, 9, 3)
    assert arr[1:] == regs[1:]


# ---------------------------------------------------------------- the replay against the standard library

def stdlib_control_starts(n_random, size, length, lo, hi, dist, found, tss, strand):
    """generate_control_regions' loop with the standard library's own randint / choice; `found` False = the reference's None."""
    starts, attempts = [], []
    for i in range(len(length)):
        tried, kept = 0, 0
        if lo is None:
            for _ in range(n_random):
                starts.append(random.randint(0, size[i] - length[i]))
                tried += 1
        elif hi[i] > lo[i]:
            d = dist[i] if found[i] else None
            while kept < n_random:
                if d is None:
                    d = random.randint(10000, 100000)
                g = random.choice(range(lo[i], hi[i]))
                tried += 1
                s = tss[g] + d if strand[g] == 1 else tss[g] - d
                if s >= 0 and s + length[i] <= size[i]:
                    starts.append(s)
                    kept += 1
        attempts.append(tried)
    return starts, attempts


def replay_case(seed):
    rng = np.random.default_rng(seed)
    n_genes, n = 300, 400
    tss = rng.integers(0, 300000, n_genes)
    tss[0] = 150000                                               # the one-gene ranges' gene: every drawn distance fits
    strand = rng.integers(1, 3, n_genes).astype(np.int8)
    size = np.full(n, 350000)
    length = rng.integers(1, 600, n)
    dist, found = rng.integers(-9999, 10000, n), rng.random(n) < 0.6
    lo, hi = np.zeros(n, dtype=np.int64), np.full(n, n_genes, dtype=np.int64)
    hi[::7] = 1                                                   # choice over one gene: _randbelow(1) consumes words
    lo[3::11], hi[3::11] = 5, 5                                   # no genes: skipped
    dist[::7], found[::7] = 0, False
    return size, length, lo, hi, dist, found, tss, strand


@pytest.mark.parametrize("n_random", [1, 3])
def test_replay_with_genes_equals_the_standard_library(n_random):
    size, length, lo, hi, dist, found, tss, strand = replay_case(5)
    random.seed(5)
    want, want_att = stdlib_control_starts(n_random, size.tolist(), length.tolist(), lo.tolist(), hi.tolist(), dist.tolist(), found.tolist(),
                                           tss.tolist(), strand.tolist())
    want_state = random.getstate()
    assert max(want_att) > n_random                                # starts were rejected
    random.seed(5)
    got, att = regions._replay_control_starts(size, length, n_random, 10 ** 6, lambda i: "x", (lo, hi, dist, found, tss, strand))
    assert got[hi > lo].ravel().tolist() == want and att.tolist() == want_att
    assert random.getstate() == want_state


@pytest.mark.parametrize("chunk", [None, 41])
def test_replay_widths_around_a_power_of_two_and_seed_none(chunk, monkeypatch):
    # randint widths 2^17 - 1, 2^17, 2^17 + 1, 1 and 248 955 923; random_seed=None continues from a state set earlier
    length = np.array([300, 300, 300, 300, 500] * 40, dtype=np.int64)
    size = np.array([300 + 2 ** 17 - 2, 300 + 2 ** 17 - 1, 300 + 2 ** 17, 300, 248956422] * 40, dtype=np.int64)
    chroms = [f"c{i % 5}" for i in range(200)]
    regs = [GenomicRegion(c, 10, 10 + int(n)) for c, n in zip(chroms, length)]
    chrom_size = {f"c{i}": int(size[i]) for i in range(5)}
    random.seed(77)
    random.random()
    state = random.getstate()
    want, _ = stdlib_control_starts(5, size.tolist(), length.tolist(), None, None, None, None, None, None)
    want_state = random.getstate()
    random.setstate(state)
    if chunk is not None:                                          # the driver gets 41 words at a time: it resumes inside regions
        monkeypatch.setattr(regions, "_CHUNK_WORDS", chunk)
    stops = spy_on_replay(monkeypatch)
    got = regions.generate_control_regions(5, regs, chrom_size, random_seed=None)
    assert (len(stops) > 20 and all(nd > 0 for _, nd in stops[:-1])) if chunk else len(stops) == 1
    assert got.start.tolist() == want and (got.end - got.start).tolist() == np.repeat(length, 5).tolist()
    assert [r.chrom for r in got] == [c for c in chroms for _ in range(5)]
    assert random.getstate() == want_state


def spy_on_replay(monkeypatch):
    """Records (stop, n_done) of every ms_control_regions_replay_host call the driver makes."""
    calls, real = [], _lib.control_regions_replay

    def spy(*a, **k):
        out = real(*a, **k)
        calls.append((out[4], out[3]))
        return out

    monkeypatch.setattr(_lib, "control_regions_replay", spy)
    return calls


@pytest.mark.parametrize("chunk", [37, 2])
def test_driver_resumes_when_its_words_run_out_mid_region(chunk, monkeypatch):
    """The driver itself (_replay_control_starts) with a word supply far below what the regions need: 37 words at a time it completes
    a few regions per call and restarts the one the words ran out in; 2 words at a time no region completes (a one-gene region
    with n_random = 3 needs at least 3) until the driver has doubled its supply.  Starts, attempts and the state afterwards are the
    standard library's."""
    size, length, lo, hi, dist, found, tss, strand = replay_case(13)
    random.seed(31)
    random.random()
    state = random.getstate()
    want, want_att = stdlib_control_starts(3, size.tolist(), length.tolist(), lo.tolist(), hi.tolist(), dist.tolist(), found.tolist(), tss.tolist(),
                                           strand.tolist())
    want_state = random.getstate()
    random.setstate(state)
    monkeypatch.setattr(regions, "_CHUNK_WORDS", chunk)
    stops = spy_on_replay(monkeypatch)
    got, att = regions._replay_control_starts(size, length, 3, 10 ** 6, lambda i: "x", (lo, hi, dist, found, tss, strand))
    assert got[hi > lo].ravel().tolist() == want and att.tolist() == want_att
    assert random.getstate() == want_state
    out_of_words = [nd for stop, nd in stops if stop == _lib.MS_REPLAY_WORDS]
    assert len(out_of_words) > 20 and stops[-1][0] == _lib.MS_REPLAY_DONE
    if chunk == 2:
        assert out_of_words.count(0) > 20                          # calls that completed nothing: the supply was doubled
    else:
        assert 0 < min(out_of_words) and max(out_of_words) < len(length) // 4


def test_replay_resumes_when_the_words_run_out_mid_region():
    size, length, lo, hi, dist, found, tss, strand = replay_case(9)
    random.seed(21)
    state = random.getstate()
    want, want_att = stdlib_control_starts(3, size.tolist(), length.tolist(), lo.tolist(), hi.tolist(), dist.tolist(), found.tolist(), tss.tolist(),
                                           strand.tolist())
    random.setstate(state)
    n_words = 4 * sum(want_att) + 4 * len(length)
    words = np.frombuffer(random.getrandbits(32 * n_words).to_bytes(4 * n_words, "little"), dtype="<u4").astype(np.uint32)
    done, pos, got, att, calls = 0, 0, [], [], 0
    while done < len(length):                                     # 37 words at a time: most calls end inside a region
        sl = slice(done, len(length))
        s, used, a, nd, stop, stop_words = _lib.control_regions_replay(words[pos:pos + 37], size[sl], length[sl], 3, 10 ** 6, lo[sl], hi[sl],
                                                                       dist[sl], found[sl], tss, strand)
        assert stop in (_lib.MS_REPLAY_WORDS, _lib.MS_REPLAY_DONE) and nd > 0
        assert stop_words == used[nd - 1]
        got += s[:nd][(hi[sl] > lo[sl])[:nd]].ravel().tolist()
        att += a[:nd].tolist()
        pos, done, calls = pos + stop_words, done + nd, calls + 1
    assert got == want and att == want_att and calls > 10
    random.setstate(state)
    random.getrandbits(32 * pos)
    after = random.getstate()
    random.setstate(state)
    stdlib_control_starts(3, size.tolist(), length.tolist(), lo.tolist(), hi.tolist(), dist.tolist(), found.tolist(), tss.tolist(), strand.tolist())
    assert random.getstate() == after


# ---------------------------------------------------------------- generate_control_regions(genes=None) against the real reference

@pytest.mark.parametrize("seed", [3, 11])
@pytest.mark.parametrize("n_random", [1, 5])
def test_control_regions_without_genes_equal_the_reference(gold, seed, n_random):
    chroms, regs, chrom_size = gold_regions(gold)
    random.seed(12345)
    got = regions.generate_control_regions(n_random, regs, chrom_size, random_seed=seed)
    key = f"ctl_0_{seed}_{n_random}"
    assert isinstance(got, regions.RegionArray) and len(got) == n_random * len(regs)
    assert [got.chroms[c] for c in got.chrom_idx] == [chroms[c] for c in gold[key + "_chrom"]]
    assert np.array_equal(got.start, gold[key + "_start"]) and np.array_equal(got.end, gold[key + "_end"])
    assert digest() == str(gold[key + "_digest"])
    again = regions.generate_control_regions(n_random, regions.RegionArray.from_regions(regs), chrom_size, random_seed=seed)
    assert again == got


def test_reference_test_call_without_genes():
    toy = [GenomicRegion("chr1", 9868, 13868), GenomicRegion("chr1", 50000, 51000), GenomicRegion("chr1", 17200, 17500)]
    assert len(regions.generate_control_regions(n_random=2, regions=toy, chrom_size={"chr1": 1000000})) == 6


# ---------------------------------------------------------------- errors, with the state where the reference has it

def test_missing_chromosome_size_raises_keyerror_after_the_earlier_draws():
    regs = [GenomicRegion("a", 0, 100), GenomicRegion("a", 5, 50), GenomicRegion("zz", 1, 2), GenomicRegion("a", 1, 2)]
    random.seed(4)
    for r in regs[:2]:
        for _ in range(3):
            random.randint(0, 5000 - (r.end - r.start))
    want = random.getstate()
    with pytest.raises(KeyError, match="zz"):
        regions.generate_control_regions(3, regs, {"a": 5000}, random_seed=4)
    assert random.getstate() == want


def test_region_longer_than_its_chromosome_raises_valueerror_where_randint_does():
    regs = [GenomicRegion("a", 0, 100), GenomicRegion("b", 0, 301), GenomicRegion("a", 1, 2)]
    random.seed(8)
    for _ in range(2):
        random.randint(0, 5000 - 100)
    want = random.getstate()
    with pytest.raises(ValueError, match="empty range"):
        regions.generate_control_regions(2, regs, {"a": 5000, "b": 300}, random_seed=8)
    assert random.getstate() == want


def test_width_of_two_to_the_32_raises_valueerror():
    regs = [GenomicRegion("a", 0, 100), GenomicRegion("big", 0, 100)]
    random.seed(8)
    random.randint(0, 5000 - 100)
    want = random.getstate()
    with pytest.raises(ValueError, match="2\\^32"):
        regions.generate_control_regions(1, regs, {"a": 5000, "big": 2 ** 32 + 99}, random_seed=8)
    assert random.getstate() == want
    assert len(regions.generate_control_regions(1, regs, {"a": 5000, "big": 2 ** 32 + 98}, random_seed=8)) == 2     # 2^32 - 1 starts: one word each


def test_attempt_cap_raises_runtimeerror_with_the_attempts_consumed():
    # one gene on '+' at 100 and a distance of -500: every start is negative, the reference would never end
    size, length = np.array([10000, 10000]), np.array([10, 10])
    lo, hi = np.array([0, 1]), np.array([1, 2])
    tss, strand = np.array([5000, 100]), np.array([1, 1], dtype=np.int8)
    dist, found = np.array([7, -500]), np.array([True, True])
    random.seed(2)
    for _ in range(2 + 50):
        random.choice([0])
    want = random.getstate()
    random.seed(2)
    with pytest.raises(RuntimeError, match="50 attempts"):
        regions._replay_control_starts(size, length, 2, 50, lambda i: "chr", (lo, hi, dist, found, tss, strand))
    assert random.getstate() == want


def test_genes_paths_raise_without_a_device():
    if _lib.device_count() > 0:
        pytest.skip("a device is visible: the device paths are covered by tests/test_gpu_regions.py")
    genes = annotation.Genes(TOY)
    toy = [GenomicRegion("chr1", 9868, 13868)]
    state = random.getstate()
    for call in (lambda: regions.generate_control_regions(2, toy, {"chr1": 1000000}, genes=genes),
                 lambda: regions.subset_by_location(toy, genes, "promoter"),
                 lambda: regions.dis_to_nearest_gene(toy[0], genes.fetch("chr1")),
                 lambda: regions.nearest_gene_distances(toy, genes)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    assert random.getstate() == state


def test_new_symbols_are_exported_and_validate_their_arguments():
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("ms_genes_create", "ms_genes_free", "ms_genes_nearest_tss", "ms_genes_promoter_overlap", "ms_control_regions_replay_host"):
        assert hasattr(L, name)
    with pytest.raises(ValueError):
        _lib.GeneTable([0, 2], [1, 2], [1, 3])                       # strand code 3
    with pytest.raises(ValueError):
        _lib.GeneTable([1, 2], [1, 2], [1, 2])                       # offsets must start at 0
    _lib.GeneTable([0, 0, 2], [1, 2], [1, 2]).close()
