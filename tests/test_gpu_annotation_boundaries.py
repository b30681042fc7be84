"""
ms_genes_nearest_tss and ms_genes_promoter_overlap (ms_annotation.hip) on their own boundaries, through _lib.GeneTable: gene lists on
the LDS tile's edges, region counts on the block's, blocks of which one lane, one wave or nothing stays live behind the first tile,
distances equal to the running minimum and one either side of it, the reference's freeze at a negative distance; the literal binary
search on and one base off an interval's ends, with empty and inverted regions and intervals, and the cached promoter table switched
between two extent pairs and back.  The sizes come from ms_debug_genome_dims (_lib.genome_dims).  Expected values are worked out by
hand where the case is small, else they come from fuzz_parity's restatements of the reference's walks, which
tests/test_fuzz_cases_host.py holds against plain Python loops.  Everything is exact.  tests/fuzz_parity.py --annot runs seeded cases.
Run with -m gpu.
"""
import numpy as np
import pytest

import fuzz_parity as fp
from motifscan_amd import _lib

pytestmark = pytest.mark.gpu
FWD, REV = 1, 2
# the sizes of the parametrised cases, in units of the library's constants (read when a test runs, not when the module is collected)
SIZES = {"0": lambda u: 0, "1": lambda u: 1, "63": lambda u: 63, "64": lambda u: 64, "unit-1": lambda u: u - 1, "unit": lambda u: u,
         "unit+1": lambda u: u + 1, "2units": lambda u: 2 * u, "2units+1": lambda u: 2 * u + 1}


def dims():
    return _lib.genome_dims()


def size(name, unit):
    return SIZES[name](dims()[unit])


@pytest.fixture(scope="module", autouse=True)
def _device():
    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible")
    _lib.set_device(0)


def table_of(chroms):
    """GeneTable of [(tss list, strand list)] per chromosome, with the arrays."""
    off = np.concatenate([[0], np.cumsum([len(t) for t, _ in chroms])]).astype(np.int64)
    tss = np.concatenate([np.asarray(t, dtype=np.int64) for t, _ in chroms]) if chroms else np.zeros(0, dtype=np.int64)
    strand = np.concatenate([np.asarray(s, dtype=np.int8) for _, s in chroms]) if chroms else np.zeros(0, dtype=np.int8)
    return _lib.GeneTable(off, tss, strand), off, tss, strand


def nearest(chroms, chrom, start, cutoff=10000):
    t, off, tss, strand = table_of(chroms)
    try:
        got = t.nearest_tss(chrom, start, cutoff)
    finally:
        t.close()
    want = fp.nearest_restated(off, tss, strand, np.asarray(chrom, dtype=np.int32), np.asarray(start, dtype=np.int64), cutoff, dims()["gene_tile"])
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[0], want[0]), np.flatnonzero((got[0] != want[0]) | (got[1] != want[1]))[:8]
    return got


# ------------------------------------------------------------------------------------------------ nearest_tss

def test_ties_neighbours_of_the_minimum_and_the_freeze_by_hand():
    genes = ([1000 - 100, 1000 - 100, 1000 - 101, 1000 + 99, 1000 - 98, 1000 + 98, 1000, 1000 + 1, 1000],
             [FWD, REV, FWD, REV, FWD, REV, REV, FWD, FWD])
    # start 1000: d = 100 (accepted, m = 100), 100 on the other strand (|d| == m: the first keeps it), 101 (m + 1: no), -99 (m - 1: accepted,
    # m = -99 < 0: frozen -- the closer genes behind it, d == 0 among them, are ignored); distance of a '-' gene is negated: 99
    dist, found = nearest([genes], [0, 0, 0, 0, 0, 1, -1], [1000, 1099, 900, 1000 + 20000, 899 - 10000, 1000, 1000])
    assert found.tolist() == [True, True, True, False, False, False, False]
    # start 1099: d = 199, 199 (tie), 200, 0 at gene 3 (accepted, m = 0, '-': distance -0 = 0) -- frozen at zero
    # start 900: d = 0 at gene 0: found, distance 0
    # start 21000: every |d| >= 10000; start 899 - 10000: d = -10001, -10001, -10000 (not below the cutoff), ...: nothing
    assert dist.tolist() == [99, 0, 0, 0, 0, 0, 0]
    dist, found = nearest([genes], [0, 0], [900 - 9999, 899 - 10000])     # d = -9999 at gene 0 ('+'): accepted, frozen
    assert found.tolist() == [True, False] and dist.tolist() == [-9999, 0]


@pytest.mark.parametrize("n_genes", ["1", "unit-1", "unit", "unit+1", "2units", "2units+1"])
def test_gene_lists_on_the_tile_edges_and_region_counts_on_the_block_edges(n_genes):
    n_genes, BLOCK = size(n_genes, "gene_tile"), dims()["near_threads"]
    rng = np.random.default_rng(n_genes)
    tss = rng.integers(-50_000, 3_000_000, size=n_genes)
    tss[1::7] = tss[0::7][:len(tss[1::7])]                                  # equal TSS, strands as they fall
    chroms = [([], []), (tss, rng.integers(1, 3, size=n_genes)), ([5], [REV])]
    for n in (1, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK + 1):
        start = tss[rng.integers(0, n_genes, size=n)] + np.where(rng.random(n) < 0.1, 0, rng.integers(-10001, 10002, size=n))
        chrom = np.where(rng.random(n) < 0.9, 1, rng.integers(-1, 4, size=n))
        dist, found = nearest(chroms, chrom, start)
        assert not found[(chrom != 1) & (chrom != 2)].any() and (n < BLOCK or 0.3 < found.mean() <= 1)
        # the only gene within the cutoff is the last of the last tile
        far = int(tss.max()) + 100_000
        genes = (np.concatenate([tss[:-1], [far + 3]]), chroms[1][1])
        got = nearest([genes], np.zeros(n, dtype=np.int32), np.full(n, far))[0]
        assert np.all(got == (3 if genes[1][-1] == REV else -3))


@pytest.mark.parametrize("cutoff", [0, 1, -5, 10000, 1 << 59])
def test_cutoffs(cutoff):
    rng, TILE, BLOCK = np.random.default_rng(2), dims()["gene_tile"], dims()["near_threads"]
    tss = rng.integers(-5000, 200_000, size=TILE + 5)
    start = tss[rng.integers(0, len(tss), size=BLOCK + 3)] + rng.integers(-2, 3, size=BLOCK + 3)
    dist, found = nearest([(tss, rng.integers(1, 3, size=len(tss)))], np.zeros(len(start), dtype=np.int32), start, cutoff)
    assert found.any() == (cutoff > 0) and (cutoff != 1 or np.all(dist[found] == 0)) and (cutoff < 1 << 59 or found.all())


def lone_case(rng, live_lanes, n_lanes, last_tss_shift):
    """tile + 1 genes: the first freezes every lane but `live_lanes` (they sit 60 000 away from every gene but the last one, which is
    `last_tss_shift` from them); the genes between are closer to the frozen lanes than the first."""
    T, far, TILE = 1_000_000, 1_060_000, dims()["gene_tile"]
    tss = T + rng.integers(-4000, 4001, size=TILE + 1)
    tss[0], tss[-1] = T, far - last_tss_shift
    start = T - rng.integers(0, 3000, size=n_lanes)
    start[live_lanes] = far
    return (tss, rng.integers(1, 3, size=TILE + 1)), start


@pytest.mark.parametrize("lane", ["0", "63", "64", "unit-1"])
def test_one_lane_stays_live_to_the_last_gene_of_the_last_tile(lane):
    lane, BLOCK = size(lane, "near_threads"), dims()["near_threads"]
    rng = np.random.default_rng(lane)
    genes, start = lone_case(rng, [lane], BLOCK, 7)
    dist, found = nearest([genes], np.zeros(BLOCK, dtype=np.int32), start)
    assert found.all() and abs(int(dist[lane])) == 7
    others = np.delete(np.arange(BLOCK), lane)
    want = (1_000_000 - start[others]) * np.where(genes[1][0] == REV, 1, -1)      # d = start - T <= 0, negated for a '-' gene
    assert np.array_equal(dist[others], want)


@pytest.mark.parametrize("wave", ["first", "second", "last"])
def test_one_wave_stays_live_among_frozen_waves(wave):
    BLOCK = dims()["near_threads"]
    wave = {"first": 0, "second": 1, "last": BLOCK // 64 - 1}[wave]
    rng = np.random.default_rng(wave)
    lanes = np.arange(64 * wave, 64 * wave + 64)
    genes, start = lone_case(rng, lanes, BLOCK, -5)
    dist, found = nearest([genes], np.zeros(BLOCK, dtype=np.int32), start)
    assert found.all() and np.all(np.abs(dist[lanes]) == 5) and np.all(np.abs(np.delete(dist, lanes)) < 3000)


def test_a_block_frozen_in_the_first_tile_and_a_chain_that_accepts_in_every_tile():
    rng, TILE, BLOCK = np.random.default_rng(8), dims()["gene_tile"], dims()["near_threads"]
    genes, start = lone_case(rng, [], BLOCK + 1, 7)                         # nobody lives: two blocks leave the gene loop after tile 1
    dist, found = nearest([genes], np.zeros(BLOCK + 1, dtype=np.int32), start)
    assert found.all() and np.all(np.abs(dist) < 3000)
    D = 9900 + np.cumsum(rng.choice([-3, -2, -1, -1, 0, 0, 1], size=2 * TILE + 1))
    strand = rng.integers(1, 3, size=len(D))
    start = 500_000 + rng.integers(0, 90, size=70)
    dist, found = nearest([(500_000 - D, strand)], np.zeros(70, dtype=np.int32), start)
    last = int(np.flatnonzero(D == D.min())[0])                              # the first gene at the least distance wins
    assert found.all() and np.array_equal(np.abs(dist), start - (500_000 - D[last])) and D.min() > 0


# ------------------------------------------------------------------------------------------------ promoter_overlap

def overlap(table_arrays, chrom, start, end, up, down):
    t, off, tss, strand = table_arrays
    got = t.promoter_overlap(chrom, start, end, up, down)
    iv = fp.promoter_lists({"off": off, "tss": tss, "strand": strand}, up, down)
    want = [0 <= c < len(iv) and fp.overlap_literal(iv[c], s, e) for c, s, e in zip(np.asarray(chrom).tolist(), np.asarray(start).tolist(), np.asarray(end).tolist())]
    assert got.tolist() == want, np.flatnonzero(got != np.array(want))[:8]
    return got


def edge_regions(rng, off, tss, strand, chrom, up, down, n):
    """n regions on chromosome `chrom`, each placed against one gene's interval: ending on lo and lo + 1, starting on hi and hi - 1,
    empty inside and on both ends, inverted, overlapping, far."""
    g = rng.integers(off[chrom], off[chrom + 1], size=n)
    lo, hi = np.where(strand[g] == FWD, tss[g] - up, tss[g] - down), np.where(strand[g] == FWD, tss[g] + down, tss[g] + up)
    w, mid, k = rng.integers(1, 300, size=n), (lo + hi) // 2, np.arange(n) % 10
    forms = np.array([(lo - w, lo), (lo - w, lo + 1), (hi, hi + w), (hi - 1, hi + w), (mid, mid), (lo, lo), (hi, hi), (mid + w, mid - w), (mid - w, mid + w),
                      (hi + 10 ** 7, hi + 10 ** 7 + w)])
    return forms[k, 0, np.arange(n)], forms[k, 1, np.arange(n)]


def test_interval_ends_by_hand():
    ta = table_of([([1000], [FWD]), ([1000], [REV]), ([], [])])            # (300, 100): [700, 1100) on '+', [900, 1300) on '-'
    try:
        start = [600, 600, 1100, 1099, 800, 700, 1100, 900, 650]
        end = [700, 701, 1200, 1200, 800, 700, 1100, 800, 1150]
        # (900, 800): neither end <= lo nor start >= hi -- the literal test calls an inverted region inside the interval an overlap
        assert overlap(ta, [0] * 9, start, end, 300, 100).tolist() == [False, True, False, True, True, False, False, True, True]
        assert overlap(ta, [1] * 3 + [2, -1, 3], [800, 800, 1300, 0, 0, 0], [900, 901, 1400, 9999, 9999, 9999], 300, 100).tolist() == [False, True, False, False, False, False]
        # an empty interval [1000, 1000) and an inverted one [900, 700): by the literal test a region that spans them overlaps
        assert overlap(ta, [0, 0, 0], [1000, 999, 0], [1000, 1001, 5000], 0, 0).tolist() == [False, True, True]
        assert overlap(ta, [0, 0, 0], [1000, 0, 750], [1001, 5000, 850], 100, -300).tolist() == [False, True, False]
    finally:
        ta[0].close()


@pytest.mark.parametrize("up,down", [(2000, 2000), (3000, 1000), (0, 0), (500, -500), (100, -300), (-200, 1000)])
def test_gene_counts_around_the_powers_of_two(up, down):
    rng = np.random.default_rng(up + 7 * down + 10 ** 6)
    sizes = fp.annot_gene_counts(dims())
    chroms = []
    for n in sizes:
        tss = rng.integers(0, 40 * max(n, 1), size=n) * 100                # dense: neighbours' promoters overlap
        if n >= 4:
            tss[1::5] = tss[0::5][:len(tss[1::5])]                          # duplicate intervals where the strands agree
        chroms.append((tss, rng.integers(1, 3, size=n)))
    ta = table_of(chroms)
    try:
        for c, n in enumerate(sizes):
            if n:
                s, e = edge_regions(rng, ta[1], ta[2], ta[3], c, up, down, 40)
                overlap(ta, np.full(40, c, dtype=np.int32), s, e, up, down)
        overlap(ta, [sizes.index(0), -1, len(sizes)], [0, 0, 0], [10 ** 9] * 3, up, down)
    finally:
        ta[0].close()


def test_one_table_switched_between_two_extent_pairs_and_back():
    rng, TILE, OBLOCK = np.random.default_rng(4), dims()["gene_tile"], dims()["overlap_threads"]
    n_genes = TILE + 1
    tss = rng.integers(0, 10 ** 6, size=n_genes)
    ta = table_of([(tss, rng.integers(1, 3, size=n_genes)), ([77], [REV])])
    try:
        A, B = (2000, 2000), (2000, 500)                                    # only `downstream` changes
        runs = []
        for (up, down), n in ((A, OBLOCK - 1), (B, OBLOCK), (A, OBLOCK + 1), (B, 2 * OBLOCK + 1), (A, OBLOCK - 1)):
            r = np.random.default_rng(n)                                    # the first and the last call: the same regions
            s, e = edge_regions(r, ta[1], ta[2], ta[3], 0, *A, n)           # (placed against A's intervals in every call)
            runs.append((s, e, overlap(ta, np.zeros(n, dtype=np.int32), s, e, up, down)))
            dist, found = ta[0].nearest_tss(np.zeros(5, dtype=np.int32), tss[:5] + 3)
            want = fp.nearest_restated(ta[1], ta[2], ta[3], np.zeros(5, dtype=np.int32), tss[:5] + 3, 10000, TILE)
            assert found.all() and np.array_equal(dist, want[0])
        assert np.array_equal(runs[0][2], runs[4][2])
        s, e = runs[0][0], runs[0][1]
        assert not np.array_equal(overlap(ta, np.zeros(len(s), dtype=np.int32), s, e, *B), runs[0][2])     # B differs from A somewhere
    finally:
        ta[0].close()
