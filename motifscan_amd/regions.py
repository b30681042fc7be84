"""
motifscan_amd.regions -- genomic regions and the region utilities of `motifscan scan`: the surface of the reference's
`motifscan.region` (GenomicRegion, region/__init__.py:17-70) and `motifscan.region.utils` (region/utils.py), with the walks over a
chromosome's genes on the device and the region lists as arrays.

    GenomicRegion(chrom, start, end, summit=None, score=None)                               region/__init__.py:17-70
    RegionArray                       a region list as arrays: `chroms` (names) + chrom_idx / start / end / summit; len, indexing and
                                      iteration give GenomicRegion objects, == compares with a RegionArray or a list of regions
    overlap_with(intervals, start, end)                                                     utils.py:16-48 (plain Python, literal)
    subset_by_location(regions, genes, location, upstream=2000, downstream=2000)            utils.py:51-86
    generate_control_regions(n_random, regions, chrom_size, genes=None, random_seed=None)   utils.py:89-145 -> RegionArray
    dis_to_nearest_gene(region, genes, distance_cutoff=10000)                               utils.py:148-180
    nearest_gene_distances(regions, genes, distance_cutoff=10000) -> (distance, found)      the same for a whole region list

`regions` is a list of objects with .chrom .start .end (.summit) -- the reference's own GenomicRegion works -- or a RegionArray;
`genes` is a motifscan_amd.annotation.Genes.  Everything that reads `genes` runs on the device (ms_genes_nearest_tss,
ms_genes_promoter_overlap) and raises without one; generate_control_regions(genes=None) needs none.  The random draws are the
reference's: Python's global `random` generator, the same values in the same order, and its state afterwards is the state the
reference leaves (ms_control_regions_replay_host replays randint / choice from the generator's raw 32-bit words).
"""
import logging
import random

import numpy as np

from . import _lib

logger = logging.getLogger(__name__)


class GenomicRegion:
    """One region [start, end) of a chromosome, 0-based, with a summit (the middle unless given) and an optional score.
    The reference's checks: an empty or reversed region is a ValueError, a summit outside the region only a warning."""

    def __init__(self, chrom, start, end, summit=None, score=None):
        lo, hi = int(start), int(end)
        if not lo < hi:
            raise ValueError(f"region {chrom}:{start}-{end} is empty: start must be below end")
        peak = (lo + hi) // 2 if summit is None else int(summit)
        if peak < lo or peak >= hi:
            logger.warning(f"summit {summit} of region {chrom}:{start}-{end} lies outside it")
        self.chrom, self.start, self.end, self.summit, self.score = chrom, lo, hi, peak, score

    def __repr__(self):
        return f"GenomicRegion({self.chrom}:{self.start}-{self.end})"


class RegionArray:
    """A region list as a struct of arrays: chroms (distinct names) and, per region, chrom_idx (into chroms), start, end, summit."""

    def __init__(self, chroms, chrom_idx, start, end, summit=None):
        self.chroms = list(chroms)
        self.chrom_idx = np.ascontiguousarray(chrom_idx, dtype=np.int32)
        self.start = np.ascontiguousarray(start, dtype=np.int64)
        self.end = np.ascontiguousarray(end, dtype=np.int64)
        self.summit = (self.start + self.end) // 2 if summit is None else np.ascontiguousarray(summit, dtype=np.int64)
        if not (self.chrom_idx.shape == self.start.shape == self.end.shape == self.summit.shape) or self.start.ndim != 1:
            raise ValueError("chrom_idx, start, end and summit must have one entry per region")
        if self.chrom_idx.size and (self.chrom_idx.min() < 0 or self.chrom_idx.max() >= len(self.chroms)):
            raise ValueError("chrom_idx outside chroms")

    @classmethod
    def from_regions(cls, regions):
        """From any iterable of objects with .chrom .start .end and, optionally, .summit."""
        if isinstance(regions, cls):
            return regions
        chroms, index = [], {}
        ci, st, en, su = [], [], [], []
        for r in regions:
            k = index.get(r.chrom)
            if k is None:
                k = index[r.chrom] = len(chroms)
                chroms.append(r.chrom)
            ci.append(k)
            st.append(r.start)
            en.append(r.end)
            summit = getattr(r, "summit", None)
            su.append((r.start + r.end) // 2 if summit is None else summit)
        return cls(chroms, ci, st, en, su)

    def __len__(self):
        return self.start.size

    def chrom_names(self):
        """The chromosome name of every region (an object array)."""
        return np.array(self.chroms, dtype=object)[self.chrom_idx] if self.chroms else np.zeros(0, dtype=object)

    def take(self, idx):
        idx = np.asarray(idx)
        return RegionArray(self.chroms, self.chrom_idx[idx], self.start[idx], self.end[idx], self.summit[idx])

    def __getitem__(self, i):
        if isinstance(i, (int, np.integer)):
            return GenomicRegion(self.chroms[self.chrom_idx[i]], self.start[i], self.end[i], self.summit[i])
        return self.take(np.arange(len(self))[i])

    def __iter__(self):
        for c, s, e, m in zip(self.chrom_idx.tolist(), self.start.tolist(), self.end.tolist(), self.summit.tolist()):
            yield GenomicRegion(self.chroms[c], s, e, m)

    def __eq__(self, other):
        if not isinstance(other, (RegionArray, list, tuple)):
            return NotImplemented
        other = RegionArray.from_regions(other)
        return (len(self) == len(other) and np.array_equal(self.start, other.start) and np.array_equal(self.end, other.end)
                and np.array_equal(self.summit, other.summit) and bool((self.chrom_names() == other.chrom_names()).all()))

    __hash__ = None

    def __repr__(self):
        return f"RegionArray({len(self)} regions on {len(self.chroms)} chromosomes)"


def overlap_with(intervals, start, end):
    """Whether [start, end) overlaps one of `intervals` (sorted [lo, hi] pairs), by the reference's binary search -- which, for
    intervals of unequal width, can miss an overlap that exists; subset_by_location only ever gives it equal widths."""
    left, right = 0, len(intervals) - 1
    while left <= right:
        mid = (left + right) // 2
        lo, hi = intervals[mid][0], intervals[mid][1]
        if not (end <= lo or start >= hi):
            return True
        if start >= hi:
            left = mid + 1
        else:
            right = mid - 1
    return False


def _gene_chrom_idx(arr, genes):
    """The gene table's chromosome index of every region (-1: the annotation does not know the chromosome)."""
    lut = np.array([genes.index.get(c, -1) for c in arr.chroms], dtype=np.int32)
    return lut[arr.chrom_idx] if len(arr) else np.zeros(0, dtype=np.int32)


def nearest_gene_distances(regions, genes, distance_cutoff=10000):
    """dis_to_nearest_gene of every region against its chromosome's genes: (distance int64, found bool); found is False where the
    reference returns None (distance is 0 there), also on chromosomes without genes."""
    arr = RegionArray.from_regions(regions)
    return genes.table().nearest_tss(_gene_chrom_idx(arr, genes), arr.start, distance_cutoff)


def dis_to_nearest_gene(region, genes, distance_cutoff=10000):
    """The signed distance of region.start to the gene the reference's file-order walk ends on, or None.  `genes`: the list of one
    chromosome's genes (Genes.fetch)."""
    genes = list(genes)
    if not genes:
        return None
    table = _lib.GeneTable([0, len(genes)], [g.tss for g in genes], [1 if g.strand == "+" else 2 for g in genes])
    try:
        dist, found = table.nearest_tss([0], [region.start], distance_cutoff)
    finally:
        table.close()
    return int(dist[0]) if found[0] else None


def subset_by_location(regions, genes, location, upstream=2000, downstream=2000):
    """The regions that overlap a promoter (location == 'promoter') or do not (any other string, as in the reference), in input
    order: a list of the input's own objects for a list, a RegionArray for a RegionArray."""
    arr = RegionArray.from_regions(regions)
    if len(arr) == 0:
        return arr if isinstance(regions, RegionArray) else []
    overlap = genes.table().promoter_overlap(_gene_chrom_idx(arr, genes), arr.start, arr.end, upstream, downstream)
    keep = np.flatnonzero(overlap == (location == "promoter"))
    if isinstance(regions, RegionArray):
        return arr.take(keep)
    regions = regions if isinstance(regions, (list, tuple)) else list(regions)
    return [regions[i] for i in keep.tolist()]


_CHUNK_WORDS = 1 << 22            # generator words drawn ahead per replay call, at most (16 MiB); tests lower it


class _WordReplay:
    """The global `random` generator's next raw 32-bit words, drawn in bulk; commit(n) leaves the generator as if exactly n of them
    had been consumed."""

    def __init__(self):
        self.state0 = random.getstate()
        self.buf = np.zeros(0, dtype=np.uint32)        # words not yet consumed
        self.consumed = 0                              # words in front of buf[0]

    def need(self, n):
        if self.buf.size < n:
            k = int(n - self.buf.size)
            more = np.frombuffer(random.getrandbits(32 * k).to_bytes(4 * k, "little"), dtype="<u4")   # least significant word first
            self.buf = np.concatenate([self.buf, more.astype(np.uint32)])

    def advance(self, n):
        self.buf = self.buf[n:]
        self.consumed += int(n)

    def commit(self, n_words):
        random.setstate(self.state0)
        if n_words:
            random.getrandbits(32 * int(n_words))


def _replay_control_starts(chrom_size, length, n_random, max_attempts, chrom_name, gene_args=None):
    """Drive ms_control_regions_replay_host over all regions from the global generator: (start [n, n_random], attempts [n])."""
    n = len(length)
    start = np.zeros((n, n_random), dtype=np.int64)
    attempts = np.zeros(n, dtype=np.int64)
    replay = _WordReplay()
    done, want = 0, 0
    while done < n:
        want = max(2 * want, min(2 * (n - done) * (n_random + 1) + 64, _CHUNK_WORDS))
        replay.need(want)
        sl = slice(done, n)
        kw = {} if gene_args is None else dict(gene_lo=gene_args[0][sl], gene_hi=gene_args[1][sl], distance=gene_args[2][sl],
                                               found=gene_args[3][sl], tss=gene_args[4], strand=gene_args[5])
        s, _, a, nd, stop, stop_words = _lib.control_regions_replay(replay.buf, chrom_size[sl], length[sl], n_random, max_attempts, **kw)
        start[done:done + nd] = s[:nd]
        attempts[done:done + nd] = a[:nd]
        if stop in (_lib.MS_REPLAY_DONE, _lib.MS_REPLAY_WORDS):
            replay.advance(stop_words)
            if nd:
                want = 0                               # progress: the next chunk is sized afresh (no progress: twice the words)
            done += nd
            continue
        bad = done + nd                                # the reference raises (or never ends) here, with these words consumed
        replay.commit(replay.consumed + stop_words)
        if stop == _lib.MS_REPLAY_NO_SIZE:
            raise KeyError(chrom_name(bad))
        if stop == _lib.MS_REPLAY_EMPTY_RANGE:
            width = int(chrom_size[bad] - length[bad] + 1)
            raise ValueError(f"empty range for randrange() (0, {width}, {width})")
        if stop == _lib.MS_REPLAY_WIDE:
            raise ValueError(f"region {bad} on {chrom_name(bad)}: {int(chrom_size[bad] - length[bad] + 1)} possible starts; draws of "
                             f"2^32 or more values take several generator words each and are not replayed")
        raise RuntimeError(f"region {bad} on {chrom_name(bad)}: {max_attempts} attempts did not give {n_random} control regions inside "
                           f"the chromosome (the reference would never end; raise max_attempts)")
    replay.commit(replay.consumed)
    return start, attempts


def generate_control_regions(n_random, regions, chrom_size, genes=None, random_seed=None, max_attempts=None):
    """n_random control regions per input region, of its length and on its chromosome, drawn as the reference draws them from the
    global `random` generator (seeded first if random_seed is not None): uniformly without `genes`; with `genes`, at the input
    region's signed distance from a random gene's TSS (a random distance of 10 - 100 kb where no gene is within 10 kb), and none for
    regions on chromosomes without genes.  Returns a RegionArray in the reference's order.
    Errors, each with the generator where the reference leaves it: KeyError for a chromosome missing in chrom_size, ValueError for a
    region longer than its chromosome (genes=None), ValueError for 2^32 or more possible starts, and -- where the reference loops
    forever because no gene gives a start inside the chromosome -- RuntimeError after max_attempts attempts for one region (default
    100 * n_random + 10^6)."""
    if random_seed is not None:
        logger.debug(f"Setting random seed: {random_seed}")
        random.seed(random_seed)
    arr = RegionArray.from_regions(regions)
    n, n_random = len(arr), max(int(n_random), 0)
    cap = int(max_attempts) if max_attempts is not None else 100 * n_random + 1_000_000
    length = arr.end - arr.start
    sizes = []
    for c in arr.chroms:
        try:
            sizes.append(int(chrom_size[c]))
        except KeyError:
            sizes.append(_lib.MS_REPLAY_SIZE_MISSING)
    size = np.array(sizes, dtype=np.int64)[arr.chrom_idx] if n else np.zeros(0, dtype=np.int64)
    keep = np.ones(n, dtype=bool)
    gene_args = None
    if genes is not None and n:
        gidx = _gene_chrom_idx(arr, genes)
        dist, found = genes.table().nearest_tss(gidx, arr.start, 10000)
        off = np.append(genes.chrom_offsets, genes.chrom_offsets[-1])        # (an annotation without chromosomes: offsets [0], every gidx -1)
        lo = np.where(gidx >= 0, off[np.maximum(gidx, 0)], 0)
        hi = np.where(gidx >= 0, off[np.maximum(gidx, 0) + 1], 0)
        keep = hi > lo
        gene_args = (lo, hi, dist, found, genes.tss, genes.strand)
    if n:
        start, _ = _replay_control_starts(size, length, n_random, max(cap, 1), lambda i: arr.chroms[arr.chrom_idx[i]], gene_args)
    else:
        start = np.zeros((0, n_random), dtype=np.int64)
    start = start[keep].reshape(-1)
    out_len = np.repeat(length[keep], n_random)
    out = RegionArray(arr.chroms, np.repeat(arr.chrom_idx[keep], n_random), start, start + out_len)
    return out
