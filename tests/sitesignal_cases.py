"""
The named cases of the site-signal tests (ms_result_site_signal): synthetic hit lists over synthetic tracks, each placed on one boundary
of the kernel, sized from ms_debug_sitesignal_dims.  tests/test_sitesignal_host.py holds every case to what it claims;
tests/test_gpu_sitesignal.py runs them on the device.  No device is needed to build them.

A case is a dict: name, widths [P], lengths [R] (the regions), values int32 [sum lengths], hits = (motif_offsets, seq_idx, pos, strand)
in ms_result order, flank, and for the large ones closed=True: their expected sums are closed forms, not the sequential restatement.
"""
import numpy as np

from motifscan_amd import _lib

DIMS = _lib.sitesignal_dims()                      # constants of the build: no device
THREADS, CHUNK, PANEL, MAX_BX = DIMS["threads"], DIMS["chunk_sites"], DIMS["panel_columns"], DIMS["max_blocks_x"]
MAX_FLANK = 512


def hit_arrays(per_motif):
    """per motif a list of (region, pos, strand) -> (motif_offsets, seq_idx, pos, strand) in ms_result order."""
    rows = [np.asarray(sorted(p), dtype=np.int64).reshape(-1, 3) for p in per_motif]
    offsets = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    flat = np.concatenate(rows) if rows else np.zeros((0, 3), dtype=np.int64)
    return offsets, flat[:, 0].copy(), flat[:, 1].copy(), flat[:, 2].astype(np.int8)


def offsets_of(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


def random_values(rng, n, big=False):
    """Signed values; big: the whole int32 range, so a sum of a few sites leaves 32 bits."""
    if big:
        return rng.integers(-2 ** 31, 2 ** 31, size=n, dtype=np.int64).astype(np.int32)
    return rng.integers(-1000, 1000, size=n, dtype=np.int64).astype(np.int32)


def edge_sites(lengths, widths, rng=None, extra=0):
    """Per motif: both strands at pos 0 and L - W of every region that holds the motif, and `extra` random positions."""
    sites = []
    for W in widths:
        per = []
        for r, L in enumerate(lengths):
            if L < W:
                continue
            ps = {0, int(L) - W}
            if extra and rng is not None:
                ps |= set(rng.integers(0, int(L) - W + 1, size=extra).tolist())
            per += [(r, int(p), st) for p in ps for st in (1, 2)]
        sites.append(per)
    return sites


def case(name, widths, lengths, values, sites, flank, **kw):
    lengths = [int(x) for x in lengths]
    assert len(values) == sum(lengths)
    return dict(name=name, widths=[int(w) for w in widths], lengths=lengths, values=np.asarray(values, dtype=np.int32),
                hits=hit_arrays(sites) if isinstance(sites, list) else sites, flank=int(flank), **kw)


def column_case(ncol):
    """W + 2 * flank = ncol for the first motif; a second, narrower motif shares the pitch."""
    rng = np.random.default_rng(ncol)
    flank = min(ncol // 2 - 1, MAX_FLANK)
    W = ncol - 2 * flank
    lengths = [W, W + 1, W + 31, W + 40, 2 * W + 70, 3, W + 2 * flank + 9]
    widths = [W, max(1, W // 2)]
    return case(f"columns_{ncol}", widths, lengths, random_values(rng, sum(lengths), big=True), edge_sites(lengths, widths, rng, extra=2), flank)


def flank_case(flank):
    rng = np.random.default_rng(1000 + flank)
    widths = [6, 11]
    lengths = [11, 40, 700, 13, 1200, 11]
    return case(f"flank_{flank}", widths, lengths, random_values(rng, sum(lengths)), edge_sites(lengths, widths, rng, extra=3), flank)


def pad_case():
    """The first region's site at pos 0 and the last region's site ending on its L, both strands, with the maximal flank: every flank
    column of the first site's left and of the last site's right lies outside the track."""
    lengths = [5, 9, 6]
    values = np.arange(1, 21, dtype=np.int32) * 1000 + 7
    sites = [[(0, 0, 1), (0, 0, 2), (2, 3, 1), (2, 3, 2)]]
    return case("pad", [3], lengths, values, sites, MAX_FLANK)


def chunk_case():
    """CHUNK - 1, CHUNK and CHUNK + 1 sites, with empty motifs at the start, in the middle and at the end of the range."""
    rng = np.random.default_rng(7)
    lengths = rng.integers(20, 60, size=40)
    widths = [2, 3, 4, 2, 5, 3, 2]
    n_hits = [0, CHUNK - 1, CHUNK, 0, CHUNK + 1, 5, 0]
    sites = []
    for W, n in zip(widths, n_hits):
        r = rng.integers(0, len(lengths), size=n)
        sites.append([(int(x), int(rng.integers(0, lengths[x] - W + 1)), int(rng.integers(1, 3))) for x in r])
    return case("chunks", widths, lengths, random_values(rng, int(lengths.sum())), sites, 2, n_hits=n_hits)


def stride_case():
    """More chunks than blocks in x: MAX_BX * CHUNK + CHUNK + 7 sites of one region, W = 1, flank 0 -- closed form."""
    n = MAX_BX * CHUNK + CHUNK + 7
    L = 50
    rng = np.random.default_rng(8)
    k = np.arange(n, dtype=np.int64)
    pos = np.sort(k % L)
    strand = (1 + (k * 7 // 3) % 2).astype(np.int8)
    hits = (np.array([0, n], dtype=np.int64), np.zeros(n, dtype=np.int64), pos, strand)
    return case("stride", [1], [L], random_values(rng, L, big=True), hits, 0, closed=True)


def int64_case(value):
    """2^22 + 1 sites of one base that holds `value`: the sum is odd (for 2^31 - 1) and above 2^53 in magnitude."""
    n = 2 ** 22 + 1
    hits = (np.array([0, n], dtype=np.int64), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64), np.ones(n, dtype=np.int8))
    return case(f"int64_{value}", [1], [1], np.array([value], dtype=np.int64).astype(np.int32), hits, 0, closed=True)


def strands_case():
    """Motif 0: both strands at one position; motif 1: every site '-'."""
    rng = np.random.default_rng(9)
    lengths = [30, 12, 25]
    sites = [[(0, 10, 1), (0, 10, 2)], [(0, 3, 2), (1, 0, 2), (1, 6, 2), (2, 19, 2), (2, 7, 2)]]
    return case("strands", [4, 6], lengths, random_values(rng, sum(lengths)), sites, 5)


def general_case():
    """Several motifs of unequal numbers of sites over ragged regions, for the output combinations, the sub-ranges and the shards."""
    rng = np.random.default_rng(10)
    lengths = rng.integers(10, 90, size=30)
    widths = [6, 11, 2, 9]
    return case("general", widths, lengths, random_values(rng, int(lengths.sum()), big=True), edge_sites(lengths, widths, rng, extra=4), 7)


def closed_form(c):
    """(sum, cover, n_sites, per_site) of a closed=True case: one motif of W = 1, flank 0, one column."""
    _, seq_idx, pos, strand = c["hits"]
    off = offsets_of(c["lengths"])
    v = c["values"].astype(np.int64)[off[seq_idx] + pos]
    total, cover = np.zeros((1, 2, 1), dtype=np.int64), np.zeros((1, 2, 1), dtype=np.int64)
    for s in (0, 1):
        sel = strand == s + 1
        total[0, s, 0] = int(v[sel].astype(object).sum()) if sel.any() else 0        # Python ints: no float, no wrap
        cover[0, s, 0] = int(sel.sum())
    per_site = np.zeros((len(v), 3), dtype=np.int64)
    per_site[:, 1] = v
    return total, cover, cover[:, :, 0].copy(), per_site


COLUMN_COUNTS = (63, 64, 65, 128, 129, PANEL, PANEL + 1)
FLANKS = (0, MAX_FLANK)


def all_cases():
    """Every case that is checked against the restatement (the closed-form ones are built where they are used: they are large)."""
    return [column_case(n) for n in COLUMN_COUNTS] + [flank_case(f) for f in FLANKS] + [pad_case(), chunk_case(), strands_case(), general_case()]
