"""
ms_scan_regions_once (ms_regions.hip) against the pinned oracle over the regions cut as strings: the boundary fuzz of
tests/fuzz_parity.py (--once) and directed region lists for what the hand-out does beside the scan -- the host merge into spans (touching
regions, equal starts, empty regions and spans, one region, none, two radix passes), the two forms of the span hits' keys, the inclusion
test one base either side of a region's ends, a site handed to a thousand regions.  Every directed list runs at an all-pass cutoff (every
window of every region is compared) and at cutoffs on attainable scores, through fuzz_parity.check_once: as is with region counts and
site tables, twice, with global-position keys, de-duplicated.  Every comparison is exact (integers by value, scores by their bits).
"""
import numpy as np
import pytest

import fuzz_parity as fp
from motifscan_amd import _lib, scanner

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _device():
    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible")
    _lib.set_device(0)


def test_fuzz_once(oracle):
    total = {}
    for seed in fp.SEEDS["once"]:
        ok, info = fp.run_once_case(seed, oracle, _lib)
        assert ok, info
        fp.add_tally(total, info)
    print(f"once: seeds {fp.SEEDS['once']}: {fp.shown(total)}")
    assert not fp.unmet_conditions("once", total)


# ------------------------------------------------------------------------------------------------ directed region lists

def sequence(rng, n):
    """n bases with lower case, N and another IUPAC letter, and one run of N."""
    s = "".join(rng.choice(list("ACGTNacgtR"), p=[.2, .2, .2, .2, .03, .04, .04, .04, .04, .01], size=n))
    a = int(rng.integers(0, max(n - 30, 1)))
    return s[:a] + "N" * min(25, n - a) + s[a + 25:]


def motifs(rng, extra_widths=()):
    """A handful of motifs of fuzz_parity's kinds that can have sites (max_raw > 0), and one of every width asked for."""
    mats = [m for m in fp.random_motifs(rng, [5]) if fp.max_raw_of(m) > 0]
    for w in extra_widths:
        m = fp.random_matrix(rng, w)
        while fp.max_raw_of(m) == 0:
            m = fp.random_matrix(rng, w)
        mats.append(m)
    assert mats
    return mats


def check(oracle, rng, chroms, regions, mats, strand=3):
    """The region list [(chromosome, start, end)] at the all-pass cutoff and at attainable ones; returns the all-pass expected hits."""
    ci, st, en = (np.array([r[k] for r in regions], dtype=t) for k, t in enumerate((np.int32, np.int64, np.int64)))
    seqs = [chroms[c][a:b] for c, a, b in regions]
    wants = []
    for cutoffs in (np.full(len(mats), fp.ALL_PASS), np.array([fp.attainable_cutoff(rng, m, seqs) for m in mats])):
        case = {"mats": mats, "cutoffs": cutoffs, "chroms": chroms, "chrom_idx": ci, "start": st, "end": en, "seqs": seqs, "strand": strand,
                "layout": "directed"}
        want, _ = fp.expected_once(oracle, case)
        bad = fp.check_once(case, want, _lib, dedup=True)
        assert bad is None, bad
        wants.append(want)
    return wants[0]


def default_form(chroms, regions, n_motifs):
    """"local" / "global": the key form the library chooses for the span set of these regions."""
    case = {"chrom_idx": [r[0] for r in regions], "start": [r[1] for r in regions], "end": [r[2] for r in regions]}
    return "local" if _lib.key_layout(*fp.once_span_shape(case), n_motifs)[1] > 0 else "global"


def test_empty_region_list():
    rng = np.random.default_rng(1)
    mats = motifs(rng)
    genome = _lib.ResidentGenome({"c0": sequence(rng, 200)})
    pw = _lib.PwmSet.from_matrices(mats, np.full(len(mats), fp.ALL_PASS))
    none32, none64 = np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int64)
    for flags in (0, _lib.MS_SCAN_EXACT_ONLY):
        res = _lib.scan_regions_once(pw, genome, none32, none64, none64, 3, flags)
        assert res.n_hits == 0 and np.array_equal(res.motif_offsets, np.zeros(len(mats) + 1, dtype=np.int64))
        assert all(len(res.hits()[k]) == 0 for k in ("seq_idx", "pos", "score", "strand"))
        assert np.array_equal(res.region_counts(), np.zeros(len(mats), dtype=np.int64))
        res.close()
    pw.close()
    genome.close()


def test_degenerate_region_lists(oracle):
    rng = np.random.default_rng(2)
    chroms = [sequence(rng, 45), sequence(rng, 300)]
    mats = motifs(rng)
    for one in ((1, 0, 300), (1, 33, 34), (0, 44, 45), (1, 7, 7)):                       # one region: a chromosome, one base, none
        want = check(oracle, rng, chroms, [one], mats)
        assert (len(want["pos"]) > 0) == (one[2] - one[1] >= min(m.shape[1] for m in mats))
    # all regions empty: inside one another, equal, at both chromosome ends -- every one a span of no bases
    check(oracle, rng, chroms, [(1, 5, 5), (1, 5, 5), (0, 0, 0), (0, 45, 45), (1, 300, 300), (1, 64, 64), (1, 0, 0)], mats)
    # all regions shorter than every motif, overlapping, nested and apart
    mats = [fp.random_matrix(rng, w) for w in (6, 9, 17, 64)]
    short = [(int(c), int(a), int(a) + int(n)) for c, a, n in zip(rng.integers(0, 2, 40), rng.integers(0, 40, 40), rng.integers(0, 6, 40))]
    want = check(oracle, rng, chroms, short, mats)
    assert len(want["pos"]) == 0


def test_one_base_grid(oracle):
    """Two regions that touch, that share one base, and one of them a base longer: a motif of one column and one as wide as the first
    region, so that at the all-pass cutoff every window that ends flush with a region, or sticks out of it by one base, is decided."""
    rng = np.random.default_rng(3)
    chroms = [sequence(rng, 13), sequence(rng, 100)]
    a, b, c = 37, 48, 70
    mats = motifs(rng, extra_widths=(1, b - a))
    for first, second in (((a, b), (b, c)), ((a, b), (b - 1, c)), ((a, b + 1), (b, c))):
        for strand in (1, 2, 3):
            want = check(oracle, rng, chroms, [(1, *first), (1, *second)], mats, strand)
            assert len(want["pos"]) > 0
    assert fp.merge_spans([1, 1], [a, b], [b, c])[1].tolist() == [0, 1] and fp.merge_spans([1, 1], [a, b - 1], [b, c])[1].tolist() == [0, 0]


def long_span_layout(rng, equalised):
    """64 spans with empty regions (spans of no bases) between them.  Not equalised: 63 regions of 40 bases on their own and one of 5000
    that 200 nested regions of 1..60 bases overlap.  Equalised: 64 regions of 256 bases with three nested ones each."""
    regions = []
    if equalised:
        for k in range(64):
            regions += [(0, 300 * k, 300 * k + 256), (0, 300 * k + 280, 300 * k + 280)]
            regions += [(0, 300 * k + int(x), 300 * k + int(x) + int(n)) for x, n in zip(rng.integers(0, 196, 3), rng.integers(1, 61, 3))]
        length = 64 * 300
    else:
        for k in range(63):
            regions += [(0, 45 * k, 45 * k + 40), (0, 45 * k + 42, 45 * k + 42)]
        regions.append((0, 2900, 7900))
        regions += [(0, 2900 + int(x), 2900 + int(x) + int(n)) for x, n in zip(rng.integers(0, 4940, 200), rng.integers(1, 61, 200))]
        length = 7950
    return [sequence(rng, length)], [regions[int(k)] for k in rng.permutation(len(regions))]


def test_long_span_among_small_ones_takes_global_keys(oracle):
    rng = np.random.default_rng(4)
    chroms, regions = long_span_layout(rng, equalised=False)
    mats = motifs(rng)
    assert default_form(chroms, regions, len(mats)) == "global"
    want = check(oracle, rng, chroms, regions, mats)
    assert len(want["pos"]) > 50_000


def test_equal_spans_take_local_keys_and_global_ones_when_told(oracle):
    rng = np.random.default_rng(5)
    chroms, regions = long_span_layout(rng, equalised=True)
    mats = motifs(rng)
    assert default_form(chroms, regions, len(mats)) == "local"
    want = check(oracle, rng, chroms, regions, mats)                 # (check_once runs it by itself and under MS_HIT_COORD=global)
    assert len(want["pos"]) > 50_000


def test_one_site_handed_to_a_thousand_duplicates(oracle):
    rng = np.random.default_rng(6)
    chroms = [sequence(rng, 90)]
    mats = motifs(rng)[:3]
    region = (0, 21, 61)
    single = check(oracle, rng, chroms, [region], mats, strand=3)
    want = check(oracle, rng, chroms, [region] * 1000, mats, strand=3)
    k = np.diff(single["motif_offsets"])
    assert len(single["pos"]) > 0 and len(want["pos"]) == 1000 * len(single["pos"])
    assert np.array_equal(want["motif_offsets"], 1000 * single["motif_offsets"])
    # region-major within the motif: the single copy's sites, a thousand times over
    assert np.array_equal(want["seq_idx"], np.concatenate([np.repeat(np.arange(1000), n) for n in k]))
    assert np.array_equal(want["pos"], np.concatenate([np.tile(single["pos"][a:a + n], 1000) for a, n in zip(single["motif_offsets"][:-1], k)]))


def test_starts_beyond_16_bits_in_descending_order(oracle):
    """Five chromosomes and region starts above 2^16: chromosome << sbits | start takes more than 16 bits, the host's radix sort two
    passes.  The regions come in descending (chromosome, start) order."""
    rng = np.random.default_rng(7)
    chroms = [sequence(rng, 70_000) for _ in range(5)]
    regions = []
    for c in range(5):
        regions += [(c, int(a), int(a) + int(n)) for a, n in zip(rng.integers(65_536, 67_000, 25), rng.integers(0, 90, 25))]
        regions += [(c, int(a), int(a) + int(n)) for a, n in zip(rng.integers(0, 300, 5), rng.integers(0, 90, 5))]
        regions.append((c, 69_950, 70_000))
    regions.sort(key=lambda r: (-r[0], -r[1]))
    assert max(r[1] for r in regions) >= 1 << 16
    want = check(oracle, rng, chroms, regions, motifs(rng))
    assert len(want["pos"]) > 10_000


def test_scanner_takes_the_path_with_the_per_region_result():
    """A region list Scanner hands to ms_scan_regions_once by itself (_as_overlapping) gives the arrays and the region counts of the
    per-region scan over the same regions cut by ResidentGenome.extract()."""
    rng = np.random.default_rng(8)
    chroms = {"chrA": sequence(rng, 700), "chrB": sequence(rng, 1500)}
    mats = motifs(rng)

    class Region:
        def __init__(self, c, s, e):
            self.chrom, self.start, self.end, self.summit = c, s, e, (s + e) // 2

    class Pwm:
        def __init__(self, m, c):
            self.matrix, self.cutoffs, self.length = m, {"1e-3": c}, m.shape[1]

    regions = []
    for name, seq in chroms.items():
        for s in rng.integers(0, len(seq), 60).tolist():
            regions.append(Region(name, max(s - 50, 0), min(s + 50, len(seq))))
    seqs = [chroms[r.chrom][r.start:r.end] for r in regions]
    pwms = [Pwm(m, fp.attainable_cutoff(rng, m, seqs)) for m in mats]
    genome = _lib.ResidentGenome(chroms)
    for strand, dedup in (("both", True), ("+", False), ("-", True)):
        once = scanner.Scanner(genome, regions, 0, strand, "1e-3", remove_dup=dedup)
        per = scanner.Scanner(genome, regions, 0, strand, "1e-3", remove_dup=dedup)
        per._as_overlapping = lambda: None                      # the per-region scan of the extract()-ed set
        assert once._as_overlapping() is not None and once._as_sweep() is None
        got, want = once.scan_motifs_arrays(pwms, with_tables=True), per.scan_motifs_arrays(pwms, with_tables=True)
        assert len(want["score"]) > 100
        for k in ("motif", "region", "start", "strand", "motif_offsets", "n_regions_with_site", "n_sites"):
            assert np.array_equal(got[k], want[k]), (strand, k)
        assert fp.same_bits(got["score"], want["score"]) and np.array_equal(got["max_score"], want["max_score"], equal_nan=True)
        assert np.array_equal(once.count_regions_with_sites(pwms), per.count_regions_with_sites(pwms))
        assert np.array_equal(once.count_regions_with_sites(pwms), want["n_regions_with_site"])
        once.close()
        per.close()
    genome.close()
