"""
ms_seqset_shuffle (ms_shuffle.hip) on the GPU against its sequential restatement motifscan_amd.shuffle.shuffle_host: every comparison is
byte for byte, of SeqSet.shuffled(...).to_strings() with the restatement's strings and of all four device arrays with the host packer's
(ms_debug_host_pack) of those strings.  Sized from ms_debug_shuffle_dims: runs either side of the LDS tile, a run through the global
path, every phase of a 32-base unit, sequences that share units, block and unit edges, empty / all-N / alternating sets, low-complexity
runs on both paths, shards, sets cut from a (personal) genome, the argument checks, the scan entry points downstream and Scanner.shuffled.
"""
import ctypes

import numpy as np
import pytest

import shuffle_cases as sc
from motifscan_amd import _lib, scanner, shuffle

pytestmark = pytest.mark.gpu

KINDS = ("mono", "dinuc")


@pytest.fixture(scope="module", autouse=True)
def _device():
    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible")
    _lib.set_device(0)


@pytest.fixture(scope="module")
def dims():
    d = _lib.shuffle_dims()
    assert 3 <= d["lane_run"] <= d["lds_run"] and d["block_bases"] % 32 == 0
    return d


def as_packed_text(s):
    """what a packed set can give back of a string: ACGT in upper case, N for anything else"""
    return "".join(c if c in "ACGT" else "N" for c in s.upper())


def offsets_of(seqs):
    off = np.zeros(len(seqs) + 1, dtype=np.int64)
    if seqs:
        np.cumsum([len(s) for s in seqs], out=off[1:])
    return off


def check_against_host(seqs, kind, seed, base=0, source=None):
    """shuffle `source` (default: a set made of `seqs`) on the device and hold strings and all four device arrays against the restatement"""
    sq = source if source is not None else _lib.SeqSet.from_strings(seqs)
    sh = None
    try:
        sh = _lib.seqset_shuffled(sq, kind, seed, base)
        want = shuffle.shuffle_host(seqs, kind, seed, base)
        got = sh.to_strings()
        assert len(got) == len(want)
        for k, (g, w) in enumerate(zip(got, want)):
            assert g == as_packed_text(w), (kind, seed, base, k, len(w))
        joined = np.frombuffer("".join(want).encode("latin-1"), dtype=np.uint8)
        ref = _lib.host_pack(joined, offsets_of(want))
        dev = _lib.seqset_planes(sh)
        for g, w, what in zip(dev, ref, ("codes", "nmask", "blk2reg", "blkinfo")):
            assert np.array_equal(g, w), (what, kind, seed, base)
        assert (sh.n_seqs, sh.n_bases) == (len(seqs), sum(len(s) for s in seqs))
        return want
    finally:
        if sh is not None:
            sh.close()
        if source is None:
            sq.close()


def rand_run(rng, n, letters=4):
    return "".join(rng.choice(list("ACGT"[:letters]), size=n).tolist()) if n else ""


@pytest.mark.parametrize("kind", KINDS)
def test_hand_written_set(kind):
    want = check_against_host(sc.HAND_SET, kind, 7)
    if kind == "dinuc":
        assert want[0] == sc.VECTORS[1][3]
    for s, w in zip(sc.HAND_SET, want):
        sc.check_properties(s, w, kind)
    times = _lib.shuffle_stage_ms()
    assert times.shape == (4,) and (times >= 0).all() and times.sum() > 0


@pytest.mark.parametrize("kind", KINDS)
def test_runs_either_side_of_the_tiers(dims, kind):
    rng = np.random.default_rng(31)
    sizes = sorted({dims[k] + d for k in ("lane_run", "lds_run") for d in (-1, 0, 1)})
    seqs = [rand_run(rng, n) for n in sizes] + ["N" + rand_run(rng, n) + "n" + rand_run(rng, 5) for n in sizes]
    want = check_against_host(seqs, kind, 123)
    assert sum(a.upper() != b for a, b in zip(seqs, want)) == len(seqs)


@pytest.mark.parametrize("kind", KINDS)
def test_long_run_through_the_global_path(dims, kind):
    rng = np.random.default_rng(32)
    n = 3 * dims["lds_run"] + 5
    seqs = ["ACGTN", rand_run(rng, n), "TTGCA"]
    want = check_against_host(seqs, kind, 5, base=17)
    sc.check_properties(seqs[1], want[1], kind)
    assert want[1] != seqs[1]


@pytest.mark.parametrize("kind", KINDS)
def test_low_complexity_runs_on_both_paths(dims, kind):
    t = dims["lds_run"]
    seqs = ["A" * (t - 1) + "C", "AC" * ((t - 2) // 2) + "G", "A" * (t + 50) + "C", "AC" * (t // 2 + 10) + "G", "A" * 50 + "C" * 50 + "A" * 50,
            "AC" * (t // 2 + 20) + "GT" * 30 + "AC" * 30]
    want = check_against_host(seqs, kind, 77)
    for s, w in zip(seqs, want):
        sc.check_properties(s, w, kind)


@pytest.mark.parametrize("kind", KINDS)
def test_every_phase_of_a_unit(kind):
    rng = np.random.default_rng(33)
    seqs = [sc.random_sequence(rng, 33, 4, 0.05) for _ in range(34)]          # sequence k starts at phase k mod 32
    check_against_host(seqs, kind, 1)
    seqs = [sc.random_sequence(rng, 31, 4, 0.0) for _ in range(34)]
    check_against_host(seqs, kind, 2)


@pytest.mark.parametrize("kind", KINDS)
def test_tiny_sequences_share_units(kind):
    rng = np.random.default_rng(34)
    seqs = [rand_run(rng, 1 + k % 2) for k in range(90)]                       # more than 32 sequences in one 32-base unit
    seqs[10], seqs[11], seqs[40] = "", "N", "n"
    check_against_host(seqs, kind, 3)
    check_against_host([rand_run(rng, 1) for _ in range(70)], kind, 4)


@pytest.mark.parametrize("kind", KINDS)
def test_block_and_unit_edges(dims, kind):
    rng = np.random.default_rng(35)
    bb = dims["block_bases"]
    # a sequence (one run) that straddles the block edge; its neighbours end a run exactly on the edge / one base past it
    seqs = [sc.random_sequence(rng, bb - 7, 4, 0.3), rand_run(rng, 20), rand_run(rng, 19), sc.random_sequence(rng, bb - 32, 4, 0.3), rand_run(rng, 1)]
    check_against_host(seqs, kind, 8)
    seqs = [sc.random_sequence(rng, bb - 40, 4, 0.3), rand_run(rng, 40), rand_run(rng, 41)]      # a run that ends on the block edge, the next starts there
    check_against_host(seqs, kind, 9)
    # runs that end exactly on a unit edge and one base past it, inside a sequence and at its end
    seqs = [rand_run(rng, 32), rand_run(rng, 33), rand_run(rng, 31), rand_run(rng, 20) + "N" + rand_run(rng, 11) + "N" + rand_run(rng, 32) + "NN", rand_run(rng, 64)]
    check_against_host(seqs, kind, 10)


@pytest.mark.parametrize("kind", KINDS)
def test_empty_all_n_and_alternating(kind):
    check_against_host(["", "", "ACGTAC", "", "", "GGTCA", ""], kind, 1)
    check_against_host([], kind, 1)
    check_against_host([""], kind, 1)
    check_against_host(["", ""], kind, 1)
    check_against_host(["NNNNNNN"], kind, 1)
    check_against_host(["N" * 70, "n" * 3], kind, 1)
    check_against_host(["AN" * 40, "NA" * 40 + "CG", "ACN" * 30], kind, 1)


@pytest.mark.parametrize("kind", KINDS)
def test_shards_get_the_bytes_of_the_whole(kind):
    rng = np.random.default_rng(36)
    seqs = [sc.random_sequence(rng, int(n), 4, 0.02) for n in rng.integers(0, 200, size=30)]
    whole = check_against_host(seqs, kind, 2024)
    a = check_against_host(seqs[:13], kind, 2024, base=0)
    b = check_against_host(seqs[13:], kind, 2024, base=13)
    assert a + b == whole
    assert check_against_host(seqs[13:], kind, 2024, base=0) != whole[13:]


@pytest.mark.parametrize("kind", KINDS)
def test_sets_cut_from_a_genome_and_a_personal_genome(kind):
    rng = np.random.default_rng(37)
    chroms = {"c0": sc.random_sequence(rng, 700, 4, 0.01).upper(), "c1": sc.random_sequence(rng, 500, 4, 0.0)}
    g = _lib.ResidentGenome(chroms)
    try:
        ci, lo, hi = [0, 1, 0, 1, 0], [5, 0, 100, 498, 650], [205, 150, 400, 499, 700]
        names = list(chroms)
        cut = g.extract(ci, lo, hi)
        try:
            check_against_host([chroms[names[c]][a:b] for c, a, b in zip(ci, lo, hi)], kind, 4, source=cut)
        finally:
            cut.close()
        check_against_host([chroms[n] for n in names], kind, 5, source=g)                      # the genome itself: its chromosomes are the sequences
        alt, lm = _lib.apply_alleles(g, [0, 0, 1], [10, 300, 20], [1, 4, 0], ["GGG", "", "TTAC"])
        try:
            spliced = [alt.fetch_sequence(n, 0, alt.chrom_sizes[n]) for n in names]
            assert [len(s) for s in spliced] == [700 + 2 - 4, 500 + 4]
            check_against_host(spliced, kind, 6, source=alt)
            cut = alt.extract([0, 1], [3, 10], [333, 504])
            try:
                check_against_host([spliced[0][3:333], spliced[1][10:504]], kind, 6, base=2, source=cut)
            finally:
                cut.close()
        finally:
            lm.close()
            alt.close()
    finally:
        g.close()


def test_argument_checks():
    L = _lib.lib()
    sq = _lib.SeqSet.from_strings(["ACGTACGT"])
    try:
        out = ctypes.c_void_p()
        call = lambda kind, base, flags: L.ms_seqset_shuffle(sq.h, kind, 0, base, flags, ctypes.byref(out))
        for kind in (0, 3, -1):
            assert call(kind, 0, 0) == _lib.MS_ERR_INVALID and not out.value
        assert call(2, 0, 1) == _lib.MS_ERR_INVALID and not out.value
        assert call(1, -1, 0) == _lib.MS_ERR_INVALID and not out.value
        assert L.ms_seqset_shuffle(sq.h, 2, 0, 0, 0, None) == _lib.MS_ERR_INVALID
        assert L.ms_seqset_shuffle(None, 2, 0, 0, 0, ctypes.byref(out)) == _lib.MS_ERR_INVALID
        with pytest.raises(ValueError):
            sq.shuffled("trinuc", 0)
        assert call(2, 2 ** 40, 0) == _lib.MS_OK and out.value                               # any index base >= 0 is valid
        L.ms_seqset_free(out)
        big = sq.shuffled("mono", 2 ** 64 - 1)                                                # the whole range of seeds
        try:
            assert big.to_strings() == shuffle.shuffle_host(["ACGTACGT"], "mono", 2 ** 64 - 1)
        finally:
            big.close()
    finally:
        sq.close()


def test_packed_host_round_trips_against_the_debug_planes():
    rng = np.random.default_rng(38)
    seqs = [sc.random_sequence(rng, int(n), 4, 0.1) for n in (0, 5, 64, 97, 1, 300)]
    sq = _lib.SeqSet.from_strings(seqs)
    try:
        codes, nmask = sq.packed_host()
        dev = _lib.seqset_planes(sq)
        assert np.array_equal(codes, dev[0]) and np.array_equal(nmask, dev[1])
        assert sq.to_strings() == [as_packed_text(s) for s in seqs]
    finally:
        sq.close()
    empty = _lib.SeqSet.from_strings([])
    try:
        assert empty.to_strings() == [] and empty.packed_host()[0].size == 0
    finally:
        empty.close()
    assert _lib.lib().ms_seqset_packed_host(None, None, None) == _lib.MS_ERR_INVALID


def seeded_matrix(width, seed):
    rng = np.random.default_rng(seed)
    ppm = rng.dirichlet(np.full(4, 0.4), size=width).T
    return np.round(np.log((ppm + 0.01) / 1.04 / 0.25), 5)


@pytest.mark.parametrize("kind", KINDS)
def test_scan_entry_points_take_the_shuffled_set_as_it_is(kind):
    rng = np.random.default_rng(39)
    seqs = [sc.random_sequence(rng, int(n), 4, 0.03) for n in (180, 0, 7, 333, 64, 1200, 12)]
    mats = [seeded_matrix(w, 100 + w) for w in (5, 8, 13, 21)]
    pw = _lib.PwmSet.from_matrices(mats, [0.55] * len(mats))
    src = _lib.SeqSet.from_strings(seqs)
    dev = src.shuffled(kind, 99)
    host = _lib.SeqSet.from_strings(shuffle.shuffle_host(seqs, kind, 99))
    try:
        ra, rb = _lib.scan(pw, dev, 3), _lib.scan(pw, host, 3)
        try:
            ha, hb = ra.hits(), rb.hits()
            assert set(ha) == set(hb) and ha["score"].size > 0
            for k in ha:
                assert np.array_equal(ha[k], hb[k]), k
        finally:
            ra.close()
            rb.close()
        ba, bb = _lib.scan_best(pw, dev, 3), _lib.scan_best(pw, host, 3)
        try:
            for x, y in zip(ba.sites(), bb.sites()):
                assert np.array_equal(x, y, equal_nan=True)
        finally:
            ba.close()
            bb.close()
        aa, ab, a0 = _lib.scan_affinity(pw, dev, 3), _lib.scan_affinity(pw, host, 3), _lib.scan_affinity(pw, src, 3)
        try:
            ca, cb, c0 = aa.cells(), ab.cells(), a0.cells()
            for x, y in zip(ca, cb):
                assert np.array_equal(x, y, equal_nan=True)
            assert np.array_equal(ca[2], c0[2]) and ca[2].dtype == np.int32                   # n_terms: the input's count of windows
            amax, amax0 = _lib.scan_affinity(pw, dev, 3, max_n=0), _lib.scan_affinity(pw, src, 3, max_n=0)
            try:
                assert np.array_equal(amax.cells()[2], amax0.cells()[2])                      # ... and of windows without a non-ACGT base
            finally:
                amax.close()
                amax0.close()
        finally:
            aa.close()
            ab.close()
            a0.close()
        hist = [_lib.score_histogram(pw, s, 3, 0.0, 1.0, 64) for s in (dev, host, src)]
        assert np.array_equal(hist[0], hist[1])
        assert np.array_equal(hist[0].sum(axis=1), hist[2].sum(axis=1))                       # the same windows, other scores
    finally:
        for h in (pw, src, dev, host):
            h.close()


def test_scanner_shuffled_is_a_control():
    rng = np.random.default_rng(40)
    mats = [seeded_matrix(w, 200 + w) for w in (8, 10, 12)]
    planted = "".join("ACGT"[int(c)] for c in mats[1].argmax(axis=0))
    seqs = []
    for _ in range(120):
        s = rand_run(rng, 100)
        at = int(rng.integers(0, 100 - len(planted)))
        seqs.append(s[:at] + planted + s[at + len(planted):])
    seqs[3] = seqs[3][:50] + "NNnN" + seqs[3][54:]

    class Genome:
        chrom_sizes = {"chr1": 100 * len(seqs)}

        def fetch_sequence(self, chrom, start, end):
            return seqs[start // 100]

    class Region:
        def __init__(self, k):
            self.chrom, self.start, self.end, self.summit = "chr1", 100 * k, 100 * k + 100, 100 * k + 50

    class Pwm:
        def __init__(self, matrix):
            self.matrix, self.length, self.cutoffs = matrix, matrix.shape[1], {"1e-4": 0.8}

    pwms = [Pwm(m) for m in mats]
    a = scanner.Scanner(Genome(), [Region(k) for k in range(len(seqs))], strand="+", p_value="1e-4", remove_dup=False)
    ctrl = a.shuffled("mono", seed=1)
    di = a.shuffled(seed=2)
    try:
        assert ctrl._resident is None and ctrl.seq_starts is a.seq_starts and ctrl.seq_ends is a.seq_ends
        assert (ctrl.strand, ctrl.p_value, ctrl.remove_dup) == ("+", "1e-4", False)
        assert list(ctrl.sequences) == [as_packed_text(s) for s in shuffle.shuffle_host(seqs, "mono", 1)]
        assert list(di.sequences) == [as_packed_text(s) for s in shuffle.shuffle_host(seqs, "dinuc", 2)]
        rs = a.rank_sum(pwms, control=ctrl)
        assert (rs.na, rs.nb) == (len(seqs), len(seqs))
        assert rs.auroc()[1] > 0.5 and rs.auroc()[1] > 0.9                                    # the planted motif stands out against its own shuffle
        # the same numbers as against a scanner made of the restatement's strings
        host_seqs = shuffle.shuffle_host(seqs, "mono", 1)

        class HostGenome(Genome):
            def fetch_sequence(self, chrom, start, end):
                return host_seqs[start // 100]

        b = scanner.Scanner(HostGenome(), [Region(k) for k in range(len(seqs))], strand="+", remove_dup=False)
        try:
            want = a.rank_sum(pwms, control=b)
            assert np.array_equal(rs.u2, want.u2) and rs.ties == want.ties
            got, ref = a.affinity_rank_sum(pwms, ctrl), a.affinity_rank_sum(pwms, b)
            assert np.array_equal(got.u2, ref.u2)
            assert np.array_equal(ctrl.best_sites(pwms).score, b.best_sites(pwms).score, equal_nan=True)
            assert np.array_equal(ctrl.score_histogram(pwms, n_bins=32).counts, b.score_histogram(pwms, n_bins=32).counts)
            sa, sb = ctrl.scan_motifs(pwms), b.scan_motifs(pwms)
            assert [[[(s.start, s.score, s.strand) for s in reg] for reg in mot] for mot in sa] == \
                   [[[(s.start, s.score, s.strand) for s in reg] for reg in mot] for mot in sb]
        finally:
            b.close()
    finally:
        a.close()
        ctrl.close()
        di.close()


def test_seeded_family_around_the_dims(dims):
    """40 random sets: run lengths drawn around the tile size and far below it, N at 0, 1 % or 30 %, both kinds, random seeds and bases"""
    rng = np.random.default_rng(41)
    t = dims["lds_run"]
    for case in range(40):
        dirt = (0.0, 0.01, 0.3)[case % 3]
        n_seqs = int(rng.integers(1, 7))
        lens = []
        for _ in range(n_seqs):
            pick = rng.integers(0, 4)
            lens.append(int(rng.integers(0, 40)) if pick == 0 else int(rng.integers(40, 400)) if pick == 1
                        else int(rng.integers(t - 40, t + 40)) if pick == 2 else int(rng.integers(t + 1, 2 * t + 100)))
        if sum(lens) > 6000:
            lens = lens[:2]
        seqs = [sc.random_sequence(rng, n, int(rng.integers(1, 5)), dirt) for n in lens]
        kind = KINDS[case % 2]
        want = check_against_host(seqs, kind, int(rng.integers(0, 2 ** 63)), base=int(rng.integers(0, 1000)))
        for s, w in zip(seqs, want):
            sc.check_properties(s, w, kind)
