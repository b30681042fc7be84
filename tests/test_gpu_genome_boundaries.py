"""
The kernels either side of the scan on their own boundaries -- pack_kernel / blk2reg_kernel / extract_kernel (ms_seqset.hip), base_count_kernel /
window_flag_kernel / window_take_kernel (ms_background.hip), score_kernel / gather_ranks_kernel and ms_score_ranks' batches (ms_pwmset.hip).
Every boundary size comes from ms_debug_genome_dims (_lib.genome_dims), so the cases follow the constants if one moves; the device's
planes and region hints are read back with ms_debug_seqset_planes and compared with the host packer (held against the oracle's
convert_seq by tests/test_genome.py and tests/test_fuzz_cases_host.py), counts with numpy, windows with byte counts, scores with the oracle.
Everything is exact.  tests/fuzz_parity.py --genome runs the same comparisons over seeded cases.  Run with -m gpu.
"""
import numpy as np
import pytest

import fuzz_parity as fp
from motifscan_amd import _lib

pytestmark = pytest.mark.gpu
# the sizes of the parametrised cases, in units of the library's constants (read when a test runs, not when the module is collected)
SIZES = {"0": lambda u: 0, "1": lambda u: 1, "31": lambda u: 31, "32": lambda u: 32, "33": lambda u: 33, "63": lambda u: 63, "64": lambda u: 64,
         "65": lambda u: 65, "unit-1": lambda u: u - 1, "unit": lambda u: u, "unit+1": lambda u: u + 1, "2units+1": lambda u: 2 * u + 1,
         "3units+1": lambda u: 3 * u + 1}


def dims():
    return _lib.genome_dims()


def size(name, unit):
    """The size a parametrised case names, `unit` being the key of the library constant it is counted in."""
    return SIZES[name](dims()[unit])


@pytest.fixture(scope="module", autouse=True)
def _device():
    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible")
    _lib.set_device(0)


def genome_of(parts):
    return _lib.ResidentGenome({f"c{i}": p for i, p in enumerate(parts)})


def split(a, offsets):
    return [a[offsets[i]:offsets[i + 1]] for i in range(len(offsets) - 1)]


# ------------------------------------------------------------------------------------------------ pack

@pytest.mark.parametrize("total", ["0", "1", "31", "32", "33", "63", "64", "65", "unit-1", "unit", "unit+1"])
def test_packed_planes_and_region_hints_equal_the_host_packer(total):
    total = size(total, "pack_block_bases")
    assert total in fp.pack_totals(dims())
    rng = np.random.default_rng(total)
    a = fp.genome_bytes(rng, total, all_bytes=True)
    for n_seqs in (1, 2, 5):
        offsets = fp.random_offsets(rng, total, n_seqs)
        g = genome_of(split(a, offsets))
        try:
            got = _lib.seqset_planes(g)
        finally:
            g.close()
        assert fp.planes_differ(got, _lib.host_pack(a, offsets)) is None, (total, n_seqs)
        assert fp.plane_invariants_broken(got[0], got[1], total) is None, (total, n_seqs)


def test_sets_of_empty_sequences_and_of_none():
    for offsets in (np.zeros(5, dtype=np.int64), np.zeros(1, dtype=np.int64)):
        g = genome_of([np.zeros(0, dtype=np.uint8)] * (len(offsets) - 1))
        try:
            codes, nmask, blk2reg, blkinfo = _lib.seqset_planes(g)
            assert g.base_counts().shape == (len(offsets) - 1, 4) and not g.base_counts().any()
        finally:
            g.close()
        assert codes.size == 0 and nmask.size == 0
        assert fp.planes_differ((codes, nmask, blk2reg, blkinfo), _lib.host_pack(np.zeros(0, dtype=np.uint8), offsets)) is None
        assert len(blk2reg) == 1 and (len(offsets) > 1 or (blk2reg.tolist() == [0] and blkinfo.tolist() == [[0, 0, 0, 0]]))


def test_ascii_at_every_unaligned_device_address_plane_for_plane():
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(5)
    for total in (33, 65, dims()["pack_block_bases"] + 1):
        a = fp.genome_bytes(rng, total, all_bytes=True)
        offsets = fp.random_offsets(rng, total, 3)
        want = _lib.host_pack(a, offsets)
        t = torch.zeros(total + 32, dtype=torch.uint8, device="cuda:0")
        for shift in range(0, 16):                      # 0: the aligned 16-byte loads; 1 .. 15: the byte loads
            t[shift:shift + total] = torch.from_numpy(a).to("cuda:0")
            torch.cuda.synchronize()
            sq = _lib.SeqSet.from_device(t.data_ptr() + shift, offsets)
            try:
                assert fp.planes_differ(_lib.seqset_planes(sq), want) is None, (total, shift)
            finally:
                sq.close()


# ------------------------------------------------------------------------------------------------ extract

LENS = [0, 700, 1, 33, 64, 1500, 0, 900, 31, 2500, 0]


@pytest.fixture(scope="module")
def small_genome():
    rng = np.random.default_rng(17)
    goff = np.concatenate([[0], np.cumsum(LENS)]).astype(np.int64)
    bases = fp.genome_bytes(rng, int(goff[-1]), all_bytes=True)
    g = genome_of(split(bases, goff))
    yield bases, goff, g
    g.close()


def extracted(g, regions):
    reg = np.array(regions, dtype=np.int64).reshape(-1, 3)
    sq = g.extract(reg[:, 0], reg[:, 1], reg[:, 2])
    try:
        return _lib.seqset_planes(sq)
    finally:
        sq.close()


def assert_extraction(small_genome, regions):
    bases, goff, g = small_genome
    cut, offsets = fp.packed_cut(bases, goff, regions)
    got = extracted(g, regions)
    assert fp.planes_differ(got, _lib.host_pack(cut, offsets)) is None
    assert fp.plane_invariants_broken(got[0], got[1], len(cut)) is None
    return offsets


@pytest.mark.parametrize("tail", [0, 1, 2])
def test_every_source_phase_meets_every_output_phase(small_genome, tail):
    """fuzz_parity.extract_regions: regions of 0 .. 70 bases until all 32 x 32 (source, output) phases occurred, boundaries on the
    extract block's edges, the output one base short of a multiple of the block, on it, and one base over."""
    bases, goff, g = small_genome
    BLK = dims()["pack_block_bases"]
    regions = fp.extract_regions(np.random.default_rng(100 + tail), LENS, BLK, tail)
    offsets = assert_extraction(small_genome, regions)
    reg = np.array(regions, dtype=np.int64)
    ne = reg[:, 2] > reg[:, 1]
    table = np.zeros((32, 32), dtype=np.int64)
    np.add.at(table, ((goff[reg[:, 0]] + reg[:, 1])[ne] % 32, offsets[:-1][ne] % 32), 1)
    assert table.min() >= 1 and (offsets[-1] + 1) % BLK == tail
    assert {int(BLK - 1), int(BLK), int(BLK + 1)} <= set(offsets.tolist())


def test_more_than_32_regions_in_one_output_unit(small_genome):
    rng = np.random.default_rng(3)
    regions = [(1, 10, 42)]                                  # 32 bases: the next unit starts a region
    for k in range(32):                                      # 32 one-base regions of four chromosomes and 32 empty ones in one unit
        c = (1, 5, 7, 9)[k % 4]
        a = int(rng.integers(0, LENS[c]))
        regions += [(c, a, a + 1), (c, a, a)]
    regions += [(2, 0, 1)] * 40                              # 40 one-base regions: a unit and a quarter
    regions += [(9, LENS[9], LENS[9])] * 40 + [(0, 0, 0)] * 3 + [(5, 0, 0)]      # 44 empty ones in a row, on an empty chromosome too
    regions += [(3, 0, 33), (9, LENS[9] - 70, LENS[9]), (8, 30, 31), (4, 63, 64)]   # ... ending on a chromosome's and the genome's last base
    offsets = assert_extraction(small_genome, regions)
    assert np.bincount(offsets[:-1] // 32).max() > 32


@pytest.mark.parametrize("n_out", ["unit-1", "unit", "unit+1"])
def test_output_across_the_extract_block(small_genome, n_out):
    n_out = size(n_out, "pack_block_bases")
    regions, left, k = [], n_out, 0
    while left:
        c = (9, 5, 7, 1)[k % 4]
        n = min(left, LENS[c] - k % 7, 61 + k % 10)
        regions.append((c, k % 7, k % 7 + n))
        left -= n
        k += 1
    offsets = assert_extraction(small_genome, regions)
    assert offsets[-1] == n_out
    assert_extraction(small_genome, [])
    assert_extraction(small_genome, [(5, 3, 3)])


# ------------------------------------------------------------------------------------------------ base counts

def assert_counts(parts):
    g = genome_of(parts)
    try:
        got = g.base_counts()
    finally:
        g.close()
    want = np.array([[np.count_nonzero((p | 0x20) == ord(b)) for b in "acgt"] for p in parts], dtype=np.int64).reshape(len(parts), 4)
    assert np.array_equal(got, want), np.flatnonzero((got != want).any(axis=1))[:8]


@pytest.mark.parametrize("n_bases", ["unit-1", "unit", "unit+1", "2units+1"])
@pytest.mark.parametrize("clustered", [True, False])
def test_base_counts_at_the_tile_sizes(n_bases, clustered):
    """fuzz_parity.count_genome: LDS + 1 or more short chromosomes in the first tile (or short ones behind LDS empty ones), ends on every
    bit of a unit, an end on a tile edge and a chromosome across one, an all-N and a lower-case chromosome, empty ones at both ends."""
    TILE, LDS, n_bases = dims()["count_tile_bases"], dims()["lds_chroms"], size(n_bases, "count_tile_bases")
    rng = np.random.default_rng(n_bases + clustered)
    lens, a = fp.count_genome(rng, n_bases, TILE, LDS, clustered, True)
    t = fp.count_tally(lens, dims())
    assert t["global_by_nonempty" if clustered else "global_by_empty"] > 0 and t["lds_path"] > 0 and t["leading_empty"] and t["trailing_empty"]
    assert not clustered or t["end_bits"].min() > 0
    assert n_bases <= TILE or t["end_on_tile_edge"] + t["straddles_tile_edge"] > 0
    assert_counts(split(a, np.concatenate([[0], np.cumsum(lens)])))


def test_base_counts_with_a_chromosome_end_on_every_bit_and_past_the_lds_counters():
    rng, LDS = np.random.default_rng(9), dims()["lds_chroms"]
    for lens in ([33] * (2 * LDS + 3),                                       # more non-empty chromosomes than LDS counters, ends on every bit
                 [1] * (LDS + 1), [1] * LDS, [1] * (LDS - 1),                # one past the counters, exactly as many, one fewer
                 [7] + [0] * LDS + [9] + [0] * (LDS - 1) + [11, 0, 0],       # index LDS + 1 reached by empty chromosomes alone; the next at index 2 LDS + 1
                 [0, 0, 31, 1, 32, 0, 64, 0],
                 [5] * LDS + [0, 6]):                                        # an empty chromosome pushes the last one past the counters
        a = fp.genome_bytes(rng, sum(lens))
        assert_counts(split(a, np.concatenate([[0], np.cumsum(lens)])))
    for n in (1, 31, 32, 33):                                                # a last unit of 1 and of 31 bases; all N; lower case only
        assert_counts([np.full(n, ord("N"), dtype=np.uint8), np.frombuffer(b"acgtn" * 13, dtype=np.uint8)[:n]])


def test_base_counts_with_ends_either_side_of_a_tile_edge():
    rng, TILE = np.random.default_rng(10), dims()["count_tile_bases"]
    for first in (TILE - 1, TILE, TILE + 1, TILE - 31, TILE + 31):
        lens = [first, 3, 40, 0, 77]
        a = fp.genome_bytes(rng, sum(lens))
        assert_counts(split(a, np.concatenate([[0], np.cumsum(lens)])))


# ------------------------------------------------------------------------------------------------ the window filter

def filter_reference(raw, gstart, length, max_n, n_want):
    ok = [k for k, g in enumerate(gstart) if raw[g:g + length].count(b"N") + raw[g:g + length].count(b"n") <= max_n]
    return ok[:n_want], len(ok)


def exceptions_of(raw):
    return np.array([i for i, x in enumerate(raw) if chr(x) not in "ACGTacgtNn"], dtype=np.int64)


@pytest.mark.parametrize("length", fp.FILTER_LENGTHS)
def test_window_filter_with_exceptions_on_both_window_ends(length):
    """A genome of A with N N R N N at one place: windows whose ends sit on, before and behind the R, at every start phase; counts of
    exactly max_n and max_n + 1; windows that pass only because the R is no N."""
    raw = bytearray(b"A" * 700)
    for p in (200, 361):                                # at bit 8 and at bit 9 of their units
        raw[p - 2:p + 3] = b"NnRNN"
    raw[695:700] = b"NRNAN"                             # ... and on the genome's last bases
    raw = bytes(raw)
    g = genome_of([np.frombuffer(raw, dtype=np.uint8)[:300], np.frombuffer(raw, dtype=np.uint8)[300:]])
    try:
        exc = exceptions_of(raw)
        starts = sorted({s for p in (200, 361, 696) for e in (p + 1, p, p - length + 1, p - length) for s in range(e - 3, e + 4)
                         if 0 <= s <= len(raw) - length} | set(range(150, 182)) | {len(raw) - length, 0})
        assert {s % 32 for s in starts} == set(range(32))
        for max_n in (0, 1, 2, 3, 4, length, length + 7):
            for n_want in (1, len(starts) + 5):
                want, acc = filter_reference(raw, starts, length, max_n, n_want)
                assert _lib.window_filter(g, starts, length, max_n, exc, n_want).tolist() == want, (length, max_n, n_want)
            counts = {raw[s:s + length].count(b"N") + raw[s:s + length].count(b"n") for s in starts}
            assert length < 31 or max_n > 3 or {max_n, max_n + 1} <= counts      # windows sit on both sides of max_n
        # without the exception list the R counts as an N: the windows that pass only because it is none are the difference
        max_n = 2 if length >= 3 else 0
        want, _ = filter_reference(raw, starts, length, max_n, len(starts))
        blind = _lib.window_filter(g, starts, length, max_n, np.zeros(0, dtype=np.int64), len(starts)).tolist()
        assert set(blind) < set(want)
    finally:
        g.close()


@pytest.mark.parametrize("n_cand", ["1", "63", "64", "65", "unit-1", "unit", "unit+1", "3units+1"])
def test_window_take_on_the_wave_and_block_edges(n_cand):
    n_cand = size(n_cand, "filter_threads")
    rng = np.random.default_rng(n_cand)
    a = fp.genome_bytes(rng, 5000)
    raw = a.tobytes()
    g = genome_of([a[:1234], a[1234:]])
    try:
        exc = exceptions_of(raw)
        starts = rng.integers(0, len(raw) - 33 + 1, size=n_cand).tolist()
        starts[-1] = len(raw) - 33
        for max_n in (0, 1, 33):
            _, acc = filter_reference(raw, starts, 33, max_n, n_cand)
            for n_want in sorted({1, max(1, acc - 1), max(1, acc), acc + 1, n_cand + 1}):
                want, _ = filter_reference(raw, starts, 33, max_n, n_want)
                assert _lib.window_filter(g, starts, 33, max_n, exc, n_want).tolist() == want, (n_cand, max_n, n_want, acc)
        inside = [2000] * n_cand                        # all rejected, all accepted
        run = bytearray(raw)
        run[1990:2100] = b"N" * 110
        g2 = genome_of([np.frombuffer(bytes(run), dtype=np.uint8)])
        try:
            assert _lib.window_filter(g2, inside, 33, 32, exceptions_of(bytes(run)), n_cand).size == 0
            assert _lib.window_filter(g2, inside, 33, 33, exceptions_of(bytes(run)), n_cand).tolist() == list(range(n_cand))
        finally:
            g2.close()
    finally:
        g.close()


# ------------------------------------------------------------------------------------------------ scores and ranks

def test_score_ranks_do_not_depend_on_the_batch(oracle):
    """ms_score by bits for the three strand masks over windows cut on the device at odd phases, sequences shorter than the motif and
    empty ones among them; ms_score_ranks against the sorted oracle row with the library's budget, with batches of one motif and of three
    (P = 11), the three results the same bytes; ranks -1 and R give NaN."""
    rng = np.random.default_rng(21)
    lens = [900, 0, 40, 1300]
    goff = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    bases = fp.genome_bytes(rng, int(goff[-1]))
    mats = []
    for w in list(fp.RANK_WIDTHS) + [5, 17, 40]:
        m = fp.random_matrix(rng, w)
        while fp.max_raw_of(m) == 0:
            m = fp.random_matrix(rng, w)
        mats.append(m)
    regions = [(0, a, a + 70) for a in range(0, 640, 3)] + [(3, a, a + int(n)) for a, n in zip(range(1, 1200, 11), rng.integers(0, 101, size=200))]
    regions += [(1, 0, 0), (2, 39, 40), (2, 0, 40), (0, 5, 5)]
    raw, soff = fp.packed_cut(bases, goff, regions)
    vals, widths = oracle.flatten_pwms(mats)
    R, P = len(regions), len(mats)
    assert P % 3 and dims()["rank_budget"] // R >= P
    reg = np.array(regions, dtype=np.int64)
    g = genome_of(split(bases, goff))
    pw = _lib.PwmSet.from_matrices(mats)
    sq = g.extract(reg[:, 0], reg[:, 1], reg[:, 2])
    try:
        want = {s: oracle.score_arrays(vals, widths, raw.tobytes(), soff, s) for s in (1, 2, 3)}
        for s in (1, 2, 3):
            assert fp.same_bits(_lib.score(pw, sq, s), want[s]), s
        ranks = np.array([0, int(R * 0.1) - 1, int(R * 0.01) - 1, int(R * 0.1 ** 5) - 1, R - 1, -1, R], dtype=np.int64)
        assert ranks[3] == -1
        runs = {}
        for budget in (0, R, 3 * R + 2):
            prev = _lib.score_rank_budget(budget)
            try:
                runs[budget] = _lib.score_ranks(pw, sq, ranks, 3)
            finally:
                assert _lib.score_rank_budget(prev) == budget
        assert runs[0].tobytes() == runs[R].tobytes() == runs[3 * R + 2].tobytes()
        for p in range(P):
            desc = sorted(want[3][p].tolist(), reverse=True)
            assert fp.same_bits(runs[0][p, [0, 1, 2, 4]], [desc[int(r)] for r in ranks[[0, 1, 2, 4]]]), p
        assert np.isnan(runs[0][:, [3, 5, 6]]).all()
    finally:
        sq.close()
        pw.close()
        g.close()
