"""
ms_scan_variants (ms_variants.hip) on the GPU: the motif sites single-base substitutions create and destroy on a resident genome --
against the pinned oracle at the smallest shapes that can go wrong, against the project's own scan of the two alleles' flanks at
moderate size, for its order / determinism / chunking, its validation, and through motifscan_amd.variants with a VCF.
"""
import numpy as np
import pytest

from motifscan_amd import _lib, synth, variants
from variant_cases import expected_snv_records as expected_records, n_windows, seeded_matrix, snv_flank_table

pytestmark = pytest.mark.gpu

ALL_PASS = -1e30


@pytest.fixture(scope="module", autouse=True)
def _device():
    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible")
    _lib.set_device(0)


def sites_of(res):
    s = res.sites()
    res.close()
    return s


# ------------------------------------------------------------------------------------------------ 1. the oracle, smallest shapes

WIDTHS = (1, 4, 6, 19, 33, 64, 70)
ALTS = "ACGTNt"


@pytest.fixture(scope="module")
def small(oracle, rnd):
    rng = np.random.default_rng(20240917)
    chroms = {}
    for name, n in (("c5", 5), ("c40", 40), ("c97", 97)):
        chroms[name] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)].copy()
    c97 = chroms["c97"]
    c97[15:30] = ord("N")                               # an N run across a word boundary of the packed genome (bases 60 .. 74 of it)
    c97[50:63] = np.frombuffer(bytes(c97[50:63]).lower(), dtype=np.uint8)
    c97[80] = ord("R")                                  # one IUPAC letter
    c40 = chroms["c40"]
    c40[3:12] = np.frombuffer(bytes(c40[3:12]).lower(), dtype=np.uint8)
    chroms["c5"][2] = ord("n")
    chroms = {k: v.tobytes() for k, v in chroms.items()}
    names = list(chroms)
    lens = np.array([len(chroms[n]) for n in names])

    by_width = {int(w): rnd["mats"][i] for i, w in reversed(list(enumerate(rnd["widths"])))}
    mats = [np.array(by_width[w]) if w in by_width else seeded_matrix(w, 100 + w) for w in WIDTHS]
    mats[1][0, 2] = -np.inf                             # the width-4 motif: A at column 2 and T at column 0 can never be part of a site
    mats[1][3, 0] = -np.inf

    chrom_idx = np.repeat(np.arange(3), lens).astype(np.int32)
    pos = np.concatenate([np.arange(n) for n in lens]).astype(np.int64)
    V0 = len(pos)                                       # 142 positions x 6 alts
    chrom_idx, pos = np.tile(chrom_idx, len(ALTS)), np.tile(pos, len(ALTS))
    alt = np.repeat(np.frombuffer(ALTS.encode(), dtype=np.uint8), V0)

    # every window that covers a variant, scored by the oracle on the ref and on the alt flank [x - W + 1, x + W) clipped to the chromosome
    table = snv_flank_table(oracle, chroms, names, mats, chrom_idx, pos, alt)

    quant = []
    for t in table:
        finite = t["ref"][np.isfinite(t["ref"])]
        quant.append(float(np.quantile(finite, 0.9)))
    genome = _lib.ResidentGenome(chroms)
    yield {"genome": genome, "chroms": chroms, "names": names, "mats": mats, "chrom_idx": chrom_idx, "pos": pos, "alt": alt, "table": table,
           "cutoffs": {"q90": np.array(quant), "all": np.full(len(mats), ALL_PASS), "none": np.full(len(mats), 2.0)}, "lens": lens}
    genome.close()


@pytest.mark.parametrize("strand_mask", [1, 2, 3])
@pytest.mark.parametrize("which", ["q90", "all", "none"])
def test_records_equal_the_oracle(small, oracle, which, strand_mask):
    cutoffs = small["cutoffs"][which]
    pw = _lib.PwmSet.from_matrices(small["mats"], cutoffs)
    res = _lib.scan_variants(pw, small["genome"], small["chrom_idx"], small["pos"], small["alt"], strand_mask)
    ref_codes = res.ref_codes()
    got = sites_of(res)
    pw.close()
    want, offsets = expected_records(small["table"], cutoffs, strand_mask)
    print(f"{which} strands {strand_mask}: {len(got['state'])} records, expected {offsets[-1]}; states {np.bincount(got['state'], minlength=4).tolist()}")
    assert np.array_equal(got["motif_offsets"], offsets)
    for k in ("variant", "start", "strand", "state"):
        assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(got["score_ref"], want["score_ref"]) and np.array_equal(got["score_alt"], want["score_alt"])
    if which == "none":
        assert offsets[-1] == 0
    if which == "all":                                  # nothing is lost, however dense: every window x strand with a finite score
        n_strands = bin(strand_mask).count("1")
        L = small["lens"][small["chrom_idx"]]
        for m, mat in enumerate(small["mats"]):
            total = int(n_windows(small["pos"], L, mat.shape[1]).sum()) * n_strands
            if np.isfinite(mat).all():
                assert offsets[m + 1] - offsets[m] == total
            else:
                assert 0 < offsets[m + 1] - offsets[m] < total
        assert (got["state"] != 3).sum() > 0            # (the motif with -inf entries: an allele that cannot be part of a site)
    if which == "q90":
        assert all(np.any(got["state"] == s) for s in (1, 2, 3))
    genome_bytes = b"".join(small["chroms"][n] for n in small["names"])
    goff = np.concatenate([[0], np.cumsum(small["lens"])])
    assert np.array_equal(ref_codes, oracle.convert_seq(genome_bytes)[goff[small["chrom_idx"]] + small["pos"]])


# ------------------------------------------------------------------------------------------------ 2. the project's own scan, moderate size

N_MOTIFS, N_VARIANTS = 40, 3000


@pytest.fixture(scope="module")
def moderate(jaspar579):
    bases, offsets = synth.make_regions(4, 5000, seed=77)
    raw = bases.tobytes()
    chroms = {f"chr{i + 1}": raw[offsets[i]:offsets[i + 1]] for i in range(4)}
    rng = np.random.default_rng(4242)
    chrom_idx = rng.integers(0, 4, N_VARIANTS).astype(np.int32)
    pos = rng.integers(0, 5000, N_VARIANTS).astype(np.int64)
    pos[:8] = [0, 1, 4999, 4998, 0, 4999, 2, 4997]     # both chromosome ends
    alt = np.frombuffer(b"ACGTNacgt", dtype=np.uint8)[rng.integers(0, 9, N_VARIANTS)]
    widths = jaspar579["widths"][:N_MOTIFS]
    mats = synth.matrices_of(jaspar579["pwm_values"], widths)
    genome = _lib.ResidentGenome(chroms)
    yield {"genome": genome, "chroms": chroms, "names": list(chroms), "chrom_idx": chrom_idx, "pos": pos, "alt": alt, "mats": mats,
           "widths": np.asarray(widths), "cutoffs": {k: jaspar579["cutoffs"][k][:N_MOTIFS] for k in ("1e-4", "1e-3")}, "cache": {}}
    genome.close()


def scan_moderate(case, key, chrom_idx=None, pos=None, alt=None):
    pw = _lib.PwmSet.from_matrices(case["mats"], case["cutoffs"][key])
    res = _lib.scan_variants(pw, case["genome"], case["chrom_idx"] if chrom_idx is None else chrom_idx, case["pos"] if pos is None else pos,
                             case["alt"] if alt is None else alt)
    counts = res.motif_counts()
    s = sites_of(res)
    pw.close()
    return s, counts


def base_result(case, key="1e-3"):
    if key not in case["cache"]:
        case["cache"][key] = scan_moderate(case, key)
    return case["cache"][key]


def record_keys(motif, variant, start, strand, V):
    return ((motif.astype(np.int64) * V + variant) * 8192 + start) * 2 + (strand.astype(np.int64) - 1)


@pytest.mark.parametrize("key", ["1e-4", "1e-3"])
def test_records_equal_two_scans_of_the_flanks(moderate, key):
    case = moderate
    V, wmax = N_VARIANTS, int(case["widths"].max())
    los, seqs = [], []
    for allele in (0, 1):
        for v in range(V):
            seq, x = case["chroms"][case["names"][case["chrom_idx"][v]]], int(case["pos"][v])
            lo, hi = max(0, x - wmax + 1), min(len(seq), x + wmax)
            seqs.append(seq[lo:hi] if allele == 0 else seq[lo:x] + bytes([case["alt"][v]]) + seq[x + 1:hi])
            if allele == 0:
                los.append(lo)
    los = np.array(los)
    pw = _lib.PwmSet.from_matrices(case["mats"], case["cutoffs"][key])
    sq = _lib.SeqSet.from_strings(seqs)
    r = _lib.scan(pw, sq, 3)
    h = r.hits()
    r.close(), sq.close(), pw.close()
    variant, allele = h["seq_idx"] % V, h["seq_idx"] // V
    xr = case["pos"][variant] - los[variant]
    covers = (h["pos"] <= xr) & (h["pos"] + case["widths"][h["motif"]] > xr)
    keys = record_keys(h["motif"], variant, h["pos"] + los[variant], h["strand"], V)
    k_ref, s_ref = keys[covers & (allele == 0)], h["score"][covers & (allele == 0)]
    k_alt, s_alt = keys[covers & (allele == 1)], h["score"][covers & (allele == 1)]
    want_keys = np.union1d(k_ref, k_alt)                # sorted: motif, variant, start, '+' before '-'
    want_state = np.isin(want_keys, k_ref).astype(np.uint8) | (np.isin(want_keys, k_alt).astype(np.uint8) << 1)

    got, _ = base_result(case, key)
    got_keys = record_keys(got["motif"], got["variant"], got["start"], got["strand"], V)
    print(f"p = {key}: {len(got_keys)} records, expected {len(want_keys)}; states {np.bincount(got['state'], minlength=4).tolist()}")
    assert np.array_equal(got_keys, want_keys) and np.array_equal(got["state"], want_state)
    assert np.array_equal(got["motif_offsets"], np.searchsorted(want_keys, np.arange(N_MOTIFS + 1) * V * 8192 * 2))
    o_ref, o_alt = np.argsort(k_ref), np.argsort(k_alt)
    assert np.array_equal(got["score_ref"][(got["state"] & 1) != 0], s_ref[o_ref])
    assert np.array_equal(got["score_alt"][(got["state"] & 2) != 0], s_alt[o_alt])
    assert len(want_keys) > 100 and all(np.any(want_state == s) for s in (1, 2, 3))


# ------------------------------------------------------------------------------------------------ 3. order, duplicates, determinism, chunks

def test_order_duplicates_determinism_and_chunks(moderate):
    case = moderate
    V, P = N_VARIANTS, N_MOTIFS
    base, (gained0, lost0) = base_result(case)
    rng = np.random.default_rng(99)
    src = np.concatenate([np.arange(V), rng.integers(0, V, 200)])
    rng.shuffle(src)
    args = (case["chrom_idx"][src], case["pos"][src], case["alt"][src])
    got, (gained, lost) = scan_moderate(case, "1e-3", *args)

    cell = base["motif"].astype(np.int64) * V + base["variant"]
    cnt = np.bincount(cell, minlength=P * V)
    first = (np.cumsum(cnt) - cnt).reshape(P, V)[:, src].ravel()
    tot = cnt.reshape(P, V)[:, src].ravel()
    take = np.repeat(first - (np.cumsum(tot) - tot), tot) + np.arange(int(tot.sum()))
    assert np.array_equal(got["variant"], np.repeat(np.tile(np.arange(len(src)), P), tot))
    for k in ("start", "strand", "score_ref", "score_alt", "state", "motif"):
        assert np.array_equal(got[k], base[k][take]), k
    assert np.array_equal(got["motif_offsets"], np.concatenate([[0], np.cumsum(tot.reshape(P, -1).sum(axis=1))]))

    again, (gained2, lost2) = scan_moderate(case, "1e-3", *args)
    for k in got:
        assert got[k].tobytes() == again[k].tobytes(), k
    assert np.array_equal(gained, gained2) and np.array_equal(lost, lost2)

    for state, dev in ((2, gained), (1, lost)):         # duplicates are variants of their own
        sel = got["state"] == state
        pairs = np.unique(got["motif"][sel].astype(np.int64) * len(src) + got["variant"][sel])
        assert np.array_equal(dev, np.bincount(pairs // len(src), minlength=P))
    assert gained.sum() > 0 and lost.sum() > 0 and gained.sum() >= gained0.sum() and lost.sum() >= lost0.sum()

    prev = _lib.varscan_chunk(7)
    try:
        chunked, (gained7, lost7) = scan_moderate(case, "1e-3", *args)
    finally:
        _lib.varscan_chunk(prev)
    for k in got:
        assert got[k].tobytes() == chunked[k].tobytes(), k
    assert np.array_equal(gained, gained7) and np.array_equal(lost, lost7)


# ------------------------------------------------------------------------------------------------ 4. validation

def test_validation_and_empty_results(small):
    genome, lens = small["genome"], small["lens"]
    pw = _lib.PwmSet.from_matrices(small["mats"], small["cutoffs"]["all"])
    try:
        for ci, x in ((1, int(lens[1])), (1, -1), (0, 5), (len(lens), 0), (-1, 0)):
            with pytest.raises(ValueError):
                _lib.scan_variants(pw, genome, [1, ci], [3, x], b"AC")
        with pytest.raises(ValueError):
            _lib.scan_variants(pw, genome, [1], [3], b"A", strand_mask=0)
        with pytest.raises(ValueError):
            _lib.scan_variants(pw, genome, [1], [3], b"A", strand_mask=4)
        with pytest.raises(ValueError):
            _lib.scan_variants(pw, genome, [1], [3], b"A", flags=1)
        res = _lib.scan_variants(pw, genome, [], [], b"")
        gained, lost = res.motif_counts()
        assert res.n_sites == 0 and not res.motif_offsets.any() and len(res.motif_offsets) == len(small["mats"]) + 1
        assert not gained.any() and not lost.any() and res.ref_codes().size == 0
        s = sites_of(res)
        assert all(len(s[k]) == 0 for k in ("variant", "start", "strand", "score_ref", "score_alt", "state"))
    finally:
        pw.close()
    wide = _lib.PwmSet.from_matrices([seeded_matrix(98, 1), seeded_matrix(120, 2)], [ALL_PASS, ALL_PASS])
    try:
        res = _lib.scan_variants(wide, genome, small["chrom_idx"], small["pos"], small["alt"])
        assert res.n_sites == 0 and not res.motif_offsets.any()
        assert not np.any(res.motif_counts())
        res.close()
    finally:
        wide.close()


# ------------------------------------------------------------------------------------------------ 5. through the Python module

class Pwm:
    def __init__(self, matrix, cutoff):
        self.matrix, self.cutoffs, self.length = matrix, {"1e-4": cutoff}, matrix.shape[1]


def test_gained_and_lost_sites_from_a_vcf(tmp_path):
    consensus = "GATTACAG"
    matrix = np.full((4, len(consensus)), -2.0)
    for c, b in enumerate(consensus):
        matrix["ACGT".index(b), c] = 1.5                # an exact match scores 1, one mismatch (12 - 3.5) / 12
    seq = "T" * 10 + "GATTACAG" + "T" * 12 + "CTGTAATC" + "T" * 7 + "GATTCCAG" + "T" * 7
    assert len(seq) == 60 and seq[30:38] == "CTGTAATC" and seq[45:53] == "GATTCCAG"
    lines = ["##fileformat=VCFv4.2", "#CHROM\tPOS\tID\tREF\tALT",
             "chrT\t13\tbreak_fwd\tT\tG", "chrT\t34\tbreak_rev\tt\tC", "chrT\t50\tcomplete\tC\ta", "chrT\t20\tindel\tT\tTA", "chrT\t6\twrong_ref\tG\tA"]
    path = tmp_path / "v.vcf"
    path.write_text("\n".join(lines) + "\n")
    v = variants.read_vcf(path)
    assert v.id.tolist() == ["break_fwd", "break_rev", "complete", "wrong_ref"] and v.skipped["indel"] == 1
    genome = _lib.ResidentGenome({"chrT": seq})
    pwms = [Pwm(matrix, 0.9)]
    try:
        with pytest.raises(ValueError, match="chrT:6 REF G but the genome has T"):
            variants.scan_variants(genome, pwms, v.chrom, v.pos, v.alt, ref=v.ref)
        with pytest.raises(KeyError):
            variants.scan_variants(genome, pwms, ["chrU"], [3], ["A"])
        s = variants.scan_variants(genome, pwms, v.chrom, v.pos, v.alt, ref=v.ref, on_mismatch="skip")
        unchecked = variants.scan_variants(genome, pwms, v.chrom, v.pos, v.alt)
    finally:
        genome.close()
    assert s.skipped.tolist() == [3] and unchecked.skipped.size == 0
    assert s.variant.tolist() == [0, 1, 2] and s.start.tolist() == [10, 30, 45] and s.strand.tolist() == [1, 2, 1]
    assert s.lost.tolist() == [True, True, False] and s.gained.tolist() == [False, False, True] and not s.kept.any()
    assert s.delta[0] < 0 and s.delta[1] < 0 and s.delta[2] > 0
    assert s.score_ref[0] == 1.0 and s.score_ref[1] == 1.0 and s.score_alt[2] == 1.0
    assert s.motif_offsets.tolist() == [0, 3] and s.motif.tolist() == [0, 0, 0]
    gained, lost = s.motif_counts()
    assert gained.tolist() == [1] and lost.tolist() == [2]
    assert "ACGT"[s.ref_codes[3]] == "T"
    assert len(unchecked) == 3 and np.array_equal(unchecked.state, s.state)      # (the T -> A in the T run makes no site)
