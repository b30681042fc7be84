"""
ms_scan_alleles (ms_alleles.hip) on the GPU: the motif sites on the ref and on the spliced alt haplotype of alleles of any length --
against the pinned oracle at the smallest shapes that can go wrong (every allele shape at every position of three tiny chromosomes),
against ms_scan_variants where both apply, against the project's own scan of the haplotype flanks at moderate size, for its order /
determinism / chunking, its validation, and through motifscan_amd.variants with a VCF.
"""
import numpy as np
import pytest

from motifscan_amd import _lib, synth, variants
from variant_cases import allele_flank_table, expected_allele_records as expected_records, flanks, n_affected, seeded_matrix

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
SHAPES = ((1, 1), (0, 1), (1, 0), (0, 3), (3, 0), (2, 2), (2, 5), (5, 2), (0, 40), (35, 0), (1, 33))
ALT_LETTERS = b"ACGTACGTNacgtn"


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

    # every shape at every position it fits, x = L included for the pure insertions; seeded alt letters with N and lower case
    arng = np.random.default_rng(7)
    chrom_idx, pos, ref_len, alts = [], [], [], []
    for r, a in SHAPES:
        for ci, L in enumerate(lens):
            for x in range(0, int(L) - r + 1):
                chrom_idx.append(ci), pos.append(x), ref_len.append(r)
                alts.append(np.frombuffer(ALT_LETTERS, dtype=np.uint8)[arng.integers(0, len(ALT_LETTERS), a)].tobytes())
    chrom_idx, pos, ref_len = np.array(chrom_idx, dtype=np.int32), np.array(pos, dtype=np.int64), np.array(ref_len, dtype=np.int32)
    alt_len = np.array([len(a) for a in alts])
    V = len(pos)
    assert any(b"N" in a for a in alts) and any(a != a.upper() for a in alts)
    assert np.any((ref_len > 0) & (pos + ref_len == lens[chrom_idx])) and np.any((ref_len == 0) & (pos == lens[chrom_idx]))

    # per motif: every affected window of either haplotype, scored by the oracle on Python-built flank strings (ref, alt per variant)
    table = allele_flank_table(oracle, chroms, names, mats, chrom_idx, pos, ref_len, alts)
    assert any(np.any(n_affected(pos, alt_len, lens[chrom_idx] - ref_len + alt_len, m.shape[1]) == 0) for m in mats)

    quant = [float(np.quantile(t["score"][np.isfinite(t["score"])], 0.9)) for t in table]
    genome = _lib.ResidentGenome(chroms)
    yield {"genome": genome, "chroms": chroms, "names": names, "mats": mats, "chrom_idx": chrom_idx, "pos": pos, "ref_len": ref_len, "alts": alts,
           "table": table, "lens": lens, "V": V,
           "cutoffs": {"q90": np.array(quant), "all": np.full(len(mats), ALL_PASS), "none": np.full(len(mats), 2.0)}}
    genome.close()


@pytest.mark.parametrize("strand_mask", [1, 2, 3])
@pytest.mark.parametrize("which", ["q90", "all", "none"])
def test_records_equal_the_oracle(small, which, strand_mask):
    cutoffs = small["cutoffs"][which]
    pw = _lib.PwmSet.from_matrices(small["mats"], cutoffs)
    res = _lib.scan_alleles(pw, small["genome"], small["chrom_idx"], small["pos"], small["ref_len"], small["alts"], strand_mask=strand_mask)
    gained, lost = res.motif_counts()
    mismatch = res.ref_mismatch()
    got = sites_of(res)
    pw.close()
    want, offsets, want_gained, want_lost = expected_records(small["table"], cutoffs, strand_mask, small["V"])
    print(f"{which} strands {strand_mask}: {len(got['score'])} records, expected {offsets[-1]}; per allele {np.bincount(got['allele'], minlength=2).tolist()}; "
          f"gained {gained.tolist()} lost {lost.tolist()}")
    assert np.array_equal(got["motif_offsets"], offsets)
    for k in ("variant", "allele", "start", "strand"):
        assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(got["score"], want["score"])
    assert np.array_equal(gained, want_gained) and np.array_equal(lost, want_lost)
    assert not mismatch.any() and mismatch.shape == (small["V"],)
    if which == "none":
        assert offsets[-1] == 0
    if which == "all":                                  # nothing is lost, however dense: every affected window x strand with a finite score
        n_strands = bin(strand_mask).count("1")
        for m, (mat, t) in enumerate(zip(small["mats"], small["table"])):
            total = len(t["variant"]) * n_strands
            if np.isfinite(mat).all():
                assert offsets[m + 1] - offsets[m] == total
            else:
                assert 0 < offsets[m + 1] - offsets[m] < total
    if which == "q90":
        assert gained.sum() > 0 and lost.sum() > 0 and np.any(got["allele"] == 0) and np.any(got["allele"] == 1)


def test_equal_to_the_snv_scan_where_both_apply(small):
    sel = np.flatnonzero(small["ref_len"] == 1)
    sel = sel[[len(small["alts"][i]) == 1 for i in sel]]
    assert len(sel) == small["lens"].sum()
    alts = [small["alts"][i] for i in sel]
    pw = _lib.PwmSet.from_matrices(small["mats"], small["cutoffs"]["q90"])
    al = sites_of(_lib.scan_alleles(pw, small["genome"], small["chrom_idx"][sel], small["pos"][sel], small["ref_len"][sel], alts))
    snv = sites_of(_lib.scan_variants(pw, small["genome"], small["chrom_idx"][sel], small["pos"][sel], b"".join(alts)))
    pw.close()
    n = len(sel)
    # the SNV records are ordered (motif, variant, start, strand); the allele records (motif, variant, allele, start, strand)
    for allele, bit, score in ((0, 1, "score_ref"), (1, 2, "score_alt")):
        a = al["allele"] == allele
        s = (snv["state"] & bit) != 0
        assert a.sum() == s.sum() and a.sum() > 0
        for k, ks in (("motif", "motif"), ("variant", "variant"), ("start", "start"), ("strand", "strand"), ("score", score)):
            assert np.array_equal(al[k][a], snv[ks][s]), (allele, k)
    assert n > 0


# ------------------------------------------------------------------------------------------------ 2. the project's own scan, moderate size

N_VARIANTS, N_CHROMS, CHROM_BP, SPAN = 20000, 4, 750_000, 1 << 20


def mixed_alleles(rng, n, chroms, names, chrom_bp):
    """80 % SNVs, 10 % insertions and 10 % deletions of 1 .. 20 bases, a few multi-base alleles, both chromosome ends."""
    kind = rng.random(n)
    chrom_idx = rng.integers(0, len(names), n).astype(np.int32)
    length = rng.integers(1, 21, n)
    ref_len = np.where(kind < 0.8, 1, np.where(kind < 0.9, 0, length)).astype(np.int32)
    alt_len = np.where(kind < 0.8, 1, np.where(kind < 0.9, length, 0))
    multi = rng.random(n) < 0.03
    ref_len[multi], alt_len[multi] = rng.integers(2, 6, multi.sum()), rng.integers(2, 6, multi.sum())
    pos = rng.integers(0, chrom_bp - 25, n).astype(np.int64)
    pos[:6] = [0, 1, chrom_bp - ref_len[2], chrom_bp - ref_len[3] - 1, 0, 2]
    letters = np.frombuffer(b"ACGTACGTACGTNacgt", dtype=np.uint8)
    alts = [letters[rng.integers(0, len(letters), a)].tobytes() for a in alt_len]
    return chrom_idx, pos, ref_len, alts


@pytest.fixture(scope="module")
def moderate(jaspar579):
    bases, offsets = synth.make_regions(N_CHROMS, CHROM_BP, seed=78)
    raw = bases.tobytes()
    names = [f"chr{i + 1}" for i in range(N_CHROMS)]
    chroms = {n: raw[offsets[i]:offsets[i + 1]] for i, n in enumerate(names)}
    chrom_idx, pos, ref_len, alts = mixed_alleles(np.random.default_rng(4243), N_VARIANTS, chroms, names, CHROM_BP)
    widths = np.asarray(jaspar579["widths"])
    mats = synth.matrices_of(jaspar579["pwm_values"], widths)
    genome = _lib.ResidentGenome(chroms)
    yield {"genome": genome, "chroms": chroms, "names": names, "chrom_idx": chrom_idx, "pos": pos, "ref_len": ref_len, "alts": alts, "mats": mats,
           "widths": widths, "cutoffs": {k: jaspar579["cutoffs"][k] for k in ("1e-4", "1e-3")}}
    genome.close()


def record_keys(motif, variant, allele, start, strand, V):
    return ((((motif.astype(np.int64) * V + variant) * 2 + allele) * SPAN + start) * 2) + (strand.astype(np.int64) - 1)


@pytest.mark.parametrize("key", ["1e-4", "1e-3"])
def test_records_equal_two_scans_of_the_haplotype_flanks(moderate, key):
    case = moderate
    V, P, wmax = N_VARIANTS, len(case["widths"]), int(case["widths"].max())
    los, seqs = np.zeros(V, dtype=np.int64), [[], []]
    for v in range(V):
        lo, fr, fa = flanks(case["chroms"][case["names"][case["chrom_idx"][v]]], int(case["pos"][v]), int(case["ref_len"][v]), case["alts"][v], wmax)
        los[v] = lo
        seqs[0].append(fr), seqs[1].append(fa)
    alt_len = np.array([len(a) for a in case["alts"]])
    pw = _lib.PwmSet.from_matrices(case["mats"], case["cutoffs"][key])
    keys, scores = [], []
    for allele, length in ((0, case["ref_len"].astype(np.int64)), (1, alt_len)):
        sq = _lib.SeqSet.from_strings(seqs[allele])
        r = _lib.scan(pw, sq, 3)
        h = r.hits()
        r.close(), sq.close()
        v, start, x = h["seq_idx"], h["pos"] + los[h["seq_idx"]], case["pos"][h["seq_idx"]]
        affected = (start >= x - case["widths"][h["motif"]] + 1) & (start <= x + length[v] - 1)
        keys.append(record_keys(h["motif"][affected], v[affected], allele, start[affected], h["strand"][affected], V))
        scores.append(h["score"][affected])
    want_keys, want_score = np.concatenate(keys), np.concatenate(scores)
    order = np.argsort(want_keys, kind="stable")        # motif, variant, allele, start, '+' before '-'
    want_keys, want_score = want_keys[order], want_score[order]

    res = _lib.scan_alleles(pw, case["genome"], case["chrom_idx"], case["pos"], case["ref_len"], case["alts"])
    gained, lost = res.motif_counts()
    got = sites_of(res)
    pw.close()
    got_keys = record_keys(got["motif"], got["variant"], got["allele"], got["start"], got["strand"], V)
    print(f"p = {key}: {len(got_keys)} records, expected {len(want_keys)}; per allele {np.bincount(got['allele'], minlength=2).tolist()}; "
          f"gained {int(gained.sum())} lost {int(lost.sum())}")
    assert np.array_equal(got_keys, want_keys) and np.array_equal(got["score"], want_score)
    assert np.array_equal(got["motif_offsets"], np.searchsorted(want_keys, np.arange(P + 1) * V * 2 * SPAN * 2))
    cell = want_keys // (2 * SPAN * 2)                  # motif * V + variant
    has = np.zeros((P * V, 2), dtype=bool)
    has[cell, (want_keys // (SPAN * 2)) % 2] = True
    assert np.array_equal(gained, (has[:, 1] & ~has[:, 0]).reshape(P, V).sum(axis=1))
    assert np.array_equal(lost, (has[:, 0] & ~has[:, 1]).reshape(P, V).sum(axis=1))
    assert len(want_keys) > 1000 and gained.sum() > 0 and lost.sum() > 0
    long_allele = (case["ref_len"] + alt_len)[got["variant"]] > 2
    assert np.any(long_allele & (got["allele"] == 0)) and np.any(long_allele & (got["allele"] == 1))


# ------------------------------------------------------------------------------------------------ 3. order, duplicates, determinism, chunks

N_SUB_MOTIFS, N_SUB = 40, 3000


def scan_sub(case, src):
    pw = _lib.PwmSet.from_matrices(case["mats"][:N_SUB_MOTIFS], case["cutoffs"]["1e-3"][:N_SUB_MOTIFS])
    res = _lib.scan_alleles(pw, case["genome"], case["chrom_idx"][src], case["pos"][src], case["ref_len"][src], [case["alts"][i] for i in src])
    counts = res.motif_counts()
    s = sites_of(res)
    pw.close()
    return s, counts


def test_order_duplicates_determinism_and_chunks(moderate):
    case = moderate
    V, P = N_SUB, N_SUB_MOTIFS
    base, (gained0, lost0) = scan_sub(case, np.arange(V))
    rng = np.random.default_rng(99)
    src = np.concatenate([np.arange(V), rng.integers(0, V, 200)])
    rng.shuffle(src)
    got, (gained, lost) = scan_sub(case, src)

    # the records of input variant i are the base run's records of variant src[i], in its order
    cell = base["motif"].astype(np.int64) * V + base["variant"]
    cnt = np.bincount(cell, minlength=P * V)
    first = (np.cumsum(cnt) - cnt).reshape(P, V)[:, src].ravel()
    tot = cnt.reshape(P, V)[:, src].ravel()
    take = np.repeat(first - (np.cumsum(tot) - tot), tot) + np.arange(int(tot.sum()))
    assert np.array_equal(got["variant"], np.repeat(np.tile(np.arange(len(src)), P), tot))
    for k in ("allele", "start", "strand", "score", "motif"):
        assert np.array_equal(got[k], base[k][take]), k
    assert np.array_equal(got["motif_offsets"], np.concatenate([[0], np.cumsum(tot.reshape(P, -1).sum(axis=1))]))

    again, (gained2, lost2) = scan_sub(case, src)
    for k in got:
        assert got[k].tobytes() == again[k].tobytes(), k
    assert np.array_equal(gained, gained2) and np.array_equal(lost, lost2)

    has = np.zeros((P * len(src), 2), dtype=bool)       # duplicates are variants of their own
    has[got["motif"].astype(np.int64) * len(src) + got["variant"], got["allele"]] = True
    assert np.array_equal(gained, (has[:, 1] & ~has[:, 0]).reshape(P, -1).sum(axis=1))
    assert np.array_equal(lost, (has[:, 0] & ~has[:, 1]).reshape(P, -1).sum(axis=1))
    assert gained.sum() > 0 and lost.sum() > 0 and gained.sum() >= gained0.sum() and lost.sum() >= lost0.sum()

    prev = _lib.varscan_chunk(7)
    try:
        chunked, (gained7, lost7) = scan_sub(case, src[:500])
    finally:
        _lib.varscan_chunk(prev)
    whole, (gained_w, lost_w) = scan_sub(case, src[:500])
    assert len(whole["score"]) > 0
    for k in whole:
        assert whole[k].tobytes() == chunked[k].tobytes(), k
    assert np.array_equal(gained_w, gained7) and np.array_equal(lost_w, lost7)


# ------------------------------------------------------------------------------------------------ 4. validation

def test_validation_empty_results_and_the_ref_check(small):
    genome, lens = small["genome"], small["lens"]
    pw = _lib.PwmSet.from_matrices(small["mats"], small["cutoffs"]["all"])
    L1 = int(lens[1])
    try:
        bad = [(len(lens), 0, 1, b"A"), (-1, 0, 1, b"A"),                   # chromosome index
               (1, -1, 1, b"A"), (1, L1 + 1, 0, b"A"),                      # x outside [0, L]
               (1, 3, -1, b"A"), (1, L1 - 1, 2, b"A"), (1, L1, 1, b""),     # r < 0, x + r > L
               (1, 3, 0, b""),                                              # r + a = 0
               (1, 3, 1, b"A" * (65536 + 1))]                               # longer than MS_ALLELE_MAX_LEN
        for ci, x, r, alt in bad:
            with pytest.raises(ValueError):
                _lib.scan_alleles(pw, genome, [1, ci], [3, x], [1, r], [b"C", alt])
        for kw in ({"strand_mask": 0}, {"strand_mask": 4}, {"flags": 1}):
            with pytest.raises(ValueError):
                _lib.scan_alleles(pw, genome, [1], [3], [1], [b"A"], **kw)
        import ctypes
        h = ctypes.c_void_p()
        ci, ps, rl = np.zeros(2, dtype=np.int32), np.full(2, 3, dtype=np.int64), np.ones(2, dtype=np.int32)
        for offs in ([0, 2, 1], [1, 2, 3]):                                  # alt_offsets that decrease / do not start at 0
            ao = np.array(offs, dtype=np.int64)
            rc = _lib.lib().ms_scan_alleles(pw.h, genome.h, _lib.ptr(ci, ctypes.c_int32), _lib.ptr(ps, ctypes.c_int64), _lib.ptr(rl, ctypes.c_int32),
                                            b"ACGT", _lib.ptr(ao, ctypes.c_int64), None, 2, 3, 0, ctypes.byref(h))
            assert rc == _lib.MS_ERR_INVALID and not h.value
        rc = _lib.lib().ms_scan_alleles(None, genome.h, _lib.ptr(ci, ctypes.c_int32), _lib.ptr(ps, ctypes.c_int64), _lib.ptr(rl, ctypes.c_int32),
                                        b"AC", _lib.ptr(np.array([0, 1, 2], dtype=np.int64), ctypes.c_int64), None, 2, 3, 0, ctypes.byref(h))
        assert rc == _lib.MS_ERR_INVALID and not h.value

        res = _lib.scan_alleles(pw, genome, [], [], [], [])                  # V = 0
        gained, lost = res.motif_counts()
        assert res.n_sites == 0 and not res.motif_offsets.any() and len(res.motif_offsets) == len(small["mats"]) + 1
        assert not gained.any() and not lost.any() and res.ref_mismatch().size == 0
        s = sites_of(res)
        assert all(len(s[k]) == 0 for k in ("variant", "allele", "start", "strand", "score"))
        # an allele of the greatest length allowed is taken (a deletion of nothing is not: the chromosomes are short, so as an insertion)
        res = _lib.scan_alleles(pw, genome, [0], [2], [0], [b"ACGT" * (65536 // 4)])
        assert res.n_sites > 0
        res.close()
    finally:
        pw.close()
    none = _lib.PwmSet.from_matrices([], [])                                 # P = 0
    try:
        res = _lib.scan_alleles(none, genome, [1, 2], [3, 4], [1, 0], [b"A", b"CG"])
        assert res.n_sites == 0 and res.motif_offsets.tolist() == [0] and res.motif_counts()[0].size == 0
        res.close()
    finally:
        none.close()

    # REF strings against the genome: upper and lower case, an N run, the IUPAC letter, a deletion up to the chromosome's end
    c97 = small["chroms"]["c97"]
    pw = _lib.PwmSet.from_matrices(small["mats"][:2], small["cutoffs"]["none"][:2])
    wrong = bytes([{65: 67, 67: 71, 71: 84, 84: 65}[c97[40]]])
    cases = [(40, c97[40:44], False), (40, c97[40:44].lower(), False), (40, c97[40:43] + wrong, True), (40, wrong + c97[41:44], True),
             (50, c97[50:63].upper(), False), (50, c97[50:63], False),          # the lower-case run of the genome
             (14, c97[14:16], False), (14, c97[14:15] + b"n", False), (14, c97[14:15] + b"R", False), (14, c97[14:15] + b"A", True),
             (28, b"NN" + c97[30:31], False), (28, b"NNN", True),               # the base behind the N run is ACGT
             (80, b"R", False), (80, b"N", False), (80, b"a", True),            # the IUPAC letter is "not ACGT" to either side
             (94, c97[94:97], False), (97, b"", False), (0, c97[0:1], False), (0, b"N", True)]
    try:
        res = _lib.scan_alleles(pw, genome, [2] * len(cases), [c[0] for c in cases], [len(c[1]) for c in cases], [b"T"] * len(cases),
                                refs=[c[1] for c in cases])
        assert res.ref_mismatch().tolist() == [c[2] for c in cases]
        res.close()
        with pytest.raises(ValueError, match="refs"):
            _lib.scan_alleles(pw, genome, [2], [3], [2], [b"T"], refs=[b"A"])
    finally:
        pw.close()


# ------------------------------------------------------------------------------------------------ 5. through the Python module

class Pwm:
    def __init__(self, matrix, cutoff):
        self.matrix, self.cutoffs, self.length = matrix, {"1e-4": cutoff}, matrix.shape[1]


def test_sites_of_indels_from_a_vcf(tmp_path):
    consensus = "GATTACAG"
    matrix = np.full((4, len(consensus)), -2.0)
    for c, b in enumerate(consensus):
        matrix["ACGT".index(b), c] = 1.5                # an exact match scores 1, one mismatch (12 - 3.5) / 12
    #      0         10        20        30        40        50        60
    seq = "T" * 10 + "GATTACAG" + "T" * 6 + "GATACAG" + "T" * 5 + "CTGTCCAATC" + "T" * 14
    assert len(seq) == 60 and seq[24:31] == "GATACAG" and seq[36:46] == "CTGTCCAATC"
    lines = ["##fileformat=VCFv4.2", "#CHROM\tPOS\tID\tREF\tALT",
             "chrT\t13\tdel_breaks\tTTA\tT",             # GATTACAG -> GATCAG: the site at 10 is lost
             "chrT\t26\tins_completes\tA\tAT",           # GATACAG -> GATTACAG: a site at 24 is made
             "chrT\t40\tdel_completes_rev\ttCC\tt",      # CTGTCCAATC -> CTGTAATC: a '-' site at 36 is made
             "chrT\t50\tquiet\tT\tTTT",                  # an insertion in the T run: no site either way
             "chrT\t5\twrong_ref\tTG\tT",
             "chrT\t7\tsymbolic\tT\t<DEL>"]
    path = tmp_path / "v.vcf"
    path.write_text("\n".join(lines) + "\n")
    v = variants.read_vcf_alleles(path)
    assert v.id.tolist() == ["del_breaks", "ins_completes", "del_completes_rev", "quiet", "wrong_ref"] and v.skipped["symbolic"] == 1
    # (T -> TTT: the shared suffix goes first, so the two inserted bases stay at the anchor's own position, 49)
    assert v.pos.tolist() == [13, 26, 40, 49, 5] and v.ref.tolist() == ["TA", "", "CC", "", "G"] and v.alt.tolist() == ["", "T", "", "TT", ""]
    genome = _lib.ResidentGenome({"chrT": seq})
    pwms = [Pwm(matrix, 0.9)]
    try:
        with pytest.raises(ValueError, match="chrT:6 REF G"):
            variants.scan_alleles(genome, pwms, v.chrom, v.pos, v.ref, v.alt)
        with pytest.raises(KeyError):
            variants.scan_alleles(genome, pwms, ["chrU"], [3], ["A"], ["C"])
        s = variants.scan_alleles(genome, pwms, v.chrom, v.pos, v.ref, v.alt, on_mismatch="skip")
        plus = variants.scan_alleles(genome, pwms, v.chrom[:4], v.pos[:4], v.ref[:4], v.alt[:4], strand="+")
    finally:
        genome.close()
    assert s.skipped.tolist() == [4] and plus.skipped.size == 0
    assert s.variant.tolist() == [0, 1, 2] and s.allele.tolist() == [0, 1, 1] and s.start.tolist() == [10, 24, 36] and s.strand.tolist() == [1, 1, 2]
    assert s.score.tolist() == [1.0, 1.0, 1.0]
    assert s.ref_start().tolist() == [10, 24, 36]
    assert s.motif_offsets.tolist() == [0, 3] and s.motif.tolist() == [0, 0, 0]
    gained, lost = s.motif_counts()
    assert gained.tolist() == [2] and lost.tolist() == [1]
    pv = s.per_variant()
    assert pv["variant"].tolist() == [0, 1, 2] and pv["n_ref"].tolist() == [1, 0, 0] and pv["n_alt"].tolist() == [0, 1, 1]
    assert plus.variant.tolist() == [0, 1] and plus.motif_counts()[0].tolist() == [1]
