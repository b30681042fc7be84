"""
motifscan_amd.kmers on the host: the code of a k-mer, the sequential restatement of ms_seqset_kmer_counts (kmer_counts_host) against
numbers written out by hand and against a plain triple loop, the Markov table, the enrichment statistics, the seed matrix, and the path
constants of the build (ms_debug_kmer_dims).  No GPU.  HAND and random_seqs are shared with tests/test_gpu_kmers.py.
"""
import ctypes
import math
import random

import numpy as np
import pytest

from motifscan_amd import _lib, kmers

ALPHABET = "ACGT" * 5 + "acgtNnRYK"

# every number by hand.  occ / nseq: {code: count}, everything else 0; totals: (sequences, counted windows, left-out windows, sequences < k)
HAND = [
    # AC 1, CG 6, GT 11
    dict(name="ACGT_k2", seqs=["ACGT"], k=2, canonical=False, occ={1: 1, 6: 1, 11: 1}, nseq={1: 1, 6: 1, 11: 1}, totals=(1, 3, 0, 0)),
    # GT folds onto AC (rc(GT) = AC); CG is its own reverse complement and counts once per window
    dict(name="ACGT_k2_canonical", seqs=["ACGT"], k=2, canonical=True, occ={1: 2, 6: 1}, nseq={1: 1, 6: 1}, totals=(1, 3, 0, 0)),
    # AA, AN, NA, AA
    dict(name="AANAA_k2", seqs=["AANAA"], k=2, canonical=False, occ={0: 2}, nseq={0: 1}, totals=(1, 2, 2, 0)),
    dict(name="AANAA_k2_canonical", seqs=["AANAA"], k=2, canonical=True, occ={0: 2}, nseq={0: 1}, totals=(1, 2, 2, 0)),
    # lower case counts, u is no base: ac 1, cg 6, gu left out
    dict(name="acgu_k2", seqs=["acgu"], k=2, canonical=False, occ={1: 1, 6: 1}, nseq={1: 1, 6: 1}, totals=(1, 2, 1, 0)),
    dict(name="length_k_minus_1", seqs=["AC"], k=3, canonical=False, occ={}, nseq={}, totals=(1, 0, 0, 1)),
    dict(name="empty", seqs=[""], k=2, canonical=True, occ={}, nseq={}, totals=(1, 0, 0, 1)),
    # ACAC: AC, CA, AC; TAC: TA 12, AC -- AC in both sequences, twice in the first
    dict(name="shared_kmer", seqs=["ACAC", "TAC"], k=2, canonical=False, occ={1: 3, 4: 1, 12: 1}, nseq={1: 2, 4: 1, 12: 1}, totals=(2, 5, 0, 0)),
    # GTG: GT -> AC 1, TG 14 -> CA 4
    dict(name="shared_kmer_canonical", seqs=["ACAC", "GTG"], k=2, canonical=True, occ={1: 3, 4: 2}, nseq={1: 2, 4: 2}, totals=(2, 5, 0, 0)),
    dict(name="selected", seqs=["ACAC", "TAC"], k=2, canonical=False, sel=[0, 1], occ={1: 1, 12: 1}, nseq={1: 1, 12: 1}, totals=(1, 2, 0, 0)),
    # k = 1: the base counts; AAC, k = 3 canonical: rc = GTT 47 > AAC 1
    dict(name="k1", seqs=["AACGTTT", "N"], k=1, canonical=False, occ={0: 2, 1: 1, 2: 1, 3: 3}, nseq={0: 1, 1: 1, 2: 1, 3: 1}, totals=(2, 7, 1, 0)),
    dict(name="GTT_k3_canonical", seqs=["GTT"], k=3, canonical=True, occ={1: 1}, nseq={1: 1}, totals=(1, 1, 0, 0)),
]


def dense(d, k):
    out = np.zeros(4 ** k, dtype=np.int64)
    for c, n in d.items():
        out[c] = n
    return out


def assert_hand(case, got):
    k = case["k"]
    assert (got.k, got.canonical) == (k, case["canonical"])
    assert np.array_equal(got.occ, dense(case["occ"], k)), case["name"]
    assert np.array_equal(got.nseq, dense(case["nseq"], k)), case["name"]
    assert tuple(got.totals.tolist()) == case["totals"], case["name"]
    assert int(got.occ.sum()) == got.n_windows


def random_seqs(rng, n, max_len, alphabet=ALPHABET):
    return ["".join(rng.choice(alphabet) for _ in range(rng.randint(0, max_len))) for _ in range(n)]


def triple_loop(seqs, k, canonical, sel=None):
    """sequence by sequence, start by start, base by base"""
    code_of = {"A": 0, "C": 1, "G": 2, "T": 3, "a": 0, "c": 1, "g": 2, "t": 3}
    occ, nseq, totals = np.zeros(4 ** k, dtype=np.int64), np.zeros(4 ** k, dtype=np.int64), [0, 0, 0, 0]
    for r, s in enumerate(seqs):
        if sel is not None and not sel[r]:
            continue
        totals[0] += 1
        if len(s) < k:
            totals[3] += 1
        mine = set()
        for p in range(len(s) - k + 1):
            fwd = rc = 0
            ok = True
            for j in range(k):
                b = code_of.get(s[p + j])
                if b is None:
                    ok = False
                    break
                fwd += b << (2 * (k - 1 - j))
                rc += (3 - b) << (2 * j)
            if not ok:
                totals[2] += 1
                continue
            c = min(fwd, rc) if canonical else fwd
            occ[c] += 1
            totals[1] += 1
            mine.add(c)
        for c in mine:
            nseq[c] += 1
    return occ, nseq, tuple(totals)


@pytest.mark.parametrize("case", HAND, ids=[c["name"] for c in HAND])
def test_restatement_on_hand_cases(case):
    assert_hand(case, kmers.kmer_counts_host(case["seqs"], case["k"], case["canonical"], case.get("sel")))


def test_codes_round_trip():
    assert kmers.encode("A") == 0 and kmers.encode("t") == 3 and kmers.decode(2, 1) == "G"
    assert [kmers.revcomp_code(c, 1) for c in range(4)] == [3, 2, 1, 0]
    assert kmers.encode("ACGT") == 0b00011011 and kmers.revcomp_code(kmers.encode("ACGT"), 4) == kmers.encode("ACGT")
    assert kmers.decode(kmers.revcomp_code(kmers.encode("GATAAG"), 6), 6) == "CTTATC"
    rng = random.Random(5)
    for k in (1, 12):
        for code in [0, 4 ** k - 1] + [rng.randrange(4 ** k) for _ in range(50)]:
            text = kmers.decode(code, k)
            assert len(text) == k and kmers.encode(text) == code and kmers.encode(text.lower()) == code
            rc = kmers.revcomp_code(code, k)
            assert kmers.revcomp_code(rc, k) == code
            assert kmers.decode(rc, k) == text[::-1].translate(str.maketrans("ACGT", "TGCA"))
    assert kmers.decode(kmers.encode("ACGTACGTACGT"), 12) == "ACGTACGTACGT"
    for bad in ("", "ACGTACGTACGTA", "ACN"):
        with pytest.raises(ValueError):
            kmers.encode(bad)
    with pytest.raises(ValueError):
        kmers.decode(4, 1)
    with pytest.raises(ValueError):
        kmers.decode(0, 13)


def test_restatement_equals_a_triple_loop():
    rng = random.Random(11)
    for case in range(40):
        k = 1 + case % 6
        canonical = bool((case // 6) & 1)
        seqs = random_seqs(rng, rng.randint(0, 6), 40)
        sel = None if case % 3 else [rng.randint(0, 1) for _ in seqs]
        got = kmers.kmer_counts_host(seqs, k, canonical, sel)
        occ, nseq, totals = triple_loop(seqs, k, canonical, sel)
        assert np.array_equal(got.occ, occ) and np.array_equal(got.nseq, nseq), case
        assert tuple(got.totals.tolist()) == totals, case
        assert (got.nseq <= got.occ).all() and (got.nseq <= got.n_seqs).all()
    assert np.array_equal(kmers.kmer_counts_host([b"ACGT"], 2).occ, kmers.kmer_counts_host(["ACGT"], 2).occ)


def test_shards_add_up():
    rng = random.Random(3)
    seqs = random_seqs(rng, 12, 60)
    whole = kmers.kmer_counts_host(seqs, 3, True)
    parts = kmers.kmer_counts_host(seqs[:5], 3, True) + kmers.kmer_counts_host(seqs[5:], 3, True)
    assert np.array_equal(whole.occ, parts.occ) and np.array_equal(whole.nseq, parts.nseq)
    assert np.array_equal(whole.totals, parts.totals)
    with pytest.raises(ValueError):
        whole + kmers.kmer_counts_host(seqs, 3, False)


def test_markov_rows():
    # ACGTACGTA: AC, CG, GT, TA twice each
    kc = kmers.kmer_counts_host(["ACGTACGTA"], 2)
    assert {c: int(n) for c, n in enumerate(kc.occ) if n} == {1: 2, 6: 2, 11: 2, 12: 2}
    m = kc.markov()
    assert m.shape == (4, 4) and np.allclose(m.sum(axis=1), 1.0)
    want = np.array([[1, 3, 1, 1], [1, 1, 3, 1], [1, 1, 1, 3], [3, 1, 1, 1]]) / 6.0
    assert np.allclose(m, want, rtol=0, atol=1e-15)
    assert np.array_equal(kc.markov(pseudocount=0), np.array([[0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1], [1, 0, 0, 0]], dtype=np.float64))
    m3 = kmers.kmer_counts_host(["ACGTACGTA"], 3).markov(0.5)
    assert m3.shape == (16, 4) and np.allclose(m3.sum(axis=1), 1.0)
    assert np.allclose(m3[kmers.encode("AC")], np.array([0.5, 0.5, 2.5, 0.5]) / 4.0)          # ACG twice
    assert np.allclose(m3[kmers.encode("AA")], 0.25)
    m1 = kmers.kmer_counts_host(["AACG"], 1).markov(0)
    assert m1.shape == (1, 4) and np.allclose(m1[0], [0.5, 0.25, 0.25, 0.0])
    assert np.allclose(kmers.kmer_counts_host(["AACG"], 1).frequencies(), [0.5, 0.25, 0.25, 0.0])
    with pytest.raises(ValueError):
        kmers.kmer_counts_host(["ACGT"], 2, canonical=True).markov()


def hand_counts(k, nseq, n_seqs):
    return kmers.KmerCounts(k, True, dense(nseq, k), dense(nseq, k), n_seqs, int(sum(nseq.values())), 0, 0)


def test_enrichment_on_hand_counts():
    inp, ctl = hand_counts(1, {0: 6, 1: 2, 2: 0}, 10), hand_counts(1, {0: 1, 1: 2, 2: 0}, 10)
    e = kmers.enrichment(inp, ctl)
    # code 0: a = 6 of 10, b = 1 of 10: p = 7 / 20, var = 0.35 * 0.65 * 0.2 = 0.0455
    assert math.isclose(e.log2_fold[0], math.log2(6.5 / 1.5), rel_tol=1e-14)
    z0 = 0.5 / math.sqrt(0.0455)
    assert math.isclose(e.z[0], z0, rel_tol=1e-13) and math.isclose(e.p_value[0], 0.5 * math.erfc(z0 / math.sqrt(2.0)), rel_tol=1e-13)
    assert 0.009 < e.p_value[0] < 0.01                                                   # z = 2.344: P = 0.0095
    # code 1: equal fractions; code 2: in neither set (variance 0)
    assert e.log2_fold[1] == 0.0 and e.z[1] == 0.0 and e.p_value[1] == 0.5
    assert e.log2_fold[2] == 0.0 and e.z[2] == 0.0 and e.p_value[2] == 0.5
    top = e.top(2)
    assert top[0][:4] == ("A", 0, 6, 1) and top[1][1] == 1 and len(e.top(10)) == 4
    # unequal set sizes: a = 3 of 4, b = 5 of 20: p = 8 / 24
    e2 = kmers.enrichment(hand_counts(1, {3: 3}, 4), hand_counts(1, {3: 5}, 20))
    assert math.isclose(e2.z[3], (0.75 - 0.25) / math.sqrt((1 / 3) * (2 / 3) * (1 / 4 + 1 / 20)), rel_tol=1e-13)
    assert math.isclose(e2.log2_fold[3], math.log2((3.5 / 4.5) / (5.5 / 20.5)), rel_tol=1e-14)
    with pytest.raises(ValueError):
        kmers.enrichment(inp, hand_counts(2, {}, 10))
    with pytest.raises(ValueError):
        kmers.enrichment(inp, hand_counts(1, {}, 0))


def test_seed_matrix():
    m = kmers.seed_matrix(kmers.encode("GATAAG"), 6)
    assert m.shape == (4, 6)
    assert [int(np.argmax(m[:, j])) for j in range(6)] == [2, 0, 3, 0, 0, 2]
    assert np.allclose(m.max(axis=0), math.log(0.85 / 0.25)) and np.allclose(m.min(axis=0), math.log(0.05 / 0.25))
    bg = np.array([0.3, 0.2, 0.2, 0.3])
    assert np.allclose(np.exp(kmers.seed_matrix(0, 2, bg, hit=0.7)) * bg[:, None], [[0.7, 0.7], [0.1, 0.1], [0.1, 0.1], [0.1, 0.1]])
    with pytest.raises(ValueError):
        kmers.seed_matrix(0, 2, hit=1.0)


def test_kmer_dims_are_sane():
    d = _lib.kmer_dims()
    assert d["threads"] % 64 == 0 and d["tile_bases"] % (32 * d["threads"]) == 0
    assert 1 <= d["lds_k"] <= 12 and d["sort_windows"] >= 64 and d["sort_seqs_per_block"] >= 1 and d["bitmap_budget_mib"] >= 2
    assert 4 * 4 ** d["lds_k"] <= 160 * 1024                                            # the block table fits a CU's LDS
    prev = _lib.kmer_bitmap_budget(4096)
    try:
        assert _lib.kmer_bitmap_budget(0) == 4096
    finally:
        _lib.kmer_bitmap_budget(prev)
    with pytest.raises(ValueError):
        _lib.kmer_bitmap_budget(-1)


def test_new_symbols_are_exported():
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("ms_seqset_kmer_counts", "ms_genome_kmer_counts", "ms_debug_kmer_dims", "ms_debug_kmer_bitmap_budget"):
        assert hasattr(L, name), name
    assert (_lib.MS_KMER_MAX_K, kmers.MAX_K) == (12, 12)
