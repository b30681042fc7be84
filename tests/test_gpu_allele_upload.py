"""
The upload that ms_scan_alleles, ms_scan_alleles_best and ms_genome_apply_alleles share (al_upload, ms_allele_dev.h), pinned from all
three sides at once: ONE variant set goes through the three entry points and the three ref_mismatch arrays must be equal to each other
and to a numpy restatement of the rule -- case-insensitive, and a non-ACGT genome base matches any letter that is not A, C, G or T.
129 variants (a tile of the record scan and one more) on two chromosomes of a few hundred bases, REF strings given and a few of them
wrong, one empty alt, one insertion at a chromosome's last position.
"""
import numpy as np
import pytest

from motifscan_amd import _lib

pytestmark = pytest.mark.gpu

ACGT = b"ACGT"
OTHER = b"NRYKMSWnrykmsw"


@pytest.fixture(scope="module", autouse=True)
def _device():
    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible")
    _lib.set_device(0)


def make_case():
    rng = np.random.default_rng(129)
    chroms = []
    for n in (317, 263):
        s = np.frombuffer(ACGT, dtype=np.uint8)[rng.integers(0, 4, n)].copy()
        s[rng.random(n) < 0.08] = ord("N")
        s[rng.random(n) < 0.03] = ord("R")
        lower = rng.random(n) < 0.2
        s[lower] |= 0x20
        chroms.append(s.tobytes())
    V = 129
    chrom = rng.integers(0, 2, V).astype(np.int32)
    ref_len = rng.integers(0, 6, V).astype(np.int32)
    pos = np.array([rng.integers(0, len(chroms[c]) - r + 1) for c, r in zip(chrom, ref_len)], dtype=np.int64)
    alts = [np.frombuffer(b"ACGTNacgtn", dtype=np.uint8)[rng.integers(0, 10, rng.integers(0 if r else 1, 6))].tobytes() for r in ref_len]
    # one empty alt (a deletion), one insertion at a chromosome's last position (x = L: no reference base behind it)
    ref_len[7], alts[7] = 3, b""
    pos[7] = min(pos[7], len(chroms[chrom[7]]) - 3)
    chrom[64], pos[64], ref_len[64], alts[64] = 1, len(chroms[1]), 0, b"GATTACA"
    refs, wrong = [], rng.random(V) < 0.15
    for v in range(V):
        c, x, r = chroms[chrom[v]], int(pos[v]), int(ref_len[v])
        s = bytearray(c[x:x + r])
        for i in range(r):
            if bytes([s[i]]).upper() in (b"A", b"C", b"G", b"T"):
                s[i] ^= 0x20 if rng.random() < 0.5 else 0                # either case
            else:
                s[i] = OTHER[rng.integers(0, len(OTHER))]                # any other letter for a non-ACGT genome base
        if wrong[v] and r:
            i = int(rng.integers(0, r))
            up = bytes([s[i]]).upper()
            if up in (b"A", b"C", b"G", b"T"):                           # another base, or a letter that is no base
                s[i] = OTHER[rng.integers(0, len(OTHER))] if rng.random() < 0.3 else ACGT[(ACGT.index(up) + int(rng.integers(1, 4))) % 4] ^ (0x20 * int(rng.integers(0, 2)))
            else:                                                        # a base where the genome has none
                s[i] = ACGT[rng.integers(0, 4)]
        refs.append(bytes(s))
    return chroms, chrom, pos, ref_len, alts, refs


def rule(chroms, chrom, pos, ref_len, refs):
    """The header's rule, byte by byte."""
    out = np.zeros(len(pos), dtype=np.uint8)
    for v in range(len(pos)):
        g = chroms[chrom[v]][int(pos[v]):int(pos[v]) + int(ref_len[v])].upper()
        for gb, rb in zip(g, refs[v].upper()):
            g_base, r_base = gb in ACGT, rb in ACGT
            if (r_base and (not g_base or gb != rb)) or (not r_base and g_base):
                out[v] = 1
    return out


def test_ref_mismatch_is_the_same_from_the_three_entry_points():
    chroms, chrom, pos, ref_len, alts, refs = make_case()
    want = rule(chroms, chrom, pos, ref_len, refs)
    assert len(pos) == 129 and 3 <= int(want.sum()) < 40 and alts[7] == b"" and pos[64] == len(chroms[1])
    g = _lib.ResidentGenome({f"c{i}": s for i, s in enumerate(chroms)})
    rng = np.random.default_rng(5)
    mats = [np.round(np.log2((rng.dirichlet(np.full(4, 0.4), size=w).T + 0.01) / 1.04 / 0.25), 5) for w in (6, 11)]
    pw = _lib.PwmSet.from_matrices(mats, [0.3, 0.3])
    al = _lib.scan_alleles(pw, g, chrom, pos, ref_len, alts, refs=refs)
    ab = _lib.scan_alleles_best(pw, g, chrom, pos, ref_len, alts, refs=refs)
    out, lm = _lib.apply_alleles(g, chrom, pos, ref_len, alts, refs=refs)
    got = [np.asarray(m).astype(np.uint8) for m in (al.ref_mismatch(), ab.ref_mismatch(), lm.ref_mismatch)]
    for m in got:
        assert m.shape == want.shape and np.array_equal(m, want)
    assert np.array_equal(got[0], got[1]) and np.array_equal(got[1], got[2])
    # without REF strings nothing is compared
    assert not np.asarray(_lib.scan_alleles(pw, g, chrom, pos, ref_len, alts).ref_mismatch()).any()
    for h in (al, ab, lm, out, pw, g):
        h.close()
