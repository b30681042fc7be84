"""
Hand-written cases of ms_genome_apply_alleles' rule, shared by tests/test_personal_host.py (which pins personal.apply_alleles_host with
them) and tests/test_gpu_personal.py (which runs them on the device), and the seeded random cases of both.  Every expected string and
every lift map below was written out by hand from the rule in include/motifscan_amd.h, position by position -- nothing here is computed.

A case: chroms (list of bytes), variants [(chromosome, x, ref string, alt string)], check (compare the ref strings with the chromosomes),
skip (MS_APPLY_SKIP_MISMATCH), and the expected seqs, status, mismatch, to_alt / to_ref = per chromosome (out, inside).
"""
import numpy as np

S8 = b"ACGTACGT"


def ident(n, inside=()):
    """The identity map of a chromosome of n bases (n + 1 positions), inside = 1 at the given positions."""
    return list(range(n + 1)), [1 if p in inside else 0 for p in range(n + 1)]


CASES = {
    "substitution": dict(
        chroms=[S8], variants=[(0, 2, "G", "T")], seqs=[b"ACTTACGT"], status=[1],
        to_alt=[ident(8, [2])], to_ref=[ident(8, [2])]),
    "insertion": dict(
        chroms=[S8], variants=[(0, 2, "", "TT")], seqs=[b"ACTTGTACGT"], status=[1],
        to_alt=[([0, 1, 4, 5, 6, 7, 8, 9, 10], [0] * 9)],
        to_ref=[([0, 1, 2, 2, 2, 3, 4, 5, 6, 7, 8], [0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0])]),
    "deletion": dict(
        chroms=[S8], variants=[(0, 2, "GT", "")], seqs=[b"ACACGT"], status=[1],
        to_alt=[([0, 1, 2, 2, 2, 3, 4, 5, 6], [0, 0, 1, 1, 0, 0, 0, 0, 0])],
        to_ref=[([0, 1, 4, 5, 6, 7, 8], [0] * 7)]),
    "multi_base": dict(                                      # 3 -> 2 bases, one of them not ACGT
        chroms=[S8], variants=[(0, 1, "CGT", "NA")], seqs=[b"ANAACGT"], status=[1],
        to_alt=[([0, 1, 2, 3, 3, 4, 5, 6, 7], [0, 1, 1, 1, 0, 0, 0, 0, 0])],
        to_ref=[([0, 1, 2, 4, 5, 6, 7, 8], [0, 1, 1, 0, 0, 0, 0, 0])]),
    "insertion_at_0_and_L": dict(
        chroms=[S8], variants=[(0, 0, "", "GG"), (0, 8, "", "CC")], seqs=[b"GGACGTACGTCC"], status=[1, 1],
        to_alt=[([2, 3, 4, 5, 6, 7, 8, 9, 12], [0] * 9)],
        to_ref=[([0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 8, 8], [1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 0])]),
    "two_insertions_one_point": dict(                        # both applied, in input-index order
        chroms=[S8], variants=[(0, 4, "", "AA"), (0, 4, "", "CC")], seqs=[b"ACGTAACCACGT"], status=[1, 1],
        to_alt=[([0, 1, 2, 3, 8, 9, 10, 11, 12], [0] * 9)],
        to_ref=[([0, 1, 2, 3, 4, 4, 4, 4, 4, 5, 6, 7, 8], [0, 0, 0, 0, 1, 1, 1, 1, 0, 0, 0, 0, 0])]),
    "two_insertions_one_point_swapped": dict(
        chroms=[S8], variants=[(0, 4, "", "CC"), (0, 4, "", "AA")], seqs=[b"ACGTCCAAACGT"], status=[1, 1],
        to_alt=[([0, 1, 2, 3, 8, 9, 10, 11, 12], [0] * 9)],
        to_ref=[([0, 1, 2, 3, 4, 4, 4, 4, 4, 5, 6, 7, 8], [0, 0, 0, 0, 1, 1, 1, 1, 0, 0, 0, 0, 0])]),
    "insertion_then_substitution_at_x": dict(                # the insertion ends at x: it does not block the substitution at x
        chroms=[S8], variants=[(0, 4, "", "GG"), (0, 4, "A", "T")], seqs=[b"ACGTGGTCGT"], status=[1, 1],
        to_alt=[([0, 1, 2, 3, 6, 7, 8, 9, 10], [0, 0, 0, 0, 1, 0, 0, 0, 0])],
        to_ref=[([0, 1, 2, 3, 4, 4, 4, 5, 6, 7, 8], [0, 0, 0, 0, 1, 1, 1, 0, 0, 0, 0])]),
    "substitution_then_insertion_at_x": dict(                # the substitution ends at x + 1 > x: the insertion behind it is skipped
        chroms=[S8], variants=[(0, 4, "A", "T"), (0, 4, "", "GG")], seqs=[b"ACGTTCGT"], status=[1, 0],
        to_alt=[ident(8, [4])], to_ref=[ident(8, [4])]),
    "skipped_variant_still_blocks": dict(                    # A [0, 2), B [1, 5), C [3, 5): C is skipped although B is
        chroms=[S8], variants=[(0, 0, "AC", "TT"), (0, 1, "CGTA", "G"), (0, 3, "TA", "CC")], seqs=[b"TTGTACGT"], status=[1, 0, 0],
        to_alt=[ident(8, [0, 1])], to_ref=[ident(8, [0, 1])]),
    "duplicate": dict(
        chroms=[S8], variants=[(0, 2, "G", "T"), (0, 2, "G", "T")], seqs=[b"ACTTACGT"], status=[1, 0],
        to_alt=[ident(8, [2])], to_ref=[ident(8, [2])]),
    # REF "GA" is not the genome's "GT"; "t" is (case does not count)
    "ref_mismatch_unchecked": dict(
        chroms=[S8], variants=[(0, 2, "GA", "C"), (0, 3, "t", "G")], seqs=[b"ACCACGT"], status=[1, 0], mismatch=[0, 0],
        to_alt=[([0, 1, 2, 3, 3, 4, 5, 6, 7], [0, 0, 1, 1, 0, 0, 0, 0, 0])],
        to_ref=[([0, 1, 2, 4, 5, 6, 7, 8], [0, 0, 1, 0, 0, 0, 0, 0])]),
    "ref_mismatch_applied": dict(
        chroms=[S8], variants=[(0, 2, "GA", "C"), (0, 3, "t", "G")], check=True, seqs=[b"ACCACGT"], status=[1, 0], mismatch=[1, 0],
        to_alt=[([0, 1, 2, 3, 3, 4, 5, 6, 7], [0, 0, 1, 1, 0, 0, 0, 0, 0])],
        to_ref=[([0, 1, 2, 4, 5, 6, 7, 8], [0, 0, 1, 0, 0, 0, 0, 0])]),
    "ref_mismatch_skipped": dict(                            # ... and a variant that takes no part blocks nothing
        chroms=[S8], variants=[(0, 2, "GA", "C"), (0, 3, "t", "G")], check=True, skip=True, seqs=[b"ACGGACGT"], status=[2, 1], mismatch=[1, 0],
        to_alt=[ident(8, [3])], to_ref=[ident(8, [3])]),
    "ref_rule_non_acgt": dict(                               # a non-ACGT genome base matches any letter that is not A, C, G or T, and no other
        chroms=[b"ANGT"], variants=[(0, 1, "R", "C"), (0, 1, "A", "G")], check=True, skip=True, seqs=[b"ACGT"], status=[1, 2], mismatch=[0, 1],
        to_alt=[ident(4, [1])], to_ref=[ident(4, [1])]),
    "whole_chromosome_deleted": dict(
        chroms=[b"ACGT", b"GGCC"], variants=[(0, 0, "ACGT", "")], seqs=[b"", b"GGCC"], status=[1],
        to_alt=[([0, 0, 0, 0, 0], [1, 1, 1, 1, 0]), ident(4)],
        to_ref=[([4], [0]), ident(4)]),
    "insertion_into_empty_chromosome": dict(
        chroms=[b"", b"ACGT"], variants=[(0, 0, "", "TTT")], seqs=[b"TTT", b"ACGT"], status=[1],
        to_alt=[([3], [0]), ident(4)],
        to_ref=[([0, 0, 0, 0], [1, 1, 1, 0]), ident(4)]),
}


def case_args(case):
    """(chrom, pos, ref, alt, refs_check, skip) of a hand-written case"""
    v = case["variants"]
    ref = [x[2] for x in v]
    return [x[0] for x in v], [x[1] for x in v], ref, [x[3] for x in v], (ref if case.get("check") else None), bool(case.get("skip"))


def random_dna(rng, n, frac_n=0.05):
    s = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)].copy()
    s[rng.random(n) < frac_n] = ord("N")
    return s.tobytes()


def random_case(seed):
    """Three or four chromosomes of 40 .. 300 bases, one empty and one shorter than 32, and 1 .. 40 variants of random kinds: single
    substitutions, insertions, deletions, replacements, clustered around a few points so that they overlap, with duplicates, some REF
    strings falsified, in random input order.  Returns (chroms, chrom, pos, ref, alt)."""
    rng = np.random.default_rng(seed)
    lens = [int(rng.integers(40, 301)) for _ in range(int(rng.integers(1, 3)))] + [0, int(rng.integers(1, 32))]
    rng.shuffle(lens)
    chroms = [random_dna(rng, n) for n in lens]
    V = int(rng.integers(1, 41))
    centres = [(int(c), int(rng.integers(0, lens[c] + 1))) for c in rng.integers(0, len(lens), 4)]
    chrom, pos, ref, alt = [], [], [], []
    while len(pos) < V:
        if pos and rng.random() < 0.1:                          # a duplicate
            i = int(rng.integers(0, len(pos)))
            c, x, r, a = chrom[i], pos[i], len(ref[i]), len(alt[i])
        else:
            c, x0 = centres[int(rng.integers(0, 4))] if rng.random() < 0.6 else (int(rng.integers(0, len(lens))), None)
            L = lens[c]
            x = int(rng.integers(0, L + 1)) if x0 is None else min(L, max(0, x0 + int(rng.integers(-3, 4))))
            kind = rng.integers(0, 4)
            r = [1, 0, int(rng.integers(1, 6)), int(rng.integers(1, 40))][kind]
            a = [1, int(rng.integers(1, 40)), 0, int(rng.integers(1, 40))][kind]
            r = min(r, L - x)
            if r + a == 0:
                a = 1
        rs = chroms[c][x:x + r].decode()
        if r and rng.random() < 0.15:
            rs = ("T" if rs[0] in "Aa" else "A") + rs[1:]        # a REF that is not the genome's (or, on an N, one that is an ACGT letter)
        chrom.append(c)
        pos.append(x)
        ref.append(rs)
        alt.append(random_dna(rng, a, 0.1).decode())
    return chroms, chrom, pos, ref, alt
