"""Cases shared by tests/test_shuffle_host.py and tests/test_gpu_shuffle.py: the vectors of include/motifscan_amd.h's shuffle
specification, a hand-written set of awkward sequences, and the property checks a shuffle must pass whatever produced it."""
import numpy as np

from motifscan_amd import shuffle

HASH_VECTORS = [
    ((0, 0, 0, 0), 0x1957A7604E215178),
    ((1, 2, 3, 4), 0x1D4407EF703B1906),
    ((2 ** 64 - 1, 5, 6, 2 ** 62 | 7), 0xE29FAA2116BC6367),
]

VECTOR_IN = "ACGTACGGTCANNTTGACCAGTAGGCATnACGATTTTTTTTTTCAGAGAGAGAGAGC"
# (kind, seed, sequence index) -> output
VECTORS = [
    ("mono", 7, 0, "GAACTGGACTCNNACGATTGGCGATCTAnACAAGCGTAGATGTTGCGTAATTATTTG"),
    ("dinuc", 7, 0, "ACGGTCGTACANNTTGAGCATACCAGGTnACGAGAGAGAGATTTTTTTTTTCAGAGC"),
    ("dinuc", 7, 3, "ACGTCGGTACANNTAGACCATTGCAGGTnAGACAGAGAGAGAGCGATTTTTTTTTTC"),
    ("dinuc", 8, 0, "ACACGTCGGTANNTTACATGGCCAGAGTnAGAGCGATTTTTTTTTTCAGAGAGAGAC"),
]

# runs of 0, 1, 2, 3 bases, one letter, the low-complexity runs rejection sampling chokes on, non-ACGT letters of every kind
HAND_SET = [
    VECTOR_IN,
    "",
    "A",
    "AC",
    "ACG",
    "N",
    "NANCANACGN",
    "TTTTTTTTTTTTTTTTTTTT",
    "A" * 200 + "C",
    "AC" * 100 + "G",
    "A" * 50 + "C" * 50 + "A" * 50,
    "acgtRYKMacgtnnACGTTGCAxACGGT-ACTGACTGGTCA",
    "GATTACAGATTACANGATTACAGATTACAGATTACA",
    "",
    "CGCGCGCGCGCGATATATATATCGCGCGAT",
]

_ACGT = set("ACGTacgt")


def runs_of(seq):
    """[(start, end)] of the maximal ACGT runs, by a plain loop (not the module's own splitter)"""
    out, b = [], None
    for i, ch in enumerate(seq):
        if ch in _ACGT:
            if b is None:
                b = i
        elif b is not None:
            out.append((b, i))
            b = None
    if b is not None:
        out.append((b, len(seq)))
    return out


def check_properties(seq, out, kind):
    """What any shuffle of `seq` must keep: length, every non-ACGT character in place and verbatim, ACGT in upper case, per-run base
    counts; for dinuc per-run dinucleotide counts and both end bases."""
    assert len(out) == len(seq)
    for i, ch in enumerate(seq):
        if ch not in _ACGT:
            assert out[i] == ch, (i, ch, out[i])
        else:
            assert out[i] in "ACGT", (i, out[i])
    for b, e in runs_of(seq):
        src, dst = seq[b:e].upper(), out[b:e]
        assert sorted(src) == sorted(dst)
        if kind in ("dinuc", 2):
            assert src[0] == dst[0] and src[-1] == dst[-1]
            pairs = lambda s: sorted(s[i:i + 2] for i in range(len(s) - 1))
            assert pairs(src) == pairs(dst)
    if kind in ("dinuc", 2):
        a, b = shuffle.dinuc_counts(seq), shuffle.dinuc_counts(out)
        assert len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def random_sequence(rng, length, letters, dirt):
    """`length` characters over the first `letters` of ACGT, a fraction `dirt` of them replaced by N, n, IUPAC letters or lower case"""
    s = rng.choice(list("ACGT"[:letters]), size=length) if length else np.array([], dtype="<U1")
    s = s.astype("<U1")
    if length and dirt > 0:
        hit = rng.random(length) < dirt
        junk = rng.choice(list("NnRYKMSWBDHVacgt"), size=length)
        s = np.where(hit, junk, s)
    return "".join(s.tolist())
