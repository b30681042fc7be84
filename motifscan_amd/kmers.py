"""
motifscan_amd.kmers -- the k-mer spectrum of a sequence set or of a resident genome, counted on the device (ms_kmers.hip), and what is
made of it: a Markov background, the k-mer enrichment of one region set against another, the seed matrix of a k-mer.  The reference's
only composition statistic is cal_bg_freq (genome/__init__.py:179-220), the k = 1 case.

    encode(kmer) / decode(code, k) / revcomp_code(code, k)
        the code of a k-mer: first base most significant, A 0, C 1, G 2, T 3 -- numeric order is lexicographic order
    KmerCounts            k, canonical, occ [4^k] (windows per code), nseq [4^k] or None (sequences holding the code at least once), and
                          the four totals; a + b adds the counts of two shards
    kmer_counts_host(seqs, k, canonical=False, sel=None)
                          the definition of ms_seqset_kmer_counts restated over ASCII strings, one window at a time (tests)
    KmerCounts.markov(pseudocount=1.0)    float64 [4^(k-1)][4]: P(next base | the k - 1 bases before it), rows summing to 1
    KmerCounts.frequencies()              occ / counted windows
    enrichment(inp, ctl) -> KmerEnrichment: per k-mer the log2 fold of the fractions of sequences that hold it, a pooled two-proportion z
                          and its one-sided normal P-value; .top(n)
    seed_matrix(code, k, bg, hit=0.85)    the 4 x k natural-log-odds matrix of a seed k-mer, for _lib.PwmSet.from_matrices / matrix.py

The device side is `_lib.SeqSet.kmer_counts`, `_lib.ResidentGenome.kmer_counts` and `Scanner.kmer_counts` / `Scanner.kmer_enrichment`.
There is no CPU path behind those: without a device they raise.
"""
import math
from collections import namedtuple

import numpy as np

MAX_K = 12
_CODE = {"A": 0, "C": 1, "G": 2, "T": 3, "a": 0, "c": 1, "g": 2, "t": 3}
_TOTALS = ("n_seqs", "n_windows", "n_skipped", "n_short")


def _check_k(k):
    k = int(k)
    if not 1 <= k <= MAX_K:
        raise ValueError(f"k must be in [1, {MAX_K}]")
    return k


def encode(kmer):
    """The code of a k-mer given as text: base j, 0-based from the left, at bits [2(k - 1 - j), 2(k - j))."""
    _check_k(len(kmer))
    code = 0
    for ch in kmer:
        if ch not in _CODE:
            raise ValueError(f"{ch!r} is not one of ACGT")
        code = code << 2 | _CODE[ch]
    return code


def decode(code, k):
    """The k-mer of a code, upper case."""
    k, code = _check_k(k), int(code)
    if not 0 <= code < 4 ** k:
        raise ValueError(f"code {code} outside [0, 4^{k})")
    return "".join("ACGT"[(code >> (2 * (k - 1 - j))) & 3] for j in range(k))


def revcomp_code(code, k):
    """The code of the reverse complement: sum_j (3 - b_j) << 2j."""
    k, code = _check_k(k), int(code)
    out = 0
    for _ in range(k):
        out = out << 2 | (3 - (code & 3))
        code >>= 2
    return out


_KmerCounts = namedtuple("KmerCounts", ["k", "canonical", "occ", "nseq", "n_seqs", "n_windows", "n_skipped", "n_short"])


class KmerCounts(_KmerCounts):
    """k; canonical; occ int64 [4^k]: the counted windows per code; nseq int64 [4^k] or None: the selected sequences that hold the code
    at least once; n_seqs: the selected sequences; n_windows: the counted windows (= occ.sum()); n_skipped: the windows left out for a
    non-ACGT base; n_short: the selected sequences shorter than k."""
    __slots__ = ()

    @property
    def totals(self):
        return np.array([self.n_seqs, self.n_windows, self.n_skipped, self.n_short], dtype=np.int64)

    def __add__(self, other):
        """The counts of two shards of the sequences (nseq included: a sequence lies wholly in one shard)."""
        if not isinstance(other, KmerCounts):
            return NotImplemented
        if (self.k, self.canonical) != (other.k, other.canonical):
            raise ValueError("the shards differ in k or in the canonical flag")
        nseq = None if self.nseq is None or other.nseq is None else self.nseq + other.nseq
        return KmerCounts(self.k, self.canonical, self.occ + other.occ, nseq, *(self.totals + other.totals).tolist())

    def frequencies(self):
        """float64 [4^k]: occ / counted windows (all zero when nothing was counted)."""
        n = float(self.n_windows)
        return self.occ / n if n > 0 else np.zeros(self.occ.shape, dtype=np.float64)

    def markov(self, pseudocount=1.0):
        """float64 [4^(k - 1)][4]: the conditional table of order k - 1 -- row p, column b: (occ[4p + b] + pseudocount) / (the row's
        sum), the probability of base b after the k - 1 bases of code p.  k = 1 gives one row, the base frequencies.  Needs a
        non-canonical count: folding a k-mer onto its reverse complement destroys the direction the table conditions on."""
        if self.canonical:
            raise ValueError("a Markov table needs non-canonical counts")
        pc = float(pseudocount)
        if pc < 0:
            raise ValueError("pseudocount must be >= 0")
        t = self.occ.reshape(-1, 4).astype(np.float64) + pc
        tot = t.sum(axis=1, keepdims=True)
        return np.divide(t, tot, out=np.full_like(t, 0.25), where=tot > 0)


def kmer_counts_host(seqs, k, canonical=False, sel=None):
    """The definition of ms_seqset_kmer_counts restated over ASCII strings (str or bytes), one window at a time.  Returns a KmerCounts
    with nseq."""
    k = _check_k(k)
    n_codes, mask = 4 ** k, 4 ** k - 1
    occ, nseq = np.zeros(n_codes, dtype=np.int64), np.zeros(n_codes, dtype=np.int64)
    n_seqs = n_windows = n_skipped = n_short = 0
    if sel is not None and len(sel) != len(seqs):
        raise ValueError("sel must hold one flag per sequence")
    for r, s in enumerate(seqs):
        if sel is not None and not sel[r]:
            continue
        if isinstance(s, (bytes, bytearray)):
            s = s.decode("latin-1")
        n_seqs += 1
        if len(s) < k:
            n_short += 1
            continue
        seen = {}
        fwd = rc = 0
        good = 0                                   # ACGT bases in a row up to and including position p
        for p, ch in enumerate(s):
            b = _CODE.get(ch)
            if b is None:
                good, fwd, rc = 0, 0, 0
            else:
                good += 1
                fwd = (fwd << 2 | b) & mask
                rc = rc >> 2 | (3 - b) << (2 * (k - 1))
            if p >= k - 1:                         # the window of starts p - k + 1 ends here
                if good >= k:
                    c = min(fwd, rc) if canonical else fwd
                    seen[c] = seen.get(c, 0) + 1
                else:
                    n_skipped += 1
        for c, n in seen.items():
            occ[c] += n
            nseq[c] += 1
            n_windows += n
    return KmerCounts(k, bool(canonical), occ, nseq, n_seqs, n_windows, n_skipped, n_short)


_KmerEnrichment = namedtuple("KmerEnrichment", ["k", "canonical", "n_inp", "n_ctl", "inp", "ctl", "log2_fold", "z", "p_value"])


class KmerEnrichment(_KmerEnrichment):
    """Per code: inp, ctl int64 [4^k] the sequences of either set that hold the k-mer; log2_fold; z; p_value (one-sided: enriched in
    the input); n_inp, n_ctl the sequences of either set."""
    __slots__ = ()

    def top(self, n=10):
        """The n most enriched k-mers as (kmer, code, inp, ctl, log2_fold, z, p_value), by z descending, ties by code."""
        order = np.lexsort((np.arange(self.z.size), -self.z))[:int(n)]
        return [(decode(c, self.k), int(c), int(self.inp[c]), int(self.ctl[c]), float(self.log2_fold[c]), float(self.z[c]), float(self.p_value[c]))
                for c in order.tolist()]


def enrichment(inp, ctl):
    """The k-mer enrichment of the input sequences against the control sequences, counted HOMER's way -- a sequence counts a k-mer at
    most once (the nseq planes), so one microsatellite does not make a k-mer enriched.  With a = inp.nseq, b = ctl.nseq, na, nb the
    sequences of either set:
        log2_fold = log2(((a + 0.5) / (na + 0.5)) / ((b + 0.5) / (nb + 0.5)))
        z         = (a / na - b / nb) / sqrt(p (1 - p) (1 / na + 1 / nb)),  p = (a + b) / (na + nb);  0 where that variance is 0
        p_value   = erfc(z / sqrt(2)) / 2"""
    if (inp.k, inp.canonical) != (ctl.k, ctl.canonical):
        raise ValueError("input and control differ in k or in the canonical flag")
    if inp.nseq is None or ctl.nseq is None:
        raise ValueError("both counts need their nseq plane")
    na, nb = int(inp.n_seqs), int(ctl.n_seqs)
    if na < 1 or nb < 1:
        raise ValueError("both sets need at least one sequence")
    a, b = inp.nseq.astype(np.float64), ctl.nseq.astype(np.float64)
    fold = np.log2(((a + 0.5) / (na + 0.5)) / ((b + 0.5) / (nb + 0.5)))
    p = (a + b) / (na + nb)
    var = p * (1.0 - p) * (1.0 / na + 1.0 / nb)
    z = np.divide(a / na - b / nb, np.sqrt(var), out=np.zeros_like(a), where=var > 0)
    uniq, inv = np.unique(z, return_inverse=True)                  # math.erfc once per distinct z: no scipy
    pv = np.array([0.5 * math.erfc(v / math.sqrt(2.0)) for v in uniq.tolist()], dtype=np.float64)[inv].reshape(z.shape)
    return KmerEnrichment(inp.k, inp.canonical, na, nb, inp.nseq, ctl.nseq, fold, z, pv)


def seed_matrix(code, k, bg=None, hit=0.85):
    """float64 [4][k], rows A, C, G, T: ln(p / bg) with p = hit for the seed's base of the column and (1 - hit) / 3 for the others --
    the natural-log-odds matrix of a seed k-mer, in the form _lib.PwmSet.from_matrices and matrix.py take.  bg: four background
    frequencies, uniform by default."""
    kmer = decode(code, k)
    hit = float(hit)
    if not 0.25 < hit < 1.0:
        raise ValueError("hit must be in (0.25, 1)")
    bg = np.full(4, 0.25) if bg is None else np.asarray(bg, dtype=np.float64)
    if bg.shape != (4,) or not (bg > 0).all():
        raise ValueError("bg must hold four frequencies > 0")
    p = np.full((4, len(kmer)), (1.0 - hit) / 3.0)
    for j, ch in enumerate(kmer):
        p[_CODE[ch], j] = hit
    return np.log(p / bg[:, None])
