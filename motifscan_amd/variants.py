"""
motifscan_amd.variants -- motif sites gained and lost by single-base substitutions, and by alleles of any length.

The reference has no counterpart: it scans regions, not alleles.  Here the genome is resident in HBM (a `_lib.ResidentGenome`), and
for every variant only the windows that cover it are scored, for both alleles, with the scan's own fp64 arithmetic and hit test
(cscore.c:336-390; ms_variants.hip).  `read_vcf` reads the variants, `scan_variants` runs them, `VariantSites` holds the flat result
arrays -- they are the interface; no writer is part of this module.

Alleles whose REF and ALT differ in length, or are longer than one base, take the second route: `read_vcf_alleles`, `scan_alleles` and
`AlleleSites` (ms_alleles.hip).  There the two haplotypes are scanned apiece -- the chromosome as it is, and the chromosome with the
allele spliced in -- and a record belongs to ONE haplotype, with a start in that haplotype's coordinates.

`best_alleles` and `AlleleEffects` are the dense form (ms_allelebest.hip): no cutoff, one best window per (motif, variant, haplotype) --
what ranking variants by motif disruption needs for every pair, also where neither allele passes a cutoff.
"""
import gzip
from collections import namedtuple

import numpy as np

from . import _lib

_STRAND_FLAG = {"both": 3, "+": 1, "-": 2}
_BASES = "ACGT"

VcfVariants = namedtuple("VcfVariants", ["chrom", "pos", "ref", "alt", "id", "skipped"])


def read_vcf(path):
    """The single-base substitutions of a VCF (plain text or .gz): tab-separated CHROM, POS (1-based in the file, 0-based here), ID, REF,
    ALT; '#' lines are skipped, a comma-separated ALT gives one variant per allele.  Only single-letter REF and ALT become variants; the
    rest is skipped and counted per reason in `.skipped`: 'indel' (alleles of different lengths), 'multi_base' (equal lengths > 1),
    'symbolic' (<...>), 'star' (*), 'missing' (.).  Returns VcfVariants(chrom names, pos int64, ref, alt, id, skipped)."""
    chrom, pos, ref, alt, ids = [], [], [], [], []
    skipped = {"indel": 0, "multi_base": 0, "symbolic": 0, "star": 0, "missing": 0}
    opener = gzip.open if str(path).endswith(".gz") else open
    with opener(path, "rt") as fh:
        for line in fh:
            if not line.strip() or line.startswith("#"):
                continue
            f = line.rstrip("\r\n").split("\t")
            if len(f) < 5:
                raise ValueError(f"VCF line with fewer than 5 tab-separated columns: {line!r}")
            r = f[3]
            for a in f[4].split(","):
                if a == "." or r == ".":
                    skipped["missing"] += 1
                elif a == "*":
                    skipped["star"] += 1
                elif a.startswith("<") or "[" in a or "]" in a:
                    skipped["symbolic"] += 1
                elif len(r) != len(a):
                    skipped["indel"] += 1
                elif len(r) > 1:
                    skipped["multi_base"] += 1
                else:
                    chrom.append(f[0])
                    pos.append(int(f[1]) - 1)
                    ref.append(r)
                    alt.append(a)
                    ids.append(f[2])
    return VcfVariants(np.array(chrom, dtype=object), np.array(pos, dtype=np.int64), np.array(ref, dtype="U1"), np.array(alt, dtype="U1"),
                       np.array(ids, dtype=object), skipped)


class VariantSites:
    """Flat records of a variant scan in the library's order (motif, variant index, start, '+' before '-'): motif, variant (index into
    the caller's arrays), start (0-based on the chromosome), strand (1 '+', 2 '-'), score_ref, score_alt, state (bit 0 ref passes,
    bit 1 alt passes), motif_offsets [P + 1]; `skipped` = indices of the variants dropped for a REF mismatch (on_mismatch='skip')."""

    def __init__(self, motif, variant, start, strand, score_ref, score_alt, state, motif_offsets, ref_codes=None, counts=None, skipped=None):
        self.motif = np.asarray(motif)
        self.variant = np.asarray(variant)
        self.start = np.asarray(start)
        self.strand = np.asarray(strand)
        self.score_ref = np.asarray(score_ref, dtype=np.float64)
        self.score_alt = np.asarray(score_alt, dtype=np.float64)
        self.state = np.asarray(state, dtype=np.uint8)
        self.motif_offsets = np.asarray(motif_offsets, dtype=np.int64)
        self.ref_codes = ref_codes
        self._counts = counts
        self.skipped = np.zeros(0, dtype=np.int64) if skipped is None else np.asarray(skipped, dtype=np.int64)

    def __len__(self):
        return len(self.state)

    @property
    def gained(self):
        return self.state == 2

    @property
    def lost(self):
        return self.state == 1

    @property
    def kept(self):
        return self.state == 3

    @property
    def delta(self):
        return self.score_alt - self.score_ref

    def motif_counts(self):
        """(gained, lost) int64 [P]: per motif the variants with at least one gained / lost site, as the device counted them (variants
        dropped by on_mismatch='skip' taken out again)."""
        if self._counts is None:
            raise ValueError("these sites do not come from a device scan")
        return self._counts


def _marshal(pwms, p_value):
    """Scanner._marshal: matrices and the cutoffs of `p_value`, the same ValueError for a PWM without that cutoff."""
    pwms = list(pwms)
    cutoffs = []
    for pwm in pwms:
        try:
            cutoffs.append(pwm.cutoffs[p_value])
        except (TypeError, KeyError):
            raise ValueError(f"PWM has no motif score cutoff set for P-value {p_value!r}")
    return [np.asarray(pwm.matrix, dtype=np.float64) for pwm in pwms], np.asarray(cutoffs, dtype=np.float64)


def scan_variants(genome, pwms, chrom, pos, alt, ref=None, strand="both", p_value="1e-4", on_mismatch="raise"):
    """Score the windows that cover each variant for both alleles (ms_scan_variants) and return the VariantSites.

    genome: a _lib.ResidentGenome; pwms: objects with .matrix (4 x W) and .cutoffs[p_value]; chrom: chromosome names (KeyError for one the
    genome does not have); pos: 0-based; alt (and ref): one letter per variant.  With `ref`, the genome's base at every variant is
    compared with it, case-insensitively (a non-ACGT genome base matches any letter that is not A, C, G or T): on_mismatch='raise' raises
    ValueError naming the first few, 'skip' drops those variants' records and lists them in `.skipped`."""
    if on_mismatch not in ("raise", "skip"):
        raise ValueError("on_mismatch must be 'raise' or 'skip'")
    if strand not in _STRAND_FLAG:
        raise ValueError("strand must be one of 'both', '+', '-'")
    matrices, cutoffs = _marshal(pwms, p_value)
    chrom_idx = np.array([genome.index[c] for c in chrom], dtype=np.int32)
    pos = np.ascontiguousarray(pos, dtype=np.int64)
    alt = np.asarray(alt, dtype="U1") if not isinstance(alt, (bytes, str)) else alt
    pw = _lib.PwmSet.from_matrices(matrices, cutoffs)
    try:
        res = _lib.scan_variants(pw, genome, chrom_idx, pos, alt, _STRAND_FLAG[strand])
    finally:
        pw.close()
    try:
        ref_codes = res.ref_codes()
        bad = np.zeros(0, dtype=np.int64)
        if ref is not None:
            letters = np.char.upper(np.asarray(ref, dtype="U1"))
            if letters.shape != ref_codes.shape:
                raise ValueError("ref must have one letter per variant")
            want = np.full(letters.shape, -1, dtype=np.int8)
            for code, base in enumerate(_BASES):
                want[letters == base] = code
            bad = np.flatnonzero(want != ref_codes)
            if bad.size and on_mismatch == "raise":
                shown = ", ".join(f"{chrom[i]}:{int(pos[i]) + 1} REF {letters[i]} but the genome has {_BASES[ref_codes[i]] if ref_codes[i] >= 0 else 'N'}"
                                  for i in bad[:5].tolist())
                raise ValueError(f"{bad.size} variant(s) whose REF is not the genome's base: {shown}" + (" ..." if bad.size > 5 else ""))
        s = res.sites()
        gained, lost = res.motif_counts()
    finally:
        res.close()
    if bad.size:
        drop = np.isin(s["variant"], bad)
        for name, col in (("gained", gained), ("lost", lost)):            # the dropped variants leave the counts too
            sel = drop & (s["state"] == (2 if name == "gained" else 1))
            pairs = np.unique(np.stack([s["motif"][sel].astype(np.int64), s["variant"][sel]]), axis=1)
            np.subtract.at(col, pairs[0], 1)
        keep = ~drop
        offsets = np.zeros(len(matrices) + 1, dtype=np.int64)
        np.cumsum(np.bincount(s["motif"][keep], minlength=len(matrices)), out=offsets[1:])
        s = {k: (v[keep] if k != "motif_offsets" else offsets) for k, v in s.items()}
    return VariantSites(s["motif"], s["variant"], s["start"], s["strand"], s["score_ref"], s["score_alt"], s["state"], s["motif_offsets"],
                        ref_codes=ref_codes, counts=(gained, lost), skipped=bad)


# ---------------------------------------------------------------------------------------------- alleles of any length

VcfAlleles = namedtuple("VcfAlleles", ["chrom", "pos", "ref", "alt", "id", "skipped"])


def trim_allele(pos, ref, alt):
    """The shared suffix, then the shared prefix, of REF and ALT removed (compared without case) and pos moved past the prefix: VCF's
    anchored AT -> A at p becomes T -> '' at p + 1.  Identical alleles are left as they are; nothing is left-aligned."""
    if ref.upper() == alt.upper():
        return pos, ref, alt
    ru, au = ref.upper(), alt.upper()
    n = min(len(ref), len(alt))
    k = 0
    while k < n and ru[len(ru) - 1 - k] == au[len(au) - 1 - k]:
        k += 1
    if k:
        ref, alt, ru, au = ref[:-k], alt[:-k], ru[:-k], au[:-k]
    n = min(len(ref), len(alt))
    k = 0
    while k < n and ru[k] == au[k]:
        k += 1
    return pos + k, ref[k:], alt[k:]


def read_vcf_alleles(path, max_len=1000, trim=True):
    """Every sequence-resolved allele of a VCF (plain text or .gz) -- substitutions, multi-base alleles, insertions, deletions -- read as
    `read_vcf` reads it: POS 0-based here, a comma-separated ALT gives one variant per allele.  trim=True applies `trim_allele`, so an
    insertion has ref '' and a deletion alt ''.  Skipped and counted per reason in `.skipped`: 'symbolic' (<...>, breakends), 'star' (*),
    'missing' (.), 'too_long' (REF or ALT of more than max_len bases, after trimming).
    Returns VcfAlleles(chrom names, pos int64, ref, alt, id, skipped); ref and alt are object arrays of str."""
    chrom, pos, ref, alt, ids = [], [], [], [], []
    skipped = {"symbolic": 0, "star": 0, "missing": 0, "too_long": 0}
    opener = gzip.open if str(path).endswith(".gz") else open
    with opener(path, "rt") as fh:
        for line in fh:
            if not line.strip() or line.startswith("#"):
                continue
            f = line.rstrip("\r\n").split("\t")
            if len(f) < 5:
                raise ValueError(f"VCF line with fewer than 5 tab-separated columns: {line!r}")
            r = f[3]
            for a in f[4].split(","):
                if a == "." or r == ".":
                    skipped["missing"] += 1
                elif a == "*":
                    skipped["star"] += 1
                elif a.startswith("<") or "[" in a or "]" in a:
                    skipped["symbolic"] += 1
                else:
                    x, rr, aa = trim_allele(int(f[1]) - 1, r, a) if trim else (int(f[1]) - 1, r, a)
                    if len(rr) > max_len or len(aa) > max_len:
                        skipped["too_long"] += 1
                        continue
                    chrom.append(f[0])
                    pos.append(x)
                    ref.append(rr)
                    alt.append(aa)
                    ids.append(f[2])
    obj = lambda items: np.array(items + [None], dtype=object)[:-1]         # (an object array whatever the strings' lengths)
    return VcfAlleles(obj(chrom), np.array(pos, dtype=np.int64), obj(ref), obj(alt), obj(ids), skipped)


class AlleleSites:
    """Flat records of an allele scan in the library's order (motif, variant index, allele, start, '+' before '-'): motif, variant (index
    into the caller's arrays), allele (0 ref haplotype, 1 alt haplotype), start (0-based, in THAT haplotype's coordinates), strand
    (1 '+', 2 '-'), score, motif_offsets [P + 1]; pos / ref_len / alt_len are the caller's variants (what `ref_start` needs); `skipped` =
    indices of the variants dropped for a REF mismatch (on_mismatch='skip')."""

    def __init__(self, motif, variant, allele, start, strand, score, motif_offsets, pos=None, ref_len=None, alt_len=None, counts=None, skipped=None):
        self.motif = np.asarray(motif)
        self.variant = np.asarray(variant, dtype=np.int64)
        self.allele = np.asarray(allele, dtype=np.uint8)
        self.start = np.asarray(start, dtype=np.int64)
        self.strand = np.asarray(strand)
        self.score = np.asarray(score, dtype=np.float64)
        self.motif_offsets = np.asarray(motif_offsets, dtype=np.int64)
        self.pos = None if pos is None else np.asarray(pos, dtype=np.int64)
        self.ref_len = None if ref_len is None else np.asarray(ref_len, dtype=np.int64)
        self.alt_len = None if alt_len is None else np.asarray(alt_len, dtype=np.int64)
        self._counts = counts
        self.skipped = np.zeros(0, dtype=np.int64) if skipped is None else np.asarray(skipped, dtype=np.int64)

    def __len__(self):
        return len(self.score)

    def ref_start(self):
        """The records' starts in reference coordinates: a ref-haplotype start, and an alt-haplotype start in front of the allele, is one
        already; an alt-haplotype start at or behind the allele's end x + a maps to start - a + r; one INSIDE the alt bases has no
        reference base of its own and maps to the allele's, x + min(start - x, r)."""
        if self.pos is None or self.ref_len is None or self.alt_len is None:
            raise ValueError("these sites carry no variants (pos, ref_len, alt_len)")
        x, r, a = self.pos[self.variant], self.ref_len[self.variant], self.alt_len[self.variant]
        behind = self.start - a + r
        inside = x + np.minimum(self.start - x, r)
        out = np.where(self.start >= x + a, behind, np.where(self.start > x, inside, self.start))
        return np.where(self.allele == 1, out, self.start)

    def per_variant(self):
        """One row per (motif, variant) that has records, in record order: dict of motif, variant, n_ref, n_alt (records on either
        haplotype, both strands), best_ref, best_alt (their highest score, NaN where there is none)."""
        n = len(self)
        if n == 0:
            z = np.zeros(0, dtype=np.int64)
            return {"motif": z.astype(np.int32), "variant": z, "n_ref": z, "n_alt": z, "best_ref": np.zeros(0), "best_alt": np.zeros(0)}
        motif = self.motif.astype(np.int64)
        first = np.flatnonzero(np.concatenate([[True], (motif[1:] != motif[:-1]) | (self.variant[1:] != self.variant[:-1])]))
        is_alt = self.allele == 1
        n_all = np.diff(np.concatenate([first, [n]]))
        n_alt = np.add.reduceat(is_alt.astype(np.int64), first)
        best = []
        for sel in (~is_alt, is_alt):
            b = np.maximum.reduceat(np.where(sel, self.score, -np.inf), first)
            best.append(np.where(np.isneginf(b), np.nan, b))
        return {"motif": self.motif[first], "variant": self.variant[first], "n_ref": n_all - n_alt, "n_alt": n_alt, "best_ref": best[0], "best_alt": best[1]}

    def motif_counts(self):
        """(gained, lost) int64 [P]: per motif the variants with records on the alt haplotype only / the ref haplotype only, as the
        device counted them (variants dropped by on_mismatch='skip' taken out again)."""
        if self._counts is None:
            raise ValueError("these sites do not come from a device scan")
        return self._counts


def scan_alleles(genome, pwms, chrom, pos, ref, alt, strand="both", p_value="1e-4", on_mismatch="raise"):
    """Score the windows each allele touches on the ref and on the alt haplotype (ms_scan_alleles) and return the AlleleSites.

    genome: a _lib.ResidentGenome; pwms: objects with .matrix (4 x W) and .cutoffs[p_value]; chrom: chromosome names (KeyError for one the
    genome does not have); pos: 0-based; ref / alt: one string per variant, '' for an insertion's ref / a deletion's alt (what
    `read_vcf_alleles` returns).  Every ref is compared with the genome, case-insensitively (a non-ACGT genome base matches any letter that
    is not A, C, G or T): on_mismatch='raise' raises ValueError naming the first few, 'skip' drops those variants' records and lists them
    in `.skipped`."""
    if on_mismatch not in ("raise", "skip"):
        raise ValueError("on_mismatch must be 'raise' or 'skip'")
    if strand not in _STRAND_FLAG:
        raise ValueError("strand must be one of 'both', '+', '-'")
    matrices, cutoffs = _marshal(pwms, p_value)
    ref, alt = [str(r) for r in ref], [str(a) for a in alt]
    chrom_idx = np.array([genome.index[c] for c in chrom], dtype=np.int32)
    pos = np.ascontiguousarray(pos, dtype=np.int64)
    ref_len = np.array([len(r) for r in ref], dtype=np.int32)
    alt_len = np.array([len(a) for a in alt], dtype=np.int64)
    pw = _lib.PwmSet.from_matrices(matrices, cutoffs)
    try:
        res = _lib.scan_alleles(pw, genome, chrom_idx, pos, ref_len, alt, refs=ref, strand_mask=_STRAND_FLAG[strand])
    finally:
        pw.close()
    try:
        bad = np.flatnonzero(res.ref_mismatch())
        if bad.size and on_mismatch == "raise":
            shown = ", ".join(f"{chrom[i]}:{int(pos[i]) + 1} REF {ref[i]}" for i in bad[:5].tolist())
            raise ValueError(f"{bad.size} variant(s) whose REF is not the genome's sequence: {shown}" + (" ..." if bad.size > 5 else ""))
        s = res.sites()
        gained, lost = res.motif_counts()
    finally:
        res.close()
    if bad.size:
        drop = np.isin(s["variant"], bad)
        gone = AlleleSites(s["motif"][drop], s["variant"][drop], s["allele"][drop], s["start"][drop], s["strand"][drop], s["score"][drop],
                           s["motif_offsets"]).per_variant()                 # the dropped variants leave the counts too
        np.subtract.at(gained, gone["motif"][gone["n_ref"] == 0], 1)
        np.subtract.at(lost, gone["motif"][gone["n_alt"] == 0], 1)
        keep = ~drop
        offsets = np.zeros(len(matrices) + 1, dtype=np.int64)
        np.cumsum(np.bincount(s["motif"][keep], minlength=len(matrices)), out=offsets[1:])
        s = {k: (v[keep] if k != "motif_offsets" else offsets) for k, v in s.items()}
    return AlleleSites(s["motif"], s["variant"], s["allele"], s["start"], s["strand"], s["score"], s["motif_offsets"], pos=pos, ref_len=ref_len,
                       alt_len=alt_len, counts=(gained, lost), skipped=bad)


# ---------------------------------------------------------------------------------------------- the best site per (motif, variant, haplotype)

class AlleleEffects:
    """The dense result of `best_alleles`: per (motif, variant) the best-scoring affected window of the ref and of the alt haplotype.
    score_ref / score_alt (float64), offset_ref / offset_alt (int32: winning start - pos, in that haplotype's coordinates) and
    strand_ref / strand_alt (int8: 1 '+', 2 '-') are (P, V) arrays; a cell without a winner holds NaN / 0 / 0 (strand == 0 marks it).
    pos / ref_len / alt_len are the caller's variants; `skipped` = indices of the variants blanked for a REF mismatch
    (on_mismatch='skip')."""

    def __init__(self, score_ref, score_alt, offset_ref, offset_alt, strand_ref, strand_alt, pos, ref_len, alt_len, skipped=None):
        self.score_ref = np.asarray(score_ref, dtype=np.float64)
        self.score_alt = np.asarray(score_alt, dtype=np.float64)
        self.offset_ref = np.asarray(offset_ref, dtype=np.int32)
        self.offset_alt = np.asarray(offset_alt, dtype=np.int32)
        self.strand_ref = np.asarray(strand_ref, dtype=np.int8)
        self.strand_alt = np.asarray(strand_alt, dtype=np.int8)
        self.pos = np.asarray(pos, dtype=np.int64)
        self.ref_len = np.asarray(ref_len, dtype=np.int64)
        self.alt_len = np.asarray(alt_len, dtype=np.int64)
        self.skipped = np.zeros(0, dtype=np.int64) if skipped is None else np.asarray(skipped, dtype=np.int64)

    @property
    def shape(self):
        return self.score_ref.shape

    @property
    def delta(self):
        """score_alt - score_ref, NaN where either haplotype has no winner."""
        return self.score_alt - self.score_ref

    def start_ref(self):
        """The winning start on the ref haplotype (reference coordinates), -1 where there is no winner."""
        return np.where(self.strand_ref != 0, self.pos[None, :] + self.offset_ref, -1)

    def start_alt(self):
        """The winning start on the alt haplotype, in ALT-haplotype coordinates, -1 where there is no winner."""
        return np.where(self.strand_alt != 0, self.pos[None, :] + self.offset_alt, -1)

    def start_alt_in_ref(self):
        """start_alt() in reference coordinates, by `AlleleSites.ref_start`'s rule: a start in front of the allele is one already; one at
        or behind the allele's end x + a maps to start - a + r; one INSIDE the alt bases maps to x + min(start - x, r); -1: no winner."""
        x, r, a = self.pos[None, :], self.ref_len[None, :], self.alt_len[None, :]
        start = x + self.offset_alt
        out = np.where(start >= x + a, start - a + r, np.where(start > x, x + np.minimum(start - x, r), start))
        return np.where(self.strand_alt != 0, out, -1)


def best_alleles(genome, pwms, chrom, pos, ref, alt, strand="both", on_mismatch="raise", motif_batch=None):
    """The best-scoring affected window of every (motif, variant) on the ref and on the alt haplotype (ms_scan_alleles_best): the
    cutoff-free, dense counterpart of `scan_alleles`.  Returns an AlleleEffects.

    genome, chrom, pos, ref, alt and on_mismatch as in `scan_alleles` ('skip' sets the variant's columns to the no-winner triple and
    lists it in `.skipped`); pwms: objects with .matrix (4 x W) -- no cutoffs are needed.  motif_batch: motifs copied from the device
    per step (None: all at once)."""
    if on_mismatch not in ("raise", "skip"):
        raise ValueError("on_mismatch must be 'raise' or 'skip'")
    if strand not in _STRAND_FLAG:
        raise ValueError("strand must be one of 'both', '+', '-'")
    if motif_batch is not None and int(motif_batch) < 1:
        raise ValueError("motif_batch must be at least 1")
    matrices = [np.asarray(pwm.matrix, dtype=np.float64) for pwm in pwms]
    ref, alt = [str(r) for r in ref], [str(a) for a in alt]
    pos = np.ascontiguousarray(pos, dtype=np.int64)
    if not (len(chrom) == len(pos) == len(ref) == len(alt)):
        raise ValueError("chrom, pos, ref and alt must have one entry per variant")
    chrom_idx = np.array([genome.index[c] for c in chrom], dtype=np.int32)
    ref_len = np.array([len(r) for r in ref], dtype=np.int32)
    alt_len = np.array([len(a) for a in alt], dtype=np.int64)
    P, V = len(matrices), len(pos)
    pw = _lib.PwmSet.from_matrices(matrices)
    try:
        res = _lib.scan_alleles_best(pw, genome, chrom_idx, pos, ref_len, alt, refs=ref, strand_mask=_STRAND_FLAG[strand])
    finally:
        pw.close()
    try:
        bad = np.flatnonzero(res.ref_mismatch())
        if bad.size and on_mismatch == "raise":
            shown = ", ".join(f"{chrom[i]}:{int(pos[i]) + 1} REF {ref[i]}" for i in bad[:5].tolist())
            raise ValueError(f"{bad.size} variant(s) whose REF is not the genome's sequence: {shown}" + (" ..." if bad.size > 5 else ""))
        out = {k: np.zeros((P, V), dtype=t) for k, t in (("score_ref", np.float64), ("score_alt", np.float64), ("offset_ref", np.int32),
                                                          ("offset_alt", np.int32), ("strand_ref", np.int8), ("strand_alt", np.int8))}
        step = P if motif_batch is None else int(motif_batch)
        for m0 in range(0, P, max(step, 1)):
            part = res.sites(m0, min(P, m0 + step))
            for k in out:
                out[k][m0:m0 + step] = part[k]
    finally:
        res.close()
    if bad.size:
        for k in out:
            out[k][:, bad] = np.nan if k.startswith("score") else 0
    return AlleleEffects(out["score_ref"], out["score_alt"], out["offset_ref"], out["offset_alt"], out["strand_ref"], out["strand_alt"],
                         pos, ref_len, alt_len, skipped=bad)
