"""
motifscan_amd.personal -- personal haplotypes: the alleles of an individual applied TOGETHER to a resident genome, on the device
(ms_genome_apply_alleles, ms_personal.hip), so that two variants closer than a motif width are seen on one haplotype and every
region-based entry point -- Scanner, the sweeps, the best-site and histogram scans, the batch stream -- runs on the individual's sequence.

    vcf = variants.read_vcf_alleles("sample.vcf.gz")
    hap0 = personal_genome(genome, vcf.chrom, vcf.pos, vcf.ref, vcf.alt, select=haplotype_mask("sample.vcf.gz", "NA12878", 0))
    personal, liftmap = hap0
    sites = Scanner(personal, ...)                       # unchanged
    ref_pos, inside = lift_sites(liftmap, chrom_idx, region_start, hit_pos)

`apply_alleles_host` restates the whole rule in plain sequential Python -- the order, the overlap rule, the splice of `bytes`, both lift
maps position by position -- and is what the GPU tests compare the device against.
"""
import gzip

import numpy as np

from . import _lib
from .variants import trim_allele

_ACGT = frozenset(b"ACGTacgt")


def _as_bytes(s):
    if isinstance(s, str):
        return s.encode("latin-1")
    if isinstance(s, np.ndarray):
        return s.tobytes()
    return bytes(s)


def _ref_differs(seq, x, want):
    """ms_scan_alleles' REF rule: case-insensitive; a non-ACGT genome base matches any letter that is not A, C, G or T."""
    for i, w in enumerate(want):
        g = seq[x + i]
        if w in _ACGT:
            if g not in _ACGT or (g | 0x20) != (w | 0x20):
                return True
        elif g in _ACGT:
            return True
    return False


def apply_alleles_host(chroms, chrom, pos, ref, alt, refs_check=None, skip_mismatch=False, lifts=True):
    """The rule of ms_genome_apply_alleles, sequentially, on the host.

    chroms: dict name -> sequence, or a list of sequences (insertion order = chromosome index); chrom: chromosome indices; pos: 0-based x;
    ref: per variant the replaced reference bases, as a string (its length is r) or as the number r itself; alt: the alt strings.
    refs_check: None, or the REF strings to compare with the chromosomes (`ref_mismatch`); with skip_mismatch a variant that differs gets
    status 2 and takes no further part.

    Returns a dict: seqs (the spliced chromosomes, bytes), sizes (int64), status (uint8 per variant: 1 applied, 0 overlap, 2 REF mismatch),
    ref_mismatch (uint8), n_applied, and per chromosome c the two lift maps written out for EVERY position: to_alt[c] = (out int64
    [L + 1], inside uint8 [L + 1]) and to_ref[c] = (out [L' + 1], inside [L' + 1]); lifts=False leaves the two maps out (they cost
    chromosome length x applied variants steps, written for clarity)."""
    seqs = [_as_bytes(s) for s in (chroms.values() if isinstance(chroms, dict) else chroms)]
    chrom, pos = [int(c) for c in chrom], [int(p) for p in pos]
    V = len(pos)
    rlen = [int(r) if isinstance(r, (int, np.integer)) else len(r) for r in ref]
    alts = [_as_bytes(a) for a in alt]
    mismatch = np.zeros(V, dtype=np.uint8)
    if refs_check is not None:
        for v in range(V):
            mismatch[v] = _ref_differs(seqs[chrom[v]], pos[v], _as_bytes(refs_check[v]))
    status = np.ones(V, dtype=np.uint8)
    takes_part = [v for v in range(V) if not (skip_mismatch and mismatch[v])]
    status[[v for v in range(V) if skip_mismatch and mismatch[v]]] = 2
    applied = [[] for _ in seqs]
    run_chrom, run_end = -1, 0
    for v in sorted(takes_part, key=lambda v: (chrom[v], pos[v], v)):
        if chrom[v] != run_chrom:
            run_chrom, run_end = chrom[v], 0
        if run_end > pos[v]:                                    # an earlier variant of the chromosome -- applied or not -- ends behind x
            status[v] = 0
        else:
            applied[chrom[v]].append(v)
        run_end = max(run_end, pos[v] + rlen[v])
    out_seqs, to_alt, to_ref = [], [], []
    for c, seq in enumerate(seqs):
        parts, cur = [], 0
        for v in applied[c]:
            parts += [seq[cur:pos[v]], alts[v]]
            cur = pos[v] + rlen[v]
        parts.append(seq[cur:])
        new = b"".join(parts)
        out_seqs.append(new)
        if not lifts:
            continue
        xs, rs, as_ = [pos[v] for v in applied[c]], [rlen[v] for v in applied[c]], [len(alts[v]) for v in applied[c]]
        xa, shift = [], 0
        for x, r, a in zip(xs, rs, as_):
            xa.append(x + shift)
            shift += a - r
        fwd, fin = np.zeros(len(seq) + 1, dtype=np.int64), np.zeros(len(seq) + 1, dtype=np.uint8)
        for p in range(len(seq) + 1):
            hit = [i for i in range(len(xs)) if xs[i] <= p < xs[i] + rs[i]]
            if hit:
                i = hit[0]
                fwd[p], fin[p] = xa[i] + min(p - xs[i], as_[i]), 1
            else:
                fwd[p] = p + sum(as_[j] - rs[j] for j in range(len(xs)) if xs[j] + rs[j] <= p)
        bwd, bin_ = np.zeros(len(new) + 1, dtype=np.int64), np.zeros(len(new) + 1, dtype=np.uint8)
        for q in range(len(new) + 1):
            hit = [i for i in range(len(xs)) if xa[i] <= q < xa[i] + as_[i]]
            if hit:
                i = hit[0]
                bwd[q], bin_[q] = xs[i] + min(q - xa[i], rs[i]), 1
            else:
                bwd[q] = q - sum(as_[j] - rs[j] for j in range(len(xs)) if xa[j] + as_[j] <= q)
        to_alt.append((fwd, fin))
        to_ref.append((bwd, bin_))
    return {"seqs": out_seqs, "sizes": np.array([len(s) for s in out_seqs], dtype=np.int64), "status": status, "ref_mismatch": mismatch,
            "n_applied": int((status == 1).sum()), "to_alt": to_alt, "to_ref": to_ref}


def personal_genome(genome, chrom, pos, ref, alt, select=None, on_mismatch="raise"):
    """Apply alleles (what `variants.read_vcf_alleles` returns: chromosome names, 0-based pos, ref and alt strings) to a
    _lib.ResidentGenome and return (personal ResidentGenome, _lib.LiftMap).  select: a boolean mask of the alleles to apply -- those of
    one haplotype (`haplotype_mask`); the map's `status` / `ref_mismatch` are per SELECTED allele, and `liftmap.selected` holds their
    indices in the caller's arrays.  Every REF is compared with the genome: on_mismatch='raise' raises ValueError naming the first few,
    'skip' leaves those alleles out (status 2), 'apply' applies them all the same.  Overlapping alleles are resolved by the library's rule
    (include/motifscan_amd.h); a KeyError for a chromosome the genome does not have."""
    if on_mismatch not in ("raise", "skip", "apply"):
        raise ValueError("on_mismatch must be 'raise', 'skip' or 'apply'")
    n = len(pos)
    if not (len(chrom) == len(ref) == len(alt) == n):
        raise ValueError("chrom, pos, ref and alt must have one entry per variant")
    sel = np.arange(n) if select is None else np.flatnonzero(np.asarray(select, dtype=bool))
    if select is not None and len(select) != n:
        raise ValueError("select must have one entry per variant")
    ref_s, alt_s = [str(ref[i]) for i in sel], [str(alt[i]) for i in sel]
    chrom_idx = np.array([genome.index[chrom[i]] for i in sel], dtype=np.int32)
    pos_s = np.ascontiguousarray(np.asarray(pos, dtype=np.int64)[sel])
    ref_len = np.array([len(r) for r in ref_s], dtype=np.int32)
    out, lm = _lib.apply_alleles(genome, chrom_idx, pos_s, ref_len, alt_s, refs=ref_s, skip_mismatch=on_mismatch == "skip")
    lm.selected = sel
    bad = np.flatnonzero(lm.ref_mismatch)
    if bad.size and on_mismatch == "raise":
        out.close()
        lm.close()
        shown = ", ".join(f"{chrom[sel[i]]}:{int(pos_s[i]) + 1} REF {ref_s[i]}" for i in bad[:5].tolist())
        raise ValueError(f"{bad.size} variant(s) whose REF is not the genome's sequence: {shown}" + (" ..." if bad.size > 5 else ""))
    return out, lm


def haplotype_mask(path, sample, hap, max_len=1000, trim=True):
    """Which alleles of a VCF one haplotype of one sample carries: a boolean array with one entry per allele `variants.read_vcf_alleles(path,
    max_len, trim)` returns, in its record order (the same records are left out: symbolic, '*', missing, too long).  sample: a column
    name of the #CHROM line, or its 0-based index; hap: 0 or 1, the side of a phased genotype a|b.  The entry of ALT allele k (1-based in
    its record) is True iff that haplotype's allele index is k.  An unphased genotype a/b cannot be assigned to a side: it counts -- for
    either haplotype -- only when homozygous; a missing allele '.' (or a haploid genotype asked for its second side) is False."""
    if hap not in (0, 1):
        raise ValueError("hap must be 0 or 1")
    out, col = [], None if isinstance(sample, str) else 9 + int(sample)
    opener = gzip.open if str(path).endswith(".gz") else open
    with opener(path, "rt") as fh:
        for line in fh:
            if line.startswith("#CHROM"):
                names = line.rstrip("\r\n").split("\t")[9:]
                if isinstance(sample, str):
                    if sample not in names:
                        raise KeyError(f"sample {sample!r} is not in the VCF (it has {names[:5]}{' ...' if len(names) > 5 else ''})")
                    col = 9 + names.index(sample)
                continue
            if not line.strip() or line.startswith("#"):
                continue
            f = line.rstrip("\r\n").split("\t")
            if len(f) < 5:
                raise ValueError(f"VCF line with fewer than 5 tab-separated columns: {line!r}")
            if col is None:
                raise ValueError("the VCF has no #CHROM line to look the sample up in")
            carried = None                                       # the haplotype's allele index, None: unknown
            if len(f) > col and len(f) > 8 and "GT" in f[8].split(":"):
                gt = f[col].split(":")[f[8].split(":").index("GT")] if len(f[col].split(":")) > f[8].split(":").index("GT") else "."
                if "|" in gt:
                    side = gt.split("|")
                    carried = side[hap] if hap < len(side) else None
                elif "/" in gt:
                    side = gt.split("/")
                    carried = side[0] if all(s == side[0] for s in side) else None
                else:
                    carried = gt if hap == 0 else None
                carried = int(carried) if carried is not None and carried.isdigit() else None
            r = f[3]
            for k, a in enumerate(f[4].split(","), start=1):
                if a == "." or r == "." or a == "*" or a.startswith("<") or "[" in a or "]" in a:
                    continue
                _, rr, aa = trim_allele(int(f[1]) - 1, r, a) if trim else (0, r, a)
                if len(rr) > max_len or len(aa) > max_len:
                    continue
                out.append(carried == k)
    return np.array(out, dtype=bool)


def lift_sites(liftmap, chrom_idx_of_region, region_start, hit_pos):
    """Hit positions on a personal genome in REFERENCE coordinates: per hit the chromosome index and the start of its region on the
    personal genome (index the per-region arrays with the hits' seq_idx first; scalars broadcast) and the hit's position in the region.
    Returns (ref_pos int64, inside uint8): inside = 1 for a start that lies in the alt bases of an applied variant and has no reference
    base of its own -- it maps to the variant's (AlleleSites.ref_start's convention)."""
    hit_pos = np.asarray(hit_pos, dtype=np.int64)
    start = np.broadcast_to(np.asarray(region_start, dtype=np.int64), hit_pos.shape)
    return liftmap.to_ref(np.broadcast_to(np.asarray(chrom_idx_of_region, dtype=np.int32), hit_pos.shape), start + hit_pos)
