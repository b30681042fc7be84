"""
motifscan_amd.build -- the score-cutoff half of `motifscan motif --build` on the GPU
(/root/reference/motifscan/cli/motif.py:119-153 and motif/__init__.py:378-401).

The reference scores n_random background sequences with every PWM (`c_score`, both strands), sorts
each PWM's scores in descending order and takes, for e = 2 .. min(len(str(n)), 7) - 1, the score
at index int(n * 0.1**e) - 1 as the cutoff for P-value 1e-e; over `n_repeat` samplings the cutoffs
are averaged and rounded to 8 decimals.  Here the scoring, the sorting and the rank pick run on the
device (ms_score_ranks); only the P x (number of P-values) cutoffs come back.  build_motif runs the whole
job against a resident genome: background frequencies, seeded window sampling and scoring all on the device,
with no sequence strings made.
"""
import numpy as np

from . import _lib


def cutoff_ranks(n_scores):
    """{'1e-2': rank, ...}: the 0-based ranks get_score_cutoffs reads for n_scores samples."""
    if n_scores < 100:
        raise ValueError("each motif must have at least 100 sampling scores")
    n_bits = min(len(str(n_scores)), 7)
    return {f"1e-{e}": int(n_scores * 0.1 ** e) - 1 for e in range(2, n_bits)}


def get_score_cutoffs(matrices, sequences, strand=3):
    """Per PWM a dict {p_value: cutoff} from ONE sampling (no averaging / rounding yet)."""
    pw = _lib.PwmSet.from_matrices(matrices)
    sq = _lib.SeqSet.from_strings(sequences)
    try:
        ranks = cutoff_ranks(sq.n_seqs)
        vals = _lib.score_ranks(pw, sq, list(ranks.values()), strand)
    finally:
        sq.close()
        pw.close()
    return [{k: float(vals[p, i]) for i, k in enumerate(ranks)} for p in range(len(matrices))]


def build_cutoffs(matrices, samplings, strand=3):
    """cli/motif.py:144-153: mean over the samplings' cutoffs, rounded to 8 decimals.
    samplings: list of sequence lists (one per repeat)."""
    per_repeat = [get_score_cutoffs(matrices, seqs, strand) for seqs in samplings]
    out = []
    for p in range(len(matrices)):
        keys = per_repeat[0][p].keys()
        out.append({k: float(np.around(np.mean([rep[p][k] for rep in per_repeat]), 8)) for k in keys})
    return out


def build_motif(pfms, genome, n_random=1_000_000, n_repeat=1, max_n=0, seed=None, bg_freq=None, strand=3, out_path=None):
    """cli/motif.py:101-155 without the config plumbing.  pfms: a 'pfm' MotifSet or a list of PFM motifs (formats.read_jaspar_pfms);
    genome: a ResidentGenome (kept on the device across repeats), a PackedGenome, a genome file or a FASTA path.
    PWMs = to_ppm().to_pwm(bg), bg = cal_bg_freq(genome) unless given; repeat i samples n_random windows of the widest PFM's length
    (Genome.random_sequences with seed + i, or the global state as it stands for seed=None), scores them (both strands for strand=3)
    and takes the get_score_cutoffs ranks; per P-value the cutoff is the mean over the repeats, np.around(, 8).
    Returns the PWM MotifSet with its cutoffs set; out_path: also written with formats.write_motifscan_pwms."""
    from . import formats, matrix
    from . import genome as _genome
    if isinstance(pfms, matrix.MotifSet):
        pfm_set = pfms
    else:
        pfms = list(pfms)
        pfm_set = matrix.MotifSet.from_matrices("pfm", [m.matrix for m in pfms], [m.name for m in pfms], [m.matrix_id for m in pfms])
    ranks = cutoff_ranks(int(n_random))
    resident, owned = _genome.open_resident(genome)
    try:
        if bg_freq is None:
            bg_freq = _genome.cal_bg_freq(resident)
        pwms = pfm_set.to_ppm().to_pwm(bg_freq)
        max_length = int(pwms.widths.max())
        vals, widths = pwms.flat()
        pw = _lib.PwmSet(vals, widths, None)
        per_repeat = []
        try:
            for i in range(int(n_repeat)):
                ci, st = resident.random_windows(n_random, max_length, max_n, None if seed is None else seed + i)
                sq = resident.extract(ci, st, st + max_length)
                try:
                    per_repeat.append(_lib.score_ranks(pw, sq, list(ranks.values()), strand))
                finally:
                    sq.close()
        finally:
            pw.close()
    finally:
        if owned:
            resident.close()
    for p in range(len(pwms)):
        pwms.cutoffs[p] = {k: float(np.around(np.mean([rep[p, i] for rep in per_repeat]), 8)) for i, k in enumerate(ranks)}
    if out_path is not None:
        formats.write_motifscan_pwms(out_path, pwms)
    return pwms
