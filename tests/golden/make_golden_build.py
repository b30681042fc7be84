#!/usr/bin/env python3
"""
tests/golden/make_golden_build.py -- goldens of `motifscan motif --build`'s two genome-wide jobs, made by running the REAL reference
(MotifScan 1.3.0) where its source tree is present, the way make_golden.py does.  Nothing here needs a GPU and nothing here is product
code.

How the reference is reached (no reference source enters this repo):
  * make_golden.import_reference(): the reference tree (make_golden.REF) on sys.path, its cscore.c compiled unmodified into
    oracle/_ref/, an EMPTY `pysam` placeholder module;
  * cal_bg_freq opens its FASTA with pysam.FastaFile: the placeholder gets a minimal FastaFile stand-in over the genome held here as a
    dict (references, fetch, get_reference_length, close -- the four members cal_bg_freq calls);
  * Genome.random_sequences is called unbound on a dict-backed object with the members it reads (chroms, chrom_sizes, fetch_sequence:
    0-based half-open slices);
  * the cutoffs are cli/motif.py:101-155 step by step: PFM.to_ppm().to_pwm(bg), random_sequences(n_random, max_length, max_n, seed + i),
    the reference's c_score (strand 3) and get_score_cutoffs, the mean over the repeats and np.around(, 8).

Output: tests/golden/ref_build.npz
  genome          names (file order) + the chromosomes' bytes: N runs, lower case, IUPAC letters, names the skip rule matches, and one
                  chromosome of exactly 21 bases = the widest sampled length + 1 (the reference draws its start with randint(1): no word)
  samp_*          Genome.random_sequences cases (n_times, length, max_n, seed; seed -1 = None after np.random.seed(pre_seed)): the
                  sequences and numpy's global state after the call
  bg_skip / bg_all   cal_bg_freq with and without the skip rule
  pfm_*, cut_*    40 seeded PFMs and the cutoffs of motif --build for n_random = 20 000, n_repeat = 3, seed = 11 and for n_repeat = 1,
                  seed = None after np.random.seed(cut_none_pre_seed)

Usage:  python3 tests/golden/make_golden_build.py
"""
import os
import sys
from collections import defaultdict

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402

TINY = "chr3"
WMAX = 20


class DictFasta:
    """pysam.FastaFile stand-in over FASTAS[path] = {name: sequence} (file order)."""
    FASTAS = {}

    def __init__(self, path):
        self._c = self.FASTAS[path]
        self.references = tuple(self._c)

    def fetch(self, chrom, start, end):
        return self._c[chrom][start:end]

    def get_reference_length(self, chrom):
        return len(self._c[chrom])

    def close(self):
        pass


class DictGenome:
    """The members Genome.random_sequences reads (genome/__init__.py:88-176); records every window it cuts."""

    def __init__(self, chroms):
        self._c = dict(chroms)
        self.chrom_sizes = {k: len(v) for k, v in self._c.items()}
        self.chroms = sorted(self._c)
        self.cut = []

    def fetch_sequence(self, chrom, start, end):
        self.cut.append((chrom, start))
        return self._c[chrom][start:end]


def make_genome(rng):
    """Seeded synthetic chromosomes with N runs, soft-masked runs and IUPAC letters in both cases."""
    bgp = np.array([0.29, 0.21, 0.21, 0.29])
    sizes = {"chr1": 60013, "chr2": 45007, "chrX": 30011, TINY: WMAX + 1, "chrM": 20001, "chrUn_a": 21017, "chr7_random": 25031}
    chroms = {}
    for name, n in sizes.items():
        seq = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.choice(4, size=n, p=bgp)].copy()
        if n > 1000:
            for _ in range(rng.integers(8, 20)):                        # soft-masked runs
                a = int(rng.integers(0, n)); seq[a:a + int(rng.integers(50, 2000))] |= 0x20
            for _ in range(rng.integers(10, 30)):                       # N runs, some lower case
                a = int(rng.integers(0, n)); seq[a:a + int(rng.integers(1, 300))] = ord("N") if rng.random() < 0.7 else ord("n")
            iu = rng.choice(n, size=n // 400, replace=False)            # IUPAC letters
            seq[iu] = np.frombuffer(b"RYKMSWBDHVrykmswbdhv", dtype=np.uint8)[rng.integers(0, 20, size=iu.size)]
        chroms[name] = seq.tobytes().decode("ascii")
    return chroms


def state_arrays(st):
    return np.asarray(st[1], dtype=np.uint32), np.array([st[2], st[3]], dtype=np.int64), np.array([st[4]], dtype=np.float64)


def main():
    R = make_golden.import_reference()
    import pysam
    pysam.FastaFile = DictFasta
    from motifscan.genome import Genome, cal_bg_freq
    rng = np.random.default_rng(20261016)
    chroms = make_genome(rng)
    DictFasta.FASTAS["golden.fa"] = chroms
    save = {"names": np.array(list(chroms)), "chrom_bytes": np.frombuffer("".join(chroms.values()).encode(), dtype=np.uint8),
            "chrom_sizes": np.array([len(v) for v in chroms.values()], dtype=np.int64),
            "reference_version": np.array(R["version"])}
    bg_skip = cal_bg_freq("golden.fa", skip_non_autosomes=True)
    bg_all = cal_bg_freq("golden.fa", skip_non_autosomes=False)
    save["bg_skip"] = np.array([bg_skip[b] for b in "ACGT"])
    save["bg_all"] = np.array([bg_all[b] for b in "ACGT"])

    # sampling cases; the first one's seed is the first that draws the 21-base chromosome at length 20 (randint(1): the no-draw case)
    cases = [[3000, WMAX, 0, None], [2500, 12, 0, 7], [4000, 7, 2, 123], [2000, WMAX, 5, -1]]
    for s in range(1, 1000):
        g = DictGenome(chroms)
        list(Genome.random_sequences(g, 3000, WMAX, 0, s))
        if any(c == TINY for c, _ in g.cut):
            cases[0][3] = s
            break
    pre_seed = 99
    for i, (n, length, max_n, seed) in enumerate(cases):
        g = DictGenome(chroms)
        if seed == -1:
            np.random.seed(pre_seed)
        seqs = list(Genome.random_sequences(g, n, length, max_n, None if seed == -1 else seed))
        assert len(seqs) == n and len(g.cut) > n, "every case must reject windows"
        save[f"samp{i}_args"] = np.array([n, length, max_n, seed], dtype=np.int64)
        save[f"samp{i}_seqs"] = np.frombuffer("".join(seqs).encode(), dtype=np.uint8)
        save[f"samp{i}_key"], save[f"samp{i}_pos"], save[f"samp{i}_gauss"] = state_arrays(np.random.get_state())
        print(f"case {i}: n={n} length={length} max_n={max_n} seed={seed}: {len(g.cut)} attempts, "
              f"{sum(c == TINY for c, _ in g.cut)} on {TINY}")
    save["samp_pre_seed"] = np.array(pre_seed)

    # motif --build (cli/motif.py:101-155) for 40 PFMs of widths 5 ... 20
    widths = np.clip(rng.integers(5, WMAX + 1, size=40), 5, WMAX)
    widths[0] = WMAX
    pfms = [make_golden.random_pfm(rng, int(w)) for w in widths]
    pwms = [R["PFM"](p).to_ppm().to_pwm(bg_skip) for p in pfms]
    matrices = [p.matrix.tolist() for p in pwms]
    max_length = max(p.length for p in pwms)

    def build(n_random, n_repeat, seed):
        cutoffs_all = []
        for i in range(n_repeat):
            seqs = list(Genome.random_sequences(DictGenome(chroms), n_random, max_length, 0, None if seed is None else seed + i))
            cutoffs_all.append(R["get_score_cutoffs"](R["ext"].c_score(matrices, seqs, 3, 8)))
        out = []
        for i in range(len(pwms)):
            cut = defaultdict(list)
            for rep in cutoffs_all:
                for p_value, c in rep[i].items():
                    cut[p_value].append(c)
            out.append({p_value: np.around(np.mean(v), 8) for p_value, v in cut.items()})
        keys = list(out[0])
        return keys, np.array([[o[k] for k in keys] for o in out], dtype=np.float64)

    save["pfm_widths"] = widths.astype(np.int32)
    save["pfm_counts"] = np.concatenate([p.ravel() for p in pfms]).astype(np.int64)
    save["pwm_values"] = np.concatenate([np.asarray(p.matrix).ravel() for p in pwms])
    keys, save["cut_seed11"] = build(20000, 3, 11)
    save["cut_keys"] = np.array(keys)
    np.random.seed(2024)
    _, save["cut_none"] = build(20000, 1, None)
    save["cut_none_pre_seed"] = np.array(2024)
    out = os.path.join(HERE, "ref_build.npz")
    np.savez_compressed(out, **save)
    print(f"wrote {out} ({os.path.getsize(out)} bytes), bg {bg_skip} / {bg_all}, keys {keys}")


if __name__ == "__main__":
    main()
