"""
motif --build's genome-wide jobs on the device (ms_background.hip): cal_bg_freq's base counts, Genome.random_sequences' seeded
sampling and build_motif's cutoffs, against the reference's own known answers (its toy genome, tests/golden/ref_genome.json), the
goldens made by the real reference (tests/golden/ref_build.npz, make_golden_build.py) and host recomputations.
"""
import json
import os

import numpy as np
import pytest

from fuzz_parity import ref_random_sequences          # Genome.random_sequences restated step by step (shared with the genome fuzz family)
from motifscan_amd import _lib, build, genome, matrix

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def _device():
    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible")
    _lib.set_device(0)


@pytest.fixture(scope="module")
def gold():
    d = np.load(os.path.join(ROOT, "tests", "golden", "ref_build.npz"))
    out = {k: d[k] for k in d.files}
    names = [str(n) for n in out["names"]]
    raw = out["chrom_bytes"].tobytes().decode("ascii")
    off = np.concatenate([[0], np.cumsum(out["chrom_sizes"])])
    out["chroms"] = {n: raw[off[i]:off[i + 1]] for i, n in enumerate(names)}
    return out


@pytest.fixture(scope="module")
def gold_genome(gold):
    pg = genome.PackedGenome.from_arrays(list(gold["chroms"]), list(gold["chroms"].values()))
    rg = pg.to_resident()
    yield pg, rg
    rg.close()


def _state(d, i):
    return "MT19937", d[f"samp{i}_key"], int(d[f"samp{i}_pos"][0]), int(d[f"samp{i}_pos"][1]), float(d[f"samp{i}_gauss"][0])


def _same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


@pytest.fixture(scope="module")
def toy(tmp_path_factory):
    with open(os.path.join(ROOT, "tests", "golden", "ref_genome.json")) as fh:
        g = json.load(fh)
    d = tmp_path_factory.mktemp("toy")
    for name, text in g["files"].items():
        (d / name).write_text(text)
    return str(d / "test.fa"), g


def test_reference_known_answers_on_its_toy_genome(toy):
    fasta, g = toy                                        # tests/test_genome_class.py:24-47
    pg = genome.PackedGenome.from_fasta(fasta)
    assert list(pg.random_sequences(n_times=3, length=5, random_seed=1)) == ["AAAAA", "AaTtC", "AAAaC"]
    rg = pg.to_resident()
    try:
        assert list(rg.random_sequences(n_times=3, length=5, random_seed=1)) == ["AAAAA", "AaTtC", "AAAaC"]
        assert len(list(rg.random_sequences(n_times=3, length=5))) == 3
        for src in (fasta, pg, rg):
            assert genome.cal_bg_freq(src, skip_non_autosomes=True) == {"A": 0.3, "C": 0.3, "G": 0.15, "T": 0.25}
            assert genome.cal_bg_freq(src, skip_non_autosomes=False) == {"A": 0.51111, "C": 0.22222, "G": 0.11111, "T": 0.15556}
        path = pg.save(os.path.join(os.path.dirname(fasta), "toy.msg"))
        assert genome.cal_bg_freq(path) == {"A": 0.3, "C": 0.3, "G": 0.15, "T": 0.25}
        # a chromosome shorter than the window: numpy's ValueError at the attempt where the reference draws it, and its state
        np.random.seed(3)
        s0 = np.random.get_state()
        with pytest.raises(ValueError, match="high <= 0"):
            ref_random_sequences(g["whole"], 50, 12, 0)
        want = np.random.get_state()
        np.random.set_state(s0)
        with pytest.raises(ValueError, match="high <= 0"):
            rg.random_windows(50, 12)
        assert _same_state(np.random.get_state(), want)
    finally:
        rg.close()


def test_golden_sampling_cases_byte_for_byte(gold, gold_genome):
    pg, rg = gold_genome
    for i in range(4):
        n, length, max_n, seed = (int(x) for x in gold[f"samp{i}_args"])
        want = gold[f"samp{i}_seqs"].tobytes().decode("ascii")
        want = [want[k * length:(k + 1) * length] for k in range(n)]
        for src in (rg, pg):
            if seed == -1:
                np.random.seed(int(gold["samp_pre_seed"]))
            got = list(src.random_sequences(n, length, max_n, None if seed == -1 else seed))
            assert got == want, f"case {i}"
            assert _same_state(np.random.get_state(), _state(gold, i)), f"case {i}: global RandomState"


def test_iupac_letters_are_not_n():
    chroms = {"chrA": "RYKMSWrykmsw" * 5, "chrB": "N" * 40 + "ACGT" * 5, "chrC": "acgtRNNa" * 8}
    pg = genome.PackedGenome.from_arrays(list(chroms), list(chroms.values()))
    for max_n in (0, 1, 3):
        np.random.seed(8)
        want = ref_random_sequences(chroms, 500, 9, max_n)
        s_want = np.random.get_state()
        np.random.seed(8)
        got = list(pg.random_sequences(500, 9, max_n))
        assert got == want and _same_state(np.random.get_state(), s_want)
        if max_n == 0:
            assert any(set(s) <= set("RYKMSWrykmsw") for s in got)     # windows of IUPAC letters only, accepted at max_n = 0
    rg = _lib.ResidentGenome(chroms)                                     # no host side: the exception list is unknown
    try:
        with pytest.raises(RuntimeError, match="keep_host"):
            rg.random_windows(10, 9)
    finally:
        rg.close()
    rg = _lib.ResidentGenome(chroms, keep_host=True)
    try:
        np.random.seed(8)
        want = ref_random_sequences(chroms, 500, 9, 0)
        np.random.seed(8)
        assert list(rg.random_sequences(500, 9, 0)) == want
    finally:
        rg.close()


def test_background_frequencies_equal_the_goldens(gold, gold_genome):
    pg, rg = gold_genome
    for src in (rg, pg):
        assert genome.cal_bg_freq(src) == dict(zip("ACGT", gold["bg_skip"].tolist()))
        assert genome.cal_bg_freq(src, skip_non_autosomes=False) == dict(zip("ACGT", gold["bg_all"].tolist()))


def test_base_counts_of_100_mbp_equal_numpy_counts():
    rng = np.random.default_rng(4)
    sizes = [int(x) | 1 for x in rng.integers(1_000_000, 9_000_000, size=20)]
    sizes += [0, 1, 5, 31, 33, 7, 0, 64, 3] + [int(x) for x in rng.integers(1, 40, size=300)]     # many contigs inside one unit / block
    sizes += [int(x) for x in rng.integers(1_000_000, 9_000_000, size=6)]
    assert all(s % 32 for s in sizes[:20])
    alphabet = np.frombuffer(b"ACGTacgtNnRYkm", dtype=np.uint8)
    p = np.array([0.2, 0.15, 0.15, 0.2, 0.07, 0.05, 0.05, 0.07, 0.03, 0.01, 0.005, 0.005, 0.005, 0.005])
    seqs = [alphabet[rng.choice(alphabet.size, size=s, p=p / p.sum())] for s in sizes]
    assert sum(sizes) > 100_000_000
    names = [f"c{i}" for i in range(len(sizes))]
    pg = genome.PackedGenome.from_arrays(names, seqs)
    rg = pg.to_resident()
    try:
        got = rg.base_counts()
    finally:
        rg.close()
    want = np.array([[np.count_nonzero((s | 0x20) == ord(b)) for b in "acgt"] for s in seqs], dtype=np.int64)
    assert np.array_equal(got, want)


def _pfm_set(gold):
    mats, o = [], 0
    for w in gold["pfm_widths"].tolist():
        mats.append(gold["pfm_counts"][o:o + 4 * w].reshape(4, w))
        o += 4 * w
    return matrix.MotifSet.from_matrices("pfm", mats)


def test_build_motif_cutoffs_bit_for_bit(gold, gold_genome, tmp_path):
    pg, rg = gold_genome
    keys = [str(k) for k in gold["cut_keys"]]
    out = str(tmp_path / "built.pwms")
    pwms = build.build_motif(_pfm_set(gold), rg, n_random=20000, n_repeat=3, seed=11, out_path=out)
    assert np.array_equal(pwms.flat()[0], gold["pwm_values"])
    got = np.array([[c[k] for k in keys] for c in pwms.cutoffs])
    assert np.array_equal(got, gold["cut_seed11"])
    assert os.path.getsize(out) > 0
    np.random.seed(int(gold["cut_none_pre_seed"]))
    pwms = build.build_motif(_pfm_set(gold), pg, n_random=20000, n_repeat=1, seed=None)
    got = np.array([[c[k] for k in keys] for c in pwms.cutoffs])
    assert np.array_equal(got, gold["cut_none"])


def test_a_million_windows_match_the_host_replay_and_numpy_n_counts():
    rng = np.random.default_rng(12)
    sizes = [2_000_003, 1_500_007, 999_983, 700_001, 31]
    alphabet = np.frombuffer(b"ACGTacgtNnR", dtype=np.uint8)
    seqs = []
    for s in sizes:
        a = alphabet[rng.choice(8, size=s)]
        for _ in range(s // 2000):                                     # N runs
            k = int(rng.integers(0, s)); a[k:k + int(rng.integers(1, 60))] = ord("N") if rng.random() < 0.8 else ord("n")
        a[rng.choice(s, size=s // 500, replace=False)] = ord("R")
        seqs.append(a)
    names = ["chr2", "chr1", "chrZ", "chr10", "chr_small"]
    pg = genome.PackedGenome.from_arrays(names, seqs)
    n_times, length, max_n = 1_000_000, 30, 1
    rg = pg.to_resident()
    try:
        np.random.seed(77)
        ci, st = rg.random_windows(n_times, length, max_n)
        s_dev = np.random.get_state()
    finally:
        rg.close()
    # the same draws on the host: numpy's choice, the host replay, N counts from prefix sums of the bytes
    np.random.seed(77)
    order = sorted(names)
    sz = [sizes[names.index(c)] for c in order]
    rc = np.random.choice(len(order), size=n_times, p=[x / sum(sz) for x in sz])
    isn = [np.concatenate([[0], np.cumsum((s | 0x20) == ord("n"))]) for s in seqs]
    rep = genome.RandintReplay()
    att = np.arange(int(1.3 * n_times)) % n_times
    start, used = rep.draw(np.array(sz, dtype=np.int64)[rc[att]] - length)
    fidx = np.array([names.index(c) for c in order])[rc[att]]
    nn = np.array([isn[f][s + length] - isn[f][s] for f, s in zip(fidx.tolist(), start.tolist())])
    keep = np.flatnonzero(nn <= max_n)[:n_times]
    assert keep.size == n_times
    rep.commit(int(used[keep[-1]]))
    assert np.array_equal(ci, fidx[keep]) and np.array_equal(st, start[keep])
    assert _same_state(np.random.get_state(), s_dev)
