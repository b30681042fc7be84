"""
motif --build's genome-wide jobs, the host side (no device): the replay of numpy's legacy randint from raw words
(ms_randint_replay_host + genome.RandintReplay), the background-frequency text format, cal_bg_freq's skip rule, and the argument
errors the sampler raises before it touches a device.
"""
import os

import numpy as np
import pytest

from motifscan_amd import _lib, formats, genome

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


HIGHS = [
    [1, 1, 1, 2, 1, 3],                                                  # rng == 0 takes no word
    [2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 255, 256, 257, 65535, 65536, 65537],
    [2 ** 31 - 1, 2 ** 31, 2 ** 31 + 1, 2 ** 31 + 12345, 3 * 2 ** 30, 2 ** 32 - 1, 2 ** 32],
    [60013 - 20, 45007 - 20, 1, 30011 - 20, 2 ** 20 + 1, 2 ** 24 - 3],
]


@pytest.mark.parametrize("seed", [0, 1, 12345])
@pytest.mark.parametrize("mix", range(len(HIGHS)))
def test_replay_equals_sequential_randint_and_leaves_the_same_state(seed, mix):
    rng = np.random.default_rng(seed + 17 * mix)
    highs = np.array(HIGHS[mix], dtype=np.int64)[rng.integers(0, len(HIGHS[mix]), size=3000)]
    np.random.seed(seed)
    s0 = np.random.get_state()
    want = [np.random.randint(int(h)) for h in highs]
    s_want = np.random.get_state()
    np.random.set_state(s0)
    rep = genome.RandintReplay()
    got, used = rep.draw(highs[:1000])                  # in two pieces: the second continues the word stream
    got2, used2 = rep.draw(highs[1000:])
    rep.commit(int(used2[-1]))
    assert np.array_equal(np.concatenate([got, got2]), want)
    assert np.all(np.diff(np.concatenate([used, used2])) >= 0)
    assert _same_state(np.random.get_state(), s_want)


def test_replay_stops_where_the_words_run_out_and_refuses_what_numpy_would_not_draw():
    words = np.array([0xFFFFFFFF, 5, 0xFFFFFFFF, 0xFFFFFFFF], dtype=np.uint32)
    start, used, done = _lib.randint_replay(words, [10, 1, 10, 10])     # mask 15: 15 rejected, 5 taken; rng 0; then two rejections
    assert done == 2 and start[:2].tolist() == [5, 0] and used[:2].tolist() == [2, 2]
    for bad in ([0], [-3], [2 ** 32 + 1]):
        with pytest.raises(ValueError):
            _lib.randint_replay(words, bad)


def test_bg_freq_round_trip(tmp_path):
    bg = {"A": 0.3, "C": 0.3, "G": 0.15, "T": 0.25}
    p = str(tmp_path / "bg.txt")
    formats.write_bg_freq(p, bg)
    with open(p) as fh:
        assert fh.read() == "A\t0.3\nC\t0.3\nG\t0.15\nT\t0.25\n"
    assert formats.read_bg_freq(p) == bg
    odd = {"A": 0.28945, "C": 0.2129, "G": 0.20849, "T": 0.28916}
    formats.write_bg_freq(p, odd)
    assert formats.read_bg_freq(p) == odd


@pytest.mark.parametrize("text,line", [
    ("C\t0.3\nA\t0.3\nG\t0.15\nT\t0.25\n", 1),                     # the reference's test_bg_freq_bad1.txt: bases out of order
    ("A\t0.3\nC\tstring\nG\t0.15\nT\t0.25\n", 2),                  # ... bad2: not a number
    ("A\t0.3\nC 0.3\nG\t0.15\nT\t0.25\n", 2),                      # no tab
    ("A\t0.3\nC\t0.3\tx\nG\t0.15\nT\t0.25\n", 2),                  # three fields
    ("A\t0.3\nC\t0.3\n", 3),                                       # short file
])
def test_bg_freq_format_errors(tmp_path, text, line):
    p = tmp_path / "bad.txt"
    p.write_text(text)
    with pytest.raises(formats.BackgroundFormatError) as e:
        formats.read_bg_freq(str(p))
    assert e.value.line_num == line and f"line {line}" in str(e.value)
    assert isinstance(e.value, ValueError)


def test_skip_rule():
    skipped = ["chrX", "chrY", "chrM", "chrUn_gl000220", "chr1_gl000191_random", "chr6_apd_hap1", "chr1_KI270706v1_alt", "xchrXy"]
    kept = ["chr1", "chr22", "chrx", "chrUn", "chrUnplaced", "2L", "scaffold_7"]
    assert all(genome.is_non_autosome(n) for n in skipped)
    assert not any(genome.is_non_autosome(n) for n in kept)


def test_sampling_argument_errors_come_before_any_device_work():
    # a genome table with a chromosome of 2^32 + 21 bases: its starts would come from 64-bit words, which are not replayed
    offsets = np.array([0, 1000, 1000 + 2 ** 32 + 21], dtype=np.int64)
    pg = genome.PackedGenome(["chr1", "chr2"], offsets, None, None)
    with pytest.raises(ValueError, match="2\\^32"):
        pg.random_windows(10, 20)
    ok = genome.PackedGenome(["chr1", "chr2"], np.array([0, 1000, 1000 + 2 ** 32 + 20]), None, None)
    genome.check_sampling(ok.chrom_sizes, 20, 0)                          # exactly 2^32 + length: the last size numpy draws from 32 bits
    with pytest.raises(ValueError, match="max_n"):
        genome.PackedGenome(["chr1"], np.array([0, 100]), None, None).random_windows(10, 20, max_n=-1)
    with pytest.raises(ValueError, match="length"):
        genome.PackedGenome(["chr1"], np.array([0, 100]), None, None).random_windows(10, 0)


def test_golden_genome_has_what_the_gpu_tests_rely_on():
    d = np.load(os.path.join(ROOT, "tests", "golden", "ref_build.npz"))
    names = [str(n) for n in d["names"]]
    sizes = dict(zip(names, d["chrom_sizes"].tolist()))
    lengths = [int(d[f"samp{i}_args"][1]) for i in range(4)]
    assert sizes["chr3"] == max(lengths) + 1 == int(d["pfm_widths"].max()) + 1
    assert all(s > max(lengths) for n, s in sizes.items() if n != "chr3")
    assert {"chrX", "chrM", "chrUn_a", "chr7_random"} <= set(names)
    raw = d["chrom_bytes"].tobytes()
    assert b"N" in raw and b"n" in raw and any(c in raw for c in b"RYKMSWBDHV") and any(c in raw for c in b"acgt")
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "ref_build.npz")) < (1 << 20)
