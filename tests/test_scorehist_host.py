"""
The host side of the score histogram (ms_scan_score_histogram; motifscan_amd.scoredist), no GPU: the symbols, the "no device" answer, the
numpy restatement of the contract (`scoredist.restate_histogram`) against the pinned oracle -- per strand against its all-pass scan, per
position against its c_score of every window -- and the ScoreHistogram arithmetic (bin floors, tails, P-values, cutoffs, addition).
tests/test_gpu_scorehist.py compares the device against the same restatement and the same oracle-derived arrays.
"""
import ctypes
import os
import re

import numpy as np
import pytest

from fuzz_parity import ALL_PASS
from motifscan_amd import _lib, scoredist
from motifscan_amd.scoredist import ScoreHistogram

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def seeded_matrix(width, seed):
    """A log-odds-like matrix: Dirichlet columns against a flat background, five decimals as the reference keeps them."""
    rng = np.random.default_rng(seed)
    ppm = rng.dirichlet(np.full(4, 0.4), size=width).T
    return np.round(np.log2((ppm + 0.01) / 1.04 / 0.25), 5)


def random_dna(rng, n):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)].tobytes().decode()


def n_windows(mats, seqs):
    """int64 [P]: sum over the sequences of max(L - W + 1, 0)."""
    lens = np.array([len(s) for s in seqs], dtype=np.int64)
    return np.array([np.maximum(lens - m.shape[1] + 1, 0).sum() for m in mats], dtype=np.int64)


def oracle_per_strand(oracle, mats, seqs, strand, lo, hi, n_bins):
    """The histogram from the oracle's all-pass scan: its scores binned by bin_of; "below" = the analytic number of (window, strand)
    minus the rest -- where the -inf windows go, which the oracle reports none of.  An unscorable motif has no site and a zero row."""
    vals, widths = oracle.flatten_pwms(mats)
    bases, off = oracle.flatten_seqs(seqs)
    r = oracle.scan_arrays(vals, widths, np.full(len(mats), ALL_PASS), bases, off, strand)
    h = ScoreHistogram.from_range(np.zeros((len(mats), n_bins + 2), dtype=np.int64), lo, hi, n_bins)
    total = n_windows(mats, seqs) * (2 if strand == 3 else 1)
    for m, mat in enumerate(mats):
        a, b = int(r["motif_offsets"][m]), int(r["motif_offsets"][m + 1])
        if not scoredist.scorable(mat):
            assert a == b
            continue
        slots = h.bin_of(m, r["score"][a:b]) + 1
        h.counts[m] = np.bincount(slots, minlength=n_bins + 2)
        h.counts[m, 0] += total[m] - (b - a)
    return h.counts


def oracle_per_position(oracle, mats, seqs, strand, lo, hi, n_bins):
    """The histogram from the oracle's c_score (cscore.c:174-229) of every window, each handed in as its own sequence."""
    h = ScoreHistogram.from_range(np.zeros((len(mats), n_bins + 2), dtype=np.int64), lo, hi, n_bins)
    for m, mat in enumerate(mats):
        W = mat.shape[1]
        windows = [s[p:p + W] for s in seqs for p in range(len(s) - W + 1)]
        if not windows or not scoredist.scorable(mat):
            continue
        vals, widths = oracle.flatten_pwms([mat])
        bases, off = oracle.flatten_seqs(windows)
        score = oracle.score_arrays(vals, widths, bases, off, strand)[0]
        h.counts[m] = np.bincount(h.bin_of(m, score) + 1, minlength=n_bins + 2)
    return h.counts


def host_case():
    rng = np.random.default_rng(20260101)
    mats = [seeded_matrix(w, 300 + w) for w in (1, 4, 9, 33)]
    holes = seeded_matrix(4, 104)
    holes[0, 2] = -np.inf
    holes[3, 0] = -np.inf
    mats.append(holes)
    mats.append(-np.abs(seeded_matrix(7, 107)))                  # max_raw = 0: unscorable
    seqs = [random_dna(rng, n) for n in (1, 3, 4, 5, 9, 32, 33, 34, 200)]
    marked = bytearray(random_dna(rng, 120).encode())
    marked[20:31] = b"N" * 11
    marked[50:70] = bytes(marked[50:70]).lower()
    marked[90] = ord("R")
    seqs += [marked.decode(), "N" * 40, "ACGT" * 3 + "AAAAC", "AAAA"]
    return mats, seqs


BINNINGS = ((0.0, None, 64), (-2.0, 1.5, 7), (0.6, 1.0, 16), (0.25, 0.75, 1))


# ------------------------------------------------------------------------------------------------ the symbols, no device

def test_header_declares_the_entry_point_and_the_library_has_it():
    with open(os.path.join(ROOT, "include", "motifscan_amd.h")) as fh:
        text = fh.read()
    table = text[:text.index("#ifndef MOTIFSCAN_AMD_H")]
    assert re.search(r"\bint\s+ms_scan_score_histogram\s*\(", text)
    assert re.search(r"ms_scan_score_histogram\s+c_score at EVERY window", table)
    assert "cscore.c:174-229" in table and "motif/__init__.py:378-401" in table
    assert re.search(r"#define\s+MS_SCOREHIST_MAX_BINS\s+4096\b", text) and re.search(r"#define\s+MS_HIST_PER_POSITION\s+1u\b", text)
    assert "NOT the reference's filter" in text
    assert hasattr(_lib.lib(), "ms_scan_score_histogram") and hasattr(_lib.lib(), "ms_debug_scorehist_dims")
    with open(os.path.join(ROOT, "include", "motifscan_amd_debug.h")) as fh:
        assert re.search(r"\bint\s+ms_debug_scorehist_dims\s*\(\s*int32_t\s+out\[4\]\s*\)", fh.read())
    assert (_lib.MS_SCOREHIST_MAX_BINS, _lib.MS_HIST_PER_POSITION) == (4096, 1)


def test_dims_are_constants_of_the_build():
    d = _lib.scorehist_dims()
    assert d["segment_windows"] >= 64 and d["segment_windows"] % 64 == 0
    assert d["tile_max_width"] >= 64
    assert d["lds_slots"] == _lib.MS_SCOREHIST_MAX_BINS + 2
    assert d["flush_windows"] % d["segment_windows"] == 0 and d["segment_windows"] < d["flush_windows"]
    assert 2 * d["flush_windows"] < 2 ** 32                      # a 32-bit LDS counter holds both strands of one flush interval
    # two blocks per CU: the widest tile (+ its zero entry), the counters and some slack within half of the 160 KB
    assert 16 * (4 * d["tile_max_width"] + 1) + 4 * d["lds_slots"] <= 80 * 1024
    assert _lib.lib().ms_debug_scorehist_dims(None) == _lib.MS_ERR_INVALID


def test_no_gpu_means_loud_failure_before_any_validation():
    L = _lib.lib()
    args = (None, None, 0, 99, None, None, 0, 0, None, None)     # every one of them invalid
    have_device = _lib.device_count() > 0
    rc = L.ms_scan_score_histogram(*args)
    if have_device:
        assert rc == _lib.MS_ERR_INVALID
        return
    assert rc == _lib.MS_ERR_RUNTIME
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _lib.check(rc)


# ------------------------------------------------------------------------------------------------ the restatement against the oracle

@pytest.mark.parametrize("strand", (1, 2, 3))
def test_restatement_per_strand_against_the_oracle_scan(oracle, strand):
    mats, seqs = host_case()
    for lo, hi, n_bins in BINNINGS:
        hi = scoredist.default_hi(lo, n_bins) if hi is None else hi
        want = oracle_per_strand(oracle, mats, seqs, strand, lo, hi, n_bins)
        got = scoredist.restate_histogram(mats, seqs, strand, lo, hi, n_bins)
        assert got.dtype == np.int64 and np.array_equal(got, want), (lo, hi, n_bins)
        assert np.array_equal(got.sum(axis=1)[:5], n_windows(mats, seqs)[:5] * (2 if strand == 3 else 1))
        assert not got[5].any()                                  # the unscorable motif
    full = scoredist.restate_histogram(mats, seqs, strand, -2.0, 1.5, 7)
    assert full[4, 0] > 0                                        # the -inf windows of the motif with holes are "below"


@pytest.mark.parametrize("strand", (1, 2, 3))
def test_restatement_per_position_against_the_oracle_c_score(oracle, strand):
    mats, seqs = host_case()
    for lo, hi, n_bins in BINNINGS:
        hi = scoredist.default_hi(lo, n_bins) if hi is None else hi
        want = oracle_per_position(oracle, mats, seqs, strand, lo, hi, n_bins)
        got = scoredist.restate_histogram(mats, seqs, strand, lo, hi, n_bins, per_position=True)
        assert np.array_equal(got, want), (lo, hi, n_bins)
        assert np.array_equal(got.sum(axis=1)[:5], n_windows(mats, seqs)[:5]) and not got[5].any()


def test_restatement_max_n_counts_the_windows_own_non_acgt_bases():
    mat = seeded_matrix(4, 1)
    seq = "ACGTNACGTRRACGTnnnACGT"
    per = {k: scoredist.restate_histogram([mat], [seq], 1, -3.0, 1.5, 5, max_n=k).sum() for k in (-1, 0, 1, 2, 3, 4)}
    n_non = np.array([sum(ch not in "ACGTacgt" for ch in seq[p:p + 4]) for p in range(len(seq) - 3)])
    assert per[-1] == len(n_non) == per[4]
    for k in (0, 1, 2, 3):
        assert per[k] == int((n_non <= k).sum())
    assert per[0] < per[1] < per[2] < per[3]


# ------------------------------------------------------------------------------------------------ ScoreHistogram

def test_bin_of_is_the_rule_and_bin_floor_its_exact_boundary():
    h = ScoreHistogram.from_range(np.zeros((3, 66), dtype=np.int64), [0.0, 0.5, -1.25], [scoredist.default_hi(0.0, 64), 1.0, 3.0], 64)
    assert h.bin_of(0, [-np.inf, -1e-300, -0.0, 0.0, 1.0, 1.5, 2.0, np.inf]).tolist() == [-1, -1, 0, 0, 63, 64, 64, 64]
    assert h.bin_of(1, [0.5, np.nextafter(0.5, 0), 1.0, np.nextafter(1.0, 0)]).tolist() == [0, -1, 64, 63]
    for m in range(3):
        for i in (-1, 0, 1, 17, 63, 64):
            c = h.bin_floor(m, i)
            if i == -1:
                assert c == -np.inf
                continue
            assert h.bin_of(m, np.nextafter(c, -np.inf)) < i <= h.bin_of(m, c), (m, i)
        many = h.bin_floor(m, np.arange(0, 65))
        assert np.all(np.diff(many) > 0) and np.all(h.bin_of(m, many) == np.arange(0, 65))
        assert np.all(h.bin_of(m, np.nextafter(many, -np.inf)) == np.arange(-1, 64))
    assert h.bin_floor(0, 0) == 0.0 or h.bin_floor(0, 0) == -0.0
    assert h.bin_floor(1, 0) == 0.5 and h.bin_floor(1, 64) == 1.0
    with pytest.raises(ValueError):
        h.bin_floor(0, 65)


def test_default_hi_puts_one_in_the_last_bin():
    for lo, n_bins in ((0.0, 1), (0.0, 1024), (0.0, 4096), (0.7, 1024), (-3.0, 7), (0.999, 4096)):
        hi = scoredist.default_hi(lo, n_bins)
        h = ScoreHistogram.from_range(np.zeros((1, n_bins + 2), dtype=np.int64), lo, hi, n_bins)
        assert hi > 1.0 and h.bin_of(0, 1.0) == n_bins - 1 and hi - 1.0 < 1e-9


def test_tail_p_value_and_cutoffs_on_hand_made_counts():
    #            below  [0,.25) [.25,.5) [.5,.75) [.75,1)  above
    counts = [[90, 5, 3, 1, 1, 0],
              [0, 0, 0, 0, 0, 0],
              [10, 0, 0, 0, 0, 90]]
    h = ScoreHistogram.from_range(np.array(counts), 0.0, 1.0, 4)
    assert h.n_windows.tolist() == [100, 0, 100]
    assert h.tail(0).tolist() == [100, 10, 5, 2, 1, 0]
    assert h.p_value(0, [-5.0, 0.0, 0.3, 0.5, 0.74, 0.75, 0.99, 1.0]).tolist() == [1.0, 0.1, 0.05, 0.02, 0.02, 0.01, 0.01, 0.0]
    assert np.all(np.isnan(h.p_value(1, [0.5])))
    cut = h.cutoffs(["1e-1", "5e-2", "1e-2", "0.011", "1e-3", "1", 0.02])
    assert cut[0] == {"1e-1": 0.0, "5e-2": 0.25, "1e-2": 0.75, "0.011": 0.75, "1e-3": 1.0, "1": -np.inf, 0.02: 0.5}
    assert all(v is None for v in cut[1].values())               # nothing counted
    assert cut[2]["1e-1"] is None and cut[2]["1"] == -np.inf and cut[2]["1e-3"] is None      # 90 % of the windows sit in "above"
    assert h.cutoffs(["0.9"])[2]["0.9"] == 0.0                   # ... at p = 0.9 every slot above "below" has tail 90: the lowest bin's floor
    assert h.cutoff_slots(["1e-1", "1e-3"]).tolist() == [[1, 5], [-1, -1], [-1, -1]]
    # the defining property: tail at the cutoff's slot <= p n, and one slot lower > p n
    for p, c in cut[0].items():
        if c == -np.inf:
            continue
        s = int(h.bin_of(0, c)) + 1
        f = float(p)
        assert h.tail(0)[s] <= f * 100 + 1e-9 and h.tail(0)[s - 1] > f * 100 - 1e-9


def test_addition_adds_counts_and_refuses_mismatched_binning():
    a = ScoreHistogram.from_range(np.arange(12).reshape(2, 6), 0.0, 1.0, 4)
    b = ScoreHistogram.from_range(np.ones((2, 6), dtype=np.int64), 0.0, 1.0, 4)
    s = a + b
    assert np.array_equal(s.counts, np.arange(12).reshape(2, 6) + 1) and s.same_binning(a) and s.n_bins == 4
    assert np.array_equal(a.counts, np.arange(12).reshape(2, 6))                       # the operands are untouched
    for other in (ScoreHistogram.from_range(np.ones((2, 6), dtype=np.int64), 0.0, 1.5, 4),
                  ScoreHistogram.from_range(np.ones((2, 6), dtype=np.int64), [0.0, 0.1], 1.0, 4),
                  ScoreHistogram.from_range(np.ones((2, 7), dtype=np.int64), 0.0, 1.0, 5),
                  ScoreHistogram.from_range(np.ones((3, 6), dtype=np.int64), 0.0, 1.0, 4)):
        with pytest.raises(ValueError, match="binning"):
            a + other
    with pytest.raises(ValueError):
        ScoreHistogram(np.ones((2, 5)), 0.0, 4.0, 4)
    with pytest.raises(TypeError):
        a + 1


def test_binding_refuses_a_wrong_out_array_without_a_library_call():
    class Handle:
        h, n = None, 2
    for bad in (np.zeros((2, 5), dtype=np.int64), np.zeros((2, 6), dtype=np.int32), np.zeros((6, 2), dtype=np.int64).T):
        with pytest.raises(ValueError, match="out must be"):
            _lib.score_histogram(Handle, Handle, 3, 0.0, 1.0, 4, out=bad)
    lo, inv = _lib.histogram_binning(3, 0.5, [1.0, 1.5, 2.5], 4)
    assert lo.tolist() == [0.5, 0.5, 0.5] and inv.tolist() == [8.0, 4.0, 2.0]
