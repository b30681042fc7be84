"""
The host side of the expected-counts step (ms_affinity_expected_counts; motifscan_amd.em, _lib.Affinity.expected_counts,
Scanner.expected_counts / refine_motifs): the numpy restatement against the mpmath reference, the closed forms, the invariants the header
promises, what must fail loudly without a GPU, and the refinement loop on a planted motif.  No GPU.

The cases of tests/test_gpu_expected_counts.py are made here (make_cases), so that the cap on `slack` is asserted on the CPU: the GPU
tests compare by |device - host| <= slack, and a test may not hide behind a slack that is non-zero everywhere.
"""
import math
import os
import re

import numpy as np
import pytest

from motifscan_amd import _lib, affinity, em, scanner

LN2 = math.log(2.0)
INF = math.inf
TWO32 = 1 << 32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def random_seq(rng, length, p_n=0.0):
    p = np.array([.3, .2, .2, .3]) * (1.0 - p_n)
    return "".join(rng.choice(list("ACGTN"), p=list(p) + [p_n], size=length)) if length else ""


def random_mat(rng, width, spread=2.0):
    """A matrix whose raw sums have about `spread` as standard deviation at any width: 2 keeps every window's weight above a unit of
    2^-32, 12 (a sharp matrix) leaves a few windows per hundred with a weight -- and so few terms per cell of `counts` that one of
    them hitting the slack band is rare (test_slack_is_rare_over_the_cases_of_the_gpu_file)."""
    return np.round(rng.normal(0.0, 1.0, size=(4, width)) * (spread / math.sqrt(width)), 3)


def plant(seq, mat, at, minus=False):
    """seq with the best-scoring word of mat written at window start `at` (on '-': its reverse complement)."""
    word = "".join("ACGT"[b] for b in np.argmax(mat, axis=0))
    if minus:
        word = "".join({"A": "T", "C": "G", "G": "C", "T": "A"}[b] for b in reversed(word))
    assert 0 <= at and at + len(word) <= len(seq)
    return seq[:at] + word + seq[at + len(word):]


SHARP = 12.0


def make_cases(dims):
    """name -> (mats, seqs, strand, scale, max_n, prior_logit), sized by ms_debug_expected_dims."""
    seg, max_w, tile_cols, waves = dims["segment_windows"], dims["max_width"], dims["tile_entries"] // 4, dims["waves"]
    lanes = seg // dims["strips"]
    rng = np.random.default_rng(20250311)
    cases = {}

    # every width around a code word (32 columns), two, and the widest, each on regions of W - 1, W, W + 1 and W + 2 bases, N at 2 % in
    # every third region; the strand masks, scales, max_n and priors take turns
    widths = (1, 31, 32, 33, 64, 65, max_w)
    combos = [(3, 1.0, -1, 0.0), (1, LN2, 0, INF), (2, 1.0, 2, 20.0), (3, LN2, -1, -20.0), (3, 1.0, 0, INF), (1, 1.0, -1, 0.0), (2, LN2, 2, INF)]
    k = 0
    for w, combo in zip(widths, combos):
        seqs = []
        for d in (-1, 0, 1, 2):
            if w + d > 0:
                seqs.append(random_seq(rng, w + d, 0.02 if k % 3 == 0 else 0.0))
                k += 1
        if w == 31:
            seqs[1] = seqs[1].lower()
        cases[f"w{w}"] = ([random_mat(rng, w)], seqs, *combo)
    cases["never"] = (cases["w33"][0], cases["w33"][1], 3, 1.0, -1, -INF)

    # regions around one segment (the last window of the first segment; one segment against two), of three segments, and last strips of
    # 1, 63 and 64 lanes -- under sharp matrices of 1 and 33 columns, the wider one's best word planted at the windows that matter
    m1, m33 = random_mat(rng, 1, SHARP), random_mat(rng, 33, SHARP)
    lengths = [seg + w + d for w in (1, 33) for d in (-2, -1, 0)] + [2 * seg + 40]
    lengths += [3 * lanes + 1, 4 * lanes - 1, 4 * lanes]                     # (W = 1) the last strip holds 1, 63 and 64 lanes with a window
    lengths += [4 * lanes + 33, 5 * lanes + 31]                              # (W = 33) 1 and 63 lanes in the fifth strip
    seqs = [random_seq(rng, n, 0.02 if i % 3 == 0 else 0.0) for i, n in enumerate(lengths)]
    seqs[1] = seqs[1].lower()
    for i, n in enumerate(lengths):
        seqs[i] = plant(seqs[i], m33, n - 33, minus=bool(i % 2))                # the region's last window
        if n >= seg + 32:
            seqs[i] = plant(seqs[i], m33, seg - 1)                           # the last window of the first segment
        if n >= 2 * seg + 33:
            seqs[i] = plant(seqs[i], m33, 2 * seg, minus=True)               # the first window of the third
    cases["segments"] = ([m1, m33], seqs, 3, 1.0, -1, 0.0)
    cases["segments_plus"] = ([m1, m33], seqs[3:9], 1, LN2, 2, INF)
    cases["segments_minus"] = ([m1, m33], seqs[3:9], 2, 1.0, -1, 20.0)

    # max_n on windows with runs of N, on a narrow motif and on one wider than a code word; an all-N region
    m5, m48 = random_mat(rng, 5, SHARP), random_mat(rng, 48, SHARP)
    base = random_seq(rng, 130)
    one_n = base[:70] + "N" + base[71:]
    runs = base[:20] + "N" * 3 + base[23:60] + "NN" + base[62:100] + "N" * 7 + base[107:]
    nseqs = [one_n, runs, "N" * 60, base, random_seq(rng, seg + 70, 0.05)]
    cases["max_n_0"] = ([m5, m48], nseqs, 3, 1.0, 0, 0.0)
    cases["max_n_2"] = ([m5, m48], nseqs, 3, LN2, 2, INF)
    cases["max_n_all"] = ([m5, m48], nseqs, 3, 1.0, -1, INF)

    # a set whose tables overflow one tile; a narrow motif behind the wide ones (the narrow ones see hundreds of windows: sharp)
    wide_w = [max_w, tile_cols - max_w - 10, 40, 3, max_w - 1, 7]            # the third motif does not fit the first tile
    assert wide_w[0] + wide_w[1] <= tile_cols < wide_w[0] + wide_w[1] + wide_w[2]
    cases["tiles"] = ([random_mat(rng, w, 2.0 if w > 200 else SHARP) for w in wide_w],
                      [random_seq(rng, max_w + 6, 0.01), random_seq(rng, max_w, 0.0), random_seq(rng, max_w + 40, 0.0)], 3, 1.0, -1, 0.0)

    # -inf entries: some terms, every term (also over two segments); a NaN row and a +inf row; the all-negative matrix
    some = random_mat(rng, 6, SHARP)
    some[0, 2] = -np.inf
    every = random_mat(rng, 4, SHARP)
    every[:, 1] = -np.inf
    half = random_mat(rng, 3, SHARP)
    half[0, 0] = -np.inf
    nan_row, inf_row = random_mat(rng, 7), random_mat(rng, 2)
    nan_row[3, 6] = np.nan
    inf_row[1, 0] = np.inf
    neg = -np.abs(random_mat(rng, 9, SHARP)) - 0.01
    iseqs = [random_seq(rng, 90), random_seq(rng, seg + 50), "A" * (seg + 30), "A" * 20 + random_seq(rng, 70), random_seq(rng, 3), ""]
    cases["minus_inf"] = ([some, every, nan_row, half, inf_row, neg], iseqs, 3, 1.0, -1, 0.0)
    cases["minus_inf_oops"] = ([some, every, nan_row, half, inf_row, neg], iseqs, 1, 1.0, -1, INF)

    # more segments than two blocks hold: the grid-stride loop takes several trips under a cap of 1 or 2
    many = [random_seq(rng, 30 + 3 * i, 0.02 if i % 4 == 0 else 0.0) for i in range(2 * waves + 5)] + [random_seq(rng, 2 * seg + 17)]
    cases["loop"] = ([random_mat(rng, 5, SHARP), random_mat(rng, 12, SHARP), random_mat(rng, 33, SHARP)], many, 3, 1.0, -1, 0.0)
    return cases


def planted_case():
    """(seed matrix, sequences, planted ppm, background): 60 regions x 60 bp of composition (.3, .2, .2, .3); an 8-column motif with
    0.85 on its consensus planted in three regions of four, on alternating strands; the seed is the consensus at 0.5."""
    rng = np.random.default_rng(7)
    bg = np.array([.3, .2, .2, .3])
    cons = [0, 2, 3, 1, 1, 0, 3, 2]                                            # AGTCCATG
    planted = np.full((4, 8), 0.05)
    planted[cons, np.arange(8)] = 0.85
    comp = {"A": "T", "C": "G", "G": "C", "T": "A"}
    seqs, k = [], 0
    for r in range(60):
        s = list(rng.choice(list("ACGT"), p=bg, size=60))
        if r % 4 != 3:
            site = ["ACGT"[rng.choice(4, p=planted[:, c])] for c in range(8)]
            if k % 2:
                site = [comp[b] for b in reversed(site)]
            k += 1
            at = int(rng.integers(0, 53))
            s[at:at + 8] = site
        seqs.append("".join(s))
    seed_ppm = np.full((4, 8), 0.5 / 3)
    seed_ppm[cons, np.arange(8)] = 0.5
    return np.log(seed_ppm / bg[:, None]), seqs, planted, bg


def ppm_of(mat, bg):
    return np.exp(mat) * np.asarray(bg)[:, None]


def assert_invariants(exp):
    """Every used column sums to total; the columns behind W are zero."""
    for i, W in enumerate(exp.widths.tolist()):
        assert np.all(exp.counts[i, :W].sum(axis=1) == exp.total[i]), i
        assert not exp.counts[i, W:].any(), i
    assert exp.counts.dtype == exp.total.dtype == exp.n_regions.dtype == np.int64


def assert_within_slack(got, want, slack):
    """|got - want| <= slack cell by cell; total by the slack of a column; n_regions exactly."""
    diff = np.abs(got.counts - want.counts)
    assert np.all(diff <= slack), (int(diff.max()), np.argwhere(diff > slack)[:4].tolist())
    assert np.all(np.abs(got.total - want.total) <= slack[:, 0, :].sum(axis=1))
    assert np.array_equal(got.n_regions, want.n_regions)


CASES = make_cases(_lib.expected_dims())
_HOST = {}


def host(name):
    if name not in _HOST:
        _HOST[name] = em.expected_counts_host(*CASES[name])
    return _HOST[name]


SMALL = ("w1", "w33", "w65", "segments_plus", "segments_minus", "max_n_0", "max_n_2", "minus_inf", "minus_inf_oops")


@pytest.mark.parametrize("name", SMALL)
def test_restatement_matches_the_reference(name):
    mats, seqs, strand, scale, max_n, prior = CASES[name]
    got, slack = em.expected_counts_host(mats, seqs, strand, scale, max_n, prior)
    ref, real, n_contrib = em.expected_counts_reference(mats, seqs, strand, scale, max_n, prior)
    assert_invariants(got)
    assert_invariants(ref)
    assert np.array_equal(got.counts[slack == 0], ref.counts[slack == 0])
    assert_within_slack(got, ref, slack)
    worst = 0.0
    for idx in np.argwhere(n_contrib > 0):
        i = tuple(idx)
        err = abs(int(ref.counts[i]) - real[i])
        assert err <= n_contrib[i] * 0.5
        worst = max(worst, float(err / (n_contrib[i] * 0.5)))
    assert not got.counts[n_contrib == 0].any()
    print(f"{name}: {int((n_contrib > 0).sum())} cells, {int((slack > 0).sum())} with slack, largest |q - real| / bound = {worst:.3f}")


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_used_column_sums_to_total(name):
    exp, slack = host(name)
    assert_invariants(exp)
    assert slack.shape == exp.counts.shape and slack.min() >= 0


def test_slack_is_rare_over_the_cases_of_the_gpu_file():
    cells = flagged = 0
    for name in sorted(CASES):
        exp, slack = host(name)
        nz = exp.counts != 0
        cells += int(nz.sum())
        flagged += int((nz & (slack > 0)).sum())
        share = (nz & (slack > 0)).sum() / max(int(nz.sum()), 1)
        print(f"{name}: {int(nz.sum())} non-zero cells, {int((nz & (slack > 0)).sum())} with slack")
        assert share <= 0.01, name
    assert cells > 3000 and flagged <= 0.01 * cells


CONS = "AACGT"                                                                   # its reverse complement is ACGTT: no palindrome


def consensus_matrix():
    m = np.full((4, len(CONS)), -np.inf)
    for c, b in enumerate(CONS):
        m["ACGT".index(b), c] = 0.0
    return m


CLOSED_SEQS = ["GGAACGTGGG", "GGGAACGTGGGACGTTGG", "CCAACGTCCACGTTCCCAACGTCC"]     # k = 1 ('+'), 2 ('+', '-'), 3 ('+', '-', '+') occurrences


def closed_expected():
    counts = np.zeros((1, len(CONS), 5), dtype=np.int64)
    per_region = [k * int(np.rint(TWO32 / k)) for k in (1, 2, 3)]
    for c, b in enumerate(CONS):
        counts[0, c, "ACGT".index(b)] = sum(per_region)
    return counts, sum(per_region)


def test_closed_forms_consensus_only_and_all_n():
    exp, slack = em.expected_counts_host([consensus_matrix()], CLOSED_SEQS, 3, 1.0, -1, INF)
    counts, total = closed_expected()
    assert total == TWO32 + TWO32 + 3 * 1431655765
    assert np.array_equal(exp.counts, counts) and exp.total[0] == total and exp.n_regions[0] == 3
    assert not slack.any()
    assert exp.pfm(0).shape == (4, 5) and exp.pfm(0)[0, 0] == total * 2.0 ** -32
    assert exp.occupancy(0) == total * 2.0 ** -32 / 3
    mat = np.round(np.random.default_rng(3).normal(size=(4, 5)), 2)
    alln, _ = em.expected_counts_host([mat], ["NNNNNN"], 3, 1.0, -1, INF)      # 2 windows x 2 strands, raw = 0 each: w = 1/4
    assert np.array_equal(alln.counts[0, :, 4], np.full(5, TWO32)) and not alln.counts[0, :, :4].any() and alln.total[0] == TWO32
    assert np.array_equal(alln.n_weight(0), np.ones(5)) and not alln.pfm(0).any()
    none, _ = em.expected_counts_host([mat], ["NNNNNN"], 3, 1.0, 0, INF)       # max_n drops every window
    assert not none.counts.any() and none.total[0] == 0 and none.n_regions[0] == 0 and math.isnan(none.occupancy(0))


def test_shards_add_up_exactly():
    for name in ("segments", "minus_inf"):
        mats, seqs, strand, scale, max_n, prior = CASES[name]
        whole, _ = host(name)
        cut = len(seqs) // 3
        a, _ = em.expected_counts_host(mats, seqs[:cut], strand, scale, max_n, prior)
        b, _ = em.expected_counts_host(mats, seqs[cut:], strand, scale, max_n, prior)
        assert np.array_equal(a.counts + b.counts, whole.counts)
        assert np.array_equal(a.total + b.total, whole.total) and np.array_equal(a.n_regions + b.n_regions, whole.n_regions)


def test_responsibility_is_one_zero_and_a_half():
    zeros = np.zeros((4, 3))
    seqs = ["ACGTACGTAC"]                                                      # 8 windows x 2 strands = 16 terms of raw 0: log_mean = 0
    for prior, want in ((INF, TWO32), (-INF, 0), (0.0, TWO32 // 2)):
        exp, _ = em.expected_counts_host([zeros], seqs, 3, 1.0, -1, prior)
        assert exp.total[0] == want and exp.n_regions[0] == 1
    assert em.responsibility(np.array([[0.0, -np.inf, np.nan, 3.0]]), np.array([[4, 4, 0, 4]]), 0.0).tolist() == [[0.5, 0.0, 0.0, 1.0 / (1.0 + math.exp(-3.0))]]
    assert em.responsibility(np.array([[0.0, -np.inf]]), np.array([[4, 4]]), INF).tolist() == [[1.0, 1.0]]
    assert em.prior_logit_of(None) == INF and em.prior_logit_of(0.5) == 0.0 and em.prior_logit_of(0.0) == -INF and em.prior_logit_of(1.0) == INF
    with pytest.raises(ValueError, match="NaN"):
        em.expected_counts_host([zeros], seqs, 3, 1.0, -1, math.nan)
    with pytest.raises(ValueError, match="gamma"):
        em.prior_logit_of(1.5)
    with pytest.raises(ValueError, match="strand"):
        em.expected_counts_host([zeros], seqs, 0)
    with pytest.raises(ValueError, match="prec"):
        em.expected_counts_reference([zeros], seqs, 3, prec=64)


def test_log_likelihood_and_m_step():
    mats, seqs = [np.log(np.array([[.7, .1], [.1, .1], [.1, .1], [.1, .7]]) / 0.25)], ["ACGTAT", "AT", "C"]
    a = affinity.affinity_host(mats, seqs, 3)
    g = 0.3
    ll = em.log_likelihood(a, em.prior_logit_of(g))
    want = sum(math.log(1 - g + g * math.exp(x)) for x, n in zip(a.log_mean[0].tolist(), a.n_terms[0].tolist()) if n > 0)
    assert ll.shape == (1,) and ll[0] == pytest.approx(want, rel=1e-13)
    assert em.log_likelihood(a, INF)[0] == pytest.approx(a.log_mean[0, :2].sum(), rel=1e-13)
    exp, _ = em.expected_counts_host(mats, seqs, 3, 1.0, -1, 0.0)
    bg = {"A": .3, "C": .2, "G": .2, "T": .3}
    (new,) = em.m_step(exp, bg, 0.01)
    ppm = ppm_of(new, [.3, .2, .2, .3])
    assert new.shape == (4, 2) and np.allclose(ppm.sum(axis=0), 1.0, atol=1e-12)
    raw = exp.pfm(0) / exp.pfm(0).sum(axis=0)
    assert np.allclose(ppm, (raw + 0.01 * np.array([.3, .2, .2, .3])[:, None]) / 1.01, atol=1e-12)
    empty = em.ExpectedCounts(np.zeros((1, 2, 5), dtype=np.int64), np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.int64), [2])
    assert not em.m_step(empty)[0].any()                                       # no weight at all: the background
    with pytest.raises(ValueError, match="pseudo"):
        em.m_step(exp, None, 0.0)


def test_header_symbols_and_loud_failure_without_a_gpu():
    with open(os.path.join(ROOT, "include", "motifscan_amd.h")) as f:
        header = f.read()
    head = header[:header.index("#ifndef MOTIFSCAN_AMD_H")]
    assert re.search(r"ms_affinity_expected_counts\s*\n \*\s+no reference counterpart", head)
    assert re.search(r"#define MS_EXPECTED_MAX_WIDTH 256\b", header)
    L = _lib.lib()
    for sym in ("ms_affinity_expected_counts", "ms_debug_expected_dims", "ms_debug_expected_grid_cap"):
        assert hasattr(L, sym)
    dims = _lib.expected_dims()
    assert dims["max_width"] == 256 and dims["segment_windows"] == 64 * dims["strips"] and dims["tile_entries"] >= 4 * dims["max_width"]
    assert dims["acc_bytes_per_column"] == 40 and dims["grid_cap"] >= 1 and dims["waves"] >= 1
    assert 2 * (16 * (dims["tile_entries"] + 1) + dims["acc_bytes_per_column"] * dims["tile_entries"] // 4) <= 160 * 1024
    assert L.ms_debug_expected_dims(None) == _lib.MS_ERR_INVALID
    assert L.ms_debug_expected_grid_cap(-1) == _lib.MS_ERR_INVALID
    with _lib.expected_grid_cap(2):
        pass
    if _lib.device_count() == 0:
        rc = L.ms_affinity_expected_counts(None, None, None, 0.0, 0, 0, 0, None, None, None, None)      # said before the handles are looked at
        assert rc == _lib.MS_ERR_RUNTIME
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            _lib.check(rc)
        sc = _scanner()
        with pytest.raises(RuntimeError):
            sc.expected_counts([_Pwm()])
        with pytest.raises(RuntimeError):
            sc.refine_motifs([_Pwm()], iters=1)
    sc = _scanner()
    for kw in ({"scale": 0.0}, {"max_n": -2}, {"gamma": 1.5}):
        with pytest.raises(ValueError):
            sc.expected_counts([_Pwm()], **kw)
    with pytest.raises(ValueError):
        sc.refine_motifs([_Pwm()], gamma=0.0)


class _Pwm:
    matrix, length, cutoffs = np.ones((4, 3)), 3, None


def _scanner():
    class Region:
        chrom, start, end, summit = "chr1", 2, 12, 7

    class Genome:
        chrom_sizes = {"chr1": 20}

        def fetch_sequence(self, chrom, start, end):
            return "ACGTACGTACGTACGTACGT"[start:end]
    return scanner.Scanner(Genome(), [Region()])


def check_refinement(res, planted, bg):
    """The consensus is the planted one, and the error after the last iteration is below the error after the first."""
    errs = [float(np.abs(ppm_of(step["mats"][0], bg) - planted).max()) for step in res.steps[1:]]
    errs.append(float(np.abs(ppm_of(res.mats[0], bg) - planted).max()))
    print("max |ppm - planted| after each iteration:", [round(e, 4) for e in errs], "gamma:", res.gammas[:, 0].round(4).tolist())
    assert np.array_equal(ppm_of(res.mats[0], bg).argmax(axis=0), planted.argmax(axis=0))
    assert errs[-1] < errs[0]
    return errs


def test_refine_recovers_a_planted_motif_on_the_host():
    seed, seqs, planted, bg = planted_case()
    res = em.refine([seed], seqs, iters=4, gamma=0.5, strand=3, bg=bg, pseudo=0.01, device=False, keep=True)
    assert len(res.steps) == 4 and res.gammas.shape == (5, 1) and res.log_likelihood.shape == (4, 1)
    check_refinement(res, planted, bg)
    assert np.all(np.diff(res.log_likelihood[:, 0]) > 0)                       # the seed is far from the optimum: every iteration gains
    assert 0.5 < res.gammas[-1, 0] < 0.95                                      # three regions of four hold a site
