"""
The host side of the site stacks (ms_result_site_base_counts; motifscan_amd.sitestack): the sequential restatement
sitestack.site_base_counts_host pinned by hand-written cases whose expected arrays are typed out below, the column-sum invariant on
seeded random cases, SiteStack.pfm through matrix.PositionFrequencyMatrix, the restatement against a direct numpy count over the
oracle's sites, the exported symbols and what must fail loudly without a GPU.  No GPU.  tests/test_gpu_sitestack.py runs the device
against the same cases and the same restatement.
"""
import ctypes
import os
import re

import numpy as np
import pytest

from motifscan_amd import _lib, matrix, sitestack

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def hit_arrays(per_motif):
    """per motif a list of (region, pos, strand) -> (motif_offsets, seq_idx, pos, strand) in ms_result order."""
    rows = [np.asarray(sorted(p), dtype=np.int64).reshape(-1, 3) for p in per_motif]
    offsets = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    flat = np.concatenate(rows) if rows else np.zeros((0, 3), dtype=np.int64)
    return offsets, flat[:, 0].copy(), flat[:, 1].copy(), flat[:, 2].astype(np.int8)


def dense(shape, entries):
    """int64 zeros(shape) with entries {(row, column, cell): count} set."""
    out = np.zeros(shape, dtype=np.int64)
    for idx, v in entries.items():
        out[idx] = v
    return out


# Every case: the regions, the motif widths, per motif the sites (region, pos, strand: 1 '+', 2 '-'), the flank, and the expected
# counts [P][C][6] and dinuc [P][C][16] (as {(row, column, 4 * a + b): count}), worked out by hand from the definition: slots A0 C1 G2 T3
# after orientation, 4 non-ACGT, 5 outside the region.
#
# "ACGTNacgtR", W = 3, sites at pos 0 and L - W = 7 on both strands.  The columns' slots per site, flank 0:
#   (0, +) A C G -> 0 1 2      (0, -) reads G C A complemented -> 1 2 3      (7, +) g t R -> 2 3 4      (7, -) reads R t g -> 4 0 1
# flank 2 (columns 0 .. 6; the region is bases 0 .. 9):
#   (0, +) . . A C G T N -> 5 5 0 1 2 3 4         (0, -) reads N T G C A . . -> 4 0 1 2 3 5 5
#   (7, +) a c g t R . . -> 0 1 2 3 4 5 5         (7, -) reads . . R t g c a -> 5 5 4 0 1 2 3
_ONE = dict(seqs=["ACGTNacgtR"], widths=[3], sites=[[(0, 0, 1), (0, 0, 2), (0, 7, 1), (0, 7, 2)]])
HAND = [
    dict(_ONE, name="one region, flank 0", flank=0,
         counts=[[[1, 1, 1, 0, 1, 0], [1, 1, 1, 1, 0, 0], [0, 1, 1, 1, 1, 0]]],
         dinuc={(0, 0, 1): 1, (0, 0, 6): 1, (0, 0, 11): 1, (0, 1, 6): 1, (0, 1, 11): 1, (0, 1, 1): 1}),
    dict(_ONE, name="one region, flank 2", flank=2,
         counts=[[[1, 0, 0, 0, 1, 2], [1, 1, 0, 0, 0, 2], [1, 1, 1, 0, 1, 0], [1, 1, 1, 1, 0, 0], [0, 1, 1, 1, 1, 0], [0, 0, 1, 1, 0, 2],
                  [0, 0, 0, 1, 1, 2]]],
         dinuc={(0, 0, 1): 1, (0, 1, 1): 1, (0, 1, 6): 1, (0, 2, 1): 1, (0, 2, 6): 1, (0, 2, 11): 1, (0, 3, 1): 1, (0, 3, 6): 1, (0, 3, 11): 1,
                (0, 4, 6): 1, (0, 4, 11): 1, (0, 5, 11): 1}),
    # W = 1 on "ACGN": every position on '+', position 0 on '-' (A -> T).  No pair of columns inside a site at flank 0.
    dict(name="W = 1, flank 0", seqs=["ACGN"], widths=[1], sites=[[(0, 0, 1), (0, 0, 2), (0, 1, 1), (0, 2, 1), (0, 3, 1)]], flank=0,
         counts=[[[1, 1, 1, 1, 1, 0]]], dinuc={}),
    # flank 1: (0, +) . A C -> 5 0 1   (0, -) reads C A . -> 2 3 5   (1, +) A C G -> 0 1 2   (2, +) C G N -> 1 2 4   (3, +) G N . -> 2 4 5
    dict(name="W = 1, flank 1", seqs=["ACGN"], widths=[1], sites=[[(0, 0, 1), (0, 0, 2), (0, 1, 1), (0, 2, 1), (0, 3, 1)]], flank=1,
         counts=[[[1, 1, 2, 0, 0, 1], [1, 1, 1, 1, 1, 0], [0, 1, 1, 0, 1, 2]]],
         dinuc={(0, 0, 1): 1, (0, 0, 6): 1, (0, 0, 11): 1, (0, 1, 1): 1, (0, 1, 6): 1}),
    # Two regions back to back, "ACG" and "TTT": a flank column of one never shows the other's bases.  Motif 0 (W = 2), flank 2:
    #   (region 0, pos 1, +) . A C G . . -> 5 0 1 2 5 5  (column 4 is NOT region 1's T)
    #   (region 1, pos 0, -) reads . T T T . . complemented -> 5 0 0 0 5 5  (column 4 is NOT region 0's G)
    # Motif 1 (W = 1, five used columns of C = 6): (region 1, pos 2, +) T T T . . -> 3 3 3 5 5
    dict(name="two adjacent regions", seqs=["ACG", "TTT"], widths=[2, 1], sites=[[(0, 1, 1), (1, 0, 2)], [(1, 2, 1)]], flank=2,
         counts=[[[0, 0, 0, 0, 0, 2], [2, 0, 0, 0, 0, 0], [1, 1, 0, 0, 0, 0], [1, 0, 1, 0, 0, 0], [0, 0, 0, 0, 0, 2], [0, 0, 0, 0, 0, 2]],
                 [[0, 0, 0, 1, 0, 0], [0, 0, 0, 1, 0, 0], [0, 0, 0, 1, 0, 0], [0, 0, 0, 0, 0, 1], [0, 0, 0, 0, 0, 1], [0, 0, 0, 0, 0, 0]]],
         dinuc={(0, 1, 1): 1, (0, 2, 6): 1, (0, 1, 0): 1, (0, 2, 0): 1, (1, 0, 15): 1, (1, 1, 15): 1}),
]


def hand_expected(case):
    counts = np.asarray(case["counts"], dtype=np.int64)
    return counts, dense(counts.shape[:2] + (16,), case["dinuc"])


LETTERS = "ACGT" * 6 + "acgt" + "NnRYKMSWBDHVU-"


def random_case(rng, n_regions=None, max_len=40):
    """Regions of every length from 1 (letters of either case, N runs, IUPAC codes), motifs of widths 1 .. 12 -- one of them without a
    site -- and sites at random legal positions, pos 0 and L - W among them, on both strands."""
    R = int(rng.integers(1, 6)) if n_regions is None else n_regions
    seqs = ["".join(rng.choice(list(LETTERS), size=int(rng.integers(1, max_len + 1)))) for _ in range(R)]
    widths = [int(w) for w in rng.integers(1, 13, size=int(rng.integers(1, 5)))]
    sites = []
    for m, W in enumerate(widths):
        per = []
        for r, s in enumerate(seqs):
            if len(s) < W or m == 1:
                continue
            for p in {0, len(s) - W, *rng.integers(0, len(s) - W + 1, size=int(rng.integers(0, 4))).tolist()}:
                per += [(r, int(p), int(st)) for st in ((1, 2) if rng.random() < 0.5 else (int(rng.integers(1, 3)),))]
        sites.append(per)
    return seqs, widths, sites


def check_invariants(stack, widths):
    for i, W in enumerate(widths):
        n = W + 2 * stack.flank
        assert np.array_equal(stack.counts[i, :n].sum(axis=1), np.full(n, stack.n_sites[i]))
        assert not stack.counts[i, n:].any()
        if stack.dinuc is not None:
            assert not stack.dinuc[i, max(n - 1, 0):].any()
            # a pair needs both columns in slots 0 .. 3: per first base, no more pairs than sites with that base at the column
            first = stack.dinuc[i, :n].reshape(n, 4, 4).sum(axis=2)
            assert (first <= stack.counts[i, :n, :4]).all()


@pytest.mark.parametrize("case", HAND, ids=[c["name"] for c in HAND])
def test_restatement_against_hand_written_cases(case):
    want_counts, want_dinuc = hand_expected(case)
    got = sitestack.site_base_counts_host(*hit_arrays(case["sites"]), case["widths"], case["seqs"], case["flank"], dinuc=True)
    assert got.counts.dtype == np.int64 and got.counts.shape == want_counts.shape and got.dinuc.shape == want_dinuc.shape
    assert np.array_equal(got.counts, want_counts)
    assert np.array_equal(got.dinuc, want_dinuc)
    assert np.array_equal(got.n_sites, [len(s) for s in case["sites"]]) and got.flank == case["flank"]
    assert sitestack.site_base_counts_host(*hit_arrays(case["sites"]), case["widths"], case["seqs"], case["flank"]).dinuc is None
    check_invariants(got, case["widths"])
    as_bytes = sitestack.site_base_counts_host(*hit_arrays(case["sites"]), case["widths"], [s.encode() for s in case["seqs"]], case["flank"], dinuc=True)
    assert np.array_equal(as_bytes.counts, want_counts) and np.array_equal(as_bytes.dinuc, want_dinuc)


def test_views_of_a_stack():
    case = HAND[4]
    got = sitestack.site_base_counts_host(*hit_arrays(case["sites"]), case["widths"], case["seqs"], case["flank"], dinuc=True)
    assert got.columns(0).shape == (6, 6) and got.columns(1).shape == (5, 6)
    assert np.array_equal(got.pfm(0), [[1, 1], [1, 0], [0, 1], [0, 0]]) and np.array_equal(got.pfm(1), [[0], [0], [0], [1]])
    ic = got.information_content(1)
    assert ic.shape == (5,) and np.allclose(ic, [2, 2, 2, 0, 0])               # T only; then no base at all
    assert np.allclose(got.information_content(0)[2], 1.0)                     # A and C, one each
    assert np.allclose(got.information_content(1, bg=[0.1, 0.1, 0.1, 0.7])[0], np.log2(1 / 0.7))


def test_refusals_of_the_restatement():
    off, si, po, st = hit_arrays([[(0, 2, 1)]])
    for seqs, widths, flank in ((["ACGT"], [3], 0), (["ACGTA"], [3], 65), (["ACGTA"], [3], -1), ([], [3], 0)):
        with pytest.raises(ValueError):
            sitestack.site_base_counts_host(off, si, po, st, widths, seqs, flank)
    with pytest.raises(ValueError):
        sitestack.site_base_counts_host(off, si, np.array([-1]), st, [3], ["ACGTA"], 0)


def test_every_used_column_sums_to_the_number_of_sites():
    rng = np.random.default_rng(20)
    for _ in range(40):
        seqs, widths, sites = random_case(rng)
        flank = int(rng.choice([0, 1, 2, 7, 64]))
        got = sitestack.site_base_counts_host(*hit_arrays(sites), widths, seqs, flank, dinuc=True)
        assert got.counts.shape == (len(widths), max(widths) + 2 * flank, 6)
        check_invariants(got, widths)
        if len(widths) > 1:
            assert not got.counts[1].any() and got.n_sites[1] == 0             # the motif without a site


def test_pfm_feeds_the_matrix_classes():
    rng = np.random.default_rng(4)
    seqs = ["".join(rng.choice(list("ACGT"), size=60)) for _ in range(30)]
    sites = [[(r, int(p), 1) for r in range(30) for p in rng.integers(0, 53, size=3)]]
    got = sitestack.site_base_counts_host(*hit_arrays(sites), [8], seqs, 3)
    pfm = matrix.PositionFrequencyMatrix(got.pfm(0), name="observed", matrix_id="M0001")
    assert np.array_equal(np.asarray(pfm.matrix).sum(axis=0), np.full(8, 90))
    pwm = pfm.to_ppm().to_pwm()
    assert np.asarray(pwm.matrix).shape == (4, 8) and np.isfinite(np.asarray(pwm.matrix)).all()


def test_restatement_against_a_numpy_count_over_the_oracles_sites(oracle, rnd):
    mats, seqs = rnd["mats"], rnd["seqs"]
    flat = oracle.c_scan_motif([m.tolist() for m in mats], rnd["cutoff_by_key"]["1e-3"].tolist(), seqs, 1, 1)
    hits = hit_arrays([[(int(s), int(p), int(d)) for s, p, _, d in per] for per in flat])
    widths = [m.shape[1] for m in mats]
    got = sitestack.site_base_counts_host(*hits, widths, seqs, 0)
    assert got.n_sites.sum() > 1000                                            # (a scan that found nothing would prove nothing)
    lut = np.full(256, 4, dtype=np.int64)
    for i, ch in enumerate("ACGT"):
        lut[ord(ch)] = lut[ord(ch.lower())] = i
    for m, per in enumerate(flat):
        W = widths[m]
        want = np.zeros((W, 6), dtype=np.int64)
        if per:
            words = np.array([list(seqs[int(s)][int(p):int(p) + W].encode()) for s, p, _, _ in per], dtype=np.uint8)      # [sites][W]
            for c in range(W):
                want[c] = np.bincount(lut[words[:, c]], minlength=6)
        assert np.array_equal(got.columns(m), want), m


def test_symbols_header_and_constants():
    with open(os.path.join(ROOT, "include", "motifscan_amd.h")) as fh:
        text = fh.read()
    table = text[:text.index("#ifndef MOTIFSCAN_AMD_H")]
    assert re.search(r"\bint\s+ms_result_site_base_counts\s*\(", text) and re.search(r"ms_result_site_base_counts\s+no reference counterpart", table)
    assert re.search(r"#define\s+MS_SITESTACK_MAX_FLANK\s+64\b", text)
    with open(os.path.join(ROOT, "include", "motifscan_amd_debug.h")) as fh:
        assert re.search(r"\bint\s+ms_debug_sitestack_dims\s*\(\s*int32_t\s+out\[4\]\s*\)", fh.read())
    assert hasattr(_lib.lib(), "ms_result_site_base_counts") and hasattr(_lib.lib(), "ms_debug_sitestack_dims")
    d = _lib.sitestack_dims()                                                  # no device needed
    assert d["threads"] % 64 == 0 and d["chunk_hits"] % d["threads"] == 0
    assert d["lds_columns"] * (6 + 16) * 4 <= 64 * 1024 < (d["lds_columns"] + 1) * (6 + 16) * 4
    assert d["lds_columns_no_dinuc"] >= d["lds_columns"]


def test_no_gpu_means_loud_failure_not_fallback():
    have_device = _lib.device_count() > 0
    out = np.zeros((1, 3, 6), dtype=np.int64)
    rc = _lib.lib().ms_result_site_base_counts(None, None, None, 0, 0, 1, 0, ctypes.c_void_p(out.ctypes.data), None, None, None)
    if have_device:
        assert rc == _lib.MS_ERR_INVALID                                       # NULL handles
        return
    assert rc == _lib.MS_ERR_RUNTIME                                           # no device: said before the handles are looked at
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _lib.check(rc)
    with pytest.raises(RuntimeError):
        sitestack.site_base_counts([[[]]], [np.ones((4, 3))], ["ACGT"])
