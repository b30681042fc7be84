"""
The host side of the bipartite motifs (motifscan_amd.bipartite; ms_scan_best_bipartite, ms_best_gaps), no GPU: the numpy restatement
`bipartite.best_bipartite_host` pinned to a scalar loop written straight from the definition (one placement, one strand, one gap and one
addition at a time), whose element sums are in turn tied to ms_scan_best's walk in plain Python floats; the planted case, whose margins
are established here on the restatement alone; `specs_from_spacing` on hand-built histograms; what must fail loudly without a GPU; and
the plan header's stand-alone program under ASan + UBSan (motifscan_amd/csrc/ms_bipartite_plan.h,
tests/sanitize/bipartite_plan_asan.cpp).  tests/test_gpu_bipartite.py holds the device to the same restatement byte for byte.

ms_scan_best's walk "in plain Python floats" is tests/test_gpu_best.py::python_best; it is imported from there, unchanged.
"""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import bipartite_cases as bc
from dimodel_cases import random_dna, random_pwm
from motifscan_amd import _lib, bipartite, enrich, pairs, scanner
from motifscan_amd.bipartite import Bipartite
from test_gpu_best import python_best

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "motifscan_amd", "csrc")
BIN = os.path.join(ROOT, "tests", "sanitize", "bipartite_plan_asan.bin")


# ------------------------------------------------------------------------------------------------ the symbols, no device

def test_headers_declare_the_entry_points_and_the_library_has_them():
    with open(os.path.join(ROOT, "include", "motifscan_amd.h")) as fh:
        text = fh.read()
    for name in ("ms_scan_best_bipartite", "ms_best_gaps", "ms_best_gaps_device"):
        assert re.search(r"\bint\s+%s\s*\(" % name, text) and hasattr(_lib.lib(), name)
    with open(os.path.join(ROOT, "include", "motifscan_amd_debug.h")) as fh:
        assert re.search(r"\bint\s+ms_debug_bipartite_dims\s*\(", fh.read())
    d = _lib.bipartite_dims()
    assert d["threads"] % 64 == 0 and d["seg_windows"] % 64 == 0 and d["max_width"] >= 64 and d["max_gap"] >= 64
    assert 64 * d["halo_strips"] >= d["max_width"] + d["max_gap"]                     # a second half lies inside the halo
    assert 4 * 2 * d["max_width"] <= d["tile_entries"]                                # every spec fits one tile
    assert d["lds_bytes"] >= 16 * (d["tile_entries"] + 1) and 2 * d["lds_bytes"] <= 160 * 1024       # the tile and the rings; two blocks a CU
    assert _lib.lib().ms_debug_bipartite_dims(None) == _lib.MS_ERR_INVALID


def test_binding_checks_its_arguments_without_a_library_call():
    class Handle:
        h = None
    for mask in (0, 4, -1):
        with pytest.raises(ValueError, match="strand mask"):
            _lib.scan_best_bipartite(Handle(), [], Handle(), mask)
    with pytest.raises(ValueError, match="flags"):
        _lib.scan_best_bipartite(Handle(), [], Handle(), 3, flags=1)
    with pytest.raises(ValueError, match="gap_min, gap_max"):
        _lib.scan_best_bipartite(Handle(), [(0, 0, 0, 1)], Handle())
    with pytest.raises(ValueError, match="strand mask"):
        bipartite.best_bipartite_host([], [], [], 5)
    a, b, flip, g0, g1 = bipartite.spec_arrays([Bipartite(1, 2, 1, 3, 4), (5, 6, 0, 7, 8)])
    assert (a.tolist(), b.tolist(), flip.tolist(), g0.tolist(), g1.tolist()) == ([1, 5], [2, 6], [1, 0], [3, 7], [4, 8])
    assert (a.dtype, flip.dtype, g1.dtype) == (np.int32, np.uint8, np.int32) and bipartite.spec_arrays([])[2].shape == (0,)


def test_no_gpu_means_loud_failure_not_fallback():
    if _lib.device_count() > 0:
        pytest.skip("a GPU is visible")
    pw = _lib.PwmSet.from_matrices([random_pwm(3, 1)])
    h = ctypes.c_void_p()
    zero = np.zeros(1, dtype=np.int32)
    p32 = _lib.ptr(zero, ctypes.c_int32)
    rc = _lib.lib().ms_scan_best_bipartite(pw.h, p32, p32, _lib.ptr(np.zeros(1, dtype=np.uint8), ctypes.c_uint8), p32, p32, 1, None, 3, 0, ctypes.byref(h))
    assert rc == _lib.MS_ERR_RUNTIME and not h.value       # no device: said before the handles are looked at
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _lib.check(rc)
    pw.close()

    class Region:
        chrom, start, end, summit = "chr1", 2, 12, 7

    class Genome:
        chrom_sizes = {"chr1": 20}

        def fetch_sequence(self, chrom, start, end):
            return "ACGTACGTACGTACGTACGT"[start:end]

    class Pwm:
        matrix = random_pwm(3, 1)
    sc = scanner.Scanner(Genome(), [Region()])
    with pytest.raises(RuntimeError):
        sc.best_sites_bipartite([Pwm], [Bipartite(0, 0, 0, 0, 2)])
    with pytest.raises(RuntimeError):
        sc.rank_sum_bipartite([Pwm], [Bipartite(0, 0, 0, 0, 2)], sc)


# ------------------------------------------------------------------------------------------------ the restatement against the scalar loop

@pytest.fixture(scope="module")
def small():
    d = _lib.bipartite_dims()
    mats = bc.matrices(d["max_width"])
    specs = bc.world_specs(d["max_gap"])
    return mats, specs, bc.short_regions(mats, specs)


def test_element_sums_are_ms_scan_bests():
    """F(p) and R(p) of the scalar loop and of the restatement are the raw sums of ms_scan_best's walk: python_best on the one window
    seq[p : p + W] returns raw / max_raw of '+' (mask 1) and of '-' (mask 2)."""
    rng = np.random.default_rng(5)
    n = 0
    for w in (1, 2, 3, 6, 31, 32, 33, 64):
        mat = random_pwm(w, 300 + w)
        seq = bc.with_n(random_dna(rng, w + 11), 3, w + 2) if w > 3 else random_dna(rng, w + 11)
        max_raw = bc.scalar_max_raw(mat)
        assert max_raw == bipartite.max_raw_host(mat) > 0
        sums = bc.scalar_element_sums(mat, seq)
        fwd, rev = bipartite.element_sums_host(mat, seq)
        assert len(sums) == len(fwd) == 12
        for p, (f, r) in enumerate(sums):
            assert (fwd[p], rev[p]) == (f, r)
            assert python_best(mat, seq[p:p + w], 1)[0] == f / max_raw and python_best(mat, seq[p:p + w], 2)[0] == r / max_raw
            n += 1
    assert n == 96


@pytest.mark.parametrize("mask", (1, 2, 3))
def test_best_bipartite_host_equals_the_scalar_walk(small, mask):
    mats, specs, seqs = small
    got = bipartite.best_bipartite_host(mats, specs, seqs, mask)
    want = bc.scalar_planes(mats, specs, seqs, mask)
    bc.same_planes(got, want)
    score, pos, strand, gap = got
    unscorable = [k for k, sp in enumerate(specs) if not bipartite.scorable_host(mats, sp)]
    assert unscorable == [0, 9, 13, len(specs) - 1] and np.isnan(score[unscorable]).all()
    assert [bc.scalar_scorable(mats, sp) for sp in specs] == [k not in unscorable for k in range(len(specs))]
    assert (strand == 1).any() == bool(mask & 1) and (strand == 2).any() == bool(mask & 2)
    ok = [k for k in range(len(specs)) if k not in unscorable]
    assert np.isfinite(score[ok]).sum() > 500 and np.isnan(score[ok]).sum() > 100          # (the cases hold what they are meant to hold)
    for k in ok:                                           # a spec of several gaps between two random elements wins with more than one of them
        if k in (6, 8, 10, 11, 21, 23):
            assert specs[k].gap_max > specs[k].gap_min and len(set(gap[k][gap[k] >= 0].tolist())) > 1, k
        assert np.all((gap[k] == -1) | ((gap[k] >= specs[k].gap_min) & (gap[k] <= specs[k].gap_max)))


@pytest.mark.parametrize("mask", (1, 3))
def test_random_specs_and_regions_equal_the_scalar_walk(mask):
    rng = np.random.default_rng(100 + mask)
    mats = [random_pwm(int(w), 40 + i) for i, w in enumerate(rng.integers(1, 13, 7))] + [random_pwm(40, 50)]
    specs = []
    for _ in range(24):
        g0 = int(rng.integers(0, 12))
        specs.append(Bipartite(int(rng.integers(0, 8)), int(rng.integers(0, 8)), int(rng.integers(0, 2)), g0, g0 + int(rng.integers(0, 9))))
    seqs = [random_dna(rng, int(n)) for n in rng.integers(0, 140, 30)]
    seqs += [bc.with_n(random_dna(rng, 90), *rng.integers(0, 90, 6).tolist()) for _ in range(6)]
    got = bipartite.best_bipartite_host(mats, specs, seqs, mask)
    bc.same_planes(got, bc.scalar_planes(mats, specs, seqs, mask))
    assert np.isfinite(got[0]).sum() > 400 and len(set(got[3].ravel().tolist())) > 10


def test_ties_flips_and_holes_by_hand(small):
    mats, specs, _ = small
    m = bc.M
    ties = bc.tie_regions()
    # a homopolymer under column-constant matrices: every placement ties -> pos 0, '+', g_min
    s, p, d, g = bipartite.best_bipartite_host(mats, [Bipartite(m["const"], m["const"], 0, 2, 5)], ties[:1], 3)
    assert (p[0, 0], d[0, 0], g[0, 0]) == (0, 1, 2) and s[0, 0] == 1.0
    s, p, d, g = bipartite.best_bipartite_host(mats, [Bipartite(m["const"], m["const"], 1, 2, 5)], ties[:1], 2)
    assert (p[0, 0], d[0, 0], g[0, 0]) == (0, 2, 2)
    # HALF then CA at gaps 2 and 4 only: the smaller gap; on '-' the composite is not there
    s, p, d, g = bipartite.best_bipartite_host(mats, [Bipartite(m["half"], m["ca"], 0, 0, 6)], ties[1:2], 3)
    assert (p[0, 0], d[0, 0], g[0, 0]) == (4, 1, 2) and s[0, 0] == 1.0
    # the same site twice: the earlier position
    s, p, d, g = bipartite.best_bipartite_host(mats, [Bipartite(m["half"], m["half"], 0, 1, 5)], ties[2:3], 3)
    assert (p[0, 0], d[0, 0], g[0, 0]) == (3, 1, 3) and s[0, 0] == 1.0
    # a == b with flip 1: the '+' and the '-' placement of every (p, g) are the same sum, so '+' keeps every cell
    seqs = [random_dna(np.random.default_rng(k), 50) for k in range(6)]
    s, p, d, g = bipartite.best_bipartite_host(mats, [Bipartite(m["w3"], m["w3"], 1, 0, 4)], seqs, 3)
    assert (d == 1).all()
    only_minus = bipartite.best_bipartite_host(mats, [Bipartite(m["w3"], m["w3"], 1, 0, 4)], seqs, 2)
    assert np.array_equal(only_minus[0], s) and np.array_equal(only_minus[1], p) and np.array_equal(only_minus[3], g) and (only_minus[2] == 2).all()
    # flip 0 against flip 1 on a reverse-complemented second half
    rc = "TGACCT"
    s0 = bipartite.best_bipartite_host(mats, [Bipartite(m["half"], m["half"], 0, 0, 3), Bipartite(m["half"], m["half"], 1, 0, 3)], ["CC" + bc.HALF + "GG" + rc + "CC"], 1)
    assert s0[0][1, 0] == 1.0 and s0[0][0, 0] < 1.0 and (s0[1][1, 0], s0[3][1, 0]) == (2, 2)
    # -inf entries: a region in which every placement sums to -inf has no winner; one finite placement wins
    hs = Bipartite(m["holes"], m["w1"], 0, 0, 4)
    s, p, d, g = bipartite.best_bipartite_host(mats, [hs], ["A" * 30, "A" * 12 + "C" + "A" * 17], 1)
    assert np.isnan(s[0, 0]) and (p[0, 0], d[0, 0], g[0, 0]) == (-1, 0, -1)
    assert p[0, 1] == 12 and np.isfinite(s[0, 1])
    bc.same_planes((s, p, d, g), bc.scalar_planes(mats, [hs], ["A" * 30, "A" * 12 + "C" + "A" * 17], 1))
    # non-ACGT bases in the spacer are never read
    site = bc.HALF + "TTT" + bc.HALF
    a = bipartite.best_bipartite_host(mats, [Bipartite(m["half"], m["half"], 0, 1, 5)], ["CC" + site + "CC", "CC" + bc.HALF + "NNN" + bc.HALF + "CC"], 3)
    assert all(np.array_equal(x[:, 0], x[:, 1]) for x in a) and a[0][0, 0] == 1.0
    # the rule is on the SUM of the max_raw: an all-zero partner is legal, two of them are not
    assert bipartite.scorable_host(mats, Bipartite(m["half"], m["zero"], 0, 0, 0)) and not bipartite.scorable_host(mats, Bipartite(m["zero"], m["zero"], 0, 0, 0))
    assert bipartite.scorable_host(mats, Bipartite(m["neg"], m["half"], 0, 0, 0)) and not bipartite.scorable_host(mats, Bipartite(m["neg"], m["zero"], 0, 0, 0))


# ------------------------------------------------------------------------------------------------ the planted case, on the restatement

def planted_host():
    """(bipartite RankSum, half-site RankSum, fixed-spacer RankSum) on the restatement alone."""
    inputs, controls, mats = bc.planted_case()
    specs = [bc.PLANTED_SPEC, bc.PLANTED_FIXED]
    xa, xb = bipartite.best_bipartite_host(mats, specs, inputs, 3)[0], bipartite.best_bipartite_host(mats, specs, controls, 3)[0]

    def half(seqs):                                        # the half-site PWM's best score per region, both strands
        mr = bipartite.max_raw_host(mats[0])
        return np.array([[max(np.concatenate(bipartite.element_sums_host(mats[0], s))) / mr for s in seqs]])
    return enrich.rank_sum_host(xa[:1], xb[:1]), enrich.rank_sum_host(half(inputs), half(controls)), enrich.rank_sum_host(xa[1:], xb[1:])


def test_planted_case_margins_on_the_restatement():
    bip, half, fixed = planted_host()
    a, h, f = float(bip.auroc()[0]), float(half.auroc()[0]), float(fixed.auroc()[0])
    print(f"planted case: bipartite AUROC {a:.4f}, half-site PWM AUROC {h:.4f}, fixed-spacer-3 AUROC {f:.4f}")
    assert (bip.na, bip.nb) == (200, 200)
    assert a >= 0.95 and h <= 0.55 and f <= 0.60


# ------------------------------------------------------------------------------------------------ specs_from_spacing

def hand_spacing(widths, anchor, partners, max_dist, pairs_at):
    """A PairSpacing built by hand: pairs_at = [(row, orientation o = 2 (anchor on '-') + (partner on '-'), anchor start, partner start, count)]
    in forward coordinates; the bins follow ms_result_pair_spacing's axis."""
    n_bins = 2 * max_dist + 1
    counts = np.zeros((len(partners), 4, n_bins), dtype=np.int64)
    diff = np.array([widths[p] - widths[anchor] for p in partners])
    for row, o, pa, pp, c in pairs_at:
        twice = 2 * (pp - pa) + int(diff[row])             # twice (partner centre - anchor centre)
        counts[row, o, (twice - (int(diff[row]) & 1)) // 2 + max_dist] += c
    x = np.stack([pairs.spacing_axis(max_dist, d) for d in diff])
    return pairs.PairSpacing(counts, counts.sum(axis=(1, 2)), x, pairs.fold_orientations(counts, diff))


def test_specs_from_spacing_on_hand_built_histograms():
    widths = [6, 6, 9, 4]                                  # anchor 0; partner 1: even difference, partners 2 and 3: odd
    sp = hand_spacing(widths, 0, [1, 2, 3], 40, [
        (0, 0, 100, 109, 5), (0, 0, 100, 111, 2),          # '+/+', partner downstream at gaps 3 and 5
        (0, 3, 100, 88, 4),                                # '-/-', partner at lower coordinates: seen from the anchor's strand it is DOWNSTREAM at gap 6
        (0, 0, 100, 103, 9),                               # overlapping sites: no spec
        (0, 1, 100, 108, 3),                               # '+/-' downstream, gap 2: the halves face each other
        (0, 2, 100, 90, 1),                                # '-/+', partner at lower coordinates = downstream along the anchor's strand, gap 4
        (0, 1, 100, 90, 6),                                # '+/-' upstream: the halves point away from each other -- no spec under the definition
        (1, 0, 100, 80, 2), (1, 0, 100, 79, 2),            # a wider partner (odd difference) upstream on the same strand: gaps 11 and 12
        (1, 0, 100, 134, 7),                               # gap 28: above max_gap = 20
        (2, 1, 100, 107, 1), (2, 1, 100, 111, 1),          # a narrower partner (odd difference), opposite strand downstream: gaps 1 and 5
        (2, 0, 100, 102, 8),                               # overlap
    ])
    got = bipartite.specs_from_spacing(sp, 0, [1, 2, 3], widths, min_count=1, max_gap=20)
    assert got == [Bipartite(0, 1, 0, 3, 6), Bipartite(0, 1, 1, 2, 4), Bipartite(2, 0, 0, 11, 12), Bipartite(0, 3, 1, 1, 5)]
    got = bipartite.specs_from_spacing(sp, 0, [1, 2, 3], widths, min_count=2, max_gap=20)
    assert got == [Bipartite(0, 1, 0, 3, 6), Bipartite(0, 1, 1, 2, 2), Bipartite(2, 0, 0, 11, 12)]
    got = bipartite.specs_from_spacing(sp, 0, [1, 2, 3], widths, min_count=1, max_gap=64)
    assert Bipartite(0, 2, 0, 28, 28) in got and len(got) == 5
    assert bipartite.specs_from_spacing(sp, 0, [1, 2, 3], widths, min_count=100) == []
    with pytest.raises(ValueError, match="oriented=True"):
        bipartite.specs_from_spacing(sp._replace(oriented=None), 0, [1, 2, 3], widths)
    with pytest.raises(ValueError, match="rows"):
        bipartite.specs_from_spacing(sp, 0, [1, 2], widths)


def test_a_spec_from_a_spacing_bin_scores_the_pair_that_made_the_bin():
    """The arithmetic of specs_from_spacing closes the loop: two sites placed by hand, their bin, the spec, and the restatement's best
    placement is that pair at that gap -- for every arrangement a spec can express."""
    mats = [bc.consensus_pwm("AGGTCA"), bc.consensus_pwm("CCATGTTAC")]
    widths = [6, 9]
    rc = {"A": "T", "C": "G", "G": "C", "T": "A"}

    def word(m, minus):
        w = "AGGTCA" if m == 0 else "CCATGTTAC"
        return "".join(rc[c] for c in reversed(w)) if minus else w
    for o, pa, pp in ((0, 20, 31), (0, 31, 18), (1, 20, 29), (3, 31, 18), (2, 31, 20)):
        seq = list("T" * 60)
        seq[pa:pa + 6] = word(0, o >= 2)
        seq[pp:pp + 9] = word(1, o & 1)
        sp = hand_spacing(widths, 0, [1], 40, [(0, o, pa, pp, 1)])
        specs = bipartite.specs_from_spacing(sp, 0, [1], widths)
        assert len(specs) == 1
        s, p, d, g = bipartite.best_bipartite_host(mats, specs, ["".join(seq)], 3)
        left = min(pa, pp)
        assert s[0, 0] == 1.0 and p[0, 0] == left and g[0, 0] == specs[0].gap_min == specs[0].gap_max
        assert g[0, 0] == max(pa, pp) - left - (6 if pa < pp else 9)
        assert d[0, 0] == (2 if o >= 2 else 1)             # the anchor on '-': the composite is read on '-'


# ------------------------------------------------------------------------------------------------ the plan header under the sanitizers

@pytest.mark.skipif(shutil.which("g++") is None or shutil.which("make") is None, reason="needs g++ and make")
def test_plan_header_under_address_and_ub_sanitizers():
    asan = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    if not (os.path.isabs(asan) and os.path.exists(asan)):
        pytest.skip("the sanitizer runtimes are not installed on this box")
    subprocess.run(["make", "-s", "-C", CSRC, "bipartite_plan_asan"], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([BIN], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "bipartite_plan_asan: ok" in out.stdout, (out.stdout + out.stderr)[-4000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-4000:]
    assert int(out.stdout.split("(")[1].split()[0]) >= 100
