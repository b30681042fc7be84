"""
The host side of the first-order models (motifscan_amd.dimodel; ms_dimodelset_*, ms_scan_best_dimodels), no GPU: the numpy restatement
`dimodel.best_sites_host` pinned to a scalar loop that scores one window, one strand and one addition at a time; the Viterbi maximum
against brute force over all 4^W sequences and against the C++ header's value; the degenerate model of a PWM against the PWM's own sums
and against the best-site reference the PWM scan is held to; `from_counts` against exact rational arithmetic and hand-written values;
`from_site_stack`'s slots; the planted case, whose margins are established here on the restatements alone; what must fail loudly
without a GPU; and the plan header's stand-alone program under ASan + UBSan (motifscan_amd/csrc/ms_dimodel_plan.h,
tests/sanitize/dimodel_plan_asan.cpp).  tests/test_gpu_dimodel.py holds the device to the same restatement byte for byte.

The best-site reference of the PWM scan: tests/test_best_host.py itself restates no walk (it checks the binding's host side);
ms_scan_best's walk "in plain Python floats" is tests/test_gpu_best.py::python_best, next to the oracle that file compares with.  It is
imported from there, unchanged.
"""
import ctypes
import math
import os
import re
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import dimodel_cases as dc
from motifscan_amd import _lib, dimodel, enrich, kmers, scanner, sitestack
from test_gpu_best import python_best

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "motifscan_amd", "csrc")
BIN = os.path.join(ROOT, "tests", "sanitize", "dimodel_plan_asan.bin")


# ------------------------------------------------------------------------------------------------ the symbols, no device

def test_headers_declare_the_entry_points_and_the_library_has_them():
    with open(os.path.join(ROOT, "include", "motifscan_amd.h")) as fh:
        text = fh.read()
    for name in ("ms_dimodelset_create", "ms_dimodelset_size", "ms_dimodelset_max_raw", "ms_scan_best_dimodels"):
        assert re.search(r"\bint\s+%s\s*\(" % name, text) and hasattr(_lib.lib(), name)
    assert re.search(r"\bvoid\s+ms_dimodelset_free\s*\(", text) and hasattr(_lib.lib(), "ms_dimodelset_free")
    with open(os.path.join(ROOT, "include", "motifscan_amd_debug.h")) as fh:
        assert re.search(r"\bint\s+ms_debug_dimodel_dims\s*\(", fh.read())
    d = _lib.dimodel_dims()
    assert d["threads"] % 64 == 0 and d["seg_windows"] == 64 * d["strips"] and d["max_width"] >= 64 and d["word_steps"] == 31
    assert 4 * (4 * d["max_width"] - 3) <= d["tile_entries"] < 4 * (4 * (d["max_width"] + 1) - 3)       # every admissible model fits one tile, the next does not
    assert _lib.lib().ms_debug_dimodel_dims(None) == _lib.MS_ERR_INVALID


def test_model_set_needs_no_device_and_checks_its_arguments():
    cap = _lib.dimodel_dims()["max_width"]
    models = [dc.random_model(w, 10 + w) for w in (1, 2, 9, 64, cap)]
    ms = _lib.DiModelSet.from_models(models)
    n = ctypes.c_int32(-1)
    _lib.check(_lib.lib().ms_dimodelset_size(ms.h, ctypes.byref(n)))
    assert n.value == len(ms) == 5
    assert ms.max_raw().tobytes() == np.array([dimodel.max_raw_host(m) for m in models]).tobytes()
    ms.close()
    empty = _lib.DiModelSet.from_models([])
    assert len(empty) == 0 and empty.max_raw().shape == (0,)
    empty.close()
    L, h = _lib.lib(), ctypes.c_void_p()
    one = np.zeros((1, 16))
    for widths, text in (([0], "width 0"), ([-3], "width -3"), ([cap + 1], "at most %d columns" % cap)):
        w = np.array(widths, dtype=np.int32)
        vals = np.zeros((max(int(w[0]), 1), 16))
        with pytest.raises(ValueError, match=text):
            _lib.DiModelSet(vals, w)
    assert L.ms_dimodelset_create(_lib.ptr(one, ctypes.c_double), _lib.ptr(np.ones(1, dtype=np.int32), ctypes.c_int32), 1, None) == _lib.MS_ERR_INVALID
    assert L.ms_dimodelset_create(None, None, 1, ctypes.byref(h)) == _lib.MS_ERR_INVALID and not h.value
    assert L.ms_dimodelset_create(None, None, -1, ctypes.byref(h)) == _lib.MS_ERR_INVALID
    assert L.ms_dimodelset_size(None, ctypes.byref(n)) == _lib.MS_ERR_INVALID and L.ms_dimodelset_max_raw(None, None) == _lib.MS_ERR_INVALID
    with pytest.raises(ValueError, match="16 \\* width"):
        _lib.DiModelSet(np.zeros((3, 16)), [2])
    with pytest.raises(TypeError):
        dimodel.DiModelSet([np.zeros((4, 3))])
    with pytest.raises(ValueError):
        dimodel.DiModel(np.zeros(3), np.zeros((2, 16)))
    with pytest.raises(ValueError):
        dimodel.DiModel(np.zeros(4), np.zeros((2, 4)))


def test_binding_checks_strand_and_flags_without_a_library_call():
    class Handle:
        h = None
    for mask in (0, 4, -1):
        with pytest.raises(ValueError, match="strand mask"):
            _lib.scan_best_dimodels(Handle(), Handle(), mask)
    with pytest.raises(ValueError, match="flags"):
        _lib.scan_best_dimodels(Handle(), Handle(), 3, flags=1)
    with pytest.raises(ValueError, match="strand mask"):
        dimodel.best_sites_host([], [], 5)


def test_no_gpu_means_loud_failure_not_fallback():
    if _lib.device_count() > 0:
        pytest.skip("a GPU is visible")
    ms = _lib.DiModelSet.from_models([dc.random_model(3, 1)])
    h = ctypes.c_void_p()
    rc = _lib.lib().ms_scan_best_dimodels(ms.h, None, 3, 0, ctypes.byref(h))                   # no device: said before the handles are looked at
    assert rc == _lib.MS_ERR_RUNTIME and not h.value
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _lib.check(rc)
    ms.close()

    class Region:
        chrom, start, end, summit = "chr1", 2, 12, 7

    class Genome:
        chrom_sizes = {"chr1": 20}

        def fetch_sequence(self, chrom, start, end):
            return "ACGTACGTACGTACGTACGT"[start:end]
    sc = scanner.Scanner(Genome(), [Region()])
    with pytest.raises(RuntimeError):
        sc.best_sites_dimodels([dc.random_model(3, 1)])
    with pytest.raises(RuntimeError):
        sc.rank_sum_dimodels([dc.random_model(3, 1)], sc)


# ------------------------------------------------------------------------------------------------ the restatement against the scalar loop

@pytest.fixture(scope="module")
def small():
    return dc.small_models() + [dc.negative_model(5, 3)], dc.small_regions()


@pytest.mark.parametrize("mask", (1, 2, 3))
def test_best_sites_host_equals_the_scalar_walk(small, mask):
    models, seqs = small
    assert {m.width for m in models} >= {1, 2, 3, 31, 32, 33, 34, 64}
    got = dimodel.best_sites_host(models, seqs, mask)
    want = dc.scalar_planes(models, seqs, mask)
    dc.same_planes(got, want)
    score, pos, strand = got
    assert np.isnan(score[-1]).all()                       # the unscorable model's row
    assert np.isnan(score).any() and (strand == 1).any() == bool(mask & 1) and (strand == 2).any() == bool(mask & 2)
    holes = [i for i, m in enumerate(models[:-1]) if np.isneginf(m.trans).any() or np.isneginf(m.start).any()]
    assert len(holes) >= 8 and np.isfinite(score[holes]).any()


def test_n_placements_by_hand():
    m = dimodel.DiModel(np.ones(4), np.ones((3, 16)))     # every window scores alike: the earliest window without an N wins
    core = "ACGTAC"
    s, p, d = dimodel.best_sites_host([m], [dc.with_n(core, 0), dc.with_n(core, 5), dc.with_n(core, 0, 5), dc.with_n(core, 1), dc.with_n(core, 4), dc.with_n(core, 2)], 1)
    assert p[0].tolist() == [1, 0, 1, 2, 0, -1] and d[0].tolist() == [1, 1, 1, 1, 1, 0] and np.isnan(s[0, 5])
    r = dc.random_model(4, 5)
    lower = dimodel.best_sites_host([r], ["acgtAC"], 3)
    upper = dimodel.best_sites_host([r], ["ACGTAC"], 3)
    dc.same_planes(lower, upper)


@pytest.mark.parametrize("mask", (1, 2, 3))
def test_ties_keep_the_earliest_window_and_the_plus_strand(mask):
    models, seqs = dc.tie_cases()
    got = dimodel.best_sites_host(models, seqs, mask)
    dc.same_planes(got, dc.scalar_planes(models, seqs, mask))
    score, pos, strand = got
    assert pos[0, 0] < 12                                  # nine copies of a 12-base unit: the first copy's window
    assert pos[1, 1] == 4 and score[1, 1] == 1.0           # the first of two palindromic sites
    if mask == 3:
        assert (strand[1] == 1).all()                      # a strand-symmetric model ties on every window: '+' comes first


def test_every_window_forbidden_gives_no_winner():
    m = dimodel.DiModel([1.0, 1.0, 1.0, 1.0], np.full((2, 16), 0.5))
    m.trans[0, 4 * 0 + 0] = -np.inf                        # A after A at column 1 ...
    m.trans[1, 4 * 3 + 3] = -np.inf                        # ... and T after T at column 2: "AAAA" is barred on both strands
    assert dimodel.scorable_host(m)
    s, p, d = dimodel.best_sites_host([m], ["AAAAAA", "AAACAA"], 3)
    assert np.isnan(s[0, 0]) and p[0, 0] == -1 and d[0, 0] == 0
    assert (p[0, 1], d[0, 1]) == (2, 1) and s[0, 1] == 1.0     # ACA: 1 + 0.5 + 0.5 = max_raw
    dc.same_planes((s, p, d), dc.scalar_planes([m], ["AAAAAA", "AAACAA"], 3))


# ------------------------------------------------------------------------------------------------ max_raw

def test_max_raw_is_the_brute_force_maximum_and_the_headers_value():
    models = [dc.random_model(w, 300 + 10 * w + k, holes=k) for w in range(1, 7) for k in (0, 1, 2, 3)]
    models.append(dimodel.DiModel([-np.inf] * 4, np.zeros((2, 16))))                          # nothing is reachable: -inf
    ms = _lib.DiModelSet.from_models(models)
    lib_values = ms.max_raw()
    ms.close()
    n_inf = 0
    for m, from_lib in zip(models, lib_values.tolist()):
        got = dimodel.max_raw_host(m)
        assert got == dc.scalar_max_raw(m) == dc.brute_max_raw(m)
        assert np.float64(got).tobytes() == np.float64(from_lib).tobytes()
        n_inf += int(np.isneginf(m.trans).any())
        if dimodel.scorable_host(m):
            site = dc.viterbi_sequence(m)
            assert dc.scalar_window(m, site, 0, False) == got
            s, p, d = dimodel.best_sites_host([m], ["".join(site)], 1)
            assert s[0, 0] == 1.0 and (p[0, 0], d[0, 0]) == (0, 1)
    assert n_inf >= 12 and not dimodel.scorable_host(models[-1])
    wide = dc.random_model(64, 9, holes=3)
    assert dimodel.max_raw_host(wide) == dc.scalar_max_raw(wide) == dc.scalar_window(wide, dc.viterbi_sequence(wide), 0, False)


def test_scorable_follows_the_header():
    ok = dc.random_model(4, 1)
    assert dimodel.scorable_host(ok) and not dimodel.scorable_host(dc.negative_model(4, 1))
    for bad in (np.nan, np.inf):
        m = dimodel.DiModel(ok.start, ok.trans)
        m.trans[1, 7] = bad
        assert not dimodel.scorable_host(m)
        m = dimodel.DiModel(ok.start, ok.trans)
        m.start[2] = bad
        assert not dimodel.scorable_host(m)
    m = dimodel.DiModel(ok.start, ok.trans)
    m.trans[1, 7] = -np.inf
    assert dimodel.scorable_host(m)
    v = ok.values()
    v[0, 4:] = np.nan                                      # entries 4 .. 15 of row 0 are never read
    ms = _lib.DiModelSet(v, [4])
    assert ms.max_raw()[0] == dimodel.max_raw_host(ok)
    ms.close()


# ------------------------------------------------------------------------------------------------ the degenerate model

def pwm_sums(mat, seq, p):
    """The PWM scan's raw sums of one window, in its order: column c adds M[b][c] forward and M[3 - b][W - 1 - c] reverse."""
    W = mat.shape[1]
    fwd = rev = 0.0
    for c in range(W):
        b = dc.CODE[seq[p + c]]
        fwd += float(mat[b, c])
        rev += float(mat[3 - b, W - 1 - c])
    return fwd, rev


def test_from_pwm_gives_the_pwm_sums_on_both_strands_byte_for_byte():
    rng = np.random.default_rng(11)
    n = 0
    for w in list(range(1, 12)) + [31, 32, 33, 64]:
        for k in range(3):
            mat = dc.random_pwm(w, 50 * w + k)
            deg = dimodel.DiModel.from_pwm(mat)
            assert deg.width == w
            seq = dc.random_dna(rng, w + 9)
            fwd, rev = dimodel.window_sums_host(deg, seq)
            for p in range(10):
                assert (fwd[p], rev[p]) == pwm_sums(mat, seq, p) == (dc.scalar_window(deg, seq, p, False), dc.scalar_window(deg, seq, p, True))
                n += 1
    assert n == 450


@pytest.mark.parametrize("mask", (1, 2, 3))
def test_from_pwm_best_sites_equal_the_pwm_scans_reference_on_n_free_regions(mask):
    rng = np.random.default_rng(12)
    mats = [dc.random_pwm(w, 900 + w) for w in (1, 2, 5, 8, 12, 31, 33)]
    seqs = [dc.random_dna(rng, n) for n in (0, 4, 12, 40, 97)] + ["ACGT" * 12]
    got = dimodel.best_sites_host([dimodel.DiModel.from_pwm(m) for m in mats], seqs, mask)
    want = [[python_best(m, s, mask) for s in seqs] for m in mats]
    ws = np.array([[c[0] for c in row] for row in want])
    wp = np.array([[c[1] for c in row] for row in want], dtype=np.int32)
    wd = np.array([[c[2] for c in row] for row in want], dtype=np.int8)
    dc.same_planes(got, (ws, wp, wd))
    for m in mats:                                         # (the PWM's clamped max_raw is the Viterbi maximum here: every column holds a positive entry)
        assert dimodel.max_raw_host(dimodel.DiModel.from_pwm(m)) == dc.pwm_max_raw(m)


# ------------------------------------------------------------------------------------------------ from_counts, from_site_stack

def test_from_counts_against_exact_fractions_and_by_hand():
    rng = np.random.default_rng(3)
    first = rng.integers(0, 50, 4)
    pairs = rng.integers(0, 30, (4, 16))
    pairs[2, 4:8] = 0                                      # a row without a single site: the pseudocounts alone
    cond = rng.dirichlet(np.full(4, 3.0), size=4)
    init = rng.dirichlet(np.full(4, 3.0))
    for pc in (1.0, 0.5):
        m = dimodel.DiModel.from_counts(first, pairs, cond, init, pseudocount=pc)
        assert m.width == 5
        fpc = Fraction(pc)
        for b in range(4):
            exact = (Fraction(int(first[b])) + fpc) / (Fraction(int(first.sum())) + 4 * fpc) / Fraction(float(init[b]))
            assert abs(m.start[b] - math.log(exact)) <= 0.5e-5 + 1e-12
        for j in range(4):
            for a in range(4):
                row = sum(int(v) for v in pairs[j, 4 * a:4 * a + 4])
                for b in range(4):
                    exact = (Fraction(int(pairs[j, 4 * a + b])) + fpc) / (Fraction(row) + 4 * fpc) / Fraction(float(cond[a, b]))
                    assert abs(m.trans[j, 4 * a + b] - math.log(exact)) <= 0.5e-5 + 1e-12
        assert np.array_equal(m.trans, np.around(m.trans, 5)) and np.array_equal(m.start, np.around(m.start, 5))
    # by hand, three columns, a flat background: first = (6, 0, 0, 2) -> (7, 1, 1, 3) / 12 / 0.25
    pairs = np.zeros((2, 16), dtype=np.int64)
    pairs[0, 4 * 0 + 1] = 6                                # A then C six times: row A = (1, 7, 1, 1) / 10
    pairs[0, 4 * 3 + 3] = 2                                # T then T twice:     row T = (1, 1, 1, 3) / 6
    pairs[1, 4 * 1 + 2] = 4                                # C then G four times, C then T twice: row C = (1, 1, 5, 3) / 10
    pairs[1, 4 * 1 + 3] = 2
    m = dimodel.DiModel.from_counts([6, 0, 0, 2], pairs, np.full((4, 4), 0.25), np.full(4, 0.25))
    assert m.start.tolist() == [0.84730, -1.09861, -1.09861, 0.0]
    assert m.trans[0, 0:4].tolist() == [-0.91629, 1.02962, -0.91629, -0.91629]
    assert m.trans[0, 12:16].tolist() == [-0.40547, -0.40547, -0.40547, 0.69315]
    assert m.trans[0, 4:8].tolist() == [0.0, 0.0, 0.0, 0.0] == m.trans[1, 0:4].tolist()       # no site: (1, 1, 1, 1) / 4 against 0.25
    assert m.trans[1, 4:8].tolist() == [-0.91629, -0.91629, 0.69315, 0.18232]
    one = dimodel.DiModel.from_counts([1, 2, 3, 4], np.zeros((0, 16)), np.full((4, 4), 0.25), np.full(4, 0.25))
    assert one.width == 1
    for bad in (dict(pseudocount=0.0), dict(pseudocount=-1.0)):
        with pytest.raises(ValueError):
            dimodel.DiModel.from_counts([1, 2, 3, 4], pairs, np.full((4, 4), 0.25), np.full(4, 0.25), **bad)
    with pytest.raises(ValueError):
        dimodel.DiModel.from_counts([1, 2, 3], pairs, np.full((4, 4), 0.25), np.full(4, 0.25))
    with pytest.raises(ValueError):
        dimodel.DiModel.from_counts([1, 2, 3, 4], pairs, np.zeros((4, 4)), np.full(4, 0.25))


@pytest.mark.parametrize("flank", (0, 2))
def test_from_site_stack_reads_the_motifs_own_columns(flank):
    rng = np.random.default_rng(4 + flank)
    widths = np.array([3, 5], dtype=np.int64)
    C = 5 + 2 * flank
    counts = rng.integers(0, 40, (2, C, 6))
    dinuc = rng.integers(0, 40, (2, C, 16))
    stack = sitestack.SiteStack(counts, dinuc, np.array([9, 9]), widths, flank)
    cond, init = rng.dirichlet(np.full(4, 3.0), size=4), rng.dirichlet(np.full(4, 3.0))
    for i, W in enumerate(widths.tolist()):
        got = dimodel.DiModel.from_site_stack(stack, i, cond, init, 0.5)
        want = dimodel.DiModel.from_counts(counts[i, flank, :4], dinuc[i, flank:flank + W - 1], cond, init, 0.5)
        assert got.width == W and np.array_equal(got.start, want.start) and np.array_equal(got.trans, want.trans)
    with pytest.raises(ValueError, match="dinuc=True"):
        dimodel.DiModel.from_site_stack(sitestack.SiteStack(counts, None, np.array([9, 9]), widths, flank), 0, cond, init)


# ------------------------------------------------------------------------------------------------ the planted case, on the restatements

def planted_host():
    """The end-to-end flow of tests/test_gpu_dimodel.py on the restatements alone: (first-order RankSum, PWM RankSum, the model)."""
    inputs, controls, pwm = dc.planted_case()
    hits = dc.planted_hits_host(pwm, inputs)
    stack = sitestack.site_base_counts_host(*hits, [8], inputs, 0, dinuc=True)
    cond, init = kmers.kmer_counts_host(inputs, 2).markov(), kmers.kmer_counts_host(inputs, 1).markov()[0]
    model = dimodel.DiModel.from_site_stack(stack, 0, cond, init, 1.0)
    xa, xb = dimodel.best_sites_host([model], inputs, 3)[0], dimodel.best_sites_host([model], controls, 3)[0]
    deg = dimodel.DiModel.from_pwm(pwm)                    # the PWM's best scores (N-free regions: the degenerate model's)
    pa, pb = dimodel.best_sites_host([deg], inputs, 3)[0], dimodel.best_sites_host([deg], controls, 3)[0]
    return enrich.rank_sum_host(xa, xb), enrich.rank_sum_host(pa, pb), model, stack


def test_planted_case_margins_on_the_restatements():
    first, pwm_rs, model, stack = planted_host()
    assert stack.n_sites[0] >= 2 * 300                     # both strands of every palindromic true site
    auroc, auroc_pwm = float(first.auroc()[0]), float(pwm_rs.auroc()[0])
    print(f"planted case: first-order AUROC {auroc:.4f}, PWM AUROC {auroc_pwm:.4f}")
    assert auroc >= 0.9 and auroc_pwm <= 0.7
    assert (first.na, first.nb) == (300, 300)
    t = model.trans[3]                                     # column 4 given column 3: C -> G and G -> C are the sites', C -> C and G -> G the decoys'
    assert t[4 * 1 + 2] > 0 > t[4 * 1 + 1] and t[4 * 2 + 1] > 0 > t[4 * 2 + 2]


# ------------------------------------------------------------------------------------------------ the plan header under the sanitizers

@pytest.mark.skipif(shutil.which("g++") is None or shutil.which("make") is None, reason="needs g++ and make")
def test_plan_header_under_address_and_ub_sanitizers():
    asan = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    if not (os.path.isabs(asan) and os.path.exists(asan)):
        pytest.skip("the sanitizer runtimes are not installed on this box")
    subprocess.run(["make", "-s", "-C", CSRC, "dimodel_plan_asan"], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([BIN], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "dimodel_plan_asan: ok" in out.stdout, (out.stdout + out.stderr)[-4000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-4000:]
    assert int(out.stdout.split("(")[1].split()[0]) >= 100
