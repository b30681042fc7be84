"""
ms_scan_affinity and ms_affinity_rank_sum (ms_affinity.hip) on the GPU, against motifscan_amd.affinity: the numpy restatement for the
exact planes (n_terms, peak -- tests/test_affinity_host.py pins it to scoredist.window_raw_sums), the mpmath reference for `sum`, the
device's own planes for log_mean, ms_scan_best for peak / max_raw, and enrich.rank_sum_host (tests/test_ranksum_host.py) for the rank sums.
Every size at which the kernel changes path comes from ms_debug_affinity_dims.

The bound on `sum` is derived, not measured: after the shift every argument x of exp is <= 0; rounding the argument
moves exp(x) by at most |x| e^x 2^-52 <= 2^-52 / e; exp itself is within 1 ulp; n additions add at most n 2^-53 S; with S >= 1 that is
about 4 n 2^-53 S, and the factor 16 leaves room for the multiplications of a rescale or a fold:
    |S_dev - S_ref| <= 16 (n_terms + 8) 2^-53 S_ref.
The largest ratio of error to bound over all cases is printed by test_sum_is_within_the_derived_bound.

Each case is scanned once on the device, restated once on the host and summed once by mpmath; the tests share the three results.
"""
import ctypes
import math

import numpy as np
import pytest

from motifscan_amd import _lib, affinity, enrich, scanner

pytestmark = pytest.mark.gpu

PLANES = ("peak", "sum", "n_terms", "log_mean")


@pytest.fixture(scope="module", autouse=True)
def _device():
    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible")
    _lib.set_device(0)


def device_planes(mats, seqs, strand=3, scale=1.0, max_n=-1):
    pw, sq = _lib.PwmSet.from_matrices(mats), _lib.SeqSet.from_strings(list(seqs))
    try:
        res = _lib.scan_affinity(pw, sq, strand, scale, max_n)
        try:
            assert res.shape == (len(mats), len(seqs))
            return affinity.AffinityArrays(*res.cells())
        finally:
            res.close()
    finally:
        sq.close()
        pw.close()


def same_bytes(a, b):
    return all(getattr(a, k).tobytes() == getattr(b, k).tobytes() and getattr(a, k).shape == getattr(b, k).shape for k in PLANES)


def random_seq(rng, length, p_n=0.0):
    p = np.array([.3, .2, .2, .3]) * (1.0 - p_n)
    return "".join(rng.choice(list("ACGTN"), p=list(p) + [p_n], size=length)) if length else ""


def random_mat(rng, width):
    return np.round(rng.normal(0.0, 1.2, size=(4, width)), 3)


def make_cases(dims):
    """name -> (mats, seqs, strand, scale, max_n)"""
    seg, tile_w, tile_entries = dims["segment_windows"], dims["tile_max_width"], dims["tile_entries"]
    rng = np.random.default_rng(20240607)
    cases = {}

    # motif widths around a code word (32 columns) and two; region lengths around a motif, a segment and a strip
    widths = (1, 31, 32, 33, 64, 65)
    mats = [random_mat(rng, w) for w in widths]
    lengths = sorted({w + d for w in widths for d in (-1, 0, 1)} - {0})
    lengths += [seg + w + d for w in (1, 33) for d in (-2, -1, 0)]            # the last window of the first segment, and one segment against two
    lengths += [2 * seg + 40]                                                # three segments
    lanes = seg // dims["strips"]                                            # window starts per strip: one per lane
    lengths += [3 * lanes + 1, 4 * lanes - 1, 4 * lanes]                     # (W = 1) the last strip holds 1, 63 and 64 lanes with a window
    lengths += [4 * lanes + 33, 5 * lanes + 31]                              # (W = 33) 1 and 63 lanes in the fifth strip
    seqs = [random_seq(rng, n, 0.02 if i % 3 == 0 else 0.0) for i, n in enumerate(lengths)]
    seqs[5] = seqs[5].lower()
    cases["shapes"] = (mats, seqs, 3, 1.0, -1)
    few = [seqs[i] for i in (0, 7, len(seqs) - 9, len(seqs) - 6, len(seqs) - 1)]
    cases["plus"] = (mats, few, 1, 1.0, -1)
    cases["minus"] = (mats, few, 2, math.log(2.0), -1)

    # the widest motif of an LDS tile and one column more (its table in HBM), on a region just longer; a set whose tables overflow one
    # tile, so that a second tile starts; a narrow motif behind the wide ones (its own tile)
    cols = tile_entries // 4
    wide = [random_mat(rng, cols // 2 + 90), random_mat(rng, cols // 2 - 10), random_mat(rng, tile_w), random_mat(rng, tile_w + 1), random_mat(rng, 3)]
    wide = [m * (0.05 if m.shape[1] > 64 else 1.0) for m in wide]               # (raw sums of a thousand columns stay within a few units)
    cases["tiles"] = (wide, [random_seq(rng, tile_w + 6, 0.01), random_seq(rng, tile_w, 0.0), random_seq(rng, tile_w + 1, 0.0)], 3, 1.0, -1)
    cases["tiles_max_n"] = (wide, [random_seq(rng, tile_w + 6, 0.003)], 3, 1.0, 2)

    # max_n: -1, 0, the exact count of a window and one below it, on a narrow motif and on one wider than a code word with the N at column 40;
    # runs of N; an all-N region
    m5, m48 = random_mat(rng, 5), random_mat(rng, 48)
    base = random_seq(rng, 130)
    one_n = base[:70] + "N" + base[71:]                                      # windows of the 48-column motif at 30 hold it at column 40
    runs = base[:20] + "N" * 3 + base[23:60] + "NN" + base[62:100] + "N" * 7 + base[107:]
    nseqs = [one_n, runs, "N" * 60, base, random_seq(rng, seg + 70, 0.05)]
    for max_n in (-1, 0, 1, 2, 3):                                           # 5-column windows of `runs` hold 0 .. 5 N: every value here is a count and one below the next
        cases[f"max_n_{max_n}"] = ([m5, m48], nseqs, 3, 1.0, max_n)

    # -inf entries: (a) some terms -inf, (b) every term -inf -- also in a region of two segments, so that a -inf partial is folded; a row
    # with a NaN entry and one with +inf beside scorable rows; the all-negative matrix
    some = random_mat(rng, 6)
    some[0, 2] = -np.inf
    every = random_mat(rng, 4)
    every[:, 1] = -np.inf
    half = random_mat(rng, 3)
    half[0, 0] = -np.inf                                                     # '+' windows that start with A, '-' windows that end with T
    nan_row, inf_row = random_mat(rng, 7), random_mat(rng, 2)
    nan_row[3, 6] = np.nan
    inf_row[1, 0] = np.inf
    neg = -np.abs(random_mat(rng, 9)) - 0.01
    iseqs = [random_seq(rng, 90), random_seq(rng, seg + 50), "A" * (seg + 30), "A" * 20 + random_seq(rng, seg + 5), random_seq(rng, 3), ""]
    cases["minus_inf"] = ([some, every, nan_row, half, inf_row, neg], iseqs, 3, 1.0, -1)
    cases["minus_inf_plus"] = ([some, every, half], iseqs, 1, 0.5, -1)

    # scores that rise along the region: a two-column matrix whose first column dominates (v = 4 b0 + b1, in units of 0.37) over blocks of
    # one strip of bases of one repeated dinucleotide whose two readings both rise block by block -- a lane meets a new peak at every strip --
    # and whole segments of one letter that rise segment by segment, so that the fold rescales at every partial; the same falling
    dom = 0.37 * np.array([[0.0, 0.0], [4.0, 1.0], [8.0, 2.0], [12.0, 3.0]])
    blocks = ["AA", "AC", "CC", "CG", "GG", "GT", "TT", "TT"]
    rising = "".join(b * (lanes // 2) for b in blocks)
    stairs = "A" * seg + "C" * seg + "G" * seg + "T" * 40
    cases["rising"] = ([dom, random_mat(rng, 8)], [rising, rising[::-1], stairs, stairs[::-1], rising + stairs], 1, 1.0, -1)
    cases["rising_both"] = ([dom], [rising, stairs[::-1]], 3, 2.5, -1)

    # a scale at which most terms underflow to 0
    cases["steep"] = ([random_mat(rng, 12), random_mat(rng, 20)], [random_seq(rng, 300), random_seq(rng, seg + 100)], 3, 400.0, -1)
    return cases


class World:
    def __init__(self):
        self.dims = _lib.affinity_dims()
        self.cases = make_cases(self.dims)
        self._dev, self._host, self._ref = {}, {}, {}

    def dev(self, name):
        if name not in self._dev:
            self._dev[name] = device_planes(*self.cases[name])
        return self._dev[name]

    def host(self, name):
        if name not in self._host:
            self._host[name] = affinity.affinity_host(*self.cases[name])
        return self._host[name]

    def ref(self, name):
        if name not in self._ref:
            self._ref[name] = affinity.affinity_reference(*self.cases[name], as_mpf=True)
        return self._ref[name]


@pytest.fixture(scope="module")
def world():
    return World()


CASE_NAMES = ("shapes", "plus", "minus", "tiles", "tiles_max_n", "max_n_-1", "max_n_0", "max_n_1", "max_n_2", "max_n_3", "minus_inf",
              "minus_inf_plus", "rising", "rising_both", "steep")


def test_the_cases_cover_what_they_claim(world):
    assert set(world.cases) == set(CASE_NAMES)
    seg = world.dims["segment_windows"]
    h = world.host("max_n_-1")
    assert h.n_terms[1, 0] > 0 and world.host("max_n_0").n_terms[1, 0] == h.n_terms[1, 0] - 2 * 48      # one N: 48 windows of the wide motif hold it
    runs = [world.host(f"max_n_{k}").n_terms[0, 1] for k in (-1, 0, 1, 2, 3)]
    assert runs[1] < runs[2] < runs[3] < runs[4] < runs[0]                      # (5 columns over runs of 2, 3 and 7 N: windows hold 0 .. 5 of them)
    h = world.host("minus_inf")
    assert np.isneginf(h.peak[1]).sum() >= 4 and np.isneginf(h.peak[0]).sum() == 0 and (h.n_terms[2] == 0).all() and (h.n_terms[4] == 0).all()
    assert (h.n_terms[5, :4] > 0).all() and (h.peak[5, :4] < 0).all()            # the all-negative matrix is scored
    steep = world.host("steep")
    assert (steep.sum < 10.0).all() and (steep.n_terms > 500).all()              # nearly every term underflows
    lens = [len(s) for s in world.cases["shapes"][1]]
    assert max(lens) > 2 * seg and sum(seg < n <= 2 * seg for n in lens) >= 3


@pytest.mark.parametrize("name", CASE_NAMES)
def test_n_terms_and_peak_are_exact(world, name):
    dev, host = world.dev(name), world.host(name)
    assert dev.n_terms.dtype == np.int32 and np.array_equal(dev.n_terms, host.n_terms)
    both = ~np.isnan(host.peak)
    assert np.array_equal(np.isnan(dev.peak), ~both)
    assert dev.peak[both].tobytes() == host.peak[both].tobytes()                # bit for bit (a NaN's payload is not part of the contract)


@pytest.mark.parametrize("name", ("shapes", "plus", "minus", "tiles", "minus_inf", "rising"))
def test_peak_over_max_raw_is_the_best_site_score(world, name):
    """max_n = -1: the greatest raw sum over max_raw is ms_scan_best's score, bit for bit, wherever that scan scores the motif."""
    mats, seqs, strand, _, max_n = world.cases[name]
    assert max_n == -1
    pw, sq = _lib.PwmSet.from_matrices(mats), _lib.SeqSet.from_strings(list(seqs))
    try:
        max_raw = pw.max_raw()
        best = _lib.scan_best(pw, sq, strand)
        try:
            score = best.sites()[0]
        finally:
            best.close()
    finally:
        sq.close()
        pw.close()
    dev, checked = world.dev(name), 0
    for m, mat in enumerate(mats):
        if not (np.isfinite(max_raw[m]) and max_raw[m] > 0 and not affinity.empty_row(mat)):
            assert np.isnan(score[m]).all()
            continue
        with np.errstate(all="ignore"):
            want = dev.peak[m] / max_raw[m]
        want = np.where(np.isneginf(dev.peak[m]), np.nan, want)                 # a cell of -inf windows only has no winner there
        assert np.array_equal(np.isnan(score[m]), np.isnan(want))
        ok = ~np.isnan(want)
        assert score[m][ok].tobytes() == want[ok].tobytes()
        checked += int(ok.sum())
    assert checked > 0


def test_sum_is_within_the_derived_bound(world):
    worst, where, cells = 0.0, None, 0
    for name in CASE_NAMES:
        dev, ref = world.dev(name), world.ref(name)
        P, R = dev.sum.shape
        for m in range(P):
            for r in range(R):
                s_ref, n = ref.sum[m, r], int(dev.n_terms[m, r])
                if s_ref == 0:
                    assert dev.sum[m, r] == 0.0 and (n == 0 or np.isneginf(dev.peak[m, r])), (name, m, r)
                    continue
                err = abs(float(dev.sum[m, r]) - s_ref)
                limit = 16.0 * (n + 8.0) * 2.0 ** -53 * s_ref
                ratio = float(err / limit)
                print(f"{name}[{m}, {r}]: n_terms {n}, S {float(s_ref):.17g}, error / bound {ratio:.5f}")
                if ratio > worst:
                    worst, where = ratio, (name, m, r)
                cells += 1
                assert err <= limit, (name, m, r, float(err), float(limit))
                assert 1.0 - 2.0 ** -40 <= dev.sum[m, r] <= n * (1.0 + 2.0 ** -40)
    print(f"sum: {cells} cells, largest error / bound = {worst:.5f} at {where}")
    assert cells > 200


@pytest.mark.parametrize("name", CASE_NAMES)
def test_log_mean_follows_from_the_device_s_own_planes(world, name):
    dev, scale = world.dev(name), world.cases[name][3]
    none, dead = dev.n_terms == 0, np.isneginf(dev.peak)
    assert np.isnan(dev.log_mean[none]).all() and np.isnan(dev.peak[none]).all() and (dev.sum[none] == 0.0).all()
    assert np.isneginf(dev.log_mean[dead]).all() and (dev.sum[dead] == 0.0).all()
    live = ~none & ~dead
    assert np.isfinite(dev.log_mean[live]).all()
    a = scale * dev.peak[live]
    b = np.log(dev.sum[live] / dev.n_terms[live])
    tol = 8.0 * 2.0 ** -53 * (np.abs(a) + np.abs(b) + 1.0)                     # one ulp each for the divide, the log, the multiply and the add
    assert (np.abs(dev.log_mean[live] - (a + b)) <= tol).all()
    arr = affinity.AffinityArrays(dev.peak, dev.sum, dev.n_terms, dev.log_mean)
    assert np.allclose(arr.log_sum()[live], dev.log_mean[live] + np.log(dev.n_terms[live]), rtol=0, atol=1e-12)


def test_empty_sets_give_empty_results(world):
    mats = world.cases["max_n_0"][0]
    none = device_planes(mats, [], 3)
    assert all(getattr(none, k).shape == (2, 0) for k in PLANES)
    nothing = device_planes([], ["ACGT", "AC"], 3)
    assert all(getattr(nothing, k).shape == (0, 2) for k in PLANES)
    short = device_planes(mats, ["", "AC"], 3)
    assert (short.n_terms == 0).all() and np.isnan(short.peak).all() and (short.sum == 0).all() and np.isnan(short.log_mean).all()


def test_two_runs_give_the_same_bytes_and_cells_do_not_depend_on_their_neighbours(world):
    for name in ("shapes", "minus_inf", "rising", "tiles"):
        assert same_bytes(world.dev(name), device_planes(*world.cases[name])), name
    mats, seqs, strand, scale, max_n = world.cases["shapes"]
    dev = world.dev("shapes")
    seg, lens = world.dims["segment_windows"], [len(x) for x in seqs]
    for r in (3, lens.index(seg + 33), lens.index(2 * seg + 40), len(seqs) - 1):  # a short region, one of two segments, of three, the last
        alone = device_planes(mats, [seqs[r]], strand, scale, max_n)
        assert all(getattr(alone, k)[:, 0].tobytes() == np.ascontiguousarray(getattr(dev, k)[:, r]).tobytes() for k in PLANES), r
    for m in (0, 3, 5):
        alone = device_planes([mats[m]], seqs, strand, scale, max_n)
        assert all(getattr(alone, k)[0].tobytes() == getattr(dev, k)[m].tobytes() for k in PLANES), m
    mats, seqs, strand, scale, max_n = world.cases["tiles"]                       # a motif in the second LDS tile, and the one read from HBM
    dev = world.dev("tiles")
    for m in (1, 3):
        alone = device_planes([mats[m]], seqs, strand, scale, max_n)
        assert all(getattr(alone, k)[0].tobytes() == getattr(dev, k)[m].tobytes() for k in PLANES), m


# ------------------------------------------------------------------------------------------------------------ rank sums --

def rank_world():
    rng = np.random.default_rng(77)
    ints = [rng.integers(-2, 3, size=(4, w)).astype(np.float64) for w in (1, 4, 9)]      # small integer PWMs: ties are the rule
    nan_row = random_mat(rng, 5)
    nan_row[0, 0] = np.nan                                                      # an all-NaN row
    holes = rng.integers(-2, 3, size=(4, 3)).astype(np.float64)
    holes[:, 1] = -np.inf                                                       # every window of a region without N is -inf: cells of -inf
    mats = ints + [nan_row, holes]
    letters = np.frombuffer(b"AACCAGTN", dtype=np.uint8)

    def regions(n, seed):
        r = np.random.default_rng(seed)
        return [letters[r.integers(0, len(letters), int(r.integers(0, 30)))].tobytes().decode() for _ in range(n)]
    return mats, regions(150, 5), regions(97, 6)


def test_rank_sum_equals_the_integer_restatement_on_the_log_mean_planes():
    mats, seqs_a, seqs_b = rank_world()
    pw = _lib.PwmSet.from_matrices(mats)
    sa, sb = _lib.SeqSet.from_strings(seqs_a), _lib.SeqSet.from_strings(seqs_b)
    a, b = _lib.scan_affinity(pw, sa, 3), _lib.scan_affinity(pw, sb, 3)
    try:
        la, lb = a.log_mean, b.log_mean
        assert np.isnan(la[3]).all() and np.isneginf(la[4]).any() and np.isnan(la[2]).any() and np.isfinite(la[2]).any()
        rng = np.random.default_rng(8)
        sel_a, sel_b = rng.integers(0, 2, len(seqs_a)).astype(np.uint8), rng.integers(0, 3, len(seqs_b)).astype(np.uint8)
        none = np.zeros(len(seqs_a), dtype=np.uint8)
        for other, lo, s1, s2 in ((b, lb, None, None), (b, lb, sel_a, sel_b), (a, la, None, None), (a, la, sel_a, 1 - sel_a), (b, lb, none, None),
                                  (b, lb, sel_a, np.zeros(len(seqs_b), dtype=np.uint8))):
            xa = la if s1 is None else la[:, s1 != 0]
            xb = lo if s2 is None else lo[:, s2 != 0]
            want = enrich.rank_sum_host(xa, xb)
            u2, ties, na, nb = a.rank_sum(other, s1, s2)
            assert (na, nb) == (want.na, want.nb) == (xa.shape[1], xb.shape[1])
            assert np.array_equal(u2, want.u2) and ties == want.ties
        u2, ties, na, nb = a.rank_sum(b, None, None, 1, 4)                       # a motif range
        want = enrich.rank_sum_host(la[1:4], lb[1:4])
        assert np.array_equal(u2, want.u2) and ties == want.ties
        u2, ties, na, nb = a.rank_sum(b, none, None)
        assert na == 0 and (u2 == 0).all()
        n_all = len(seqs_a) + len(seqs_b)
        u2, ties, na, nb = a.rank_sum(b, None, None, 3, 4)                       # the all-NaN row: everything ties
        assert u2.tolist() == [na * nb] and ties == [n_all ** 3 - n_all]
        timing = {}
        a.rank_sum(b, timing=timing)
        assert timing["device_ms"] > 0
    finally:
        a.close()
        b.close()
        sa.close()
        sb.close()
        pw.close()


class _Genome:
    def __init__(self, chroms):
        self.chroms = chroms
        self.chrom_sizes = {k: len(v) for k, v in chroms.items()}

    def fetch_sequence(self, chrom, start, end):
        return self.chroms[chrom][start:end]


class _Region:
    def __init__(self, chrom, start, end):
        self.chrom, self.start, self.end, self.summit = chrom, start, end, (start + end) // 2


class _Pwm:
    def __init__(self, mat):
        self.matrix, self.length, self.cutoffs = mat, mat.shape[1], None


def planted_world():
    """60 input and 60 control regions of 150 bp of one background; a WEAK form of the motif's consensus (two of its eight columns
    replaced) is planted three times in every input region and nowhere in the controls."""
    rng = np.random.default_rng(99)
    consensus = "TGACGTCA"
    code = {c: i for i, c in enumerate("ACGT")}
    mat = np.full((4, 8), -1.2)
    for c, ch in enumerate(consensus):
        mat[code[ch], c] = 1.1
    n, length = 60, 150
    inputs, controls = [], []
    for i in range(n):
        s = list(random_seq(rng, length))
        for k in range(3):
            weak = list(consensus)
            for c in rng.choice(8, size=2, replace=False):
                weak[c] = "ACGT"[(code[weak[c]] + 1 + int(rng.integers(0, 3))) % 4]
            at = 10 + 45 * k + int(rng.integers(0, 30))
            s[at:at + 8] = weak
        inputs.append("".join(s))
        controls.append(random_seq(rng, length))
    genome = _Genome({"in": "".join(inputs), "ctl": "".join(controls)})
    reg_in = [_Region("in", i * length, (i + 1) * length) for i in range(n)]
    reg_ctl = [_Region("ctl", i * length, (i + 1) * length) for i in range(n)]
    return mat, genome, reg_in, reg_ctl, inputs, controls


def test_scanner_affinity_rank_sum_end_to_end_on_a_planted_case():
    mat, genome, reg_in, reg_ctl, inputs, controls = planted_world()
    sc, ctl = scanner.Scanner(genome, reg_in, strand="both"), scanner.Scanner(genome, reg_ctl, strand="both")
    try:
        arr = sc.affinity([_Pwm(mat)])
        host = affinity.affinity_host([mat], inputs, 3)
        assert isinstance(arr, affinity.AffinityArrays) and np.array_equal(arr.n_terms, host.n_terms) and arr.peak.tobytes() == host.peak.tobytes()
        rs = sc.affinity_rank_sum([_Pwm(mat)], ctl)
        want = enrich.rank_sum_host(arr.log_mean, ctl.affinity([_Pwm(mat)]).log_mean)
        assert isinstance(rs, enrich.RankSum) and np.array_equal(rs.u2, want.u2) and rs.ties == want.ties and (rs.na, rs.nb) == (60, 60)
        best = sc.rank_sum([_Pwm(mat)], ctl)
        print(f"planted case: AUROC by affinity {rs.auroc()[0]:.4f} (z {rs.z()[0]:.2f}), by best site {best.auroc()[0]:.4f} (z {best.z()[0]:.2f})")
        assert rs.auroc()[0] > 0.5
        sel = np.arange(60) % 2
        half = sc.affinity_rank_sum([_Pwm(mat)], ctl, sel=sel, sel_control=1 - sel, scale=0.5, max_n=0)
        assert (half.na, half.nb) == (30, 30)
        plus = scanner.Scanner(genome, reg_in, strand="+")
        try:
            assert np.array_equal(plus.affinity([_Pwm(mat)]).n_terms, affinity.affinity_host([mat], inputs, 1).n_terms)
        finally:
            plus.close()
    finally:
        sc.close()
        ctl.close()


# --------------------------------------------------------------------------------------------------------------- errors --

def test_every_invalid_argument_is_a_value_error():
    L = _lib.lib()
    pw, sq = _lib.PwmSet.from_matrices([np.ones((4, 3))]), _lib.SeqSet.from_strings(["ACGTACGT"])
    h = ctypes.c_void_p()

    def call(pwh, sqh, mask, scale, max_n, flags):
        rc = L.ms_scan_affinity(pwh, sqh, mask, scale, max_n, flags, ctypes.byref(h))
        assert not h.value or rc == _lib.MS_OK
        return rc
    try:
        bad = [(None, sq.h, 3, 1.0, -1, 0), (pw.h, None, 3, 1.0, -1, 0), (pw.h, sq.h, 0, 1.0, -1, 0), (pw.h, sq.h, 4, 1.0, -1, 0), (pw.h, sq.h, 3, 1.0, -1, 1),
               (pw.h, sq.h, 3, 0.0, -1, 0), (pw.h, sq.h, 3, -1.0, -1, 0), (pw.h, sq.h, 3, math.inf, -1, 0), (pw.h, sq.h, 3, math.nan, -1, 0), (pw.h, sq.h, 3, 1.0, -2, 0)]
        for args in bad:
            rc = call(*args)
            assert rc == _lib.MS_ERR_INVALID, args
            with pytest.raises(ValueError):
                _lib.check(rc)
        assert L.ms_scan_affinity(pw.h, sq.h, 3, 1.0, -1, 0, None) == _lib.MS_ERR_INVALID
        res = _lib.scan_affinity(pw, sq, 3)
        try:
            with pytest.raises(ValueError, match="motif range"):
                res.cells(0, 2)
            with pytest.raises(ValueError):
                _lib.check(L.ms_affinity_cells(res.h, 1, 0, None, None, None, None))
            with pytest.raises(ValueError):
                _lib.check(L.ms_affinity_shape(None, None, None))
            with pytest.raises(ValueError, match="one flag per region"):
                res.rank_sum(res, sel=[1, 0])
            with pytest.raises(ValueError, match="motif range"):
                res.rank_sum(res, m0=0, m1=2)
            two = _lib.PwmSet.from_matrices([np.ones((4, 3)), np.ones((4, 2))])
            other = _lib.scan_affinity(two, sq, 3)
            try:
                with pytest.raises(ValueError, match="affinity results disagree"):
                    res.rank_sum(other)
            finally:
                other.close()
                two.close()
            u2, ties, n = np.zeros(1, dtype=np.int64), np.zeros(2, dtype=np.uint64), np.zeros(2, dtype=np.int64)
            for a, b, flags in ((None, res.h, 0), (res.h, None, 0), (res.h, res.h, 1)):
                rc = L.ms_affinity_rank_sum(a, None, b, None, 0, 1, flags, _lib.ptr(u2, ctypes.c_int64), _lib.ptr(ties, ctypes.c_uint64), _lib.ptr(n, ctypes.c_int64), None)
                assert rc == _lib.MS_ERR_INVALID
            assert res.device_ms() > 0 and all(res.device_pointers())
        finally:
            res.close()
    finally:
        sq.close()
        pw.close()
