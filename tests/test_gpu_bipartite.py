"""
ms_scan_best_bipartite (ms_bipartite.hip) on the GPU: the best placement of every (bipartite spec, region) cell, all four planes -- score,
pos, strand and the winner's gap -- compared byte for byte with `bipartite.best_bipartite_host` (which tests/test_bipartite_host.py pins
to a scalar loop) at the smallest shapes that can go wrong: element widths 1 to 3, around the 32-base word edge and at the cap, gaps
0..0, one value and 0..G, regions in which only some gaps fit, regions around 64 placement starts and around a segment, sites across a
segment edge, ties between strands, gaps and positions, -inf entries, non-ACGT bases, unscorable specs first, between and last, tiles
that fill and split; tied to ms_scan_best through an all-zero partner, followed downstream into the rank sums, and run end to end on the
planted case.  The cases are tests/bipartite_cases.py's, sized by ms_debug_bipartite_dims.

One spec can never fill a tile alone (two cap-wide elements take a quarter of it), so "a tile one spec fills" is exercised as a tile
filled to its last entry by four such specs.  One of the MS_ERR_INVALID cases is not exercised, as in tests/test_gpu_best.py and for its
reason: a region of 2^31 bases or more needs 2 GiB of host bytes for one comparison of two integers (dense_regions_fit, shared with
ms_scan_best).
"""
import ctypes

import numpy as np
import pytest

import bipartite_cases as bc
from dimodel_cases import random_dna, random_pwm
from motifscan_amd import _lib, bipartite, enrich, scanner
from motifscan_amd.bipartite import Bipartite

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _device():
    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible")
    _lib.set_device(0)


def run(mats, specs, seqs, mask=3, pw=None, sq=None):
    own_pw, own_sq = pw is None, sq is None
    if own_pw:
        pw = _lib.PwmSet.from_matrices(mats)
    if own_sq:
        sq = _lib.SeqSet.from_strings(seqs)
    try:
        res = _lib.scan_best_bipartite(pw, specs, sq, mask)
        try:
            assert res.shape == (len(specs), len(seqs))
            return res.sites() + (res.gaps(),)
        finally:
            res.close()
    finally:
        if own_sq:
            sq.close()
        if own_pw:
            pw.close()


def same_bytes(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------ 1. the smallest shapes

@pytest.fixture(scope="module")
def world():
    d = _lib.bipartite_dims()
    mats = bc.matrices(d["max_width"])
    specs = bc.world_specs(d["max_gap"])
    seqs = bc.short_regions(mats, specs) + bc.long_regions(mats, specs, d["seg_windows"])
    return {"mats": mats, "specs": specs, "seqs": seqs, "dims": d, "want": {}}


def want_of(world, mask):
    if mask not in world["want"]:
        world["want"][mask] = bipartite.best_bipartite_host(world["mats"], world["specs"], world["seqs"], mask)
    return world["want"][mask]


@pytest.mark.parametrize("mask", (1, 2, 3))
def test_smallest_shapes_equal_the_restatement_byte_for_byte(world, mask):
    want = want_of(world, mask)
    got = run(world["mats"], world["specs"], world["seqs"], mask)
    bc.same_planes(got, want)
    score, pos, strand, gap = got
    specs, mats, seg = world["specs"], world["mats"], world["dims"]["seg_windows"]
    unscorable = [k for k, sp in enumerate(specs) if not bipartite.scorable_host(mats, sp)]
    assert unscorable == [0, 9, 13, len(specs) - 1] and np.isnan(score[unscorable]).all() and (gap[unscorable] == -1).all()
    ok = [k for k in range(len(specs)) if k not in unscorable]
    assert np.isfinite(score[ok]).sum() > 800 and np.isnan(score[ok]).sum() > 100          # (the cases hold what they are meant to hold)
    if mask == 3:
        assert (strand == 1).any() and (strand == 2).any()
    assert pos[ok].max() > 2 * seg and len(set(gap[ok].ravel().tolist())) > 20              # a winner in the third segment; many gaps win
    # the widths at the cap and a gap range of 0 .. G: only some gaps fit the regions between S(g_min) and S(g_max)
    k = 10
    assert specs[k] == Bipartite(bc.M["w1"], bc.M["cap"], 0, 0, world["dims"]["max_gap"])
    by_len = {len(s): r for r, s in enumerate(world["seqs"])}
    s_min, s_max = bc.span(mats, specs[k], 0), bc.span(mats, specs[k], specs[k].gap_max)
    assert np.isnan(score[k, by_len[s_min - 1]]) and (pos[k, by_len[s_min]], gap[k, by_len[s_min]]) == (0, 0)
    assert gap[k, by_len[s_max - 1]] < specs[k].gap_max and pos[k, by_len[s_max]] >= 0
    # the sites across a segment edge: the HALF x{3} HALF spec finds each where it was put
    k = 21
    n_short = len(bc.short_regions(mats, specs))
    at = {n_short + 9: seg - 1, n_short + 10: seg - 12, n_short + 11: seg - 15, n_short + 12: 100, n_short + 13: seg + 107, n_short + 14: 2 * seg + 114}
    if mask & 1:
        for r, p in at.items():
            assert (pos[k, r], strand[k, r], gap[k, r], score[k, r]) == (p, 1, 3, 1.0), r


def test_the_width_and_gap_caps_are_statuses(world):
    d = world["dims"]
    mats = [random_pwm(d["max_width"] + 1, 1), random_pwm(3, 2)]
    pw, sq = _lib.PwmSet.from_matrices(mats), _lib.SeqSet.from_strings(["ACGT" * 60])
    try:
        for spec, text in ((Bipartite(0, 1, 0, 0, 1), "more than %d columns" % d["max_width"]), (Bipartite(1, 0, 0, 0, 1), "more than %d columns" % d["max_width"]),
                           (Bipartite(1, 1, 0, 0, d["max_gap"] + 1), "gap_max <= %d" % d["max_gap"])):
            with pytest.raises(ValueError, match=text):
                _lib.scan_best_bipartite(pw, [Bipartite(1, 1, 0, 0, 0), spec], sq)
        res = _lib.scan_best_bipartite(pw, [Bipartite(1, 1, 1, d["max_gap"], d["max_gap"])], sq)          # the caps themselves are fine
        assert res.gaps()[0, 0] == d["max_gap"]
        res.close()
    finally:
        sq.close()
        pw.close()


# ------------------------------------------------------------------------------------------------ 2. tiles

def test_tiles_that_fill_and_split(world):
    """Nine specs of two cap-wide elements: four fill a tile to its last entry, the ninth shares the third tile with a narrow spec; the
    element order repeats throughout."""
    d = world["dims"]
    per_spec = 4 * 2 * d["max_width"]
    assert d["tile_entries"] % per_spec == 0 and 9 * per_spec > 2 * d["tile_entries"]
    specs = bc.tile_specs(bc.M["cap"], bc.M["w1"], 9)
    rng = np.random.default_rng(8)
    seqs = [random_dna(rng, n) for n in (2 * d["max_width"] + 1, 200, d["seg_windows"] + 70)]
    got = run(world["mats"], specs, seqs)
    bc.same_planes(got, bipartite.best_bipartite_host(world["mats"], specs, seqs, 3))
    assert np.isfinite(got[0]).sum() >= 2 * len(specs)


# ------------------------------------------------------------------------------------------------ 3. flips, masks, ties

@pytest.mark.parametrize("mask", (1, 2, 3))
def test_ties_keep_the_earliest_placement(world, mask):
    m, mats = bc.M, world["mats"]
    specs = [Bipartite(m["const"], m["const"], 0, 2, 5), Bipartite(m["const"], m["const"], 1, 2, 5), Bipartite(m["half"], m["ca"], 0, 0, 6),
             Bipartite(m["half"], m["half"], 0, 1, 5), Bipartite(m["w3"], m["w3"], 1, 0, 4), Bipartite(m["w3"], m["w3"], 0, 0, 4)]
    seqs = bc.tie_regions() + ["A" * (world["dims"]["seg_windows"] + 200)] + [random_dna(np.random.default_rng(k), 50 + 200 * k) for k in range(4)]
    got = run(mats, specs, seqs, mask)
    bc.same_planes(got, bipartite.best_bipartite_host(mats, specs, seqs, mask))
    score, pos, strand, gap = got
    first = 1 if mask & 1 else 2
    for r in (0, 3):                                       # a homopolymer (one of more than a segment): every placement ties
        for k in (0, 1):
            assert (pos[k, r], strand[k, r], gap[k, r], score[k, r]) == (0, first, 2, 1.0)
    if mask & 1:
        assert (pos[2, 1], strand[2, 1], gap[2, 1]) == (4, 1, 2)          # between two gaps only: the smaller
        assert (pos[3, 2], strand[3, 2], gap[3, 2]) == (3, 1, 3)          # between two positions only: the earlier
    assert (strand[4] == first).all()                      # a == b with flip 1: '+' and '-' coincide, '+' comes first
    if mask == 3:
        assert (strand[5] == 2).any()


def test_minus_inf_entries_never_win_and_may_be_all_there_is(world):
    m, mats = bc.M, world["mats"]
    specs = [Bipartite(m["holes"], m["w1"], 0, 0, 4), Bipartite(m["w2"], m["holes"], 1, 0, 3)]
    seqs = ["A" * 30, "A" * 12 + "C" + "A" * 17, "A" * 700, "A" * 600 + "C" + "A" * 99]
    got = run(mats, specs, seqs, 1)
    bc.same_planes(got, bipartite.best_bipartite_host(mats, specs, seqs, 1))
    assert np.isnan(got[0][0, [0, 2]]).all() and (got[1][0, 1], got[1][0, 3]) == (12, 600)


# ------------------------------------------------------------------------------------------------ 4. the tie to ms_scan_best

def test_an_all_zero_partner_gives_ms_scan_bests_planes(world):
    """flip 0, g = 0, a one-column all-zero partner.  Mask 1: raw = F_a(p) + 0.0 for p <= L - W_a - 1 -- ms_scan_best's '+' walk of the
    regions cut one base short, the same pos.  Mask 2: raw = 0.0 + R_a(p + 1) -- its '-' walk of the regions cut at the front, whose
    positions are one less than in the whole region: the bipartite pos again."""
    rng = np.random.default_rng(77)
    widths = [1, 2, 3, 8, 12, 31, 32, 33, 34, 63, 64]
    mats = [random_pwm(w, 600 + i) for i, w in enumerate(widths)] + [np.zeros((4, 1))]
    zero = len(widths)
    specs = [Bipartite(i, zero, 0, 0, 0) for i in range(len(widths))]
    seqs = [random_dna(rng, n) for n in (1, 8, 34, 65, 66, 130, 513, 514, 1100)] + [bc.with_n(random_dna(rng, 90), 31, 32, 70)]
    for mask, cut in ((1, [s[:-1] for s in seqs]), (2, [s[1:] for s in seqs])):
        score, pos, strand, gap = run(mats, specs, seqs, mask)
        pw, sq = _lib.PwmSet.from_matrices(mats[:zero]), _lib.SeqSet.from_strings(cut)
        try:
            res = _lib.scan_best(pw, sq, mask)
            ws, wp, wd = res.sites()
            res.close()
        finally:
            sq.close()
            pw.close()
        assert score.tobytes() == ws.tobytes() and np.array_equal(pos, wp) and np.array_equal(strand, wd)
        assert np.array_equal(gap, np.where(wp >= 0, 0, -1)) and np.isfinite(score).sum() > 60


# ------------------------------------------------------------------------------------------------ 5. downstream: the handles are ordinary ms_best

def test_rank_sum_and_count_passing_take_the_handles_and_gaps_belong_to_this_scan(world):
    rng = np.random.default_rng(13)
    mats, specs = world["mats"], world["specs"][:14]
    a = [random_dna(rng, int(n)) for n in rng.integers(1, 160, 130)]
    b = [random_dna(rng, int(n)) for n in rng.integers(1, 160, 77)]
    pw, sa, sb = _lib.PwmSet.from_matrices(mats[:-1]), _lib.SeqSet.from_strings(a), _lib.SeqSet.from_strings(b)
    specs = [sp for sp in specs if bc.M["pinf"] not in (sp.a, sp.b)]
    try:
        ha, hb = _lib.scan_best_bipartite(pw, specs, sa, 3), _lib.scan_best_bipartite(pw, specs, sb, 3)
        try:
            xa, xb = bipartite.best_bipartite_host(mats, specs, a, 3)[0], bipartite.best_bipartite_host(mats, specs, b, 3)[0]
            u2, ties, na, nb = ha.rank_sum(hb)
            want = enrich.rank_sum_host(xa, xb)
            assert np.array_equal(u2, want.u2) and [int(t) for t in ties] == want.ties and (na, nb) == (130, 77)
            sel = rng.random(130) < 0.5
            u2, ties, na, nb = ha.rank_sum(hb, sel)
            want = enrich.rank_sum_host(xa[:, sel], xb)
            assert np.array_equal(u2, want.u2) and [int(t) for t in ties] == want.ties and (na, nb) == (int(sel.sum()), 77)
            cut = np.tile([0.2, 0.5, 0.8, 1.0], (len(specs), 1))
            assert np.array_equal(ha.count_passing(cut), enrich.count_passing_host(xa, cut))
            assert all(ha.device_pointers()) and ha.gaps_device_pointer() and ha.device_ms() > 0
            assert np.array_equal(ha.gaps(2, 5), ha.gaps()[2:5])
            with pytest.raises(ValueError, match="motif range"):
                ha.gaps(0, len(specs) + 1)
        finally:
            ha.close()
            hb.close()
        plain = _lib.scan_best(pw, sa, 3)                  # a handle of another scan holds no gaps
        try:
            g = np.zeros(4, dtype=np.int16)
            p = ctypes.c_void_p()
            assert _lib.lib().ms_best_gaps(plain.h, 0, 1, _lib.ptr(g, ctypes.c_int16)) == _lib.MS_ERR_INVALID
            assert _lib.lib().ms_best_gaps_device(plain.h, ctypes.byref(p)) == _lib.MS_ERR_INVALID and not p.value
            with pytest.raises(ValueError, match="no gap plane"):
                plain.gaps()
        finally:
            plain.close()
        assert _lib.lib().ms_best_gaps(None, 0, 0, None) == _lib.MS_ERR_INVALID and _lib.lib().ms_best_gaps_device(None, None) == _lib.MS_ERR_INVALID
    finally:
        sa.close()
        sb.close()
        pw.close()


# ------------------------------------------------------------------------------------------------ 6. end to end on the planted case

def test_planted_case_end_to_end():
    inputs, controls, mats = bc.planted_case()
    chroms = {"in": "".join(inputs), "ctl": "".join(controls)}

    class Genome:
        chrom_sizes = {k: len(v) for k, v in chroms.items()}

        def fetch_sequence(self, chrom, start, end):
            return chroms[chrom][start:end]

    class Region:
        def __init__(self, chrom, start, end):
            self.chrom, self.start, self.end, self.summit = chrom, start, end, (start + end) // 2

    class Pwm:
        matrix = mats[0]
    specs = [bc.PLANTED_SPEC, bc.PLANTED_FIXED]
    sc = scanner.Scanner(Genome(), [Region("in", 100 * i, 100 * i + 100) for i in range(200)])
    ctl = scanner.Scanner(Genome(), [Region("ctl", 100 * i, 100 * i + 100) for i in range(200)])
    try:
        assert list(sc.sequences) == inputs and list(ctl.sequences) == controls
        want_in, want_ctl = bipartite.best_bipartite_host(mats, specs, inputs, 3), bipartite.best_bipartite_host(mats, specs, controls, 3)
        best = sc.best_sites_bipartite([Pwm], specs)
        assert isinstance(best, bipartite.BipartiteSites) and best.score.shape == (2, 200)
        assert best.score.tobytes() == want_in[0].tobytes() and np.array_equal(best.strand, want_in[2]) and np.array_equal(best.gap, want_in[3])
        assert np.array_equal(best.start, want_in[1] + 100 * np.arange(200))
        assert set(best.gap[0].tolist()) == {1, 2, 4, 5}    # every planted spacer is found at its own length
        got = sc.rank_sum_bipartite([Pwm], specs, ctl)
        want = enrich.rank_sum_host(want_in[0], want_ctl[0])
        assert isinstance(got, enrich.RankSum) and np.array_equal(got.u2, want.u2) and got.ties == want.ties and (got.na, got.nb) == (200, 200)
        half = sc.rank_sum([Pwm], ctl)
        print(f"planted case: bipartite AUROC {got.auroc()[0]:.4f}, fixed-spacer-3 AUROC {got.auroc()[1]:.4f}, half-site PWM AUROC {half.auroc()[0]:.4f}")
        assert np.array_equal(got.auroc(), want.auroc())   # the AUROC tests/test_bipartite_host.py establishes on the restatement
        assert got.auroc()[0] >= 0.95 and got.auroc()[1] <= 0.60 and half.auroc()[0] <= 0.55
    finally:
        sc.close()
        ctl.close()


# ------------------------------------------------------------------------------------------------ 7. recycled memory, determinism, independence

def representative(world):
    seg = world["dims"]["seg_windows"]
    rng = np.random.default_rng(21)
    specs = world["specs"][:3] + world["specs"][8:14] + world["specs"][20:]            # four unscorable ones among them (first, between, last)
    seqs = [random_dna(rng, n) for n in (0, 5, 64, 300, seg + 40, 2 * seg + 3)] + [bc.with_n(random_dna(rng, 90), 31, 32, 70)]
    return specs, seqs


def test_recycled_memory_does_not_reach_the_result(world):
    mats = world["mats"]
    specs, seqs = representative(world)
    want = bipartite.best_bipartite_host(mats, specs, seqs, 3)
    other = (world["specs"][1:5], [random_dna(np.random.default_rng(3), 150)] * 3)
    plain = run(mats, specs, seqs)
    bc.same_planes(plain, want)
    try:
        for byte in (0x00, 0xFF, 0xA5):
            with _lib.alloc_fill(byte):
                run(mats, *other)                          # another call in between: its blocks are what the next one is handed
                filled = run(mats, specs, seqs)
            assert same_bytes(filled, plain), hex(byte)
            bc.same_planes(filled, want)
    finally:
        _lib.check(_lib.lib().ms_debug_alloc_fill(-1, None))
    assert same_bytes(run(mats, specs, seqs), plain)


def test_two_runs_give_the_same_bytes_and_a_cell_does_not_depend_on_its_company(world):
    mats = world["mats"]
    specs, seqs = representative(world)
    first, second = run(mats, specs, seqs), run(mats, specs, seqs)
    assert same_bytes(first, second)
    rows, cols = [1, 3, 4, 9, 11, len(specs) - 1], [1, 4, 5, 6]      # (the subset, too, ends on an unscorable spec)
    sub = run(mats, [specs[i] for i in rows], [seqs[r] for r in cols])
    for plane, part in zip(first, sub):
        assert np.ascontiguousarray(plane[np.ix_(rows, cols)]).tobytes() == part.tobytes()
    alone = run(mats, [specs[10]], [seqs[5]])             # one cell of a long region, alone
    assert np.isfinite(alone[0][0, 0])
    assert all(np.ascontiguousarray(p[10:11, 5:6]).tobytes() == a.tobytes() for p, a in zip(first, alone))


# ------------------------------------------------------------------------------------------------ 8. empty sets, invalid arguments

def test_empty_spec_list_and_empty_region_set(world):
    mats = world["mats"][:3]
    assert all(p.shape == (0, 2) for p in run(mats, [], ["ACGT", "AC"]))
    assert all(p.shape == (2, 0) for p in run(mats, [Bipartite(0, 1, 0, 0, 1), Bipartite(2, 2, 1, 0, 0)], []))
    assert run(mats, [], [])[3].shape == (0, 0)


def test_every_invalid_argument_raises_with_the_librarys_message():
    L = _lib.lib()
    pw, sq = _lib.PwmSet.from_matrices([random_pwm(3, 1), random_pwm(5, 2)]), _lib.SeqSet.from_strings(["ACGTACGTACGTACGT"])
    h = ctypes.c_void_p()
    G = _lib.bipartite_dims()["max_gap"]

    def raw(spec, n=1, mask=3, flags=0, pwms=pw.h, seqs=sq.h, out=h, null=False):
        a, b, flip, g0, g1 = bipartite.spec_arrays([spec])
        ptrs = [None] * 5 if null else [_lib.ptr(a, ctypes.c_int32), _lib.ptr(b, ctypes.c_int32), _lib.ptr(flip, ctypes.c_uint8), _lib.ptr(g0, ctypes.c_int32), _lib.ptr(g1, ctypes.c_int32)]
        return L.ms_scan_best_bipartite(pwms, *ptrs, n, seqs, mask, flags, ctypes.byref(out) if out is not None else None)
    good = (0, 1, 0, 0, 2)
    try:
        for kwargs, spec, text in ((dict(pwms=None), good, "NULL handle"), (dict(seqs=None), good, "NULL handle"), (dict(null=True), good, "spec array is NULL"),
                                   (dict(n=-1), good, "n_specs must be >= 0"), (dict(), (2, 0, 0, 0, 0), "outside \\[0, 2\\)"), (dict(), (0, -1, 0, 0, 0), "outside \\[0, 2\\)"),
                                   (dict(), (0, 1, 2, 0, 0), "flip 2"), (dict(), (0, 1, 0, -1, 0), "gaps -1 .. 0"), (dict(), (0, 1, 0, 3, 2), "gaps 3 .. 2"),
                                   (dict(), (0, 1, 0, 0, G + 1), "gap_max <= %d" % G), (dict(mask=0), good, "invalid strand mask 0"),
                                   (dict(mask=4), good, "invalid strand mask 4"), (dict(flags=1), good, "unknown bipartite best-site scan flags 0x1")):
            rc = raw(spec, **kwargs)
            assert rc == _lib.MS_ERR_INVALID and not h.value, text
            with pytest.raises(ValueError, match=text):
                _lib.check(rc)
        rc = raw(good, out=None)
        assert rc == _lib.MS_ERR_INVALID
        with pytest.raises(ValueError, match="out is NULL"):
            _lib.check(rc)
        assert raw(good, n=0, null=True) == _lib.MS_OK and h.value      # n_specs = 0 reads no array
        L.ms_best_free(h)
        res = _lib.scan_best_bipartite(pw, [good], sq)       # ... and the handles still work
        assert res.shape == (1, 1) and res.pos[0, 0] >= 0 and 0 <= res.gaps()[0, 0] <= 2
        with pytest.raises(ValueError, match="motif range"):
            res.sites(0, 2)
        res.close()
    finally:
        sq.close()
        pw.close()
