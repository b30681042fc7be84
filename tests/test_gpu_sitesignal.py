"""
The site signal on the device (ms_track_*, ms_result_site_signal; motifscan_amd.footprint, Scanner.site_signal) against the sequential
restatement footprint.site_signal_host, or against a closed form where a case is too large for it.  Every comparison is exact: the sums are
int64 reductions.  Most results are made of chosen hit arrays (ms_result_from_hits), which places every boundary where the test wants it
-- the wave's 64 columns, the panel of a block, the first region's left flank and the last region's right flank (the track's pad), the
chunk of a block, the blocks' stride loop -- with the sizes from ms_debug_sitesignal_dims (tests/sitesignal_cases.py); the last test scans.
Run with -m gpu.
"""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest

import sitesignal_cases as cases
from motifscan_amd import _lib, footprint, synth
from motifscan_amd.scanner import Scanner

pytestmark = pytest.mark.gpu

CASES = {c["name"]: c for c in cases.all_cases()}
_HOST = {}


@pytest.fixture(scope="module", autouse=True)
def device():
    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests need an MI355X (there is no CPU fallback)")
    _lib.set_device(0)


def host_of(c):
    """The restatement of a case, computed once and shared."""
    if c["name"] not in _HOST:
        _HOST[c["name"]] = footprint.site_signal_host(*c["hits"], c["widths"], c["values"], cases.offsets_of(c["lengths"]), c["flank"])
    return _HOST[c["name"]]


class Case:
    """A result of a case's hits with the PWM set (widths only) and the resident track it goes with."""

    def __init__(self, c, n_regions=None):
        self.c = c
        offsets, seq_idx, pos, strand = c["hits"]
        R = len(c["lengths"])
        self.res = _lib.result_from_hits(len(offsets) - 1, R if n_regions is None else n_regions, offsets, seq_idx, pos, np.zeros(len(pos)), strand)
        self.pw = _lib.PwmSet.from_matrices([np.ones((4, w)) for w in c["widths"]])
        self.tr = _lib.Track.from_values(c["values"], cases.offsets_of(c["lengths"]))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.res.close()
        self.pw.close()
        self.tr.close()

    def device(self, flank=None, **kw):
        kw.setdefault("per_site", True)
        return self.res.site_signal(self.pw, self.tr, self.c["flank"] if flank is None else flank, **kw)


def same(got, want):
    """(sum, cover, n_sites, per_site) of the device == the SiteSignal of the restatement."""
    total, cover, n_sites, per_site = got
    assert total.dtype == np.int64 and total.shape == want.sum.shape and cover.shape == want.cover.shape
    assert np.array_equal(total, want.sum)
    assert np.array_equal(cover, want.cover)
    assert np.array_equal(n_sites, want.n_sites)
    assert per_site.shape == want.per_site.shape and np.array_equal(per_site, want.per_site)
    assert (cover <= n_sites[:, :, None]).all()


# ------------------------------------------------------------------------------------------------------------ the track --

def test_a_track_comes_back_as_it_went_in():
    import torch
    rng = np.random.default_rng(1)
    lengths = [5, 0, 300, 1]
    values = cases.random_values(rng, sum(lengths), big=True)
    tr = _lib.Track.from_values(values, cases.offsets_of(lengths))
    try:
        assert (tr.n_seqs, tr.n_values) == (4, 306)
        assert np.array_equal(tr.values(), values) and np.array_equal(tr.values(5, 300), values[5:305]) and tr.values(306, 0).size == 0
        with pytest.raises(ValueError):
            tr.values(300, 7)
    finally:
        tr.close()
    dev = torch.from_numpy(values).cuda()
    torch.cuda.synchronize()
    tr = _lib.Track.from_values(int(dev.data_ptr()), cases.offsets_of(lengths))       # values in device memory
    try:
        assert np.array_equal(tr.values(), values)
    finally:
        tr.close()
    empty = _lib.Track.from_values(np.zeros(0, dtype=np.int32), [0])
    assert (empty.n_seqs, empty.n_values) == (0, 0)
    empty.close()
    for offsets in ([1, 3], [0, 3, 2]):
        with pytest.raises(ValueError):
            _lib.Track.from_values(np.zeros(3, dtype=np.int32), np.array(offsets))
    h = ctypes.c_void_p()
    off = np.array([0, 2], dtype=np.int64)
    assert _lib.lib().ms_track_create(None, _lib.ptr(off, ctypes.c_int64), 1, ctypes.byref(h)) == _lib.MS_ERR_INVALID     # NULL values
    assert _lib.lib().ms_track_create(None, _lib.ptr(off, ctypes.c_int64), -1, ctypes.byref(h)) == _lib.MS_ERR_INVALID


# ------------------------------------------------------------------------------------------- the cases, device == restatement --

@pytest.mark.parametrize("name", list(CASES))
def test_case_against_the_restatement(name):
    """Columns on the wave's and the panel's edges, flank 0 and the largest, the track's two ends under the largest flank, the chunk of a
    block with empty motifs around it, both strands at one position and a motif of '-' sites only."""
    c = CASES[name]
    want = host_of(c)
    with Case(c) as k:
        same(k.device(), want)
    assert want.cover.any() and want.per_site.any()
    if name == "pad":                                                          # the outside columns stay uncovered
        f = c["flank"]
        assert not want.cover[0, 0, :f - 3].any() and not want.cover[0, 0, f + 3 + 2:].any() and want.cover[0, 0, f - 3:f + 5].all()


def test_one_above_the_largest_flank_is_refused():
    with Case(CASES["strands"]) as k:
        for flank in (cases.MAX_FLANK + 1, -1):
            with pytest.raises(ValueError, match="flank"):
                k.device(flank)


def test_sub_ranges_empty_motifs_and_the_empty_range():
    """The full range and every single-row range give the same rows; per_site of a range starts at the range's first hit; an empty motif's
    row is zero; m0 == m1 does nothing."""
    c = CASES["chunks"]
    want = host_of(c)
    P = len(c["widths"])
    off = c["hits"][0]
    with Case(c) as k:
        for m0, m1 in [(m, m + 1) for m in range(P)] + [(1, 5), (2, 3), (3, P)]:
            total, cover, n_sites, per_site = k.device(m0=m0, m1=m1)
            assert total.shape[0] == m1 - m0 and np.array_equal(total, want.sum[m0:m1]) and np.array_equal(cover, want.cover[m0:m1]), (m0, m1)
            assert np.array_equal(n_sites, want.n_sites[m0:m1]) and np.array_equal(per_site, want.per_site[off[m0]:off[m1]]), (m0, m1)
        for m in (0, 3, P - 1):
            assert not want.sum[m].any() and not want.n_sites[m].any()
        total, cover, n_sites, per_site = k.device(m0=2, m1=2)
        assert total.shape == (0, 2, want.sum.shape[2]) and n_sites.shape == (0, 2) and per_site.shape == (0, 3)
        spare = np.full(4, -1, dtype=np.int64)
        rc = _lib.lib().ms_result_site_signal(k.res.h, k.pw.h, k.tr.h, 0, 4, 4, 0, ctypes.c_void_p(spare.ctypes.data), None, None, None, None)
        assert rc == _lib.MS_OK and (spare == -1).all()


def test_profile_alone_per_site_alone_and_both_agree():
    c = CASES["general"]
    want = host_of(c)
    off = c["hits"][0]
    with Case(c) as k:
        both = k.device()
        same(both, want)
        total, cover, n_sites, none = k.device(per_site=False)
        assert none is None and np.array_equal(total, both[0]) and np.array_equal(cover, both[1]) and np.array_equal(n_sites, both[2])
        none_s, none_c, n_sites, per_site = k.device(profile=False)
        assert none_s is None and none_c is None and np.array_equal(n_sites, both[2]) and np.array_equal(per_site, both[3])
        _, _, n_mid, mid = k.device(profile=False, m0=1, m1=3)                 # a middle range: row 0 is the range's first hit
        assert np.array_equal(mid, want.per_site[off[1]:off[3]]) and np.array_equal(n_mid, want.n_sites[1:3])
        # sum without cover, through the C ABI
        s = np.full(want.sum.shape, -1, dtype=np.int64)
        rc = _lib.lib().ms_result_site_signal(k.res.h, k.pw.h, k.tr.h, c["flank"], 0, len(c["widths"]), 0, ctypes.c_void_p(s.ctypes.data), None, None, None, None)
        assert rc == _lib.MS_OK and np.array_equal(s, want.sum)


def test_the_wide_flank_agrees_between_the_output_combinations():
    """Several panels: per_site is added panel by panel there, with and without the profile."""
    c = CASES[f"flank_{cases.MAX_FLANK}"]
    want = host_of(c)
    with Case(c) as k:
        _, _, _, per_site = k.device(profile=False)
        assert np.array_equal(per_site, want.per_site)
        assert np.array_equal(k.device(per_site=False)[0], want.sum)
        _, _, _, mid = k.device(profile=False, m0=1, m1=2)
        assert np.array_equal(mid, want.per_site[c["hits"][0][1]:])


# -------------------------------------------------------------------------------------------------- large cases, closed forms --

def test_more_chunks_than_blocks():
    c = cases.stride_case()
    want = cases.closed_form(c)
    with Case(c) as k:
        for got, exp in zip(k.device(), want):
            assert np.array_equal(got, exp)
        total, cover, n_sites, _ = k.device(per_site=False)
        assert np.array_equal(total, want[0]) and np.array_equal(cover, want[1]) and np.array_equal(n_sites, want[2])


@pytest.mark.parametrize("value", [2 ** 31 - 1, -2 ** 31])
def test_sums_are_int64_not_fp64(value):
    """2^22 + 1 sites of one base: (2^22 + 1)(2^31 - 1) is odd and above 2^53, no double holds it."""
    c = cases.int64_case(value)
    with Case(c) as k:
        total, cover, n_sites, _ = k.device(per_site=False)
    n = 2 ** 22 + 1
    assert int(total[0, 0, 0]) == n * value and total[0, 1, 0] == 0
    assert cover.tolist() == [[[n], [0]]] and n_sites.tolist() == [[n, 0]]


# ---------------------------------------------------------------------------------------------- additivity and determinism --

def test_two_runs_give_the_same_bytes_and_three_region_shards_add_up():
    c = CASES["general"]
    with Case(c) as k:
        a = k.device()
        b = k.device()
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)) and a[0].any()
    off = cases.offsets_of(c["lengths"])
    hit_off, seq_idx, pos, strand = c["hits"]
    motif = np.repeat(np.arange(len(c["widths"])), np.diff(hit_off))
    cuts = [0, 9, 20, len(c["lengths"])]
    P = len(c["widths"])
    parts, order = [], []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        per_motif = [np.flatnonzero((seq_idx >= lo) & (seq_idx < hi) & (motif == m)) for m in range(P)]
        sites = [[(int(seq_idx[i]) - lo, int(pos[i]), int(strand[i])) for i in idx] for idx in per_motif]
        shard = cases.case("shard", c["widths"], c["lengths"][lo:hi], c["values"][off[lo]:off[hi]], sites, c["flank"])
        with Case(shard) as k:
            parts.append(k.device())
        order.append(np.concatenate(per_motif))                                # the whole's hit index of every row of the shard's per_site
    assert all(len(o) > 0 for o in order)
    for i in range(3):
        assert np.array_equal(a[i], parts[0][i] + parts[1][i] + parts[2][i])
    whole = np.zeros_like(a[3])                                                # every site's triple is the same in its shard
    for part, idx in zip(parts, order):
        whole[idx] = part[3]
    assert np.array_equal(whole, a[3])


def test_outputs_in_device_memory_equal_the_host_ones():
    import torch
    c = CASES["general"]
    want = host_of(c)
    off = c["hits"][0]
    with Case(c) as k:
        hostside = k.device(m0=1, m1=4)
        C = want.sum.shape[2]
        n_sel = int(off[4] - off[1])
        dev = [torch.full(shape, -1, dtype=torch.int64, device="cuda") for shape in ((3, 2, C), (3, 2, C), (3, 2), (n_sel, 3))]
        torch.cuda.synchronize()                                  # the fills run on torch's stream, the library writes on its own
        ptrs = tuple(int(t.data_ptr()) for t in dev)
        assert k.device(m0=1, m1=4, out=ptrs) == ptrs
        torch.cuda.synchronize()
        for h, t in zip(hostside, dev):
            assert h.tobytes() == t.cpu().numpy().tobytes() and h.any()
        mixed = k.device(m0=1, m1=4, out=(None, ptrs[1], None, ptrs[3]))       # host sum and n_sites, device cover and per_site
        assert np.array_equal(mixed[0], hostside[0]) and mixed[1] == ptrs[1] and np.array_equal(mixed[2], hostside[2]) and mixed[3] == ptrs[3]
        torch.cuda.synchronize()
        assert np.array_equal(dev[3].cpu().numpy(), hostside[3])


# ---------------------------------------------------------------------------------------------------------------- refusals --

def test_refused_calls():
    c = CASES["strands"]
    P = len(c["widths"])
    with Case(c) as k:
        for kw in (dict(flags=1), dict(m0=1, m1=P + 1), dict(m0=-1, m1=1), dict(m0=2, m1=1)):
            with pytest.raises(ValueError):
                k.device(**kw)
        rc = _lib.lib().ms_result_site_signal(k.res.h, k.pw.h, k.tr.h, 0, 0, P, 0, None, None, None, None, None)
        assert rc == _lib.MS_ERR_INVALID                                       # sum and per_site both NULL
        n = np.zeros((P, 2), dtype=np.int64)
        rc = _lib.lib().ms_result_site_signal(k.res.h, k.pw.h, k.tr.h, 0, 0, P, 0, None, None, ctypes.c_void_p(n.ctypes.data), None, None)
        assert rc == _lib.MS_ERR_INVALID and not n.any()
        pw3 = _lib.PwmSet.from_matrices([np.ones((4, 3))] * 3)
        lengths = c["lengths"]
        short = _lib.Track.from_values(c["values"][:sum(lengths[:2])], cases.offsets_of(lengths[:2]))
        longer = _lib.Track.from_values(np.concatenate([c["values"], [1, 2]]).astype(np.int32), cases.offsets_of(lengths + [2]))
        try:
            with pytest.raises(ValueError, match="number of PWMs"):
                k.res.site_signal(pw3, k.tr, 0)
            for tr in (short, longer):
                with pytest.raises(ValueError, match="regions"):
                    k.res.site_signal(k.pw, tr, 0)
            with pytest.raises(ValueError):
                k.device(out=(np.zeros((P, 2, 4), dtype=np.int32), None, None, None))
            with pytest.raises(ValueError):
                k.device(per_site=False, out=(None, None, None, np.zeros((7, 3), dtype=np.int64)))      # per_site not asked for
        finally:
            pw3.close()
            short.close()
            longer.close()
    vals, w8, cutoffs = synth.load_motif_set(8)
    bases, offsets = synth.make_regions(200, 300, seed=3)
    pw8, sq8 = _lib.PwmSet(vals, w8, cutoffs), _lib.SeqSet(bases, offsets)
    tr8 = _lib.Track.from_values(np.ones(int(offsets[-1]), dtype=np.int32), offsets)
    counts_only = _lib.scan(pw8, sq8, 3, _lib.MS_SCAN_COUNTS_ONLY)
    try:
        with pytest.raises(ValueError, match="counts-only"):
            counts_only.site_signal(pw8, tr8, 0)
    finally:
        counts_only.close()
        pw8.close()
        sq8.close()
        tr8.close()


@pytest.mark.parametrize("bad", ["pos + W = L + 1", "pos = -1", "the last region against a shorter one"])
@pytest.mark.parametrize("wide", [False, True])
def test_sites_outside_their_region_are_refused_with_the_outputs_zeroed(bad, wide):
    """Only ms_result_from_hits or the wrong track can bring such a site: it is found on the device while reducing -- with one panel and
    with several -- nothing is read for it, and the outputs are zero afterwards."""
    lengths = [10, 10, 8]
    flank = cases.PANEL if wide else 2
    good = [(0, 0, 1), (1, 7, 2), (2, 5, 1)]
    if bad == "pos + W = L + 1":
        sites = [good + [(2, 6, 1)], []]
    elif bad == "pos = -1":
        sites = [good[:2] + [(2, -1, 2)], []]
    else:                                                                       # regions of the same number, but the last one too short for the site
        sites = [good, []]
        lengths = [10, 10, 7]
    c = cases.case("bad", [3, 4], lengths, np.arange(sum(lengths)) + 1, [sorted(s) for s in sites], flank)
    with Case(c) as k:
        C = 4 + 2 * flank
        out = (np.full((2, 2, C), -7, dtype=np.int64), np.full((2, 2, C), -7, dtype=np.int64), np.full((2, 2), -7, dtype=np.int64),
               np.full((len(sites[0]), 3), -7, dtype=np.int64))
        with pytest.raises(ValueError, match="inside its region"):
            k.device(out=out)
        assert not any(o.any() for o in out)
        only = np.full((len(sites[0]), 3), -7, dtype=np.int64)
        with pytest.raises(ValueError, match="inside its region"):
            k.device(profile=False, out=(None, None, None, only))
        assert not only.any()


# ------------------------------------------------------------------------------------------------------------- end to end --

class ChromGenome:
    """One synthetic chromosome, with what Scanner reads of a genome."""

    def __init__(self, seq):
        self.seq = seq
        self.chrom_sizes = {"chr1": len(seq)}

    def fetch_sequence(self, chrom, start, end):
        return self.seq[start:end]


def test_scanner_site_signal_end_to_end_with_a_planted_footprint():
    """200 regions x 300 bp, 20 motifs, one scan on the device; the consensus of one motif planted in every second region with a dip of
    the track under it: Scanner.site_signal == the restatement over the scan's own hits, and the planted motif shows a footprint."""
    n_regions, L, flank, planted, at = 200, 300, 20, 7, 140
    vals, widths, cutoffs = synth.load_motif_set(20)
    bases, offsets = synth.make_regions(n_regions, L, seed=5, frac_n=0.0)
    mats, o = [], 0
    for w in widths:
        mats.append(vals[o:o + 4 * w].reshape(4, w).copy())
        o += 4 * w
    W = int(widths[planted])
    consensus = np.frombuffer(b"ACGT", dtype=np.uint8)[mats[planted].argmax(axis=0)]
    values = (40 + (np.arange(n_regions * L) * 7) % 13).astype(np.int32)
    bases = bases.copy()
    for r in range(0, n_regions, 2):
        bases[r * L + at:r * L + at + W] = consensus
        values[r * L + at:r * L + at + W] = 3
    seq = bases.tobytes().decode()
    regions = [SimpleNamespace(chrom="chr1", start=r * L, end=(r + 1) * L, summit=r * L, score=None) for r in range(n_regions)]
    pwms = [SimpleNamespace(matrix=m, length=m.shape[1], cutoffs={"1e-4": float(c)}, matrix_id=f"M{i}", name=f"m{i}")
            for i, (m, c) in enumerate(zip(mats, cutoffs))]
    track = footprint.Track(values, offsets)
    sc = Scanner(ChromGenome(seq), regions, window_size=0, strand="both", p_value="1e-4", remove_dup=False)
    try:
        got = sc.site_signal(pwms, track, flank=flank, per_site=True)
        a = sc.scan_motifs_arrays(pwms)
        pos = a["start"] - np.asarray(sc.seq_starts, dtype=np.int64)[a["region"]]
        want = footprint.site_signal_host(a["motif_offsets"], a["region"], pos, a["strand"], widths, values, offsets, flank)
        a["_result"].close()
    finally:
        sc.close()
    assert isinstance(got, footprint.SiteSignal) and got.flank == flank and np.array_equal(got.widths, widths)
    for x, y in zip(got[:5], want[:5]):
        assert np.array_equal(x, y)
    assert got.n_sites[planted].sum() >= n_regions // 2 and got.n_sites.sum() > 200
    assert got.depth(planted) > 0
    scores = got.site_scores(planted)
    assert len(scores) == got.n_sites[planted].sum() and np.median(scores) > 0
