"""
The host side of the site signal (ms_result_site_signal; motifscan_amd.footprint): the sequential restatement footprint.site_signal_host
pinned by hand-written cases whose expected numbers are typed out below, the Track constructors and formats.read_bedgraph on tiny inputs,
the SiteSignal arithmetic, the cases of tests/sitesignal_cases.py held to what they claim, the exported symbols and what must fail loudly
without a GPU.  No GPU.  tests/test_gpu_sitesignal.py runs the device against the restatement.
"""
import ctypes
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import sitesignal_cases as cases
from motifscan_amd import _lib, footprint, formats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()


def host(sites, widths, values, lengths, flank):
    return footprint.site_signal_host(*cases.hit_arrays(sites), widths, values, cases.offsets_of(lengths), flank)


# ------------------------------------------------------------------------------------------- the restatement, by hand --

def test_plus_and_minus_at_one_position_read_the_columns_in_opposite_order():
    # one region of 10 bases holding 1 .. 10; W = 2 at pos 4 (values 5, 6), flank 2: '+' reads 3 4 | 5 6 | 7 8, '-' the reverse
    got = host([[(0, 4, 1), (0, 4, 2)]], [2], np.arange(1, 11), [10], 2)
    assert got.sum.tolist() == [[[3, 4, 5, 6, 7, 8], [8, 7, 6, 5, 4, 3]]]
    assert got.cover.tolist() == [[[1] * 6, [1] * 6]]
    assert got.n_sites.tolist() == [[1, 1]]
    assert got.per_site.tolist() == [[7, 11, 15], [15, 11, 7]]                  # hit order: '+' then '-'; upstream follows the motif
    assert got.site_offsets.tolist() == [0, 2] and got.flank == 2 and got.widths.tolist() == [2]


def test_a_site_at_pos_0_has_its_upstream_columns_outside():
    # values 1 .. 8, W = 2 at pos 0, flank 3: columns 0 .. 2 are outside on '+', columns 5 .. 7 on '-'
    got = host([[(0, 0, 1)]], [2], np.arange(1, 9), [8], 3)
    assert got.sum.tolist() == [[[0, 0, 0, 1, 2, 3, 4, 5], [0] * 8]]
    assert got.cover.tolist() == [[[0, 0, 0, 1, 1, 1, 1, 1], [0] * 8]]
    assert got.per_site.tolist() == [[0, 3, 12]]
    got = host([[(0, 0, 2)]], [2], np.arange(1, 9), [8], 3)
    assert got.sum.tolist() == [[[0] * 8, [5, 4, 3, 2, 1, 0, 0, 0]]]
    assert got.cover.tolist() == [[[0] * 8, [1, 1, 1, 1, 1, 0, 0, 0]]]
    assert got.per_site.tolist() == [[12, 3, 0]] and got.n_sites.tolist() == [[0, 1]]


def test_a_site_ending_on_the_region_end():
    # values 1 .. 6, W = 3 at pos 3 (values 4 5 6), flank 2: downstream columns outside
    got = host([[(0, 3, 1)]], [3], np.arange(1, 7), [6], 2)
    assert got.sum.tolist() == [[[2, 3, 4, 5, 6, 0, 0], [0] * 7]]
    assert got.cover.tolist() == [[[1, 1, 1, 1, 1, 0, 0], [0] * 7]]
    assert got.per_site.tolist() == [[5, 15, 0]]


def test_a_region_of_exactly_the_motif_width():
    got = host([[(0, 0, 1), (0, 0, 2)]], [4], [10, 20, 30, 40], [4], 1)
    assert got.sum.tolist() == [[[0, 10, 20, 30, 40, 0], [0, 40, 30, 20, 10, 0]]]
    assert got.cover.tolist() == [[[0, 1, 1, 1, 1, 0], [0, 1, 1, 1, 1, 0]]]
    assert got.per_site.tolist() == [[0, 100, 0], [0, 100, 0]]


def test_nothing_leaks_from_a_neighbouring_region():
    # three regions of 4; the middle one holds 1 2 3 4, its neighbours 10^6 everywhere: no sum may reach 10^6
    values = [10 ** 6] * 4 + [1, 2, 3, 4] + [10 ** 6] * 4
    got = host([[(1, 0, 1), (1, 2, 2)]], [2], values, [4, 4, 4], 3)
    assert got.sum.tolist() == [[[0, 0, 0, 1, 2, 3, 4, 0], [0, 0, 0, 4, 3, 2, 1, 0]]]
    assert got.cover.tolist() == [[[0, 0, 0, 1, 1, 1, 1, 0], [0, 0, 0, 1, 1, 1, 1, 0]]]
    assert got.per_site.tolist() == [[0, 3, 7], [0, 7, 3]]


def test_two_motifs_share_the_pitch_and_refusals():
    got = host([[(0, 1, 1)], [(0, 0, 1), (0, 2, 1)]], [1, 3], [1, 2, 3, 4, 5], [5], 1)
    assert got.sum.shape == (2, 2, 5)
    assert got.sum[:, 0].tolist() == [[1, 2, 3, 0, 0], [0 + 2, 1 + 3, 2 + 4, 3 + 5, 4]]
    assert got.cover[:, 0].tolist() == [[1, 1, 1, 0, 0], [1, 2, 2, 2, 1]]
    assert got.site_offsets.tolist() == [0, 1, 3] and got.per_site.tolist() == [[1, 2, 3], [0, 6, 4], [2, 12, 0]]
    for sites in ([[(0, 3, 1)], []], [[(0, -1, 1)], []], [[(1, 0, 1)], []]):
        with pytest.raises(ValueError):
            host(sites, [3, 1], [1, 2, 3, 4, 5], [5], 0)
    with pytest.raises(ValueError):
        host([[]], [1], [1], [1], footprint.MAX_FLANK + 1)


# --------------------------------------------------------------------------------------------------------- SiteSignal --

def test_site_signal_arithmetic():
    total = np.array([[[2, 4, 6, 1, 8, 10, 0], [0, 6, 2, 1, 2, 0, 0]]], dtype=np.int64)
    cover = np.array([[[1, 2, 2, 2, 2, 2, 0], [0, 2, 1, 1, 1, 0, 0]]], dtype=np.int64)
    per_site = np.array([[8, 2, 20], [3, 6, 3]], dtype=np.int64)
    s = footprint.SiteSignal(total, cover, np.array([[2, 2]]), per_site, np.array([0, 2]), np.array([2]), 2)
    assert s.profile(0).tolist() == [2, 10, 8, 2, 10, 10] and s.profile(0, "-").tolist() == [0, 6, 2, 1, 2, 0] and s.profile(0, 0).tolist() == [2, 4, 6, 1, 8, 10]
    assert s.mean_profile(0).tolist() == [2.0, 2.5, 8 / 3, 2 / 3, 10 / 3, 5.0]
    assert s.depth(0) == pytest.approx((2.0 + 2.5 + 10 / 3 + 5.0) / 4 - (8 / 3 + 2 / 3) / 2)
    assert s.site_scores(0).tolist() == [28 / 4 - 1.0, 6 / 4 - 3.0]
    # the second site at pos 1 of a region of 6: one upstream column, two downstream
    assert s.site_scores(0, pos=[2, 1], lengths=[6, 6]).tolist() == [28 / 4 - 1.0, 6 / 3 - 3.0]
    with pytest.raises(ValueError):
        s._replace(per_site=None).site_scores(0)


# ------------------------------------------------------------------------------------------------------------- tracks --

def R(chrom, start, end):
    return SimpleNamespace(chrom=chrom, start=start, end=end)


def test_track_from_arrays_and_chrom_arrays():
    t = footprint.Track.from_arrays([[1, 2, 3], [], np.array([7, -8], dtype=np.int64)])
    assert t.values.dtype == np.int32 and t.values.tolist() == [1, 2, 3, 7, -8] and t.offsets.tolist() == [0, 3, 3, 5] and t.n_regions == 3
    assert t.region(2).tolist() == [7, -8]
    with pytest.raises(ValueError):
        footprint.Track.from_arrays([[2 ** 31]])
    with pytest.raises(ValueError):
        footprint.Track.from_arrays([[0.5]])
    with pytest.raises(ValueError):
        footprint.Track([1, 2, 3], [0, 2])
    chroms = {"chr1": np.arange(10), "chr2": np.arange(100, 105)}
    t = footprint.Track.from_chrom_arrays(chroms, [R("chr1", 2, 5), R("chr2", 3, 8), R("chr1", 8, 10), R("chrX", 0, 2)])
    assert t.offsets.tolist() == [0, 3, 8, 10, 12]
    assert t.values.tolist() == [2, 3, 4, 103, 104, 0, 0, 0, 8, 9, 0, 0]       # past the chromosome's array, and chrX: 0


def test_track_from_points():
    regions = [R("chr1", 10, 15), R("chr1", 13, 16), R("chr2", 0, 3)]
    chrom = ["chr1", "chr1", "chr1", "chr2", "chr1", "chr3", "chr1", "chr2"]
    pos = [10, 14, 14, 2, 15, 1, 9, 3]                                          # 15: only the second region; 9, chr3, chr2:3: outside every region
    t = footprint.Track.from_points(chrom, pos, regions)
    assert t.offsets.tolist() == [0, 5, 8, 11]
    assert t.values.tolist() == [1, 0, 0, 0, 2, 0, 2, 1, 0, 0, 1]
    t = footprint.Track.from_points(chrom, pos, regions, weight=[1, 2, 3, 4, 5, 6, 7, 8])
    assert t.values.tolist() == [1, 0, 0, 0, 5, 0, 5, 5, 0, 0, 4]
    with pytest.raises(ValueError):
        footprint.Track.from_points(["chr1"] * 2, [10, 10], regions, weight=2 ** 30)


def test_track_from_intervals_clips_rows_to_the_regions():
    regions = [R("chr1", 10, 16), R("chr2", 0, 4)]
    chrom = ["chr1", "chr1", "chr1", "chr2", "chr9"]
    start, end, value = [5, 12, 15, 2, 0], [11, 14, 30, 9, 50], [7, 3, -2, 9, 1]   # rows that overlap the region's start, its end, chr2's end
    t = footprint.Track.from_intervals(chrom, start, end, value, regions)
    assert t.values.tolist() == [7, 0, 3, 3, 0, -2, 0, 0, 9, 9]
    later = footprint.Track.from_intervals(["chr1", "chr1"], [10, 12], [16, 13], [1, 5], regions[:1])
    assert later.values.tolist() == [1, 1, 5, 1, 1, 1]                          # the last row that covers a base wins


def test_track_from_float_rounds_to_even_and_refuses_what_does_not_fit():
    t = footprint.Track.from_float([0.5, 1.5, 2.5, -0.5, -1.5, 0.25, 1.26], [0, 7], 1)
    assert t.values.tolist() == [0, 2, 2, 0, -2, 0, 1]
    t = footprint.Track.from_float([0.125, 0.375, 1.0], [0, 2, 3], 4)
    assert t.values.tolist() == [0, 2, 4] and t.offsets.tolist() == [0, 2, 3]
    assert footprint.Track.from_float([2 ** 31 - 1, -2 ** 31], [0, 2], 1).values.tolist() == [2 ** 31 - 1, -2 ** 31]
    for bad in ([2.0 ** 31], [-2.0 ** 31 - 1], [float("nan")], [float("inf")]):
        with pytest.raises(ValueError):
            footprint.Track.from_float(bad, [0, 1], 1)
    with pytest.raises(ValueError):
        footprint.Track.from_float([1.0], [0, 1], 3e9)


def test_read_bedgraph(tmp_path):
    path = tmp_path / "t.bedgraph"
    path.write_text("track type=bedGraph name=x\n# a comment\nchr1\t0\t10\t1.5\nchr1 10 12 -2\n\nchr2\t5\t6\t3e2\nchrM\t0\t0\t0\n")
    chrom, start, end, value = formats.read_bedgraph(str(path))
    assert chrom.tolist() == ["chr1", "chr1", "chr2", "chrM"] and start.tolist() == [0, 10, 5, 0] and end.tolist() == [10, 12, 6, 0]
    assert start.dtype == np.int64 and value.dtype == np.float64 and value.tolist() == [1.5, -2.0, 300.0, 0.0]
    for text, line in (("chr1\t0\t10\n", 1), ("chr1\t0\t10\t1\nchr1\t9\t3\t1\n", 2), ("chr1\tx\t10\t1\n", 1)):
        path.write_text(text)
        with pytest.raises(ValueError, match=f"line {line}"):
            formats.read_bedgraph(str(path))


# ---------------------------------------------------------------------------------------- the GPU cases, held to their claims --

def columns(c, m=0):
    return c["widths"][m] + 2 * c["flank"]


@pytest.mark.parametrize("ncol", cases.COLUMN_COUNTS)
def test_column_cases_have_the_columns_they_name(ncol):
    c = cases.column_case(ncol)
    assert columns(c) == ncol == max(c["widths"]) + 2 * c["flank"] and c["widths"][1] < c["widths"][0]
    off, seq_idx, pos, strand = c["hits"]
    assert np.diff(off).min() > 0 and set(strand.tolist()) == {1, 2}
    L = np.asarray(c["lengths"])[seq_idx]
    W = np.repeat(c["widths"], np.diff(off))
    assert (pos >= 0).all() and (pos + W <= L).all() and (pos == 0).any() and (pos + W == L).any()
    assert np.abs(c["values"].astype(np.int64)).max() > 2 ** 30               # sums of two sites leave 32 bits


def test_the_panel_cases_sit_on_the_panel():
    assert cases.PANEL in cases.COLUMN_COUNTS and cases.PANEL + 1 in cases.COLUMN_COUNTS
    assert set(cases.COLUMN_COUNTS) >= {63, 64, 65, 128, 129}
    assert cases.PANEL % 64 == 0 and cases.THREADS % 64 == 0 and cases.CHUNK % cases.THREADS == 0 and cases.MAX_BX >= 1


def test_flank_cases():
    assert cases.FLANKS == (0, cases.MAX_FLANK) and cases.MAX_FLANK == footprint.MAX_FLANK == 512
    for f in cases.FLANKS:
        c = cases.flank_case(f)
        assert c["flank"] == f and min(c["lengths"]) == max(c["widths"])       # a region of exactly the widest motif's width
    wide = cases.flank_case(cases.MAX_FLANK)
    assert columns(wide, 1) > 4 * cases.PANEL and max(wide["lengths"]) > 2 * cases.MAX_FLANK    # several panels; a region longer than both flanks


def test_pad_case_touches_both_ends_of_the_track():
    c = cases.pad_case()
    off, seq_idx, pos, strand = c["hits"]
    assert c["flank"] == cases.MAX_FLANK and len(pos) == 4
    assert [(int(r), int(p), int(s)) for r, p, s in zip(seq_idx, pos, strand)] == [(0, 0, 1), (0, 0, 2), (2, 3, 1), (2, 3, 2)]
    assert pos[2] + c["widths"][0] == c["lengths"][-1] and len(c["lengths"]) == 3
    want = footprint.site_signal_host(*c["hits"], c["widths"], c["values"], cases.offsets_of(c["lengths"]), c["flank"])
    f, W = c["flank"], 3
    assert want.cover[0, 0, :f].sum() == 3 and want.cover[0, 0, f + W:].sum() == 2 + 0     # '+': region 2's site has 3 bases upstream, region 0's 2 downstream
    assert want.cover[0].sum() == 2 * (5 + 6)                                  # every site covers its whole region and nothing else


def test_chunk_case_counts():
    c = cases.chunk_case()
    n = np.diff(c["hits"][0]).tolist()
    assert n == c["n_hits"] == [0, cases.CHUNK - 1, cases.CHUNK, 0, cases.CHUNK + 1, 5, 0]
    assert len(c["widths"]) == len(n)


def test_stride_and_int64_cases():
    c = cases.stride_case()
    off, seq_idx, pos, strand = c["hits"]
    n = int(off[-1])
    assert n > cases.MAX_BX * cases.CHUNK and -(-n // cases.CHUNK) > cases.MAX_BX and n % cases.CHUNK not in (0, cases.CHUNK)
    assert c["widths"] == [1] and c["flank"] == 0 and len(c["lengths"]) == 1 and (np.diff(pos) >= 0).all() and pos.max() == c["lengths"][0] - 1
    assert set(strand.tolist()) == {1, 2}
    total, cover, n_sites, per_site = cases.closed_form(c)
    assert cover.sum() == n and per_site[:, 1].sum() == total.sum()
    small = cases.case("s", [1], [3], [5, -7, 9], [[(0, 0, 1), (0, 1, 2), (0, 2, 1), (0, 2, 1)]], 0)      # the closed form against the restatement
    want = footprint.site_signal_host(*small["hits"], [1], small["values"], [0, 3], 0)
    for a, b in zip(cases.closed_form(small), (want.sum, want.cover, want.n_sites, want.per_site)):
        assert np.array_equal(a, b)
    for value in (2 ** 31 - 1, -2 ** 31):
        c = cases.int64_case(value)
        assert int(c["hits"][0][-1]) == 2 ** 22 + 1 and c["values"].tolist() == [value]
        total = cases.closed_form(c)[0]
        assert int(total[0, 0, 0]) == (2 ** 22 + 1) * value and abs(int(total[0, 0, 0])) > 2 ** 53
    assert ((2 ** 22 + 1) * (2 ** 31 - 1)) % 2 == 1


def test_strands_and_general_cases():
    c = cases.strands_case()
    off, seq_idx, pos, strand = c["hits"]
    assert (seq_idx[0], pos[0], strand[0]) == (seq_idx[1], pos[1], 1) and strand[1] == 2 and off[1] == 2
    assert (strand[off[1]:] == 2).all() and off[2] - off[1] > 1
    g = cases.general_case()
    assert len(g["widths"]) == 4 and np.diff(g["hits"][0]).min() > 0 and len(g["lengths"]) >= 3


# --------------------------------------------------------------------------------------------------------- the library --

def test_symbols_header_and_constants():
    with open(os.path.join(ROOT, "include", "motifscan_amd.h")) as fh:
        text = fh.read()
    table = text[:text.index("#ifndef MOTIFSCAN_AMD_H")]
    assert re.search(r"\bint\s+ms_result_site_signal\s*\(", text) and re.search(r"ms_result_site_signal\s+\*\s+no reference counterpart", table)
    assert re.search(r"#define\s+MS_SITESIGNAL_MAX_FLANK\s+512\b", text)
    with open(os.path.join(ROOT, "include", "motifscan_amd_debug.h")) as fh:
        assert re.search(r"\bint\s+ms_debug_sitesignal_dims\s*\(\s*int32_t\s+out\[4\]\s*\)", fh.read())
    for name in ("ms_track_create", "ms_track_size", "ms_track_values_host", "ms_track_free", "ms_result_site_signal", "ms_debug_sitesignal_dims"):
        assert hasattr(_lib.lib(), name), name
    d = _lib.sitesignal_dims()                                                 # no device needed
    assert all(v > 0 for v in d.values()) and len(d) == 4
    assert d["threads"] % 64 == 0 and d["chunk_sites"] % d["threads"] == 0 and d["panel_columns"] % 64 == 0
    assert _lib.lib().ms_debug_sitesignal_dims(None) == _lib.MS_ERR_INVALID


def test_no_gpu_means_loud_failure_not_fallback():
    have_device = _lib.device_count() > 0
    out = np.zeros((1, 2, 3), dtype=np.int64)
    rc = _lib.lib().ms_result_site_signal(None, None, None, 0, 0, 1, 0, ctypes.c_void_p(out.ctypes.data), None, None, None, None)
    h = ctypes.c_void_p()
    offsets = np.array([0, 2], dtype=np.int64)
    values = np.array([1, 2], dtype=np.int32)
    if have_device:
        assert rc == _lib.MS_ERR_INVALID                                       # NULL handles
        return
    assert rc == _lib.MS_ERR_RUNTIME                                           # no device: said before the handles are looked at
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _lib.check(rc)
    rc = _lib.lib().ms_track_create(ctypes.c_void_p(values.ctypes.data), _lib.ptr(offsets, ctypes.c_int64), 1, ctypes.byref(h))
    assert rc == _lib.MS_ERR_RUNTIME and not h.value
    with pytest.raises(RuntimeError):
        footprint.Track.from_arrays([[1, 2]]).upload()
    with pytest.raises(RuntimeError):
        footprint.site_signal([[[]]], [np.ones((4, 3))], footprint.Track.from_arrays([[1, 2, 3, 4]]))
