"""
What ms_result.hip does to a scan's hits after they are ordered, at its boundaries, over the synthetic hit lists of
tests/result_cases.py (ms_result_from_hits: no scan, no golden): dedup_kernel, the prefix sum with remap_offsets_kernel and
compact_hits_kernel, site_tables_kernel with fill_nan_kernel, pack_hits_kernel in its 8-byte and 4-byte forms, and the three accessors
that share the result's one pinned host buffer.  Run with -m gpu.

Expected values are the reference's recurrence in plain Python (result_cases.literal_keep, site_tables_expected) and the compact
words as include/motifscan_amd.h states them (result_cases.encode16 / encode12); tests/test_result_cases_host.py holds the cases to
their conditions (result_cases.CONDITIONS) without a GPU.  Every comparison is exact: integers by value, scores and maxima by their bits.
"""
import numpy as np
import pytest

import result_cases as rc
from motifscan_amd import _lib, synth

pytestmark = pytest.mark.gpu

ARRAYS = ("seq_idx", "pos", "score", "strand")


@pytest.fixture(scope="module", autouse=True)
def device():
    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests need an MI355X (there is no CPU fallback)")
    _lib.set_device(0)


def result_of(case):
    return _lib.result_from_hits(len(case["widths"]), case["n_regions"], case["motif_offsets"], case["seq_idx"], case["pos"], case["score"],
                                 case["strand"])


def pwms_of(case):
    return _lib.PwmSet.from_matrices([np.full((4, int(w)), 0.25) for w in case["widths"]])


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def assert_hits(got, want, what=""):
    assert np.array_equal(got["motif_offsets"], want["motif_offsets"]), (what, got["motif_offsets"].tolist()[:12], want["motif_offsets"].tolist()[:12])
    for k in ("seq_idx", "pos", "strand"):
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (what, k, np.flatnonzero(np.asarray(got[k]) != np.asarray(want[k]))[:8].tolist())
    assert same_bits(got["score"], want["score"]), (what, "score")


def read_every_way(res, want, fits12, what):
    """ms_result_hits into caller buffers, the pinned arrays, the 16-byte form and (where the list fits it) the 12-byte form"""
    assert res.n_hits == len(want["pos"]), what
    assert_hits(res.hits_pageable(), want, what + ": ms_result_hits")
    assert_hits(res.hits(), want, what + ": hits()")
    assert_hits(res.hits(copy=False), want, what + ": hits(copy=False)")
    assert_hits(res.hits(packed=16), want, what + ": hits(packed=16)")
    assert res.packed_form() == 16
    if fits12:
        assert_hits(res.hits(packed=12), want, what + ": hits(packed=12)")
        assert res.packed_form() == 12
    assert_hits(res.hits(copy=False), want, what + ": hits(copy=False) after the compact forms")


def recount_regions(h, n_pwms):
    """per motif the regions with a site, from the hit list itself"""
    motif = np.repeat(np.arange(n_pwms), np.diff(h["motif_offsets"]))
    new = np.ones(len(motif), dtype=bool)
    new[1:] = (motif[1:] != motif[:-1]) | (h["seq_idx"][1:] != h["seq_idx"][:-1])
    return np.bincount(motif[new], minlength=n_pwms).astype(np.int64)


# ---------------------------------------------------------------------------------------------------------------- de-dup --

@pytest.mark.parametrize("name", rc.SMALL_DEDUP + rc.ROUNDING)
def test_dedup_equals_the_literal_recurrence(name):
    c = rc.dedup_cases()[name]
    want = rc.filtered(c, c["keep"])
    P = len(c["widths"])
    res, pw = result_of(c), pwms_of(c)
    try:
        counts = res.region_counts()
        assert np.array_equal(counts, recount_regions(c, P))
        assert_hits(res.hits_pageable(), c, "before de-dup")
        res.dedup(pw)
        assert res.n_hits == int(c["keep"].sum())
        assert np.array_equal(res.motif_offsets, want["motif_offsets"]), (res.motif_offsets.tolist()[:12], want["motif_offsets"].tolist()[:12])
        read_every_way(res, want, rc.fits12(c), "after de-dup")
        assert np.array_equal(res.region_counts(), counts) and np.array_equal(counts, recount_regions(want, P))
        res.dedup(pw)                                            # a second de-dup changes nothing
        assert np.array_equal(res.motif_offsets, want["motif_offsets"])
        read_every_way(res, want, rc.fits12(c), "after a second de-dup")
        assert np.array_equal(res.region_counts(), counts)
    finally:
        res.close()
        pw.close()


@pytest.mark.parametrize("name", rc.SMALL_DEDUP + rc.ROUNDING)
def test_site_tables_before_and_after_dedup(name):
    c = rc.dedup_cases()[name]
    R = c["n_regions"]
    res, pw = result_of(c), pwms_of(c)
    try:
        for keep in (None, c["keep"]):
            if keep is not None:
                res.dedup(pw)
            want_n, want_max = rc.site_tables_expected(c, keep)
            got_n, got_max = res.site_tables(R)
            what = "before" if keep is None else "after"
            assert got_n.dtype == np.int32 and np.array_equal(got_n, want_n), (what, np.argwhere(got_n != want_n)[:8].tolist())
            assert same_bits(got_max, want_max), (what, np.argwhere(got_max.view(np.uint64) != want_max.view(np.uint64))[:8].tolist())
            assert np.array_equal(res.region_counts(), (want_n > 0).sum(axis=1))
    finally:
        res.close()
        pw.close()


# --------------------------------------------------------------------------------------------------------- compact forms --

@pytest.mark.parametrize("name", list(rc.compact_cases()))
def test_compact_forms_accept_what_fits_and_refuse_the_next_position(name):
    c = rc.compact_cases()[name]
    n = len(c["pos"])
    res = result_of(c)
    try:
        assert res.packed_form() == 0
        for form in (12, 16):
            if not c["accept%d" % form]:
                with pytest.raises(ValueError):
                    res.hits(packed=form)
                with pytest.raises(ValueError):
                    res.packed_words(form)
                continue
            coord, score, shift = res.packed_words(form)
            assert res.packed_form() == form
            if form == 12:
                assert coord.dtype == np.uint32 and (shift == c["shift"] if n else 1 <= shift <= 31)
                assert np.array_equal(coord, rc.encode12(c, shift)), np.flatnonzero(coord != rc.encode12(c, shift))[:8].tolist()
            else:
                assert coord.dtype == np.uint64 and shift == 0
                assert np.array_equal(coord, rc.encode16(c)), np.flatnonzero(coord != rc.encode16(c))[:8].tolist()
            assert same_bits(score, c["score"])
            assert_hits(res.hits(packed=form), c, f"hits(packed={form})")
        # refused or not, the result stays fully usable
        assert_hits(res.hits(copy=False), c, "hits(copy=False) afterwards")
        assert_hits(res.hits_pageable(), c, "ms_result_hits afterwards")
        assert res.n_hits == n and np.array_equal(res.motif_offsets, c["motif_offsets"])
        assert np.array_equal(res.region_counts(), recount_regions(c, len(c["widths"])))
        if c["n_regions"] <= 300:
            want_n, want_max = rc.site_tables_expected(c)
            got_n, got_max = res.site_tables(c["n_regions"])
            assert np.array_equal(got_n, want_n) and same_bits(got_max, want_max)
    finally:
        res.close()


@pytest.mark.parametrize("name", ["empty", "one_hit"] + list(rc.ROUNDING))
def test_compact_forms_at_the_hit_counts_either_side_of_the_rounding(name):
    """0, 1, 65 535, 65 536 and 65 537 hits (after de-dup) and 65 536 / 65 540 (before it) in each of the three forms"""
    c = rc.compact_cases()[name] if name in ("empty", "one_hit") else rc.dedup_cases()[name]
    res, pw = result_of(c), pwms_of(c)
    try:
        read_every_way(res, c, True, "as uploaded")
        if "keep" in c:
            res.dedup(pw)
            assert res.n_hits in (rc.ROUND - 1, rc.ROUND, rc.ROUND + 1)
            want = rc.filtered(c, c["keep"])
            coord, score, shift = res.packed_words(12)
            assert shift == rc.twelve_shift(c["n_regions"]) and np.array_equal(coord, rc.encode12(want, shift)) and same_bits(score, want["score"])
            coord, score, shift = res.packed_words(16)
            assert shift == 0 and np.array_equal(coord, rc.encode16(want)) and same_bits(score, want["score"])
    finally:
        res.close()
        pw.close()


# ----------------------------------------------------------------------------------------------------------- transitions --

ACCESSORS = ("plain", 16, 12)
FORM_OF = {"plain": 0, 16: 16, 12: 12}


def fetch(res, which, views):
    h = res.hits(copy=not views, motif=False) if which == "plain" else res.hits(packed=which)
    return {k: h[k] for k in ARRAYS + ("motif_offsets",)}


@pytest.mark.parametrize("views", [False, True], ids=["copies", "views"])
@pytest.mark.parametrize("name", ["seams", "sixteen_corners", "sixteen_refused_at_128"])
def test_every_accessor_after_every_other_returns_what_it_returned_before(name, views):
    """The three accessors refill ONE pinned buffer.  For every ordered pair (first, second) of (plain, 16-byte, 12-byte): first, then
    second -- which succeeds or is refused, and a refused call has overwritten the buffer all the same -- then first again must give
    the arrays it gave before.  `seams` fits every form, `sixteen_corners` not the 12-byte one, `sixteen_refused_at_128` neither compact
    form.  views: the plain arrays as hits(copy=False) views, fetched again after the second call (a view taken before it is void: the
    documented contract); copies: hits() arrays, which must stay what they were whatever is asked for later."""
    c = rc.dedup_cases()[name] if name == "seams" else rc.compact_cases()[name]
    accepted = {"plain": True, 16: rc.fits16(c), 12: rc.fits12(c)}
    assert (name == "seams") == accepted[12] and (name != "sixteen_refused_at_128") == accepted[16]
    res = result_of(c)
    state = {"form": 0, "cached": False}

    def call(which, what):
        """fetch, or None where the form is refused; afterwards packed_form() must name what the pinned buffer holds now"""
        no_call = which == "plain" and not views and state["cached"]      # hits() hands out the copies it made the first time
        if accepted[which]:
            got = fetch(res, which, views)
        else:
            with pytest.raises(ValueError):
                fetch(res, which, views)
            got = None
        if not no_call:
            state["form"] = FORM_OF[which] if accepted[which] else 0      # a refused call leaves no form in the buffer
            state["cached"] = state["cached"] or (which == "plain" and not views)
        assert res.packed_form() == state["form"], what
        return got

    try:
        for first in ACCESSORS:
            for second in ACCESSORS:
                if second == first:
                    continue
                what = f"{first}, {second}, {first}"
                got = call(first, what + ": the first call")
                if got is not None:
                    before = {k: np.array(v, copy=True) for k, v in got.items()}
                    assert_hits(before, c, what + ": the first call")
                then = call(second, what + ": the second call")
                if then is not None:
                    assert_hits(then, c, what + ": the second call")
                again = call(first, what + ": the first call again")
                if got is None:
                    assert again is None
                    assert_hits(fetch(res, "plain", True), c, what + ": the plain arrays after the refusals")
                    state["form"] = 0
                    continue
                assert_hits(again, before, what + ": the first call again")
                if not views or first != "plain":
                    assert_hits(got, before, what + ": arrays handed out as copies have changed")
        assert_hits(res.hits_pageable(), c, "ms_result_hits at the end")
    finally:
        res.close()


# ---------------------------------------------------------------------------------------------------- de-dup under a stream --

def test_stream_dedup_with_the_twelve_byte_copy_out():
    """MS_STREAM_DEDUP | MS_STREAM_PACKED12: ms_result_dedup frees the coordinate words the scan made of the hits before
    de-duplication (coord_blk), and the copy-out stage packs the kept hits on demand."""
    vals, widths, cutoffs = synth.load_motif_set(rc.STREAM_MOTIFS)
    pw = _lib.PwmSet(vals, widths, cutoffs)
    batches = rc.stream_batches()
    dropped = 0
    try:
        stream = _lib.scan_stream(pw, iter(batches), 3, _lib.MS_STREAM_DEDUP, packed=12)
        for (bases, offsets), res in zip(batches, stream):
            sq = _lib.SeqSet(bases, offsets)
            single = _lib.scan(pw, sq, 3)
            h = single.hits()
            keep = _lib.dedup_keep(h["motif_offsets"], widths, h["seq_idx"], h["pos"], h["score"], h["strand"])
            want = rc.filtered(h, keep)
            dropped += int((~keep).sum())
            try:
                assert res.packed_form() == 12
                assert res.n_hits == int(keep.sum())
                assert_hits(res.hits(packed=True), want, "the stream's batch")
                assert res.packed_form() == 12
                assert_hits(res.hits(), want, "the stream's batch, plain arrays")
                assert np.array_equal(res.region_counts(), single.region_counts())
            finally:
                res.close()
                single.close()
                sq.close()
        assert dropped >= rc.STREAM_MIN_DROPPED                  # the repeats did make sites overlap
    finally:
        pw.close()
