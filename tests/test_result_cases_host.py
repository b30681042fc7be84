"""
CPU-only: the cases of tests/result_cases.py held to their conditions before tests/test_gpu_result_boundaries.py puts them in front of
ms_result.hip's kernels -- every case is in ms_result order with unique keys, the cases together meet result_cases.CONDITIONS, the host
restatement ms_dedup_hits gives the literal keep flags (oracle.deduplicate_motif_sites on every (motif, region)), the expected compact
words decode to the case's arrays, and the entry points refuse NULL handles.  No GPU.
"""
import ctypes

import numpy as np

import result_cases as rc
from motifscan_amd import _lib


def test_constants_are_the_sources():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "motifscan_amd", "csrc", "ms_result.hip")).read()
    for kernel in ("dedup_kernel", "compact_hits_kernel", "site_tables_kernel", "pack_hits_kernel"):
        assert re.search(r"__launch_bounds__\(%d\) %s\(" % (rc.BLOCK, kernel), text), kernel
    assert text.count("(n + %d) / %d" % (rc.BLOCK - 1, rc.BLOCK)) >= 4
    assert text.count("(n + %d) & ~(size_t) %d" % (rc.ROUND - 1, rc.ROUND - 1)) >= 5         # result_block_bytes, result_carve, three accessors


def test_every_case_is_in_result_order_with_unique_keys():
    for name, c in {**rc.dedup_cases(), **rc.compact_cases()}.items():
        assert rc.order_problems(c) == [], name
    assert set(rc.SMALL_DEDUP + rc.ROUNDING) == set(rc.dedup_cases())


def test_the_cases_meet_the_conditions():
    total = {}
    for c in rc.dedup_cases().values():
        rc.add_tally(total, rc.tally_of(c, c["keep"]))
    for c in rc.compact_cases().values():
        rc.add_tally(total, c["tally"])
    print({k: total.get(k, 0) for k in rc.CONDITIONS})
    assert len(rc.GAP_CELLS) == 18
    assert rc.unmet_conditions(total) == []


def test_what_the_families_promise_beside_the_tallies():
    d = rc.dedup_cases()
    # rounding: more than ROUND hits with ROUND - 1, ROUND, ROUND + 1 survivors; exactly ROUND hits that all survive
    assert [(len(d[k]["keep"]) > rc.ROUND, int(d[k]["keep"].sum()) - rc.ROUND) for k in rc.ROUNDING[:3]] == [(True, -1), (True, 0), (True, 1)]
    assert len(d["round_all_survive"]["keep"]) == rc.ROUND and d["round_all_survive"]["keep"].all()
    assert d["nothing_dropped"]["keep"].all() and len(d["nothing_dropped"]["keep"]) > 0
    assert len(d["empty"]["keep"]) == 0 and len(d["empty"]["widths"]) == 3 and d["empty"]["n_regions"] == 5
    assert len(d["single_motif"]["widths"]) == 1
    # segments of 1, 255, 256, 257 and 513 hits; one of 513 from a block's last thread on
    seams = d["seams"]
    seg = rc.segments(seams)
    assert {1, 255, 256, 257, 513} <= {e - s for _, s, e in seg}
    assert any(e - s == 513 and s % rc.BLOCK == rc.BLOCK - 1 and (e - 1) // rc.BLOCK - s // rc.BLOCK == 2 for _, s, e in seg)
    assert 0 < seams["keep"].sum() < len(seams["keep"])
    # chains of 2, 3, 17 and 300 sites: only the last survives the ascending ones; only the first the descending and the constant ones
    # that lie within one width of it (a longer one starts again with the first site a width away: the recurrence compares with the kept
    # site, not with the neighbour)
    fam = d["families"]
    first_only, last_only = set(), set()
    for p, s, e in rc.segments(fam):
        k = fam["keep"][s:e]
        if k.sum() == 1 and (fam["strand"][s:e] == fam["strand"][s]).all():
            (first_only if k[0] else last_only).add(e - s)
    assert {2, 3, 17} <= first_only and set(rc.CHAIN_LENGTHS) <= last_only
    # empty motifs first, in the middle, two in a row, last
    n_per = np.diff(d["motif_edges"]["motif_offsets"])
    assert n_per[0] == 0 and n_per[3] == 0 and n_per[6] == 0 and n_per[7] == 0 and n_per[-1] > 0
    for k, last in (("motif_edges_last_dropped", False), ("motif_edges_last_kept", True)):
        assert np.diff(d[k]["motif_offsets"])[-2:].tolist() == [0, 0] and bool(d[k]["keep"][-1]) == last
    # the sites either side of a motif edge in one region would merge if the edge were not there
    c = d["motif_edges"]
    cut = {k: c[k][2:7] for k in ("seq_idx", "pos", "score", "strand")}
    cut.update(motif_offsets=np.array([0, 5]), widths=np.array([33], dtype=np.int32), n_regions=12)
    assert rc.order_problems(cut) == [] and rc.literal_keep(cut).sum() < c["keep"][2:7].sum()


def test_host_dedup_equals_the_literal_recurrence():
    for name, c in rc.dedup_cases().items():
        got = _lib.dedup_keep(c["motif_offsets"], c["widths"], c["seq_idx"], c["pos"], c["score"], c["strand"])
        assert np.array_equal(got, c["keep"]), (name, np.flatnonzero(got != c["keep"])[:8].tolist())
        f = rc.filtered(c, c["keep"])
        assert f["motif_offsets"][-1] == c["keep"].sum() == len(f["pos"])


def test_site_tables_expected_are_counts_and_maxima():
    c = rc.dedup_cases()["motif_edges"]
    for keep in (None, c["keep"]):
        n_sites, max_score = rc.site_tables_expected(c, keep)
        sel = np.ones(len(c["pos"]), dtype=bool) if keep is None else keep
        assert n_sites.sum() == sel.sum() and n_sites.shape == max_score.shape == (9, 12)
        assert np.array_equal(np.isnan(max_score), n_sites == 0)
        assert n_sites[0].sum() == 0 and n_sites[8, 0] == (4 if keep is None else 2) and max_score[8, 11] == 2.0


def test_compact_words_decode_to_the_arrays():
    for name, c in rc.compact_cases().items():
        if c["accept16"]:
            seq, pos, strand = rc.decode16(rc.encode16(c))
            assert np.array_equal(seq, c["seq_idx"]) and np.array_equal(pos, c["pos"]) and np.array_equal(strand, c["strand"]), name
        else:
            assert (c["pos"] >= 2 ** 31).sum() == 1 and c["pos"].max() == 2 ** 31, name
        assert c["shift"] == rc.twelve_shift(c["n_regions"])
        if c["accept12"]:
            w = rc.encode12(c, c["shift"])
            seq, pos, strand = rc.decode12(w, c["shift"])
            assert np.array_equal(seq, c["seq_idx"]) and np.array_equal(pos, c["pos"]) and np.array_equal(strand, c["strand"]), name
        elif name.startswith("twelve_refused"):
            assert (c["pos"] >> (c["shift"] - 1) != 0).sum() == 1 and c["pos"].max() == 2 ** (c["shift"] - 1), name
    cc = rc.compact_cases()
    assert [rc.twelve_shift(R) for R in rc.TWELVE_R] == [31, 31, 30, 30, 29, 24, 23, 16, 15, 12, 11]
    for R in rc.TWELVE_R:
        c = cc[f"twelve_accepted_R{R}"]
        w = rc.encode12(c, c["shift"])
        # region R - 1, the last position that fits, '-': every bit below the region's is set, every bit of the word where R is a power of two
        assert w[-1] & np.uint32((1 << c["shift"]) - 1) == (1 << c["shift"]) - 1 and w[-1] >> np.uint32(c["shift"]) == R - 1
        if R >= 2 and R & (R - 1) == 0:
            assert w[-1] == 0xFFFFFFFF
        assert not cc[f"twelve_refused_R{R}"]["accept12"] and cc[f"twelve_refused_R{R}"]["accept16"]
    corners = cc["sixteen_corners"]
    for s in (1, 2):
        assert {0, 1, 2 ** 31 - 2, 2 ** 31 - 1} <= set(corners["pos"][corners["strand"] == s].tolist())
    assert len(corners["pos"]) == 257 and not corners["accept12"]
    assert [int(np.argmax(cc[f"sixteen_refused_at_{k}"]["pos"])) for k in (0, 128, 256)] == [0, 128, 256]


def test_stream_batches_hold_overlapping_sites(oracle):
    from motifscan_amd import synth
    vals, widths, cutoffs = synth.load_motif_set(rc.STREAM_MOTIFS)
    dropped = 0
    for bases, offsets in rc.stream_batches():
        h = oracle.scan_arrays(vals, widths, cutoffs, bases.tobytes(), offsets, 3, 4)
        keep = _lib.dedup_keep(h["motif_offsets"], widths, h["seq_idx"], h["pos"], h["score"], h["strand"])
        case = dict(h, widths=np.asarray(widths), n_regions=len(offsets) - 1, strand=h["strand"].astype(np.int8))
        assert rc.order_problems(case) == [] and np.array_equal(rc.literal_keep(case), keep)
        dropped += int((~keep).sum())
    assert dropped >= rc.STREAM_MIN_DROPPED, dropped


def test_result_entry_points_refuse_null_handles():
    L = _lib.lib()
    bad = _lib.MS_ERR_INVALID
    out32, shift = ctypes.c_int32(), ctypes.c_int32()
    pc64, pc32, pv = ctypes.POINTER(ctypes.c_uint64)(), ctypes.POINTER(ctypes.c_uint32)(), ctypes.POINTER(ctypes.c_double)()
    assert L.ms_result_dedup(None, None) == bad
    assert L.ms_result_site_tables(None, None, None) == bad
    assert L.ms_result_hits_packed_host(None, ctypes.byref(pc64), ctypes.byref(pv)) == bad
    assert L.ms_result_hits_packed12_host(None, ctypes.byref(pc32), ctypes.byref(pv), ctypes.byref(shift)) == bad
    assert L.ms_result_packed_form(None, ctypes.byref(out32)) == bad
    assert L.ms_result_hits_host(None, None, None, None, None) == bad
    assert L.ms_result_hits(None, None, None, None, None) == bad
    assert b"NULL" in L.ms_last_error()
