"""
The host side of the motif-pair reductions (ms_result_cooccurrence, ms_result_pair_spacing; motifscan_amd.pairs): the contract restated in
numpy as brute force per region -- tests/test_gpu_pairs.py compares the device against these --, the restatements themselves against a
hand-written case, the strand folding of pairs.py against a brute force that reflects the coordinates of every pair whose anchor lies on
'-', and what the library says without a device.  No GPU.
"""
import ctypes
import os
import re

import numpy as np
import pytest

from motifscan_amd import _lib, pairs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# --------------------------------------------------------------------------------------------------- the restatements --

def np_cooccurrence(offsets, seq_idx, P, R):
    """int64 [P][P]: regions that hold a site of motif a and a site of motif j, region by region."""
    has = np.zeros((P, R), dtype=np.int64)
    has[np.repeat(np.arange(P), np.diff(offsets)), seq_idx] = 1
    out = np.zeros((P, P), dtype=np.int64)
    for r in range(R):
        out += np.outer(has[:, r], has[:, r])
    return out


def np_pair_spacing(offsets, seq_idx, pos, strand, widths, anchor, max_dist):
    """(counts int64 [P][4][2 * max_dist + 1], n_pairs int64 [P]) of motif `anchor` against every motif: per region, every site of the
    anchor against every site of every motif (itself excepted) -- t2 = 2 * (pos_t - pos_s) + Wj - Wa, counted iff |t2| <= 2 * max_dist in
    bin (t2 + 2 * max_dist) >> 1, orientation 2 * (strand_s - 1) + (strand_t - 1); n_pairs counts the pairs at any distance."""
    offsets, seq_idx, pos = np.asarray(offsets, dtype=np.int64), np.asarray(seq_idx, dtype=np.int64), np.asarray(pos, dtype=np.int64)
    strand, widths = np.asarray(strand, dtype=np.int64), np.asarray(widths, dtype=np.int64)
    P, D2 = len(offsets) - 1, 2 * max_dist
    counts = np.zeros((P, 4, D2 + 1), dtype=np.int64)
    n_pairs = np.zeros(P, dtype=np.int64)
    motif = np.repeat(np.arange(P), np.diff(offsets))
    index = np.arange(len(seq_idx))
    a_idx = index[offsets[anchor]:offsets[anchor + 1]]
    for r in np.unique(seq_idx[a_idx]):
        s_all = a_idx[seq_idx[a_idx] == r]
        t = index[seq_idx == r]
        for c in range(0, len(s_all), 512):                      # bounded temporaries for a region of thousands of sites
            s = s_all[c:c + 512]
            other = s[:, None] != t[None, :]
            t2 = 2 * (pos[t][None, :] - pos[s][:, None]) + (widths[motif[t]] - widths[anchor])[None, :]
            o = 2 * (strand[s][:, None] - 1) + (strand[t][None, :] - 1)
            m = np.broadcast_to(motif[t][None, :], t2.shape)
            n_pairs += np.bincount(m[other], minlength=P)
            keep = other & (np.abs(t2) <= D2)
            np.add.at(counts, (m[keep], o[keep], (t2[keep] + D2) >> 1), 1)
    return counts, n_pairs


def hit_arrays(per_motif):
    """(offsets, seq_idx, pos, strand) in ms_result order from one [n][3] array of (region, position, strand) per motif."""
    rows, offsets = [], [0]
    for h in per_motif:
        h = np.asarray(h, dtype=np.int64).reshape(-1, 3)
        rows.append(h[np.lexsort((h[:, 2], h[:, 1], h[:, 0]))])
        offsets.append(offsets[-1] + len(h))
    flat = np.concatenate(rows) if rows else np.zeros((0, 3), dtype=np.int64)
    return np.array(offsets, dtype=np.int64), flat[:, 0].copy(), flat[:, 1].copy(), flat[:, 2].astype(np.int8)


def random_hits(rng, n_regions, n_sites, max_pos):
    """[n][3] distinct (region, position, strand) triples, n <= n_sites."""
    h = np.stack([rng.integers(0, n_regions, n_sites), rng.integers(0, max_pos, n_sites), rng.integers(1, 3, n_sites)], axis=1)
    return np.unique(h, axis=0)


# ------------------------------------------------------------------------------------------------------------ the tests --

HAND = hit_arrays([
    [(0, 10, 1), (0, 10, 2), (0, 12, 1), (2, 5, 2)],                       # motif 0, width 4: the anchor
    [(0, 9, 1), (0, 12, 2), (1, 10, 1), (2, 3, 1), (2, 6, 2)],            # motif 1, width 6: W - Wa even
    [(0, 11, 2), (1, 0, 1), (1, 1, 1)],                                    # motif 2, width 5: W - Wa odd
])
HAND_WIDTHS = [4, 6, 5]


def test_restatements_on_a_hand_written_case():
    offsets, seq_idx, pos, strand = HAND
    assert offsets.tolist() == [0, 4, 9, 12]
    assert np_cooccurrence(offsets, seq_idx, 3, 3).tolist() == [[2, 2, 1], [2, 3, 2], [1, 2, 2]]
    counts, n_pairs = np_pair_spacing(offsets, seq_idx, pos, strand, HAND_WIDTHS, 0, 2)
    # region 0 holds the anchor at (10 +), (10 -), (12 +); region 2 at (5 -).  Bins: t2 = -4, -2, 0, 2, 4 (even) / -3, -1, 1, 3, unused (odd)
    assert counts[0].tolist() == [[1, 0, 0, 0, 1],       # + / +: (12 +) -> (10 +) at -4, (10 +) -> (12 +) at +4
                                  [1, 0, 1, 0, 0],       # + / -: (12 +) -> (10 -) at -4, (10 +) -> its twin (10 -) at 0
                                  [0, 0, 1, 0, 1],       # - / +: (10 -) -> its twin at 0, (10 -) -> (12 +) at +4
                                  [0, 0, 0, 0, 0]]
    assert counts[1].tolist() == [[1, 0, 1, 0, 0],       # t2 = 2 * (q - p) + 2: (12 +) -> (9 +) at -4, (10 +) -> (9 +) at 0
                                  [0, 0, 0, 1, 0],       # (12 +) -> (12 -) at +2; (10 +-) -> (12 -) would be +6
                                  [0, 1, 1, 0, 0],       # (10 -) -> (9 +) at 0; region 2: (5 -) -> (3 +) at -2
                                  [0, 0, 0, 0, 1]]       # region 2: (5 -) -> (6 -) at +4
    assert counts[2].tolist() == [[0, 0, 0, 0, 0],       # t2 = 2 * (q - p) + 1, partner (11 -) in region 0
                                  [0, 1, 0, 1, 0],       # (12 +) at -1, (10 +) at +3
                                  [0, 0, 0, 0, 0],
                                  [0, 0, 0, 1, 0]]       # (10 -) at +3
    assert n_pairs.tolist() == [3 * 3 - 3 + 1 * 1 - 1, 3 * 2 + 1 * 2, 3 * 1]
    # max_dist = 0: only coinciding centres -- the strand twins of the anchor, the (9 +) partner of width 6 under the anchor at 10
    c0, n0 = np_pair_spacing(offsets, seq_idx, pos, strand, HAND_WIDTHS, 0, 0)
    assert c0[:, :, 0].tolist() == [[0, 1, 1, 0], [1, 0, 1, 0], [0, 0, 0, 0]] and np.array_equal(n0, n_pairs)


def reflected_brute_force(offsets, seq_idx, pos, strand, widths, anchor, max_dist):
    """int64 [P][2][2 * max_dist + 1] straight from the definition of `oriented`: a pair whose anchor site lies on '-' is looked at from
    the other strand -- every site interval [p, p + W) becomes [-p - W, -p) and every strand is swapped -- and then binned like any other;
    [0] partner on the anchor's strand, [1] on the opposite one."""
    P, D2 = len(offsets) - 1, 2 * max_dist
    out = np.zeros((P, 2, D2 + 1), dtype=np.int64)
    for s in range(offsets[anchor], offsets[anchor + 1]):
        for j in range(P):
            for t in range(offsets[j], offsets[j + 1]):
                if t == s or seq_idx[t] != seq_idx[s]:
                    continue
                ps, pt, ss, st = int(pos[s]), int(pos[t]), int(strand[s]), int(strand[t])
                if ss == 2:
                    ps, pt, ss, st = -ps - widths[anchor], -pt - widths[j], 1, 3 - st
                t2 = 2 * (pt - ps) + widths[j] - widths[anchor]
                if abs(t2) <= D2:
                    out[j, st - 1, (t2 + D2) >> 1] += 1
    return out


@pytest.mark.parametrize("max_dist", [0, 1, 6])
def test_oriented_folding_is_the_reflection_of_the_minus_anchors(max_dist):
    rng = np.random.default_rng(5 + max_dist)
    widths = [7, 9, 12, 7, 4]                                    # against anchor 0: even, odd, the same width, odd
    offsets, seq_idx, pos, strand = hit_arrays([random_hits(rng, 4, 40, 25) for _ in widths])
    for anchor in (0, 2):
        counts, _ = np_pair_spacing(offsets, seq_idx, pos, strand, widths, anchor, max_dist)
        diff = np.array(widths) - widths[anchor]
        want = reflected_brute_force(offsets, seq_idx, pos, strand, widths, anchor, max_dist)
        got = pairs.fold_orientations(counts, diff)
        assert got.shape == want.shape and np.array_equal(got, want)
        assert want.sum() == counts.sum() and (max_dist == 0 or want.sum() > 0)
        assert np.array_equal(pairs.fold_orientations(counts[1], diff[1]), want[1])        # one row, a scalar width difference
        assert not got[diff % 2 == 1, :, -1].any()               # an odd width difference leaves the last bin unused
    assert pairs.spacing_axis(2, 4).tolist() == [-2, -1, 0, 1, 2]
    assert pairs.spacing_axis(2, -3).tolist() == [-1.5, -0.5, 0.5, 1.5, 2.5]


def test_the_lds_bin_limit_is_a_constant_of_the_build():
    L = _lib.lib()
    n = L.ms_debug_pair_lds_bins()
    assert n == _lib.pair_lds_bins() > 0 and n % 2 == 1         # 2 * max_dist + 1 can sit exactly on it
    assert 16 * n <= 160 * 1024                                  # four orientations of 32-bit counters in a CU's LDS
    assert L.ms_debug_cooc_chunk_regions() == _lib.cooc_chunk_regions() > 0 and _lib.cooc_chunk_regions() % 64 == 0


def test_the_lds_pair_limit_hook_round_trips_without_a_device():
    assert _lib.pair_lds_pair_limit(12345) == 2 ** 32 - 1
    assert _lib.pair_lds_pair_limit(0) == 12345 and _lib.pair_lds_pair_limit(0) == 2 ** 32 - 1
    for bad in (-1, 2 ** 32):
        with pytest.raises(ValueError, match="limit"):
            _lib.pair_lds_pair_limit(bad)


def test_header_declares_the_pair_entry_points():
    with open(os.path.join(ROOT, "include", "motifscan_amd.h")) as fh:
        text = fh.read()
    table = text[:text.index("#ifndef MOTIFSCAN_AMD_H")]
    for name in ("ms_result_cooccurrence", "ms_result_pair_spacing"):
        assert re.search(rf"\bint\s+{name}\s*\(", text), name
        assert re.search(rf"{name}\s+no reference counterpart", table), name
        assert hasattr(_lib.lib(), name)
    with open(os.path.join(ROOT, "include", "motifscan_amd_debug.h")) as fh:
        assert re.search(r"\bint\s+ms_debug_pair_lds_bins\s*\(\s*void\s*\)", fh.read())


def test_null_handles_are_refused_before_any_device_is_touched():
    L = _lib.lib()
    buf = np.zeros(4, dtype=np.int64)
    assert L.ms_result_cooccurrence(None, 0, 1, ctypes.c_void_p(buf.ctypes.data)) == _lib.MS_ERR_INVALID
    assert L.ms_result_pair_spacing(None, None, 0, 0, 1, 10, _lib.ptr(buf, ctypes.c_int64), _lib.ptr(buf, ctypes.c_int64)) == _lib.MS_ERR_INVALID
    with pytest.raises(ValueError, match="NULL handle"):
        _lib.check(_lib.MS_ERR_INVALID)
