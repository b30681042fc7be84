"""
The host arithmetic of the bucketed hit list (ms_scan_geom.cpp, through ms_debug_bucket_plan; no GPU): a long predicted-size scan has its
fp64 stage write the hits in 256 buckets of the radix digit d0 = (key >> L) & 255, so that the hit sort can skip its pass over that digit.

  weights   the (motif, window start) pairs whose key falls into each bucket, from the set's offsets, the motif widths and the key layout
  need_b    expected count e_b = mu * w_b / sum(w) plus 6 sigma of a Poisson count: ceil(e_b + 6 sqrt(e_b + 1)) + 1, 0 for an empty bucket
  gate      every condition of the form, and sum(need_b) <= n_pred: the slack fits inside the prediction's own margin
  cap_b     need_b + the bucket's share of n_pred - sum(need_b), cut off where the running sum would pass n_pred
"""
import math

import numpy as np
import pytest

from motifscan_amd import _lib

C4 = dict(gbits=29, pbits=9, end_bit=40, low_bits=16, n_pwms=579, n_regions=1_000_000)          # a million 500-base regions x 579 motifs


@pytest.fixture(scope="module", autouse=True)
def built():
    import os
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()


def n_pred_of(mu, margin=0.04):
    """the predicted list size of scan_locked"""
    return int(min(mu * (1.0 + margin) + 6.0 * math.sqrt(mu + 1.0) + 256.0, 3.0e9))


def need_of(w, mu):
    tot = int(w.sum())
    e = [mu * float(x) / float(tot) if tot else 0.0 for x in w]
    return e, [int(math.ceil(x + 6.0 * math.sqrt(x + 1.0))) + 1 if wb else 0 for x, wb in zip(e, w)]


def weight_sets():
    rng = np.random.default_rng(3)
    uniform = np.full(256, 3_906_250 * 480, dtype=np.uint64)
    c4 = uniform.copy()
    c4[:9] += np.uint64(64 * 480 * 579)                          # 15 625 stripes of 64 regions over 256 buckets: nine carry one more
    dominant = np.full(256, 1000, dtype=np.uint64)
    dominant[17] = 10 ** 11
    holes = uniform.copy()
    holes[rng.random(256) < 0.6] = 0
    one = np.zeros(256, dtype=np.uint64)
    one[255] = 12345
    ragged = rng.integers(1, 10 ** 9, size=256).astype(np.uint64)
    return {"uniform": uniform, "c4": c4, "dominant": dominant, "holes": holes, "one": one, "ragged": ragged}


@pytest.mark.parametrize("name", list(weight_sets()))
def test_capacities_fit_the_list_and_cover_six_sigma(name):
    w = weight_sets()[name]
    for mu in (0.0, 3.0, 2.3e4, 1.0e6, 5.8e7, 2.0e9):
        for n_pred in (n_pred_of(mu), n_pred_of(mu, 0.5), max(1, int(mu / 2)), 0):
            for cap_max in (None, 40):
                got = _lib.bucket_plan(mu, n_pred, weights=w, cap_max=cap_max, **C4)
                e, need = need_of(w, mu)
                base, cap = got["base"].astype(object), got["cap"].astype(object)
                assert got["need"] == sum(need)
                assert int(cap.sum()) <= n_pred
                assert all(int(base[b]) + int(cap[b]) <= int(base[b + 1]) for b in range(255)) and int(base[255]) + int(cap[255]) <= n_pred
                assert all(int(cap[b]) == 0 for b in range(256) if w[b] == 0)          # no key can fall there
                if cap_max is not None:
                    assert int(cap.max()) <= cap_max
                assert got["gate"] == (sum(need) <= n_pred)
                if got["gate"] and cap_max is None:
                    for b in range(256):
                        if w[b]:
                            assert int(cap[b]) >= e[b] + 6.0 * math.sqrt(e[b] + 1.0), (name, mu, b)


def test_gate_threshold_follows_from_the_slack_formula():
    """256 equal buckets at the settled 4 % margin: the gate opens where the sum of the buckets' 6-sigma needs first fits into the margin --
    about 36 / 0.04^2 = 22 500 expected hits per bucket -- and not a hit sooner."""
    w = weight_sets()["uniform"]

    def fits(mu):
        return sum(need_of(w, mu)[1]) <= n_pred_of(mu)
    lo, hi = 1.0e5, 1.0e8
    assert not fits(lo) and fits(hi)
    while hi - lo > 1.0:
        mid = math.floor((lo + hi) / 2)
        lo, hi = (lo, mid) if fits(mid) else (mid, hi)
    assert 4.5e6 < hi < 6.5e6
    for mu in (hi * 0.5, hi - 65536, hi + 65536, hi * 2, 5.8e7):
        assert _lib.bucket_plan(mu, n_pred_of(mu), weights=w, **C4)["gate"] == fits(mu) == (mu > hi)
    # the benchmark's default line (5.8e7 hits per scan) passes with the initial 6 % margin and with the settled one
    assert _lib.bucket_plan(5.8e7, n_pred_of(5.8e7, 0.06), weights=weight_sets()["c4"], **C4)["gate"]
    assert _lib.bucket_plan(5.8e7, n_pred_of(5.8e7), weights=weight_sets()["c4"], **C4)["gate"]


def test_gate_declines_every_excluded_form():
    w, mu = weight_sets()["c4"], 5.8e7
    n_pred = n_pred_of(mu)
    ok = dict(C4)
    assert _lib.bucket_plan(mu, n_pred, weights=w, **ok)["gate"]
    for form in (dict(predicted=False), dict(counts_only=True), dict(carry_only=False), dict(sticky_off=True), dict(force=0)):
        assert not _lib.bucket_plan(mu, n_pred, weights=w, **ok, **form)["gate"], form
    for layout in (dict(pbits=0), dict(low_bits=0), dict(end_bit=31),            # global-position keys; every bit by radix passes; < 8 bits left above the digit
                   dict(low_bits=24),                                             # the digit would reach into the motif bits
                   dict(low_bits=32, end_bit=64)):                                # beyond the coordinate field
        assert not _lib.bucket_plan(mu, n_pred, weights=w, **{**ok, **layout})["gate"], layout
    assert not _lib.bucket_plan(mu, n_pred, weights=np.zeros(256, dtype=np.uint64), **ok)["gate"]
    # forced on: any size -- but never a digit with motif bits in it, and never an excluded form
    small = 2.0e4
    assert not _lib.bucket_plan(small, n_pred_of(small), weights=w, **ok)["gate"]
    assert _lib.bucket_plan(small, n_pred_of(small), weights=w, force=1, **ok)["gate"]
    assert _lib.bucket_plan(small, n_pred_of(small), weights=w, force=1, gbits=23, pbits=8, end_bit=30, low_bits=16, n_pwms=50, n_regions=16411)["gate"]
    assert _lib.bucket_plan(small, n_pred_of(small), weights=w, force=1, gbits=19, pbits=8, end_bit=26, low_bits=8, n_pwms=50, n_regions=2003)["gate"]
    assert not _lib.bucket_plan(small, n_pred_of(small), weights=w, force=1, gbits=19, pbits=8, end_bit=26, low_bits=16, n_pwms=50, n_regions=2003)["gate"]
    assert not _lib.bucket_plan(small, n_pred_of(small), weights=w, force=1, gbits=12, pbits=6, end_bit=19, low_bits=8, n_pwms=50, n_regions=40)["gate"]
    assert not _lib.bucket_plan(small, n_pred_of(small), weights=w, force=1, counts_only=True, **ok)["gate"]
    assert not _lib.bucket_plan(small, n_pred_of(small), weights=w, force=1, sticky_off=True, **ok)["gate"]
    # a hit key that is all ones in the bits the passes sort would tie with the padding keys in front of it: 1024 motifs x 2^20 regions
    full = dict(ok, n_pwms=1024, n_regions=1 << 20)
    assert not _lib.bucket_plan(mu, n_pred, weights=w, **full)["gate"] and not _lib.bucket_plan(mu, n_pred, weights=w, force=1, **full)["gate"]
    assert _lib.bucket_plan(mu, n_pred, weights=w, **dict(full, n_regions=(1 << 20) - (1 << 14)))["gate"]
    assert _lib.bucket_plan(mu, n_pred, weights=w, **dict(full, n_pwms=1023))["gate"]


def brute_weights(offsets, widths, gbits, pbits, low_bits):
    w = np.zeros(256, dtype=np.uint64)
    for m, width in enumerate(widths):
        for r in range(len(offsets) - 1):
            n = int(offsets[r + 1] - offsets[r])
            for p in range(max(n - int(width) + 1, 0)):
                key = (m << (gbits + 1)) | (((r << pbits) | p) << 1)
                w[(key >> low_bits) & 255] += np.uint64(1)
    return w


@pytest.mark.parametrize("low_bits", [8, 9, 12, 16])
def test_weights_count_the_windows_of_every_bucket(low_bits):
    """against an enumeration of every (motif, region, window start): digits made of position and region bits (L = 8) and of region bits
    only (L = 9 and up); regions shorter than a motif, empty regions, a region
    count that is no multiple of the stripe."""
    rng = np.random.default_rng(low_bits)
    lens = rng.integers(0, 200, size=101)
    lens[[5, 77]] = 0
    lens[[6, 100]] = 3
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    widths = rng.integers(5, 31, size=19).astype(np.int32)
    gbits, pbits = 15 + 8, 8                                    # (as if the set had 2^15 regions: the digit stays inside the coordinate)
    got = _lib.bucket_plan(1000.0, 5000, offsets=offsets, widths=widths, gbits=gbits, pbits=pbits, end_bit=gbits + 1 + 6, low_bits=low_bits, force=1)
    want = brute_weights(offsets, widths, gbits, pbits, low_bits)
    assert np.array_equal(got["weights"], want)
    assert int(want.sum()) == sum(max(int(n) - int(wd) + 1, 0) for n in lens for wd in widths)


def test_c4_weights_are_striped_by_64_regions():
    """the benchmark's default geometry: 2^20-aligned or not, d0 is region bits 6 ... 13 -- stripes of 64 regions dealt round-robin"""
    R, n, widths = 100_000, 500, np.array([8, 12, 30], dtype=np.int32)
    offsets = (np.arange(R + 1, dtype=np.int64) * n)
    got = _lib.bucket_plan(1.0e6, n_pred_of(1.0e6), offsets=offsets, widths=widths, gbits=17 + 9, pbits=9, end_bit=17 + 9 + 1 + 2, low_bits=16)
    per_region = sum(n - int(w) + 1 for w in widths)
    stripes = np.bincount((np.arange(R) >> 6) & 255, minlength=256)
    assert np.array_equal(got["weights"], (stripes * per_region).astype(np.uint64))
