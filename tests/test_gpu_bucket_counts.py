"""
The digit counts of a bucketed hit list (BucketOut::hist, ms_kernels.h): the bucketed fp64 stage counts every hit its buckets hold by the
digits of the radix passes that are left, fill_tail_buckets_kernel adds the all-ones padding keys, and sort_hit_pairs_counted (ms_sort.hip)
runs the passes from those counts, without a histogram pass over the list.  Wrong counts scatter hits to wrong slots, so every case compares
hits, offsets and region counts with the oracle bit for bit, and with the same scans unbucketed (MS_ORDER_BUCKETS=0: rocPRIM's own histogram).

About a thousand regions of 500 bases under 40 motifs of mixed widths at L = 8: nine position and ten or eleven region bits, so the digit
is coordinate bits only, the passes that are left cover the bits 16 ... 25 or 26, and the last place is narrower than eight bits (the padding
keys count in its bin 2^bits - 1, not 255).  tests/test_gpu_bucketed_order.py has the empty buckets, the capped buckets, the direct path of a
full stage and the stream; here are the region counts around a power of two, the strand masks and a motif count the layout gate declines.

Measurement switches (honoured only with MS_MEASURE=1): MS_ORDER_BUCKETS, MS_SORT_LOW_BITS, MS_ORDER_BUCKET_CAP, MS_RESCORE_SORTED_MIN.
"""
import numpy as np
import pytest

from motifscan_amd import _lib, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def device():
    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests need an MI355X (there is no CPU fallback)")
    _lib.set_device(0)


def _set_env(monkeypatch, buckets, cap=None):
    monkeypatch.setenv("MS_MEASURE", "1")
    monkeypatch.setenv("MS_RESCORE_SORTED_MIN", "0")
    monkeypatch.setenv("MS_SORT_LOW_BITS", "8")
    monkeypatch.setenv("MS_ORDER_BUCKETS", str(buckets))
    if cap is None:
        monkeypatch.delenv("MS_ORDER_BUCKET_CAP", raising=False)
    else:
        monkeypatch.setenv("MS_ORDER_BUCKET_CAP", str(cap))


def _take(res):
    h = res.hits()
    out = {k: np.array(h[k]) for k in ("seq_idx", "pos", "strand", "score", "motif_offsets")}
    out["region_counts"] = np.asarray(res.region_counts(), dtype=np.int64).copy()
    st = res.stats()
    out["flags"] = (st["order_bucketed"], st["n_passes"])
    res.close()
    return out


def _same(got, want, what):
    for k in ("motif_offsets", "seq_idx", "pos", "score"):
        assert np.array_equal(got[k], want[k]), f"{what}: {k} differs"
    assert np.array_equal(got["strand"].astype(np.int32), want["strand"].astype(np.int32)), f"{what}: strand differs"
    if "region_counts" in want:
        assert np.array_equal(got["region_counts"], want["region_counts"]), f"{what}: region counts differ"


def _scans(monkeypatch, motifs, bases, offsets, strand, buckets, n=2, cap=None):
    _set_env(monkeypatch, buckets, cap)
    pw, sq = _lib.PwmSet(*motifs), _lib.SeqSet(bases, offsets)
    return [_take(_lib.scan(pw, sq, strand)) for _ in range(n)]       # the first scan of a set has no prediction and is never bucketed


@pytest.fixture(scope="module")
def data(oracle):
    motifs = {P: synth.load_motif_set(P, p_value="1e-3") for P in (40, 32)}
    regions = {R: synth.make_regions(R, 500, seed=R, frac_n=0.02) for R in (1023, 1024, 1025, 2000)}
    want = {}

    def get(P, R, strand):
        if (P, R, strand) not in want:
            bases, offsets = regions[R]
            want[P, R, strand] = oracle.scan_arrays(*motifs[P], bases.tobytes(), offsets, strand, 8)
        return motifs[P], regions[R][0], regions[R][1], want[P, R, strand]
    return get


@pytest.mark.parametrize("n_regions,strand", [(1023, 3), (1024, 3), (1025, 3), (2000, 1), (2000, 2), (2000, 3)])
def test_counted_passes_equal_oracle_and_plain(data, monkeypatch, n_regions, strand):
    motifs, bases, offsets, want = data(40, n_regions, strand)
    assert len(want["pos"]) > 10000
    plain = _scans(monkeypatch, motifs, bases, offsets, strand, 0)
    bucketed = _scans(monkeypatch, motifs, bases, offsets, strand, 1)
    assert [r["flags"] for r in plain] == [(0, 1), (0, 1)]
    assert bucketed[0]["flags"] == (0, 1) and bucketed[1]["flags"] in ((1, 1), (0, 2))      # (0, 2): a bucket overflowed, the scan was run again, plain
    for i, (p, b) in enumerate(zip(plain, bucketed)):
        _same(b, want, f"bucketed scan {i} against the oracle")
        _same(b, p, f"bucketed scan {i} against the plain one")


def test_power_of_two_motif_count_is_declined(data, monkeypatch):
    """32 motifs: the last motif's keys are all ones in the motif bits and would tie with the padding keys: the gate declines, forced or not"""
    motifs, bases, offsets, want = data(32, 1024, 3)
    bucketed = _scans(monkeypatch, motifs, bases, offsets, 3, 1)
    assert [r["flags"] for r in bucketed] == [(0, 1), (0, 1)]
    for i, b in enumerate(bucketed):
        _same(b, want, f"scan {i}")


def test_capped_buckets_fall_back_to_the_exact_rerun(data, monkeypatch):
    """Buckets of four slots: the second scan drops hits -- its counts still describe the list it sorts -- and is run again, plain"""
    motifs, bases, offsets, want = data(40, 1025, 3)
    runs = _scans(monkeypatch, motifs, bases, offsets, 3, 1, n=2, cap=4)
    assert [r["flags"] for r in runs] == [(0, 1), (0, 2)]
    for i, r in enumerate(runs):
        _same(r, want, f"scan {i}")


def test_a_list_far_below_one_stage(oracle, monkeypatch):
    """1030 regions of 120 bases: some ten thousand hits, a few chunks in all, so most blocks flush an empty stage and add no counts"""
    motifs = synth.load_motif_set(40, p_value="1e-3")
    bases, offsets = synth.make_regions(1030, 120, seed=5)
    want = oracle.scan_arrays(*motifs, bases.tobytes(), offsets, 3, 4)
    assert 100 < len(want["pos"]) < 20000
    plain = _scans(monkeypatch, motifs, bases, offsets, 3, 0)
    bucketed = _scans(monkeypatch, motifs, bases, offsets, 3, 1)
    assert bucketed[1]["flags"] in ((1, 1), (0, 2), (0, 1))
    for p, b in zip(plain, bucketed):
        _same(b, want, "against the oracle")
        _same(b, p, "against the plain scan")
