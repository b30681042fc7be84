"""
The host side of the dense allele scan (ms_scan_alleles_best; _lib.scan_alleles_best / AlleleBest, variants.best_alleles /
AlleleEffects): the views of an AlleleEffects on hand-made arrays, the argument errors that are raised before any device call, what
must fail loudly without a GPU, and the path constants the GPU tests size their cases from.  No GPU.
"""
import ctypes

import numpy as np
import pytest

from motifscan_amd import _lib, variants


def effects():
    """Two motifs x five variants, made by hand: an SNV, an insertion of 4 at 100, a deletion of 3 at 200, a 2 -> 5 replacement at 300,
    and a variant without a winner on either haplotype."""
    nan = np.nan
    pos, ref_len, alt_len = [10, 100, 200, 300, 50], [1, 0, 3, 2, 1], [1, 4, 0, 5, 1]
    score_ref = np.array([[0.5, 0.25, nan, 0.75, nan], [0.1, nan, 0.3, 0.4, nan]])
    score_alt = np.array([[0.75, 0.5, 0.25, nan, nan], [0.1, 0.9, 0.2, 0.6, nan]])
    offset_ref = np.array([[-3, -2, 0, 1, 0], [0, 0, 2, -5, 0]], dtype=np.int32)
    #   alt-haplotype starts: in front of the allele, inside the inserted bases, at the junction of a deletion, behind a longer allele
    offset_alt = np.array([[-3, 2, -1, 0, 0], [0, 4, 0, 4, 0]], dtype=np.int32)
    strand_ref = np.array([[1, 2, 0, 1, 0], [2, 0, 1, 1, 0]], dtype=np.int8)
    strand_alt = np.array([[1, 1, 2, 0, 0], [2, 1, 1, 2, 0]], dtype=np.int8)
    return variants.AlleleEffects(score_ref, score_alt, offset_ref, offset_alt, strand_ref, strand_alt, pos, ref_len, alt_len, skipped=[4])


def test_allele_effects_views_on_hand_made_arrays():
    e = effects()
    assert e.shape == (2, 5) and e.skipped.tolist() == [4]
    d = e.delta
    assert np.array_equal(np.isnan(d), [[False, False, True, True, True], [False, True, False, False, True]])
    assert d[0, 0] == 0.25 and d[0, 1] == 0.25 and d[1, 0] == 0.0 and d[1, 2] == 0.2 - 0.3 and d[1, 3] == 0.6 - 0.4
    assert e.start_ref().tolist() == [[7, 98, -1, 301, -1], [10, -1, 202, 295, -1]]
    assert e.start_alt().tolist() == [[7, 102, 199, -1, -1], [10, 104, 200, 304, -1]]
    # start 102 lies inside the four inserted bases of the insertion at 100 (r = 0): it has no reference base of its own -> 100;
    # start 104 = x + a is the first base behind them -> 100; start 199 is in front of the deletion; start 200 on the alt haplotype is
    # the first base behind the deleted three -> 203; start 304 lies inside the five alt bases of the 2 -> 5 replacement -> 300 + min(4, 2)
    assert e.start_alt_in_ref().tolist() == [[7, 100, 199, -1, -1], [10, 100, 203, 302, -1]]
    assert e.start_ref().dtype == np.int64 and e.start_alt_in_ref().dtype == np.int64

    behind = variants.AlleleEffects([[0.5]], [[0.5]], [[9]], [[9]], [[1]], [[2]], [3_000_000_000], [3], [0])
    assert behind.start_ref().tolist() == [[3_000_000_009]] and behind.start_alt().tolist() == [[3_000_000_009]]
    assert behind.start_alt_in_ref().tolist() == [[3_000_000_012]]          # behind a deletion of three
    empty = variants.AlleleEffects(np.zeros((3, 0)), np.zeros((3, 0)), np.zeros((3, 0)), np.zeros((3, 0)), np.zeros((3, 0)), np.zeros((3, 0)), [], [], [])
    assert empty.delta.shape == (3, 0) and empty.start_alt_in_ref().shape == (3, 0) and empty.skipped.size == 0


def test_start_alt_in_ref_is_ref_start_of_allele_sites():
    """The same rule as AlleleSites.ref_start, cell by cell."""
    rng = np.random.default_rng(3)
    V = 200
    pos = rng.integers(50, 1000, V)
    ref_len, alt_len = rng.integers(0, 8, V), rng.integers(0, 8, V)
    offset = rng.integers(-10, 9, (1, V)).astype(np.int32)
    strand = np.ones((1, V), dtype=np.int8)
    e = variants.AlleleEffects(np.zeros((1, V)), np.zeros((1, V)), offset, offset, strand, strand, pos, ref_len, alt_len)
    s = variants.AlleleSites(np.zeros(V, dtype=np.int32), np.arange(V), np.ones(V, dtype=np.uint8), pos + offset[0], np.ones(V, dtype=np.int8),
                             np.zeros(V), [0, V], pos=pos, ref_len=ref_len, alt_len=alt_len)
    assert np.array_equal(e.start_alt_in_ref()[0], s.ref_start())


def test_best_alleles_argument_errors_come_before_any_device_call():
    class Pwm:
        matrix = np.ones((4, 3))

    class Genome:                                                           # touching the device would need .h
        index = {"chr1": 0}
    g, p = Genome(), [Pwm()]
    with pytest.raises(ValueError, match="on_mismatch"):
        variants.best_alleles(g, p, ["chr1"], [3], ["A"], ["C"], on_mismatch="ignore")
    with pytest.raises(ValueError, match="strand"):
        variants.best_alleles(g, p, ["chr1"], [3], ["A"], ["C"], strand="plus")
    with pytest.raises(ValueError, match="motif_batch"):
        variants.best_alleles(g, p, ["chr1"], [3], ["A"], ["C"], motif_batch=0)
    with pytest.raises(ValueError, match="one entry per variant"):
        variants.best_alleles(g, p, ["chr1"], [3, 4], ["A"], ["C"])
    with pytest.raises(KeyError):
        variants.best_alleles(g, p, ["chrU"], [3], ["A"], ["C"])

    class Handle:
        h, n = None, 0
    with pytest.raises(ValueError, match="one entry per variant"):
        _lib.scan_alleles_best(Handle(), Handle(), [0, 0], [1], [1], [b"A"])
    with pytest.raises(ValueError, match="refs"):
        _lib.scan_alleles_best(Handle(), Handle(), [0], [1], [2], [b"A"], refs=[b"A"])


def test_path_constants_are_three_positive_numbers():
    L = _lib.lib()
    dims = np.zeros(3, dtype=np.int32)
    assert L.ms_debug_allelebest_dims(_lib.ptr(dims, ctypes.c_int32)) == _lib.MS_OK           # the symbols exist, with or without a device
    assert np.all(dims > 0)
    d = _lib.allelebest_dims()
    assert [d["tile"], d["long_windows"], d["lds_max_width"]] == dims.tolist()
    assert d["tile"] % 64 == 0 and d["long_windows"] >= 2 and d["lds_max_width"] >= 64
    assert L.ms_debug_allelebest_dims(None) == _lib.MS_ERR_INVALID


def test_no_gpu_means_loud_failure_not_fallback():
    L = _lib.lib()
    assert hasattr(L, "ms_scan_alleles_best") and hasattr(L, "ms_allelebest_free")            # the symbols exist, with or without a device
    if _lib.device_count() > 0:
        pytest.skip("a GPU is visible")
    pw = _lib.PwmSet.from_matrices([np.ones((4, 3))])
    h = ctypes.c_void_p()
    ci, ps, rl, ao = np.zeros(1, dtype=np.int32), np.ones(1, dtype=np.int64), np.ones(1, dtype=np.int32), np.array([0, 1], dtype=np.int64)
    rc = L.ms_scan_alleles_best(pw.h, None, _lib.ptr(ci, ctypes.c_int32), _lib.ptr(ps, ctypes.c_int64), _lib.ptr(rl, ctypes.c_int32), b"A",
                                _lib.ptr(ao, ctypes.c_int64), None, 1, 3, 0, ctypes.byref(h))   # no device: said before the handles are looked at
    assert rc == _lib.MS_ERR_RUNTIME and not h.value
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _lib.check(rc)

    class Handle:
        h = None
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _lib.scan_alleles_best(pw, Handle(), [0], [1], [1], [b"A"])
    pw.close()

    class Pwm:
        matrix = np.ones((4, 3))

    class Genome:
        h, index = None, {"chr1": 0}
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        variants.best_alleles(Genome(), [Pwm()], ["chr1"], [3], ["A"], ["C"])
