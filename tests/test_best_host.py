"""
The host side of the best-site scan (ms_scan_best; _lib.scan_best / BestSites, cscore.best_site_lists / c_best_site,
scanner.Scanner.best_sites): what must fail loudly without a GPU, the arrays -> nested lists helper, the genome-coordinate helper and
the binding's argument checks.  No GPU.
"""
import ctypes

import numpy as np
import pytest

from motifscan_amd import _lib, cscore, scanner


def test_no_gpu_means_loud_failure_not_fallback():
    L = _lib.lib()
    assert L.ms_debug_best_segment_windows() == _lib.best_segment_windows() >= 64            # the symbols exist, with or without a device
    if _lib.device_count() > 0:
        pytest.skip("a GPU is visible")
    pw = _lib.PwmSet.from_matrices([np.ones((4, 3))])
    h = ctypes.c_void_p()
    rc = L.ms_scan_best(pw.h, None, 3, 0, ctypes.byref(h))                                   # no device: said before the handles are looked at
    assert rc == _lib.MS_ERR_RUNTIME and not h.value
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _lib.check(rc)

    class Handle:
        h = None
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _lib.scan_best(pw, Handle(), 3)
    pw.close()

    class Region:
        chrom, start, end, summit = "chr1", 2, 12, 7

    class Genome:
        chrom_sizes = {"chr1": 20}

        def fetch_sequence(self, chrom, start, end):
            return "ACGTACGTACGTACGTACGT"[start:end]

    class Pwm:
        matrix, length, cutoffs = np.ones((4, 3)), 3, None
    sc = scanner.Scanner(Genome(), [Region()])
    with pytest.raises(RuntimeError):
        sc.best_sites([Pwm()])
    with pytest.raises(RuntimeError):
        cscore.c_best_site([np.ones((4, 3))], ["ACGTA"], 3)


def test_best_site_lists_on_hand_made_arrays():
    score = np.array([[0.5, np.nan, -0.25], [np.nan, np.nan, 1.0]])
    pos = np.array([[3, -1, 0], [-1, -1, 2147483000]], dtype=np.int32)
    strand = np.array([[1, 0, 2], [0, 0, 1]], dtype=np.int8)
    out = cscore.best_site_lists(score, pos, strand)
    assert out == [[[3, 0.5, 1], None, [0, -0.25, 2]], [None, None, [2147483000, 1.0, 1]]]
    assert type(out[0][0][0]) is int and type(out[0][0][1]) is float and type(out[0][0][2]) is int
    assert cscore.best_site_lists(np.zeros((0, 4)), np.zeros((0, 4), dtype=np.int32), np.zeros((0, 4), dtype=np.int8)) == []
    assert cscore.best_site_lists(np.zeros((2, 0)), np.zeros((2, 0), dtype=np.int32), np.zeros((2, 0), dtype=np.int8)) == [[], []]
    with pytest.raises(ValueError, match="one shape"):
        cscore.best_site_lists(score, pos[:1], strand)
    with pytest.raises(ValueError, match="one shape"):
        cscore.best_site_lists(score[0], pos[0], strand[0])


def test_best_site_starts_are_genome_coordinates():
    pos = np.array([[0, -1, 7], [-1, 2147483000, 0]], dtype=np.int32)
    start = scanner.best_site_starts(pos, [100, 5, 3_000_000_000])
    assert start.dtype == np.int64
    assert start.tolist() == [[100, -1, 3_000_000_007], [-1, 2147483005, 3_000_000_000]]
    with pytest.raises(ValueError, match="one column per region"):
        scanner.best_site_starts(pos, [1, 2])
    b = scanner.BestSiteArrays(1, 2, 3)
    assert (b.score, b.start, b.strand) == (1, 2, 3)


def test_binding_checks_its_arguments_without_a_library_call():
    class Handle:
        h, n = None, 0
    for mask in (0, 4, -1):
        with pytest.raises(ValueError, match="strand mask"):
            _lib.scan_best(Handle(), Handle(), mask)
    with pytest.raises(ValueError, match="flags"):
        _lib.scan_best(Handle(), Handle(), 3, flags=1)
    with pytest.raises(ValueError, match="strand flag"):
        cscore.c_best_site([np.ones((4, 2))], ["ACGT"], 5)
