"""
The host side of the variant scan (motifscan_amd/variants.py): the VCF reader, the views of VariantSites, and what must happen before any
device is asked for anything.  No GPU.
"""
import ctypes
import gzip

import numpy as np
import pytest

from motifscan_amd import _lib, variants

VCF = "\n".join([
    "##fileformat=VCFv4.2",
    "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO",
    "chr1\t1\trs1\tA\tG\t.\tPASS\t.",
    "chr1\t10\trs2\tc\tt,G\t.\tPASS\t.",            # lower case, two ALTs
    "chr2\t7\t.\tAT\tA\t.\tPASS\t.",                # deletion
    "chr2\t8\t.\tA\tATT,C\t.\tPASS\t.",             # insertion + a substitution on one line
    "chr2\t9\t.\tAC\tGT\t.\tPASS\t.",               # multi-base
    "chr2\t11\t.\tA\t<DEL>\t.\tPASS\t.",
    "chr2\t12\t.\tA\t*,T\t.\tPASS\t.",
    "chr2\t13\t.\tA\t.\t.\tPASS\t.",
    "chrX\t100\trs9\tN\ta",                          # five columns are enough
    "",
])


def check_vcf(v):
    assert v.chrom.tolist() == ["chr1", "chr1", "chr1", "chr2", "chr2", "chrX"]
    assert v.pos.tolist() == [0, 9, 9, 7, 11, 99] and v.pos.dtype == np.int64           # 1-based -> 0-based
    assert v.ref.tolist() == ["A", "c", "c", "A", "A", "N"]
    assert v.alt.tolist() == ["G", "t", "G", "C", "T", "a"]
    assert v.id.tolist() == ["rs1", "rs2", "rs2", ".", ".", "rs9"]
    assert v.skipped == {"indel": 2, "multi_base": 1, "symbolic": 1, "star": 1, "missing": 1}


def test_read_vcf_plain_and_gz(tmp_path):
    plain = tmp_path / "a.vcf"
    plain.write_text(VCF)
    check_vcf(variants.read_vcf(str(plain)))
    gz = tmp_path / "a.vcf.gz"
    with gzip.open(gz, "wt") as fh:
        fh.write(VCF)
    check_vcf(variants.read_vcf(gz))
    empty = tmp_path / "e.vcf"
    empty.write_text("##only a header\n")
    v = variants.read_vcf(empty)
    assert len(v.pos) == 0 and sum(v.skipped.values()) == 0
    short = tmp_path / "s.vcf"
    short.write_text("chr1\t5\t.\tA\n")
    with pytest.raises(ValueError, match="fewer than 5"):
        variants.read_vcf(short)


def test_variant_sites_views_and_delta():
    s = variants.VariantSites(motif=[0, 0, 1, 1], variant=[3, 4, 0, 3], start=[10, 11, 5, 9], strand=[1, 2, 1, 2],
                              score_ref=[0.9, 0.2, 0.8, 0.5], score_alt=[0.1, 0.95, 0.85, 0.5], state=[1, 2, 3, 3], motif_offsets=[0, 2, 4])
    assert len(s) == 4
    assert s.lost.tolist() == [True, False, False, False]
    assert s.gained.tolist() == [False, True, False, False]
    assert s.kept.tolist() == [False, False, True, True]
    assert np.array_equal(s.delta, s.score_alt - s.score_ref) and s.delta[0] < 0 < s.delta[1] and s.delta[3] == 0
    assert s.skipped.size == 0 and s.motif_offsets.dtype == np.int64
    with pytest.raises(ValueError):
        s.motif_counts()


class Pwm:
    def __init__(self, matrix, cutoffs):
        self.matrix, self.cutoffs, self.length = np.asarray(matrix, dtype=np.float64), cutoffs, np.asarray(matrix).shape[1]


class NoGenome:
    """Stands where a ResidentGenome would: touching it at all is the failure."""

    def __getattr__(self, name):
        raise AssertionError("the genome was used before the PWMs were checked")


def test_missing_cutoff_is_the_scanners_error_before_any_device_call():
    pwms = [Pwm(np.ones((4, 3)), {"1e-4": 0.9}), Pwm(np.ones((4, 5)), {"1e-3": 0.8})]
    with pytest.raises(ValueError, match="no motif score cutoff set for P-value '1e-4'"):
        variants.scan_variants(NoGenome(), pwms, ["chr1"], [3], ["A"])
    with pytest.raises(ValueError, match="no motif score cutoff"):
        variants.scan_variants(NoGenome(), [Pwm(np.ones((4, 3)), None)], ["chr1"], [3], ["A"])
    with pytest.raises(ValueError, match="on_mismatch"):
        variants.scan_variants(NoGenome(), pwms, ["chr1"], [3], ["A"], on_mismatch="ignore")
    with pytest.raises(ValueError, match="strand"):
        variants.scan_variants(NoGenome(), pwms, ["chr1"], [3], ["A"], strand="*")


def test_binding_checks_its_arrays_and_the_chunk_knob_needs_no_device():
    class Handle:
        h, n = None, 0
    with pytest.raises(ValueError, match="one entry per variant"):
        _lib.scan_variants(Handle(), Handle(), [0, 0], [1], b"AC")
    prev = _lib.varscan_chunk(7)
    try:
        assert _lib.varscan_chunk(0) == 7
        with pytest.raises(ValueError):
            _lib.varscan_chunk(-1)
    finally:
        _lib.varscan_chunk(prev)


def test_no_gpu_means_loud_failure_not_fallback():
    if _lib.device_count() > 0:
        pytest.skip("a GPU is visible")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _lib.ResidentGenome({"chr1": "ACGTACGT"})
    pw = _lib.PwmSet.from_matrices([np.ones((4, 3))], cutoffs=[0.5])
    h = ctypes.c_void_p()
    zero32, zero64 = np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int64)
    rc = _lib.lib().ms_scan_variants(pw.h, None, _lib.ptr(zero32, ctypes.c_int32), _lib.ptr(zero64, ctypes.c_int64), b"A", 1, 3, 0, ctypes.byref(h))
    assert rc == _lib.MS_ERR_RUNTIME and not h.value
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _lib.check(rc)
