"""
The host side of the allele scan (motifscan_amd/variants.py: read_vcf_alleles, AlleleSites, scan_alleles; _lib.scan_alleles): the VCF
reader and its trimming, the views of AlleleSites, and what must happen before any device is asked for anything.  No GPU.
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
    "chr2\t7\t.\tAT\tA\t.\tPASS\t.",                # deletion, anchored
    "chr2\t8\t.\tA\tATT,C\t.\tPASS\t.",             # insertion + a substitution on one line
    "chr2\t9\t.\tAC\tGT\t.\tPASS\t.",               # multi-base, nothing shared
    "chr2\t20\tmnv\tACG\tATG\t.\tPASS\t.",          # multi-base that is one substitution
    "chr2\t30\tlong\tA\tACGTACGT\t.\tPASS\t.",      # 7 bases inserted
    "chr2\t11\t.\tA\t<DEL>\t.\tPASS\t.",
    "chr2\t12\t.\tA\t*,T\t.\tPASS\t.",
    "chr2\t13\t.\tA\t.\t.\tPASS\t.",
    "chr2\t14\tbnd\tA\tA[chr3:5[\t.\tPASS\t.",
    "chrX\t100\trs9\tN\ta",                          # five columns are enough
    "",
])


def check_trimmed(v, max_len=1000):
    rows = [("chr1", 0, "A", "G", "rs1"), ("chr1", 9, "c", "t", "rs2"), ("chr1", 9, "c", "G", "rs2"),
            ("chr2", 7, "T", "", "."), ("chr2", 8, "", "TT", "."), ("chr2", 7, "A", "C", "."), ("chr2", 8, "AC", "GT", "."),
            ("chr2", 20, "C", "T", "mnv"), ("chr2", 30, "", "CGTACGT", "long"), ("chr2", 11, "A", "T", "."), ("chrX", 99, "N", "a", "rs9")]
    too_long = [r for r in rows if max(len(r[2]), len(r[3])) > max_len]
    rows = [r for r in rows if r not in too_long]
    assert v.chrom.tolist() == [r[0] for r in rows]
    assert v.pos.tolist() == [r[1] for r in rows] and v.pos.dtype == np.int64           # 1-based -> 0-based, moved past the shared prefix
    assert v.ref.tolist() == [r[2] for r in rows] and v.alt.tolist() == [r[3] for r in rows]
    assert v.id.tolist() == [r[4] for r in rows]
    assert v.skipped == {"symbolic": 2, "star": 1, "missing": 1, "too_long": len(too_long)}
    assert v.ref.dtype == object and v.alt.dtype == object


def test_read_vcf_alleles_trims_and_counts(tmp_path):
    plain = tmp_path / "a.vcf"
    plain.write_text(VCF)
    check_trimmed(variants.read_vcf_alleles(str(plain)))
    gz = tmp_path / "a.vcf.gz"
    with gzip.open(gz, "wt") as fh:
        fh.write(VCF)
    check_trimmed(variants.read_vcf_alleles(gz))
    check_trimmed(variants.read_vcf_alleles(plain, max_len=6), max_len=6)               # the 7-base insertion goes
    v = variants.read_vcf_alleles(plain, max_len=1)                                     # ... and TT and AC -> GT
    assert v.skipped["too_long"] == 3 and v.ref.tolist() == ["A", "c", "c", "T", "A", "C", "A", "N"]

    raw = variants.read_vcf_alleles(plain, trim=False)                                  # the alleles as the file has them
    assert raw.pos.tolist() == [0, 9, 9, 6, 7, 7, 8, 19, 29, 11, 99]
    assert raw.ref.tolist() == ["A", "c", "c", "AT", "A", "A", "AC", "ACG", "A", "A", "N"]
    assert raw.alt.tolist() == ["G", "t", "G", "A", "ATT", "C", "GT", "ATG", "ACGTACGT", "T", "a"]
    assert raw.skipped == {"symbolic": 2, "star": 1, "missing": 1, "too_long": 0}
    assert variants.read_vcf_alleles(plain, trim=False, max_len=2).skipped["too_long"] == 3

    empty = tmp_path / "e.vcf"
    empty.write_text("##only a header\n")
    v = variants.read_vcf_alleles(empty)
    assert len(v.pos) == 0 and sum(v.skipped.values()) == 0 and v.ref.dtype == object
    short = tmp_path / "s.vcf"
    short.write_text("chr1\t5\t.\tA\n")
    with pytest.raises(ValueError, match="fewer than 5"):
        variants.read_vcf_alleles(short)
    # read_vcf still sees the file its own way
    old = variants.read_vcf(plain)
    assert old.skipped["indel"] == 3 and old.skipped["multi_base"] == 2 and len(old.pos) == 6


def test_trim_allele_suffix_first_then_prefix():
    assert variants.trim_allele(6, "AT", "A") == (7, "T", "")
    assert variants.trim_allele(7, "A", "ATT") == (8, "", "TT")
    assert variants.trim_allele(8, "AC", "GT") == (8, "AC", "GT")
    assert variants.trim_allele(19, "ACG", "ATG") == (20, "C", "T")
    assert variants.trim_allele(5, "TTT", "T") == (5, "TT", "")                           # the suffix goes first: no left-alignment, pos stays
    assert variants.trim_allele(5, "gA", "GT") == (6, "A", "T")                           # compared without case, letters kept as written
    assert variants.trim_allele(5, "A", "a") == (5, "A", "a")                             # identical alleles are left alone


def test_allele_sites_ref_start_and_per_variant():
    # variant 0: SNV at 100; variant 1: insertion of 3 at 50 (r = 0); variant 2: deletion of 4 at 70 (a = 0); variant 3: 2 -> 5 at 20
    s = variants.AlleleSites(motif=[0, 0, 0, 0, 0, 0, 0, 1, 1, 1], variant=[0, 0, 1, 1, 1, 2, 2, 1, 3, 3], allele=[0, 1, 1, 1, 1, 0, 1, 0, 1, 1],
                             start=[95, 100, 45, 51, 53, 68, 70, 48, 22, 25], strand=[1, 2, 1, 1, 2, 1, 1, 2, 1, 1],
                             score=[0.9, 0.95, 0.8, 0.7, 0.85, 0.6, 0.65, 0.75, 0.5, 0.55], motif_offsets=[0, 7, 10],
                             pos=[100, 50, 70, 20], ref_len=[1, 0, 4, 2], alt_len=[1, 3, 0, 5])
    assert len(s) == 10
    # ref records and alt records left of the allele keep their start; 51 lies inside the inserted bases -> x; 53 = x + a -> x + r;
    # the deletion's alt start 70 = x + a -> 74; 22 inside the 5 alt bases -> x + min(2, r) = 22; 25 = x + a -> 22
    assert s.ref_start().tolist() == [95, 100, 45, 50, 50, 68, 74, 48, 22, 22]
    pv = s.per_variant()
    assert pv["motif"].tolist() == [0, 0, 0, 1, 1] and pv["variant"].tolist() == [0, 1, 2, 1, 3]
    assert pv["n_ref"].tolist() == [1, 0, 1, 1, 0] and pv["n_alt"].tolist() == [1, 3, 1, 0, 2]
    assert np.array_equal(pv["best_ref"], [0.9, np.nan, 0.6, 0.75, np.nan], equal_nan=True)
    assert np.array_equal(pv["best_alt"], [0.95, 0.85, 0.65, np.nan, 0.55], equal_nan=True)
    assert s.skipped.size == 0 and s.motif_offsets.dtype == np.int64
    with pytest.raises(ValueError):
        s.motif_counts()
    bare = variants.AlleleSites([], [], [], [], [], [], [0, 0])
    assert len(bare) == 0 and all(len(col) == 0 for col in bare.per_variant().values())
    with pytest.raises(ValueError):
        bare.ref_start()


class Pwm:
    def __init__(self, matrix, cutoffs):
        self.matrix, self.cutoffs, self.length = np.asarray(matrix, dtype=np.float64), cutoffs, np.asarray(matrix).shape[1]


class NoGenome:
    """Stands where a ResidentGenome would: touching it at all is the failure."""

    def __getattr__(self, name):
        raise AssertionError("the genome was used before the PWMs were checked")


def test_argument_errors_come_before_the_genome_is_touched():
    pwms = [Pwm(np.ones((4, 3)), {"1e-4": 0.9}), Pwm(np.ones((4, 5)), {"1e-3": 0.8})]
    with pytest.raises(ValueError, match="no motif score cutoff set for P-value '1e-4'"):
        variants.scan_alleles(NoGenome(), pwms, ["chr1"], [3], ["A"], ["AT"])
    with pytest.raises(ValueError, match="no motif score cutoff"):
        variants.scan_alleles(NoGenome(), [Pwm(np.ones((4, 3)), None)], ["chr1"], [3], ["A"], [""])
    with pytest.raises(ValueError, match="on_mismatch"):
        variants.scan_alleles(NoGenome(), pwms, ["chr1"], [3], ["A"], ["C"], on_mismatch="ignore")
    with pytest.raises(ValueError, match="strand"):
        variants.scan_alleles(NoGenome(), pwms, ["chr1"], [3], ["A"], ["C"], strand="*")


def test_binding_checks_its_arrays_without_a_library_call():
    class Handle:
        h, n = None, 0
    with pytest.raises(ValueError, match="one entry per variant"):
        _lib.scan_alleles(Handle(), Handle(), [0, 0], [1], [1, 1], ["A", "C"])
    with pytest.raises(ValueError, match="one entry per variant"):
        _lib.scan_alleles(Handle(), Handle(), [0, 0], [1, 2], [1, 1], ["A"])
    with pytest.raises(ValueError, match="one entry per variant"):
        _lib.scan_alleles(Handle(), Handle(), [0, 0], [1, 2], [1], ["A", b"C"])
    with pytest.raises(ValueError, match="refs"):
        _lib.scan_alleles(Handle(), Handle(), [0, 0], [1, 2], [1, 2], ["A", ""], refs=["A"])
    with pytest.raises(ValueError, match="refs"):
        _lib.scan_alleles(Handle(), Handle(), [0, 0], [1, 2], [1, 2], ["A", ""], refs=["A", "C"])
    bases, offsets = _lib._flatten_alleles(["AC", b"", "g", b"TTT"])
    assert bases.tobytes() == b"ACgTTT" and offsets.tolist() == [0, 2, 2, 3, 6] and offsets.dtype == np.int64


def test_no_gpu_means_loud_failure_not_fallback():
    if _lib.device_count() > 0:
        pytest.skip("a GPU is visible")
    pw = _lib.PwmSet.from_matrices([np.ones((4, 3))], cutoffs=[0.5])
    h = ctypes.c_void_p()
    zero32, one32, zero64 = np.zeros(1, dtype=np.int32), np.ones(1, dtype=np.int32), np.zeros(1, dtype=np.int64)
    offs = np.array([0, 2], dtype=np.int64)
    rc = _lib.lib().ms_scan_alleles(pw.h, None, _lib.ptr(zero32, ctypes.c_int32), _lib.ptr(zero64, ctypes.c_int64), _lib.ptr(one32, ctypes.c_int32),
                                    b"AC", _lib.ptr(offs, ctypes.c_int64), None, 1, 3, 0, ctypes.byref(h))
    assert rc == _lib.MS_ERR_RUNTIME and not h.value
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _lib.check(rc)
