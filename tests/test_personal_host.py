"""
The host side of personal genomes (ms_genome_apply_alleles / ms_liftmap_*; motifscan_amd.personal): the exported symbols and the path
constants, what must fail loudly without a GPU, the sequential restatement personal.apply_alleles_host pinned by hand-written cases
(tests/personal_cases.py: expected strings and both lift maps for every position, written out by hand), haplotype_mask on a small VCF,
and the lift maps' properties on seeded random cases.  No GPU.
"""
import ctypes

import numpy as np
import pytest

import personal_cases as pc
from motifscan_amd import _lib, personal, variants

SYMBOLS = ["ms_genome_apply_alleles", "ms_liftmap_shape", "ms_liftmap_status", "ms_liftmap_ref_mismatch", "ms_liftmap_chrom_sizes", "ms_liftmap_lift",
           "ms_liftmap_device_ms", "ms_liftmap_free", "ms_debug_personal_dims", "ms_debug_liftmap_stage_ms"]


def test_new_symbols_are_exported():
    L = _lib.lib()
    for name in SYMBOLS:
        assert hasattr(L, name), name
    assert (_lib.MS_APPLY_SKIP_MISMATCH, _lib.MS_LIFT_REF_TO_ALT, _lib.MS_LIFT_ALT_TO_REF) == (1, 0, 1)


def test_path_constants_answer_without_a_device():
    L = _lib.lib()
    dims = np.full(4, -1, dtype=np.int32)
    assert L.ms_debug_personal_dims(_lib.ptr(dims, ctypes.c_int32)) == _lib.MS_OK
    assert dims[0] > 0 and dims[0] % 32 == 0 and dims[1] >= 0 and dims[2] > 0 and dims[3] == 0
    d = _lib.personal_dims()
    assert [d["block_bases"], d["stage_variants"], d["lift_block"]] == dims[:3].tolist()
    assert L.ms_debug_personal_dims(None) == _lib.MS_ERR_INVALID


def test_no_gpu_means_loud_failure_not_fallback():
    if _lib.device_count() > 0:
        return                                                   # (a GPU is visible: tests/test_gpu_personal.py covers the call)
    L = _lib.lib()
    h, hm = ctypes.c_void_p(), ctypes.c_void_p()
    ci, ps, rl, ao = np.zeros(1, dtype=np.int32), np.ones(1, dtype=np.int64), np.ones(1, dtype=np.int32), np.array([0, 1], dtype=np.int64)
    rc = L.ms_genome_apply_alleles(None, _lib.ptr(ci, ctypes.c_int32), _lib.ptr(ps, ctypes.c_int64), _lib.ptr(rl, ctypes.c_int32), b"A",
                                   _lib.ptr(ao, ctypes.c_int64), None, 1, 0, ctypes.byref(h), ctypes.byref(hm))
    assert rc == _lib.MS_ERR_RUNTIME and not h.value and not hm.value      # no device: said before the handle or the flags are looked at
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _lib.check(rc)
    rc = L.ms_genome_apply_alleles(None, None, None, None, None, None, None, 0, 0xFF, ctypes.byref(h), None)
    assert rc == _lib.MS_ERR_RUNTIME

    class Genome:
        h, index, names = None, {"chr1": 0}, ["chr1"]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _lib.apply_alleles(Genome(), [0], [1], [1], [b"A"])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        personal.personal_genome(Genome(), ["chr1"], [1], ["A"], ["C"])


def test_argument_errors_come_before_any_device_call():
    class Genome:                                                # touching the device would need .h
        index = {"chr1": 0}
    with pytest.raises(ValueError, match="on_mismatch"):
        personal.personal_genome(Genome(), ["chr1"], [1], ["A"], ["C"], on_mismatch="ignore")
    with pytest.raises(ValueError, match="one entry per variant"):
        personal.personal_genome(Genome(), ["chr1"], [1, 2], ["A"], ["C"])
    with pytest.raises(ValueError, match="select"):
        personal.personal_genome(Genome(), ["chr1"], [1], ["A"], ["C"], select=[True, False])
    with pytest.raises(KeyError):
        personal.personal_genome(Genome(), ["chrU"], [1], ["A"], ["C"])
    with pytest.raises(ValueError, match="one entry per variant"):
        _lib.apply_alleles(Genome(), [0, 0], [1], [1], [b"A"])
    with pytest.raises(ValueError, match="refs"):
        _lib.apply_alleles(Genome(), [0], [1], [2], [b"A"], refs=[b"A"])
    with pytest.raises(ValueError, match="hap"):
        personal.haplotype_mask("nowhere.vcf", 0, 2)


@pytest.mark.parametrize("name", list(pc.CASES))
def test_restatement_on_hand_written_cases(name):
    case = pc.CASES[name]
    chrom, pos, ref, alt, check, skip = pc.case_args(case)
    got = personal.apply_alleles_host(case["chroms"], chrom, pos, ref, alt, refs_check=check, skip_mismatch=skip)
    assert got["seqs"] == case["seqs"]
    assert got["sizes"].tolist() == [len(s) for s in case["seqs"]]
    assert got["status"].tolist() == case["status"] and got["n_applied"] == case["status"].count(1)
    assert got["ref_mismatch"].tolist() == case.get("mismatch", [0] * len(pos))
    for c in range(len(case["chroms"])):
        for key in ("to_alt", "to_ref"):
            out, inside = got[key][c]
            assert out.tolist() == case[key][c][0], (key, c)
            assert inside.tolist() == case[key][c][1], (key, c, "inside")
    # the same variants by their lengths alone, and chromosomes given as a dict of str
    by_len = personal.apply_alleles_host({f"c{i}": s.decode() for i, s in enumerate(case["chroms"])}, chrom, pos, [len(r) for r in ref], alt)
    if check is None:
        assert by_len["seqs"] == case["seqs"] and by_len["status"].tolist() == case["status"]


@pytest.mark.parametrize("seed", range(12))
def test_lift_properties_on_random_cases(seed):
    chroms, chrom, pos, ref, alt = pc.random_case(1000 + seed)
    for skip in (False, True):
        got = personal.apply_alleles_host(chroms, chrom, pos, ref, alt, refs_check=ref, skip_mismatch=skip)
        assert set(got["status"].tolist()) <= ({0, 1, 2} if skip else {0, 1})
        delta = np.zeros(len(chroms), dtype=np.int64)
        for v in np.flatnonzero(got["status"] == 1):
            delta[chrom[v]] += len(alt[v]) - len(ref[v])
        assert got["sizes"].tolist() == [len(s) + int(d) for s, d in zip(chroms, delta)]
        for c, seq in enumerate(chroms):
            fwd, fin = got["to_alt"][c]
            bwd, bin_ = got["to_ref"][c]
            L, L2 = len(seq), len(got["seqs"][c])
            assert fwd.size == L + 1 and bwd.size == L2 + 1
            assert np.all(np.diff(fwd) >= 0) and np.all(np.diff(bwd) >= 0)                     # monotone
            assert fwd[L] == L2 and bwd[L2] == L and fin[L] == 0 and bin_[L2] == 0              # ends map to ends
            out = np.flatnonzero(fin == 0)
            assert np.array_equal(bwd[fwd[out]], out)                                           # to_ref(to_alt(p)) == p outside every variant
            # a base outside every applied variant is the same base on both haplotypes
            keep = out[out < L]
            assert bytes(got["seqs"][c][int(q)] for q in fwd[keep]) == bytes(seq[int(p)] for p in keep)


VCF = """##fileformat=VCFv4.2
##contig=<ID=chr1>
#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS1\tS2
chr1\t10\ta\tA\tC\t.\t.\t.\tGT\t0|1\t1|0
chr1\t20\tb\tAT\tA,ATT\t.\t.\t.\tGT:DP\t1|2:9\t2/2:3
chr1\t30\tc\tG\tT\t.\t.\t.\tDP:GT\t7:0/1\t4:1/1
chr1\t40\td\tC\t<DEL>,G\t.\t.\t.\tGT\t2|1\t.|2
chr1\t50\te\tT\tA\t.\t.\t.\tGT\t./.\t1
chr1\t60\tf\tG\t*,C\t.\t.\t.\tGT\t2|2\t0|0
"""


def test_haplotype_mask_on_a_small_vcf(tmp_path):
    path = tmp_path / "small.vcf"
    path.write_text(VCF)
    alleles = variants.read_vcf_alleles(str(path))
    # the records read_vcf_alleles keeps, in order: a; b ALT 1, b ALT 2; c; d ALT 2 (<DEL> is symbolic); e; f ALT 2 ('*' is left out)
    assert alleles.id.tolist() == ["a", "b", "b", "c", "d", "e", "f"]
    mask = lambda sample, hap: personal.haplotype_mask(str(path), sample, hap).tolist()
    #                         a      b1     b2     c      d2     e      f2
    assert mask("S1", 0) == [False, True, False, False, True, False, True]       # 0|1, 1|2, 0/1 (unphased het: nobody's), 2|1, ./., 2|2
    assert mask("S1", 1) == [True, False, True, False, False, False, True]
    assert mask("S2", 0) == [True, False, True, True, False, True, False]        # 1|0, 2/2 (homozygous: both), 1/1, .|2, haploid 1, 0|0
    assert mask("S2", 1) == [False, False, True, True, True, False, False]
    assert mask(1, 1) == mask("S2", 1) and mask(0, 0) == mask("S1", 0)
    assert personal.haplotype_mask(str(path), "S1", 0).dtype == bool
    with pytest.raises(KeyError):
        personal.haplotype_mask(str(path), "S3", 0)


def test_lift_sites_adds_the_region_start():
    class Map:
        def to_ref(self, chrom, pos):
            return np.asarray(pos) * 10 + np.asarray(chrom), np.zeros(len(pos), dtype=np.uint8)
    starts, chrom_of_region = np.array([100, 200]), np.array([0, 3])
    seq_idx, hit_pos = np.array([0, 1, 1]), np.array([5, 6, 7])
    out, inside = personal.lift_sites(Map(), chrom_of_region[seq_idx], starts[seq_idx], hit_pos)
    assert out.tolist() == [1050, 2063, 2073] and inside.tolist() == [0, 0, 0]
