"""
ms_scan_variants (ms_variants.hip) and ms_scan_alleles (ms_alleles.hip) on the GPU where their kernels change path: motifs at and one
column past the widest table staged in LDS (the HBM-table kernels, the second launch over the same grid, the set of wide motifs only,
the dynamic-LDS raise), the width classes of var_scan_kernel's item stepping, alleles of up to MS_ALLELE_MAX_LEN bases, and variant
counts and chunks around one tile.  The cases and their expected records are tests/variant_cases.py's (every size from
_lib.varscan_dims(); tests/test_variant_cases_host.py proves without a GPU that each case sits where it claims); the expected scores
are the pinned oracle's on Python-built flank strings.

Integers are compared by value, scores and states by their bytes: there is no tolerance anywhere.

Out of scope: chromosomes of more than 2^30 bases (the kVarFar / kAlFar clamp of a variant's distance to the chromosome's ends) -- they
need a genome too large for a test of a few seconds.
"""
import numpy as np
import pytest

import variant_cases as vc
from motifscan_amd import _lib

pytestmark = pytest.mark.gpu

CUTOFF_SETS = ("q90", "all", "none")
RUNS = [(name, mask) for name in vc.CASES for mask in ((1, 2, 3) if name in vc.ALL_STRANDS else (3,))]


@pytest.fixture(scope="module", autouse=True)
def _device():
    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible")
    _lib.set_device(0)


@pytest.fixture(scope="module")
def dims():
    return _lib.varscan_dims()


@pytest.fixture(scope="module")
def built(oracle, dims):
    """name -> (case, resident genome): the oracle's tables and the genomes, made once"""
    cache = {}

    def get(name):
        if name not in cache:
            case = vc.build(name, oracle, dims)
            cache[name] = (case, _lib.ResidentGenome(case["chroms"]))
        return cache[name]
    yield get
    for _, genome in cache.values():
        genome.close()


def scan(case, genome, which, strand_mask, sel=None, motifs=None):
    """One scan of the case's variant list sel (default all): every array of the result, and gained / lost."""
    sel = np.arange(case["V"]) if sel is None else np.asarray(sel)
    mats, cutoffs = case["mats"], case["cutoffs"][which]
    if motifs is not None:
        mats, cutoffs = [mats[m] for m in motifs], cutoffs[list(motifs)]
    pw = _lib.PwmSet.from_matrices(mats, cutoffs)
    try:
        if case["kind"] == "snv":
            res = _lib.scan_variants(pw, genome, case["chrom_idx"][sel], case["pos"][sel], case["alt"][sel], strand_mask)
        else:
            res = _lib.scan_alleles(pw, genome, case["chrom_idx"][sel], case["pos"][sel], case["ref_len"][sel], [case["alts"][i] for i in sel],
                                    strand_mask=strand_mask)
        try:
            got = res.sites()
            got["gained"], got["lost"] = res.motif_counts()
            assert np.array_equal(got["motif_offsets"], res.motif_offsets)
        finally:
            res.close()
    finally:
        pw.close()
    return got


def same_bytes(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k


def compare(got, want):
    rec, offsets, gained, lost = want
    assert np.array_equal(got["motif_offsets"], offsets)
    for k, v in rec.items():
        if v.dtype.kind == "f" or k == "state":
            assert got[k].dtype == v.dtype and got[k].tobytes() == v.tobytes(), k
        else:
            assert np.array_equal(got[k], v), k
    assert np.array_equal(got["motif"], np.repeat(np.arange(len(offsets) - 1), np.diff(offsets)))
    assert np.array_equal(got["gained"], gained) and np.array_equal(got["lost"], lost)


@pytest.mark.parametrize("which", CUTOFF_SETS)
@pytest.mark.parametrize("name,strand_mask", RUNS)
def test_records_equal_the_oracle(built, name, strand_mask, which):
    case, genome = built(name)
    for list_name, sel in case["lists"].items():
        got = scan(case, genome, which, strand_mask, sel)
        want = vc.expected(case, which, strand_mask, None if len(sel) == case["V"] else sel)
        print(f"{name} / {list_name}, {which}, strands {strand_mask}: {len(got['variant'])} records, expected {want[1][-1]}; "
              f"gained {got['gained'].tolist()} lost {got['lost'].tolist()}")
        compare(got, want)
        same_bytes(got, scan(case, genome, which, strand_mask, sel))              # scanned twice: byte-identical
        if which == "none":
            assert len(got["variant"]) == 0 and not got["gained"].any() and not got["lost"].any()
        else:
            assert len(got["variant"]) > 0


@pytest.mark.parametrize("which", CUTOFF_SETS)
@pytest.mark.parametrize("name,scan_name", [("snv_steps", "variants"), ("al_tiles", "alleles")])
def test_variant_counts_around_one_tile(built, dims, name, scan_name, which):
    case, genome = built(name)
    for n in vc.tile_counts(dims[scan_name]["tile"]):
        sel = np.arange(n)
        got = scan(case, genome, which, 3, sel)
        compare(got, vc.expected(case, which, 3, sel))
        if which == "q90":
            assert got["gained"].sum() > 0 and got["lost"].sum() > 0


@pytest.mark.parametrize("which", CUTOFF_SETS)
@pytest.mark.parametrize("name,scan_name", [("snv_steps", "variants"), ("al_tiles", "alleles")])
def test_chunks_of_a_tile_and_of_a_tile_and_one(built, dims, name, scan_name, which):
    case, genome = built(name)
    whole = scan(case, genome, which, 3)
    compare(whole, vc.expected(case, which, 3))
    for chunk in vc.chunk_sizes(dims[scan_name]["tile"]):
        prev = _lib.varscan_chunk(chunk)
        try:
            chunked = scan(case, genome, which, 3)
        finally:
            _lib.varscan_chunk(prev)
        same_bytes(whole, chunked)


def test_allele_scan_equals_the_snv_scan_on_wide_motifs(built):
    """ms_scan_alleles against ms_scan_variants on al_lds_edge's single-base substitutions: the two HBM-table kernels and the two
    LDS-table kernels on the same windows (as test_gpu_alleles.py::test_equal_to_the_snv_scan_where_both_apply does at small widths)."""
    case, genome = built("al_lds_edge")
    sel = np.flatnonzero((case["ref_len"] == 1) & (case["alt_len"] == 1))
    assert len(sel) >= 5
    for which in ("q90", "all"):
        al = scan(case, genome, which, 3, sel)
        pw = _lib.PwmSet.from_matrices(case["mats"], case["cutoffs"][which])
        res = _lib.scan_variants(pw, genome, case["chrom_idx"][sel], case["pos"][sel], b"".join(case["alts"][i] for i in sel))
        snv = res.sites()
        res.close(), pw.close()
        # the SNV records are ordered (motif, variant, start, strand); the allele records (motif, variant, allele, start, strand)
        for allele, bit, score in ((0, 1, "score_ref"), (1, 2, "score_alt")):
            a = al["allele"] == allele
            s = (snv["state"] & bit) != 0
            assert a.sum() == s.sum() and a.sum() > 0
            for k, ks in (("motif", "motif"), ("variant", "variant"), ("start", "start"), ("strand", "strand")):
                assert np.array_equal(al[k][a], snv[ks][s]), (allele, k)
            assert al["score"][a].tobytes() == snv[score][s].tobytes(), allele
            assert len(np.unique(al["motif"][a])) == len(case["mats"])


@pytest.mark.parametrize("name,edge", [("snv_lds_edge", 767), ("al_lds_edge", 639)])
def test_either_side_of_the_lds_raise_alone(built, name, edge):
    """The motif of the last width that needs no raise of the dynamic-LDS limit, alone, then the first that does, alone: each launch
    asks for its own motif's bytes only."""
    case, genome = built(name)
    widths = [m.shape[1] for m in case["mats"]]
    for W in (edge, edge + 1):
        m = widths.index(W)
        got = scan(case, genome, "all", 3, motifs=[m])
        rec, offsets, gained, lost = vc.expected(case, "all", 3)
        a, b = int(offsets[m]), int(offsets[m + 1])
        assert got["motif_offsets"].tolist() == [0, b - a] and b > a
        for k, v in rec.items():
            assert got[k].tobytes() == v[a:b].tobytes(), (W, k)
        assert got["gained"].tolist() == [gained[m]] and got["lost"].tolist() == [lost[m]]
