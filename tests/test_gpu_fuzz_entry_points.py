"""
The boundary fuzz of tests/fuzz_parity.py on the four entry points beside ms_scan that judge windows -- ms_scan_variants (ms_variants.hip),
ms_scan_alleles (ms_alleles.hip), ms_scan_best (ms_best.hip) and ms_scan_sweep (ms_sweep.hip; the full hand-out, and the counts-only one
of a MS_STREAM_NO_HITS span) -- against the pinned oracle: tie-rich
matrices, cutoffs on attainable scores and one ulp / 1e-10 either side, huge and tiny magnitudes, max_raw == 0, N runs and lower case.
The plot family (ms_result_site_histogram, ms_result_rank_profile; ms_plotdata.hip) runs beside them over synthetic hit arrays: centres
on and around the bin edges, region counts on the rank words' and profile tiles' edges, against numpy alone.  The genome family holds the
kernels either side of the scan (pack, extract, region hints, base counts, the window filter, scores and ranks) against the host packer,
numpy counts, the restated sampler and the oracle's c_score; the annot family holds ms_genes_nearest_tss and ms_genes_promoter_overlap
against the reference's walks restated.
Every comparison is exact (integers by value, scores by their bits; the smoothed profiles within their derived bound).  After its seeds each test asserts, on the tallies of what was
compared, that the seeds did sit on the boundary (fuzz_parity.CONDITIONS); tests/test_fuzz_cases_host.py asserts the same without a GPU.
"""
import pytest

import fuzz_parity
from motifscan_amd import _lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _device():
    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible")
    _lib.set_device(0)


@pytest.mark.parametrize("family", ["variants", "alleles", "best", "plot", "genome", "annot"])
def test_fuzz_entry_point(oracle, family):
    total = {}
    for seed in fuzz_parity.SEEDS[family]:
        ok, info = fuzz_parity.FAMILIES[family](seed, oracle, _lib)
        assert ok, info
        fuzz_parity.add_tally(total, info)
    print(f"{family}: seeds {fuzz_parity.SEEDS[family]}: {total}")
    assert not fuzz_parity.unmet_conditions(family, total)


def test_fuzz_sweep(oracle):
    total = {}
    for seed in fuzz_parity.SEEDS["sweep"]:
        ok, info = fuzz_parity.run_sweep_case(seed, oracle, _lib)
        assert ok, info
        tally = fuzz_parity.sweep_tally(seed, oracle)
        assert tally["sites"] == info
        fuzz_parity.add_tally(total, tally)
    print(f"sweep: seeds {fuzz_parity.SEEDS['sweep']}: {total}")
    assert not fuzz_parity.unmet_conditions("sweep", total)


def test_fuzz_sweep_counts(oracle):
    """The same seeds as spans of a MS_STREAM_NO_HITS stream: the counts-only hand-out (sweep_countonly_kernel), with and without
    MS_STREAM_DEDUP; the sweep family's tallies and conditions."""
    total = {}
    for seed in fuzz_parity.SEEDS["sweep"]:
        ok, info = fuzz_parity.run_sweep_counts_case(seed, oracle, _lib)
        assert ok, info
        tally = fuzz_parity.sweep_tally(seed, oracle)
        assert tally["sites"] == info
        fuzz_parity.add_tally(total, tally)
    print(f"sweep-counts: seeds {fuzz_parity.SEEDS['sweep']}: {total}")
    assert not fuzz_parity.unmet_conditions("sweep", total)
