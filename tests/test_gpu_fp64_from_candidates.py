"""
The fp64 stage -- rescore_kernel and rescore_carry_kernel (ms_fp64.hip) -- driven from candidate lists of our choosing
(ms_debug_scan_from_candidates: the scan with the pre-filter's launch replaced by an upload), among them shapes the pre-filter makes only
rarely: every field flagged, windows hanging over region ends and over the set's end, a whole chunk of empty records, more hits in a chunk
than the hit stage holds.  What a list must give is prefilter_model.hits_from_candidates: the oracle's hits of the fast motifs at the flagged
(motif, window start) pairs -- with both strands scanned either strand's flag keeps both -- and every oracle hit of the motifs on the
all-fp64 path, in the reference's order.  Integers are compared by value, scores by their bits.  Every list runs under
MS_RESCORE_SORTED_MIN=0 (rescore_carry_kernel) and 1e30 (rescore_kernel).

Duplicate records and flags on empty fields are outside the contract and are not fed.  The bucketed hit list belongs to predicted-size scans,
which these entries never are: tests/test_gpu_bucketed_order.py covers it.  The sets: fp64_cases.py (their conditions are asserted without a
GPU in tests/test_prefilter_model_host.py).
"""
import numpy as np
import pytest

import fp64_cases as fc
import prefilter_model as pm
from motifscan_amd import _lib

pytestmark = pytest.mark.gpu

KERNELS = {"carry": "0", "list": "1e30"}          # MS_RESCORE_SORTED_MIN


@pytest.fixture(scope="module", autouse=True)
def device():
    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible: the gpu-marked tests need an MI355X (there is no CPU fallback)")
    _lib.set_device(0)


@pytest.fixture(scope="module")
def sets(oracle):
    """per (set, strand): the case, its handles, and the geometry of its scans"""
    out = {}

    def get(name, strand=3):
        if (name, strand) not in out:
            case = fc.build(name, _lib, oracle, strand)
            pw, sq = _lib.PwmSet(case["vals"], case["widths"], case["cutoffs"]), _lib.SeqSet(case["raw"], case["offsets"])
            _, geom, _ = _lib.scan_candidates(pw, sq, strand)
            out[name, strand] = (case, pw, sq, geom)
        return out[name, strand]
    return get


def _env(monkeypatch, kernel):
    monkeypatch.setenv("MS_MEASURE", "1")
    for k in ("MS_PF_DENSE", "MS_PF_RARE_CAP", "MS_PF_MAX_BLOCKS", "MS_PF_LDS_BUDGET", "MS_PF_PAIR", "MS_NO_PREDICT"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("MS_RESCORE_SORTED_MIN", KERNELS[kernel])


def _name_hit(case, m, hit):
    r, p, sd = hit
    return (f"region {r} of {int(np.diff(case['offsets'])[r])} bases, pos {p}, strand {sd}: the window ends "
            f"{int(np.diff(case['offsets'])[r]) - p - int(case['widths'][m])} bases before the region's end")


def _same(got, want, what, case=None):
    if not np.array_equal(got["motif_offsets"], want["motif_offsets"]):
        ng, nw = np.diff(got["motif_offsets"]), np.diff(want["motif_offsets"])
        m = int(np.flatnonzero(ng != nw)[0])
        msg = f"{what}: {int((ng != nw).sum())} motifs differ in their hit count, the first motif {m}: {int(ng[m])} hits for {int(nw[m])}"
        if case is not None:
            hits = [{(int(x["seq_idx"][i]), int(x["pos"][i]), int(x["strand"][i])) for i in range(int(x["motif_offsets"][m]), int(x["motif_offsets"][m + 1]))}
                    for x in (got, want)]
            msg += f" (width {int(case['widths'][m])})"
            for label, d in (("missing", hits[1] - hits[0]), ("not the oracle's", hits[0] - hits[1])):
                if d:
                    msg += f"; first {label}: {_name_hit(case, m, min(d))}"
        raise AssertionError(msg)
    for k in ("seq_idx", "pos"):
        if not np.array_equal(got[k], want[k]):
            i = int(np.flatnonzero(got[k] != want[k])[0])
            m = int(np.searchsorted(want["motif_offsets"], i, side="right") - 1)
            raise AssertionError(f"{what}: {k} differs first at hit {i} (motif {m}): region {int(got['seq_idx'][i])} pos {int(got['pos'][i])} "
                                 f"for region {int(want['seq_idx'][i])} pos {int(want['pos'][i])}")
    assert np.array_equal(got["strand"].astype(np.int32), want["strand"].astype(np.int32)), f"{what}: strand differs"
    assert np.array_equal(np.ascontiguousarray(got["score"]).view(np.uint64), np.ascontiguousarray(want["score"]).view(np.uint64)), f"{what}: score bits differ"


def _run(sets, monkeypatch, name, kernel, records, want, what, strand=3):
    case, pw, sq, _ = sets(name, strand)
    _env(monkeypatch, kernel)
    res = _lib.scan_from_candidates(pw, sq, records, strand)
    got, st = res.hits(), res.stats()
    print(f"{what}: {len(records)} slots, {int(np.count_nonzero(np.asarray(records) & np.uint64(0xFFFF)))} live, {st['n_hits']} hits, {st['n_candidates']} candidate slots, {st['n_passes']} passes")
    _same(got, want, what, case)
    res.close()
    return st


def test_the_carried_stage_chunk_is_the_one_the_cases_are_cut_by(sets):
    """geom's records-per-chunk is the library's own copy of kRwChunk: it must be ms_fp64.hip's"""
    assert sets("narrow")[3]["rescore_chunk"] == fc.rw_chunk_from_source()


@pytest.mark.parametrize("kernel", sorted(KERNELS))
@pytest.mark.parametrize("name,strand", [("narrow", 3), ("wide", 3), ("narrow", 1), ("wide", 2)])
def test_model_list_shuffled(sets, monkeypatch, name, strand, kernel):
    """(a) the model's own list in a seeded random order: the scan's result, which is the oracle's"""
    case, pw, sq, _ = sets(name, strand)
    rec = np.random.default_rng(12).permutation(pm.pack_records(case["model"]))
    want = pm.hits_from_candidates(None, case, case["model"])
    _same(want, case["oracle"], f"{name}: the model keeps every oracle hit")
    _run(sets, monkeypatch, name, kernel, rec, case["oracle"], f"{name}, strand {strand}, {kernel}, model list", strand)
    _env(monkeypatch, kernel)
    res = _lib.scan(pw, sq, strand)
    _same(res.hits(), case["oracle"], f"{name}, strand {strand}, {kernel}: ms_scan")
    res.close()


@pytest.mark.parametrize("kernel", sorted(KERNELS))
@pytest.mark.parametrize("name,strand", [("narrow", 3), ("wide", 3), ("narrow", 2), ("wide", 1)])
def test_every_field_flagged_everywhere(sets, monkeypatch, name, strand, kernel):
    """(b) every occupied field at every base: windows across region ends and past the set's end give nothing, the rest is the oracle's scan"""
    case = sets(name, strand)[0]
    _run(sets, monkeypatch, name, kernel, pm.pack_records(fc.all_flagged(case)), case["oracle"], f"{name}, strand {strand}, {kernel}, all flagged", strand)


@pytest.mark.parametrize("kernel", sorted(KERNELS))
@pytest.mark.parametrize("name", ["narrow", "wide"])
def test_list_lengths_around_the_chunk_and_the_static_blocks(sets, monkeypatch, name, kernel):
    """(c) the all-flagged list cut to the waves' own first blocks (nothing behind them: counters[0] = 0), and to one record less than a
    chunk of the carried stage, a chunk, one more, and two chunks and one -- shorter lists are padded with empty slots up to the static blocks"""
    case, _, _, geom = sets(name)
    full = np.random.default_rng(5).permutation(pm.pack_records(fc.all_flagged(case)))
    chunk = geom["rescore_chunk"]
    assert 0 < geom["cand_static"] < len(full) and 2 * chunk + 1 < len(full)
    for n in (geom["cand_static"], chunk - 1, chunk, chunk + 1, 2 * chunk + 1):
        rec = full[:n]
        st = _run(sets, monkeypatch, name, kernel, rec, pm.hits_from_candidates(None, case, fc.flags_of(rec, case)), f"{name}, {kernel}, first {n} records")
        assert st["n_candidates"] == max(n, geom["cand_static"])


@pytest.mark.parametrize("kernel", sorted(KERNELS))
@pytest.mark.parametrize("name", ["narrow", "wide"])
def test_a_chunk_of_empty_records(sets, monkeypatch, name, kernel):
    """(d) a whole chunk of empty slots in the middle of the all-flagged list, and single empty slots scattered through it"""
    case, _, _, geom = sets(name)
    full = pm.pack_records(fc.all_flagged(case))
    chunk = geom["rescore_chunk"]
    assert len(full) > 3 * chunk
    rec = np.concatenate([full[:2 * chunk], np.zeros(chunk, dtype=np.uint64), full[2 * chunk:]])
    rec = np.insert(rec, np.arange(7, len(rec), 1013), np.uint64(0))
    _run(sets, monkeypatch, name, kernel, rec, case["oracle"], f"{name}, {kernel}, a chunk of empty slots")


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_more_hits_in_a_chunk_than_the_stage_holds(sets, monkeypatch, oracle, kernel):
    """(e) poly-A regions, the poly-A motifs flagged at every base: a chunk of the list holds several times the hits a block stages"""
    case = sets("polya")[0]
    t = fc.tally(case, oracle)
    assert t["hits_of_fullest_chunk"] > fc.HIT_STAGE, t
    _run(sets, monkeypatch, "polya", kernel, pm.pack_records(fc.all_flagged(case)), case["oracle"], f"polya, {kernel}, all flagged")


def test_a_record_outside_the_scan_is_refused(sets):
    case, pw, sq, _ = sets("narrow")
    n_groups, n_bases = case["plan"]["group_fields"].shape[0], int(case["offsets"][-1])
    for rec in ((n_bases << 30) | 1, (n_groups << 16) | 1):
        with pytest.raises(ValueError):
            _lib.scan_from_candidates(pw, sq, np.array([rec], dtype=np.uint64), 3)
    res = _lib.scan_from_candidates(pw, sq, np.array([(n_bases << 30) | (n_groups << 16)], dtype=np.uint64), 3)       # an empty slot names nothing
    assert res.n_hits == 0
    res.close()
