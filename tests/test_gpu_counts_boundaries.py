"""
The counts-only forms on the device, at the edges of their kernels (cases: tests/counts_cases.py, sized from ms_debug_counts_dims and
held to their claims without a GPU by tests/test_counts_cases_host.py):

  * MS_SCAN_COUNTS_ONLY's flag map -- count_only_kernel, count_rows_kernel, motif_prefix_kernel (ms_regions.hip) behind scan_counts_fast
    (ms_scan.hip): motif numbers on the prefix kernel's thread ranges and on the LDS histogram's limit, region numbers on the flag rows'
    word edges, neighbouring flag bytes of two rows, many motifs in one wave, hit numbers on the wave, block and grid edges, the gate's
    own edge; three scans per set (the second and third in the predicted-size form), against the oracle (the closed form where the case
    has one) and the ordered scan; which form answered is asserted, and counted;
  * predictions that are too small and too large;
  * the stream's counts-only batches, region batches of a resident genome, and MS_STREAM_DEDUP beside MS_STREAM_NO_HITS;
  * sweep_countonly_kernel (ms_sweep.hip) behind a MS_STREAM_NO_HITS span, on the edges of its window arithmetic.

Every expected value is an integer: all comparisons are exact.
"""
import math
import time

import numpy as np
import pytest

import counts_cases as cc
import fuzz_parity
from motifscan_amd import _lib

pytestmark = pytest.mark.gpu

DIMS = _lib.counts_dims()                                # constants of the build: no device
FLAG_GROUPS = ("P", "R", "many_motifs", "n", "gate", "second_trip")


@pytest.fixture(scope="module", autouse=True)
def _device():
    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible")
    _lib.set_device(0)


@pytest.fixture(scope="module")
def flag_cases():
    return cc.flag_map_cases(DIMS)


def oracle_counts(oracle, mats, cutoffs, seqs, strand):
    vals, widths, raw, offsets = cc.flat(mats, seqs)
    return cc.expected_counts(oracle.scan_arrays(vals, widths, cutoffs, raw, offsets, strand, 4), len(mats))


def counts_of(res):
    return res.n_hits, res.motif_offsets.copy(), res.region_counts()


def assert_counts(got, want, what):
    assert got[0] == want[0], (what, "n_hits", got[0], want[0])
    assert np.array_equal(got[1], want[1]), (what, "motif_offsets")
    assert np.array_equal(got[2], want[2]), (what, "region_counts")


def took_flag_map(res):
    """True: hits() refuses as a counts-only result does (the flag map answered).  False: the ordered path answered -- the result holds
    its n_hits sites."""
    try:
        h = res.hits()
    except ValueError as e:
        assert "counts-only" in str(e)
        return True
    assert h["pos"].size == res.n_hits == h["seq_idx"].size
    return False


def scan_flag_case(name, case, want, cross_check=True):
    """Three counts-only scans of one PwmSet / SeqSet (the first exactly sized, the others in the predicted-size form) and the ordered
    scan.  Returns whether the FIRST scan took the flag map: the one that gates on the true number of hits."""
    mats, cutoffs, seqs, strand, must = case
    vals, widths, raw, offsets = cc.flat(mats, seqs)
    pw, sq = _lib.PwmSet(vals, widths, cutoffs), _lib.SeqSet(raw, offsets)
    try:
        took = None
        for rep in range(3):
            res = _lib.scan(pw, sq, strand, _lib.MS_SCAN_COUNTS_ONLY)
            try:
                assert_counts(counts_of(res), want, (name, "counts-only scan", rep))
                flagged = took_flag_map(res)
            finally:
                res.close()
            if rep == 0:
                took = flagged
                assert flagged == must, (name, "first scan of a fresh PWM set")
            elif must:
                assert flagged, (name, rep)               # (the predicted size is above the true one: the gate holds all the more)
            elif len(mats) > DIMS["bins"]:
                assert not flagged, (name, rep)           # (not supported at any size)
        if cross_check:
            full = _lib.scan(pw, sq, strand)
            try:
                assert_counts(counts_of(full), want, (name, "ordered scan"))
            finally:
                full.close()
        return took
    finally:
        sq.close()
        pw.close()


def in_group(name, group):
    return name == "second_trip" if group == "second_trip" else name.startswith(group + "_")


@pytest.mark.parametrize("group", FLAG_GROUPS)
def test_flag_map_cases_equal_the_oracle_and_take_the_form_they_must(oracle, flag_cases, group):
    names = [k for k in flag_cases if in_group(k, group)]
    assert names and sum(len([k for k in flag_cases if in_group(k, g)]) for g in FLAG_GROUPS) == len(flag_cases)
    took, t0 = 0, time.perf_counter()
    for name in names:
        case = flag_cases[name]
        want = cc.closed_form_of(case) if cc.is_closed_form(name) else oracle_counts(oracle, *case[:4])
        took += scan_flag_case(name, case, want)
    n_must = sum(flag_cases[k][4] for k in names)
    print(f"flag-map cases {group}: {len(names)} cases, {took} took the flag map on their first scan ({n_must} must), {1e3 * (time.perf_counter() - t0):.1f} ms")
    assert took == n_must


def test_counts_only_is_exact_when_the_predicted_size_is_wrong(oracle):
    """set_cutoffs to all-pass and back (a new cutoff version: sized exactly again); then the real thing -- a denser set of the same
    shape behind a sparse one (more hits than predicted: a second, exactly-sized run) and the sparse one behind the dense one (far
    fewer: most slots are all-ones padding, which the kernel must neither count nor flag)."""
    mats, cutoffs, sparse, dense, strand = cc.prediction_case()
    vals, widths, raw_s, off_s = cc.flat(mats, sparse)
    _, _, raw_d, off_d = cc.flat(mats, dense)
    assert np.array_equal(off_s, off_d)
    want_s, want_d = oracle_counts(oracle, mats, cutoffs, sparse, strand), oracle_counts(oracle, mats, cutoffs, dense, strand)
    all_pass = np.full(len(mats), cc.ALL_PASS)
    want_all = cc.closed_form_of((mats, all_pass, dense, strand, True))
    assert_counts(want_all, oracle_counts(oracle, mats, all_pass, dense, strand), "closed form")
    n_pred = want_s[0] * 1.06 + 6 * math.sqrt(want_s[0] + 1) + 256         # the largest size the library predicts from the sparse set
    assert want_d[0] > 1.5 * n_pred and want_s[0] * DIMS["gate_ratio"] >= len(mats) * len(sparse)
    pw, sq_s, sq_d = _lib.PwmSet(vals, widths, cutoffs), _lib.SeqSet(raw_s, off_s), _lib.SeqSet(raw_d, off_d)

    def scan(sq, want, what, passes=None):
        res = _lib.scan(pw, sq, strand, _lib.MS_SCAN_COUNTS_ONLY)
        try:
            assert_counts(counts_of(res), want, what)
            assert took_flag_map(res), what
            if passes is not None:
                assert res.stats()["n_passes"] == passes, what
        finally:
            res.close()

    try:
        scan(sq_d, want_d, "dense, first")
        scan(sq_d, want_d, "dense, predicted")
        pw.set_cutoffs(all_pass)
        scan(sq_d, want_all, "all-pass")
        scan(sq_d, want_all, "all-pass, predicted")
        pw.set_cutoffs(cutoffs)
        scan(sq_d, want_d, "back to the cutoffs")
        scan(sq_s, want_s, "sparse behind dense: predicted too large", passes=1)
        scan(sq_s, want_s, "sparse, predicted", passes=1)
        scan(sq_s, want_s, "sparse, predicted again", passes=1)
        scan(sq_d, want_d, "dense behind sparse: predicted too small", passes=2)
        scan(sq_s, want_s, "sparse behind dense again", passes=1)
    finally:
        sq_d.close()
        sq_s.close()
        pw.close()


# ------------------------------------------------------------------------------------------------ streams

@pytest.fixture(scope="module")
def stream_set(oracle):
    mats, cutoffs, seqs, strand = cc.stream_case()
    vals, widths, raw, offsets = cc.flat(mats, seqs)
    cut = 17
    halves = [(seqs[:cut], oracle.scan_arrays(vals, widths, cutoffs, "".join(seqs[:cut]).encode(), offsets[:cut + 1], strand, 4)),
              (seqs[cut:], oracle.scan_arrays(vals, widths, cutoffs, "".join(seqs[cut:]).encode(), offsets[cut:] - offsets[cut], strand, 4))]
    return {"mats": mats, "vals": vals, "widths": widths, "cutoffs": cutoffs, "seqs": seqs, "strand": strand, "halves": halves}


def batch_of(seqs):
    raw = "".join(seqs).encode()
    return np.frombuffer(raw, dtype=np.uint8), np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64)


def drain(st, n):
    out = [st.next() for _ in range(n)]
    assert st.next() is None
    return out


def test_stream_counts_only_batch_beside_a_hit_carrying_one(stream_set):
    s = stream_set
    P = len(s["mats"])
    pw = _lib.PwmSet(s["vals"], s["widths"], s["cutoffs"])
    st = _lib.Stream(pw, s["strand"], 0, depth=2)
    try:
        for order in ((True, False), (False, True)):
            for (seqs, _), co in zip(s["halves"], order):
                st.submit(*batch_of(seqs), counts_only=co)
            for res, (seqs, want), co in zip(drain(st, 2), s["halves"], order):
                try:
                    assert_counts(counts_of(res), cc.expected_counts(want, P), ("batch", order, co))
                    assert took_flag_map(res) == co
                    if not co:
                        h = res.hits()
                        for k in ("seq_idx", "pos", "score"):
                            assert np.array_equal(h[k], want[k]), k
                        assert np.array_equal(h["strand"].astype(np.int32), want["strand"].astype(np.int32))
                finally:
                    res.close()
    finally:
        st.close()
        pw.close()


def test_stream_no_hits_region_batches_of_a_resident_genome(oracle, stream_set):
    s = stream_set
    P = len(s["mats"])
    rng = np.random.default_rng(3)
    chroms = {"a": "".join(s["seqs"][:20]), "b": "".join(s["seqs"][20:]), "c": "ACGTN"}
    names, sizes = list(chroms), [len(v) for v in chroms.values()]
    batches = []
    for n_regions in (1, 9, 64):
        ci = rng.integers(0, 3, size=n_regions).astype(np.int32)
        start = np.array([rng.integers(0, sizes[c]) for c in ci], dtype=np.int64)
        end = np.array([rng.integers(a, min(sizes[c], a + 40) + 1) for c, a in zip(ci, start)], dtype=np.int64)
        end[0] = start[0] if n_regions > 1 else end[0]         # (an empty region in front)
        batches.append((ci, start, end))
    genome = _lib.ResidentGenome(chroms)
    pw = _lib.PwmSet(s["vals"], s["widths"], s["cutoffs"])
    st = _lib.Stream(pw, s["strand"], _lib.MS_STREAM_NO_HITS, depth=2)
    try:
        for rep in range(2):                               # (the second round in the queued, predicted-size form)
            got = []
            for ci, start, end in batches:
                while st.in_flight >= st.capacity:
                    got.append(st.next())
                st.submit_regions(genome, ci, start, end)
            got += drain(st, len(batches) - len(got))
            for res, (ci, start, end) in zip(got, batches):
                cut = [chroms[names[c]][a:b] for c, a, b in zip(ci, start, end)]
                try:
                    assert_counts(counts_of(res), oracle_counts(oracle, s["mats"], s["cutoffs"], cut, s["strand"]), ("regions", rep, len(ci)))
                finally:
                    res.close()
    finally:
        st.close()
        pw.close()
        genome.close()


def test_stream_dedup_beside_no_hits_dedups_a_batch(oracle, stream_set):
    """A counts-only BATCH under MS_STREAM_DEDUP goes down the ordered path and is de-duplicated: its site numbers are those of the
    de-duplicated ordered result (and of the oracle's restatement of scanner.py:156-193); de-duplication never empties a region."""
    s = stream_set
    P = len(s["mats"])
    seqs, want = s["halves"][0]
    off = want["motif_offsets"]
    cols = [want[k].tolist() for k in ("seq_idx", "pos", "score", "strand")]
    nested = [[[cols[0][k], cols[1][k], cols[2][k], cols[3][k]] for k in range(off[p], off[p + 1])] for p in range(P)]
    dd = oracle.deduplicate_motif_sites(oracle.make_motif_sites(nested, [0] * len(seqs)), s["widths"].tolist())
    kept = np.array([sum(len(sites) for sites in per) for per in dd], dtype=np.int64)
    assert 0 < kept.sum() < len(want["pos"])
    raw, offsets = batch_of(seqs)
    pw, sq = _lib.PwmSet(s["vals"], s["widths"], s["cutoffs"]), _lib.SeqSet(raw, offsets)
    ordered = _lib.scan(pw, sq, s["strand"]).dedup(pw)
    st = _lib.Stream(pw, s["strand"], _lib.MS_STREAM_DEDUP | _lib.MS_STREAM_NO_HITS, depth=2)
    try:
        for counts_only in (False, True):
            st.submit(raw, offsets, counts_only=counts_only)
            res = st.next()
            try:
                assert res.n_hits == ordered.n_hits == kept.sum()
                assert np.array_equal(res.motif_offsets, ordered.motif_offsets) and np.array_equal(np.diff(res.motif_offsets), kept)
                assert np.array_equal(res.region_counts(), cc.expected_counts(want, P)[2]) and np.array_equal(ordered.region_counts(), res.region_counts())
                assert not took_flag_map(res)
            finally:
                res.close()
    finally:
        st.close()
        ordered.close()
        sq.close()
        pw.close()


# ------------------------------------------------------------------------------------------------ the sweep's counts-only hand-out

@pytest.mark.parametrize("name", sorted(cc.sweep_count_cases(DIMS)))
def test_sweep_count_case_equals_the_oracle(oracle, name):
    case = cc.sweep_case_dict(cc.sweep_count_cases(DIMS)[name])
    ok, info = fuzz_parity.run_sweep_counts_case(name, oracle, _lib, case=case)
    assert ok, info
