"""
CPU-only: the pre-filter model's helpers (tests/prefilter_model.py) against the per-field emulation the plan's proof uses
(test_host_cabi.emulate_prefilter), the record list's round trip, hits_from_candidates on a case small enough to check by hand -- and that
every case of tests/test_gpu_prefilter_candidates.py and tests/test_gpu_fp64_from_candidates.py puts in front of the kernels what it claims
(prefilter_cases.CONDITIONS, fp64_cases.CONDITIONS), from the plan and the model alone.
"""
import numpy as np
import pytest

import fp64_cases as fc
import prefilter_cases as pc
import prefilter_model as pm
from motifscan_amd import _lib
from test_host_cabi import emulate_prefilter, field_strand, random_seqs


@pytest.fixture(scope="module", autouse=True)
def built():
    import os
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()


def _set_env(monkeypatch, env):
    monkeypatch.setenv("MS_MEASURE", "1")
    for k in ("MS_PF_DENSE", "MS_PF_RARE_CAP", "MS_PF_MAX_BLOCKS", "MS_PF_LDS_BUDGET", "MS_PF_PAIR", "MS_RESCORE_SORTED_MIN"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize("strand", [1, 2, 3])
def test_model_flags_is_the_per_field_emulation(rnd, strand):
    """on the small cases of the plan's proof: random PWMs at three cutoffs, sequences with and without runs of N"""
    rng = np.random.default_rng(5)
    seqs = random_seqs(rng, 2, 700, 0.0) + random_seqs(rng, 2, 500, 0.05) + ["N" * 90 + "ACGT" * 5, "a"]
    for pkey in ("1e-2", "1e-4"):
        plan = _lib.PwmSet.from_matrices(rnd["mats"], rnd["cutoff_by_key"][pkey]).plan(strand)
        for s in seqs:
            codes, isn = pm.encode(s)
            flags = pm.model_flags(plan, codes, isn)
            assert flags.shape == (plan["group_fields"].shape[0], len(s)) and flags.dtype == np.uint16
            got = {(int(plan["group_fields"][q, n]), int(g), field_strand(plan, n))
                   for q, g in zip(*np.nonzero(flags)) for n in range(16) if (flags[q, g] >> n) & 1}
            assert got == emulate_prefilter(plan, codes, isn)
            q, g = (int(v[0]) for v in np.nonzero(flags)) if flags.any() else (0, 0)
            for n in range(16):
                assert (pm.model_acc(plan, codes, isn, q, n, g) >= 0) == bool((flags[q, g] >> n) & 1)


def test_decode_records_round_trips_and_tallies():
    rng = np.random.default_rng(3)
    n_groups, L = 7, 300
    flags = (rng.integers(0, 1 << 16, size=(n_groups, L)) * (rng.random((n_groups, L)) < 0.2)).astype(np.uint16)
    rec = pm.pack_records(flags)
    assert len(rec) == np.count_nonzero(flags) and (rec != 0).all()
    back, t = pm.decode_records(rng.permutation(rec), n_groups, L)
    assert np.array_equal(back, flags) and t == {"empty": 0, "bad_g": 0, "bad_group": 0, "repeated": 0}
    extra = np.array([0, 0, 0, (L << 30) | (1 << 16) | 5, (3 << 30) | (n_groups << 16) | 1, int(rec[0]), int(rec[1]), int(rec[1])], dtype=np.uint64)
    back, t = pm.decode_records(np.concatenate([rec, extra]), n_groups, L)
    assert np.array_equal(back, flags) and t == {"empty": 3, "bad_g": 1, "bad_group": 1, "repeated": 3}
    g, q = int(rec[5] >> np.uint64(30)), int((rec[5] >> np.uint64(16)) & np.uint64(0x3FFF))
    assert int(rec[5] & np.uint64(0xFFFF)) == flags[q, g]
    assert pm.decode_records(np.zeros(0, dtype=np.uint64), 2, 0)[0].shape == (2, 0)


def test_dead_windows():
    isn = pm.encode("ACG" + "N" * 33 + "T" + "N" * 32 + "AC" + "N" * 40)[1]
    d = pm.dead_windows(isn, 32)
    assert np.flatnonzero(d).tolist() == [3, 4, 37, 71, 72, 73, 74, 75, 76, 77, 78, 79]      # a window past the end is not made of N only
    assert not pm.dead_windows(isn, 64).any()


def test_hits_from_candidates_keeps_what_is_flagged(oracle):
    """the word AAC on both strands and one 70-column motif (all-fp64 path: poly-A) on regions where AAC hits at the bases 0, 4 and 8"""
    mats = [np.log2(np.array([[.91, .91, .03], [.03, .03, .91], [.03, .03, .03], [.03, .03, .03]]) / .25), np.full((4, 70), -1.0)]
    mats[1][0] = 1.0
    vals, widths = pc.flat(mats)
    cut = np.array([0.9, 0.99])
    raw, offsets = b"AACTAACTAACT" + b"A" * 70, np.array([0, 4, 12, 82])
    plan = _lib.PwmSet(vals, widths, cut).plan(3)
    case = {"vals": vals, "widths": widths, "cutoffs": cut, "raw": raw, "offsets": offsets, "strand": 3, "plan": plan}
    full = oracle.scan_arrays(vals, widths, cut, raw, offsets, 3, 1)
    assert full["motif_offsets"].tolist() == [0, 3, 4] and full["pos"].tolist() == [0, 0, 4, 0] and full["seq_idx"].tolist() == [0, 1, 1, 2]
    (q, n), = [(q, n) for q, n in zip(*np.nonzero(plan["group_fields"] == 0)) if n % 2 == 1]      # the reverse strand's field keeps the forward hit too
    flags = np.zeros((plan["group_fields"].shape[0], 82), dtype=np.uint16)
    flags[q, 4] = 1 << n
    got = pm.hits_from_candidates(oracle, case, flags)
    assert got["motif_offsets"].tolist() == [0, 1, 2] and got["pos"].tolist() == [0, 0] and got["seq_idx"].tolist() == [1, 2]
    flags[q, 0] = flags[q, 8] = 1 << (n - 1)
    got = pm.hits_from_candidates(oracle, dict(case, oracle=full), flags)
    assert all(np.array_equal(got[k], full[k]) for k in full)


@pytest.mark.parametrize("name", sorted(pc.CASES))
def test_prefilter_case_meets_its_conditions(monkeypatch, name):
    case = pc.CASES[name]
    _set_env(monkeypatch, case["env"])
    b = pc.build(case, _lib)
    plan = b["plan"]
    fast = set(plan["group_fields"][plan["group_fields"] >= 0].tolist())
    wide64 = [i for i, w in enumerate(b["widths"]) if w > 63]
    assert plan["exact_motifs"].tolist() == wide64 and fast == set(range(len(b["widths"]))) - set(wide64)
    assert (len(wide64) == 1) == (case["set"] == "wide")
    widths = set(b["widths"].tolist())
    assert {"narrow": {1, 7, 8, 15, 16, 23, 24, 31}, "alln": {10}, "wide": {1, 15, 16, 31, 32, 47, 48, 63, 64}}.get(case["set"], set()) <= widths
    assert len(b["text"]) == (case["prefix"] or case["seq"][1] or len(b["text"]))
    t = pc.tally(plan, b["model"], b["isn"], case, b["widths"])
    print(name, len(b["text"]), "bases:", {k: v for k, v in t.items() if k != "forms"})
    assert not pc.unmet(case, t), pc.unmet(case, t)
    alln = any(b["cutoffs"] == 0.0)
    assert alln == (case["expect"].get("skip_alln", 1) == 0)      # (a bias >= 0 alone does not make it so: the shortest motifs have one at any cutoff)
    if case["kind"] == "counter":
        blocks, pw = case["expect"]["blocks_per_tile"], case["expect"]["pass_windows"]
        n = len(b["text"])
        assert pc.counter_point(blocks, pw) < n <= pc.counter_point(blocks, pw) + 1024 and -(-n // (2 * pw)) > 16 * blocks      # more units (of 2 passes) than waves


@pytest.mark.parametrize("name", sorted(fc.SETS))
def test_fp64_case_meets_its_conditions(oracle, name):
    case = fc.build(name, _lib, oracle)
    t = fc.tally(case, oracle)
    print(name, t)
    assert not fc.unmet(name, t), fc.unmet(name, t)
