"""
The cases of tests/fuzz_parity.py's variant, allele, best-site, sweep, scan-once and plot families without a GPU: that their seeds put what they should
on the decision boundary (fuzz_parity.CONDITIONS, tallied from the oracle's output alone -- the same conditions the GPU tests assert on
what they compared), and that the builders of the expected records are right, against the same scoring in plain Python floats (columns
in order, raw / max_raw, score - cutoff >= -1e-10) on every seed small enough for it.  For the scan-once family also that its tally's
view of the merged spans and of the hit keys' form is the library's own (_lib.union_bases, ms_debug_key_layout).
"""
import numpy as np
import pytest

import fuzz_parity as fp
from motifscan_amd import _lib

PYTHON_MAX_PAIRS = 2000                                 # (window, strand[, allele]) pairs a case may hold to be redone in Python
CODE = {c: i for i, c in enumerate("ACGT")}
CODE.update({c.lower(): i for c, i in list(CODE.items())})


@pytest.fixture(scope="module")
def expected(oracle):
    """family -> [(seed, case, expected arrays, tally)] over the family's seeds, computed once."""
    seg = _lib.best_segment_windows()
    out = {"variants": [], "alleles": [], "best": [], "once": []}
    for seed in fp.SEEDS["variants"]:
        case = fp.make_variants_case(seed)
        out["variants"].append((seed, case, *fp.expected_variants(oracle, case)))
    for seed in fp.SEEDS["alleles"]:
        case = fp.make_alleles_case(seed)
        out["alleles"].append((seed, case, *fp.expected_alleles(oracle, case)))
    for seed in fp.SEEDS["best"]:
        case = fp.make_best_case(seed)
        out["best"].append((seed, case, *fp.expected_best(oracle, case, seg)))
    for seed in fp.SEEDS["once"]:
        case = fp.make_once_case(seed)
        out["once"].append((seed, case, *fp.expected_once(oracle, case)))
    return out


# ------------------------------------------------------------------------------------------------ the conditions

@pytest.mark.parametrize("family", ["variants", "alleles", "best", "once"])
def test_seeds_meet_the_conditions(expected, family):
    total = {}
    for _, _, _, tally in expected[family]:
        fp.add_tally(total, tally)
    print(f"{family}: seeds {fp.SEEDS[family]}: {fp.shown(total)}")
    assert not fp.unmet_conditions(family, total)


def test_sweep_seeds_meet_the_conditions(oracle):
    total = {}
    for seed in fp.SEEDS["sweep"]:
        fp.add_tally(total, fp.sweep_tally(seed, oracle))
    print(f"sweep: seeds {fp.SEEDS['sweep']}: {total}")
    assert not fp.unmet_conditions("sweep", total)


def test_generators_reach_the_edges(expected):
    """What the families promise beside the tallies: every strand mask, variants at both chromosome ends, alt letters that add nothing,
    insertions behind the last base, deletions, long alleles, REF strings that match and that do not, regions of three segments."""
    v = [case for _, case, _, _ in expected["variants"]]
    assert {c["strand"] for c in v} == {1, 2, 3}
    assert any(np.any(c["pos"] == 0) for c in v) and any(np.any(c["pos"] == np.array([len(s) for s in c["chroms"]])[c["chrom_idx"]] - 1) for c in v)
    assert any(len(np.unique(c["chrom_idx"].astype(np.int64) << 32 | c["pos"])) < len(c["pos"]) for c in v)      # duplicates
    assert {chr(b) for c in v for b in c["alt"]} == set(fp.ALT_LETTERS)
    assert all(sum(t[f"state_{s}"] for _, _, _, t in expected["variants"]) > 1000 for s in (1, 2, 3))
    a = [case for _, case, _, _ in expected["alleles"]]
    assert {c["strand"] for c in a} == {1, 2, 3}
    assert sum(t["at_chrom_end"] for _, _, _, t in expected["alleles"]) > 0
    assert any(np.any(c["ref_len"] == 0) for c in a) and any("" in c["alts"] for c in a)
    assert any(np.any(c["ref_len"] > 3) for c in a) and any(max(map(len, c["alts"])) > 3 for c in a)
    with_refs = [(c, w) for _, c, w, _ in expected["alleles"] if c["refs"] is not None]
    assert len(with_refs) == len(a) // 2 and all(not w["ref_mismatch"].any() for _, c, w, _ in expected["alleles"] if c["refs"] is None)
    assert sum(int(w["ref_mismatch"].sum()) for _, w in with_refs) > 100 and sum(int((~w["ref_mismatch"]).sum()) for _, w in with_refs) > 100
    b = [case for _, case, _, _ in expected["best"]]
    seg = _lib.best_segment_windows()
    assert {c["strand"] for c in b} == {1, 2, 3}
    assert any(len(s) > 2 * seg for c in b for s in c["seqs"]) and any(s == "" for c in b for s in c["seqs"])
    assert any(np.isnan(w[0]).any() for _, _, w, _ in expected["best"]) and any((w[1] >= 0).any() for _, _, w, _ in expected["best"])


def test_plot_seeds_meet_the_conditions_and_the_integer_bin_rule():
    """The plot family needs no oracle: its tallies come from numpy's own histogram and prefix counts.  Every case is also binned by the
    rule the kernel uses -- t = 2 * (pos - summit) + W + 2 * (extend + 5) in integers, bin t / 20, the last bin closed -- which must
    agree with np.histogram everywhere, and a sample of ranks is redone as the reference's slice sum."""
    total, dims = {}, _lib.plot_dims()
    for seed in fp.SEEDS["plot"]:
        case = fp.make_plot_case(seed, dims)
        want, tally = fp.expected_plot(case)
        fp.add_tally(total, tally)
        off, n_bins = case["motif_offsets"], want["counts"].shape[1]
        assert n_bins == fp.plot_n_bins(case["extend"]) and sorted(case["order"].tolist()) == list(range(case["R"])), seed
        m = np.repeat(np.arange(case["P"]), np.diff(off))
        t = 2 * (case["pos"] - case["summit_rel"][case["region"]]) + case["widths"][m].astype(np.int64) + 2 * (case["extend"] + 5)
        b = np.where(t == 20 * n_bins, n_bins - 1, t // 20)
        ok = (t >= 0) & (b < n_bins)
        rule = np.zeros_like(want["counts"])
        np.add.at(rule, (m[ok], b[ok]), 1)
        assert np.array_equal(rule, want["counts"]) and tally["in_range"] == int(ok.sum()), seed
        R, f = case["R"], case["R"] // 100
        for row in range(case["P"]):
            has = np.zeros(R, dtype=bool)
            has[case["region"][off[row]:off[row + 1]]] = True
            flags = has[case["order"]].tolist()
            for i in {0, 1, f - 1, f, f + 1, R // 2, R - f - 1, R - f, R - 2, R - 1}:
                head, tail = max(0, i - f), min(i + f, R)
                assert want["raw"][row, i] == sum(flags[head:tail]) / (tail - head) / float(case["ratio"][row]), (seed, row, i)
    print(f"plot: seeds {fp.SEEDS['plot']}: {fp.shown(total)}")
    assert not fp.unmet_conditions("plot", total)
    assert 0 < total["cases_without_sites"] <= fp.PLOT_MAX_EMPTY


# ------------------------------------------------------------------------------------------------ the builders, against Python floats

def python_windows(mat, seq, strand_mask):
    """[(pos, strand, score)] of every window x strand of the mask, the reference's walk in plain Python floats; nothing for a motif
    whose max_raw is 0 (raw / 0 is -inf or NaN: the reference never reports a site of it)."""
    W, rows = mat.shape[1], mat.tolist()
    max_raw = 0.0
    for c in range(W):
        max_raw += max(0.0, max(rows[b][c] for b in range(4)))
    out = []
    if max_raw == 0.0:
        return out
    for p in range(len(seq) - W + 1):
        fwd = rev = 0.0
        for c in range(W):
            b = CODE.get(seq[p + c])
            if b is not None:
                fwd += rows[b][c]
                rev += rows[3 - b][W - 1 - c]
        for s, raw in ((1, fwd), (2, rev)):
            if strand_mask & s:
                out.append((p, s, raw / max_raw))
    return out


def passes(score, cutoff):
    return score - cutoff >= -1e-10


def small_cases(expected, family):
    cases = [(seed, case, want) for seed, case, want, tally in expected[family] if 0 < tally["pairs"] <= PYTHON_MAX_PAIRS]
    assert len(cases) >= 5, f"{family}: only {len(cases)} seeds are small enough to be redone in Python"
    return cases


def columns(records, dtypes):
    return [np.array([r[i] for r in records], dtype=dt) for i, dt in enumerate(dtypes)]


def test_expected_variants_equal_python_floats(expected):
    for seed, case, want in small_cases(expected, "variants"):
        recs, offsets, gained, lost = [], [0], [], []
        alt = case["alt"].decode()
        for mat, cutoff in zip(case["mats"], case["cutoffs"]):
            W = mat.shape[1]
            g, l = set(), set()
            for v, (ci, x) in enumerate(zip(case["chrom_idx"].tolist(), case["pos"].tolist())):
                seq = case["chroms"][ci]
                lo, hi = max(0, x - W + 1), min(len(seq), x + W)
                ref_w = python_windows(mat, seq[lo:hi], case["strand"])
                alt_w = python_windows(mat, seq[lo:x] + alt[v] + seq[x + 1:hi], case["strand"])
                for (p, s, qr), (_, _, qa) in zip(ref_w, alt_w):
                    state = int(passes(qr, cutoff)) | int(passes(qa, cutoff)) << 1
                    if state:
                        recs.append((v, lo + p, s, qr, qa, state))
                        g.update([v] if state == 2 else [])
                        l.update([v] if state == 1 else [])
            offsets.append(len(recs))
            gained.append(len(g)), lost.append(len(l))
        variant, start, strand, qr, qa, state = columns(recs, (np.int64, np.int64, np.int8, np.float64, np.float64, np.uint8))
        for k, a in (("variant", variant), ("start", start), ("strand", strand), ("state", state), ("motif_offsets", offsets), ("gained", gained),
                     ("lost", lost)):
            assert np.array_equal(want[k], a), (seed, k)
        assert fp.same_bits(want["score_ref"], qr) and fp.same_bits(want["score_alt"], qa), seed
        codes = [CODE.get(case["chroms"][ci][x], -1) for ci, x in zip(case["chrom_idx"].tolist(), case["pos"].tolist())]
        assert want["ref_codes"].tolist() == codes, seed


def test_expected_alleles_equal_python_floats(expected):
    for seed, case, want in small_cases(expected, "alleles"):
        recs, offsets, gained, lost = [], [0], [], []
        for mat, cutoff in zip(case["mats"], case["cutoffs"]):
            W = mat.shape[1]
            g = l = 0
            for v, (ci, x, r) in enumerate(zip(case["chrom_idx"].tolist(), case["pos"].tolist(), case["ref_len"].tolist())):
                seq, a = case["chroms"][ci], case["alts"][v]
                lo, hi = max(0, x - W + 1), min(len(seq), x + r + W - 1)
                n = [0, 0]
                for allele, flank in ((0, seq[lo:hi]), (1, seq[lo:x] + a + seq[x + r:hi])):
                    for p, s, q in python_windows(mat, flank, case["strand"]):
                        if passes(q, cutoff):
                            recs.append((v, allele, lo + p, s, q))
                            n[allele] += 1
                g += n[1] > 0 and n[0] == 0
                l += n[0] > 0 and n[1] == 0
            offsets.append(len(recs))
            gained.append(g), lost.append(l)
        variant, allele, start, strand, q = columns(recs, (np.int64, np.uint8, np.int64, np.int8, np.float64))
        for k, a in (("variant", variant), ("allele", allele), ("start", start), ("strand", strand), ("motif_offsets", offsets), ("gained", gained),
                     ("lost", lost)):
            assert np.array_equal(want[k], a), (seed, k)
        assert fp.same_bits(want["score"], q), seed
        if case["refs"] is not None:
            differs = [any(CODE.get(g) != CODE.get(q) for g, q in zip(case["chroms"][ci][x:x + r], ref))
                       for ci, x, r, ref in zip(case["chrom_idx"].tolist(), case["pos"].tolist(), case["ref_len"].tolist(), case["refs"])]
            assert want["ref_mismatch"].tolist() == differs, seed


def test_expected_best_equals_python_floats(expected):
    for seed, case, want in small_cases(expected, "best"):
        score, pos, strand = want
        assert score.shape == (len(case["mats"]), len(case["seqs"]))
        for m, mat in enumerate(case["mats"]):
            for r, seq in enumerate(case["seqs"]):
                best, where = -np.inf, (-1, 0)
                for p, s, q in python_windows(mat, seq, case["strand"]):
                    if q > best:                        # replace iff greater: ties keep the earlier window, '+' before '-'
                        best, where = q, (p, s)
                assert (int(pos[m, r]), int(strand[m, r])) == where, (seed, m, r)
                if where[1]:
                    assert fp.same_bits(score[m, r], best), (seed, m, r)
                else:
                    assert np.isnan(score[m, r]), (seed, m, r)


def test_expected_once_equals_python_floats(expected):
    for seed, case, want in small_cases(expected, "once"):
        recs, offsets = [], [0]
        for mat, cutoff in zip(case["mats"], case["cutoffs"]):
            for r, (c, a, b) in enumerate(zip(case["chrom_idx"].tolist(), case["start"].tolist(), case["end"].tolist())):
                recs += [(r, p, s, q) for p, s, q in python_windows(mat, case["chroms"][c][a:b], case["strand"]) if passes(q, cutoff)]
            offsets.append(len(recs))
        region, pos, strand, q = columns(recs, (np.int64, np.int64, np.int8, np.float64))
        for k, a in (("seq_idx", region), ("pos", pos), ("strand", strand), ("motif_offsets", offsets)):
            assert np.array_equal(want[k], a), (seed, k)
        assert fp.same_bits(want["score"], q), seed


# ------------------------------------------------------------------------------------------------ the scan-once tally's view of the spans

def test_once_span_merge_agrees_with_union_bases(expected):
    for seed, case, _, _ in expected["once"]:
        order, span_of, sp_chrom, sp_start, sp_end = fp.merge_spans(case["chrom_idx"], case["start"], case["end"])
        assert int((sp_end - sp_start).sum()) == _lib.union_bases(case["chrom_idx"], case["start"], case["end"]), seed
        # spans are ordered, apart (they may touch) and every region lies inside its own
        same = sp_chrom[1:] == sp_chrom[:-1]
        assert np.all(np.diff(sp_chrom) >= 0) and np.all(sp_start[1:][same] >= sp_end[:-1][same]), seed
        assert np.all(case["start"][order] >= sp_start[span_of]) and np.all(case["end"][order] <= sp_end[span_of]), seed
        assert np.array_equal(case["chrom_idx"][order], sp_chrom[span_of]), seed


def test_once_key_form_is_the_librarys(expected):
    """cases_local / cases_global of the tally say which form of hit key ms_scan_regions_once's span scan takes by itself: held against
    key_layout (ms_scan_geom.cpp) through ms_debug_key_layout on every seed's span set, so that the restatement cannot drift."""
    for seed, case, want, tally in expected["once"]:
        n_bases, n_spans, longest = fp.once_span_shape(case)
        gbits, pbits = _lib.key_layout(n_bases, n_spans, longest, len(case["mats"]))
        assert (1 << gbits) > n_bases or pbits > 0, seed
        assert fp.default_key_form(n_bases, n_spans, longest) == ("local" if pbits > 0 else "global"), seed
        has = int(len(want["pos"]) > 0)
        assert (tally["cases_local"], tally["cases_global"]) == ((has, 0) if pbits > 0 else (0, has)), seed
        assert _lib.key_layout(n_bases, n_spans, longest, len(case["mats"]), coord_global=True)[1] == 0, seed
    assert _lib.key_layout(64 * 256, 64, 256, 5)[1] > 0                       # 64 spans of 256 bases: (span, position)
    assert _lib.key_layout(63 * 40 + 5000, 64, 5000, 5)[1] == 0               # 63 spans of 40 bases and one of 5000: global positions
    with pytest.raises(ValueError):
        _lib.key_layout(10, 1, 11, 1)
