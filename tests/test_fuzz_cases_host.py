"""
The cases of tests/fuzz_parity.py's variant, allele, best-site, sweep, scan-once and plot families without a GPU: that their seeds put what they should
on the decision boundary (fuzz_parity.CONDITIONS, tallied from the oracle's output alone -- the same conditions the GPU tests assert on
what they compared), and that the builders of the expected records are right, against the same scoring in plain Python floats (columns
in order, raw / max_raw, score - cutoff >= -1e-10) on every seed small enough for it.  For the scan-once family also that its tally's
view of the merged spans and of the hit keys' form is the library's own (_lib.union_bases, ms_debug_key_layout).
The genome and annot families need no scoring oracle for most of what they expect: their cases are checked here against plain Python --
byte counts, the oracle's convert_seq over the cut regions, a per-region loop of the reference's nearest-gene recurrence, any-overlap by
brute force -- and the three debug entries they are sized and driven by are checked as far as no GPU is needed.
"""
import ctypes
import os
import re

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

@pytest.mark.parametrize("family", ["variants", "alleles", "best", "once", "genome", "annot"])
def test_seeds_meet_the_conditions(request, family):
    if family == "genome":
        tallies = list(request.getfixturevalue("genome_tallies").values())
    elif family == "annot":
        tallies = [tally for _, _, _, tally in request.getfixturevalue("annot_expected")]
    else:
        tallies = [tally for _, _, _, tally in request.getfixturevalue("expected")[family]]
    total = {}
    for tally in tallies:
        fp.add_tally(total, tally)
    print(f"{family}: seeds {fp.SEEDS[family]}: {fp.shown(total)}")
    assert not fp.unmet_conditions(family, total)
    if family in ("genome", "annot"):                   # one counter per boundary: each at least 40 over the seeds, its floor at most half of it
        assert all(total[k] >= 40 and 2 * n <= total[k] for k, n in fp.CONDITIONS[family].items()), {k: total[k] for k in fp.CONDITIONS[family]}


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


# ------------------------------------------------------------------------------------------------ the genome and annot families

@pytest.fixture(scope="module")
def genome_tallies(oracle):
    """seed -> tally of the genome family, with every case checked against plain Python while it is at hand (a case holds 1.5 MB)."""
    dims, out = _lib.genome_dims(), {}
    for seed in fp.SEEDS["genome"]:
        case = fp.make_genome_case(seed, dims)
        want, out[seed] = fp.expected_genome(oracle, case)
        check_genome_case(oracle, seed, case, want, out[seed])
    return out


def unpacked(codes, nmask, n):
    """The planes as one int8 code per base, -1 under a mask bit: convert_seq's own output format."""
    i = np.arange(n)
    cw = codes[0::2].astype(np.uint64) | (codes[1::2].astype(np.uint64) << np.uint64(32))
    code = ((cw[i // 32] >> (2 * (i % 32)).astype(np.uint64)) & np.uint64(3)).astype(np.int8)
    return np.where((nmask[i // 32] >> (i % 32).astype(np.uint32)) & 1, np.int8(-1), code)


def check_genome_case(oracle, seed, case, want, tally):
    bases, goff, dims = case["bases"], case["goff"], case["dims"]
    # the expected planes are the oracle's convert_seq of the bytes, and keep the invariants the device's are asked for
    for (b, o), (codes, nmask, blk2reg, blkinfo) in zip(case["packs"], want["packs"]):
        assert np.array_equal(unpacked(codes, nmask, len(b)), oracle.convert_seq(b.tobytes())), seed
        assert fp.plane_invariants_broken(codes, nmask, len(b)) is None, seed
        assert np.all(o[blk2reg] <= 64 * np.arange(len(blk2reg))) and np.array_equal(blkinfo[:, 0], blk2reg), seed
    cut, offsets = fp.packed_cut(bases, goff, case["regions"])
    codes, nmask, blk2reg, blkinfo = want["extract"]
    assert np.array_equal(unpacked(codes, nmask, len(cut)), oracle.convert_seq(cut.tobytes())), seed
    assert fp.plane_invariants_broken(codes, nmask, len(cut)) is None, seed
    # blkinfo restated: the region of position 64 b (the last one that starts at or before it), its start and the next two, relative
    R = len(case["regions"])
    for b in {0, 1, len(blk2reg) // 2, len(blk2reg) - 2, len(blk2reg) - 1, *range(dims["pack_block_bases"] // 64 - 2, dims["pack_block_bases"] // 64 + 2)}:
        r = max(k for k in range(R) if offsets[k] <= 64 * b)
        assert blk2reg[b] == r, (seed, b)
        assert blkinfo[b].tolist() == [r, offsets[r] - 64 * b, offsets[min(r + 1, R)] - 64 * b, offsets[min(r + 2, R)] - 64 * b], (seed, b)
    assert tally["phase_table"].min() >= 1 and tally["extract_lengths"] == set(range(fp.EXTRACT_MAX_LEN + 1)), seed
    # base counts by bytes.count
    for (cl, a), w in zip(case["counts"], want["counts"]):
        off = np.concatenate([[0], np.cumsum(cl)])
        for c in {0, len(cl) - 1, *np.flatnonzero(np.asarray(cl) == 33)[:3].tolist(), int(np.argmax(cl))}:
            raw = a[off[c]:off[c + 1]].tobytes()
            assert w[c].tolist() == [raw.count(x) + raw.count(x.lower()) for x in (b"A", b"C", b"G", b"T")], (seed, c)
        assert int(w.sum()) == sum(a.tobytes().count(x) for x in (b"A", b"C", b"G", b"T", b"a", b"c", b"g", b"t")), seed
    # the window filter in plain Python: count N and n in the byte slice, keep the first n_want indices
    raw = bases.tobytes()
    for call, taken in zip(case["calls"], want["taken"]):
        L = call["length"]
        ok = [k for k, g in enumerate(call["gstart"].tolist()) if raw[g:g + L].count(b"N") + raw[g:g + L].count(b"n") <= call["max_n"]]
        assert taken.tolist() == ok[:call["n_want"]], seed
        assert call["gstart"].min() >= 0 and call["gstart"].max() + L <= len(raw), seed
    assert np.array_equal(want["exc_pos"], [i for i, x in enumerate(raw) if chr(x) not in "ACGTacgtNn"]), seed
    # the sampled windows hold at most max_n N / n
    names, arrs = fp.sampling_chroms(case)
    for sm, (ci, st, _) in zip(case["samples"], want["samples"]):
        assert len(ci) == sm["n_times"], seed
        for c, a in zip(ci.tolist(), st.tolist()):
            w = arrs[c][a:a + sm["length"]].tobytes()
            assert len(w) == sm["length"] and w.count(b"N") + w.count(b"n") <= sm["max_n"], seed
    # ranks: one motif with a NaN row at most, on the seeds that are meant to hold one; P no multiple of 3
    assert tally["rank_rows_with_nan"] == int(seed in fp.GENOME_NAN_SEEDS) <= 1, seed
    assert len(case["mats"]) % 3 and tally["max_raw_zero"] == tally["rank_rows_with_nan"], seed
    R = len(want["score_regions"])
    row = want["score"][case["strand"]]
    for p in np.flatnonzero(want["rank_compared"]).tolist():
        desc = -np.sort(-row[p], kind="stable")
        for k, r in enumerate(want["ranks"].tolist()):
            assert (np.isnan(want["rank_rows"][p, k]) and not 0 <= r < R) or want["rank_rows"][p, k] == desc[r], (seed, p, k)


def test_genome_nan_rows_are_capped(genome_tallies):
    """A motif whose oracle row holds a NaN is left out of the rank comparison: one per seed at most, GENOME_MAX_NAN_ROWS in all."""
    n = [t["rank_rows_with_nan"] for t in genome_tallies.values()]
    assert max(n) == 1 and 0 < sum(n) <= fp.GENOME_MAX_NAN_ROWS


@pytest.fixture(scope="module")
def annot_expected():
    dims, out = _lib.genome_dims(), []
    for seed in fp.SEEDS["annot"]:
        case = fp.make_annot_case(seed, dims)
        out.append((seed, case, *fp.expected_annot(None, case)))
    return out


def test_every_annot_seed_holds_the_three_kinds_of_block(annot_expected):
    for seed, _, _, tally in annot_expected:
        assert tally["lone_live_lane_blocks"] >= 1 and tally["lone_live_wave_blocks"] >= 1 and tally["blocks_frozen_in_tile_1"] >= 1, seed


def test_annot_restatements_equal_plain_loops(annot_expected):
    """nearest_restated (chunks of genes) against the reference's loop over one region's genes, on the lanes the scenarios are about and
    a sample of the others at every cutoff, and against the gene-by-gene numpy recurrence on every region of three seeds; the literal
    binary search against any-overlap by brute force where the two must agree (a hit is a real overlap; with intervals of one positive
    width no overlap is missed)."""
    for seed, case, want, _ in annot_expected:
        off, tss, strand, chrom, start = case["off"], case["tss"], case["strand"], case["near_chrom"], case["near_start"]
        rng = np.random.default_rng(seed)
        c_lone = case["sizes"].index(case["dims"]["gene_tile"] + 1)
        mine = np.flatnonzero(chrom == c_lone)
        block = case["dims"]["near_threads"]
        sample = {int(mine[case["lone"]]), int(mine[block + 64 * case["wave"]]), int(mine[block + 64 * (1 - case["wave"])]), int(mine[0 if case["lone"] else 1]),
                  *np.flatnonzero(chrom == case["sizes"].index(2 * case["dims"]["gene_tile"] + 1))[:2].tolist(),
                  *np.flatnonzero((chrom < 0) | (chrom >= len(case["sizes"]))).tolist(), *rng.integers(0, len(chrom), 12).tolist()}
        for cutoff in fp.ANNOT_CUTOFFS:
            dist, found = want["nearest"][cutoff]
            for r in sample:
                assert (int(dist[r]), bool(found[r])) == fp.nearest_plain(off, tss, strand, int(chrom[r]), int(start[r]), cutoff), (seed, cutoff, r)
            if seed < 3:
                d2, f2 = fp.nearest_stepwise(off, tss, strand, chrom, start, cutoff)
                assert np.array_equal(dist, d2) and np.array_equal(found, f2), (seed, cutoff)
        # the scenario lanes do what the case says they do, at the reference's own cutoff
        dist, found = want["nearest"][fp.ANNOT_CUTOFFS[0]]
        assert found[mine[case["lone"]]] and abs(int(dist[mine[case["lone"]]])) == 7, seed
        others = np.delete(mine[:block], case["lone"])
        assert found[others].all() and np.all(np.abs(dist[others]) < 3000), seed
        for call, got in zip(case["calls"], want["overlap"]):
            iv = fp.promoter_lists(case, call["upstream"], call["downstream"])
            for r in rng.integers(0, len(got), 60).tolist():
                ch, s_, e_ = int(call["chrom"][r]), int(call["start"][r]), int(call["end"][r])
                brute = 0 <= ch < len(iv) and any(not (e_ <= lo or s_ >= hi) for lo, hi in iv[ch])
                assert not got[r] or brute, (seed, r)
                if call["upstream"] + call["downstream"] > 0 and s_ < e_ and call["upstream"] == call["downstream"]:
                    assert got[r] == brute, (seed, r)


def test_genome_debug_entries_without_a_gpu():
    L = _lib.lib()
    out = (ctypes.c_int32 * 8)()
    assert L.ms_debug_genome_dims(out) == _lib.MS_OK
    d = _lib.genome_dims()
    assert list(out) == list(d.values()) and all(v > 0 for v in out)
    assert d["count_tile_bases"] % 32 == 0 and d["pack_block_bases"] % 64 == 0 and d["filter_threads"] % 64 == 0 and d["near_threads"] % 64 == 0
    assert d["rank_budget"] // 1_000_000 >= 100                    # build_motif's own n_random fits: a batch holds 100 motifs or more
    assert L.ms_debug_genome_dims(None) == _lib.MS_ERR_INVALID
    assert L.ms_debug_seqset_planes(None, None, None, None, None) == _lib.MS_ERR_INVALID
    prev = _lib.score_rank_budget(12345)
    try:
        assert prev == 0 and _lib.score_rank_budget(7) == 12345
        with pytest.raises(ValueError):
            _lib.score_rank_budget(-1)
        assert _lib.score_rank_budget(0) == 7
    finally:
        _lib.score_rank_budget(0)
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "motifscan_amd_debug.h")) as fh:
        text = fh.read()
    assert re.search(r"\bint\s+ms_debug_genome_dims\s*\(\s*int32_t\s+out\s*\[\s*8\s*\]\s*\)", text)
    assert re.search(r"\bint\s+ms_debug_seqset_planes\s*\(", text) and re.search(r"\bint\s+ms_debug_score_rank_budget\s*\(", text)
    for name in ("genome_dims", "seqset_planes", "score_rank_budget"):
        assert callable(getattr(_lib, name))


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
