"""
The cases of tests/counts_cases.py without a GPU: that the dims come from the library, that expected_counts and closed_form_counts are
right against plain loops and the oracle, and -- from the oracle alone -- that every named case holds what it claims: the hit numbers,
P x R against ratio x n for every case that must take the flag map, the empty motifs at the prefix kernel's thread-range edges, the
flag bytes that are neighbours across two rows, windows that take sites from more than one hit and hits that fall in no window.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import counts_cases as cc
import fuzz_parity as fp
from motifscan_amd import _lib


@pytest.fixture(scope="module")
def dims():
    return _lib.counts_dims()


def oracle_hits(oracle, mats, cutoffs, seqs, strand):
    vals, widths, raw, offsets = cc.flat(mats, seqs)
    return oracle.scan_arrays(vals, widths, cutoffs, raw, offsets, strand, 4)


@pytest.fixture(scope="module")
def flag_cases(oracle, dims):
    """name -> (case, oracle hits or None for the one case too large for it, (n_hits, motif_offsets, region_counts))."""
    out = {}
    for name, case in cc.flag_map_cases(dims).items():
        mats, cutoffs, seqs, strand, _ = case
        want = None if name == "second_trip" else oracle_hits(oracle, mats, cutoffs, seqs, strand)
        out[name] = (case, want, cc.closed_form_of(case) if want is None else cc.expected_counts(want, len(mats)))
    return out


def same_counts(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


# ------------------------------------------------------------------------------------------------ the dims and the restatements

def test_counts_dims_come_from_the_library(dims):
    L = _lib.lib()
    out = (ctypes.c_int32 * 8)()
    assert L.ms_debug_counts_dims(out) == _lib.MS_OK
    assert list(out)[:7] == list(dims.values()) and out[7] == 0 and all(v > 0 for v in list(out)[:7])
    assert L.ms_debug_counts_dims(None) == _lib.MS_ERR_INVALID
    assert dims["threads"] % 64 == 0 and dims["sweep_threads"] % 64 == 0 and dims["keys_per_block"] % dims["threads"] == 0
    assert dims["bins"] >= 2 * dims["threads"] + 1                    # the P edges of the cases are distinct
    with open(os.path.join(fp.ROOT, "include", "motifscan_amd_debug.h")) as fh:
        assert re.search(r"\bint\s+ms_debug_counts_dims\s*\(\s*int32_t\s+out\s*\[\s*8\s*\]\s*\)", fh.read())
    # the code reads the constants it reports, not literals of its own
    src = os.path.join(fp.ROOT, "motifscan_amd", "csrc")
    with open(os.path.join(src, "ms_regions.hip")) as fh:
        launch = fh.read().split("int launch_count_only(")[1].split("\n}\n")[0]
    assert not re.search(r"\b(256|2048|4095|4096)\b", launch)
    with open(os.path.join(src, "ms_scan.hip")) as fh:
        gate = fh.read().split("static bool scan_counts_fast(")[1].split("\n}\n")[0]
    assert "kCountsGateRatio" in gate and not re.search(r"\b50(\.0)?\b", gate)
    with open(os.path.join(src, "ms_sweep.hip")) as fh:
        sweep = fh.read().split("static int sweep_counts_only(")[1].split("\n}\n")[0]
    assert "kSweepCountMaxMotifs" in sweep and "65536" not in sweep


def test_expected_counts_equals_plain_loops(oracle):
    rng = np.random.default_rng(5)
    mats = [cc.small_int_matrix(rng, w) for w in (1, 2, 3, 4, 2)]
    seqs = ["", "ACGTTGCAAC", "AC", "GGGGGGGGGGGG", "ANNACGTNNCA", "acgtacgtac"]
    cutoffs = np.array([cc.ALL_PASS, 0.5, cc.NEVER, 0.0, 1.0])
    want = oracle_hits(oracle, mats, cutoffs, seqs, 3)
    n, offsets, regions = cc.expected_counts(want, len(mats))
    assert n == len(want["pos"]) > 50 and offsets[0] == 0 and offsets[-1] == n and offsets[2] == offsets[3]
    for m in range(len(mats)):
        seen = {int(r) for r in want["seq_idx"][offsets[m]:offsets[m + 1]]}
        assert regions[m] == len(seen)
    assert regions[0] == 5 and regions[2] == 0
    empty = {"pos": np.zeros(0, np.int64), "seq_idx": np.zeros(0, np.int64), "motif_offsets": np.zeros(4, np.int64)}
    assert same_counts(cc.expected_counts(empty, 3), (0, np.zeros(4, np.int64), np.zeros(3, np.int64)))


@pytest.mark.parametrize("strand", [1, 2, 3])
def test_closed_form_equals_the_oracle(oracle, strand):
    """Regions shorter than a motif, as long as one, empty ones; motifs that pass everything and nothing."""
    rng = np.random.default_rng(9 + strand)
    widths = [1, 3, 5, 2, 20, 7]
    mats = [cc.small_int_matrix(rng, w) for w in widths]
    passes = np.array([True, True, False, True, True, True])
    seqs = [cc.random_dna(rng, L) for L in (0, 1, 2, 3, 5, 7, 19, 20, 21, 30, 0)]
    cutoffs = np.where(passes, cc.ALL_PASS, cc.NEVER)
    want = cc.expected_counts(oracle_hits(oracle, mats, cutoffs, seqs, strand), len(mats))
    got = cc.closed_form_counts(widths, [len(s) for s in seqs], passes, cc.n_strands(strand))
    assert same_counts(got, want) and got[0] > 0
    assert got[2].tolist() == [9, 7, 0, 8, 3, 5]
    assert same_counts(cc.closed_form_of((mats, cutoffs, seqs, strand, True)), want)


# ------------------------------------------------------------------------------------------------ the flag-map cases

def test_flag_map_cases_are_the_named_sizes(flag_cases, dims):
    bins, T, kpb = dims["bins"], dims["threads"], dims["keys_per_block"]
    sizes = lambda prefix: sorted(int(k.split("_")[1]) for k in flag_cases if re.fullmatch(prefix + r"_\d+", k))
    assert sizes("P") == sorted({1, 2, T - 1, T, T + 1, 2 * T - 1, 2 * T + 1, bins - 1, bins, bins + 1})
    assert sizes("n") == sorted({1, 63, 64, 65, 255, 256, 257, kpb - 1, kpb, kpb + 1, 2 * kpb + 1})
    assert sorted({int(k.split("_")[1]) for k in flag_cases if k.startswith("R_")}) == [1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 257]
    for name, (case, _, (n, offsets, regions)) in flag_cases.items():
        mats, cutoffs, seqs, strand, must = case
        if name.startswith("P_") and name != "P_1_no_hit":
            assert len(mats) == int(name.split("_")[1]) and 5 <= len(seqs) <= 9, name
            assert all(10 <= len(s) <= 16 for s in seqs) and all(1 <= m.shape[1] <= 3 for m in mats), name
        if name.startswith("R_"):
            assert len(seqs) == int(name.split("_")[1]) and len(mats) == 3, name
        if name.startswith("n_"):
            assert n == int(name.split("_")[1]), name
        assert all(fp.max_raw_of(m) > 0 for m in mats), name
    assert flag_cases["second_trip"][2][0] == dims["max_blocks"] * kpb + 65
    assert 200 <= len(flag_cases["second_trip"][0][2]) + 160 and len(flag_cases["second_trip"][0][2]) >= 40
    assert flag_cases["P_1_no_hit"][2][0] == 0


def test_flag_map_gate_holds_for_every_case_that_must_take_it(flag_cases, dims):
    """scan_counts_fast restated: the flag map is taken iff the form is supported (region-local keys, P <= bins) and P x R <= ratio x
    max(n, 1) -- on a set's first scan n is the true number of hits."""
    n_must = 0
    for name, (case, _, (n, _, _)) in flag_cases.items():
        mats, cutoffs, seqs, strand, must = case
        P, R = len(mats), len(seqs)
        gbits, pbits = _lib.key_layout(sum(map(len, seqs)), R, max(map(len, seqs)), P)
        supported = pbits > 0 and 0 < P <= dims["bins"] and P * (R + 16) <= 6.0e9
        assert must == (supported and P * R <= dims["gate_ratio"] * max(n, 1)), name
        assert pbits > 0, name                             # (no case loses the form by its key layout: each refusal is the one it is named for)
        n_must += must
    assert n_must == len(flag_cases) - 2
    assert not flag_cases[f"P_{dims['bins'] + 1}"][0][4] and not flag_cases["gate_off"][0][4]
    # the gate's edge: equality takes the map; one hit fewer, by one base, does not
    (on, _, (n_on, _, _)), (off, _, (n_off, _, _)) = flag_cases["gate_on"], flag_cases["gate_off"]
    P, R = len(on[0]), len(on[2])
    assert P * R == dims["gate_ratio"] * n_on and n_off == n_on - 1 and P * R == dims["gate_ratio"] * n_off + dims["gate_ratio"]
    assert sum(a != b for a, b in zip("".join(on[2]), "".join(off[2]))) == 1 and [len(s) for s in on[2]] == [len(s) for s in off[2]]
    assert len({len(s) for s in on[2]}) == 1


def test_p_edge_cases_put_empty_motifs_on_the_prefix_kernels_edges(flag_cases, dims):
    T, last_ranges = dims["threads"], set()
    for name, (case, _, (n, offsets, regions)) in flag_cases.items():
        if not re.fullmatch(r"P_\d+", name):
            continue
        P = len(case[0])
        sites = np.diff(offsets)
        empty = sites == 0
        assert np.array_equal(empty, regions == 0), name
        assert np.all(empty[case[1] == cc.NEVER]), name
        if P <= 2:
            assert not empty[P - 1] and (P == 1 or empty[0]), name
            continue
        assert empty[0] and empty[P - 1] and not empty.all(), name
        assert 0.25 <= empty.mean() <= 0.55, (name, empty.mean())
        per, edges = cc.prefix_ranges(P, T)
        assert per == -(-P // T) and all(0 < e < P for e in edges), name
        left = sum(empty[e - 1] and not empty[e] for e in edges)
        right = sum(empty[e] and not empty[e - 1] for e in edges)
        both = sum(empty[e - 1] and empty[e] for e in edges)
        neither = sum(not empty[e - 1] and not empty[e] for e in edges)
        assert left >= 3 and right >= 3 and both >= 3 and neither >= 3, (name, left, right, both, neither)
        assert np.any(empty[1:-1] & empty[2:]) and np.any(offsets[1:-1] == offsets[2:]), name        # runs: equal neighbours in motif_first
        assert len(set(sites[~empty].tolist())) > 3, name                                       # ... between unequal steps
        last = min(P, T * per) - min(P, (T - 1) * per)     # motifs in the range of the last thread, the one that writes motif_first[P]
        last_ranges.add("empty" if last == 0 else "full" if last == per else "short")
    assert last_ranges == {"empty", "short", "full"}


def test_r_edge_cases_put_hits_in_the_cells_they_name(flag_cases):
    for name, (case, want, (n, offsets, regions)) in flag_cases.items():
        if not name.startswith("R_"):
            continue
        mats, cutoffs, seqs, strand, must = case
        R = len(seqs)
        cells = np.zeros((3, R), dtype=np.int64)
        np.add.at(cells, (np.repeat(np.arange(3), np.diff(offsets)), want["seq_idx"]), 1)
        if name.endswith("random"):
            assert np.all(cells[0] > 0) and regions[0] == R, name          # a flag in every byte of row 0, the unused bytes of its last word beside row 1
        elif name.endswith("empty_ends"):
            assert seqs[0] == "" and seqs[-1] == "" and not cells[:, 0].any() and not cells[:, -1].any() and np.all(cells[0, 1:-1] > 0), name
        elif name.endswith("cross"):
            only = np.zeros_like(cells)
            only[0, R - 1] = only[1, 0] = 16
            assert np.array_equal(cells, only), name
        else:
            assert name.endswith("last_region") and not cells[:, :-1].any() and np.all(cells[:, -1] > 0), name


def test_many_motif_cases_hold_each_motif_at_most_twice(flag_cases):
    for R in (1, 4):
        case, want, (n, offsets, regions) = flag_cases[f"many_motifs_R_{R}"]
        sites = np.diff(offsets)
        assert len(case[0]) == 300 and len(case[2]) == R and set(sites.tolist()) == {0, 1, 2}, R
        assert all(6 <= m.shape[1] <= 8 for m in case[0]) and np.all(case[1] == 1.0)
        assert min((sites == k).sum() for k in (0, 1, 2)) >= 60
        # neighbours in position are different motifs: 64 consecutive hits of a region hold many of them
        order = np.lexsort((want["pos"], want["seq_idx"]))
        motif = np.repeat(np.arange(300), sites)[order]
        assert min(len(set(motif[a:a + 64].tolist())) for a in range(0, max(1, n - 64), 16)) >= 40


def test_closed_form_cases_equal_the_oracle(flag_cases):
    n_checked = 0
    for name, (case, want, counts) in flag_cases.items():
        if cc.is_closed_form(name) and want is not None:
            assert same_counts(cc.closed_form_of(case), counts), name
            n_checked += 1
    assert n_checked == 11
    case = flag_cases["second_trip"][0]
    assert all(set(s) <= set("ACGT") for s in case[2]) and np.all(case[1] == cc.ALL_PASS) and max(len(s) for s in case[2]) - min(len(s) for s in case[2]) <= 1


# ------------------------------------------------------------------------------------------------ the sweep-count cases

def restated_sweep_counts(hits, widths, window, stride, n_win):
    """(n_sites, motif_offsets, window_counts, tally) from the hits of the span scanned as ONE region, by the definition: a hit is a site
    of every window that holds it whole."""
    P = len(widths)
    sites, windows = np.zeros(P, dtype=np.int64), [set() for _ in range(P)]
    tally = {"hits": len(hits["pos"]), "hits_in_no_window": 0, "shared_windows": 0, "two_hits_at_one_position": 0, "first_hit_behind_another_motifs": 0}
    off = hits["motif_offsets"]
    prev_last = None                                      # the window range of the hit in front of a motif's first one, another motif's
    for m in range(P):
        W, seen_twice = int(widths[m]), set()
        pos = hits["pos"][off[m]:off[m + 1]].tolist()
        for i, p in enumerate(pos):
            ks = cc.hit_windows(p, W, window, stride, n_win)
            sites[m] += len(ks)
            tally["hits_in_no_window"] += not ks
            seen_twice |= windows[m] & set(ks)
            windows[m] |= set(ks)
            tally["two_hits_at_one_position"] += i > 0 and pos[i - 1] == p
            if i == 0 and ks and prev_last is not None and cc.hit_windows(prev_last, W, window, stride, n_win) and \
                    max(cc.hit_windows(prev_last, W, window, stride, n_win)) >= min(ks):
                tally["first_hit_behind_another_motifs"] += 1
        tally["shared_windows"] += len(seen_twice)
        if pos:
            prev_last = pos[-1]
    return int(sites.sum()), np.concatenate([[0], np.cumsum(sites)]), np.array([len(w) for w in windows], dtype=np.int64), tally


@pytest.fixture(scope="module")
def sweep_cases(oracle, dims):
    """name -> (case dict, expected counts from the oracle over the windows as regions, tally of the restatement over the span's hits)."""
    out = {}
    for name, case in cc.sweep_count_cases(dims).items():
        d = cc.sweep_case_dict(case)
        vals, widths, want = fp.expected_sweep(oracle, d)
        counts = cc.expected_counts(want, len(widths))
        used = (d["n_win"] - 1) * d["stride"] + d["window"] if d["n_win"] else 0
        hits = oracle_hits(oracle, d["mats"], d["cutoffs"], [d["chrom"][:used]], d["strand"])
        *restated, tally = restated_sweep_counts(hits, widths, d["window"], d["stride"], d["n_win"])
        assert same_counts(tuple(restated), counts), name   # the windows as separate regions == the span's hits handed to their windows
        tally.update(used=used, hits_per_motif=np.diff(hits["motif_offsets"]), sites_per_motif=np.diff(counts[1]))
        out[name] = (d, counts, tally)
    return out


def test_sweep_count_cases_hold_what_they_claim(sweep_cases, dims):
    T = dims["sweep_threads"]
    c = sweep_cases
    widths = lambda name: [m.shape[1] for m in c[name][0]["mats"]]
    d, counts, t = c["window_equals_W"]
    assert widths("window_equals_W")[0] == d["window"] and t["sites_per_motif"][0] > 0
    d, counts, t = c["W_above_window"]
    wide = np.array(widths("W_above_window")) > d["window"]
    assert wide.tolist() == [True, False, True] and np.all(t["hits_per_motif"][wide] > 0) and not t["sites_per_motif"][wide].any()
    assert t["sites_per_motif"][1] > 0 and t["hits_in_no_window"] >= t["hits_per_motif"][wide].sum()
    d, counts, t = c["stride_equals_window"]
    assert d["stride"] == d["window"] and t["hits_in_no_window"] > 0 and counts[0] > 0          # (a site across two windows' seam is in neither)
    d, counts, t = c["stride_above_window"]
    assert d["stride"] > d["window"] and t["hits_in_no_window"] > 100 and counts[0] > 0 and widths("stride_above_window")[2] == d["window"]
    d, counts, t = c["stride_one_wide_window"]
    assert d["stride"] == 1 and d["window"] > 30 * max(widths("stride_one_wide_window")) and t["shared_windows"] > 100
    assert counts[0] > 20 * t["hits"] > 0
    d, counts, t = c["bases_past_last_window"]
    assert 0 < len(d["chrom"]) - t["used"] < d["stride"] and t["hits_per_motif"][1] == t["used"]
    d, counts, t = c["span_below_window"]
    assert d["n_win"] == 0 and 0 < len(d["chrom"]) < d["window"] and counts[0] == 0 and not counts[2].any()
    assert c["span_is_one_window"][0]["n_win"] == 1 and c["span_is_one_window"][1][2].max() == 1
    d, counts, t = c["palindromes"]
    assert d["strand"] == 3 and t["two_hits_at_one_position"] >= 20 and t["hits_per_motif"][0] % 2 == 0 and t["hits_per_motif"][1] % 2 == 0
    for name in ("low_complexity_A", "low_complexity_AC"):
        d, counts, t = c[name]
        assert len(set(d["chrom"])) <= 2 and t["shared_windows"] > 50 and counts[0] > 500, name
    for name in ("many_motifs", "many_tied_motifs"):
        d, counts, t = c[name]
        assert len(d["mats"]) >= 200 and t["first_hit_behind_another_motifs"] >= 50 and (t["hits_per_motif"] > 0).sum() >= 150, name
    assert 3 <= c["many_motifs"][2]["hits_per_motif"].mean() <= 9
    for n in (T - 1, T, T + 1):
        assert c[f"hits_{n}"][2]["hits"] == n and c[f"hits_{n}"][2]["hits_in_no_window"] == 0
    # over the cases: every term of n_first = hi - max(lo, prev_hi + 1) + 1 is met
    assert sum(t["shared_windows"] > 0 for _, _, t in c.values()) >= 8 and sum(t["hits_in_no_window"] > 0 for _, _, t in c.values()) >= 4
    assert sum(t["first_hit_behind_another_motifs"] > 0 for _, _, t in c.values()) >= 6


# ------------------------------------------------------------------------------------------------ the prediction and stream cases

def test_prediction_and_stream_cases_hold_what_they_claim(oracle, dims):
    mats, cutoffs, sparse, dense, strand = cc.prediction_case()
    assert [len(s) for s in sparse] == [len(s) for s in dense] and all(set(s) <= set("ACGT") for s in dense) and any("N" in s for s in sparse)
    n_s = cc.expected_counts(oracle_hits(oracle, mats, cutoffs, sparse, strand), len(mats))[0]
    n_d = cc.expected_counts(oracle_hits(oracle, mats, cutoffs, dense, strand), len(mats))[0]
    # what ms_scan predicts from the sparse set's density at its widest margin: mu * 1.06 + 6 sqrt(mu + 1) + 256 slots
    assert n_d > 1.5 * (n_s * 1.06 + 6 * (n_s + 1) ** 0.5 + 256) and len(mats) * len(sparse) <= dims["gate_ratio"] * n_s
    assert _lib.key_layout(sum(map(len, sparse)), len(sparse), 30, len(mats))[1] > 0
    mats, cutoffs, seqs, strand = cc.stream_case()
    widths = [m.shape[1] for m in mats]
    for part in (seqs[:17], seqs[17:]):
        want = oracle_hits(oracle, mats, cutoffs, part, strand)
        n, offsets, regions = cc.expected_counts(want, len(mats))
        assert len(mats) * len(part) <= dims["gate_ratio"] * n and _lib.key_layout(sum(map(len, part)), len(part), max(map(len, part)), len(mats))[1] > 0
        cols = [want[k].tolist() for k in ("seq_idx", "pos", "score", "strand")]
        nested = [[[cols[0][k], cols[1][k], cols[2][k], cols[3][k]] for k in range(offsets[p], offsets[p + 1])] for p in range(len(mats))]
        kept = sum(len(sites) for per in oracle.deduplicate_motif_sites(oracle.make_motif_sites(nested, [0] * len(part)), widths) for sites in per)
        assert 0 < kept < n - 100                          # overlapping sites: de-duplication has something to remove
