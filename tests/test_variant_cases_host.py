"""
tests/variant_cases.py on the host: every case of tests/test_gpu_variant_boundaries.py sits where it claims -- the width classes of
var_scan_kernel's item stepping, the clipped and the missing windows, the long alleles' item counts and the pieces of their spliced
steps, the tile counts, what the quantile cutoffs let through -- and the LDS arithmetic of both kernels at their width limits.  The
kernels' own formulas (allele_windows, alt_step's split of a 32-column step) are restated here in Python and checked against brute force
over the built haplotype strings.  No GPU.
"""
import ctypes

import numpy as np
import pytest

import variant_cases as vc
from motifscan_amd import _lib

LDS_LIMIT = 160 * 1024                                  # bytes of LDS a gfx950 workgroup may take


@pytest.fixture(scope="module")
def dims():
    return _lib.varscan_dims()


@pytest.fixture(scope="module")
def cases(oracle, dims):
    return {name: vc.build(name, oracle, dims) for name in vc.CASES}


def widths_of(case):
    return [m.shape[1] for m in case["mats"]]


def test_dims_are_six_positive_numbers(dims):
    L = _lib.lib()
    out = np.zeros(6, dtype=np.int32)
    assert L.ms_debug_varscan_dims(_lib.ptr(out, ctypes.c_int32)) == _lib.MS_OK                # the symbol exists, with or without a device
    assert np.all(out > 0)
    keys = ("tile", "threads", "lds_max_width")
    assert [dims["variants"][k] for k in keys] + [dims["alleles"][k] for k in keys] == out.tolist()
    for d in dims.values():
        assert d["threads"] % 64 == 0 and d["tile"] <= d["threads"] and d["lds_max_width"] >= 64
    assert dims["alleles"]["tile"] & (dims["alleles"]["tile"] - 1) == 0                        # (al_scan_kernel's binary search halves it)
    assert L.ms_debug_varscan_dims(None) == _lib.MS_ERR_INVALID


def lds_bytes(dims):
    """(dynamic, static) bytes of LDS per scan at its lds_max_width: the table's W x 4 entries of 16 bytes and the all-zero one; the
    kernels' __shared__ arrays restated -- var_scan_kernel: s_wtot [2][threads / 64] and s_flag [tile] of 4 bytes; al_scan_kernel: the
    same two, s_pre [tile + 1] and s_half [2] of 4 bytes, s_rec [tile] of 32 (AlRec), the sum rounded up to s_rec's alignment of 8."""
    v, a = dims["variants"], dims["alleles"]
    static_v = 4 * (2 * (v["threads"] // 64) + v["tile"])
    static_a = 4 * (2 * (a["threads"] // 64) + a["tile"] + a["tile"] + 1 + 2) + 32 * a["tile"]
    static_a = (static_a + 7) // 8 * 8
    return {"variants": ((v["lds_max_width"] * 4 + 1) * 16, static_v), "alleles": ((a["lds_max_width"] * 4 + 1) * 16, static_a)}


def test_lds_at_the_width_limits_fits_a_workgroup(dims):
    for scan, (dyn, static) in lds_bytes(dims).items():
        print(f"{scan}: lds_max_width {dims[scan]['lds_max_width']}: {dyn} B dynamic + {static} B static = {dyn + static} B")
        assert dyn + static <= LDS_LIMIT
        one_more = ((dims[scan]["lds_max_width"] + 1) * 4 + 1) * 16
        assert one_more > dyn                           # (the next width reads its table from HBM: nothing more is ever asked for)


# ------------------------------------------------------------------------------------------------ SNV cases

def test_snv_steps_has_every_width_class_of_the_stepping(cases, dims):
    R = dims["variants"]["threads"]
    widths = widths_of(cases["snv_steps"])
    assert {R // w for w in widths} == {2, 1, 0}
    assert any(R % w == 0 for w in widths) and any(R // w == 1 and R % w for w in widths) and any(R // w == 2 and R % w for w in widths)
    assert R - 1 in widths and R + 1 in widths and R // 2 in widths


@pytest.mark.parametrize("name", ["snv_steps", "snv_lds_edge", "snv_only_wide"])
def test_snv_windows_are_clipped_where_claimed(cases, name):
    case = cases[name]
    L = case["lens"][case["chrom_idx"]]
    x = case["pos"]
    for W in widths_of(case):
        fits = L >= W
        assert np.any(fits & (x < W - 1)) and np.any(fits & (x == 0))                          # clipped at the chromosome's start
        assert np.any(fits & (x > L - W)) and np.any(fits & (x == L - 1))                      # ... and at its end
        if name == "snv_steps" or W == max(widths_of(case)):
            assert np.any(fits & (x == W - 1)) and np.any(fits & (x == L - W))                 # the first / last position that is not
        if W > 11:
            assert np.any(fits & (x < W - 1) & (x > 0)) and np.any(fits & (x > L - W) & (x < L - 1))
    run = case["marks"]["n_run"]
    on_run = (case["chrom_idx"] == case["marks"]["n_run_chrom"]) & (x >= run[0]) & (x < run[1])
    assert on_run.sum() >= 2
    alts = bytes(case["alt"])
    assert b"N" in alts and alts != alts.upper()


def test_snv_steps_chromosomes_and_variant_count(cases, dims):
    case = cases["snv_steps"]
    T, R = dims["variants"]["tile"], dims["variants"]["threads"]
    assert case["lens"].tolist() == [100, R, 700] and case["V"] == 2 * T + 1
    widths = np.array(widths_of(case))
    assert np.all(case["lens"][0] < widths)
    L = case["lens"][case["chrom_idx"]]
    nw = np.array([vc.n_windows(case["pos"], L, W) for W in widths])              # [motif, variant]
    assert np.any(nw.sum(axis=0) == 0)                                             # a variant with no window at all
    whole = (case["chrom_idx"] == 1) & (nw[widths.tolist().index(R)] == 1)         # one window, and it is the whole chromosome
    assert whole.sum() >= 2 and np.any(nw[:, whole] == 0)
    # the N run crosses a 32-base word of the packed genome, and the chromosome holds lower case and an IUPAC letter
    goff = np.concatenate([[0], np.cumsum(case["lens"])])
    run = case["marks"]["n_run"]
    assert (goff[2] + run[0]) // 32 != (goff[2] + run[1] - 1) // 32
    seq = case["chroms"]["c700"]
    assert seq != seq.upper() and b"R" in seq and seq[run[0]:run[1]] == b"N" * (run[1] - run[0])
    # every tile count keeps the placed variants: they are listed first
    assert np.flatnonzero(nw.sum(axis=0) == 0)[0] < T - 1 and np.flatnonzero(whole)[0] < T - 1


def test_snv_lds_edge_widths_and_order(cases, dims):
    M = dims["variants"]["lds_max_width"]
    assert widths_of(cases["snv_lds_edge"]) == [M + 1, 11, M, 768, 767]            # a wide motif first: its blocks' rows come before the others'
    assert cases["snv_lds_edge"]["V"] == 40 and cases["snv_lds_edge"]["lens"].tolist() == [2 * (M + 1) + 50]
    assert widths_of(cases["snv_only_wide"]) == [M + 1, M + 77] and cases["snv_only_wide"]["V"] == 20
    assert cases["snv_only_wide"]["chroms"] == cases["snv_lds_edge"]["chroms"]
    # the dynamic-LDS request is raised above 48 KB: 767 columns stay below, 768 do not
    assert (767 * 4 + 1) * 16 <= 48 * 1024 < (768 * 4 + 1) * 16 and M > 768


# ------------------------------------------------------------------------------------------------ allele cases

def hap_counts_brute(L, x, r, a, W):
    """Affected windows of the ref and of the alt haplotype, by looking at every window start of either haplotype."""
    out = []
    for length, Lh in ((r, L), (a, L - r + a)):
        s = np.arange(max(Lh - W + 1, 0))
        if length > 0:
            hit = (s <= x + length - 1) & (s + W - 1 >= x)         # the window holds a base of the allele
        else:
            hit = (s <= x - 1) & (s + W - 1 >= x)                  # ... or the junction an empty allele leaves
        out.append(int(hit.sum()))
    return out


@pytest.mark.parametrize("name", ["al_long", "al_lds_edge"])
def test_allele_windows_restated_equals_brute_force(cases, name):
    case = cases[name]
    L = int(case["lens"][0])
    for W in widths_of(case):
        for v in range(case["V"]):
            x, r, a = int(case["pos"][v]), int(case["ref_len"][v]), int(case["alt_len"][v])
            lo, hi = x, L - x - r
            got = [vc.allele_windows(lo, hi, r, W), vc.allele_windows(lo, hi, a, W)]
            assert got == hap_counts_brute(L, x, r, a, W), (W, v, x, r, a)
            hap = case["chroms"][case["names"][0]][:x] + case["alts"][v] + case["chroms"][case["names"][0]][x + r:]
            assert len(hap) == L - r + a


def alt_steps(lo, hi, r, a, W):
    """alt_step of ms_allele_dev.h, restated for every (alt-haplotype window, 32-column step) of a variant: arrays nl, na, n and `mid`
    (the step is put together of pieces, neither wholly left nor wholly right of the allele)."""
    n_alt = vc.allele_windows(lo, hi, a, W)
    rel = np.arange(n_alt) - min(lo, W - 1)
    c0 = np.arange(0, W, 32)
    d = rel[:, None] + c0[None, :]
    n = np.minimum(32, W - c0)[None, :] + 0 * d
    mid = ~(d + n <= 0) & ~(d >= a)
    nl = np.where(d < 0, -d, 0)
    ja = np.where(d < 0, 0, d)
    na = np.minimum(a - ja, 32 - nl)
    return {"nl": nl, "na": na, "n": n, "mid": mid, "ja": ja}


def test_al_long_reaches_the_long_allele_paths(cases, dims):
    case = cases["al_long"]
    R = dims["alleles"]["threads"]
    L = int(case["lens"][0])
    assert case["lens"].tolist() == [70_000] and widths_of(case) == [1, 8, 33, 70]
    r, a, x = case["ref_len"], case["alt_len"], case["pos"]
    assert np.any((a == vc.MS_ALLELE_MAX_LEN) & (r == 0)) and np.any((r == vc.MS_ALLELE_MAX_LEN) & (a == 0))
    for n in vc.LONG_LENGTHS:
        assert np.any((a == n) & (r == 0)) and np.any((r == n) & (a == 0))
    assert r[0] == 0 and a[0] == 5                                                  # the 5-base insertion listed first
    big = case["alts"][int(np.argmax(a))]
    assert b"N" * 32 in big and big != big.upper() and b"n" * 33 in big
    assert np.any((r > max(widths_of(case))) & (a == 0))                            # a deletion longer than the motif
    seq = case["chroms"]["long"]
    assert all(seq[lo:hi] == b"N" * (hi - lo) for lo, hi in case["marks"]["n_runs"]) and len(case["marks"]["n_runs"]) == 2
    for W in widths_of(case):
        items = np.array([vc.allele_windows(int(x[v]), L - int(x[v]) - int(r[v]), int(r[v]), W) +
                          vc.allele_windows(int(x[v]), L - int(x[v]) - int(r[v]), int(a[v]), W) for v in range(case["V"])])
        assert np.any(items > R) and np.any(items > 65536 - (W == 1))               # many rounds of one variant's items (W - 1 junction windows more)
    # the alt planes: every long allele starts off a 32-base edge, and deep reads are made at such offsets
    for name, sel in case["lists"].items():
        aoff = np.concatenate([[0], np.cumsum(a[sel])])
        long_ = a[sel] >= 31
        assert long_.sum() >= 11 and np.all(aoff[:-1][long_] % 32 != 0), name
    inside = three = deep = False
    for W in (33, 70):
        for v in range(case["V"]):
            if a[v] == 0:
                continue
            s = alt_steps(int(x[v]), L - int(x[v]) - int(r[v]), int(r[v]), int(a[v]), W)
            m = s["mid"]
            inside |= bool(np.any(m & (s["nl"] == 0) & (s["na"] == 32)))            # a step wholly inside the allele
            three |= bool(np.any(m & (s["nl"] > 0) & (s["na"] > 0) & (s["nl"] + s["na"] < s["n"])))    # left genome, alt, right genome
            deep |= bool(np.any(m & (s["ja"] > 4096)))
    assert inside and three and deep
    # the two lists: alt bytes in all one short of and one past a multiple of 32; they differ in the last allele only
    la, lb = case["lists"]["tail_32k_minus_1"], case["lists"]["tail_32k_plus_1"]
    assert a[la].sum() % 32 == 31 and a[lb].sum() % 32 == 1 and np.array_equal(la[:-1], lb[:-1]) and la[-1] != lb[-1]


def test_al_lds_edge_shapes_and_places(cases, dims):
    case = cases["al_lds_edge"]
    M = dims["alleles"]["lds_max_width"]
    L = int(case["lens"][0])
    assert widths_of(case) == [M + 1, 11, M, 640, 639] and L == 2 * (M + 1) + 50 and 35 <= case["V"] <= 45
    assert (639 * 4 + 1) * 16 <= 40 * 1024 < (640 * 4 + 1) * 16 and M > 640        # either side of the allele scan's dynamic-LDS raise
    shapes = set(zip(case["ref_len"].tolist(), case["alt_len"].tolist()))
    assert shapes == {(1, 1), (0, 1), (1, 0), (0, 300), (300, 0), (40, 33), (2, 700), (0, 5)}
    run = case["marks"]["n_run"]
    for r, a in shapes - {(0, 5)}:
        sel = (case["ref_len"] == r) & (case["alt_len"] == a)
        x = case["pos"][sel]
        assert sel.sum() == 5 and np.any(x == 0) and np.any(x == L - r)
        assert np.any((x + max(r, 1) > run[0] - 3) & (x < run[1]))                 # on, or within three bases of, the N run
    assert np.any((case["ref_len"] == 0) & (case["alt_len"] == 5) & (case["pos"] == L))
    snv = (case["ref_len"] == 1) & (case["alt_len"] == 1)
    assert snv.sum() == 5                                                           # what the comparison with ms_scan_variants runs on
    assert widths_of(cases["al_only_wide"]) == [M + 1] and cases["al_only_wide"]["V"] == 12


def test_tile_cases(cases, dims):
    for name, scan in (("snv_steps", "variants"), ("al_tiles", "alleles")):
        T = dims[scan]["tile"]
        counts = vc.tile_counts(T)
        assert counts == (T - 1, T, T + 1, 2 * T, 2 * T + 1) and max(counts) == cases[name]["V"]
        assert any(n % T == 1 for n in counts) and any(n % T == 0 for n in counts) and any(n % T == T - 1 for n in counts)
        assert vc.chunk_sizes(T) == (7, T, T + 1)
    case = cases["al_tiles"]
    T = dims["alleles"]["tile"]
    assert widths_of(case) == [5, 33, 129] and case["lens"].tolist() == [900]
    assert (case["ref_len"][T - 1], case["alt_len"][T - 1]) == (0, 300) and (case["ref_len"][T], case["alt_len"][T]) == (300, 0)
    assert len(set(zip(case["ref_len"].tolist(), case["alt_len"].tolist()))) >= 8


# ------------------------------------------------------------------------------------------------ what the cutoffs let through

@pytest.mark.parametrize("name", vc.CASES)
def test_cutoff_sets_compare_what_they_claim(cases, name):
    case = cases[name]
    P = len(case["mats"])
    for list_name, sel in case["lists"].items():
        sel = None if len(sel) == case["V"] else sel
        rec, offsets, gained, lost = vc.expected(case, "q90", 3, sel)
        motif = np.repeat(np.arange(P), np.diff(offsets))
        for m in range(P):
            if case["kind"] == "snv":
                assert set(np.unique(rec["state"][motif == m]).tolist()) == {1, 2, 3}, (name, m)
            else:
                assert set(np.unique(rec["allele"][motif == m]).tolist()) == {0, 1}, (name, m)
        assert np.any((gained > 0) & (lost > 0)), (name, list_name)
        n_all = vc.expected(case, "all", 3, sel)[1]
        n_none = vc.expected(case, "none", 3, sel)[1]
        total = sum(2 * len(t["variant"]) for t in (case["table"] if sel is None else vc.subset_table(case["table"], sel, case["V"])))
        print(f"{name} / {list_name}: {n_all[-1]} records at all-pass, {offsets[-1]} at q90; gained {gained.tolist()} lost {lost.tolist()}")
        assert n_all[-1] == total and n_none[-1] == 0 and 0 < offsets[-1] < total  # (the seeded matrices are finite: every window x strand scores)


def test_subset_table_renumbers_and_keeps_order(cases):
    case = cases["al_tiles"]
    sel = np.array([3, 4, 200])
    sub = vc.subset_table(case["table"], sel, case["V"])
    for t, s in zip(case["table"], sub):
        keep = np.isin(t["variant"], sel)
        assert np.array_equal(sel[s["variant"]], t["variant"][keep]) and np.array_equal(s["score"], t["score"][keep])
    first = vc.subset_table(case["table"], np.arange(10), case["V"])
    assert all(np.array_equal(f["variant"], t["variant"][t["variant"] < 10]) for f, t in zip(first, case["table"]))
